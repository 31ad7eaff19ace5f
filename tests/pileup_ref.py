"""Restatement of "pileup" (include/ffhip.h) in plain Python integers, and of the table `flappie --map-pileup` writes.

A pileup belongs to a reference of K records of M_k bases: off_k the lengths before record k, P their sum.  12 planes of P uint32, [strand o][column c][position],
c = 0 .. 3 the base A C G T, 4 del, 5 ins; eight uint64 totals (TOTALS).  A read counts when its map record and its truth record both say status 1 and
1000 n_match >= min_identity (n_match + n_mismatch + n_ins + n_del); with both statuses 1 and the test failed it adds 1 to `skipped`; otherwise nothing.

`Pileup.add` is the header's walk in SIGNAL order: from (0, 0), j truth and i call bases consumed,
  = / X   f = o ? M_k - 1 - (tstart + j) : tstart + j;  base = o ? 3 - code(s_i) : code(s_i);  count[o][base][off_k + f] += 1;  j++, i++
  D       count[o][4][off_k + f] += 1;  j++
  I       1 <= j <= m - 1: p = o ? M_k - 1 - tstart - j : tstart + j - 1;  count[o][5][off_k + p] += 1;  else an edge insertion: no plane changes;  i++
`forward_add` is the independent statement tests/test_pileup.py holds it to: the read as a SAM line would give it -- forward start, forward CIGAR, turned SEQ --
piled up left to right, an insertion counted at the position to its left, leading and trailing insertions dropped."""
import numpy as np

import map_ref as R

TOTALS = ("reads", "skipped", "match", "mismatch", "del", "ins", "edge_ins", "reserved")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "Z": 1}
MASK = (1 << 32) - 1


def passes(n_match: int, n_mismatch: int, n_ins: int, n_del: int, min_identity: int) -> bool:
    return 1000 * int(n_match) >= int(min_identity) * (int(n_match) + int(n_mismatch) + int(n_ins) + int(n_del))


class Pileup:
    def __init__(self, lens, min_identity: int = 0):
        self.lens = [int(m) for m in lens]
        self.off = [sum(self.lens[:k]) for k in range(len(self.lens))]
        self.P = sum(self.lens)
        self.min_identity = max(0, int(min_identity))
        self.reset()

    def reset(self):
        self.counts = np.zeros((2, 6, self.P), np.uint32)
        self.totals = {k: 0 for k in TOTALS}

    def _bump(self, o, c, at):
        self.counts[o, c, at] = (int(self.counts[o, c, at]) + 1) & MASK      # counters wrap at 2^32

    def add(self, q: int, tstart: int, tend: int, call: str, ops):
        """one alignment through the identity test and, if it passes, the signal-order walk"""
        ops = [int(x) for x in ops]
        cnt = [ops.count(c) for c in range(4)]
        if not passes(cnt[0], cnt[1], cnt[2], cnt[3], self.min_identity):
            self.totals["skipped"] += 1
            return
        k, o = q >> 1, q & 1
        Mk, off, m = self.lens[k], self.off[k], tend - tstart
        assert 0 <= tstart < tend <= Mk and cnt[0] + cnt[1] + cnt[3] == m and cnt[0] + cnt[1] + cnt[2] == len(call)
        self.totals["reads"] += 1
        j = i = 0
        for op in ops:
            if op in (0, 1):
                f = Mk - 1 - (tstart + j) if o else tstart + j
                base = 3 - CODE[call[i]] if o else CODE[call[i]]
                self._bump(o, base, off + f)
                self.totals["match" if op == 0 else "mismatch"] += 1
                j, i = j + 1, i + 1
            elif op == 3:
                f = Mk - 1 - (tstart + j) if o else tstart + j
                self._bump(o, 4, off + f)
                self.totals["del"] += 1
                j += 1
            else:
                if 1 <= j <= m - 1:
                    p = Mk - 1 - tstart - j if o else tstart + j - 1
                    self._bump(o, 5, off + p)
                    self.totals["ins"] += 1
                else:
                    self.totals["edge_ins"] += 1
                i += 1

    def add_read(self, mp: dict, tr: dict, call: str):
        """a read of a finished batch from its map record, its truth record and its call (Batch.map, Batch.truth, Batch.basecall)"""
        if mp["status"] != 1 or tr["status"] != 1:
            return
        assert tr["n"] == len(call) and tr["m"] == mp["tend"] - mp["tstart"]
        self.add(mp["q"], mp["tstart"], mp["tend"], call, tr["ops"])

    def forward_add(self, q: int, tstart: int, tend: int, call: str, ops):
        """the same read as its SAM line has it, piled up left to right on the forward strand"""
        ops = [int(x) for x in ops]
        if not passes(ops.count(0), ops.count(1), ops.count(2), ops.count(3), self.min_identity):
            self.totals["skipped"] += 1
            return
        k, strand, a, b = R.forward(q, tstart, tend, self.lens)
        o = 1 if strand == "-" else 0
        seq = call.replace("Z", "C")
        if o:
            seq, ops = R.revcomp(seq), ops[::-1]
        self.totals["reads"] += 1
        pos, i = a, 0                                             # the next reference position, the next letter of SEQ
        for op in ops:
            if op in (0, 1):
                self._bump(o, "ACGT".index(seq[i]), self.off[k] + pos)
                self.totals["match" if op == 0 else "mismatch"] += 1
                pos, i = pos + 1, i + 1
            elif op == 3:
                self._bump(o, 4, self.off[k] + pos)
                self.totals["del"] += 1
                pos += 1
            else:
                if a < pos < b:                                   # something aligned on either side
                    self._bump(o, 5, self.off[k] + pos - 1)
                    self.totals["ins"] += 1
                else:
                    self.totals["edge_ins"] += 1
                i += 1
        assert pos == b and i == len(seq)

    # ---- the host side (include/flappie_align.h): pileup.tsv and the lines of stderr
    def depth(self):
        return self.counts[:, :5, :].astype(np.int64).sum(axis=(0, 1))

    def tsv(self, names, records) -> str:
        """a line a position of every record, in reference order: name, 0-based position, reference letter, depth (A C G T del of both strands), the six + strand
        counts, the six - strand counts"""
        depth = self.depth()
        out = []
        for k, (nm, rec) in enumerate(zip(names, records)):
            for x in range(self.lens[k]):
                at = self.off[k] + x
                out.append("\t".join([nm, str(x), rec[x].upper(), str(int(depth[at]))] + [str(int(self.counts[o, c, at])) for o in (0, 1) for c in range(6)]) + "\n")
        return "".join(out)

    def stderr_lines(self):
        d = {"reads": self.totals["reads"], "skipped": self.totals["skipped"], "positions": self.P, "covered": int((self.depth() >= 1).sum()),
             "match": self.totals["match"], "mismatch": self.totals["mismatch"], "del": self.totals["del"], "ins": self.totals["ins"], "edge_ins": self.totals["edge_ins"]}
        return d
