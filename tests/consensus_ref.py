"""Restatement of "consensus" (include/ffhip.h) in plain Python integers, and of the files `flappie --map-consensus` writes.

A consensus belongs to a reference of K records of M_k bases: off_k the lengths before record k, P their sum.  PLANES = 37 planes of P uint32, [plane][position]:
0 .. 3 the forward base A C G T, 4 del, 5 + 4 d + base the inserted base at forward offset d (0 .. MINOR - 1) in the gap behind the position; eight uint64 totals
(TOTALS).  Which read counts is the pileup's rule (pileup_ref.passes).

`Consensus.add` is the header's walk in SIGNAL order: from (0, 0), j truth and i call bases consumed,
  = / X   f = o ? M_k - 1 - (tstart + j) : tstart + j;  base = o ? 3 - code(s_i) : code(s_i);  plane[base][off_k + f] += 1;  bases += 1;  j++, i++
  D       plane[4][off_k + f] += 1;  del += 1;  j++
  a maximal run of l I ops at j: j < 1 or j > m - 1: edge_ins += l.  Else p = o ? M_k - 1 - tstart - j : tstart + j - 1; the r-th letter s_(i + r) stands at
          forward offset d = o ? l - 1 - r : r; d < 8: plane[5 + 4 d + base][off_k + p] += 1, ins_bases += 1; else long_ins += 1.  i += l
`forward_add` is the independent statement tests/test_consensus.py holds it to: the read as its SAM line gives it -- forward start, forward CIGAR, turned SEQ --
walked left to right, the letters of an insertion taken left to right, leading and trailing insertions dropped.
`call` is k_consensus_call's rule, `fasta`, `changes` and `stderr_lines` the host side (include/flappie_consensus.h)."""
import numpy as np

import map_ref as R
from pileup_ref import CODE, MASK, passes

TOTALS = ("reads", "skipped", "bases", "del", "ins_bases", "long_ins", "edge_ins", "reserved")
MINOR = 8
PLANES = 5 + 4 * MINOR
LOW, SAME, SUB, DEL, INS = 0, 1, 2, 3, 4
CELL = np.dtype([("n", "u1"), ("what", "u1"), ("s", "S10"), ("depth", "<u4")])
LINE = 70


class Consensus:
    def __init__(self, lens, min_identity: int = 0):
        self.lens = [int(m) for m in lens]
        self.off = [sum(self.lens[:k]) for k in range(len(self.lens))]
        self.P = sum(self.lens)
        self.min_identity = max(0, int(min_identity))
        self.reset()

    def reset(self):
        self.counts = np.zeros((PLANES, self.P), np.uint32)
        self.totals = {k: 0 for k in TOTALS}

    def _bump(self, plane, at):
        self.counts[plane, at] = (int(self.counts[plane, at]) + 1) & MASK      # counters wrap at 2^32

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
        j = i = x = 0
        while x < len(ops):
            op = ops[x]
            if op in (0, 1):
                f = Mk - 1 - (tstart + j) if o else tstart + j
                self._bump(3 - CODE[call[i]] if o else CODE[call[i]], off + f)
                self.totals["bases"] += 1
                j, i, x = j + 1, i + 1, x + 1
            elif op == 3:
                f = Mk - 1 - (tstart + j) if o else tstart + j
                self._bump(4, off + f)
                self.totals["del"] += 1
                j, x = j + 1, x + 1
            else:
                ell = 1
                while x + ell < len(ops) and ops[x + ell] == 2:
                    ell += 1
                if j < 1 or j > m - 1:
                    self.totals["edge_ins"] += ell
                else:
                    p = Mk - 1 - tstart - j if o else tstart + j - 1
                    for r in range(ell):
                        d = ell - 1 - r if o else r
                        base = 3 - CODE[call[i + r]] if o else CODE[call[i + r]]
                        if d < MINOR:
                            self._bump(5 + 4 * d + base, off + p)
                            self.totals["ins_bases"] += 1
                        else:
                            self.totals["long_ins"] += 1
                i, x = i + ell, x + ell

    def add_read(self, mp: dict, tr: dict, call: str):
        """a read of a finished batch from its map record, its truth record and its call (Batch.map, Batch.truth, Batch.basecall)"""
        if mp["status"] != 1 or tr["status"] != 1:
            return
        assert tr["n"] == len(call) and tr["m"] == mp["tend"] - mp["tstart"]
        self.add(mp["q"], mp["tstart"], mp["tend"], call, tr["ops"])

    def forward_add(self, q: int, tstart: int, tend: int, call: str, ops):
        """the same read as its SAM line has it, walked left to right on the forward strand: an insertion is a string of SEQ, its letters taken in order"""
        ops = [int(x) for x in ops]
        if not passes(ops.count(0), ops.count(1), ops.count(2), ops.count(3), self.min_identity):
            self.totals["skipped"] += 1
            return
        k, strand, a, b = R.forward(q, tstart, tend, self.lens)
        seq = call.replace("Z", "C")
        if strand == "-":
            seq, ops = R.revcomp(seq), ops[::-1]
        self.totals["reads"] += 1
        cigar = []                                               # [op, length] with I runs merged, as a CIGAR has them
        for op in ops:
            kind = "M" if op in (0, 1) else "I" if op == 2 else "D"
            if cigar and cigar[-1][0] == kind:
                cigar[-1][1] += 1
            else:
                cigar.append([kind, 1])
        pos, i = a, 0
        for kind, length in cigar:
            if kind == "M":
                for t in range(length):
                    self._bump("ACGT".index(seq[i + t]), self.off[k] + pos + t)
                self.totals["bases"] += length
                pos, i = pos + length, i + length
            elif kind == "D":
                for t in range(length):
                    self._bump(4, self.off[k] + pos + t)
                self.totals["del"] += length
                pos += length
            else:
                inserted = seq[i:i + length]
                if a < pos < b:                                  # something aligned on either side
                    for d, letter in enumerate(inserted):
                        if d < MINOR:
                            self._bump(5 + 4 * d + "ACGT".index(letter), self.off[k] + pos - 1)
                            self.totals["ins_bases"] += 1
                        else:
                            self.totals["long_ins"] += 1
                else:
                    self.totals["edge_ins"] += length
                i += length
        assert pos == b and i == len(seq)

    # ---- the call (k_consensus_call)
    def depth(self):
        return self.counts[:5].astype(np.int64).sum(axis=0)


def ref_codes(records):
    """the reference's letters as codes 0 .. 3, all records behind each other"""
    return [CODE[c] for rec in records for c in rec.upper()]


def call(counts, codes, min_depth: int) -> np.ndarray:
    """the cells of ffhip_consensus_call from planes [37][P] and the reference's codes [P]"""
    assert min_depth >= 1
    counts = np.asarray(counts)
    P = counts.shape[1]
    cells = np.zeros(P, CELL)
    for g in range(P):
        c = [int(counts[x, g]) for x in range(5)]
        depth = sum(c)
        rf = codes[g]
        letters, what = "", LOW
        if depth < min_depth:
            letters = "acgt"[rf]
        else:
            top = max(c)
            win = rf if c[rf] == top else c.index(top)
            what = DEL if win == 4 else SAME if win == rf else SUB
            if win < 4:
                letters = "ACGT"[win]
            for d in range(MINOR):
                v = [int(counts[5 + 4 * d + x, g]) for x in range(4)]
                if not 2 * sum(v) > depth:
                    break
                letters += "ACGT"[v.index(max(v))]
                what |= INS
        cells[g] = (len(letters), what, letters.encode(), min(depth, MASK))
    return cells


def letters(cell) -> str:
    return bytes(cell["s"])[:int(cell["n"])].decode()


def fasta(names, lens, cells) -> str:
    """cons.fa: a record a reference record, the cells' letters concatenated in lines of 70; an empty consensus writes an empty line"""
    out, at = [], 0
    for nm, M in zip(names, lens):
        s = "".join(letters(cells[at + x]) for x in range(M))
        at += M
        out.append(">%s\n" % nm)
        out.append("".join(s[x:x + LINE] + "\n" for x in range(0, len(s), LINE)) if s else "\n")
    return "".join(out)


def changes(names, records, cells, counts) -> str:
    """changes.tsv: a line for every cell that is not plain SAME or LOW: record, position, reference letter, letters or -, depth, the winner's count, the first
    insertion column's total (0 without inserted letters)"""
    out, at = [], 0
    for nm, rec in zip(names, records):
        for x in range(len(rec)):
            cell, g = cells[at + x], at + x
            what = int(cell["what"])
            if what in (LOW, SAME):
                continue
            s = letters(cell)
            plane = 4 if (what & 3) == DEL else "ACGT".index(s[0])
            first = sum(int(counts[5 + b, g]) for b in range(4)) if what & INS else 0
            out.append("%s\t%d\t%s\t%s\t%d\t%d\t%d\n" % (nm, x, rec[x].upper(), s or "-", int(cell["depth"]), int(counts[plane, g]), first))
        at += len(rec)
    return "".join(out)


STDERR_KEYS = ("reads", "skipped", "positions", "called", "low_depth", "same", "sub", "del", "ins", "long_ins", "edge_ins")


def stderr_lines(totals: dict, cells) -> dict:
    kind = cells["what"].astype(int) & 3
    has = (cells["what"].astype(int) & INS) != 0
    n = cells["n"].astype(int)
    return {"reads": totals["reads"], "skipped": totals["skipped"], "positions": len(cells), "called": int((kind != LOW).sum()), "low_depth": int((kind == LOW).sum()),
            "same": int((kind == SAME).sum()), "sub": int((kind == SUB).sum()), "del": int((kind == DEL).sum()),
            "ins": int((n - (kind != DEL))[has].sum()), "long_ins": totals["long_ins"], "edge_ins": totals["edge_ins"]}


def stderr_text(totals: dict, cells) -> str:
    d = stderr_lines(totals, cells)
    return "".join("consensus\t%s\t%d\n" % (k, d[k]) for k in STDERR_KEYS)
