"""Restatement of "mod pileup" (include/ffhip.h) in plain Python integers, and of the bedMethyl table `flappie --map-mods` writes.

A mod pileup belongs to a reference of K records of M_k bases: off_k the lengths before record k, P their sum.  10 planes of P uint32, [strand o][column c][position],
c = 0 mod, 1 canon, 2 fail, 3 diff, 4 del (row 5 o + c of `counts`); eight uint64 totals (TOTALS); a histogram of 256 words.  A read counts by the pileup's rule
(pileup_ref.passes).

`ModPileup.add` is the header's walk in signal order: from (0, 0), j truth and i call bases consumed,
  = / X   f = o ? M_k - 1 - (tstart + j) : tstart + j;  a site when the record's forward letter at f is C (o = 0) or G (o = 1);  on a site: sites += 1; the call's
          letter C or Z: v = ml[i], hist[v] += 1, column mod (v >= hi), canon (v <= lo) or fail; another letter: diff;  j++, i++
  D       on a site: sites += 1, column del;  j++
  I       i++
The class follows the call's letter, never the op code."""
import numpy as np

from pileup_ref import MASK, passes

TOTALS = ("reads", "skipped", "sites", "mod", "canon", "fail", "diff", "del")
COLUMNS = ("mod", "canon", "fail", "diff", "del")


class ModPileup:
    def __init__(self, lens, refs, min_identity: int = 0, lo: int = 50, hi: int = 205):
        self.lens = [int(m) for m in lens]
        self.refs = [str(r).upper() for r in refs]
        assert [len(r) for r in self.refs] == self.lens and 0 <= lo < hi <= 255
        self.off = [sum(self.lens[:k]) for k in range(len(self.lens))]
        self.P = sum(self.lens)
        self.min_identity = max(0, int(min_identity))
        self.lo, self.hi = int(lo), int(hi)
        self.reset()

    def reset(self):
        self.counts = np.zeros((10, self.P), np.uint32)
        self.totals = {k: 0 for k in TOTALS}
        self.hist = np.zeros(256, np.uint64)

    def _bump(self, o, column, at):
        c = COLUMNS.index(column)
        self.counts[5 * o + c, at] = (int(self.counts[5 * o + c, at]) + 1) & MASK      # counters wrap at 2^32
        self.totals[column] += 1

    def classify(self, v: int) -> str:
        return "mod" if v >= self.hi else "canon" if v <= self.lo else "fail"

    def add(self, q: int, tstart: int, tend: int, call: str, ml, ops):
        """one alignment through the identity test and, if it passes, the signal-order walk"""
        ops = [int(x) for x in ops]
        cnt = [ops.count(c) for c in range(4)]
        if not passes(cnt[0], cnt[1], cnt[2], cnt[3], self.min_identity):
            self.totals["skipped"] += 1
            return
        k, o = q >> 1, q & 1
        Mk, off, m = self.lens[k], self.off[k], tend - tstart
        assert 0 <= tstart < tend <= Mk and cnt[0] + cnt[1] + cnt[3] == m and cnt[0] + cnt[1] + cnt[2] == len(call) == len(ml)
        self.totals["reads"] += 1
        j = i = 0
        for op in ops:
            if op == 2:
                i += 1
                continue
            f = Mk - 1 - (tstart + j) if o else tstart + j
            if self.refs[k][f] == "CG"[o]:
                self.totals["sites"] += 1
                if op == 3:
                    self._bump(o, "del", off + f)
                elif call[i] in "CZ":
                    v = int(ml[i])
                    self.hist[v] += np.uint64(1)
                    self._bump(o, self.classify(v), off + f)
                else:
                    self._bump(o, "diff", off + f)
            j += 1
            i += op != 3

    def add_read(self, mp: dict, tr: dict, call: str, ml):
        """a read of a finished batch from its map record, its truth record, its call and its 5mC bytes (Batch.map, Batch.truth, Batch.basecall, Batch.mod_probs)"""
        if mp["status"] != 1 or tr["status"] != 1:
            return
        assert tr["n"] == len(call) and tr["m"] == mp["tend"] - mp["tstart"]
        self.add(mp["q"], mp["tstart"], mp["tend"], call, ml, tr["ops"])

    # ---- the host side (include/flappie_modpileup.h): mods.bed, hist.tsv and the lines of stderr
    def rows(self, motif: str = "CG", combine: bool = False):
        """(k, f, strand, [mod canon fail diff del]) of every row the writer writes, in its order: a site of its strand that passes the motif and whose five counters
        sum to 1 or more; reference order, + before - at one position.  combine (CG only): the - strand's counters of the G at f + 1 added to the + row, strand '.'"""
        assert motif in ("CG", "C") and not (combine and motif != "CG")
        out = []
        for k, rec in enumerate(self.refs):
            for f in range(self.lens[k]):
                for o in (0, 1):
                    if rec[f] != "CG"[o]:
                        continue
                    if motif == "CG" and not (f + 1 < self.lens[k] and rec[f + 1] == "G" if o == 0 else f >= 1 and rec[f - 1] == "C"):
                        continue
                    if combine and o == 1:
                        continue
                    c = [int(self.counts[5 * o + x, self.off[k] + f]) for x in range(5)]
                    if combine:
                        c = [a + int(self.counts[5 + x, self.off[k] + f + 1]) for x, a in enumerate(c)]
                    if sum(c) >= 1:
                        out.append((k, f, "." if combine else "+-"[o], c))
        return out

    def bed(self, names, motif: str = "CG", combine: bool = False) -> str:
        out = []
        for k, f, strand, (mod, canon, fail, diff, dele) in self.rows(motif, combine):
            nv = mod + canon
            pct = "%.2f" % (100.0 * mod / nv) if nv else "0.00"
            out.append("\t".join([names[k], str(f), str(f + 1), "m", str(nv), strand, str(f), str(f + 1), "255,0,0", str(nv), pct, str(mod), str(canon), "0", str(dele),
                                  str(fail), str(diff), "0"]) + "\n")
        return "".join(out)

    def hist_tsv(self) -> str:
        return "".join("%d\t%d\n" % (v, int(self.hist[v])) for v in range(256))

    def stderr_lines(self, motif: str = "CG", combine: bool = False):
        d = {k: self.totals[k] for k in TOTALS}
        d["rows"] = len(self.rows(motif, combine))
        return d
