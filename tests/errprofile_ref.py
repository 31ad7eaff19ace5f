"""Restatement of "error profile" (include/ffhip.h) in plain Python integers, and of the table `flappie --truth-errors` writes.

One flat array of WORDS uint64: sub[4][5], ins[4], qual[94][3], ctx[1024][4], hp[4][16][33] (SECTIONS: name, first word, shape), then the twelve TOTALS.  Which read
counts is the pileup's rule (pileup_ref.passes).

`ErrProfile.add` is the header's statement as the kernel has it, an op at a time: from (0, 0), j truth and i call bases consumed before the op,
  = / X   sub[t_j][code(s_i)], qual[qv_i][0 | 1]; 2 <= j <= m - 3: ctx[w(j)][0 | 1]
  D       sub[t_j][4]; 2 <= j <= m - 3: ctx[w(j)][2]
  I       1 <= j <= m - 1 (interior): ins[code(s_i)], qual[qv_i][2]; 3 <= j <= m - 2: ctx[w(j - 1)][3].  Else edge_ins
  and, at the op that consumes the first base t_a of a maximal run [a, a + r) of letter b with a >= 1: the run's first 17 letters decide -- the run reaches the
  truth's end within them: nothing; 17 equal letters and a + 17 <= m - 1: hp_long; else the walk over the op indices: back over the I ops ahead (F), forward to
  the op of t_(a + r - 1) and over the I ops behind (B); more than 64 ops: hp_wide; else c = the '=' between + the I ops of letter b among them all,
  hp[b][r - 1][min(c, 32)], hp_runs.
`brute` is the independent statement tests/test_errprofile.py holds it to: the alignment as COLUMNS per truth position -- what consumed it and what was inserted
behind it -- with the 5-mers as slices of the truth's text and the runs found by a regular expression.
`tsv_lines` and `stderr_lines` are the host side (include/flappie_errprofile.h)."""
import re

import numpy as np

import map_ref as R
from pileup_ref import CODE, passes

TOTALS = ("reads", "skipped", "match", "mismatch", "del", "ins", "edge_ins", "ctx_sites", "hp_runs", "hp_long", "hp_wide", "reserved")
SECTIONS = (("sub", 0, (4, 5)), ("ins", 20, (4,)), ("qual", 24, (94, 3)), ("ctx", 306, (1024, 4)), ("hp", 4402, (4, 16, 33)))
TABLE_WORDS = 6514
WORDS = TABLE_WORDS + len(TOTALS)
HP_MAX_RUN, HP_MAX_CALLED, HP_MAX_OPS = 16, 32, 64
MASK = (1 << 64) - 1


def qv(ch: int) -> int:
    return min(93, max(0, int(ch) - 33))


def fold(truth):
    """a truth's codes 0 .. 4 with 4 read as 1"""
    return [1 if int(c) == 4 else int(c) for c in truth]


def mapped_truth(records, q: int, tstart: int, tend: int):
    """the codes of y_q[tstart : tend], the truth of a read in the mode of truth from map"""
    return [CODE[c] for c in R.searches(records)[q][tstart:tend]]


class ErrProfile:
    def __init__(self, min_identity: int = 0):
        self.min_identity = max(0, int(min_identity))
        self.reset()

    def reset(self):
        self.counts = np.zeros(TABLE_WORDS, np.uint64)
        self.totals = {k: 0 for k in TOTALS}
        self.sec = {name: self.counts[at:at + int(np.prod(shape))].reshape(shape) for name, at, shape in SECTIONS}

    def _bump(self, name, *idx):
        a = self.sec[name]
        a[idx] = np.uint64((int(a[idx]) + 1) & MASK)             # counters wrap at 2^64

    def _tot(self, name, by=1):
        self.totals[name] = (self.totals[name] + by) & MASK

    def _passes(self, ops):
        if passes(ops.count(0), ops.count(1), ops.count(2), ops.count(3), self.min_identity):
            return True
        self._tot("skipped")
        return False

    def add(self, call, qual: bytes, truth, ops):
        """one alignment through the identity test and, if it passes, the walk an op at a time"""
        ops, t = [int(x) for x in ops], fold(truth)
        s = call.decode() if isinstance(call, bytes) else call
        n, m, K = len(s), len(t), len(ops)
        assert m >= 1 and len(qual) == n and ops.count(0) + ops.count(1) + ops.count(3) == m and ops.count(0) + ops.count(1) + ops.count(2) == n
        if not self._passes(ops):
            return
        self._tot("reads")

        def w(c):
            return sum(4 ** (2 - d) * t[c + d] for d in range(-2, 3))

        j = i = 0
        for k, op in enumerate(ops):
            if op == 2:
                if 1 <= j <= m - 1:
                    self._bump("ins", CODE[s[i]])
                    self._bump("qual", qv(qual[i]), 2)
                    self._tot("ins")
                    if 3 <= j <= m - 2:
                        self._bump("ctx", w(j - 1), 3)
                        self._tot("ctx_sites")
                else:
                    self._tot("edge_ins")
                i += 1
                continue
            if op == 3:
                self._bump("sub", t[j], 4)
                self._tot("del")
            else:
                self._bump("sub", t[j], CODE[s[i]])
                self._bump("qual", qv(qual[i]), op)
                self._tot("match" if op == 0 else "mismatch")
            if 2 <= j <= m - 3:
                self._bump("ctx", w(j), 2 if op == 3 else op)
                self._tot("ctx_sites")
            if j >= 1 and t[j - 1] != t[j]:
                self._run(s, t, ops, k, j, i)
            j += 1
            i += op != 3

    def _run(self, s, t, ops, k, a, i):
        n, m, K, b = len(s), len(t), len(ops), t[a]
        r = 1
        while r <= HP_MAX_RUN and a + r < m and t[a + r] == b:
            r += 1
        if a + r > m - 1:
            return
        if r > HP_MAX_RUN:
            self._tot("hp_long")
            return
        nop, c = 1, int(ops[k] == 0)
        kk, ii = k - 1, i - 1
        while kk >= 0 and ops[kk] == 2:
            nop += 1
            if nop > HP_MAX_OPS:
                break
            c += CODE[s[ii]] == b
            kk, ii = kk - 1, ii - 1
        kk, ii, left = k + 1, i + (ops[k] != 3), r - 1
        while nop <= HP_MAX_OPS and kk < K and (left > 0 or ops[kk] == 2):
            nop += 1
            if nop > HP_MAX_OPS:
                break
            if ops[kk] == 2:
                c += CODE[s[ii]] == b
                ii += 1
            else:
                left -= 1
                c += ops[kk] == 0
                ii += ops[kk] != 3
            kk += 1
        if nop > HP_MAX_OPS:
            self._tot("hp_wide")
            return
        self._bump("hp", b, r - 1, min(c, HP_MAX_CALLED))
        self._tot("hp_runs")

    def add_read(self, tr: dict, call, qual: bytes, truth, mp: dict = None):
        """a read of a finished batch from its truth record, its call, its quality string and its truth (Batch.truth, Batch.basecall; the codes given or
        mapped_truth of its map record `mp`, which then has to say status 1 and the truth's length)"""
        if tr["status"] != 1 or (mp is not None and (mp["status"] != 1 or mp["tend"] - mp["tstart"] != tr["m"])):
            return
        assert tr["n"] == len(call) and tr["m"] == len(truth)
        self.add(call, qual, truth, tr["ops"])

    def brute(self, call, qual: bytes, truth, ops):
        """the same alignment by truth position: col[p] = (the op that consumed t_p, its call index or None), gap[p] = the call indices inserted between t_(p - 1)
        and t_p (gap[0] and gap[m] are the edges)"""
        ops, t = [int(x) for x in ops], fold(truth)
        s = (call.decode() if isinstance(call, bytes) else call).replace("Z", "C")
        m = len(t)
        if not self._passes(ops):
            return
        self._tot("reads")
        text = "".join("ACGT"[c] for c in t)
        col, gap = [], [[] for _ in range(m + 1)]
        i = 0
        for op in ops:
            if op == 2:
                gap[len(col)].append(i)
                i += 1
            else:
                col.append((op, None if op == 3 else i))
                i += op != 3
        assert len(col) == m and i == len(s)
        for p, (op, at) in enumerate(col):
            self._bump("sub", t[p], 4 if op == 3 else "ACGT".index(s[at]))
            self._tot(("match", "mismatch", None, "del")[op])
            if op != 3:
                self._bump("qual", qv(qual[at]), op)
            if 2 <= p < m - 2:
                self._bump("ctx", int("".join(str(c) for c in t[p - 2:p + 3]), 4), 2 if op == 3 else op)
                self._tot("ctx_sites")
        self._tot("edge_ins", len(gap[0]) + (len(gap[m]) if m > 0 else 0))
        for p in range(1, m):
            for at in gap[p]:
                self._bump("ins", "ACGT".index(s[at]))
                self._bump("qual", qv(qual[at]), 2)
                self._tot("ins")
                if 2 <= p - 1 < m - 2:                           # the gap behind the centre p - 1
                    self._bump("ctx", int("".join(str(c) for c in t[p - 3:p + 2]), 4), 3)
                    self._tot("ctx_sites")
        for mt in re.finditer(r"A+|C+|G+|T+", text):
            a, e = mt.span()
            r, b = e - a, "ACGT".index(text[a])
            if a < 1:
                continue
            if r > HP_MAX_RUN:                                   # read off the first 17 letters: the 17th is not the last
                if a + HP_MAX_RUN + 1 <= m - 1:
                    self._tot("hp_long")
                continue
            if e > m - 1:
                continue
            ins = [at for p in range(a, e + 1) for at in gap[p]]
            if r + len(ins) > HP_MAX_OPS:
                self._tot("hp_wide")
                continue
            c = sum(col[p][0] == 0 for p in range(a, e)) + sum(s[at] == text[a] for at in ins)
            self._bump("hp", b, r - 1, min(c, HP_MAX_CALLED))
            self._tot("hp_runs")

    def tsv_lines(self):
        """errors.tsv as flappie_errprofile_write writes it"""
        sec, out = self.sec, []
        for t in range(4):
            for c in range(5):
                out.append("sub\t%s\t%s\t%d" % ("ACGT"[t], "ACGT-"[c], int(sec["sub"][t, c])))
        for c in range(4):
            out.append("ins\t%s\t%d" % ("ACGT"[c], int(sec["ins"][c])))
        for q in range(94):
            out.append("qual\t%d\t%d\t%d\t%d" % ((q,) + tuple(int(v) for v in sec["qual"][q])))
        for w in range(1024):
            if sec["ctx"][w].any():
                out.append("ctx\t%s\t%d\t%d\t%d\t%d" % (("".join("ACGT"[(w >> (2 * (4 - d))) & 3] for d in range(5)),) + tuple(int(v) for v in sec["ctx"][w])))
        for b in range(4):
            for r in range(HP_MAX_RUN):
                for c in range(HP_MAX_CALLED + 1):
                    if sec["hp"][b, r, c]:
                        out.append("hp\t%s\t%d\t%d\t%d" % ("ACGT"[b], r + 1, c, int(sec["hp"][b, r, c])))
        return out

    def stderr_lines(self):
        return ["errors\t%s\t%d" % (k, self.totals[k]) for k in TOTALS]


def from_tsv(lines):
    """the flat counts of a table's lines"""
    p = ErrProfile()
    for ln in lines:
        f = ln.split("\t")
        if f[0] == "sub":
            p.sec["sub"]["ACGT".index(f[1]), "ACGT-".index(f[2])] = int(f[3])
        elif f[0] == "ins":
            p.sec["ins"]["ACGT".index(f[1])] = int(f[2])
        elif f[0] == "qual":
            p.sec["qual"][int(f[1])] = [int(v) for v in f[2:5]]
        elif f[0] == "ctx":
            p.sec["ctx"][int("".join(str("ACGT".index(c)) for c in f[1]), 4)] = [int(v) for v in f[2:6]]
        elif f[0] == "hp":
            p.sec["hp"]["ACGT".index(f[1]), int(f[2]) - 1, int(f[3])] = int(f[4])
        else:
            raise ValueError(ln)
    return p.counts
