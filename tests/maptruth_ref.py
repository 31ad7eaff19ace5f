"""Restatement of "truth from map" (include/ffhip.h) in plain numpy integers, on top of map_ref.py and truth_ref.py.

  stretch of a map record with status 1, search q = 2 k + o, span [tstart, tend):  y_q[tstart : tend] as codes 0 .. 3, m = tend - tstart bases
  truth of a read in the mode:  map status 1 and 1 <= m <= bound: the stretch, aligned as under "truth";  any other map status: no truth, truth status 0
  bound(N, e) = (N + 1) + (N + 1) e // 1000 for a read of N blocks: a mapped call of n <= N + 1 bases has m <= n + n e // 1000

and of the host side (include/flappie_align.h): the line of acc.tsv in the mode and the lines of the aligned SAM file."""
import numpy as np

import map_ref as R
import truth_ref as T

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def bound(nblock: int, max_error: int) -> int:
    return (int(nblock) + 1) + (int(nblock) + 1) * int(max_error) // 1000


def stretch_text(records, rec: dict):
    """the stretch as letters -- what --map-records writes --, None unless the record says mapped"""
    if rec["status"] != 1:
        return None
    return R.searches(records)[rec["q"]][rec["tstart"]:rec["tend"]]


def codes(text: str):
    return np.array([CODE[c] for c in text], np.uint8)


def stretch(records, q: int, start: int, end: int):
    """y_q[start : end] as codes 0 .. 3 (ffhip_op_map_stretch)"""
    return codes(R.searches(records)[q][start:end])


def no_truth(n: int) -> dict:
    return {"status": 0, "n": n, "m": 0, "dist": 0, "n_match": 0, "n_mismatch": 0, "n_ins": 0, "n_del": 0, "maxdev": 0, "ops": np.zeros(0, np.uint8)}


def truth_from_map(records, call: str, band: int, window: int = 4096, max_error: int = 250, nblock=None, map_rec=None):
    """(the map record, the truth record) of one call in the mode; nblock: the read's blocks (None: the call's n - 1, the smallest a call of n bases can have)"""
    mp = R.record(records, call, window, max_error) if map_rec is None else map_rec
    n = len(call)
    if mp["status"] != 1:
        return mp, no_truth(n)
    t = stretch_text(records, mp)
    m = len(t)
    assert m >= 1
    if m > bound(max(n - 1, 0) if nblock is None else nblock, max_error):      # (cannot be: test_maptruth.py holds the bound)
        out = no_truth(n)
        out.update(status=2, m=m)
        return mp, out
    return mp, T.truth(call, codes(t), band)


# ---- the host side (include/flappie_align.h)
def acc_line(name: str, tr: dict, band: int, mp: dict, names, lens) -> str:
    """the line of acc.tsv in the mode: truth's thirteen columns, then record, strand, tstart, tend of hits.tsv"""
    k, o, a, b = R.forward(mp["q"], mp["tstart"], mp["tend"], lens)
    return T.tsv_line(name, tr, band)[:-1] + "\t%s\t%s\t%d\t%d\n" % (names[k], o, a, b)


def sam_header(names, lens) -> str:
    return "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (nm, m) for nm, m in zip(names, lens)) + "@PG\tID:flappie\n"


def sam_line(name: str, call: str, qual: str, tr, mp, names, lens) -> str:
    """one line of aln.sam: call and qual in signal order; tr / mp None for a read without a truth record"""
    seq = call.replace("Z", "C")
    if tr is None or mp is None or mp["status"] != 1 or tr["status"] != 1:
        return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, seq or "*", qual or "*")
    k, o, a, b = R.forward(mp["q"], mp["tstart"], mp["tend"], lens)
    ops = tr["ops"] if o == "+" else tr["ops"][::-1]
    if o == "-":
        seq, qual = R.revcomp(seq), qual[::-1]
    return "%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\n" % (name, 0 if o == "+" else 16, names[k], a + 1, T.cigar(ops), seq, qual, tr["dist"])


def replay(line: str, ref: dict) -> dict:
    """an aligned SAM line replayed over the reference (name -> sequence): asserts that its CIGAR consumes all of SEQ, has equal letters at every = and different
    ones at every X, and that NM is X + I + D; returns {"start", "end" (forward strand, half open), "nm", "flag"}"""
    import re
    f = line.rstrip("\n").split("\t")
    flag, rname, pos, cig, seq, qual = int(f[1]), f[2], int(f[3]), f[5], f[9], f[10]
    assert flag in (0, 16) and f[4] == "255" and f[6:9] == ["*", "0", "0"] and len(seq) == len(qual), line
    y = ref[rname]
    parts = re.findall(r"(\d+)([=XID])", cig)
    assert "".join(n + c for n, c in parts) == cig and parts, cig
    i, j, nm = 0, pos - 1, 0
    for cnt, op in parts:
        cnt = int(cnt)
        assert cnt >= 1
        if op == "=":
            assert seq[i:i + cnt] == y[j:j + cnt] and len(y[j:j + cnt]) == cnt, (line, i, j)
            i, j = i + cnt, j + cnt
        elif op == "X":
            assert len(y[j:j + cnt]) == cnt and all(a != b for a, b in zip(seq[i:i + cnt], y[j:j + cnt])), (line, i, j)
            i, j, nm = i + cnt, j + cnt, nm + cnt
        elif op == "I":
            i, nm = i + cnt, nm + cnt
        else:
            j, nm = j + cnt, nm + cnt
    assert i == len(seq) and j <= len(y), line
    tags = dict(t.split(":", 2)[::2] for t in f[11:])
    assert int(tags["NM"]) == nm, line
    return {"start": pos - 1, "end": j, "nm": nm, "flag": flag}
