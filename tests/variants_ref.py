"""Restatement of the "variants" semantics of include/ffhip.h in numpy, on the pieces of sitemods_ref.py (starts, score_best, score_all, brute, check's rule).

A read of N blocks with transition scores T [N][nstate (nbase + 1)], nbase 4 or 5, a sequence `codes` of L codes in signal order, its remap path rm (a byte a
block, L - 1 ones), a list of variants (pos, nref, alt codes), a context c (1 .. 23) and a mode:
variants(T, nbase, codes, rm, vars, c, all_paths) -> VARIANT_CALL_DTYPE, one record a variant in list order.
Best-path scores are float32, one rounded add a term: reproducible to the bit.  All-paths scores are float64, rounded to float32 once."""
import numpy as np

from remap_ref import flipflop_code
from sitemods_ref import SITE_MOD_DTYPE, brute, score_all, score_best, starts      # noqa: F401 (brute: for the tests)
from sitemods_ref import check as sitemods_check
from sitemods_ref import check_hostile as sitemods_check_hostile

VARIANT_DTYPE = np.dtype([("pos", np.int32), ("nref", np.uint8), ("nalt", np.uint8), ("alt", np.uint8, (16,)), ("pad", np.uint8, (2,))])
VARIANT_CALL_DTYPE = np.dtype([("index", np.int32), ("nblock", np.int32), ("ref", np.float32), ("alt", np.float32)])
MIN_CONTEXT, MAX_CONTEXT, MAX_ALLELE, MAX_POSITIONS = 1, 23, 16, 62


def valid(L, nbase, p, r, alt):
    k = len(alt)
    return (0 <= r <= MAX_ALLELE and 0 <= k <= MAX_ALLELE and r + k >= 1 and 0 <= p and p + r <= L and all(0 <= int(x) < nbase for x in alt)
            and L - r + k >= 1)


def pack(vars):
    """(pos, nref, alt codes) triples as an array of VARIANT_DTYPE"""
    out = np.zeros(len(vars), VARIANT_DTYPE)
    for i, (p, r, alt) in enumerate(vars):
        out[i]["pos"], out[i]["nref"], out[i]["nalt"] = p, r, len(alt)
        out[i]["alt"][:len(alt)] = alt
    return out


def unpack(packed):
    return [(int(v["pos"]), int(v["nref"]), [int(x) for x in v["alt"][:int(v["nalt"])]]) for v in packed]


def edited(codes, p, r, alt):
    """s^alt = s[0:p] + alt + s[p+r:]"""
    s = [int(x) for x in codes]
    return s[:p] + [int(x) for x in alt] + s[p + r:]


def window(start, L, p, r, k, c):
    """(lo, hi, P_ref, P_alt, t0, t1): positions lo .. hi of s, lo .. lo + P_alt - 1 of s^alt, blocks t0 .. t1 - 1"""
    N = start[L]
    lo, hi = max(0, p - c), min(L - 1, p + r + c - 1)
    P_ref = hi - lo + 1
    P_alt = P_ref - r + k
    assert 1 <= P_ref <= MAX_POSITIONS and 1 <= P_alt <= MAX_POSITIONS, (L, p, r, k, c)
    t0 = start[lo]
    t1 = start[hi + 1] - 1 if hi < L - 1 else N
    assert t1 - t0 >= P_ref - 1
    return lo, hi, P_ref, P_alt, t0, t1


def hypotheses(codes, nbase, p, r, alt):
    """(q_ref, q_alt): the flip-flop codings of the WHOLE s and of the WHOLE s^alt"""
    return flipflop_code([int(x) for x in codes], nbase), flipflop_code(edited(codes, p, r, alt), nbase)


def variants(T, nbase, codes, rm, vars, c, all_paths=False):
    assert nbase in (4, 5) and MIN_CONTEXT <= c <= MAX_CONTEXT
    L = len(codes)
    st = starts(rm, L)
    out = np.zeros(len(vars), VARIANT_CALL_DTYPE)
    score = score_all if all_paths else score_best
    for i, (p, r, alt) in enumerate(vars):
        assert valid(L, nbase, p, r, alt), (i, p, r, alt)
        lo, hi, P_ref, P_alt, t0, t1 = window(st, L, p, r, len(alt), c)
        q_ref, q_alt = hypotheses(codes, nbase, p, r, alt)
        assert q_ref[:p] == q_alt[:p]
        ref = score(T, q_ref, lo, hi, t0, t1, nbase)
        alt_score = score(T, q_alt, lo, lo + P_alt - 1, t0, t1, nbase)
        with np.errstate(over="ignore"):
            out[i] = (i, t1 - t0, np.float32(ref), np.float32(alt_score))
    return out


def check(got, want, all_paths, where):
    """sitemods_ref.check's rule on records of the same layout: best path byte for byte; all paths index and nblock equal, ref and alt within 1 float32 ulp, no NaN"""
    assert got.dtype == VARIANT_CALL_DTYPE and want.dtype == VARIANT_CALL_DTYPE, where
    sitemods_check(got.view(SITE_MOD_DTYPE), want.view(SITE_MOD_DTYPE), all_paths, where)


def check_hostile(got, want, all_paths, where):
    """sitemods_ref.check_hostile's rule, for scores of any kind: a NaN equal to a NaN, +-inf equal"""
    assert got.dtype == VARIANT_CALL_DTYPE and want.dtype == VARIANT_CALL_DTYPE, where
    sitemods_check_hostile(got.view(SITE_MOD_DTYPE), want.view(SITE_MOD_DTYPE), all_paths, where)
