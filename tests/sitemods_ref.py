"""Restatement of the "site mods" semantics of include/ffhip.h in numpy, and a brute-force enumerator of every monotone path for tiny windows.

A read of N blocks with transition scores T [N][nstate (nbase + 1)], nbase = 5 (A 0, C 1, G 2, T 3, Z 4), a sequence `codes` of L codes in signal order, its remap
path rm (a byte a block, L - 1 ones), a context c (0 .. 31) and a mode: site_mods(T, nbase, codes, rm, c, all_paths) -> SITE_MOD_DTYPE, one record a C / Z.
Best-path scores are float32, one rounded add a term: reproducible to the bit.  All-paths scores are float64, rounded to float32 once."""
import itertools

import numpy as np

from remap_ref import flipflop_code, trans_lookup

SITE_MOD_DTYPE = np.dtype([("pos", np.int32), ("nblock", np.int32), ("can", np.float32), ("mod", np.float32)])
CAN, MOD = 1, 4
MAX_CONTEXT = 31


def sites(codes):
    """every i with s_i in {C, Z}, in increasing i"""
    return [i for i, x in enumerate(codes) if int(x) in (CAN, MOD)]


def starts(rm, L):
    """start[0 .. L]: the block every base starts at, start[L] = N"""
    rm = np.asarray(rm, np.uint8)
    st = [0] + [int(b) + 1 for b in np.flatnonzero(rm)] + [int(rm.size)]
    assert len(st) == L + 1, (len(st), L)
    return st


def window(start, L, i, c):
    """(lo, hi, t0, t1) of site i: positions lo .. hi, blocks t0 .. t1 - 1"""
    N = start[L]
    lo, hi = max(0, i - c), min(L - 1, i + c)
    t0 = start[lo]
    t1 = start[hi + 1] - 1 if hi < L - 1 else N
    assert t1 - t0 >= hi - lo
    return lo, hi, t0, t1


def code_hypothesis(codes, i, letter, nbase):
    """the flip-flop coding of the WHOLE sequence with position i set to `letter`"""
    s = [int(x) for x in codes]
    s[i] = int(letter)
    return flipflop_code(s, nbase)


def _indices(q, lo, hi, nbase):
    stay = np.array([trans_lookup(q[j], q[j], nbase) for j in range(lo, hi + 1)], np.int64)
    move = np.array([0] + [trans_lookup(q[j - 1], q[j], nbase) for j in range(lo + 1, hi + 1)], np.int64)
    return stay, move


def score_best(T, q, lo, hi, t0, t1, nbase):
    """float32; X_{t+1}[j] = move if move > stay (strictly) else stay, each term one rounded add"""
    T = np.asarray(T, np.float32)
    stay_idx, move_idx = _indices(q, lo, hi, nbase)
    P = hi - lo + 1
    X = np.full(P, -np.inf, np.float32)
    X[0] = np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(t0, t1):
            row = T[t]
            stay = X + row[stay_idx]
            move = np.full(P, -np.inf, np.float32)
            move[1:] = X[:-1] + row[move_idx[1:]]
            X = np.where(move > stay, move, stay).astype(np.float32)
    return np.float32(X[P - 1])


def score_all(T, q, lo, hi, t0, t1, nbase):
    """float64, IEEE arithmetic as written: m = move if move > stay else stay; X_{t+1}[j] = -inf if m == -inf else m + log1p(exp(-|stay - move|)).
    From finite or -inf scores never a NaN; a NaN entry, or +inf met by +inf, on a term gives NaN."""
    T = np.asarray(T, np.float32).astype(np.float64)
    stay_idx, move_idx = _indices(q, lo, hi, nbase)
    P = hi - lo + 1
    X = np.full(P, -np.inf, np.float64)
    X[0] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(t0, t1):
            row = T[t]
            stay = X + row[stay_idx]
            move = np.full(P, -np.inf, np.float64)
            move[1:] = X[:-1] + row[move_idx[1:]]
            m = np.where(move > stay, move, stay)
            X = np.where(m == -np.inf, -np.inf, m + np.log1p(np.exp(-np.abs(stay - move))))
    return np.float64(X[P - 1])


def site_mods(T, nbase, codes, rm, c, all_paths=False):
    assert nbase == 5 and 0 <= c <= MAX_CONTEXT
    L = len(codes)
    st = starts(rm, L)
    where = sites(codes)
    out = np.zeros(len(where), SITE_MOD_DTYPE)
    score = score_all if all_paths else score_best
    for k, i in enumerate(where):
        lo, hi, t0, t1 = window(st, L, i, c)
        can = score(T, code_hypothesis(codes, i, CAN, nbase), lo, hi, t0, t1, nbase)
        mod = score(T, code_hypothesis(codes, i, MOD, nbase), lo, hi, t0, t1, nbase)
        with np.errstate(over="ignore"):
            out[k] = (i, t1 - t0, np.float32(can), np.float32(mod))
    return out


def brute(T, q, lo, hi, t0, t1, nbase):
    """every monotone path from (t0, lo) to (t1, hi): (the best float32 in-order sum, log(sum(exp)) of the float64 sums computed directly)"""
    T32 = np.asarray(T, np.float32)
    T64 = T32.astype(np.float64)
    n, P = t1 - t0, hi - lo + 1
    best, sums = None, []
    for ones in itertools.combinations(range(n), P - 1):
        p, s32, s64 = lo, np.float32(0.0), 0.0
        for k in range(n):
            pn = p + (1 if k in ones else 0)
            e = trans_lookup(q[p], q[pn], nbase)
            s32 = np.float32(s32 + T32[t0 + k][e])
            s64 += float(T64[t0 + k][e])
            p = pn
        best = s32 if best is None or s32 > best else best
        sums.append(s64)
    if not sums:
        return np.float32(-np.inf), -np.inf
    a = np.array(sums, np.float64)
    return np.float32(best), float(a.max() + np.log(np.exp(a - a.max()).sum()))


def path_sum(T, q, rm, lo, t0, t1, nbase):
    """the float32 in-order sum of the remap path's own terms over blocks t0 .. t1 - 1, starting at position lo"""
    T = np.asarray(T, np.float32)
    p, s = lo, np.float32(0.0)
    for t in range(t0, t1):
        pn = p + int(rm[t])
        s = np.float32(s + T[t][trans_lookup(q[p], q[pn], nbase)])
        p = pn
    return s, p


def ulp32(x):
    return float(np.spacing(np.abs(np.float32(x)))) if np.isfinite(x) else 0.0


def check_hostile(got, want, all_paths, where):
    """scores of any kind.  Best path: equal to the bit, a NaN equal to a NaN whatever its payload or sign.  All paths: pos and nblock equal, the same NaN
    pattern, +-inf equal, finite values within 1 float32 ulp."""
    assert got.dtype == SITE_MOD_DTYPE and got.shape == want.shape, (where, got.shape, want.shape)
    assert np.array_equal(got["pos"], want["pos"]) and np.array_equal(got["nblock"], want["nblock"]), where
    for f in ("can", "mod"):
        g, w = got[f], want[f]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, f, g, w)
        ok = ~np.isnan(w)
        if not all_paths:
            assert g[ok].tobytes() == w[ok].tobytes(), (where, f, g, w)
            continue
        for x, y in zip(g[ok], w[ok]):
            assert x == y or (np.isfinite(x) and np.isfinite(y) and abs(float(x) - float(y)) <= ulp32(y)), (where, f, x, y)


def check(got, want, all_paths, where):
    """scores that are finite or -inf.  Best path: byte for byte.  All paths: pos and nblock equal, can and mod within 1 float32 ulp, no NaN."""
    assert got.dtype == SITE_MOD_DTYPE and got.shape == want.shape, (where, got.shape, want.shape)
    if not all_paths:
        assert got.tobytes() == want.tobytes(), (where, got, want)
        return
    for f in ("can", "mod"):
        assert not np.any(np.isnan(got[f])) and not np.any(np.isnan(want[f])), (where, f)
    check_hostile(got, want, all_paths, where)
