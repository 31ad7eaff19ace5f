"""The statement of include/ffhip.h "events" once more, in numpy float64: the signal under every base of a mapped read.

  spans(n, stride, rm, L)      first sample and sample count of every base: start[0] = 0, start[i] = 1 + (index of the i-th one of rm), start[L] = N,
                               s_i = min(start[i] stride, n), e_i = min(start[i + 1] stride, n)
  events(x, stride, rm, L)     the L events { first, count, mean, sd }: two passes in float64 over the span, the population form, each rounded to float32 once
  events_naive(...)            the same with a Python loop and math.fsum (exactly rounded sums), for cross-checking
  tolerance(x, ev)             per base 2^-23 max|x| over its span: two float32 roundings of at most half an ulp of a value bounded by max|x| (the float64
                               accumulation error, count 2^-53 max|x|, is negligible below 2^24 samples)
"""
import math

import numpy as np

EVENT_DTYPE = np.dtype([("first", np.int32), ("count", np.int32), ("mean", np.float32), ("sd", np.float32)])


def spans(n, stride, rm, L):
    rm = np.asarray(rm)
    N = rm.size
    ones = np.flatnonzero(rm)
    assert L >= 1 and ones.size == L - 1 and stride >= 1 and N >= 1, (L, ones.size, stride, N)
    start = np.concatenate(([0], ones + 1, [N])).astype(np.int64)
    s = np.minimum(start[:-1] * stride, n)
    e = np.minimum(start[1:] * stride, n)
    return s, e - s


def rm_of_starts(start, N):
    """the path's bytes from the block every base starts at (map.tsv's last column)"""
    rm = np.zeros(N, np.uint8)
    for b in start[1:]:
        rm[b - 1] = 1
    return rm


def events(x, stride, rm, L):
    x = np.asarray(x, np.float32).astype(np.float64)
    s, c = spans(x.size, stride, rm, L)
    out = np.zeros(L, EVENT_DTYPE)
    out["first"], out["count"] = s, c
    for i in np.flatnonzero(c):
        seg = x[s[i]:s[i] + c[i]]
        mu = seg.sum() / c[i]
        d = seg - mu
        out["mean"][i] = mu
        out["sd"][i] = math.sqrt((d * d).sum() / c[i])
    return out


def events_naive(x, stride, rm, L):
    x = [float(np.float32(v)) for v in x]
    n, N = len(x), len(rm)
    start, out = [0], np.zeros(L, EVENT_DTYPE)
    for b in range(N):
        if rm[b]:
            start.append(b + 1)
    start.append(N)
    assert len(start) == L + 1
    for i in range(L):
        s, e = min(start[i] * stride, n), min(start[i + 1] * stride, n)
        out[i]["first"], out[i]["count"] = s, e - s
        if e > s:
            mu = math.fsum(x[s:e]) / (e - s)
            out[i]["mean"] = mu
            out[i]["sd"] = math.sqrt(math.fsum((v - mu) * (v - mu) for v in x[s:e]) / (e - s))
    return out


def tolerance(x, ev):
    x = np.abs(np.asarray(x, np.float32).astype(np.float64))
    return np.array([2.0 ** -23 * x[f:f + c].max() if c else 0.0 for f, c in zip(ev["first"], ev["count"])])


def check(got, want, x, where=None):
    """first and count exact; mean and sd within tolerance(x, want); a span without samples has zeros"""
    got = np.asarray(got)
    assert got.dtype == EVENT_DTYPE and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    assert np.array_equal(got["first"], want["first"]) and np.array_equal(got["count"], want["count"]), where
    tol = tolerance(x, want)
    for f in ("mean", "sd"):
        err = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64))
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, (where, f, bad[:4], got[f][bad[:4]], want[f][bad[:4]], tol[bad[:4]])


def check_hostile(got, want, x, where=None):
    """check's rule for a signal with samples that are not finite: first and count exact; mean and sd NaN exactly where the statement's are, +-inf equal, every
    finite one within tolerance(x, want) as in check"""
    got = np.asarray(got)
    assert got.dtype == EVENT_DTYPE and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    assert np.array_equal(got["first"], want["first"]) and np.array_equal(got["count"], want["count"]), where
    with np.errstate(invalid="ignore"):
        tol = tolerance(x, want)
    for f in ("mean", "sd"):
        g, w = got[f].astype(np.float64), want[f].astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (where, f, np.flatnonzero(np.isnan(g) != np.isnan(w))[:4])
        inf = np.isinf(w)
        assert np.array_equal(g[inf], w[inf]), (where, f, g[inf][:4], w[inf][:4])
        fin = np.isfinite(w)
        bad = np.flatnonzero(fin)[~(np.abs(g[fin] - w[fin]) <= tol[fin])]
        assert bad.size == 0, (where, f, bad[:4], got[f][bad[:4]], want[f][bad[:4]], tol[bad[:4]])


def rm_of_lengths(blocks):
    """the path of bases that hold these many blocks each (the last may hold none: L = N + 1)"""
    N = int(sum(blocks))
    rm = np.zeros(N, np.uint8)
    at = 0
    for k in blocks[:-1]:
        at += k
        rm[at - 1] = 1
    return rm


def special_cases():
    """(name, x, stride, rm, L, constant): the inputs that rule out a one-pass sum of squares and a lane a base; constant: every span holds one repeated value, so
    mean is that value and sd is 0.0 exactly"""
    rng = np.random.default_rng(11)
    # one repeated float a span, spans of 1, 5 and 1000 samples (stride 1), and of 5, 1000 and -- the read ends inside its last block -- 1 sample (stride 5)
    vals = np.array([1000.1, -3.3, 7e-5], np.float32)
    yield "constant, stride 1", np.repeat(vals, [1, 5, 1000]), 1, rm_of_lengths([1, 5, 1000]), 3, True
    yield "constant, stride 5", np.repeat(vals, [5, 1000, 1]), 5, rm_of_lengths([1, 200, 1]), 3, True
    yield "one value", np.full(1000, 1000.1, np.float32), 5, rm_of_lengths([1, 1, 198]), 3, True
    # a small spread on a large level
    N = 300
    rm = np.zeros(N, np.uint8)
    rm[rng.choice(N, 40, replace=False)] = 1
    yield "1000 + 1e-3 noise", (1000.0 + 1e-3 * rng.standard_normal(N * 5)).astype(np.float32), 5, rm, 41, False
    # large and small magnitudes of both signs in one span
    x = rng.choice(np.array([1e4, -1e4, 1e-4, -1e-4], np.float32), N * 5) * (1.0 + 0.25 * rng.random(N * 5)).astype(np.float32)
    yield "+-1e4 with +-1e-4", x.astype(np.float32), 5, rm, 41, False
    yield "+-1e4 with +-1e-4, one base", x.astype(np.float32), 5, np.zeros(N, np.uint8), 1, False
    # one base of 3900 blocks between 100 bases of one block
    yield "long span", rng.standard_normal(4000 * 5).astype(np.float32), 5, rm_of_lengths([1] * 50 + [3900] + [1] * 50), 101, False
