"""Restatement of the remap semantics of include/ffhip.h ("remap") in numpy float32, and a brute-force enumerator of all paths for tiny cases.

A read of N blocks with transition scores T [N][nstate (nbase + 1)], a sequence s of L codes 0 .. nbase - 1 in signal order, a band half-width W:
remap(T, s, nbase, W) -> (score float32, rm uint8 [N]).  One float32 add a term and a strict compare: the result is reproducible to the bit."""
import itertools

import numpy as np

NEG = np.float32(-np.inf)


def trans_lookup(frm, to, nbase):
    """decode.c:104-114"""
    ns = 2 * nbase
    return to * ns + frm if to < nbase else nbase * ns + frm


def flipflop_code(s, nbase):
    q = []
    for i, x in enumerate(s):
        x = int(x)
        if i == 0 or x != int(s[i - 1]):
            q.append(x)
        else:
            q.append(x + nbase if q[-1] < nbase else x)
    return q


def centre(b, L, N):
    return (int(b) * (int(L) - 1)) // int(N)


def _indices(s, nbase):
    q = flipflop_code(s, nbase)
    stay = np.array([trans_lookup(x, x, nbase) for x in q], np.int64)
    move = np.array([0] + [trans_lookup(q[i - 1], q[i], nbase) for i in range(1, len(q))], np.int64)
    return stay, move


def remap(T, s, nbase, W):
    T = np.asarray(T, np.float32)
    N, L = T.shape[0], len(s)
    assert N >= 1 and 1 <= L <= N + 1 and W >= 0
    stay_idx, move_idx = _indices(s, nbase)
    V = np.full(L, NEG, np.float32)
    V[0] = np.float32(0.0)
    bits = []
    with np.errstate(invalid="ignore"):
        for b in range(N):
            c = centre(b + 1, L, N)
            a, e = max(0, c - W), min(L - 1, c + W)
            row = T[b]
            stay = V[a:e + 1] + row[stay_idx[a:e + 1]]
            prev = np.full(e + 1 - a, NEG, np.float32)
            if a == 0:
                prev[1:] = V[0:e]
            else:
                prev[:] = V[a - 1:e]
            move = prev + row[move_idx[a:e + 1]]
            win = move > stay
            V = np.full(L, NEG, np.float32)
            V[a:e + 1] = np.where(win, move, stay)
            bits.append((a, win))
    rm = np.zeros(N, np.uint8)
    p = L - 1
    for b in range(N - 1, -1, -1):
        a, win = bits[b]
        rm[b] = 1 if win[p - a] else 0
        p -= int(rm[b])
    assert p == 0
    return np.float32(V[L - 1]), rm


def brute(T, s, nbase, W):
    """every allowed path; the score of a path is its entries added in block order in float32; the best score, and of the paths that attain it the one
    whose moves read from the LAST block backwards are smallest (what "stay unless the move is strictly greater" picks when the sums are exact)"""
    T = np.asarray(T, np.float32)
    N, L = T.shape[0], len(s)
    q = flipflop_code(s, nbase)
    best = None
    for ones in itertools.combinations(range(N), L - 1):
        rm = np.zeros(N, np.uint8)
        rm[list(ones)] = 1
        p, ok, sc = 0, True, np.float32(0.0)
        for b in range(N):
            pn = p + int(rm[b])
            if abs(pn - centre(b + 1, L, N)) > W:
                ok = False
                break
            sc = np.float32(sc + T[b][trans_lookup(q[p], q[pn], nbase)])
            p = pn
        if not ok:
            continue
        key = (-float(sc), tuple(int(x) for x in rm[::-1]))
        if best is None or key < best[0]:
            best = (key, sc, rm)
    assert best is not None
    return np.float32(best[1]), best[2]


def starts_maxdev(rm, L):
    """start[] (the block each base starts at) and maxdev = max_b |p_b - c(b)|, b = 0 .. N"""
    rm = np.asarray(rm, np.uint8)
    N = rm.size
    start = [0] + [int(b) + 1 for b in np.flatnonzero(rm)]
    assert len(start) == L
    p = np.concatenate([[0], np.cumsum(rm.astype(np.int64))])
    c = np.array([centre(b, L, N) for b in range(N + 1)], np.int64)
    return start, int(np.abs(p - c).max())
