"""Restatement of the remap semantics of include/ffhip.h ("remap") in numpy float32, and a brute-force enumerator of all paths for tiny cases.

A read of N blocks with transition scores T [N][nstate (nbase + 1)], a sequence s of L codes 0 .. nbase - 1 in signal order, a band half-width W:
remap(T, s, nbase, W) -> (score float32, rm uint8 [N]).  One float32 add a term and a strict compare: the result is reproducible to the bit.
remap_status(T, s, nbase, W) -> (status, score, rm) for scores of any kind: a score that is not finite is status 2 and has no path."""
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


def _forward(T, s, nbase, W):
    """the recursion: (V_N, [(a, win)] a block: the first allowed cell and the bits of the allowed cells)"""
    T = np.asarray(T, np.float32)
    N, L = T.shape[0], len(s)
    assert N >= 1 and 1 <= L <= N + 1 and W >= 0
    stay_idx, move_idx = _indices(s, nbase)
    V = np.full(L, NEG, np.float32)
    V[0] = np.float32(0.0)
    bits = []
    with np.errstate(invalid="ignore", over="ignore"):
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
    return V, bits


def traceback(bits, L):
    """follow the bits from (N, L - 1): (rm, the position it ends at, whether it stayed on allowed cells, position 0 included).  A cell outside a block's allowed
    cells has no bit in this restatement (in a kernel: some other cell's); it reads as 0 and the walk is marked as having left."""
    N = len(bits)
    rm = np.zeros(N, np.uint8)
    p, inside = L - 1, True
    for b in range(N - 1, -1, -1):
        a, win = bits[b]
        if p < a or p - a >= win.size:
            inside = False
        elif win[p - a]:
            rm[b] = 1
            if p == 0:
                inside = False
            p -= 1
    return rm, p, inside


def remap(T, s, nbase, W):
    V, bits = _forward(T, s, nbase, W)
    rm, p, inside = traceback(bits, len(s))
    assert p == 0 and inside
    return np.float32(V[len(s) - 1]), rm


def remap_status(T, s, nbase, W):
    """(status, score, rm) by the rule of "remap": mapped (1, score, rm) iff V_N[L - 1] is finite; otherwise (2, 0.0, None), "not mapped: the scores leave no
    finite path", and no bit is followed"""
    V, bits = _forward(T, s, nbase, W)
    score = np.float32(V[len(s) - 1])
    if not np.isfinite(score):
        return 2, np.float32(0.0), None
    rm, p, inside = traceback(bits, len(s))
    assert p == 0 and inside
    return 1, score, rm


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
