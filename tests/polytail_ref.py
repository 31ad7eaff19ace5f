"""The poly tail of include/ffhip.h ("poly tail") once more, in plain Python and numpy float64: the windows' sums sample after sample, the merge of step 4 as a walk
over the flags, the tie rules of step 5, the record and the rate.  candidates_scan is a second, scan-shaped statement of step 4 (what k_polytail's two scans are
built on); tests/test_polytail.py holds the two to each other.  Nothing here imports the package.

check(got, want, x): every integer field, rate and bases bit for bit; level within 2^-23 max|x| over the interval (events_ref.tolerance's argument: the fp64 sums
differ by far less than one float32 rounding of the result)."""
import numpy as np

POLYTAIL_DTYPE = np.dtype([("status", np.int32), ("first", np.int32), ("count", np.int32), ("flat", np.int32), ("calls", np.int32),
                           ("level", np.float32), ("rate", np.float32), ("bases", np.float32)])
PARAM_FIELDS = ("base", "from_end", "window", "min_calls", "gap", "min_windows", "search", "min_bases", "max_sd")
DEFAULTS = dict(base=0, from_end=0, window=8, min_calls=4, gap=2, min_windows=5, search=500, min_bases=20, max_sd=0.3)


def params(**kw):
    p = dict(DEFAULTS)
    if "window" in kw and "min_calls" not in kw:
        p["min_calls"] = (kw["window"] + 1) // 2
    p.update(kw)
    assert set(p) == set(PARAM_FIELDS), sorted(p)
    return p


def block_bases(path, nbase):
    """step 1: base_b = path[b + 1] % nbase, Z read as C"""
    b = np.asarray(path, np.int64)[1:] % nbase
    return np.where(b == 4, 1, b)


def moves(path):
    """the move table of include/ffhip.h: mv[b] = 1 iff b <= N - 2 and path[b + 1] != path[b]"""
    path = np.asarray(path, np.int64)
    mv = (path[1:] != path[:-1]).astype(np.int64)
    mv[-1] = 0
    return mv


def nwindows(n, S, N, K):
    return min(N, n // S) // K


def windows(x, S, path, nbase, p):
    """steps 2 and 3: (mu, q, flag, threshold) of the NW windows; every sum runs sample after sample (the loop is over a window's samples, all windows abreast)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    N, K = len(path) - 1, p["window"]
    NW, KS = nwindows(x.size, S, N, K), p["window"] * S
    X = x[:NW * KS].reshape(NW, KS)
    a = np.zeros(NW)
    for k in range(KS):
        a = a + X[:, k]
    mu = a / float(KS)
    q = np.zeros(NW)
    for k in range(KS):
        d = X[:, k] - mu
        q = q + d * d
    sd = float(np.float32(p["max_sd"]))
    thr = (sd * sd) * float(KS)
    calls = (block_bases(path, nbase)[:NW * K].reshape(NW, K) == p["base"]).sum(axis=1)
    with np.errstate(invalid="ignore"):
        flag = (q <= thr) & (calls >= p["min_calls"])
    return mu, q, flag.astype(np.uint8), thr


def margin(q, thr):
    """min_w |q_w - threshold| / threshold: how far the nearest window is from changing its flag (inf without windows or with a threshold of 0)"""
    q = np.asarray(q, np.float64)
    return float(np.min(np.abs(q - thr)) / thr) if q.size and thr > 0 else float("inf")


def candidates(flag, G):
    """step 4 as a walk: the maximal runs [ws, we) of flagged windows merged across at most G unflagged ones"""
    out, ws, last = [], None, None
    for w, f in enumerate(flag):
        if not f:
            continue
        if ws is None:
            ws = w
        elif w - last - 1 > G:
            out.append((ws, last + 1))
            ws = w
        last = w
    if ws is not None:
        out.append((ws, last + 1))
    return out


def candidates_scan(flag, G):
    """step 4 as scans: prev[w] the last flagged window at or before w (an inclusive max-scan), next[w] the next at or after w (a reverse min-scan);
    merged_w = flag_w, or both exist and next - prev - 1 <= G; starts and ends from neighbours"""
    flag = np.asarray(flag).astype(bool)
    NW = flag.size
    if NW == 0:
        return []
    idx = np.arange(NW)
    prev = np.maximum.accumulate(np.where(flag, idx, -1))
    nxt = np.minimum.accumulate(np.where(flag, idx, NW)[::-1])[::-1]
    merged = flag | ((prev >= 0) & (nxt < NW) & (nxt - prev - 1 <= G))
    m = np.concatenate(([False], merged, [False]))
    starts = np.flatnonzero(m[1:-1] & ~m[:-2])
    ends = np.flatnonzero(m[1:-1] & ~m[2:]) + 1
    return list(zip(starts.tolist(), ends.tolist()))


def choose(cands, NW, p):
    """step 5: the winner (ws, we) or None"""
    R, best = p["search"], None
    for ws, we in cands:
        if we - ws < p["min_windows"] or not (we > NW - R if p["from_end"] else ws < R):
            continue
        if best is None or we - ws > best[1] - best[0] or (we - ws == best[1] - best[0] and p["from_end"]):
            best = (ws, we)         # (in window order: a later one of equal length wins only from the end)
    return best


def record(x, S, path, nbase, p, scan=False):
    """steps 1 .. 7: the read's record (a numpy scalar of POLYTAIL_DTYPE)"""
    x = np.asarray(x, np.float32)
    path = np.asarray(path, np.int64)
    N, K, n, t = len(path) - 1, p["window"], x.size, p["base"]
    assert N >= 1 and path.min() >= 0 and path.max() < 2 * nbase
    out = np.zeros((), POLYTAIL_DTYPE)
    mu, _, flag, _ = windows(x, S, path, nbase, p)
    win = choose((candidates_scan if scan else candidates)(flag, p["gap"]), flag.size, p)
    if win is None:
        out["status"] = 2
        return out
    ws, we = win
    bs, be = ws * K, we * K
    mv, base = moves(path), block_bases(path, nbase)
    fl = flag[ws:we].astype(bool)
    out["first"], out["count"], out["flat"] = bs * S, (be - bs) * S, int(fl.sum())
    out["calls"] = int(((mv[bs:be] == 1) & (base[bs:be] == t)).sum())
    out["level"] = np.float32(mu[ws:we][fl].sum() / float(fl.sum()))
    if p["from_end"]:
        c, so = int(mv[:bs].sum()), bs * S
    else:
        c, so = int(mv[be:].sum()), min(N * S, n) - be * S
    if c < p["min_bases"] or so <= 0:
        out["status"] = 3
        return out
    out["status"] = 1
    out["rate"] = np.float32(float(so) / float(c))
    out["bases"] = np.float32((float(out["count"]) * float(c)) / float(so))
    return out


def check(got, want, x, where=None):
    """every integer field, rate and bases bit for bit; level within 2^-23 max|x| over the interval"""
    got = np.asarray(got)
    assert got.dtype == POLYTAIL_DTYPE and got.shape == (), (where, got.dtype, got.shape)
    for f in ("status", "first", "count", "flat", "calls"):
        assert int(got[f]) == int(want[f]), (where, f, int(got[f]), int(want[f]), got, want)
    for f in ("rate", "bases"):
        assert got[f].tobytes() == np.asarray(want[f]).tobytes(), (where, f, float(got[f]), float(want[f]))
    if int(want["status"]) in (1, 3):
        seg = np.abs(np.asarray(x, np.float32).astype(np.float64)[int(want["first"]):int(want["first"]) + int(want["count"])])
        tol = 2.0 ** -23 * seg.max()
        assert abs(float(got["level"]) - float(want["level"])) <= tol, (where, "level", float(got["level"]), float(want["level"]), tol)
    else:
        assert got["level"].tobytes() == b"\0\0\0\0", (where, "level", float(got["level"]))


def path_of_bases(bases, nbase=4):
    """a path of N + 1 flip states whose block b holds bases[b] (entry 0 repeats the first): equal neighbours are stays, a new base is a move"""
    bases = np.asarray(bases, np.int64)
    return np.concatenate(([bases[0]], bases)).astype(np.int32)
