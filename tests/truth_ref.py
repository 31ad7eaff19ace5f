"""Restatement of the truth semantics of include/ffhip.h ("truth") in numpy integers.

A call s of n bases (letters A C G T Z, or codes), a truth t of m codes 0 .. nbase - 1, a band half-width W:
truth(call, t, W) -> dict(status, n, m, dist, n_match, n_mismatch, n_ins, n_del, maxdev, ops uint8 [dist + n_match]).
Everything is an integer: results are compared with exact equality."""
import numpy as np

INF = 1 << 40
OPS = "=XID"          # op codes 0 .. 3
FIELDS = ("status", "n", "m", "dist", "n_match", "n_mismatch", "n_ins", "n_del", "maxdev")


def call_codes(call):
    """the called letters as the comparison reads them: Z is C"""
    if isinstance(call, (bytes, str)):
        s = call.decode() if isinstance(call, bytes) else call
        return np.array(["ACGT".index("C" if ch == "Z" else ch) for ch in s], np.int64)
    return fold(call)


def fold(codes):
    c = np.asarray(codes, np.int64).reshape(-1).copy()
    c[c == 4] = 1
    return c


def centre(j, n, m):
    return (int(j) * int(n)) // int(m)


def _empty(status, n, m):
    return {"status": status, "n": n, "m": m, "dist": 0, "n_match": 0, "n_mismatch": 0, "n_ins": 0, "n_del": 0, "maxdev": 0, "ops": np.zeros(0, np.uint8)}


def truth(call, t, W):
    s, t = call_codes(call), fold(t)
    n, m, W = int(s.size), int(t.size), int(W)
    assert W >= 0
    if m == 0:
        return _empty(2, n, m)
    idx = np.arange(n + 1, dtype=np.int64)
    D = np.full((m + 1, n + 1), INF, np.int64)
    lim = np.zeros((m + 1, 2), np.int64)
    for j in range(m + 1):
        c = centre(j, n, m)
        a, e = max(0, c - W), min(n, c + W)
        lim[j] = a, e
        if j == 0:
            best = np.full(e + 1 - a, INF, np.int64)
            if a == 0:
                best[0] = 0
        else:
            up = D[j - 1, a:e + 1] + 1                       # (+inf + 1 stays beyond every distance)
            diag = np.full(e + 1 - a, INF, np.int64)
            lo = max(a, 1)
            diag[lo - a:] = D[j - 1, lo - 1:e] + (s[lo - 1:e] != t[j - 1])
            best = np.minimum(up, diag)
        # D[j][i] = min(best_i, D[j][i-1] + 1) = i + prefix-min(best_k - k) over the row's allowed cells
        row = idx[a:e + 1] + np.minimum.accumulate(best - idx[a:e + 1])
        D[j, a:e + 1] = np.where(row >= INF // 2, INF, row)
    if D[m, n] >= INF:
        return _empty(2, n, m)

    def allowed(j, i):
        return lim[j, 0] <= i <= lim[j, 1]

    ops, j, i, maxdev = [], m, n, 0
    while j > 0 or i > 0:
        maxdev = max(maxdev, abs(i - centre(j, n, m)))
        if j > 0 and i > 0 and allowed(j - 1, i - 1) and D[j - 1, i - 1] + int(s[i - 1] != t[j - 1]) == D[j, i]:
            ops.append(int(s[i - 1] != t[j - 1]))
            j, i = j - 1, i - 1
        elif j > 0 and allowed(j - 1, i) and D[j - 1, i] + 1 == D[j, i]:
            ops.append(3)
            j -= 1
        else:
            assert i > 0 and allowed(j, i - 1) and D[j, i - 1] + 1 == D[j, i]
            ops.append(2)
            i -= 1
    ops = np.array(ops[::-1], np.uint8)
    cnt = np.bincount(ops, minlength=4)
    out = {"status": 1, "n": n, "m": m, "dist": int(D[m, n]), "n_match": int(cnt[0]), "n_mismatch": int(cnt[1]), "n_ins": int(cnt[2]), "n_del": int(cnt[3]),
           "maxdev": int(maxdev), "ops": ops}
    assert out["n_match"] + out["n_mismatch"] + out["n_ins"] == n and out["n_match"] + out["n_mismatch"] + out["n_del"] == m
    assert out["dist"] == out["n_mismatch"] + out["n_ins"] + out["n_del"] and ops.size == out["dist"] + out["n_match"]
    return out


def cigar(ops):
    """the ops run-length coded as an extended CIGAR (=XID); `*` for none"""
    ops = np.asarray(ops, np.uint8)
    if ops.size == 0:
        return "*"
    cut = np.flatnonzero(np.diff(ops)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [ops.size]])
    return "".join("%d%s" % (e - b, OPS[ops[b]]) for b, e in zip(starts, ends))


def identity(rec):
    d = rec["n_match"] + rec["n_mismatch"] + rec["n_ins"] + rec["n_del"]
    return rec["n_match"] / d if d else 0.0


def tsv_line(name, rec, band):
    """one line of acc.tsv (include/flappie_truth.h)"""
    if rec["status"] != 1:
        return "%s\t%d\t%d\t%d\t%d\t*\t*\t*\t*\t*\t*\t*\t*\n" % (name, rec["status"], rec["n"], rec["m"], band)
    return "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%s\n" % (name, rec["status"], rec["n"], rec["m"], band, rec["maxdev"], rec["dist"], rec["n_match"],
                                                                      rec["n_mismatch"], rec["n_ins"], rec["n_del"], identity(rec), cigar(rec["ops"]))
