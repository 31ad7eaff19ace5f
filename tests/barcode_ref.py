"""Restatement of the barcode classification (include/ffhip.h "barcodes", include/flappie_barcodes.h) in plain numpy: the contract the kernel,
the C-ABI, the tag formatter and the trim are held to.  Everything here is integer arithmetic.

  windows of a call s (Z read as C) at window size W:  front = s[:min(W, len)],  rear = revcomp(s)[:min(W, len)]
  infix edit distance of pattern p (L) in window x (m):  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (p[i] != x[j]), D[i-1][j] + 1, D[i][j-1] + 1);
      dist = min_j D[L][j] over j = 0 .. m, end = the smallest j that attains it
  classification:  s_k = min(front, rear) (both_ends: max), best = smallest k of the minimum, second = min over the others (255 for a kit of one),
      classified iff s_best <= max_dist and second - s_best >= min_sep
"""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FIELDS = ("best", "best_dist", "second_dist", "front_dist", "rear_dist", "ends", "front_end", "rear_end")


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def windows(call: str, W: int):
    s = call.replace("Z", "C")
    m = min(W, len(s))
    return s[:m], revcomp(s)[:m]


def infix_matrix(patterns, x: str):
    """(dist, end) int arrays [n] of every pattern in window x: the recurrence a column at a time, all patterns and rows at once
    (D[i][j] = i + min_{i' <= i} (t[i'] - i'), t[i] = min(D[i-1][j-1] + sub, D[i][j-1] + 1), t[0] = 0)"""
    n, Lmax = len(patterns), max(len(p) for p in patterns)
    L = np.array([len(p) for p in patterns])
    P = np.full((n, Lmax), ord("#"), np.int64)
    for k, p in enumerate(patterns):
        P[k, :len(p)] = np.frombuffer(p.encode(), np.uint8)
    rows = np.arange(Lmax + 1)
    D = np.tile(rows, (n, 1)).astype(np.int64)                  # column 0: D[i][0] = i
    at = np.arange(n)
    best, end = D[at, L].copy(), np.zeros(n, np.int64)
    for j, c in enumerate(x, start=1):
        t = np.zeros_like(D)
        t[:, 1:] = np.minimum(D[:, :-1] + (P != ord(c)), D[:, 1:] + 1)
        D = rows + np.minimum.accumulate(t - rows, axis=1)
        d = D[at, L]
        better = d < best
        best[better], end[better] = d[better], j
    return best, end


def infix(p: str, x: str):
    d, e = infix_matrix([p], x)
    return int(d[0]), int(e[0])


def scores(patterns, call: str, W: int = 150):
    """dist, end as int32 [2][n]: front, rear"""
    f, r = windows(call, W)
    df, ef = infix_matrix(patterns, f)
    dr, er = infix_matrix(patterns, r)
    return np.stack([df, dr]).astype(np.int32), np.stack([ef, er]).astype(np.int32)


def default_max_dist(patterns) -> int:
    return min(len(p) for p in patterns) // 4


def classify(patterns, call: str, W: int = 150, max_dist=None, min_sep: int = 3, both_ends: bool = False) -> dict:
    if max_dist is None:
        max_dist = default_max_dist(patterns)
    dist, end = scores(patterns, call, W)
    s = np.maximum(dist[0], dist[1]) if both_ends else np.minimum(dist[0], dist[1])
    best = int(np.argmin(s))                                    # the first of the minimum
    others = np.delete(s, best)
    second = int(others.min()) if others.size else 255
    ok = s[best] <= max_dist and second - s[best] >= min_sep
    return {"best": best if ok else -1, "best_dist": int(s[best]), "second_dist": second,
            "front_dist": int(dist[0][best]), "rear_dist": int(dist[1][best]),
            "ends": int(dist[0][best] <= max_dist) | (int(dist[1][best] <= max_dist) << 1),
            "front_end": int(end[0][best]), "rear_end": int(end[1][best])}


EMPTY = {"best": -1, "best_dist": 255, "second_dist": 255, "front_dist": 255, "rear_dist": 255, "ends": 0, "front_end": 0, "rear_end": 0}


def category(rec: dict, max_dist: int) -> str:
    """what happened to the read: classified by its front / by its rear (the end that gave s_best), or rejected by max_dist / by min_sep"""
    if rec["best"] >= 0:
        return "front" if rec["front_dist"] <= rec["rear_dist"] else "rear"
    return "max_dist" if rec["best_dist"] > max_dist else "min_sep"


def tags(rec: dict, names) -> str:
    """the record's tags, tab-separated, no tab in front"""
    return "BC:Z:%s\tbd:i:%d\tbn:i:%d\tbp:B:s,%d,%d" % (names[rec["best"]] if rec["best"] >= 0 else "unclassified", rec["best_dist"], rec["second_dist"],
                                                         rec["front_end"], rec["rear_end"])


def trim_range(rec: dict, length: int):
    """[from, to) of the call (signal order) that --trim-barcodes keeps; (0, 0) when the two cuts meet or cross"""
    lo, hi = 0, length
    if rec["best"] >= 0:
        if rec["ends"] & 1:
            lo = rec["front_end"]
        if rec["ends"] & 2:
            hi = length - rec["rear_end"]
    return (lo, hi) if lo < hi else (0, 0)


def parse_kit(text: str):
    """the kit file's records: [(name, pattern)], or ValueError with the refusal"""
    recs, name, seq = [], None, []

    def flush():
        if name is not None:
            recs.append((name, "".join(seq).upper()))
    for line in text.splitlines():
        line = line.strip()
        if not line:
            continue
        if line.startswith(">"):
            flush()
            name, seq = (line[1:].split() or [""])[0], []
        elif name is None:
            raise ValueError("sequence before the first record")
        else:
            seq.append(line)
    flush()
    if not recs:
        raise ValueError("empty kit")
    if len(recs) > 128:
        raise ValueError("more than 128 records")
    seen = set()
    for nm, sq in recs:
        if not nm:
            raise ValueError("a record without a name")
        if nm in seen:
            raise ValueError("duplicate name")
        seen.add(nm)
        if not 1 <= len(sq) <= 128:
            raise ValueError("pattern length")
        if set(sq) - set("ACGT"):
            raise ValueError("non-ACGT character")
    return recs
