"""Restatement of the adapter search (include/ffhip.h "adapters", include/flappie_adapters.h) in plain numpy: the contract the kernel, the C-ABI, the tag
formatter, the trim and the split are held to.  Everything here is integer arithmetic.

  searches of a kit on a call x (Z read as C, signal order):  q = 2 k + o, pattern k as given (o = 0) or its reverse complement (o = 1)
  score row:  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (p[i] != x[j]), D[i-1][j] + 1, D[i][j-1] + 1);  d_q[j] = D[L][j], j = 0 .. len
  hit end j of q (R = 64):  d_q[j] <= md_k,  d_q[j] < d_q[j'] for j' in [j - R, j),  d_q[j] <= d_q[j'] for j' in (j, j + R]  (j' within [0, len])
      md_k = L_k // 4 (max_dist < 0) or min(max_dist, L_k - 1)
  start of (q, j, d):  the reversed pattern against x[j-1], x[j-2], ... from an anchored start (D[0][c] = c), the first column c with D[L][c] = d;  start = j - c
  record:  hits ordered by (end, q);  nhit counts all,  kept = min(nhit, 15) are stored
"""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
R = 64
MAX_HITS = 15
MAX_KIT, MAX_LEN = 32, 64


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def searches(patterns):
    """the oriented patterns, q = 2 k + o"""
    out = []
    for p in patterns:
        out += [p, revcomp(p)]
    return out


def bounds(patterns, max_dist: int = -1):
    """md of every SEARCH"""
    md = [len(p) // 4 if max_dist < 0 else min(max_dist, len(p) - 1) for p in patterns]
    return np.repeat(np.array(md, np.int64), 2)


def _rows(pats, xs, anchored: bool):
    """D[L][j], j = 0 .. len, of pattern pats[r] in text xs[r] (texts of one length; one str: the same text for all): the recurrence a column at a time, all
    patterns and rows at once (D[i][j] = i + min_{i' <= i} (t[i'] - i'), t[i] = min(D[i-1][j-1] + sub, D[i][j-1] + 1), t[0] = D[0][j]: 0, or j for an anchored start)"""
    if isinstance(xs, str):
        xs = [xs] * len(pats)
    n, Lmax, m = len(pats), max(len(p) for p in pats), len(xs[0])
    assert len(xs) == n and all(len(x) == m for x in xs)
    L = np.array([len(p) for p in pats])
    P = np.full((n, Lmax), ord("#"), np.int64)
    for k, p in enumerate(pats):
        P[k, :len(p)] = np.frombuffer(p.encode(), np.uint8)
    X = np.frombuffer("".join(xs).encode(), np.uint8).reshape(n, m).astype(np.int64)
    rows = np.arange(Lmax + 1)
    D = np.tile(rows, (n, 1)).astype(np.int64)                  # column 0: D[i][0] = i
    at = np.arange(n)
    out = np.zeros((n, m + 1), np.int64)
    out[:, 0] = D[at, L]
    for j in range(1, m + 1):
        t = np.full_like(D, j if anchored else 0)
        t[:, 1:] = np.minimum(D[:, :-1] + (P != X[:, j - 1:j]), D[:, 1:] + 1)
        D = rows + np.minimum.accumulate(t - rows, axis=1)
        out[:, j] = D[at, L]
    return out


def score_rows(patterns, call: str, start_at: int = 0):
    """d as uint8 [2 n][len + 1]; start_at = a: the search started FRESH at column a (D[i][a] = i), columns before a zero -- the locality claim's other side"""
    x = call.replace("Z", "C")
    d = np.zeros((2 * len(patterns), len(x) + 1), np.int64)
    d[:, start_at:] = _rows(searches(patterns), x[start_at:], False)
    return d.astype(np.uint8)


def score_rows_many(patterns, calls):
    """score_rows of several calls of ONE length in one sweep: uint8 [ncall][2 n][len + 1]"""
    sp = searches(patterns)
    xs = [c.replace("Z", "C") for c in calls for _ in sp]
    return _rows(sp * len(calls), xs, False).reshape(len(calls), len(sp), -1).astype(np.uint8)


def hit_ends(d, md):
    """[(j, q)] in (end, q) order: the leftmost minimum of a row within R columns either way, at most md"""
    d = np.asarray(d, np.int64)
    nq, ncol = d.shape
    hits = []
    for q in range(nq):
        for j in np.flatnonzero(d[q] <= md[q]):
            v = d[q, j]
            if (d[q, max(0, j - R):j] > v).all() and (d[q, j + 1:min(ncol, j + R + 1)] >= v).all():
                hits.append((int(j), q))
    return sorted(hits)


def hit_start(p: str, x: str, j: int, d: int) -> int:
    """start of the hit of the ORIENTED pattern p ending at column j of x with distance d"""
    back = x[max(0, j - 2 * MAX_LEN):j][::-1]
    row = _rows([p[::-1]], back, True)[0]
    c = int(np.flatnonzero(row == d)[0])
    return j - c


def record(patterns, call: str, max_dist: int = -1, d=None) -> dict:
    """nhit, len, kept, hits = the first `kept` of (start, end, pattern, orientation, dist) by (end, q); d: the call's score rows when the caller has them"""
    x = call.replace("Z", "C")
    if d is None:
        d = score_rows(patterns, call)
    ends = hit_ends(d, bounds(patterns, max_dist))
    sp = searches(patterns)
    hits = [(hit_start(sp[q], x, j, int(d[q, j])), j, q >> 1, q & 1, int(d[q, j])) for j, q in ends[:MAX_HITS]]
    return {"nhit": len(ends), "len": len(x), "kept": len(hits), "hits": hits}


def records_many(patterns, calls, max_dist: int = -1):
    """record of several calls of ONE length: the score rows in one sweep, the starts of all their kept hits in another"""
    sp, md = searches(patterns), bounds(patterns, max_dist)
    ds = score_rows_many(patterns, calls)
    xs = [c.replace("Z", "C") for c in calls]
    ends = [hit_ends(d, md) for d in ds]
    todo = [(i, j, q) for i, e in enumerate(ends) for j, q in e[:MAX_HITS]]
    starts = {}
    if todo:                                                     # the reversed patterns against the 128 characters before each end ('#' where the call begins)
        back = [xs[i][max(0, j - 2 * MAX_LEN):j][::-1].ljust(2 * MAX_LEN, "#") for i, j, q in todo]
        rows = _rows([sp[q][::-1] for i, j, q in todo], back, True)
        for (i, j, q), row in zip(todo, rows):
            starts[(i, j, q)] = j - int(np.flatnonzero(row == ds[i][q, j])[0])
    out = []
    for i, e in enumerate(ends):
        hits = [(starts[(i, j, q)], j, q >> 1, q & 1, int(ds[i][q, j])) for j, q in e[:MAX_HITS]]
        out.append({"nhit": len(e), "len": len(xs[i]), "kept": len(hits), "hits": hits})
    return out


EMPTY = {"nhit": 0, "len": 0, "kept": 0, "hits": []}


def raw_slots(rec: dict) -> np.ndarray:
    """the 15 hit slots as 60 int32, the slots no hit took zero: what the device buffer holds behind the header"""
    out = np.zeros((MAX_HITS, 4), np.int64)
    for i, (s, e, k, o, dd) in enumerate(rec["hits"]):
        out[i] = (s, e, (k & 0xFFFF) | (o << 16) | (dd << 24), 0)
    return out.astype(np.uint32).view(np.int32).reshape(-1)


# ---- the host side: tags, trim, split (include/flappie_adapters.h)
def tags(rec: dict, names) -> str:
    """the record's two tags, tab-separated, no tab in front"""
    return "an:i:%d\tah:Z:%s" % (rec["nhit"], "".join("%s,%s,%d,%d,%d;" % (names[k], "-" if o else "+", s, e, dd) for s, e, k, o, dd in rec["hits"]))


def trim_range(rec: dict, length: int, W: int = 150):
    """[from, to) of the call (signal order) that --trim-adapters keeps: the front cut is the largest end among the kept hits with end <= W, the rear cut the smallest
    start among those with start >= length - W; (0, 0) when the two cuts meet or cross"""
    lo = max([e for s, e, k, o, dd in rec["hits"] if e <= W], default=0)
    hi = min([s for s, e, k, o, dd in rec["hits"] if s >= length - W], default=length)
    if (lo > 0 or hi < length) and lo >= hi:
        return (0, 0)
    return (lo, hi)


def combine_trims(a, b, length: int):
    """--trim-barcodes with --trim-adapters: the larger cut at each end wins; a crossed one of either, or a crossing of the two, leaves nothing"""
    crossed = lambda r: r == (0, 0) and length > 0
    if crossed(a) or crossed(b):
        return (0, 0)
    lo, hi = max(a[0], b[0]), min(a[1], b[1])
    return (lo, hi) if lo < hi or length == 0 else (0, 0)


def split_pieces(rec: dict, length: int, W: int = 150, M: int = 200, clip=None):
    """--split-reads: (mode, pieces, dropped).  mode "overflow": nhit > 15, the read is written unsplit.  mode "whole": no interior hit (every kept hit is a front
    or a rear one of trim_range) -- pieces = [trim_range within the clip], written under the read's own name whatever its length.  mode "split": the pieces are
    the maximal stretches of that range covered by no kept hit, in signal order; those shorter than M are dropped and counted.  clip: the range --trim-barcodes
    keeps."""
    if rec["nhit"] > MAX_HITS:
        return "overflow", [], 0
    lo, hi = combine_trims(trim_range(rec, length, W), clip if clip is not None else (0, length), length)
    interior = [h for h in rec["hits"] if not (h[1] <= W or h[0] >= length - W)]
    if not interior:
        return "whole", [(lo, hi)], 0
    covered = np.zeros(length + 1, bool)
    covered[length] = True
    covered[:lo] = True
    covered[hi:] = True
    for s, e, k, o, dd in rec["hits"]:
        covered[s:e] = True
    pieces, i = [], 0
    while i < length:
        if covered[i]:
            i += 1
            continue
        j = i
        while not covered[j]:
            j += 1
        pieces.append((i, j))
        i = j
    kept = [p for p in pieces if p[1] - p[0] >= M]
    return "split", kept, len(pieces) - len(kept)


def cuts(rec: dict, length: int, trim: bool = False, split: bool = False, W: int = 150, M: int = 200, clip=None):
    """what one read becomes on stdout: (mode, pieces, dropped) -- mode "one": one record under the read's own name, pieces = [the range of the call it keeps];
    mode "split": a record a piece, named <name>:<k>; overflow tells whether the read had more than 15 hits under --split-reads (it is then written as without)"""
    whole = (0, length)
    clip = clip if clip is not None else whole
    crossed = lambda r: r == (0, 0) and length > 0
    if split and not crossed(clip):
        mode, pieces, dropped = split_pieces(rec, length, W, M, clip)
        if mode == "split":
            return "split", pieces, dropped, False
        if mode == "whole":
            return "one", pieces, 0, False
    rng = combine_trims(trim_range(rec, length, W) if trim else whole, clip, length)
    return "one", [rng], 0, split and not crossed(clip)


def records_text(fmt: str, head: str, call: str, qual, rec: dict, names, name: str, extra_tags: str = "", reverse: bool = False, **kw) -> str:
    """the read's record(s) with --adapters: `head` is the first line of its default record (SAM: the whole line), call / qual in SIGNAL order; extra_tags: the
    tags in front of the adapter tags (no tab at either end); kw: what cuts takes"""
    mode, pieces, _, _ = cuts(rec, len(call), **kw)
    out = []
    for k, (a, b) in enumerate(pieces, start=1):
        seq, q = call[a:b], (qual[a:b] if qual is not None else None)
        if reverse:
            seq, q = seq[::-1], (q[::-1] if q is not None else None)
        t = (extra_tags + "\t" if extra_tags else "") + tags(rec, names)
        h = head
        if mode == "split":
            t += "\tpi:Z:%s\tsp:B:i,%d,%d" % (name, a, b)
            h = head.replace(name, "%s:%d" % (name, k))
        if fmt == "sam":
            f = h.split("\t")
            out.append("\t".join(f[:9] + [seq, q or "", t]) + "\n")
        elif fmt == "fasta":
            out.append(h + "\t" + t + "\n" + seq + "\n")
        else:
            out.append(h + "\t" + t + "\n" + seq + "\n+\n" + q + "\n")
    return "".join(out)


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
    if len(recs) > MAX_KIT:
        raise ValueError("more than 32 records")
    seen = set()
    for nm, sq in recs:
        if not nm:
            raise ValueError("a record without a name")
        if nm in seen:
            raise ValueError("duplicate name")
        if set(nm) & set(",;"):
            raise ValueError("a name with , or ;")
        seen.add(nm)
        if not 1 <= len(sq) <= MAX_LEN:
            raise ValueError("pattern length")
        if set(sq) - set("ACGT"):
            raise ValueError("non-ACGT character")
    return recs
