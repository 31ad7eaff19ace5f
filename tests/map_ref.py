"""Restatement of the map (include/ffhip.h "map") in plain numpy: the contract the kernels, the C-ABI and the binding are held to.  Everything here is integer
arithmetic.

  reference:  K records over ACGT;  search q = 2 k + o, text y_q = record k as given (o = 0) or its reverse complement (o = 1)
  anchors of a call x of n bases (Z read as C, signal order), window W:  na = 1 if n <= W else 2;  p_0 = x[:min(n, W)],  p_1 = x[n - min(n, W):]
  score row:  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (p[i] != y[j]), D[i-1][j] + 1, D[i][j-1] + 1);  d_q[j] = D[L][j], j = 0 .. m_k
  best place:  the smallest (d, q, j);  second = min d over q' != q
  start of (q, j, d):  the reversed anchor against y[j-1], y[j-2], ... from an anchored start (D[0][c] = c), the first column c with D[L][c] = d;  start = j - c
  bound:  md = L e // 1000;  status 0 no call, 1 mapped, 2 some anchor over its bound, 3 discordant (q differ, start_0 >= end_1, |(end_1 - start_0) - n| > n e // 1000)

The sweep works a pattern ROW at a time over all columns of all searches at once: D[i][j] = j + cummin_j (t[j] - j), t[j] = min(D[i-1][j-1] + sub, D[i-1][j] + 1),
t[0] = i; a search's columns are kept from the next one's by a bias no value can cross.
"""
import numpy as np

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
MAX_RECORDS, MAX_TOTAL, MAX_ANCHOR = 1024, 1 << 20, 4096
FIELDS = ("status", "n", "nanchor", "q", "tstart", "tend")
ANCHOR_FIELDS = ("q", "start", "end", "dist", "second")


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def searches(records):
    """the texts y_q, q = 2 k + o"""
    out = []
    for r in records:
        out += [r, revcomp(r)]
    return out


def sweep(p: str, texts, anchored: bool = False):
    """D[L][j], j = 0 .. m, of pattern p in every text: a list of int64 arrays (anchored: D[0][c] = c instead of 0)"""
    L = len(p)
    m = [len(y) for y in texts]
    col0 = np.concatenate([[0], np.cumsum([x + 1 for x in m])[:-1]]).astype(np.int64)
    ncol = int(sum(m)) + len(m)
    Y = np.full(ncol, 255, np.int64)
    jloc = np.zeros(ncol, np.int64)
    sidx = np.zeros(ncol, np.int64)
    for s, y in enumerate(texts):
        Y[col0[s] + 1:col0[s] + 1 + m[s]] = np.frombuffer(y.encode(), np.uint8)
        jloc[col0[s]:col0[s] + 1 + m[s]] = np.arange(m[s] + 1)
        sidx[col0[s]:col0[s] + 1 + m[s]] = s
    bias = jloc + (L + max(m) + 2) * sidx
    P = np.frombuffer(p.encode(), np.uint8).astype(np.int64)
    prev = jloc.copy() if anchored else np.zeros(ncol, np.int64)
    for i in range(1, L + 1):
        t = prev + 1
        np.minimum(t[1:], prev[:-1] + (Y[1:] != P[i - 1]), out=t[1:])
        t[col0] = i
        prev = np.minimum.accumulate(t - bias) + bias
    return [prev[col0[s]:col0[s] + 1 + m[s]].copy() for s in range(len(texts))]


def score_rows(records, pattern: str):
    """the rows d_q of ONE anchor: a list of 2 K int64 arrays of m_k + 1 entries"""
    return sweep(pattern.replace("Z", "C"), searches(records))


def fresh_row(p: str, y: str, a: int):
    """d of a search started FRESH at column a of y (D[i][a] = i): entries a .. m; the locality claim's other side"""
    return sweep(p, [y[a:]])[0]


def start_of(p: str, y: str, j: int, d: int) -> int:
    back = y[max(0, j - 2 * len(p)):j][::-1]
    row = sweep(p[::-1], [back], True)[0]
    return j - int(np.flatnonzero(row == d)[0])


def place(records, p: str, rows=None) -> dict:
    """the best place of anchor p: q, start, end, dist, second"""
    ys = searches(records)
    if rows is None:
        rows = sweep(p, ys)
    mins = [int(r.min()) for r in rows]
    d = min(mins)
    q = mins.index(d)
    j = int(np.argmin(rows[q]))                  # (the first of equals)
    second = min(v for k, v in enumerate(mins) if k != q)
    return {"q": q, "start": start_of(p, ys[q], j, d), "end": j, "dist": d, "second": second}


def record(records, call: str, window: int = 4096, max_error: int = 250, rows=None) -> dict:
    """the record of a call; rows: the score rows of its front anchor when the caller has them"""
    x = call.replace("Z", "C")
    n = len(x)
    zero = dict(zip(ANCHOR_FIELDS, (0,) * 5))
    if n == 0:
        return dict(zip(FIELDS, (0,) * 6), anchors=[dict(zero), dict(zero)])
    L = min(n, window)
    na = 1 if n <= window else 2
    an = [place(records, x[:L], rows)]
    an.append(place(records, x[n - L:]) if na == 2 else dict(an[0]))
    md = L * max_error // 1000
    status = 1
    if an[0]["dist"] > md or an[1]["dist"] > md:
        status = 2
    elif na == 2 and (an[0]["q"] != an[1]["q"] or an[0]["start"] >= an[1]["end"] or abs(an[1]["end"] - an[0]["start"] - n) > n * max_error // 1000):
        status = 3
    ok = status == 1
    return {"status": status, "n": n, "nanchor": na, "q": an[0]["q"] if ok else 0, "tstart": an[0]["start"] if ok else 0, "tend": an[1]["end"] if ok else 0, "anchors": an}


def raw(rec: dict):
    """the record's sixteen int32 as the kernel writes them"""
    return np.array([rec[f] for f in FIELDS] + [rec["anchors"][a][f] for a in range(2) for f in ANCHOR_FIELDS], np.int32)


def edit(rng, s: str, rate: float) -> str:
    """s with about rate * len(s) random edits (substitution, insertion, deletion in equal parts)"""
    out = []
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append("ACGT"[(("ACGT".index(c)) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * rate / 3:
            out.append(c)
            out.append("ACGT"[int(rng.integers(0, 4))])
        elif u < rate:
            continue
        else:
            out.append(c)
    return "".join(out) or "A"


def random_seq(rng, n: int) -> str:
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


# ---- the host side (include/flappie_map.h): the line of hits.tsv, the record of --map-records, the summary
def forward(q: int, start: int, end: int, lens):
    """(record, strand, forward start, forward end) of [start, end) of search q"""
    k, m = q >> 1, lens[q >> 1]
    return (k, "+", start, end) if q & 1 == 0 else (k, "-", m - end, m - start)


def hits_line(name: str, rec: dict, names, lens) -> str:
    f = [name, rec["status"], rec["n"], rec["nanchor"]]
    if rec["status"] == 1:
        k, o, a, b = forward(rec["q"], rec["tstart"], rec["tend"], lens)
        f += [names[k], o, a, b, lens[k]]
    else:
        f += ["*"] * 5
    f += [rec["anchors"][0]["dist"], rec["anchors"][0]["second"], rec["anchors"][1]["dist"], rec["anchors"][1]["second"]]
    if rec["status"] >= 2:
        for an in rec["anchors"]:
            k, o, a, b = forward(an["q"], an["start"], an["end"], lens)
            f += [names[k], o, a, b]
    return "\t".join(str(x) for x in f) + "\n"


def record_text(name: str, rec: dict, records) -> str:
    """the mapped read's own stretch in signal order, "" for the others"""
    if rec["status"] != 1:
        return ""
    return ">%s\n%s\n" % (name, searches(records)[rec["q"]][rec["tstart"]:rec["tend"]])


def summary(recs, window: int = 4096) -> dict:
    """the stderr lines' values: reads, mapped, unmapped, discordant, anchor_dist, anchor_bases, pooled_error"""
    s = {"reads": len(recs), "mapped": 0, "unmapped": 0, "discordant": 0, "anchor_dist": 0, "anchor_bases": 0}
    for r in recs:
        if r["status"]:
            s[("mapped", "unmapped", "discordant")[r["status"] - 1]] += 1
        if r["status"] == 1:
            s["anchor_dist"] += sum(a["dist"] for a in r["anchors"][:r["nanchor"]])
            s["anchor_bases"] += r["nanchor"] * min(r["n"], window)
    out = {k: str(v) for k, v in s.items()}
    out["pooled_error"] = "%.6f" % (s["anchor_dist"] / s["anchor_bases"] if s["anchor_bases"] else 0.0)
    return out
