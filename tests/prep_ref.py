"""Signal preparation once more, in plain numpy: quantilef, medianf, madf, medmad_normalise_array, shift_scale_array, difference_array (util.c:100-223,278-287) and
trim_raw_by_mad, trim_and_segment_raw (flappie_common.c:13-81), by a stable sort -- what ffhip_prep.hip's exact selections have to equal.  Nothing here imports the
package; tests/test_prep_ref.py holds this file to the oracle's C restatement on every input listed below.

The interpolation is the reference's, operation for operation (util.c:126-129): p * (nx - 1) is a float product, its integer part the index, the rest `remf` a float;
`(1.0 - remf) * s[idx]` is a double product, `remf * s[idx + 1]` a FLOAT product, their sum a double rounded to float.  With remf == 0 the second product is still
taken: an infinity just above the selected rank makes the quantile NaN.

Where the reference says nothing, this file says nothing either:
  * floatcmp (util.c:77-83) orders by the sign of a subtraction, so NaN has no place in its order and what qsort makes of one is anybody's guess.  quantilef() here refuses
    an array that holds NaN beside other values.  An array of NOTHING BUT NaN has one answer under any order (NaN), and is let through: madf about a NaN median is one.
  * +0 and -0 tie under floatcmp, and which of a tie qsort puts first is unspecified; the kernels' keys put -0 first.  same() therefore reads +0 and -0 as equal.
  * a read without one whole chunk (nchunk == 0) makes the reference read madarr[0] of an empty allocation.  trim_raw_by_mad() returns None for it -- the read is rejected,
    which is what the kernel does -- and the oracle must never be asked about such a read.

The second half of the file is the list of hostile inputs the CPU and the GPU tests share: single arrays, rank-boundary "step" arrays, the trim grid, element-wise values."""
import numpy as np

F32, F64 = np.float32, np.float64
MAD_SCALE = F32(1.4826)


def bits(*words):
    return np.array(words, dtype=np.uint32).view(F32)


def same(a, b):
    """the equality used everywhere: equal bits, NaN equals NaN, +0 equals -0 (for float32 that is equality of values with NaN equal to itself)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def quantile_index(p, n):
    """util.c:126-127: (idx, remf)"""
    pos = F32(F32(p) * F32(n - 1))
    idx = int(pos)
    return idx, F32(pos - F32(idx))


def _mix(s, idx, remf, n):
    """util.c:128-133 on the sorted values along the last axis"""
    a = s[..., idx]
    if idx >= n - 1:
        return F32(a) if a.ndim == 0 else a.copy()
    with np.errstate(all="ignore"):
        hi = (F32(remf) * s[..., idx + 1]).astype(F32)
        return ((1.0 - F64(remf)) * a.astype(F64) + hi.astype(F64)).astype(F32)


def _sorted(x):
    x = np.ascontiguousarray(x, dtype=F32)
    nan = np.isnan(x)
    assert x.shape[-1] > 0 and (not nan.any() or nan.all()), "NaN among other values has no order under floatcmp"
    return np.sort(x, axis=-1, kind="stable")


def quantilef(x, p):
    """quantiles `p` (a scalar or a list) of the 1-D array x"""
    s = _sorted(x)
    n = s.size
    if np.ndim(p) == 0:
        return _mix(s, *quantile_index(p, n), n)
    return np.array([_mix(s, *quantile_index(q, n), n) for q in p], dtype=F32)


def medianf(x):
    return quantilef(x, 0.5)


def madf(x, med=None):
    """util.c:164-187: MAD about `med`, or about the median"""
    x = np.ascontiguousarray(x, dtype=F32)
    if x.size == 1:
        return F32(0.0)
    m = F32(medianf(x) if med is None else med)
    with np.errstate(all="ignore"):
        return F32(medianf(np.abs(x - m)) * MAD_SCALE)


def medmad_normalise_array(x):
    """util.c:198-212: (normalised signal, median, MAD)"""
    x = np.ascontiguousarray(x, dtype=F32)
    if x.size == 1:
        return np.zeros(1, dtype=F32), F32(x[0]), F32(0.0)          # (the statistics of one sample: medianf and madf of it)
    med = medianf(x)
    mad = madf(x, med)
    with np.errstate(all="ignore"):
        return ((x - med) / mad).astype(F32), med, mad


def shift_scale_array(x, shift, scale):
    with np.errstate(all="ignore"):
        return ((np.asarray(x, dtype=F32) - F32(shift)) / F32(scale)).astype(F32)


def difference_array(x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        return np.concatenate([x[1:] - x[:-1], np.zeros(1, dtype=F32)]).astype(F32)


def chunk_mads(raw, start, nchunk, chunk):
    """madf(raw + start + i * chunk, chunk, NULL) for every chunk, all rows at once"""
    c = np.ascontiguousarray(raw[start:start + nchunk * chunk], dtype=F32).reshape(nchunk, chunk)
    idx, remf = quantile_index(0.5, chunk)
    med = _mix(_sorted(c), idx, remf, chunk)
    with np.errstate(all="ignore"):
        return (_mix(_sorted(np.abs(c - med[:, None])), idx, remf, chunk) * MAD_SCALE).astype(F32)


def trim_raw_by_mad(raw, start, end, chunk, perc):
    """flappie_common.c:47-81: the new (start, end) -- `end` absolute from nchunk * chunk, as the reference has it -- or None without one whole chunk"""
    assert chunk > 1 and 0.0 <= perc <= 1.0 and 0 <= start <= end <= len(raw)
    nchunk = (end - start) // chunk
    if nchunk == 0:
        return None
    end = nchunk * chunk
    mad = chunk_mads(raw, start, nchunk, chunk)
    thresh = quantilef(mad, perc)
    for i in range(nchunk):
        if mad[i] > thresh:
            break
        start += chunk
    for i in range(nchunk, 0, -1):
        if mad[i - 1] > thresh:
            break
        end -= chunk
    return start, end


def trim_and_segment_raw(raw, start, end, trim_start, trim_end, chunk, perc):
    """flappie_common.c:13-28: (start, end), or None for a rejected read"""
    r = trim_raw_by_mad(raw, start, end, chunk, perc)
    if r is None:
        return None
    start, end = r
    n = len(raw)
    start = start + trim_start if (n - start) > trim_start else n
    end = end - trim_end if end > trim_end else 0
    return None if start >= end else (start, end)


# ------------------------------------------------------------------------------------------------ hostile inputs, shared by the CPU and the GPU tests
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 1000, 4097)
QUANTILES = np.array([0.0, 0.25, 1.0 / 3.0, 0.5, 0.5000001, 0.75, 0.9, 0.999, 1.0], dtype=F32)
FLT_MAX = np.finfo(F32).max
DENORM = F32(1e-45)                                   # the smallest denormal
EDGE_BITS = (0x3f7fffff, 0x3f800000, 0x3effffff, 0x3f000000, 0xbf800000, 0xbf7fffff, 0x00800000, 0x007fffff, 0x80000001)
CLUSTER_BASE = 0x42b40000                             # 90.0
GIVEN_MEDIAN = F32(0.75)                              # madf(x, n, &med) with a median that is not the array's

FAMILIES = ("normal", "quarters", "two", "zeros", "cluster", "edges", "huge", "inf", "spread", "constant")


def family(name, n, rng):
    if name == "normal":
        return rng.standard_normal(n).astype(F32)
    if name == "quarters":                            # signed, plenty of duplicates
        return (np.round(rng.normal(0.0, 3.0, n) * 4) / 4).astype(F32)
    if name == "two":
        return rng.choice(np.array([-1.5, 2.25], dtype=F32), n)
    if name == "zeros":                               # +-0 and +-denormal: the four keys around the sign boundary
        return rng.choice(np.array([0.0, -0.0, DENORM, -DENORM], dtype=F32), n)
    if name == "cluster":                             # 700 ulp: the last key byte wraps, the third changes
        return (np.uint32(CLUSTER_BASE) + rng.integers(0, 700, n).astype(np.uint32)).view(F32)
    if name == "edges":
        return rng.choice(bits(*EDGE_BITS), n)
    if name == "huge":                                # the top pass's first and last bins
        return rng.choice(np.array([FLT_MAX, -FLT_MAX, 1.8e38, -1.8e38, 1.0, -1.0], dtype=F32), n)
    if name == "inf":
        x = rng.standard_normal(n).astype(F32)
        i, j = rng.choice(n, 2, replace=False)
        x[i], x[j] = np.inf, -np.inf
        return x
    if name == "spread":
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    if name == "constant":
        return np.full(n, 90.125, dtype=F32)
    raise KeyError(name)


def single_arrays():
    """[(family, n, x)]: section a"""
    out = []
    for k, name in enumerate(FAMILIES):
        for n in LENGTHS:
            if name == "inf" and n < 3:
                continue
            out.append((name, n, family(name, n, np.random.default_rng([11, k, n]))))
    return out


STEP_LENGTHS = (2, 3, 5, 64, 100, 257, 1000)
STEP_QUANTILES = np.array([0.0, 0.25, 0.5, 0.9, 1.0], dtype=F32)
_C = CLUSTER_BASE
STEP_PAIRS = {"sign": (F32(-1.5), F32(2.25)),
              "byte2": tuple(bits(_C, _C + (1 << 16))), "byte3": tuple(bits(_C, _C + (1 << 8))), "byte4": tuple(bits(_C, _C + 1)),
              "last_bin": (F32(1.8e38), F32(3.4e38)), "first_bin": (F32(-3.4e38), F32(-1.8e38))}


def step_arrays():
    """[(pair, n, p, extra, idx, x)]: idx + 1 + extra copies of a, the rest b > a, shuffled -- sorted[idx] is the LAST a when extra == 0 (section b)"""
    out = []
    for k, (name, (a, b)) in enumerate(STEP_PAIRS.items()):
        assert a < b
        for n in STEP_LENGTHS:
            for p in STEP_QUANTILES:
                idx, _ = quantile_index(p, n)
                for extra in (0, 1):
                    x = np.full(n, b, dtype=F32)
                    x[:min(n, idx + 1 + extra)] = a
                    np.random.default_rng([12, k, n, idx, extra]).shuffle(x)
                    out.append((name, n, p, extra, idx, x))
    return out


LARGE_N = (1 << 24) + 3                               # past 2^24: floats are 2 apart at n - 1, so p * (n - 1) and (float)idx round to even integers
LARGE_QUANTILES = np.array([0.5, 0.9999999], dtype=F32)


def large_array():
    return np.random.default_rng(13).standard_normal(LARGE_N).astype(F32)


TRIM_CHUNKS = (2, 3, 63, 64, 65, 100, 1023, 1024)
TRIM_KINDS = ("dac", "dac0", "round", "cluster")


def trim_params(chunk):
    """(perc, trim_start, trim_end) of a chunk size"""
    return ((0.0, 0, 0), (0.0, chunk // 2, 1), (0.5, 0, 0), (0.9, 1, 1))


def trim_whole_chunks(chunk):
    return (1, 2, 3, 4, 5, 8, 9, 257 if chunk <= 100 else 6)


def trim_values(kind, n, rng):
    if kind == "dac":                                 # quantised like DAC values around 90: plenty of duplicates
        return (np.round(rng.normal(90.0, 12.0, n) * 8) / 8).astype(F32)
    if kind == "dac0":
        return (np.round(rng.normal(0.0, 12.0, n) * 8) / 8).astype(F32)
    if kind == "round":                               # few distinct values: chunk MADs tie at the threshold
        return np.round(rng.normal(0.0, 1.2, n)).astype(F32)
    if kind == "cluster":
        return (np.uint32(CLUSTER_BASE) + rng.integers(0, 40, n).astype(np.uint32)).view(F32)
    raise KeyError(kind)


def trim_reads(chunk):
    """[(label, raw, start, end)]: the reads of one chunk size -- whole chunks x (start, cut) x value kind; the first chunks // 4 and the last chunks // 5 chunks
    of the stretch [start, end) are stalls (constant).  Every read has at least one whole chunk."""
    out = []
    ci = TRIM_CHUNKS.index(chunk)
    for chunks in trim_whole_chunks(chunk):
        for si, (start, cut) in enumerate(((0, 0), (chunk + 1, 0), (7, 5))):
            for ki, kind in enumerate(TRIM_KINDS):
                n = start + chunks * chunk + chunk // 2 + cut
                rng = np.random.default_rng([15, ci, chunks, si, ki])
                x = trim_values(kind, n, rng)
                lead, tail = chunks // 4, chunks // 5
                x[start:start + lead * chunk] = x[start]
                if tail:
                    x[start + (chunks - tail) * chunk:start + chunks * chunk] = x[start + chunks * chunk - 1]
                out.append(("%s chunks %d start %d cut %d" % (kind, chunks, start, cut), x, start, n - cut))
    return out


ELEMENT_LENGTHS = (1, 2, 255, 256, 257, 4097)


def element_values(n, rng):
    """finite values of every size with +-inf, NaN, +-0 and denormals strewn in (element-wise modes only: no selection sees these)"""
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, DENORM, -DENORM, 5e-39, FLT_MAX, -FLT_MAX], dtype=F32)
    k = max(1, n // 3)
    x[rng.choice(n, k, replace=False)] = rng.choice(special, k)
    return x
