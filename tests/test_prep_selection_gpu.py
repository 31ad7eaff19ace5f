"""Signal preparation's exact selections (ffhip_prep.hip: wave_select2, wg_select2; kernels k_prep, k_quantiles, k_mad) held to a sort -- tests/prep_ref.py, itself held
to the oracle by tests/test_prep_ref.py -- on inputs chosen against them rather than for them:

  * values in the last bin of a radix pass and the first bin of the top one (>= 2^127, +-inf, large negatives), denormals and +-0, clusters that differ in the last key
    bytes only, constants and two-valued arrays;
  * "step" arrays whose sorted[idx] and sorted[idx + 1] sit on a bucket boundary of each of the four passes, with and without one duplicate to spare
    (the `kk + 1 < nequal` test at its edge);
  * chunk sizes that are no multiple of 64, the limits 2 and 1024 and the refusal at 1025; reads of fewer chunks than a workgroup's four waves; stalls; chunk MADs
    tied at the threshold; raw_table.start != 0 and end != n; the MAD half of ffhip_prep_stats;
  * the element-wise modes on +-inf, NaN, +-0 and denormals.

Equality is prep_ref.same(): equal bits, NaN equals NaN, +0 equals -0 (floatcmp ties them; see prep_ref.py).  NaN never enters a selection beside other values."""
import ctypes as C

import numpy as np
import pytest

import prep_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
PREP_DIFFERENCE, PREP_SHIFT_SCALE = 3, 4                  # include/ffhip.h: ffhip_array_transform only


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def gpu_quantiles(B, engine, x, p):
    got = np.array(p, dtype=F32, ndmin=1)
    assert B.lib().ffhip_quantiles(engine.h, _f(x), x.size, _f(got), got.size) == 0
    return got


# ---------------------------------------------------------------------------------------------------------------- a. single arrays
@pytest.mark.parametrize("name", R.FAMILIES)
def test_single_arrays(B, engine, name):
    """ffhip_quantiles (nine quantiles), ffhip_mad without and with a given median, ffhip_medmad_normalise with its statistics: 14 lengths of one value family"""
    L = B.lib()
    arrays = [(n, x) for fam, n, x in R.single_arrays() if fam == name]
    assert len(arrays) == len(R.LENGTHS) - (2 if name == "inf" else 0)
    nan_quantiles = 0
    for n, x in arrays:
        keep = x.copy()
        want = R.quantilef(x, R.QUANTILES)
        got = gpu_quantiles(B, engine, x, R.QUANTILES)
        assert R.same(got, want), (name, n, got, want)
        nan_quantiles += int(np.isnan(want).sum())
        mad = C.c_float(-1.0)
        assert L.ffhip_mad(engine.h, _f(x), n, None, C.byref(mad)) == 0
        assert R.same(F32(mad.value), R.madf(x)), (name, n, mad.value, R.madf(x))
        med = C.c_float(R.GIVEN_MEDIAN)
        assert L.ffhip_mad(engine.h, _f(x), n, C.byref(med), C.byref(mad)) == 0
        assert R.same(F32(mad.value), R.madf(x, R.GIVEN_MEDIAN)), (name, n, mad.value, R.madf(x, R.GIVEN_MEDIAN))
        assert np.array_equal(x.view(np.uint32), keep.view(np.uint32))             # inputs of the const entry points untouched
        y, wmed, wmad = R.medmad_normalise_array(x)
        a, gmed, gmad = x.copy(), C.c_float(-1.0), C.c_float(-1.0)
        assert L.ffhip_medmad_normalise(engine.h, _f(a), n, C.byref(gmed), C.byref(gmad)) == 0
        assert R.same(F32(gmed.value), wmed) and R.same(F32(gmad.value), wmad), (name, n, gmed.value, wmed, gmad.value, wmad)
        assert R.same(a, y), (name, n)
    if name == "inf":
        assert nan_quantiles > 0                          # 0 * inf above the selected rank: NaN on both sides (util.c:129)


# ---------------------------------------------------------------------------------------------------------------- b. rank-boundary steps
@pytest.mark.parametrize("pair", list(R.STEP_PAIRS))
def test_step_arrays(B, engine, pair):
    """idx + 1 (+ 1) copies of a, the rest b: sorted[idx] is the last a -- or the last but one -- and a, b differ in the sign, in one key byte, or inside the top pass's
    last or first bin"""
    cases = [c for c in R.step_arrays() if c[0] == pair]
    assert len(cases) == len(R.STEP_LENGTHS) * len(R.STEP_QUANTILES) * 2
    a, b = R.STEP_PAIRS[pair]
    boundaries = 0
    for _, n, p, extra, idx, x in cases:
        s = np.sort(x, kind="stable")
        if extra == 0 and idx + 1 < n:
            assert s[idx] == a and s[idx + 1] == b and s[idx] != s[idx + 1], (pair, n, p)      # the boundary the case claims to probe is there
            boundaries += 1
        want = R.quantilef(x, p)
        got = gpu_quantiles(B, engine, x, p)[0]
        assert R.same(got, want), (pair, n, float(p), extra, idx, got, want)
    assert boundaries == len(R.STEP_LENGTHS) * (len(R.STEP_QUANTILES) - 1)


# ---------------------------------------------------------------------------------------------------------------- c. one large array
def test_large_array(B, engine):
    """n = 2^24 + 3: floats are 2 apart at n - 1, so the position p * (n - 1), its integer part and (float)idx all round on the way"""
    x = R.large_array()
    want = R.quantilef(x, R.LARGE_QUANTILES)
    got = gpu_quantiles(B, engine, x, R.LARGE_QUANTILES)
    assert R.same(got, want), (got, want)


# ---------------------------------------------------------------------------------------------------------------- d. the trim grid
@pytest.fixture(scope="module")
def grid():
    """{chunk: (reads, {params: [None | (start, end, signal, median, MAD)]})} from prep_ref alone, computed once and left unchanged"""
    out = {}
    for chunk in R.TRIM_CHUNKS:
        reads = R.trim_reads(chunk)
        want = {}
        for prm in R.trim_params(chunk):
            perc, trim_start, trim_end = prm
            rows = []
            for _, raw, start, end in reads:
                r = R.trim_and_segment_raw(raw, start, end, trim_start, trim_end, chunk, perc)
                rows.append(None if r is None else r + R.medmad_normalise_array(raw[r[0]:r[1]]))
            want[prm] = rows
        out[chunk] = (reads, want)
    return out


def test_trim_grid_keeps_and_rejects(grid):
    """on the reference's answers alone: the grid cannot be passed by rejecting everything, nor by keeping everything, and it holds a kept read whose MAD is 0"""
    rows = [r for _, want in grid.values() for rs in want.values() for r in rs]
    kept = [r for r in rows if r is not None]
    assert len(rows) == 3072
    assert len(kept) >= 0.4 * len(rows), len(kept)
    assert len(rows) - len(kept) >= 0.1 * len(rows), len(kept)
    flat = [r for r in kept if r[1] - r[0] > 1 and r[4] == 0]
    assert flat and all(not np.isfinite(r[2]).any() for r in flat), len(flat)          # (x - med) / 0: +-inf or NaN, every sample


def check_prepared(p, reads, rows, what):
    for i, ((label, raw, _, _), want) in enumerate(zip(reads, rows)):
        s, e = p.range(i)
        if want is None:
            assert s >= e, (what, label, s, e)
            continue
        assert (s, e) == want[:2], (what, label, (s, e), want[:2])
        med, mad = p.stats(i)
        assert R.same(F32(med), want[3]) and R.same(F32(mad), want[4]), (what, label, med, want[3], mad, want[4])
        assert R.same(p.signal(i), want[2]), (what, label)


@pytest.mark.parametrize("chunk", R.TRIM_CHUNKS)
def test_trim_grid(B, engine, grid, chunk):
    """all 96 reads of a chunk size -- 1 .. 257 whole chunks, three (start, end) stretches, four value kinds, stalls at both ends -- in ONE launch per (quantile, trims):
    range, signal, median and MAD of every read"""
    reads, want = grid[chunk]
    raws = [r[1] for r in reads]
    ranges = [(r[2], r[3]) for r in reads]
    for prm, rows in want.items():
        perc, trim_start, trim_end = prm
        p = B.Prepared(engine, raws, trim_start=trim_start, trim_end=trim_end, varseg_chunk=chunk, varseg_thresh=perc, ranges=ranges)
        try:
            check_prepared(p, reads, rows, (chunk, prm))
        finally:
            p.close()


def test_begin_and_finish_equal_create_on_the_hostile_batch(B, engine, grid):
    chunk = 65
    reads, want = grid[chunk]
    raws = [r[1] for r in reads]
    ranges = [(r[2], r[3]) for r in reads]
    prm = R.trim_params(chunk)[2]
    p = B.Prepared(engine, raws, trim_start=prm[1], trim_end=prm[2], varseg_chunk=chunk, varseg_thresh=prm[0], ranges=ranges, begin_only=True)
    try:
        p.finish()
        check_prepared(p, reads, want[prm], ("begin/finish", chunk, prm))
    finally:
        p.close()


def test_reads_without_a_whole_chunk_are_rejected(B, engine):
    """nchunk == 0: the reference reads past an empty allocation there, the kernel rejects the read -- between reads that are kept, in one launch"""
    chunk = 100
    good = [r for r in R.trim_reads(chunk) if r[0] in ("dac chunks 8 start 0 cut 0", "round chunks 9 start 7 cut 5")]
    assert len(good) == 2 and all(R.trim_and_segment_raw(raw, s, e, 0, 0, chunk, 0.0) for _, raw, s, e in good)
    rng = np.random.default_rng(16)
    short = [(R.trim_values("dac", n, rng), s, e) for n, s, e in ((1, 0, 1), (99, 0, 99), (350, 120, 219), (350, 350, 350), (3, 1, 2))]
    batch = [short[0], good[0][1:], short[1], short[2], good[1][1:], short[3], short[4]]
    p = B.Prepared(engine, [b[0] for b in batch], trim_start=0, trim_end=0, varseg_chunk=chunk, varseg_thresh=0.0, ranges=[b[1:] for b in batch])
    try:
        for i, (raw, start, end) in enumerate(batch):
            s, e = p.range(i)
            if (end - start) // chunk == 0:
                assert s >= e, (i, s, e)
                with pytest.raises(B.FFHipError):
                    p.signal(i)
                continue
            r = R.trim_and_segment_raw(raw, start, end, 0, 0, chunk, 0.0)
            assert r is not None and (s, e) == r
            y, med, mad = R.medmad_normalise_array(raw[s:e])
            assert R.same(p.signal(i), y) and R.same(F32(p.stats(i)[0]), med) and R.same(F32(p.stats(i)[1]), mad)
    finally:
        p.close()


def test_chunk_limits(B, engine):
    x = R.trim_values("dac", 5000, np.random.default_rng(17))
    with pytest.raises(B.FFHipError):
        B.Prepared(engine, [x], varseg_chunk=1025)                                 # kMaxChunk = 1024 samples of LDS a wave
    with pytest.raises(B.FFHipError):
        B.Prepared(engine, [x], varseg_chunk=100, ranges=[(0, x.size + 1)])       # end beyond the read
    with pytest.raises(B.FFHipError):
        B.Prepared(engine, [x], varseg_chunk=100, ranges=[(11, 10)])              # start beyond end
    p = B.Prepared(engine, [x], trim_start=0, trim_end=0, varseg_chunk=1024)
    assert p.range(0) == R.trim_and_segment_raw(x, 0, x.size, 0, 0, 1024, 0.0)
    p.close()


# ---------------------------------------------------------------------------------------------------------------- e. element-wise modes
@pytest.mark.parametrize("n", R.ELEMENT_LENGTHS)
def test_element_wise_modes(B, engine, n):
    """ffhip_array_transform in its three modes and Prepared(mode = PREP_NONE / PREP_DELTA) against the one-line float32 forms, IEEE propagation included"""
    L = B.lib()
    x = R.element_values(n, np.random.default_rng([18, n]))
    assert n < 255 or (np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[x != 0]) < 1e-38).any() and np.signbit(x[x == 0]).any())
    a = x.copy()
    assert L.ffhip_array_transform(engine.h, _f(a), n, PREP_DIFFERENCE, 0.0, 1.0) == 0
    assert R.same(a, R.difference_array(x)), n
    for shift, scale in ((-3.25, 2.5), (1e30, -7e-4), (0.0, 3e38)):
        a = x.copy()
        assert L.ffhip_array_transform(engine.h, _f(a), n, PREP_SHIFT_SCALE, shift, scale) == 0
        assert R.same(a, R.shift_scale_array(x, shift, scale)), (n, shift, scale)
    want = R.shift_scale_array(R.difference_array(x), 0.0, 2.5)                    # flappie.c:257-258
    a = x.copy()
    assert L.ffhip_array_transform(engine.h, _f(a), n, B.PREP_DELTA, 0.0, 2.5) == 0
    assert R.same(a, want), n
    for mode in (PREP_SHIFT_SCALE, B.PREP_DELTA):
        a = x.copy()
        assert L.ffhip_array_transform(engine.h, _f(a), n, mode, 0.0, 0.0) != 0   # scale 0 is refused
        assert np.array_equal(a.view(np.uint32), x.view(np.uint32))
    # through a preparation without trimming (varseg_chunk = 0): the whole read, and a stretch of it
    lo, hi = (0, n) if n < 3 else (1, n - 1)
    for rng_ in ((0, n), (lo, hi)):
        p = B.Prepared(engine, [x], varseg_chunk=0, mode=B.PREP_NONE, ranges=[rng_])
        assert p.range(0) == rng_ and np.array_equal(p.signal(0).view(np.uint32), x[rng_[0]:rng_[1]].view(np.uint32))
        p.close()
        p = B.Prepared(engine, [x], varseg_chunk=0, mode=B.PREP_DELTA, delta=2.5, ranges=[rng_])
        assert p.range(0) == rng_ and R.same(p.signal(0), R.shift_scale_array(R.difference_array(x[rng_[0]:rng_[1]]), 0.0, 2.5))
        p.close()
    with pytest.raises(B.FFHipError):
        B.Prepared(engine, [x], varseg_chunk=0, mode=B.PREP_DELTA, delta=0.0)
