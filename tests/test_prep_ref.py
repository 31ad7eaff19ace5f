"""tests/prep_ref.py (the sort-based numpy statement of signal preparation that tests/test_prep_selection_gpu.py and tests/test_host_layer.py hold the kernels to)
against the oracle's C restatement of util.c / flappie_common.c, on every hostile input those tests use -- every case but the reads without one whole chunk, on which
the reference reads past an empty allocation.  No GPU.  Passing here also shows that the inputs are what the GPU tests take them for: no NaN beside other values in
any selection, a real rank boundary in every "step" array, enough kept and rejected reads in the trim grid."""
import ctypes as C

import numpy as np
import pytest

import prep_ref as R
from oracle import ffo


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_quantiles_mad_and_normalisation_of_single_arrays():
    L = ffo.lib()
    seen_nan = 0
    for name, n, x in R.single_arrays():
        want = R.QUANTILES.copy()
        L.fo_quantilef(_f(x), n, _f(want), want.size)
        got = R.quantilef(x, R.QUANTILES)
        assert R.same(got, want), (name, n, got, want)
        seen_nan += int(np.isnan(want).any())
        assert R.same(R.medianf(x), np.float32(L.fo_medianf(_f(x), n))), (name, n)
        assert R.same(R.madf(x), np.float32(L.fo_madf(_f(x), n, None))), (name, n)
        med = C.c_float(R.GIVEN_MEDIAN)
        assert R.same(R.madf(x, R.GIVEN_MEDIAN), np.float32(L.fo_madf(_f(x), n, C.byref(med)))), (name, n)
        y = x.copy()
        L.fo_medmad_normalise_array(_f(y), n)
        assert R.same(R.medmad_normalise_array(x)[0], y), (name, n)
    assert seen_nan > 0                                # 0 * inf above the selected rank (util.c:129)


def test_step_arrays_have_their_rank_boundary():
    L = ffo.lib()
    boundaries = 0
    for name, n, p, extra, idx, x in R.step_arrays():
        s = np.sort(x, kind="stable")
        if extra == 0 and idx + 1 < n:
            assert s[idx] != s[idx + 1], (name, n, p)
            boundaries += 1
        want = np.array([p], dtype=np.float32)
        L.fo_quantilef(_f(x), n, _f(want), 1)
        assert R.same(R.quantilef(x, p), want[0]), (name, n, p, extra)
    assert boundaries == len(R.STEP_PAIRS) * len(R.STEP_LENGTHS) * (len(R.STEP_QUANTILES) - 1)      # every p < 1


def test_large_array_quantiles():
    x = R.large_array()
    assert np.spacing(np.float32(x.size - 1)) == 2     # positions round to even integers up here
    want = R.LARGE_QUANTILES.copy()
    ffo.lib().fo_quantilef(_f(x), x.size, _f(want), want.size)
    assert R.same(R.quantilef(x, R.LARGE_QUANTILES), want)


@pytest.mark.parametrize("chunk", R.TRIM_CHUNKS)
def test_trim_grid(chunk):
    L = ffo.lib()
    kept = rejected = 0
    for label, raw, start, end in R.trim_reads(chunk):
        assert (end - start) // chunk >= 1
        for perc, trim_start, trim_end in R.trim_params(chunk):
            s, e = C.c_size_t(start), C.c_size_t(end)
            rc = L.fo_trim_and_segment_raw(_f(raw), raw.size, C.byref(s), C.byref(e), trim_start, trim_end, chunk, perc)
            got = R.trim_and_segment_raw(raw, start, end, trim_start, trim_end, chunk, perc)
            assert got == (None if rc else (s.value, e.value)), (label, perc, trim_start, trim_end)
            s, e = C.c_size_t(start), C.c_size_t(end)
            assert L.fo_trim_raw_by_mad(_f(raw), C.byref(s), C.byref(e), chunk, perc) == 0
            assert R.trim_raw_by_mad(raw, start, end, chunk, perc) == (s.value, e.value), (label, perc)
            if got is None:
                rejected += 1
                continue
            kept += 1
            x = raw[got[0]:got[1]].copy()
            y, med, mad = R.medmad_normalise_array(x)
            assert R.same(med, np.float32(L.fo_medianf(_f(x), x.size))) and R.same(mad, np.float32(L.fo_madf(_f(x), x.size, C.byref(C.c_float(med)))))
            z = x.copy()
            L.fo_medmad_normalise_array(_f(z), z.size)
            assert R.same(y, z), (label, perc, trim_start, trim_end)
    assert kept and rejected


def test_element_wise_forms():
    x = np.array([1.0, 3.5, -2.0, np.inf, 0.0], dtype=np.float32)
    assert R.same(R.difference_array(x), np.array([2.5, -5.5, np.inf, -np.inf, 0.0], dtype=np.float32))                 # util.c:278-287
    assert R.same(R.shift_scale_array(x, 1.0, 2.0), np.array([0.0, 1.25, -1.5, np.inf, -0.5], dtype=np.float32))       # util.c:215-223
    assert R.same(R.difference_array(x[:1]), np.zeros(1, dtype=np.float32))


def test_refusals_of_the_reference_itself():
    with pytest.raises(AssertionError):
        R.quantilef(np.array([1.0, np.nan, 2.0], dtype=np.float32), 0.5)              # no order for NaN under floatcmp
    assert np.isnan(R.quantilef(np.full(4, np.nan, dtype=np.float32), 0.5))           # ... but one answer when there is nothing else
    assert R.trim_raw_by_mad(np.zeros(10, dtype=np.float32), 3, 7, 5, 0.0) is None    # no whole chunk
    assert R.same(np.float32(0.0), np.float32(-0.0)) and not R.same(np.float32(1.0), np.float32(1.0000001))
