"""Signal preparation from DAC values (ffhip_prep_create_dac / ffhip_prep_begin_dac, k_dac_to_pa in ffhip_prep.hip): the reads of a multi-read fast5
file reach the device as the int16 values the file holds, and a kernel in front of k_prep scales them to picoamperes -- (dac + offset) * raw_unit, an
add and a multiply, each rounded, which is what read_raw's host loop does for single-read files.  Everything here is bit for bit: against numpy
float32 for the kernel alone, against the float entries on host-scaled samples for what stands behind it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
# offset, range, digitisation: the reference's test constants (test_flappie_signal.c), a negative offset, a fractional one
CALS = [(16.0, 1373.41, 8192.0), (-231.0, 1467.61, 8192.0), (3.4375, 1402.882, 2048.0)]


def cal(offset, rng_, dig):
    """(offset, raw_unit) as the readers compute them: raw_unit = range / digitisation in float"""
    return F(offset), F(rng_) / F(dig)


def host_pa(dac, c):
    return ((dac.astype(F) + c[0]) * c[1]).astype(F)


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def dac_reads(seed, lens):
    """reads shaped like the signal-preparation tests' inputs: a quiet stretch in front, then noise around 500 +- 60 counts"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        x = 500 + 60 * rng.standard_normal(n)
        lead = min(300, n // 4)
        x[:lead] = 520 + 4 * rng.standard_normal(lead)
        out.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return out


@pytest.mark.parametrize("c", CALS)
def test_every_int16_value_against_numpy(B, engine, c):
    """(a) all 65 536 values in one read, no trimming, samples copied: the kernel's arithmetic alone"""
    x = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    x = np.random.default_rng(3).permutation(x)
    cc = cal(*c)
    p = B.Prepared(engine, [x], trim_start=0, trim_end=0, varseg_chunk=0, mode=B.PREP_NONE, calibrations=[cc])
    assert p.range(0) == (0, x.size)
    got = p.signal(0)
    p.close()
    want = host_pa(x, cc)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero(got != want)[:8]


def test_tails_offsets_and_upload_bytes(B, engine):
    """(b) lengths at which a vector tail or a read's offset can go wrong, each read with a calibration of its own; the bytes uploaded are the
    arithmetic of the layout: 2 a sample, every read padded to four samples, the four size_t tables and the calibrations"""
    lens = [1, 2, 3, 5, 4097, 9000]
    rng = np.random.default_rng(11)
    reads = [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens]
    cals = [cal(*CALS[i % 3]) if i < 3 else (F(rng.uniform(-300, 300)), F(rng.uniform(0.1, 0.3))) for i in range(len(lens))]
    counts = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts(counts, 1)
    p = B.Prepared(engine, reads, trim_start=0, trim_end=0, varseg_chunk=0, mode=B.PREP_NONE, calibrations=cals)
    B.lib().ffhip_copy_counts(counts, 0)
    padded = sum((n + 3) // 4 * 4 for n in lens)
    assert counts[1] == 2 * padded + 4 * 8 * len(lens) + 8 * len(lens), counts[1]
    for i, (r, c) in enumerate(zip(reads, cals)):
        assert p.range(i) == (0, r.size)
        got, want = p.signal(i), host_pa(r, c)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, np.flatnonzero(got != want)[:8])
    p.close()
    # the float entry uploads 4 bytes a sample for the same reads -- and takes varseg_chunk = 0 (no trimming at all) as the DAC entry does
    floats = [host_pa(r, c) for r, c in zip(reads, cals)]
    B.lib().ffhip_copy_counts(counts, 1)
    q = B.Prepared(engine, floats, trim_start=0, trim_end=0, varseg_chunk=0, mode=B.PREP_NONE)
    B.lib().ffhip_copy_counts(counts, 0)
    assert counts[1] == 4 * padded + 4 * 8 * len(lens)
    for i, x in enumerate(floats):
        assert q.range(i) == (0, x.size) and np.array_equal(q.signal(i).view(np.uint32), x.view(np.uint32)), i
    q.close()


LENS12 = [1200, 1500, 1999, 2600, 3000, 4000, 4013, 4097, 5555, 7001, 8192, 9000]


@pytest.mark.parametrize("mode", ["medmad", "delta"])
def test_the_two_entries_are_one(B, engine, mode):
    """(c) default trim and segmentation: ranges, statistics and prepared signals of the DAC entry equal the float entry's on host-scaled samples"""
    reads = dac_reads(29, LENS12)
    cals = [cal(*CALS[i % 3]) for i in range(len(reads))]
    kw = dict(mode=B.PREP_DELTA, delta=2.5) if mode == "delta" else {}
    a = B.Prepared(engine, [host_pa(r, c) for r, c in zip(reads, cals)], **kw)
    d = B.Prepared(engine, reads, calibrations=cals, **kw)
    e = B.Prepared(engine, reads, calibrations=cals, begin_only=True, **kw)
    e.finish()
    for i in range(len(reads)):
        assert a.range(i)[1] > a.range(i)[0]
        for x in (d, e):
            assert x.range(i) == a.range(i), i
            assert np.array_equal(np.array(x.stats(i), dtype=F).view(np.uint32), np.array(a.stats(i), dtype=F).view(np.uint32)), i
            assert np.array_equal(x.signal(i).view(np.uint32), a.signal(i).view(np.uint32)), i
    for x in (a, d, e):
        x.close()


def test_packed_batches_from_either_entry_call_the_same(B, engine):
    """(c) set_prepared_packed from the DAC entry gives the basecalls it gives from the float entry"""
    from flappie_amd import model as M
    reads = dac_reads(31, LENS12)
    cals = [cal(*CALS[i % 3]) for i in range(len(reads))]
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=3))
    calls = []
    for p in (B.Prepared(engine, [host_pa(r, c) for r, c in zip(reads, cals)]), B.Prepared(engine, reads, calibrations=cals)):
        lens = [p.range(i)[1] - p.range(i)[0] for i in range(len(reads))]
        pb = B.Batch(dm, 16, 10240, max_reads=len(reads))
        slot, off = pb.pack_plan(lens)
        assert all(s >= 0 for s in slot)
        pb.set_prepared_packed(p, list(range(len(reads))), list(slot), list(off))
        pb.run()
        pb.finish()
        calls.append([(pb.basecall(i), pb.quality(i)) for i in range(pb.nreads())])
        pb.close()
        p.close()
    dm.close()
    assert len(calls[0]) == len(reads) and all(len(c[0]) > 0 for c in calls[0])
    assert calls[0] == calls[1]


@pytest.mark.parametrize("first", ["dac", "float"])
@pytest.mark.parametrize("second", ["dac", "float"])
def test_one_preparation_may_be_pending(B, engine, first, second):
    """(d) a second preparation (either entry, begun or whole) while one is pending is refused, and the first is what it would have been"""
    reads = dac_reads(37, [1500, 4013, 2600])
    cals = [cal(*CALS[i]) for i in range(3)]
    floats = [host_pa(r, c) for r, c in zip(reads, cals)]

    def make(kind, **kw):
        return B.Prepared(engine, reads, calibrations=cals, **kw) if kind == "dac" else B.Prepared(engine, floats, **kw)

    ref = make("float")
    p = make(first, begin_only=True)
    for begin_only in (True, False):
        with pytest.raises(B.FFHipError):
            make(second, begin_only=begin_only)
    p.finish()
    for i in range(3):
        assert p.range(i) == ref.range(i) and np.array_equal(p.signal(i), ref.signal(i))
    q = make(second, begin_only=True)              # finish cleared the pending state ...
    q.close()                                      # ... and so does destroy
    r = make(second)
    assert r.range(0) == ref.range(0)
    for x in (p, r, ref):
        x.close()


_REHEARSAL_DAC = """
import numpy as np
from flappie_amd import binding as B
import test_prep_dac_gpu as T
eng = B.Engine(0)
reads = T.dac_reads(41, [150, 1500, 4013, 9000])
cals = [T.cal(*T.CALS[i % 3]) for i in range(len(reads))]
floats = [T.host_pa(r, c) for r, c in zip(reads, cals)]
for begin_only in (False, True):
    d = B.Prepared(eng, reads, calibrations=cals, begin_only=begin_only)
    f = B.Prepared(eng, floats, begin_only=begin_only)          # (nothing is pending under the rehearsal: the call is done when it returns)
    d.finish(); f.finish()
    for i, r in enumerate(reads):
        start = min(r.size, 200)
        assert d.range(i) == f.range(i) == (start, max(start, r.size - 10)), (i, d.range(i))
        assert d.stats(i) == f.stats(i) == (0.0, 1.0)
    d.close(); f.close()
print("rehearsal ok")
"""


def test_rehearsal_hook_takes_the_dac_entries():
    """the host-load rehearsal without the GPU (the hooks build; tools/host_scaling.py's emulated processes): the DAC entries do the host's share -- the int16
    gather into pinned staging -- and answer as the float entries do there: fixed trims, statistics (0, 1)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "tools", "test_hooks", "libffhip.so")
    assert os.path.exists(hooks), "tools/test_hooks/libffhip.so is missing: `make -C flappie_amd/csrc hooks`"
    env = dict(os.environ, FFHIP_BINDING_LIBRARY=hooks, FFHIP_DEBUG_HOST_REHEARSAL_MSPS="1000", FFHIP_DEBUG_HOST_REHEARSAL_NOGPU="1",
               PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", _REHEARSAL_DAC], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rehearsal ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
