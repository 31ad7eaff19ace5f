"""flappie --modbase-tags on the CPU: the exported tag formatter and the tagged record writers of libflappie_host.so (include/flappie_modbase.h)
against the restatement in modbase_ref.py; the ML byte at its interval boundaries; the option's refusals, which need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import modbase_ref as R
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, BasecallInfo, _cfile, needs_hdf5
from test_host_layer import RawTable


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_modbase_tags.restype = C.c_int
    L.flappie_modbase_tags.argtypes = [C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.fprintf_format.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo]
    L.fprintf_modbase_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo, C.POINTER(C.c_uint8)]
    L.flappie_model_has_modbase.restype = C.c_int
    L.flappie_model_has_modbase.argtypes = [C.c_int]
    return L


def _tags(L, seq, ml):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    arr = np.ascontiguousarray(ml, dtype=np.uint8)
    mm, mv = C.c_void_p(), C.c_void_p()
    assert L.flappie_modbase_tags(seq.encode(), arr.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(mm), C.byref(mv)) == 0
    out = (C.string_at(mm.value).decode(), C.string_at(mv.value).decode())
    libc.free(mm)
    libc.free(mv)
    return out


def test_formatter_equals_the_restatement(L):
    rng = np.random.default_rng(3)
    cases = [("", []), ("AGTAGT", [7, 0, 0, 9, 1, 2]), ("CCCC", [0, 255, 128, 1]), ("ACGTTGCAC", list(range(9)))]
    call = "".join(rng.choice(list("ACGTZ"), 300))
    ml = [int(v) if c in "CZ" else 0 for c, v in zip(call, rng.integers(0, 256, 300))]
    cases.append((R.seq_of(call), ml))
    rcall, _, rml = R.oriented(call, "!" * 300, ml, True)
    cases.append((R.seq_of(rcall), rml))
    big = "".join(rng.choice(list("ACGT"), 100000))
    cases.append((big, [int(v) for v in rng.integers(0, 256, 100000)]))
    every = "".join("CA"[k % 2] for k in range(512))      # every ML value 0 .. 255 at a C, with an A between
    cases.append((every, [k // 2 if k % 2 == 0 else 77 for k in range(512)]))
    for seq, ml in cases:
        assert _tags(L, seq, ml) == R.tags(seq, ml)
    assert R.tags("", []) == ("MM:Z:C+m?;", "ML:B:C")
    assert R.tags("AGT", [0, 0, 0]) == ("MM:Z:C+m?;", "ML:B:C")
    assert R.tags("CAC", [5, 0, 255]) == ("MM:Z:C+m?,0,0;", "ML:B:C,5,255")
    assert R.ml_values(_tags(L, every, cases[-1][1])[1]) == list(range(256))


def test_ml_byte_boundaries():
    assert R.ml_byte(0.0) == 0 and R.ml_byte(1.0) == 255
    for k in range(256):
        assert R.ml_byte(k / 256.0) == k                     # the interval [k/256, (k+1)/256) starts at k/256
        assert R.ml_byte(np.nextafter((k + 1) / 256.0, 0.0)) == k
    # from posterior rows: all mass on Z, all on C, equal, none (underflow), and p = k/256 exactly
    row = np.full(60, -np.inf)
    row[40] = 0.0
    assert R.ml_byte(R.p_mod(row)) == 255
    row = np.full(60, -np.inf)
    row[51] = 0.0
    assert R.ml_byte(R.p_mod(row)) == 0
    row[54] = 0.0
    assert R.ml_byte(R.p_mod(row)) == 128
    assert R.p_mod(np.full(60, -np.inf)) == 0.0
    zs, cs = [40 + f for f in range(10)] + [54, 59], [10 + f for f in range(10)] + [51, 56]      # the 12 entries of occ(4) and of occ(1)
    for nz, nc, k in ((1, 7, 32), (1, 3, 64), (1, 1, 128), (3, 1, 192), (7, 1, 224), (12, 0, 255), (0, 12, 0)):
        row = np.full(60, -np.inf)
        row[zs[:nz]] = 0.0
        row[cs[:nc]] = 0.0
        row[[0, 25, 33]] = 0.0                               # (A, G, T mass counts for nothing)
        assert R.p_mod(row) == nz / (nz + nc) and R.ml_byte(R.p_mod(row)) == k


def test_tagged_records_equal_the_restatement(L, tmp_path):
    libc = C.CDLL(None)
    call, qual = "ZACGTZCCAZT", "!#%+5?IJ+,-"
    ml = [201, 0, 3, 0, 0, 255, 0, 128, 0, 17, 0]
    for reverse in (False, True):
        c, q, m = R.oriented(call, qual, ml, reverse)
        res = BasecallInfo(score=np.float32(-123.5), basecall=c.encode(), quality=q.encode(), basecall_length=len(c), nblock=37)
        res.rt = RawTable(uuid=b"u-1", n=4000, start=200, end=3990, raw=None)
        arr = np.array(m, dtype=np.uint8)
        for fmt in range(3):
            pd, pt = tmp_path / ("d%d" % fmt), tmp_path / ("t%d" % fmt)
            fp = _cfile(libc, pd)
            L.fprintf_format(fmt, fp, b"u-1", b"a.fast5", True, b"PRE_", res)
            libc.fclose(fp)
            fp = _cfile(libc, pt)
            L.fprintf_modbase_record(fmt, fp, b"u-1", b"a.fast5", True, b"PRE_", res, arr.ctypes.data_as(C.POINTER(C.c_uint8)))
            libc.fclose(fp)
            default, tagged = pd.read_text().split("\n"), pt.read_text()
            if fmt == 0:
                assert default[1] == c
                assert tagged == R.tagged_fasta(default[0][1:], c, m)
            elif fmt == 1:
                assert default[1] == c and default[3] == q
                assert tagged == R.tagged_fastq(default[0][1:], c, q, m)
            else:
                assert tagged == R.tagged_sam(default[0].split("\t")[0], c, q, m)
                assert len(tagged.rstrip("\n").split("\t")) == 13
            assert "Z" not in tagged.split("\n")[1 if fmt < 2 else 0].split("\tMM:")[0]
    assert [L.flappie_model_has_modbase(k) for k in range(4)] == [0, 0, 1, 0]


@needs_hdf5
def test_option_and_its_refusals_without_gpu():
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--modbase-tags" in r.stdout
    r = subprocess.run([FLAPPIE, "--model", "r941_native", "--modbase-tags", "x.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "modified base" in r.stderr
    r = subprocess.run([FLAPPIE, "--modbase-tags", "x.fast5"], capture_output=True, text=True, timeout=60)      # (the default model has none either)
    assert r.returncode != 0
    r = subprocess.run([RUNNIE, "--modbase-tags", "x.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
