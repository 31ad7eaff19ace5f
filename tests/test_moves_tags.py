"""flappie --emit-moves on the CPU: the definition of the move table against the oracle's and the host library's change_positions and against the
oracle's basecall; the inverse map from (ts, stride, mv) to sample ranges; the exported formatter, mean quality and record writer of
libflappie_host.so (include/flappie_moves.h) against the restatement in moves_ref.py, byte for byte; the option's presence and refusal, which need no GPU."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import modbase_ref as MR
import moves_ref as R
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, BasecallInfo, _cfile, needs_hdf5
from test_host_layer import RawTable

U8P = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_mean_quality.restype = C.c_double
    L.flappie_mean_quality.argtypes = [C.c_char_p]
    L.flappie_moves_tags.restype = C.c_void_p
    L.flappie_moves_tags.argtypes = [U8P, C.c_size_t, C.c_int, C.POINTER(RawTable), C.c_char_p, C.c_float, C.c_float, C.c_bool]
    L.fprintf_format.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo]
    L.fprintf_modbase_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo, U8P]
    L.fprintf_moves_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo, U8P, U8P, C.c_int, C.c_float, C.c_float,
                                       C.c_bool]
    L.change_positions.restype = C.c_size_t
    L.change_positions.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_int)]
    return L


def crafted_paths(nstate=8):
    """seeded random paths of 1, 2, 3, 64, 65, 1000 blocks (nblock + 1 entries), with all-stay and all-change ones"""
    rng = np.random.default_rng(5)
    out = []
    for nblock in (1, 2, 3, 64, 65, 1000):
        out.append(np.full(nblock + 1, 3, dtype=np.int32))                                  # all stay
        out.append((np.arange(nblock + 1) % nstate).astype(np.int32))                       # all change
        for frac in (0.2, 0.5, 0.9):
            p = rng.integers(0, nstate, nblock + 1).astype(np.int32)
            stay = rng.random(nblock + 1) < frac
            for i in range(1, nblock + 1):
                if stay[i]:
                    p[i] = p[i - 1]
            out.append(p)
    return out


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def test_positions_equal_change_positions_and_moves_sit_one_block_before(L):
    from oracle import ffo
    for path in crafted_paths():
        nblock = path.size - 1
        want = R.positions(path)
        for fn in (ffo.lib().fo_change_positions, L.change_positions):
            idx = np.zeros(nblock + 1, dtype=np.int32)
            n = fn(_ip(path), nblock, _ip(idx))
            assert list(idx[:n]) == want, nblock
        mv = R.moves(path)
        assert mv.size == nblock and mv[-1] == 0
        assert list(np.flatnonzero(mv)) == [p - 1 for p in want]
    assert list(R.moves(np.array([0, 1], np.int32))) == [0]                                 # one block: path[1] is never emitted
    assert list(R.moves(np.array([0, 1, 2], np.int32))) == [1, 0]
    assert list(R.moves(np.array([0, 0, 2, 2, 3], np.int32))) == [0, 1, 0, 0]


def test_moves_of_the_oracle_path_spell_the_oracle_call():
    from oracle import ffo
    bases = 0
    for kind, nbase in ((M.NET_LSTM5, 4), (M.NET_GRUMOD5, 5)):
        mdl = M.synthetic_model(kind, 48, seed=6)
        assert mdl.nbase == nbase
        om = ffo.OracleModel(mdl)
        rng = np.random.default_rng(nbase)
        for n in (700, 1500):
            sig = rng.standard_normal(n).astype(np.float32)
            for viterbi in (False, True):
                ref = om.basecall(sig, viterbi_only=viterbi)
                mv = R.moves(ref["path"])
                assert mv.size == ref["nblock"]
                assert int(mv.sum()) == len(ref["basecall"])
                assert R.call_through_moves(ref["path"], mv, nbase) == ref["basecall"]
                bases += len(ref["basecall"])
    assert bases >= 200


def test_sample_ranges_from_the_tags_alone():
    for stride in (2, 5):
        for path in crafted_paths():
            nblock = path.size - 1
            start = 203
            mv = R.moves(path)
            fields = R.tags(mv, stride, 99999, start, "", 0.0, 1.0, True)
            ts = int(fields[1][len("ts:i:"):])
            got_stride, kept = R.parse_mv(fields[-1])
            assert got_stride == stride
            pos = R.positions(path)
            rng = R.base_samples(ts, stride, kept)
            assert len(rng) == len(pos)
            if not pos:
                assert kept == [] and ts == start
                continue
            assert kept[0] == 1 and kept[-1] == 0
            assert rng[0][0] == ts
            assert ts + stride * len(kept) == start + stride * nblock                       # the table reaches the last block's end
            for k, (a, e) in enumerate(rng):
                assert a == start + stride * (pos[k] - 1) and a < e
                if k:
                    assert rng[k - 1][1] == a                                               # disjoint and ascending: one base's range ends where the next begins


def _tags(L, mv, stride, rt, qual, median, mad, delta):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    arr = np.ascontiguousarray(mv, dtype=np.uint8)
    p = L.flappie_moves_tags(arr.ctypes.data_as(U8P) if arr.size else None, arr.size, stride, C.byref(rt), qual.encode() if qual is not None else None,
                             median, mad, delta)
    assert p
    out = C.string_at(p).decode()
    libc.free(p)
    return out


def test_formatter_equals_the_restatement(L):
    rng = np.random.default_rng(8)
    rt = RawTable(uuid=b"u", n=123456, start=211, end=120000, raw=None)
    big = (rng.random(100001) < 0.4).astype(np.int32).cumsum().astype(np.int32) % 8        # a path of 100 000 blocks
    cases = [np.array([2, 2], np.int32), np.array([2, 2, 2, 2, 2], np.int32),               # empty calls
             np.array([0, 0, 0, 5, 5, 5], np.int32),                                         # one base, b0 = 2
             np.array([0, 1, 1], np.int32),                                                  # one base, b0 = 0
             big] + crafted_paths()
    med, mad = np.float32(87.31234), np.float32(11.0476)
    for path in cases:
        mv = R.moves(path)
        n = int(mv.sum())
        qual = "".join(chr(33 + int(v)) for v in rng.integers(0, 60, n))
        for stride in (2, 5):
            for delta in (False, True):
                want = "\t".join(R.tags(mv, stride, rt.n, rt.start, qual, med, mad, delta))
                assert _tags(L, mv, stride, rt, qual, med, mad, delta) == want, (path.size, stride, delta)
    empty = _tags(L, R.moves(cases[0]), 5, rt, "", med, mad, False).split("\t")
    assert empty[0] == "ns:i:123456" and empty[1] == "ts:i:211" and empty[-1] == "mv:B:c,5"
    assert empty[2:5] == ["sm:f:%.9g" % float(med), "sd:f:%.9g" % float(mad), "sv:Z:med_mad"]
    one = _tags(L, R.moves(cases[2]), 2, rt, "5", med, mad, True).split("\t")
    assert one == ["qs:f:20.000", "ns:i:123456", "ts:i:215", "mv:B:c,2,1,0,0"]
    assert len(_tags(L, R.moves(big), 5, rt, "", med, mad, True).split("\t")[-1]) > 150000
    # a stride that does not fit int8 is refused
    arr = np.ones(3, np.uint8)
    assert not L.flappie_moves_tags(arr.ctypes.data_as(U8P), 3, 128, C.byref(rt), b"", med, mad, False)


def test_mean_quality(L):
    for n in (1, 7, 1000):
        assert "%.3f" % L.flappie_mean_quality(("!" * n).encode()) == "0.000"
        for q in (1, 10, 20, 37, 93):
            got = L.flappie_mean_quality((chr(33 + q) * n).encode())
            assert "%.3f" % got == "%.3f" % float(q), (n, q, got)
    # a two-value mix against the closed form: a characters of quality p, b of quality q
    for a, p, b, q in ((1, 10, 1, 20), (3, 7, 5, 30), (100, 2, 1, 60)):
        s = chr(33 + p) * a + chr(33 + q) * b
        closed = -10.0 * math.log10((a * 10.0 ** (-p / 10.0) + b * 10.0 ** (-q / 10.0)) / (a + b))
        got = L.flappie_mean_quality(s.encode())
        assert "%.3f" % got == "%.3f" % closed, (s, got, closed)
        assert got == R.mean_quality(s)
    rng = np.random.default_rng(1)
    s = "".join(chr(33 + int(v)) for v in rng.integers(0, 94, 5000))
    assert L.flappie_mean_quality(s.encode()) == R.mean_quality(s)


def _write(L, libc, path, fn, *a):
    fp = _cfile(libc, path)
    fn(*a[:1], fp, *a[1:])
    libc.fclose(fp)
    return path.read_text()


def test_records_equal_the_restatement(L, tmp_path):
    libc = C.CDLL(None)
    # an 11-base call of a 10-state model over 40 blocks: path with moves at chosen blocks
    call, qual = "ZACGTZCCAZT", "!#%+5?IJ+,-"
    ml = [201, 0, 3, 0, 0, 255, 0, 128, 0, 17, 0]
    blocks = [3, 4, 9, 10, 15, 20, 21, 30, 31, 35, 38]
    state = {"A": 0, "C": 1, "G": 2, "T": 3, "Z": 4}
    # entry b + 1 is the state after block b
    path = np.zeros(41, dtype=np.int32)
    path[0] = 2
    for b in range(40):
        prev = int(path[b])
        if b in blocks:
            s = state[call[blocks.index(b)]]
            path[b + 1] = s + 5 if prev == s else s
        else:
            path[b + 1] = prev
    path[40] = (int(path[39]) + 1) % 10
    mv = R.moves(path)
    assert list(np.flatnonzero(mv)) == blocks and R.call_through_moves(path, mv, 5) == call
    mva = np.ascontiguousarray(mv)
    med, mad = np.float32(93.25), np.float32(12.625001)
    for reverse in (False, True):
        for with_ml in (False, True):
            c, q, m = R.oriented(call, qual, ml if with_ml else None, reverse)
            res = BasecallInfo(score=np.float32(-123.5), basecall=c.encode(), quality=q.encode(), basecall_length=len(c), nblock=40)
            res.rt = RawTable(uuid=b"u-1", n=4000, start=200, end=3990, raw=None)
            mla = np.array(m, dtype=np.uint8) if with_ml else None
            mlp = mla.ctypes.data_as(U8P) if with_ml else None
            for stride in (2, 5):
                for delta in (False, True):
                    for fmt in range(3):
                        default = _write(L, libc, tmp_path / "d", L.fprintf_format, fmt, b"u-1", b"a.fast5", True, b"PRE_", res).split("\n")
                        tagged = _write(L, libc, tmp_path / "t", L.fprintf_moves_record, fmt, b"u-1", b"a.fast5", True, b"PRE_", res, mlp,
                                        mva.ctypes.data_as(U8P), stride, med, mad, delta)
                        args = (c, q, mv, stride, 4000, 200, med, mad, delta, m)
                        ntag = 4 + (0 if delta else 3) + (2 if with_ml else 0)
                        if fmt == 0:
                            assert tagged == R.tagged_fasta(default[0][1:], *args)
                        elif fmt == 1:
                            assert tagged == R.tagged_fastq(default[0][1:], *args)
                            assert tagged.split("\n")[3] == q
                        else:
                            assert tagged == R.tagged_sam(default[0].split("\t")[0], *args)
                            f = tagged.rstrip("\n").split("\t")
                            assert len(f) == 11 + ntag and tagged.count("\n") == 1
                            assert f[9] == (MR.seq_of(c) if with_ml else c) and f[10] == q
                        line = tagged.split("\n")[0]
                        assert len(line.split("\t")) == (11 if fmt == 2 else 1) + ntag
                        # mv is in signal order whatever the orientation
                        assert R.parse_mv(line.split("\t")[-1]) == (stride, [int(v) for v in mv[3:]])
                        assert ("ts:i:%d" % (200 + stride * 3)) in line.split("\t")
                        if with_ml:
                            assert line.split("\t")[-ntag:][:2] == list(MR.tags(MR.seq_of(c), m))
            # the writers without these tags write what they wrote
            if with_ml:
                for fmt in range(3):
                    default = _write(L, libc, tmp_path / "d", L.fprintf_format, fmt, b"u-1", b"a.fast5", True, b"PRE_", res).split("\n")
                    tagged = _write(L, libc, tmp_path / "t", L.fprintf_modbase_record, fmt, b"u-1", b"a.fast5", True, b"PRE_", res, mlp)
                    want = (MR.tagged_fasta(default[0][1:], c, m) if fmt == 0 else MR.tagged_fastq(default[0][1:], c, q, m) if fmt == 1
                            else MR.tagged_sam(default[0].split("\t")[0], c, q, m))
                    assert tagged == want
    # the tagless records: the reference's layout, untouched
    res = BasecallInfo(score=np.float32(-10.0), basecall=b"ACGT", quality=b"!!!!", basecall_length=4, nblock=20)
    res.rt = RawTable(uuid=b"u-2", n=100, start=0, end=100, raw=None)
    fq = _write(L, libc, tmp_path / "d", L.fprintf_format, 1, b"u-2", b"b.fast5", False, b"", res)
    assert fq.split("\n")[1:] == ["ACGT", "+", "!!!!", ""] and fq.startswith("@b.fast5  { \"filename\" : \"b.fast5\", \"uuid\" : \"u-2\", ") and "\t" not in fq
    sam = _write(L, libc, tmp_path / "d", L.fprintf_format, 2, b"u-2", b"b.fast5", False, b"", res)
    assert sam == "b.fast5\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t!!!!\nACGT\t!!!!\n"
    # an empty call
    res = BasecallInfo(score=np.float32(-1.0), basecall=b"", quality=b"", basecall_length=0, nblock=3)
    res.rt = RawTable(uuid=b"u-3", n=100, start=7, end=100, raw=None)
    z = np.zeros(3, np.uint8)
    sam = _write(L, libc, tmp_path / "t", L.fprintf_moves_record, 2, b"u-3", b"c.fast5", True, b"", res, None, z.ctypes.data_as(U8P), 5, med, mad, False)
    assert sam == R.tagged_sam("u-3", "", "", z, 5, 100, 7, med, mad, False)
    assert sam.rstrip("\n").split("\t")[11:] == ["ns:i:100", "ts:i:7", "sm:f:93.25", "sd:f:%.9g" % float(mad), "sv:Z:med_mad", "mv:B:c,5"]


@needs_hdf5
def test_option_and_its_refusal_without_gpu():
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--emit-moves" in r.stdout
    r = subprocess.run([RUNNIE, "--emit-moves", "x.fast5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--emit-moves" not in r.stdout
