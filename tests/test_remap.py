"""flappie --remap on the CPU: the restatement (remap_ref.py) against a brute-force enumeration of every path; the reader of the sequences and the start[] /
maxdev derivation of libflappie_host.so (include/flappie_remap.h) through ctypes; the options and their refusals; the library's new entries.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import remap_ref as R
from test_cli import FLAPPIE, HOSTLIB, ROOT, RUNNIE, _cfile, needs_hdf5

U8P = C.POINTER(C.c_uint8)
LIBFFHIP = os.path.join(ROOT, "flappie_amd", "libffhip.so")


class Refs(C.Structure):
    _fields_ = [("n", C.c_int), ("name", C.POINTER(C.c_char_p)), ("codes", C.POINTER(U8P)), ("len", C.POINTER(C.c_size_t)), ("bad", C.POINTER(C.c_int)),
                ("order", C.POINTER(C.c_int))]


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_remap_refs_parse.restype = C.POINTER(Refs)
    L.flappie_remap_refs_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_remap_refs_read.restype = C.POINTER(Refs)
    L.flappie_remap_refs_read.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_remap_refs_free.argtypes = [C.POINTER(Refs)]
    L.flappie_remap_refs_free.restype = None
    L.flappie_remap_refs_find.argtypes = [C.POINTER(Refs), C.c_char_p, C.c_char_p]
    L.flappie_remap_starts.argtypes = [U8P, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.flappie_remap_write_line.restype = C.c_long
    L.flappie_remap_write_line.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, U8P, C.c_float]
    return L


def test_restatement_equals_brute_force_on_every_small_case():
    rng = np.random.default_rng(3)
    n = 0
    for nbase in (4, 5):
        P = 2 * nbase * (nbase + 1)
        for N in range(1, 9):
            for Ln in range(1, N + 2):
                T = (rng.integers(-6, 7, (N, P)) * 0.25).astype(np.float32)      # multiples of 0.25: exact sums, ties abound
                s = rng.integers(0, 2 if (N + Ln) % 2 else nbase, Ln)           # (two letters: homopolymers, the flip / flop coding)
                for W in (0, 1, Ln):
                    score, rm = R.remap(T, s, nbase, W)
                    bscore, brm = R.brute(T, s, nbase, W)
                    assert score == bscore and np.array_equal(rm, brm), (nbase, N, Ln, W, score, bscore, rm, brm)
                    assert int(rm.sum()) == Ln - 1
                    start, maxdev = R.starts_maxdev(rm, Ln)
                    assert maxdev <= W and start[0] == 0 and len(start) == Ln
                    n += 1
    assert n == 2 * 3 * sum(N + 1 for N in range(1, 9))
    assert R.flipflop_code([0, 0, 0, 1, 1, 0], 4) == [0, 4, 0, 1, 5, 0] and R.trans_lookup(3, 1, 4) == 11 and R.trans_lookup(3, 7, 4) == 35
    assert [R.centre(b, 4, 7) for b in range(8)] == [0, 0, 0, 1, 1, 2, 2, 3]


FASTA = ">read-1 first record\nacgt\nAC\n\n>file_b.fast5\tcomment\nTTTT\n>bad one\nACGN\nAC\n>zed\nACGZ\n>empty\n>file_c\nG\n"


def test_reader_of_the_sequences(L, tmp_path):
    err = C.create_string_buffer(256)
    for alphabet, zbad in ((b"ACGT", 1), (b"ACGTZ", 0)):
        p = L.flappie_remap_refs_parse(FASTA.encode(), alphabet, err, 256)
        assert p, err.value
        r = p.contents
        assert r.n == 6 and [r.name[k] for k in range(6)] == [b"read-1", b"file_b.fast5", b"bad", b"zed", b"empty", b"file_c"]
        assert [r.bad[k] for k in range(6)] == [0, 0, 1, zbad, 0, 0]
        assert [r.codes[0][i] for i in range(r.len[0])] == [0, 1, 2, 3, 0, 1]              # two lines, lower case
        assert r.len[1] == 4 and r.len[4] == 0 and r.len[5] == 1 and r.codes[5][0] == 2
        if not zbad:
            assert [r.codes[3][i] for i in range(r.len[3])] == [0, 1, 2, 4]
        # by read id first, then by the file's base name, then by that without its extension; a missing record
        assert L.flappie_remap_refs_find(p, b"read-1", b"/x/file_b.fast5") == 0
        assert L.flappie_remap_refs_find(p, b"nobody", b"/x/file_b.fast5") == 1
        assert L.flappie_remap_refs_find(p, b"", b"dir/file_c.fast5") == 5
        assert L.flappie_remap_refs_find(p, b"read-", b"dir/file_") == -1 and L.flappie_remap_refs_find(p, None, None) == -1
        L.flappie_remap_refs_free(p)
    assert not L.flappie_remap_refs_parse(b"ACGT\n>a\nAC\n", b"ACGT", err, 256) and b"first record" in err.value
    assert not L.flappie_remap_refs_parse(b"> \nAC\n", b"ACGT", err, 256)
    assert not L.flappie_remap_refs_read(str(tmp_path / "missing.fa").encode(), b"ACGT", err, 256) and b"read" in err.value
    f = tmp_path / "refs.fa"
    f.write_text(FASTA * 3000)                              # (longer than the reader's first buffer)
    p = L.flappie_remap_refs_read(str(f).encode(), b"ACGT", err, 256)
    assert p and p.contents.n == 18000 and L.flappie_remap_refs_find(p, b"zed", None) == 3      # the first of equal names
    L.flappie_remap_refs_free(p)


def _starts(L, rm, Ln):
    rm = np.ascontiguousarray(rm, np.uint8)
    start, dev = (C.c_size_t * max(1, Ln))(), C.c_size_t(12345)
    rc = L.flappie_remap_starts(rm.ctypes.data_as(U8P), rm.size, Ln, start, C.byref(dev))
    return rc, list(start)[:Ln], dev.value


def test_starts_and_maxdev(L, tmp_path):
    rng = np.random.default_rng(9)
    cases = [(np.zeros(7, np.uint8), 1), (np.ones(7, np.uint8), 8), (np.array([0, 0, 1, 0, 1, 1, 0], np.uint8), 4), (np.array([1], np.uint8), 2)]
    for _ in range(40):
        N = int(rng.integers(1, 60))
        rm = (rng.random(N) < rng.random()).astype(np.uint8)
        cases.append((rm, int(rm.sum()) + 1))
    for rm, Ln in cases:
        rc, start, dev = _starts(L, rm, Ln)
        wstart, wdev = R.starts_maxdev(rm, Ln)
        assert rc == 0 and start == wstart and dev == wdev, (rm, Ln)
    assert _starts(L, np.zeros(7, np.uint8), 1)[1:] == ([0], 0) and _starts(L, np.ones(7, np.uint8), 8)[1:] == (list(range(8)), 0)
    assert _starts(L, np.ones(7, np.uint8), 7)[0] == -1 and _starts(L, np.zeros(7, np.uint8), 0)[0] == -1
    # the table's line
    libc = C.CDLL(None)
    out = tmp_path / "map.tsv"
    fh = _cfile(libc, out)
    rm = np.array([0, 0, 1, 0, 1, 1, 0], np.uint8)
    assert L.flappie_remap_write_line(fh, b"r1", 1, 7, 5, 210, 4, 2048, rm.ctypes.data_as(U8P), np.float32(-3.14159274)) == R.starts_maxdev(rm, 4)[1]
    assert L.flappie_remap_write_line(fh, b"r2", 2, 7, 5, 0, 9, 16, None, 0.0) == 0
    assert L.flappie_remap_write_line(fh, b"r3", 1, 7, 5, 0, 3, 16, rm.ctypes.data_as(U8P), 0.0) == -1
    libc.fclose(fh)
    assert out.read_text() == "r1\t1\t7\t5\t210\t4\t2048\t%d\t%.9g\t0,3,5,6\nr2\t2\t7\t5\t0\t9\t16\t*\t*\t*\n" % (R.starts_maxdev(rm, 4)[1], np.float32(-3.14159274))


@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    refs = tmp_path / "refs.fa"
    refs.write_text(FASTA)
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--remap=", "--remap-out=", "--remap-band="):
        assert opt in r.stdout, opt
    assert "SIGNAL order" in r.stdout
    # long options only: no short form stands before any of the three (argp makes one of a printable key)
    for line in r.stdout.split("\n"):
        if re.search(r"--remap(-out|-band)?=", line):
            assert re.match(r"^ {6}--remap(-out|-band)?=", line), line
    assert "0-2303" in r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--remap" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out = tmp_path / "map.tsv"
    assert "--remap" in refused(RUNNIE, "--remap", str(refs))
    assert "--remap-out" in refused(FLAPPIE, "--remap", str(refs))
    assert "--remap" in refused(FLAPPIE, "--remap-out", str(out))
    assert "--remap" in refused(FLAPPIE, "--remap-band", "5")
    assert "--remap-band" in refused(FLAPPIE, "--remap", str(refs), "--remap-out", str(out), "--remap-band", "-1")
    # a band whose window 2 W + 1 no kernel form holds (4608 cells) is refused here, not when a long sequence meets it in a batch; so is what is no number
    for w in ("2304", "100000", "12x", ""):
        assert "--remap-band" in refused(FLAPPIE, "--remap", str(refs), "--remap-out", str(out), "--remap-band", w)
    assert "invalid option" in refused(FLAPPIE, "-!", "5") and "--remap-band" not in refused(FLAPPIE, "-!", "5")
    assert "missing.fa" in refused(FLAPPIE, "--remap", str(tmp_path / "missing.fa"), "--remap-out", str(out))
    assert not out.exists()


def test_library_exports_the_new_entries():
    lib = C.CDLL(LIBFFHIP)
    for name in ("ffhip_batch_set_remap", "ffhip_batch_remap", "ffhip_op_remap", "ffhip_debug_remap_form"):
        assert hasattr(lib, name), name
    lib.ffhip_debug_remap_form.argtypes = [C.c_size_t, C.c_int]
    # the kernel form by the window min(2 W + 1, L): one wave up to 256 cells, a workgroup up to 4608, none beyond
    assert [lib.ffhip_debug_remap_form(Ln, W) for Ln, W in ((64, 2048), (65, 31), (65, 32), (256, 2048), (257, 2048), (1025, 600), (30000, 2048), (5000, 2304), (4608, 9999))] == \
        [0, 0, 1, 1, 2, 3, 3, -1, 3]
    from flappie_amd import binding
    assert binding.RUN_REMAP == 32768 and hasattr(binding.Batch, "set_remap") and hasattr(binding.Batch, "remap") and hasattr(binding, "op_remap")


def test_a_finite_score_has_a_path_and_a_score_that_is_not_finite_is_not_mapped():
    """the status rule of include/ffhip.h "remap" on scores no network emits (hostile_scores.py): under a finite V_N[L - 1] the bits lead through allowed cells to
    position 0; under a NaN or an infinity they need not, and remap_status follows none of them.  Both directions occur for every sparse style."""
    import hostile_scores as H
    seen = {style: [0, 0] for style in H.STYLES}
    astray = 0
    for style, nbase, N, L, W, seed in H.remap_cases(H.REMAP_SHAPES[:4]):
        T, s = H.styled(style, seed, N, nbase), H.sequence(seed, L, nbase)
        V, bits = R._forward(T, s, nbase, W)
        rm, p, inside = R.traceback(bits, L)
        status, score, srm = R.remap_status(T, s, nbase, W)
        finite = bool(np.isfinite(V[L - 1]))
        assert status == (1 if finite else 2), (style, nbase, N, L, W)
        seen[style][status - 1] += 1
        if finite:
            assert p == 0 and inside and int(rm.sum()) == L - 1 and R.starts_maxdev(rm, L)[1] <= W, (style, nbase, N, L, W, p, inside)
            assert score.tobytes() == np.float32(V[L - 1]).tobytes() and np.array_equal(srm, rm)
            if np.isfinite(T).all():
                assert (score, rm.tolist()) == (lambda a: (a[0], a[1].tolist()))(R.remap(T, s, nbase, W))      # (remap() is unchanged for finite input)
        else:
            assert srm is None and score.tobytes() == b"\0\0\0\0"
            astray += not (p == 0 and inside)
    for style in H.SPARSE:
        assert min(seen[style]) >= 1, (style, seen)
    for style in ("flat", "quantised"):
        assert seen[style][1] == 0, (style, seen)
    for style in ("nan block", "all nan", "all -inf", "all +inf", "+-3e38"):
        assert seen[style][0] == 0, (style, seen)
    assert astray >= 20, astray      # why the rule is needed: the bits under such a score often describe no path
