"""flappie --poly-tail without a GPU: the restatement of include/ffhip.h "poly tail" (polytail_ref.py) against its scan-shaped second statement on random flags; the
host side (options, tag text, rounding, summary of libflappie_host.so); the CLI's refusals."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import polytail_ref as R
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, needs_hdf5


# ------------------------------------------------------------------------------------ the restatement
def test_walk_and_scans_give_the_same_candidates():
    rng = np.random.default_rng(5)
    assert R.candidates([], 2) == R.candidates_scan([], 2) == []
    for n in (1, 2, 7, 64, 300):
        for G in (0, 1, 2, 16):
            assert R.candidates(np.ones(n, np.uint8), G) == R.candidates_scan(np.ones(n, np.uint8), G) == [(0, n)]
            assert R.candidates(np.zeros(n, np.uint8), G) == R.candidates_scan(np.zeros(n, np.uint8), G) == []
    cases = 0
    for _ in range(3000):
        n, G = int(rng.integers(1, 200)), int(rng.integers(0, 17))
        flag = (rng.random(n) < rng.choice([0.05, 0.3, 0.6, 0.95])).astype(np.uint8)
        a, b = R.candidates(flag, G), R.candidates_scan(flag, G)
        assert a == b, (flag.tolist(), G, a, b)
        for ws, we in a:                                    # starts and ends on a flagged window; no unflagged run inside is longer than G
            assert flag[ws] and flag[we - 1]
            gaps = np.diff(np.flatnonzero(flag[ws:we])) - 1
            assert gaps.size == 0 or gaps.max() <= G
        for (_, e0), (s1, _) in zip(a, a[1:]):              # ... and more than G between two of them
            assert s1 - e0 > G
        assert sum(int(flag[ws:we].sum()) for ws, we in a) == int(flag.sum())
        cases += len(a) > 1
    assert cases > 1000


def test_the_tie_rules_and_the_reach():
    p = R.params(min_windows=2, search=4, gap=0)
    cands = [(0, 3), (5, 8), (9, 12)]
    assert R.choose(cands, 12, p) == (0, 3)                              # equal lengths: the smallest ws
    assert R.choose(cands, 12, dict(p, from_end=1)) == (9, 12)          # ... from the end: the largest we
    assert R.choose(cands, 12, dict(p, search=12)) == (0, 3) and R.choose(cands, 12, dict(p, from_end=1, search=12)) == (9, 12)
    assert R.choose([(0, 3), (5, 8), (10, 12)], 12, dict(p, from_end=1, search=5)) == (5, 8)      # the longest of those in reach (we > 12 - 5)
    assert R.choose([(0, 3), (5, 8), (10, 12)], 12, dict(p, from_end=1, search=4)) == (10, 12)    # we = NW - R is not in reach
    assert R.choose(cands, 12, dict(p, search=1)) == (0, 3) and R.choose([(1, 4)], 12, dict(p, search=1)) is None
    assert R.choose(cands, 12, dict(p, min_windows=4)) is None and R.choose(cands, 12, dict(p, min_windows=3)) == (0, 3)
    assert R.choose([(0, 2), (3, 9)], 12, p) == (3, 9)                   # ws = R - 1 is in reach ...
    assert R.choose([(0, 2), (4, 10)], 12, p) == (0, 2)                  # ... ws = R is not


def test_record_by_hand_and_both_statements():
    S, K = 5, 2
    # 40 blocks: a noisy start, a flat stretch over windows 3 .. 9 with one noisy window inside, then the transcript
    rng = np.random.default_rng(1)
    x = rng.standard_normal(40 * S).astype(np.float32)
    x[3 * K * S:10 * K * S] = 0.75
    x[6 * K * S:7 * K * S] = rng.standard_normal(K * S)
    bases = np.concatenate((rng.integers(0, 4, 6), np.zeros(14, int), np.tile([1, 2, 3, 0], 5)))
    path = R.path_of_bases(bases)
    p = R.params(window=K, min_calls=2, gap=1, min_windows=3, search=10, min_bases=5, max_sd=0.01)
    for scan in (False, True):
        rec = R.record(x, S, path, 4, p, scan=scan)
        assert (int(rec["status"]), int(rec["first"]), int(rec["count"]), int(rec["flat"])) == (1, 3 * K * S, 7 * K * S, 6)
        assert float(rec["level"]) == 0.75
        c = int(R.moves(path)[20:].sum())
        assert c == 19 and float(rec["rate"]) == float(np.float32(100.0 / c)) and float(rec["bases"]) == float(np.float32(70.0 * c / 100.0))
    assert int(R.record(x, S, path, 4, dict(p, min_bases=20))["status"]) == 3
    assert int(R.record(x, S, path, 4, dict(p, gap=0, min_windows=4))["status"]) == 2
    assert int(R.record(x[:3], S, path, 4, p)["status"]) == 2                 # NW = 0
    mu, q, flag, thr = R.windows(x, S, path, 4, p)
    assert flag.tolist() == [0, 0, 0, 1, 1, 1, 0, 1, 1, 1] + [0] * 10 and q[3] == 0.0 and R.margin(q, thr) > 1e-9
    # Z read as C on an nbase 5 path
    p5 = R.path_of_bases(np.where(bases == 0, 4, bases), nbase=5)
    assert int(R.record(x, S, p5, 5, dict(p, base=1))["status"]) == 1 and int(R.record(x, S, p5, 5, p)["status"]) == 2


# ------------------------------------------------------------------------------------ the host side
class Opts(C.Structure):
    _fields_ = [("base", C.c_int), ("from_end", C.c_int), ("window", C.c_int), ("min_calls", C.c_int), ("gap", C.c_int), ("min_windows", C.c_int),
                ("search", C.c_long), ("min_bases", C.c_int), ("max_sd", C.c_float)]


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in R.PARAM_FIELDS[:8]] + [("max_sd", C.c_float)]


class Rec(C.Structure):
    _fields_ = [("status", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("flat", C.c_int32), ("calls", C.c_int32),
                ("level", C.c_float), ("rate", C.c_float), ("bases", C.c_float)]


class Summary(C.Structure):
    _fields_ = [("reads", C.c_ulonglong), ("found", C.c_ulonglong), ("no_rate", C.c_ulonglong), ("bases", C.POINTER(C.c_float)), ("n", C.c_size_t), ("cap", C.c_size_t)]


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_polytail_defaults.argtypes = [C.POINTER(Opts)]
    L.flappie_polytail_defaults.restype = None
    L.flappie_polytail_set.argtypes = [C.POINTER(Opts), C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_polytail_params.argtypes = [C.POINTER(Opts), C.c_int, C.POINTER(Params), C.c_char_p, C.c_size_t]
    L.flappie_polytail_bases.argtypes = [C.POINTER(Rec)]
    L.flappie_polytail_bases.restype = C.c_long
    L.flappie_polytail_tags.argtypes = [C.POINTER(Rec), C.c_size_t]
    L.flappie_polytail_tags.restype = C.c_void_p
    L.flappie_polytail_count.argtypes = [C.POINTER(Summary), C.POINTER(Rec)]
    L.flappie_polytail_median.argtypes = [C.POINTER(Summary)]
    L.flappie_polytail_median.restype = C.c_double
    L.flappie_polytail_summary_print.argtypes = [C.c_void_p, C.POINTER(Summary)]
    L.flappie_polytail_summary_print.restype = None
    L.flappie_polytail_summary_free.argtypes = [C.POINTER(Summary)]
    L.flappie_polytail_summary_free.restype = None
    return L


def _tags(L, rec, trim):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    p = L.flappie_polytail_tags(C.byref(rec), trim)
    assert p
    text = C.string_at(p).decode()
    libc.free(p)
    return text


def test_options_and_parameters(L):
    o, p, err = Opts(), Params(), C.create_string_buffer(256)
    L.flappie_polytail_defaults(C.byref(o))
    assert L.flappie_polytail_params(C.byref(o), 5, C.byref(p), err, 256) == 0
    assert [getattr(p, k) for k in R.PARAM_FIELDS[:8]] == [0, 0, 8, 4, 2, 5, 500, 20] and p.max_sd == np.float32(0.3)
    assert L.flappie_polytail_params(C.byref(o), 2, C.byref(p), err, 256) == 0 and p.search == 1250
    for name, value in (("base", "T"), ("window", "7"), ("gap", "0"), ("min-windows", "1"), ("search", "30"), ("min-bases", "1"), ("max-sd", "0.5")):
        assert L.flappie_polytail_set(C.byref(o), name.encode(), value.encode(), err, 256) == 0, err.value
    assert L.flappie_polytail_params(C.byref(o), 5, C.byref(p), err, 256) == 0
    assert [getattr(p, k) for k in R.PARAM_FIELDS[:8]] == [3, 0, 7, 4, 0, 1, 1, 1] and p.max_sd == 0.5       # half of 7 rounded up; R = max(1, 30 // 35)
    assert L.flappie_polytail_set(C.byref(o), b"min-calls", b"0", err, 256) == 0
    assert L.flappie_polytail_params(C.byref(o), 5, C.byref(p), err, 256) == 0 and p.min_calls == 0
    assert L.flappie_polytail_set(C.byref(o), b"min-calls", b"8", err, 256) == 0            # within 0 .. 64, beyond this window
    assert L.flappie_polytail_params(C.byref(o), 5, C.byref(p), err, 256) == -1 and b"--poly-tail-min-calls" in err.value
    before = bytes(o)
    for name, value in (("base", "U"), ("base", "AC"), ("base", ""), ("base", "a"), ("window", "0"), ("window", "65"), ("window", "8x"), ("window", ""), ("min-calls", "-1"),
                        ("min-calls", "65"), ("gap", "17"), ("gap", "-1"), ("min-windows", "0"), ("search", "0"), ("min-bases", "0"), ("max-sd", "-0.1"), ("max-sd", "nan"),
                        ("max-sd", "x"), ("max-sd", "1e9"), ("sd", "1")):
        assert L.flappie_polytail_set(C.byref(o), name.encode(), value.encode(), err, 256) == -1, (name, value)
        assert ("--poly-tail-" + name).encode() in err.value and bytes(o) == before, (name, value, err.value)


def test_tags_and_rounding(L):
    for bases, want in ((0.0, 0), (0.49999997, 0), (0.5, 1), (1.5, 2), (2.5, 3), (99.5, 100), (100.49999, 100), (123456.5, 123457)):
        rec = Rec(1, 1000, 4000, 90, 3, 0.8, 41.25, bases)
        assert L.flappie_polytail_bases(C.byref(rec)) == want, bases
        assert _tags(L, rec, 250) == "pt:i:%d\tpa:B:i,1250,5250\tpr:f:41.25" % want
    rate = np.float32(1234567.0 / 891.0)
    assert _tags(L, Rec(1, 0, 40, 1, 0, 0.0, rate, 7.0), 0) == "pt:i:7\tpa:B:i,0,40\tpr:f:%.9g" % rate
    assert np.float32(_tags(L, Rec(1, 0, 40, 1, 0, 0.0, rate, 7.0), 0).split("pr:f:")[1]) == rate       # written so that it reads back
    for status in (2, 3, 0):
        rec = Rec(status, 1000, 4000, 90, 3, 0.8, 0.0, 0.0)
        assert L.flappie_polytail_bases(C.byref(rec)) == -1 and _tags(L, rec, 250) == "pt:i:-1"
    assert L.flappie_polytail_tags(None, 0) is None


def test_summary(L, tmp_path):
    from test_cli import _cfile
    libc = C.CDLL(None)
    s = Summary()
    assert math.isnan(L.flappie_polytail_median(C.byref(s)))
    rng = np.random.default_rng(2)
    vals = []
    for i in range(2501):                                    # (beyond the first room of 1024)
        status = (1, 1, 2, 3)[i % 4]
        v = np.float32(rng.uniform(0, 300))
        assert L.flappie_polytail_count(C.byref(s), C.byref(Rec(status, 0, 0, 0, 0, 0.0, 1.0 if status == 1 else 0.0, v if status == 1 else 0.0))) == 0
        if status == 1:
            vals.append(v)
        if i in (0, 1, 4, 2500):
            assert L.flappie_polytail_median(C.byref(s)) == float(np.median(np.array(vals, np.float64))), i
    assert (s.reads, s.found, s.no_rate) == (2501, len(vals), 625)
    out = tmp_path / "summary.txt"
    fp = _cfile(libc, out)
    L.flappie_polytail_summary_print(fp, C.byref(s))
    libc.fclose.argtypes = [C.c_void_p]
    libc.fclose(fp)
    assert out.read_text() == "polytail\treads\t2501\npolytail\tfound\t%d\npolytail\tno_rate\t625\npolytail\tmedian\t%.1f\n" % (len(vals), np.median(np.array(vals, np.float64)))
    L.flappie_polytail_summary_free(C.byref(s))
    assert s.n == 0 and not s.bases


# ------------------------------------------------------------------------------------ the binary, without a GPU
OPTS = ("--poly-tail", "--poly-tail-base", "--poly-tail-end", "--poly-tail-window", "--poly-tail-min-calls", "--poly-tail-max-sd", "--poly-tail-gap",
        "--poly-tail-min-windows", "--poly-tail-search", "--poly-tail-min-bases")


@needs_hdf5
def test_cli_refusals_without_gpu(tmp_path):
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in OPTS:
        assert opt in r.stdout, opt
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert not any(opt in r.stdout for opt in OPTS)

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    for args in (["--poly-tail"], ["--poly-tail-end"], ["--poly-tail-window", "4"], ["--poly-tail-base", "A"], ["--poly-tail", "--poly-tail-gap", "1"]):
        assert "--poly-tail is flappie's" in refused(RUNNIE, *args)
    for args in (["--poly-tail-end"], ["--poly-tail-base", "A"], ["--poly-tail-search", "100"]):
        assert "go with --poly-tail" in refused(FLAPPIE, *args)
    kit = tmp_path / "kit.fa"                                 # (never written: the refusal comes before any file is read)
    assert "--split-reads" in refused(FLAPPIE, "--poly-tail", "--adapters", str(kit), "--split-reads")
    for opt, value in (("base", "U"), ("base", "AC"), ("window", "0"), ("window", "65"), ("min-calls", "65"), ("max-sd", "-1"), ("max-sd", "abc"), ("gap", "17"),
                       ("min-windows", "0"), ("search", "0"), ("min-bases", "0")):
        assert "--poly-tail-" + opt in refused(FLAPPIE, "--poly-tail", "--poly-tail-" + opt, value), (opt, value)
    assert "--poly-tail-min-calls" in refused(FLAPPIE, "--poly-tail-min-calls", "5", "--poly-tail", "--poly-tail-window", "4")
    assert "--poly-tail-min-calls" in refused(FLAPPIE, "--poly-tail", "--poly-tail-window", "4", "--poly-tail-min-calls", "5")
