"""The run-length ("runnie") decode kernels, both families, held to the oracle bit for bit where only additions and comparisons lie on the
way, and to float64 (tests/fp64_ref.py) where logarithms do.

    product path (nbase 4, stride 40; ffhip_decode.hip)     k_viterbi8x<1>, k_crf_fb<8, 1> + k_rle_post8, k_rle_partition8x
    generic path (ffhip_rle.hip)                            k_rle_viterbi, k_rle_transpost, k_rle_partition: nbase 1, 2, 3, 5; ALWAYS the C function
                                                            transpost_crf_runlength; a batch's posterior when 10 / temperature > kFbRange

The oracle (oracle/ffo) is the compiled reference bit for bit on these inputs, NaNs included, at every nbase 1..5.

1. Viterbi through decode_crf_runlength on any scores (ties, constants, NaN, +-inf): path equal, score equal to the bit, every state in range;
   block counts at the edges of the kernels' groups of 8 blocks, the ring of three groups, and one, two and three 2048-block traceback chunks.
2. The generic partition function against the oracle (fp64 re-association only) and against enumeration.
3. A batch's posterior on the batch's OWN transitions against fp64.  Error unit of a transition column (the shape / scale columns: equal bits):
       |got - want| / (ulp32(want) + ulp32(max_s |alpha[t]|) + ulp32(max_s |beta[t+1]|) + ulp32(max_p |S[t]|) + 2.5e-7)
   k_rle_post8 rounds log(fwd) and log(bwd) once each to fp32 and adds twice in fp32 (half an ulp a term); 2.5e-7 covers the float mantissa and
   logf on it, in both vectors.  Bound: 4 units (8 half-ulp roundings; the flip-flop chains' check allows 8 on a two-term sum).
   Path and score of the batch equal the oracle's decode of the matrix the batch decoded: its posterior, or its transitions in a
   RUN_VITERBI_ONLY run (decode.c reads whichever runnie.c hands it; only additions lie along the path).
   A read of this architecture has at least 4 blocks (a 19-sample window at stride 5; the engine refuses shorter ones, asserted below), so the
   shortest read stands where 1- and 2-block reads would; the operators of items 1, 2 and 4 take 1 and 2 blocks.
4. The generic posterior kernel, which repeats the reference's fp32 log-space order: its error is the reference's, moved by the device's
   expf / log1pf (1-2 ulp against glibc's sub-ulp).  Bound per matrix: 2 x (the oracle's own error on that matrix, same units) + 4.
   With NaN or -inf scores the NaN mask is the oracle's.  This found the backward chain's first step, written as a copy of x for
   lse(-inf, x), returning -inf where the reference's (-inf) - (-inf) gives NaN; the copy now selects NaN there.

Worst normalised errors, kernel / fp32 oracle on the same input, are printed with the module's report (run with -s).
Records of the first MI355X run, kernel / fp32 oracle, worst normalised over every read or matrix of the line:
    batch, k_crf_fb<8, 1> + k_rle_post8 (bound 4)     temperature 1        temperature 0.8
        ragged, 4 .. 129 blocks                       0.51 / 0.91          0.47 / 1.30
        packed, 4 .. 241 blocks                       0.51 / 4.61          0.48 / 4.86
        one read of 4101 blocks                       0.50 / 40.8          0.54 / 128.8
    k_rle_transpost (bound 2 x oracle + 4)
        operator, nbase 2 .. 5:   1 block 0 / 0;  2 blocks 0.31 / 0.31;  63: 1.57 / 1.57;  64: 1.82 / 2.01;  65: 1.72 / 1.72;
                                  129: 3.73 / 3.73;  800: 73.6 / 70.9
        batch at temperature 0.09, 4, 65 and 201 blocks     12.6 / 12.6   (scores of +-55: the logsumexp terms are mostly exact copies)
Every Viterbi and partition-function case was equal as stated at that run; the planted -inf cases failed before the select and pass with it.
"""
import ctypes as C

import numpy as np
import pytest

import fp64_ref as R
from flappie_amd import model as M
from oracle import ffo
from test_decode_gpu import _scores
from test_host_layer import CMat, HOSTLIB, _f
from test_packed_rle_gpu import _packed
from test_runlength import brute_force, random_param

pytestmark = pytest.mark.gpu

IP = C.POINTER(C.c_int)
PM = C.POINTER(CMat)
STYLES = ["normal", "tanh5", "ties", "flat", "nan", "some_nan", "nan_block", "rare_bad"]
K_FB_RANGE = 100.0          # kFbRange (ffhip_internal.hpp): the widest block of scores the fp64 linear-space chains take


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host():
    """the reference-named C functions of the host layer"""
    L = C.CDLL(HOSTLIB)
    L.mat_from_array.restype = PM
    L.mat_from_array.argtypes = [C.POINTER(C.c_float), C.c_size_t, C.c_size_t]
    L.free_flappie_matrix.restype = PM
    L.free_flappie_matrix.argtypes = [PM]
    L.runlengthV2_partition_function.restype = C.c_double
    L.runlengthV2_partition_function.argtypes = [PM]
    L.transpost_crf_runlength.restype = PM
    L.transpost_crf_runlength.argtypes = [PM]
    L.decode_crf_runlength.restype = C.c_float
    L.decode_crf_runlength.argtypes = [PM, IP]
    L.flappie_hip_shutdown.restype = None
    yield L
    L.flappie_hip_shutdown()


SEEN = {}


def note(key, kern, orac):
    k, o = SEEN.get(key, (0.0, 0.0))
    SEEN[key] = (max(k, kern), max(o, orac))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(SEEN):
        print("worst normalised error %-34s kernel %8.3f   fp32 oracle %8.3f" % (key, SEEN[key][0], SEEN[key][1]))


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_score(a, b):
    return bool(_bits([a])[0] == _bits([b])[0] or (np.isnan(a) and np.isnan(b)))


def _param(rng, nbase, nblock, style):
    """[nblock, 2 nbase (nbase + 1)]: scores of tests/test_decode_gpu.py's styles, the shape and scale columns made positive"""
    dense = _scores(rng, 2 * nbase * (nbase + 1), nblock, style)
    dense[:, : 2 * nbase] = np.abs(dense[:, : 2 * nbase]) + 1.0
    return np.ascontiguousarray(dense)


def _mk(host, a):
    return host.mat_from_array(_f(a), a.shape[1], a.shape[0])


def _host_transpost(host, param):
    m = _mk(host, param)
    post = host.transpost_crf_runlength(m)
    assert post
    c = post.contents
    got = np.ctypeslib.as_array(c.f, shape=(c.nc, c.stride))[:, : c.nr].copy()
    host.free_flappie_matrix(post)
    host.free_flappie_matrix(m)
    return got


def _oracle_decode(mat):
    """(path [nblock], score) of fo_decode_crf_runlength"""
    path = np.full(mat.shape[0] + 1, -7, np.int32)
    score = ffo.lib().fo_decode_crf_runlength(ffo.HostMat.from_dense(mat).ptr, path.ctypes.data_as(IP))
    return path[:-1], score


def _oracle_transpost(mat):
    return ffo.take(ffo.lib().fo_transpost_crf_runlength(ffo.HostMat.from_dense(mat).ptr))


def _amax(a):
    """row-wise largest finite magnitude"""
    return np.where(np.isfinite(a), np.abs(a), 0.0).max(axis=1, keepdims=True)


def norm_err(got, S, want, alpha, beta):
    """the error of transition columns `got` in the units of the module docstring (item 3); S, want, alpha, beta float64"""
    T = S.shape[0]
    denom = R.ulp32(np.where(np.isfinite(want), want, 0.0)) + R.ulp32(_amax(alpha[:T])) + R.ulp32(_amax(beta[1:])) + R.ulp32(_amax(S)) + 2.5e-7
    with np.errstate(invalid="ignore"):
        return np.abs(got.astype(np.float64) - want) / denom


def check_posterior(post, trans, nbase, key, generic):
    """a posterior [nblock, P] of the float32 matrix `trans` against fp64; generic: the bound of item 4 (else 4 units).  Returns (kernel, oracle) figures."""
    ns = 2 * nbase
    assert post.shape == trans.shape
    assert np.array_equal(_bits(post[:, :ns]), _bits(trans[:, :ns])), "%s: shape / scale columns are not the input's bits" % key
    S = trans[:, ns:].astype(np.float64)
    want, alpha, beta = R.runlength_transpost64(S, nbase)
    err = float(norm_err(post[:, ns:], S, want, alpha, beta).max())
    oerr = float(norm_err(_oracle_transpost(trans)[:, ns:], S, want, alpha, beta).max())
    note(key, err, oerr)
    bound = 2.0 * oerr + 4.0 if generic else 4.0
    print("%-34s %5d blocks: kernel %8.3f  fp32 oracle %8.3f  bound %8.3f" % (key, trans.shape[0], err, oerr, bound))
    assert err <= bound, "%s, %d blocks: worst normalised error %.3f above %.3f (fp32 oracle %.3f)" % (key, trans.shape[0], err, bound, oerr)
    return err, oerr


# ---- 1. Viterbi, operator level, any scores --------------------------------------------------------------------------------------
VITERBI_BLOCKS = {4: (1, 7, 8, 9, 17, 23, 24, 25, 300, 2047, 2048, 2049, 4097), 2: (1, 8, 9, 300, 2049, 4097), 3: (1, 8, 9, 300, 2049, 4097),
                  5: (1, 8, 9, 300, 2049, 4097)}


@pytest.mark.parametrize("style", STYLES)
@pytest.mark.parametrize("nbase", [4, 2, 3, 5])
def test_viterbi_any_scores_equal_the_oracle(host, nbase, style):
    """decode_crf_runlength (decode.c:927-1013): k_viterbi8x<1> for nbase 4 -- the literal scan of a group of 8 blocks holding a NaN or an infinity,
    the tie order (move b2, stay b2, b2 ascending; the stay state only if strictly greater), a -inf destination keeping traceback 0, the tail of
    fewer than 8 blocks, the 2048-block traceback chunks -- and k_rle_viterbi for nbase 2, 3, 5"""
    rng = np.random.default_rng(1000 * nbase + len(style) + ord(style[0]))
    for nblock in VITERBI_BLOCKS[nbase]:
        param = _param(rng, nbase, nblock, style)
        m = _mk(host, param)
        path = np.full(nblock + 1, -7, np.int32)
        score = host.decode_crf_runlength(m, path.ctypes.data_as(IP))
        host.free_flappie_matrix(m)
        want_path, want_score = _oracle_decode(param)
        assert path[:nblock].min() >= 0 and path[:nblock].max() < 2 * nbase, (nblock, path[:nblock].min(), path[:nblock].max())
        assert np.array_equal(path[:nblock], want_path), (nblock, int(np.flatnonzero(path[:nblock] != want_path)[0]))
        assert _same_score(score, want_score), (nblock, score, want_score)


# ---- 2. partition function, generic kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbase", [2, 3, 5])
def test_generic_partition_function(host, nbase):
    """runlengthV2_partition_function through k_rle_partition: the oracle's number up to fp64 re-association, and the enumeration's where it can be had"""
    rng = np.random.default_rng(20 + nbase)
    for nblock in (1, 8, 9, 150) + ((2, 5) if nbase == 2 else (3,) if nbase == 3 else ()):
        param = random_param(rng, nblock, nbase, scale=2.0)
        m = _mk(host, param)
        z = host.runlengthV2_partition_function(m)
        host.free_flappie_matrix(m)
        zw = ffo.lib().fo_runlengthV2_partition_function(ffo.HostMat.from_dense(param).ptr)
        assert abs(z - zw) <= 1e-9 * max(1.0, abs(zw)), (nblock, z, zw)
        if nbase <= 3 and nblock <= 5:
            logz = brute_force(param, nbase)[0]
            assert abs(z - logz) <= 2e-6 * max(1.0, abs(logz)), (nblock, z, logz)          # (the stay states go through the float logsumexpf)


# ---- 3. posterior, path and score of a batch on its own matrices ------------------------------------------------------------------
def _samples_for(mdl, nblock):
    """a read length of exactly nblock blocks"""
    n = nblock * mdl.total_stride
    assert mdl.nblock(n) == nblock
    return n


def _check_decode(b, r, mat, key):
    """the batch's path and score against the oracle's decode of `mat`, the matrix the batch decoded"""
    want_path, want_score = _oracle_decode(mat)
    path = b.path(r)[0]
    assert path.shape[0] == mat.shape[0] + 1 and np.array_equal(path[:-1], want_path), "%s read %d: path differs from the oracle's" % (key, r)
    assert _same_score(b.score(r), want_score), "%s read %d: score %r, the oracle's %r" % (key, r, b.score(r), want_score)


def _check_batch(B, dm, sigs, temperature, key, generic=False, make=None):
    """run the reads (ragged, or through make()), check every read's posterior against fp64 and its decode against the oracle, then the same
    reads Viterbi-only: the decode of the transitions"""
    for flags in (0, B.RUN_VITERBI_ONLY):
        if make is not None:
            b = make()
        else:
            b = B.Batch(dm, len(sigs), max(s.size for s in sigs))
            b.set_signals_ragged(sigs)
        b.run(temperature, flags)
        b.finish()
        for r in range(len(sigs)):
            trans = b.transitions(r)
            assert trans.shape == (b.read_nblock(r), 40)
            if flags == 0:
                post = b.posterior(r)
                check_posterior(post, trans, 4, key, generic)
                _check_decode(b, r, post, key)
            else:
                _check_decode(b, r, trans, key + " viterbi")
        b.close()


@pytest.fixture(scope="module")
def rle128(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=31)
    dm = B.DeviceModel(engine, mdl)
    yield mdl, dm
    dm.close()


RAGGED_BLOCKS = (33, 64, 65, 129)        # behind the shortest read, 4 blocks (module docstring)


@pytest.mark.parametrize("temperature", [1.0, 0.8])
def test_ragged_batch_posterior_against_fp64(B, rle128, temperature):
    """k_crf_fb<8, 1> + k_rle_post8 and k_viterbi8x<1> on a ragged batch: the shortest read, then block counts around the 32-block chunks of the
    chains and the 64-block rows of their vectors"""
    mdl, dm = rle128
    rng = np.random.default_rng(7)
    short = mdl.convs[-1].winlen                                 # one window of the last convolution: the shortest read the reference takes
    assert short == 19 and mdl.nblock(short) == 4
    # 1 and 2 blocks: no read of this architecture is that short, and the engine says so
    for nblock in (1, 2):
        b = B.Batch(dm, 1, 64)
        with pytest.raises(B.FFHipError):
            b.set_signals_ragged([np.zeros(_samples_for(mdl, nblock), dtype=np.float32)])
        b.close()
    sigs = [rng.standard_normal(short).astype(np.float32)] + [rng.standard_normal(_samples_for(mdl, n)).astype(np.float32) for n in RAGGED_BLOCKS]
    _check_batch(B, dm, sigs, temperature, "batch ragged T=%g" % temperature)


@pytest.mark.parametrize("temperature", [1.0, 0.8])
def test_packed_batch_posterior_against_fp64(B, rle128, temperature):
    """the same kernels per READ of a packed batch (several reads to a row, a gap between them)"""
    mdl, dm = rle128
    rng = np.random.default_rng(8)
    lens = [19, 23, 163, 318, 323, 643, 100, 45, 700, 21, 1203, 333]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    rows, cap = 4, 1500
    probe, slot, off, order = _packed(B, dm, rows, cap, sigs)
    probe.close()
    assert len(order) == len(sigs) and max(np.bincount([slot[i] for i in order])) >= 3, "the plan should put several reads in a row"

    def make():
        return _packed(B, dm, rows, cap, sigs)[0]
    _check_batch(B, dm, sigs, temperature, "batch packed T=%g" % temperature, make=make)


@pytest.mark.parametrize("temperature", [1.0, 0.8])
def test_long_read_posterior_against_fp64(B, rle128, temperature):
    """one read of more than 4096 blocks: three traceback chunks of k_viterbi8x<1>, 129 chunks of the chains"""
    mdl, dm = rle128
    sig = np.random.default_rng(9).standard_normal(_samples_for(mdl, 4101)).astype(np.float32)
    _check_batch(B, dm, [sig], temperature, "batch long T=%g" % temperature)


# ---- 4. the generic posterior kernel ----------------------------------------------------------------------------------------------
def _normalised(param, nbase):
    """globally normalised as globalnorm_runlengthV2 hands a matrix over: logZ / nblock subtracted (float64, rounded once)"""
    ns = 2 * nbase
    S = param[:, ns:].astype(np.float64)
    out = param.copy()
    out[:, ns:] = (S - R.crf_logz(S, R.runlength_map(nbase)) / S.shape[0]).astype(np.float32)
    return out


@pytest.mark.parametrize("nbase", [2, 3, 4, 5])
def test_generic_posterior_operator_against_fp64(host, nbase):
    """transpost_crf_runlength (always k_rle_transpost): block counts around the 64-block flush of its vectors"""
    rng = np.random.default_rng(40 + nbase)
    for nblock in (1, 2, 63, 64, 65, 129, 800):
        for style in ("tanh5", "normal", "ties"):
            param = _normalised(_param(rng, nbase, nblock, style), nbase)
            check_posterior(_host_transpost(host, param), param, nbase, "generic op %4d blocks" % nblock, True)


def test_generic_posterior_in_a_batch_at_low_temperature(B, rle128):
    """the engine's posterior beyond kFbRange: k_rle_transpost with several reads and their block counts (tbs)"""
    mdl, dm = rle128
    temperature = 0.09
    assert 10.0 / np.float32(temperature) > K_FB_RANGE          # plan_run's rule: not the fp64 linear-space chains
    rng = np.random.default_rng(10)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (19, 323, 1001)]
    # ... and the engine agrees: a packed batch, which has the linear-space chains only, refuses this temperature
    pb = _packed(B, dm, 2, 1500, sigs)[0]
    with pytest.raises(B.FFHipError):
        pb.run(temperature, 0)
    pb.close()
    _check_batch(B, dm, sigs, temperature, "generic batch T=%g" % temperature, generic=True)


def _planted(rng, nbase, nblock, what):
    """normal scores with -inf planted in the middle block"""
    param = _param(rng, nbase, nblock, "normal")
    ns, t = 2 * nbase, nblock // 2
    idx = lambda base_from, stay_from, base_to: ns + base_to * ns + base_from + (nbase if stay_from else 0)      # noqa: E731  (rle_trans_lookup)
    if what == "first_move":          # the entry the backward chain of a source state visits first: its move to the lowest other base
        param[t, idx(1, False, 0)] = -np.inf          # source: move state of base 1
        param[t, idx(0, True, 1)] = -np.inf           # source: stay state of base 0
    elif what == "stay":
        param[t, idx(2 % nbase, False, 2 % nbase)] = -np.inf
        param[t - 1, idx(1, True, 1)] = -np.inf
    else:
        param[t, ns:] = -np.inf
    return param


@pytest.mark.parametrize("what", ["some_nan", "nan_block", "first_move", "stay", "block"])
@pytest.mark.parametrize("nblock", [9, 65])
@pytest.mark.parametrize("nbase", [4, 5])
def test_generic_posterior_non_finite_scores(host, nbase, nblock, what):
    """NaN and -inf scores: the NaN mask (and every infinity) of k_rle_transpost's result is the oracle's; what is finite on both sides is within
    item 4's bound of fp64"""
    rng = np.random.default_rng(100 * nbase + nblock)
    param = _param(rng, nbase, nblock, what) if what in ("some_nan", "nan_block") else _planted(rng, nbase, nblock, what)
    ns = 2 * nbase
    got, orac = _host_transpost(host, param), _oracle_transpost(param)
    assert np.array_equal(_bits(got[:, :ns]), _bits(param[:, :ns]))
    got, orac = got[:, ns:], orac[:, ns:]
    assert np.array_equal(np.isnan(got), np.isnan(orac)), "NaN masks differ at %s" % (np.argwhere(np.isnan(got) != np.isnan(orac))[:4].tolist(),)
    inf = np.isinf(orac)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], orac[inf])
    both = np.isfinite(got) & np.isfinite(orac)
    if both.any():
        S = param[:, ns:].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            want, alpha, beta = R.runlength_transpost64(S, nbase)
        err = norm_err(got, S, want, alpha, beta)[both]
        oerr = float(norm_err(orac, S, want, alpha, beta)[both].max())
        assert np.all(err <= 2.0 * oerr + 4.0), (float(err.max()), oerr)
