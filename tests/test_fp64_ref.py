"""The float64 references of tests/fp64_ref.py against the oracle's fp32 functions (within fp32 error) and the posterior
against autograd of the partition function: the GPU tests of the convolutions, heads and chains trust these helpers."""
import numpy as np
import pytest
import torch

from flappie_amd import model as M
from oracle import ffo
import fp64_ref as R
from test_oracle_vs_torch import omat, torch_logz


def _oracle_conv(x, cv, swish):
    y = ffo.lib().fo_convolution(ffo.HostMat.from_dense(x).ptr, ffo.HostMat.from_model_mat(cv.W).ptr,
                                 ffo.HostMat.from_model_mat(cv.b).ptr, cv.stride)
    (ffo.lib().fo_swish_inplace if swish else ffo.lib().fo_tanh_inplace)(y)
    return ffo.take(y)


@pytest.mark.parametrize("nf,nfilter,winlen,stride,swish", [(1, 4, 5, 1, True), (4, 16, 5, 1, True), (16, 24, 19, 5, True),
                                                           (1, 16, 19, 2, False), (3, 16, 3, 1, True), (16, 8, 17, 5, True)])
@pytest.mark.parametrize("T", [19, 20, 101, 402, 403])
def test_conv_activation_matches_oracle_within_fp32_error(nf, nfilter, winlen, stride, swish, T):
    rng = np.random.default_rng(T * 7 + winlen)
    cv = M.ConvLayer(M._conv_mat(rng, nf, nfilter, winlen), M.Mat.vector(rng.uniform(-0.1, 0.1, nfilter).astype(np.float32)), stride, nf, winlen)
    cv.W.data *= np.float32(3.0)
    x = (rng.standard_normal((T, nf)) * 2).astype(np.float32)
    got = _oracle_conv(x, cv, swish)
    z, cond = R.conv_terms(x.astype(np.float64), cv.taps(), cv.b.data[0, :nfilter], stride)
    f, df = R.activation(swish)
    want = f(z)
    assert got.shape == want.shape
    # the oracle: winlen * nf products and as many additions in fp32, then the activation (a few ulp)
    bound = 2 * winlen * nf * R.F32_EPS * np.abs(df(z)) * cond + R.act_rounding(want, swish)
    assert (np.abs(got - want) <= bound).all()


def test_conv_terms_marks_every_window_with_a_nan():
    x = np.ones((60, 1))
    x[0, 0] = np.nan
    x[59, 0] = np.inf
    taps = np.ones((2, 19, 1), dtype=np.float32)
    z, _ = R.conv_terms(x, taps, np.zeros(2, dtype=np.float32), 2)
    cols = sorted({c for c, x0 in R.conv_windows(60, 19, 2)[1] if x0 <= 0 < x0 + 19 or x0 <= 59 < x0 + 19})
    assert sorted(np.flatnonzero(~np.isfinite(z[:, 0]))) == cols


@pytest.mark.parametrize("nbase,temperature", [(4, 1.0), (5, 1.0), (4, 0.8), (5, 1.3)])
def test_flipflop_head_matches_oracle(nbase, temperature):
    rng = np.random.default_rng(nbase * 10 + int(temperature * 10))
    H, T, P = 64, 300, 2 * nbase * (nbase + 1)
    h = np.tanh(rng.standard_normal((T, H))).astype(np.float32)
    W = (rng.uniform(-1, 1, (P, H)) * 2 / np.sqrt(H)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, P).astype(np.float32)
    got = ffo.take(ffo.lib().fo_globalnorm_flipflop(omat(h).ptr, omat(W).ptr, omat(b[None, :]).ptr, temperature))
    want, S, z, cond, logz = R.flipflop_head(h, W, b, temperature, nbase)
    assert abs(ffo.lib().fo_partition_function(omat(S).ptr) - logz) <= 1e-9 * abs(logz)
    # fp32: H products and additions, tanh (a few ulp), the scale, then logZ / T (fp32 scores) subtracted
    bound = (5 / temperature) * (2 * H * R.F32_EPS * R.dtanh64(z) * cond + R.act_rounding(np.tanh(z), False)) + 4 * R.ulp32(S) + 2 * R.ulp32(want) + 4 * R.ulp32(logz / T)
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_runlength_head_matches_oracle(temperature):
    rng = np.random.default_rng(5)
    nbase, H, T = 4, 64, 250
    P = 2 * nbase * (nbase + 1)
    h = np.tanh(rng.standard_normal((T, H))).astype(np.float32)
    W = (rng.uniform(-1, 1, (P, H)) * 2 / np.sqrt(H)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, P).astype(np.float32)
    got = ffo.take(ffo.lib().fo_globalnorm_runlengthV2(omat(h).ptr, omat(W).ptr, omat(b[None, :]).ptr, temperature))
    want, z, cond, logz = R.runlength_head(h, W, b, temperature, nbase)
    tr = 5 * np.tanh(z[:, 8:]) / temperature
    assert abs(ffo.lib().fo_runlengthV2_partition_function(omat(np.hstack([want[:, :8], tr])).ptr) - logz) <= 1e-6 * abs(logz)
    lin = 2 * H * R.F32_EPS * cond
    bound = np.empty_like(want)
    bound[:, :8] = lin[:, :8] + 4 * R.ulp32(want[:, :8])           # softplus' <= 1
    bound[:, 8:] = (5 / temperature) * (R.dtanh64(z[:, 8:]) * lin[:, 8:] + R.act_rounding(np.tanh(z[:, 8:]), False)) + 4 * R.ulp32(tr) + 2 * R.ulp32(want[:, 8:]) + 4 * R.ulp32(logz / T)
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("nbase,T", [(4, 60), (5, 33), (4, 1)])
def test_posterior_matches_autograd_and_oracle(nbase, T):
    P = 2 * nbase * (nbase + 1)
    rng = np.random.default_rng(nbase * T + 3)
    s = (rng.standard_normal((T, P)) * 1.5).astype(np.float32)
    S = torch.tensor(s, dtype=torch.float64, requires_grad=True)
    logz = torch_logz(S, nbase)
    logz.backward()
    post, lz = R.crf_posterior(s, R.flipflop_map(nbase))
    assert abs(lz - float(logz.detach())) <= 1e-12 * max(1.0, abs(lz))
    assert abs(R.crf_logz(s.astype(np.float64), R.flipflop_map(nbase)) - lz) <= 1e-12 * max(1.0, abs(lz))
    np.testing.assert_allclose(post, S.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    got = ffo.take(ffo.lib().fo_transpost(omat(s).ptr, 0))           # the oracle's fp32 log-space chains
    np.testing.assert_allclose(got, post, rtol=0, atol=1e-4)


def _enumerate_runlength(param, nbase):
    """tests/test_runlength.py's enumeration over every state path (free start state, cost 0), kept per transition: the log-sum of exp(path score)
    over the paths that take transition p in block t -- what alpha[t][src] + S[t] + beta[t+1][dst] is"""
    import itertools
    from test_runlength import allowed, rle_idx
    T, ns = param.shape[0], 2 * nbase
    S = param[:, ns:].astype(np.float64)
    post = np.full(S.shape, -np.inf)
    for start in range(ns):
        for path in itertools.product(range(ns), repeat=T):
            prev, sc, used = start, 0.0, []
            for t, cur in enumerate(path):
                if not allowed(prev, cur, nbase):
                    break
                p = rle_idx(prev % nbase, prev >= nbase, cur % nbase, nbase)
                sc += S[t, p]
                used.append(p)
                prev = cur
            else:
                for t, p in enumerate(used):
                    post[t, p] = np.logaddexp(post[t, p], sc)
    return post


@pytest.mark.parametrize("nbase,T", [(2, 1), (2, 2), (2, 5), (3, 1), (3, 3), (3, 5)])
def test_runlength_helpers_against_enumeration(nbase, T):
    """runlength_transpost64, runlength_best_path and crf_logz(., runlength_map) against the enumeration over all state paths: 1e-12 relative"""
    from test_runlength import brute_force, random_param
    param = random_param(np.random.default_rng(10 * nbase + T), T, nbase, scale=2.0)
    S = param[:, 2 * nbase:].astype(np.float64)
    logz, best, best_path = brute_force(param, nbase)

    def close(got, want):
        return np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert close(R.crf_logz(S, R.runlength_map(nbase)), logz)
    post, alpha, beta = R.runlength_transpost64(S, nbase)
    assert post.shape == S.shape and alpha.shape == beta.shape == (T + 1, 2 * nbase)
    assert close(post, _enumerate_runlength(param, nbase))
    # the chains' ends: every state starts and ends at log 1; alpha's last and beta's first vector both sum to Z
    assert not alpha[0].any() and not beta[T].any()
    assert close(np.logaddexp.reduce(alpha[T]), logz) and close(np.logaddexp.reduce(beta[0]), logz)
    score, path = R.runlength_best_path(S, nbase)
    assert close(score, best) and tuple(path) == best_path
