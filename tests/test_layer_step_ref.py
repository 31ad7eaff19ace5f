"""The step-local float64 check of the recurrent layers (tests/fp64_ref.py: lstm_step_ref / grumod_step_ref, tests/layer_forced.py), shown
on the CPU to pass what is right and to fail what is wrong before tests/test_layers_fp64_gpu.py applies it to the kernels.

The reference against the oracle and torch:
- forced on the oracle's OWN activations, the oracle's restated step (layer_forced.forced_oracle) returns the oracle's output bit for bit, and
  its normalised error stays under the bound of the fp32 forms (32 K16 + 16, K16 = 2 ceil(H / 16): 528 at H = 128);
- the LSTM's running bound e_c really bounds |c_oracle - c64|: within 4 e_c everywhere (e_c is the allowance for ONE unit of pre-activation error,
  and the oracle's own worst normalised error under forcing, 2.8, says how many it uses: 4 is that figure rounded up to a power of two);
- forced on torch's own float64 trajectory (torch.nn.LSTM; torch.nn.GRU, whose candidate tanh(W_in x + b_in + r (W_hn h)) is GRUmod's with the
  gates permuted), the reference reproduces it within 1e-12.
Measured here (worst over H = 36, 96, 128, five layers, reads of 140 / 150, one and two blocks): the oracle's normalised error under forcing
2.8 (LSTM) and 0.85 (GRUmod) against bounds of 208 ... 528.  e_c / |c_oracle - c64|: 15 ... 19 at the median, 0.4 at the least (the oracle's
cell state uses up to 2.5 units): the running bound holds everywhere and is one order loose at the median.

Mutants.  The split layer kernel is emulated in numpy (two fp16 slices per operand, test_split_numerics.split_f16; per 32-wide K chunk the
products w1 x0, w0 x1, w0 x0 accumulated in fp32 in the scaled space 2^S; fp32 gates) on layer 1 (forward) or 2 (backward) of
synthetic_model(LSTM, 128 | 384), 32 reads of 64 blocks, running free on its own h.  The check then is the GPU test's: worst normalised error
against split_bound(H), and per unit tile the RMS of the normalised error against 1.25 x the larger of the forced fp32 GEMM's and the forced
oracle's.  The clean emulation passes both (worst 0.3 ... 0.7, tile RMS 0.04 ... 0.06 against limits from 0.08).
Every mutant fails, and where it was planted:
                                                              H = 128 (bound 72): worst, tile RMS / limit      H = 384 (bound 168): worst, tile RMS / limit
    (a) w1 x0 dropped in one K chunk of one gate row block     15 (hidden), 2.6 / 0.11                          8.3 (hidden), 1.06 / 0.15
    (b) w0 x1 dropped everywhere                               596, 61 / 0.10                                   564, 52 / 0.15
    (c) h(t-2) for h(t-1), one read tile, one step             3.3e5                                            2.6e5
    (d) gate rows f and g exchanged for one unit tile          1.7e6                                            1.5e6
    (e) bias at 2^(S-1)                                        5.3e4                                            4.2e4
    (f) second slice of h at 2^11                              85, 9.2 / 0.11                                   60 (hidden), 7.7 / 0.15
    (g) backward layer's read moved by one block               1.6e6                                            1.7e6
(a), and (f) at H = 384, stay under the worst-case bound -- 6 per K chunk allows every chunk and every rounding the whole condition -- and are
caught by the RMS relation alone, (a) at its unit tile only; that relation is therefore part of the check, not a report.  (c): the cell state
is not forced, so the steps behind the planted one carry its wrong c until the forget gates have damped it; the first step over the bound is
the planted one.  Not covered: a fault below ~0.15 RMS over a unit tile (e.g. w1 x0 dropped in one chunk for a single unit of H = 384: 1.06 / 4 over its tile
is still seen, the same for one read tile of many is not -- the GPU file's RMS runs over one read of every read tile)."""
import numpy as np
import pytest
import torch

import fp64_ref as R
import layer_forced as LF
from flappie_amd import model as M
from oracle import ffo
from test_split_numerics import split_f16

torch.set_num_threads(1)


# ---- the oracle's stack, layer by layer ------------------------------------------------------------------------------------------
def oracle_front(mdl, sig):
    L = ffo.lib()
    x = np.ascontiguousarray(sig, dtype=np.float32).reshape(-1, 1)
    for cv in mdl.convs:
        y = L.fo_convolution(ffo.HostMat.from_dense(x).ptr, ffo.HostMat.from_model_mat(cv.W).ptr, ffo.HostMat.from_model_mat(cv.b).ptr, cv.stride)
        (L.fo_tanh_inplace if mdl.kind == M.NET_GRUMOD5 else L.fo_swish_inplace)(y)
        x = ffo.take(y)
    return x


def oracle_layers(mdl, x0):
    """[x0, output of layer 0, ..., of layer 4] from the convolutions' output x0 [T, H]"""
    L = ffo.lib()
    acts = [np.ascontiguousarray(x0, dtype=np.float32)]
    for l, r in enumerate(mdl.rnns):
        xa = L.fo_affine_map(ffo.HostMat.from_dense(acts[-1]).ptr, ffo.HostMat.from_model_mat(r.iW).ptr, ffo.HostMat.from_model_mat(r.b).ptr)
        fn = L.fo_grumod if mdl.kind == M.NET_GRUMOD5 else L.fo_lstm
        acts.append(ffo.take(fn(xa, ffo.HostMat.from_model_mat(r.sW).ptr, int(R.layer_backward(l)))))
        L.fo_free_mat(xa)
    return acts


SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(SEEN):
        print("%-40s %s" % (key, SEEN[key]))


@pytest.mark.parametrize("kind", [M.NET_LSTM5, M.NET_GRUMOD5])
@pytest.mark.parametrize("H", [36, 96, 128])
def test_oracle_under_forcing(kind, H):
    mdl = M.synthetic_model(kind, H, seed=20 + H)
    lstm = LF.is_lstm(mdl)
    rng = np.random.default_rng(H)
    x0 = oracle_front(mdl, rng.standard_normal(700 if lstm else 300))
    worst, slack_min, slack_med = 0.0, np.inf, []
    for xs in (x0, x0[:1], x0[:2]):                       # a read of 140 / 150 blocks, of one block, of two
        acts = oracle_layers(mdl, xs)
        for l in range(5):
            iW, sW, b = LF.weights(mdl, l)
            back = R.layer_backward(l)
            r = mdl.rnns[l]
            h, c = LF.forced_oracle(lstm, acts[l], acts[l + 1], r.iW, r.sW, r.b, back)
            assert np.array_equal(h.view(np.uint32), acts[l + 1].view(np.uint32)), "layer %d: the restated step is not the oracle's" % l
            if lstm:
                want, allow, c64, e_c = R.lstm_step_ref(acts[l], acts[l + 1], iW, sW, b, back)
                dc = np.abs(c.astype(np.float64) - c64)
                assert (dc <= 4 * e_c).all(), "layer %d: the running bound does not hold the cell state" % l
                ratio = e_c[dc > 0] / dc[dc > 0]
                slack_min = min(slack_min, float(ratio.min()))
                slack_med.append(float(np.median(ratio)))
            else:
                want, allow = R.grumod_step_ref(acts[l], acts[l + 1], iW, sW, b, back)
            err = LF.norm_err(acts[l + 1], want, allow)
            worst = max(worst, float(err.max()))
            assert err.max() <= LF.f32_bound(H), "layer %d: the oracle at %.2f, above %d" % (l, err.max(), LF.f32_bound(H))
            g, _ = LF.forced_gemm(lstm, acts[l], acts[l + 1], iW, sW, b, back)
            assert LF.norm_err(g, want, allow).max() <= LF.f32_bound(H)
    SEEN["oracle forced %s H=%d" % ("lstm" if lstm else "grumod", H)] = "worst normalised %.2f (bound %d)%s" % (
        worst, LF.f32_bound(H), "  e_c / |c - c64|: min %.1f, median %.1f" % (slack_min, float(np.median(slack_med))) if lstm else "")


@pytest.mark.parametrize("backward", [False, True])
def test_references_equal_torch_in_float64(backward):
    H, T = 24, 40
    torch.manual_seed(7)
    x = torch.randn(T, 1, H, dtype=torch.float64)
    xt = torch.flip(x, [0]) if backward else x
    xn = x[:, 0, :].numpy()
    for lstm in (True, False):
        net = (torch.nn.LSTM if lstm else torch.nn.GRU)(H, H, bias=True).double()
        with torch.no_grad():
            net.bias_hh_l0.zero_()
            out, _ = net(xt)
        h = (torch.flip(out, [0]) if backward else out)[:, 0, :].numpy()
        iW, sW, b = (getattr(net, n).detach().numpy() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0"))
        if lstm:
            want = R.lstm_step_ref(xn, h, iW, sW, b, backward)[0]
        else:                                             # torch's rows are r, z, n; GRUmod's z, r, candidate
            perm = np.r_[H:2 * H, 0:H, 2 * H:3 * H]
            want = R.grumod_step_ref(xn, h, iW[perm], sW[perm], b[perm], backward)[0]
        assert np.abs(want - h).max() <= 1e-12


# ---- the split layer kernel, emulated; mutants -------------------------------------------------------------------------------------
def weight_exp(maxabs):
    """split_weight_exp (ffhip_split.hpp)"""
    return 14 - int(np.floor(np.log2(maxabs)))


def emulate_split_lstm(x, iW, sW, b, backward, first, mut=None):
    """x [N, T, H] -> h [N, T, H] of the split LSTM layer kernel's arithmetic, free running.  mut: (name, parameters) of one planted fault."""
    f32 = np.float32
    N, T, H = x.shape
    name, arg = mut if mut else (None, None)
    ex, eh = (4 if first else 12), 12
    S = min(weight_exp(np.abs(iW).max()) + ex, weight_exp(np.abs(sW).max()) + eh)       # one total exponent for both products
    wi = [np.ascontiguousarray(s.T) for s in split_f16(iW, S - ex)]                      # [H, 4H] per slice
    ws = [np.ascontiguousarray(s.T) for s in split_f16(sW, S - eh)]
    bias = (b.astype(f32) * f32(2.0 ** (S - 1 if name == "bias_half" else S)))
    xs = split_f16(x, ex)
    if name == "shift_read":                              # the layer reads block t + 1 where block t stands (the last block: nothing)
        xs = [np.concatenate([s[:, 1:], np.zeros((N, 1, H), dtype=f32)], axis=1) for s in xs]
    sig = lambda v: f32(1.0) / (f32(1.0) + np.exp(-v))
    h = np.zeros((N, T, H), dtype=f32)
    c = np.zeros((N, H), dtype=f32)
    hprev = np.zeros((N, H), dtype=f32)
    hprev2 = np.zeros((N, H), dtype=f32)
    terms = ((1, 0), (0, 1), (0, 0))                      # slice of w, slice of the operand: smallest first (FFHIP_SPLIT_TERMS_*)
    for i in range(T):
        t = T - 1 - i if backward else i
        hin = hprev
        if name == "stale_h" and i == arg["step"]:
            hin = hprev.copy()
            hin[arg["reads"]] = hprev2[arg["reads"]]
        h0 = (hin * f32(4096.0)).astype(np.float16).astype(f32)
        h1 = (hin * f32(4096.0) - h0).astype(np.float16).astype(f32)
        if name == "slice_scale":
            h1 = h1 * f32(0.5)
        acc = np.tile(bias, (N, 1))
        for w, op in ((wi, (xs[0][:, t], xs[1][:, t])), (ws, (h0, h1))):
            for k0 in range(0, H, 32):
                for sw_, so in terms:
                    if name == "drop_w0x1" and (sw_, so) == (0, 1):
                        continue
                    p = op[so][:, k0:k0 + 32] @ w[sw_][k0:k0 + 32]
                    if name == "drop_w1x0_chunk" and (sw_, so) == (1, 0) and w is ws and k0 == arg["k0"]:
                        p[:, arg["rows"]] = 0.0
                    acc = acc + p
        z = acc * f32(2.0 ** -S)
        if name == "swap_fg":
            u = arg["units"]
            zf = z[:, H:2 * H][:, u].copy()
            z[:, H + u.start:H + u.stop] = z[:, 2 * H + u.start:2 * H + u.stop]
            z[:, 2 * H + u.start:2 * H + u.stop] = zf
        c = sig(z[:, H:2 * H]) * c + sig(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
        hprev2 = hprev
        hprev = (sig(z[:, 3 * H:]) * np.tanh(c)).astype(f32)
        h[:, t] = hprev
    return h


def verdict(mdl, l, x, h, oracle_reads=(0, 17)):
    """the GPU test's check of one layer: [(what, value, limit, where)] of every failure; plus the figures"""
    H = mdl.hidden
    iW, sW, b = LF.weights(mdl, l)
    back = R.layer_backward(l)
    fx, fh = LF.split_floors(l, True)
    want, allow = R.layer_step_ref(True, x, h, iW, sW, b, back, fx, fh)
    err = LF.norm_err(h, want, allow)
    fails = []
    worst, where = LF.locate(err)
    if worst > LF.split_bound(H):
        fails.append(("worst", worst, LF.split_bound(H), where))
    rms = LF.tile_rms(err)
    gem = np.stack([LF.forced_gemm(True, x[n], h[n], iW, sW, b, back)[0] for n in range(x.shape[0])])
    r = mdl.rnns[l]
    sel = list(oracle_reads)
    orc = np.stack([LF.forced_oracle(True, x[n], h[n], r.iW, r.sW, r.b, back)[0] for n in sel])
    limit = 1.25 * np.maximum(LF.tile_rms(LF.norm_err(gem, want, allow)), LF.tile_rms(LF.norm_err(orc, want[sel], allow[sel])))
    for u in np.flatnonzero(rms > limit):
        fails.append(("rms", float(rms[u]), float(limit[u]), int(u)))
    return fails, dict(worst=worst, where=where, rms=rms, limit=limit)


_SETUP = {}


def setup(H):
    if H not in _SETUP:
        mdl = M.synthetic_model(M.NET_LSTM5, H, seed=H)
        rng = np.random.default_rng(H + 1)
        acts = [oracle_layers(mdl, oracle_front(mdl, rng.standard_normal(320)))[:3] for _ in range(32)]       # 64 blocks a read
        _SETUP[H] = (mdl, [np.stack([a[k] for a in acts]) for k in range(3)])
    return _SETUP[H]


def emulate(H, l, mut=None):
    mdl, xs = setup(H)
    iW, sW, b = LF.weights(mdl, l)
    return mdl, xs[l], emulate_split_lstm(xs[l], iW, sW, b, R.layer_backward(l), l == 0, mut)


@pytest.mark.parametrize("H", [128, 384])
@pytest.mark.parametrize("l", [1, 2])
def test_clean_emulation_passes(H, l):
    mdl, x, h = emulate(H, l)
    fails, fig = verdict(mdl, l, x, h)
    SEEN["clean H=%d layer %d" % (H, l)] = "worst %.2f (bound %d), tile RMS %.2f .. %.2f (limits from %.2f)" % (
        fig["worst"], LF.split_bound(H), fig["rms"].min(), fig["rms"].max(), fig["limit"].min())
    assert not fails, fails


MUTANTS = {
    # name: (layer, fault, (read tile, step in time order, unit tile) it must be found at; None = anywhere in that coordinate)
    "a_w1x0_one_chunk": (1, lambda H: ("drop_w1x0_chunk", dict(k0=64, rows=slice(H + 32, H + 48))), (None, None, 2)),
    "b_w0x1_everywhere": (1, lambda H: ("drop_w0x1", None), (None, None, None)),
    "c_stale_h": (1, lambda H: ("stale_h", dict(step=40, reads=slice(16, 32))), (1, 40, None)),
    "d_swap_f_g": (1, lambda H: ("swap_fg", dict(units=slice(48, 64))), (None, None, 3)),
    "e_bias_half": (1, lambda H: ("bias_half", None), (None, None, None)),
    "f_slice_scale": (1, lambda H: ("slice_scale", None), (None, None, None)),
    "g_shift_read": (2, lambda H: ("shift_read", None), (None, None, None)),
}


@pytest.mark.parametrize("H", [128, 384])
@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_fails_where_it_was_planted(H, name):
    l, make, (rt, step, ut) = MUTANTS[name]
    mdl, x, h = emulate(H, l, make(H))
    fails, fig = verdict(mdl, l, x, h)
    SEEN["mutant %s H=%d" % (name, H)] = "worst %.3g at %s (bound %d), tile RMS max %.3g (limit %.2f)" % (
        fig["worst"], fig["where"], LF.split_bound(H), fig["rms"].max(), fig["limit"][int(np.argmax(fig["rms"]))])
    assert fails, "the check does not see mutant %s" % name
    n, t, u = fig["where"]
    by_worst = any(f[0] == "worst" for f in fails)
    if rt is not None:
        assert by_worst and n // 16 == rt
    if step is not None:
        assert by_worst and t >= step
    if ut is not None:
        tiles = {f[3] for f in fails if f[0] == "rms"} | ({u // 16} if by_worst else set())
        assert tiles == {ut}, "found at unit tiles %s, planted at %d" % (sorted(tiles), ut)
    if name == "c_stale_h":
        # one step of one read tile.  The cell state is not forced (it cannot be read), so the wrong c(40) stays in c(41), c(42), ... until the
        # forget gates have damped it: the FIRST step over the bound is the planted one, and no other read tile is touched
        want, allow = R.layer_step_ref(True, x, h, *LF.weights(mdl, l), R.layer_backward(l), *LF.split_floors(l, True))
        over = np.argwhere(LF.norm_err(h, want, allow) > LF.split_bound(H))
        assert over[:, 1].min() == 40 and set(over[:, 0] // 16) == {1}
