"""Every recurrent layer kernel a run can take, held step by step to float64 on the kernel's OWN input (tests/fp64_ref.py lstm_step_ref /
grumod_step_ref).  FFHIP_RUN_KEEP_ACTS keeps the convolutions' output and every layer's, as the kernels wrote them; for layer l of a read,
x = activation(l - 1), h = activation(l), and every step t is recomputed in float64 from x(t) and the kernel's own h(t-1) ("teacher forced").
The state is forced every step, so no error feeds back through the matrix products and a check does not absorb the error of the steps or
layers before it: a dropped split product in one K chunk, a weight tile in the wrong gate row block, a stale h(t-1) in one read tile at one
step, a bias at the wrong power of two or a read moved by one block each show at the (layer, step, unit, read) where they happen
(tests/test_layer_step_ref.py plants each of them in an emulation of the split kernel and requires this check to find it).  The LSTM's cell
state cannot be read out; the reference carries it in float64 from the gates of the kernel's h, with a running first-order bound on the
kernel's own cell error (e_c, lstm_step_ref), which enters the allowance.

Error metric, per element:  |h_kernel(t) - h64(t)| / allowance(t), where the allowance is what ONE unit of pre-activation error -- cond 2^-24
with cond = |iW||x(t)| + |sW||h(t-1)| + |b|, + 2^-37 sum|sW| and, for the first LSTM layer, 2^-29 sum|iW| where the operand travels in the
split format -- costs at the output through the gates' derivatives, plus the gate phase's own fp32 roundings (4 ulp a logistic, 4 ulp +
4 x 2^-24 a tanh: the reference's own error, which level 2 of the split kernels stays within, tests/test_gate_math_gpu.py).

Bounds in those units, from the formats and the kernels' summation order (not fitted; written before the first GPU run):
    split forms (k_lstm_split and its dense form, k_inproj_split + k_rnn_split): K = 2 H in chunks of 32, per chunk three
        v_mfma_f32_16x16x32_f16 of exact products into an fp32 accumulator
        4 (weight slices hold w to 2^-22) + 4 (the slices of x and h hold the fp32 copy this test reads to 2^-22) + 8 (dropped w1 x1 <= 2^-21
        of a product) + 8 (bias, the K split over waves and its partial sums) + 6 per chunk = 24 + 6 (2 H / 32)            [layer_forced.split_bound]
    fp32 forms (k_lstm_fused, k_rnn_persist behind k_inproj or k_inproj_split, k_lstm_step / k_gru_step): every product runs on
        v_mfma_f32_16x16x4_f32 (ffhip_kernels.hip, ffhip_rnn_persist.hip: no sequential VALU sum anywhere), four per 16-wide K chunk, so the
        f32 MFMA convolution's 32 K16 + 16 with K16 = 2 ceil(H / 16) -- which also covers the forms whose projection runs on split operands
        (its 24 + 6 H / 32 is less than the 32 H / 16 the f32 projection is allowed)                                       [layer_forced.f32_bound]
The same metric applied to the fp32 oracle's arithmetic and to a plain fp32 numpy GEMM on the kernel's x with the kernel's h forced the same
way (layer_forced.forced_oracle / forced_gemm) must lie under the fp32 forms' bound on every case; kernel / oracle worst are printed per case
and layer (-s).  The worst-case bounds are loose (every rounding is allowed the whole condition), so beside them EVERY form, at both gate levels,
must keep the relation tests/test_split_numerics.py fixes for the split products (the fp32 forms are an fp32 GEMM themselves): per unit tile of
16 units, the RMS of the normalised error over the sampled reads and steps at most 1.25 x the larger of the fp32 GEMM's and the oracle's.
Not covered by that relation: a fault of fp16-only size in one K chunk confined to ONE read tile -- the RMS runs over one read of every read
tile, so it is diluted by the square root of the number of read tiles (16 ... 33 here) and shows only if it passes the worst-case bound.

Cases: the PATHS table of tests/gate_probe.py with real weights (M.synthetic_model: input driven, non-chaotic) -- rnn_path 0 (k_lstm_step,
k_gru_step), 1 (k_rnn_persist behind k_inproj or k_inproj_split), 2 (k_lstm_fused, LSTM and GRUmod, H = 36 padded to 48, 64, 96, 128, 256,
384), 3 (k_lstm_split one-tile and dense forms, LSTM 128 ... 512, GRUmod 128 ... 384), 4 (k_inproj_split + k_rnn_split) -- at full launches of
256 ... 520 ragged reads of four lengths, at the default gate level and, where the kernel follows the level, FFHIP_RUN_EXACT_GATES; and a batch
of the shapes of test_split_kernel_ragged_and_empty_slots (block counts unequal inside a tile pair, the shortest legal read, a tile of empty
slots).  No read of ONE block exists on the device (the shortest legal read is one window of the last convolution: 4 blocks); the reference's
one-block case is in tests/test_layer_step_ref.py.
Sample rule: all five layers and every step of reads 0 and nread - 1, of read 16 k + (5 k + 3) mod 16 of every read tile k, and of the first
read of every distinct length; the oracle's arithmetic (sequential, slow) on the first sampled read of the shortest length and, below H = 256,
of the longest.  Every sampled read is zero beyond its end in every layer.

The forms that keep no activations -- k_lstm_split_pair (two batches in one launch), k_lstm_pack, k_grumod_pack -- stay tied to the checked
forms bit for bit: test_gate_levels_gpu.py::test_lean_only_forms_follow_the_level, test_split_gpu.py::test_dense_launch_matches_the_one_tile_launches
and test_paired_layer_launches_*, and here test_lean_forms_head_input_bit_identical: at real weights the whole of the last layer's h as the
head reads it (Batch.head_input, 22 bits a value) equals that of the one-tile launches (FFHIP_DEBUG=no_dense,no_pair).  (The library reports
no name of the layer kernel a launch took: that 1040 reads at H = 256 take the packed forms and a paired run k_lstm_split_pair rests on the
dispatch, as in the tests named above; Batch.paired() is asserted.)  activation(4) and head_input: in a kept run the head reads the fp32 copy
(no split head), so head_input IS activation(4) -- asserted in test_ragged_edges_against_fp64, a check of the read-outs, not of a rounding.
Across runs (a default run's head_input against a kept run's activation(4) rounded to two slices) the two are not tied: the kept run's last
convolution writes fp32 and a converter makes the first layer's slices, the default run's writes them from its epilogue, and reading the two did
not establish that the stack's INPUT has the same bits in both.

Records of the first MI355X run: worst normalised error kernel / fp32 oracle / fp32 GEMM (bound), and the largest tile RMS of the kernel /
of the larger fp32 evaluation; worst over the five layers and the gate levels of a case.  36 tests, 50 s (test_front_head_fp64_gpu.py: the same range).
    split_lstm128   k_lstm_split            1.43 / 6.29 / 3.29  (72)     0.131 / 0.232      split_grumod128  k_lstm_split<GRUmod>     0.52 / 0.66 / 0.99  (72)    0.086 / 0.108
    split_lstm256   k_lstm_split            1.22 / 4.58 / 3.36  (120)    0.101 / 0.202      split_grumod256                           0.49 / 0.94 / 1.32  (120)   0.078 / 0.119
    split_lstm384   dense form              1.46 / 6.02 / 4.17  (168)    0.112 / 0.201      split_grumod384                           0.48 / 1.10 / 1.20  (168)   0.078 / 0.132
    split_lstm512   k_lstm_split<0, 4, 2>   1.48 / 4.11 / 2.62  (216)    0.112 / 0.230      unfused_lstm256  k_inproj_split + k_rnn_split  1.97 / 3.96 / 3.27  (120)  0.124 / 0.258
    f32_lstm128     k_lstm_fused            2.53 / 4.85 / 3.46  (528)    0.164 / 0.229      f32_grumod256    k_lstm_fused<GRUmod>     0.68 / 0.90 / 1.09  (1040)  0.087 / 0.123
    f32_lstm384     k_lstm_fused            2.41 / 7.27 / 5.25  (1552)   0.153 / 0.210      small_grumod64   k_lstm_fused<GRUmod>     0.47 / 0.58 / 0.68  (272)   0.088 / 0.099
    small_lstm36 / 64 / 96  k_lstm_fused    1.70, 2.61, 2.03 / 2.19, 3.40, 3.69 / 1.76, 2.61, 2.46  (208, 272, 400)
    f32_unfused_lstm128    k_inproj + k_rnn_persist           3.72 / 5.80 / 3.47  (528)     f32_unfused_grumod128  k_inproj + k_rnn_persist  0.94 / 0.72 / 1.08  (528)
    unfused_grumod128      k_inproj_split + k_rnn_persist     0.73 / 0.70 / 1.00  (528)
    stepwise_lstm128       k_inproj_split + k_lstm_step       5.01 / 6.31 / 3.33  (528)     stepwise_grumod128     k_inproj_split + k_gru_step  0.72 / 0.69 / 1.00  (528)
    ragged edges: split LSTM 1.40 / 3.58 / 2.59 (72), split GRUmod 0.46 / 0.83 / 0.82 (72), k_lstm_fused 1.55 / 3.58 / 3.23 (528), k_lstm_step 4.27 / 3.35 / 2.58 (528)
    NaN sample: split 1.12 / 3.16 / 2.23 (72), k_lstm_fused 1.56 / 3.22 / 1.94 (528)
Every kernel sits at or below the reference's own arithmetic on the same inputs (the LSTM's first layer is the worst everywhere: its x is the
unbounded swish output).  The worst-case bounds are one to two orders above what any correct form needs -- they allow every rounding the whole
condition -- so it is the tile RMS relation (kernel 0.05 ... 0.25 against limits of 0.08 ... 0.69) that a fault of fp16-only size in one place
has to pass; the bounds catch what is wrong by more than a few 2^-12 of a product, or wrong in one place by a whole term.  Nothing was found."""
import time

import numpy as np
import pytest

import fp64_ref as R
import gate_probe as GP
import layer_forced as LF
from flappie_amd import model as M

pytestmark = pytest.mark.gpu

CASES = dict(GP.PATHS)
CASES["split_grumod384"] = (M.NET_GRUMOD5, 384, 0, 256, 3, True)
CASES["f32_unfused_grumod128"] = (M.NET_GRUMOD5, 128, "F32|UNFUSED", 256, 1, False)      # k_inproj + k_rnn_persist<GRUmod>
RUNS = [(c, s) for c in CASES for s in (("default", "exact") if CASES[c][5] else ("default",))]


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    for key in sorted(SEEN):
        print("worst normalised error %-36s %s" % (key, SEEN[key]))
    print("tests/test_layers_fp64_gpu.py: %.0f s" % (time.time() - t0))


def sample_reads(lens):
    """the module docstring's sample rule; empty slots (length 0) are never sampled"""
    nread = len(lens)
    s = {0, nread - 1}
    for k in range(-(-nread // 16)):
        s.add(min(nread - 1, 16 * k + (5 * k + 3) % 16))
    for n in sorted(set(lens)):
        s.add(lens.index(n))
    return sorted(r for r in s if lens[r] > 0)


def check_layers(b, mdl, lens, sample, path, f32_flag, key):
    """the sampled reads' five layers against float64; asserts the bounds, notes the worst"""
    lstm = LF.is_lstm(mdl)
    H = mdl.hidden
    split = path in (3, 4)
    bound = LF.split_bound(H) if split else LF.f32_bound(H)
    acts = {r: [b.activation(l, r) for l in range(-1, 5)] for r in sample}
    nbs = {r: mdl.nblock(lens[r]) for r in sample}
    for r in sample:
        assert b.read_nblock(r) == nbs[r]
        for l in range(1, 6):
            assert not acts[r][l][nbs[r]:].any(), "%s layer %d read %d: output beyond the read's end" % (key, l - 1, r)
    shortest, longest = min(nbs.values()), max(nbs.values())
    orc_reads = [next(r for r in sample if nbs[r] == shortest)] + ([next(r for r in sample if nbs[r] == longest)] if H < 256 and longest != shortest else [])
    for l in range(5):
        iW, sW, bias = LF.weights(mdl, l)
        rn = mdl.rnns[l]
        back = R.layer_backward(l)
        fx, fh = LF.split_floors(l, lstm)
        if f32_flag or path == 2:
            fx = 0.0                                       # the projection reads fp32
        if not split:
            fh = 0.0                                       # the recurrence reads fp32
        kern, gemm, orac, worst = [], [], [], (0.0, None)
        for nb in sorted(set(nbs.values())):
            rs = [r for r in sample if nbs[r] == nb]
            x = np.stack([acts[r][l][:nb] for r in rs])
            h = np.stack([acts[r][l + 1][:nb] for r in rs])
            assert np.isfinite(h).all(), "%s layer %d: a non-finite output" % (key, l)
            want, allow = R.layer_step_ref(lstm, x, h, iW, sW, bias, back, fx, fh)
            err = LF.norm_err(h, want, allow)
            kern.append(err.reshape(-1, H))
            w, (n, t, u) = LF.locate(err)
            if w > worst[0]:
                worst = (w, (rs[n], t, u))
            for n, r in enumerate(rs):
                g, _ = LF.forced_gemm(lstm, x[n], h[n], iW, sW, bias, back)
                gemm.append(LF.norm_err(g, want[n], allow[n]))
                if r in orc_reads:
                    o, _ = LF.forced_oracle(lstm, x[n], h[n], rn.iW, rn.sW, rn.b, back)
                    orac.append(LF.norm_err(o, want[n], allow[n]))
        kern, gemm, orac = np.concatenate(kern), np.concatenate(gemm), np.concatenate(orac)
        rk, rg, ro = LF.tile_rms(kern), LF.tile_rms(gemm), LF.tile_rms(orac)
        limit = 1.25 * np.maximum(rg, ro)
        k = int(np.argmax(rk / limit))
        SEEN["%s layer %d" % (key, l)] = "kernel %7.3f  fp32 oracle %7.3f  fp32 GEMM %7.3f  (bound %d)   tile RMS kernel %.3f oracle %.3f GEMM %.3f (limit %.3f)" % (
            worst[0], orac.max(), gemm.max(), bound, rk[k], ro[k], rg[k], limit[k])
        assert orac.max() <= LF.f32_bound(H) and gemm.max() <= LF.f32_bound(H), "%s layer %d: an fp32 evaluation above the fp32 forms' bound" % (key, l)
        assert worst[0] <= bound, "%s layer %d: worst normalised error %.2f above the format's bound %d at (read, block, unit) %s, read tile %d, unit tile %d" % (
            key, l, worst[0], bound, worst[1], worst[1][0] // 16, worst[1][2] // 16)
        assert (rk <= limit).all(), "%s layer %d: RMS of the normalised error %.3f above %.3f at unit tile %d" % (key, l, rk[k], limit[k], k)


def run_case(B, engine, mdl, sigs, flags, nslot=None):
    dm = B.DeviceModel(engine, mdl)
    b = B.Batch(dm, nslot or len(sigs), max(max(x.size for x in sigs), 1))
    b.set_signals_ragged(sigs)
    b.run(1.0, flags | B.RUN_KEEP_ACTS)
    b.finish()
    return dm, b


@pytest.mark.parametrize("case,switch", RUNS, ids=["%s-%s" % c for c in RUNS])
def test_layer_kernel_steps_against_fp64(B, engine, monkeypatch, case, switch):
    kind, H, path_flags, nread, want_path, _ = CASES[case]
    monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    monkeypatch.delenv("FFHIP_DEBUG", raising=False)
    mdl = M.synthetic_model(kind, H, seed=11 + H)
    lens = GP.read_lengths(kind, nread)
    rng = np.random.default_rng(H + nread)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    flags = GP.run_flags(B, path_flags) | (B.RUN_EXACT_GATES if switch == "exact" else 0)
    dm, b = run_case(B, engine, mdl, sigs, flags)
    try:
        assert b.rnn_path() == want_path, "%s took path %d" % (case, b.rnn_path())
        assert b.f32_reruns() == 0
        check_layers(b, mdl, lens, sample_reads(lens), want_path, bool(flags & B.RUN_F32_RNN), "%s %s" % (case, switch))
    finally:
        b.close(); dm.close()


@pytest.mark.parametrize("kind,flag,want_path", [(M.NET_LSTM5, 0, 3), (M.NET_GRUMOD5, 0, 3), (M.NET_LSTM5, "F32", 2), (M.NET_LSTM5, "STEPWISE", 0)])
def test_ragged_edges_against_fp64(B, engine, monkeypatch, kind, flag, want_path):
    """EVERY read of a batch whose block counts differ inside a tile pair, with the shortest legal read, reads one sample apart and a tile of
    empty slots (the shapes of test_split_gpu.py::test_split_kernel_ragged_and_empty_slots)"""
    monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    monkeypatch.delenv("FFHIP_DEBUG", raising=False)
    mdl = M.synthetic_model(kind, 128, seed=11)
    short = 19                                             # one window of the last convolution (winlen 19) in either network
    lens = [1200, 1199, 600, 601, 37, short, 1000, 800, 801, 802, 803, 804, 805, 806, 807, 808, 300, 1200, 45]
    rng = np.random.default_rng(5)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    lens = lens + [0] * (40 - len(lens))                   # slots 19 .. 39 stay empty: tile 2 is all empty
    dm, b = run_case(B, engine, mdl, sigs + [np.zeros(0, dtype=np.float32)] * (40 - len(sigs)), GP.run_flags(B, flag))
    try:
        assert b.rnn_path() == want_path and b.f32_reruns() == 0
        check_layers(b, mdl, lens, [r for r in range(40) if lens[r]], want_path, flag == "F32",
                     "ragged %s %s" % ("lstm" if kind == M.NET_LSTM5 else "grumod", flag or "split"))
        for r in (0, 5, 18):                               # a kept run's head reads the fp32 copy of the last layer: the two read-outs are one buffer
            assert np.array_equal(b.head_input(r).view(np.uint32), b.activation(4, r)[:mdl.nblock(lens[r])].view(np.uint32))
    finally:
        b.close(); dm.close()


@pytest.mark.parametrize("flag,want_path", [(0, 3), ("F32", 2)])
def test_nan_and_inf_in_the_input(B, engine, monkeypatch, flag, want_path):
    """A NaN sample makes the blocks of the swish convolutions' output that see it NaN.  In the reference every pre-activation of those steps
    of the first layer is then NaN, every gate takes its clamped value (logistic 4.156e-39, tanh -1: tests/test_gate_math_gpu.py
    test_nan_pre_activation_gives_a_finite_gate) and the layer's output stays finite: lstm_step_ref does the same, so the non-finite set of
    every layer's output is the reference's -- empty -- and the values are held to the metric like any other, in the NaN's read and its neighbours.
    On the f32 path (no clamp of the split format, which would send the read round again) another read carries +inf and -inf samples: a
    pre-activation is then +-inf where every infinite product has one sign (logistic 1 or 4.156e-39, tanh +-1) and NaN where both occur, in
    any summation order."""
    monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    monkeypatch.delenv("FFHIP_DEBUG", raising=False)
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=11)
    rng = np.random.default_rng(8)
    lens = [1000] * 16
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    sigs[5][500] = np.nan
    if flag == "F32":
        sigs[9][300], sigs[9][700] = np.inf, -np.inf
    dm, b = run_case(B, engine, mdl, sigs, GP.run_flags(B, flag))
    try:
        assert b.rnn_path() == want_path and b.f32_reruns() == 0
        assert np.isnan(b.activation(-1, 5)).any() and np.isfinite(b.activation(-1, 4)).all()
        if flag == "F32":
            assert not np.isfinite(b.activation(-1, 9)).all()
        check_layers(b, mdl, lens, [0, 4, 5, 6, 8, 9, 10, 15], want_path, flag == "F32", "nan %s" % (flag or "split"))
    finally:
        b.close(); dm.close()


def _head_inputs(B, dm, sigs, flags, pair):
    bs = []
    for k in range(2 if pair else 1):
        b = B.Batch(dm, len(sigs[k]), max(x.size for x in sigs[k]))
        b.set_signals_ragged(sigs[k])
        bs.append(b)
    if pair:
        bs[0].run_pair(bs[1], 1.0, flags)
        assert bs[0].paired()
    else:
        bs[0].run(1.0, flags)
    out = []
    for b in bs:
        b.finish()
        assert b.rnn_path() == 3 and b.f32_reruns() == 0
        out.append([b.head_input(r) for r in range(len(b._place))])
        b.close()
    return out


@pytest.mark.parametrize("form", ["pair_lstm384", "pack_lstm256", "pack_grumod256"])
def test_lean_forms_head_input_bit_identical(B, engine, monkeypatch, form):
    """k_lstm_split_pair, k_lstm_pack and k_grumod_pack keep no activations.  On the default path Batch.head_input is the stack's own output as
    the head reads it: at real weights it equals, bit for bit and for every read, that of the same reads through the one-tile launches
    (FFHIP_DEBUG=no_dense,no_pair), which the cases above hold to float64."""
    kind, H, nread = {"pair_lstm384": (M.NET_LSTM5, 384, 256), "pack_lstm256": (M.NET_LSTM5, 256, 1040), "pack_grumod256": (M.NET_GRUMOD5, 256, 1040)}[form]
    pair = form.startswith("pair")
    monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    mdl = M.synthetic_model(kind, H, seed=40 + H)
    rng = np.random.default_rng(3)
    sigs = [[rng.standard_normal(n).astype(np.float32) for n in GP.read_lengths(kind, nread)] for _ in range(2 if pair else 1)]
    dm = B.DeviceModel(engine, mdl)
    try:
        monkeypatch.delenv("FFHIP_DEBUG", raising=False)
        lean = _head_inputs(B, dm, sigs, 0, pair)
        monkeypatch.setenv("FFHIP_DEBUG", "no_dense,no_pair")
        plain = _head_inputs(B, dm, sigs, 0, False) + (_head_inputs(B, dm, sigs[1:], 0, False) if pair else [])
    finally:
        dm.close()
    for k in range(len(lean)):
        for r in range(nread):
            assert lean[k][r].shape == (mdl.nblock(sigs[k][r].size), H) and np.abs(lean[k][r]).max() > 0.01
            ok = GP.same_bits(lean[k][r], plain[k][r])
            assert ok.all(), "%s batch %d read %d: %d values of the head's input differ" % (form, k, r, (~ok).sum())
