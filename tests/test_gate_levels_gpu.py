"""Gate math inside every layer kernel, through probe models (tests/gate_probe.py): every iW and sW of the recurrent layers zero, biases
drawn per unit from moderate, tiny, near-clamp, infinite and NaN values.  A gate's pre-activation is then its bias, exactly, in every kernel
and at every step, so a layer's output is a function of the gate arithmetic alone -- and the end-to-end tolerance of the parity tests
(|dtrans| 5e-5), which a kernel running the wrong gate level stays inside, does not enter.

The contract (include/ffhip.h):
- gate level 0 (FFHIP_RUN_EXACT_GATES, FFHIP_FAST_GATES=0) on every kernel, and every level on the kernels that always replay the reference's
  exp_ps (k_rnn_split, k_lstm_fused, k_rnn_persist, the launch-per-step kernels): activations bit-identical to the oracle, every step, every read;
- level 2 -- the default, FFHIP_RUN_FAST_GATES2, FFHIP_RUN_FAST_GATES and FFHIP_FAST_GATES=1|2 (level 1 runs as level 2) -- on the split
  fused-projection forms (k_lstm_split, its pair and dense forms, k_lstm_pack, k_grumod_pack): activations bit-identical to the host composition
  of the device's logistic_hw / tanh_hw (ffhip_debug_gate_math) in the kernels' operation order, for the first steps of every read;
- a run flag beats FFHIP_FAST_GATES; a value of FFHIP_FAST_GATES other than 0, 1, 2 gives the default.
Batches are full (256-1040 reads, ragged, four distinct lengths), so every lane, wave and read tile of a launch takes part."""
import numpy as np
import pytest

from flappie_amd import model as M

import gate_probe as GP

pytestmark = pytest.mark.gpu

KSTEPS = 8          # steps of each read composed on the host at level 2


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


PATHS = GP.PATHS          # (kind, H, run flags, reads, rnn path, whether the kernel follows the gate level): shared with tests/test_layers_fp64_gpu.py

# (run flags, FFHIP_FAST_GATES, the level that must result)
SWITCHES = {
    "default": (0, None, 2),
    "exact": ("EXACT", None, 0),
    "fast": ("FAST", None, 2),                # level 1 runs as level 2
    "fast2": ("FAST2", None, 2),
    "env0": (0, "0", 0),
    "env1": (0, "1", 2),
    "env2": (0, "2", 2),
    "env_off": (0, "off", 2),                 # not 0, 1 or 2: reported, the default
    "exact_over_env2": ("EXACT", "2", 0),
    "fast2_over_env0": ("FAST2", "0", 2),
}
FULL_MATRIX = ("split_lstm128", "split_grumod128", "f32_lstm128", "small_lstm64")


_flags = GP.run_flags
_lengths = GP.read_lengths


_CACHE = {}


def _setup(name):
    """the probe model, its reads and the oracle's layer outputs per distinct length (once per path)"""
    if name in _CACHE:
        return _CACHE[name]
    kind, H = PATHS[name][:2]
    mdl = GP.probe_model(kind, H, seed=11 + H)
    lens = _lengths(kind, PATHS[name][3])
    rng = np.random.default_rng(H)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    oracle = {}
    for n in sorted(set(lens)):
        nb = mdl.nblock(n)
        oracle[nb] = [GP.oracle_layer(mdl, l, nb) for l in range(5)]
    _CACHE[name] = (mdl, sigs, oracle)
    return _CACHE[name]


def _composed(engine, mdl):
    """[layer] -> [KSTEPS, H] outputs of the first steps at level 2, from the device's gate forms"""
    sig = lambda v: engine.gate_math("logistic_hw2", v)
    tanh = lambda v: engine.gate_math("tanh_hw2", v)
    return [GP.compose(mdl.kind, GP.layer_bias(mdl, l), KSTEPS, sig, tanh) for l in range(5)]


def _run(B, engine, name, flags_spec, env, monkeypatch):
    kind, H, path_flags, nread, want_path, _ = PATHS[name]
    mdl, sigs, _ = _setup(name)
    if env is None:
        monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    else:
        monkeypatch.setenv("FFHIP_FAST_GATES", env)
    dm = B.DeviceModel(engine, mdl)
    b = B.Batch(dm, nread, max(x.size for x in sigs))
    b.set_signals_ragged(sigs)
    b.run(1.0, _flags(B, path_flags) | _flags(B, flags_spec) | B.RUN_KEEP_ACTS)
    b.finish()
    assert b.rnn_path() == want_path, "%s took path %d" % (name, b.rnn_path())
    assert b.f32_reruns() == 0
    acts = [[b.activation(l, r) for r in range(nread)] for l in range(5)]
    b.close()
    dm.close()
    return acts


def _check(engine, name, acts, level):
    kind, H, _, nread, _, follows = PATHS[name]
    mdl, sigs, oracle = _setup(name)
    hw = follows and level != 0
    comp = _composed(engine, mdl) if hw else None
    for l in range(5):
        for r in range(nread):
            nb = mdl.nblock(sigs[r].size)
            a = acts[l][r]
            assert not a[nb:].any(), "%s layer %d read %d: output beyond the read's end" % (name, l, r)
            if not hw:
                ok = GP.same_bits(a[:nb], oracle[nb][l])
                assert ok.all(), "%s layer %d read %d: %d of %d values differ from the oracle, first (step, unit) %s" % (
                    name, l, r, (~ok).sum(), ok.size, np.argwhere(~ok)[:3].tolist())
            else:
                steps = a[:KSTEPS] if l % 2 else a[nb - 1::-1][:KSTEPS]
                ok = GP.same_bits(steps, comp[l])
                assert ok.all(), "%s layer %d read %d: %d of %d values differ from the composed level-2 gates, first (step, unit) %s" % (
                    name, l, r, (~ok).sum(), ok.size, np.argwhere(~ok)[:3].tolist())


CASES = [(p, s) for p in PATHS for s in (SWITCHES if p in FULL_MATRIX else ("default", "exact", "env0"))]


@pytest.mark.parametrize("path,switch", CASES, ids=["%s-%s" % c for c in CASES])
def test_layer_kernel_gate_level(B, engine, monkeypatch, path, switch):
    flags_spec, env, level = SWITCHES[switch]
    acts = _run(B, engine, path, flags_spec, env, monkeypatch)
    _check(engine, path, acts, level)


@pytest.mark.parametrize("kind", [M.NET_LSTM5, M.NET_GRUMOD5])
def test_probe_tells_the_levels_apart(B, engine, kind):
    """the probe biases give level-2 outputs that differ from the exact replay's, so the tests above can tell the levels apart"""
    mdl = GP.probe_model(kind, 128, seed=11 + 128)
    comp = _composed(engine, mdl)
    exact = [GP.compose(kind, GP.layer_bias(mdl, l), KSTEPS, GP.oracle_map(2), GP.oracle_map(3)) for l in range(5)]
    assert any((~GP.same_bits(c, e)).any() for c, e in zip(comp, exact))


def _transitions(B, dm, sigs, nread, flags, pair=False):
    bs = []
    for k in range(2 if pair else 1):
        b = B.Batch(dm, nread, max(x.size for x in sigs[k]))
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
        out.append([b.transitions(r) for r in range(nread)])
        b.close()
    return out


@pytest.mark.parametrize("form", ["pair_lstm384", "pack_lstm256", "pack_grumod256"])
@pytest.mark.parametrize("switch", ["default", "exact"])
def test_lean_only_forms_follow_the_level(B, engine, monkeypatch, form, switch):
    """the paired launch (k_lstm_split_pair) and the packed forms (k_lstm_pack / k_grumod_pack) keep no activations: their transition
    scores must equal, bit for bit, those of the same reads with FFHIP_DEBUG=no_dense,no_pair (the one-tile split kernel, held to the gate
    level above) at the same level.  This route sees the last layer's h only through the split head, which reads 22 bits of it: a
    difference in h below that does not show."""
    kind, H, nread = {"pair_lstm384": (M.NET_LSTM5, 384, 256), "pack_lstm256": (M.NET_LSTM5, 256, 1040),
                      "pack_grumod256": (M.NET_GRUMOD5, 256, 1040)}[form]
    pair = form.startswith("pair")
    flags = _flags(B, SWITCHES[switch][0])
    monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
    mdl = GP.probe_model(kind, H, seed=40 + H)
    rng = np.random.default_rng(3)
    sigs = [[rng.standard_normal(n).astype(np.float32) for n in _lengths(kind, nread)] for _ in range(2 if pair else 1)]
    dm = B.DeviceModel(engine, mdl)
    try:
        monkeypatch.delenv("FFHIP_DEBUG", raising=False)
        lean = _transitions(B, dm, sigs, nread, flags, pair)
        monkeypatch.setenv("FFHIP_DEBUG", "no_dense,no_pair")
        plain = _transitions(B, dm, sigs, nread, flags, False) + (_transitions(B, dm, sigs[1:], nread, flags, False) if pair else [])
    finally:
        dm.close()
    for k in range(len(lean)):
        for r in range(nread):
            ok = GP.same_bits(lean[k][r], plain[k][r])
            assert ok.all(), "%s batch %d read %d: %d transition scores differ" % (form, k, r, (~ok).sum())


def test_outlier_rerun_replays_exp_ps_under_env0(B, engine, monkeypatch):
    """a read beyond the split format's range is run again on the f32 path (k_lstm_fused); under FFHIP_FAST_GATES=0 -- and at any level --
    that path replays the reference's exp_ps: its transition scores equal those of the read run with FFHIP_RUN_F32_RNN | FFHIP_RUN_EXACT_GATES"""
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=7)
    rng = np.random.default_rng(9)
    sig = rng.standard_normal((16, 1500)).astype(np.float32)
    sig[3, 200] = 6.0e4
    dm = B.DeviceModel(engine, mdl)
    try:
        monkeypatch.delenv("FFHIP_FAST_GATES", raising=False)
        d = B.Batch(dm, 16, 1500)
        d.set_signals(sig)
        d.run(1.0, B.RUN_F32_RNN | B.RUN_EXACT_GATES)
        d.finish()
        want = d.transitions(3)
        d.close()
        for env in ("0", "2"):
            monkeypatch.setenv("FFHIP_FAST_GATES", env)
            b = B.Batch(dm, 16, 1500)
            b.set_signals(sig)
            b.run()
            b.finish()
            assert b.f32_reruns() == 1
            ok = GP.same_bits(b.transitions(3), want)
            b.close()
            assert ok.all(), "FFHIP_FAST_GATES=%s: %d transition scores of the re-run read differ from the exact replay's" % (env, (~ok).sum())
    finally:
        dm.close()
