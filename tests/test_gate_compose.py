"""The host composition of tests/gate_probe.py, fed the oracle's own gate functions (fo_logisticf / fo_tanhf), reproduces the oracle's
layer outputs for a probe model bit for bit, forward and backward layers, LSTM and GRUmod.  tests/test_gate_levels_gpu.py composes the
device's hardware gate forms the same way and holds the split layer kernels to the result, so this test is what makes that comparison
mean "the kernel runs exactly these gate functions in this order"."""
import numpy as np
import pytest

from flappie_amd import model as M

import gate_probe as GP


@pytest.mark.parametrize("kind,hidden", [(M.NET_LSTM5, 64), (M.NET_LSTM5, 36), (M.NET_GRUMOD5, 64)])
def test_composition_reproduces_the_oracle(kind, hidden):
    mdl = GP.probe_model(kind, hidden, seed=3)
    sig, tanh = GP.oracle_map(2), GP.oracle_map(3)
    n = 23
    seen = set()
    for l in range(5):
        b = GP.layer_bias(mdl, l)
        seen.update(np.unique(b.view(np.uint32)).tolist())
        ref = GP.oracle_layer(mdl, l, n)
        assert ref.shape == (n, hidden)
        got = GP.compose(kind, b, n, sig, tanh)
        if l % 2 == 0:                                   # backward: step i is block n - 1 - i
            got = got[::-1]
        ok = GP.same_bits(got, ref)
        assert ok.all(), "layer %d: %d of %d differ, first at %s" % (l, (~ok).sum(), ok.size, np.argwhere(~ok)[:3].tolist())
        assert np.isfinite(ref).all()
    # the probe reaches every class of PROBE_VALUES
    assert len(seen) >= len(GP.PROBE_VALUES) - 2


def test_probe_model_pre_activations_are_the_bias():
    """zero weights: the oracle's affine input of a layer is its bias at every step (the premise of the probe)"""
    from oracle import ffo
    mdl = GP.probe_model(M.NET_LSTM5, 64, seed=4)
    L = ffo.lib()
    x = ffo.HostMat.from_dense(np.random.default_rng(0).standard_normal((9, 64)).astype(np.float32))
    r = mdl.rnns[1]
    xa = ffo.take(L.fo_affine_map(x.ptr, ffo.HostMat.from_model_mat(r.iW).ptr, ffo.HostMat.from_model_mat(r.b).ptr))
    b = GP.layer_bias(mdl, 1)
    same = GP.same_bits(xa, np.tile(b, (9, 1))) | ((xa == 0) & (b == 0)) | (np.isnan(xa) & np.isnan(b))
    assert same.all()
