"""Shared pieces of the gate-math tests (tests/test_gate_compose.py, tests/test_gate_levels_gpu.py): probe models whose every gate
pre-activation is exactly its bias, the oracle's layer outputs for them, and the host composition of a layer's steps from gate values.

Probe model: synthetic_model with every iW and sW of the five recurrent layers set to zero.  The products are then exact zeros, the bias
enters the layer kernels' scaled accumulator space by a power of two (2^S with S = 4 for the first LSTM layer, 12 for the others: both
weight matrices are zero, so their exponents are 0; GRUmod adds its bias outside that space), and the library is built with
-ffp-contract=off -- so in any kernel and at any step the pre-activation of a gate is its bias, bit for bit, and the layer's output
depends on the bias and on the step count from the read's start (forward) or end (backward) alone.  Every value of PROBE_VALUES,
+-1e30 included, survives the scaling: |b| 2^12 stays below FLT_MAX for |b| < 8e34, and 2^12 times a denormal is exact."""
import ctypes as C

import numpy as np

from flappie_amd import model as M

# moderate, tiny (denormal included), near the clamp of exp_ps (+-88.3762626647949) and the 2^126 branch of the lean reciprocal (-87.34),
# large, infinite and NaN pre-activations
PROBE_VALUES = np.array([0.0, -0.0, 0.1, -0.1, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.5, -3.5, 7.0, -7.0, 15.0, -15.0, 40.0, -40.0,
                         1e-7, -1e-7, 1e-30, -1e-30, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                         88.3762626647949, -88.3762626647949, 88.37627, -88.37627, 88.0, -88.0, 87.34, -87.34, 87.5, -87.5, 89.0, -89.0, 100.0, -100.0,
                         1e30, -1e30, np.inf, -np.inf, np.nan], dtype=np.float32)


# the layer kernels a run can take, by rnn_path() and run flags (tests/test_gate_levels_gpu.py with probe models, tests/test_layers_fp64_gpu.py with real weights)
# (kind, H, run flags, reads, rnn path, whether the kernel follows the gate level)
PATHS = {
    "split_lstm128": (M.NET_LSTM5, 128, 0, 256, 3, True),
    "split_lstm256": (M.NET_LSTM5, 256, 0, 520, 3, True),
    "split_lstm384": (M.NET_LSTM5, 384, 0, 512, 3, True),        # the dense pair form at a full launch
    "split_lstm512": (M.NET_LSTM5, 512, 0, 256, 3, True),        # k_lstm_split<0, 4, 2>
    "split_grumod128": (M.NET_GRUMOD5, 128, 0, 256, 3, True),
    "split_grumod256": (M.NET_GRUMOD5, 256, 0, 520, 3, True),
    "unfused_lstm256": (M.NET_LSTM5, 256, "UNFUSED", 256, 4, False),       # k_inproj_split + k_rnn_split
    "unfused_grumod128": (M.NET_GRUMOD5, 128, "UNFUSED", 256, 1, False),   # (no recurrence-only split kernel for GRUmod: k_rnn_persist)
    "f32_lstm128": (M.NET_LSTM5, 128, "F32", 256, 2, False),               # k_lstm_fused
    "f32_lstm384": (M.NET_LSTM5, 384, "F32", 256, 2, False),
    "f32_grumod256": (M.NET_GRUMOD5, 256, "F32", 256, 2, False),
    "f32_unfused_lstm128": (M.NET_LSTM5, 128, "F32|UNFUSED", 256, 1, False),   # k_rnn_persist
    "stepwise_lstm128": (M.NET_LSTM5, 128, "STEPWISE", 256, 0, False),
    "stepwise_grumod128": (M.NET_GRUMOD5, 128, "STEPWISE", 256, 0, False),
    "small_lstm64": (M.NET_LSTM5, 64, 0, 256, 2, False),                   # the small-H default: k_lstm_fused
    "small_lstm96": (M.NET_LSTM5, 96, 0, 256, 2, False),
    "small_lstm36": (M.NET_LSTM5, 36, 0, 256, 2, False),                   # padded to 48 units
    "small_grumod64": (M.NET_GRUMOD5, 64, 0, 256, 2, False),
}


def run_flags(B, spec):
    if not spec:
        return 0
    names = {"UNFUSED": B.RUN_UNFUSED_RNN, "F32": B.RUN_F32_RNN, "STEPWISE": B.RUN_STEPWISE_RNN, "EXACT": B.RUN_EXACT_GATES,
             "FAST": B.RUN_FAST_GATES, "FAST2": B.RUN_FAST_GATES2}
    f = 0
    for n in spec.split("|"):
        f |= names[n]
    return f


def read_lengths(kind, nread):
    """four distinct lengths (samples), ragged over the batch"""
    base = (1500, 1237, 905, 1496) if kind == M.NET_LSTM5 else (800, 655, 421, 797)
    return [base[(r * 7) % 4] for r in range(nread)]


def probe_model(kind: int, hidden: int, seed: int = 5):
    """synthetic_model(kind, hidden) with zero recurrent-layer weights and biases drawn per unit and gate from PROBE_VALUES"""
    mdl = M.synthetic_model(kind, hidden, seed=seed)
    rng = np.random.default_rng(seed + 1000 * hidden + kind)
    for r in mdl.rnns:
        r.iW.data[:] = 0.0
        r.sW.data[:] = 0.0
        n = r.b.nr
        r.b.data[0, :n] = rng.choice(PROBE_VALUES, size=n)
    return mdl


def gates_of(kind: int) -> int:
    return 3 if kind == M.NET_GRUMOD5 else 4


def layer_bias(mdl, l: int) -> np.ndarray:
    r = mdl.rnns[l]
    return r.b.data[0, : r.b.nr].copy()


def compose(kind: int, bias: np.ndarray, nstep: int, sig, tanh) -> np.ndarray:
    """[nstep, H] outputs of a layer whose pre-activations are `bias` at every step, in float32 and in the order of the layer kernels'
    gate phase (ffhip_rnn_split.hip gate_tile) and of the reference's lstm_step / grumod_step; sig / tanh map a float32 array to the
    gate function's values (the oracle's fo_logisticf / fo_tanhf, or the device's forms through ffhip_debug_gate_math)"""
    f32 = np.float32
    bias = np.asarray(bias, dtype=f32)
    out = []
    if kind == M.NET_GRUMOD5:
        H = bias.size // 3
        bz, br, bc = bias[:H], bias[H:2 * H], bias[2 * H:]
        z = sig(bz)
        r = sig(br)
        hbar = tanh(r * f32(0.0) + bc)              # r (sW h)_c + x_c with (sW h)_c = 0: the candidate's pre-activation is its bias
        h = np.zeros(H, dtype=f32)
        for _ in range(nstep):
            h = z * h + (f32(1.0) - z) * hbar
            out.append(h)
    else:
        H = bias.size // 4
        bi, bf, bg, bo = bias[:H], bias[H:2 * H], bias[2 * H:3 * H], bias[3 * H:]
        Li, Lf, Lo, Tg = sig(bi), sig(bf), sig(bo), tanh(bg)
        c = np.zeros(H, dtype=f32)
        for _ in range(nstep):
            forget = Lf * c
            update = Li * Tg
            c = forget + update
            out.append(Lo * tanh(c))
    return np.array(out, dtype=f32).reshape(nstep, H)


def oracle_map(kind: int):
    """fo_logisticf (kind 2) / fo_tanhf (kind 3) of a float32 array, through the oracle's array form"""
    from oracle import ffo
    L = ffo.lib()
    L.fo_map_array.argtypes = [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]

    def f(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        if x.size:
            assert L.fo_map_array(kind, x.ctypes.data_as(C.POINTER(C.c_float)), y.ctypes.data_as(C.POINTER(C.c_float)), x.size) == 0
        return y
    return f


def oracle_layer(mdl, l: int, nblock: int) -> np.ndarray:
    """[nblock, H] output of recurrent layer l for a read of nblock blocks: the oracle's fo_lstm / fo_grumod on the layer's affine input,
    which for a probe model is the bias at every step (fo_affine_map adds iW x = 0 to it)"""
    from oracle import ffo
    L = ffo.lib()
    r = mdl.rnns[l]
    xa = ffo.HostMat.from_dense(np.tile(layer_bias(mdl, l), (nblock, 1)))
    sw = ffo.HostMat.from_model_mat(r.sW)
    fn = L.fo_grumod if mdl.kind == M.NET_GRUMOD5 else L.fo_lstm
    return ffo.take(fn(xa.ptr, sw.ptr, int(l % 2 == 0)))


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.asarray(a, dtype=np.float32).view(np.uint32) == np.asarray(b, dtype=np.float32).view(np.uint32)
