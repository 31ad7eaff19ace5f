"""Shared pieces of the step-local layer checks (tests/test_layer_step_ref.py on the CPU, tests/test_layers_fp64_gpu.py on the GPU): fp32
evaluations of one recurrent layer with h(t-1) FORCED to a given trajectory, to be measured with the same metric as a kernel -- the oracle's
own arithmetic (fo_affine_map for iW x + b, then sW h accumulated onto it in the reference's sequential order, its logistic and tanh, the
cell chain in fp32) and a plain fp32 numpy GEMM --, the metric itself, and the bounds of the kernel forms.
TEST INFRASTRUCTURE: no code of the product imports this."""
import numpy as np

import fp64_ref as R
import gate_probe as GP
from flappie_amd import model as M

FLOOR_X, FLOOR_H = 2.0 ** -29, 2.0 ** -37       # absolute floors of the split operand format (ffhip_split.hpp): swish outputs at 2^4, bounded ones at 2^12
TILE = 16                                       # units of a unit tile, reads of a read tile


def weights(mdl, l):
    """dense [G H, H] iW, sW and [G H] bias of recurrent layer l"""
    r = mdl.rnns[l]
    return r.iW.dense(), r.sW.dense(), r.b.data[0, :r.b.nr]


def is_lstm(mdl):
    return mdl.kind != M.NET_GRUMOD5


def f32_bound(H):
    """fp32 forms (module docstring of tests/test_layers_fp64_gpu.py): 32 per 16-wide K chunk over K = 2 H padded to 16, + 16"""
    return 32 * 2 * (-(-H // 16)) + 16


def split_bound(H):
    """split forms: 4 + 4 + 8 + 8 + 6 per 32-wide K chunk over K = 2 H"""
    return 24 + 6 * (2 * H // 32)


def split_floors(l, lstm):
    """the split format's floors of layer l's operands: x of the first LSTM layer is the swish convolution's output (2^4), every other operand is bounded by 1 (2^12)"""
    return (FLOOR_X if (l == 0 and lstm) else FLOOR_H), FLOOR_H


# ---- fp32 evaluations with h forced ---------------------------------------------------------------------------------------------
def _gate_phase(lstm, z, u, xc, hp, backward, sig, tanh):
    """fp32 gate phase in the order of lstm_step / grumod_step; z [T, G H] (GRUmod: the z and r rows), u, xc: GRUmod's (sW h)_c and (iW x)_c + b_c.
    Returns (h, c) with c the LSTM's cell state (None for GRUmod)."""
    f32 = np.float32
    H = hp.shape[-1]
    T = hp.shape[0]
    if not lstm:
        Z, Rg = sig(z[:, :H]), sig(z[:, H:2 * H])
        hbar = tanh(Rg * u + xc)
        return (Z * hp + (f32(1.0) - Z) * hbar).astype(f32), None
    Li, Lf, Tg, Lo = sig(z[:, :H]), sig(z[:, H:2 * H]), tanh(z[:, 2 * H:3 * H]), sig(z[:, 3 * H:])
    c = np.zeros(H, dtype=f32)
    cs = np.zeros((T, H), dtype=f32)
    for t in (range(T - 1, -1, -1) if backward else range(T)):
        c = Lf[t] * c + Li[t] * Tg[t]
        cs[t] = c
    return (Lo * tanh(cs)).astype(f32), cs


def forced_oracle(lstm, x, h, iW_mat, sW_mat, b_mat, backward):
    """the oracle's arithmetic on x [T, H] with every step started from the given h: (h, c).  On the oracle's OWN h this returns that h bit for bit."""
    from oracle import ffo
    L = ffo.lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    hp = R.previous_state(np.ascontiguousarray(h, dtype=np.float32), backward)
    T, H = hp.shape
    xa = ffo.take(L.fo_affine_map(ffo.HostMat.from_dense(x).ptr, ffo.HostMat.from_model_mat(iW_mat).ptr, ffo.HostMat.from_model_mat(b_mat).ptr))
    sw = ffo.HostMat.from_model_mat(sW_mat)
    G = 4 if lstm else 3
    z = np.empty((T, G * H), dtype=np.float32)
    for t in range(T):
        bias = xa[t:t + 1].copy()
        if not lstm:
            bias[0, 2 * H:] = 0.0                # grumod_step zeroes the candidate's rows before the product (layers.c:691)
        z[t] = ffo.take(L.fo_affine_map(ffo.HostMat.from_dense(hp[t:t + 1]).ptr, sw.ptr, ffo.HostMat.from_dense(bias).ptr))[0]
    sig, tanh = GP.oracle_map(2), GP.oracle_map(3)
    if lstm:
        return _gate_phase(True, z, None, None, hp, backward, sig, tanh)
    return _gate_phase(False, z, z[:, 2 * H:], xa[:, 2 * H:], hp, backward, sig, tanh)


def forced_gemm(lstm, x, h, iW, sW, b, backward):
    """a plain fp32 numpy GEMM for both products, the oracle's gate functions: (h, c)"""
    f32 = np.float32
    x = np.ascontiguousarray(x, dtype=f32)
    hp = R.previous_state(np.ascontiguousarray(h, dtype=f32), backward)
    H = hp.shape[-1]
    zx = x @ np.ascontiguousarray(iW.T, dtype=f32) + b.astype(f32)
    zh = hp @ np.ascontiguousarray(sW.T, dtype=f32)
    sig, tanh = GP.oracle_map(2), GP.oracle_map(3)
    if lstm:
        return _gate_phase(True, zx + zh, None, None, hp, backward, sig, tanh)
    z = zx + zh
    return _gate_phase(False, z, zh[:, 2 * H:], zx[:, 2 * H:], hp, backward, sig, tanh)


# ---- the metric -------------------------------------------------------------------------------------------------------------
def norm_err(got, want, allow):
    """|got - want| / allowance per element; a non-finite `got` counts as infinite error (the layers' outputs are finite for any input: the
    reference's gates clamp, tests/test_gate_math_gpu.py::test_nan_pre_activation_gives_a_finite_gate)"""
    g = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(g), np.abs(g - want) / allow, np.inf)


def tile_rms(err):
    """err [..., T, H] -> root mean square of the normalised error per unit tile of 16 units (the last one may be short), over every read and step"""
    H = err.shape[-1]
    e2 = (err.reshape(-1, H) ** 2).mean(axis=0)
    return np.sqrt(np.array([e2[u:u + TILE].mean() for u in range(0, H, TILE)]))


def locate(err):
    """(worst normalised error, its index) of err [N, T, H] or [T, H]"""
    k = np.unravel_index(int(np.argmax(err)), err.shape)
    return float(err[k]), tuple(int(v) for v in k)
