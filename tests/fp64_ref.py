"""Plain float64 restatements of the network's operations: the convolutions with their activations, one step of the recurrent
layers (LSTM and GRUmod) from given x(t) and h(t-1), the flip-flop and run-length CRF heads with their global normalisation, and
the flip-flop forward-backward posterior.  The GPU tests (tests/test_front_head_fp64_gpu.py, tests/test_layers_fp64_gpu.py) hold
each kernel to these on the kernel's OWN input, so a check does not depend on how the rounding upstream went; tests/test_fp64_ref.py
and tests/test_layer_step_ref.py hold these to the oracle, to torch and to autograd.
TEST INFRASTRUCTURE: no code of the product imports this."""
import numpy as np

F32_EPS = 2.0 ** -24          # unit roundoff of fp32


def ulp32(x):
    """spacing of fp32 numbers at |x| (the smallest subnormal spacing at 0)"""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


# ---- convolution: the reference's three regions (layers.c:189-276) ----------------------------
def conv_windows(T, winlen, stride):
    """[(output column, first input sample)] of every window the reference accumulates (a column may take two at a strided right edge)"""
    s = stride
    padL, padR = (winlen - 1) // 2, winlen // 2
    Tout = -(-T // s)
    ncolsL = -(-padL // s)
    shiftX = ncolsL * s - padL
    nstepC = -(-winlen // s)
    nstepX = s * nstepC
    out = []

    def add(col, x0):
        if 0 <= col < Tout:
            out.append((col, x0))
    for w in range(0, padL, s):
        add(w // s, w - padL)
    for w in range(0, winlen, s):
        for k in range((T - shiftX - w) // nstepX):
            add(ncolsL + w // s + nstepC * k, shiftX + w + nstepX * k)
    maxCol, rem = (T - shiftX) // nstepX, (T - shiftX) % nstepX
    colR = ncolsL + nstepC * (maxCol - 1) + rem // s + 1
    startR = s - (padL + T - winlen) % s - 1
    for w in range(startR, padR, s):
        add(colR + w // s, T - winlen + 1 + w)
    return Tout, out


def conv_terms(x, taps, bias, stride):
    """x[T, nf]; taps[nfilter, winlen, nf] -> (z, cond): the float64 pre-activation of every output and its condition
    sum |w x| + |b| (what an fp32 evaluation's rounding error is proportional to).  Samples outside [0, T) are zero."""
    T, nf = x.shape
    nfilter, winlen, _ = taps.shape
    Tout, wins = conv_windows(T, winlen, stride)
    xp = np.zeros((T + 2 * winlen, nf))
    xp[winlen:winlen + T] = x
    w64 = taps.astype(np.float64).reshape(nfilter, winlen * nf)
    z = np.tile(bias.astype(np.float64), (Tout, 1))
    cond = np.tile(np.abs(bias.astype(np.float64)), (Tout, 1))
    cols = np.array([c for c, _ in wins], dtype=np.int64)
    x0s = np.array([x0 for _, x0 in wins], dtype=np.int64)
    idx = x0s[:, None] + winlen + np.arange(winlen)[None, :]
    win = xp[idx].reshape(len(wins), winlen * nf)                # [window][winlen * nf]
    np.add.at(z, cols, win @ w64.T)
    np.add.at(cond, cols, np.abs(win) @ np.abs(w64).T)
    # a NaN or inf anywhere in a window reaches its column (0 x inf included)
    bad = ~np.isfinite(win).all(axis=1)
    if bad.any():
        np.add.at(z, cols[bad], np.nan)
    return z, cond


def numpy_conv_recipe(x, taps, bias, stride):
    """x[T, nf]; taps[nfilter, winlen, nf].  float64 evaluation of the reference's three regions."""
    return conv_terms(np.asarray(x, dtype=np.float64), taps, bias, stride)[0]


def swish64(z):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(z < -745.0, -0.0, z / (1.0 + np.exp(-z)))


def dswish64(z):
    with np.errstate(over="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-z))
        return s * (1.0 + z * (1.0 - s))


def tanh64(z):
    """the reference's tanh (2 logistic(2x) - 1 on a clamped exp) takes a NaN to -1: so does this one"""
    return np.where(np.isnan(z), -1.0, np.tanh(z))


def dtanh64(z):
    return 1.0 - np.tanh(z) ** 2


def act_rounding(y, swish):
    """what the reference's fp32 activations add on top of their argument's error: swish (x * logistic(x)) a few ulp of its value;
    tanh (built on the logistic: 2 logistic(2x) - 1) an ABSOLUTE error of up to 3 x 2^-24 (measured 2.97 over [-3, 3])"""
    return 4 * ulp32(y) + (0.0 if swish else 4 * F32_EPS)


def activation(kind_swish):
    """(f, f') of the convolutions of a model: swish for the LSTM models, tanh for GRUmod (layers.c:24-49)"""
    return (swish64, dswish64) if kind_swish else (tanh64, dtanh64)


# ---- CRF chains: a transition p goes from state src[p] to state dst[p] -------------------------------------------------------
def flipflop_map(nbase):
    """flip-flop transitions (layers.c:1035-1079): p = to * nstate + from into a flip state; nbase * nstate + b: flip b -> flop b;
    nbase * nstate + nbase + b: flop b stays"""
    ns = 2 * nbase
    src, dst = [], []
    for to in range(nbase):
        for fr in range(ns):
            src.append(fr); dst.append(to)
    for b in range(nbase):
        src.append(b); dst.append(b + nbase)
    for b in range(nbase):
        src.append(b + nbase); dst.append(b + nbase)
    return np.array(src), np.array(dst), ns


def runlength_map(nbase):
    """the run-length model's 2 nbase^2 transitions behind its 2 nbase shape/scale rows (rle_trans_lookup, layers.c:1241-1246)"""
    src, dst = [], []
    for p in range(2 * nbase * nbase):
        to, rem = divmod(p, 2 * nbase)
        fr, stay_from = rem % nbase, rem >= nbase
        src.append(fr + (nbase if stay_from else 0))
        dst.append(to + nbase if fr == to else to)
    return np.array(src), np.array(dst), 2 * nbase


def _lse_into(vals, groups, n):
    """log sum exp of vals[i] into bin groups[i] (n bins), float64"""
    m = np.max(vals)
    if not np.isfinite(m):
        m = 0.0
    s = np.bincount(groups, weights=np.exp(vals - m), minlength=n)
    with np.errstate(divide="ignore"):
        return np.log(s) + m


def crf_logz(S, cmap):
    """log partition function, every state starting at log 1 (S [T, P] float64)"""
    src, dst, ns = cmap
    alpha = np.zeros(ns)
    for t in range(S.shape[0]):
        alpha = _lse_into(alpha[src] + S[t], dst, ns)
    m = alpha.max()
    return float(m + np.log(np.exp(alpha - m).sum()))


def crf_posterior(S, cmap):
    """posterior probability of every transition of every block: exp(alpha[t-1][src] + S[t] + beta[t][dst] - logZ), float64 [T, P]"""
    src, dst, ns = cmap
    S = np.asarray(S, dtype=np.float64)
    T = S.shape[0]
    alpha = np.zeros((T + 1, ns))
    for t in range(T):
        alpha[t + 1] = _lse_into(alpha[t][src] + S[t], dst, ns)
    beta = np.zeros((T + 1, ns))
    for t in range(T, 0, -1):
        beta[t - 1] = _lse_into(S[t - 1] + beta[t][dst], src, ns)
    m = alpha[T].max()
    logz = m + np.log(np.exp(alpha[T] - m).sum())
    return np.exp(alpha[:T][:, src] + S + beta[1:][:, dst] - logz), logz


def runlength_transpost64(S, nbase):
    """transpost_crf_runlength's transition columns in float64, as decode.c:1102-1126 writes them: alpha[t][src] + S[t] + beta[t+1][dst], not
    normalised, no - logZ (S [T, 2 nbase^2]: the transition columns alone).  Returns (post [T, P], alpha [T + 1, ns], beta [T + 1, ns])."""
    src, dst, ns = runlength_map(nbase)
    S = np.asarray(S, dtype=np.float64)
    T = S.shape[0]
    alpha = np.zeros((T + 1, ns))
    for t in range(T):
        alpha[t + 1] = _lse_into(alpha[t][src] + S[t], dst, ns)
    beta = np.zeros((T + 1, ns))
    for t in range(T, 0, -1):
        beta[t - 1] = _lse_into(S[t - 1] + beta[t][dst], src, ns)
    return alpha[:T][:, src] + S + beta[1:][:, dst], alpha, beta


def runlength_best_path(S, nbase):
    """plain float64 Viterbi over the run-length states, every state starting at 0 (decode_crf_runlength, decode.c:927-1013): (score, path [T]).
    np.argmax takes the first maximum, which is NOT the reference's order among equal scores: for scores without ties only."""
    src, dst, ns = runlength_map(nbase)
    S = np.asarray(S, dtype=np.float64)
    T = S.shape[0]
    v = np.zeros(ns)
    back = np.zeros((T, ns), dtype=np.int64)
    for t in range(T):
        cand = np.full((ns, ns), -np.inf)                     # [dst][src]
        cand[dst, src] = v[src] + S[t]
        back[t] = cand.argmax(axis=1)
        v = cand.max(axis=1)
    path = np.zeros(T, dtype=np.int64)
    last = int(v.argmax())
    for t in range(T - 1, -1, -1):
        path[t] = last
        last = back[t, last]
    return float(v.max()), path


# ---- heads ---------------------------------------------------------------------------------------------------------------
def head_terms(h, W, b):
    """h [T, H]; W [P, H]; b [P] -> (z, cond): float64 W h + b and sum |W h| + |b|"""
    h64, W64, b64 = (np.asarray(a, dtype=np.float64) for a in (h, W, b))
    return h64 @ W64.T + b64, np.abs(h64) @ np.abs(W64).T + np.abs(b64)


def flipflop_head(h, W, b, temperature, nbase):
    """globalnorm_manystay (layers.c:1082-1106) in float64: S = tanh(W h + b) * 5 / temperature, minus logZ(S) / T.
    Returns (scores, S, z, cond, logZ)."""
    z, cond = head_terms(h, W, b)
    S = np.tanh(z) * (5.0 / temperature)
    logz = crf_logz(S, flipflop_map(nbase))
    return S - logz / S.shape[0], S, z, cond, logz


def softplus64(x):
    return np.logaddexp(0.0, x)


def runlength_head(h, W, b, temperature, nbase):
    """globalnorm_runlengthV2 (layers.c:1325-1358) in float64: shape 1 + softplus, scale 1e-8 + softplus, transitions
    5 tanh / temperature minus logZ / T.  Returns (params, z, cond, logZ)."""
    z, cond = head_terms(h, W, b)
    out = np.empty_like(z)
    out[:, :nbase] = 1.0 + softplus64(z[:, :nbase])
    out[:, nbase:2 * nbase] = 1e-8 + softplus64(z[:, nbase:2 * nbase])
    tr = 5.0 * np.tanh(z[:, 2 * nbase:]) / temperature
    logz = crf_logz(tr, runlength_map(nbase))
    out[:, 2 * nbase:] = tr - logz / z.shape[0]
    return out, z, cond, logz


# ---- recurrent layers, one step at a time ("teacher forced": every step starts from the h(t-1) the code under test wrote) ---
LOGISTIC_CLAMP = 88.3762626647949      # the reference's exp_ps clamps its argument here: logistic(x <= -clamp) = 4.156e-39, and a NaN goes the same way


def logistic64(z):
    with np.errstate(invalid="ignore"):
        zc = np.where(np.isnan(z), -LOGISTIC_CLAMP, np.clip(z, -LOGISTIC_CLAMP, LOGISTIC_CLAMP))
    return 1.0 / (1.0 + np.exp(-zc))


def layer_backward(l):
    """layers 0, 2, 4 of both networks run from the read's end (networks.c:450-489, 539-586)"""
    return l % 2 == 0


def previous_state(h, backward):
    """h [..., T, H] -> the state every step starts from: h(t-1) (h(t+1) in a backward layer), zero at the read's first step"""
    hp = np.zeros_like(h)
    if backward:
        hp[..., :-1, :] = h[..., 1:, :]
    else:
        hp[..., 1:, :] = h[..., :-1, :]
    return hp


def layer_terms(x, hp, iW, sW, b):
    """x, hp [..., T, H]; iW, sW [G H, H] ([out][in]); b [G H] -> float64 (iW x + b, |iW||x| + |b|, sW h, |sW||h|)"""
    x64, h64, i64, s64, b64 = (np.asarray(a, dtype=np.float64) for a in (x, hp, iW, sW, b))
    with np.errstate(invalid="ignore", over="ignore"):
        zx = x64 @ i64.T + b64
        cx = np.abs(x64) @ np.abs(i64).T + np.abs(b64)
        zh = h64 @ s64.T
        ch = np.abs(h64) @ np.abs(s64).T
    return zx, cx, zh, ch


def _budget(cond, floor):
    """one unit of pre-activation error: cond 2^-24 (0 where the pre-activation is not finite: its gate is a constant there) + the format's floor"""
    return np.where(np.isfinite(cond), cond, 0.0) * F32_EPS + floor


def _dlogistic(s):
    return s * (1.0 - s)


def grumod_step_ref(x, h, iW, sW, b, backward, floor_x=0.0, floor_h=0.0):
    """grumod_step (layers.c:664-715) in float64, every step from the given h(t-1): gate order z, r, candidate;
    hbar = tanh(r (sW h)_c + (iW x)_c + b_c); h' = z h + (1 - z) hbar.  floor_x / floor_h: absolute error floor of the operand
    format of x / h (0 for fp32 operands).  Returns (expected h, allowance for ONE unit of pre-activation error + the roundings
    of the gate phase)."""
    H = sW.shape[1]
    hp = previous_state(np.asarray(h, dtype=np.float64), backward)
    zx, cx, zh, ch = layer_terms(x, hp, iW, sW, b)
    fx = floor_x * np.abs(np.asarray(iW, dtype=np.float64)).sum(axis=1)
    fh = floor_h * np.abs(np.asarray(sW, dtype=np.float64)).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        bud = _budget(cx + ch, fx + fh)
        Z, Rg = logistic64((zx + zh)[..., :H]), logistic64((zx + zh)[..., H:2 * H])
        dZ = _dlogistic(Z) * bud[..., :H] + 4 * ulp32(Z)
        dR = _dlogistic(Rg) * bud[..., H:2 * H] + 4 * ulp32(Rg)
        u, xc = zh[..., 2 * H:], zx[..., 2 * H:]
        du, dxc = _budget(ch[..., 2 * H:], fh[2 * H:]), _budget(cx[..., 2 * H:], fx[2 * H:])
        a = Rg * u + xc
        afin = np.isfinite(a)
        a0 = np.where(afin, a, 0.0)
        da = np.abs(u) * dR + Rg * du + dxc + ulp32(np.where(afin, Rg * u, 0.0)) + ulp32(a0)
        hbar = tanh64(a)
        dhbar = np.where(afin, dtanh64(a0) * np.where(afin, da, 0.0), 0.0) + act_rounding(hbar, False)
        want = Z * hp + (1.0 - Z) * hbar
        allow = np.abs(hp - hbar) * dZ + (1.0 - Z) * dhbar + ulp32(Z * hp) + ulp32((1.0 - Z) * hbar) + ulp32(1.0 - Z) * np.abs(hbar) + ulp32(want)
    return want, allow


def lstm_step_ref(x, h, iW, sW, b, backward, floor_x=0.0, floor_h=0.0):
    """lstm_step (layers.c:979-1026) in float64, gate order i, f, g, o, the gates of every step from the given h(t-1).  The cell state is
    not part of the layer's output, so it is carried here, c64(t) = f c64(t-1) + i g, and beside it a first-order running bound e_c(t) on
    |c - c64| of an evaluation whose pre-activations are off by one unit (cond 2^-24 + floor) and whose gate phase rounds in fp32:
        e_c(t) = f e_c(t-1) + |c64(t-1)| d_f + |g| d_i + |i| d_g + ulp(f c) + ulp(i g) + ulp(c),   d_gate = |gate'(z)| unit + the gate's own rounding.
    Returns (expected h = o tanh(c64), its allowance |tanh c| d_o + o tanh'(c) e_c + roundings, c64, e_c)."""
    H = sW.shape[1]
    hp = previous_state(np.asarray(h, dtype=np.float64), backward)
    zx, cx, zh, ch = layer_terms(x, hp, iW, sW, b)
    fl = floor_x * np.abs(np.asarray(iW, dtype=np.float64)).sum(axis=1) + floor_h * np.abs(np.asarray(sW, dtype=np.float64)).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        z = zx + zh
        bud = _budget(cx + ch, fl)
        gi, gf, go = logistic64(z[..., :H]), logistic64(z[..., H:2 * H]), logistic64(z[..., 3 * H:])
        zg = z[..., 2 * H:3 * H]
        gg = tanh64(zg)
        d_i = _dlogistic(gi) * bud[..., :H] + 4 * ulp32(gi)
        d_f = _dlogistic(gf) * bud[..., H:2 * H] + 4 * ulp32(gf)
        d_o = _dlogistic(go) * bud[..., 3 * H:] + 4 * ulp32(go)
        d_g = np.where(np.isfinite(zg), dtanh64(np.where(np.isfinite(zg), zg, 0.0)), 0.0) * bud[..., 2 * H:3 * H] + act_rounding(gg, False)
    T = z.shape[-2]
    c64, e_c = np.zeros_like(gi), np.zeros_like(gi)
    c, e = np.zeros(gi.shape[:-2] + (H,)), np.zeros(gi.shape[:-2] + (H,))
    for t in (range(T - 1, -1, -1) if backward else range(T)):
        f, i, g = gf[..., t, :], gi[..., t, :], gg[..., t, :]
        cn = f * c + i * g
        e = f * e + np.abs(c) * d_f[..., t, :] + np.abs(g) * d_i[..., t, :] + np.abs(i) * d_g[..., t, :] + ulp32(f * c) + ulp32(i * g) + ulp32(cn)
        c = cn
        c64[..., t, :], e_c[..., t, :] = c, e
    tc = np.tanh(c64)
    want = go * tc
    allow = np.abs(tc) * d_o + go * (1.0 - tc * tc) * e_c + go * act_rounding(tc, False) + ulp32(want)
    return want, allow, c64, e_c


def layer_step_ref(lstm, x, h, iW, sW, b, backward, floor_x=0.0, floor_h=0.0):
    """(expected h, allowance) of either cell"""
    if lstm:
        return lstm_step_ref(x, h, iW, sW, b, backward, floor_x, floor_h)[:2]
    return grumod_step_ref(x, h, iW, sW, b, backward, floor_x, floor_h)
