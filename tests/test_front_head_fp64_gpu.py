"""The convolutions, the CRF head and the fp64 chains, each held to a float64 restatement (tests/fp64_ref.py) on the kernel's OWN
input, read back through the debug read-outs of include/ffhip.h (Batch.keep_front / front / head_input / forms).  A check here
does not absorb the error of the recurrent layers, so a fault of fp16-only accuracy (a dropped split product, ~2^-11 of a
product), a window off by one at a strided right edge or a packed read boundary, or a phantom tap reading a live sample shows.

Error metric (per element, normalised by the problem's condition):
    convolution   |got - f(z)| / (|f'(z)| (sum|w x| + |b|) 2^-24 + ulp(f(z)) + [tanh: 2^-24] + floor)
    head          |got - ref| / (5/T (|tanh'(z)| (sum|w h| + |b|) 2^-24 + 2^-24) + ulp(S) + ulp(ref) + ulp(logZ/T) + mean_t max_p of the first part)
    chains        |log post - log post64| / (ulp(log post64) + ulp(max |score| of the block))
floor: the split format's absolute floor (ffhip_split.hpp): 2^-29 for swish outputs at 2^4, 2^-37 for bounded ones at 2^12.
Bounds, from the formats (not fitted), in those units:
    fp32 VALU convolution of K = winlen * Fin taps     2K + 8 (K products, K sums, the activation), + 8 when it writes fp16 slices
    split convolution, NC = ceil(winlen / 2) chunks    4 (weight slices hold w to 2^-22) + 8 (dropped w1 x1 <= 2^-21 of a product)
                                                       + 6 NC (two roundings per MFMA, three MFMAs per chunk) + 8 (activation) + 8 (output slices)
    f32 MFMA convolution, K16 chunks of 16             32 K16 + 16
    split head, Hc = H / 32                            28 + 6 Hc;   f32 head: 2H + 16
    chains                                             8 (fp64 linear space; the stored scores are the chains' input rounded once)
A dropped split product (w0 x1 or w1 x0) costs ~2^-12 of every product: ~2^12 / sqrt(K) in these units on average over an
output (~240 at K = 304, ~180 for the head at H = 512), several times that at the worst element of a read -- above every bound
of a split form.  The measured worst of the kernel and of the fp32 oracle on the same input are printed (run with -s).
Records of the first MI355X run, kernel / fp32 oracle, worst normalised over every case:
    thin convolutions (small<4,5>, <16,20>, <4>, <16>, <32>)    3.87 / 3.87
    split last convolution (ws<10>, <4,4>)                      3.56 / 6.50   (bound 82 .. 94)
    f32 MFMA last convolution (mfma<true>, mfma<false>)         6.52 / 6.03
    heads (head_split<3|4>, head<3|4>, run-length)              0.97 / 1.20
    chains (k_crf_fb, 8 and 10 states, 20 000 blocks included) 1.66 / 107 (the oracle's fp32 log-space chains)
This test found k_conv_mfma carrying a NaN from the live samples behind a 19-tap window (the fragment's padding to 32 taps, zero
weights: 0 x NaN) into the column (GRUmod, one input feature); the padded elements now read as zero."""
import numpy as np
import pytest

import fp64_ref as R
from flappie_amd import model as M
from oracle import ffo

pytestmark = pytest.mark.gpu

EPS = R.F32_EPS
FLOOR_X, FLOOR_H = 2.0 ** -29, 2.0 ** -37


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


def note(key, kern, orac):
    k, o = SEEN.get(key, (0.0, 0.0))
    SEEN[key] = (max(k, kern), max(o, orac))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(SEEN):
        print("worst normalised error %-28s kernel %8.3f   fp32 oracle %8.3f" % (key, SEEN[key][0], SEEN[key][1]))


# ---- models ------------------------------------------------------------------------------------------------------------------
def custom_front(mdl, layers, seed):
    """replace the thin front of an LSTM model: layers = [(nfilter, winlen, stride)] in front of a last 16/32 -> H convolution"""
    rng = np.random.default_rng(seed)
    convs, nf = [], 1
    for nfilter, winlen, stride in layers:
        cm = M._conv_mat(rng, nf, nfilter, winlen)
        cm.data *= np.float32(3.0)
        convs.append(M.ConvLayer(cm, M.Mat.vector(rng.uniform(-0.1, 0.1, nfilter).astype(np.float32)), stride, nf, winlen))
        nf = nfilter
    last = mdl.convs[-1]
    winlen = last.winlen
    cm = M._conv_mat(rng, nf, mdl.hidden, winlen)
    cm.data *= np.float32(3.0)
    convs.append(M.ConvLayer(cm, last.b, last.stride, nf, winlen))
    mdl.convs = convs
    return mdl


def last_winlen(mdl, winlen, seed):
    rng = np.random.default_rng(seed)
    last = mdl.convs[-1]
    cm = M._conv_mat(rng, last.nf, mdl.hidden, winlen)
    cm.data *= np.float32(3.0)
    mdl.convs[-1] = M.ConvLayer(cm, last.b, last.stride, last.nf, winlen)
    return mdl


CASES = {
    # name: (model, run flags, expected forms, expected head form)
    "lstm128": (lambda: M.synthetic_model(M.NET_LSTM5, 128, seed=3), 0, ["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>"),
    "lstm256": (lambda: M.synthetic_model(M.NET_LSTM5, 256, seed=4), 0, ["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>"),
    "lstm384": (lambda: M.synthetic_model(M.NET_LSTM5, 384, seed=5), 0, ["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>"),
    "lstm512": (lambda: M.synthetic_model(M.NET_LSTM5, 512, seed=6), 0, ["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>"),
    "lstm256_f32": (lambda: M.synthetic_model(M.NET_LSTM5, 256, seed=4), 64, ["small<4,5>", "small<16,20>", "mfma<true>"], "head<3>"),
    "lstm256_w17": (lambda: last_winlen(M.synthetic_model(M.NET_LSTM5, 256, seed=8), 17, 8), 0, ["small<4,5>", "small<16,20>", "split<4,4>"], "head_split<3>"),
    "lstm256_w21": (lambda: last_winlen(M.synthetic_model(M.NET_LSTM5, 256, seed=9), 21, 9), 0, ["small<4,5>", "small<16,20>", "split<4,4>"], "head_split<3>"),
    "gru256": (lambda: M.synthetic_model(M.NET_GRUMOD5, 256, seed=10), 0, ["mfma<false>"], "head_split<4>"),
    "gru256_f32": (lambda: M.synthetic_model(M.NET_GRUMOD5, 256, seed=10), 64, ["mfma<false>"], "head<4>"),
    "thin32": (lambda: custom_front(M.synthetic_model(M.NET_LSTM5, 256, seed=11), [(4, 5, 1), (32, 5, 1)], 11), 0,
               ["small<4,5>", "small<32>", "mfma<true>"], "head_split<3>"),
    "generic": (lambda: custom_front(M.synthetic_model(M.NET_LSTM5, 256, seed=12), [(3, 7, 1), (16, 3, 1)], 12), 0,
                ["small<4>", "small<16>", "split_ws<10>"], "head_split<3>"),
}


def conv_bound(mdl, l, flags):
    """the format's bound of convolution l's kernel form (module docstring) and the floor of its output"""
    cv = mdl.convs[l]
    K = cv.winlen * cv.nf
    last = l == len(mdl.convs) - 1
    swish = mdl.kind != M.NET_GRUMOD5
    f32 = bool(flags & 64)
    if not last:
        slices = (l == len(mdl.convs) - 2) and cv.W.nc == 16 and mdl.convs[-1].nf == 16 and swish and not f32
        return 2 * K + 8 + (8 if slices else 0), (FLOOR_X if slices else 0.0)
    floor = 0.0 if f32 else (FLOOR_X if swish else FLOOR_H)
    if cv.nf == 16 and swish and not f32:
        return 28 + 6 * ((cv.winlen + 1) // 2), floor
    return 32 * (-(-K // 16)) + 16, floor


def conv_norm_err(got, x, cv, swish, floor):
    """normalised error of `got` against the float64 convolution + activation of x; the non-finite set is returned apart"""
    z, cond = R.conv_terms(np.asarray(x, dtype=np.float64), cv.taps(), cv.b.data[0, :cv.W.nc], cv.stride)
    f, df = R.activation(swish)
    with np.errstate(invalid="ignore", over="ignore"):
        want = f(z)
        fin = np.isfinite(z)
        denom = np.where(fin, np.abs(df(np.where(fin, z, 0.0))) * np.where(fin, cond, 0.0), 0.0) * EPS + \
            R.ulp32(np.where(np.isfinite(want), want, 0.0)) + (0.0 if swish else EPS) + floor
        ok = np.isfinite(want)
        err = np.where(ok, np.abs(got.astype(np.float64) - np.where(ok, want, 0.0)) / denom, 0.0)
    return err, ok, want


def oracle_conv(x, cv, swish):
    y = ffo.lib().fo_convolution(ffo.HostMat.from_dense(np.ascontiguousarray(x, dtype=np.float32)).ptr,
                                 ffo.HostMat.from_model_mat(cv.W).ptr, ffo.HostMat.from_model_mat(cv.b).ptr, cv.stride)
    (ffo.lib().fo_swish_inplace if swish else ffo.lib().fo_tanh_inplace)(y)
    return ffo.take(y)


def check_front(b, mdl, read, sig, flags, key):
    """every convolution of `read` against fp64 on its own input; returns the per-layer outputs"""
    swish = mdl.kind != M.NET_GRUMOD5
    x = sig.reshape(-1, 1)
    outs = []
    for l, cv in enumerate(mdl.convs):
        got = b.front(l, read)
        bound, floor = conv_bound(mdl, l, flags)
        err, ok, want = conv_norm_err(got, x, cv, swish, floor)
        assert got.shape == want.shape
        # the non-finite outputs are exactly the reference's (a NaN stays NaN, reaches every window that holds it and no other)
        assert np.array_equal(~np.isfinite(got), ~ok), "layer %d: non-finite outputs differ from the reference's" % l
        orac = oracle_conv(x, cv, swish)
        oerr, _, _ = conv_norm_err(orac, x, cv, swish, floor)
        note("%s conv%d" % (key, l), float(err.max()), float(oerr.max()))
        assert err.max() <= bound, "layer %d: worst normalised error %.2f above the format's bound %d" % (l, err.max(), bound)
        outs.append(got)
        x = got
    return outs


def check_head(b, mdl, read, temperature, key, bound):
    h = b.head_input(read)
    W, bias = mdl.FF_W.data[:, :mdl.hidden], mdl.FF_b.data[0, :mdl.nparam]
    got = b.transitions(read).astype(np.float64)
    nb = mdl.nbase
    if mdl.kind == M.NET_LSTM5_RLE:
        want, z, cond, logz = R.runlength_head(h, W, bias, temperature, nb)
        orac = ffo.take(ffo.lib().fo_globalnorm_runlengthV2(ffo.HostMat.from_dense(h).ptr, ffo.HostMat.from_model_mat(mdl.FF_W).ptr,
                                                             ffo.HostMat.from_model_mat(mdl.FF_b).ptr, temperature))
        S = np.hstack([want[:, :2 * nb], 5 * np.tanh(z[:, 2 * nb:]) / temperature])
        dS = np.empty_like(z)
        dS[:, :2 * nb] = cond[:, :2 * nb] * EPS + EPS + R.ulp32(want[:, :2 * nb])
        dS[:, 2 * nb:] = (5 / temperature) * (R.dtanh64(z[:, 2 * nb:]) * (cond[:, 2 * nb:] * EPS + FLOOR_H * np.abs(W[2 * nb:]).sum(1)) + EPS) + R.ulp32(S[:, 2 * nb:])
        extra = np.zeros_like(z)
        extra[:, 2 * nb:] = dS[:, 2 * nb:].max(axis=1).mean() + R.ulp32(logz / z.shape[0])
    else:
        want, S, z, cond, logz = R.flipflop_head(h, W, bias, temperature, nb)
        orac = ffo.take(ffo.lib().fo_globalnorm_flipflop(ffo.HostMat.from_dense(h).ptr, ffo.HostMat.from_model_mat(mdl.FF_W).ptr,
                                                         ffo.HostMat.from_model_mat(mdl.FF_b).ptr, temperature))
        dS = (5 / temperature) * (R.dtanh64(z) * (cond * EPS + FLOOR_H * np.abs(W).sum(1)) + EPS) + R.ulp32(S)
        extra = dS.max(axis=1).mean() + R.ulp32(logz / z.shape[0])
    denom = dS + extra + R.ulp32(want)
    err = np.abs(got - want) / denom
    oerr = np.abs(orac - want) / denom
    note("%s head T=%g" % (key, temperature), float(err.max()), float(oerr.max()))
    assert err.max() <= bound, "head: worst normalised error %.2f above the format's bound %d" % (err.max(), bound)


def check_chains(b, mdl, read, key):
    """Batch.posterior against the float64 forward-backward on the batch's own transitions"""
    trans = b.transitions(read).astype(np.float64)
    post64, _ = R.crf_posterior(trans, R.flipflop_map(mdl.nbase))
    with np.errstate(divide="ignore"):
        want = np.log(post64)
    got = b.posterior(read).astype(np.float64)
    denom = R.ulp32(want) + R.ulp32(np.abs(trans).max(axis=1, keepdims=True))
    err = np.abs(got - want) / denom
    orac = ffo.take(ffo.lib().fo_transpost(ffo.HostMat.from_dense(trans.astype(np.float32)).ptr, 1))
    note("%s chains" % key, float(err.max()), float((np.abs(orac - want) / denom).max()))
    assert err.max() <= 8, "chains: worst normalised error %.2f above 8" % err.max()


def head_bound(mdl, flags):
    H = mdl.hidden
    return (2 * H + 16) if flags & 64 else (28 + 6 * (H // 32))


def run_ragged(B, dm, sigs, flags=0, temperature=1.0, keep=True):
    b = B.Batch(dm, len(sigs), max(s.size for s in sigs))
    b.keep_front(keep)
    b.set_signals_ragged(sigs)
    b.run(temperature, flags)
    b.finish()
    return b


def shortest_read(mdl):
    """the fewest samples the reference's convolution takes (build_conv_plan): every layer sees at least one full window"""
    for T in range(1, 1000):
        t, ok = T, True
        for c in mdl.convs:
            padL, s = (c.winlen - 1) // 2, c.stride
            shiftX = -(-padL // s) * s - padL
            ok = ok and t >= c.winlen and t - shiftX - (c.winlen - 1) >= 0
            t = -(-t // s)
        if ok:
            return T


def read_lengths(mdl, base):
    """every residue of T modulo the total stride, the shortest legal read (one window), an odd T"""
    st = mdl.total_stride
    return [base + k for k in range(st)] + [shortest_read(mdl), base + 2 * st + 1]


@pytest.mark.parametrize("case", list(CASES))
def test_front_and_head_against_fp64(B, engine, case):
    """Each convolution form and head form of the table, asserted reached through Batch.forms(), on reads of every length residue,
    the shortest legal read and one with a NaN at its first and last sample and one inside (the NaN's windows and no others)."""
    make, flags, forms, head = CASES[case]
    mdl = make()
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(len(case) * 31)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in read_lengths(mdl, 1500)]
    nan = rng.standard_normal(1203).astype(np.float32)
    nan[0] = nan[-1] = nan[600] = np.nan
    sigs.append(nan)
    temps = (1.0, 0.8) if case in ("lstm256", "gru256") else (1.0,)
    for temperature in temps:
        b = run_ragged(B, dm, sigs, flags, temperature)
        assert b.forms() == (forms, head), b.forms()
        for r, s in enumerate(sigs):
            check_front(b, mdl, r, s, flags, case)
            if r < len(sigs) - 1:
                check_head(b, mdl, r, temperature, case, head_bound(mdl, flags))
                if temperature == 1.0:
                    check_chains(b, mdl, r, case)
        b.close()
    dm.close()


def test_split_forms_bit_identical(B, engine):
    """k_conv_split_ws<10>, <4, 4> and <2, 2> run the same products in the same order per accumulator (ffhip_kernels.hip): the same input
    gives the same bits.  <2, 2> is the form a batch's last convolution takes while another batch is between run and finish."""
    rng = np.random.default_rng(5)
    for make, fat in ((lambda: M.synthetic_model(M.NET_LSTM5, 256, seed=4), "split_ws<10>"),
                      (lambda: last_winlen(M.synthetic_model(M.NET_LSTM5, 256, seed=8), 17, 8), "split<4,4>")):
        mdl = make()
        dm = B.DeviceModel(engine, mdl)
        sig = rng.standard_normal((20, 3001)).astype(np.float32)
        b0, b1 = B.Batch(dm, 20, 3001), B.Batch(dm, 20, 3001)
        for b in (b0, b1):
            b.keep_front(True)
            b.set_signals(sig)
        b0.run()
        b1.run()                       # b0 is in flight: b1's last convolution takes the lean form
        b0.finish(); b1.finish()
        assert b0.forms()[0][-1] == fat and b1.forms()[0][-1] == "split<2,2>", (b0.forms(), b1.forms())
        for r in range(20):
            assert np.array_equal(b0.front(2, r).view(np.uint32), b1.front(2, r).view(np.uint32))
            assert np.array_equal(b0.transitions(r), b1.transitions(r))
        b0.close(); b1.close(); dm.close()


def _packed(B, dm, sigs, rows, nsample):
    b = B.Batch(dm, rows, nsample, max_reads=len(sigs))
    b.keep_front(True)
    slot, off = b.pack_plan([s.size for s in sigs])
    assert min(slot) >= 0
    b.set_signals_packed(sigs, slot, off)
    b.run()
    b.finish()
    return b, slot, off


def test_packed_rows(B, engine):
    """Packed rows of mixed lengths: each read's columns of every convolution equal the read alone (a ragged batch) bit for bit, every
    column of a thin layer outside a read is exactly 0 (the next convolution's padding), head and chains against fp64 on the packed
    batch's own inputs, and a NaN at a read's first and last sample turns exactly the reference's outputs non-finite and changes no
    neighbour in the row."""
    mdl = M.synthetic_model(M.NET_LSTM5, 256, seed=4)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(17)
    lens = [3000, 95, 1234, 2001, 777, 96, 1500, 2999, 500, 1003]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    b, slot, off = _packed(B, dm, sigs, 5, 4000)
    assert b.forms() == (["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>")
    alone = run_ragged(B, dm, sigs)
    for r, s in enumerate(sigs):
        for l in range(3):
            assert np.array_equal(b.front(l, r).view(np.uint32), alone.front(l, r).view(np.uint32)), "read %d layer %d" % (r, l)
        check_front(b, mdl, r, s, 0, "packed")
        check_head(b, mdl, r, 1.0, "packed", head_bound(mdl, 0))
        check_chains(b, mdl, r, "packed")
    for row in range(5):
        for l in range(2):
            full = b.front_row(l, row)
            inside = np.zeros(full.shape[0], dtype=bool)
            for r in range(len(sigs)):
                if slot[r] == row:
                    _, c0, n = b._span(l, r)
                    inside[c0:c0 + n] = True
            assert not full[~inside].any(), "row %d layer %d: a column outside every read is not 0" % (row, l)
    clean = {r: [b.front(l, r) for l in range(3)] for r in range(len(sigs))}
    alone.close(); b.close()
    # NaN at the first and last sample of two reads
    bad = [2, 6]
    sigs2 = [s.copy() for s in sigs]
    for r in bad:
        sigs2[r][0] = sigs2[r][-1] = np.nan
    b, slot2, off2 = _packed(B, dm, sigs2, 5, 4000)
    assert (slot2, off2) == (slot, off)
    for r, s in enumerate(sigs2):
        if r in bad:
            check_front(b, mdl, r, s, 0, "packed nan")
        else:
            for l in range(3):
                assert np.array_equal(b.front(l, r).view(np.uint32), clean[r][l].view(np.uint32)), "neighbour %d changed at layer %d" % (r, l)
    b.close(); dm.close()


def test_f32_path_inf_at_read_edges(B, engine):
    """The f32 path (no split format, no clamp): an inf at a read's first and last sample makes exactly the reference's outputs non-finite"""
    mdl = M.synthetic_model(M.NET_LSTM5, 256, seed=4)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(3)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (1500, 1001)]
    sigs[1][0], sigs[1][-1] = np.inf, -np.inf
    b = run_ragged(B, dm, sigs, flags=64)
    for r, s in enumerate(sigs):
        check_front(b, mdl, r, s, 64, "lstm256_f32 inf")
    b.close(); dm.close()


def test_clamp_of_the_split_format(B, engine):
    """A swish output beyond the split format's range reads back as exactly +-4094 (ffhip_split.hpp), and the read goes round the f32 path
    again (its row's `sat` word)"""
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=3)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(9)
    sig = rng.standard_normal(2000).astype(np.float32)
    sig[900:1000] *= 3000.0
    b = run_ragged(B, dm, [sig, rng.standard_normal(2000).astype(np.float32)])
    assert b.f32_reruns() == 1
    x = sig.reshape(-1, 1)
    for l, cv in enumerate(mdl.convs):
        got = b.front(l, 0)
        z, _ = R.conv_terms(x.astype(np.float64), cv.taps(), cv.b.data[0, :cv.W.nc], cv.stride)
        want = R.swish64(z)
        if l >= 1:
            big = np.abs(want) >= 4094.0 * (1 + 2.0 ** -20)
            assert big.any()
            assert np.array_equal(got[big], np.sign(want[big]).astype(np.float32) * np.float32(4094.0))
        x = got
    assert np.isfinite(b.transitions(0)).all()
    b.close(); dm.close()


def test_keep_front_changes_nothing(B, engine):
    """keep_front on and off: every result bit for bit the same, and the same kernel forms"""
    for kind, H in ((M.NET_LSTM5, 256), (M.NET_GRUMOD5, 256), (M.NET_LSTM5_RLE, 256)):
        mdl = M.synthetic_model(kind, H, seed=2)
        dm = B.DeviceModel(engine, mdl)
        rng = np.random.default_rng(4)
        sigs = [rng.standard_normal(n).astype(np.float32) for n in (2000, 1003, 95)]
        res = []
        for keep in (False, True):
            b = run_ragged(B, dm, sigs, keep=keep)
            res.append((b.forms(), [(b.transitions(r), b.posterior(r), b.path(r)[0], b.score(r)) for r in range(3)]))
            b.close()
        assert res[0][0] == res[1][0]
        for a, c in zip(res[0][1], res[1][1]):
            for u, v in zip(a, c):
                assert np.array_equal(u, v)
        dm.close()


def test_runlength_head_against_fp64(B, engine):
    """the run-length model: k_head_split's raw epilogue, then the head finish (shape, scale, transitions, normalisation), packed rows included"""
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 256, seed=13)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(13)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (1500, 1001, 95)]
    b = run_ragged(B, dm, sigs)
    assert b.forms() == (["small<4,5>", "small<16,20>", "split_ws<10>"], "head_split<3>")
    for r in range(3):
        check_head(b, mdl, r, 1.0, "rle", head_bound(mdl, 0))
    b.close()
    b, _, _ = _packed(B, dm, sigs + [s[::-1].copy() for s in sigs], 2, 4000)
    for r in range(6):
        check_head(b, mdl, r, 1.0, "rle packed", head_bound(mdl, 0))
    b.close(); dm.close()


@pytest.mark.parametrize("kind", [M.NET_LSTM5, M.NET_GRUMOD5])
def test_chains_one_window_and_long(B, engine, kind):
    """8 and 10 states; a one-window read; a 100 000-sample read at H = 256 (20 000 blocks of the rescaled linear-space chains)"""
    mdl = M.synthetic_model(kind, 256, seed=21)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(21)
    n_long = 100000 if kind == M.NET_LSTM5 else 40000
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (n_long, shortest_read(mdl))]
    b = run_ragged(B, dm, sigs, keep=False)
    for r in range(2):
        check_chains(b, mdl, r, "chains nstate=%d" % mdl.nstate)
    b.close(); dm.close()
