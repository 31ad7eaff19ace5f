"""The per-read feature kernels on input no network emits but a caller of the C API may pass (hostile_scores.py): NaN, +-inf, ties everywhere, constant
matrices, +-3e38 -- k_remap, k_site_mods, k_variants, k_events and k_polytail through their operators, held to the statements of include/ffhip.h as the
restatements give them, and one batch with every per-read feature and a read that is NaN throughout.

  * remap: mapped iff the score V_N[L - 1] is finite (remap_ref.remap_status).  A mapped read's score bits and path are the restatement's at all four kernel
    forms; a read that is not mapped is FFHIP_EINVAL from the operator, never FFHIP_EHIP, and the engine goes on;
  * site mods and variants: best path to the bit with the strict compare, NaN for NaN; all paths by the IEEE arithmetic as written: the same NaN pattern, +-inf
    equal, finite values within 1 float32 ulp; on flat and quantised scores every path of small windows enumerated;
  * events and poly tail: one poisoned sample changes the events and windows that hold it, in the way the two-pass fp64 statement says, and nothing else;
  * a batch: no accessor reports a device error for a property of the input, and the other reads' bytes do not depend on the NaN read.
Nothing here is meant to fault: these are ordinary arguments with defined results."""
import ctypes as C
import functools

import numpy as np
import pytest

from flappie_amd import model as M
import events_ref as E
import hostile_scores as H
import moves_ref as MV
import polytail_ref as PT
import remap_ref as R
import sitemods_ref as S
import truth_ref as TR
import variants_ref as V
from test_polytail_gpu import _read_of_flags
from test_truth_gpu import same_record
from test_variants_gpu import _letters, _variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ------------------------------------------------------------------------------------ remap
def _remap_tally(shapes):
    """per style [mapped, not mapped], per kernel form likewise: the REFERENCE's outcomes"""
    styles, forms = {s: [0, 0] for s in H.STYLES}, {f: [0, 0] for f in range(4)}
    for N, L in shapes:
        for (style, nbase, W), (T, s, status, score, rm) in H.remap_reference(N, L).items():
            styles[style][status - 1] += 1
            forms[H.form(L, W)][status - 1] += 1
    return styles, forms


def test_remap_sweep_holds_both_outcomes_for_every_sparse_style_and_form():
    styles, forms = _remap_tally(H.REMAP_SHAPES)
    print("remap, the reference's [mapped, not mapped] per style:", styles)
    print("remap, the reference's [mapped, not mapped] per kernel form:", forms)
    for style in H.SPARSE:
        assert min(styles[style]) >= 1, (style, styles)
    for f in range(4):
        assert min(forms[f]) >= 1, (f, forms)


@pytest.mark.parametrize("N,L", H.REMAP_SHAPES)
def test_remap_maps_iff_the_score_is_finite(B, engine, N, L):
    rng = np.random.default_rng(3)
    T0, s0 = rng.standard_normal((8, 40)).astype(np.float32), np.array([0, 1, 1, 3], np.uint8)
    score0, rm0 = R.remap(T0, s0, 4, 16)
    for (style, nbase, W), (T, s, status, score, rm) in H.remap_reference(N, L).items():
        where = (style, nbase, N, L, W)
        assert B.lib().ffhip_debug_remap_form(C.c_size_t(L), W) == H.form(L, W), where
        if status == 1:
            grm, gscore = B.op_remap(engine, T, nbase, s, W)
            assert bits(gscore) == bits(score), (where, float(gscore), float(score))
            assert np.array_equal(grm, rm), (where, np.flatnonzero(grm != rm)[:6])
            assert int(grm.sum()) == L - 1 and R.starts_maxdev(grm, L)[1] <= W, where
        else:
            with pytest.raises(B.FFHipError) as e:
                B.op_remap(engine, T, nbase, s, W)
            assert "ffhip error -1:" in str(e.value) and "score" in str(e.value), (where, str(e.value))      # FFHIP_EINVAL, not FFHIP_EHIP (-3)
            grm, gscore = B.op_remap(engine, T0, 4, s0, 16)                                                  # the engine is usable
            assert bits(gscore) == bits(score0) and np.array_equal(grm, rm0), where


# ------------------------------------------------------------------------------------ site mods and variants
SITE_SHAPES = ((300, 120), (65, 40))
SITE_CONTEXTS = (0, 3, 15, 31)
VARIANT_CONTEXTS = (1, 10, 23)


@functools.lru_cache(maxsize=None)
def _read(N, L, nbase):
    """a finite base matrix, a sequence and ITS remap path by the restatement: the poison goes in afterwards, so the path is valid whatever the scores"""
    seed = 77000 + 10 * N + nbase
    rng = np.random.default_rng(seed)
    codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L) if nbase == 5 else _letters(rng, nbase, L)
    T = H.base_scores(seed, N, nbase)
    return seed, codes, R.remap(T, codes, nbase, 2048)[1], tuple(_variants(np.random.default_rng(seed + 1), codes, nbase, 4))


@functools.lru_cache(maxsize=None)
def _site_reference(style, N, L, c, mode):
    seed, codes, rm, _ = _read(N, L, 5)
    T = H.styled(style, seed, N, 5)
    return T, codes, rm, S.site_mods(T, 5, codes, rm, c, mode)


@functools.lru_cache(maxsize=None)
def _variant_reference(style, N, L, nbase, c, mode):
    seed, codes, rm, vars = _read(N, L, nbase)
    T = H.styled(style, seed, N, nbase)
    return T, codes, rm, list(vars), V.variants(T, nbase, codes, rm, list(vars), c, mode)


def _kinds(values):
    v = np.asarray(values, np.float32)
    return np.array([int(np.isnan(v).sum()), int(np.isneginf(v).sum()), int(np.isfinite(v).sum())])


def test_variant_lists_hold_every_kind_of_edit():
    """substitutions, insertions and deletions for every read, and over the reads an alt with more positions than its window has blocks (no path: -inf from
    finite scores)"""
    no_path = 0
    for N, L in SITE_SHAPES:
        for nbase in (4, 5):
            seed, codes, rm, vars = _read(N, L, nbase)
            assert any(r == len(alt) >= 1 for p, r, alt in vars) and any(r == 0 for p, r, alt in vars) and any(not alt for p, r, alt in vars), (N, L, nbase)
            no_path += int(np.isneginf(V.variants(H.base_scores(seed, N, nbase), nbase, codes, rm, list(vars), 1)["alt"]).sum())
    assert no_path >= 1


@pytest.mark.parametrize("style", H.STYLES)
def test_site_mods_on_hostile_scores(B, engine, style):
    count = {False: np.zeros(3, int), True: np.zeros(3, int)}
    for N, L in SITE_SHAPES:
        for c in SITE_CONTEXTS:
            for mode in (False, True):
                T, codes, rm, want = _site_reference(style, N, L, c, mode)
                got = B.op_site_mods(engine, T, 5, codes, rm, c, mode, (60, 64)[c % 2])
                S.check_hostile(got, want, mode, (style, N, L, c, mode))
                if np.isfinite(T).all() or np.all((T == -np.inf) | np.isfinite(T)):
                    S.check(got, want, mode, (style, N, L, c, mode))      # finite or -inf scores: never a NaN
                count[mode] += _kinds(want["can"]) + _kinds(want["mod"])
    print("site mods, %s: the reference's [NaN, -inf, finite] scores, best path %s, all paths %s" % (style, count[False].tolist(), count[True].tolist()))


@pytest.mark.parametrize("style", H.STYLES)
def test_variants_on_hostile_scores(B, engine, style):
    count = {False: np.zeros(3, int), True: np.zeros(3, int)}
    for N, L in SITE_SHAPES:
        for nbase in (4, 5):
            ns = 2 * nbase * (nbase + 1)
            for c in VARIANT_CONTEXTS:
                for mode in (False, True):
                    T, codes, rm, vars, want = _variant_reference(style, N, L, nbase, c, mode)
                    got = B.op_variants(engine, T, nbase, codes, rm, V.pack(vars), c, mode, (ns, 64)[c % 2])
                    V.check_hostile(got, want, mode, (style, N, L, nbase, c, mode))
                    if np.all((T == -np.inf) | np.isfinite(T)):
                        V.check(got, want, mode, (style, N, L, nbase, c, mode))
                    count[mode] += _kinds(want["ref"]) + _kinds(want["alt"])
    print("variants, %s: the reference's [NaN, -inf, finite] scores, best path %s, all paths %s" % (style, count[False].tolist(), count[True].tolist()))


def test_site_scores_of_poisoned_matrices_hold_nan_neg_inf_and_finite_in_both_modes():
    """the sweeps above are worth their name only if the reference's own results are of every kind: from POISONED matrices, in either mode and for either operator,
    at least one NaN, one -inf and one finite score (here on the part of the sweep that settles it: N = 300, L = 120)"""
    for mode in (False, True):
        sm, vr = np.zeros(3, int), np.zeros(3, int)
        for style in ("nan 0.1%", "nan 5%", "-inf 5%"):
            for c in (3, 15):
                want = _site_reference(style, 300, 120, c, mode)[3]
                sm += _kinds(want["can"]) + _kinds(want["mod"])
            want = _variant_reference(style, 300, 120, 4, 10, mode)[4]
            vr += _kinds(want["ref"]) + _kinds(want["alt"])
        print("mode all paths" if mode else "mode best path", "site mods [NaN, -inf, finite]", sm.tolist(), "variants", vr.tolist())
        assert sm.min() >= 1 and vr.min() >= 1, (mode, sm, vr)


def test_every_path_of_small_windows_on_flat_and_quantised_scores(B, engine):
    """flat and quarter-quantised scores: every sum is exact, ties abound.  Windows of at most 12 blocks: the recursion, the kernel and the enumeration of every
    monotone path agree -- best path to the bit, all paths within 1e-9 (restatement) and 1 float32 ulp (kernel)"""
    n = 0
    for style in ("flat", "quantised"):
        for N, L in SITE_SHAPES:
            seed, codes, rm, _ = _read(N, L, 5)
            T = H.styled(style, seed, N, 5)
            st = S.starts(rm, L)
            for c in (0, 1, 2):
                best, every = (B.op_site_mods(engine, T, 5, codes, rm, c, mode) for mode in (False, True))
                for k, i in enumerate(S.sites(codes)):
                    lo, hi, t0, t1 = S.window(st, L, i, c)
                    if t1 - t0 > 12:
                        continue
                    for f, letter in (("can", S.CAN), ("mod", S.MOD)):
                        q = S.code_hypothesis(codes, i, letter, 5)
                        bbest, blog = S.brute(T, q, lo, hi, t0, t1, 5)
                        where = (style, N, L, c, i, f)
                        assert best[k]["pos"] == i and best[k][f].tobytes() == bbest.tobytes() == S.score_best(T, q, lo, hi, t0, t1, 5).tobytes(), where
                        assert abs(float(S.score_all(T, q, lo, hi, t0, t1, 5)) - blog) <= 1e-9, where
                        assert abs(float(every[k][f]) - float(np.float32(blog))) <= S.ulp32(np.float32(blog)), (where, every[k][f], blog)
                        n += 1
    assert n >= 200, n


# ------------------------------------------------------------------------------------ events
POISON = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(3e38))


def _events_read():
    """300 bases of 1 .. 3 blocks at stride 5 (spans of at most 15 samples: a thread's own), two of 20 blocks (100 samples: the whole wave's), one of each in
    either round of 256 bases; the read ends 3 samples inside its last block (the last span is clipped)"""
    rng = np.random.default_rng(21)
    lengths = rng.integers(1, 4, 300)
    lengths[[10, 270]] = 20
    rm = E.rm_of_lengths([int(k) for k in lengths])
    x = (100.0 + 10.0 * rng.standard_normal(rm.size * 5 - 3)).astype(np.float32)
    return x, rm, 300, {"short": (5, 290), "wave": (10, 270), "clipped": (299,)}


def test_events_with_one_poisoned_sample(B, engine):
    x, rm, L, places = _events_read()
    clean = B.op_events(engine, x, 5, rm, L)
    E.check(clean, E.events(x, 5, rm, L), x, "clean")
    assert clean["count"][299] == 5 * (rm.size - 1 - int(np.flatnonzero(rm)[-1])) - 3 and clean["count"][10] == 100 and clean["count"][:10].max() <= 32
    seen = np.zeros(3, int)
    for value in POISON:
        for place, bases in places.items():
            for i in bases:
                for at in sorted({0, int(clean["count"][i]) // 2, int(clean["count"][i]) - 1}):
                    y = x.copy()
                    y[int(clean["first"][i]) + at] = value
                    with np.errstate(invalid="ignore", over="ignore"):
                        want = E.events(y, 5, rm, L)
                    got = B.op_events(engine, y, 5, rm, L)
                    where = (float(value), place, i, at)
                    E.check_hostile(got, want, y, where)
                    others = np.arange(L) != i
                    assert got[others].tobytes() == clean[others].tobytes(), where      # a span without the sample: the bytes of the clean run
                    assert got["first"][i] == clean["first"][i] and got["count"][i] == clean["count"][i], where
                    if np.isfinite(value):
                        assert np.isfinite(got["mean"][i]) and np.isfinite(got["sd"][i]) and got["sd"][i] > 1e30, (where, got[i])
                    else:                   # the two-pass statement: the mean is the sample's kind, and x - mean is NaN at that sample at the latest
                        assert (np.isnan(got["mean"][i]) if np.isnan(value) else got["mean"][i] == value) and np.isnan(got["sd"][i]), (where, got[i])
                    seen += _kinds([want["mean"][i], want["sd"][i]])
    print("events: the poisoned spans' [NaN, -inf, finite] means and sds in the reference:", seen.tolist())
    assert seen.min() >= 1, seen


# ------------------------------------------------------------------------------------ poly tail
def _polytail_check(got, want, x, flag, K, S_, where):
    """polytail_ref.check's rule with the level's bound taken over the samples the level is made of: the interval's FLAGGED windows (a poisoned window inside a
    merged interval is not flagged and adds nothing)"""
    for f in ("status", "first", "count", "flat", "calls"):
        assert int(got[f]) == int(want[f]), (where, f, got, want)
    for f in ("rate", "bases"):
        assert got[f].tobytes() == np.asarray(want[f]).tobytes(), (where, f, got, want)
    if int(want["status"]) in (1, 3):
        ws, we = int(want["first"]) // (K * S_), (int(want["first"]) + int(want["count"])) // (K * S_)
        top = max(float(np.abs(x[w * K * S_:(w + 1) * K * S_].astype(np.float64)).max()) for w in range(ws, we) if flag[w])
        assert abs(float(got["level"]) - float(want["level"])) <= 2.0 ** -23 * top, (where, got, want)
    else:
        assert got["level"].tobytes() == b"\0\0\0\0", (where, got)


def test_polytail_with_poisoned_windows(B, engine):
    rng = np.random.default_rng(31)
    K, S_ = 2, 5
    flags = np.array([0] * 3 + [1] * 12 + [0] * 5 + [1] * 5 + [0] * 3)
    x, path = _read_of_flags(rng, flags, K, S_, tail_blocks=30)
    seen = set()
    for gap in (2, 0):
        p = PT.params(window=K, min_calls=K, gap=gap, min_windows=3, search=10 ** 6, min_bases=5, max_sd=0.01)
        cmu, cq, cflag = B.op_polytail_windows(engine, x, S_, path, 4, **p)
        assert np.array_equal(cflag[:flags.size], flags) and not cflag[flags.size:].any()
        clean = B.op_polytail(engine, x, S_, path, 4, **p)
        assert (int(clean["status"]), int(clean["first"]), int(clean["count"])) == (1, 3 * K * S_, 12 * K * S_)
        for value in POISON:
            # one window inside the winner (gap 2: bridged, one flat window fewer; gap 0: the winner is split); one that was not flagged; the winner's first; every window
            for windows in ((8,), (1,), (3,), (8, 9, 10), tuple(range(cflag.size))):
                y = x.copy()
                for w in windows:
                    y[w * K * S_ + (w % (K * S_))] = value
                with np.errstate(invalid="ignore", over="ignore"):
                    mu, q, flag, _ = PT.windows(y, S_, path, 4, p)
                    want = PT.record(y, S_, path, 4, p)
                where = (gap, float(value), windows)
                gmu, gq, gflag = B.op_polytail_windows(engine, y, S_, path, 4, **p)
                hit = np.zeros(cflag.size, bool)
                hit[list(windows)] = True
                assert not gflag[hit].any() and np.array_equal(gflag[~hit], cflag[~hit]) and np.array_equal(gflag, flag), where      # only the poisoned ones, unflagged
                assert gmu[~hit].tobytes() == cmu[~hit].tobytes() and gq[~hit].tobytes() == cq[~hit].tobytes(), where
                for g, w in ((gmu, mu), (gq, q)):           # the poisoned windows too: NaN where the statement's sums are, the same value elsewhere
                    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)]), where
                _polytail_check(B.op_polytail(engine, y, S_, path, 4, **p), want, y, flag, K, S_, where)
                seen.add((gap, len(windows), int(want["status"]), int(want["first"]) // (K * S_), (int(want["first"]) + int(want["count"])) // (K * S_), int(want["flat"])))
    assert (2, 1, 1, 3, 15, 11) in seen and (0, 1, 1, 9, 15, 6) in seen, sorted(seen)      # bridged with one flat window fewer; split, the longer part wins
    assert (2, 3, 1, 3, 8, 5) in seen, sorted(seen)                                          # three in a row at gap 2: split
    assert any(k[1] == cflag.size and k[2] == 2 for k in seen), sorted(seen)                 # every window poisoned: no tail found


# ------------------------------------------------------------------------------------ one batch with every per-read feature
def _codes(call, nbase):
    return np.array(["ACGTZ".index(x) for x in call], np.uint8) if call else np.array([1], np.uint8)


def _snapshot(B, b, v, nbase):
    """everything the per-read features return for read v, as bytes where it can be; an accessor that fails raises"""
    rec = b.remap(v)
    ev, vc = b.events(v), b.variant_calls(v)
    sm = b.site_mods(v) if nbase == 5 else None
    tr = b.truth(v)
    path, qpath = b.path(v)
    return dict(remap=(rec["status"], rec["L"], bits(rec["score"]), None if rec["rm"] is None else rec["rm"].tobytes()), events=None if ev is None else ev.tobytes(),
                site_mods=None if sm is None else sm.tobytes(), variants=None if vc is None else vc.tobytes(), polytail=b.polytail(v).tobytes(), moves=b.moves(v).tobytes(),
                truth=tuple(tr[f] for f in TR.FIELDS) + (None if tr["ops"] is None else tr["ops"].tobytes(),), call=b.basecall(v), qual=b.quality(v),
                path=path.tobytes(), qpath=qpath.tobytes(), trans=b.transitions(v).tobytes())


@pytest.mark.parametrize("kind,nbase", [(M.NET_GRUMOD5, 5), (M.NET_LSTM5, 4)])
def test_batch_with_a_nan_read_and_every_per_read_feature(B, engine, kind, nbase):
    mdl = M.synthetic_model(kind, 128, seed=1)
    stride, BAND, NANREAD = mdl.total_stride, 64, 3
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(17 + nbase)
    clean_sig = rng.standard_normal((8, 1500)).astype(np.float32)
    clean_sig[:, 200:575] = np.float32(0.3)                  # (a flat stretch: the poly tail's windows have something to flag)
    nan_sig = clean_sig.copy()
    nan_sig[NANREAD] = np.nan
    ptp = dict(window=8, min_calls=0, max_sd=1e-3, min_windows=2, gap=2, min_bases=1, search=10 ** 6)
    flags = B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_EVENTS | B.RUN_REMAP_VARIANTS | B.RUN_POLYTAIL | B.RUN_MOVES | B.RUN_TRUTH | (B.RUN_REMAP_MODS if nbase == 5 else 0)
    statuses = set()
    for layout in ("rows", "packed"):
        def batch(sig):
            if layout == "rows":
                b = B.Batch(dm, 8, 1500)
                b.set_signals(sig)
            else:
                b = B.Batch(dm, 4, 3200, max_reads=8)         # (two reads and the free blocks behind each a row)
                slot, off = b.pack_plan([1500] * 8)
                assert min(slot) >= 0 and len(set(slot)) < 8, "every read placed, several to a row"
                b.set_signals_packed(list(sig), slot, off)
            return b
        b = batch(clean_sig)
        b.run(1.0, B.RUN_NO_TRACE)
        b.finish()
        seqs = [_codes(b.basecall(v), nbase) for v in range(8)]      # the clean run's own calls
        vars = [_variants(np.random.default_rng(900 + v), q, nbase, 3) for v, q in enumerate(seqs)]
        shots = {}
        for name, sig in (("clean", clean_sig), ("nan", nan_sig)):
            if name == "nan":
                b.close()
                b = batch(sig)
            b.set_remap(seqs, BAND)
            b.set_truth(seqs, BAND)
            b.set_remap_variants([V.pack(v) for v in vars], 10, True)
            if nbase == 5:
                b.set_remap_mods(15, True)
            b.set_polytail(**ptp)
            b.run(1.0, flags)
            b.finish()
            shots[name] = [_snapshot(B, b, v, nbase) for v in range(8)]      # (no accessor raised: none returned FFHIP_EHIP)
        for v in range(8):
            if v != NANREAD:
                for key in shots["nan"][v]:
                    assert shots["nan"][v][key] == shots["clean"][v][key], (layout, v, key)      # byte for byte those of the batch without the NaN read
                assert shots["nan"][v]["remap"][0] == 1, (layout, v)
        # the NaN read: every record against the restatements on this run's own transitions, path and signal
        v, where = NANREAD, (layout, kind)
        trans, (path, _), seq = b.transitions(v), b.path(v), seqs[NANREAD]
        got = b.remap(v)
        status, score, rm = R.remap_status(trans, seq, nbase, BAND) if seq.size <= trans.shape[0] + 1 else (2, np.float32(0.0), None)
        statuses.add((status, bool(np.isnan(trans).any())))
        assert got["status"] == status and got["L"] == seq.size and bits(got["score"]) == bits(score), (where, got, status, score)
        ev, vc, sm = b.events(v), b.variant_calls(v), b.site_mods(v) if nbase == 5 else None
        if status == 1:
            assert np.array_equal(got["rm"], rm), where
            with np.errstate(invalid="ignore", over="ignore"):
                E.check_hostile(ev, E.events(nan_sig[v], stride, rm, seq.size), nan_sig[v], where)
            assert np.isnan(ev["mean"][ev["count"] > 0]).all() and np.isnan(ev["sd"][ev["count"] > 0]).all(), where
            V.check_hostile(vc, V.variants(trans, nbase, seq, rm, vars[v], 10, True), True, where)
            if nbase == 5:
                S.check_hostile(sm, S.site_mods(trans, 5, seq, rm, 15, True), True, where)
        else:
            assert got["rm"] is None and ev is None and vc is None and sm is None, where
        with np.errstate(invalid="ignore", over="ignore"):
            want = PT.record(nan_sig[v], stride, path, nbase, PT.params(**ptp))
        assert int(want["status"]) == 2 and b.polytail(v).tobytes() == want.tobytes(), (where, b.polytail(v), want)      # every window holds NaN: no tail found
        assert np.array_equal(b.moves(v), MV.moves(path)), where
        same_record(b.truth(v), TR.truth(b.basecall(v), seq, BAND), where)
        b.close()
    print("batch, nbase %d: the NaN read's (remap status, NaN among its transitions) by layout:" % nbase, sorted(statuses))
    dm.close()
