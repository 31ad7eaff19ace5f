"""flappie --remap-variants on the GPU: the scores of a mapped sequence as given and as edited by k_variants (include/ffhip.h FFHIP_RUN_REMAP_VARIANTS,
ffhip_batch_set_remap_variants, ffhip_batch_variant_calls, ffhip_op_variants).

  * the operator against the restatement (variants_ref.py) for both alphabets, at every wave and chunk edge, at both strides of a block's scores, with one base,
    with a base a block (insertions without a path), with every kind of edit, alleles of 16 and windows of 62 positions in either hypothesis, with scores of
    -1e30, with one base of 5000 blocks inside a window; its identities with ffhip_op_site_mods and ffhip_op_remap; the refusals;
  * on synthetic models, every read's records against the operator on the batch's OWN transitions and path, byte for byte in both modes -- one read a row,
    ragged, packed, launch per step, paired, f32 re-run -- and the same bytes wherever the transitions and the path are the same; nothing for status 0 and 2;
    remap, events and site mods unchanged by the flag; one more device-to-host copy call a batch, the buffers counted;
  * the flag's refusals; the binary's calls.tsv against the batch API's records.
Best-path scores are equal to the bit; all-paths scores are within 1 float32 ulp of the fp64 restatement (the rule of k_site_mods<true>) and never a NaN."""
import ctypes as C

import numpy as np
import pytest

from flappie_amd import model as M
import remap_ref as RR
import sitemods_ref as S
import variants_ref as V
from test_remap_gpu import _d2h_calls, _same, _state

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


def _path(rng, N, L):
    rm = np.zeros(N, np.uint8)
    rm[rng.choice(N, L - 1, replace=False)] = 1
    return rm


def _letters(rng, nbase, L):
    """runs of equal letters are common, and so are C and Z where the alphabet has Z"""
    q = rng.integers(0, nbase, L).astype(np.uint8)
    rep = rng.random(L) < 0.4
    for i in range(1, L):
        if rep[i]:
            q[i] = q[i - 1]
    return q


def _variants(rng, codes, nbase, extra=6):
    """every kind of edit that fits the sequence: SNP, MNP, insertions (at 0 and at L), deletions (at either end), edits inside runs, ref = alt, alleles of 16"""
    L = len(codes)
    s = [int(x) for x in codes]
    mid = L // 2
    run = max(range(L), key=lambda i: (i > 0 and s[i] == s[i - 1]) + (i + 1 < L and s[i] == s[i + 1]))      # inside a run, if there is one
    other = lambda x: (x + 1 + int(rng.integers(0, nbase - 1))) % nbase
    cand = [(mid, 1, [other(s[mid])]), (mid, 1, [s[mid]]), (0, 1, [other(s[0])]), (L - 1, 1, [other(s[-1])]),
            (mid, 2, [other(x) for x in s[mid:mid + 2]]), (mid, 3, s[mid:mid + 3][::-1]),
            (0, 0, [s[0]]), (0, 0, [other(s[0]), 1]), (L, 0, [s[-1]]), (L, 0, [0, 1, 2]), (mid, 0, [s[mid]] * 2),
            (0, 1, []), (0, 2, []), (L - 1, 1, []), (L - 2, 2, []), (mid, 1, []),
            (run, 1, []), (run, 0, [s[run]]), (run, 1, [other(s[run])]), (run, 1, [s[run]] * 2),
            (mid, 1, [int(x) for x in rng.integers(0, nbase, 16)]), (mid, 16, [other(s[mid])]), (max(0, mid - 8), 16, []), (mid, 16, [int(x) for x in rng.integers(0, nbase, 16)]),
            (mid, 0, [s[mid]] * 16), (23, 16, [other(s[min(23, L - 1)])]), (23, 0, [int(x) for x in rng.integers(0, nbase, 16)])]      # (c = 23: windows of 62 positions)
    for _ in range(extra):
        p = int(rng.integers(0, L + 1))
        r = int(rng.integers(0, min(4, L - p) + 1))
        cand.append((p, r, [int(x) for x in rng.integers(0, nbase, int(rng.integers(0, 4)))]))
    return [v for v in cand if V.valid(L, nbase, *v)]


def _both_modes(B, engine, T, nbase, codes, rm, vars, c, stride, where):
    for mode in (False, True):
        got = B.op_variants(engine, T, nbase, codes, rm, V.pack(vars), c, mode, stride)
        V.check(got, V.variants(T, nbase, codes, rm, vars, c, mode), mode, (where, c, mode, stride))
    return got


# ------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("nbase", [4, 5])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1500])
def test_operator_against_the_restatement(B, engine, N, nbase):
    rng = np.random.default_rng(700 + 10 * N + nbase)
    ns = 2 * nbase * (nbase + 1)
    k, no_path, widest = 0, 0, [0, 0]
    for L in sorted({1, N + 1, int(rng.integers(1, N + 2)), int(rng.integers(1, min(N + 1, 40) + 1))}):
        codes, rm = _letters(rng, nbase, L), _path(rng, N, L)
        T = (rng.random((N, ns)) * 100.0 - 50.0).astype(np.float32)          # |T| <= 50
        vars = _variants(rng, codes, nbase)
        st = S.starts(rm, L)
        for c in ((1, 10, 23) if N <= 65 else ((10, 1), (23, 1), (1, 23))[k % 3]):
            got = _both_modes(B, engine, T, nbase, codes, rm, vars, c, (ns, 64)[(k + c) % 2], (N, L))
            no_path += int(np.isneginf(got["alt"]).sum())
            for p, r, alt in vars:
                w = V.window(st, L, p, r, len(alt), c)
                widest = [max(widest[0], w[2]), max(widest[1], w[3])]
        k += 1
    assert no_path > 0                                      # L = N + 1, a base a block: an insertion has no path
    if 63 <= N <= 65:
        assert widest == [62, 62], widest                   # L = N + 1 at c = 23 with an allele of 16, in either hypothesis


def test_operator_hostile_scores_long_dwell_and_the_same_bytes_again(B, engine):
    rng = np.random.default_rng(9)
    for nbase in (4, 5):
        ns = 2 * nbase * (nbase + 1)
        # entries of -1e30: paths through them lose by far, sums stay finite, nothing is NaN
        N, L = 300, 60
        codes, rm = _letters(rng, nbase, L), _path(rng, N, L)
        T = (rng.random((N, ns)) * 100.0 - 50.0).astype(np.float32)
        T[rng.random((N, ns)) < 0.2] = np.float32(-1e30)
        vars = _variants(rng, codes, nbase)
        for c in (1, 10):
            _both_modes(B, engine, T, nbase, codes, rm, vars, c, ns, "-1e30")
        # one base dwells 5000 blocks, inside the windows of its neighbours
        lengths = [3] * 6 + [5000] + [2] * 6
        rm = np.concatenate([np.r_[np.zeros(n - 1, np.uint8), np.uint8(1)] for n in lengths])[:-1]
        codes = np.array([0, 2, 1, 1, 3, 0, 3, 2, 1, 3, 0, 2, 3], np.uint8)
        T = (rng.random((rm.size, ns)) * 100.0 - 50.0).astype(np.float32)
        vars = [(6, 1, [0]), (6, 1, []), (6, 0, [3]), (5, 2, [1, 1, 1]), (0, 1, [3]), (13, 0, [3, 3])]
        _both_modes(B, engine, T, nbase, codes, rm, vars, 10, 64, "dwell")
        for mode in (False, True):
            a, b = (B.op_variants(engine, T, nbase, codes, rm, V.pack(vars), 4, mode) for _ in range(2))
            assert a.tobytes() == b.tobytes() and a["nblock"].max() > 5000, mode


def test_operator_identities_with_site_mods_and_remap(B, engine):
    rng = np.random.default_rng(13)
    n = 0
    for N in (5, 64, 300):                                   # a SNP between C and Z is the site's record
        for L in sorted({1, N + 1, int(rng.integers(1, N + 2))}):
            codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L)
            rm = _path(rng, N, L)
            T = (rng.random((N, 60)) * 100.0 - 50.0).astype(np.float32)
            for c in (1, 10, 23):
                sm = B.op_site_mods(engine, T, 5, codes, rm, c)
                vars = [(int(i), 1, [S.CAN + S.MOD - int(codes[i])]) for i in sm["pos"]]
                got = B.op_variants(engine, T, 5, codes, rm, V.pack(vars), c)
                for rec, site in zip(got, sm):
                    ref, alt = (site["can"], site["mod"]) if codes[site["pos"]] == S.CAN else (site["mod"], site["can"])
                    assert rec["nblock"] == site["nblock"] and rec["ref"].tobytes() == ref.tobytes() and rec["alt"].tobytes() == alt.tobytes(), (N, L, c, site, rec)
                    n += 1
    assert n >= 100
    n = 0
    for nbase in (4, 5):                                    # the whole read as the window: the ref score is remap's
        for N in (1, 5, 64, 300):
            for L in sorted({1, min(N + 1, 24), int(rng.integers(1, min(N + 1, 24) + 1))}):
                codes = _letters(rng, nbase, L)
                T = (rng.random((N, 2 * nbase * (nbase + 1))) * 100.0 - 50.0).astype(np.float32)
                rm, score = B.op_remap(engine, T, nbase, codes, 2048)          # W >= L - 1
                vars = [(p, 1, [int(rng.integers(0, nbase))]) for p in range(L)] + [(L - 1, 1, [0, 1])]
                for rec in B.op_variants(engine, T, nbase, codes, rm, V.pack(vars), 23):
                    assert rec["nblock"] == N and rec["ref"].tobytes() == np.float32(score).tobytes(), (nbase, N, L, rec, score)
                    n += 1
    assert n >= 40


def _var(pos, nref, alt, nalt=None):
    v = V.pack([(pos, nref, list(alt)[:16])])
    if nalt is not None:
        v["nalt"] = nalt
    return v


def _invalid_variants(L, nbase):
    """every limit of include/ffhip.h "variants", broken once, for a sequence of L >= 3 codes"""
    return [_var(0, 0, []), _var(0, 17, [0]), _var(0, 1, [0] * 16, nalt=17), _var(-1, 1, [0]), _var(L, 1, [0]), _var(L - 1, 2, [0]), _var(L + 1, 0, [0]),
            _var(0, 1, [nbase]), _var(0, 1, [0, 255])] + ([_var(0, L, [])] if L <= 16 else [])


def test_operator_refusals(B, engine):
    rng = np.random.default_rng(3)
    for nbase in (4, 5):
        ns = 2 * nbase * (nbase + 1)
        T = rng.standard_normal((10, ns)).astype(np.float32)
        codes, rm = np.array([0, 1, 3], np.uint8), np.array([0, 1, 0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
        ok = V.pack([(1, 1, [2]), (3, 0, [0])])
        good = B.op_variants(engine, T, nbase, codes, rm, ok, 10)
        assert good["index"].tolist() == [0, 1] and good.tobytes() == V.variants(T, nbase, codes, rm, V.unpack(ok), 10).tobytes()
        two = rm.copy()
        two[0] = 2
        bad = [(T, nbase, codes, rm, ok, 0), (T, nbase, codes, rm, ok, 24), (T, nbase, codes, rm, ok, -1), (T, nbase, codes[:2], rm, ok[:1], 10),
               (T, nbase, np.array([0, 1, nbase], np.uint8), rm, ok, 10), (T, nbase, codes, two, ok, 10), (T, nbase, codes, rm[:9], ok, 10),
               (T, nbase, np.zeros(0, np.uint8), np.zeros(10, np.uint8), ok[:0], 10), (T, 9 - nbase, codes, rm, ok, 10), (T, 3, codes, rm, ok, 10)]
        bad += [(T, nbase, codes, rm, np.concatenate([ok, v]), 10) for v in _invalid_variants(3, nbase)]
        for args in bad:
            with pytest.raises(B.FFHipError) as e:
                B.op_variants(engine, *args)
            assert "ffhip error -1:" in str(e.value), (args[1:], str(e.value))      # FFHIP_EINVAL
            assert B.op_variants(engine, T, nbase, codes, rm, ok, 10).tobytes() == good.tobytes()      # the engine is usable
        with pytest.raises(B.FFHipError) as e:
            B.op_variants(engine, T, nbase, codes, rm, np.concatenate([ok, _var(2, 2, [0])]), 10)
        assert "read 0, index 2" in str(e.value)
        assert B.op_variants(engine, T, nbase, codes, rm, ok[:0], 10).size == 0      # no variants: no records


# ------------------------------------------------------------------------------------ batches
def _bytes_held(B, x):
    B.lib().ffhip_debug_batch_device_bytes.restype = C.c_size_t
    B.lib().ffhip_debug_batch_device_bytes.argtypes = [C.c_void_p]
    return B.lib().ffhip_debug_batch_device_bytes(x.h)


def _sequences(rng, calls, nblocks, nbase):
    """per read, in turn: its own call (three times), none (status 0), one base too many for its blocks (status 2)"""
    letters = "ACGTZ"[:nbase]
    seqs = []
    for v, call in enumerate(calls):
        kind = v % 5
        if kind == 3:
            seqs.append(None)
        elif kind == 4:
            seqs.append(rng.integers(0, nbase, nblocks[v] + 2).astype(np.uint8))
        else:
            seqs.append(np.array([letters.index(x) for x in call], np.uint8) if call else np.array([1], np.uint8))
    return seqs


def _check_batches(B, engine, bs, nreads, flags, where, nbase, every=1, reruns=False, seen_records=None):
    """every read's records against the operator on the batch's own transitions and path, in both modes; remap, events and site mods unchanged by the flag; the
    copies counted; returns the number of variants compared.  seen_records: {(transitions, path, sequence, context, mode): records} across batches"""
    also = B.RUN_EVENTS | (B.RUN_REMAP_MODS if nbase == 5 else 0)

    def run(fl):
        _d2h_calls(B)
        if len(bs) == 1:
            bs[0].run(1.0, fl)
        else:
            bs[0].run_pair(bs[1], 1.0, fl)
        for x in bs:
            x.finish()
        return _d2h_calls(B)[0]
    run(flags)
    rng = np.random.default_rng(29)
    seqs, vars = [], []
    for k, x in enumerate(bs):
        seqs.append(_sequences(rng, [x.basecall(v) for v in range(nreads[k])], [x.read_nblock(v) for v in range(nreads[k])], nbase))
        x.set_remap(seqs[k], 2048)
        vars.append([None if q is None else _variants(np.random.default_rng(1000 + v), q, nbase, 3) for v, q in enumerate(seqs[k])])      # (the same read: the same variants)
    run(flags | B.RUN_REMAP | also)                         # (the first run creates the siblings' buffers)
    copies = run(flags | B.RUN_REMAP | also)
    before = [[(_state(B, x, v, flags), x.remap(v), x.events(v), x.site_mods(v) if nbase == 5 else None) for v in range(0, nreads[k], every)] for k, x in enumerate(bs)]
    held = [_bytes_held(B, x) for x in bs]
    with pytest.raises(B.FFHipError):
        bs[0].variant_calls(0)                              # a run without the flag made none
    total, seen = 0, set()
    for c, mode in ((10, False), (23, True), (1, False)):
        for k, x in enumerate(bs):
            x.set_remap_variants([None if v is None else V.pack(v) for v in vars[k]], c, mode)
        copies_vr = run(flags | B.RUN_REMAP | also | B.RUN_REMAP_VARIANTS)
        if not reruns:                                      # (a re-run's side batch brings its own copies)
            assert copies_vr == copies + len(bs), (where, copies, copies_vr)
        for k, x in enumerate(bs):
            n_here = 0
            for n, v in enumerate(range(0, nreads[k], every)):
                st, (old, rec, ev, sm) = _state(B, x, v, flags), before[k][n]
                for key in st:
                    assert _same(st[key], old[key]), (where, k, v, key)
                got, vc = x.remap(v), x.variant_calls(v)
                assert got["status"] == rec["status"] and got["L"] == rec["L"] and _same(got["score"].view(np.uint32), rec["score"].view(np.uint32)), (where, k, v)
                seen.add(got["status"])
                if got["status"] != 1:
                    assert vc is None and x.events(v) is None, (where, k, v)
                    continue
                assert np.array_equal(got["rm"], rec["rm"]) and x.events(v).tobytes() == ev.tobytes(), (where, k, v)
                if nbase == 5:
                    assert x.site_mods(v).tobytes() == sm.tobytes(), (where, k, v)
                packed = V.pack(vars[k][v])
                trans = x.transitions(v)
                want = B.op_variants(engine, trans, nbase, seqs[k][v], got["rm"], packed, c, mode)
                assert vc.dtype == B.VARIANT_CALL_DTYPE and vc.tobytes() == want.tobytes(), (where, k, v, c, mode)
                assert vc["index"].tolist() == list(range(len(vars[k][v]))) and not np.any(np.isnan(vc["ref"])) and not np.any(np.isnan(vc["alt"])), (where, k, v)
                assert np.all(np.isfinite(vc["ref"])), (where, k, v)
                if seen_records is not None:                # the same scores, path and sequence in another batch: the same bytes
                    key = (trans.tobytes(), got["rm"].tobytes(), seqs[k][v].tobytes(), packed.tobytes(), c, mode)
                    other = seen_records.setdefault(key, (where, vc.tobytes()))
                    assert other[1] == vc.tobytes(), (where, other[0], k, v)
                    seen_records["shared"] = seen_records.get("shared", 0) + (other[0] != where)
                n_here += vc.size
            assert n_here > 0, (where, k)
            total += n_here
            if every == 1 and not getattr(x, "_had_variants", False):      # (the batch's first run with the flag: the buffers are new)
                assert _bytes_held(B, x) >= held[k] + 16 * n_here, (where, k, n_here)
            x._had_variants = True
        again = [[x.variant_calls(v) for v in range(0, nreads[k], every)] for k, x in enumerate(bs)]
        run(flags | B.RUN_REMAP | also | B.RUN_REMAP_VARIANTS)      # a second run: the same bytes
        for k, x in enumerate(bs):
            for n, v in enumerate(range(0, nreads[k], every)):
                a, b = again[k][n], x.variant_calls(v)
                assert (a is None and b is None) or a.tobytes() == b.tobytes(), (where, k, v)
    assert seen == {0, 1, 2}, (where, seen)
    if not reruns:
        assert run(flags | B.RUN_REMAP | also) == copies, where      # without the flag again: no copy more
    for x in bs:
        x.set_remap_variants(None)
        with pytest.raises(B.FFHipError):                   # detached: the flag is refused, the batch stays usable
            x.run(1.0, flags | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
        x.set_remap(None)
    return total


@pytest.mark.parametrize("hidden", [64, 256])
def test_batch_records_rows_ragged_packed(B, engine, hidden):
    nbase = 5 if hidden == 64 else 4
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5 if nbase == 5 else M.NET_LSTM5, hidden, seed=1))
    rng = np.random.default_rng(hidden)
    shared = {}
    sig = rng.standard_normal((16, 1500)).astype(np.float32)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(sig)
    n = _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE, ("rows", hidden), nbase, seen_records=shared)
    b.close()
    sigs = list(sig[:4]) + [rng.standard_normal(int(k)).astype(np.float32) for k in rng.integers(300, 1501, 12)]
    b = B.Batch(dm, 16, 1500)
    b.set_signals_ragged(sigs)
    n += _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE | B.RUN_MOVES, ("ragged", hidden), nbase, seen_records=shared)
    b.close()
    if hidden >= 128:                                       # (packed batches: models of 128 .. 512 hidden units)
        pb = B.Batch(dm, 8, 3000, max_reads=16)
        slot, off = pb.pack_plan([x.size for x in sigs])
        assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
        pb.set_signals_packed(sigs, slot, off)
        n += _check_batches(B, engine, [pb], [16], B.RUN_NO_TRACE, ("packed", hidden), nbase, seen_records=shared)
        n += _check_batches(B, engine, [pb], [16], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, ("packed per step", hidden), nbase, seen_records=shared)
        pb.close()
    else:
        b = B.Batch(dm, 16, 1500)
        b.set_signals_ragged(sigs)
        n += _check_batches(B, engine, [b], [16], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, ("ragged per step", hidden), nbase, seen_records=shared)
        b.close()
    dm.close()
    assert n >= 1000, n
    assert shared["shared"] > 0, "no read had the same scores and path in two layouts"


def _lstm_trunk_with_the_5_base_head(hidden, seed):
    """layer launches pair for the LSTM trunk at H = 384 only, and only the LSTM trunk's convolution lets a sample leave the split format's range (GRUmod's ends in
    tanh): the LSTM trunk under the GRUmod model's 5-base head is the 10-state model of both shapes"""
    lstm, gru = M.synthetic_model(M.NET_LSTM5, hidden, seed=seed), M.synthetic_model(M.NET_GRUMOD5, hidden, seed=seed)
    return M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b)


def test_batch_records_paired(B, engine):
    dm = B.DeviceModel(engine, _lstm_trunk_with_the_5_base_head(384, 2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 256, 600)
        b.set_signals(rng.standard_normal((256, 600)).astype(np.float32))
        pair.append(b)
    pair[0].run_pair(pair[1], 1.0, B.RUN_NO_TRACE)
    assert pair[0].paired() and pair[1].paired()
    for b in pair:
        b.finish()
    assert _check_batches(B, engine, pair, [256, 256], B.RUN_NO_TRACE, "pair", 5, every=16) > 100
    for b in pair:
        b.close()
    dm.close()


@pytest.mark.parametrize("nbase", [4, 5])
def test_batch_records_after_an_f32_rerun(B, engine, nbase):
    dm = B.DeviceModel(engine, _lstm_trunk_with_the_5_base_head(128, 1) if nbase == 5 else M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 1501, 16)]
    sigs[0][200] = 6.0e4                                    # (reads 0 and 5: their own calls are their sequences, so they are mapped)
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 1500)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], 0, "rerun rows", nbase, reruns=True)
    b.set_remap(_sequences(rng, [b.basecall(v) for v in range(16)], [b.read_nblock(v) for v in range(16)], nbase), 2048)
    b.run(1.0, B.RUN_REMAP)
    b.finish()
    assert b.f32_reruns() == 2 and b.remap(0)["status"] == 1 and b.remap(5)["status"] == 1
    b.close()
    if nbase == 5:
        pb = B.Batch(dm, 16, 3000, max_reads=16)
        slot, off = pb.pack_plan([x.size for x in sigs])
        assert min(slot) >= 0
        pb.set_signals_packed(sigs, slot, off)
        _check_batches(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", nbase, reruns=True)
        assert pb.f32_reruns() >= 2
        pb.close()
    dm.close()


def test_flag_and_setter_refusals_leave_the_batch_usable(B, engine):
    rng = np.random.default_rng(2)
    sig = rng.standard_normal((4, 1000)).astype(np.float32)

    def refused(what, f, *args):
        with pytest.raises(B.FFHipError) as e:
            f(*args)
        assert "ffhip error -1:" in str(e.value) and what in str(e.value), (what, str(e.value))
    for nbase, kind in ((5, M.NET_GRUMOD5), (4, M.NET_LSTM5)):
        dm = B.DeviceModel(engine, M.synthetic_model(kind, 64 if nbase == 5 else 128, seed=1))
        b = B.Batch(dm, 4, 1000)
        b.set_signals(sig)
        ok = [V.pack([(3, 1, [0]), (40, 0, [1, 2])]), None, V.pack([(0, 2, [])]), V.pack([])]
        refused("no sequences", b.set_remap_variants, ok)                       # before ffhip_batch_set_remap
        seqs = [_letters(rng, nbase, 40) for _ in range(3)] + [None]
        b.set_remap(seqs, 2048)
        refused("variants", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)      # no variants set
        for c in (0, 24, -1):
            refused("context", b.set_remap_variants, ok, c)
        refused("reads", b.set_remap_variants, ok[:3])
        refused("read 3, index 0", b.set_remap_variants, ok[:3] + [V.pack([(0, 1, [0])])])      # a read without a sequence
        for v in _invalid_variants(40, nbase):
            refused("read 2, index 1", b.set_remap_variants, ok[:2] + [np.concatenate([ok[2], v])] + ok[3:])
        b.set_remap_variants(ok)
        refused("FFHIP_RUN_REMAP", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP_VARIANTS)
        refused("FFHIP_RUN_NO_DECODE", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_NO_DECODE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
        refused("running", b.set_remap_variants, ok)            # not between a run and its finish
        b.finish()
        for v in range(3):
            rec = b.remap(v)
            assert rec["status"] == 1
            want = B.op_variants(engine, b.transitions(v), nbase, seqs[v], rec["rm"], ok[v] if ok[v] is not None else V.pack([]), 10, False)      # the defaults
            assert b.variant_calls(v).tobytes() == want.tobytes(), v
        assert b.remap(3)["status"] == 0 and b.variant_calls(3) is None
        b.set_remap(seqs, 2048)                                 # new sequences detach the variants
        refused("variants", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP)
        b.finish()
        assert b.remap(0)["status"] == 1
        b.close()
        dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))      # the run-length model: refused as for remap
    b = B.Batch(dm, 4, 1000)
    b.set_signals(sig)
    refused("no sequences", b.set_remap_variants, [None] * 4)
    refused("FFHIP_RUN_REMAP", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP_VARIANTS)
    refused("flip-flop model", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    b.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_remap_variants(B, engine, tmp_path):
    import os
    import re
    import subprocess
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC")
    M.write_mdl(str(tmp_path / "flipflop_r941native5mC.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 12
    names = ["uuid-%04d" % i for i in range(nread)]
    for i, n in enumerate(rng.integers(1500, 4000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), names[i], synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_5mC", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    trace = tmp_path / "trace.hdf5"
    default, _ = run(["--trace", str(trace)])
    lines = default.split("\n")[:-1]
    recs = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    order = [r[0][1:].split("  {")[0] for r in recs]
    calls = {r[0][1:].split("  {")[0]: r[1] for r in recs}
    assert sorted(order) == names
    seqs, text = {}, ""
    for i, name in enumerate(names):                        # own call; none; a bad letter
        call, kind = calls[name], i % 4
        if kind < 2:
            seqs[name] = call
        elif kind == 2:
            seqs[name] = call[:3] + "N" + call[3:]
        if name in seqs:
            text += ">%s\n%s\n" % (name, seqs[name])
    text += ">ghost\nACGTACGTACGT\n"                        # a record no read has
    refs = tmp_path / "refs.fa"
    refs.write_text(text)
    letters = "ACGTZ"
    wanted, vlines, skipped = {}, ["# name\tpos\tref\talt", ""], 0
    for i, name in enumerate(names):
        if name not in seqs:
            vlines.append("%s\t0\tA\tC" % name)            # no record: skipped
            skipped += 1
            continue
        s = seqs[name]
        if "N" in s:
            vlines.append("%s\t0\t%s\tC" % (name, s[0]))    # a record that cannot be used: skipped
            skipped += 1
            continue
        mine = []
        for p in sorted(int(x) for x in rng.choice(len(s) - 3, 6, replace=False)):
            kind = int(rng.integers(0, 4))
            ref, alt = (s[p], letters[(letters.index(s[p]) + 1) % 5]) if kind == 0 else ("-", s[p] + "G") if kind == 1 else (s[p:p + 2], "-") if kind == 2 else (s[p:p + 3], s[p:p + 3][::-1])
            vlines.append("%s\t%d\t%s\t%s" % (name, p, ref, alt))
            mine.append((p, 0 if ref == "-" else len(ref), [] if alt == "-" else [letters.index(x) for x in alt], ref, alt))
        mine.append((len(s), 0, [0], "-", "A"))
        vlines.append("%s\t%d\t-\tA" % (name, len(s)))
        wanted[name] = mine
        vlines.append("%s\t1\t%s\tA" % (name, letters[(letters.index(s[1]) + 2) % 5]))      # ref is not the record's letter: skipped
        vlines.append("%s\t%d\tA\tC" % (name, len(s)))     # beyond the record: skipped
        skipped += 2
    vlines += ["ghost\t2\tG\tT", "ghost\t3\tT\t-", "broken line", "ghost\t2\tG\tX", "ghost\t2\tG\t" + "A" * 17]
    skipped += 3
    vars_path = tmp_path / "vars.tsv"
    vars_path.write_text("\n".join(vlines) + "\n")
    plain_map = tmp_path / "plain.tsv"
    assert run(["--remap", str(refs), "--remap-out", str(plain_map)])[0] == default
    tables = {}
    for tag, extra in (("best", []), ("all", ["--remap-variants-all-paths"]), ("c3", ["--remap-variants-context", "3"])):
        mp, out = tmp_path / (tag + "_map.tsv"), tmp_path / (tag + "_calls.tsv")
        stdout, err = run(["--remap", str(refs), "--remap-out", str(mp), "--remap-variants", str(vars_path), "--remap-variants-out", str(out)] + extra)
        assert stdout == default and mp.read_bytes() == plain_map.read_bytes(), tag
        tables[tag] = (out.read_text().split("\n")[:-1], err)
    by_name = {}
    for line in plain_map.read_text().split("\n")[:-1]:
        f = line.split("\t")
        by_name[f[0]] = f
    mapped = [name for name in order if name in wanted and by_name[name][1] == "1"]
    assert len(mapped) >= 4
    # the batch API on the signals the binary prepared (--trace), the same sequences and variants: wherever the mapping is the binary's, so are the lines
    sigs = [dump_trace(trace, name)[0] for name in mapped]
    dm = B.DeviceModel(engine, mdl)
    b = B.Batch(dm, len(mapped), max(x.size for x in sigs))
    b.set_signals_ragged(sigs)
    b.set_remap([np.array([letters.index(x) for x in seqs[name]], np.uint8) for name in mapped], 2048)
    for tag, c, mode in (("best", 10, False), ("all", 10, True), ("c3", 3, False)):
        b.set_remap_variants([V.pack([w[:3] for w in wanted[name]]) for name in mapped], c, mode)
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_VARIANTS)
        b.finish()
        got, err = tables[tag]
        at, compared = 0, 0
        for v, name in enumerate(mapped):
            rec, vc = b.remap(v), b.variant_calls(v)
            mine = [g.split("\t") for g in got if g.split("\t")[0] == name]
            assert got[at:at + len(mine)] == ["\t".join(f) for f in mine], (tag, name)          # reads in output order ...
            at += len(mine)
            assert [(int(f[1]), f[2], f[3]) for f in mine] == [(w[0], w[3], w[4]) for w in wanted[name]], (tag, name)      # ... variants in file order
            for f in mine:
                assert len(f) == 8 and f[5] == "%.9g" % np.float32(f[5]) and f[6] == "%.9g" % np.float32(f[6]), f
                assert f[7] == ("inf" if f[6] == "-inf" else "%.9g" % (float(np.float32(f[5])) - float(np.float32(f[6])))), f
            starts = ",".join(str(x) for x in RR.starts_maxdev(rec["rm"], rec["L"])[0])
            if rec["status"] == 1 and by_name[name][9] == starts and by_name[name][8] == "%.9g" % rec["score"]:
                assert [f[4:7] for f in mine] == [["%d" % r["nblock"], "%.9g" % r["ref"], "%.9g" % r["alt"]] for r in vc], (tag, name)
                compared += 1
        assert at == len(got) and compared >= 4, (tag, at, len(got), compared)
        count = dict((k, int(v)) for k, v in re.findall(r"^variants\t(\S+)\t(\d+)$", err, re.M))
        kept = sum(len(w) for w in wanted.values()) + 2
        assert count == {"reads": len(mapped), "scored": len(got), "skipped": skipped, "unmapped": kept - len(got)}, (err, skipped, kept)
        assert count["scored"] + count["skipped"] + count["unmapped"] == len([x for x in vlines if x and not x.startswith("#")])
        for kind in ("is malformed", "outside the model's alphabet", "longer than 16", "names no record", "lies beyond", "not the record's letters"):
            assert kind in err, kind                        # the first line of each kind is quoted
    b.close()
    dm.close()
