"""flappie --map-mods on the GPU: per reference C, how the aligned reads of all batches class their 5mC bytes (include/ffhip.h "mod pileup": ffhip_modpileup_*,
ffhip_batch_set_modpileup, FFHIP_RUN_MOD_PILEUP, ffhip_op_modpileup; the kernel k_modpileup).

  * the operator against modpileup_ref.py on a reference with records of 1, 15, 16, 17, 33, 100 and 1100 bases, one all C, one all G, one without C or G (every
    lane, and no lane, issues an atomic), on both strands, spans touching either end, op counts at the wave and chunk edges of the prefix counts, each as all '=',
    all 'D', 'I' at both edges and random mixes; bytes drawn so that 0, lo, lo + 1, hi - 1, hi and 255 occur; calls drawn independently of the ops; several
    alignments in one object; reset; the identity test at equality; its refusals;
  * batches of the 5mC model (one read a row, ragged with an empty slot, packed, paired): planes, totals and histogram equal modpileup_ref over the batch's own
    final map(), truth(), basecall() and mod_probs(); the run's records and device bytes are those of the run without the flag; a second run doubles every counter;
    min_identity moves exactly the reads below it to `skipped`; with RUN_PILEUP as well both objects hold what each holds alone;
  * after an f32 re-run (the LSTM trunk under the 5-base head) every read is counted once, from the patched letters and bytes (the fall-back to the
    launch-per-step kernels cannot be taken without a launch that times out and is not tested: it rests on where ffhip_batch_finish launches the kernel);
  * two batches in flight into one object give the sum; another batch size and a packed batch give the same bytes;
  * the refusals of the flag and of ffhip_batch_set_modpileup, with their texts;
  * the `flappie` binary: mods.bed and hist.tsv rebuilt from acc.tsv, hits.tsv, the calls and the ML tags of the same run; the same files at two batch sizes and
    with --reverse; both motifs and combine-strands; everything else unchanged; with --map-pileup as well; an LSTM model and runnie refuse.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import map_ref as R
import modpileup_ref as MP
import pileup_ref as PU
import truth_ref as T
from test_barcodes_gpu import _packed_batch, _records, rand_seq
from test_maptruth_gpu import reference_of, same_truth
from test_pileup_gpu import _run, permille

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


def assert_same(got, want, where):
    counts, totals, hist = got
    assert counts.dtype == np.uint32 and counts.shape == want.counts.shape and hist.dtype == np.uint64 and hist.shape == (256,), (where, counts.shape)
    assert totals == want.totals, (where, totals, want.totals)
    assert np.array_equal(hist, want.hist), (where, [(v, int(hist[v]), int(want.hist[v])) for v in np.flatnonzero(hist != want.hist)[:8]])
    if not np.array_equal(counts, want.counts):
        bad = np.argwhere(counts != want.counts)
        raise AssertionError((where, len(bad), [(tuple(int(v) for v in ix), int(counts[tuple(ix)]), int(want.counts[tuple(ix)])) for ix in bad[:8]]))
    assert int(hist.sum()) == totals["mod"] + totals["canon"] + totals["fail"] and totals["sites"] == sum(totals[c] for c in MP.COLUMNS), (where, totals)


# ------------------------------------------------------------------------------------ the operator
OP_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
LENS = (1, 15, 16, 1100, 17, 33, 100)
LO, HI = 77, 180


def operator_reference(rng):
    """records of LENS: 15 all C, 16 all G, 17 without C or G; the others random (the record of one base: a C)"""
    recs = [rand_seq(rng, m) for m in LENS]
    recs[0], recs[1], recs[2], recs[4] = "C", "C" * 15, "G" * 16, rand_seq(rng, 17, "AT")
    return recs


def draw(rng, n):
    """a call over ACGTZ and its bytes: the edges of the three classes and anything between"""
    call = "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n))
    edges = np.array([0, LO, LO + 1, HI - 1, HI, 255], np.uint8)
    ml = np.where(rng.random(n) < 0.5, edges[rng.integers(0, 6, n)], rng.integers(0, 256, n).astype(np.uint8)).astype(np.uint8)
    return call, ml


def operator_cases(rng):
    """(K, kind, q, tstart, tend, call, ml, ops) for every op count in four kinds, on both strands, on the shortest records that hold them and on the last, at either
    end of the record; then every record between filled by one path of '=' and by a mix"""
    out = []
    for K in OP_COUNTS:
        kinds = {"=": np.zeros(K, np.uint8), "D": np.full(K, 3, np.uint8)}
        kinds["I..I"] = np.array([2] + [0] * (K - 2) + [2], np.uint8) if K >= 3 else np.array([2, 0, 2], np.uint8)
        for s in range(3):
            mix = rng.choice(4, size=K, p=(0.55, 0.15, 0.15, 0.15)).astype(np.uint8)
            if (mix != 2).sum() == 0:
                mix[int(rng.integers(0, K))] = 0
            kinds["mix%d" % s] = mix
        for kind, ops in kinds.items():
            m, n = int((ops != 2).sum()), int((ops != 3).sum())
            fits = sorted((k for k, Mk in enumerate(LENS) if Mk >= m), key=lambda k: LENS[k])
            for k in {fits[0], fits[-1], 6 if m <= LENS[6] else 3}:
                for o in (0, 1):
                    for at_end in (0, 1):
                        ts = LENS[k] - m if at_end else 0
                        out.append((K, kind, 2 * k + o, ts, ts + m) + draw(rng, n) + (ops,))
    for k in (1, 2, 4, 5):
        for o in (0, 1):
            Mk = LENS[k]
            mix = rng.choice(4, size=Mk, p=(0.55, 0.15, 0.15, 0.15)).astype(np.uint8)
            mix[0] = 0
            for kind, ops in (("=", np.zeros(Mk, np.uint8)), ("mix", mix)):
                m, n = int((ops != 2).sum()), int((ops != 3).sum())
                ts = (Mk - m) if o else 0
                out.append((int(ops.size), kind, 2 * k + o, ts, ts + m) + draw(rng, n) + (ops,))
    return out


def test_operator_at_the_wave_and_chunk_edges(B, engine):
    rng = np.random.default_rng(43)
    recs = operator_reference(rng)
    ref = B.MapRef(engine, recs)
    pile = B.ModPileup(engine, ref, 0, LO, HI)
    assert pile.positions == sum(LENS)
    want = MP.ModPileup(LENS, recs, 0, LO, HI)
    assert_same(pile.download(), want, "created")
    cases = operator_cases(rng)
    assert {c[0] for c in cases} >= set(OP_COUNTS) and {c[2] & 1 for c in cases} == {0, 1} and {c[2] >> 1 for c in cases} == set(range(len(LENS)))
    # letter and op disagree somewhere: an '=' whose call letter is not the reference's, and the edges of the classes all occur on counted calls
    for i, (K, kind, q, ts, te, call, ml, ops) in enumerate(cases):
        B.op_modpileup(engine, pile, q, ts, te, call, ml, ops)
        want.add(q, ts, te, call, ml, ops)
        if kind != "=" or i % 8 == 0:                          # several alignments added into one object before it is looked at
            assert_same(pile.download(), want, (K, kind, q, ts, te))
    assert_same(pile.download(), want, "all")
    t = want.totals
    assert t["reads"] == len(cases) and min(t[k] for k in MP.TOTALS if k != "skipped") > 0 and t["diff"] > 0, t
    assert all(want.hist[v] > 0 for v in (0, LO, LO + 1, HI - 1, HI, 255)), "every edge of the three classes"
    assert want.counts[:, sum(LENS[:4]):sum(LENS[:5])].sum() == 0 and want.counts[5:, sum(LENS[:1]):sum(LENS[:2])].sum() == 0      # no C or G: nothing; all C: nothing on -
    pile.reset()
    want.reset()
    assert_same(pile.download(), want, "reset")
    # the identity test inside the kernel: 3 matches in 4 columns, equality passes (record 4 is the 1100-base one at q = 6, 7)
    span = recs[3][3:7]
    for min_id, counted in ((750, 1), (751, 0)):
        p2, w2 = B.ModPileup(engine, ref, min_id, LO, HI), MP.ModPileup(LENS, recs, min_id, LO, HI)
        B.op_modpileup(engine, p2, 6, 3, 7, "CZC", [200, 10, 100], [0, 0, 3, 0])
        w2.add(6, 3, 7, "CZC", [200, 10, 100], [0, 0, 3, 0])
        assert w2.totals["reads"] == counted and w2.totals["skipped"] == 1 - counted and w2.totals["sites"] == counted * span.count("C")
        assert_same(p2.download(), w2, min_id)
        p2.close()
    p2 = B.ModPileup(engine, ref, -7, 0, 1)                   # negative: 0; the narrowest thresholds
    B.op_modpileup(engine, p2, 0, 0, 1, "", [], [3])
    B.op_modpileup(engine, p2, 0, 0, 1, "Z", [1], [0])
    B.op_modpileup(engine, p2, 0, 0, 1, "C", [0], [1])
    got = p2.download()
    assert got[1] == dict(reads=3, skipped=0, sites=3, mod=1, canon=1, fail=0, diff=0) | {"del": 1} and got[0][:, 0].tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    p2.close()
    # every refusal, and nothing added by any
    eq = [0, 0, 0]
    by = [1, 2, 3]
    for q, a, b, call, ml, ops, text in ((-1, 0, 3, "ACG", by, eq, "search"), (14, 0, 3, "ACG", by, eq, "search"), (2, -1, 2, "ACG", by, eq, "span"),
                                         (2, 13, 16, "ACG", by, eq, "span"), (2, 3, 3, "", [], [], "span"), (2, 5, 4, "", [], [], "span"), (0, 0, 2, "AC", [1, 2], [0, 0], "span"),
                                         (2, 0, 3, "ACN", by, eq, "not one of A C G T Z"), (2, 0, 3, "AcG", by, eq, "not one of A C G T Z"),
                                         (2, 0, 3, "ACG", by, [0, 4, 0], "not one of 0 .. 3"), (2, 0, 3, "ACG", by, [0, 0], "consume"), (2, 0, 3, "ACG", by, [0, 0, 0, 0], "consume"),
                                         (2, 0, 3, "AC", [1, 2], eq, "consume"), (2, 0, 3, "ACG", by, [0, 0, 3, 3], "consume"), (2, 0, 3, "ACG", by, [0, 0, 0, 2], "consume"),
                                         (2, 0, 3, "ACG", None, eq, "bad mod pileup arguments")):
        with pytest.raises(B.FFHipError) as ei:
            B.op_modpileup(engine, pile, q, a, b, call, ml, ops)
        assert text in str(ei.value) and ("mod pileup" in str(ei.value)), (q, a, b, call, ops, str(ei.value))
    for args, text in (((1001, LO, HI), "0 .. 1000"), ((0, -1, 5), "0 <= lo < hi <= 255"), ((0, 5, 5), "0 <= lo < hi <= 255"), ((0, 9, 5), "0 <= lo < hi <= 255"),
                       ((0, 5, 256), "0 <= lo < hi <= 255")):
        with pytest.raises(B.FFHipError) as ei:
            B.ModPileup(engine, ref, *args)
        assert text in str(ei.value), (args, str(ei.value))
    assert_same(pile.download(), want, "after the refusals")
    pile.close()
    ref.close()


# ------------------------------------------------------------------------------------ batches
def _thresholds(hist):
    """lo and hi at about the 1/3 and 2/3 quantiles of the counted bytes, so that all three classes occur"""
    cum = np.cumsum(hist.astype(np.int64))
    lo = int(np.searchsorted(cum, cum[-1] / 3.0))
    hi = int(np.searchsorted(cum, 2.0 * cum[-1] / 3.0))
    lo = min(lo, 253)
    return lo, min(max(hi, lo + 2), 255)


def _expected(bs, slots, lens, recs, min_identity, lo, hi):
    """modpileup_ref accumulated over the batches' own final records, letters and bytes; and what was seen"""
    want = MP.ModPileup(lens, recs, min_identity, lo, hi)
    seen = {"reads": 0, "plus": 0, "minus": 0, "not mapped": 0}
    for k, v in slots:
        mp, tr = bs[k].map(v), bs[k].truth(v)
        want.add_read(mp, tr, bs[k].basecall(v), bs[k].mod_probs(v))
        ok = mp["status"] == 1 and tr["status"] == 1
        seen["reads"] += 1
        seen["plus"] += ok and not mp["q"] & 1
        seen["minus"] += ok and mp["q"] & 1
        seen["not mapped"] += mp["status"] != 1
    return want, seen


def _batches_into_a_modpileup(B, engine, bs, nreads, flags, where, band=48, window=-1, e=-1, empty=(), reruns=None, whole=True):
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    _run(bs, flags)
    calls = [bs[k].basecall(v) for k, v in slots]
    recs = reference_of(np.random.default_rng(23), calls)
    lens = [len(r) for r in recs]
    ref = B.MapRef(engine, recs)
    for x in bs:
        x.set_map(ref, window, e)
        x.set_truth_from_map(True, band)
    fl = flags | B.RUN_MAP | B.RUN_TRUTH | B.RUN_MOD_PROBS
    _run(bs, fl)                                              # without the flag
    plain = {kv: (bs[kv[0]].map(kv[1]), bs[kv[0]].truth(kv[1]), bs[kv[0]].mod_probs(kv[1])) for kv in slots}
    held = [x.device_bytes() for x in bs]
    lo, hi = _thresholds(_expected(bs, slots, lens, recs, 0, 50, 205)[0].hist)      # (the histogram does not depend on the thresholds)
    pile = B.ModPileup(engine, ref, 0, lo, hi)
    for x in bs:
        x.set_modpileup(pile)
    _run(bs, fl | B.RUN_MOD_PILEUP)
    if reruns is not None:
        assert reruns(bs[0].f32_reruns()), bs[0].f32_reruns()
    for kv, call in zip(slots, calls):                        # everything the run returns is what the same run returns without the flag
        k, v = kv
        assert bs[k].basecall(v) == call and np.array_equal(bs[k].map(v)["raw"], plain[kv][0]["raw"]) and same_truth(bs[k].truth(v), plain[kv][1]), (where, kv)
        assert np.array_equal(bs[k].mod_probs(v), plain[kv][2]), (where, kv)
    assert [x.device_bytes() for x in bs] == held, where       # the counters are the object's, not the batch's
    want, seen = _expected(bs, slots, lens, recs, 0, lo, hi)
    assert_same(pile.download(), want, where)
    # what keeps the test from passing empty
    t = want.totals
    assert t["reads"] * 4 >= seen["reads"] * 3 and seen["plus"] >= 2 and seen["minus"] >= 2 and seen["not mapped"] >= 1, (where, seen, t)
    assert min(t[c] for c in MP.COLUMNS) > 0 and t["skipped"] == 0 and int((want.hist > 0).sum()) >= 8, (where, t, lo, hi)
    # a second run doubles every counter
    _run(bs, fl | B.RUN_MOD_PILEUP)
    counts, totals, hist = pile.download()
    assert np.array_equal(counts, 2 * want.counts) and totals == {k: 2 * v for k, v in want.totals.items()} and np.array_equal(hist, 2 * want.hist), where
    pile.close()
    if whole:
        # min_identity from the batch's own records, so that it splits the reads: exactly those below it go from `reads` to `skipped`
        vals = sorted(permille(bs[k].truth(v)) for k, v in slots if bs[k].map(v)["status"] == 1 and bs[k].truth(v)["status"] == 1)
        cut = vals[-1]
        below = sum(x < cut for x in vals)
        assert 0 < below < len(vals), (where, vals)
        strict = B.ModPileup(engine, ref, cut, lo, hi)
        for x in bs:
            x.set_modpileup(strict)
        _run(bs, fl | B.RUN_MOD_PILEUP)
        want2, _ = _expected(bs, slots, lens, recs, cut, lo, hi)
        assert (want2.totals["reads"], want2.totals["skipped"]) == (len(vals) - below, below) and want2.totals["reads"] + below == want.totals["reads"], (where, want2.totals)
        assert_same(strict.download(), want2, (where, cut))
        strict.close()
        # with RUN_PILEUP as well: both objects hold what each holds alone, the pileup's bytes those of the run without the new flag
        alone = B.Pileup(engine, ref)
        for x in bs:
            x.set_pileup(alone)
        _run(bs, fl | B.RUN_PILEUP)
        pu_alone = alone.download()
        alone.reset()
        both = B.ModPileup(engine, ref, 0, lo, hi)
        for x in bs:
            x.set_modpileup(both)
        _run(bs, fl | B.RUN_PILEUP | B.RUN_MOD_PILEUP)
        assert_same(both.download(), want, (where, "beside the pileup"))
        pu_both = alone.download()
        assert pu_both[1] == pu_alone[1] and pu_both[0].tobytes() == pu_alone[0].tobytes() and pu_alone[1]["reads"] == want.totals["reads"], where
        both.close()
        for x in bs:
            x.set_pileup(None)
        alone.close()
    for x in bs:
        x.set_modpileup(None)
        x.set_truth(None)
        x.set_map(None)
    ref.close()


def test_rows_ragged_packed_paired(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 128, seed=1))
    rng = np.random.default_rng(128)
    b = B.Batch(dm, 16, 1000)
    b.set_signals(rng.standard_normal((16, 1000)).astype(np.float32))
    _batches_into_a_modpileup(B, engine, [b], [16], B.RUN_NO_TRACE, "rows")
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(800, 1301, 13)) + [0, 1400, 900] + list(rng.integers(800, 1301, 4))]
    b = B.Batch(dm, 20, 1400)
    b.set_signals_ragged(sigs)
    _batches_into_a_modpileup(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, "ragged", band=100, window=128, e=200, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 3000, 24, rng, lo=800, hi=1300)
    _batches_into_a_modpileup(B, engine, [pb], [n], B.RUN_NO_TRACE, "packed", band=64)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, 1000)
        x.set_signals(rng.standard_normal((16, 1000)).astype(np.float32))
        pair.append(x)
    _batches_into_a_modpileup(B, engine, pair, [16, 16], B.RUN_NO_TRACE, "pair", band=32)
    for x in pair:
        x.close()
    dm.close()


def test_every_read_is_counted_once_after_an_f32_rerun(B, engine):
    # the outlier case every re-run test of the suite uses (H = 128, these signals) under the model whose re-run carries the 5mC bytes: the LSTM trunk under the
    # 5-base head.  The outlier's reads come from the side batch, whose records, letters and bytes are patched into this batch's before the kernel is launched
    lstm, gru = M.synthetic_model(M.NET_LSTM5, 128, seed=1), M.synthetic_model(M.NET_GRUMOD5, 128, seed=1)
    dm = B.DeviceModel(engine, M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _batches_into_a_modpileup(B, engine, [b], [16], 0, "rerun rows", reruns=lambda r: r == 2, whole=False)
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _batches_into_a_modpileup(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", band=300, reruns=lambda r: r >= 2, whole=False)
    pb.close()
    dm.close()


@pytest.fixture(scope="module")
def small(B, engine):
    """one 5mC model, the signals of 16 reads and a reference from their calls, shared by the tests below"""
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 128, seed=1))
    rng = np.random.default_rng(31)
    sig = rng.standard_normal((16, 1000)).astype(np.float32)
    b = B.Batch(dm, 16, 1000)
    b.set_signals(sig)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    calls = [b.basecall(v) for v in range(16)]
    recs = reference_of(np.random.default_rng(37), calls)
    ref = B.MapRef(engine, recs)
    b.close()
    yield dm, sig, calls, recs, ref
    ref.close()
    dm.close()


def _attached(B, dm, ref, pile, sig, band=48):
    b = B.Batch(dm, sig.shape[0], sig.shape[1])
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, band)
    b.set_modpileup(pile)
    return b


def test_two_batches_in_flight_another_size_and_packed(B, engine, small):
    dm, sig, calls, recs, ref = small
    lens = [len(r) for r in recs]
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH | B.RUN_MOD_PROBS | B.RUN_MOD_PILEUP
    lo, hi = 90, 160
    # one batch of 16: the bytes everything below is held to
    pile = B.ModPileup(engine, ref, 0, lo, hi)
    b = _attached(B, dm, ref, pile, sig)
    b.run(1.0, fl)
    b.finish()
    want, seen = _expected([b], [(0, v) for v in range(16)], lens, recs, 0, lo, hi)
    one = pile.download()
    assert_same(one, want, "one batch")
    assert want.totals["reads"] >= 12 and seen["plus"] >= 2 and seen["minus"] >= 2 and want.totals["sites"] > 0 and int(want.hist.sum()) > 0
    # two batches attached to one object, both between run and finish: the sum of the two
    other = np.ascontiguousarray(sig[::-1][:11])              # (eleven of the same reads in another order: they map onto this reference too)
    b2 = _attached(B, dm, ref, pile, other)
    pile.reset()
    b.run(1.0, fl)
    b2.run(1.0, fl)
    b.finish()
    b2.finish()
    want2, _ = _expected([b, b2], [(0, v) for v in range(16)] + [(1, v) for v in range(11)], lens, recs, 0, lo, hi)
    assert_same(pile.download(), want2, "two in flight")
    assert (want2.counts >= want.counts).all() and want.totals["reads"] + 8 <= want2.totals["reads"] < 2 * want.totals["reads"]
    b.close()
    b2.close()
    # the same reads through batches of another size: the same bytes
    pile.reset()
    halves = [_attached(B, dm, ref, pile, sig[:8]), _attached(B, dm, ref, pile, sig[8:])]
    for x in halves:
        x.run(1.0, fl)
    for x in halves:
        x.finish()
    got = pile.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes() and got[2].tobytes() == one[2].tobytes(), "two batches of 8"
    for x in halves:
        x.close()
    # ... and packed, several reads a row, in another order
    pile.reset()
    order = [5, 0, 11, 3, 15, 8, 1, 13, 2, 7, 10, 4, 14, 6, 9, 12]
    sigs = [sig[v] for v in order]
    pb = B.Batch(dm, 8, 2500, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < 16
    pb.set_signals_packed(sigs, slot, off)
    pb.set_map(ref)
    pb.set_truth_from_map(True, 48)
    pb.set_modpileup(pile)
    pb.run(1.0, fl)
    pb.finish()
    assert [pb.basecall(i) for i in range(16)] == [calls[v] for v in order]
    got = pile.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes() and got[2].tobytes() == one[2].tobytes(), "packed"
    pb.close()
    pile.close()


def test_the_refusals_and_their_texts(B, engine, small):
    dm, sig, calls, recs, ref = small
    pile = B.ModPileup(engine, ref)
    b = B.Batch(dm, 16, 1000)
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, 48)
    base = B.RUN_NO_TRACE
    full = base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_MOD_PROBS | B.RUN_MOD_PILEUP

    def refused(flags, text):
        with pytest.raises(B.FFHipError) as ei:
            b.run(1.0, flags)
        assert text in str(ei.value), (text, str(ei.value))

    b.set_modpileup(pile)
    refused(full & ~B.RUN_MAP, "mod pileup: the run does not make the map records")
    refused(full & ~B.RUN_TRUTH, "mod pileup: the run does not make the truth records")
    refused(full & ~B.RUN_MOD_PROBS, "mod pileup: the run does not make the 5mC probabilities")
    b.set_truth([np.zeros(5, np.uint8)] * 16, 48)             # outside the mode: host truths
    refused(full, "mod pileup: the batch is not in the mode of truth from map")
    b.set_truth_from_map(True, 48)
    b.set_modpileup(None)
    refused(full, "no mod pileup is attached")
    other = B.MapRef(engine, recs)                            # the same letters, another reference
    foreign = B.ModPileup(engine, other)
    b.set_modpileup(foreign)
    refused(full, "another reference")
    b.set_modpileup(pile)
    b.run(1.0, full)
    for p in (None, pile):                                    # not between a run and its finish
        with pytest.raises(B.FFHipError) as ei:
            b.set_modpileup(p)
        assert "between a run and its finish" in str(ei.value)
    b.finish()
    counts, totals, hist = pile.download()
    got = foreign.download()
    assert totals["reads"] >= 12 and int(got[0].sum()) == 0 and got[1]["reads"] == 0 and int(got[2].sum()) == 0      # no refused run added anything, anywhere
    b.set_modpileup(None)
    b.run(1.0, full & ~B.RUN_MOD_PILEUP)                      # detached, without the flag: as before
    b.finish()
    assert pile.download()[1] == totals
    b.close()
    for kind, H in ((M.NET_LSTM5_RLE, 128), (M.NET_LSTM5, 128)):      # a model whose alphabet is not ACGTZ
        dm4 = B.DeviceModel(engine, M.synthetic_model(kind, H, seed=1))
        x = B.Batch(dm4, 4, 1000)
        with pytest.raises(B.FFHipError) as ei:
            x.set_modpileup(pile)
        assert "no modified base" in str(ei.value)
        x.set_modpileup(None)
        x.close()
        dm4.close()
    eng2 = B.Engine(0)                                        # another engine's object
    ref2 = B.MapRef(eng2, recs)
    pile2 = B.ModPileup(eng2, ref2)
    x = B.Batch(dm, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_modpileup(pile2)
    assert "another engine" in str(ei.value)
    x.close()
    pile2.close()
    ref2.close()
    eng2.close()
    foreign.close()
    other.close()
    pile.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_map_mods(tmp_path):
    import modbase_ref as MB
    from test_cli import FAST5LIB, FLAPPIE, RUNNIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop_r941native5mC.h"), M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 14
    for i, n in enumerate(rng.integers(1500, 4000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, batch="16", fmt="sam"):
        r = subprocess.run([FLAPPIE, "--model", "r941_5mC", "--batch", batch, "--format", fmt] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    tagged, _ = run(["--modbase-tags"])                       # SEQ (Z written as C) and the bytes of its Cs, one line a read
    seqs, mls, order = {}, {}, []
    for ln in tagged.splitlines():
        f = ln.split("\t")
        assert len(f) == 13 and f[11].startswith("MM:Z:")
        seqs[f[0]], mls[f[0]] = f[9], MB.spread_ml(f[9], MB.ml_values(f[12]))
        order.append(f[0])
    assert len(order) == nread
    krng = np.random.default_rng(5)
    records = ["", "", ""]
    for i, nm in enumerate(order[:-2]):                       # two reads have no place
        x = R.edit(krng, seqs[nm], 0.05)
        records[i % 3] += rand_seq(krng, 200 + 31 * i) + (x if i % 2 == 0 else R.revcomp(x))
    records = [r + rand_seq(krng, 150) for r in records]
    records[2] = records[2].lower()                           # lower case is upper-cased as --map does
    names, lens = ["chrA", "plasmid.1", "third"], [len(r) for r in records]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join(r[k:k + 70] for k in range(0, len(r), 70))) for nm, r in zip(names, records)))
    on_c = sorted(v for nm in order for c, v in zip(seqs[nm], mls[nm]) if c == "C")
    lo, hi = on_c[len(on_c) // 3], on_c[2 * len(on_c) // 3]
    assert 0 <= lo < hi <= 255, (lo, hi)

    FILES = ("hits.tsv", "acc.tsv", "aln.sam", "pileup.tsv", "mods.bed", "hist.tsv")

    def files(tag):
        return {k: tmp_path / ("%s_%s" % (tag, k)) for k in FILES}

    def options(f, mods, extra=()):
        return ["--map", str(fa), "--map-out", str(f["hits.tsv"]), "--truth-from-map", "--truth-out", str(f["acc.tsv"]), "--map-sam", str(f["aln.sam"]),
                "--map-pileup", str(f["pileup.tsv"])] + \
            (["--map-mods", str(f["mods.bed"]), "--map-mods-hist", str(f["hist.tsv"]), "--map-mods-lo", str(lo), "--map-mods-hi", str(hi)] + list(extra) if mods else [])

    def summary(err, keys):
        return [ln for ln in err.splitlines() if ln.split("\t")[0] in keys]

    # the run without the option, then the run with it: stdout and every other file unchanged, --map-pileup's table among them
    f0 = files("without")
    out0, err0 = run(["--modbase-tags"] + options(f0, False))
    assert out0 == tagged and summary(err0, ("mods_pileup",)) == [] and len(summary(err0, ("pileup",))) == 9
    f1 = files("b16")
    out1, err1 = run(["--modbase-tags"] + options(f1, True))
    assert out1 == out0 and summary(err1, ("map", "truth", "pileup")) == summary(err0, ("map", "truth", "pileup"))
    for k in ("hits.tsv", "acc.tsv", "aln.sam", "pileup.tsv"):
        assert f1[k].read_bytes() == f0[k].read_bytes() and f1[k].stat().st_size > 0, k
    # mods.bed and hist.tsv rebuilt from acc.tsv (the CIGAR in signal order), hits.tsv (record, strand, span), the calls and the ML tags of the same run
    want = MP.ModPileup(lens, records, 0, lo, hi)
    hit = {f[0]: f for f in (ln.split("\t") for ln in f1["hits.tsv"].read_text().splitlines())}
    strands = set()
    for f in (ln.split("\t") for ln in f1["acc.tsv"].read_text().splitlines()):
        if f[1] != "1":
            continue
        h = hit[f[0]]
        assert h[1] == "1" and f[13:] == h[4:8]
        k, minus, a, b = names.index(h[4]), h[5] == "-", int(h[6]), int(h[7])
        ops = [T.OPS.index(c) for cnt, c in re.findall(r"(\d+)([=XID])", f[12]) for _ in range(int(cnt))]
        want.add(2 * k + minus, lens[k] - b if minus else a, lens[k] - a if minus else b, seqs[f[0]], mls[f[0]], ops)
        strands.add(h[5])
    t = want.totals
    assert t["reads"] >= nread - 4 and strands == {"+", "-"} and min(t[c] for c in MP.COLUMNS) > 0 and int((want.hist > 0).sum()) >= 8, t
    bed, hist = f1["mods.bed"].read_text(), f1["hist.tsv"].read_text()
    assert bed == want.bed(names) and hist == want.hist_tsv() and len(hist.splitlines()) == 256
    got = {k: int(v) for k, v in (ln.split("\t")[1:] for ln in summary(err1, ("mods_pileup",)))}
    assert got == want.stderr_lines() and list(got) == list(MP.TOTALS) + ["rows"] and got["rows"] == len(bed.splitlines()) > 0, (got, want.stderr_lines())
    rows = [ln.split("\t") for ln in bed.splitlines()]
    assert {r[5] for r in rows} == {"+", "-"} and {r[0] for r in rows} == set(names)
    assert sum(int(r[11]) for r in rows) <= got["mod"] and all(records[names.index(r[0])][int(r[1])].upper() == ("C" if r[5] == "+" else "G") for r in rows)
    # the same files at two other batch sizes (one without --modbase-tags: no tag appears, the bytes are made all the same) and with --reverse
    plain, _ = run([])
    for tag, extra, batch in (("b4", [], "4"), ("b64", ["--modbase-tags"], "64"), ("rev", ["--modbase-tags", "--reverse"], "16")):
        f2 = files(tag)
        out2, err2 = run(extra + options(f2, True), batch)
        assert out2 == (plain if tag == "b4" else out1) or tag == "rev", tag
        assert "MM:Z:" not in out2 or extra, tag
        for k in FILES:
            assert f2[k].read_bytes() == f1[k].read_bytes(), (tag, k)
        assert summary(err2, ("mods_pileup",)) == summary(err1, ("mods_pileup",)), tag
    # the other motif, and combine-strands, against the restatement's writer
    for tag, extra, motif, combine in (("c", ["--map-mods-motif", "C"], "C", False), ("comb", ["--map-mods-motif", "CG", "--map-mods-combine-strands"], "CG", True)):
        f2 = files(tag)
        out2, err2 = run(["--modbase-tags"] + options(f2, True, extra))
        assert out2 == out1 and f2["mods.bed"].read_text() == want.bed(names, motif, combine) and f2["hist.tsv"].read_text() == hist, tag
        assert summary(err2, ("mods_pileup",)) == ["mods_pileup\t%s\t%d" % kv for kv in want.stderr_lines(motif, combine).items()], tag
        rows2 = [ln.split("\t") for ln in f2["mods.bed"].read_text().splitlines()]
        assert len(rows2) > len(rows) if motif == "C" else (0 < len(rows2) <= len(rows) and {r[5] for r in rows2} == {"."}), tag      # (every read lies on one strand: a CpG's two rows become one only where reads of both strands cover it)
    # a model without a modified base is refused, and so is runnie
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    f3 = files("lstm")
    r = subprocess.run([FLAPPIE, "--model", "r941_native"] + options(f3, True) + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and r.stdout == "" and "--map-mods needs a model with a modified base (r941_5mC); \"r941_native\" has none" in r.stderr
    r = subprocess.run([RUNNIE, "--map-mods", str(f3["mods.bed"]), str(reads)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and r.stdout == "" and "--map-mods and its --map-mods-* options are flappie's" in r.stderr
    assert not f3["mods.bed"].exists()
