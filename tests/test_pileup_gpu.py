"""flappie --map-pileup on the GPU: per reference position, the counts of all aligned reads of all batches (include/ffhip.h "pileup": ffhip_pileup_*,
ffhip_batch_set_pileup, FFHIP_RUN_PILEUP, ffhip_op_pileup; the kernel k_pileup).

  * the operator against pileup_ref.py on a reference with records of 1, 15, 16, 17, 33 and 100 bases -- and one of 1100 between them, since a path of 1025 '='
    needs a span of 1025 -- on both strands, spans touching either end, op counts at the wave and chunk edges of the prefix counts, each as all '=', all 'D', 'I' at
    both edges and random mixes; several alignments in one pileup; reset; its refusals;
  * batches (one read a row, ragged with an empty slot, packed, paired): planes and totals equal pileup_ref over the batch's own final map(), truth() and
    basecall(); a second run doubles every counter; the records of the run are those of the run without the flag; min_identity moves exactly the reads below it
    from `reads` to `skipped`; two batches in flight into one pileup give the sum; another batch size and a packed batch give the same bytes;
  * after an f32 re-run every read is counted once, from the final records (the fall-back to the launch-per-step kernels cannot be taken without a launch that
    times out and is not tested: it rests on where ffhip_batch_finish launches the kernel);
  * the refusals of the flag and of ffhip_batch_set_pileup, with their texts;
  * the `flappie` binary: pileup.tsv rebuilt from acc.tsv, hits.tsv and the calls; the same table at two batch sizes and with --reverse; everything else unchanged.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import map_ref as R
import pileup_ref as PU
import truth_ref as T
from test_barcodes_gpu import _packed_batch, _records, rand_seq
from test_maptruth_gpu import reference_of, same_truth

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
    counts, totals = got
    assert counts.dtype == np.uint32 and counts.shape == want.counts.shape, (where, counts.shape)
    assert totals == want.totals, (where, totals, want.totals)
    if not np.array_equal(counts, want.counts):
        bad = np.argwhere(counts != want.counts)
        raise AssertionError((where, len(bad), [(tuple(int(v) for v in ix), int(counts[tuple(ix)]), int(want.counts[tuple(ix)])) for ix in bad[:8]]))


# ------------------------------------------------------------------------------------ the operator
OP_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
LENS = (1, 15, 16, 1100, 17, 33, 100)


def operator_cases(rng):
    """(q, tstart, tend, call, ops) for every op count in four kinds, on both strands, on the shortest records that hold them, at either end of the record"""
    out = []
    for K in OP_COUNTS:
        kinds = {"=": np.zeros(K, np.uint8), "D": np.full(K, 3, np.uint8)}
        if K >= 3:
            kinds["I..I"] = np.array([2] + [0] * (K - 2) + [2], np.uint8)
        else:
            kinds["I"] = None                                  # (one op cannot be an insertion: it consumes no truth base; below as 'I' around one '=')
        for s in range(3):
            mix = rng.choice(4, size=K, p=(0.55, 0.15, 0.15, 0.15)).astype(np.uint8)
            if (mix != 2).sum() == 0:
                mix[int(rng.integers(0, K))] = 0
            kinds["mix%d" % s] = mix
        for kind, ops in kinds.items():
            if ops is None:
                ops = np.array([2, 0, 2], np.uint8)
            m, n = int((ops != 2).sum()), int((ops != 3).sum())
            fits = sorted((k for k, Mk in enumerate(LENS) if Mk >= m), key=lambda k: LENS[k])
            for k in {fits[0], fits[-1], 6 if m <= LENS[6] else 3}:      # the shortest record that holds the span, the longest, the last
                for o in (0, 1):
                    for at_end in (0, 1):
                        ts = LENS[k] - m if at_end else 0
                        call = "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n))
                        out.append((K, kind, 2 * k + o, ts, ts + m, call, ops))
    for k in (1, 2, 4, 5):                                     # the records between: filled by one path of '=', and by a mix, on both strands
        for o in (0, 1):
            Mk = LENS[k]
            mix = rng.choice(4, size=Mk, p=(0.55, 0.15, 0.15, 0.15)).astype(np.uint8)
            mix[0] = 0
            for kind, ops in (("=", np.zeros(Mk, np.uint8)), ("mix", mix)):
                m, n = int((ops != 2).sum()), int((ops != 3).sum())
                ts = (Mk - m) if o else 0
                out.append((int(ops.size), kind, 2 * k + o, ts, ts + m, "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n)), ops))
    return out


def test_operator_at_the_wave_and_chunk_edges(B, engine):
    rng = np.random.default_rng(41)
    recs = [rand_seq(rng, m) for m in LENS]
    ref = B.MapRef(engine, recs)
    pile = B.Pileup(engine, ref)
    assert pile.positions == sum(LENS)
    want = PU.Pileup(LENS)
    assert_same(pile.download(), want, "created")
    cases = operator_cases(rng)
    assert {c[0] for c in cases} >= set(OP_COUNTS) and {c[2] & 1 for c in cases} == {0, 1} and {c[2] >> 1 for c in cases} == set(range(len(LENS)))
    for i, (K, kind, q, ts, te, call, ops) in enumerate(cases):
        B.op_pileup(engine, pile, q, ts, te, call, ops)
        want.add(q, ts, te, call, ops)
        if kind != "=" or i % 8 == 0:                          # several alignments added into one pileup before it is looked at
            assert_same(pile.download(), want, (K, kind, q, ts, te))
    assert_same(pile.download(), want, "all")
    assert want.totals["reads"] == len(cases) and min(want.totals[k] for k in ("match", "mismatch", "del", "ins", "edge_ins")) > 0
    pile.reset()
    want.reset()
    assert_same(pile.download(), want, "reset")
    # the identity test inside the kernel: 3 matches in 4 columns, equality passes
    for min_id, counted in ((750, 1), (751, 0)):
        p2, w2 = B.Pileup(engine, ref, min_id), PU.Pileup(LENS, min_id)
        B.op_pileup(engine, p2, 9, 3, 7, "AZG", [0, 0, 3, 0])
        w2.add(9, 3, 7, "AZG", [0, 0, 3, 0])
        assert w2.totals["reads"] == counted and w2.totals["skipped"] == 1 - counted
        assert_same(p2.download(), w2, min_id)
        p2.close()
    p2 = B.Pileup(engine, ref, -7)                            # negative: 0
    B.op_pileup(engine, p2, 0, 0, 1, "", [3])
    assert p2.download()[1]["reads"] == 1
    p2.close()
    # every refusal, and nothing added by any
    eq = [0, 0, 0]
    for q, a, b, call, ops, text in ((-1, 0, 3, "ACG", eq, "search"), (14, 0, 3, "ACG", eq, "search"), (2, -1, 2, "ACG", eq, "span"), (2, 13, 16, "ACG", eq, "span"),
                                     (2, 3, 3, "", [], "span"), (2, 5, 4, "", [], "span"), (0, 0, 2, "AC", [0, 0], "span"), (2, 0, 3, "ACN", eq, "not one of A C G T Z"),
                                     (2, 0, 3, "AcG", eq, "not one of A C G T Z"), (2, 0, 3, "ACG", [0, 4, 0], "not one of 0 .. 3"), (2, 0, 3, "ACG", [0, 0], "consume"),
                                     (2, 0, 3, "ACG", [0, 0, 0, 0], "consume"), (2, 0, 3, "AC", eq, "consume"), (2, 0, 3, "ACG", [0, 0, 3, 3], "consume"),
                                     (2, 0, 3, "ACG", [0, 0, 0, 2], "consume")):
        with pytest.raises(B.FFHipError) as ei:
            B.op_pileup(engine, pile, q, a, b, call, ops)
        assert text in str(ei.value), (q, a, b, call, ops, str(ei.value))
    with pytest.raises(B.FFHipError) as ei:
        B.Pileup(engine, ref, 1001)
    assert "0 .. 1000" in str(ei.value)
    assert_same(pile.download(), want, "after the refusals")
    pile.close()
    ref.close()


# ------------------------------------------------------------------------------------ batches
def permille(tr):
    return 1000 * tr["n_match"] // (tr["n_match"] + tr["n_mismatch"] + tr["n_ins"] + tr["n_del"])


def _run(bs, fl):
    if len(bs) == 1:
        bs[0].run(1.0, fl)
    else:
        bs[0].run_pair(bs[1], 1.0, fl)
    for x in bs:
        x.finish()


def _expected(bs, slots, lens, min_identity=0):
    """pileup_ref accumulated over the batches' own final records; and what was seen"""
    want = PU.Pileup(lens, min_identity)
    seen = {"reads": 0, "plus": 0, "minus": 0, "not mapped": 0}
    for k, v in slots:
        mp, tr = bs[k].map(v), bs[k].truth(v)
        want.add_read(mp, tr, bs[k].basecall(v))
        ok = mp["status"] == 1 and tr["status"] == 1
        seen["reads"] += 1
        seen["plus"] += ok and not mp["q"] & 1
        seen["minus"] += ok and mp["q"] & 1
        seen["not mapped"] += mp["status"] != 1
    return want, seen


def _batches_into_a_pileup(B, engine, bs, nreads, flags, where, band=48, window=-1, e=-1, empty=(), reruns=None):
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    _run(bs, flags)
    calls = [bs[k].basecall(v) for k, v in slots]
    recs = reference_of(np.random.default_rng(23), calls)
    lens = [len(r) for r in recs]
    ref = B.MapRef(engine, recs)
    for x in bs:
        x.set_map(ref, window, e)
        x.set_truth_from_map(True, band)
    fl = flags | B.RUN_MAP | B.RUN_TRUTH
    _run(bs, fl)                                              # without the flag
    plain = {kv: (bs[kv[0]].map(kv[1]), bs[kv[0]].truth(kv[1])) for kv in slots}
    held = [x.device_bytes() for x in bs]
    pile = B.Pileup(engine, ref)
    for x in bs:
        x.set_pileup(pile)
    _run(bs, fl | B.RUN_PILEUP)
    if reruns is not None:
        assert reruns(bs[0].f32_reruns()), bs[0].f32_reruns()
    for kv, call in zip(slots, calls):                        # everything the run returns is what the same run returns without the flag
        k, v = kv
        assert bs[k].basecall(v) == call and np.array_equal(bs[k].map(v)["raw"], plain[kv][0]["raw"]) and same_truth(bs[k].truth(v), plain[kv][1]), (where, kv)
    assert [x.device_bytes() for x in bs] == held, where       # the counters are the pileup's, not the batch's
    want, seen = _expected(bs, slots, lens)
    assert_same(pile.download(), want, where)
    # what keeps the test from passing empty
    t = want.totals
    assert t["reads"] * 4 >= seen["reads"] * 3 and seen["plus"] >= 2 and seen["minus"] >= 2 and seen["not mapped"] >= 1, (where, seen, t)
    assert t["mismatch"] > 0 and t["del"] > 0 and t["ins"] > 0 and t["skipped"] == 0, (where, t)
    # a second run doubles every counter
    _run(bs, fl | B.RUN_PILEUP)
    counts, totals = pile.download()
    assert np.array_equal(counts, 2 * want.counts) and totals == {k: 2 * v for k, v in want.totals.items()}, where
    pile.close()
    # min_identity from the batch's own records, so that it splits the reads: exactly those below it go from `reads` to `skipped`
    vals = sorted(permille(bs[k].truth(v)) for k, v in slots if bs[k].map(v)["status"] == 1 and bs[k].truth(v)["status"] == 1)
    cut = vals[-1]
    below = sum(x < cut for x in vals)
    assert 0 < below < len(vals), (where, vals)
    strict = B.Pileup(engine, ref, cut)
    for x in bs:
        x.set_pileup(strict)
    _run(bs, fl | B.RUN_PILEUP)
    want2, _ = _expected(bs, slots, lens, cut)
    assert (want2.totals["reads"], want2.totals["skipped"]) == (len(vals) - below, below) and want2.totals["reads"] + below == want.totals["reads"], (where, want2.totals)
    assert_same(strict.download(), want2, (where, cut))
    for x in bs:
        x.set_pileup(None)
        x.set_truth(None)
        x.set_map(None)
    strict.close()
    ref.close()


def test_rows_ragged_packed_paired(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=1))
    rng = np.random.default_rng(256)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
    _batches_into_a_pileup(B, engine, [b], [16], B.RUN_NO_TRACE, "rows")
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(1500, 2501, 13)) + [0, 2600, 1800] + list(rng.integers(1500, 2501, 4))]
    b = B.Batch(dm, 20, 2600)
    b.set_signals_ragged(sigs)
    _batches_into_a_pileup(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, "ragged", band=100, window=128, e=200, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 5000, 24, rng, lo=1500, hi=2500)
    _batches_into_a_pileup(B, engine, [pb], [n], B.RUN_NO_TRACE, "packed", band=64)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, 2000)
        x.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
        pair.append(x)
    _batches_into_a_pileup(B, engine, pair, [16, 16], B.RUN_NO_TRACE, "pair", band=32)
    for x in pair:
        x.close()
    dm.close()


def test_every_read_is_counted_once_after_an_f32_rerun(B, engine):
    # the outlier case every re-run test of the suite uses (H = 128, these signals): the outlier's reads come from the side batch, whose records are patched into
    # this batch's before the kernel is launched
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _batches_into_a_pileup(B, engine, [b], [16], 0, "rerun rows", reruns=lambda r: r == 2)
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _batches_into_a_pileup(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", band=300, reruns=lambda r: r >= 2)
    pb.close()
    dm.close()


@pytest.fixture(scope="module")
def small(B, engine):
    """one model, the signals of 16 reads and a reference from their calls, shared by the tests below"""
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=3))
    rng = np.random.default_rng(31)
    sig = rng.standard_normal((16, 2000)).astype(np.float32)
    b = B.Batch(dm, 16, 2000)
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
    b.set_pileup(pile)
    return b


def test_two_batches_in_flight_another_size_and_packed(B, engine, small):
    dm, sig, calls, recs, ref = small
    lens = [len(r) for r in recs]
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP
    # one batch of 16: the bytes everything below is held to
    pile = B.Pileup(engine, ref)
    b = _attached(B, dm, ref, pile, sig)
    b.run(1.0, fl)
    b.finish()
    want, seen = _expected([b], [(0, v) for v in range(16)], lens)
    one = pile.download()
    assert_same(one, want, "one batch")
    assert want.totals["reads"] >= 12 and seen["plus"] >= 2 and seen["minus"] >= 2 and want.totals["ins"] > 0
    # two batches attached to one pileup, both between run and finish: the sum of the two
    other = np.ascontiguousarray(sig[::-1][:11])              # (eleven of the same reads in another order: they map onto this reference too)
    b2 = _attached(B, dm, ref, pile, other)
    pile.reset()
    b.run(1.0, fl)
    b2.run(1.0, fl)
    b.finish()
    b2.finish()
    want2, _ = _expected([b, b2], [(0, v) for v in range(16)] + [(1, v) for v in range(11)], lens)
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
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "two batches of 8"
    for x in halves:
        x.close()
    # ... and packed, several reads a row, in another order
    pile.reset()
    order = [5, 0, 11, 3, 15, 8, 1, 13, 2, 7, 10, 4, 14, 6, 9, 12]
    sigs = [sig[v] for v in order]
    pb = B.Batch(dm, 8, 5000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < 16
    pb.set_signals_packed(sigs, slot, off)
    pb.set_map(ref)
    pb.set_truth_from_map(True, 48)
    pb.set_pileup(pile)
    pb.run(1.0, fl)
    pb.finish()
    assert [pb.basecall(i) for i in range(16)] == [calls[v] for v in order]
    got = pile.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "packed"
    pb.close()
    pile.close()


def test_the_refusals_and_their_texts(B, engine, small):
    dm, sig, calls, recs, ref = small
    pile = B.Pileup(engine, ref)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, 48)
    base = B.RUN_NO_TRACE

    def refused(flags, text):
        with pytest.raises(B.FFHipError) as ei:
            b.run(1.0, flags)
        assert text in str(ei.value), (text, str(ei.value))

    refused(base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP, "no pileup is attached")
    b.set_pileup(pile)
    refused(base | B.RUN_MAP | B.RUN_PILEUP, "does not make the truth records")
    refused(base | B.RUN_TRUTH | B.RUN_PILEUP, "pileup: the run does not make the map records")
    refused(base | B.RUN_PILEUP, "does not make the truth records")
    other = B.MapRef(engine, recs)                            # the same letters, another reference
    foreign = B.Pileup(engine, other)
    b.set_pileup(foreign)
    refused(base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP, "another reference")
    b.set_pileup(pile)
    b.set_truth([np.zeros(5, np.uint8)] * 16, 48)             # outside the mode: host truths
    refused(base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP, "not in the mode of truth from map")
    b.set_truth_from_map(True, 48)
    b.run(1.0, base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP)
    for p in (None, pile):                                    # not between a run and its finish
        with pytest.raises(B.FFHipError) as ei:
            b.set_pileup(p)
        assert "between a run and its finish" in str(ei.value)
    b.finish()
    counts, totals = pile.download()
    assert totals["reads"] >= 12 and int(foreign.download()[0].sum()) == 0 and foreign.download()[1]["reads"] == 0      # no refused run added anything, anywhere
    b.set_pileup(None)
    b.run(1.0, base | B.RUN_MAP | B.RUN_TRUTH)                # detached, without the flag: as before
    b.finish()
    assert pile.download()[1] == totals
    b.close()
    rle = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    x = B.Batch(rle, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_pileup(pile)
    assert "flip-flop model only" in str(ei.value)
    x.set_pileup(None)
    x.close()
    rle.close()
    foreign.close()
    other.close()
    pile.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_map_pileup(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 14
    for i, n in enumerate(rng.integers(1500, 4000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, batch="16"):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", batch, "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    fq = _records(default, "fastq")
    assert len(fq) == nread
    calls = {r[0]: r[1] for r in fq}
    order = [r[0] for r in fq]
    krng = np.random.default_rng(5)
    records = ["", "", ""]
    for i, nm in enumerate(order[:-2]):                       # two reads have no place
        x = R.edit(krng, calls[nm].replace("Z", "C"), 0.05)
        records[i % 3] += rand_seq(krng, 200 + 31 * i) + (x if i % 2 == 0 else R.revcomp(x))
    records = [r + rand_seq(krng, 150) for r in records]
    names, lens = ["chrA", "plasmid.1", "third"], [len(r) for r in records]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join(r[k:k + 70] for k in range(0, len(r), 70))) for nm, r in zip(names, records)))

    def files(tag):
        return {k: tmp_path / ("%s_%s" % (tag, k)) for k in ("hits.tsv", "acc.tsv", "aln.sam", "pileup.tsv")}

    def options(f, pileup):
        return ["--map", str(fa), "--map-out", str(f["hits.tsv"]), "--truth-from-map", "--truth-out", str(f["acc.tsv"]), "--map-sam", str(f["aln.sam"])] + \
            (["--map-pileup", str(f["pileup.tsv"])] if pileup else [])

    def summary(err, keys):
        return [ln for ln in err.splitlines() if ln.split("\t")[0] in keys]

    tables, without = {}, {}
    for tag, extra, batch, base in (("b16", [], "16", None), ("b4", [], "4", "b16"), ("rev", ["--reverse"], "16", None)):
        f1 = files(tag)
        if base is None:                                       # the run without the option (another batch size: the same run's files)
            f0 = files(tag + "_without")
            without[tag] = (f0,) + run(options(f0, False) + extra, batch)
        f0, out0, err0 = without[base or tag]
        out1, err1 = run(options(f1, True) + extra, batch)
        assert out1 == out0 and summary(err1, ("map", "truth")) == summary(err0, ("map", "truth")) and summary(err0, ("pileup",)) == []
        for k in ("hits.tsv", "acc.tsv", "aln.sam"):
            assert f1[k].read_bytes() == f0[k].read_bytes(), (tag, k)
        # the table, rebuilt from acc.tsv (the CIGAR in signal order), hits.tsv (record, strand, span) and the calls
        want = PU.Pileup(lens)
        hit = {f[0]: f for f in (ln.split("\t") for ln in f1["hits.tsv"].read_text().splitlines())}
        strands = set()
        for f in (ln.split("\t") for ln in f1["acc.tsv"].read_text().splitlines()):
            if f[1] != "1":
                continue
            h = hit[f[0]]
            assert h[1] == "1" and f[13:] == h[4:8]
            k, minus, a, b = names.index(h[4]), h[5] == "-", int(h[6]), int(h[7])
            ops = [T.OPS.index(c) for cnt, c in re.findall(r"(\d+)([=XID])", f[12]) for _ in range(int(cnt))]
            want.add(2 * k + minus, lens[k] - b if minus else a, lens[k] - a if minus else b, calls[f[0]], ops)
            strands.add(h[5])
        t = want.totals
        assert t["reads"] >= nread - 4 and strands == {"+", "-"} and min(t[k] for k in ("mismatch", "del", "ins")) > 0, t
        tables[tag] = f1["pileup.tsv"].read_text()
        assert tables[tag] == want.tsv(names, records), tag
        got = {k: int(v) for k, v in (ln.split("\t")[1:] for ln in err1.splitlines() if ln.startswith("pileup\t"))}
        assert got == want.stderr_lines() and list(got) == ["reads", "skipped", "positions", "covered", "match", "mismatch", "del", "ins", "edge_ins"], (got, want.stderr_lines())
        rows = [[int(x) for x in ln.split("\t")[3:]] for ln in tables[tag].splitlines()]
        assert sum(r[0] >= 1 for r in rows) == got["covered"] and len(rows) == got["positions"] == sum(lens)
        assert sum(sum(r[1:5]) + sum(r[7:11]) for r in rows) == got["match"] + got["mismatch"] and sum(r[5] + r[11] for r in rows) == got["del"]
        assert sum(r[6] + r[12] for r in rows) == got["ins"]
    assert tables["b16"] == tables["b4"] == tables["rev"]
