"""flappie --map-consensus on the GPU: per reference position, the forward letters, deletions and INSERTED letters of all aligned reads of all batches, and the
consensus called from them (include/ffhip.h "consensus": ffhip_consensus_*, ffhip_batch_set_consensus, FFHIP_RUN_CONSENSUS, ffhip_op_consensus; the kernels
k_consensus and k_consensus_call).

  * the operator against consensus_ref.py on a reference of three records (off_k != 0): op counts at the wave and chunk edges of the prefix counts, insertion runs
    that straddle ops 63|64 and 255|256 on each strand, runs of 8, 9 and 20, runs at j = 0 and j = m, runs directly behind and ahead of a deletion, spans touching
    position 0 and M_k - 1, calls with Z; reset; the identity test; its refusals;
  * 64 random alignments that share positions, added in two orders: the same bytes as the restatement;
  * the call kernel on the hostile counts of tests/test_consensus.py, reached through the operator: cells byte-equal to consensus_ref.call;
  * batches (one read a row, ragged with an empty slot, packed, paired): planes and totals equal consensus_ref over the batch's own final map(), truth() and
    basecall(), and planes 0 .. 4 equal the strand sum of a pileup attached to the same runs; a second run doubles every counter; the records of the run are those of
    the run without the flag; two batches in flight into one object give the sum; another batch size and a packed batch give the same bytes; after an f32 re-run
    every read is counted once;
  * the refusals of the flag and of ffhip_batch_set_consensus, with their texts;
  * the `flappie` binary: every read written three times, a reference from the calls with a substitution, a missing base and an extra pair planted in every
    stretch, 300 bases and more from its ends (the reads have 6500 .. 9000 samples: this model calls about 0.15 bases a sample, and a call has to hold the two
    margins and the three differences, test_consensus.SHORTEST = 770 bases): the consensus gives every call back; cons.fa, changes.tsv and the lines of stderr rebuilt from acc.tsv, hits.tsv and the calls; the same files at two
    batch sizes and with --reverse; everything else unchanged.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import consensus_ref as CR
import map_ref as R
import pileup_ref as PU
import truth_ref as T
from test_barcodes_gpu import _packed_batch, _records, rand_seq
from test_consensus import HOSTILE_MIN_DEPTH, HOSTILE_REF, HOSTILE_WANT, MARGIN, SHORTEST, hostile_alignments, planted_reference, restored
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
    if counts.tobytes() != want.counts.tobytes():
        bad = np.argwhere(counts != want.counts)
        raise AssertionError((where, len(bad), [(tuple(int(v) for v in ix), int(counts[tuple(ix)]), int(want.counts[tuple(ix)])) for ix in bad[:8]]))


# ------------------------------------------------------------------------------------ the operator
OP_COUNTS = (1, 64, 256, 257, 513)
LENS = (1000, 64, 777)


def _call(rng, ops):
    return "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, int((np.asarray(ops) != 3).sum())))


def operator_cases(rng):
    """(what, q, tstart, tend, call, ops): every op count in four kinds on both strands at either end of a record that holds it, then the runs the kernel's
    neighbour reads are aimed at"""
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
            m = int((ops != 2).sum())
            for k in sorted({min((k for k in range(3) if LENS[k] >= m), key=lambda k: LENS[k]), 2 if m <= LENS[2] else 0}):
                for o in (0, 1):
                    for at_end in (0, 1):                      # touching position 0 of the search, and its last: either end of the record on either strand
                        ts = LENS[k] - m if at_end else 0
                        out.append(((K, kind), 2 * k + o, ts, ts + m, _call(rng, ops), ops))
    eq = lambda n: [0] * n                                       # noqa: E731
    runs = {"3 over ops 63|64": eq(62) + [2] * 3 + eq(10), "3 over ops 255|256": eq(254) + [2] * 3 + eq(10), "2, =, 1 over 63|64": eq(62) + [2, 2] + eq(1) + [2] + eq(9),
            "20 over ops 255|256": eq(250) + [2] * 20 + eq(5), "9 that ends at op 63": eq(55) + [2] * 9 + eq(70), "9 that begins at op 256": eq(256) + [2] * 9 + eq(3),
            "8": eq(5) + [2] * 8 + eq(5), "9": eq(5) + [2] * 9 + eq(5), "20": eq(5) + [2] * 20 + eq(5),
            "at j = 0 and j = m": [2] * 3 + eq(10) + [2] * 4, "9 at j = 0": [2] * 9 + eq(3), "20 at j = m": eq(2) + [2] * 20,
            "behind a D": eq(4) + [3] + [2] * 2 + eq(4), "ahead of a D": eq(4) + [2] * 2 + [3] + eq(4), "between two D": eq(3) + [3] + [2] * 9 + [3] + eq(3),
            "X I X": [1, 2, 1], "512 I between two =": [0] + [2] * 512 + [0]}
    for what, ops in runs.items():
        ops = np.array(ops, np.uint8)
        m = int((ops != 2).sum())
        for o in (0, 1):
            for k, ts in ((0, 0), (2, LENS[2] - m), (0, 301)):  # touching position 0, touching M_k - 1, inside
                out.append((what, 2 * k + o, ts, ts + m, _call(rng, ops), ops))
    return out


def test_operator_at_the_edges(B, engine):
    rng = np.random.default_rng(53)
    recs = [rand_seq(rng, m) for m in LENS]
    ref = B.MapRef(engine, recs)
    cons = B.Consensus(engine, ref)
    assert cons.positions == sum(LENS)
    want = CR.Consensus(LENS)
    assert_same(cons.download(), want, "created")
    cases = operator_cases(rng)
    assert {c[1] & 1 for c in cases} == {0, 1} and {c[1] >> 1 for c in cases} == {0, 1, 2} and any("Z" in c[4] for c in cases)
    for i, (what, q, ts, te, call, ops) in enumerate(cases):
        if not isinstance(what, tuple):                        # the aimed runs: each alone first, so that a wrong one is named
            cons.reset()
            w1 = CR.Consensus(LENS)
            B.op_consensus(engine, cons, q, ts, te, call, ops)
            w1.add(q, ts, te, call, ops)
            assert_same(cons.download(), w1, (what, q, ts, te))
            continue
        B.op_consensus(engine, cons, q, ts, te, call, ops)
        want.add(q, ts, te, call, ops)
        if what[1] != "=" or i % 8 == 0:                       # several alignments added into one object before it is looked at
            assert_same(cons.download(), want, (what, q, ts, te))
    # the aimed runs once more, all into one object on top of each other
    cons.reset()
    want.reset()
    for what, q, ts, te, call, ops in cases:
        B.op_consensus(engine, cons, q, ts, te, call, ops)
        want.add(q, ts, te, call, ops)
    assert_same(cons.download(), want, "all")
    t = want.totals
    assert t["reads"] == len(cases) and min(t[k] for k in ("bases", "del", "ins_bases", "long_ins", "edge_ins")) > 0
    # the long_ins of the runs of 8, 9 and 20 alone: 0, 1 and 12 on either strand
    for run, longs in ((8, 0), (9, 1), (20, 12)):
        for q in (0, 1, 4, 5):
            cons.reset()
            ops = [0] * 5 + [2] * run + [0] * 5
            B.op_consensus(engine, cons, q, 40, 50, _call(rng, ops), ops)
            tot = cons.download()[1]
            assert (tot["long_ins"], tot["ins_bases"], tot["edge_ins"], tot["bases"]) == (longs, run - longs, 0, 10), (run, q, tot)
    cons.reset()
    want.reset()
    assert_same(cons.download(), want, "reset")
    # the identity test inside the kernel: 3 matches in 4 columns, equality passes
    for min_id, counted in ((750, 1), (751, 0)):
        c2, w2 = B.Consensus(engine, ref, min_id), CR.Consensus(LENS, min_id)
        B.op_consensus(engine, c2, 5, 3, 7, "AZG", [0, 0, 3, 0])
        w2.add(5, 3, 7, "AZG", [0, 0, 3, 0])
        assert w2.totals["reads"] == counted and w2.totals["skipped"] == 1 - counted
        assert_same(c2.download(), w2, min_id)
        c2.close()
    c2 = B.Consensus(engine, ref, -7)                         # negative: 0
    B.op_consensus(engine, c2, 0, 0, 1, "", [3])
    assert c2.download()[1]["reads"] == 1
    c2.close()
    # every refusal of ffhip_op_pileup, and nothing added by any
    eq = [0, 0, 0]
    for q, a, b, call, ops, text in ((-1, 0, 3, "ACG", eq, "search"), (6, 0, 3, "ACG", eq, "search"), (2, -1, 2, "ACG", eq, "span"), (2, 62, 65, "ACG", eq, "span"),
                                     (2, 3, 3, "", [], "span"), (2, 5, 4, "", [], "span"), (2, 0, 3, "ACN", eq, "not one of A C G T Z"),
                                     (2, 0, 3, "AcG", eq, "not one of A C G T Z"), (2, 0, 3, "ACG", [0, 4, 0], "not one of 0 .. 3"), (2, 0, 3, "ACG", [0, 0], "consume"),
                                     (2, 0, 3, "ACG", [0, 0, 0, 0], "consume"), (2, 0, 3, "AC", eq, "consume"), (2, 0, 3, "ACG", [0, 0, 3, 3], "consume"),
                                     (2, 0, 3, "ACG", [0, 0, 0, 2], "consume")):
        with pytest.raises(B.FFHipError) as ei:
            B.op_consensus(engine, cons, q, a, b, call, ops)
        assert text in str(ei.value) and "consensus: " in str(ei.value), (q, a, b, call, ops, str(ei.value))
    with pytest.raises(B.FFHipError) as ei:
        B.Consensus(engine, ref, 1001)
    assert "0 .. 1000" in str(ei.value)
    assert_same(cons.download(), want, "after the refusals")
    cons.close()
    ref.close()


def test_random_alignments_in_two_orders(B, engine):
    rng = np.random.default_rng(59)
    lens = (700, 300, 500)
    recs = [rand_seq(rng, m) for m in lens]
    ref = B.MapRef(engine, recs)
    alns = []
    for it in range(64):                                       # spans of up to 700 with 10 % edits; most lie over the same few hundred positions
        k = it % 3
        m = int(rng.integers(lens[k] // 2, lens[k] + 1))
        ts = int(rng.integers(0, lens[k] - m + 1))
        ops, j = [], 0
        while j < m:
            op = int(rng.choice(4, p=(0.9, 0.04, 0.03, 0.03)))
            if op == 2 and rng.random() < 0.3:
                ops += [2] * int(rng.integers(1, 11))
            ops.append(op)
            j += op != 2
        alns.append((2 * k + int(rng.integers(0, 2)), ts, ts + m, _call(rng, ops), np.array(ops, np.uint8)))
    want = CR.Consensus(lens)
    for a in alns:
        want.add(*a)
    assert int(want.depth().max()) >= 15 and want.totals["long_ins"] > 0 and want.totals["ins_bases"] > 100, want.totals
    cons = B.Consensus(engine, ref)
    first = None
    for order in (range(64), rng.permutation(64)):
        cons.reset()
        for i in order:
            B.op_consensus(engine, cons, *alns[int(i)])
        got = cons.download()
        assert_same(got, want, "order")
        first = first or got
        assert got[0].tobytes() == first[0].tobytes() and got[1] == first[1]
    cells = cons.call(3)
    assert cells.tobytes() == CR.call(want.counts, CR.ref_codes(recs), 3).tobytes()
    cons.close()
    ref.close()


# ------------------------------------------------------------------------------------ the call kernel
def test_the_call_kernel_on_hostile_counts(B, engine):
    rng = np.random.default_rng(61)
    recs = [rand_seq(rng, 333), HOSTILE_REF, rand_seq(rng, 70)]
    lens = [len(r) for r in recs]
    ref = B.MapRef(engine, recs)
    cons = B.Consensus(engine, ref)
    want = CR.Consensus(lens)
    for aln in hostile_alignments(k=1):
        B.op_consensus(engine, cons, *aln)
        want.add(*aln)
    for k in (0, 2):                                           # the other records: full depth with a letter changed, a base dropped and one put in
        for _ in range(HOSTILE_MIN_DEPTH):
            x = recs[k]
            call = x[:20] + "ACGT"[("ACGT".index(x[20]) + 1) % 4] + x[21:40] + x[41:50] + "Z" + x[50:]
            aln = (2 * k, 0, lens[k], call, [0] * 20 + [1] + [0] * 19 + [3] + [0] * 9 + [2] + [0] * (lens[k] - 50))
            B.op_consensus(engine, cons, *aln)
            want.add(*aln)
    assert_same(cons.download(), want, "hostile")
    codes = CR.ref_codes(recs)
    for min_depth in (HOSTILE_MIN_DEPTH, 1, 3, 5, 65535):
        cells = cons.call(min_depth)
        ref_cells = CR.call(want.counts, codes, min_depth)
        assert cells.dtype == CR.CELL and cells.shape == (sum(lens),)
        if cells.tobytes() != ref_cells.tobytes():
            bad = [int(g) for g in np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(cells, ref_cells)])]
            raise AssertionError((min_depth, [(g, cells[g], ref_cells[g]) for g in bad[:8]]))
    cells = cons.call(HOSTILE_MIN_DEPTH)
    for pos, (s, what, depth) in HOSTILE_WANT.items():        # ... and by hand
        c = cells[lens[0] + pos]
        assert (CR.letters(c), int(c["what"]), int(c["depth"]), int(c["n"])) == (s, what, depth, len(s)), (pos, c)
    assert_same(cons.download(), want, "the call changes no counter")
    for bad in (0, -1):
        with pytest.raises(B.FFHipError) as ei:
            cons.call(bad)
        assert "min_depth" in str(ei.value)
    cons.reset()
    cells = cons.call(1)                                       # nothing covered: the reference in lower case
    assert "".join(CR.letters(c) for c in cells) == "".join(recs).lower() and not cells["what"].any() and not cells["depth"].any()
    cons.close()
    ref.close()


# ------------------------------------------------------------------------------------ batches
def _run(bs, fl):
    if len(bs) == 1:
        bs[0].run(1.0, fl)
    else:
        bs[0].run_pair(bs[1], 1.0, fl)
    for x in bs:
        x.finish()


def _expected(bs, slots, lens, min_identity=0):
    """consensus_ref and pileup_ref accumulated over the batches' own final records; and what was seen"""
    want, pile = CR.Consensus(lens, min_identity), PU.Pileup(lens, min_identity)
    seen = {"reads": 0, "plus": 0, "minus": 0, "not mapped": 0}
    for k, v in slots:
        mp, tr = bs[k].map(v), bs[k].truth(v)
        want.add_read(mp, tr, bs[k].basecall(v))
        pile.add_read(mp, tr, bs[k].basecall(v))
        ok = mp["status"] == 1 and tr["status"] == 1
        seen["reads"] += 1
        seen["plus"] += ok and not mp["q"] & 1
        seen["minus"] += ok and mp["q"] & 1
        seen["not mapped"] += mp["status"] != 1
    return want, pile, seen


def with_gaps(rec):
    """the record with two or three adjacent bases cut out every 97: reference_of's edits are single letters, and the calls shall INSERT runs of letters too"""
    return "".join(rec[x + 2 + (x // 97) % 2:x + 97] for x in range(0, len(rec), 97))


def _batches_into_a_consensus(B, engine, bs, nreads, flags, where, band=48, window=-1, e=-1, empty=(), reruns=None):
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    _run(bs, flags)
    calls = [bs[k].basecall(v) for k, v in slots]
    recs = [with_gaps(r) for r in reference_of(np.random.default_rng(23), calls)]
    lens = [len(r) for r in recs]
    ref = B.MapRef(engine, recs)
    for x in bs:
        x.set_map(ref, window, e)
        x.set_truth_from_map(True, band)
    fl = flags | B.RUN_MAP | B.RUN_TRUTH
    _run(bs, fl)                                              # without the flag
    plain = {kv: (bs[kv[0]].map(kv[1]), bs[kv[0]].truth(kv[1])) for kv in slots}
    held = [x.device_bytes() for x in bs]
    cons, pile = B.Consensus(engine, ref), B.Pileup(engine, ref)
    for x in bs:
        x.set_consensus(cons)
        x.set_pileup(pile)
    _run(bs, fl | B.RUN_CONSENSUS | B.RUN_PILEUP)
    if reruns is not None:
        assert reruns(bs[0].f32_reruns()), bs[0].f32_reruns()
    for kv, call in zip(slots, calls):                        # everything the run returns is what the same run returns without the flag
        k, v = kv
        assert bs[k].basecall(v) == call and np.array_equal(bs[k].map(v)["raw"], plain[kv][0]["raw"]) and same_truth(bs[k].truth(v), plain[kv][1]), (where, kv)
    assert [x.device_bytes() for x in bs] == held, where       # the counters are the object's, not the batch's
    want, pwant, seen = _expected(bs, slots, lens)
    got = cons.download()
    assert_same(got, want, where)
    pcounts, ptotals = pile.download()                        # planes 0 .. 4 are the strand sum of the pileup of the same runs
    assert ptotals == pwant.totals and np.array_equal(got[0][:5], pcounts[0, :5] + pcounts[1, :5]), where
    assert got[1]["ins_bases"] + got[1]["long_ins"] == ptotals["ins"] and got[1]["edge_ins"] == ptotals["edge_ins"] and got[1]["reads"] == ptotals["reads"], where
    # what keeps the test from passing empty
    t = want.totals
    assert t["reads"] * 4 >= seen["reads"] * 3 and seen["plus"] >= 2 and seen["minus"] >= 2 and seen["not mapped"] >= 1, (where, seen, t)
    assert t["bases"] > 0 and t["del"] > 0 and t["ins_bases"] > 0 and t["skipped"] == 0 and int(want.counts[9:].sum()) > 0, (where, t)
    assert cons.call(1).tobytes() == CR.call(want.counts, CR.ref_codes(recs), 1).tobytes(), where
    # a second run, with this flag alone, doubles every counter
    _run(bs, fl | B.RUN_CONSENSUS)
    counts, totals = cons.download()
    assert np.array_equal(counts, 2 * want.counts) and totals == {k: 2 * v for k, v in want.totals.items()}, where
    assert pile.download()[1] == ptotals, where
    cons.close()
    pile.close()
    for x in bs:
        x.set_consensus(None)
        x.set_pileup(None)
        x.set_truth(None)
        x.set_map(None)
    ref.close()


def test_rows_ragged_packed_paired(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=1))
    rng = np.random.default_rng(256)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
    _batches_into_a_consensus(B, engine, [b], [16], B.RUN_NO_TRACE, "rows")
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(1500, 2501, 13)) + [0, 2600, 1800] + list(rng.integers(1500, 2501, 4))]
    b = B.Batch(dm, 20, 2600)
    b.set_signals_ragged(sigs)
    _batches_into_a_consensus(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, "ragged", band=100, window=128, e=200, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 5000, 24, rng, lo=1500, hi=2500)
    _batches_into_a_consensus(B, engine, [pb], [n], B.RUN_NO_TRACE, "packed", band=64)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, 2000)
        x.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
        pair.append(x)
    _batches_into_a_consensus(B, engine, pair, [16, 16], B.RUN_NO_TRACE, "pair", band=32)
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
    _batches_into_a_consensus(B, engine, [b], [16], 0, "rerun rows", reruns=lambda r: r == 2)
    b.close()
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


def _attached(B, dm, ref, cons, sig, band=48):
    b = B.Batch(dm, sig.shape[0], sig.shape[1])
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, band)
    b.set_consensus(cons)
    return b


def test_two_batches_in_flight_another_size_and_packed(B, engine, small):
    dm, sig, calls, recs, ref = small
    lens = [len(r) for r in recs]
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH | B.RUN_CONSENSUS
    # one batch of 16: the bytes everything below is held to
    cons = B.Consensus(engine, ref)
    b = _attached(B, dm, ref, cons, sig)
    b.run(1.0, fl)
    b.finish()
    want, _, seen = _expected([b], [(0, v) for v in range(16)], lens)
    one = cons.download()
    assert_same(one, want, "one batch")
    assert want.totals["reads"] >= 12 and seen["plus"] >= 2 and seen["minus"] >= 2 and want.totals["ins_bases"] > 0
    # two batches attached to one object, both between run and finish: the sum of the two
    other = np.ascontiguousarray(sig[::-1][:11])              # (eleven of the same reads in another order: they map onto this reference too)
    b2 = _attached(B, dm, ref, cons, other)
    cons.reset()
    b.run(1.0, fl)
    b2.run(1.0, fl)
    b.finish()
    b2.finish()
    want2, _, _ = _expected([b, b2], [(0, v) for v in range(16)] + [(1, v) for v in range(11)], lens)
    assert_same(cons.download(), want2, "two in flight")
    assert (want2.counts >= want.counts).all() and want.totals["reads"] + 8 <= want2.totals["reads"] < 2 * want.totals["reads"]
    cells = cons.call(2)                                      # depth 2 where both batches' copies of a read lie
    assert cells.tobytes() == CR.call(want2.counts, CR.ref_codes(recs), 2).tobytes() and int((cells["what"] != 0).sum()) > 1000
    b.close()
    b2.close()
    # the same reads through batches of another size: the same bytes
    cons.reset()
    halves = [_attached(B, dm, ref, cons, sig[:8]), _attached(B, dm, ref, cons, sig[8:])]
    for x in halves:
        x.run(1.0, fl)
    for x in halves:
        x.finish()
    got = cons.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "two batches of 8"
    for x in halves:
        x.close()
    # ... and packed, several reads a row, in another order
    cons.reset()
    order = [5, 0, 11, 3, 15, 8, 1, 13, 2, 7, 10, 4, 14, 6, 9, 12]
    sigs = [sig[v] for v in order]
    pb = B.Batch(dm, 8, 5000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < 16
    pb.set_signals_packed(sigs, slot, off)
    pb.set_map(ref)
    pb.set_truth_from_map(True, 48)
    pb.set_consensus(cons)
    pb.run(1.0, fl)
    pb.finish()
    assert [pb.basecall(i) for i in range(16)] == [calls[v] for v in order]
    got = cons.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "packed"
    pb.close()
    cons.close()


def test_the_refusals_and_their_texts(B, engine, small):
    dm, sig, calls, recs, ref = small
    cons = B.Consensus(engine, ref)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, 48)
    base = B.RUN_NO_TRACE
    full = base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_CONSENSUS

    def refused(flags, text):
        with pytest.raises(B.FFHipError) as ei:
            b.run(1.0, flags)
        assert text in str(ei.value), (text, str(ei.value))

    refused(full, "consensus: no consensus is attached to the batch (ffhip_batch_set_consensus)")
    b.set_consensus(cons)
    refused(full & ~B.RUN_TRUTH, "consensus: the run does not make the truth records (FFHIP_RUN_CONSENSUS goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)")
    refused(full & ~B.RUN_MAP, "consensus: the run does not make the map records (FFHIP_RUN_CONSENSUS goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)")
    refused(base | B.RUN_CONSENSUS, "consensus: the run does not make the truth records")
    other = B.MapRef(engine, recs)                            # the same letters, another reference
    foreign = B.Consensus(engine, other)
    b.set_consensus(foreign)
    refused(full, "consensus: the attached consensus belongs to another reference than the batch's map reference")
    b.set_consensus(cons)
    b.set_truth([np.zeros(5, np.uint8)] * 16, 48)             # outside the mode: host truths
    refused(full, "consensus: the batch is not in the mode of truth from map (ffhip_batch_set_truth_from_map)")
    b.set_truth_from_map(True, 48)
    b.run(1.0, full & ~B.RUN_CONSENSUS)                       # everything else the run returns is that of the run without the flag
    b.finish()
    plain = [(b.basecall(v), b.map(v), b.truth(v)) for v in range(16)]
    b.run(1.0, full)
    for c in (None, cons):                                    # not between a run and its finish
        with pytest.raises(B.FFHipError) as ei:
            b.set_consensus(c)
        assert "consensus: the batch is between a run and its finish" in str(ei.value)
    b.finish()
    for v, (call, mp, tr) in enumerate(plain):
        assert b.basecall(v) == call and np.array_equal(b.map(v)["raw"], mp["raw"]) and same_truth(b.truth(v), tr), v
    counts, totals = cons.download()
    assert totals["reads"] >= 12 and int(foreign.download()[0].sum()) == 0 and foreign.download()[1]["reads"] == 0      # no refused run added anything, anywhere
    b.set_consensus(None)
    b.run(1.0, full & ~B.RUN_CONSENSUS)                       # detached, without the flag: as before
    b.finish()
    assert cons.download()[1] == totals
    b.close()
    rle = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    x = B.Batch(rle, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_consensus(cons)
    assert "consensus: a flip-flop model only" in str(ei.value)
    x.set_consensus(None)
    x.close()
    rle.close()
    eng2 = B.Engine(0)                                        # another engine's object
    ref2 = B.MapRef(eng2, recs)
    cons2 = B.Consensus(eng2, ref2)
    x = B.Batch(dm, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_consensus(cons2)
    assert "consensus: the consensus belongs to another engine" in str(ei.value)
    x.close()
    with pytest.raises(B.FFHipError) as ei:
        B.Consensus(engine, ref2)
    assert "a reference of this engine" in str(ei.value)
    cons2.close()
    ref2.close()
    eng2.close()
    foreign.close()
    other.close()
    cons.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_map_consensus(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread, copies = 12, 3
    for i, n in enumerate(rng.integers(6500, 9000, nread)):    # (samples enough for calls of SHORTEST bases and more: the margins and the three differences fit)
        raw = synth_raw(rng, int(n))
        for c in range(copies):                                # every read three times under different ids: depth 3 everywhere, three identical alignments
            write_fast5(reads / ("read_%02d_%d.fast5" % (i, c)), "uuid-%04d-%d" % (i, c), raw)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, batch="16"):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", batch, "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    fq = _records(default, "fastq")
    assert len(fq) == nread * copies
    calls = {r[0]: r[1] for r in fq}
    firsts = sorted(nm for nm in calls if nm.endswith("-0"))
    assert len(firsts) == nread and all(calls[nm[:-1] + str(c)] == calls[nm] for nm in firsts for c in range(copies))
    print("call lengths", sorted(len(calls[nm]) for nm in firsts))      # (seen with -s)
    assert min(len(calls[nm]) for nm in firsts) >= SHORTEST, "a call too short for the margins"
    records, places = planted_reference(np.random.default_rng(5), [calls[nm] for nm in firsts])
    names, lens = ["chrA", "plasmid.1", "third"], [len(r) for r in records]
    off = [sum(lens[:k]) for k in range(3)]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join(r[k:k + 70] for k in range(0, len(r), 70))) for nm, r in zip(names, records)))

    def files(tag):
        return {k: tmp_path / ("%s_%s" % (tag, k)) for k in ("hits.tsv", "acc.tsv", "aln.sam", "pileup.tsv", "cons.fa", "changes.tsv")}

    def options(f, consensus):
        return ["--map", str(fa), "--map-out", str(f["hits.tsv"]), "--truth-from-map", "--truth-out", str(f["acc.tsv"]), "--map-sam", str(f["aln.sam"]),
                "--map-pileup", str(f["pileup.tsv"])] + \
            (["--map-consensus", str(f["cons.fa"]), "--map-consensus-changes", str(f["changes.tsv"]), "--map-consensus-min-depth", "3"] if consensus else [])

    def summary(err, keys):
        return [ln for ln in err.splitlines() if ln.split("\t")[0] in keys]

    out, without = {}, {}
    for tag, extra, batch, base in (("b16", [], "16", None), ("b4", [], "4", "b16"), ("rev", ["--reverse"], "16", None)):
        f1 = files(tag)
        if base is None:                                       # the run without the option (another batch size: the same run's files)
            f0 = files(tag + "_without")
            without[tag] = (f0,) + run(options(f0, False) + extra, batch)
        f0, out0, err0 = without[base or tag]
        out1, err1 = run(options(f1, True) + extra, batch)
        assert out1 == out0 and summary(err1, ("map", "truth", "pileup")) == summary(err0, ("map", "truth", "pileup")) and summary(err0, ("consensus",)) == []
        for k in ("hits.tsv", "acc.tsv", "aln.sam", "pileup.tsv"):
            assert f1[k].read_bytes() == f0[k].read_bytes(), (tag, k)
        # the planes, rebuilt from acc.tsv (the CIGAR in signal order), hits.tsv (record, strand, span) and the calls
        want = CR.Consensus(lens)
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
        assert want.totals["reads"] == nread * copies and strands == {"+", "-"}, want.totals
        cells = CR.call(want.counts, CR.ref_codes(records), 3)
        got = {k: f1[k].read_text() for k in ("cons.fa", "changes.tsv")}
        assert got["cons.fa"] == CR.fasta(names, lens, cells), tag
        assert got["changes.tsv"] == CR.changes(names, records, cells, want.counts), tag
        lines = "".join(ln + "\n" for ln in err1.splitlines() if ln.startswith("consensus\t"))
        assert lines == CR.stderr_text(want.totals, cells), (tag, lines)
        # the consensus gives every call back: over a read's stretch without MARGIN at either end, the read's own call (turned for the - strand)
        for (text, call), (k, a, b, strand, y) in zip(restored(cells, off, places), places):
            assert text == call and len(call) >= 170, (tag, k, a, b, strand)
        tot = CR.stderr_lines(want.totals, cells)
        assert tot["sub"] >= nread and tot["del"] >= 2 * nread and tot["ins"] >= nread and tot["low_depth"] > 0 and tot["skipped"] == 0, tot
        rows = got["changes.tsv"].splitlines()
        assert len(rows) >= 4 * nread and all(len(r.split("\t")) == 7 for r in rows)
        out[tag] = (got, lines)
    assert out["b16"] == out["b4"] == out["rev"]
