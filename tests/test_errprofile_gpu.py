"""flappie --truth-errors on the GPU: by class, what the aligned calls of all reads of all batches got right and wrong (include/ffhip.h "error profile":
ffhip_errprofile_*, ffhip_batch_set_errprofile, FFHIP_RUN_ERRPROFILE, ffhip_op_errprofile, ffhip_op_errprofile_mapped; the kernel k_errprofile).

  * both operators against errprofile_ref.py, case by case, byte for byte: K of 1, 63, 64, 65, 255, 256, 257 and 513 ops; a homopolymer run and each of its two gaps
    across a wave edge (ops 63|64) and a chunk edge (255|256); runs of 16 and 17; runs of exactly 64 and of 65 ops; 32 and 33 called letters; runs touching either end
    of the truth; m of 1 .. 5; n = 0; Z in call and truth; quality bytes below '!' and above '~'; an alignment below min_identity.  The mapped operator takes the same
    truths from a reference that is their concatenation -- the first at the record's first base, the last at its last -- on the + strand of one record and the -
    strand of its reverse complement; reset; the refusals, which add nothing;
  * random alignments, some below min_identity, added in two orders: the same bytes as the restatement;
  * batches in both truth modes (one read a row, ragged with an empty slot, packed, paired, the launch-per-step kernels, after an f32 re-run): the counters equal
    errprofile_ref over the batch's OWN final truth(), basecall(), quality() and the truths given or the stretch of its map(); a second run doubles every counter;
    the records of the run are those of the run without the flag;
  * the same 16 reads through two batches of 8 in flight into one object, a packed batch in another order, a refilled batch, the launch-per-step kernels and one, two
    and five workgroups: the same bytes as one batch of 16; reset zeroes the object;
  * the refusals of the flag and of ffhip_batch_set_errprofile, with their texts;
  * the `flappie` binary, once in each truth mode: errors.tsv and the lines of stderr rebuilt from the run's own FASTQ, acc.tsv (the CIGAR), refs.fa or hits.tsv and
    ref.fa; the same files at two batch sizes and with --reverse; everything else unchanged.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import errprofile_ref as ER
import map_ref as R
import truth_ref as T
from test_barcodes_gpu import _packed_batch, _records
from test_consensus_gpu import with_gaps
from test_errprofile import alignment_of, hand_cases, random_alignments, random_truth
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
    assert counts.dtype == np.uint64 and counts.shape == want.counts.shape, (where, counts.shape)
    assert totals == want.totals, (where, totals, want.totals)
    if counts.tobytes() != want.counts.tobytes():
        bad = np.flatnonzero(counts != want.counts)
        raise AssertionError((where, len(bad), [(int(ix), int(counts[ix]), int(want.counts[ix])) for ix in bad[:8]]))


# ------------------------------------------------------------------------------------ the operators
OP_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)


def placed_run(at, r, f, b, tail=5):
    """a run of r C whose first op is op `at`, f inserted C ahead of it and b behind it, among matches of a truth that alternates A and G"""
    pre = at - f
    alt = lambda n, s=0: [(0, 2)[(x + s) % 2] for x in range(n)]
    truth = alt(pre) + [1] * r + alt(tail, 1)
    ops = [0] * pre + [2] * f + [0] * r + [2] * b + [0] * tail
    call = alt(pre) + [1] * (f + r + b) + alt(tail, 1)
    s = "".join("ACGT"[c] for c in call)
    assert ops[at] == 0 and ops[at - 1] == (2 if f else 0) and len(ops) == len(s)
    return s, bytes(33 + (x % 60) for x in range(len(s))), np.array(truth, np.uint8), np.array(ops, np.uint8)


def operator_cases(rng):
    cases = list(hand_cases())
    for K in OP_COUNTS:                                           # K ops exactly, of every kind
        while True:
            aln = alignment_of(rng, random_truth(rng, max(1, (2 * K) // 3)), ins_rate=0.3, long_ins=0.0)
            if len(aln[3]) >= K and aln[3][K - 1] != 2 and aln[3][0] != 2:
                break
        ops = aln[3][:K]
        n, m = int((ops != 3).sum()), int((ops != 2).sum())
        cases.append(("K%d" % K, (aln[0][:n], aln[1][:n], aln[2][:m], ops)))
    for edge in (64, 256):
        cases.append(("run over %d" % edge, placed_run(edge - 3, 6, 2, 2)))          # the run's ops edge - 3 .. edge + 2
        cases.append(("F over %d" % edge, placed_run(edge + 2, 5, 4, 1)))            # F: ops edge - 2 .. edge + 1
        cases.append(("B over %d" % edge, placed_run(edge - 7, 5, 1, 4)))            # B: ops edge - 2 .. edge + 1
        cases.append(("64 ops over %d" % edge, placed_run(edge - 10, 12, 30, 22)))
        cases.append(("65 ops over %d" % edge, placed_run(edge - 10, 12, 30, 23)))
    cases.append(("run at the ops' end", placed_run(40, 6, 3, 5, tail=1)))
    return cases


def concatenated(cases):
    """the cases' truths as one text, and each one's span in it"""
    text, spans = "", []
    for _, (_, _, truth, _) in cases:
        spans.append((len(text), len(text) + len(truth)))
        text += "".join("ACGT"[c] for c in ER.fold(truth))
    return text, spans


def test_both_operators_case_by_case(B, engine):
    cases = operator_cases(np.random.default_rng(77))
    assert {"K%d" % K for K in OP_COUNTS} <= {nm for nm, _ in cases} and all(len(c[3]) == K for K in OP_COUNTS for nm, c in cases if nm == "K%d" % K)
    text, spans = concatenated(cases)
    recs = [text, "ACGTTGCA" * 9 + "ACGTACGT", R.revcomp(text)]               # y_0 = y_5 = text: the + strand of record 0 and the - strand of record 2 (off_k != 0)
    ref = B.MapRef(engine, recs)
    assert spans[0][0] == 0 and spans[-1][1] == len(text)         # a stretch at the record's first base and one at its last, on both strands
    p = B.ErrProfile(engine)
    seen = {k: 0 for k in ER.TOTALS}
    for (name, aln), (a, b) in zip(cases, spans):
        call, qual, truth, ops = aln
        want = ER.ErrProfile()
        want.add(*aln)
        for k in ER.TOTALS:
            seen[k] += want.totals[k]
        p.reset()
        B.op_errprofile(engine, p, call, qual, truth, ops)
        assert_same(p.download(), want, name)
        for q in (0, 5):
            assert ER.mapped_truth(recs, q, a, b) == ER.fold(truth)
            p.reset()
            B.op_errprofile_mapped(engine, p, ref, q, a, b, call, qual, ops)
            assert_same(p.download(), want, (name, "mapped", q))
    assert seen["hp_long"] >= 3 and seen["hp_wide"] >= 3 and seen["edge_ins"] > 0 and seen["ctx_sites"] > 500 and seen["hp_runs"] > 100, seen
    # reset zeroes the object
    p.reset()
    counts, totals = p.download()
    assert not counts.any() and not any(totals.values())
    # below min_identity: skipped and nothing else; at it: counted
    aln = ("ACGAACGT", b"55555555", np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8), np.array([0, 0, 0, 1, 0, 0, 0, 0], np.uint8))
    for mi, counted in ((876, False), (875, True)):
        strict, want = B.ErrProfile(engine, mi), ER.ErrProfile(mi)
        want.add(*aln)
        want.add(*aln)
        B.op_errprofile(engine, strict, *aln)
        B.op_errprofile_mapped(engine, strict, ref, 2, 72, 80, aln[0], aln[1], aln[3])      # (the same truth, at the end of record 1)
        assert_same(strict.download(), want, ("identity", mi))
        assert (want.totals["reads"], want.totals["skipped"]) == ((2, 0) if counted else (0, 2))
        strict.close()
    # the refusals: what ffhip_op_pileup refuses; nothing is added by any
    def refused(text, fn, *args):
        with pytest.raises(B.FFHipError) as ei:
            fn(engine, p, *args)
        assert text in str(ei.value), (text, str(ei.value))
    t4, o4 = np.array([0, 1, 2, 3], np.uint8), np.zeros(4, np.uint8)
    refused("is not one of A C G T Z", B.op_errprofile, "ACNT", b"!!!!", t4, o4)
    refused("the ops consume", B.op_errprofile, "ACGT", b"!!!!", t4, np.zeros(3, np.uint8))
    refused("the ops consume", B.op_errprofile, "ACG", b"!!!", t4, o4)
    refused("code 4 is not one of 0 .. 3", B.op_errprofile, "ACGT", b"!!!!", t4, np.array([0, 0, 4, 0], np.uint8))
    refused("code 5 is not one of 0 .. 4", B.op_errprofile, "ACGT", b"!!!!", np.array([0, 1, 5, 3], np.uint8), o4)
    refused("a truth of 1 or more bases", B.op_errprofile, "A", b"!", np.zeros(0, np.uint8), np.array([2], np.uint8))
    refused("is not a span of 1 or more", B.op_errprofile_mapped, ref, 0, 5, 5, "", b"", np.zeros(0, np.uint8))
    refused("is not a span of 1 or more", B.op_errprofile_mapped, ref, 0, len(text) - 2, len(text) + 2, "ACGT", b"!!!!", o4)
    refused("search 6 is not one of 0 .. 5", B.op_errprofile_mapped, ref, 6, 0, 4, "ACGT", b"!!!!", o4)
    counts, totals = p.download()
    assert not counts.any() and not any(totals.values())
    p.close()
    ref.close()


def test_random_alignments_in_two_orders(B, engine):
    rng = np.random.default_rng(2024)
    alns = random_alignments(rng, 48, max_m=700)
    want = ER.ErrProfile(350)
    for aln in alns:
        want.add(*aln)
    assert want.totals["reads"] >= 10 and want.totals["skipped"] >= 10 and want.totals["hp_runs"] > 100
    got = []
    for seed in (1, 2):
        p = B.ErrProfile(engine, 350)
        for x in np.random.default_rng(seed).permutation(len(alns)):
            B.op_errprofile(engine, p, *alns[int(x)])
        got.append(p.download())
        assert_same(got[-1], want, ("order", seed))
        p.close()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1] == got[1][1]


# ------------------------------------------------------------------------------------ batches
def _run(bs, fl):
    if len(bs) == 1:
        bs[0].run(1.0, fl)
    else:
        bs[0].run_pair(bs[1], 1.0, fl)
    for x in bs:
        x.finish()


def _quals(b, v):
    return b.quality(v).encode("latin-1")


def _expected(bs, slots, truths=None, recs=None, min_identity=0):
    """errprofile_ref accumulated over the batches' own final records -- the truths given (truths[(k, v)]) or the stretch of the read's own map record -- and what was seen"""
    want = ER.ErrProfile(min_identity)
    seen = {"reads": 0, "aligned": 0, "minus": 0}
    for k, v in slots:
        tr = bs[k].truth(v)
        seen["reads"] += 1
        seen["aligned"] += tr["status"] == 1
        if recs is not None:
            mp = bs[k].map(v)
            if mp["status"] != 1:
                assert tr["status"] != 1
                continue
            seen["minus"] += mp["q"] & 1
            want.add_read(tr, bs[k].basecall(v), _quals(bs[k], v), ER.mapped_truth(recs, mp["q"], mp["tstart"], mp["tend"]), mp)
        elif truths[(k, v)] is not None:
            want.add_read(tr, bs[k].basecall(v), _quals(bs[k], v), truths[(k, v)])
    return want, seen


def _edited_truth(rng, call, i):
    """a read's given truth: its call with edits, a C in five as Z's code where the model has one (it has not here), None for one read in eight"""
    if i % 8 == 7 or not call:
        return None
    x = call.replace("Z", "C")
    x = x[:40] + "A" * (3 + i % 9) + x[40:]                      # a homopolymer the call lacks
    return np.array([ER.CODE[c] for c in R.edit(rng, x, 0.06)], np.uint8)


def _batches_into_a_profile(B, engine, bs, nreads, flags, where, mode, band=48, empty=(), reruns=None):
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    _run(bs, flags)
    calls = {kv: bs[kv[0]].basecall(kv[1]) for kv in slots}
    rng = np.random.default_rng(23)
    ref = recs = truths = None
    fl = flags | B.RUN_TRUTH
    if mode == "map":
        recs = [with_gaps(r) for r in reference_of(rng, [calls[kv] for kv in slots])]
        ref = B.MapRef(engine, recs)
        for x in bs:
            x.set_map(ref)
            x.set_truth_from_map(True, band)
        fl |= B.RUN_MAP
    else:
        truths = {kv: _edited_truth(rng, calls[kv], i) for i, kv in enumerate(slots)}
        for k, x in enumerate(bs):
            x.set_truth([truths.get((k, v)) for v in range(nreads[k])], band)
    _run(bs, fl)                                              # without the flag
    plain = {kv: bs[kv[0]].truth(kv[1]) for kv in slots}
    held = [x.device_bytes() for x in bs]
    p = B.ErrProfile(engine)
    for x in bs:
        x.set_errprofile(p)
    _run(bs, fl | B.RUN_ERRPROFILE)
    if reruns is not None:
        assert reruns(bs[0].f32_reruns()), bs[0].f32_reruns()
    for kv in slots:                                          # everything the run returns is what the same run returns without the flag
        assert bs[kv[0]].basecall(kv[1]) == calls[kv] and same_truth(bs[kv[0]].truth(kv[1]), plain[kv]), (where, kv)
    assert [x.device_bytes() for x in bs] == held, where       # the counters are the object's, not the batch's
    want, seen = _expected(bs, slots, truths, recs)
    got = p.download()
    assert_same(got, want, where)
    t = want.totals                                           # what keeps the test from passing empty
    assert t["reads"] * 4 >= seen["reads"] * 2 and t["reads"] == seen["aligned"] and (mode != "map" or seen["minus"] >= 2), (where, seen, t)
    assert t["match"] > 1000 and t["mismatch"] > 0 and t["del"] > 0 and t["ins"] > 0 and t["ctx_sites"] > 1000 and t["hp_runs"] > 500 and t["skipped"] == 0, (where, t)
    _run(bs, fl | B.RUN_ERRPROFILE)                           # a second run doubles every counter
    counts, totals = p.download()
    assert np.array_equal(counts, 2 * want.counts) and totals == {k: 2 * v for k, v in want.totals.items()}, where
    p.close()
    for x in bs:
        x.set_errprofile(None)
        x.set_truth(None)
        x.set_map(None)
    if ref is not None:
        ref.close()


@pytest.mark.parametrize("mode", ("set", "map"))
def test_rows_ragged_packed_paired_stepwise(B, engine, mode):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=1))
    rng = np.random.default_rng(256)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
    _batches_into_a_profile(B, engine, [b], [16], B.RUN_NO_TRACE, "rows", mode)
    _batches_into_a_profile(B, engine, [b], [16], B.RUN_NO_TRACE | B.RUN_STEPWISE_RNN, "launch per step", mode, band=64)
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(1500, 2501, 13)) + [0, 2600, 1800] + list(rng.integers(1500, 2501, 4))]
    b = B.Batch(dm, 20, 2600)
    b.set_signals_ragged(sigs)
    _batches_into_a_profile(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, "ragged", mode, band=100, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 5000, 24, rng, lo=1500, hi=2500)
    _batches_into_a_profile(B, engine, [pb], [n], B.RUN_NO_TRACE, "packed", mode, band=64)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, 2000)
        x.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
        pair.append(x)
    _batches_into_a_profile(B, engine, pair, [16, 16], B.RUN_NO_TRACE, "pair", mode, band=32)
    for x in pair:
        x.close()
    dm.close()


@pytest.mark.parametrize("mode", ("set", "map"))
def test_every_read_is_counted_once_after_an_f32_rerun(B, engine, mode):
    # the outlier case every re-run test of the suite uses (H = 128, these signals): the outlier's reads come from the side batch, whose records are patched into
    # this batch's before the kernel is launched -- but not, in the mode of truth from map, the stretch the first pass gathered: the letters come from the map record
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _batches_into_a_profile(B, engine, [b], [16], 0, "rerun rows", mode, reruns=lambda r: r == 2)
    b.close()
    dm.close()


@pytest.fixture(scope="module")
def small(B, engine):
    """one model, the signals of 16 reads, their calls, a reference from the calls and a truth a read, shared by the tests below"""
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=3))
    rng = np.random.default_rng(31)
    sig = rng.standard_normal((16, 2000)).astype(np.float32)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    calls = [b.basecall(v) for v in range(16)]
    recs = reference_of(np.random.default_rng(37), calls)
    truths = [_edited_truth(np.random.default_rng(41 + v), calls[v], v) for v in range(16)]
    ref = B.MapRef(engine, recs)
    b.close()
    yield dm, sig, calls, recs, ref, truths
    ref.close()
    dm.close()


def _attached(B, dm, p, sig, mode, ref, truths, band=48, nsample=None):
    b = B.Batch(dm, len(sig), nsample or sig.shape[1])
    b.set_signals(sig)
    _mode(b, mode, ref, truths, band)
    b.set_errprofile(p)
    return b


def _mode(b, mode, ref, truths, band=48):
    if mode == "map":
        b.set_map(ref)
        b.set_truth_from_map(True, band)
    else:
        b.set_truth(truths, band)


@pytest.mark.parametrize("mode", ("set", "map"))
def test_the_same_reads_in_every_form_give_the_same_bytes(B, engine, small, mode):
    dm, sig, calls, recs, ref, truths = small
    fl = B.RUN_NO_TRACE | B.RUN_TRUTH | B.RUN_ERRPROFILE | (B.RUN_MAP if mode == "map" else 0)
    p = B.ErrProfile(engine)
    # one batch of 16: the bytes everything below is held to
    b = _attached(B, dm, p, sig, mode, ref, truths)
    b.run(1.0, fl)
    b.finish()
    want, seen = _expected([b], [(0, v) for v in range(16)], {(0, v): truths[v] for v in range(16)} if mode == "set" else None, recs if mode == "map" else None)
    one = p.download()
    assert_same(one, want, "one batch")
    assert want.totals["reads"] >= 12 and want.totals["hp_runs"] > 500 and want.totals["ins"] > 0
    # fewer workgroups than reads: a workgroup takes several entries
    for groups in (1, 2, 5, 0):
        p.reset()
        p.debug_groups(groups)
        b.run(1.0, fl)
        b.finish()
        got = p.download()
        assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), ("groups", groups)
    # the stretches k_truth read are not the source of a truth letter: zeroed behind k_truth, as a re-run whose map record moved leaves them stale, the same bytes
    if mode == "map":
        p.reset()
        b.run(1.0, fl)
        b.debug_clear_stretches()
        b.finish()
        assert [b.basecall(v) for v in range(16)] == calls
        got = p.download()
        assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "stretches cleared"
    # the launch-per-step kernels
    p.reset()
    b.run(1.0, fl | B.RUN_STEPWISE_RNN)
    b.finish()
    assert [b.basecall(v) for v in range(16)] == calls
    got = p.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "launch per step"
    # a refilled batch: the reads in another order first, every other one cut short, then these
    p.reset()
    b.set_signals_ragged([np.ascontiguousarray(x[:2000 - 500 * (v % 2)]) for v, x in enumerate(sig[::-1])])
    if mode == "set":
        b.set_truth(truths[::-1], 48)
    b.run(1.0, fl)
    b.finish()
    assert p.download()[1]["reads"] > 0
    p.reset()
    counts, totals = p.download()
    assert not counts.any() and not any(totals.values())         # reset zeroes the object
    b.set_signals(sig)
    if mode == "set":
        b.set_truth(truths, 48)
    b.run(1.0, fl)
    b.finish()
    got = p.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "refilled"
    b.close()
    # two batches of 8 sharing the object, both between run and finish
    p.reset()
    halves = [_attached(B, dm, p, sig[:8], mode, ref, truths[:8]), _attached(B, dm, p, sig[8:], mode, ref, truths[8:])]
    for x in halves:
        x.run(1.0, fl)
    for x in halves:
        x.finish()
    got = p.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "two batches of 8 in flight"
    for x in halves:
        x.close()
    # ... and packed, several reads a row, in another order
    p.reset()
    order = [5, 0, 11, 3, 15, 8, 1, 13, 2, 7, 10, 4, 14, 6, 9, 12]
    sigs = [sig[v] for v in order]
    pb = B.Batch(dm, 8, 5000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < 16
    pb.set_signals_packed(sigs, slot, off)
    _mode(pb, mode, ref, [truths[v] for v in order])
    pb.set_errprofile(p)
    pb.run(1.0, fl)
    pb.finish()
    assert [pb.basecall(i) for i in range(16)] == [calls[v] for v in order]
    got = p.download()
    assert got[1] == one[1] and got[0].tobytes() == one[0].tobytes(), "packed"
    pb.close()
    p.close()


def test_the_refusals_and_their_texts(B, engine, small):
    dm, sig, calls, recs, ref, truths = small
    p = B.ErrProfile(engine)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, 48)
    base = B.RUN_NO_TRACE
    full = base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_ERRPROFILE

    def refused(flags, text):
        with pytest.raises(B.FFHipError) as ei:
            b.run(1.0, flags)
        assert text in str(ei.value), (text, str(ei.value))

    refused(full, "error profile: no error profile is attached to the batch (ffhip_batch_set_errprofile)")
    b.set_errprofile(p)
    refused(full & ~B.RUN_TRUTH, "error profile: the run does not make the truth records (FFHIP_RUN_ERRPROFILE goes with FFHIP_RUN_TRUTH)")
    refused(full & ~B.RUN_MAP, "error profile: the run does not make the map records (in the mode of truth from map FFHIP_RUN_ERRPROFILE goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)")
    refused(base | B.RUN_ERRPROFILE, "error profile: the run does not make the truth records")
    refused(full | B.RUN_NO_DECODE, "")                       # as truth refuses it
    b.set_truth(truths, 48)                                   # a set truth: the map is neither required nor excluded
    for fl in (full & ~B.RUN_MAP, full):
        b.run(1.0, fl)
        for x in (None, p):                                   # not between a run and its finish
            with pytest.raises(B.FFHipError) as ei:
                b.set_errprofile(x)
            assert "error profile: the batch is between a run and its finish" in str(ei.value)
        b.finish()
    counts, totals = p.download()
    assert totals["reads"] >= 2 * 12 and not (counts % 2).any()   # the two runs added the same; no refused run added anything
    with pytest.raises(B.FFHipError) as ei:
        B.ErrProfile(engine, 1001)
    assert "min_identity is 1001 per mille (0 .. 1000)" in str(ei.value)
    b.set_errprofile(None)
    b.run(1.0, full & ~B.RUN_ERRPROFILE)                      # detached, without the flag: as before
    b.finish()
    assert p.download()[1] == totals
    b.close()
    rle = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    x = B.Batch(rle, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_errprofile(p)
    assert "error profile: a flip-flop model only" in str(ei.value)
    x.set_errprofile(None)
    x.close()
    rle.close()
    eng2 = B.Engine(0)                                        # another engine's object
    p2 = B.ErrProfile(eng2)
    x = B.Batch(dm, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_errprofile(p2)
    assert "error profile: the error profile belongs to another engine" in str(ei.value)
    with pytest.raises(B.FFHipError) as ei:
        B.op_errprofile(engine, p2, "A", b"!", [0], [0])
    assert "bad error profile arguments" in str(ei.value)
    x.close()
    p2.close()
    eng2.close()
    p.close()


# ------------------------------------------------------------------------------------ the binary
@pytest.mark.parametrize("mode", ("set", "map"))
def test_flappie_truth_errors(tmp_path, mode):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 10
    for i, n in enumerate(rng.integers(6500, 9000, nread)):       # (calls of 770 bases and more: ctx and hp are not empty)
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, batch="16"):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", batch, "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    fq = {r[0]: r for r in _records(default, "fastq")}
    assert len(fq) == nread
    calls = {nm: r[1] for nm, r in fq.items()}
    quals = {nm: r[2].encode("latin-1") for nm, r in fq.items()}
    assert all(len(quals[nm]) == len(calls[nm]) for nm in calls)
    names = sorted(calls)
    fa = tmp_path / "ref.fa"
    if mode == "map":
        records = reference_of(np.random.default_rng(5), [calls[nm] for nm in names])
        rnames, lens = ["chrA", "plasmid.1", "third"], [len(r) for r in records]
        fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join(r[k:k + 70] for k in range(0, len(r), 70))) for nm, r in zip(rnames, records)))
    else:
        # (a read in three is given its own call: identity 1000, what --truth-errors-min-identity 990 lets through)
        truth_of = {nm: calls[nm].replace("Z", "C") if i % 3 == 0 else "".join("ACGT"[c] for c in _edited_truth(np.random.default_rng(50 + i), calls[nm], i % 7))
                    for i, nm in enumerate(names)}
        fa.write_text("".join(">%s\n%s\n" % (nm, truth_of[nm]) for nm in names))

    def files(tag):
        return {k: tmp_path / ("%s_%s" % (tag, k)) for k in ("hits.tsv", "acc.tsv", "errors.tsv")}

    def options(f, errors, extra=()):
        head = ["--map", str(fa), "--map-out", str(f["hits.tsv"]), "--truth-from-map"] if mode == "map" else ["--truth", str(fa)]
        return head + ["--truth-out", str(f["acc.tsv"])] + (["--truth-errors", str(f["errors.tsv"])] + list(extra) if errors else [])

    def summary(err, keys):
        return [ln for ln in err.splitlines() if ln.split("\t")[0] in keys]

    out, without = {}, {}
    for tag, extra, batch, base, mi in (("b16", [], "16", None, 0), ("b4", [], "4", "b16", 0), ("rev", ["--reverse"], "16", None, 0), ("strict", [], "16", "b16", 990)):
        f1 = files(tag)
        if base is None:                                       # the run without the option (another batch size: the same run's files)
            f0 = files(tag + "_without")
            without[tag] = (f0,) + run(options(f0, False) + extra, batch)
        f0, out0, err0 = without[base or tag]
        out1, err1 = run(options(f1, True, ["--truth-errors-min-identity", str(mi)] if mi else []) + extra, batch)
        assert out1 == out0 and summary(err1, ("map", "truth")) == summary(err0, ("map", "truth")) and summary(err0, ("errors",)) == []
        for k in ("hits.tsv", "acc.tsv") if mode == "map" else ("acc.tsv",):
            assert f1[k].read_bytes() == f0[k].read_bytes(), (tag, k)
        # the counters, rebuilt from acc.tsv (the CIGAR in signal order), the calls and qualities of the FASTQ, and refs.fa or hits.tsv + ref.fa
        want = ER.ErrProfile(mi)
        hit = {f[0]: f for f in (ln.split("\t") for ln in f1["hits.tsv"].read_text().splitlines())} if mode == "map" else {}
        for f in (ln.split("\t") for ln in f1["acc.tsv"].read_text().splitlines()):
            if f[1] != "1":
                continue
            ops = [T.OPS.index(c) for cnt, c in re.findall(r"(\d+)([=XID])", f[12]) for _ in range(int(cnt))]
            if mode == "map":
                h = hit[f[0]]
                k, minus, a, b = rnames.index(h[4]), h[5] == "-", int(h[6]), int(h[7])
                truth = ER.mapped_truth(records, 2 * k + minus, lens[k] - b if minus else a, lens[k] - a if minus else b)
            else:
                truth = [ER.CODE[c] for c in truth_of[f[0]]]
            want.add(calls[f[0]], quals[f[0]], truth, ops)
        t = want.totals
        if mi == 0:
            assert t["reads"] >= nread - 3 and t["ctx_sites"] > 3000 and t["hp_runs"] > 1000 and t["ins"] > 0 and t["del"] > 0 and t["mismatch"] > 0, t
        else:
            assert t["reads"] >= 1 and t["skipped"] >= 1, t
        assert f1["errors.tsv"].read_text() == "".join(ln + "\n" for ln in want.tsv_lines()), tag
        lines = [ln for ln in err1.splitlines() if ln.startswith("errors\t")]
        assert lines == want.stderr_lines(), (tag, lines)
        out[tag] = f1["errors.tsv"].read_bytes()
    assert out["b16"] == out["b4"] == out["rev"] != out["strict"]
