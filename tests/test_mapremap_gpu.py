"""flappie --remap-from-map on the GPU: each read's signal mapped to the stretch of the reference its call was mapped to, in the run that mapped it (include/ffhip.h
"remap from map": ffhip_batch_set_remap_from_map, ffhip_op_map_remap_code, ffhip_debug_remap_from_map_form; the kernel k_map_remap_seq).

  * the coding kernel on one span equals the host's coding of the stretch: every strand of records of 100, 17 and 1 letters, every start 0 .. 33 and length up to 40,
    both alphabets, homopolymer runs of 63, 64, 65, 129 and 200 letters entered from inside, a room of m and of m - 1; its refusals;
  * batches: the one-run result IS the two-run result -- remap record, moves and events of a MAP | REMAP | EVENTS run in the mode equal, byte for byte, those of a
    second run given each mapped read's stretch through ffhip_batch_set_remap -- one read a row, ragged with an empty slot, packed, paired, after an f32 re-run, launch
    per step, refilled; and both equal remap_ref.py on the run's own transitions.  Reads whose room takes a larger kernel form than their L are among them;
  * together with truth from map in one run: neither changes the other's bytes;
  * the mode and ffhip_batch_set_remap replace each other; what a run in the mode refuses; the run-length model;
  * the buffers are sized from the reads' blocks alone and counted; a batch that never had the mode holds what the lengths of its sequences say;
  * a finished run in the mode makes no more copy calls than the two-run route's second run;
  * the `flappie` binary: one run against --map --map-records followed by --remap recs.fa.
Everything is integer- or byte-exact: no tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import map_ref as R
import mapremap_ref as MR
import maptruth_ref as MT
import remap_ref as RR

pytestmark = pytest.mark.gpu

WS_WORDS_A_BLOCK = {0: 1, 1: 4, 2: 16, 3: 72}             # 64-bit words of decisions a block, by remap's kernel form (a bit a cell of the form's window)


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def remap_form(B, L, band):
    return int(B.lib().ffhip_debug_remap_form(int(L), int(band)))


# ------------------------------------------------------------------------------------ the operator
def test_code_of_every_span_at_the_word_edges(B, engine):
    rng = np.random.default_rng(21)
    recs = [MR.rand_seq(rng, m) for m in (100, 17, 1)]
    ref = B.MapRef(engine, recs)
    ys = R.searches(recs)
    n = 0
    for nbase in (4, 5):
        for q, y in enumerate(ys):
            s = MT.codes(y)
            for start in range(0, 34):
                for length in range(1, 41):
                    if start + length > len(y):
                        break
                    got, status, L = B.op_map_remap_code(engine, ref, q, start, start + length, nbase, length)
                    want = MR.entries(s[start:start + length], nbase)
                    assert (status, L) == (1, length) and got.dtype == np.uint16 and np.array_equal(got, want), (nbase, q, start, length, got, want)
                    n += 1
    assert n == 2 * sum(min(40, len(y) - start) for y in ys for start in range(34) if start < len(y)) > 4000
    for q in range(6):                                        # whole records, either strand, in a room of one more and of one less
        m = len(ys[q])
        got, status, L = B.op_map_remap_code(engine, ref, q, 0, m, 4, m + 1)
        assert (status, L) == (1, m) and np.array_equal(got, MR.entries_by_remap_ref(MT.stretch(recs, q, 0, m), 4))
        got, status, L = B.op_map_remap_code(engine, ref, q, 0, m, 4, m - 1)
        assert (status, L) == (2, m) and (got == 0xffff).all(), (q, status, L, got)      # nothing written
    for q, a, b in ((-1, 0, 1), (6, 0, 1), (0, -1, 1), (4, 0, 2), (0, 1, 1), (2, 3, 3), (2, 5, 4), (0, 0, 101), (0, 100, 101), (3, 16, 18)):
        with pytest.raises(B.FFHipError):                     # the refusals of ffhip_op_map_stretch
            B.op_map_remap_code(engine, ref, q, a, b, 4, 200)
    for nbase, room in ((3, 10), (6, 10), (4, -1)):
        with pytest.raises(B.FFHipError):
            B.op_map_remap_code(engine, ref, 0, 0, 5, nbase, room)
    ref.close()


def test_code_of_runs_that_cross_the_passes_of_the_wave(B, engine):
    """a run's parity is carried from one pass of 64 letters to the next, and over a whole pass without a run start"""
    rng = np.random.default_rng(22)
    rec = ""
    for k, run in enumerate((63, 64, 65, 129, 200)):          # (a flank begins and ends with a letter that is neither neighbour's: the runs are as long as they say)
        rec += "ACGT"[(k + 1) % 4] + MR.rand_seq(rng, 5 + 3 * k) + "ACGT"[(k + 1) % 4] + "ACGT"[k % 4] * run
    rec += "G" + MR.rand_seq(rng, 70)
    ref = B.MapRef(engine, [rec])
    n = 0
    for q in (0, 1):
        s = MT.stretch([rec], q, 0, len(rec))
        edges = [0] + [i for i in range(1, len(s)) if s[i] != s[i - 1]]
        runs = [(a, b) for a, b in zip(edges, edges[1:] + [len(s)]) if b - a >= 63]
        assert sorted(b - a for a, b in runs) == [63, 64, 65, 129, 200]
        for a, b in runs:
            for start in sorted({max(a - 3, 0), max(a - 1, 0), a, a + 1, a + 2, a + 31, a + 62, a + 63}):
                for end in sorted({b - 1, b, b + 1, b + 2, min(b + 66, len(s)), len(s)}):
                    if not (start < end <= len(s)):
                        continue
                    for nbase in (4, 5):
                        m = end - start
                        got, status, L = B.op_map_remap_code(engine, ref, q, start, end, nbase, m)
                        want = MR.entries(s[start:end], nbase)
                        assert np.array_equal(want, MR.entries_by_remap_ref(s[start:end], nbase))
                        assert (status, L) == (1, m) and np.array_equal(got, want), (q, start, end, nbase, np.flatnonzero(got != want)[:5])
                        got, status, L = B.op_map_remap_code(engine, ref, q, start, end, nbase, m - 1)
                        assert (status, L) == (2, m) and (got == 0xffff).all()
                        n += 1
    assert n >= 400
    ref.close()


# ------------------------------------------------------------------------------------ batches
def _packed_batch(B, dm, rows, cap, lens, rng):
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    return pb, len(sigs)


def _run(bs, fl):
    if len(bs) == 1:
        bs[0].run(1.0, fl)
    else:
        bs[0].run_pair(bs[1], 1.0, fl)
    for x in bs:
        x.finish()


def same_remap(a, b):
    return (a["status"], a["L"], a["nblock"]) == (b["status"], b["L"], b["nblock"]) and np.float32(a["score"]).tobytes() == np.float32(b["score"]).tobytes() and \
        ((a["rm"] is None and b["rm"] is None) or (a["rm"] is not None and b["rm"] is not None and a["rm"].tobytes() == b["rm"].tobytes()))


def same_events(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.tobytes() == b.tobytes())


def _read_all(bs, slots):
    return {kv: (bs[kv[0]].map(kv[1]), bs[kv[0]].remap(kv[1]), bs[kv[0]].events(kv[1])) for kv in slots}


def _one_run_is_two_runs(B, engine, bs, nreads, flags, where, nbase, band=2048, window=-1, e=-1, empty=(), forms=2, check_ref=True, seed=23):
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    _run(bs, flags)
    calls = {kv: bs[kv[0]].basecall(kv[1]) for kv in slots}
    recs = MR.reference_of(np.random.default_rng(seed), [calls[kv] for kv in slots])
    ref = B.MapRef(engine, recs)
    fl = flags | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS
    for x in bs:
        x.set_map(ref, window, e)
        x.set_remap_from_map(True, band)
    _run(bs, fl)
    one = _read_all(bs, slots)
    trans = {kv: bs[kv[0]].transitions(kv[1]) for kv in slots} if check_ref else {}
    for v in empty:
        with pytest.raises(B.FFHipError):
            bs[0].remap(v)
    # the second run: every mapped read's stretch, taken from its record on the host and given as a sequence
    for k, x in enumerate(bs):
        x.set_remap([MR.sequence_of(recs, one[(k, v)][0]) if (k, v) in one else None for v in range(nreads[k])], band)
    _run(bs, fl)
    differ = 0
    for kv in slots:
        k, v = kv
        mp1, rm1, ev1 = one[kv]
        mp2, rm2, ev2 = bs[k].map(v), bs[k].remap(v), bs[k].events(v)
        N = bs[k].read_nblock(v)
        assert bs[k].basecall(v) == calls[kv], (where, kv)
        assert np.array_equal(mp1["raw"], mp2["raw"]), (where, kv)
        assert same_remap(rm1, rm2), (where, kv, rm1, rm2)                    # the feature's definition
        assert same_events(ev1, ev2), (where, kv)
        status, L, _ = MR.remap_from_map(recs, mp1, N, nbase)
        assert (rm1["status"], rm1["L"]) == (status, L), (where, kv, rm1, mp1)
        if mp1["status"] != 1:
            assert (rm1["status"], rm1["L"], np.float32(rm1["score"]).tobytes(), rm1["rm"]) == (0, 0, b"\0\0\0\0", None) and ev1 is None, (where, kv, rm1)
        if rm1["status"] == 1:
            assert ev1 is not None and ev1.size == L and rm1["rm"].size == N and int(rm1["rm"].sum()) == L - 1, (where, kv)
            differ += B.remap_from_map_form(N, band) != remap_form(B, L, band)
            if check_ref:
                score, rm = RR.remap(trans[kv], MT.stretch(recs, mp1["q"], mp1["tstart"], mp1["tend"]), nbase, band)
                assert np.float32(score).tobytes() == np.float32(rm1["score"]).tobytes() and np.array_equal(rm, rm1["rm"]), (where, kv, score, rm1["score"])
    seen = MR.tally([one[kv][0] for kv in slots], [one[kv][1] for kv in slots])
    assert MR.tally_ok(seen), (where, seen)                                   # what keeps the test from passing empty
    assert differ >= forms, (where, differ)                                   # reads whose room takes another kernel form than their L
    for x in bs:
        x.set_remap(None)
        x.set_map(None)
    ref.close()
    return seen


# Read lengths: the room N + 1 of several reads stands just above a form's window while their L stands below it.  The LSTM model (5 samples a block) calls about 0.9
# bases a block: 1285 .. 1330 samples are 257 .. 266 blocks and about 235 bases, on either side of 256.  The GRUmod model (2 samples a block) calls about 0.4:
# 1100 .. 1200 samples are 550 .. 600 blocks and about 240 bases, and 2060 .. 2200 samples 1030 .. 1100 blocks and about 440 bases, on either side of 1024.
STRADDLE = {M.NET_LSTM5: (1285, 1331), M.NET_GRUMOD5: (1100, 1201)}
ROWS = {M.NET_LSTM5: 1300, M.NET_GRUMOD5: 2060}


def _lengths(rng, kind, n, lo=1100, hi=2600):
    a, b = STRADDLE[kind]
    return [int(x) for x in rng.integers(a, b, 4)] + [int(x) for x in rng.integers(lo, hi + 1, n - 4)]


@pytest.mark.parametrize("kind,nbase", [(M.NET_LSTM5, 4), (M.NET_GRUMOD5, 5)])
def test_one_run_is_two_runs_rows_ragged_packed_paired(B, engine, kind, nbase):
    dm = B.DeviceModel(engine, M.synthetic_model(kind, 256, seed=1))
    rng = np.random.default_rng(256 + kind)
    b = B.Batch(dm, 16, ROWS[kind])
    b.set_signals(rng.standard_normal((16, ROWS[kind])).astype(np.float32))
    _one_run_is_two_runs(B, engine, [b], [16], B.RUN_NO_TRACE, ("rows", kind), nbase)
    b.close()
    lens = _lengths(rng, kind, 19)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens[:13] + [0] + lens[13:]]
    b = B.Batch(dm, 20, 2600)
    b.set_signals_ragged(sigs)
    _one_run_is_two_runs(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, ("ragged", kind), nbase, window=128, e=200, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 5400, _lengths(rng, kind, 24), rng)
    _one_run_is_two_runs(B, engine, [pb], [n], B.RUN_NO_TRACE, ("packed", kind), nbase)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, ROWS[kind])
        x.set_signals(rng.standard_normal((16, ROWS[kind])).astype(np.float32))
        pair.append(x)
    _one_run_is_two_runs(B, engine, pair, [16, 16], B.RUN_NO_TRACE, ("pair", kind), nbase)
    for x in pair:
        x.close()
    dm.close()


def test_one_run_is_two_runs_after_an_f32_rerun(B, engine):
    # the outlier case every re-run test of the suite uses (H = 128, these signals): the reads of the outlier's row come from the side batch, which is put into the
    # mode with the same band and maps and remaps them itself
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _one_run_is_two_runs(B, engine, [b], [16], 0, "rerun rows", 4, forms=0)
    assert b.f32_reruns() == 2
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _one_run_is_two_runs(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", 4, band=300, forms=0)
    assert pb.f32_reruns() >= 2
    pb.close()
    dm.close()


SMALL = {}


@pytest.fixture(scope="module")
def small(B, engine):
    """one model, one batch of 16 reads and a reference from its calls, shared by the tests below"""
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=3)
    SMALL["Tb"] = mdl.nblock(2000)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(31)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in _lengths(rng, M.NET_LSTM5, 16, hi=2000)]
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    calls = [b.basecall(v) for v in range(16)]
    recs = MR.reference_of(np.random.default_rng(37), calls)
    ref = B.MapRef(engine, recs)
    b.close()
    yield dm, sigs, calls, recs, ref
    ref.close()
    dm.close()


def _fresh(B, small):
    dm, sigs, calls, recs, ref = small
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    b.set_map(ref)
    return b


def _two_run_route(B, small, band, flags=0):
    """the records of the one run in the mode and of the second run given the stretches, on a fresh batch each"""
    dm, sigs, calls, recs, ref = small
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS | flags
    b = _fresh(B, small)
    b.set_remap_from_map(True, band)
    _run([b], fl)
    one = _read_all([b], [(0, v) for v in range(16)])
    b.close()
    b = _fresh(B, small)
    b.set_remap([MR.sequence_of(recs, one[(0, v)][0]) for v in range(16)], band)
    _run([b], fl)
    two = _read_all([b], [(0, v) for v in range(16)])
    b.close()
    return one, two


@pytest.mark.parametrize("band", [0, 2303])
def test_the_narrowest_and_the_widest_band(B, small, band):
    dm, sigs, calls, recs, ref = small
    one, two = _two_run_route(B, small, band)
    b = _fresh(B, small)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    status = set()
    for v in range(16):
        mp, rm, ev = one[(0, v)]
        assert np.array_equal(mp["raw"], two[(0, v)][0]["raw"]) and same_remap(rm, two[(0, v)][1]) and same_events(ev, two[(0, v)][2]), (band, v)
        status.add((mp["status"] == 1, rm["status"]))
        if rm["status"] == 1:
            score, path = RR.remap(b.transitions(v), MT.stretch(recs, mp["q"], mp["tstart"], mp["tend"]), 4, band)
            assert np.float32(score).tobytes() == np.float32(rm["score"]).tobytes() and np.array_equal(path, rm["rm"]), (band, v)
            assert RR.starts_maxdev(rm["rm"], rm["L"])[1] <= band
    assert (True, 1) in status and (False, 0) in status, status
    for bad in (-1, 2304):                                    # the band is --remap-band's: 0 .. 2303
        with pytest.raises(B.FFHipError):
            b.set_remap_from_map(True, bad)
    b.close()


def test_launch_per_step_and_a_refilled_batch(B, small):
    dm, sigs, calls, recs, ref = small
    band = 2048
    one, two = _two_run_route(B, small, band, B.RUN_STEPWISE_RNN)
    for v in range(16):
        assert np.array_equal(one[(0, v)][0]["raw"], two[(0, v)][0]["raw"]) and same_remap(one[(0, v)][1], two[(0, v)][1]) and same_events(one[(0, v)][2], two[(0, v)][2]), v
    assert MR.tally_ok(MR.tally([one[(0, v)][0] for v in range(16)], [one[(0, v)][1] for v in range(16)]))
    b = _fresh(B, small)                                      # a fresh batch in the mode, to hold the refilled one to
    b.set_remap_from_map(True, band)
    _run([b], B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS)
    plain = _read_all([b], [(0, v) for v in range(16)])
    b.close()
    assert MR.tally_ok(MR.tally([plain[(0, v)][0] for v in range(16)], [plain[(0, v)][1] for v in range(16)]))
    # a refilled batch: other reads first, in the mode, with another band; then these
    rng = np.random.default_rng(5)
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged([rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(1100, 2001, 16)])
    b.set_map(ref)
    b.set_remap_from_map(True, 64)
    _run([b], B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS)
    b.set_signals_ragged(sigs)
    b.set_remap_from_map(True, band)
    _run([b], B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS)
    again = _read_all([b], [(0, v) for v in range(16)])
    for v in range(16):
        assert np.array_equal(again[(0, v)][0]["raw"], plain[(0, v)][0]["raw"]) and same_remap(again[(0, v)][1], plain[(0, v)][1]) and same_events(again[(0, v)][2], plain[(0, v)][2]), v
    b.close()


def same_truth(a, b):
    keys = ("status", "n", "m", "dist", "n_match", "n_mismatch", "n_ins", "n_del", "maxdev")
    return all(a[k] == b[k] for k in keys) and ((a["ops"] is None and b["ops"] is None) or (a["ops"] is not None and b["ops"] is not None and a["ops"].tobytes() == b["ops"].tobytes()))


def test_together_with_truth_from_map_in_one_run(B, small):
    dm, sigs, calls, recs, ref = small
    base = B.RUN_NO_TRACE | B.RUN_MAP
    got = {}
    for name, fl in (("truth", B.RUN_TRUTH), ("remap", B.RUN_REMAP | B.RUN_EVENTS), ("both", B.RUN_TRUTH | B.RUN_REMAP | B.RUN_EVENTS)):
        b = _fresh(B, small)
        b.set_truth_from_map(True, 48)
        b.set_remap_from_map(True, 2048)
        _run([b], base | fl)
        got[name] = [(b.map(v), b.truth(v) if fl & B.RUN_TRUTH else None, b.remap(v) if fl & B.RUN_REMAP else None, b.events(v) if fl & B.RUN_REMAP else None) for v in range(16)]
        b.close()
    n = 0
    for v in range(16):
        mp, tr, rm, ev = got["both"][v]
        assert np.array_equal(mp["raw"], got["truth"][v][0]["raw"]) and np.array_equal(mp["raw"], got["remap"][v][0]["raw"])
        assert same_truth(tr, got["truth"][v][1]), v
        assert same_remap(rm, got["remap"][v][2]) and same_events(ev, got["remap"][v][3]), v
        n += tr["status"] == 1 and rm["status"] == 1 and tr["m"] == rm["L"]
    assert n >= 12


def test_the_mode_and_host_sequences_replace_each_other(B, small):
    dm, sigs, calls, recs, ref = small
    band, fl = 100, B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS
    seqs = [MT.codes(c.replace("Z", "C")[::-1][:len(c) // 2]) if v % 3 else None for v, c in enumerate(calls)]      # (nothing to do with the reference)
    b = _fresh(B, small)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    trans = [b.transitions(v) for v in range(16)]

    def run_and_read():
        _run([b], fl)
        return [(b.map(v), b.remap(v), b.events(v)) for v in range(16)]

    def as_host(got):
        for v in range(16):
            mp, rm, ev = got[v]
            if seqs[v] is None:
                assert (rm["status"], rm["L"], rm["rm"]) == (0, 0, None) and ev is None
            else:
                score, path = RR.remap(trans[v], seqs[v], 4, band)
                assert (rm["status"], rm["L"]) == (1, seqs[v].size) and np.float32(score).tobytes() == np.float32(rm["score"]).tobytes() and np.array_equal(path, rm["rm"]), v
                assert ev.size == seqs[v].size

    def as_mode(got):
        for v in range(16):
            mp, rm, ev = got[v]
            status, L, _ = MR.remap_from_map(recs, mp, b.read_nblock(v), 4)
            assert (rm["status"], rm["L"]) == (status, L), v
            if status == 1:
                score, path = RR.remap(trans[v], MT.stretch(recs, mp["q"], mp["tstart"], mp["tend"]), 4, band)
                assert np.float32(score).tobytes() == np.float32(rm["score"]).tobytes() and np.array_equal(path, rm["rm"]) and ev.size == L, v

    b.set_remap_from_map(True, band)
    b.set_remap(seqs, band)                                   # the later call wins: a run as without the mode
    as_host(run_and_read())
    b.set_remap_from_map(True, band)                          # ... in the other order
    as_mode(run_and_read())
    with pytest.raises(B.FFHipError) as ei:                   # REMAP without MAP in the mode
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP)
    assert "FFHIP_RUN_MAP" in str(ei.value), str(ei.value)
    with pytest.raises(B.FFHipError) as ei:                   # variants: their lists are the host's
        b.run(1.0, fl | B.RUN_REMAP_VARIANTS)
    assert "variants" in str(ei.value) and "does not have" in str(ei.value), str(ei.value)
    b.set_map(None)
    with pytest.raises(B.FFHipError) as ei:                   # no reference attached
        b.run(1.0, fl)
    assert "no reference" in str(ei.value), str(ei.value)
    b.set_map(ref)
    b.set_remap_from_map(False)                               # the mode left, and no sequences: as a batch that never had any
    with pytest.raises(B.FFHipError) as ei:
        b.run(1.0, fl)
    assert "no sequences are set" in str(ei.value), str(ei.value)
    b.set_remap(seqs, band)
    as_host(run_and_read())
    b.run(1.0, fl)
    with pytest.raises(B.FFHipError):                         # not between a run and its finish
        b.set_remap_from_map(True, band)
    b.finish()
    b.close()


def test_site_mods_and_the_run_length_model_are_refused(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 128, seed=1))
    rng = np.random.default_rng(2)
    x = B.Batch(dm, 4, 1200)
    x.set_signals(rng.standard_normal((4, 1200)).astype(np.float32))
    ref = B.MapRef(engine, [MR.rand_seq(rng, 500)])
    x.set_map(ref)
    x.set_remap_from_map(True, 100)
    with pytest.raises(B.FFHipError) as ei:                   # site mods: their lists are the host's
        x.run(1.0, B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_REMAP_MODS)
    assert "site mods" in str(ei.value) and "does not have" in str(ei.value), str(ei.value)
    x.close()
    ref.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    x = B.Batch(dm, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_remap_from_map(True, 24)
    assert "flip-flop model only" in str(ei.value)
    x.set_remap_from_map(False)
    x.close()
    dm.close()


def test_the_buffers_are_sized_by_the_blocks_and_counted(B, small):
    dm, sigs, calls, recs, ref = small
    band, fl = 2048, B.RUN_NO_TRACE | B.RUN_MAP
    cap = 16
    # a batch that never had the mode: a MAP | REMAP | EVENTS run with host sequences holds what the sequences' lengths say, to the byte
    plain = _fresh(B, small)
    _run([plain], fl)
    seqs = [MT.codes(c.replace("Z", "C")) if v % 4 else None for v, c in enumerate(calls)]
    held = plain.device_bytes()
    plain.set_remap(seqs, band)
    _run([plain], fl | B.RUN_REMAP | B.RUN_EVENTS)
    Tb = SMALL["Tb"]                                          # the batch's capacity in blocks
    fixed = cap * 16 + 16 * (Tb + 1) + cap * 24 + cap * 32   # remap's records and moves, its list, the events' list
    exact = sum(2 * s.size + 16 * s.size + 8 * WS_WORDS_A_BLOCK[remap_form(B, s.size, band)] * plain.read_nblock(v) for v, s in enumerate(seqs) if s is not None) + fixed
    assert plain.device_bytes() - held == exact, (plain.device_bytes() - held, exact)
    # the mode: the same batch shape, sized from the blocks
    b = _fresh(B, small)
    _run([b], fl)
    held = b.device_bytes()
    assert held == plain.device_bytes() - exact               # (the same object up to here)
    b.set_remap_from_map(True, band)
    assert b.device_bytes() == held                           # (nothing is taken at the call)
    _run([b], fl | B.RUN_REMAP | B.RUN_EVENTS)
    Ns = [b.read_nblock(v) for v in range(16)]
    assert all(B.remap_from_map_form(N, band) == remap_form(B, N + 1, band) for N in Ns)
    want = sum(2 * (N + 1) + 16 * (N + 1) + 8 * WS_WORDS_A_BLOCK[B.remap_from_map_form(N, band)] * N for N in Ns) + fixed
    grew = b.device_bytes() - held
    assert grew == want, (grew, want)
    # the price the header states: sequences and events have room for N + 1 positions, whatever the mapped reads' own L
    own = sum(b.remap(v)["L"] for v in range(16))
    print("sequences and events: room for %d positions, %d used (%.2f times)" % (sum(N + 1 for N in Ns), own, sum(N + 1 for N in Ns) / max(own, 1)))
    assert b.remap(0)["status"] == 1 and 0 < own < sum(N + 1 for N in Ns)
    _run([b], fl | B.RUN_REMAP | B.RUN_EVENTS)
    assert b.device_bytes() - held == grew                    # no growth on a second run
    b.close()
    plain.close()


def _copy_counts(B, reset=1):
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, reset)
    return [int(v) for v in c]


def test_no_more_copy_calls_than_the_second_run_of_two(B, small):
    dm, sigs, calls, recs, ref = small
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_REMAP | B.RUN_EVENTS
    counts = {}
    for mode in ("host", "map"):
        b = _fresh(B, small)
        if mode == "host":
            b.set_remap([MT.codes(c.replace("Z", "C")) for c in calls], 2048)
        else:
            b.set_remap_from_map(True, 2048)
        for it in range(2):                                   # (the first run creates the buffers; the counts are the second's)
            _copy_counts(B)
            _run([b], fl)
            counts[mode] = _copy_counts(B)
        b.close()
    assert counts["map"][2] <= counts["host"][2], counts         # device-to-host calls: the block, the map records, remap's records and moves, the events
    assert counts["map"][0] <= counts["host"][0], counts         # host-to-device calls: the coded stretches never leave the device


# ------------------------------------------------------------------------------------ the binary
def test_flappie_remap_from_map(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, RUNNIE, TOOL, synth_raw, write_fast5
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

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    lines = default.split("\n")[:-1]
    fq = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    assert len(fq) == nread
    order = [r[0][1:].split("  {")[0] for r in fq]
    calls = {nm: r[1] for nm, r in zip(order, fq)}
    krng = np.random.default_rng(5)
    records = ["", "", ""]
    for i, nm in enumerate(order[:-2]):                       # two reads have no place
        x = R.edit(krng, calls[nm].replace("Z", "C"), 0.05)
        records[i % 3] += MR.rand_seq(krng, 200 + 31 * i) + (x if i % 2 == 0 else R.revcomp(x))
    records = [r + MR.rand_seq(krng, 150) for r in records]
    names = ["chrA", "plasmid.1", "third"]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join(r[k:k + 70] for k in range(0, len(r), 70))) for nm, r in zip(names, records)))
    hits0, recs0 = tmp_path / "hits0.tsv", tmp_path / "recs0.fa"
    base, _ = run(["--map", str(fa), "--map-out", str(hits0), "--map-records", str(recs0)])
    assert base == default
    for opts, band in ((["--remap-band", "40"], 40),):
        hits, mp, ev = tmp_path / "hits.tsv", tmp_path / "map.tsv", tmp_path / "events.tsv"
        got, err = run(["--map", str(fa), "--map-out", str(hits), "--remap-from-map", "--remap-out", str(mp), "--remap-events", str(ev)] + opts)
        assert got == default and hits.read_text() == hits0.read_text()
        # the two-run route: --remap on the file of --map-records
        mp2, ev2 = tmp_path / "map2.tsv", tmp_path / "events2.tsv"
        got2, err2 = run(["--remap", str(recs0), "--remap-out", str(mp2), "--remap-events", str(ev2)] + opts)
        assert got2 == default
        rows, rows2 = [ln.split("\t") for ln in mp.read_text().splitlines()], [ln.split("\t") for ln in mp2.read_text().splitlines()]
        hit = {f[0]: f for f in (ln.split("\t") for ln in hits.read_text().splitlines())}
        assert len(rows) == len(rows2) == sum(f[1] == "1" for f in hit.values()) >= nread - 4
        for f, f2 in zip(rows, rows2):
            assert len(f) == 14 and len(f2) == 10 and f[:10] == f2 and f[1] == "1" and int(f[6]) == band, (f[:9], f2[:9])      # (recs.fa names a record by the read's name in hits.tsv)
            assert f[10:] == hit[f[0]][4:8], (f[10:], hit[f[0]])
            assert int(f[5]) == int(f[13]) - int(f[12]) == len(f[9].split(","))
        assert {hit[f[0]][5] for f in rows} == {"+", "-"}
        assert ev.read_text() == ev2.read_text() and len(ev.read_text().splitlines()) == sum(int(f[5]) for f in rows) > 1000
        want = {k: v for k, v in (ln.split("\t")[1:] for ln in err2.splitlines() if ln.startswith("remap\t") or ln.startswith("events\t"))}
        mine = {k: v for k, v in (ln.split("\t")[1:] for ln in err.splitlines() if ln.startswith("remap\t") or ln.startswith("events\t"))}
        assert mine == want and mine["no_record"] == str(nread - len(rows)) and mine["mapped"] == str(len(rows)), (mine, want)
    # with --truth-from-map in the same run: acc.tsv is what it is without --remap-from-map, map.tsv what it is without --truth-from-map
    acc, acc0, mp3 = tmp_path / "acc.tsv", tmp_path / "acc0.tsv", tmp_path / "map3.tsv"
    run(["--map", str(fa), "--map-out", str(hits0), "--truth-from-map", "--truth-out", str(acc0)])
    got, _ = run(["--map", str(fa), "--map-out", str(hits), "--truth-from-map", "--truth-out", str(acc), "--remap-from-map", "--remap-out", str(mp3), "--remap-band", "40"])      # (the band of map.tsv above)
    assert got == default and acc.read_text() == acc0.read_text() and mp3.read_text() == (tmp_path / "map.tsv").read_text()
    r = subprocess.run([RUNNIE, "--remap-from-map", str(reads)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "--remap-from-map is flappie's" in r.stderr, r.stderr
