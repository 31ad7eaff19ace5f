"""flappie --truth-from-map on the GPU: each call aligned to the stretch of the reference it was mapped to, in the run that mapped it (include/ffhip.h "truth from
map": ffhip_batch_set_truth_from_map, ffhip_op_map_stretch, ffhip_debug_map_truth_bound; the kernel k_map_stretch).

  * the gather kernel on one span equals numpy for every start 0 .. 33 and length 1 .. 40 on both strands of records of 1, 15, 16, 17, 33 and 100 bases; its refusals;
  * batches: the one-run result IS the two-run result -- truth record and ops of a MAP | TRUTH run in the mode equal, byte for byte, those of a second run given each
    mapped read's stretch through ffhip_batch_set_truth -- one read a row, ragged with an empty slot, packed, paired, after an f32 re-run; and both equal
    maptruth_ref.py on the batch's own calls;
  * the narrowest and the widest band against truth_ref;
  * the buffers are sized by ffhip_debug_map_truth_bound and counted, and a batch that never had the mode holds what the lengths of its truths say;
  * the mode and ffhip_batch_set_truth replace each other; TRUTH without MAP is refused in the mode;
  * a finished run in the mode makes no more copy calls than a MAP | TRUTH run with host truths;
  * the `flappie` binary: stdout and hits.tsv unchanged, acc.tsv the second run's, aln.sam replays over the reference; runnie refuses.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import map_ref as R
import maptruth_ref as MT
import truth_ref as T
from test_barcodes_gpu import _d2h_calls, _packed_batch, _records, rand_seq

pytestmark = pytest.mark.gpu

WS_WORDS_A_ROW = {0: 2, 1: 8, 2: 40, 3: 80}              # 64-bit words of decisions a row of the truth, by kernel form (include/ffhip.h "truth": two bits a cell)


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------ the operator
def test_stretch_of_every_span_at_the_word_edges(B, engine):
    rng = np.random.default_rng(21)
    recs = [rand_seq(rng, m) for m in (1, 15, 16, 17, 33, 100)]
    ref = B.MapRef(engine, recs)
    ys = R.searches(recs)
    n = 0
    for q, y in enumerate(ys):
        want_all = MT.codes(y)
        for start in range(0, 34):
            for length in range(1, 41):
                if start + length > len(y):
                    break
                got = B.op_map_stretch(engine, ref, q, start, start + length)
                assert got.dtype == np.uint8 and np.array_equal(got, want_all[start:start + length]), (q, start, length, got, want_all[start:start + length])
                n += 1
    assert n == sum(min(40, len(y) - start) for y in ys for start in range(34) if start < len(y)) > 4000
    assert np.array_equal(B.op_map_stretch(engine, ref, 11, 0, 100), MT.stretch(recs, 11, 0, 100))      # a whole record, its other strand
    for q, a, b in ((-1, 0, 1), (12, 0, 1), (0, -1, 1), (0, 0, 2), (0, 1, 1), (2, 3, 3), (2, 5, 4), (10, 0, 101), (10, 100, 101), (3, 14, 16)):
        with pytest.raises(B.FFHipError):
            B.op_map_stretch(engine, ref, q, a, b)
    ref.close()


# ------------------------------------------------------------------------------------ batches
def reference_of(rng, calls):
    """random flanks and the reads' own calls in three records: five in six of them, two in three of those with 5 % edits, on alternating strands"""
    recs = ["", "", ""]
    for i, c in enumerate(calls):
        if not c or i % 6 == 5:
            continue                                          # left out: this read does not map
        x = c.replace("Z", "C")
        if i % 3:
            x = R.edit(rng, x, 0.05)
        recs[i % 3] += rand_seq(rng, 150 + 37 * (i % 5)) + (x if i % 2 == 0 else R.revcomp(x))
    return [r + rand_seq(rng, 200) for r in recs]


def same_truth(a, b):
    return all(a[k] == b[k] for k in T.FIELDS) and ((a["ops"] is None and b["ops"] is None) or (a["ops"] is not None and b["ops"] is not None and
                                                                                                   a["ops"].tobytes() == b["ops"].tobytes()))


def _one_run_is_two_runs(B, engine, bs, nreads, flags, where, band=48, window=-1, e=-1, empty=(), check_ref=True):
    def run(fl):
        if len(bs) == 1:
            bs[0].run(1.0, fl)
        else:
            bs[0].run_pair(bs[1], 1.0, fl)
        for x in bs:
            x.finish()
    slots = [(k, v) for k, x in enumerate(bs) for v in range(nreads[k]) if not (k == 0 and v in empty)]
    run(flags)
    calls = {kv: bs[kv[0]].basecall(kv[1]) for kv in slots}
    rng = np.random.default_rng(23)
    recs = reference_of(rng, [calls[kv] for kv in slots])
    ref = B.MapRef(engine, recs)
    W, E = (4096 if window < 0 else window), (250 if e < 0 else e)
    for x in bs:
        x.set_map(ref, window, e)
        x.set_truth_from_map(True, band)
    run(flags | B.RUN_MAP | B.RUN_TRUTH)
    one = {kv: (bs[kv[0]].map(kv[1]), bs[kv[0]].truth(kv[1])) for kv in slots}
    for v in empty:
        with pytest.raises(B.FFHipError):
            bs[0].truth(v)
    # the second run: every mapped read's stretch, taken from its record on the host and given as a truth
    for k, x in enumerate(bs):
        given = []
        for v in range(nreads[k]):
            mp = one[(k, v)][0] if (k, v) in one else None
            given.append(MT.stretch(recs, mp["q"], mp["tstart"], mp["tend"]) if mp is not None and mp["status"] == 1 else None)
        x.set_truth(given, band)
    run(flags | B.RUN_MAP | B.RUN_TRUTH)
    seen = {"reads": 0, "aligned": 0, "plus": 0, "minus": 0, "not mapped": 0, "edits": 0}
    for kv in slots:
        k, v = kv
        mp1, tr1 = one[kv]
        mp2, tr2 = bs[k].map(v), bs[k].truth(v)
        assert bs[k].basecall(v) == calls[kv], (where, kv)
        assert np.array_equal(mp1["raw"], mp2["raw"]), (where, kv)
        assert same_truth(tr1, tr2), (where, kv, tr1, tr2)                   # the feature's definition
        if mp1["status"] != 1:
            assert (tr1["status"], tr1["n"], tr1["m"], tr1["ops"]) == (0, len(calls[kv]), 0, None), (where, kv, tr1)
        if check_ref:
            want_mp = R.record(recs, calls[kv], W, E)
            assert np.array_equal(mp1["raw"], R.raw(want_mp)), (where, kv)
            _, want = MT.truth_from_map(recs, calls[kv], band, W, E, nblock=bs[k].read_nblock(v), map_rec=want_mp)
            got = dict(tr1, ops=np.zeros(0, np.uint8) if tr1["ops"] is None else tr1["ops"])
            assert same_truth(got, want), (where, kv, tr1, want)
        seen["reads"] += 1
        ok = mp1["status"] == 1 and tr1["status"] == 1
        seen["aligned"] += ok
        seen["plus"] += ok and not mp1["q"] & 1
        seen["minus"] += ok and mp1["q"] & 1
        seen["not mapped"] += mp1["status"] != 1
        seen["edits"] += ok and tr1["dist"] > 0
    # what keeps the test from passing empty
    assert seen["aligned"] * 4 >= seen["reads"] * 3 and seen["plus"] >= 2 and seen["minus"] >= 2 and seen["not mapped"] >= 1 and seen["edits"] >= 1, (where, seen)
    for x in bs:
        x.set_truth(None)
        x.set_map(None)
    ref.close()
    return seen


@pytest.mark.parametrize("kind", [M.NET_LSTM5, M.NET_GRUMOD5])
def test_one_run_is_two_runs_rows_ragged_packed_paired(B, engine, kind):
    dm = B.DeviceModel(engine, M.synthetic_model(kind, 256, seed=1))
    rng = np.random.default_rng(256 + kind)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
    _one_run_is_two_runs(B, engine, [b], [16], B.RUN_NO_TRACE, ("rows", kind))
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(1500, 2501, 13)) + [0, 2600, 1800] + list(rng.integers(1500, 2501, 4))]
    b = B.Batch(dm, 20, 2600)
    b.set_signals_ragged(sigs)
    _one_run_is_two_runs(B, engine, [b], [20], B.RUN_NO_TRACE | B.RUN_MOVES, ("ragged", kind), band=100, window=128, e=200, empty=(13,))
    b.close()
    pb, n = _packed_batch(B, dm, 16, 5000, 24, rng, lo=1500, hi=2500)
    _one_run_is_two_runs(B, engine, [pb], [n], B.RUN_NO_TRACE, ("packed", kind), band=64)
    pb.close()
    pair = []
    for k in range(2):
        x = B.Batch(dm, 16, 2000)
        x.set_signals(rng.standard_normal((16, 2000)).astype(np.float32))
        pair.append(x)
    _one_run_is_two_runs(B, engine, pair, [16, 16], B.RUN_NO_TRACE, ("pair", kind), band=32)
    for x in pair:
        x.close()
    dm.close()


def test_one_run_is_two_runs_after_an_f32_rerun(B, engine):
    # the outlier case every re-run test of the suite uses (H = 128, these signals): the reads of the outlier's row come from the side batch, which is put into the
    # mode and maps and aligns them itself
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _one_run_is_two_runs(B, engine, [b], [16], 0, "rerun rows")
    assert b.f32_reruns() == 2
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _one_run_is_two_runs(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", band=300)
    assert pb.f32_reruns() >= 2
    pb.close()
    dm.close()


@pytest.fixture(scope="module")
def small(B, engine):
    """one model, one batch of 16 reads and a reference from its calls, shared by the tests below"""
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


@pytest.mark.parametrize("band", [0, 1279])
def test_the_narrowest_and_the_widest_band(B, small, band):
    dm, sig, calls, recs, ref = small
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref)
    b.set_truth_from_map(True, band)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH)
    b.finish()
    status = set()
    for v in range(16):
        assert b.basecall(v) == calls[v]
        mp, want = MT.truth_from_map(recs, calls[v], band, nblock=b.read_nblock(v))
        got = b.truth(v)
        assert np.array_equal(b.map(v)["raw"], R.raw(mp))
        assert (got["status"], got["maxdev"]) == (want["status"], want["maxdev"]), (band, v, got, want)
        assert same_truth(dict(got, ops=np.zeros(0, np.uint8) if got["ops"] is None else got["ops"]), want), (band, v)
        status.add((mp["status"] == 1, want["status"]))
    assert (True, 1) in status and (False, 0) in status, status
    for bad in (-1, 1280):                                    # the band is truth's: 0 .. 1279
        with pytest.raises(B.FFHipError):
            b.set_truth_from_map(True, bad)
    b.close()


def _predicted(B, b, nread, band, max_error):
    """what a run in the mode adds: bound bases of truth, the workspace of bound rows and bound + N + 1 bytes of ops a read; 48 bytes of record and 40 of list a read"""
    ws = ops = seq = 0
    for v in range(nread):
        N = b.read_nblock(v)
        if N <= 0:
            continue
        bound = B.map_truth_bound(N, max_error)
        assert bound == MT.bound(N, max_error)
        ws += 8 * WS_WORDS_A_ROW[B.truth_form(min(2 * band + 1, N + 2))] * bound
        ops += bound + N + 1
        seq += bound
    return ws, ops, seq, nread * (48 + 40)


def test_the_buffers_are_sized_by_the_bound_and_counted(B, small):
    dm, sig, calls, recs, ref = small
    band, fl = 24, B.RUN_NO_TRACE | B.RUN_MAP
    # a batch that never had the mode: a MAP | TRUTH run with host truths holds what the truths' lengths say, to the byte
    plain = B.Batch(dm, 16, 2000)
    plain.set_signals(sig)
    plain.set_map(ref)
    plain.run(1.0, fl)
    plain.finish()
    truths = [MT.codes(R.edit(np.random.default_rng(v), c.replace("Z", "C"), 0.05)) if v % 4 else None for v, c in enumerate(calls)]
    held = plain.device_bytes()
    plain.set_truth(truths, band)
    plain.run(1.0, fl | B.RUN_TRUTH)
    plain.finish()
    form_words = [WS_WORDS_A_ROW[B.truth_form(min(2 * band + 1, plain.read_nblock(v) + 2))] for v in range(16)]
    exact = sum(t.size for t in truths if t is not None) + sum(8 * w * t.size for w, t in zip(form_words, truths) if t is not None) + \
        sum(t.size + plain.read_nblock(v) + 1 for v, t in enumerate(truths) if t is not None) + 16 * (48 + 40)
    assert plain.device_bytes() - held == exact, (plain.device_bytes() - held, exact)
    # the mode: the same batch shape, sized from the bound
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref, -1, 250)
    b.run(1.0, fl)
    b.finish()
    held = b.device_bytes()
    assert held == plain.device_bytes() - exact               # (the same object up to here)
    b.set_truth_from_map(True, band)
    b.run(1.0, fl | B.RUN_TRUTH)
    b.finish()
    ws, ops, seq, fixed = _predicted(B, b, 16, band, 250)
    grew = b.device_bytes() - held
    granule = 4096
    assert ws + ops + seq + fixed - granule < grew <= ws + ops + seq + fixed, (grew, ws, ops, seq, fixed)
    # the price the header states: the workspace is that of bound rows, whatever the mapped reads' own m
    own = sum(8 * form_words[v] * b.truth(v)["m"] for v in range(16))
    print("workspace: %d bytes by the bound, %d by the reads' own m (%.2f times)" % (ws, own, ws / max(own, 1)))
    assert b.truth(0)["status"] == 1 and 0 < own < ws, (ws, own)
    b.run(1.0, fl | B.RUN_TRUTH)
    b.finish()
    assert b.device_bytes() - held == grew                    # no growth on a second run
    b.close()
    plain.close()


def test_the_mode_and_host_truths_replace_each_other(B, small):
    dm, sig, calls, recs, ref = small
    band, fl = 40, B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH
    truths = [MT.codes(c.replace("Z", "C")[::-1]) if v % 3 else None for v, c in enumerate(calls)]      # (nothing to do with the reference)
    b = B.Batch(dm, 16, 2000)
    b.set_signals(sig)
    b.set_map(ref)

    def run_and_read():
        b.run(1.0, fl)
        b.finish()
        return [b.truth(v) for v in range(16)]

    def as_host(got):
        for v in range(16):
            if truths[v] is None:
                assert (got[v]["status"], got[v]["m"], got[v]["ops"]) == (0, 0, None)
            else:
                want = T.truth(calls[v], truths[v], band)
                assert same_truth(dict(got[v], ops=np.zeros(0, np.uint8) if got[v]["ops"] is None else got[v]["ops"]), want), v

    def as_mode(got):
        for v in range(16):
            _, want = MT.truth_from_map(recs, calls[v], band, nblock=b.read_nblock(v))
            assert same_truth(dict(got[v], ops=np.zeros(0, np.uint8) if got[v]["ops"] is None else got[v]["ops"]), want), v

    b.set_truth_from_map(True, band)
    b.set_truth(truths, band)                                 # the later call wins: a run as without the mode
    as_host(run_and_read())
    b.set_truth_from_map(True, band)                          # ... in the other order
    as_mode(run_and_read())
    with pytest.raises(B.FFHipError) as ei:                   # TRUTH without MAP in the mode
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_TRUTH)
    assert "FFHIP_RUN_MAP" in str(ei.value), str(ei.value)
    b.set_map(None)
    with pytest.raises(B.FFHipError) as ei:                   # no reference attached
        b.run(1.0, fl)
    assert "no reference" in str(ei.value), str(ei.value)
    b.set_map(ref)
    b.set_truth_from_map(False)                               # the mode left, and no truths: as a batch that never had any
    with pytest.raises(B.FFHipError) as ei:
        b.run(1.0, fl)
    assert "no truths are set" in str(ei.value), str(ei.value)
    b.set_truth(truths, band)
    as_host(run_and_read())
    b.run(1.0, fl)
    with pytest.raises(B.FFHipError):                         # not between a run and its finish
        b.set_truth_from_map(True, band)
    b.finish()
    b.close()


def test_the_run_length_model_is_refused(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    x = B.Batch(dm, 4, 1000)
    with pytest.raises(B.FFHipError) as ei:
        x.set_truth_from_map(True, 24)
    assert "flip-flop model only" in str(ei.value)
    x.set_truth_from_map(False)
    x.close()
    dm.close()


def test_no_more_copy_calls_than_with_host_truths(B, small):
    dm, sig, calls, recs, ref = small
    fl = B.RUN_NO_TRACE | B.RUN_MAP | B.RUN_TRUTH
    counts = {}
    for mode in ("host", "map"):
        b = B.Batch(dm, 16, 2000)
        b.set_signals(sig)
        b.set_map(ref)
        if mode == "host":
            b.set_truth([MT.codes(c.replace("Z", "C")) for c in calls], 24)
        else:
            b.set_truth_from_map(True, 24)
        for it in range(2):                                   # (the first run creates the buffers; the counts are the second's)
            _d2h_calls(B)
            b.run(1.0, fl)
            b.finish()
            counts[mode] = _copy_counts(B)
        b.close()
    assert counts["map"][2] <= counts["host"][2], counts         # device-to-host calls: the block, the map records, the truth records and ops
    assert counts["map"][0] <= counts["host"][0], counts         # host-to-device calls: the stretches never leave the device


def _copy_counts(B):
    import ctypes as C
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, 1)
    return [int(v) for v in c]


# ------------------------------------------------------------------------------------ the binary
def test_flappie_truth_from_map(tmp_path):
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
    fq = _records(default, "fastq")
    assert len(fq) == nread
    calls = {r[0]: r[1] for r in fq}
    quals = {r[0]: r[2] for r in fq}
    assert all(len(calls[nm]) == len(quals[nm]) > 0 for nm in calls)
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
    hits0, recs0 = tmp_path / "hits0.tsv", tmp_path / "recs0.fa"
    base, _ = run(["--map", str(fa), "--map-out", str(hits0), "--map-records", str(recs0)])
    for opts, band in (([], 512), (["--truth-band", "30", "--reverse"], 30)):
        hits, recs, acc, sam = tmp_path / "hits.tsv", tmp_path / "recs.fa", tmp_path / "acc.tsv", tmp_path / "aln.sam"
        rev = "--reverse" in opts
        got, err = run(["--map", str(fa), "--map-out", str(hits), "--map-records", str(recs), "--truth-from-map", "--truth-out", str(acc), "--map-sam", str(sam)] + opts)
        assert got == (run(["--reverse"])[0] if rev else base)  # stdout, hits.tsv and recs.fa are what they are without the two options
        assert hits.read_text() == hits0.read_text() and recs.read_text() == recs0.read_text()
        # the two-run route: --truth on the file of --map-records
        acc2 = tmp_path / "acc2.tsv"
        _, err2 = run(["--truth", str(recs0), "--truth-out", str(acc2), "--truth-band", str(band)])
        rows, rows2 = [ln.split("\t") for ln in acc.read_text().splitlines()], [ln.split("\t") for ln in acc2.read_text().splitlines()]
        hit = {f[0]: f for f in (ln.split("\t") for ln in hits.read_text().splitlines())}
        assert len(rows) == len(rows2) == sum(f[1] == "1" for f in hit.values()) >= nread - 2
        for f, f2 in zip(rows, rows2):
            assert len(f) == 17 and len(f2) == 13 and f[1:13] == f2[1:] and f[0] == f2[0], (f, f2)      # (recs.fa names a record by the read's name in hits.tsv)
            assert f[13:] == hit[f[0]][4:8], (f, hit[f[0]])
        want = {k: v for k, v in (ln.split("\t")[1:] for ln in err2.splitlines() if ln.startswith("truth\t"))}
        mine = {k: v for k, v in (ln.split("\t")[1:] for ln in err.splitlines() if ln.startswith("truth\t"))}
        assert mine["no_record"] == str(nread - len(rows)) and {k: v for k, v in mine.items() if k != "no_record"} == {k: v for k, v in want.items() if k != "no_record"}, (mine, want)
        # aln.sam: the header, a line a read in output order, every aligned line replayed over the reference
        text = sam.read_text()
        head = MT.sam_header(names, lens)
        assert text.startswith(head)
        lines = text[len(head):].splitlines(True)
        assert [ln.split("\t")[0] for ln in lines] == order
        aligned = {f[0]: f for f in rows if f[1] == "1"}
        nal = 0
        for ln in lines:
            f = ln.rstrip("\n").split("\t")
            nm = f[0]
            if nm in aligned:
                got = MT.replay(ln, dict(zip(names, records)))
                h = hit[nm]
                assert f[2] == h[4] and (got["start"], got["end"]) == (int(h[6]), int(h[7])) and got["flag"] == (16 if h[5] == "-" else 0), (ln, h)
                assert got["nm"] == int(aligned[nm][6])
                seq = calls[nm].replace("Z", "C")
                assert f[9] == (R.revcomp(seq) if h[5] == "-" else seq) and f[10] == (quals[nm][::-1] if h[5] == "-" else quals[nm]), nm      # the whole call, whatever --reverse does
                nal += 1
            else:
                assert f[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and f[9] == calls[nm].replace("Z", "C") and f[10] == quals[nm] and len(f) == 11, ln
        assert nal == len(aligned) >= nread - 4 and {hit[nm][5] for nm in aligned} == {"+", "-"}
    for args in (["--truth-from-map"], ["--map-sam", str(tmp_path / "x.sam")]):
        r = subprocess.run([RUNNIE] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "" and "--truth-from-map and --map-sam are flappie's" in r.stderr, r.stderr
