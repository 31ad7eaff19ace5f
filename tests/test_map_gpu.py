"""flappie --map on the GPU: every call placed on a small reference by k_map_scan and k_map_finish (include/ffhip.h FFHIP_RUN_MAP, ffhip_batch_map,
ffhip_op_map_scores, ffhip_op_map).

  * the operator's whole score rows equal the restatement (map_ref.py) for anchors of every lane-group size, both sides of every word and group edge, against a
    reference whose records are 1, 2, S - 1, S, S + 1 and 3 S + 77 long (S = FFHIP_MAP_SEGMENT), Z in the call;
  * the operator's records equal the restatement when an anchor's copy ends on every column around the seams of the segments, spans them, and where strand,
    record and column tie;
  * one anchor and two, the pairing rule one base either side of its bound, every status, e = 0;
  * what the upload, the batch and the operators refuse;
  * on synthetic 8-state (H = 256, 384) and 10-state models every record equals the restatement on the batch's own calls -- one read a row, ragged, packed, paired,
    launch per step, f32 re-run, with barcodes, adapters and truth -- and everything else the batch returns is bit for bit that of the same run without the flag;
  * a finished run with the flag makes exactly one more device-to-host copy call than the same run without;
  * the `flappie` binary's hits.tsv, recs.fa and counts equal the restatement applied to its default output, and --truth on recs.fa closes the loop.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import map_ref as R
from test_barcodes_gpu import _d2h_calls, _packed_batch, _records, _state, mutate, rand_seq

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


def same(got, want):
    return np.array_equal(got["raw"], R.raw(want))


# ------------------------------------------------------------------------------------ the operators
@pytest.fixture(scope="module")
def edge_reference(B, engine):
    S = B.MAP_SEGMENT
    assert S == B.lib().ffhip_map_segment() and S % 64 == 0
    rng = np.random.default_rng(11)
    recs = [rand_seq(rng, m) for m in (1, 2, S - 1, S, S + 1, 3 * S + 77)]
    ref = B.MapRef(engine, recs)
    yield recs, ref
    ref.close()


LENGTHS = (1, 63, 64, 65, 127, 128, 129, 192, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096)


@pytest.mark.parametrize("L", LENGTHS)
def test_score_rows_at_every_edge(B, engine, edge_reference, L):
    recs, ref = edge_reference
    S = B.MAP_SEGMENT
    ys = R.searches(recs)
    rng = np.random.default_rng(L)
    anchors = [rand_seq(rng, L, "ACGTZ")]
    for q, rate in ((10, 0.0), (11, 0.15), (6 + L % 2, 0.05)):          # cut from the reference, either strand, around a seam where the record has one
        y = ys[q]
        at = max(0, min(len(y) - L, S - L // 2 + int(rng.integers(-40, 40))))
        p = (R.edit(rng, y[at:at + L], rate) + rand_seq(rng, L))[:L]
        anchors.append(p.replace("C", "Z", 3))
    for p in anchors[:2 if L > 2049 else 4]:
        got, want = B.op_map_scores(engine, ref, p), R.score_rows(recs, p)
        assert len(got) == 2 * len(recs)
        for q, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(g, w), (L, q, np.flatnonzero(g != w)[:4])
        g, w = B.op_map(engine, ref, p), R.record(recs, p, rows=want)
        assert same(g, w), (L, g, w)


def test_records_at_the_seams(B, engine, edge_reference):
    recs, ref = edge_reference
    S = B.MAP_SEGMENT
    ys = R.searches(recs)
    rng = np.random.default_rng(3)
    spans, strands, n = set(), set(), 0
    for L, nedit in ((20, 0), (24, 1), (90, 4)):
        for seam in (S, 2 * S):
            for e in range(seam - 2 * L - 3, seam + 4):
                q = 10 + (e & 1)
                p = mutate(rng, ys[q][e - L:e], nedit)
                g, w = B.op_map(engine, ref, p), R.record(recs, p)
                assert same(g, w), (L, seam, e, g, w)
                a = w["anchors"][0]
                assert w["status"] == 1 and a["q"] == q and e - L < a["end"] <= e + nedit, (L, seam, e, w)      # (the copy is found: its edits may sit at its end)
                spans.add(a["start"] < seam < a["end"])
                strands.add(q & 1)
                n += 1
    assert spans == {False, True} and strands == {0, 1} and n > 500


def test_ties_of_record_strand_and_column(B, engine):
    rng = np.random.default_rng(5)
    p = rand_seq(rng, 150)
    p1 = p[:70] + "ACGT"[("ACGT".index(p[70]) + 1) % 4] + p[71:]          # one substitution
    f = [rand_seq(rng, n) for n in (300, 400, 500, 600, 700)]
    half = rand_seq(rng, 200)
    cases = {
        "two records": ([f[0] + p + f[1], f[2] + p + f[3]], p, 0),
        "two records, the second first in the other strand": ([f[0] + R.revcomp(p) + f[1], f[2] + p + f[3]], p, 1),
        "palindrome": ([half + R.revcomp(half)], half[40:] + R.revcomp(half)[:60], 0),
        "two copies in one record": ([f[0] + p + f[1] + p + f[2]], p, 0),
        "exact on - beats one edit on +": ([f[0] + p1 + f[1], f[2] + R.revcomp(p) + f[3]], p, 3),
    }
    for name, (recs, call, q) in cases.items():
        ref = B.MapRef(engine, recs)
        g, w = B.op_map(engine, ref, call), R.record(recs, call)
        ref.close()
        assert same(g, w), (name, g, w)
        assert w["status"] == 1 and w["q"] == q and w["anchors"][0]["dist"] == 0, (name, w)
        if name == "two copies in one record":
            assert w["tend"] == 300 + 150
        if name == "exact on - beats one edit on +":
            assert w["anchors"][0]["second"] == 1
        if name in ("two records", "palindrome"):
            assert w["anchors"][0]["second"] == 0


def test_anchors_and_status(B, engine):
    rng = np.random.default_rng(9)
    recs = [rand_seq(rng, 5000), rand_seq(rng, 3000)]
    ys = R.searches(recs)
    ref = B.MapRef(engine, recs)
    W = 64
    seen = []

    def check(call, window, e, status=None, nanchor=None):
        g, w = B.op_map(engine, ref, call, window, e), R.record(recs, call, 4096 if window < 0 else window, 250 if e < 0 else e)
        assert same(g, w), (len(call), window, e, g, w)
        if status is not None:
            assert w["status"] == status, (len(call), window, e, w)
        if nanchor is not None:
            assert w["nanchor"] == nanchor
        seen.append(w["status"])
        return w

    for q in (0, 1, 3):
        y = ys[q]
        for n, na in ((W - 1, 1), (W, 1), (W + 1, 2), (3 * W, 2)):
            check(y[700:700 + n], W, 250, 1, na)
            check(R.edit(rng, y[700:700 + n], 0.05), W, 250, None, None)
        check(y[100:400].replace("C", "Z", 5), W, 250, 1, 2)                     # a concordant pair
        check(y[100:250] + ys[q ^ 2][100:250], W, 250, 3, 2)                      # a pair on different records
        check(y[100:250] + ys[q ^ 1][len(y) - 400:len(y) - 250], W, 250, 3, 2)    # ... on different strands
        check(y[1000:1150] + y[300:450], W, 250, 3, 2)                            # the rear anchor before the front one
        # n = 200, e = 100: the span may miss n by 20
        for gap, status in ((20, 1), (21, 3), (-20, 1), (-21, 3)):
            check(y[1000:1100] + y[1100 + gap:1200 + gap], W, 100, status, 2)
        check(rand_seq(rng, 150) + y[100:250], W, 100, 2, 2)                      # one anchor over its bound
        check(y[100:250] + rand_seq(rng, 150), W, 100, 2, 2)
        exact = y[2000:2300]
        check(exact, -1, 0, 1, 1)                                                 # e = 0: exact copies only
        check(exact[:150] + "ACGT"[("ACGT".index(exact[150]) + 1) % 4] + exact[151:], -1, 0, 2, 1)
        check(exact[:150] + "ACGT"[("ACGT".index(exact[150]) + 1) % 4] + exact[151:], W, 0, 1, 2)      # (the edit lies in neither anchor)
    w = check("", -1, -1, 0)
    assert not R.raw(w).any()
    check(rand_seq(rng, 5000), -1, -1, 2, 2)
    check(ys[1][200:4800], -1, -1, 1, 2)                                          # the default window: two anchors of 4096
    check(R.edit(rng, ys[2][100:2900], 0.1), 1024, -1, 1, 2)
    ref.close()
    assert set(seen) == {0, 1, 2, 3}


def test_refusals(B, engine):
    for bad in ([], ["A"] * 1025, ["ACGT", ""], ["ACGN"], ["acgt"], ["ACGZ"], ["A" * (1 << 19), "C" * (1 << 19), "G"]):
        with pytest.raises(B.FFHipError) as ei:
            B.MapRef(engine, bad)
        if len(bad) == 2:
            assert "record 1" in str(ei.value) and "position 0" in str(ei.value), str(ei.value)
    with pytest.raises(B.FFHipError) as ei:
        B.MapRef(engine, ["ACGT", "ACGTTNA"])
    assert "record 1" in str(ei.value) and "position 5" in str(ei.value), str(ei.value)
    full = B.MapRef(engine, ["A" * (1 << 19), "C" * (1 << 19)])                  # 2^20 in all
    assert B.op_map(engine, full, "C" * 100)["anchors"][0] == {"q": 2, "start": 0, "end": 100, "dist": 0, "second": 100}
    full.close()
    many = B.MapRef(engine, ["ACGT"[k % 4] for k in range(1024)])
    assert B.op_map(engine, many, "G")["anchors"][0] == {"q": 3, "start": 0, "end": 1, "dist": 0, "second": 0}      # (record 1, C, on its other strand, before record 2, G)
    many.close()
    ref = B.MapRef(engine, ["ACGTTGCA" * 20])
    for window, e in ((63, -1), (4097, -1), (0, -1), (-1, 501)):
        with pytest.raises(B.FFHipError):
            B.op_map(engine, ref, "ACGT", window, e)
    B.op_map(engine, ref, "ACGT", 64, 500)
    B.op_map(engine, ref, "ACGT", 4096, 0)
    for pattern in ("", "A" * 4097, "ACGN", "acgt"):
        with pytest.raises(B.FFHipError):
            B.op_map_scores(engine, ref, pattern)
    with pytest.raises(B.FFHipError):
        B.op_map(engine, ref, "ACGN")
    rng = np.random.default_rng(2)
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    b = B.Batch(dm, 4, 1000)
    b.set_signals(rng.standard_normal((4, 1000)).astype(np.float32))
    with pytest.raises(B.FFHipError) as ei:                   # no reference attached
        b.run(1.0, B.RUN_MAP)
    assert "no reference" in str(ei.value)
    for window, e in ((63, -1), (4097, -1), (-1, 501)):
        with pytest.raises(B.FFHipError):
            b.set_map(ref, window, e)
    b.set_map(ref)
    with pytest.raises(B.FFHipError) as ei:
        b.run(1.0, B.RUN_MAP | B.RUN_NO_DECODE)
    assert "map needs a decoded run" in str(ei.value)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    with pytest.raises(B.FFHipError):                         # a run without the flag made none
        b.map(0)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_MAP)
    b.finish()
    assert b.map(0)["n"] == len(b.basecall(0))
    b.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    b = B.Batch(dm, 4, 1000)
    b.set_signals(rng.standard_normal((4, 1000)).astype(np.float32))
    b.set_map(ref)
    with pytest.raises(B.FFHipError) as ei:
        b.run(1.0, B.RUN_MAP)
    assert "map: a flip-flop model only" in str(ei.value)
    b.close()
    dm.close()
    ref.close()


# ------------------------------------------------------------------------------------ batches
def reference_of(rng, calls):
    """random filler plus every read's own call with 5 % edits on an alternating strand, in three records"""
    recs = ["", "", ""]
    for i, c in enumerate(calls):
        x = R.edit(rng, c.replace("Z", "C"), 0.05) if c else ""
        recs[i % 3] += rand_seq(rng, 150 + 37 * (i % 5)) + (x if i % 2 == 0 else R.revcomp(x))
    return [r + rand_seq(rng, 200) for r in recs]


def _check_batches(B, engine, bs, nreads, flags, seen, where, params=((-1, -1), (128, 200)), temperature=1.0, others=False, empty=()):
    """the batches (one, or a pair run together) without the flag; a reference from those calls; then with the flag: nothing else moves, and every record equals
    the restatement on the batch's own call.  empty: slots of bs[0] without a read -- the batch gives nothing of theirs out, a map record no more than a call"""
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
        for x in bs:
            x.finish()
    rng = np.random.default_rng(17)
    kits = []
    if others:                                            # together with barcodes, adapters and truth
        flags |= B.RUN_BARCODES | B.RUN_ADAPTERS | B.RUN_TRUTH
        kits = [B.Barcodes(engine, [rand_seq(rng, 24) for _ in range(5)]), B.Adapters(engine, [rand_seq(rng, 12) for _ in range(4)])]
        for k, x in enumerate(bs):
            x.set_barcodes(kits[0])
            x.set_adapters(kits[1])
            x.set_truth([rng.integers(0, 4, 300).astype(np.uint8) for _ in range(nreads[k])])
    run(flags)

    def state(x, v):
        st = _state(B, x, v, flags)
        if others:
            t = x.truth(v)
            st.update(bc=repr(x.barcode(v)), ad=repr(x.adapters(v)), tr=repr({k: t[k] for k in t if k != "ops"}), ops=np.zeros(0, np.uint8) if t["ops"] is None else t["ops"])
        return st
    before = [[state(x, v) if v not in empty else None for v in range(nreads[k])] for k, x in enumerate(bs)]
    with pytest.raises(B.FFHipError):
        bs[0].map(0)                                      # a run without the flag made none
    recs = reference_of(rng, [st["call"] for sts in before for st in sts if st is not None])
    ref = B.MapRef(engine, recs)
    for window, e in params:
        for x in bs:
            x.set_map(ref, window, e)
        run(flags | B.RUN_MAP)
        for k, x in enumerate(bs):
            for v in range(nreads[k]):
                if v in empty:
                    with pytest.raises(B.FFHipError):
                        x.map(v)
                    seen["empty"] += 1
                    continue
                st, old = state(x, v), before[k][v]
                for key in st:
                    assert st[key] == old[key] if isinstance(st[key], str) else np.array_equal(np.asarray(st[key]), np.asarray(old[key])), (where, k, v, key)
                want = R.record(recs, st["call"], 4096 if window < 0 else window, 250 if e < 0 else e)
                got = x.map(v)
                assert same(got, want), (where, k, v, window, e, got, want)
                seen["reads"] += 1
                seen["status"][want["status"]] += 1
                seen["two"] += want["nanchor"] == 2
                seen["minus"] += want["status"] == 1 and want["q"] & 1
    for x in bs:
        x.set_map(None)
    with pytest.raises(B.FFHipError):                     # no reference attached
        bs[0].run(temperature, flags | B.RUN_MAP)
    ref.close()
    for k in kits:
        k.close()
    if others:
        for x in bs:
            x.set_truth(None)


def _tally():
    return {"reads": 0, "status": [0, 0, 0, 0], "two": 0, "minus": 0, "empty": 0}


def _mapped_enough(seen):
    """the restatement itself says that at least 90 % of the reads with a call map: a condition on the inputs"""
    called = seen["reads"] - seen["status"][0]
    assert called > 0 and seen["status"][1] * 10 >= called * 9, seen


@pytest.mark.parametrize("kind,hidden", [(M.NET_LSTM5, 256), (M.NET_LSTM5, 384), (M.NET_GRUMOD5, 256)])
def test_batch_records_rows_ragged_packed(B, engine, kind, hidden):
    seen = _tally()
    dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
    rng = np.random.default_rng(hidden + kind)
    # one read a row, all of one length
    b = B.Batch(dm, 16, 1500)
    b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
    _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE, seen, ("rows", kind, hidden))
    _check_batches(B, engine, [b], [16], B.RUN_MOVES, seen, ("rows + others", kind, hidden), params=((-1, -1),), others=True)
    b.close()
    # ragged, with an empty slot
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(600, 2001, 13)) + [0, 5000, 3000]]
    b = B.Batch(dm, 16, 5000)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE, seen, ("ragged --viterbi", kind, hidden), empty=(13,))
    b.close()
    assert seen["empty"] == 2, seen                       # the empty slot, under both parameter sets: the kernels passed it by, its neighbours' records are whole
    # packed: default, launch per step
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    _check_batches(B, engine, [pb], [n], B.RUN_NO_TRACE, seen, ("packed", kind, hidden), params=((-1, -1),))
    _check_batches(B, engine, [pb], [n], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, seen, ("packed per step", kind, hidden), params=((100, 250),), others=True)
    pb.close()
    dm.close()
    _mapped_enough(seen)
    assert seen["reads"] >= 120 and seen["two"] >= 30 and seen["minus"] >= 20, seen


def test_batch_records_paired_and_after_an_f32_rerun(B, engine):
    seen = _tally()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 16, 1500)
        b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
        pair.append(b)
    _check_batches(B, engine, pair, [16, 16], B.RUN_NO_TRACE, seen, "pair", params=((-1, -1),))
    for b in pair:
        b.close()
    pbs = [_packed_batch(B, dm, 16, 4000, 24, rng) for _ in range(2)]
    _check_batches(B, engine, [p[0] for p in pbs], [p[1] for p in pbs], B.RUN_NO_TRACE | B.RUN_MOVES, seen, "packed pair", params=((128, 200),))
    for p in pbs:
        p[0].close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their records
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], 0, seen, "rerun rows", params=((-1, -1),))
    assert b.f32_reruns() == 1
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, engine, [pb], [16], B.RUN_MOVES, seen, "rerun packed", params=((128, 250),), others=True)
    assert pb.f32_reruns() == sum(1 for k in range(16) if slot[k] == slot[1]) >= 1
    pb.close()
    dm.close()
    _mapped_enough(seen)
    assert seen["reads"] >= 100, seen


def test_exactly_one_more_copy_call(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(1)
    b = B.Batch(dm, 8, 2000)
    b.set_signals(rng.standard_normal((8, 2000)).astype(np.float32))
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    ref = B.MapRef(engine, [rand_seq(rng, 5000), rand_seq(rng, 300)])
    for x, nr in ((b, 8), (pb, n)):
        x.set_map(ref)
        calls, held = {}, {}
        for fl in (B.RUN_MAP, 0, B.RUN_MAP):                    # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            before = x.device_bytes() if fl and not held else None
            x.run(1.0, B.RUN_NO_TRACE | fl)
            x.finish()
            calls[fl] = _d2h_calls(B)
            if before is not None:
                held = {"grew": x.device_bytes() - before}
        assert calls[B.RUN_MAP][0] == calls[0][0] + 1, calls
        assert calls[B.RUN_MAP][1] == calls[0][1] + 64 * nr, calls          # ... of 64 bytes a read
        assert held["grew"] >= 64 * nr, held                                 # the device buffers are counted, and taken by the first run with the flag only
        assert set(x.map(0)) == {"status", "n", "nanchor", "q", "tstart", "tend", "anchors", "raw"}
    ref.close()
    b.close()
    pb.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_map(tmp_path):
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

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    recs = _records(default, "fastq")
    assert len(recs) == nread
    calls = [(r[0], r[1]) for r in recs]
    longest = max(len(c) for _, c in calls)
    assert 300 <= longest <= 1279, longest                    # (--truth-band takes 1279 at most)
    # the reference: filler, and the calls but two with 5 % edits on alternating strands, in three records; several lines a record, some lower case
    krng = np.random.default_rng(5)
    records = ["", "", ""]
    for i, (_, c) in enumerate(calls[:-2]):
        x = R.edit(krng, c.replace("Z", "C"), 0.05)
        records[i % 3] += rand_seq(krng, 200 + 31 * i) + (x if i % 2 == 0 else R.revcomp(x))
    records = [r + rand_seq(krng, 150) for r in records]
    names, lens = ["chrA", "plasmid.1", "third"], [len(r) for r in records]
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(">%s some words\n%s\n" % (nm, "\n".join((r[k:k + 70].lower() if k % 140 else r[k:k + 70]) for k in range(0, len(r), 70))) for nm, r in zip(names, records)))
    seen = set()
    for opts, W, e in (([], 4096, 250), (["--map-window", "128", "--map-max-error", "200"], 128, 200), (["--reverse"], 4096, 250)):
        hits, fasta = tmp_path / "hits.tsv", tmp_path / "recs.fa"
        got, err = run(["--map", str(fa), "--map-out", str(hits), "--map-records", str(fasta)] + opts)
        base = default if "--reverse" not in opts else run(["--reverse"])[0]
        assert got == base                                    # stdout does not change
        want = [R.record(records, c, W, e) for _, c in calls]
        assert hits.read_text() == "".join(R.hits_line(nm, w, names, lens) for (nm, _), w in zip(calls, want))
        assert fasta.read_text() == "".join(R.record_text(nm, w, records) for (nm, _), w in zip(calls, want))
        assert dict(re.findall(r"^map\t(\S+)\t(\S+)$", err, re.M)) == R.summary(want, W), err
        seen |= {(w["status"], w["nanchor"]) for w in want}
        if not opts:
            first = want
    assert {(1, 1), (1, 2), (2, 1)} <= seen, seen
    assert sum(w["status"] == 1 for w in first) >= nread - 2
    # the loop closed: the same reads against their own stretches; the band excludes nothing, so dist is the anchor's dist
    run(["--map", str(fa), "--map-out", str(tmp_path / "hits.tsv"), "--map-records", str(tmp_path / "recs.fa")])
    acc = tmp_path / "acc.tsv"
    run(["--truth", str(tmp_path / "recs.fa"), "--truth-out", str(acc), "--truth-band", "1279"])
    rows = {f[0]: f for f in (line.split("\t") for line in acc.read_text().splitlines())}
    checked = 0
    for (nm, _), w in zip(calls, first):
        if w["status"] == 1 and w["nanchor"] == 1:
            assert rows[nm][1] == "1" and int(rows[nm][6]) == w["anchors"][0]["dist"], (nm, rows[nm][:8], w)
            assert int(rows[nm][3]) == w["tend"] - w["tstart"]
            checked += 1
        else:
            assert nm not in rows
    assert checked >= nread - 2
