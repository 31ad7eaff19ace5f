"""flappie --truth on the GPU: a call aligned to the sequence it should have been by k_truth (include/ffhip.h FFHIP_RUN_TRUTH, ffhip_batch_set_truth,
ffhip_batch_truth, ffhip_op_truth).

  * the operator's record and op bytes equal the restatement (truth_ref.py) at every kernel form and window edge, with planted edits that leave the band alone,
    touch it, or leave no path; a call with Z; a pair of one letter; the refusals;
  * on synthetic 8-state and 10-state models every record equals the restatement on the call that run returned -- one read a row, ragged, packed, launch per step,
    paired, with the barcode and remap records, after an f32 re-run -- with status 0 and status 2 reads beside aligned ones, and everything else the batch returns
    is bit for bit that of the same run without the flag;
  * a finished run with the flag makes exactly one more device-to-host copy call; the workspace is counted and does not grow on a second run;
  * the binary's acc.tsv and summary.
Integers and bytes only: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from flappie_amd import model as M
import truth_ref as T
from test_truth import brute

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


def letters(codes):
    return "".join("ACGTZ"[c] for c in codes)


def same_record(got, want, where):
    for f in T.FIELDS:
        assert got[f] == want[f], (where, f, got[f], want[f])
    if want["status"] == 1:
        assert np.array_equal(got["ops"], want["ops"]), (where, T.cigar(got["ops"])[:120], T.cigar(want["ops"])[:120])
    else:
        assert got["ops"] is None, where


def planted(rng, n, m):
    """a truth of m random bases and a call of n made from it: the length difference as ONE gap near the front (the path must leave the centre line by about that
    much), then a few substitutions and a balanced insertion / deletion further on"""
    t = rng.integers(0, 4, m)
    s = list(t)
    at = min(3, n, m)
    if n > m:
        s[at:at] = list(rng.integers(0, 4, n - m))
    elif n < m:
        del s[at:at + (m - n)]
    for _ in range(min(4, n // 8)):
        s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 4))
    if len(s) > 40:
        del s[len(s) // 2]
        s.insert(3 * len(s) // 4, int(rng.integers(0, 4)))
    assert len(s) == n
    return letters(s), t.astype(np.uint8)


SIZES = [(0, 1), (1, 1), (1, 64), (63, 64), (64, 65), (65, 64), (257, 300), (800, 760), (3000, 2900)]


@pytest.fixture(scope="module")
def seen():
    return {"forms": set(), "kinds": set()}


@pytest.mark.parametrize("n,m", SIZES)
def test_operator_against_the_restatement(B, engine, seen, n, m):
    rng = np.random.default_rng(1000 * n + m)
    call, t = planted(rng, n, m)
    for W in (0, 1, 7, 64, 512, B.TRUTH_BAND_MAX):
        want = T.truth(call, t, W)
        got = B.op_truth(engine, call, t, W)
        same_record(got, want, (n, m, W))
        seen["forms"].add(B.truth_form(min(2 * W + 1, n + 1)))
        kind = "no path" if want["status"] == 2 else "touched" if want["maxdev"] == W else "inside"
        seen["kinds"].add(kind)
        if kind == "inside" and max(n, m) <= 65:          # the band did not matter: the unbanded programme gives the same path
            dist, ops = brute(list(T.call_codes(call)), list(T.fold(t)))
            assert got["dist"] == dist and list(got["ops"]) == ops, (n, m, W)


def test_operator_took_every_form_and_every_kind_of_case(B, seen):
    """(after the sweep above) the four kernel forms, and cases inside the band, on its edge and without a path"""
    assert seen["forms"] == {0, 1, 2, 3}, seen
    assert seen["kinds"] == {"inside", "touched", "no path"}, seen
    # the windows at which the form changes: 64 | 65 cells (one register to four), 256 | 257 (one wave to a workgroup), 1280 | 1281
    assert [B.truth_form(w) for w in (63, 64, 65, 256, 257, 1280, 1281, 2560, 2561)] == [0, 0, 1, 1, 2, 2, 3, 3, -1]


def test_operator_special_inputs(B, engine):
    rng = np.random.default_rng(6)
    # Z in the call and in the truth reads as C
    t = rng.integers(0, 5, 300).astype(np.uint8)
    s = list(t)
    del s[40:43]
    s[100] = 4
    s[101] = 1
    call = letters(s)
    assert "Z" in call and 4 in t
    for W in (2, 3, 30, 512):
        same_record(B.op_truth(engine, call, t, W), T.truth(call, t, W), ("Z", W))
    assert B.op_truth(engine, "AZZC", [0, 1, 4, 4], 1)["dist"] == 0
    # one letter: every cell ties, the rule alone decides the path
    for n, m in ((64, 64), (65, 60), (60, 65), (300, 257), (700, 900)):
        for W in (0, 5, 64, 400, B.TRUTH_BAND_MAX):
            same_record(B.op_truth(engine, "A" * n, np.zeros(m, np.uint8), W), T.truth("A" * n, np.zeros(m, np.uint8), W), ("one letter", n, m, W))
    # the call much the longer (the window jumps by tens of cells a row) and much the shorter
    for n, m in ((2000, 17), (17, 2000), (2561, 1), (5000, 40)):
        call, t = letters(rng.integers(0, 4, n)), rng.integers(0, 4, m).astype(np.uint8)
        for W in (0, 9, 200, B.TRUTH_BAND_MAX):
            same_record(B.op_truth(engine, call, t, W), T.truth(call, t, W), ("skew", n, m, W))
    # m = 0: status 2; n = 0: m deletions
    got = B.op_truth(engine, "ACGT", np.zeros(0, np.uint8), 4)
    assert (got["status"], got["n"], got["m"], got["ops"]) == (2, 4, 0, None)
    got = B.op_truth(engine, "", np.array([0, 1, 2], np.uint8), 0)
    assert (got["status"], got["dist"], got["n_del"], list(got["ops"])) == (1, 3, 3, [3, 3, 3])


def test_operator_refusals(B, engine):
    ok = np.array([0, 1, 2, 3], np.uint8)
    B.op_truth(engine, "ACGT", ok, 3)
    for call, t, W in (("ACGN", ok, 3), ("acgt", ok, 3), ("ACGT", np.array([0, 5], np.uint8), 3), ("ACGT", ok, -1), ("ACGT", ok, B.TRUTH_BAND_MAX + 1)):
        with pytest.raises(B.FFHipError):
            B.op_truth(engine, call, t, W)
    B.op_truth(engine, "ACGT", ok, B.TRUTH_BAND_MAX)


# ------------------------------------------------------------------------------------ batches
def codes_of(call):
    return np.array(["ACGTZ".index(c) for c in call], np.uint8)


def test_batch_refusals(B, engine):
    """what ffhip_batch_set_truth and a run with the flag refuse (include/ffhip.h "truth"), and that a refusal leaves the batch as it was"""
    rng = np.random.default_rng(2)
    sig = rng.standard_normal((4, 1500)).astype(np.float32)
    seqs = [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(4)]

    def refused(what, f, *args):
        with pytest.raises(B.FFHipError) as e:
            f(*args)
        assert what in str(e.value), (what, str(e.value))
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    b = B.Batch(dm, 4, 1500)
    b.set_signals(sig)
    refused("no truths", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_TRUTH)
    refused("band", b.set_truth, seqs, -1)
    refused("2560", b.set_truth, seqs, B.TRUTH_BAND_MAX + 1)
    refused("code 4", b.set_truth, seqs[:3] + [np.array([0, 1, 4, 2], np.uint8)], 8)
    refused("reads", b.set_truth, seqs[:3], 8)
    refused("no truths", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_TRUTH)           # (a refused call set nothing)
    b.set_truth(seqs, 8)
    refused("FFHIP_RUN_NO_DECODE", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_NO_DECODE | B.RUN_TRUTH)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_TRUTH)
    refused("between a run and its finish", b.set_truth, seqs, 9)
    b.finish()
    for v in range(4):
        same_record(b.truth(v), T.truth(b.basecall(v), seqs[v], 8), v)      # (band 8: the refused call between run and finish changed nothing)
    refused("band", b.set_truth, seqs, B.TRUTH_BAND_MAX + 1)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_TRUTH)
    b.finish()
    same_record(b.truth(2), T.truth(b.basecall(2), seqs[2], 8), "after a refusal")
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    refused("FFHIP_RUN_TRUTH", b.truth, 0)                                   # a run without the flag made none
    b.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    b = B.Batch(dm, 4, 1500)
    b.set_signals(sig)
    refused("run-length", b.set_truth, seqs, 8)
    refused("run-length", b.run, 1.0, B.RUN_TRUTH)
    b.run(1.0, 0)
    b.finish()
    b.close()
    dm.close()


def _state(B, b, v, flags):
    path, qpath = b.path(v)
    st = dict(path=path, qpath=qpath.view(np.uint32), score=np.float32(b.score(v)).view(np.uint32), call=b.basecall(v), qual=b.quality(v),
              trans=b.transitions(v).view(np.uint32))
    if not (flags & B.RUN_NO_TRACE):
        st["trace"] = b.trace(v)
    if flags & B.RUN_MOVES:
        st["mv"] = b.moves(v)
    if flags & B.RUN_BARCODES:
        st["bc"] = tuple(sorted(b.barcode(v).items()))
    if flags & B.RUN_REMAP:
        rm = b.remap(v)
        st["rm_status"], st["rm_score"] = np.int64(rm["status"]), np.float32(rm["score"]).view(np.uint32)
        st["rm"] = np.zeros(0, np.uint8) if rm["rm"] is None else rm["rm"]
    return st


def _same(a, b):
    return a == b if isinstance(a, (str, tuple)) else np.array_equal(np.asarray(a), np.asarray(b))


def _truths(rng, calls, nbase):
    """per read, in turn: its own call, its call with planted edits, a random sequence, none (status 0), an empty one (status 2)"""
    seqs = []
    for v, call in enumerate(calls):
        own, kind = codes_of(call), v % 5
        if kind == 0:
            q = own
        elif kind == 1:
            q = list(own)
            for _ in range(8):
                at = int(rng.integers(0, max(1, len(q))))
                what = int(rng.integers(0, 3))
                if what == 0 and q:
                    q[at] = int(rng.integers(0, nbase))
                elif what == 1:
                    q.insert(at, int(rng.integers(0, nbase)))
                elif len(q) > 1:
                    del q[at]
            q = np.array(q, np.uint8)
        elif kind == 2:
            q = rng.integers(0, nbase, max(1, own.size + int(rng.integers(-20, 21)))).astype(np.uint8)
        elif kind == 3:
            q = None
        else:
            q = np.zeros(0, np.uint8)
        seqs.append(q)
    return seqs


def _check_batches(B, bs, nreads, flags, where, nbase, band=24, temperature=1.0):
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
            assert bs[0].paired() and bs[1].paired(), where
        for x in bs:
            x.finish()
    run(flags)
    before = [[_state(B, x, v, flags) for v in range(nreads[k])] for k, x in enumerate(bs)]
    rng = np.random.default_rng(29)
    seen = set()
    for k, x in enumerate(bs):
        x._truths = _truths(rng, [st["call"] for st in before[k]], nbase)
        x.set_truth(x._truths, band)
    run(flags | B.RUN_TRUTH)
    for k, x in enumerate(bs):
        for v in range(nreads[k]):
            st, old = _state(B, x, v, flags), before[k][v]
            for key in st:
                assert _same(st[key], old[key]), (where, k, v, key)
            q, got = x._truths[v], x.truth(v)
            if q is None:
                assert (got["status"], got["n"], got["m"], got["ops"]) == (0, len(st["call"]), 0, None), (where, k, v, got)
                seen.add(0)
                continue
            want = T.truth(st["call"], q, band)
            same_record(got, want, (where, k, v))
            seen.add(want["status"])
            if v % 5 == 0 and q.size:
                assert got["dist"] == 0 and got["n_match"] == q.size and not got["ops"].any(), (where, k, v)
    assert seen == {0, 1, 2}, (where, seen)
    for x in bs:
        x.set_truth(None)


def _packed_batch(B, dm, rows, cap, nreads, rng, lo=600, hi=2000):
    lens = [int(x) for x in rng.integers(lo, hi + 1, nreads)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    return pb, len(sigs)


@pytest.mark.parametrize("kind,nbase", [(M.NET_LSTM5, 4), (M.NET_GRUMOD5, 5)])
def test_batch_records_rows_ragged_packed(B, engine, kind, nbase):
    dm = B.DeviceModel(engine, M.synthetic_model(kind, 256, seed=1))
    rng = np.random.default_rng(256 + kind)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
    _check_batches(B, [b], [16], B.RUN_NO_TRACE, ("rows", kind), nbase)
    _check_batches(B, [b], [16], B.RUN_MOVES, ("rows + moves", kind), nbase, band=B.TRUTH_BAND_MAX)
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, [b], [16], B.RUN_NO_TRACE, ("ragged", kind), nbase, band=40)
    # with the barcode and the remap records of the same run
    kit = B.Barcodes(engine, ["ACGTACGTACGTACGTACGTAAAA", "TTGACCATGACCATGGTACCATGA"])
    b.set_barcodes(kit)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    b.set_remap([codes_of(b.basecall(v)) if len(b.basecall(v)) else None for v in range(16)], 64)
    _check_batches(B, [b], [16], B.RUN_NO_TRACE | B.RUN_BARCODES | B.RUN_REMAP, ("ragged + barcodes + remap", kind), nbase, band=512)
    b.close()
    kit.close()
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    _check_batches(B, [pb], [n], B.RUN_NO_TRACE, ("packed", kind), nbase, band=150)
    _check_batches(B, [pb], [n], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE | B.RUN_MOVES, ("packed per step", kind), nbase, band=7)
    pb.close()
    dm.close()


def test_batch_records_paired_and_after_an_f32_rerun(B, engine):
    # paired launches: one layer launch for two batches is what the H = 384 pair kernel takes, 256 reads a batch
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 256, 1000)
        b.set_signals(rng.standard_normal((256, 1000)).astype(np.float32))
        pair.append(b)
    _check_batches(B, pair, [256, 256], B.RUN_NO_TRACE | B.RUN_MOVES, "pair", 4)
    for b in pair:
        b.close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their records and ops.  H = 128 and these signals are the outlier case every re-run test
    # of the suite uses (test_barcodes_gpu, test_remap_gpu, test_packed_gpu): which reads go again is known there.  What is checked here -- the side batch's
    # records and ops patched into both halves of the batch's buffer -- is host code that does not depend on H
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, [b], [16], 0, "rerun rows", 4)
    assert b.f32_reruns() == 2
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, [pb], [16], B.RUN_MOVES, "rerun packed", 4, band=300)
    assert pb.f32_reruns() >= 2
    pb.close()
    dm.close()


def _d2h_calls(B):
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, 1)
    return int(c[2]), int(c[3])


def test_exactly_one_more_copy_call_and_the_workspace_is_counted(B, engine):
    B.lib().ffhip_debug_batch_device_bytes.restype = C.c_size_t
    B.lib().ffhip_debug_batch_device_bytes.argtypes = [C.c_void_p]
    rng = np.random.default_rng(1)

    def one_more(xs, nrs, flags, where):
        held = [B.lib().ffhip_debug_batch_device_bytes(x.h) for x in xs]
        for x, nr in zip(xs, nrs):
            x.set_truth([rng.integers(0, 4, 100).astype(np.uint8)] * nr, 24)
        calls, grown = {}, []
        for fl in (B.RUN_TRUTH, 0, B.RUN_TRUTH):               # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            if len(xs) == 1:
                xs[0].run(1.0, flags | fl)
            else:
                xs[0].run_pair(xs[1], 1.0, flags | fl)
            for x in xs:
                x.finish()
            calls[fl] = _d2h_calls(B)
            grown.append([B.lib().ffhip_debug_batch_device_bytes(x.h) for x in xs])
        assert calls[B.RUN_TRUTH][0] == calls[0][0] + len(xs), (where, calls)
        assert grown[0] == grown[1] == grown[2], (where, grown)                # no growth on a second run
        for x, nr, h, g in zip(xs, nrs, held, grown[0]):
            # a window of 49 cells: the one-wave form of one register, two 64-bit words a row of the truth; 48 bytes of record and m + blocks + 1 of ops a read
            assert g >= h + nr * (100 * 2 * 8 + 48) + sum(100 + x.read_nblock(v) + 1 for v in range(nr)), where
            assert x.truth(0)["status"] == 1, where
            x.set_truth(None)

    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    b = B.Batch(dm, 8, 2000)
    b.set_signals(rng.standard_normal((8, 2000)).astype(np.float32))
    one_more([b], [8], B.RUN_NO_TRACE, "rows")
    b.close()
    b = B.Batch(dm, 8, 2000)
    b.set_signals_ragged([rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 8)])
    one_more([b], [8], B.RUN_NO_TRACE, "ragged")
    one_more([b], [8], B.RUN_NO_TRACE | B.RUN_STEPWISE_RNN | B.RUN_MOVES, "ragged per step")
    b.close()
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    one_more([pb], [n], B.RUN_NO_TRACE, "packed")
    one_more([pb], [n], B.RUN_NO_TRACE | B.RUN_STEPWISE_RNN, "packed per step")
    pb.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_truth(tmp_path):
    import os
    import re
    import subprocess
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 12
    names = ["uuid-%04d" % i for i in range(nread)]
    for i, n in enumerate(rng.integers(1500, 5000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), names[i], synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default, _ = run([])
    lines = default.split("\n")[:-1]
    recs = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    order = [r[0][1:].split("  {")[0] for r in recs]
    calls = {r[0][1:].split("  {")[0]: r[1] for r in recs}
    assert sorted(order) == names
    # records: by read id (own call), by file name (edited call), a bad letter, an empty one, none
    seqs, text = {}, ""
    for i, name in enumerate(names):
        call, kind = calls[name], i % 5
        if kind == 0:
            seqs[name] = (name, call)
            text += ">%s own call\n%s\n%s\n" % (name, call[:7].lower(), call[7:])
        elif kind == 1:
            q = call[:5] + call[9:40] + "T" + call[40:] + "ACGT"
            seqs[name] = ("read_%02d" % i, q)
            text += ">read_%02d\n%s\n" % (i, q)
        elif kind == 2:
            seqs[name] = (name, call[:3] + "N" + call[3:])
            text += ">%s\n%s\n" % seqs[name]
        elif kind == 3:
            seqs[name] = ("read_%02d.fast5" % i, "")
            text += ">read_%02d.fast5\n" % i
    refs = tmp_path / "refs.fa"
    refs.write_text(text)
    first = None
    for band_opts, band in (([], 512), (["--truth-band", "3"], 3)):
        out = tmp_path / ("acc%d.tsv" % band)
        stdout, err = run(["--truth", str(refs), "--truth-out", str(out)] + band_opts)
        assert stdout == default
        want, ids, counts, pooled = "", [], {"aligned": 0, "not_aligned": 0, "no_record": 0, "band_touched": 0}, [0, 0]
        for name in order:
            if name not in seqs:
                counts["no_record"] += 1
                continue
            ref_name, q = seqs[name]
            rec = T.truth(calls[name], [] if "N" in q else ["ACGT".index(c) for c in q], band)
            want += T.tsv_line(ref_name, rec, band)
            if rec["status"] == 1:
                counts["aligned"] += 1
                counts["band_touched"] += int(rec["maxdev"] == band)
                ids.append(T.identity(rec))
                pooled[0] += rec["n_match"]
                pooled[1] += rec["dist"] + rec["n_match"]
            else:
                counts["not_aligned"] += 1
        assert out.read_text() == want
        summary = dict(re.findall(r"^truth\t(\S+)\t(\S+)$", err, re.M))
        for key, val in counts.items():
            assert int(summary[key]) == val, (key, summary)
        assert summary["pooled_identity"] == "%.6f" % (pooled[0] / pooled[1]) and summary["median_identity"] == "%.6f" % float(np.median(ids)), summary
        assert counts["aligned"] >= 5 and counts["not_aligned"] >= 4 and counts["no_record"] >= 2
        first = first or want
    assert "\t1.000000\t" in first
    # --reverse turns the output round, not the alignment; --remap may read the same file in the same run
    rev = tmp_path / "rev.tsv"
    stdout, _ = run(["--reverse", "--truth", str(refs), "--truth-out", str(rev)])
    assert stdout != default and rev.read_text() == first
    both, rmap = tmp_path / "both.tsv", tmp_path / "map.tsv"
    stdout, err = run(["--truth", str(refs), "--truth-out", str(both), "--remap", str(refs), "--remap-out", str(rmap)])
    assert stdout == default and both.read_text() == first and len(rmap.read_text().split("\n")) == len(first.split("\n"))
    assert "remap\tmapped" in err and "truth\taligned" in err
