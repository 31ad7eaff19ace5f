"""flappie --remap on the GPU: a read's transition scores mapped to a given sequence by k_remap (include/ffhip.h FFHIP_RUN_REMAP, ffhip_batch_set_remap,
ffhip_batch_remap, ffhip_op_remap).

  * the operator's score bits and move bytes equal the restatement (remap_ref.py) at every wave, window and kernel-form edge, on random, all-zero and
    quarter-quantised scores, homopolymers and alternating sequences; the refusals;
  * on synthetic 8-state and 10-state models every record equals the restatement on that run's own ffhip_batch_get_transitions -- one read a row, ragged,
    packed, paired, launch per step, f32 re-run, with and without the move table and the barcode records -- with status 0 and status 2 reads beside mapped
    ones, and everything else the batch returns is bit for bit that of the same run without the flag;
  * a finished run with the flag makes exactly one more device-to-host copy call than the same run without;
  * one read of 20 000+ blocks at W = 2048 takes the workgroup form.
No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from flappie_amd import model as M
import remap_ref as R

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


def check_op(B, engine, T, s, nbase, W, where):
    rm, score = B.op_remap(engine, T, nbase, s, W)
    wscore, wrm = R.remap(T, s, nbase, W)
    assert bits(score) == bits(wscore), (where, float(score), float(wscore))
    assert np.array_equal(rm, wrm), (where, np.flatnonzero(rm != wrm)[:6])
    assert int(rm.sum()) == len(s) - 1


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 800])
def test_operator_random_scores(B, engine, N):
    rng = np.random.default_rng(100 + N)
    for nbase in (4, 5):
        P = 2 * nbase * (nbase + 1)
        T = rng.standard_normal((N, P)).astype(np.float32)
        for L in sorted({1, 2, (N + 1) // 2, N, N + 1}):
            if L > N + 1:
                continue
            s = rng.integers(0, nbase, L).astype(np.uint8)
            for W in (0, 1, 31, 32, 33, 2048):
                check_op(B, engine, T, s, nbase, W, (N, nbase, L, W))


def test_operator_special_inputs(B, engine):
    rng = np.random.default_rng(5)
    for nbase in (4, 5):
        P = 2 * nbase * (nbase + 1)
        for N, L in ((65, 40), (300, 300), (300, 170)):
            seqs = [np.full(L, nbase - 1, np.uint8), np.arange(L, dtype=np.uint8) % 2, np.repeat(rng.integers(0, nbase, L), 3)[:L].astype(np.uint8)]
            scores = [np.zeros((N, P), np.float32), (rng.integers(-8, 9, (N, P)) * 0.25).astype(np.float32), rng.standard_normal((N, P)).astype(np.float32)]
            for si, s in enumerate(seqs):
                for ti, T in enumerate(scores):
                    for W in (0, 5, 40, 2048):
                        check_op(B, engine, T, s, nbase, W, (nbase, N, L, si, ti, W))


def test_operator_refusals(B, engine):
    T = np.zeros((10, 40), np.float32)
    ok = np.zeros(5, np.uint8)
    B.op_remap(engine, T, 4, ok, 3)
    for s, nbase, W in ((np.zeros(0, np.uint8), 4, 3), (np.zeros(12, np.uint8), 4, 3), (np.array([0, 4], np.uint8), 4, 3), (ok, 4, -1), (ok, 5, 3)):
        with pytest.raises(B.FFHipError):
            B.op_remap(engine, T, nbase, s, W)
    B.op_remap(engine, T, 4, np.zeros(11, np.uint8), 0)


def test_batch_refusals(B, engine):
    """what ffhip_batch_set_remap and a run with the flag refuse (include/ffhip.h "remap"), each on a batch, and that a refusal leaves the batch as it was"""
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
    refused("no sequences", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP)
    refused("band", b.set_remap, seqs, -1)
    refused("code 4", b.set_remap, seqs[:3] + [np.array([0, 1, 4, 2], np.uint8)], 8)
    refused("reads", b.set_remap, seqs[:3], 8)
    refused("4608", b.set_remap, seqs[:3] + [np.zeros(4610, np.uint8)], 2304)
    refused("no sequences", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP)          # (a refused call set nothing)
    b.set_remap(seqs, 8)
    refused("FFHIP_RUN_NO_DECODE", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_NO_DECODE | B.RUN_REMAP)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP)
    b.finish()
    for v in range(4):
        got = b.remap(v)
        wscore, wrm = R.remap(b.transitions(v), seqs[v], 4, 8)
        assert got["status"] == 1 and bits(got["score"]) == bits(wscore) and np.array_equal(got["rm"], wrm), v
    b.close()
    dm.close()
    # the run-length model: when the sequences are set, and when a run asks
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    b = B.Batch(dm, 4, 1500)
    b.set_signals(sig)
    refused("run-length", b.set_remap, seqs, 8)
    refused("run-length", b.run, 1.0, B.RUN_REMAP)
    b.run(1.0, 0)
    b.finish()
    b.close()
    dm.close()


def test_long_read_takes_the_workgroup_form(B, engine):
    rng = np.random.default_rng(8)
    N, L, W = 20011, 9001, 2048
    assert B.lib().ffhip_debug_remap_form(C.c_size_t(L), W) == 3 and B.lib().ffhip_debug_remap_form(C.c_size_t(64), W) == 0
    T = rng.standard_normal((N, 40)).astype(np.float32)
    s = rng.integers(0, 4, L).astype(np.uint8)
    check_op(B, engine, T, s, 4, W, "long")
    rm, _ = B.op_remap(engine, T, 4, s, W)
    assert R.starts_maxdev(rm, L)[1] <= W


# ------------------------------------------------------------------------------------ batches
def codes_of(call):
    return np.array(["ACGTZ".index(c) for c in call], np.uint8)


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
    return st


def _same(a, b):
    return a == b if isinstance(a, (str, tuple)) else np.array_equal(np.asarray(a), np.asarray(b))


def _sequences(rng, calls, nblocks, nbase):
    """per read, in turn: its own call, its call with planted edits, a random sequence, none (status 0), one base too many for its blocks (status 2)"""
    seqs = []
    for v, call in enumerate(calls):
        own, kind = codes_of(call), v % 5
        if kind == 0 and own.size:
            q = own
        elif kind == 1 and own.size > 4:
            q = list(own)
            for _ in range(6):
                at = int(rng.integers(0, len(q)))
                what = int(rng.integers(0, 3))
                if what == 0:
                    q[at] = int(rng.integers(0, nbase))
                elif what == 1:
                    q.insert(at, int(rng.integers(0, nbase)))
                elif len(q) > 1:
                    del q[at]
            q = np.array(q, np.uint8)
        elif kind == 3:
            q = None
        elif kind == 4:
            q = rng.integers(0, nbase, nblocks[v] + 2).astype(np.uint8)
        else:
            q = rng.integers(0, nbase, max(1, nblocks[v] // 3)).astype(np.uint8)
        seqs.append(q)
    return seqs


def _check_batches(B, bs, nreads, flags, where, nbase, band=24, temperature=1.0):
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
            assert bs[0].paired() and bs[1].paired(), where      # (one layer launch for both: what k_lstm_split_pair takes, 256 reads a batch at H = 384)
        for x in bs:
            x.finish()
    with pytest.raises(B.FFHipError):                     # no sequences set
        bs[0].run(temperature, flags | B.RUN_REMAP)
    run(flags)
    before = [[_state(B, x, v, flags) for v in range(nreads[k])] for k, x in enumerate(bs)]
    with pytest.raises(B.FFHipError):
        bs[0].remap(0)                                    # a run without the flag made none
    rng = np.random.default_rng(23)
    seen = set()
    for k, x in enumerate(bs):
        nblocks = [x.read_nblock(v) for v in range(nreads[k])]
        seqs = _sequences(rng, [st["call"] for st in before[k]], nblocks, nbase)
        x.set_remap(seqs, band)
        x._remap_seqs = seqs
    run(flags | B.RUN_REMAP)
    for k, x in enumerate(bs):
        for v in range(nreads[k]):
            st, old = _state(B, x, v, flags), before[k][v]
            for key in st:
                assert _same(st[key], old[key]), (where, k, v, key)
            q, got, N = x._remap_seqs[v], x.remap(v), x.read_nblock(v)
            want = 0 if q is None else (1 if 1 <= q.size <= N + 1 else 2)
            assert got["status"] == want and got["nblock"] == N, (where, k, v, got["status"], want)
            seen.add(want)
            if want == 1:
                wscore, wrm = R.remap(x.transitions(v), q, nbase, band)
                assert got["L"] == q.size and bits(got["score"]) == bits(wscore), (where, k, v, got["score"], wscore)
                assert np.array_equal(got["rm"], wrm), (where, k, v)
            else:
                assert got["rm"] is None
    assert seen == {0, 1, 2}, (where, seen)
    for x in bs:
        x.set_remap(None)


def _packed_batch(B, dm, rows, cap, nreads, rng, lo=600, hi=2000):
    lens = [int(x) for x in rng.integers(lo, hi + 1, nreads)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    return pb, len(sigs)


@pytest.mark.parametrize("kind,hidden,nbase", [(M.NET_LSTM5, 256, 4), (M.NET_GRUMOD5, 256, 5)])
def test_batch_records_rows_ragged_packed(B, engine, kind, hidden, nbase):
    dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
    rng = np.random.default_rng(hidden + kind)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
    _check_batches(B, [b], [16], B.RUN_NO_TRACE, ("rows", kind), nbase)
    _check_batches(B, [b], [16], B.RUN_MOVES, ("rows + moves", kind), nbase, band=2048)
    b.close()
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, [b], [16], B.RUN_NO_TRACE, ("ragged", kind), nbase, band=40)
    b.close()
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    _check_batches(B, [pb], [n], B.RUN_NO_TRACE, ("packed", kind), nbase, band=150)
    _check_batches(B, [pb], [n], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE | B.RUN_MOVES, ("packed per step", kind), nbase, band=600)
    pb.close()
    dm.close()


def test_batch_records_paired_with_barcodes_and_after_an_f32_rerun(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 256, 1000)
        b.set_signals(rng.standard_normal((256, 1000)).astype(np.float32))
        pair.append(b)
    kit = B.Barcodes(engine, ["ACGTACGTACGTACGTACGTAAAA", "TTGACCATGACCATGGTACCATGA"])
    for b in pair:
        b.set_barcodes(kit)
    _check_batches(B, pair, [256, 256], B.RUN_NO_TRACE | B.RUN_BARCODES | B.RUN_MOVES, "pair", 4)
    for b in pair:
        b.close()
    kit.close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their records and moves
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
    """per batch and finished run, in every batch shape and run form: one read a row, ragged, packed, packed launch per step, paired"""
    B.lib().ffhip_debug_batch_device_bytes.restype = C.c_size_t
    B.lib().ffhip_debug_batch_device_bytes.argtypes = [C.c_void_p]
    rng = np.random.default_rng(1)

    def one_more(xs, nrs, flags, where):
        held = [B.lib().ffhip_debug_batch_device_bytes(x.h) for x in xs]
        for x, nr in zip(xs, nrs):
            x.set_remap([rng.integers(0, 4, 100).astype(np.uint8)] * nr, 2048)
        calls = {}
        for fl in (B.RUN_REMAP, 0, B.RUN_REMAP):              # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            if len(xs) == 1:
                xs[0].run(1.0, flags | fl)
            else:
                xs[0].run_pair(xs[1], 1.0, flags | fl)
            for x in xs:
                x.finish()
            calls[fl] = _d2h_calls(B)
        assert calls[B.RUN_REMAP][0] == calls[0][0] + len(xs), (where, calls)
        for x, nr, h in zip(xs, nrs, held):
            words = sum(x.read_nblock(v) * 4 for v in range(nr))      # a window of 100 cells: the one-wave form of four registers, four 64-bit words a block
            assert B.lib().ffhip_debug_batch_device_bytes(x.h) >= h + 8 * words, where
            assert x.remap(0)["status"] == 1, where
            x.set_remap(None)

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
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    pair = []
    for k in range(2):
        b = B.Batch(dm, 256, 1000)
        b.set_signals(rng.standard_normal((256, 1000)).astype(np.float32))
        pair.append(b)
    one_more(pair, [256, 256], B.RUN_NO_TRACE, "paired")
    assert all(x.paired() for x in pair)
    for b in pair:
        b.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_remap(B, engine, tmp_path):
    import os
    import re
    import subprocess
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 24
    names = ["uuid-%04d" % i for i in range(nread)]
    for i, n in enumerate(rng.integers(1500, 6000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), names[i], synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, extra=None):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    trace = tmp_path / "trace.hdf5"
    default, _ = run(["--format", "fastq", "--trace", str(trace)])
    lines = default.split("\n")[:-1]
    recs = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    order = [r[0][1:].split("  {")[0] for r in recs]
    calls = {r[0][1:].split("  {")[0]: r[1] for r in recs}
    assert sorted(order) == names
    # the engine on the signals the binary saw: transitions, blocks and trimmed starts of every read
    dm = B.DeviceModel(engine, mdl)
    sigs = [dump_trace(trace, name)[0] for name in names]
    b = B.Batch(dm, nread, max(s.size for s in sigs))
    b.set_signals_ragged(sigs)
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    trans = {name: b.transitions(v) for v, name in enumerate(names)}
    assert all(b.basecall(v) == calls[name] for v, name in enumerate(names))
    b.close()
    dm.close()
    # records: by read id (own call, lower case on several lines), by file name (edited call), none, a bad letter, too long
    seqs, text = {}, ""
    for i, name in enumerate(names):
        call, kind = calls[name], i % 5
        if kind == 0:
            seqs[name] = (name, call)
            text += ">%s own call\n%s\n%s\n" % (name, call[:7].lower(), call[7:])
        elif kind == 1:
            q = call[:5] + call[9:] + "ACGT"
            seqs[name] = ("read_%02d" % i, q)
            text += ">read_%02d\n%s\n" % (i, q)
        elif kind == 2:
            seqs[name] = (name, call[:3] + "N" + call[3:])
            text += ">%s\n%s\n" % seqs[name]
        elif kind == 3:
            seqs[name] = ("read_%02d.fast5" % i, "ACGT" * len(call))
            text += ">read_%02d.fast5\n%s\n" % (i, seqs[name][1])
    refs = tmp_path / "refs.fa"
    refs.write_text(text)
    for band_opts, band in (([], 2048), (["--remap-band", "12"], 12)):
        out = tmp_path / ("map%d.tsv" % band)
        stdout, err = run(["--format", "fastq", "--remap", str(refs), "--remap-out", str(out)] + band_opts)
        assert stdout == default
        want, counts = [], {"mapped": 0, "no_record": 0, "refused": 0, "band_touched": 0}
        for name in order:
            if name not in seqs:
                counts["no_record"] += 1
                continue
            ref_name, q = seqs[name]
            T = trans[name]
            N = T.shape[0]
            head = None
            if "N" in q or len(q) > N + 1:
                counts["refused"] += 1
                want.append("%s\t2\t%d\t%d\t%%s\t%d\t%d\t*\t*\t*" % (ref_name, N, mdl.total_stride, 0 if "N" in q else len(q), band))
                continue
            score, rm = R.remap(T, codes_of(q), 4, band)
            start, maxdev = R.starts_maxdev(rm, len(q))
            counts["mapped"] += 1
            counts["band_touched"] += int(maxdev == band)
            want.append("%s\t1\t%d\t%d\t%%s\t%d\t%d\t%d\t%.9g\t%s" % (ref_name, N, mdl.total_stride, len(q), band, maxdev, score, ",".join(str(x) for x in start)))
        got = out.read_text().split("\n")[:-1]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            f = g.split("\t")
            assert int(f[4]) >= 0 and g == w % f[4], (g[:200], w[:200])
        assert dict((k, int(v)) for k, v in re.findall(r"^remap\t(\S+)\t(\d+)$", err, re.M)) == counts, err
        assert counts["mapped"] >= 8 and counts["refused"] >= 8 and counts["no_record"] >= 4
    assert run(["--format", "fastq", "--remap", str(refs), "--remap-out", str(tmp_path / "np.tsv")], {"FLAPPIE_DEBUG": "no_pack"})[0] == default
    assert (tmp_path / "np.tsv").read_text() == (tmp_path / "map2048.tsv").read_text()
