"""flappie --remap-events on the GPU: the signal under every base of a mapped read by k_events (include/ffhip.h FFHIP_RUN_EVENTS, ffhip_batch_events,
ffhip_op_events).

  * the operator against the restatement (events_ref.py) at every wave and round edge, with one base, with a base a block and a last base without one, with the read
    ending inside its last block, with one base of 3900 blocks, and on values a one-pass sum of squares gets wrong; the refusals;
  * on synthetic models, the events of every mapped read against the restatement on the batch's OWN path and the signal it was given -- one read a row, ragged,
    packed, launch per step, paired, f32 re-run -- with nothing for status 0 and 2, everything else the batch returns unchanged, one more device-to-host copy
    call a batch, the buffer counted, the same bytes on a second run and wherever the same path stands in another batch shape;
  * the binary's events.tsv against the restatement on --trace's signal and map.tsv's starts.
first and count are exact; mean and sd are within 2^-23 max|x| of the span (events_ref.tolerance); a span of one repeated value is exact."""
import ctypes as C

import numpy as np
import pytest

from flappie_amd import model as M
import events_ref as E
from test_remap_gpu import _d2h_calls, _same, _sequences, _state

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


# ------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 800])
def test_operator_against_the_restatement(B, engine, N):
    rng = np.random.default_rng(300 + N)
    for stride in (5, 2):
        for L in sorted({1, N + 1, int(rng.integers(1, N + 2)), int(rng.integers(1, N + 2))}):
            rm = np.zeros(N, np.uint8)
            rm[rng.choice(N, L - 1, replace=False)] = 1
            for nsample in (N * stride, N * stride - (stride - 1)):
                x = (rng.standard_normal(nsample) * 3.0 + 1.0).astype(np.float32)
                E.check(B.op_events(engine, x, stride, rm, L), E.events(x, stride, rm, L), x, (N, stride, L, nsample))


def test_operator_long_span_and_hostile_values(B, engine):
    for name, x, stride, rm, L, constant in E.special_cases():
        got, want = B.op_events(engine, x, stride, rm, L), E.events(x, stride, rm, L)
        E.check(got, want, x, name)
        if constant:          # two passes in fp64 give this in any order of summation; a sum of squares does not
            assert np.array_equal(got["mean"], x[got["first"]]) and np.all(got["sd"] == 0.0) and not np.any(np.signbit(got["sd"])), (name, got)
        assert got.tobytes() == B.op_events(engine, x, stride, rm, L).tobytes(), name


def test_operator_refusals(B, engine):
    x, rm = np.ones(50, np.float32), np.array([0, 1, 0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
    assert B.op_events(engine, x, 5, rm, 3)["count"].tolist() == [10, 15, 25]
    two = rm.copy()
    two[0] = 2
    for args in ((x, 5, rm, 2), (x, 5, rm, 4), (x, 5, rm, 0), (x, 0, rm, 3), (x, -1, rm, 3), (x, 5, np.zeros(0, np.uint8), 1), (x, 5, two, 3)):
        with pytest.raises(B.FFHipError) as e:
            B.op_events(engine, *args)
        assert "ffhip error -1:" in str(e.value), (args[1:], str(e.value))          # FFHIP_EINVAL
    assert B.op_events(engine, np.zeros(0, np.float32), 5, rm, 3)["count"].tolist() == [0, 0, 0]      # a read of no samples: every span is empty


# ------------------------------------------------------------------------------------ batches
def _bytes_held(B, x):
    B.lib().ffhip_debug_batch_device_bytes.restype = C.c_size_t
    B.lib().ffhip_debug_batch_device_bytes.argtypes = [C.c_void_p]
    return B.lib().ffhip_debug_batch_device_bytes(x.h)


def _check_batches(B, bs, sigs, flags, where, nbase, stride, band=2048, reruns=False):
    """sigs[k][v]: the signal read v of batch k was given.  Returns {(k, v): (rm bytes, events bytes)} of the mapped reads."""
    def run(fl):
        _d2h_calls(B)
        if len(bs) == 1:
            bs[0].run(1.0, fl)
        else:
            bs[0].run_pair(bs[1], 1.0, fl)
            assert bs[0].paired() and bs[1].paired(), where
        for x in bs:
            x.finish()
        return _d2h_calls(B)[0]
    nreads = [len(s) for s in sigs]
    run(flags)
    rng = np.random.default_rng(23)
    for k, x in enumerate(bs):
        calls = [x.basecall(v) for v in range(nreads[k])]
        x.set_remap(_sequences(rng, calls, [x.read_nblock(v) for v in range(nreads[k])], nbase), band)
    copies = run(flags | B.RUN_REMAP)
    before = [[(_state(B, x, v, flags), x.remap(v)) for v in range(nreads[k])] for k, x in enumerate(bs)]
    held = [_bytes_held(B, x) for x in bs]
    with pytest.raises(B.FFHipError):
        bs[0].events(0)                                     # a run without the flag made none
    copies_ev = run(flags | B.RUN_REMAP | B.RUN_EVENTS)
    if not reruns:                                          # (a re-run's side batch brings its own copies)
        assert copies_ev == copies + len(bs), (where, copies, copies_ev)
    out, seen = {}, set()
    for k, x in enumerate(bs):
        bases = 0
        for v in range(nreads[k]):
            st, (old, rec) = _state(B, x, v, flags), before[k][v]
            for key in st:
                assert _same(st[key], old[key]), (where, k, v, key)
            got, ev = x.remap(v), x.events(v)
            assert got["status"] == rec["status"] and got["L"] == rec["L"] and _same(got["score"].view(np.uint32), rec["score"].view(np.uint32)), (where, k, v)
            seen.add(got["status"])
            if got["status"] != 1:
                assert ev is None and got["rm"] is None, (where, k, v)
                continue
            assert np.array_equal(got["rm"], rec["rm"]), (where, k, v)
            E.check(ev, E.events(sigs[k][v], stride, got["rm"], got["L"]), sigs[k][v], (where, k, v))
            out[(k, v)] = (got["rm"].tobytes(), ev.tobytes())
            bases += got["L"]
        assert bases > 0, (where, k)
        if not getattr(x, "_had_events", False):            # (the batch's first run with the flag: the buffer is new)
            assert _bytes_held(B, x) >= held[k] + 16 * bases, (where, k, bases)
        x._had_events = True
    assert seen == {0, 1, 2}, (where, seen)
    run(flags | B.RUN_REMAP | B.RUN_EVENTS)                 # a second run: the same bytes
    for (k, v), (rm, ev) in out.items():
        assert bs[k].events(v).tobytes() == ev, (where, k, v)
    for x in bs:
        x.set_remap(None)
    return out


def _same_bytes_for_the_same_path(a, b, where):
    """two shapes of the same reads: wherever a read's path is the same, so are its events, byte for byte"""
    n = 0
    for key in a:
        if key in b and a[key][0] == b[key][0]:
            assert a[key][1] == b[key][1], (where, key)
            n += 1
    return n


@pytest.mark.parametrize("kind,hidden,nbase,stride", [(M.NET_LSTM5, 256, 4, 5), (M.NET_GRUMOD5, 256, 5, 2)])
def test_batch_events_rows_ragged_packed(B, engine, kind, hidden, nbase, stride):
    mdl = M.synthetic_model(kind, hidden, seed=1)
    assert mdl.total_stride == stride
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(hidden + kind)
    sig = rng.standard_normal((16, 1500)).astype(np.float32)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(sig)
    rows = _check_batches(B, [b], [list(sig)], B.RUN_NO_TRACE, ("rows", kind), nbase, stride)
    b.close()
    sigs = list(sig[:4]) + [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 12)]
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    ragged = _check_batches(B, [b], [sigs], B.RUN_NO_TRACE | B.RUN_MOVES, ("ragged", kind), nbase, stride)
    b.close()
    pb = B.Batch(dm, 8, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    packed = _check_batches(B, [pb], [sigs], B.RUN_NO_TRACE, ("packed", kind), nbase, stride)
    stepwise = _check_batches(B, [pb], [sigs], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, ("packed per step", kind), nbase, stride)
    pb.close()
    dm.close()
    same = [_same_bytes_for_the_same_path(ragged, packed, "ragged / packed"), _same_bytes_for_the_same_path(packed, stepwise, "packed / per step"),
            _same_bytes_for_the_same_path({k: v for k, v in rows.items() if k[1] < 4}, ragged, "rows / ragged")]
    assert sum(same) > 0, same


def test_batch_events_paired_and_after_an_f32_rerun(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5, 384, seed=2)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(7)
    pair, sigs = [], []
    for k in range(2):
        sig = rng.standard_normal((256, 1000)).astype(np.float32)
        b = B.Batch(dm, 256, 1000)
        b.set_signals(sig)
        pair.append(b)
        sigs.append(list(sig))
    _check_batches(B, pair, sigs, B.RUN_NO_TRACE, "pair", 4, mdl.total_stride)
    for b in pair:
        b.close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their events
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[0][200] = 6.0e4                                    # (reads 0 and 5: their own calls are their sequences, so they are mapped)
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    got = _check_batches(B, [b], [sigs], 0, "rerun rows", 4, mdl.total_stride, reruns=True)
    assert b.f32_reruns() == 2 and (0, 0) in got and (0, 5) in got
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    gotp = _check_batches(B, [pb], [sigs], B.RUN_MOVES, "rerun packed", 4, mdl.total_stride, reruns=True)
    assert pb.f32_reruns() >= 2 and (0, 0) in gotp and (0, 5) in gotp
    _same_bytes_for_the_same_path(got, gotp, "rerun rows / rerun packed")
    pb.close()
    dm.close()


def test_batch_refusals_leave_the_batch_usable(B, engine):
    rng = np.random.default_rng(2)
    sig = rng.standard_normal((4, 1500)).astype(np.float32)
    seqs = [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(4)]

    def refused(what, f, *args):
        with pytest.raises(B.FFHipError) as e:
            f(*args)
        assert "ffhip error -1:" in str(e.value) and what in str(e.value), (what, str(e.value))
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    b = B.Batch(dm, 4, 1500)
    b.set_signals(sig)
    b.set_remap(seqs, 8)
    refused("FFHIP_RUN_REMAP", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_EVENTS)
    refused("FFHIP_RUN_NO_DECODE", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_NO_DECODE | B.RUN_REMAP | B.RUN_EVENTS)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_EVENTS)
    b.finish()
    for v in range(4):
        rec = b.remap(v)
        assert rec["status"] == 1
        E.check(b.events(v), E.events(sig[v], 5, rec["rm"], rec["L"]), sig[v], v)
    b.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    b = B.Batch(dm, 4, 1500)
    b.set_signals(sig)
    refused("run-length", b.run, 1.0, B.RUN_REMAP | B.RUN_EVENTS)
    refused("FFHIP_RUN_REMAP", b.run, 1.0, B.RUN_EVENTS)
    b.run(1.0, 0)
    b.finish()
    b.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_remap_events(tmp_path):
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
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=dict(env, **(extra or {})),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    trace = tmp_path / "trace.hdf5"
    default, _ = run(["--trace", str(trace)])
    lines = default.split("\n")[:-1]
    recs = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    order = [r[0][1:].split("  {")[0] for r in recs]
    calls = {r[0][1:].split("  {")[0]: r[1] for r in recs}
    assert sorted(order) == names
    # records: by read id (own call), by file name (edited call), none, a bad letter, too long
    seqs, text = {}, ""
    for i, name in enumerate(names):
        call, kind = calls[name], i % 5
        if kind == 0:
            seqs[name] = (name, call)
        elif kind == 1:
            seqs[name] = ("read_%02d" % i, call[:5] + call[9:] + "ACGT")
        elif kind == 2:
            seqs[name] = (name, call[:3] + "N" + call[3:])
        elif kind == 3:
            seqs[name] = ("read_%02d.fast5" % i, "ACGT" * len(call))
        if name in seqs:
            text += ">%s\n%s\n" % seqs[name]
    refs = tmp_path / "refs.fa"
    refs.write_text(text)
    plain_map, ev_map, events = tmp_path / "plain.tsv", tmp_path / "map.tsv", tmp_path / "events.tsv"
    assert run(["--remap", str(refs), "--remap-out", str(plain_map)])[0] == default
    stdout, err = run(["--remap", str(refs), "--remap-out", str(ev_map), "--remap-events", str(events)])
    assert stdout == default and ev_map.read_text() == plain_map.read_text()
    by_name = {}
    for line in ev_map.read_text().split("\n")[:-1]:
        f = line.split("\t")
        by_name[f[0]] = f
    want, signal_of, nreads = [], [], 0
    for name in order:                                      # reads in output order, bases in signal order
        if name not in seqs or by_name[seqs[name][0]][1] != "1":
            continue
        ref_name, q = seqs[name]
        f = by_name[ref_name]
        N, stride, trim, L = int(f[2]), int(f[3]), int(f[4]), int(f[5])
        assert L == len(q) and stride == mdl.total_stride
        x = dump_trace(trace, name)[0]
        ev = E.events(x, stride, E.rm_of_starts([int(s) for s in f[9].split(",")], N), L)
        nreads += 1
        for i in range(L):
            want.append((ref_name, i, q[i], trim + int(ev["first"][i]), int(ev["count"][i]), float(ev["mean"][i]), float(ev["sd"][i]), float(E.tolerance(x, ev[i:i + 1])[0])))
    got = events.read_text().split("\n")[:-1]
    assert len(got) == len(want) and nreads >= 8
    for g, w in zip(got, want):
        f = g.split("\t")
        assert len(f) == 7 and (f[0], int(f[1]), f[2], int(f[3]), int(f[4])) == w[:5], (g, w)
        assert abs(float(f[5]) - w[5]) <= w[7] and abs(float(f[6]) - w[6]) <= w[7], (g, w)
        assert f[5] == "%.9g" % np.float32(f[5]) and f[6] == "%.9g" % np.float32(f[6]), g      # float32 values, written so that they read back
    assert dict((k, int(v)) for k, v in re.findall(r"^events\t(\S+)\t(\d+)$", err, re.M)) == {"reads": nreads, "bases": len(want)}, err
    assert run(["--remap", str(refs), "--remap-out", str(tmp_path / "np.tsv"), "--remap-events", str(tmp_path / "np_events.tsv")], {"FLAPPIE_DEBUG": "no_pack"})[0] == default
    assert (tmp_path / "np_events.tsv").read_bytes() == events.read_bytes()
