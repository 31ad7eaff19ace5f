"""flappie --emit-moves on the GPU: the move table made by k_moves (include/ffhip.h FFHIP_RUN_MOVES, ffhip_batch_moves, ffhip_op_moves).

  * the operator on crafted paths (1, 2, 3, 64, 65, 1000 blocks, all-stay and all-change among them; lengths that are no multiple of the kernel's four blocks a
    lane) equals the restatement (moves_ref.py); the refusals;
  * on synthetic 8-state (H = 256, 384) and 10-state models the device moves equal the restatement on the batch's own path -- one read a row, ragged, packed,
    launch per step, paired, f32 re-run, --viterbi, temperature 0.05, with and without the 5mC bytes -- their ones number the call's length, the call re-read
    through them is the call, and everything else the batch returns is bit for bit that of the same run without the flag;
  * a finished run with the flag makes as many device-to-host copy calls as one without;
  * the `flappie` binary's tagged FASTQ / FASTA / SAM equal the restatement applied to its default output and an engine run on the signals its trace file holds.
Everything is integer- or byte-exact: no tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import modbase_ref as MR
import moves_ref as R

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


class Tally:
    """what the comparisons covered: reads, called bases, reads whose first block has a move and reads whose first block has none"""
    def __init__(self):
        self.reads = self.bases = self.b0_zero = self.b0_later = 0

    def add(self, mv):
        self.reads += 1
        self.bases += int(mv.sum())
        b0 = R.first_move(mv)
        self.b0_zero += int(b0 == 0)
        self.b0_later += int(b0 is not None and b0 > 0)


def _state(B, b, v, flags):
    path, qpath = b.path(v)
    st = dict(path=path, qpath=qpath.view(np.uint32), score=np.float32(b.score(v)).view(np.uint32), call=b.basecall(v), qual=b.quality(v))
    if not (flags & B.RUN_NO_TRACE):
        st["trace"] = b.trace(v)
    if flags & B.RUN_MOD_PROBS:
        st["ml"] = b.mod_probs(v)
    return st


def _run_both(B, b, reads, temperature, flags, tally, where, pair=None):
    """the batch (and its pair partner) without the flag, then with it: nothing else moves, and the moves equal the restatement on the batch's own path"""
    bs = [b] if pair is None else [b, pair[0]]
    nr = [reads] if pair is None else [reads, pair[1]]
    nbase = b.nstate // 2
    before = []
    for mvf in (0, B.RUN_MOVES):
        if pair is None:
            b.run(temperature, flags | mvf)
        else:
            b.run_pair(pair[0], temperature, flags | mvf)
        for x in bs:
            x.finish()
        for k, x in enumerate(bs):
            for v in nr[k]:
                st = _state(B, x, v, flags)
                if not mvf:
                    before.append(st)
                    continue
                old = before.pop(0)
                for key in st:
                    assert st[key] == old[key] if key in ("call", "qual") else np.array_equal(np.asarray(st[key]), np.asarray(old[key])), (where, v, key)
                got = x.moves(v)
                assert got.dtype == np.uint8 and got.size == x.read_nblock(v), (where, v)
                assert np.array_equal(got, R.moves(st["path"])), (where, v, np.flatnonzero(got != R.moves(st["path"]))[:8])
                assert int(got.sum()) == len(st["call"]), (where, v)
                assert R.call_through_moves(st["path"], got, nbase) == st["call"], (where, v)
                tally.add(got)
        if not mvf:
            with pytest.raises(B.FFHipError):
                bs[0].moves(nr[0][0])                     # a run without the flag made none


def _packed_batch(B, dm, rows, cap, nreads, rng, mean):
    """a packed batch of reads of mixed lengths: the reads stand at whatever block offsets the plan gives them (odd ones among them)"""
    lens = [int(x) for x in np.clip(np.exp(np.log(mean) + 0.8 * rng.standard_normal(nreads)), 25, cap - 50)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    order = [i for i in range(len(sigs)) if slot[i] >= 0]
    pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
    assert any(off[i] % 4 for i in order), "no read at a block offset that is not a multiple of four"
    return pb, len(order)


def crafted_paths(nstate):
    rng = np.random.default_rng(5)
    out = []
    for nblock in (1, 2, 3, 4, 5, 7, 64, 65, 1000, 1023, 1024, 1025, 4099):
        out.append(np.full(nblock + 1, 3, dtype=np.int32))
        out.append((np.arange(nblock + 1) % nstate).astype(np.int32))
        for frac in (0.2, 0.5, 0.9):
            p = rng.integers(0, nstate, nblock + 1).astype(np.int32)
            stay = rng.random(nblock + 1) < frac
            for i in range(1, nblock + 1):
                if stay[i]:
                    p[i] = p[i - 1]
            out.append(p)
    return out


def test_operator_on_crafted_paths_and_refusals(B, engine):
    n = 0
    for nstate in (8, 10):
        for path in crafted_paths(nstate):
            got = B.moves_op(engine, path)
            want = R.moves(path)
            assert got.size == path.size - 1 and np.array_equal(got, want), (path.size, np.flatnonzero(got != want)[:8])
            assert got[-1] == 0
            n += int(got.sum())
    assert n >= 5000
    assert list(B.moves_op(engine, np.array([0, 1], np.int32))) == [0]
    assert list(B.moves_op(engine, np.array([0, 0, 2, 2, 3], np.int32))) == [0, 1, 0, 0]
    one, out = np.zeros(1, np.int32), np.zeros(1, np.uint8)      # no block at all
    assert B.lib().ffhip_op_moves(engine.h, one.ctypes.data_as(C.POINTER(C.c_int)), 0, out.ctypes.data_as(C.POINTER(C.c_uint8))) != 0
    sig = np.random.default_rng(0).standard_normal((4, 1000)).astype(np.float32)
    # the run-length model has no move table
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1))
    b = B.Batch(dm, 4, 1000)
    b.set_signals(sig)
    with pytest.raises(B.FFHipError):
        b.run(1.0, B.RUN_MOVES)
    b.close()
    dm.close()
    # nor has a run that is not decoded; and a run without the flag made none
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1)
    dm = B.DeviceModel(engine, mdl)
    assert dm.stride == mdl.total_stride == 5
    b = B.Batch(dm, 4, 1000)
    b.set_signals(sig)
    with pytest.raises(B.FFHipError):
        b.run(1.0, B.RUN_MOVES | B.RUN_NO_DECODE)
    b.run()
    b.finish()
    with pytest.raises(B.FFHipError):
        b.moves(0)
    b.run(1.0, B.RUN_MOVES)
    b.finish()
    assert b.moves(0).size == b.read_nblock(0)
    b.run()
    b.finish()
    with pytest.raises(B.FFHipError):                      # (the flag of an earlier run does not carry over)
        b.moves(0)
    b.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 128, seed=1))
    assert dm.stride == 2
    dm.close()


def test_engine_moves_on_every_run_form(B, engine):
    tally = Tally()
    # one read a row (ragged; reads of a few blocks among them), default decode, --viterbi, temperature 0.05, with and without the trace
    for kind, hidden in ((M.NET_LSTM5, 48), (M.NET_GRUMOD5, 48)):
        dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=3))
        rng = np.random.default_rng(hidden + kind)
        lens = [30, 31, 33] + [int(n) for n in rng.integers(400, 3000, 13)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        b = B.Batch(dm, 16, 3000)
        b.set_signals_ragged(sigs)
        for temperature, flags in ((1.0, 0), (1.0, B.RUN_VITERBI_ONLY), (0.05, 0), (1.0, B.RUN_NO_TRACE)):
            _run_both(B, b, range(16), temperature, flags, tally, ("rows", kind, temperature, flags))
            if kind == M.NET_GRUMOD5:
                _run_both(B, b, range(16), temperature, flags | B.RUN_MOD_PROBS, tally, ("rows + ml", temperature, flags))
        b.close()
        dm.close()
    # packed (default, launch per step, --viterbi) and one read a row: 8 states at H = 256 and 384, 10 states at H = 256 with and without the 5mC bytes
    for kind, hidden, rows, cap, nreads in ((M.NET_LSTM5, 256, 64, 3000, 660), (M.NET_LSTM5, 384, 64, 3000, 660), (M.NET_GRUMOD5, 256, 64, 1500, 800)):
        dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
        rng = np.random.default_rng(hidden)
        pb, n = _packed_batch(B, dm, rows, cap, nreads, rng, cap / 12)
        for flags in (0, B.RUN_STEPWISE_RNN, B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE):
            _run_both(B, pb, range(n), 1.0, flags, tally, ("packed", kind, hidden, flags))
        if kind == M.NET_GRUMOD5:
            # moves first, then moves and 5mC bytes (the 5mC section arrives in front of the moves'), then 5mC alone, then moves alone again
            _run_both(B, pb, range(n), 1.0, B.RUN_MOD_PROBS, tally, ("packed + ml", hidden))
            _run_both(B, pb, range(n), 1.0, B.RUN_MOD_PROBS | B.RUN_STEPWISE_RNN, tally, ("packed + ml, per step", hidden))
            _run_both(B, pb, range(n), 1.0, 0, tally, ("packed again", hidden))
        pb.close()
        sigs = [rng.standard_normal(int(k)).astype(np.float32) for k in rng.integers(300, cap, 16)]
        b = B.Batch(dm, 16, cap)
        b.set_signals_ragged(sigs)
        _run_both(B, b, range(16), 1.0, 0, tally, ("rows", kind, hidden))
        b.close()
        dm.close()
    assert tally.reads >= 2000 and tally.bases >= 2000, (tally.reads, tally.bases)
    assert tally.b0_zero > 0 and tally.b0_later > 0, (tally.b0_zero, tally.b0_later)


def test_engine_moves_paired_and_after_an_f32_rerun(B, engine):
    tally = Tally()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 256, seed=2))
    rng = np.random.default_rng(7)
    pbs = []
    for k in range(2):
        pb, n = _packed_batch(B, dm, 32, 1500, 100, rng, 300)
        pbs.append((pb, range(n)))
    _run_both(B, pbs[0][0], pbs[0][1], 1.0, 0, tally, "pair", pair=pbs[1])
    for pb, _ in pbs:
        pb.close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their moves; 8 states, and 10 states with the 5mC bytes (the LSTM trunk with the
    # 5-base head: the GRUmod trunk's convolution ends in tanh, so no sample takes it out of the split format's range)
    lstm, gru = M.synthetic_model(M.NET_LSTM5, 128, seed=1), M.synthetic_model(M.NET_GRUMOD5, 128, seed=1)
    for mdl, extra in ((lstm, 0), (M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b), B.RUN_MOD_PROBS)):
        dm = B.DeviceModel(engine, mdl)
        rng = np.random.default_rng(4)
        sigs = [rng.standard_normal(n).astype(np.float32) for n in (1900, 400, 1800, 800)]
        sigs[1][200] = 6.0e4
        pb = B.Batch(dm, 16, 4000, max_reads=4)
        slot, off = pb.pack_plan([x.size for x in sigs])
        assert min(slot) >= 0
        pb.set_signals_packed(sigs, slot, off)
        for flags in (extra, extra | B.RUN_VITERBI_ONLY):
            _run_both(B, pb, range(4), 1.0, flags, tally, ("rerun", flags))
            assert pb.f32_reruns() == sum(1 for k in range(4) if slot[k] == slot[1])      # (every read of the outlier's row goes again)
        pb.close()
        b = B.Batch(dm, 4, 2000)
        b.set_signals_ragged(sigs)
        _run_both(B, b, range(4), 1.0, extra, tally, "rerun rows")
        assert b.f32_reruns() == 1
        # the whole batch forced onto the f32 kernels
        _run_both(B, b, range(4), 1.0, extra | B.RUN_F32_RNN, tally, "f32")
        b.close()
        dm.close()
    assert tally.reads >= 100 and tally.bases >= 2000, (tally.reads, tally.bases)


def _d2h_calls(B):
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, 1)
    return int(c[2]), int(c[3])


def test_no_extra_copy_call(B, engine):
    for kind, extra in ((M.NET_LSTM5, 0), (M.NET_GRUMOD5, 0), (M.NET_GRUMOD5, B.RUN_MOD_PROBS)):
        dm = B.DeviceModel(engine, M.synthetic_model(kind, 128, seed=1))
        rng = np.random.default_rng(1)
        b = B.Batch(dm, 8, 2000)
        b.set_signals(rng.standard_normal((8, 2000)).astype(np.float32))
        pb, n = _packed_batch(B, dm, 16, 2000, 60, rng, 300)
        for x in (b, pb):
            calls = {}
            for mvf in (B.RUN_MOVES, 0, B.RUN_MOVES):          # (the first run grows the result block; the counts are taken from the later two)
                _d2h_calls(B)
                x.run(1.0, extra | B.RUN_NO_TRACE | mvf)
                x.finish()
                calls[mvf] = _d2h_calls(B)
            assert calls[B.RUN_MOVES][0] == calls[0][0] >= 1, (kind, extra, calls)
            assert calls[B.RUN_MOVES][1] > calls[0][1], (kind, extra, calls)      # ... and that one copy carries the section
            assert x.moves(0).size == x.read_nblock(0)
        b.close()
        pb.close()
        dm.close()


# ------------------------------------------------------------------------------------ the binary
def _split_records(text, step):
    lines = text.split("\n")[:-1]
    return [lines[k:k + step] for k in range(0, len(lines), step)]


_HDR = re.compile(r'"nsample" : (\d+), "trim" : \[ (\d+), (\d+) \]')


def _tag(fields, key):
    hit = [f for f in fields if f.startswith(key)]
    assert len(hit) <= 1, (key, fields[:12])
    return hit[0][len(key):] if hit else None


def _check_output(default, tagged, fmt, moves_of, info, delta, stride, ml_of=None):
    """the tagged output against the restatement applied to the default output, record by record.  moves_of: name -> the engine's moves; info: name -> (n, start,
    end), filled from FASTQ / FASTA headers and read for SAM; ml_of: name -> the ML bytes of every base (records with MM / ML as well).  Returns name -> (sm, sd)."""
    step = {"fastq": 4, "fasta": 2, "sam": 2}[fmt]
    d, t = _split_records(default, step), _split_records(tagged, 1 if fmt == "sam" else step)
    assert len(t) == len(d) > 0, fmt
    stats = {}
    for dr, tr in zip(d, t):
        fields = tr[0].split("\t")
        if fmt == "sam":
            f = dr[0].split("\t")
            assert len(f) == 11 and dr[1] == f[9] + "\t" + f[10]
            name, call, qual = f[0], f[9], f[10]
        else:
            hdr, call = dr[0][1:], dr[1]
            qual = dr[3] if fmt == "fastq" else None
            name = hdr.split("  {")[0]
            m = _HDR.search(hdr)
            info[name] = (int(m.group(1)), int(m.group(2)), int(m.group(3)))
        n, start, end = info[name]
        mv = moves_of[name]
        sm, sd = _tag(fields, "sm:f:"), _tag(fields, "sd:f:")
        assert (sm is None) == (sd is None) == bool(delta), name
        assert (_tag(fields, "sv:Z:") is None) == bool(delta)
        med, mad = (np.float32(0), np.float32(1)) if delta else (np.float32(sm), np.float32(sd))
        if not delta:
            assert sm == "%.9g" % float(med) and sd == "%.9g" % float(mad)
            stats[name] = (med, mad)
        qs = _tag(fields, "qs:f:")
        if qual is None:                                   # FASTA shows no qualities: the qs tag is held to the FASTQ record's (info keeps it)
            q = info[(name, "qual")]
        else:
            q = info[(name, "qual")] = qual
        assert qs == ("%.3f" % R.mean_quality(q) if q else None), name
        ml = None if ml_of is None else ml_of[name]
        args = (call, q, mv, stride, n, start, med, mad, delta, ml)
        if fmt == "fastq":
            want, got = R.tagged_fastq(hdr, *args), "\n".join(tr) + "\n"
        elif fmt == "fasta":
            want, got = R.tagged_fasta(hdr, *args), "\n".join(tr) + "\n"
        else:
            want, got = R.tagged_sam(name, *args), tr[0] + "\n"
            assert len(fields) == 11 + 4 - (0 if q else 1) + (0 if delta else 3) + (0 if ml is None else 2), name
        assert got == want, (fmt, name)
        assert int(_tag(fields, "ns:i:")) == n
        ts = int(_tag(fields, "ts:i:"))
        got_stride, kept = R.parse_mv(fields[-1])
        assert got_stride == stride
        if kept:
            assert kept[0] == 1 and kept[-1] == 0 and sum(kept) == len(call), name
            assert end <= ts + stride * len(kept) < end + stride, (name, ts, len(kept), end)      # the table reaches the end of the trimmed signal
        else:
            assert ts == start and call == ""
    return stats


def test_flappie_emit_moves(B, engine, tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    lstm = M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), lstm)
    gru = M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC")
    M.write_mdl(str(tmp_path / "flipflop_r941native5mC.h"), gru)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    lens = np.clip(np.exp(np.log(2500) + 1.0 * rng.standard_normal(40)), 1500, 30000).astype(int)
    pa = {}
    for i, n in enumerate(lens):
        raw = synth_raw(rng, int(n))
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, raw)
        pa["uuid-%04d" % i] = (raw.astype(np.float32) + np.float32(10.0)) * (np.float32(1400.0) / np.float32(8192.0))      # (fast5_interface.c:289-291)
    (reads / "read_30b.fast5").write_bytes(b"not an HDF5 file")
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(model, args, extra=None):
        r = subprocess.run([FLAPPIE, "--model", model, "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout

    def engine_moves(mdl, trace, names, flags):
        """the engine's moves (and calls) on the signals the trace file holds"""
        dm = B.DeviceModel(engine, mdl)
        sigs = [dump_trace(trace, name)[0] for name in names]
        b = B.Batch(dm, len(sigs), max(s.size for s in sigs))
        b.set_signals_ragged(sigs)
        b.run(1.0, B.RUN_MOVES | flags)
        b.finish()
        out = {name: (b.moves(v), b.basecall(v), sigs[v]) for v, name in enumerate(names)}
        b.close()
        dm.close()
        return out

    names = sorted(pa)
    k = 0

    def variant(model, mdl, opts, engine_flags=0, delta=False, reverse=False, fmts=("fastq",), debug=()):
        nonlocal k
        k += 1
        trace = tmp_path / ("trace%d.hdf5" % k)
        info, stats = {}, {}
        eng_out = None
        for fmt in fmts:
            default = run(model, opts + ["--format", fmt])
            tagged = run(model, opts + ["--format", fmt, "--emit-moves"] + (["--trace", str(trace)] if eng_out is None else []))
            if eng_out is None:
                eng_out = engine_moves(mdl, trace, names, engine_flags)
                moves_of = {name: eng_out[name][0] for name in names}
            stats = _check_output(default, tagged, fmt, moves_of, info, delta, mdl.total_stride) or stats
            if fmt == "fastq":
                for dbg in debug:
                    assert run(model, opts + ["--format", fmt, "--emit-moves"], {"FLAPPIE_DEBUG": dbg}) == tagged, dbg
                assert run(model, opts + ["--format", fmt]) == default
                calls = {r[0][1:].split("  {")[0]: r[1] for r in _split_records(default, 4)}
                for name in names:                         # the engine run is the binary's run: the same call (reversed under --reverse)
                    assert calls[name] == (eng_out[name][1][::-1] if reverse else eng_out[name][1]), name
        for name in names:
            n, start, end = info[name]
            assert n == pa[name].size, name
            if not delta:                                  # (pA - sm) / sd in float IS the signal the network saw
                med, mad = stats[name]
                sig = (pa[name][start:end] - med) / mad
                assert sig.dtype == np.float32 and np.array_equal(sig.view(np.uint32), eng_out[name][2].view(np.uint32)), name
        return trace

    t0 = variant("r941_native", lstm, [], fmts=("fastq", "fasta", "sam"), debug=("no_pack", "pack_fail"))
    variant("r941_native", lstm, ["--viterbi"], engine_flags=B.RUN_VITERBI_ONLY)
    variant("r941_native", lstm, ["--reverse"], reverse=True)
    variant("r941_native", lstm, ["--trim", "350:40"])
    variant("r941_native", lstm, ["--delta", "1.0"], delta=True)
    # the trace file is that of a run without the option
    plain = tmp_path / "plain.hdf5"
    run("r941_native", ["--trace", str(plain)])
    for name in names:
        a, b = dump_trace(t0, name), dump_trace(plain, name)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), name
    # the 5mC model (stride 2), alone and together with --modbase-tags: the MM / ML tags of --modbase-tags alone, then these
    variant("r941_5mC", gru, [], fmts=("fastq", "sam"), debug=("no_pack",))
    only = run("r941_5mC", ["--format", "fastq", "--modbase-tags"])
    trace = tmp_path / "both.hdf5"
    both = run("r941_5mC", ["--format", "fastq", "--modbase-tags", "--emit-moves", "--trace", str(trace)])
    default = run("r941_5mC", ["--format", "fastq"])
    eng_out = engine_moves(gru, trace, names, B.RUN_MOD_PROBS)
    ml_of = {}
    for rec in _split_records(only, 4):
        f = rec[0].split("\t")
        ml_of[f[0][1:].split("  {")[0]] = MR.spread_ml(rec[1], MR.ml_values(f[-1]))
    _check_output(default, both, "fastq", {name: eng_out[name][0] for name in names}, {}, False, 2, ml_of=ml_of)
    for ro, rb in zip(_split_records(only, 4), _split_records(both, 4)):
        assert rb[0].startswith(ro[0] + "\t") and rb[1:] == ro[1:]
    assert run("r941_5mC", ["--format", "fastq", "--modbase-tags", "--emit-moves"], {"FLAPPIE_DEBUG": "no_pack"}) == both
    assert run("r941_5mC", ["--format", "fastq", "--modbase-tags"]) == only
    # --reverse with both: SEQ, QUAL and ML reversed, mv not
    rev = run("r941_5mC", ["--format", "fastq", "--modbase-tags", "--emit-moves", "--reverse"])
    for rf, rr in zip(_split_records(both, 4), _split_records(rev, 4)):
        ff, fr = rf[0].split("\t"), rr[0].split("\t")
        assert rr[1] == rf[1][::-1] and rr[3] == rf[3][::-1]
        assert MR.ml_values(_tag_full(fr, "ML:B:C")) == MR.ml_values(_tag_full(ff, "ML:B:C"))[::-1]
        assert fr[-1] == ff[-1] and _tag(fr, "ts:i:") == _tag(ff, "ts:i:")


def _tag_full(fields, key):
    hit = [f for f in fields if f.startswith(key)]
    assert len(hit) == 1
    return hit[0]
