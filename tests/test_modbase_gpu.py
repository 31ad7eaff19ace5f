"""flappie --modbase-tags on the GPU: 5mC probabilities made by k_mod_probs (include/ffhip.h FFHIP_RUN_MOD_PROBS, ffhip_op_mod_probs).

  * the operator on crafted posteriors: all mass on Z 255, all on C 0, equal mass 128, underflow 0; a path entry beyond the states is refused;
  * on synthetic 5-base models the device bytes equal the fp64 restatement (modbase_ref.py) on the batch's own path and posterior -- one read a row,
    packed, launch per step, paired, f32 re-run, --viterbi, temperature 0.05 -- and everything else the batch returns is bit for bit that of the same
    run without the flag;
  * the bytes agree with the --trace columns of the same run;
  * the `flappie` binary's tagged FASTQ / FASTA / SAM equal the restatement applied to its default output, packed, one read a row and after a failed
    packed batch, under --viterbi and --reverse, and its bytes equal an engine run on the signals its trace file holds."""
import os
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import modbase_ref as R

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
    """what the comparisons covered: C / Z bases, the bins their bytes fell in, and the uses of the +-1 allowance at an interval boundary"""
    def __init__(self):
        self.cz, self.bins, self.allowed = 0, set(), 0

    def check(self, got, want, raw, where):
        assert got.shape == want.shape, where
        cz = ~np.isnan(raw)
        self.cz += int(cz.sum())
        self.bins.update(int(v) for v in got[cz])
        assert np.all(got[~cz] == 0), where
        diff = got.astype(int) - want.astype(int)
        bad = diff != 0
        near = np.zeros_like(bad)
        near[cz] = np.abs(raw[cz] - np.rint(raw[cz])) < 1e-3
        assert np.all(np.abs(diff[bad]) == 1) and np.all(near[bad]), (where, np.flatnonzero(bad)[:8], raw[bad][:8], got[bad][:8], want[bad][:8])
        self.allowed += int(bad.sum())

    def final(self):
        assert self.cz >= 2000 and len(self.bins) >= 8, (self.cz, sorted(self.bins))
        assert self.allowed * 1000 <= self.cz, (self.allowed, self.cz)


def _state(b, v, trace):
    path, qpath = b.path(v)
    return dict(path=path, qpath=qpath.view(np.uint32), score=np.float32(b.score(v)).view(np.uint32), call=b.basecall(v), qual=b.quality(v),
                trace=b.trace(v) if trace else None)


def _run_both(B, b, reads, temperature, flags, tally, where, pair=None):
    """the batch (and its pair partner) without the flag, then with it: nothing else moves, and the bytes equal the restatement"""
    bs = [b] if pair is None else [b, pair[0]]
    nr = [reads] if pair is None else [reads, pair[1]]
    trace = not (flags & B.RUN_NO_TRACE)
    before = []
    for mod in (0, B.RUN_MOD_PROBS):
        if pair is None:
            b.run(temperature, flags | mod)
        else:
            b.run_pair(pair[0], temperature, flags | mod)
        for x in bs:
            x.finish()
        for k, x in enumerate(bs):
            for v in nr[k]:
                st = _state(x, v, trace)
                if not mod:
                    before.append(st)
                    continue
                old = before.pop(0)
                for key in st:
                    if key == "trace" and st[key] is None:
                        continue
                    assert np.array_equal(np.asarray(st[key]), np.asarray(old[key])) if key not in ("call", "qual") else st[key] == old[key], (where, v, key)
                got = x.mod_probs(v)
                assert len(got) == len(st["call"]), (where, v)
                want, raw = R.mod_probs(st["path"], x.posterior(v))
                assert R.basecall(st["path"], x.read_nblock(v)) == st["call"], (where, v)
                tally.check(got, want, raw, (where, v))
        if not mod:
            with pytest.raises(B.FFHipError):
                bs[0].mod_probs(nr[0][0])                 # a run without the flag made none


def test_operator_on_crafted_posteriors(B, engine):
    path = np.array([0, 1, 4, 9, 6, 2, 2], dtype=np.int32)      # called: C (1), Z (4), Z (9), C (6), G (2)
    L = np.full((7, 60), -np.inf, dtype=np.float32)
    L[0, 40:50] = -2.0                                    # all on Z: 255
    L[1, [10, 12, 51, 56]] = -1.0                          # all on C: 0
    L[2, [14, 44]] = -0.5                                  # equal mass: 128
    # L[3]: every state underflows -- 0
    L[4, :] = 0.0                                          # (block 4 is the G's: no byte)
    got = B.mod_probs_op(engine, L, path)
    assert list(got) == [255, 0, 128, 0, 0]
    rng = np.random.default_rng(2)
    for n in (1, 2, 64, 65, 1000):
        L = (rng.standard_normal((n, 60)) * 3).astype(np.float32)
        path = rng.integers(0, 10, n).astype(np.int32)
        path[rng.random(n) < 0.4] = -1
        for i in range(n):                                 # stays: the previous state
            if path[i] < 0:
                path[i] = path[i - 1] if i else 0
        want, raw = R.mod_probs(path, L)
        t = Tally()
        t.check(B.mod_probs_op(engine, L, path), want, raw, n)
    bad = np.array([0, 1, 10, 3], dtype=np.int32)
    with pytest.raises(B.FFHipError):
        B.mod_probs_op(engine, np.zeros((4, 60), np.float32), bad)
    with pytest.raises(B.FFHipError):
        B.mod_probs_op(engine, np.zeros((4, 40), np.float32), np.zeros(4, np.int32))      # a 4-base posterior


def test_engine_bytes_one_read_a_row_and_packed(B, engine):
    tally = Tally()
    # H = 48: one read a row only (ragged), default decode, --viterbi, temperature 0.05 (the log-space chains), with and without the trace
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 48, seed=3))
    rng = np.random.default_rng(48)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(400, 3000, 12)]
    b = B.Batch(dm, 12, 3000)
    b.set_signals_ragged(sigs)
    for temperature, flags in ((1.0, 0), (1.0, B.RUN_VITERBI_ONLY), (0.05, 0), (1.0, B.RUN_NO_TRACE)):
        _run_both(B, b, range(12), temperature, flags, tally, ("h48", temperature, flags))
    with pytest.raises(B.FFHipError):
        b.run(1.0, B.RUN_MOD_PROBS | B.RUN_NO_DECODE)
    b.close()
    dm.close()
    # H = 128 / 256: packed (default and launch per step, --viterbi), and one read a row
    for hidden, rows, cap in ((128, 16, 2000), (256, 32, 3000)):
        dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, hidden, seed=1))
        rng = np.random.default_rng(hidden)
        lens = [int(x) for x in np.clip(np.exp(np.log(cap / 5) + 0.9 * rng.standard_normal(3 * rows)), 30, cap - 50)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
        slot, off = pb.pack_plan(lens)
        order = [i for i in range(len(sigs)) if slot[i] >= 0]
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        for flags in (0, B.RUN_STEPWISE_RNN, B.RUN_VITERBI_ONLY):
            _run_both(B, pb, range(len(order)), 1.0, flags, tally, ("packed", hidden, flags))
        pb.close()
        b = B.Batch(dm, 16, cap)
        b.set_signals_ragged(sigs[:16])
        _run_both(B, b, range(16), 1.0, 0, tally, ("rows", hidden))
        b.close()
        dm.close()
    tally.final()


def test_engine_bytes_paired_and_after_an_f32_rerun(B, engine):
    tally = Tally()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 256, seed=2))
    rng = np.random.default_rng(7)
    rows, cap = 32, 1500
    pbs = []
    for k in range(2):
        lens = [int(x) for x in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(100)), 25, cap - 50)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
        slot, off = pb.pack_plan(lens)
        order = [i for i in range(len(sigs)) if slot[i] >= 0]
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        pbs.append((pb, range(len(order))))
    _run_both(B, pbs[0][0], pbs[0][1], 1.0, 0, tally, "pair", pair=pbs[1])
    for pb, _ in pbs:
        pb.close()
    dm.close()
    # an outlier: the row's reads come from the f32 re-run, and so do their bytes (and, under --viterbi, their posterior).  The GRUmod trunk's convolution
    # ends in tanh, so no sample takes it out of the split format's range: the LSTM trunk (swish) with the 5-base head stands in for it here
    lstm, gru = M.synthetic_model(M.NET_LSTM5, 128, seed=1), M.synthetic_model(M.NET_GRUMOD5, 128, seed=1)
    dm = B.DeviceModel(engine, M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (1900, 400, 1800, 800)]
    sigs[1][200] = 6.0e4
    pb = B.Batch(dm, 16, 4000, max_reads=4)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    for flags in (0, B.RUN_VITERBI_ONLY):
        _run_both(B, pb, range(4), 1.0, flags, tally, ("rerun", flags))
        assert pb.f32_reruns() == sum(1 for k in range(4) if slot[k] == slot[1])      # (every read of the outlier's row goes again)
    pb.close()
    b = B.Batch(dm, 4, 2000)
    b.set_signals_ragged(sigs)
    _run_both(B, b, range(4), 1.0, 0, tally, "rerun rows")
    assert b.f32_reruns() == 1
    b.close()
    dm.close()
    assert tally.cz >= 1000 and tally.allowed * 1000 <= tally.cz


def test_bytes_agree_with_the_trace_and_other_models_refuse(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 128, seed=5))
    rng = np.random.default_rng(11)
    b = B.Batch(dm, 8, 2500)
    b.set_signals(rng.standard_normal((8, 2500)).astype(np.float32))
    b.run(1.0, B.RUN_MOD_PROBS)
    b.finish()
    n = 0
    for v in range(8):
        path, _ = b.path(v)
        tr = b.trace(v).astype(np.float64) / 255.0         # column pos: occupancy of block pos - 1, scaled by 255 and rounded
        got = b.mod_probs(v)
        for k, pos in enumerate(R.called(path, b.read_nblock(v))):
            if int(path[pos]) % 5 not in (1, 4):
                continue
            c, z = tr[pos, 1] + tr[pos, 6], tr[pos, 4] + tr[pos, 9]
            if c + z < 0.25:
                continue                                   # (the trace's rounding, 1/255 an entry, moves p by up to (1/255) / (c + z))
            p = z / (c + z)
            lo, hi = int(got[k]) / 256.0, (int(got[k]) + 1) / 256.0
            assert lo - 4 / 255 <= p <= hi + 4 / 255, (v, pos, p, got[k])
            n += 1
    assert n >= 50
    b.close()
    dm.close()
    for kind in (M.NET_LSTM5, M.NET_LSTM5_RLE):
        dm = B.DeviceModel(engine, M.synthetic_model(kind, 128, seed=1))
        b = B.Batch(dm, 4, 1000)
        b.set_signals(np.random.default_rng(0).standard_normal((4, 1000)).astype(np.float32))
        with pytest.raises(B.FFHipError):
            b.run(1.0, B.RUN_MOD_PROBS)
        b.run()
        b.finish()
        with pytest.raises(B.FFHipError):
            b.mod_probs(0)
        b.close()
        dm.close()


# ------------------------------------------------------------------------------------ the binary
def _split_records(text, step):
    lines = text.split("\n")[:-1]
    return [lines[k:k + step] for k in range(0, len(lines), step)]


def _expect(default, tagged, fmt):
    """the tagged output from the default one and the tagged output's own bytes, record by record; returns {name: (SEQ, bytes)}"""
    step = {"fastq": 4, "fasta": 2, "sam": 2}[fmt]
    d, t = _split_records(default, step), _split_records(tagged, 1 if fmt == "sam" else step)      # (tagged SAM: one line a read)
    assert len(t) == len(d), fmt
    out = {}
    for dr, tr in zip(d, t):
        if fmt == "sam":
            f = dr[0].split("\t")
            assert len(f) == 11
            name, call, qual = f[0], f[9], f[10]
            tf = tr[0].split("\t")
            assert len(tf) == 13 and tf[:9] == f[:9]
            ml = R.ml_values(tf[12])
            seq = tf[9]
            want = R.tagged_sam(name, call, qual, R.spread_ml(seq, ml))
            got = tr[0] + "\n"
            assert dr[1] == call + "\t" + qual                # (the default record's second line: the reference's repeated sequence / quality)
        else:
            hdr, call = dr[0][1:], dr[1]
            tags = tr[0].split("\t")
            ml = R.ml_values(tags[-1])
            seq = tr[1]
            if fmt == "fastq":
                want = R.tagged_fastq(hdr, call, dr[3], R.spread_ml(seq, ml))
                got = "\n".join(tr) + "\n"
            else:
                want = R.tagged_fasta(hdr, call, R.spread_ml(seq, ml))
                got = "\n".join(tr) + "\n"
            name = hdr.split("  {")[0]
        assert got == want, (fmt, name)
        assert len(ml) == seq.count("C") and seq == R.seq_of(call)
        out[name] = (seq, R.spread_ml(seq, ml))
    return out


def test_flappie_modbase_tags(B, engine, tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC")
    M.write_mdl(str(tmp_path / "flipflop_r941native5mC.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    lens = np.clip(np.exp(np.log(2500) + 1.0 * rng.standard_normal(60)), 700, 30000).astype(int)
    for i, n in enumerate(lens):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    (reads / "read_30b.fast5").write_bytes(b"not an HDF5 file")
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, extra=None):
        r = subprocess.run([FLAPPIE, "--model", "r941_5mC", "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout

    trace = tmp_path / "trace.hdf5"
    seen = None
    for fmt in ("fastq", "fasta", "sam"):
        default = run(["--format", fmt])
        tagged = run(["--format", fmt, "--modbase-tags"] + (["--trace", str(trace)] if fmt == "fastq" else []))
        got = _expect(default, tagged, fmt)
        assert len(got) == 60
        if seen is None:
            seen = got
        assert got == seen, fmt
        if fmt == "fastq":
            for extra in ({"FLAPPIE_DEBUG": "no_pack"}, {"FLAPPIE_DEBUG": "pack_fail"}):
                assert run(["--format", fmt, "--modbase-tags"], extra) == tagged, extra
            assert run(["--format", fmt]) == default
            # --reverse: the same records, each reversed with its bytes
            rev = _expect(run(["--format", fmt, "--reverse"]), run(["--format", fmt, "--reverse", "--modbase-tags"]), fmt)
            for name, (seq, ml) in rev.items():
                assert seq == seen[name][0][::-1] and ml == seen[name][1][::-1], name
            # --viterbi: its own default output, tagged the same way (the bytes from the posterior)
            _expect(run(["--format", fmt, "--viterbi"]), run(["--format", fmt, "--viterbi", "--modbase-tags"]), fmt)
    # the trace file is that of a run without the option, and the bytes are the engine's on the signals it holds
    plain = tmp_path / "plain.hdf5"
    run(["--trace", str(plain)])
    dm = B.DeviceModel(engine, mdl)
    names = sorted(seen)
    sigs, traces = [], []
    for name in names:
        sig, tr = dump_trace(trace, name)
        sig0, tr0 = dump_trace(plain, name)
        assert np.array_equal(sig, sig0) and np.array_equal(tr, tr0), name
        sigs.append(sig)
    tally = Tally()
    b = B.Batch(dm, len(sigs), max(s.size for s in sigs))
    b.set_signals_ragged(sigs)
    b.run(1.0, B.RUN_MOD_PROBS)
    b.finish()
    for v, name in enumerate(names):
        path, _ = b.path(v)
        want, raw = R.mod_probs(path, b.posterior(v))
        assert R.seq_of(b.basecall(v)) == seen[name][0], name
        tally.check(np.array(seen[name][1], dtype=np.uint8), want, raw, name)
    assert tally.cz >= 1000
    b.close()
    dm.close()
