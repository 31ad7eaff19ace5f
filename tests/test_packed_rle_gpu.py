"""Packed batches of the run-length model (include/ffhip.h "packed batches"): `runnie` on reads of any length, several to a row.

The reference `runnie` takes reads of any length one at a time (runnie.c:241-316).  The trunk of rle_r941_native is the flip-flop models' LSTM5 stack, whose
packed forms tests/test_packed_gpu.py holds; what is held here is the run-length back end on a packed batch -- partition function, subtraction, fp64 posterior
chains and their assembly, Viterbi -- per READ: every read gives, BIT FOR BIT, what the same read gives one read a row (transitions, posterior, path, score), a
sample against the oracle, the paired launch, the f32 re-run of a row with an outlier, the refusals, and the `runnie` binary on a directory of mixed lengths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
from oracle import ffo

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


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(pb, v, ub, j, post):
    # (bits, not values: this model's qpath is NaN behind the first entry -- decode_crf_runlength has none)
    return (pb.read_nblock(v) == ub.read_nblock(j) and _bits(np.float32(pb.score(v))) == _bits(np.float32(ub.score(j)))
            and np.array_equal(_bits(pb.transitions(v)), _bits(ub.transitions(j)))
            and (not post or np.array_equal(_bits(pb.posterior(v)), _bits(ub.posterior(j))))
            and np.array_equal(pb.path(v)[0], ub.path(j)[0]) and np.array_equal(_bits(pb.path(v)[1][1:]), _bits(ub.path(j)[1][1:])))


def _against_rows(B, dm, pb, sigs, order, cap, rows, temperature, flags):
    """the packed batch's reads against ragged batches of the same reads, `rows` at a time"""
    bad = []
    for k0 in range(0, len(order), rows):
        grp = order[k0:k0 + rows]
        ub = B.Batch(dm, len(grp), cap)
        ub.set_signals_ragged([sigs[i] for i in grp])
        ub.run(temperature, flags)
        ub.finish()
        bad += [grp[j] for j in range(len(grp)) if not _same(pb, k0 + j, ub, j, flags == 0)]
        ub.close()
    return bad


def _check_oracle(b, v, ref, viterbi_only):
    """tests/test_runlength.py's bounds: the parameters to 1e-4, the path bit-exact, score and posterior within their per-block bounds"""
    assert np.abs(b.transitions(v) - ref["param"]).max() <= 1e-4, v
    path, _ = b.path(v)
    assert np.array_equal(path[:-1], ref["path"]), v
    nblock = ref["param"].shape[0]
    assert abs(b.score(v) - ref["score"]) <= max(1e-4 * nblock, 1e-3 * abs(ref["score"])), v
    if not viterbi_only:
        assert np.abs(b.posterior(v) - ref["post"]).max() <= 1e-4 * nblock, v


def _packed(B, dm, rows, cap, sigs):
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan([x.size for x in sigs])
    order = [i for i in range(len(sigs)) if slot[i] >= 0]
    pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
    return pb, slot, off, order


@pytest.mark.parametrize("hidden,rows,cap", [(128, 16, 3000), (256, 32, 3000), (384, 48, 2500)])
def test_packed_runlength_reads_equal_one_read_a_row(B, engine, hidden, rows, cap):
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, hidden, seed=1)
    dm = B.DeviceModel(engine, mdl)
    assert B.lib().ffhip_model_packable(dm.h) == 1
    rng = np.random.default_rng(hidden + rows)
    # every length mod the stride, the shortest legal read (the window), reads far shorter than a row and one that fills a row
    lens = [19, 20, 21, 22, 23, 24, 45, 100, 101, 102, 103, 104, cap - 8, cap // 2, cap // 2 + 1] + [int(x) for x in np.clip(np.exp(np.log(cap / 6) + 0.9 * rng.standard_normal(3 * rows)), 30, cap - 50)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb, slot, off, order = _packed(B, dm, rows, cap, sigs)
    assert len(order) >= rows + 10 and max(np.bincount([slot[i] for i in order])) >= 3, "the plan should put several reads in a row"
    om = ffo.OracleModel(mdl)
    sample = list(range(0, 8)) + list(range(12, len(order), max(1, len(order) // 4)))
    for temperature in (1.0, 0.8):
        for flags in (0, B.RUN_VITERBI_ONLY):
            pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
            pb.run(temperature, flags)
            pb.finish()
            assert pb.nreads() == len(order) and pb.rnn_path() == 3
            assert _against_rows(B, dm, pb, sigs, order, cap, rows, temperature, flags) == []
            assert pb.basecall(0) == "" and pb.basecall(len(order) - 1) == ""      # no flip-flop strings for this model
            with pytest.raises(B.FFHipError):
                pb.trace(0)
            if temperature == 1.0:
                for v in sample:
                    _check_oracle(pb, v, om.runlength_call(sigs[order[v]], temperature=temperature, viterbi_only=flags != 0), flags != 0)
    pb.close()
    dm.close()


def test_two_packed_runlength_batches_in_a_paired_launch(B, engine):
    """the paired layer launch (k_lstm_split_pair) of two 256-row packed run-length batches at H = 384, each read as one read a row gives it"""
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 384, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(13)
    rows, cap = 256, 1500
    pbs, sets = [], []
    for k in range(2):
        lens = [int(x) for x in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(900)), 25, cap - 50)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        pb, _, _, order = _packed(B, dm, rows, cap, sigs)
        pbs.append(pb)
        sets.append((sigs, order))
    pbs[0].run_pair(pbs[1])
    for pb in pbs:
        pb.finish()
        assert pb.paired() and pb.rnn_path() == 3
    for pb, (sigs, order) in zip(pbs, sets):
        assert len(order) > 2 * rows
        assert _against_rows(B, dm, pb, sigs, order, cap, rows, 1.0, 0) == []
        pb.close()
    dm.close()


def test_outlier_in_a_packed_runlength_row_is_run_again_on_the_f32_path(B, engine):
    """a value beyond the split format in one read of a row: every read of that row goes through the f32 kernels again and comes back as the oracle's call"""
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (900, 400, 1200, 800)]
    sigs[1][200] = 6.0e4
    pb = B.Batch(dm, 16, 6000, max_reads=4)
    pb.set_signals_packed(sigs, [0, 0, 1, 0], [0, 400, 0, 800])
    pb.run()
    pb.finish()
    assert pb.f32_reruns() == 3                              # reads 0, 1 and 3 share row 0
    om = ffo.OracleModel(mdl)
    for v in range(4):
        _check_oracle(pb, v, om.runlength_call(sigs[v]), False)
    pb.close()
    dm.close()


def test_packed_runlength_refusals_and_the_query(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=3)
    dm = B.DeviceModel(engine, mdl)
    big = M.synthetic_model(M.NET_LSTM5_RLE, 384, seed=3)
    dmb = B.DeviceModel(engine, big)
    small = M.synthetic_model(M.NET_LSTM5_RLE, 64, seed=3)      # the f32 layer kernels have no packed form
    dms = B.DeviceModel(engine, small)
    assert B.lib().ffhip_model_packable(dm.h) == 1 and B.lib().ffhip_model_packable(dmb.h) == 1 and B.lib().ffhip_model_packable(dms.h) == 0
    dmb.close()
    dms.close()
    rng = np.random.default_rng(0)
    a, b2 = rng.standard_normal(500).astype(np.float32), rng.standard_normal(700).astype(np.float32)
    gap = int(B.lib().ffhip_model_pack_gap(dm.h))
    pb = B.Batch(dm, 16, 2000, max_reads=8)
    pb.set_signals_packed([a, b2], [0, 0], [0, 100 + gap])
    for temperature, flags in ((1.0, B.RUN_KEEP_ACTS), (1.0, B.RUN_F32_RNN), (0.05, 0)):      # (0.05: the fp64 chains' range ends at 0.1; no packed log-space form)
        with pytest.raises(B.FFHipError):
            pb.run(temperature, flags)
    om = ffo.OracleModel(mdl)
    # the same object one read a row again
    pb.set_signals_ragged([a] * 15 + [b2])
    pb.run()
    pb.finish()
    assert pb.nreads() == 16
    _check_oracle(pb, 5, om.runlength_call(a), False)
    _check_oracle(pb, 15, om.runlength_call(b2), False)
    pb.close()
    dm.close()


def test_runnie_packs_a_directory_of_mixed_lengths(tmp_path):
    """the `runnie` binary on single-read fast5 files of log-normal lengths: packed, one read a row (FLAPPIE_DEBUG=no_pack) and a run whose packed batch object cannot
    be created (pack_fail) give the same bytes, and every record is the oracle's"""
    from test_cli import FAST5LIB, RUNNIE, TOOL, synth_raw, write_fast5
    from test_host_layer import _f
    if not (os.path.exists(RUNNIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "runlength5_r941native.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(2)
    raws = {}
    lens = np.clip(np.exp(np.log(2500) + 1.0 * rng.standard_normal(70)), 700, 30000).astype(int)
    for i, n in enumerate(lens):
        raw = synth_raw(rng, int(n))
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, raw)
        raws["read_%02d.fast5" % i] = ("uuid-%04d" % i, raw)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path), FLAPPIE_CLI_TIMING="1")
    out = {}
    for tag, extra in (("packed", {}), ("rows", {"FLAPPIE_DEBUG": "no_pack"}), ("fallback", {"FLAPPIE_DEBUG": "pack_fail"})):
        r = subprocess.run([RUNNIE, "--batch", "16", str(reads)], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        pad = [ln for ln in r.stderr.splitlines() if ln.startswith("batches:")][-1]
        npacked = int(pad.split("(")[1].split()[0])
        if tag != "fallback":                               # (the fall-back run counts the one attempt that failed)
            assert (npacked > 0) == (tag == "packed"), pad
        assert ("packed batches are off for the rest of this run" in r.stderr) == (tag == "fallback")
        out[tag] = r.stdout
    assert out["packed"] == out["rows"] == out["fallback"]   # the same records in the same order, byte for byte
    blocks = {blk.split("\n", 1)[0]: blk for blk in out["packed"].split("# ")[1:]}
    assert sorted(blocks) == sorted(u for u, _ in raws.values())
    om = ffo.OracleModel(mdl)
    for fn in sorted(raws):
        uuid, raw = raws[fn]
        x = (raw.astype(np.float32) + np.float32(10.0)) * (np.float32(1400.0) / np.float32(8192.0))
        s, e = C.c_size_t(0), C.c_size_t(x.size)
        assert ffo.lib().fo_trim_and_segment_raw(_f(x), x.size, C.byref(s), C.byref(e), 200, 10, 100, 0.0) == 0
        y = x[s.value:e.value].copy()
        ffo.lib().fo_medmad_normalise_array(_f(y), y.size)
        ref = om.runlength_call(y)
        got = [ln.split("\t") for ln in blocks[uuid].strip().split("\n")[1:]]
        assert [g[0] for g in got] == [rec[0] for rec in ref["records"]], uuid
        assert [int(g[3]) for g in got] == [rec[3] for rec in ref["records"]], uuid
        for g, rec in zip(got, ref["records"]):
            assert abs(float(g[1]) - rec[1]) <= 2e-4 and abs(float(g[2]) - rec[2]) <= 2e-4, uuid
