"""runnie --fasta on the GPU: run records and run-length estimates made by k_rle_runs (include/ffhip.h FFHIP_RUN_RLE_RUNS / _RECORDS, ffhip_op_rle_runs).

  * the operator entry on crafted matrices that carry the golden fixture's fp32 scales gives, expanded on the host, the reference script's FASTA bytes;
  * on synthetic run-length models the device runs equal the restatement of runnie.c:282-313 on the batch's own path and posterior (transitions under
    --viterbi), read for read, shape and scale bit for bit -- one read a row, packed, paired, f32 re-run, --viterbi, temperature 0.05, launch per step;
  * the `runnie` binary's --fasta output equals decode_runnie.py's restatement applied to its own .run output of the same files, byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import runnie_fasta_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_operator_on_the_golden_records_gives_the_reference_bytes(B, engine):
    with open(os.path.join(GOLD, "runnie_fasta_records.json")) as fh:
        doc = json.load(fh)
    rng = np.random.default_rng(5)
    mats = []
    for r in doc["reads"]:
        lead = 3                                          # blocks in front of the first run: stay states, counted for nothing
        nblock = lead + sum(x[3] for x in r["runs"]) + (0 if r["runs"] else 2)
        mat = rng.standard_normal((nblock, 40)).astype(np.float32)
        path = np.full(nblock, 4 + 2, dtype=np.int32)
        p = lead
        for b, shb, scb, d in r["runs"]:
            path[p] = b
            path[p + 1:p + d] = 4 + b
            mat[p, b] = np.uint32(shb).view(np.float32)
            mat[p, 4 + b] = np.uint32(scb).view(np.float32)
            p += d
        mats.append((r, mat, path))
    for mode in ("default", "rlc", "scale"):
        f = doc["factors"][mode]
        out, err = [], []
        for r, mat, path in mats:
            got = B.rle_runs_op(engine, mat, path, None if mode == "default" else f)
            assert len(got["base"]) == len(r["runs"]) and not got["failed"]
            assert [int(x) for x in got["base"]] == [x[0] for x in r["runs"]]
            assert [int(x) for x in got["dwell"]] == [x[3] for x in r["runs"]]
            assert list(_bits(got["shape"])) == [x[1] for x in r["runs"]] and list(_bits(got["scale"])) == [x[2] for x in r["runs"]]
            assert got["length"] == int(got["est"].sum())
            rec = R.fasta_record(r["name"], got["base"], got["est"], rlc=(mode == "rlc"))
            if rec is None:
                err.append("No basecall returned for %s\n" % r["name"])
            else:
                out.append(rec)
        with open(os.path.join(GOLD, "runnie_fasta_%s.fa" % mode)) as fh:
            assert "".join(out) == fh.read()
        with open(os.path.join(GOLD, "runnie_fasta_%s.err" % mode)) as fh:
            assert "".join(err) == fh.read()
    # a failed estimate and a non-finite scale flag the read; crafted path entries beyond the states are refused
    mat = np.ones((4, 40), dtype=np.float32)
    mat[1, 4 + 2] = 3.0e9
    got = B.rle_runs_op(engine, mat, np.array([0, 2, 6, 6], dtype=np.int32))
    assert got["failed"] and len(got["base"]) == 2
    mat[1, 4 + 2] = np.inf
    assert B.rle_runs_op(engine, mat, np.array([0, 2, 6, 6], dtype=np.int32))["failed"]
    with pytest.raises(B.FFHipError):
        B.rle_runs_op(engine, mat, np.array([0, 8, 6, 6], dtype=np.int32))


def _check_reads(b, reads, viterbi, factors=R.DEFAULT, records=True):
    for v in reads:
        path = b.path(v)[0]
        mat = b.transitions(v) if viterbi else b.posterior(v)
        want = R.records(path, mat)
        got = b.rle_runs(v)
        assert [int(x) for x in got["base"]] == [w[0] for w in want], v
        est, bad = R.estimate([w[0] for w in want], [w[2] for w in want], factors)
        assert list(got["est"]) == list(est) and got["failed"] == bad and got["length"] == int(est.sum()), v
        if records:
            assert list(got["dwell"]) == [w[3] for w in want], v
            assert np.array_equal(_bits(got["shape"]), _bits([w[1] for w in want])), v
            assert np.array_equal(_bits(got["scale"]), _bits([w[2] for w in want])), v
        else:
            assert got["shape"] is None and got["dwell"] is None


@pytest.mark.parametrize("hidden", [128, 384])
def test_engine_runs_equal_the_host_loop(B, engine, hidden):
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, hidden, seed=2)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(hidden)
    # one read a row, ragged: both flags, --viterbi, temperature 0.05 (the log-space k_rle_transpost), other factors
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(300, 2500, 16)]
    b = B.Batch(dm, 16, 2500)
    b.set_signals_ragged(sigs)
    with pytest.raises(B.FFHipError):
        b.rle_runs(0)                                     # (never ran)
    for temperature, flags, factors in ((1.0, B.RUN_RLE_RECORDS, None), (1.0, B.RUN_RLE_RUNS, (1.1, 0.95, 1.3, 1.07)),
                                        (1.0, B.RUN_RLE_RECORDS | B.RUN_VITERBI_ONLY, None), (0.05, B.RUN_RLE_RECORDS, None)):
        if factors:
            b.set_run_scale(factors)
        b.run(temperature, flags)
        b.finish()
        _check_reads(b, range(16), flags & B.RUN_VITERBI_ONLY, factors or R.DEFAULT, flags & B.RUN_RLE_RECORDS)
        if factors:
            b.set_run_scale(R.DEFAULT)
    b.run(1.0, 0)
    b.finish()
    with pytest.raises(B.FFHipError):
        b.rle_runs(0)                                     # a run without the flag made none
    b.close()
    # packed, with the launch-per-step kernels as well
    lens = [int(x) for x in np.clip(np.exp(np.log(600) + 0.9 * rng.standard_normal(70)), 30, 2900)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, 16, 3000, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    order = [i for i in range(len(sigs)) if slot[i] >= 0]
    for flags in (B.RUN_RLE_RECORDS, B.RUN_RLE_RECORDS | B.RUN_STEPWISE_RNN, B.RUN_RLE_RUNS | B.RUN_VITERBI_ONLY):
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        pb.run(1.0, flags)
        pb.finish()
        _check_reads(pb, range(len(order)), flags & B.RUN_VITERBI_ONLY, records=flags & B.RUN_RLE_RECORDS)
    pb.close()
    dm.close()


def test_engine_runs_paired_and_after_an_f32_rerun(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 384, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(13)
    rows, cap = 256, 1500
    pbs = []
    for k in range(2):
        lens = [int(x) for x in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(600)), 25, cap - 50)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
        slot, off = pb.pack_plan(lens)
        order = [i for i in range(len(sigs)) if slot[i] >= 0]
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        pbs.append((pb, len(order)))
    pbs[0][0].run_pair(pbs[1][0], 1.0, B.RUN_RLE_RECORDS)
    for pb, n in pbs:
        pb.finish()
        assert pb.paired()
        _check_reads(pb, range(0, n, 7), False)
        pb.close()
    dm.close()
    # an outlier: the row's reads come from the f32 re-run, and so do their runs
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (900, 400, 1200, 800)]
    sigs[1][200] = 6.0e4
    pb = B.Batch(dm, 16, 6000, max_reads=4)
    pb.set_signals_packed(sigs, [0, 0, 1, 0], [0, 400, 0, 800])
    pb.run(1.0, B.RUN_RLE_RECORDS)
    pb.finish()
    assert pb.f32_reruns() == 3
    _check_reads(pb, range(4), False)
    pb.close()
    dm.close()


def test_flipflop_batch_refuses_run_records(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    b = B.Batch(dm, 4, 1000)
    b.set_signals(np.random.default_rng(0).standard_normal((4, 1000)).astype(np.float32))
    with pytest.raises(B.FFHipError):
        b.run(1.0, B.RUN_RLE_RUNS)
    b.run()
    b.finish()
    with pytest.raises(B.FFHipError):
        b.rle_runs(0)
    b.close()
    dm.close()


def test_runnie_fasta_equals_the_two_stage_pipeline(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, RUNNIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(RUNNIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "runlength5_r941native.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    lens = np.clip(np.exp(np.log(2500) + 1.0 * rng.standard_normal(60)), 700, 30000).astype(int)
    for i, n in enumerate(lens):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    (reads / "read_30b.fast5").write_bytes(b"not an HDF5 file")
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, extra=None):
        r = subprocess.run([RUNNIE, "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    def nocall(err):
        return [ln for ln in err.splitlines() if "No basecall returned for" in ln]

    for tag, extra in (("packed", None), ("rows", {"FLAPPIE_DEBUG": "no_pack"}), ("fallback", {"FLAPPIE_DEBUG": "pack_fail"})):
        run_out, run_err = run([], extra)
        assert run_out.count("# ") == 60
        for args, factors, rlc in (([], R.DEFAULT, False), (["--rlc"], R.DEFAULT, True), (["--run-scale", "1.1,0.95,1.3,1.07"], (1.1, 0.95, 1.3, 1.07), False)):
            want_out, want_err = R.fasta_from_run(run_out, factors, rlc)
            out, err = run(["--fasta"] + args, extra)
            assert out == want_out, (tag, args)
            assert sorted(nocall(err)) == sorted(nocall(run_err) + want_err.splitlines()), (tag, args)
            assert len(nocall(run_err)) == 1 and "read_30b.fast5" in nocall(run_err)[0]
            if tag != "packed":
                break
    run_out, _ = run(["--viterbi"])
    out, _ = run(["--viterbi", "--fasta"])
    assert out == R.fasta_from_run(run_out)[0]
    r = subprocess.run([RUNNIE, "--rlc", str(reads)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0                              # --rlc goes with --fasta
    r = subprocess.run([FLAPPIE, "--fasta", str(reads)], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0                              # the flip-flop binary has no such option
