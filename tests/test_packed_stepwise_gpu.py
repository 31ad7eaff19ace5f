"""Packed batches on the launch-per-step kernels (include/ffhip.h "packed batches"): the fall-back of a GPU another process shares.

When a persistent layer launch cannot make all its workgroups resident, ffhip_batch_finish runs the batch again on the launch-per-step kernels and sends the
engine's next runs there.  A packed batch takes that path too: the step kernels' LIVE forms force h and c to zero where the batch's live mask says a slot holds
no read, and the in-projection is computed a window of steps at a time, so that what the path holds does not grow with the row.  Held here: every read of a
packed batch run step by step is, BIT FOR BIT, what the same read gives one read a row step by step; a forced time-out (FFHIP_DEBUG=force_abort, which pre-sets
the abort word: no kernel waits) of a packed batch, of a pair, and of a batch before it is recovered; the memory bound; the f32 re-run of a saturated row; and the
`flappie` / `runnie` binaries, which lose no read when a packed batch fails and say so in their exit status when a read could not be called at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
from oracle import ffo
from test_packed_gpu import _same
from test_packed_rle_gpu import _check_oracle
from test_packed_rle_gpu import _same as _same_rle
from test_ragged_gpu import check_read

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


def _fallbacks(B, eng):
    L = B.lib()
    L.ffhip_debug_fallback_count.argtypes = [C.c_void_p]
    L.ffhip_debug_fallback_count.restype = C.c_int
    return int(L.ffhip_debug_fallback_count(eng.h))


class _env:
    """environment variables set for the calls inside the block (the library reads FFHIP_DEBUG / FFHIP_NO_FALLBACK when a run is enqueued or finished)"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _lens(rng, rows, cap):
    # every length mod the stride, the shortest legal read (the window), reads far shorter than a row and one that fills a row
    return [19, 20, 21, 22, 23, 24, 45, 100, 101, 102, 103, 104, cap - 8, cap // 2, cap // 2 + 1] + \
        [int(x) for x in np.clip(np.exp(np.log(cap / 6) + 0.9 * rng.standard_normal(3 * rows)), 30, cap - 50)]


def _packed(B, dm, rows, cap, sigs):
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan([x.size for x in sigs])
    order = [i for i in range(len(sigs)) if slot[i] >= 0]
    pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
    return pb, slot, off, order


def _snap(pb, v, rle=False, post=True):
    """everything a read's results are, as bits (the posterior: when the run computed it)"""
    p, q = pb.path(v)
    out = [pb.read_nblock(v), np.float32(pb.score(v)).view(np.uint32), pb.transitions(v).view(np.uint32), p, q[1:].view(np.uint32)]
    if post:
        out.append(pb.posterior(v).view(np.uint32))
    if not rle:
        out += [pb.basecall(v), pb.quality(v), pb.trace(v)]
    return out


def _snap_eq(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _against_rows(B, dm, pb, sigs, order, cap, rows, flags, rle):
    """the packed batch's reads against one-read-a-row batches of the same reads run with the same flags, `rows` at a time (the posterior: unless VITERBI_ONLY)"""
    post = not (flags & B.RUN_VITERBI_ONLY)
    bad = []
    for k0 in range(0, len(order), rows):
        grp = order[k0:k0 + rows]
        ub = B.Batch(dm, len(grp), cap)
        ub.set_signals_ragged([sigs[i] for i in grp])
        ub.run(1.0, flags)
        ub.finish()
        assert ub.rnn_path() == 0
        for j in range(len(grp)):
            if rle:
                ok = _same_rle(pb, k0 + j, ub, j, post)
            elif post:
                ok = _same(pb, k0 + j, ub, j)
            else:
                ok = _snap_eq(_snap(pb, k0 + j, post=False), _snap(ub, j, post=False))
            if not ok:
                bad.append(grp[j])
        ub.close()
    return bad


@pytest.mark.parametrize("kind,hidden,rows,cap", [
    (M.NET_LSTM5, 128, 16, 3000),
    (M.NET_LSTM5, 384, 32, 2500),
    (M.NET_LSTM5, 512, 16, 2000),
    (M.NET_GRUMOD5, 128, 16, 2000),
    (M.NET_GRUMOD5, 256, 32, 3000),      # 10 states, stride 2
    (M.NET_LSTM5_RLE, 128, 16, 3000),
    (M.NET_LSTM5_RLE, 384, 32, 2500),
])
def test_packed_stepwise_equals_one_read_a_row_stepwise(B, engine, kind, hidden, rows, cap):
    mdl = M.synthetic_model(kind, hidden, seed=1)
    rle = kind == M.NET_LSTM5_RLE
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(hidden + rows + 7)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in _lens(rng, rows, cap)]
    pb, slot, off, order = _packed(B, dm, rows, cap, sigs)
    assert len(order) >= rows + 10 and max(np.bincount([slot[i] for i in order])) >= 3, "the plan should put several reads in a row"
    om = ffo.OracleModel(mdl)
    for flags in (B.RUN_STEPWISE_RNN, B.RUN_STEPWISE_RNN | B.RUN_VITERBI_ONLY):
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        pb.run(1.0, flags)
        pb.finish()
        assert pb.nreads() == len(order) and pb.rnn_path() == 0
        assert _against_rows(B, dm, pb, sigs, order, cap, rows, flags, rle) == []
    # ... and a sample against the oracle itself (the last run decoded from the scores)
    for v in list(range(0, 12)) + list(range(12, len(order), 9)):
        if rle:
            _check_oracle(pb, v, om.runlength_call(sigs[order[v]], viterbi_only=True), True)
            continue
        ref = om.basecall(sigs[order[v]], viterbi_only=True)
        if hidden == 512 and pb.quality(v) != ref["quality"]:
            # (the near-tie class of DESIGN.md section 3, as in test_packed_gpu.py: a quality character on a rounding boundary, everything else the oracle's)
            assert pb.basecall(v) == ref["basecall"] and np.array_equal(pb.path(v)[0], ref["path"]) and np.abs(pb.transitions(v) - ref["trans"]).max() <= 5e-5
            assert sum(1 for x, y in zip(pb.quality(v), ref["quality"]) if x != y) == 1
            continue
        check_read(pb, v, ref, viterbi_only=True)
    pb.close()
    dm.close()


def _lstm128_packed(B, dm, seed, rows=16, cap=3000):
    rng = np.random.default_rng(seed)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in _lens(rng, rows, cap)]
    pb, slot, off, order = _packed(B, dm, rows, cap, sigs)
    return pb, sigs, order


def test_a_packed_batch_that_times_out_is_run_again_step_by_step(B):
    eng = B.Engine(0)                                  # its own engine: the fall-back state is per engine
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=7)
    dm = B.DeviceModel(eng, mdl)
    pb, sigs, order = _lstm128_packed(B, dm, 21)
    pb.run(); pb.finish()
    assert pb.rnn_path() == 3 and _fallbacks(B, eng) == 0
    with _env(FFHIP_DEBUG="force_abort"):
        pb.run(); pb.finish()                          # "times out"; finish() runs it again on the step kernels
    assert _fallbacks(B, eng) == 1 and pb.rnn_path() == 0
    got = [_snap(pb, v) for v in range(len(order))]
    pb.run(); pb.finish()                              # still wary of the co-tenant: straight to the step kernels
    assert pb.rnn_path() == 0 and _fallbacks(B, eng) == 1
    assert all(_snap_eq(got[v], _snap(pb, v)) for v in range(len(order)))
    pb.run(1.0, B.RUN_STEPWISE_RNN); pb.finish()       # an explicit stepwise run of the same batch
    assert all(_snap_eq(got[v], _snap(pb, v)) for v in range(len(order)))
    pb.close(); dm.close(); eng.close()
    with _env(FFHIP_DEBUG="force_abort", FFHIP_NO_FALLBACK="1"):
        eng2 = B.Engine(0)
        dm2 = B.DeviceModel(eng2, mdl)
        pb2, _, _ = _lstm128_packed(B, dm2, 21)
        pb2.run()
        with pytest.raises(B.FFHipError):              # the old behaviour stays available
            pb2.finish()
        pb2.close(); dm2.close(); eng2.close()


def test_packed_batches_in_the_co_tenant_window_run_step_by_step(B):
    eng = B.Engine(0)
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1)
    dm = B.DeviceModel(eng, mdl)
    sig = np.random.default_rng(5).standard_normal((16, 900)).astype(np.float32)
    b = B.Batch(dm, 16, 900)
    b.set_signals(sig)
    with _env(FFHIP_DEBUG="force_abort"):
        b.run(); b.finish()                            # a one-read-a-row batch times out: the engine's next runs go step by step
    assert _fallbacks(B, eng) == 1 and b.rnn_path() == 0
    pb, sigs, order = _lstm128_packed(B, dm, 16 + 3000)
    pb.run(); pb.finish()                              # (flags 0: refused with EINVAL before packed batches had a stepwise form)
    assert pb.rnn_path() == 0
    assert _against_rows(B, dm, pb, sigs, order, 3000, 16, B.RUN_STEPWISE_RNN, False) == []
    b.close(); pb.close(); dm.close(); eng.close()


def test_a_timed_out_pair_of_packed_batches_recovers(B):
    eng = B.Engine(0)
    mdl = M.synthetic_model(M.NET_LSTM5, 384, seed=1)
    dm = B.DeviceModel(eng, mdl)
    rng = np.random.default_rng(11)
    rows, cap = 256, 1500
    pbs = []
    for k in range(2):
        lens = [int(x) for x in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(600)), 25, cap - 50)]
        sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
        pbs.append(_packed(B, dm, rows, cap, sigs)[0])
    with _env(FFHIP_DEBUG="force_abort"):
        pbs[0].run_pair(pbs[1])
        for pb in pbs:
            pb.finish()
            assert pb.rnn_path() == 0
    assert _fallbacks(B, eng) >= 1
    sample = lambda pb: list(range(0, pb.nreads(), 7))      # noqa: E731
    got = [[_snap(pb, v) for v in sample(pb)] for pb in pbs]
    strings = [[(pb.basecall(v), pb.quality(v), pb.score(v)) for v in range(pb.nreads())] for pb in pbs]
    for k, pb in enumerate(pbs):
        pb.run(1.0, B.RUN_STEPWISE_RNN)
        pb.finish()
        assert all(_snap_eq(g, _snap(pb, v)) for g, v in zip(got[k], sample(pb)))
        assert strings[k] == [(pb.basecall(v), pb.quality(v), pb.score(v)) for v in range(pb.nreads())]
        pb.close()
    dm.close(); eng.close()


def test_the_stepwise_path_of_a_packed_batch_does_not_grow_with_the_row(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=2)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(3)
    rows, cap = 16, 30000
    sigs = [rng.standard_normal(n).astype(np.float32) for n in np.clip(np.exp(np.log(9000) + 0.6 * rng.standard_normal(44)), 500, cap - 100).astype(int)]
    pb, slot, off, order = _packed(B, dm, rows, cap, sigs)
    assert len(order) >= 30
    act = pb.nblock * 16 * mdl.hidden * 4                  # one fp32 activation buffer: Tb x rows x H x 4 bytes
    pb.run(); pb.finish()
    assert pb.rnn_path() == 3
    after_default = pb.device_bytes()
    pb.run(1.0, B.RUN_STEPWISE_RNN); pb.finish()
    assert pb.rnn_path() == 0
    grew = pb.device_bytes() - after_default
    assert 0 <= grew < act, (grew, act)
    want = [(pb.basecall(v), pb.quality(v)) for v in range(len(order))]
    fresh = _packed(B, dm, rows, cap, sigs)[0]             # a fresh object whose first run is the stepwise one
    fresh.run(1.0, B.RUN_STEPWISE_RNN); fresh.finish()
    assert fresh.device_bytes() - after_default < act, (fresh.device_bytes() - after_default, act)
    assert want == [(fresh.basecall(v), fresh.quality(v)) for v in range(len(order))]
    fresh.close(); pb.close(); dm.close()


def test_outlier_sample_in_a_packed_row_is_run_again_on_the_f32_path_behind_a_stepwise_run(B, engine):
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1)
    dm = B.DeviceModel(engine, mdl)
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(n).astype(np.float32) for n in (900, 400, 1200, 800)]
    sigs[1][200] = 6.0e4
    pb = B.Batch(dm, 16, 6000, max_reads=4)
    pb.set_signals_packed(sigs, [0, 0, 1, 0], [0, 400, 0, 800])
    pb.run(1.0, B.RUN_STEPWISE_RNN)
    pb.finish()
    assert pb.rnn_path() == 0 and pb.f32_reruns() == 3      # every read of the saturated row, none of the other
    om = ffo.OracleModel(mdl)
    for v in range(4):
        check_read(pb, v, om.basecall(sigs[v]))
    pb.close()
    dm.close()


def _reads_dir(tmp_path, write_fast5, synth_raw):
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(2)
    raws = {}
    lens = np.clip(np.exp(np.log(2500) + 1.0 * rng.standard_normal(70)), 700, 30000).astype(int)
    for i, n in enumerate(lens):
        raw = synth_raw(rng, int(n))
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, raw)
        raws["read_%02d.fast5" % i] = ("uuid-%04d" % i, raw)
    return reads, raws


def _npacked(stderr):
    pad = [ln for ln in stderr.splitlines() if ln.startswith("batches:")][-1]
    return int(pad.split("(")[1].split()[0])


FALLBACK_WARNING = "falling back to the launch-per-step kernels"


def test_cli_packed_batches_under_a_forced_time_out(tmp_path):
    from test_cli import FLAPPIE, TOOL, FAST5LIB, _oracle_calls, _parse_fastq, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), mdl)
    reads, raws = _reads_dir(tmp_path, write_fast5, synth_raw)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path), FLAPPIE_CLI_TIMING="1", FFHIP_DEBUG="force_abort")
    out = {}
    for tag, extra in (("packed", {}), ("rows", {"FLAPPIE_DEBUG": "no_pack"})):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", str(reads)], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert FALLBACK_WARNING in r.stderr
        assert (_npacked(r.stderr) > 0) == (tag == "packed"), r.stderr
        out[tag] = r.stdout
    assert out["packed"] == out["rows"]                      # the same records in the same order, byte for byte
    ref = _oracle_calls(mdl, raws)
    by_uuid = {v["uuid"]: v for v in ref.values()}
    recs = _parse_fastq(out["packed"])
    assert sorted(x[0] for x in recs) == sorted(by_uuid)
    for name, hdr, bases, quals in recs:
        assert bases == by_uuid[name]["basecall"] and quals == by_uuid[name]["quality"], name


def test_runnie_packed_batches_under_a_forced_time_out(tmp_path):
    from test_cli import FAST5LIB, RUNNIE, TOOL, synth_raw, write_fast5
    from test_host_layer import _f
    if not (os.path.exists(RUNNIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "runlength5_r941native.h"), mdl)
    reads, raws = _reads_dir(tmp_path, write_fast5, synth_raw)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path), FLAPPIE_CLI_TIMING="1", FFHIP_DEBUG="force_abort")
    out = {}
    for tag, extra in (("packed", {}), ("rows", {"FLAPPIE_DEBUG": "no_pack"})):
        r = subprocess.run([RUNNIE, "--batch", "16", str(reads)], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert FALLBACK_WARNING in r.stderr
        assert (_npacked(r.stderr) > 0) == (tag == "packed"), r.stderr
        out[tag] = r.stdout
    assert out["packed"] == out["rows"]
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


def test_cli_says_when_reads_could_not_be_called(tmp_path):
    from test_cli import FLAPPIE, TOOL, FAST5LIB, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=1, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), mdl)
    reads, raws = _reads_dir(tmp_path, write_fast5, synth_raw)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path), FFHIP_DEBUG="force_abort", FFHIP_NO_FALLBACK="1")
    r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16", str(reads)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0, r.stderr
    assert "its reads go to one-read-a-row batches" in r.stderr, r.stderr
    m = re.search(r"(\d+) read\(s\) were not called", r.stderr)
    assert m and int(m.group(1)) == len(raws), r.stderr
