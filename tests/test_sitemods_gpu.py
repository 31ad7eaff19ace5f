"""flappie --remap-mods on the GPU: the scores with C and with 5mC at every C of a mapped sequence by k_site_mods (include/ffhip.h FFHIP_RUN_REMAP_MODS,
ffhip_batch_set_remap_mods, ffhip_batch_site_mods, ffhip_op_site_mods).

  * the operator against the restatement (sitemods_ref.py) at every wave and chunk edge, at both strides of the 60 scores a block, with one base, with a base a
    block and a last base without one, in homopolymer runs of C and Z, with scores of -1e30, with one base of 5000 blocks inside a window; the whole-window
    invariant against ffhip_op_remap; the refusals;
  * on synthetic 5-base models, every read's records against the operator on the batch's OWN transitions and path, byte for byte in both modes -- one read a row,
    ragged, packed, launch per step, paired, f32 re-run -- with nothing for status 0 and 2, one more device-to-host copy call a batch, the buffers counted;
  * the flag's refusals; the binary's mods.tsv against the batch API's records.
Best-path scores are equal to the bit; all-paths scores are within 1 float32 ulp of the fp64 restatement (the recursion's error is orders below half an ulp: only
the one final rounding can differ) and never a NaN."""
import ctypes as C

import numpy as np
import pytest

from flappie_amd import model as M
import remap_ref as RR
import sitemods_ref as S
from test_remap_gpu import _d2h_calls, _same, _state

pytestmark = pytest.mark.gpu
NB = 5
LETTERS = np.array([0, 1, 1, 4, 4, 2, 3], np.uint8)          # heavy in C and Z: runs of both are common


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def _path(rng, N, L):
    rm = np.zeros(N, np.uint8)
    rm[rng.choice(N, L - 1, replace=False)] = 1
    return rm


def _both_modes(B, engine, T, codes, rm, c, stride, where):
    for mode in (False, True):
        got = B.op_site_mods(engine, T, NB, codes, rm, c, mode, stride)
        S.check(got, S.site_mods(T, NB, codes, rm, c, mode), mode, (where, c, mode, stride))


# ------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1500])
def test_operator_against_the_restatement(B, engine, N):
    rng = np.random.default_rng(500 + N)
    k = 0
    for L in sorted({1, N + 1, int(rng.integers(1, N + 2)), int(rng.integers(1, min(N + 1, 40) + 1))}):
        # (long sequences: fewer sites, the restatement is a loop in Python)
        codes = rng.choice(LETTERS, L) if L <= 300 else rng.choice(np.array([0, 2, 3, 0, 2, 3, 1, 1, 4], np.uint8), L)
        if L >= 8:
            codes[2:6] = 1                                  # a run of C, a run of Z behind it
            codes[6:8] = 4
        rm = _path(rng, N, L)
        T = (rng.random((N, 60)) * 100.0 - 50.0).astype(np.float32)          # |T| <= 50
        for c in ((0, 1, 15, 31) if N <= 65 else ((15, 0), (31, 1))[k % 2]):
            _both_modes(B, engine, T, codes, rm, c, (60, 64)[(k + c) % 2], (N, L))
        k += 1


def test_operator_hostile_scores_long_dwell_and_the_same_bytes_again(B, engine):
    rng = np.random.default_rng(9)
    # entries of -1e30: paths through them lose by far, sums stay finite, nothing is NaN
    N, L = 300, 60
    codes, rm = rng.choice(LETTERS, L), _path(rng, N, L)
    T = (rng.random((N, 60)) * 100.0 - 50.0).astype(np.float32)
    T[rng.random((N, 60)) < 0.2] = np.float32(-1e30)
    for c in (1, 15):
        _both_modes(B, engine, T, codes, rm, c, 60, "-1e30")
    # one base dwells 5000 blocks, inside the windows of its neighbours
    lengths = [3] * 6 + [5000] + [2] * 6
    rm = np.concatenate([np.r_[np.zeros(n - 1, np.uint8), np.uint8(1)] for n in lengths])[:-1]
    codes = np.array([0, 2, 1, 1, 3, 0, 4, 2, 1, 3, 0, 2, 3], np.uint8)
    T = (rng.random((rm.size, 60)) * 100.0 - 50.0).astype(np.float32)
    _both_modes(B, engine, T, codes, rm, 15, 64, "dwell")
    for mode in (False, True):
        a, b = (B.op_site_mods(engine, T, NB, codes, rm, 4, mode) for _ in range(2))
        assert a.tobytes() == b.tobytes() and a["nblock"].max() > 5000, mode


def test_operator_whole_window_equals_remap(B, engine):
    rng = np.random.default_rng(13)
    n = 0
    for N in (1, 5, 64, 300):
        for L in sorted({1, min(N + 1, 32), int(rng.integers(1, min(N + 1, 32) + 1))}):
            codes = rng.choice(LETTERS, L)
            T = (rng.random((N, 60)) * 100.0 - 50.0).astype(np.float32)
            rm, score = B.op_remap(engine, T, NB, codes, 2048)          # W >= L - 1
            got = B.op_site_mods(engine, T, NB, codes, rm, 31)           # c >= L - 1
            for rec in got:
                given = rec["can"] if codes[rec["pos"]] == S.CAN else rec["mod"]
                assert rec["nblock"] == N and np.float32(given).tobytes() == np.float32(score).tobytes(), (N, L, rec, score)
                n += 1
    assert n >= 20


def test_operator_refusals(B, engine):
    rng = np.random.default_rng(3)
    T = rng.standard_normal((10, 60)).astype(np.float32)
    codes, rm = np.array([0, 1, 4], np.uint8), np.array([0, 1, 0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
    assert B.op_site_mods(engine, T, NB, codes, rm, 15)["pos"].tolist() == [1, 2]
    two = rm.copy()
    two[0] = 2
    bad = [(T, NB, codes, rm, -1), (T, NB, codes, rm, 32), (T, NB, codes[:2], rm, 15), (T, NB, np.array([0, 1, 5], np.uint8), rm, 15), (T, NB, codes, two, 15),
           (T, NB, codes, rm[:9], 15), (T, NB, np.zeros(0, np.uint8), np.zeros(10, np.uint8), 15), (T[:, :40], 4, np.array([0, 1, 1], np.uint8), rm, 15),
           (T[:, :40], NB, codes, rm, 15)]
    for args in bad:
        with pytest.raises(B.FFHipError) as e:
            B.op_site_mods(engine, *args)
        assert "ffhip error -1:" in str(e.value), (args[1:], str(e.value))      # FFHIP_EINVAL
        assert B.op_site_mods(engine, T, NB, codes, rm, 15)["pos"].tolist() == [1, 2]      # the engine is usable
    assert B.op_site_mods(engine, T, NB, np.array([0, 2, 3], np.uint8), rm, 15).size == 0      # no C, no Z: no records


# ------------------------------------------------------------------------------------ batches
def _bytes_held(B, x):
    B.lib().ffhip_debug_batch_device_bytes.restype = C.c_size_t
    B.lib().ffhip_debug_batch_device_bytes.argtypes = [C.c_void_p]
    return B.lib().ffhip_debug_batch_device_bytes(x.h)


def _codes_of(call):
    return np.array(["ACGTZ".index(x) for x in call], np.uint8)


def _sequences(rng, calls, nblocks):
    """per read, in turn: its own call with some C and Z swapped (three times), none (status 0), one base too many for its blocks (status 2)"""
    seqs = []
    for v, call in enumerate(calls):
        kind = v % 5
        if kind == 3:
            seqs.append(None)
        elif kind == 4:
            seqs.append(rng.integers(0, NB, nblocks[v] + 2).astype(np.uint8))
        else:
            q = _codes_of(call) if call else np.array([1], np.uint8)
            cz = np.flatnonzero((q == S.CAN) | (q == S.MOD))
            swap = cz[rng.random(cz.size) < 0.3]
            q[swap] = S.CAN + S.MOD - q[swap]
            seqs.append(q)
    return seqs


def _check_batches(B, engine, bs, nreads, flags, where, every=1, reruns=False):
    """every read's records against the operator on the batch's own transitions and path, in both modes; returns the number of sites compared"""
    def run(fl):
        _d2h_calls(B)
        if len(bs) == 1:
            bs[0].run(1.0, fl)
        else:
            bs[0].run_pair(bs[1], 1.0, fl)
        for x in bs:
            x.finish()
        return _d2h_calls(B)[0]
    run(flags)
    rng = np.random.default_rng(29)
    seqs = []
    for k, x in enumerate(bs):
        seqs.append(_sequences(rng, [x.basecall(v) for v in range(nreads[k])], [x.read_nblock(v) for v in range(nreads[k])]))
        x.set_remap(seqs[k], 2048)
    copies = run(flags | B.RUN_REMAP)
    before = [[(_state(B, x, v, flags), x.remap(v)) for v in range(0, nreads[k], every)] for k, x in enumerate(bs)]
    held = [_bytes_held(B, x) for x in bs]
    with pytest.raises(B.FFHipError):
        bs[0].site_mods(0)                                  # a run without the flag made none
    assert run(flags) + len(bs) == copies or reruns, where   # (without either flag: one copy fewer again)
    sites, seen = 0, set()
    for c, mode in ((15, False), (31, True), (3, False)):
        for x in bs:
            if (c, mode) != (15, False):                    # (the first round runs on the defaults: 15, best path)
                x.set_remap_mods(c, mode)
        copies_md = run(flags | B.RUN_REMAP | B.RUN_REMAP_MODS)
        if not reruns:                                      # (a re-run's side batch brings its own copies)
            assert copies_md == copies + len(bs), (where, copies, copies_md)
        for k, x in enumerate(bs):
            total = 0
            for n, v in enumerate(range(0, nreads[k], every)):
                st, (old, rec) = _state(B, x, v, flags), before[k][n]
                for key in st:
                    assert _same(st[key], old[key]), (where, k, v, key)
                got, sm = x.remap(v), x.site_mods(v)
                assert got["status"] == rec["status"] and got["L"] == rec["L"] and _same(got["score"].view(np.uint32), rec["score"].view(np.uint32)), (where, k, v)
                seen.add(got["status"])
                if got["status"] != 1:
                    assert sm is None, (where, k, v)
                    continue
                assert np.array_equal(got["rm"], rec["rm"]), (where, k, v)
                want = B.op_site_mods(engine, x.transitions(v), NB, seqs[k][v], got["rm"], c, mode)
                assert sm.dtype == B.SITE_MOD_DTYPE and sm.tobytes() == want.tobytes(), (where, k, v, c, mode)
                assert sm["pos"].tolist() == S.sites(seqs[k][v]) and not np.any(np.isnan(sm["can"])) and not np.any(np.isnan(sm["mod"])), (where, k, v)
                total += sm.size
            assert total > 0, (where, k)
            sites += total
            if every == 1 and not getattr(x, "_had_mods", False):          # (the batch's first run with the flag: the buffers are new)
                assert _bytes_held(B, x) >= held[k] + 16 * total, (where, k, total)
            x._had_mods = True
        again = [[x.site_mods(v) for v in range(0, nreads[k], every)] for k, x in enumerate(bs)]
        run(flags | B.RUN_REMAP | B.RUN_REMAP_MODS)         # a second run: the same bytes
        for k, x in enumerate(bs):
            for n, v in enumerate(range(0, nreads[k], every)):
                a, b = again[k][n], x.site_mods(v)
                assert (a is None and b is None) or a.tobytes() == b.tobytes(), (where, k, v)
    assert seen == {0, 1, 2}, (where, seen)
    for x in bs:
        x.set_remap_mods(15, False)
        x.set_remap(None)
    return sites


@pytest.mark.parametrize("hidden", [64, 256])
def test_batch_records_rows_ragged_packed(B, engine, hidden):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, hidden, seed=1))
    rng = np.random.default_rng(hidden)
    sig = rng.standard_normal((16, 1500)).astype(np.float32)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(sig)
    n = _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE, ("rows", hidden))
    b.close()
    sigs = list(sig[:4]) + [rng.standard_normal(int(k)).astype(np.float32) for k in rng.integers(300, 1501, 12)]
    b = B.Batch(dm, 16, 1500)
    b.set_signals_ragged(sigs)
    n += _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE | B.RUN_MOVES, ("ragged", hidden))
    b.close()
    if hidden >= 128:                                       # (packed batches: models of 128 .. 512 hidden units)
        pb = B.Batch(dm, 8, 3000, max_reads=16)
        slot, off = pb.pack_plan([x.size for x in sigs])
        assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
        pb.set_signals_packed(sigs, slot, off)
        n += _check_batches(B, engine, [pb], [16], B.RUN_NO_TRACE, ("packed", hidden))
        n += _check_batches(B, engine, [pb], [16], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, ("packed per step", hidden))
        pb.close()
    else:
        b = B.Batch(dm, 16, 1500)
        b.set_signals_ragged(sigs)
        n += _check_batches(B, engine, [b], [16], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE, ("ragged per step", hidden))
        b.close()
    dm.close()
    assert n >= 1000, n


def _lstm_trunk_with_the_5_base_head(hidden, seed):
    """layer launches pair for the LSTM trunk at H = 384 only, and only the LSTM trunk's convolution lets a sample leave the split format's range (GRUmod's ends in
    tanh): the LSTM trunk under the GRUmod model's 5-base head is the 10-state model of both shapes"""
    lstm, gru = M.synthetic_model(M.NET_LSTM5, hidden, seed=seed), M.synthetic_model(M.NET_GRUMOD5, hidden, seed=seed)
    return M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b)


def test_batch_records_paired(B, engine):
    dm = B.DeviceModel(engine, _lstm_trunk_with_the_5_base_head(384, 2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 256, 600)
        b.set_signals(rng.standard_normal((256, 600)).astype(np.float32))
        pair.append(b)
    pair[0].run_pair(pair[1], 1.0, B.RUN_NO_TRACE)
    assert pair[0].paired() and pair[1].paired()
    for b in pair:
        b.finish()
    assert _check_batches(B, engine, pair, [256, 256], B.RUN_NO_TRACE, "pair", every=16) > 100
    for b in pair:
        b.close()
    dm.close()


def test_batch_records_after_an_f32_rerun(B, engine):
    dm = B.DeviceModel(engine, _lstm_trunk_with_the_5_base_head(128, 1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 1501, 16)]
    sigs[0][200] = 6.0e4                                    # (reads 0 and 5: their own calls are their sequences, so they are mapped)
    sigs[5][300] = 6.0e4
    b = B.Batch(dm, 16, 1500)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], 0, "rerun rows", reruns=True)
    assert b.f32_reruns() == 2 and b.remap(0)["status"] == 1 and b.remap(5)["status"] == 1
    b.close()
    pb = B.Batch(dm, 16, 3000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, engine, [pb], [16], B.RUN_MOVES, "rerun packed", reruns=True)
    assert pb.f32_reruns() >= 2
    pb.close()
    dm.close()


def test_flag_refusals_leave_the_batch_usable(B, engine):
    rng = np.random.default_rng(2)
    sig = rng.standard_normal((4, 1000)).astype(np.float32)

    def refused(what, f, *args):
        with pytest.raises(B.FFHipError) as e:
            f(*args)
        assert "ffhip error -1:" in str(e.value) and what in str(e.value), (what, str(e.value))
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_GRUMOD5, 64, seed=1))
    b = B.Batch(dm, 4, 1000)
    b.set_signals(sig)
    seqs = [rng.choice(LETTERS, 40) for _ in range(4)]
    b.set_remap(seqs, 2048)
    refused("FFHIP_RUN_REMAP", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP_MODS)
    refused("FFHIP_RUN_NO_DECODE", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_NO_DECODE | B.RUN_REMAP | B.RUN_REMAP_MODS)
    refused("context", b.set_remap_mods, 32)
    refused("context", b.set_remap_mods, -1)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_MODS)
    refused("running", b.set_remap_mods, 3)                 # not between a run and its finish
    b.finish()
    for v in range(4):
        rec = b.remap(v)
        assert rec["status"] == 1
        assert b.site_mods(v).tobytes() == B.op_site_mods(engine, b.transitions(v), NB, seqs[v], rec["rm"], 15, False).tobytes(), v      # the defaults
    b.close()
    dm.close()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))          # nbase 4
    b = B.Batch(dm, 4, 1000)
    b.set_signals(sig)
    b.set_remap([rng.integers(0, 4, 40).astype(np.uint8) for _ in range(4)], 2048)
    refused("modified base", b.run, 1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_MODS)
    b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP)
    b.finish()
    assert b.remap(0)["status"] == 1
    b.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_remap_mods(B, engine, tmp_path):
    import os
    import re
    import subprocess
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC")
    M.write_mdl(str(tmp_path / "flipflop_r941native5mC.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 20
    names = ["uuid-%04d" % i for i in range(nread)]
    for i, n in enumerate(rng.integers(1500, 4000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), names[i], synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_5mC", "--batch", "16", "--format", "fastq"] + args + [str(reads)], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    trace = tmp_path / "trace.hdf5"
    default, _ = run(["--trace", str(trace)])
    lines = default.split("\n")[:-1]
    recs = [lines[k:k + 4] for k in range(0, len(lines), 4)]
    order = [r[0][1:].split("  {")[0] for r in recs]
    calls = {r[0][1:].split("  {")[0]: r[1] for r in recs}
    assert sorted(order) == names
    seqs, text = {}, ""
    for i, name in enumerate(names):                        # own call with C and Z swapped; none; a bad letter
        call, kind = calls[name], i % 4
        if kind < 2:
            seqs[name] = call.translate(str.maketrans("CZ", "ZC")) if kind else call
        elif kind == 2:
            seqs[name] = call[:3] + "N" + call[3:]
        if name in seqs:
            text += ">%s\n%s\n" % (name, seqs[name])
    refs = tmp_path / "refs.fa"
    refs.write_text(text)
    plain_map, plain_ev = tmp_path / "plain.tsv", tmp_path / "plain_events.tsv"
    assert run(["--remap", str(refs), "--remap-out", str(plain_map), "--remap-events", str(plain_ev)])[0] == default
    tables = {}
    for tag, extra in (("best", []), ("all", ["--remap-mods-all-paths"]), ("c3", ["--remap-mods-context", "3"])):
        mp, ev, md = tmp_path / (tag + "_map.tsv"), tmp_path / (tag + "_events.tsv"), tmp_path / (tag + "_mods.tsv")
        args = ["--remap", str(refs), "--remap-out", str(mp), "--remap-mods", str(md)] + extra + (["--remap-events", str(ev)] if tag != "c3" else [])
        stdout, err = run(args)
        assert stdout == default and mp.read_text() == plain_map.read_text(), tag
        if tag != "c3":
            assert ev.read_bytes() == plain_ev.read_bytes(), tag
        tables[tag] = (md.read_text().split("\n")[:-1], err)
    # the batch API on the signals the binary prepared (--trace), the same sequences: wherever the mapping is the binary's, so are the lines
    by_name = {}
    for line in plain_map.read_text().split("\n")[:-1]:
        f = line.split("\t")
        by_name[f[0]] = f
    mapped = [name for name in order if name in seqs and by_name[name][1] == "1"]
    assert len(mapped) >= 8
    sigs = [dump_trace(trace, name)[0] for name in mapped]
    dm = B.DeviceModel(engine, mdl)
    b = B.Batch(dm, len(mapped), max(x.size for x in sigs))
    b.set_signals_ragged(sigs)
    b.set_remap([np.array(["ACGTZ".index(x) for x in seqs[name]], np.uint8) for name in mapped], 2048)
    for tag, c, mode in (("best", 15, False), ("all", 15, True), ("c3", 3, False)):
        b.set_remap_mods(c, mode)
        b.run(1.0, B.RUN_NO_TRACE | B.RUN_REMAP | B.RUN_REMAP_MODS)
        b.finish()
        want, nreads, compared = [], 0, 0
        got, err = tables[tag]
        at = 0
        for v, name in enumerate(mapped):
            rec, sm = b.remap(v), b.site_mods(v)
            mine = [g.split("\t") for g in got if g.split("\t")[0] == name]
            assert [int(f[1]) for f in mine] == sm["pos"].tolist() and [f[2] for f in mine] == [seqs[name][p] for p in sm["pos"]], (tag, name)
            assert got[at:at + len(mine)] == ["\t".join(f) for f in mine], (tag, name)          # reads in output order, sites in signal order
            at += len(mine)
            nreads += 1
            for f in mine:
                assert len(f) == 7 and f[4] == "%.9g" % np.float32(f[4]) and f[5] == "%.9g" % np.float32(f[5]), f
                assert f[6] == "%.9g" % (float(np.float32(f[4])) - float(np.float32(f[5]))), f
            starts = ",".join(str(x) for x in RR.starts_maxdev(rec["rm"], rec["L"])[0])
            if rec["status"] == 1 and by_name[name][9] == starts and by_name[name][8] == "%.9g" % rec["score"]:
                assert ["\t".join(f) for f in mine] == ["%s\t%d\t%s\t%d\t%.9g\t%.9g\t%.9g" % (name, r["pos"], seqs[name][r["pos"]], r["nblock"], r["can"], r["mod"],
                                                                                         float(r["can"]) - float(r["mod"])) for r in sm], (tag, name)
                compared += 1
        assert at == len(got) and compared >= 8, (tag, at, len(got), compared)
        assert dict((k, int(v)) for k, v in re.findall(r"^mods\t(\S+)\t(\d+)$", err, re.M)) == {"reads": nreads, "sites": len(got)}, err
    b.close()
    dm.close()
