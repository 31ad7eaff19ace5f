"""flappie --poly-tail on the GPU (k_polytail, FFHIP_RUN_POLYTAIL; the definition: include/ffhip.h "poly tail", restated in polytail_ref.py):
  * the windows' mu, q and flag bit for bit at every wave and round edge of the 256-thread workgroup, on inputs that rule out another order of the sums;
  * records on hand-made flags: gaps, the round's seam, ties, the reach, the least length, the three statuses, Z read as C, the refusals;
  * batches on the synthetic models -- one read a row, ragged, packed, launch per step, paired, f32 re-run -- each record against the restatement on the batch's OWN
    path and the signal it was given; nothing else the run returns moves; one more copy call; the same bytes again and in another batch shape;
  * the binary's tags against the restatement on --trace's signal and the path's bases as the mv tag and the call give them.
Every integer field, rate and bases are compared bit for bit, level within 2^-23 max|x| (polytail_ref.check)."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import polytail_ref as R
from test_barcodes_gpu import _d2h_calls, _state

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


# ------------------------------------------------------------------------------------ the windows
def _signal(rng, kind, n):
    if kind == 0:
        return rng.standard_normal(n).astype(np.float32)
    if kind == 1:
        return (1000.0 + 1e-3 * rng.standard_normal(n)).astype(np.float32)       # a one-pass sum of squares loses every digit of q here
    big = rng.choice([-1e4, 1e4], n) * rng.random(n)
    small = rng.choice([-1e-4, 1e-4], n) * rng.random(n)
    return np.where(rng.random(n) < 0.5, big, small).astype(np.float32)          # any other order of the additions rounds differently


@pytest.mark.parametrize("K,S", [(1, 5), (8, 5), (64, 5), (1, 2), (8, 2), (64, 2)])
def test_windows_bit_equal_at_every_edge(B, engine, K, S):
    rng = np.random.default_rng(100 * K + S)
    flagged = 0
    for i, NW in enumerate((0, 1, 63, 64, 65, 255, 256, 257, 513)):
        N = NW * K + (K - 1 if K > 1 else 0)                  # not a multiple of K (K = 1 has none)
        if N == 0:
            N = 1
        for short in (0, S - 1):                              # n = N S, and the read ends inside its last block
            n = max(N * S - short, 0) if NW else min(K * S - 1, N * S)
            x = _signal(rng, (i + (short > 0)) % 3, n)
            nw = R.nwindows(n, S, N, K)
            assert nw == NW or (short and nw == (N - 1) // K)
            for w in range(0, nw, 7):                         # a window of one repeated value now and then
                x[w * K * S:(w + 1) * K * S] = x[w * K * S]
            path = rng.integers(0, 8, N + 1).astype(np.int32)
            mu0, q0, _, _ = R.windows(x, S, path, 4, R.params(window=K, max_sd=0.0))
            for max_sd in (0.0, float(np.sqrt(np.median(q0) / (K * S))) if nw else 1.0):      # exactly flat only; about half of the windows
                p = R.params(window=K, base=int(rng.integers(0, 4)), min_calls=int(rng.integers(0, K // 2 + 1)), max_sd=max_sd)
                mu, q, flag, _ = R.windows(x, S, path, 4, p)
                gmu, gq, gflag = B.op_polytail_windows(engine, x, S, path, 4, **p)
                where = (K, S, NW, short, max_sd)
                assert gmu.size == nw and gmu.tobytes() == mu.tobytes(), (where, np.flatnonzero(gmu != mu)[:5])
                assert gq.tobytes() == q.tobytes(), (where, np.flatnonzero(gq != q)[:5], R.margin(q, _))
                assert np.array_equal(gflag, flag), (where, np.flatnonzero(gflag != flag)[:5])
                if max_sd == 0.0 and nw:
                    assert np.all(q[::7] == 0.0) and np.all(gq[::7] == 0.0)                    # one repeated value: q is 0.0 exactly
                    if p["min_calls"] == 0:
                        assert np.all(gflag[::7] == 1)
                flagged += int(flag.sum())
    assert flagged > 100


# ------------------------------------------------------------------------------------ records on hand-made flags
def _read_of_flags(rng, flags, K, S, t=0, nbase=4, tail_blocks=0, z=False):
    """a signal and a path whose windows carry these flags at max_sd 0.01 and min_calls K: a flagged window is one repeated value under blocks of the tail's base,
    any other is noise under bases that change every block (each a move); tail_blocks more such blocks follow the windows"""
    NW = len(flags)
    N = NW * K + tail_blocks
    x = rng.standard_normal(N * S).astype(np.float32)
    others = [b for b in range(4) if b != t]
    bases = np.array([others[b % 3] for b in range(N)])
    for w in np.flatnonzero(flags):
        x[w * K * S:(w + 1) * K * S] = 0.5 + 0.25 * (w % 3)
        bases[w * K:(w + 1) * K] = 4 if z else t
    return x, R.path_of_bases(bases, nbase)


def test_records_on_hand_made_flags(B, engine):
    rng = np.random.default_rng(9)
    K, S, G = 2, 5, 2
    seen = set()

    def run(flags, expect=None, tail=30, nbase=4, z=False, read_base=None, **kw):
        p = R.params(**dict(dict(window=K, min_calls=K, gap=G, min_windows=3, search=10 ** 6, min_bases=5, max_sd=0.01), **kw))
        x, path = _read_of_flags(rng, np.asarray(flags), p["window"], S, t=p["base"] if read_base is None else read_base, nbase=nbase, tail_blocks=tail, z=z)
        want = R.record(x, S, path, nbase, p)
        assert R.record(x, S, path, nbase, p, scan=True).tobytes() == want.tobytes()
        got = B.op_polytail(engine, x, S, path, nbase, **p)
        R.check(got, want, x, (flags if len(flags) < 40 else len(flags), kw))
        if expect is not None:
            KS = p["window"] * S
            assert (int(want["status"]), int(want["first"]) // KS, (int(want["first"]) + int(want["count"])) // KS) == expect, (want, expect)
        seen.add(int(want["status"]))
        return want

    one, zero = [1], [0]
    run(one * 5 + zero * G + one * 5, (1, 0, 10 + G))                                   # a gap of exactly G is bridged
    run(one * 5 + zero * (G + 1) + one * 4, (1, 0, 5))                                  # ... one of G + 1 is not
    run(zero * 3 + one * 252 + zero * 2 + one * 20 + zero * 3, (1, 3, 277))             # a gap that straddles windows 255 / 256
    run(zero * 3 + one * 251 + zero * 3 + one * 20 + zero * 3, (1, 3, 254))             # ... and one window too wide there
    run(zero * 3 + one * 252 + zero * 3 + one * 300, (1, 258, 558))                     # the later, longer one wins: a candidate longer than a round
    run(one * 700, (1, 0, 700))
    run(zero + one * 6 + zero * 4 + one * 6 + zero, (1, 1, 7))                          # two of equal length: the smallest ws ...
    run(zero + one * 6 + zero * 4 + one * 6 + zero, (1, 11, 17), from_end=1)            # ... the largest we from the end
    run(zero * 300 + one * 6 + zero * 4 + one * 6, (1, 300, 306))                       # (the tie beyond the first round)
    run(zero * 9 + one * 4 + zero * 5 + one * 8, (1, 9, 13), search=10)                 # ws = R - 1 is in reach, the longer one at ws = 18 is not
    run(zero * 10 + one * 4 + zero * 5, (2, 0, 0), search=10)                           # ws = R is not
    run(one * 8 + zero * 5 + one * 4 + zero * 9, (1, 13, 17), search=10, from_end=1, tail=0)       # the mirror: we = NW - R + 1 is in reach ...
    run(one * 8 + zero * 5 + one * 4 + zero * 10, (2, 0, 0), search=10, from_end=1, tail=0)        # ... we = NW - R is not
    run(zero * 2 + one * 3 + zero * 5, (1, 2, 5))                                       # Wmin met
    run(zero * 2 + one * 2 + zero * 5, (2, 0, 0))                                       # ... and missed by one
    w = run(zero * 2 + one * 4, tail=11, min_bases=10)                                  # c = 10 moves behind the tail (the last block never moves)
    assert int(w["status"]) == 1
    w = run(zero * 2 + one * 4, tail=10, min_bases=10)                                  # c = min_bases - 1
    assert int(w["status"]) == 3 and float(w["rate"]) == 0.0 and int(w["count"]) == 4 * K * S and int(w["flat"]) == 4
    run(zero * 2 + one * 4, (3, 2, 6), tail=0)                                      # the tail runs to the read's end: no samples beside it
    run(zero * 6 + one * 4, (3, 6, 10), tail=0, from_end=1, min_bases=12)               # from the end: the bases in FRONT of the tail (11 moves, the first block has none)
    run(zero * 6 + one * 4, (1, 6, 10), tail=0, from_end=1, min_bases=11)
    run(zero * 40, (2, 0, 0))                                                           # no flag at all
    run(one * 40, (2, 0, 0), max_sd=0.0, base=1, min_calls=1, read_base=0)              # flat, but none of the tail's base
    run(one * 4 + zero * 3, (1, 0, 4), nbase=5, z=True, base=1)                         # Z read as C on an nbase 5 path
    run(one * 4 + zero * 3, (2, 0, 0), nbase=5, z=True, base=0)
    run(one * 5 + zero * 3 + one * 5 + zero * 17 + one * 6, (1, 0, 13), gap=16, window=8)      # another window and the widest gap
    # N = 1: no window at K = 2, one at K = 1
    x1 = np.full(S, 0.25, np.float32)
    for K1, st in ((2, 2), (1, 3)):
        p = R.params(window=K1, min_calls=0, min_windows=1, max_sd=0.0)
        want = R.record(x1, S, [0, 0], 4, p)
        assert int(want["status"]) == st
        R.check(B.op_polytail(engine, x1, S, [0, 0], 4, **p), want, x1, ("N = 1", K1))
    R.check(B.op_polytail(engine, np.zeros(0, np.float32), S, [1, 2, 3], 4), R.record(np.zeros(0, np.float32), S, [1, 2, 3], 4, R.params()), [], "no samples")
    assert seen == {1, 2, 3}, seen
    # the refusals
    x, path = _read_of_flags(rng, np.array(one * 4), K, S)
    for bad in (dict(base=4), dict(base=-1), dict(from_end=2), dict(window=0), dict(window=65), dict(min_calls=9), dict(min_calls=-1), dict(gap=17), dict(gap=-1),
                dict(min_windows=0), dict(search=0), dict(min_bases=0), dict(max_sd=-1.0), dict(max_sd=float("nan"))):
        with pytest.raises(B.FFHipError):
            B.op_polytail(engine, x, S, path, 4, **bad)
    for args in ((x, 0, path, 4), (x, S, path[:1], 4), (x, S, np.where(path == 0, 8, path), 4), (x, S, np.where(path == 0, -1, path), 4), (x, S, path, 3), (x, S, path, 6)):
        with pytest.raises(B.FFHipError):
            B.op_polytail(engine, *args)
        with pytest.raises(B.FFHipError):
            B.op_polytail_windows(engine, *args)
    with pytest.raises(TypeError):
        B.op_polytail(engine, x, S, path, 4, windows=3)


# ------------------------------------------------------------------------------------ batches
RUN_A = dict(window=2, min_calls=1, max_sd=1e30, min_windows=1, gap=1, min_bases=1, search=10 ** 6)      # the flags are the path's alone
RUN_B = dict(window=8, min_calls=0, max_sd=1e-3, min_windows=2, gap=2, min_bases=1, search=10 ** 6)      # ... the signal's alone


def _signals(rng, lens):
    """noise with one repeated value over [200, 200 + n / 4) -- a whole number of RUN_B's windows and more"""
    out = []
    for n in lens:
        x = rng.standard_normal(int(n)).astype(np.float32)
        x[200:200 + int(n) // 4] = np.float32(0.3 + 0.01 * (int(n) % 7))
        out.append(x)
    return out


def _check_batches(B, bs, sigs, flags, where, temperature=1.0):
    """the batches (one, or a pair run together) without the flag, then with it under RUN_A and RUN_B, both ends: nothing else moves, and every record equals the
    restatement on the batch's own path and the signal it was given; every batch shows a tail with a rate"""
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
        for x in bs:
            x.finish()
    S, nbase = bs[0].dmodel.model.total_stride, bs[0].dmodel.model.nbase
    run(flags)
    before = [[_state(B, x, v, flags) for v in range(len(sigs[k]))] for k, x in enumerate(bs)]
    with pytest.raises(B.FFHipError):
        bs[0].polytail(0)                                     # a run without the flag made none
    records = {}
    for name, p in (("A", R.params(**RUN_A)), ("A end", R.params(**dict(RUN_A, from_end=1, base=1))), ("B", R.params(**RUN_B)), ("B end", R.params(**dict(RUN_B, from_end=1)))):
        for x in bs:
            x.set_polytail(**p)
        run(flags | B.RUN_POLYTAIL)
        for k, x in enumerate(bs):
            statuses = set()
            for v in range(len(sigs[k])):
                st, old = _state(B, x, v, flags), before[k][v]
                for key in st:
                    assert st[key] == old[key] if key in ("call", "qual") else np.array_equal(np.asarray(st[key]), np.asarray(old[key])), (where, k, v, key)
                got = x.polytail(v)
                R.check(got, R.record(sigs[k][v], S, st["path"], nbase, p), sigs[k][v], (where, name, k, v))
                statuses.add(int(got["status"]))
                records[(name, k, v)] = (st["path"].tobytes(), got.tobytes())
            assert 1 in statuses, (where, name, k, statuses)
        if name == "B":                                       # a second run gives the same bytes
            run(flags | B.RUN_POLYTAIL)
            for k, x in enumerate(bs):
                for v in range(len(sigs[k])):
                    assert x.polytail(v).tobytes() == records[(name, k, v)][1], (where, k, v)
    for x in bs:
        x.set_polytail(detach=True)
    with pytest.raises(B.FFHipError):                         # no parameters set
        bs[0].run(temperature, flags | B.RUN_POLYTAIL)
    with pytest.raises(B.FFHipError):
        bs[0].set_polytail(window=0)
    return records


def _packed(B, dm, rows, cap, sigs):
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    return pb


def _same_read_same_bytes(a, b, least):
    """records of the same signals from two batch shapes: where the two paths are the same bytes, so is every field but level"""
    same = 0
    for key in a:
        if key in b and a[key][0] == b[key][0]:
            ra, rb = np.frombuffer(a[key][1], R.POLYTAIL_DTYPE)[0], np.frombuffer(b[key][1], R.POLYTAIL_DTYPE)[0]
            for f in R.POLYTAIL_DTYPE.names:
                assert f == "level" or ra[f].tobytes() == rb[f].tobytes(), (key, f, ra, rb)
            same += 1
    assert same >= least, same


@pytest.mark.parametrize("kind,hidden", [(M.NET_LSTM5, 256), (M.NET_GRUMOD5, 256)])
def test_batch_records_rows_ragged_packed(B, engine, kind, hidden):
    dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
    rng = np.random.default_rng(hidden + kind)
    extra = B.RUN_MOVES | (B.RUN_MOD_PROBS if kind == M.NET_GRUMOD5 else 0)
    # one read a row, all of one length
    sigs = _signals(rng, [1500] * 16)
    b = B.Batch(dm, 16, 1500)
    b.set_signals(np.stack(sigs))
    _check_batches(B, [b], [sigs], B.RUN_NO_TRACE | extra, ("rows", kind))
    b.close()
    # ragged; then the same reads packed, by the default path and launch per step
    sigs = _signals(rng, list(rng.integers(900, 2001, 15)) + [6000])
    b = B.Batch(dm, 16, 6000)
    b.set_signals_ragged(sigs)
    ragged = _check_batches(B, [b], [sigs], B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE, ("ragged --viterbi", kind))
    b.close()
    pb = _packed(B, dm, 8, 8000, sigs)
    packed = _check_batches(B, [pb], [sigs], B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE, ("packed", kind))
    _check_batches(B, [pb], [sigs], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE | extra, ("packed per step", kind))
    pb.close()
    dm.close()
    _same_read_same_bytes(ragged, packed, 16)


def test_batch_records_paired_and_after_an_f32_rerun(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    sigs = [_signals(rng, [1500] * 16) for _ in range(2)]
    pair = []
    for k in range(2):
        b = B.Batch(dm, 16, 1500)
        b.set_signals(np.stack(sigs[k]))
        pair.append(b)
    _check_batches(B, pair, sigs, B.RUN_NO_TRACE, "pair")
    for b in pair:
        b.close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their records
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = _signals(rng, rng.integers(900, 2001, 16))
    sigs[1][100] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, [b], [sigs], 0, "rerun rows")
    assert b.f32_reruns() == 1
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, [pb], [sigs], B.RUN_MOVES, "rerun packed")
    assert pb.f32_reruns() == sum(1 for k in range(16) if slot[k] == slot[1]) >= 1
    pb.close()
    dm.close()


def test_exactly_one_more_copy_call(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(1)
    sigs = _signals(rng, [2000] * 8)
    b = B.Batch(dm, 8, 2000)
    b.set_signals(np.stack(sigs))
    psigs = _signals(rng, rng.integers(900, 2001, 24))
    pb = _packed(B, dm, 16, 4000, psigs)
    for x, nr in ((b, 8), (pb, 24)):
        x.set_polytail(**RUN_B)
        calls, held = {}, {}
        for fl in (B.RUN_POLYTAIL, 0, B.RUN_POLYTAIL):          # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            before = x.device_bytes() if fl and not held else None
            x.run(1.0, B.RUN_NO_TRACE | fl)
            x.finish()
            calls[fl] = _d2h_calls(B)
            if before is not None:
                held = {"grew": x.device_bytes() - before}
        assert calls[B.RUN_POLYTAIL][0] == calls[0][0] + 1, calls
        assert calls[B.RUN_POLYTAIL][1] == calls[0][1] + 32 * nr, calls       # ... of 32 bytes a read
        assert held["grew"] >= 32 * nr, held                                  # the device buffers are counted
        assert x.polytail(0).dtype == B.POLYTAIL_DTYPE == R.POLYTAIL_DTYPE
    with pytest.raises(B.FFHipError):                                         # not between a run and its finish
        b.run(1.0, B.RUN_NO_TRACE)
        try:
            b.set_polytail(**RUN_A)
        finally:
            b.finish()
    b.close()
    pb.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def _tags_of(rec, trim_start):
    if int(rec["status"]) != 1:
        return "pt:i:-1"
    first = trim_start + int(rec["first"])
    return "pt:i:%d\tpa:B:i,%d,%d\tpr:f:%.9g" % (math.floor(float(rec["bases"]) + 0.5), first, first + int(rec["count"]), rec["rate"])


def _paths_from_tags(call, mv_tag, ts, trim_start, nblock):
    """the paths that fit a record: the mv tag starts at the first block with a move and the k-th one is the k-th letter of the call; the base of the blocks in front
    of the first move is not in the record, so there is one path a base it may be"""
    f = mv_tag.split(",")
    stride, tail = int(f[1]), [int(v) for v in f[2:]]
    b0 = (ts - trim_start) // stride if tail else nblock
    mv = np.array([0] * b0 + tail)
    assert mv.size == nblock and int(mv.sum()) == len(call)
    out = []
    for lead in range(4):
        path, k = [lead], 0
        for b in range(nblock):
            if mv[b]:
                c = "ACGT".index(call[k])
                k += 1
                path.append(c if path[-1] != c else c + 4)
            else:
                path.append(path[-1])
        out.append(np.array(path, np.int32))
    return stride, out


def test_flappie_poly_tail(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, dump_trace, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    mdl = M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), mdl)
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 12
    names = ["uuid-%04d" % i for i in range(nread)]
    for i, n in enumerate(rng.integers(6000, 12000, nread)):
        x = rng.normal(500, 60, int(n))
        x[:300] = rng.normal(520, 4, 300)                     # (a head for the trimming to find)
        if i % 4 != 3:                                        # a flat stretch behind the head; every fourth read has none
            # (read 5: flat up to 200 samples from its end -- the last chunk of 100 is noise, so the trimming leaves the end alone -- with fewer than 50 blocks,
            # so fewer than --poly-tail-min-bases 50 moves, behind the tail)
            a, b = (int(n) - 1700, int(n) - 200) if i == 5 else (1000 + 40 * i, 1000 + 40 * i + 300 * (1 + i))
            x[a:b] = rng.normal(430, 1.5, max(0, min(b, int(n)) - a))
        write_fast5(reads / ("read_%02d.fast5" % i), names[i], np.clip(np.rint(x), 0, 8191).astype("<i2"))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16"] + args + [str(reads)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    def records(text, fmt="fastq"):
        """name -> (header json, call, tags behind the header / the mandatory fields)"""
        out = {}
        lines = text.split("\n")[:-1]
        if fmt == "sam":
            for line in lines:
                f = line.split("\t")
                out[f[0]] = (None, f[9], f[11:])
            return out
        for k in range(0, len(lines), 4):
            head, _, tags = lines[k].partition("\t")
            name, _, js = head[1:].partition("  ")
            out[name] = (json.loads(js), lines[k + 1], tags.split("\t"))
        return out

    def summary(err):
        return dict(re.findall(r"^polytail\t(\S+)\t(\S+)$", err, re.M))

    def want_summary(recs):
        vals = sorted(float(r["bases"]) for r in recs if int(r["status"]) == 1)
        return {"reads": str(len(recs)), "found": str(len(vals)), "no_rate": str(sum(int(r["status"]) == 3 for r in recs)),
                "median": "%.1f" % (float(np.median(np.array(vals, np.float64))) if vals else float("nan"))}

    trace = tmp_path / "trace.hdf5"
    plain = records(run(["--trace", str(trace), "--emit-moves"])[0])
    assert sorted(plain) == names
    # flags from the signal alone: everything the record needs is in the trace's signal, the mv tag and the call
    base_opts = ["--poly-tail", "--poly-tail-min-calls", "0", "--poly-tail-min-bases", "50"]
    out, err = run(base_opts + ["--emit-moves"])
    tagged = records(out)
    inputs, wants, statuses = {}, [], set()
    for name in names:
        js, call, tags = tagged[name]
        assert tags[:-3] == plain[name][2] or tags[:-1] == plain[name][2], name      # behind every other tag
        t = dict((v[:4], v[5:]) for v in tags)
        stride, paths = _paths_from_tags(call, t["mv:B"], int(t["ts:i"]), js["trim"][0], js["nblock"])
        x = dump_trace(trace, name)[0]
        inputs[name] = (x, stride, paths, js["trim"][0])
        p = R.params(min_calls=0, min_bases=50, search=20000 // (8 * stride))
        want = [R.record(x, stride, path, 4, p) for path in paths]
        assert len(set(w.tobytes() for w in want)) == 1, name                        # (min_calls 0: the unknown base plays no part)
        pt = [v for v in tags if v[:2] in ("pt", "pa", "pr")]
        assert "\t".join(pt) == _tags_of(want[0], js["trim"][0]) and tags[-len(pt):] == pt, (name, pt, want[0])
        wants.append(want[0])
        statuses.add(int(want[0]["status"]))
    assert statuses == {1, 2, 3}, statuses
    assert summary(err) == want_summary(wants), err
    pt_of = {name: [v for v in tagged[name][2] if v[:2] in ("pt", "pa", "pr")] for name in names}
    # the positions are raw samples whatever happens to the strings
    kit = tmp_path / "kit.fa"
    kit.write_text(">front\n%s\n>rear\n%s\n" % (tagged[names[0]][1][2:30], tagged[names[1]][1][-30:-2]))
    for opts, fmt in ((["--reverse"], "fastq"), (["--format", "sam"], "sam"), (["--adapters", str(kit), "--trim-adapters"], "fastq")):
        out, err2 = run(base_opts + opts)
        got = records(out, fmt)
        for name in names:
            assert got[name][2][-len(pt_of[name]):] == pt_of[name], (opts, name)
            assert len(got[name][2]) == len(pt_of[name]) + (2 if "--adapters" in opts else 0), (opts, name)
        assert summary(err2) == summary(err)
    assert records(run(base_opts + ["--reverse"])[0])[names[0]][1] == tagged[names[0]][1][::-1]
    # the defaults, a base at a time: the path's bases count; one of the four bases the blocks in front of the first move may have is the path's
    found = 0
    for letter in "ACGT":
        out, err = run(["--poly-tail", "--poly-tail-base", letter] + (["--poly-tail-end", "--poly-tail-search", "1000000"] if letter == "G" else []))
        got, recs = records(out), []
        for name in names:
            x, stride, paths, trim = inputs[name]
            p = R.params(base="ACGT".index(letter), **(dict(from_end=1, search=10 ** 6 // (8 * stride)) if letter == "G" else dict(search=20000 // (8 * stride))))
            want = {_tags_of(R.record(x, stride, path, 4, p), trim): R.record(x, stride, path, 4, p) for path in paths}
            text = "\t".join(got[name][2])
            assert text in want, (letter, name, text, list(want))
            recs.append(want[text])
            found += text != "pt:i:-1"
        s = summary(err)
        assert (s["reads"], s["found"], s["no_rate"]) == tuple(want_summary(recs)[k] for k in ("reads", "found", "no_rate")), (letter, err)
    assert found >= 1
