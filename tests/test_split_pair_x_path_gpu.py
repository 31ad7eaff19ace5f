"""The headline's layer kernel (k_lstm_split_pair<0, 3, 2, true>: the recurrent layers of two 256-read batches at H = 384 as one launch) held
to recorded bits.  Round 7 moved its x waves' input (x(t) of the projection Wi x) into pieces through two register buffers, the next step's
first piece in flight across the gate phase: the same products in the same order, so every score must be what the kernel gave before.

tests/golden/split_pair_h384_bits.json holds, per probe read, a digest of the transition scores' bytes, the base string and the quality
string, recorded by tests/golden/make_split_pair_bits.py from the kernel BEFORE that change -- ragged pairs (one read a row, both gate
levels: the LIVE = false instantiations) and packed pairs (several reads a row: the LIVE = true one).  Beside the bits: the same reads
against the f32-input MFMA kernel (FFHIP_RUN_F32_RNN) and a sample against the oracle."""
import hashlib
import json
import os

import numpy as np
import pytest

from flappie_amd import model as M
from oracle import ffo
from test_ragged_gpu import check_read

pytestmark = pytest.mark.gpu

HIDDEN, ROWS = 384, 256
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_pair_h384_bits.json")


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dm(B, engine):
    d = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1))
    yield d
    d.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def digest(b, r):
    h = hashlib.sha256(np.ascontiguousarray(b.transitions(r), dtype=np.float32).tobytes())
    h.update(b.basecall(r).encode())
    h.update(b.quality(r).encode())
    return h.hexdigest()[:20]


def ragged_signals(T=1200):
    """two batches of 256 reads, lengths T/2 .. T, a tenth of the slots empty (ragged pair: the tiles end at different steps)"""
    rng = np.random.default_rng(7384)
    out = []
    for _ in range(2):
        lens = rng.integers(T // 2, T + 1, ROWS)
        lens[rng.random(ROWS) < 0.1] = 0
        lens[0] = T
        out.append([rng.standard_normal(int(n)).astype(np.float32) for n in lens])
    return T, out


def run_ragged_pair(B, dm, flags):
    """-> the two batches (finished) and the probe reads of each"""
    T, sets = ragged_signals()
    bs = [B.Batch(dm, ROWS, T) for _ in range(2)]
    for b, sg in zip(bs, sets):
        b.set_signals_ragged(sg)
    bs[0].run_pair(bs[1], 1.0, flags)
    for b in bs:
        b.finish()
    probes = [[r for r in range(0, ROWS, 5) if len(sg[r]) > 0] for sg in sets]
    return bs, sets, probes


def packed_signals(cap=1500):
    rng = np.random.default_rng(11384)
    return cap, [[rng.standard_normal(int(n)).astype(np.float32) for n in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(900)), 25, cap - 50)]
                 for _ in range(2)]


def run_packed_pair(B, dm):
    """-> the two packed batches (finished), per batch the signals in packed order, and the probe positions"""
    cap, sets = packed_signals()
    bs, ordered = [], []
    for sigs in sets:
        pb = B.Batch(dm, ROWS, cap, max_reads=len(sigs))
        slot, off = pb.pack_plan([x.size for x in sigs])
        order = [i for i in range(len(sigs)) if slot[i] >= 0]
        pb.set_signals_packed([sigs[i] for i in order], [slot[i] for i in order], [off[i] for i in order])
        bs.append(pb)
        ordered.append([sigs[i] for i in order])
    bs[0].run_pair(bs[1])
    for pb in bs:
        pb.finish()
    probes = [list(range(0, len(o), 9)) for o in ordered]
    return bs, ordered, probes


def record(B, dm):
    """what tests/golden/make_split_pair_bits.py writes: the digests of the probe reads of every case below"""
    out = {}
    for name, flags in (("ragged_fast", 0), ("ragged_exact", B.RUN_EXACT_GATES)):
        bs, _, probes = run_ragged_pair(B, dm, flags)
        out[name] = [{str(r): digest(b, r) for r in pr} for b, pr in zip(bs, probes)]
        for b in bs:
            b.close()
    bs, _, probes = run_packed_pair(B, dm)
    out["packed"] = [{str(r): digest(b, r) for r in pr} for b, pr in zip(bs, probes)]
    for b in bs:
        b.close()
    return out


def _f32_scores(B, dm, sigs, T):
    """transition scores of the same reads through the f32-input MFMA layer kernel, one read a row"""
    b = B.Batch(dm, len(sigs), T)
    b.set_signals_ragged(sigs)
    b.run(1.0, B.RUN_F32_RNN)
    b.finish()
    res = [b.transitions(r).copy() for r in range(len(sigs))]
    b.close()
    return res


@pytest.mark.parametrize("gates", ["fast", "exact"])
def test_ragged_pair_keeps_its_bits(B, dm, golden, gates):
    bs, sets, probes = run_ragged_pair(B, dm, 0 if gates == "fast" else B.RUN_EXACT_GATES)
    try:
        for k, b in enumerate(bs):
            assert b.paired() and b.rnn_path() == 3
            want = golden["ragged_" + gates][k]
            assert sorted(int(r) for r in want) == probes[k]
            bad = [r for r in probes[k] if digest(b, r) != want[str(r)]]
            assert bad == [], (gates, k, bad)
        if gates == "fast":
            # the same reads through the f32 kernel (their own rows: the scores of a read do not depend on its neighbours)
            T = max(len(s) for s in sets[0])
            for k, b in enumerate(bs):
                sel = probes[k][:48]
                ref = _f32_scores(B, dm, [sets[k][r] for r in sel], T)
                assert max(float(np.abs(b.transitions(r) - x).max()) for r, x in zip(sel, ref)) <= 1e-4
            om = ffo.OracleModel(M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1))
            for k, r in ((0, 0), (1, probes[1][3])):
                check_read(bs[k], r, om.basecall(sets[k][r]))
    finally:
        for b in bs:
            b.close()


def test_packed_pair_keeps_its_bits(B, dm, golden):
    bs, ordered, probes = run_packed_pair(B, dm)
    try:
        for k, pb in enumerate(bs):
            assert pb.paired() and pb.rnn_path() == 3 and pb.nreads() > 2 * ROWS
            want = golden["packed"][k]
            assert sorted(int(r) for r in want) == probes[k]
            bad = [v for v in probes[k] if digest(pb, v) != want[str(v)]]
            assert bad == [], (k, bad)
            sel = probes[k][:48]
            ref = _f32_scores(B, dm, [ordered[k][v] for v in sel], max(ordered[k][v].size for v in sel))
            assert max(float(np.abs(pb.transitions(v) - x).max()) for v, x in zip(sel, ref)) <= 1e-4
        om = ffo.OracleModel(M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1))
        for k, v in ((0, probes[0][1]), (1, probes[1][7])):
            check_read(bs[k], v, om.basecall(ordered[k][v]))
    finally:
        for pb in bs:
            pb.close()
