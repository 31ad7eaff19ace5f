"""The dense layer kernels write their projection partials BEHIND barrier 1 (round 9): bits held against the kernel before the change.

Until round 9 the x waves of the dense forms (k_lstm_split_pair<0, 3, 2, true, ...>, k_lstm_split<0, 3, 2, true, ...>, k_lstm_split<0 | 1, 2, 2, true, ...>)
ended their projection of step i + 1 with a wait for a "consumed" word of their h wave and the write of px in front of barrier 1; now the accumulators cross the
barrier in registers and px(i + 1) is written behind it, without any flag.  Same products in the same order, same gate arithmetic: every score, base and quality
must be what the parent commit's release library gave -- from the release library, from the library with late waves (tools/test_hooks/libffhip_skew.so: one
wave in thirteen sits out a third of a step at every phase boundary, the two around the new write site included) and from the library that re-sweeps h(t-1) on
purpose (libffhip_resweep.so: the second pass reads px(i) again, which is why the write may not stand anywhere in front of barrier 1).

tests/golden/split_pair_px_order_bits.json holds one digest per 16 reads of every case of CASES below, recorded by tests/golden/make_split_pair_px_order_bits.py
from the PARENT commit's release library on an MI355X.  The cases are every affected instantiation a run can reach, at both gate levels (GL = 2 / 0) and
with LIVE = false / true (one read a row / packed rows):
  * the H = 384 pair: uniform, ragged (a whole tile empty: a group whose second tile is absent by length), packed, 240 rows (15 read tiles: the last group's
    second tile is absent by count), and the two SHORTEST batches a run accepts, four and five blocks (step 0 writes px(0) in front of the loop, the
    last step does not project).  The issue asked for batches of one and two blocks: no run reaches them -- a read shorter than the last convolution's
    window (19 samples at stride 5: four blocks) is outside the reference convolution's domain and ffhip_batch_create refuses it, so the layer kernels
    never see Tb < 4 with these models;
  * H = 384 alone in a 512-row launch (k_lstm_split<0, 3, 2, true>), ragged and packed;
  * H = 256, LSTM and GRUmod, in 768-row launches (k_lstm_split<0 | 1, 2, 2, true>), ragged and packed.
Each library runs in a process of its own (the binding loads one library a process)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from flappie_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_pair_px_order_bits.json")
RECORDER = os.path.join(ROOT, "tests", "golden", "make_split_pair_px_order_bits.py")
LIBS = {"release": None,
        "skew": os.path.join(ROOT, "tools", "test_hooks", "libffhip_skew.so"),
        "resweep": os.path.join(ROOT, "tools", "test_hooks", "libffhip_resweep.so")}

T = 600      # samples of the longest read of a case (120 blocks: 120 steps a layer)

# name -> (cell kind, hidden, rows a batch, batches as a pair, form of the input)
CASES = {
    "pair_uniform": (M.NET_LSTM5, 384, 256, True, "uniform"),
    "pair_ragged": (M.NET_LSTM5, 384, 256, True, "ragged"),
    "pair_packed": (M.NET_LSTM5, 384, 256, True, "packed"),
    "pair_15_tiles": (M.NET_LSTM5, 384, 240, True, "ragged"),
    "pair_4_blocks": (M.NET_LSTM5, 384, 256, True, "blocks4"),
    "pair_5_blocks": (M.NET_LSTM5, 384, 256, True, "blocks5"),
    "h384_512_ragged": (M.NET_LSTM5, 384, 512, False, "ragged"),
    "h384_512_packed": (M.NET_LSTM5, 384, 512, False, "packed"),
    "h256_768_ragged": (M.NET_LSTM5, 256, 768, False, "ragged"),
    "h256_768_packed": (M.NET_LSTM5, 256, 768, False, "packed"),
    "grumod256_768_ragged": (M.NET_GRUMOD5, 256, 768, False, "ragged"),
    "grumod256_768_packed": (M.NET_GRUMOD5, 256, 768, False, "packed"),
}
GATES = ("fast", "exact")


def _digests(b, nreads):
    """one digest per 16 reads (a read tile, where the reads stand one a row): transition scores' bytes, base string, quality string"""
    out = []
    for r0 in range(0, nreads, 16):
        h = hashlib.sha256()
        for r in range(r0, min(r0 + 16, nreads)):
            if b.read_nblock(r) <= 0:          # an empty row has no results
                h.update(b"-")
                continue
            h.update(np.ascontiguousarray(b.transitions(r), dtype=np.float32).tobytes())
            h.update(b.basecall(r).encode())
            h.update(b.quality(r).encode())
        out.append(h.hexdigest()[:16])
    return out


def _nsample_for_blocks(B, dm, rows, nblock):
    """the shortest batch of `nblock` blocks"""
    for ns in range(1, 64):
        try:
            b = B.Batch(dm, rows, ns)
        except B.FFHipError:
            continue
        nb = b.nblock
        b.close()
        if nb == nblock:
            return ns
    raise AssertionError("no batch length gives %d blocks" % nblock)


def run_case(B, dm, name, gates):
    """-> per batch of the case, its digests"""
    kind, hidden, rows, pair, form = CASES[name]
    rng = np.random.default_rng(9000 + sorted(CASES).index(name))
    flags = 0 if gates == "fast" else B.RUN_EXACT_GATES
    bs = []
    for _ in range(2 if pair else 1):
        if form == "uniform":
            b = B.Batch(dm, rows, T)
            b.set_signals(rng.standard_normal((rows, T)).astype(np.float32))
        elif form in ("blocks4", "blocks5"):
            nb = int(form[-1])
            ns = _nsample_for_blocks(B, dm, rows, nb)
            b = B.Batch(dm, rows, ns)
            assert b.nblock == nb
            b.set_signals(rng.standard_normal((rows, ns)).astype(np.float32))
        elif form == "ragged":
            lens = rng.integers(T // 4, T + 1, rows)
            lens[rng.random(rows) < 0.1] = 0
            lens[80:96] = 0          # read tile 5 is empty: its group runs with an absent second tile
            lens[0] = T
            b = B.Batch(dm, rows, T)
            b.set_signals_ragged([rng.standard_normal(int(n)).astype(np.float32) for n in lens])
        else:
            sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in np.clip(np.exp(np.log(120) + 0.7 * rng.standard_normal(4 * rows)), 25, T - 50)]
            b = B.Batch(dm, rows, T, max_reads=len(sigs))
            slot, off = b.pack_plan([x.size for x in sigs])
            keep = [i for i in range(len(sigs)) if slot[i] >= 0]
            assert len(keep) > 2 * rows
            b.set_signals_packed([sigs[i] for i in keep], [slot[i] for i in keep], [off[i] for i in keep])
        bs.append(b)
    if pair:
        bs[0].run_pair(bs[1], 1.0, flags)
    else:
        bs[0].run(1.0, flags)
    out = []
    for b in bs:
        b.finish()
        assert b.rnn_path() == 3 and b.paired() == pair, (name, gates, b.rnn_path(), b.paired())      # the split layer kernel, paired where the case says so
        out.append(_digests(b, b.nreads() if form == "packed" else rows))
        b.close()
    return out


def record(B):
    """what tests/golden/make_split_pair_px_order_bits.py writes: {"case/gates": [digests of batch 0, (digests of batch 1)]}, with the library the binding loaded"""
    eng = B.Engine(0)
    out = {}
    models = {}
    for name in CASES:
        kind, hidden = CASES[name][:2]
        if (kind, hidden) not in models:
            models[(kind, hidden)] = B.DeviceModel(eng, M.synthetic_model(kind, hidden, seed=1))
        for gates in GATES:
            out["%s/%s" % (name, gates)] = run_case(B, models[(kind, hidden)], name, gates)
    for dm in models.values():
        dm.close()
    eng.close()
    return out


@pytest.mark.gpu
def test_px_behind_barrier_1_keeps_the_parents_bits(tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(want) == sorted("%s/%s" % (n, g) for n in CASES for g in GATES)
    bad = []
    for tag, lib in LIBS.items():
        if lib is not None:
            assert os.path.exists(lib), "%s is missing: __graft_entry__.build() (make hooks) builds it" % os.path.relpath(lib, ROOT)
        env = dict(os.environ)
        env.pop("FFHIP_DEBUG", None)
        env.pop("FFHIP_BINDING_LIBRARY", None)
        if lib:
            env["FFHIP_BINDING_LIBRARY"] = lib
        out = str(tmp_path / (tag + ".json"))
        r = subprocess.run([sys.executable, RECORDER, out], env=env, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        with open(out) as f:
            got = json.load(f)
        assert sorted(got) == sorted(want), tag
        for key in sorted(want):
            assert [len(x) for x in got[key]] == [len(x) for x in want[key]], (tag, key)
            for k, (g, w) in enumerate(zip(got[key], want[key])):
                tiles = [i for i, (x, y) in enumerate(zip(g, w)) if x != y]
                if tiles:
                    bad.append((tag, key, k, tiles[:8]))
        print("%s library: %d cases, %d digests compared" % (tag, len(want), sum(len(x) for v in want.values() for x in v)))
    assert bad == [], "(library, case/gates, batch, groups of 16 reads that differ): %s" % bad
