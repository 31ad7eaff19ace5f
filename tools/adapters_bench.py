#!/usr/bin/env python3
"""adapters_bench.py -- what FFHIP_RUN_ADAPTERS costs at the headline shape of bench.py: H = 384, 256 reads x 4000 samples, paired runs (ffhip_batch_run_pair).

The kit has 8 patterns of 28 bases (16 searches a read, anywhere in the call).  One process makes three timed runs with the flag and three without, alternating, after a warm-up
of each, and prints one JSON line: the six rates in Msamples/s, the mean of each kind and the spread of the runs without the flag.  k_adapters' own time comes
from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/adapters_bench.py), in a run of its own; profiles/r10_adapters_cost.txt keeps both.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NREAD, NSAMPLE, HIDDEN = 256, 4000, 384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="batches a timed run (an even number: they run in pairs)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1, ident="r941native"))
    rng = np.random.default_rng(20260928)
    sig = rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32)
    kit = B.Adapters(eng, ["".join("ACGT"[i] for i in rng.integers(0, 4, 28)) for _ in range(8)])
    batches = [B.Batch(dm, NREAD, NSAMPLE) for _ in range(4)]      # two pairs in flight, as bench.py's headline leg
    for b in batches:
        b.set_signals(sig)
        b.set_adapters(kit)

    def run_steps(n, flags):
        pending = []
        for i in range(0, n, 2):
            k = (i // 2) % 2
            b0, b1 = batches[2 * k], batches[2 * k + 1]
            if len(pending) == 2:
                for b in pending.pop(0):
                    b.finish()
            b0.run_pair(b1, 1.0, flags)
            pending.append((b0, b1))
        for bs in pending:
            for b in bs:
                b.finish()

    def timed(flags):
        eng.synchronize()
        t0 = time.perf_counter()
        run_steps(args.steps, flags)
        eng.synchronize()
        return args.steps * NREAD * NSAMPLE / (time.perf_counter() - t0) / 1e6

    base = 0                              # (bench.py's own flags)
    for flags in (base | B.RUN_ADAPTERS, base):
        run_steps(args.warmup, flags)
    rates = {"with": [], "without": []}
    for _ in range(args.runs):
        rates["with"].append(timed(base | B.RUN_ADAPTERS))
        rates["without"].append(timed(base))
    lens = [len(batches[0].basecall(v)) for v in range(NREAD)]      # the columns k_adapters walks
    out = {"metric": "Msamples/s basecalled, H = 384, 256 reads x 4000 samples, paired runs; kit of 8 x 28 bases", "paired": bool(batches[0].paired()),
           "with_flag": [round(x, 3) for x in rates["with"]], "without_flag": [round(x, 3) for x in rates["without"]],
           "mean_with": round(float(np.mean(rates["with"])), 3), "mean_without": round(float(np.mean(rates["without"])), 3),
           "spread_without": [round(min(rates["without"]), 3), round(max(rates["without"]), 3)],
           "inside_spread": bool(min(rates["without"]) <= float(np.mean(rates["with"])) <= max(rates["without"]))}
    out["call_lengths"] = [int(np.min(lens)), int(np.mean(lens)), int(np.max(lens))]
    print(json.dumps(out))
    for b in batches:
        b.close()
    kit.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
