#!/usr/bin/env python3
"""polytail_bench.py -- what FFHIP_RUN_POLYTAIL costs, from ffhip_batch_profile on one build: the milliseconds of a batch's group 5 (Viterbi, assembly and the
products behind them, k_polytail among them) and of the whole batch, once with and once without the flag, for
  * the headline shape of bench.py: H = 384, 256 reads x 4000 samples, one read a row;
  * a packed batch that holds a 200 000-sample read among ordinary ones (5000 windows at the defaults: the scans' longest chain).
Every signal carries a flat stretch, so that the kernel finds a tail and runs its last phase.  Each figure is the median of --runs profiled runs after a warm-up
of each kind, alternated in one process.  One JSON line; profiles/r07_polytail.txt keeps it."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN = 384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1, ident="r941native"))
    rng = np.random.default_rng(20261018)

    def signal(n):
        x = rng.standard_normal(n).astype(np.float32)
        x[n // 10:n // 10 + n // 5] = 0.25
        return x

    def measure(b, nsample):
        b.set_polytail(min_calls=0)
        res = {}
        for fl in (B.RUN_POLYTAIL, 0):
            b.run(1.0, fl)
            b.finish()
        eng.set_profiling(True)
        ms = {B.RUN_POLYTAIL: [], 0: []}
        for _ in range(args.runs):
            for fl in (B.RUN_POLYTAIL, 0):
                b.run(1.0, fl)
                b.finish()
                p = b.profile()
                ms[fl].append((p["viterbi_assembly"]["ms"], sum(g["ms"] for g in p.values()), p["viterbi_assembly"]["launches"]))
        eng.set_profiling(False)
        for fl, key in ((B.RUN_POLYTAIL, "with_flag"), (0, "without_flag")):
            a = np.array(ms[fl])
            res[key] = {"group5_ms": round(float(np.median(a[:, 0])), 4), "batch_ms": round(float(np.median(a[:, 1])), 4), "group5_launches": int(a[0, 2])}
        b.run(1.0, B.RUN_POLYTAIL)
        b.finish()
        res["status_1"] = int(sum(int(b.polytail(v)["status"]) == 1 for v in range(b.nreads())))
        res["samples"] = int(nsample)
        return res

    out = {"metric": "ffhip_batch_profile, ms a batch, H = 384; median of %d runs" % args.runs}
    b = B.Batch(dm, 256, 4000)
    b.set_signals(np.stack([signal(4000) for _ in range(256)]))
    out["headline_256x4000"] = measure(b, 256 * 4000)
    b.close()
    lens = [200000] + [int(n) for n in rng.integers(2000, 8001, 127)]
    sigs = [signal(n) for n in lens]
    pb = B.Batch(dm, 16, 220000, max_reads=len(sigs))      # (room for the long read and the gap behind it)
    slot, off = pb.pack_plan(lens)
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    out["packed_with_a_200000_sample_read"] = measure(pb, sum(lens))
    pb.close()
    print(json.dumps(out))
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
