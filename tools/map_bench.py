#!/usr/bin/env python3
"""map_bench.py -- what FFHIP_RUN_MAP costs a batch at the headline shape of bench.py: H = 384, 256 reads x 4000 samples.

ffhip_batch_profile (HIP events around the kernel groups of one run, on the run's own stream) of single runs without the flag, with it against a random reference
of 48 502 bases (lambda's size) and against one of 2^20 bases; the map's two kernels are launched in the last group (viterbi + assembly), so the group's time with
the flag less the same group's without it is theirs.  Then the rate of whole runs, one batch after the other, with and without the flag.  One JSON line;
profiles/r11_map_cost.txt keeps it.
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1, ident="r941native"))
    rng = np.random.default_rng(20261019)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32))
    refs = {"lambda_48502": B.MapRef(eng, ["".join("ACGT"[i] for i in rng.integers(0, 4, 48502))]),
            "max_1048576": B.MapRef(eng, ["".join("ACGT"[i] for i in rng.integers(0, 4, 1 << 20))])}
    out = {"shape": "H = 384, 256 reads x 4000 samples, one batch a run, window 4096", "groups_ms": {}, "msamples_per_s": {}}

    def one(flags):
        b.run(1.0, flags)
        b.finish()

    def profile(flags):
        eng.set_profiling(True)
        one(flags)
        rows = []
        for _ in range(args.runs):
            one(flags)
            p = b.profile()
            rows.append({k: round(v["ms"], 4) for k, v in p.items()})
        eng.set_profiling(False)
        return {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}      # the median run of each group

    def rate(flags):
        one(flags)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            one(flags)
        eng.synchronize()
        return round(args.steps * NREAD * NSAMPLE / (time.perf_counter() - t0) / 1e6, 3)

    base = B.RUN_NO_TRACE
    out["groups_ms"]["without"] = profile(base)
    out["msamples_per_s"]["without"] = rate(base)
    for name, ref in refs.items():
        b.set_map(ref)
        out["groups_ms"][name] = profile(base | B.RUN_MAP)
        out["msamples_per_s"][name] = rate(base | B.RUN_MAP)
        out["map_kernels_ms_" + name] = round(out["groups_ms"][name]["viterbi_assembly"] - out["groups_ms"]["without"]["viterbi_assembly"], 4)
    lens = [len(b.basecall(v)) for v in range(NREAD)]
    status = [b.map(v)["status"] for v in range(NREAD)]
    out["call_lengths"] = [int(np.min(lens)), int(np.mean(lens)), int(np.max(lens))]
    out["status_counts"] = [status.count(k) for k in range(4)]
    out["back_end_ms_without"] = round(sum(out["groups_ms"]["without"][k] for k in ("head_crf", "posterior", "viterbi_assembly")), 4)
    print(json.dumps(out))
    for ref in refs.values():
        ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
