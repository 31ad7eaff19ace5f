#!/usr/bin/env python3
"""modpileup_bench.py -- what FFHIP_RUN_MOD_PILEUP costs a batch at the 5mC shape of bench.py --config c4 (GRUmod5, H = 256, 1024 reads x 4000 samples, 2000 blocks
a read), against the same run without it.

The reference is built as tools/map_truth_bench.py builds its own, but from this batch's calls and 200 000 bases long: random filler with as many of the calls in
it as fit, 5 % edits, alternating strands, so that those reads map, k_truth aligns them and k_modpileup has ops on sites to count.  Two ways of running the same
batch, alternating, one batch after the other:
  without     FFHIP_RUN_MAP | FFHIP_RUN_TRUTH | FFHIP_RUN_MOD_PROBS in the mode of ffhip_batch_set_truth_from_map (the code path of the build before the flag)
  with        the same with FFHIP_RUN_MOD_PILEUP into one mod pileup
For each: the wall time of a batch (host clock around `steps` runs that end in a synchronise of the engine, so that the last batch's unwaited-for k_modpileup is
inside), every round's figure, their median and their spread.  Then what was counted.  `--trace-only N` just runs the `with` mode N times: the command to put under
`rocprofv3 --kernel-trace --stats` for k_modpileup's own time beside k_truth's.  One JSON line; profiles/r16_modpileup_cost.txt keeps it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import map_truth_bench as MT      # noqa: E402  (the same reference construction)

NREAD, NSAMPLE, HIDDEN, REF_BASES, BAND = 1024, 4000, 256, 200000, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", type=int, default=0)
    args = ap.parse_args()
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_GRUMOD5, HIDDEN, seed=1, ident="r941native5mC"))
    rng = np.random.default_rng(20261021)
    sig = rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(sig)
    base = B.RUN_NO_TRACE

    def one(flags):
        b.run(1.0, flags)
        b.finish()

    one(base)
    calls = [b.basecall(v) for v in range(NREAD)]
    MT.REF_BASES = REF_BASES
    text, used = MT.reference_of(rng, calls)
    ref = B.MapRef(eng, [text])
    pile = B.ModPileup(eng, ref)                               # the default thresholds, 50 and 205
    b.set_map(ref)
    b.set_truth_from_map(True, BAND)
    b.set_modpileup(pile)
    without = base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_MOD_PROBS
    modes = {"without": without, "with": without | B.RUN_MOD_PILEUP}
    if args.trace_only:
        one(modes["with"])
        for _ in range(args.trace_only):
            one(modes["with"])
        print(json.dumps({"trace_only_runs": args.trace_only, "totals": pile.download()[1]}))
        return
    out = {"shape": "GRUmod5 H = %d, %d reads x %d samples, one batch a run, reference of %d bases holding %d of the calls, window 4096, band %d, lo 50, hi 205"
                    % (HIDDEN, NREAD, NSAMPLE, REF_BASES, used, BAND),
           "ms_per_batch": {k: [] for k in modes}}
    for fl in modes.values():                                 # every shape warm, every buffer grown
        one(fl)
    for _ in range(args.rounds):                              # alternating, so that a drift of the box touches both alike
        for name, fl in modes.items():
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one(fl)
            eng.synchronize()
            out["ms_per_batch"][name].append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
    med = {k: sorted(v)[len(v) // 2] for k, v in out["ms_per_batch"].items()}
    out["ms_per_batch_median"] = med
    out["ms_per_batch_min_max"] = {k: [min(v), max(v)] for k, v in out["ms_per_batch"].items()}
    out["modpileup_ms_per_batch"] = round(med["with"] - med["without"], 4)
    # what one batch adds
    pile.reset()
    one(modes["with"])
    counts, totals, hist = pile.download()
    out["totals_of_one_batch"] = totals
    out["atomics_of_one_batch"] = int(counts.astype(np.int64).sum())
    out["histogram_bins_in_use"] = int((hist > 0).sum())
    out["positions"] = pile.positions
    depth = counts.astype(np.int64).sum(axis=0)
    out["sites_covered"] = int((depth >= 1).sum())
    out["deepest"] = int(depth.max())
    print(json.dumps(out))
    pile.close()
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
