#!/usr/bin/env python3
"""pileup_bench.py -- what FFHIP_RUN_PILEUP costs a batch at the headline shape of bench.py (H = 384, 256 reads x 4000 samples), against the same run without it.

Shape and reference are those of tools/map_truth_bench.py: a reference of lambda's size (48 502 bases) of random filler with the batch's own calls in it, 5 % edits,
alternating strands, so that the reads map, k_truth aligns them and k_pileup has ops to count.  Two ways of running the same batch, alternating, one batch after
the other:
  without     FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map
  with        the same with FFHIP_RUN_PILEUP into one pileup
For each: the wall time of a batch (host clock around `steps` runs that end in a synchronise of the engine, so that the last batch's unwaited-for k_pileup is inside),
the median over `rounds`.  Then what was counted.  `--trace-only N` just runs the `with` mode N times: the command to put under `rocprofv3 --kernel-trace --stats`
for k_pileup's own time beside k_truth's.  One JSON line; profiles/r13_pileup_cost.txt keeps it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_truth_bench import BAND, HIDDEN, NREAD, NSAMPLE, REF_BASES, reference_of      # noqa: E402  (the same shape and reference construction)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", type=int, default=0)
    args = ap.parse_args()
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1, ident="r941native"))
    rng = np.random.default_rng(20261019)
    sig = rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(sig)
    base = B.RUN_NO_TRACE

    def one(flags):
        b.run(1.0, flags)
        b.finish()

    one(base)
    calls = [b.basecall(v) for v in range(NREAD)]
    text, used = reference_of(rng, calls)
    ref = B.MapRef(eng, [text])
    pile = B.Pileup(eng, ref)
    b.set_map(ref)
    b.set_truth_from_map(True, BAND)
    b.set_pileup(pile)
    modes = {"without": base | B.RUN_MAP | B.RUN_TRUTH, "with": base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP}
    if args.trace_only:
        one(modes["with"])
        for _ in range(args.trace_only):
            one(modes["with"])
        print(json.dumps({"trace_only_runs": args.trace_only, "totals": pile.download()[1]}))
        return
    out = {"shape": "H = 384, 256 reads x 4000 samples, one batch a run, reference of %d bases holding %d of the calls, window 4096, band %d" % (REF_BASES, used, BAND),
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
    out["pileup_ms_per_batch"] = round(med["with"] - med["without"], 4)
    # what one batch adds
    pile.reset()
    one(modes["with"])
    counts, totals = pile.download()
    out["totals_of_one_batch"] = totals
    out["atomics_of_one_batch"] = int(counts.astype(np.int64).sum())
    out["ops_a_counted_read"] = round((totals["match"] + totals["mismatch"] + totals["del"] + totals["ins"] + totals["edge_ins"]) / max(totals["reads"], 1), 1)
    out["positions"] = pile.positions
    out["covered"] = int((counts[:, :5].astype(np.int64).sum(axis=(0, 1)) >= 1).sum())
    out["deepest"] = int(counts[:, :5].astype(np.int64).sum(axis=(0, 1)).max())
    print(json.dumps(out))
    pile.close()
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
