#!/usr/bin/env python3
"""consensus_bench.py -- what FFHIP_RUN_CONSENSUS costs a batch at the headline shape of bench.py (H = 384, 256 reads x 4000 samples), against the same run without
it, and what the one call at the run's end costs.

Shape and reference are those of tools/map_truth_bench.py and tools/pileup_bench.py: a reference of lambda's size (48 502 bases) of random filler with the batch's
own calls in it, 5 % edits, alternating strands, so that the reads map, k_truth aligns them and k_consensus has ops to count.  Two ways of running the same batch,
alternating, one batch after the other:
  without     FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map (the code path of the build before the flag)
  with        the same with FFHIP_RUN_CONSENSUS into one consensus
For each: the wall time of a batch (host clock around `steps` runs that end in a synchronise of the engine, so that the last batch's unwaited-for k_consensus is
inside), every round's figure, their median and their spread.  Then what one batch counted, and ffhip_consensus_call -- one launch of k_consensus_call and the
download of 16 bytes a position -- on a host clock, `calls` times.  `--trace-only N` just runs the `with` mode N times and calls once: the command to put under
`rocprofv3 --kernel-trace --stats` for the two kernels' own times beside k_truth's.  One JSON line; profiles/r17_consensus_cost.txt keeps it.
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

MIN_DEPTH = 1                                                # every read lies once on this reference: at the default 3 nothing would be called


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
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
    cons = B.Consensus(eng, ref)
    b.set_map(ref)
    b.set_truth_from_map(True, BAND)
    b.set_consensus(cons)
    modes = {"without": base | B.RUN_MAP | B.RUN_TRUTH, "with": base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_CONSENSUS}
    if args.trace_only:
        one(modes["with"])
        for _ in range(args.trace_only):
            one(modes["with"])
        cells = cons.call(MIN_DEPTH)
        print(json.dumps({"trace_only_runs": args.trace_only, "totals": cons.download()[1], "called": int((cells["what"] != 0).sum())}))
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
    out["ms_per_batch_min_max"] = {k: [min(v), max(v)] for k, v in out["ms_per_batch"].items()}
    out["consensus_ms_per_batch"] = round(med["with"] - med["without"], 4)
    # what one batch adds
    cons.reset()
    one(modes["with"])
    counts, totals = cons.download()
    out["totals_of_one_batch"] = totals
    out["atomics_of_one_batch"] = int(counts.astype(np.int64).sum())
    out["atomics_by_minor_column"] = [int(counts[5 + 4 * d:9 + 4 * d].astype(np.int64).sum()) for d in range(B.CONSENSUS_MINOR)]
    out["positions"] = cons.positions
    depth = counts[:5].astype(np.int64).sum(axis=0)
    out["covered"] = int((depth >= 1).sum())
    out["deepest"] = int(depth.max())
    # the call: one launch and 16 bytes a position down, on the host's clock
    cons.call(MIN_DEPTH)
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        cells = cons.call(MIN_DEPTH)
        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
    out["call_ms"] = {"median": sorted(ms)[len(ms) // 2], "min": min(ms), "max": max(ms), "bytes_down": int(cells.nbytes), "min_depth": MIN_DEPTH}
    kind = cells["what"].astype(int) & 3
    out["cells_of_one_batch"] = {"called": int((kind != 0).sum()), "same": int((kind == 1).sum()), "sub": int((kind == 2).sum()), "del": int((kind == 3).sum()),
                                 "with_inserted_letters": int(((cells["what"].astype(int) & 4) != 0).sum()), "letters": int(cells["n"].astype(int).sum())}
    print(json.dumps(out))
    cons.close()
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
