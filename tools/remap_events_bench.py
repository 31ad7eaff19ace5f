#!/usr/bin/env python3
"""remap_events_bench.py -- what FFHIP_RUN_REMAP and FFHIP_RUN_REMAP | FFHIP_RUN_EVENTS cost a batch at the headline shape of bench.py: H = 384, 256 reads x 4000
samples, every read's sequence its own call, the default band 2048.

ffhip_batch_profile of one batch alone on the chip: the kernel time of the decode group (Viterbi, assembly and the decode extras: k_remap and k_events are there)
and of the whole batch, `--runs` profiled runs of each kind, alternating, after a warm-up of each; one JSON line with every figure and the medians.  --root names
the tree whose library is measured (default: this one); a tree without FFHIP_RUN_EVENTS measures the first two kinds only."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

NREAD, NSAMPLE, HIDDEN, BAND = 256, 4000, 384, 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1, ident="r941native"))
    rng = np.random.default_rng(20261018)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32))
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    seqs = [np.array(["ACGT".index(c) for c in b.basecall(v)] or [0], np.uint8) for v in range(NREAD)]
    b.set_remap(seqs, BAND)
    kinds = [("none", 0), ("remap", B.RUN_REMAP)]
    if hasattr(B, "RUN_EVENTS"):
        kinds.append(("remap_events", B.RUN_REMAP | B.RUN_EVENTS))
    eng.set_profiling(True)
    last = B.GROUP_NAMES[5]
    decode, total = {k: [] for k, _ in kinds}, {k: [] for k, _ in kinds}
    for it in range(args.runs + 1):                    # (the first round warms up and creates the buffers)
        for name, fl in kinds:
            b.run(1.0, B.RUN_NO_TRACE | fl)
            b.finish()
            p = b.profile()
            if it:
                decode[name].append(round(p[last]["ms"], 4))
                total[name].append(round(sum(g["ms"] for g in p.values() if isinstance(g, dict) and "ms" in g), 4))
    eng.set_profiling(False)
    mapped = sum(b.remap(v)["status"] == 1 for v in range(NREAD))
    out = {"metric": "H = 384, 256 reads x 4000 samples, one batch alone; sequences = the reads' own calls, band 2048; kernel time by ffhip_batch_profile",
           "mapped": int(mapped), "mean_bases": round(float(np.mean([q.size for q in seqs])), 1), "decode_group": last,
           "decode_group_ms": decode, "batch_ms": total,
           "median_decode_group_ms": {k: statistics.median(v) for k, v in decode.items()}, "median_batch_ms": {k: statistics.median(v) for k, v in total.items()}}
    print(json.dumps(out))
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
