#!/usr/bin/env python3
"""remap_mods_bench.py -- what FFHIP_RUN_REMAP_MODS costs a batch at bench.py's c4 shape, the r941_5mC shape: GRUmod, H = 256, 1024 reads x 4000 samples, every
read's sequence its own call, the default band 2048, the default context 15.

ffhip_batch_profile of one batch alone on the chip: the kernel time of the decode group (Viterbi, assembly and the decode extras: k_remap, k_site_starts and
k_site_mods are there) and of the whole batch, `--runs` profiled runs of each kind -- FFHIP_RUN_REMAP alone, with the flag in best-path mode, with the flag in
all-paths mode -- alternating in one process, after a warm-up of each; one JSON line with every figure and the medians.  --root names the tree whose library is
measured (default: this one); a tree without FFHIP_RUN_REMAP_MODS measures FFHIP_RUN_REMAP alone."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

NREAD, NSAMPLE, HIDDEN, BAND, CONTEXT = 1024, 4000, 256, 2048, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_GRUMOD5, HIDDEN, seed=1, ident="r941native5mC"))
    rng = np.random.default_rng(20261018)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32))
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    seqs = [np.array(["ACGTZ".index(c) for c in b.basecall(v)] or [0], np.uint8) for v in range(NREAD)]
    b.set_remap(seqs, BAND)
    kinds = [("remap", B.RUN_REMAP, None)]
    if hasattr(B, "RUN_REMAP_MODS"):
        kinds += [("remap_mods_best", B.RUN_REMAP | B.RUN_REMAP_MODS, False), ("remap_mods_all", B.RUN_REMAP | B.RUN_REMAP_MODS, True)]
    eng.set_profiling(True)
    last = B.GROUP_NAMES[5]
    decode, total = {k: [] for k, _, _ in kinds}, {k: [] for k, _, _ in kinds}
    for it in range(args.runs + 1):                    # (the first round warms up and creates the buffers)
        for name, fl, mode in kinds:
            if mode is not None:
                b.set_remap_mods(CONTEXT, mode)
            b.run(1.0, B.RUN_NO_TRACE | fl)
            b.finish()
            p = b.profile()
            if it:
                decode[name].append(round(p[last]["ms"], 4))
                total[name].append(round(sum(g["ms"] for g in p.values() if isinstance(g, dict) and "ms" in g), 4))
    eng.set_profiling(False)
    mapped = sum(b.remap(v)["status"] == 1 for v in range(NREAD))
    sites = sum(int(np.isin(q, (1, 4)).sum()) for v, q in enumerate(seqs) if b.remap(v)["status"] == 1)
    out = {"metric": "GRUmod H = 256, 1024 reads x 4000 samples (bench.py c4), one batch alone; sequences = the reads' own calls, band 2048, context 15; "
                     "kernel time by ffhip_batch_profile",
           "mapped": int(mapped), "mean_bases": round(float(np.mean([q.size for q in seqs])), 1), "sites": int(sites), "decode_group": last,
           "decode_group_ms": decode, "batch_ms": total,
           "median_decode_group_ms": {k: statistics.median(v) for k, v in decode.items()}, "median_batch_ms": {k: statistics.median(v) for k, v in total.items()}}
    print(json.dumps(out))
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
