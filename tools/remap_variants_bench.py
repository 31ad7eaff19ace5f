#!/usr/bin/env python3
"""remap_variants_bench.py -- what FFHIP_RUN_REMAP_VARIANTS costs a batch at bench.py's c2 shape: the LSTM flip-flop model, H = 384, 256 reads x 4000 samples,
every read's sequence its own call, the default band 2048, the default context 10, one SNP every 50 bases and one 1-base indel every 200 (insertion and deletion
in turn).

ffhip_batch_profile of one batch alone on the chip: the kernel time of the decode group (Viterbi, assembly and the decode extras: k_remap, k_site_starts and
k_variants are there) and of the whole batch, `--runs` profiled runs of each kind -- FFHIP_RUN_REMAP alone, with the flag in best-path mode, with the flag in
all-paths mode -- alternating in one process, after a warm-up of each; one JSON line with every figure and the medians.  --root names the tree whose library is
measured (default: this one); a tree without FFHIP_RUN_REMAP_VARIANTS measures FFHIP_RUN_REMAP alone."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

NREAD, NSAMPLE, HIDDEN, BAND, CONTEXT, SNP_EVERY, INDEL_EVERY = 256, 4000, 384, 2048, 10, 50, 200


def variants_of(B, q):
    """one SNP every SNP_EVERY bases, one 1-base indel every INDEL_EVERY (an insertion, then a deletion, in turn)"""
    out = [(p, 1, [(int(q[p]) + 1) % 4]) for p in range(SNP_EVERY // 2, q.size, SNP_EVERY)]
    for n, p in enumerate(range(INDEL_EVERY // 2 + 1, q.size, INDEL_EVERY)):
        out.append((p, 0, [(int(q[p]) + 2) % 4]) if n % 2 == 0 else (p, 1, []))
    return B.make_variants(sorted(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from flappie_amd import binding as B
    from flappie_amd import model as M
    eng = B.Engine(0)
    dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, HIDDEN, seed=1))
    rng = np.random.default_rng(20261018)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32))
    b.run(1.0, B.RUN_NO_TRACE)
    b.finish()
    seqs = [np.array(["ACGT".index(c) for c in b.basecall(v)] or [0], np.uint8) for v in range(NREAD)]
    b.set_remap(seqs, BAND)
    kinds = [("remap", B.RUN_REMAP, None)]
    have = hasattr(B, "RUN_REMAP_VARIANTS")
    if have:
        lists = [variants_of(B, q) if q.size > 1 else None for q in seqs]
        kinds += [("remap_variants_best", B.RUN_REMAP | B.RUN_REMAP_VARIANTS, False), ("remap_variants_all", B.RUN_REMAP | B.RUN_REMAP_VARIANTS, True)]
    eng.set_profiling(True)
    last = B.GROUP_NAMES[5]
    decode, total = {k: [] for k, _, _ in kinds}, {k: [] for k, _, _ in kinds}
    for it in range(args.runs + 1):                    # (the first round warms up and creates the buffers)
        for name, fl, mode in kinds:
            if mode is not None:
                b.set_remap_variants(lists, CONTEXT, mode)
            b.run(1.0, B.RUN_NO_TRACE | fl)
            b.finish()
            p = b.profile()
            if it:
                decode[name].append(round(p[last]["ms"], 4))
                total[name].append(round(sum(g["ms"] for g in p.values() if isinstance(g, dict) and "ms" in g), 4))
    eng.set_profiling(False)
    mapped = [v for v in range(NREAD) if b.remap(v)["status"] == 1]
    nvar = sum(lists[v].size for v in mapped if lists[v] is not None) if have else 0
    out = {"metric": "LSTM flip-flop H = 384, 256 reads x 4000 samples (bench.py c2), one batch alone; sequences = the reads' own calls, band 2048, context 10, "
                     "a SNP every 50 bases and a 1-base indel every 200; kernel time by ffhip_batch_profile",
           "mapped": len(mapped), "mean_bases": round(float(np.mean([q.size for q in seqs])), 1), "variants": int(nvar), "decode_group": last,
           "decode_group_ms": decode, "batch_ms": total,
           "median_decode_group_ms": {k: statistics.median(v) for k, v in decode.items()}, "median_batch_ms": {k: statistics.median(v) for k, v in total.items()}}
    print(json.dumps(out))
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
