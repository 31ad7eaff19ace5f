#!/usr/bin/env python3
"""truth_bench.py -- what FFHIP_RUN_TRUTH costs at the headline shape of bench.py: H = 384, 256 reads x 4000 samples, paired runs (ffhip_batch_run_pair).

Every read's truth is its own call with a substitution, an insertion and a deletion planted every 25 bases (about 88 % identity), the band the default 512.  One
process makes three timed runs with the flag and three without, alternating, after a warm-up of each, and prints one JSON line: the rates in Msamples/s and the
wall time per step (one batch) of each kind, and the decode group's kernel time (ffhip_batch_profile, group 5: Viterbi, assembly and the decode extras) of single
profiled runs with and without the flag, whose difference is k_truth's own time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NREAD, NSAMPLE, HIDDEN, BAND = 256, 4000, 384, 512


def edited(rng, codes):
    q = []
    for k, c in enumerate(codes):
        if k % 25 == 5:
            c = (int(c) + 1) % 4
        if k % 25 == 12:
            continue
        q.append(int(c))
        if k % 25 == 20:
            q.append(int(rng.integers(0, 4)))
    return np.array(q if q else [0], np.uint8)


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
    rng = np.random.default_rng(20261018)
    sig = rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32)
    batches = [B.Batch(dm, NREAD, NSAMPLE) for _ in range(4)]      # two pairs in flight, as bench.py's headline leg
    for b in batches:
        b.set_signals(sig)
    batches[0].run(1.0, 0)
    batches[0].finish()
    calls = [batches[0].basecall(v) for v in range(NREAD)]
    truths = [edited(rng, ["ACGT".index(c) for c in call]) for call in calls]
    for b in batches:
        b.set_truth(truths, BAND)

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
        return time.perf_counter() - t0

    for flags in (B.RUN_TRUTH, 0):
        run_steps(args.warmup, flags)
    secs = {"with": [], "without": []}
    for _ in range(args.runs):
        secs["with"].append(timed(B.RUN_TRUTH))
        secs["without"].append(timed(0))
    # the records: behind a run WITH the flag (the last timed run had none, and ffhip_batch_truth refuses a run that made no records)
    batches[0].run_pair(batches[1], 1.0, B.RUN_TRUTH)
    for b in batches[:2]:
        b.finish()
    rec = [batches[0].truth(v) for v in range(NREAD)]
    paired = bool(batches[0].paired())
    # the decode group's kernel time of one batch alone on the chip
    eng.set_profiling(True)
    group = {}
    for name, flags in (("with", B.RUN_TRUTH), ("without", 0), ("with2", B.RUN_TRUTH), ("without2", 0)):
        batches[0].run(1.0, flags)
        batches[0].finish()
        group[name] = batches[0].profile()
    eng.set_profiling(False)
    last = B.GROUP_NAMES[5]

    def rate(s):
        return round(args.steps * NREAD * NSAMPLE / s / 1e6, 3)
    out = {"metric": "H = 384, 256 reads x 4000 samples, paired runs; a truth per read (its call with 12 % planted edits), band 512", "paired": paired,
           "mean_call_bases": round(float(np.mean([len(c) for c in calls])), 1), "mean_truth_bases": round(float(np.mean([t.size for t in truths])), 1),
           "aligned": int(sum(r["status"] == 1 for r in rec)), "mean_identity": round(float(np.mean([r["n_match"] / max(1, r["dist"] + r["n_match"]) for r in rec])), 4),
           "form": int(B.truth_form(min(2 * BAND + 1, batches[0].read_nblock(0) + 2))),
           "msamples_with": [rate(s) for s in secs["with"]], "msamples_without": [rate(s) for s in secs["without"]],
           "ms_per_step_with": [round(1e3 * s / args.steps, 4) for s in secs["with"]], "ms_per_step_without": [round(1e3 * s / args.steps, 4) for s in secs["without"]],
           "decode_group": last, "decode_group_ms": {k: round(v[last]["ms"], 4) for k, v in group.items()},
           "decode_group_launches": {k: v[last]["launches"] for k, v in group.items()}}
    print(json.dumps(out))
    for b in batches:
        b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
