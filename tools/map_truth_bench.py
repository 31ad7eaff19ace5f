#!/usr/bin/env python3
"""map_truth_bench.py -- what truth from map costs a batch at the headline shape of bench.py (H = 384, 256 reads x 4000 samples), against the two-run route it
replaces.

The reference has lambda's size (48 502 bases): random filler with the batch's own calls in it, 5 % edits, alternating strands, so that the reads map and k_truth
has work to do (a random reference leaves every read unmapped and the alignment empty).  Four ways of running the same batch, alternating, one batch after the other:
  none        no annotation
  map         FFHIP_RUN_MAP
  one_run     FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map
  two_runs    the route of --map --map-records, then --truth recs.fa: a run with FFHIP_RUN_MAP, the stretches cut on the host from the records, ffhip_batch_set_truth,
              and a second run with FFHIP_RUN_TRUTH
For each: the wall time of a batch (host clock around runs that end in a synchronise), the kernel groups of ffhip_batch_profile (HIP events on the run's stream; the
median run), and exposed_ms = the wall time less the recurrent group's, as bench.py defines it.  Then the device bytes the mode's sizing takes against exact sizing.
`--trace-only N` just runs the one-run mode N times: the command to put under `rocprofv3 --kernel-trace --stats` for the kernel times of k_map_stretch and k_truth.
One JSON line; profiles/r12_map_truth_cost.txt keeps it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NREAD, NSAMPLE, HIDDEN, REF_BASES, BAND = 256, 4000, 384, 48502, 512
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
WS_WORDS_A_ROW = {0: 2, 1: 8, 2: 40, 3: 80}


def edit(rng, s, rate):
    out = []
    for c in s:
        u = rng.random()
        if u < rate / 3:
            out.append("ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * rate / 3:
            out.append(c + "ACGT"[int(rng.integers(0, 4))])
        elif u >= rate:
            out.append(c)
    return "".join(out) or "A"


def reference_of(rng, calls):
    """lambda's size: as many of the calls as fit with 5 % edits, alternating strands, random filler between and behind them"""
    text, used = "", 0
    for i, c in enumerate(calls):
        x = edit(rng, c.replace("Z", "C"), 0.05)
        if len(text) + len(x) + 40 > REF_BASES:
            break
        text += "".join("ACGT"[k] for k in rng.integers(0, 4, 40)) + (x if i % 2 == 0 else "".join(COMP[ch] for ch in reversed(x)))
        used += 1
    return text + "".join("ACGT"[k] for k in rng.integers(0, 4, REF_BASES - len(text))), used


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
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
    b.set_map(ref)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    ys = [text, "".join(COMP[ch] for ch in reversed(text))]

    def stretches():
        out = []
        for v in range(NREAD):
            mp = b.map(v)
            out.append(np.array([code[c] for c in ys[mp["q"]][mp["tstart"]:mp["tend"]]], np.uint8) if mp["status"] == 1 else None)
        return out

    def mode_none():
        one(base)

    def mode_map():
        one(base | B.RUN_MAP)

    def mode_one_run():
        b.set_truth_from_map(True, BAND)
        one(base | B.RUN_MAP | B.RUN_TRUTH)

    def mode_two_runs():
        one(base | B.RUN_MAP)
        b.set_truth(stretches(), BAND)
        one(base | B.RUN_TRUTH)

    if args.trace_only:
        mode_one_run()
        for _ in range(args.trace_only):
            mode_one_run()
        status = [b.truth(v)["status"] for v in range(NREAD)]
        print(json.dumps({"trace_only_runs": args.trace_only, "truth_status_counts": [status.count(k) for k in range(3)]}))
        return
    modes = {"none": mode_none, "map": mode_map, "one_run": mode_one_run, "two_runs": mode_two_runs}
    out = {"shape": "H = 384, 256 reads x 4000 samples, one batch a run, reference of %d bases holding %d of the calls, window 4096, band %d" % (REF_BASES, used, BAND),
           "ms_per_batch": {k: [] for k in modes}, "groups_ms": {}, "exposed_ms": {}}
    for f in modes.values():                                  # every shape warm, every buffer grown
        f()
    for _ in range(args.rounds):                              # alternating, so that a drift of the box touches all four alike
        for name, f in modes.items():
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            eng.synchronize()
            out["ms_per_batch"][name].append(round((time.perf_counter() - t0) / args.steps * 1e3, 4))
    eng.set_profiling(True)
    for name, flags in (("none", base), ("map", base | B.RUN_MAP), ("one_run", base | B.RUN_MAP | B.RUN_TRUTH)):
        if name == "one_run":
            b.set_truth_from_map(True, BAND)
        one(flags)
        rows = []
        for _ in range(args.runs):
            one(flags)
            rows.append({k: round(v["ms"], 4) for k, v in b.profile().items()})
        out["groups_ms"][name] = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}
    b.set_truth(stretches(), BAND)                            # (the records of the run before are the mode's: the same)
    one(base | B.RUN_TRUTH)
    rows = []
    for _ in range(args.runs):
        one(base | B.RUN_TRUTH)
        rows.append({k: round(v["ms"], 4) for k, v in b.profile().items()})
    out["groups_ms"]["second_run_of_two"] = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}
    eng.set_profiling(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in out["ms_per_batch"].items()}
    out["ms_per_batch_median"] = med
    rec = {k: out["groups_ms"][k]["recurrent"] for k in ("none", "map", "one_run")}
    out["exposed_ms"] = {"none": round(med["none"] - rec["none"], 4), "map": round(med["map"] - rec["map"], 4), "one_run": round(med["one_run"] - rec["one_run"], 4),
                         "two_runs": round(med["two_runs"] - rec["map"] - out["groups_ms"]["second_run_of_two"]["recurrent"], 4)}
    out["truth_kernels_ms_one_run"] = round(out["groups_ms"]["one_run"]["viterbi_assembly"] - out["groups_ms"]["map"]["viterbi_assembly"], 4)
    # what the sizing takes
    mode_one_run()
    tr = [b.truth(v) for v in range(NREAD)]
    lens = [len(c) for c in calls]
    nb = [b.read_nblock(v) for v in range(NREAD)]
    words = [WS_WORDS_A_ROW[B.truth_form(min(2 * BAND + 1, n + 2))] for n in nb]
    out["call_lengths"] = [int(np.min(lens)), int(np.mean(lens)), int(np.max(lens))]
    out["blocks"] = [int(np.min(nb)), int(np.max(nb))]
    out["truth_status_counts"] = [[t["status"] for t in tr].count(k) for k in range(3)]
    out["workspace_bytes_bound"] = int(sum(8 * w * B.map_truth_bound(n, 250) for w, n in zip(words, nb)))
    out["workspace_bytes_exact"] = int(sum(8 * w * t["m"] for w, t in zip(words, tr)))
    out["truths_and_ops_bytes_bound"] = int(sum(2 * B.map_truth_bound(n, 250) + n + 1 for n in nb))
    out["truths_and_ops_bytes_exact"] = int(sum(2 * t["m"] + n + 1 for t, n in zip(tr, nb) if t["m"]))
    out["device_bytes"] = b.device_bytes()
    print(json.dumps(out))
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
