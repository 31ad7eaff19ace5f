#!/usr/bin/env python3
"""map_remap_bench.py -- what remap from map costs a batch at the headline shape of bench.py (H = 384, 256 reads x 4000 samples), against the two-run route it
replaces.

The reference has lambda's size (48 502 bases): random filler with the batch's own calls in it, 5 % edits, alternating strands, so that the reads map and k_remap
has work to do (a random reference leaves every read unmapped and the mapping empty).  Four ways of running the same batch, alternating, one batch after the other:
  none        no annotation
  map         FFHIP_RUN_MAP
  one_run     FFHIP_RUN_MAP | FFHIP_RUN_REMAP | FFHIP_RUN_EVENTS in the mode of ffhip_batch_set_remap_from_map
  two_runs    the route of --map --map-records, then --remap recs.fa --remap-events: a run with FFHIP_RUN_MAP, the stretches cut on the host from the records,
              ffhip_batch_set_remap, and a second run with FFHIP_RUN_REMAP | FFHIP_RUN_EVENTS
For each: the wall time of a batch (host clock around runs that end in a synchronise), the kernel groups of ffhip_batch_profile (HIP events on the run's stream; the
median run), and exposed_ms = the wall time less the recurrent group's, as bench.py defines it.  Then what sizing by N + 1 takes against exact sizing.
`--trace-only N` just runs the one-run mode N times: the command to put under `rocprofv3 --kernel-trace --stats` for the kernel times of k_map_remap_seq beside
k_remap and k_map_scan.  One JSON line; profiles/r19_map_remap_cost.txt keeps it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NREAD, NSAMPLE, HIDDEN, REF_BASES, BAND = 256, 4000, 384, 48502, 2048
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
WS_WORDS_A_BLOCK = {0: 1, 1: 4, 2: 16, 3: 72}


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
    rng = np.random.default_rng(20261021)
    sig = rng.standard_normal((NREAD, NSAMPLE)).astype(np.float32)
    b = B.Batch(dm, NREAD, NSAMPLE)
    b.set_signals(sig)
    base = B.RUN_NO_TRACE
    mapped = B.RUN_REMAP | B.RUN_EVENTS

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
        b.set_remap_from_map(True, BAND)
        one(base | B.RUN_MAP | mapped)

    def mode_two_runs():
        one(base | B.RUN_MAP)
        b.set_remap(stretches(), BAND)
        one(base | mapped)

    if args.trace_only:
        mode_one_run()
        for _ in range(args.trace_only):
            mode_one_run()
        status = [b.remap(v)["status"] for v in range(NREAD)]
        print(json.dumps({"trace_only_runs": args.trace_only, "remap_status_counts": [status.count(k) for k in range(3)]}))
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
    for name, flags in (("none", base), ("map", base | B.RUN_MAP), ("one_run", base | B.RUN_MAP | mapped)):
        if name == "one_run":
            b.set_remap_from_map(True, BAND)
        one(flags)
        rows = []
        for _ in range(args.runs):
            one(flags)
            rows.append({k: round(v["ms"], 4) for k, v in b.profile().items()})
        out["groups_ms"][name] = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}
    b.set_remap(stretches(), BAND)                            # (the records of the run before are the mode's: the same)
    one(base | mapped)
    rows = []
    for _ in range(args.runs):
        one(base | mapped)
        rows.append({k: round(v["ms"], 4) for k, v in b.profile().items()})
    out["groups_ms"]["second_run_of_two"] = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}
    eng.set_profiling(False)
    med = {k: sorted(v)[len(v) // 2] for k, v in out["ms_per_batch"].items()}
    out["ms_per_batch_median"] = med
    rec = {k: out["groups_ms"][k]["recurrent"] for k in ("none", "map", "one_run")}
    out["exposed_ms"] = {"none": round(med["none"] - rec["none"], 4), "map": round(med["map"] - rec["map"], 4), "one_run": round(med["one_run"] - rec["one_run"], 4),
                         "two_runs": round(med["two_runs"] - rec["map"] - out["groups_ms"]["second_run_of_two"]["recurrent"], 4)}
    out["remap_kernels_ms_one_run"] = round(out["groups_ms"]["one_run"]["viterbi_assembly"] - out["groups_ms"]["map"]["viterbi_assembly"], 4)
    out["one_run_is_faster"] = bool(med["one_run"] < med["two_runs"])
    # what the sizing takes
    mode_one_run()
    rm = [b.remap(v) for v in range(NREAD)]
    lens = [len(c) for c in calls]
    nb = [b.read_nblock(v) for v in range(NREAD)]
    forms_room = [B.remap_from_map_form(n, BAND) for n in nb]
    forms_exact = [int(B.lib().ffhip_debug_remap_form(max(r["L"], 1), BAND)) for r in rm]
    out["call_lengths"] = [int(np.min(lens)), int(np.mean(lens)), int(np.max(lens))]
    out["blocks"] = [int(np.min(nb)), int(np.max(nb))]
    out["remap_status_counts"] = [[r["status"] for r in rm].count(k) for k in range(3)]
    out["forms_by_room"] = [forms_room.count(k) for k in range(4)]
    out["forms_by_L"] = [forms_exact.count(k) for k in range(4)]
    out["workspace_bytes_room"] = int(sum(8 * WS_WORDS_A_BLOCK[f] * n for f, n in zip(forms_room, nb)))
    out["workspace_bytes_exact"] = int(sum(8 * WS_WORDS_A_BLOCK[f] * n for f, n, r in zip(forms_exact, nb, rm) if r["status"] == 1))
    out["sequences_and_events_bytes_room"] = int(sum(18 * (n + 1) for n in nb))
    out["sequences_and_events_bytes_exact"] = int(sum(18 * r["L"] for r in rm if r["status"] == 1))
    out["device_bytes"] = b.device_bytes()
    print(json.dumps(out))
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
