#!/usr/bin/env python3
"""errprofile_bench.py -- what FFHIP_RUN_ERRPROFILE costs a batch at the headline shape of bench.py (H = 384, 256 reads x 4000 samples), against the same run
without it.

Shape and reference are those of tools/map_truth_bench.py and tools/consensus_bench.py: a reference of lambda's size (48 502 bases) of random filler with the
batch's own calls in it, 5 % edits, alternating strands, so that the reads map, k_truth aligns them and k_errprofile has ops to class.  Two ways of running the same
batch, alternating, one batch after the other:
  without     FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map (the code path of the build before the flag)
  with        the same with FFHIP_RUN_ERRPROFILE into one error profile
For each: the wall time of a batch (host clock around `steps` runs that end in a synchronise of the engine, so that the last batch's unwaited-for k_errprofile is
inside), every round's figure, their median and their spread.  Then what one batch counted.  `--groups N` caps the launch's workgroups (0: the device's compute
units, the default), to hold the grid choice to another.  `--trace-only N` just runs the `with` mode N times: the command to put under `rocprofv3 --kernel-trace
--stats` for the kernel's own time beside k_truth's.  One JSON line; profiles/r18_errprofile_cost.txt keeps it.
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
    ap.add_argument("--groups", type=int, default=0)
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
    prof = B.ErrProfile(eng)
    prof.debug_groups(args.groups)
    b.set_map(ref)
    b.set_truth_from_map(True, BAND)
    b.set_errprofile(prof)
    modes = {"without": base | B.RUN_MAP | B.RUN_TRUTH, "with": base | B.RUN_MAP | B.RUN_TRUTH | B.RUN_ERRPROFILE}
    if args.trace_only:
        one(modes["with"])
        for _ in range(args.trace_only):
            one(modes["with"])
        print(json.dumps({"trace_only_runs": args.trace_only, "groups": args.groups, "totals": prof.download()[1]}))
        return
    out = {"shape": "H = 384, 256 reads x 4000 samples, one batch a run, reference of %d bases holding %d of the calls, window 4096, band %d" % (REF_BASES, used, BAND),
           "groups": args.groups, "ms_per_batch": {k: [] for k in modes}}
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
    out["errprofile_ms_per_batch"] = round(med["with"] - med["without"], 4)
    # what one batch adds
    prof.reset()
    one(modes["with"])
    counts, totals = prof.download()
    out["totals_of_one_batch"] = totals
    sec = B.ErrProfile.sections(counts)
    out["lds_adds_of_one_batch"] = {k: int(v.sum()) for k, v in sec.items()}
    out["nonzero_words_of_one_batch"] = {k: int((v != 0).sum()) for k, v in sec.items()}
    print(json.dumps(out))
    prof.close()
    ref.close()
    b.close()
    dm.close()
    eng.close()


if __name__ == "__main__":
    main()
