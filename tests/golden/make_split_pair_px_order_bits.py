#!/usr/bin/env python3
"""tests/golden/split_pair_px_order_bits.json: one digest per 16 reads of every case of tests/test_split_pair_px_order_gpu.py (the dense layer kernels at both
gate levels, one read a row and packed), recorded on an MI355X from the release library of the commit BEFORE round 9 moved the x waves' px write behind barrier 1.
The test runs this script once per library (release, late waves, forced re-sweep) and compares what it writes with the recorded file.
usage: tests/golden/make_split_pair_px_order_bits.py [OUT.json]   (FFHIP_BINDING_LIBRARY names the library to record; default: the tree's)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flappie_amd import binding as B  # noqa: E402
import test_split_pair_px_order_gpu as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "split_pair_px_order_bits.json")
rec = T.record(B)
with open(out, "w") as f:
    json.dump(rec, f, indent=0, sort_keys=True)
print("wrote", out, "from", os.environ.get("FFHIP_BINDING_LIBRARY") or "the tree's library", {k: [len(x) for x in v] for k, v in rec.items()})
