#!/usr/bin/env python3
"""tests/golden/split_pair_h384_bits.json: digests of the probe reads of tests/test_split_pair_x_path_gpu.py's cases (ragged pairs at both gate
levels, packed pairs), recorded on an MI355X from the paired H = 384 layer kernel as it was before round 7 moved its x waves' input into pieces.
usage: tests/golden/make_split_pair_bits.py [OUT.json]   (FFHIP_BINDING_LIBRARY may name the library to record)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flappie_amd import binding as B  # noqa: E402
from flappie_amd import model as M  # noqa: E402
import test_split_pair_x_path_gpu as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "split_pair_h384_bits.json")
eng = B.Engine(0)
dm = B.DeviceModel(eng, M.synthetic_model(M.NET_LSTM5, T.HIDDEN, seed=1))
rec = T.record(B, dm)
dm.close()
eng.close()
with open(out, "w") as f:
    json.dump(rec, f, indent=0, sort_keys=True)
print("wrote", out, {k: [len(x) for x in v] for k, v in rec.items()})
