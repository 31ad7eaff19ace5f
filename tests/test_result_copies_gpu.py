"""What a finished run copies to the host and what its batch holds on the device, against tests/golden/result_copies.json: the figures of the library before
the result block was described by a table (flappie_amd/csrc/ffhip_results.hpp), recorded by tests/golden/make_result_copies.py.  Three models (4 bases, 5 bases,
run-length; H = 128), batches of one read a row and packed, flag sequences that grow the block in every order, and an outlier that sends reads through the f32
re-run with each section made.  Per finish: device-to-host copy calls, device-to-host bytes, device bytes held, reads run again -- all exact, no tolerance."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


def test_copies_and_device_memory_match_the_recorded_figures():
    import make_result_copies as G
    with open(os.path.join(HERE, "golden", "result_copies.json")) as f:
        want = json.load(f)
    ncase = 2 * (sum(len(v) for v in G.SEQUENCES.values()) + len(G.OUTLIER))
    assert len(want) == ncase
    eng = G.B.Engine(0)
    got = G.record(eng)
    eng.close()
    for case, rows in got.items():
        print(case, rows)
    assert set(got) == set(want)
    bad = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not bad, bad
    # the outlier cases did take the re-run, and every section was copied by some run
    assert all(any(r[3] > 0 for r in rows) for case, rows in want.items() if case.endswith(",outlier"))
