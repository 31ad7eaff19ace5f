"""The per-read products outside the result block -- barcodes, adapters, truth, remap, events, site mods, variants -- against tests/golden/annot_copies.json: the
figures of the library before those products were described by a table (flappie_amd/csrc/ffhip_annot.hpp), recorded by tests/golden/make_annot_copies.py.  The
LSTM trunk under the 5-base head (H = 128: it takes all seven flags and lets a sample saturate), batches of one read a row and packed, with and without an
outlier that sends read 1 through the f32 re-run; each feature on, off, on; all seven; all seven before and after every input doubles.  Per finish:
device-to-host copy calls, device-to-host bytes, device bytes held, reads run again, and a SHA-256 of every valid feature's records -- all exact, no tolerance.
And, on the same runs: what all seven flags together make of a read is, byte for byte, what each flag alone makes of it."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    import make_annot_copies as G
    eng = G.B.Engine(0)
    blobs = {}
    got = G.record(eng, blobs)
    eng.close()
    for case, rows in got.items():
        print(case, rows)
    return G, got, blobs


def test_copies_device_memory_and_records_match_the_recorded_figures(recorded):
    G, got, _ = recorded
    with open(os.path.join(HERE, "golden", "annot_copies.json")) as f:
        want = json.load(f)
    assert len(want) == len(G.FORMS) * len(G.SEQUENCES)
    assert set(got) == set(want)
    bad = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not bad, bad
    # every run of the outlier cases did take the re-run, and the doubled inputs made the batch grow
    assert all(r[3] > 0 for case, rows in want.items() if ",outlier," in case for r in rows)
    assert all(rows[1][2] > rows[0][2] for case, rows in want.items() if case.endswith(",grow"))
    assert all(set(r[4]) == set(G.FEATURES) for case, rows in want.items() if case.endswith((",all", ",grow")) for r in rows)


@pytest.mark.parametrize("form", ["rows", "packed"])
def test_all_together_equals_each_alone(recorded, form):
    G, got, blobs = recorded
    every = "%s,outlier,all" % form
    assert got[every][0][3] >= 1
    for name in G.FEATURES:
        one = "%s,outlier,%s" % (form, name)
        assert got[one][0][3] >= 1
        together, alone = blobs[(every, 0, name)], blobs[(one, 0, name)]
        assert len(together) == len(alone) == (8 if form == "rows" else 40)
        assert len(together[1]) > 1, name                    # (the re-run read's record is not the "nothing" of a status other than 1: its sequence is its own call)
        differ = [v for v in range(len(alone)) if together[v] != alone[v]]
        assert not differ, (form, name, differ)
