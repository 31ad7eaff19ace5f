"""What the host side of the per-read features answers to a call it refuses -- return code and ffhip_last_error text, and which of two broken rules answers --
is what the library answered before that code moved into flappie_amd/csrc/ffhip_features.hip and every repeated check became one helper:
tests/golden/feature_refusals.json, recorded by tests/golden/make_feature_refusals.py on the parent commit's library, replayed here call for call."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_feature_refusals as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay():
    """the cases on this tree's library, once: {case: (code, text)} in the order they were called"""
    eng = G.B.Engine(0)
    rows = G.record(eng)
    eng.close()
    return rows


def _golden():
    with open(os.path.join(HERE, "golden", "feature_refusals.json")) as f:
        return json.load(f)


def test_the_same_calls_in_the_same_order(replay):
    assert [r[0] for r in replay] == [r[0] for r in _golden()]


def test_codes_and_texts_are_the_parents(replay):
    bad = [(now, then) for now, then in zip(replay, _golden()) if now != then]
    assert not bad, "%d of %d cases differ, the first: now %r, recorded %r" % (len(bad), len(replay), bad[0][0], bad[0][1])


def test_the_record_holds_refusals_of_every_part():
    rows = _golden()
    refused = [r for r in rows if not r[0].endswith("taken") and ": ok" not in r[0]]
    for part in ("barcodes_upload", "adapters_upload", "map_ref_upload", "pileup_create", "run ", "set_", "op_", "barcode:", "adapters:", "map:", "polytail:", "remap:",
                 "truth:", "events:", "site_mods:", "variant_calls:"):
        assert any(r[0].startswith(part) for r in refused), part
    assert sum("+" in r[0] for r in rows) >= 40      # two rules broken at once
    assert len({r[2] for r in rows}) >= 150          # distinct texts
