"""The rule that picks a layer launch of the split-operand kernels (ffhip_rnn_split.hip split_plan, read through ffhip_debug_split_plan) against
tests/golden/split_plan_table.json, which was recorded from the predicates split_plan replaced (tests/golden/make_split_plan_table.py).  Every parity and bit
test passes whichever of the bit-identical kernel forms is launched; this one holds the choice itself: the tiles a launch takes, its grid, the workgroups
that share a compute unit, whether it fills the chip, and whether two batches may share paired launches.  No GPU: the entry touches no device."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_split_plan_table as G  # noqa: E402
from flappie_amd import binding as B  # noqa: E402

with open(os.path.join(HERE, "golden", "split_plan_table.json")) as _f:
    TABLE = json.load(_f)


@pytest.fixture(autouse=True)
def _restore_debug():
    old = os.environ.get("FFHIP_DEBUG")
    yield
    G.set_debug(old)


def test_table_covers_the_cases():
    assert len(TABLE) == len(G.KINDS) * len(G.HS) * len(G.NCUS) * len(G.DEBUGS) * len(G.BESIDE)
    for key, runs in TABLE.items():
        assert sum(n for n, _ in runs) == G.max_remaining(int(key.split(",")[2])), key


@pytest.mark.parametrize("dbg", G.DEBUGS)
@pytest.mark.parametrize("H", G.HS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_split_plan_matches_recorded_rules(kind, H, dbg):
    supported = H <= (512 if kind == 0 else 384)
    for ncu in G.NCUS:
        for beside in G.BESIDE:
            want = [row for n, row in TABLE["%d,%d,%d,%s,%d" % (kind, H, ncu, dbg, beside)] for _ in range(n)]
            for remaining, (nrt, ts, wg, per_cu, fills, pair_ok, pair_ok_no_pair) in enumerate(want, start=1):
                where = "kind %d H %d ncu %d FFHIP_DEBUG=%r beside %d remaining %d" % (kind, H, ncu, dbg, beside, remaining)
                G.set_debug(dbg)
                p = B.split_plan(kind, H, remaining, ncu, beside)
                got_pair_ok = B.split_pair_ok(kind, H, p["nrt"], ncu)
                G.set_debug((dbg + "," if dbg else "") + "no_pair")
                p_no_pair = B.split_plan(kind, H, remaining, ncu, beside)
                # the recorded values (ts 0: a one-tile launch's grid does not show the parent's choice)
                assert (p["nrt"], p["workgroups"], p["per_cu"], p["fills_chip"], got_pair_ok) == (nrt, wg, per_cu, fills, pair_ok), where
                assert p["ts"] == ts or (ts == 0 and p["ts"] in (1, 2)), where
                assert B.split_pair_ok(kind, H, p["nrt"], ncu) == pair_ok_no_pair == 0 and p_no_pair == p, where
                # what ties the form to them
                form = p["form"]
                assert (form == "none") == (not supported), where
                assert p["fills_chip"] == int(2 * p["workgroups"] > ncu * p["per_cu"]), where
                assert 1 <= p["nrt"] <= remaining, where
                if not supported:
                    continue
                assert (form == "pack") == (p["workgroups"] == p["nrt"] // 2 * 16), where
                assert (form == "dense256") == (p["per_cu"] == 3), where
                assert (form == "one_tile") == (p["ts"] == 1), where
                assert (form == "dense3") == (kind == 0 and H == 384 and p["ts"] == 2 and p["per_cu"] == 2), where
                if form != "pack":
                    assert p["workgroups"] == (p["nrt"] + p["ts"] - 1) // p["ts"] * 32, where
                if form == "pair_tiles":
                    assert p["per_cu"] == (1 if H > 256 else 2), where
                if form in ("pack", "dense256"):
                    assert H == 256 and p["ts"] == 2, where
                if "no_dense" in dbg:
                    assert form in ("one_tile", "pair_tiles"), where
                if "no_pack" in dbg:
                    assert form != "pack", where
                if pair_ok:
                    assert B.split_plan(kind, H, p["nrt"], ncu, 1)["form"] == "dense3", where      # a paired launch is the dense form's
