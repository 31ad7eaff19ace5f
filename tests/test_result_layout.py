"""The layout of a batch's result block (flappie_amd/csrc/ffhip_results.hpp: the tables kResFields / kResSections, read through ffhip_debug_result_layout)
against tests/golden/result_layout_table.json, the arithmetic the tables replaced (tests/golden/make_result_layout_table.py): every offset, exactly.  The GPU
suites hold what the kernels write there; this one holds where.  No GPU: the entry touches no device."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_result_layout_table as G  # noqa: E402
from flappie_amd import binding as B  # noqa: E402

with open(os.path.join(HERE, "golden", "result_layout_table.json")) as _f:
    TABLE = json.load(_f)
# the recorded section ends under the sections' names
ENDS = {"core": "end", "runs": "runs_end", "records": "rec_end", "mod": "ml_end", "moves": "mv_end"}
SECTION_FIELDS = {"head": ("sat", "abort"), "core": ("lens", "score", "bases", "quals"), "runs": ("nrun", "fail", "len", "base", "est"),
                  "records": ("shape", "scale", "dwell"), "mod": ("ml",), "moves": ("mv",)}


def test_table_covers_the_grid():
    assert len(TABLE) == len(G.NREADS) * len(G.CAP_FACTORS) * len(G.TBS) * len(G.SECTION_SETS)
    assert set(TABLE) == {G.key(*c) for c in G.cases()}
    assert B.RESULT_FIELDS == tuple(n for n in G.NAMES if n not in ENDS.values())
    assert sum(len(v) for v in SECTION_FIELDS.values()) == len(B.RESULT_FIELDS) and tuple(SECTION_FIELDS) == B.RESULT_SECTIONS


@pytest.mark.parametrize("nread", G.NREADS)
def test_layout_matches_recorded_offsets(nread):
    for n, cap, Tb, secs in G.cases():
        if n != nread:
            continue
        want = dict(zip(G.NAMES, TABLE[G.key(n, cap, Tb, secs)]))
        got = B.result_layout(n, cap, Tb, secs)
        where = "nread %d cap_reads %d Tb %d sections %r" % (n, cap, Tb, secs)
        for f in B.RESULT_FIELDS:
            assert got["field"][f] == want[f], (where, f)
        for s, name in ENDS.items():
            assert got["end"][s] == want[name], (where, s)
        assert got["end"]["head"] == want["lens"], where


@pytest.mark.parametrize("secs", G.SECTION_SETS)
def test_layout_rules(secs):
    for n, cap, Tb, s in G.cases():
        if s != secs:
            continue
        lay = B.result_layout(n, cap, Tb, secs)
        fld, end = lay["field"], lay["end"]
        where = "nread %d cap_reads %d Tb %d sections %r" % (n, cap, Tb, secs)
        assert all(v % 256 == 0 for v in list(fld.values()) + list(end.values())), where            # every part is 256-aligned
        held = ("head", "core") + tuple(secs)
        order = [fld[f] for sec in B.RESULT_SECTIONS if sec in held for f in SECTION_FIELDS[sec]]
        assert order[0] == 0 and all(a < b for a, b in zip(order, order[1:])), where                # the fields of the block, one behind the other
        assert [end[sec] for sec in held] == sorted(end[sec] for sec in held), where                # a longer section set: a longer prefix
        for sec in held:                                                                             # a section ends behind its last field, which fits
            last = SECTION_FIELDS[sec][-1]
            assert end[sec] > fld[last] and all(fld[SECTION_FIELDS[sec][0]] <= fld[f] < end[sec] for f in SECTION_FIELDS[sec]), (where, sec)
        assert fld["lens"] == end["head"] and fld["nrun"] == fld["ml"] == end["core"] and fld["shape"] == end["runs"], where
        assert fld["mv"] == (end["mod"] if "mod" in secs else end["core"]), where                  # mv behind ml iff the block holds ml
        # sizes: a byte a block for the strings, the 5mC bytes and the moves; 4 a read for lens and score
        n1 = n * (Tb + 1)
        up = G.up
        assert fld["quals"] - fld["bases"] == end["core"] - fld["quals"] == end["mod"] - fld["ml"] == end["moves"] - fld["mv"] == up(n1), where
        assert fld["score"] - fld["lens"] == up(4 * cap) and fld["abort"] == up(4 * ((n + 15) // 16 * 16)) and fld["lens"] - fld["abort"] == 256, where


def test_layout_rejects_bad_arguments():
    with pytest.raises(B.FFHipError):
        B.result_layout(0, 0, 10)
    with pytest.raises(B.FFHipError):
        B.result_layout(4, 4, 0)
