"""runnie --fasta, without a GPU: the numpy restatement of decode_runnie.py (tests/runnie_fasta_ref.py) reproduces the reference script's own outputs on the
crafted fixture byte for byte, and the device's form of the run-length estimate -- rint(scale * 1e6) / 1e6 on the fp32 value -- equals the script's estimate
of the printed text on every fixture scale, including those where the fp32 value itself would give another.

The fixture (tests/golden/runnie_fasta*) is data only.  runnie_fasta.run is a crafted run-record text in runnie's format (`# name` headers, then
base<TAB>%f<TAB>%f<TAB>dwell lines, the %f text of fp32 values): a read of fp32 scales found by searching the neighbours of m / factor (m = 1 .. 59) for
values whose estimate changes when the scale is rounded to six decimals (for the default factors and for 1.1, 0.95, 1.3, 1.07), a read of scales below
1 / factor, a read without runs, a 700-run read and two of random records.  runnie_fasta_records.json holds the same records with the fp32 bit patterns
of every shape and scale, and the factors of each mode.  runnie_fasta_<mode>.fa / .err are what the reference's misc/decode_runnie.py printed on stdout
and stderr when it was run once on that text: mode default (no option), rlc (--rlc) and scale (--scale 1.1 0.95 1.3 1.07).  The last two tests below
check the restatement's own helpers, not product code."""
import json
import math
import os

import numpy as np
import pytest

import runnie_fasta_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _read(name):
    with open(os.path.join(GOLD, name)) as fh:
        return fh.read()


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(GOLD, "runnie_fasta_records.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("mode", ["default", "rlc", "scale"])
def test_restatement_reproduces_the_reference_script(doc, mode):
    out, err = R.fasta_from_run(_read("runnie_fasta.run"), doc["factors"][mode], rlc=(mode == "rlc"))
    assert out == _read("runnie_fasta_%s.fa" % mode)
    assert err == _read("runnie_fasta_%s.err" % mode)


def test_fixture_covers_the_edges(doc):
    names = [r["name"] for r in doc["reads"]]
    assert any(not r["runs"] for r in doc["reads"])
    assert "No basecall returned for read_without_runs\n" == _read("runnie_fasta_default.err")
    assert max(len(r["runs"]) for r in doc["reads"]) > 500
    edges = 0
    for mode in ("default", "scale"):
        f = doc["factors"][mode]
        for r in doc["reads"]:
            for b, _, bits, _ in r["runs"]:
                v = float(np.uint32(bits).view(np.float32))
                edges += max(1, math.floor(v * f[b])) != max(1, math.floor(float("%f" % v) * f[b]))
    assert edges >= 20, "the fixture must hold scales where the printed text's estimate differs"
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("mode", ["default", "scale"])
def test_device_estimate_form_equals_the_parsed_text(doc, mode):
    f = doc["factors"][mode]
    text = _read("runnie_fasta.run")
    want = [int(max(1, math.floor(float(ln.split("\t")[2]) * f["ACGT".index(ln[0])]))) for ln in text.splitlines() if not ln.startswith("#")]
    got = []
    for r in doc["reads"]:
        if r["runs"]:
            base = [x[0] for x in r["runs"]]
            scale = np.array([x[2] for x in r["runs"]], dtype=np.uint32).view(np.float32)
            est, bad = R.estimate(base, scale, f)
            assert not bad
            got += [int(e) for e in est]
    assert got == want


def test_records_restatement_of_the_host_loop():
    # blocks before the first run count for nothing; the last run's dwell runs to the end
    path = np.array([5, 6, 1, 5, 5, 2, 3, 7, 0, 4])
    mat = np.arange(9 * 40, dtype=np.float32).reshape(9, 40)
    recs = R.records(path, mat)
    assert [(b, d) for b, _, _, d in recs] == [(1, 3), (2, 1), (3, 2), (0, 1)]
    assert recs[0][1] == mat[2, 1] and recs[0][2] == mat[2, 5]
    assert R.records(np.array([4, 5, 6]), mat[:3]) == []


def test_failure_and_estimate_floor():
    est, bad = R.estimate([0, 1], [1e-8, 0.5])
    assert list(est) == [1, 1] and not bad
    assert R.estimate([0], [np.inf])[1] and R.estimate([0], [np.nan])[1] and R.estimate([2], [3e9])[1]
    assert not R.estimate([2], [2.0e9])[1]
