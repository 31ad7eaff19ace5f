"""`flappie` and `runnie` on multi-read fast5 files: one file, a root group read_<x> per read, the samples carried as int16 DAC values to the device
(ffhip_prep_begin_dac).  The bar is the single-read route: the same reads written as single-read files, named so that they sort as the groups do,
must give the same records.  SAM records are compared byte for byte; a FASTA/FASTQ header carries a "filename" field, which names the file a read
came from and so cannot be equal -- it is masked, and everything else is byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
from test_cli import FAST5LIB, FLAPPIE, RUNNIE, TOOL, synth_raw, write_fast5
from test_fast5_multi import writem

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(FLAPPIE) and os.path.exists(RUNNIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)),
                                 reason="libhdf5 not found when the host layer was built")]

LENS = [4000, 1200, 9000, 2600, 4013, 1500, 7001, 3100, 5555, 1999, 8192, 4097]
FILENAME = re.compile(r'"filename" : "[^"]*"')


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("multi")
    M.write_mdl(str(d / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=1, ident="r941native"))
    M.write_mdl(str(d / "runlength5_r941native.h"), M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=9, ident="r941native"))
    rng = np.random.default_rng(123)
    reads = []
    for k, n in enumerate(LENS):
        # (the calibration of write_fast5's single-read files: 8192, 10, 1400; group names whose order is not the list's)
        reads.append(dict(name="%02d-%04x" % ((7 * k) % 12, k), id="uuid-%04d" % k, dac=synth_raw(rng, n), dig=8192.0, off=10.0, rng=1400.0))
    ordered = sorted(reads, key=lambda r: "read_" + r["name"])
    (d / "one").mkdir()
    writem(d / "one" / "multi.fast5", reads, 1 | 2 | 4, 1000)
    (d / "singles").mkdir()
    singles = []
    for r in ordered:
        p = d / "singles" / ("read_%s.fast5" % r["name"])
        write_fast5(p, r["id"], r["dac"])
        singles.append(str(p))
    # two multi-read files and three single-read files in one directory
    (d / "mixed").mkdir()
    writem(d / "mixed" / "b_multi.fast5", reads[:5], 0, 0)
    writem(d / "mixed" / "d_multi.fast5", reads[5:9], 1 | 2, 700)
    for r, fn in zip(reads[9:], ("a_single.fast5", "c_single.fast5", "e_single.fast5")):
        write_fast5(d / "mixed" / fn, r["id"], r["dac"])
    for sub in ("one", "mixed"):                       # (writem's side files are no .fast5 files, but keep the directories to what a user has)
        for f in os.listdir(d / sub):
            if not f.endswith(".fast5"):
                os.unlink(d / sub / f)
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(d))
    env.pop("FLAPPIE_DEBUG", None)
    return dict(dir=d, reads=reads, ordered=ordered, singles=singles, multi=str(d / "one" / "multi.fast5"), env=env, cache={})


def run(inputs, args, debug=None, binary=FLAPPIE, ok=True, batch="16"):
    env = dict(inputs["env"], **({"FLAPPIE_DEBUG": debug} if debug else {}))
    r = subprocess.run([binary, "--batch", batch] + args, env=env, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
    return r


def singles_out(inputs, fmt_args):
    key = tuple(fmt_args)
    if key not in inputs["cache"]:
        inputs["cache"][key] = run(inputs, list(fmt_args) + ["--readers", "0"] + inputs["singles"]).stdout
    return inputs["cache"][key]


def sam_records(text):
    """a plain SAM record of this binary is two lines, as the reference prints it: the record, then sequence and quality once more (flappie_output.c)"""
    lines = text.splitlines(keepends=True)
    assert len(lines) % 2 == 0 and all(ln.count("\t") >= 10 for ln in lines[0::2]) and all(ln.count("\t") == 1 for ln in lines[1::2])
    return [a + b for a, b in zip(lines[0::2], lines[1::2])]


def names(text, fmt="fastq"):
    if fmt == "sam":
        return [rec.split("\t")[0] for rec in sam_records(text)]
    return [ln[1:].split("  {")[0] for ln in text.splitlines()[0::4]]


@pytest.mark.parametrize("readers", ["0", "2"])
@pytest.mark.parametrize("debug", [None, "no_pack"])
def test_one_multi_read_file_equals_its_reads_as_single_read_files(inputs, readers, debug):
    want = singles_out(inputs, ())
    assert names(want) == [r["id"] for r in inputs["ordered"]]
    got = run(inputs, ["--readers", readers, inputs["multi"]], debug).stdout
    assert FILENAME.sub("F", got) == FILENAME.sub("F", want)
    assert got.count('"filename" : "multi.fast5:uuid-') == len(LENS)
    want = singles_out(inputs, ("--format", "sam"))
    assert run(inputs, ["--format", "sam", "--readers", readers, inputs["multi"]], debug).stdout == want      # no file name in a SAM record: byte for byte


@pytest.mark.parametrize("readers", ["0", "2"])
def test_sam_with_move_tables(inputs, readers):
    want = singles_out(inputs, ("--format", "sam", "--emit-moves"))
    assert "\tmv:B:c," in want
    assert run(inputs, ["--format", "sam", "--emit-moves", "--readers", readers, inputs["multi"]]).stdout == want


@pytest.mark.parametrize("readers", ["0", "2"])
def test_last_read_of_the_file_fills_a_chunk(inputs, readers):
    """--batch 12: the first chunk is twelve reads, which the file's last read fills exactly -- whether a read follows is only known at the next call of the
    cursor (the end-of-file record of a reader process), so an empty last chunk follows and must be passed over; with no_reader_thread the main thread reads"""
    want = run(inputs, ["--format", "sam", "--readers", "0"] + inputs["singles"], batch="12").stdout
    assert len(sam_records(want)) == len(LENS)
    assert run(inputs, ["--format", "sam", "--readers", readers, inputs["multi"]], batch="12").stdout == want
    if readers == "0":
        assert run(inputs, ["--format", "sam", "--readers", "0", inputs["multi"]], "no_reader_thread", batch="12").stdout == want
        assert run(inputs, ["--format", "sam", "--readers", "0", inputs["multi"]], "prep_ahead_min=0", batch="12").stdout == want


def test_files_in_order_then_reads_limit_and_shards(inputs):
    mixed = str(inputs["dir"] / "mixed")
    files = run(inputs, [mixed], "list_only").stdout.split()
    assert sorted(os.path.basename(f) for f in files) == ["a_single.fast5", "b_multi.fast5", "c_single.fast5", "d_multi.fast5", "e_single.fast5"]
    reads = inputs["reads"]
    per_file = {"b_multi.fast5": sorted(reads[:5], key=lambda r: "read_" + r["name"]), "d_multi.fast5": sorted(reads[5:9], key=lambda r: "read_" + r["name"]),
                "a_single.fast5": [reads[9]], "c_single.fast5": [reads[10]], "e_single.fast5": [reads[11]]}

    def expect(fs):
        return [r["id"] for f in fs for r in per_file[os.path.basename(f)]]

    for readers in ("0", "2"):
        whole = run(inputs, ["--format", "sam", "--readers", readers, mixed]).stdout
        assert names(whole, "sam") == expect(files), readers
    for readers in ("0", "2", "4"):                                                                                # --limit counts reads (4: the default reader count)
        assert run(inputs, ["--format", "sam", "--limit", "7", "--readers", readers, mixed]).stdout == "".join(sam_records(whole)[:7]), readers
    parts = []
    for g in (0, 1):
        mine = run(inputs, ["--shard", "%d/2" % g, mixed], "list_only").stdout.split()
        part = run(inputs, ["--format", "sam", "--shard", "%d/2" % g, mixed]).stdout
        assert names(part, "sam") == expect(mine)                                                                  # shards deal files
        parts += sam_records(part)
    assert sorted(parts) == sorted(sam_records(whole)) and len(parts) == len(LENS)


def test_names_without_uuid_and_trace_groups(inputs, tmp_path):
    trace = tmp_path / "trace.hdf5"
    out = run(inputs, ["--no-uuid", "--trace", str(trace), inputs["multi"]]).stdout
    want = ["multi.fast5:" + r["id"] for r in inputs["ordered"]]
    assert names(out) == want
    for name, hdr in zip(want, out.splitlines()[0::4]):                   # one group per read, under the name the record carries
        d = subprocess.run([TOOL, "dump", str(trace), name], capture_output=True, text=True)
        assert d.returncode == 0, name
        s, e = (int(x) for x in hdr.split('"trim" : [ ')[1].split(" ]")[0].split(", "))
        assert d.stdout.splitlines()[0] == "signal %d" % (e - s)
    # ... and the signal stored is the one the single-read route stores
    trace1 = tmp_path / "trace1.hdf5"
    run(inputs, ["--trace", str(trace1), "--readers", "0"] + inputs["singles"][:2])
    trace2 = tmp_path / "trace2.hdf5"
    run(inputs, ["--trace", str(trace2), "--limit", "2", inputs["multi"]])
    for r in inputs["ordered"][:2]:
        a, b = (subprocess.run([TOOL, "dump", str(t), r["id"]], capture_output=True, text=True) for t in (trace1, trace2))
        assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout


def test_runnie_fasta(inputs):
    want = run(inputs, ["--fasta", "--readers", "0"] + inputs["singles"], binary=RUNNIE).stdout
    assert want.count(">") == len(LENS)
    for readers in ("0", "2"):
        assert run(inputs, ["--fasta", "--readers", readers, inputs["multi"]], binary=RUNNIE).stdout == want


def test_reader_death_inside_a_multi_read_file(inputs):
    """reader 0 of 2 has files 0, 2 and 4 and dies at the fourth read of file 0 (a multi-read file): its three reads that were delivered are called, the rest
    of that file is lost, files 2 and 4 are read in-process and complete, and the exit status says that a reader failed"""
    m = inputs["dir"] / "mixed"
    files = [str(m / f) for f in ("b_multi.fast5", "a_single.fast5", "d_multi.fast5", "c_single.fast5", "e_single.fast5")]
    whole = sam_records(run(inputs, ["--format", "sam", "--readers", "2"] + files).stdout)
    assert len(whole) == len(LENS)
    r = run(inputs, ["--format", "sam", "--readers", "2"] + files, "kill_reader=0:0:3", ok=False)
    assert r.returncode != 0 and "ended early" in r.stderr and "reader process(es) failed" in r.stderr
    assert sam_records(r.stdout) == whole[:3] + whole[5:]
