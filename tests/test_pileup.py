"""flappie --map-pileup without a GPU: the restatement (pileup_ref.py: the header's walk in signal order) held to an independent forward-strand walk of the read's
SAM line; the identity test at its boundary; the host side (flappie_pileup.c of libflappie_host.so: the table and the summary) against the restatement; header,
binding and library agree on the new calls; the command line's refusals.  Everything is integer- or byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_ref as R
import pileup_ref as PU
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5
from test_map import Ref

NEW_CALLS = ("ffhip_pileup_create", "ffhip_pileup_free", "ffhip_pileup_reset", "ffhip_pileup_positions", "ffhip_pileup_download", "ffhip_batch_set_pileup",
             "ffhip_op_pileup")


def random_ops(rng, m, weights=(0.8, 0.07, 0.06, 0.07), lead=0, trail=0):
    """a path that consumes m truth bases: ops drawn by `weights` (=, X, I, D) with `lead` / `trail` insertions at its ends; returns (ops, n)"""
    ops = [2] * lead
    j = 0
    while j < m:
        op = int(rng.choice(4, p=weights))
        ops.append(op)
        j += op != 2
    ops += [2] * trail
    return np.array(ops, np.uint8), sum(1 for x in ops if x != 3)


def random_alignments(rng, lens, count):
    """alignments on both strands of every record, with spans that touch either end, all-deletion paths and insertions at both edges among them"""
    out = []
    for it in range(count):
        k = int(rng.integers(0, len(lens)))
        Mk = lens[k]
        q = 2 * k + int(rng.integers(0, 2))
        a = 0 if it % 4 == 0 else int(rng.integers(0, Mk))
        b = Mk if it % 4 == 1 else int(rng.integers(a + 1, Mk + 1))
        kind = it % 7
        if kind == 5:
            ops, n = np.full(b - a, 3, np.uint8), 0                # n = 0: all deletions
        else:
            ops, n = random_ops(rng, b - a, lead=(it % 3) if kind in (1, 3) else 0, trail=(it % 4) if kind in (2, 3) else 0)
        call = "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n))
        out.append((q, a, b, call, ops))
    return out


# ------------------------------------------------------------------------------------ the two walks
def test_the_signal_order_walk_is_the_forward_strand_pileup():
    rng = np.random.default_rng(11)
    lens = [1, 15, 16, 17, 33, 100]
    alns = random_alignments(rng, lens, 400)
    alns += [(0, 0, 1, "A", [0]), (1, 0, 1, "A", [1]), (0, 0, 1, "", [3]), (1, 0, 1, "GT", [2, 3, 2]), (10, 0, 100, "ACGT", [2, 2] + [3] * 100 + [2, 2]),
             (11, 99, 100, "TZ", [2, 0]), (11, 0, 1, "ZT", [0, 2]), (3, 2, 4, "ACG", [0, 2, 0]), (2, 2, 4, "ACG", [0, 2, 0])]
    a, b = PU.Pileup(lens), PU.Pileup(lens)
    seen = {"plus": 0, "minus": 0, "start0": 0, "endM": 0, "n0": 0, "lead": 0, "trail": 0}
    for q, ts, te, call, ops in alns:
        a.add(q, ts, te, call, ops)
        b.forward_add(q, ts, te, call, ops)
        seen["minus" if q & 1 else "plus"] += 1
        seen["start0"] += ts == 0
        seen["endM"] += te == lens[q >> 1]
        seen["n0"] += len(call) == 0
        seen["lead"] += ops[0] == 2
        seen["trail"] += ops[-1] == 2
    assert min(seen.values()) >= 10, seen
    assert a.totals == b.totals and np.array_equal(a.counts, b.counts)
    t = a.totals
    assert t["reads"] == len(alns) and t["skipped"] == 0 and min(t[k] for k in ("match", "mismatch", "del", "ins", "edge_ins")) > 0 and t["reserved"] == 0
    # the planes hold what the totals say, and nothing outside a record's own positions
    assert int(a.counts[:, :4].sum()) == t["match"] + t["mismatch"] and int(a.counts[:, 4].sum()) == t["del"] and int(a.counts[:, 5].sum()) == t["ins"]
    # by hand: one read on the - strand of a record of 4 behind a record of 1: span [1, 3) of the reverse complement is forward [1, 3), walked from its right end
    p = PU.Pileup([1, 4])
    p.add(3, 1, 3, "AZG", [0, 2, 1])                          # A at forward 2 as T; Z inserted between forward 1 and 2: counted at 1; G at forward 1 as C
    want = np.zeros((2, 6, 5), np.uint32)
    want[1, 3, 1 + 2] = want[1, 5, 1 + 1] = want[1, 1, 1 + 1] = 1
    assert np.array_equal(p.counts, want) and p.totals == dict(reads=1, skipped=0, match=1, mismatch=1, ins=1, edge_ins=0, reserved=0, **{"del": 0})


def test_the_identity_test_at_its_boundary():
    # 3 matches of 4 columns: 750 per mille -- equality passes
    for min_id, counted in ((0, 1), (749, 1), (750, 1), (751, 0), (1000, 0)):
        for walk in ("add", "forward_add"):
            p = PU.Pileup([10], min_id)
            getattr(p, walk)(0, 2, 6, "ACG", [0, 0, 3, 0])
            assert (p.totals["reads"], p.totals["skipped"]) == (counted, 1 - counted), (min_id, walk)
            assert int(p.counts.sum()) == (4 if counted else 0)
    assert PU.passes(0, 0, 0, 5, 0) and not PU.passes(0, 0, 0, 5, 1) and PU.passes(7, 0, 0, 0, 1000) and not PU.passes(999, 1, 0, 0, 1000)
    assert PU.Pileup([3], -5).min_identity == 0
    # a read of a batch: both statuses 1, or nothing at all
    p = PU.Pileup([10], 900)
    mp = {"status": 1, "q": 0, "tstart": 0, "tend": 3}
    tr = {"status": 1, "n": 3, "m": 3, "ops": np.array([0, 1, 0], np.uint8)}
    p.add_read(mp, tr, "ACG")
    p.add_read(dict(mp, status=2), tr, "ACG")
    p.add_read(mp, dict(tr, status=2), "ACG")
    p.add_read(mp, dict(tr, status=0), "ACG")
    assert p.totals["skipped"] == 1 and p.totals["reads"] == 0 and int(p.counts.sum()) == 0


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    assert lib.ffhip_pileup_create.argtypes == [C.c_void_p, C.c_void_p, C.c_int] and lib.ffhip_pileup_create.restype == C.c_void_p
    assert lib.ffhip_pileup_positions.restype == C.c_size_t
    assert lib.ffhip_op_pileup.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("ffhip_pileup *ffhip_pileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity);",
                  "int ffhip_pileup_download(ffhip_pileup *p, uint32_t *counts /* [12][P] */, ffhip_pileup_totals *totals);",
                  "int ffhip_batch_set_pileup(ffhip_batch *b, ffhip_pileup *p);",
                  "int ffhip_op_pileup(ffhip_engine *eng, ffhip_pileup *p, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops);"):
        assert proto in header, proto
    m = re.search(r"#define FFHIP_RUN_PILEUP\s+(\d+)u", header)
    flags = [int(v) for v in re.findall(r"#define FFHIP_RUN_[A-Z_0-9]+\s+(\d+)u", header)]
    assert m and int(m.group(1)) == B.RUN_PILEUP == 2 * max(f for f in flags if f != B.RUN_PILEUP) and flags.count(B.RUN_PILEUP) == 1      # the next free bit
    assert B.PILEUP_TOTALS == PU.TOTALS and len(B.PILEUP_TOTALS) == 8
    assert callable(B.Pileup) and callable(B.Batch.set_pileup) and callable(B.op_pileup)
    H = C.CDLL(HOSTLIB)
    assert sorted(_declared_functions("flappie_pileup.h")) == ["flappie_pileup_summary_print", "flappie_pileup_write"]
    assert all(hasattr(H, n) for n in _declared_functions("flappie_pileup.h"))


# ------------------------------------------------------------------------------------ the host side
class Totals(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in PU.TOTALS]


def test_the_table_and_the_summary_are_the_restatements(tmp_path):
    L = C.CDLL(HOSTLIB)
    L.flappie_map_ref_parse.restype = C.POINTER(Ref)
    L.flappie_map_ref_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_free.argtypes = [C.POINTER(Ref)]
    L.flappie_map_ref_free.restype = None
    L.flappie_pileup_write.argtypes = [C.c_void_p, C.POINTER(Ref), C.POINTER(C.c_uint32), C.POINTER(C.c_ulonglong)]
    L.flappie_pileup_summary_print.argtypes = [C.c_void_p, C.POINTER(Totals), C.c_ulonglong, C.c_ulonglong]
    L.flappie_pileup_summary_print.restype = None
    rng = np.random.default_rng(17)
    records = [R.random_seq(rng, 40), "g", R.random_seq(rng, 23).lower()]
    names = ["lambda", "x", "plasmid.2"]
    text = ">lambda the control\n%s\n>x\ng\n>plasmid.2\tcircular\n%s\n" % (records[0], records[2])
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_parse(text.encode(), err, 256)
    assert ref, err.value
    p = PU.Pileup([len(r) for r in records], 500)
    for q, a, b, call, ops in random_alignments(rng, p.lens, 60):
        p.add(q, a, b, call, ops)
    assert p.totals["reads"] > 20 and p.totals["skipped"] > 0 and 0 < int((p.depth() >= 1).sum()) and int(p.counts[:, 5].sum()) > 0
    p.counts[1, 2, 7] = (1 << 32) - 1                         # a counter at its largest value is written as it stands
    libc = C.CDLL(None)
    tsv, summ = tmp_path / "pileup.tsv", tmp_path / "summary.txt"
    f = _cfile(libc, tsv)
    covered = C.c_ulonglong(0)
    flat = np.ascontiguousarray(p.counts.reshape(12, p.P))
    assert L.flappie_pileup_write(f, ref, flat.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(covered)) == 0
    libc.fclose(f)
    assert L.flappie_pileup_write(None, ref, flat.ctypes.data_as(C.POINTER(C.c_uint32)), None) == -1
    got = tsv.read_text()
    assert got == p.tsv(names, records)
    lines = got.splitlines()
    assert len(lines) == p.P and all(len(ln.split("\t")) == 16 for ln in lines)
    assert lines[40].split("\t")[:3] == ["x", "0", "G"] and lines[41].split("\t")[:3] == ["plasmid.2", "0", records[2][0].upper()]
    for ln in lines:                                          # depth is the ten base and del counts
        v = [int(x) for x in ln.split("\t")[3:]]
        assert v[0] == sum(v[1:6]) + sum(v[7:12])
    want = p.stderr_lines()
    assert covered.value == want["covered"]
    f = _cfile(libc, summ)
    t = Totals(*[p.totals[k] for k in PU.TOTALS])
    L.flappie_pileup_summary_print(f, C.byref(t), p.P, covered)
    libc.fclose(f)
    assert summ.read_text() == "".join("pileup\t%s\t%d\n" % (k, want[k]) for k in ("reads", "skipped", "positions", "covered", "match", "mismatch", "del", "ins", "edge_ins"))
    L.flappie_map_ref_free(ref)


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--map-pileup=" in r.stdout and "--map-pileup-min-identity=" in r.stdout, r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--map-pileup" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    hits, acc, tsv = str(tmp_path / "hits.tsv"), str(tmp_path / "acc.tsv"), str(tmp_path / "pileup.tsv")
    mapped = ["--map", str(fa), "--map-out", hits]
    aligned = mapped + ["--truth-from-map", "--truth-out", acc]
    assert "--map-pileup goes with --truth-from-map" in refused(FLAPPIE, "--map-pileup", tsv)
    assert "--map-pileup goes with --truth-from-map" in refused(FLAPPIE, *mapped, "--map-pileup", tsv)
    assert "--map-pileup-min-identity goes with --map-pileup" in refused(FLAPPIE, *aligned, "--map-pileup-min-identity", "900")
    for bad in ("-1", "1001", "90x", ""):
        assert "--map-pileup-min-identity must be a whole number from 0 to 1000" in refused(FLAPPIE, *aligned, "--map-pileup", tsv, "--map-pileup-min-identity", bad)
    assert "cannot be written" in refused(FLAPPIE, *aligned, "--map-pileup", str(tmp_path / "no" / "pileup.tsv"))
    assert not os.path.exists(tsv)                            # refused at option parsing: no file, no GPU
    for args in (["--map-pileup", tsv], ["--map-pileup-min-identity", "900"]):
        assert "--map-pileup and --map-pileup-min-identity are flappie's" in refused(RUNNIE, *args)
