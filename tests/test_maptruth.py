"""flappie --truth-from-map without a GPU: the restatement (maptruth_ref.py) and the bound the sizing rests on against a brute-force sweep; the host side
(flappie_align.c of libflappie_host.so: the line of acc.tsv in the mode, the aligned SAM file) against the restatement and against a replay of every line over
the reference; header, binding and library agree on the three new calls; the command line's refusals.  Everything is integer- or byte-exact."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import map_ref as R
import maptruth_ref as MT
import truth_ref as T
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5
from test_map import Call, Ref, brute_record, c_call

NEW_CALLS = ("ffhip_batch_set_truth_from_map", "ffhip_op_map_stretch", "ffhip_debug_map_truth_bound")


# ------------------------------------------------------------------------------------ the restatement and the bound
def test_the_bound_and_the_stretch_on_every_small_call():
    """every call of 1 .. 6 bases over two letters against references of 1 .. 10 bases, both strands, e in {0, 250, 500}, window 64: a mapped call of n bases has
    1 <= m <= n + floor(n e / 1000), and its stretch is the text --map-records writes"""
    rng = np.random.default_rng(3)
    refs = []
    for m in range(1, 11):                                     # (A and T: a two-letter alphabet whose reverse complement stays inside it, so both strands are hit)
        refs += [["".join(ab[i] for i in rng.integers(0, 2, m))] for ab in ("AC", "AT", "AT")]
    refs += [["ACCA", "CAC"], ["A", "CCCCCCCCCC"], ["ATTA", "TTTAT"], ["T", "AAAAATAAAA"]]
    seen = {"mapped": 0, "minus": 0, "at the bound": 0, "longer": 0, "shorter": 0}
    rows_of = {}
    for records in refs:
        ys = R.searches(records)
        for n in range(1, 7):
            for letters in itertools.product("AT" if "T" in "".join(records) else "AC", repeat=n):
                call = "".join(letters)
                key = (tuple(records), call)
                rows_of[key] = R.score_rows(records, call)
                for e in (0, 250, 500):
                    mp = R.record(records, call, 64, e, rows=rows_of[key])
                    assert R.raw(mp).tolist() == brute_record(records, call, 64, e), (records, call, e)      # the place by the recurrence as written
                    text = MT.stretch_text(records, mp)
                    if mp["status"] != 1:
                        assert text is None
                        continue
                    m = mp["tend"] - mp["tstart"]
                    assert 1 <= m <= n + n * e // 1000, (records, call, e, mp)
                    assert m <= MT.bound(n - 1, e)                      # n <= nblock + 1
                    assert R.record_text("r", mp, records) == ">r\n%s\n" % text and len(text) == m
                    assert np.array_equal(MT.stretch(records, mp["q"], mp["tstart"], mp["tend"]), MT.codes(text))
                    assert text == ys[mp["q"]][mp["tstart"]:mp["tend"]]
                    seen["mapped"] += 1
                    seen["minus"] += mp["q"] & 1
                    seen["at the bound"] += m == n + n * e // 1000 and e > 0 and m > n
                    seen["longer"] += m > n
                    seen["shorter"] += m < n
    assert seen["mapped"] > 2000 and seen["minus"] > 100 and seen["at the bound"] > 0 and seen["shorter"] > 0, seen
    # the truth of a read in the mode: the stretch aligned as under "truth", or no truth
    records = ["ACCATTGACCAGGTTACA", "GGATC"]
    for call, status in (("TTGZCCAG", 1), ("TGTAACC", 1), ("GGGGGGGGGGGG", 0), ("", 0)):
        mp, tr = MT.truth_from_map(records, call, 4, 64, 250)
        assert tr["status"] == status and tr["n"] == len(call)
        if status:
            want = T.truth(call, MT.codes(MT.stretch_text(records, mp)), 4)
            assert all(tr[k] == want[k] for k in T.FIELDS) and np.array_equal(tr["ops"], want["ops"])
        else:
            assert tr["m"] == 0 and tr["ops"].size == 0
    assert [MT.bound(N, e) for N, e in ((0, 0), (0, 500), (9, 250), (399, 250), (1000, 1), (1 << 30, 500))] == [1, 1, 12, 500, 1002, (1 << 30) + 1 + ((1 << 30) + 1) // 2]


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    assert lib.ffhip_batch_set_truth_from_map.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.ffhip_op_map_stretch.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    assert lib.ffhip_debug_map_truth_bound.argtypes == [C.c_int, C.c_int] and lib.ffhip_debug_map_truth_bound.restype == C.c_longlong
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("int ffhip_batch_set_truth_from_map(ffhip_batch *b, int on, int band);",
                  "int ffhip_op_map_stretch(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, uint8_t *codes /* end - start */);",
                  "long long ffhip_debug_map_truth_bound(int nblock, int max_error);"):
        assert proto in header, proto
    assert callable(B.Batch.set_truth_from_map) and callable(B.op_map_stretch) and callable(B.map_truth_bound)
    # the sizing rule needs no device: the library's bound is the header's
    for N in (0, 1, 2, 3, 7, 399, 400, 1000, 45670, (1 << 24), (1 << 31) - 1):
        for e in (0, 1, 249, 250, 500):
            assert B.map_truth_bound(N, e) == MT.bound(N, e), (N, e)
    assert B.map_truth_bound(-1, 250) == -1 and B.map_truth_bound(10, 501) == -1 and B.map_truth_bound(10, -1) == -1
    # the host library has the header's functions
    H = C.CDLL(HOSTLIB)
    assert sorted(_declared_functions("flappie_align.h")) == ["flappie_align_write_acc_line", "flappie_align_write_sam_header", "flappie_align_write_sam_line"]
    assert all(hasattr(H, n) for n in _declared_functions("flappie_align.h")) and hasattr(H, "flappie_truth_write_fields")


# ------------------------------------------------------------------------------------ the host side
class TruthRec(C.Structure):
    _fields_ = [("status", C.c_int), ("n", C.c_size_t), ("m", C.c_size_t)] + [(k, C.c_int) for k in ("band", "maxdev", "dist", "n_match", "n_mismatch", "n_ins", "n_del")]


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_map_ref_parse.restype = C.POINTER(Ref)
    L.flappie_map_ref_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_free.argtypes = [C.POINTER(Ref)]
    L.flappie_map_ref_free.restype = None
    u8 = C.POINTER(C.c_uint8)
    L.flappie_align_write_acc_line.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(TruthRec), u8, C.c_size_t, C.POINTER(Call), C.POINTER(Ref)]
    L.flappie_align_write_sam_header.argtypes = [C.c_void_p, C.POINTER(Ref)]
    L.flappie_align_write_sam_header.restype = None
    L.flappie_align_write_sam_line.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(TruthRec), u8, C.c_size_t, C.POINTER(Call), C.POINTER(Ref)]
    return L


def c_truth(tr, band):
    return TruthRec(tr["status"], tr["n"], tr["m"], band, tr["maxdev"], tr["dist"], tr["n_match"], tr["n_mismatch"], tr["n_ins"], tr["n_del"])


def c_ops(ops):
    a = np.ascontiguousarray(ops, np.uint8)
    return (a if a.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), a


def test_acc_lines_and_sam_lines_replay_over_the_reference(L, tmp_path):
    rng = np.random.default_rng(5)
    records = [R.random_seq(rng, 300), R.random_seq(rng, 170), "G"]
    names = ["lambda", "plasmid.2", "x"]
    lens = [len(r) for r in records]
    text = ">lambda the control\n%s\n>plasmid.2\tcircular\n%s\n>x\nG\n" % (records[0], records[1])
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_parse(text.encode(), err, 256)
    assert ref, err.value
    ys = R.searches(records)
    band = 16
    calls = []
    for i, (q, a, b, rate) in enumerate(((0, 10, 90, 0.0), (1, 20, 130, 0.08), (2, 0, 170, 0.1), (3, 100, 170, 0.05), (0, 220, 300, 0.12), (1, 0, 60, 0.1), (4, 0, 1, 0.0),
                                         (5, 0, 1, 0.0), (3, 3, 80, 0.15))):
        c = R.edit(rng, ys[q][a:b], rate) if rate else ys[q][a:b]
        calls.append(c.replace("C", "Z", 2) if i % 2 else c)
    calls += [R.random_seq(rng, 60), ""]                       # one that does not map, one without a base
    libc = C.CDLL(None)
    acc, sam = tmp_path / "acc.tsv", tmp_path / "aln.sam"
    fa, fs = _cfile(libc, acc), _cfile(libc, sam)
    L.flappie_align_write_sam_header(fs, ref)
    want_acc, want_sam, kept = [], [], []
    seen = {"+": 0, "-": 0, "X": 0, "I": 0, "D": 0, "unmapped": 0, "band": 0}
    for i, call in enumerate(calls):
        name = "read-%d" % i
        qual = "".join(chr(33 + int(v)) for v in rng.integers(0, 40, len(call)))
        mp, tr = MT.truth_from_map(records, call, band, 64, 250)
        if i == 8:                                             # aligned in a band that leaves no path: truth status 2 on a mapped read
            tr = MT.no_truth(len(call))
            tr.update(status=2, m=mp["tend"] - mp["tstart"])
            seen["band"] += 1
        ctr, cmp_ = c_truth(tr, band), c_call(mp)
        po, keep = c_ops(tr["ops"])
        kept.append(keep)
        if mp["status"] == 1:
            assert L.flappie_align_write_acc_line(fa, name.encode(), C.byref(ctr), po, tr["ops"].size, C.byref(cmp_), ref) == 0
            want_acc.append(MT.acc_line(name, tr, band, mp, names, lens))
        else:
            assert L.flappie_align_write_acc_line(fa, name.encode(), C.byref(ctr), po, 0, C.byref(cmp_), ref) == -1      # (nothing written: a line per MAPPED read)
            seen["unmapped"] += 1
        if not call:
            continue                                           # no call: no line
        rc = L.flappie_align_write_sam_line(fs, name.encode(), call.encode(), qual.encode(), len(call), C.byref(ctr), po, tr["ops"].size, C.byref(cmp_), ref)
        assert rc == (1 if mp["status"] == 1 and tr["status"] == 1 else 0), (i, rc)
        want_sam.append(MT.sam_line(name, call, qual, tr, mp, names, lens))
        if rc == 1:
            got = MT.replay(want_sam[-1], dict(zip(names, records)))
            k, o, a, b = R.forward(mp["q"], mp["tstart"], mp["tend"], lens)
            assert (got["start"], got["end"], got["nm"]) == (a, b, tr["dist"]) and got["flag"] == (16 if o == "-" else 0)
            f = want_sam[-1].split("\t")
            assert f[9] == (call.replace("Z", "C") if o == "+" else R.revcomp(call.replace("Z", "C"))) and f[10] == (qual if o == "+" else qual[::-1])
            assert f[5] == T.cigar(tr["ops"] if o == "+" else tr["ops"][::-1])
            seen[o] += 1
            for c in "XID":
                seen[c] += c in f[5]
    # a record that does not fit the reference, and ops that do not fit the call
    mp, tr = MT.truth_from_map(records, calls[0], band, 64, 250)
    bad = c_call(mp)
    bad.v[5] = 1000
    ctr = c_truth(tr, band)
    po, keep = c_ops(tr["ops"])
    assert L.flappie_align_write_acc_line(fa, b"bad", C.byref(ctr), po, tr["ops"].size, C.byref(bad), ref) == -1
    assert L.flappie_align_write_sam_line(fs, b"bad", calls[0].encode(), b"5" * len(calls[0]), len(calls[0]), C.byref(ctr), po, tr["ops"].size, C.byref(bad), ref) == -1
    good = c_call(mp)
    assert L.flappie_align_write_sam_line(fs, b"bad", calls[0].encode(), b"5" * len(calls[0]), len(calls[0]), C.byref(ctr), po, tr["ops"].size - 1, C.byref(good), ref) == -1
    assert L.flappie_align_write_acc_line(fa, b"bad", C.byref(ctr), po, tr["ops"].size - 1, C.byref(good), ref) == -1
    # a read without a truth record at all: unmapped
    assert L.flappie_align_write_sam_line(fs, b"bare", b"ACZT", b"!!!!", 4, None, None, 0, None, ref) == 0
    want_sam.append("bare\t4\t*\t0\t0\t*\t*\t0\t0\tACCT\t!!!!\n")
    libc.fclose(fa)
    libc.fclose(fs)
    L.flappie_map_ref_free(ref)
    assert acc.read_text() == "".join(want_acc)
    assert sam.read_text() == MT.sam_header(names, lens) + "".join(want_sam)
    assert sam.read_text().startswith("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:lambda\tLN:300\n@SQ\tSN:plasmid.2\tLN:170\n@SQ\tSN:x\tLN:1\n@PG\tID:flappie\nread-0\t0\tlambda\t11\t255\t80=\t*\t0\t0\t")
    assert all(len(line.split("\t")) == 17 for line in acc.read_text().splitlines())
    assert seen["+"] >= 3 and seen["-"] >= 3 and min(seen[c] for c in "XID") >= 2 and seen["unmapped"] == 2 and seen["band"] == 1, seen


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--truth-from-map" in r.stdout and "--map-sam=" in r.stdout, r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--truth-from-map" not in r.stdout and "--map-sam" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    hits, acc, sam = str(tmp_path / "hits.tsv"), str(tmp_path / "acc.tsv"), str(tmp_path / "aln.sam")
    mapped = ["--map", str(fa), "--map-out", hits]
    assert "--truth-from-map goes with --map" in refused(FLAPPIE, "--truth-from-map", "--truth-out", acc)
    assert "--truth-from-map does not go with --truth" in refused(FLAPPIE, *mapped, "--truth-from-map", "--truth", str(fa), "--truth-out", acc)
    assert "--truth-from-map and --truth-out go together" in refused(FLAPPIE, *mapped, "--truth-from-map")
    assert "--map-sam goes with --truth-from-map" in refused(FLAPPIE, *mapped, "--map-sam", sam)
    assert "--map-sam goes with --truth-from-map" in refused(FLAPPIE, "--map-sam", sam)
    assert "--truth-band goes with --truth or --truth-from-map" in refused(FLAPPIE, *mapped, "--truth-band", "100")
    assert "--truth and --truth-out go together" in refused(FLAPPIE, *mapped, "--truth-out", acc)
    assert "must be a whole number" in refused(FLAPPIE, *mapped, "--truth-from-map", "--truth-out", acc, "--truth-band", "1280")
    assert "cannot be written" in refused(FLAPPIE, *mapped, "--truth-from-map", "--truth-out", str(tmp_path / "no" / "acc.tsv"))
    assert "--map-sam" in refused(FLAPPIE, *mapped, "--truth-from-map", "--truth-out", acc, "--map-sam", str(tmp_path / "no" / "aln.sam"))
    assert not os.path.exists(sam)
    for args in (["--truth-from-map"], ["--map-sam", sam]):
        assert "flappie's" in refused(RUNNIE, *args)
    assert re.search(r"--truth-from-map and --map-sam are flappie's", refused(RUNNIE, "--truth-from-map", "--map-sam", sam))
