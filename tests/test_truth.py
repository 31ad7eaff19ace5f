"""flappie --truth on the CPU: the restatement (truth_ref.py) against an independent unbanded dynamic programme; hand cases; the line of acc.tsv, the CIGAR and
the summary of libflappie_host.so (include/flappie_truth.h) through ctypes; the options and their refusals; the library's new entries.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import truth_ref as T
from test_cli import FLAPPIE, HOSTLIB, ROOT, RUNNIE, _cfile, needs_hdf5

U8P = C.POINTER(C.c_uint8)
LIBFFHIP = os.path.join(ROOT, "flappie_amd", "libffhip.so")


def brute(s, t):
    """plain double loop over the full matrix, and the traceback's rule: (dist, ops)"""
    n, m = len(s), len(t)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for j in range(m + 1):
        for i in range(n + 1):
            if j == 0 and i == 0:
                continue
            best = None
            if j > 0 and i > 0:
                best = D[j - 1][i - 1] + (1 if s[i - 1] != t[j - 1] else 0)
            if j > 0:
                best = D[j - 1][i] + 1 if best is None else min(best, D[j - 1][i] + 1)
            if i > 0:
                best = D[j][i - 1] + 1 if best is None else min(best, D[j][i - 1] + 1)
            D[j][i] = best
    ops, j, i = [], m, n
    while j or i:
        if j and i and D[j - 1][i - 1] + (1 if s[i - 1] != t[j - 1] else 0) == D[j][i]:
            ops.append(1 if s[i - 1] != t[j - 1] else 0)
            j, i = j - 1, i - 1
        elif j and D[j - 1][i] + 1 == D[j][i]:
            ops.append(3)
            j -= 1
        else:
            ops.append(2)
            i -= 1
    return D[m][n], ops[::-1]


def test_restatement_equals_the_unbanded_programme():
    rng = np.random.default_rng(5)
    for k in range(400):
        nl = (2, 3, 4)[k % 3]
        n, m = int(rng.integers(0, 41)), int(rng.integers(1, 41))
        s, t = rng.integers(0, nl, n), rng.integers(0, nl, m)
        rec = T.truth(s, t, max(n, m) + int(rng.integers(0, 3)))
        dist, ops = brute(list(s), list(t))
        assert rec["status"] == 1 and rec["dist"] == dist and list(rec["ops"]) == ops, (n, m, s, t)
        assert rec["maxdev"] <= max(n, m)


def _ops(rec):
    return "".join(T.OPS[o] for o in rec["ops"])


def test_hand_cases():
    r = T.truth("ACGTAC", [0, 1, 2, 3, 0, 1], 3)
    assert (r["status"], r["dist"], _ops(r), r["maxdev"]) == (1, 0, "======", 0)
    r = T.truth("ACGTAC", [0, 1, 3, 3, 0, 1], 0)             # one substitution stays on the centre line: W = 0 with n == m
    assert (r["status"], r["dist"], _ops(r), r["n_mismatch"]) == (1, 1, "==X===", 1)
    # a homopolymer indel: the traceback prefers the diagonal from the END, so the gap stands at the FRONT of the run
    r = T.truth("CAAAG", [1, 0, 0, 0, 0, 2], 4)
    assert (r["dist"], _ops(r), r["n_del"]) == (1, "=D====", 1)
    r = T.truth("CAAAAG", [1, 0, 0, 0, 2], 4)
    assert (r["dist"], _ops(r), r["n_ins"]) == (1, "=I====", 1)
    r = T.truth("", [0, 1, 2], 0)                            # n = 0: m deletions, on the centre line at every band
    assert (r["status"], r["dist"], _ops(r), r["maxdev"]) == (1, 3, "DDD", 0)
    r = T.truth("ACG", [], 5)                                # m = 0
    assert (r["status"], r["n"], r["m"], r["dist"], r["ops"].size) == (2, 3, 0, 0, 0)
    r = T.truth("ACGT", [0, 1, 2], 0)                        # W = 0 with n != m: c(j) = floor(4 j / 3) skips i = 3
    assert r["status"] == 2 and (r["n"], r["m"]) == (4, 3)
    assert T.truth("ACGT", [0, 1, 2], 1)["status"] == 1
    # Z is C on both sides
    r = T.truth("AZGC", [0, 1, 2, 4], 2)
    assert (r["dist"], _ops(r)) == (0, "====")
    # the band changes the answer when the best path leaves it
    s, t = "GACTACTACTACT", T.call_codes("ACTACTACTACTG")      # a rotation by one: one insertion and one deletion, or thirteen mismatches on the diagonal
    wide, tight = T.truth(s, t, 2), T.truth(s, t, 0)
    assert (wide["dist"], wide["maxdev"], _ops(wide)) == (2, 1, "I============D") and (tight["status"], tight["dist"], tight["maxdev"]) == (1, 13, 0)
    assert [T.centre(j, 7, 4) for j in range(5)] == [0, 1, 3, 5, 7]
    assert T.cigar([0] * 12 + [1, 2, 2, 3, 0]) == "12=1X2I1D1=" and T.cigar([]) == "*"


class Rec(C.Structure):
    _fields_ = [("status", C.c_int), ("n", C.c_size_t), ("m", C.c_size_t), ("band", C.c_int), ("maxdev", C.c_int), ("dist", C.c_int), ("n_match", C.c_int),
                ("n_mismatch", C.c_int), ("n_ins", C.c_int), ("n_del", C.c_int)]


class Summary(C.Structure):
    _fields_ = [("aligned", C.c_ulonglong), ("not_aligned", C.c_ulonglong), ("no_record", C.c_ulonglong), ("band_touched", C.c_ulonglong), ("matches", C.c_ulonglong),
                ("columns", C.c_ulonglong), ("identity", C.POINTER(C.c_double)), ("nid", C.c_size_t), ("cap", C.c_size_t)]


def _host():
    L = C.CDLL(HOSTLIB)
    L.flappie_truth_identity.restype = C.c_double
    L.flappie_truth_identity.argtypes = [C.POINTER(Rec)]
    L.flappie_truth_write_cigar.restype = C.c_long
    L.flappie_truth_write_cigar.argtypes = [C.c_void_p, U8P, C.c_size_t]
    L.flappie_truth_write_line.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Rec), U8P, C.c_size_t]
    L.flappie_truth_summary_add.argtypes = [C.POINTER(Summary), C.POINTER(Rec)]
    L.flappie_truth_summary_pooled.restype = C.c_double
    L.flappie_truth_summary_pooled.argtypes = [C.POINTER(Summary)]
    L.flappie_truth_summary_median.restype = C.c_double
    L.flappie_truth_summary_median.argtypes = [C.POINTER(Summary)]
    L.flappie_truth_summary_print.restype = None
    L.flappie_truth_summary_print.argtypes = [C.c_void_p, C.POINTER(Summary)]
    L.flappie_truth_summary_free.restype = None
    L.flappie_truth_summary_free.argtypes = [C.POINTER(Summary)]
    return L


def _crec(rec, band):
    return Rec(rec["status"], rec["n"], rec["m"], band, rec["maxdev"], rec["dist"], rec["n_match"], rec["n_mismatch"], rec["n_ins"], rec["n_del"])


def test_line_cigar_and_summary_of_the_host_layer(tmp_path):
    L = _host()
    libc = C.CDLL(None)
    rng = np.random.default_rng(2)
    recs = [("same", T.truth("ACGTACGTACGTACG", [0, 1, 2, 3] * 3 + [0, 1, 2], 4), 4),              # a run longer than 9
            ("allins", T.truth("ACGTACGTACGT", [3], 12), 12),
            ("alldel", T.truth("", [0] * 23, 0), 0),
            ("none", T.truth("ACGT", [], 3), 3),
            ("nopath", T.truth("ACGT", [0, 1, 2], 0), 0)]
    s = rng.integers(0, 4, 300)
    t = np.delete(s, [5, 6, 7, 100, 250])
    t[50] ^= 1
    recs.append(("mixed", T.truth(s, t, 16), 16))
    assert T.cigar(recs[0][1]["ops"]) == "15=" and recs[1][1]["n_ins"] == 11 and T.cigar(recs[2][1]["ops"]) == "23D"
    out = tmp_path / "acc.tsv"
    fh = _cfile(libc, out)
    want = ""
    for name, rec, band in recs:
        c = _crec(rec, band)
        ops = np.ascontiguousarray(rec["ops"], np.uint8)
        assert L.flappie_truth_write_line(fh, name.encode(), C.byref(c), ops.ctypes.data_as(U8P) if ops.size else None, ops.size) == 0
        want += T.tsv_line(name, rec, band)
        assert L.flappie_truth_identity(C.byref(c)) == T.identity(rec)
    # ops that do not fit the counts write nothing
    c = _crec(recs[0][1], 4)
    bad = np.zeros(14, np.uint8)
    assert L.flappie_truth_write_line(fh, b"bad", C.byref(c), bad.ctypes.data_as(U8P), bad.size) == -1
    bad = np.full(15, 4, np.uint8)
    assert L.flappie_truth_write_line(fh, b"bad", C.byref(c), bad.ctypes.data_as(U8P), bad.size) == -1
    assert L.flappie_truth_write_cigar(fh, bad.ctypes.data_as(U8P), bad.size) == -1
    libc.fclose(fh)
    assert out.read_text() == want
    # an all-insertion path, as given ops: the host layer takes ops as they come
    allins = tmp_path / "allins.tsv"
    fh = _cfile(libc, allins)
    c = Rec(1, 12, 0, 7, 7, 12, 0, 0, 12, 0)
    ins = np.full(12, 2, np.uint8)
    assert L.flappie_truth_write_line(fh, b"ins", C.byref(c), ins.ctypes.data_as(U8P), ins.size) == 0
    assert L.flappie_truth_identity(C.byref(c)) == 0.0
    fputc = libc.fputc
    fputc.argtypes = [C.c_int, C.c_void_p]
    assert L.flappie_truth_write_cigar(fh, ins.ctypes.data_as(U8P), ins.size) == 3 and fputc(10, fh) == 10
    assert L.flappie_truth_write_cigar(fh, ins.ctypes.data_as(U8P), 0) == 1
    libc.fclose(fh)
    assert allins.read_text() == "ins\t1\t12\t0\t7\t7\t12\t0\t0\t12\t0\t0.000000\t12I\n12I\n*"
    assert want.split("\n")[0] == "same\t1\t15\t15\t4\t0\t0\t15\t0\t0\t0\t1.000000\t15="
    assert want.split("\n")[3] == "none\t2\t4\t0\t3\t*\t*\t*\t*\t*\t*\t*\t*"
    mixed = recs[-1][1]
    assert mixed["dist"] <= 6 and mixed["n_ins"] - mixed["n_del"] == 5 and re.fullmatch(r"(\d+[=XID])+", T.cigar(mixed["ops"]))

    # the summary: pooled identity, and the median of an odd and of an even count
    def rec_of(match, mis):
        return Rec(1, match + mis, match + mis, 8, 8 if mis == 3 else 0, mis, match, mis, 0, 0)
    sm = Summary()
    ids = []
    for k, (match, mis) in enumerate(((9, 1), (5, 5), (7, 3), (10, 0), (6, 4))):
        r = rec_of(match, mis)
        assert L.flappie_truth_summary_add(C.byref(sm), C.byref(r)) == 0
        ids.append(match / (match + mis))
        med = L.flappie_truth_summary_median(C.byref(sm))
        srt = sorted(ids)
        assert med == (srt[len(srt) // 2] if len(srt) % 2 else 0.5 * (srt[len(srt) // 2 - 1] + srt[len(srt) // 2])), (k, med)
    r2 = Rec(2, 4, 0, 8, 0, 0, 0, 0, 0, 0)
    assert L.flappie_truth_summary_add(C.byref(sm), C.byref(r2)) == 0 and L.flappie_truth_summary_add(C.byref(sm), None) == 0
    assert (sm.aligned, sm.not_aligned, sm.no_record, sm.band_touched, sm.matches, sm.columns) == (5, 1, 1, 1, 37, 50)
    assert L.flappie_truth_summary_pooled(C.byref(sm)) == 37 / 50
    txt = tmp_path / "summary.txt"
    fh = _cfile(libc, txt)
    L.flappie_truth_summary_print(fh, C.byref(sm))
    libc.fclose(fh)
    assert txt.read_text() == ("truth\taligned\t5\ntruth\tnot_aligned\t1\ntruth\tno_record\t1\ntruth\tband_touched\t1\ntruth\tpooled_identity\t0.740000\n"
                               "truth\tmedian_identity\t0.700000\n")
    L.flappie_truth_summary_free(C.byref(sm))
    empty = Summary()
    assert L.flappie_truth_summary_median(C.byref(empty)) == 0.0 and L.flappie_truth_summary_pooled(C.byref(empty)) == 0.0


@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    refs = tmp_path / "refs.fa"
    refs.write_text(">a\nACGT\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--truth=", "--truth-out=", "--truth-band="):
        assert opt in r.stdout, opt
    for line in r.stdout.split("\n"):                     # long options only
        if re.search(r"--truth(-out|-band)?=", line):
            assert re.match(r"^ {6}--truth(-out|-band)?=", line), line
    flat = " ".join(r.stdout.split())
    assert "0-1279" in flat and "--reverse and --trim-barcodes do not alter it" in flat
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--truth" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out = tmp_path / "acc.tsv"
    assert "--truth" in refused(RUNNIE, "--truth", str(refs))
    assert "--truth-out" in refused(FLAPPIE, "--truth", str(refs))
    assert "--truth" in refused(FLAPPIE, "--truth-out", str(out))
    assert "--truth" in refused(FLAPPIE, "--truth-band", "5")
    for w in ("-1", "1280", "100000", "12x", ""):
        assert "--truth-band" in refused(FLAPPIE, "--truth", str(refs), "--truth-out", str(out), "--truth-band", w)
    assert "missing.fa" in refused(FLAPPIE, "--truth", str(tmp_path / "missing.fa"), "--truth-out", str(out))
    assert not out.exists()


def test_library_exports_the_new_entries():
    lib = C.CDLL(LIBFFHIP)
    for name in ("ffhip_batch_set_truth", "ffhip_batch_truth", "ffhip_op_truth", "ffhip_debug_truth_form"):
        assert hasattr(lib, name), name
    lib.ffhip_debug_truth_form.argtypes = [C.c_size_t]
    # one wave up to 256 cells, a workgroup up to 2560 (W = 1024 needs 2049), none beyond
    assert [lib.ffhip_debug_truth_form(w) for w in (0, 1, 63, 64, 65, 256, 257, 1025, 1280, 1281, 2049, 2560, 2561)] == [-1, 0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 3, -1]
    from flappie_amd import binding
    assert binding.RUN_TRUTH == 65536 and binding.TRUTH_BAND_MAX == 1279 and 2 * binding.TRUTH_BAND_MAX + 1 <= 2560
    assert hasattr(binding.Batch, "set_truth") and hasattr(binding.Batch, "truth") and hasattr(binding, "op_truth") and binding.truth_form(2049) == 3
