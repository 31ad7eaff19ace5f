"""flappie --remap-variants on the CPU: the restatement of include/ffhip.h "variants" (variants_ref.py) against a brute-force enumeration of every monotone path
on tiny windows, for every kind of edit; its identities with "site mods" and with remap; the window's limits; the reader of the variants' file and the writer of
the table in libflappie_host.so (include/flappie_variants.h) through ctypes; the options and their refusals; the library's new entries.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import remap_ref as RR
import sitemods_ref as S
import variants_ref as V
from test_cli import FLAPPIE, HOSTLIB, ROOT, RUNNIE, _cfile, needs_hdf5
from test_remap import Refs

LIBFFHIP = os.path.join(ROOT, "flappie_amd", "libffhip.so")


def _path(rng, N, L):
    rm = np.zeros(N, np.uint8)
    rm[rng.choice(N, L - 1, replace=False)] = 1
    return rm


def kinds_of(codes, nbase, p, r, alt, c):
    """the kinds of include/ffhip.h "variants" an edit belongs to (the names the tests count)"""
    L, k = len(codes), len(alt)
    ref = [int(x) for x in codes[p:p + r]]
    out = set()
    if r == k and ref == list(alt):
        out.add("same")
    elif r == k == 1:
        out.add("snp")
    elif r == k:
        out.add("mnp")
    if r == 0:
        out |= {"ins"} | ({"ins at 0"} if p == 0 else set()) | ({"ins at L"} if p == L else set())
    if k == 0:
        out |= {"del"} | ({"del at the start"} if p == 0 else set()) | ({"del at the end"} if p + r == L else set())
    q_ref, q_alt = V.hypotheses(codes, nbase, p, r, alt)
    lo, hi = max(0, p - c), min(L - 1, p + r + c - 1)
    last = hi - r + k                                           # the alt window's last position
    if q_alt[last] != q_ref[hi] and q_alt[last] % nbase == q_ref[hi] % nbase and last >= p + k:
        out.add("flip at hi")                                   # behind the edit the same letters, coded the other way round up to the window's end ...
        if hi < L - 1 and q_alt[last + 1] != q_ref[hi + 1]:
            out.add("flip past hi")                             # ... and beyond it
    return out


def test_restatement_against_every_path_of_tiny_windows():
    rng = np.random.default_rng(23)
    seen = {}
    for trial in range(80):
        nbase = 4 + trial % 2
        N = int(rng.integers(1, 9))
        L = int(rng.integers(1, min(N + 1, 6) + 1))
        codes = rng.integers(0, int(rng.integers(1, 4)), L).astype(np.uint8) + (nbase - 3)          # few letters: runs are common; the last letters of the alphabet
        rm = _path(rng, N, L)
        # sums of small dyadic fractions are exact in float32 in any order: the best path's score does not depend on the order of the adds
        T = (rng.integers(-64, 65, (N, 2 * nbase * (nbase + 1))) / 8.0).astype(np.float32)
        st = S.starts(rm, L)
        cands = []
        for p in range(L + 1):
            for r in range(0, min(2, L - p) + 1):
                for k in range(0, 3):
                    alts = [[int(x) for x in rng.integers(nbase - 3, nbase, k)], [int(x) for x in codes[p:p + r]][:k] + [int(codes[min(p, L - 1)])] * max(0, k - r)]
                    for alt in alts:
                        if V.valid(L, nbase, p, r, alt):
                            cands.append((p, r, alt))
        for p, r, alt in cands:
            c = 1 + (p + r + len(alt)) % 2
            lo, hi, P_ref, P_alt, t0, t1 = V.window(st, L, p, r, len(alt), c)
            if max(P_ref, P_alt) > 5 or t1 - t0 > 7:
                continue
            q_ref, q_alt = V.hypotheses(codes, nbase, p, r, alt)
            rec, rec_all = (V.variants(T, nbase, codes, rm, [(p, r, alt)], c, mode)[0] for mode in (False, True))
            for q, P, f in ((q_ref, P_ref, "ref"), (q_alt, P_alt, "alt")):
                best, logsum = S.brute(T, q, lo, lo + P - 1, t0, t1, nbase)
                assert rec[f].tobytes() == best.tobytes(), (trial, p, r, alt, c, f, rec, best)
                full = S.score_all(T, q, lo, lo + P - 1, t0, t1, nbase)          # fp64; the record holds it rounded to float32 once
                assert full == logsum if np.isinf(logsum) else abs(float(full) - logsum) <= 1e-9, (trial, p, r, alt, c, f, full, logsum)
                assert rec_all[f].tobytes() == np.float32(full).tobytes(), (trial, p, r, alt, c, f)
            assert rec["index"] == 0 and rec["nblock"] == t1 - t0 and rec_all["nblock"] == t1 - t0
            kinds = kinds_of(codes, nbase, p, r, alt, c)
            if rec["alt"] == -np.inf:
                assert t1 - t0 < P_alt - 1                  # exactly -inf, and only where there is no path
                kinds.add("no path")
            else:
                assert t1 - t0 >= P_alt - 1
            if "same" in kinds:
                assert rec["ref"].tobytes() == rec["alt"].tobytes()
            assert rec["ref"] > -np.inf                     # the remap path itself is a path of the ref hypothesis
            for kind in kinds:
                seen[kind] = seen.get(kind, 0) + 1
    need = {"snp": 50, "mnp": 20, "ins": 50, "ins at 0": 10, "ins at L": 10, "del": 50, "del at the start": 10, "del at the end": 10, "flip at hi": 10, "flip past hi": 3,
            "no path": 10, "same": 30}
    for kind, n in need.items():
        assert seen.get(kind, 0) >= n, (kind, seen)


def test_a_run_recoded_behind_the_edit():
    # AAAAAA codes A a A a A a; without position 1 the five letters behind it code a A a A: every state behind the edit differs, at hi and past it
    codes = [0] * 6
    q_ref, q_alt = V.hypotheses(codes, 4, 1, 1, [])
    assert q_ref == [0, 4, 0, 4, 0, 4] and q_alt == [0, 4, 0, 4, 0]
    assert kinds_of(codes, 4, 1, 1, [], 1) >= {"del", "flip at hi", "flip past hi"}
    # a C put between two C: C c C c against C c, and the run ends the difference
    q_ref, q_alt = V.hypotheses([1, 1, 2, 2], 5, 1, 0, [1])
    assert q_ref == [1, 6, 2, 7] and q_alt == [1, 6, 1, 2, 7]
    # Z between two C (the case of "site mods")
    assert V.hypotheses([1, 1, 1], 5, 1, 1, [4])[1] == [1, 4, 1]


def test_snp_between_c_and_z_is_site_mods():
    rng = np.random.default_rng(31)
    n = 0
    for N in (3, 20, 90):
        for L in sorted({1, N + 1, int(rng.integers(1, N + 2))}):
            codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L)
            rm = _path(rng, N, L)
            T = (rng.standard_normal((N, 60)) * 3.0).astype(np.float32)
            for c in (1, 10, 23):
                sm = S.site_mods(T, 5, codes, rm, c)
                vars = [(int(i), 1, [S.CAN + S.MOD - int(codes[i])]) for i in sm["pos"]]
                got = V.variants(T, 5, codes, rm, vars, c)
                for rec, site in zip(got, sm):
                    given_c = codes[site["pos"]] == S.CAN
                    assert rec["nblock"] == site["nblock"]
                    assert rec["ref"].tobytes() == (site["can"] if given_c else site["mod"]).tobytes(), (N, L, c, site)
                    assert rec["alt"].tobytes() == (site["mod"] if given_c else site["can"]).tobytes(), (N, L, c, site)
                    n += 1
    assert n >= 100


def test_whole_window_ref_is_remaps_score():
    rng = np.random.default_rng(37)
    n = 0
    for nbase in (4, 5):
        for N in (1, 7, 40, 90):
            for L in sorted({1, min(N + 1, 24), int(rng.integers(1, min(N + 1, 24) + 1))}):
                codes = rng.integers(0, nbase, L).astype(np.uint8)
                T = (rng.standard_normal((N, 2 * nbase * (nbase + 1))) * 3.0).astype(np.float32)
                score, rm = RR.remap(T, codes, nbase, L)                # unbanded
                vars = [(p, 1, [int(rng.integers(0, nbase))]) for p in range(L)] + [(L - 1, 1, [0, 1]), (0, 1, [2, 3, 0])]
                for rec in V.variants(T, nbase, codes, rm, vars, 23):
                    assert rec["nblock"] == N and rec["ref"].tobytes() == np.float32(score).tobytes(), (nbase, N, L, rec, score)
                    n += 1
    assert n >= 100


def test_limits_of_the_window_over_all_edge_combinations():
    largest = [0, 0]
    for L in (1, 2, 3, 15, 16, 17, 23, 24, 45, 46, 47, 61, 62, 63, 64, 100):
        for c in (1, 2, 10, 22, 23):
            for r in (0, 1, 2, 15, 16):
                for k in (0, 1, 2, 15, 16):
                    for p in {0, 1, c - 1, c, c + 1, L - r - c - 1, L - r - c, L - r - c + 1, L - r - 1, L - r, L // 2}:
                        if not V.valid(L, 4, p, r, [0] * k):
                            continue
                        lo, hi = max(0, p - c), min(L - 1, p + r + c - 1)
                        P_ref = hi - lo + 1
                        P_alt = P_ref - r + k
                        assert 0 <= lo <= hi <= L - 1 and 1 <= P_ref <= 62 and 1 <= P_alt <= 62, (L, c, r, k, p)
                        assert lo + P_alt - 1 <= L - r + k - 1 and (hi < L - 1 or lo + P_alt == L - r + k), (L, c, r, k, p)      # the alt window inside s^alt, at its end with hi
                        largest = [max(largest[0], P_ref), max(largest[1], P_alt)]
    assert largest == [62, 62]
    assert V.VARIANT_DTYPE.itemsize == 24 and V.VARIANT_CALL_DTYPE.itemsize == 16
    assert not V.valid(5, 4, 0, 0, []) and not V.valid(5, 4, 4, 2, [0]) and not V.valid(5, 4, 0, 1, [4]) and V.valid(5, 5, 0, 1, [4])
    assert not V.valid(3, 4, 0, 3, []) and V.valid(3, 4, 0, 3, [1]) and not V.valid(20, 4, 0, 17, [1]) and not V.valid(20, 4, 0, 1, [0] * 17)


# ------------------------------------------------------------------------------------ the file's reader and the table's writer
KINDS = ("malformed", "letter", "long", "no record", "beyond", "ref mismatch")


class Variants(C.Structure):
    _fields_ = [("n", C.c_size_t), ("rec", C.POINTER(C.c_int)), ("var", C.c_void_p), ("nrec", C.c_int), ("first", C.POINTER(C.c_size_t)), ("idx", C.POINTER(C.c_size_t)),
                ("skipped", C.c_ulonglong * 6), ("skipped_line", C.c_size_t * 6), ("skipped_text", (C.c_char * 128) * 6)]


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_remap_refs_parse.restype = C.POINTER(Refs)
    L.flappie_remap_refs_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_remap_refs_free.argtypes = [C.POINTER(Refs)]
    L.flappie_variants_parse.restype = C.POINTER(Variants)
    L.flappie_variants_parse.argtypes = [C.c_char_p, C.POINTER(Refs), C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_variants_read.restype = C.POINTER(Variants)
    L.flappie_variants_read.argtypes = [C.c_char_p, C.POINTER(Refs), C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_variants_free.argtypes = [C.POINTER(Variants)]
    L.flappie_variants_of.restype = C.c_size_t
    L.flappie_variants_of.argtypes = [C.POINTER(Variants), C.c_int, C.c_void_p]
    L.flappie_variants_kind.restype = C.c_char_p
    L.flappie_variants_write.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_char_p, C.c_void_p, C.c_void_p, C.c_size_t]
    return L


FASTA = b">r1 first\nACGTACGTAC\n>r2\nAAAA\n>bad\nACNT\n>r3\nCCZ\n"
# (line, what becomes of it): a kept variant as (record, pos, nref, alt codes), or the kind it is skipped for
LINES = [
    ("# name\tpos\tref\talt", None),
    ("", None),
    ("r1\t0\tA\tC", ("r1", 0, 1, [1])),
    ("r2\t4\t-\tAC", ("r2", 4, 0, [0, 1])),                 # an insertion behind the last base
    ("r1\t2\tGT\t-", ("r1", 2, 2, [])),                     # a deletion
    ("r1\t1\tcg\tTa", ("r1", 1, 2, [3, 0])),                # lower case
    ("reads/r3.fast5\t2\tZ\tC", ("r3", 2, 1, [1])),         # a record found as a read's file finds it; the 5-base alphabet
    ("r1\t0\tA", "malformed"),
    ("r1\t0\tA\tC\tG", "malformed"),
    ("r1\t-1\tA\tC", "malformed"),
    ("r1\t0x1\tA\tC", "malformed"),
    ("r1\t\tA\tC", "malformed"),
    ("r1\t0\t\tC", "malformed"),
    ("\t0\tA\tC", "malformed"),
    ("r1\t0\t-\t-", "malformed"),
    ("r1 0 A C", "malformed"),
    ("r1\t99999999999999999999\tA\tC", "malformed"),
    ("r2\t0\tAAAA\t-", "malformed"),                        # an edit that leaves no base
    ("r1\t0\tA\tN", "letter"),
    ("r1\t0\tA\tC-", "letter"),
    ("r1\t0\tA\t" + "ACGT" * 4 + "A", "long"),
    ("r1\t0\t" + "ACGT" * 5 + "\tA", "long"),
    ("nobody\t0\tA\tC", "no record"),
    ("bad\t0\tA\tC", "no record"),
    ("r1\t10\tA\tC", "beyond"),
    ("r1\t9\tCA\tC", "beyond"),
    ("r1\t11\t-\tC", "beyond"),
    ("r1\t0\tC\tA", "ref mismatch"),
    ("r1\t3\tTAG\tA", "ref mismatch"),
    ("r1\t10\t-\t" + "ACGT" * 4, ("r1", 10, 0, [0, 1, 2, 3] * 4)),      # an allele of 16, behind the last base
    ("r2\t1\tA\tA\r", ("r2", 1, 1, [0])),                   # ref = alt; a carriage return before the line's end
]


def _parsed(L, refs, text, tmp_path=None):
    err = C.create_string_buffer(256)
    if tmp_path is None:
        vs = L.flappie_variants_parse(text, refs, b"ACGTZ", err, 256)
    else:
        (tmp_path / "vars.tsv").write_bytes(text)
        vs = L.flappie_variants_read(str(tmp_path / "vars.tsv").encode(), refs, b"ACGTZ", err, 256)
    assert vs, err.value
    return vs


def test_reader_keeps_and_skips(L, tmp_path):
    err = C.create_string_buffer(256)
    refs = L.flappie_remap_refs_parse(FASTA, b"ACGTZ", err, 256)
    assert refs and refs.contents.n == 4
    names = [refs.contents.name[k].decode() for k in range(4)]
    text = ("\n".join(x for x, _ in LINES) + "\n").encode()
    for vs in (_parsed(L, refs, text), _parsed(L, refs, text, tmp_path), _parsed(L, refs, text[:-1])):      # (the last line without its end)
        v = vs.contents
        want = [w for _, w in LINES if isinstance(w, tuple)]
        assert v.n == len(want) and v.nrec == 4
        got = np.frombuffer(C.string_at(v.var, v.n * 24), V.VARIANT_DTYPE)
        for i, (name, pos, nref, alt) in enumerate(want):                       # in file order
            assert names[v.rec[i]] == name and V.unpack(got[i:i + 1]) == [(pos, nref, alt)], (i, want[i])
            assert not got[i]["pad"].any() and not got[i]["alt"][len(alt):].any()
        for k, kind in enumerate(KINDS):                                        # every kind counted, its first line quoted
            lines = [(n + 1, x) for n, (x, w) in enumerate(LINES) if w == kind]
            assert lines and v.skipped[k] == len(lines), kind
            assert v.skipped_line[k] == lines[0][0] and v.skipped_text[k].value.decode() == lines[0][1][:127], kind
            assert L.flappie_variants_kind(k)
        for k, name in enumerate(names):                                        # a record's variants, in file order
            mine = [w[1:] for w in want if w[0] == name]
            buf = np.zeros(max(1, len(mine)), V.VARIANT_DTYPE)
            assert L.flappie_variants_of(vs, k, None) == len(mine) and L.flappie_variants_of(vs, k, buf.ctypes.data) == len(mine)
            assert V.unpack(buf[:len(mine)]) == [tuple(m) for m in mine], name
        assert L.flappie_variants_of(vs, -1, None) == 0 and L.flappie_variants_of(vs, 4, None) == 0
        L.flappie_variants_free(vs)
    vs = _parsed(L, refs, b"")
    assert vs.contents.n == 0 and sum(vs.contents.skipped) == 0
    L.flappie_variants_free(vs)
    assert not L.flappie_variants_parse(None, refs, b"ACGTZ", err, 256) and err.value
    assert not L.flappie_variants_read(str(tmp_path / "none.tsv").encode(), refs, b"ACGTZ", err, 256) and b"cannot be read" in err.value
    L.flappie_remap_refs_free(refs)


def test_writer(L, tmp_path):
    libc = C.CDLL(None)
    out = tmp_path / "calls.tsv"
    fh = _cfile(libc, out)
    codes = np.array([0, 1, 2, 3, 4, 1], np.uint8)          # ACGTZC
    var = V.pack([(1, 1, [4]), (2, 0, [0, 0]), (3, 2, []), (6, 0, [3]), (0, 1, [0])])
    inf = np.float32(np.inf)
    vc = np.zeros(5, V.VARIANT_CALL_DTYPE)
    vc[0] = (0, 12, np.float32(-3.14159274), np.float32(-2.5))
    vc[1] = (1, 7, np.float32(-1.25), -inf)                  # an alt without a path: the difference is inf
    vc[2] = (2, 0, -inf, -inf)                               # both: 0
    vc[3] = (3, 5, -inf, np.float32(-4.0))                   # (what printf gives)
    vc[4] = (4, 9, np.float32(-1e30), np.float32(-1e30))
    u8 = codes.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.flappie_variants_write(fh, b"read one", u8, 6, b"ACGTZ", var.ctypes.data, vc.ctypes.data, 5) == 0
    assert L.flappie_variants_write(fh, b"none", u8, 6, b"ACGTZ", var.ctypes.data, vc.ctypes.data, 0) == 0
    bad = vc[:1].copy()
    bad["index"] = 1
    assert L.flappie_variants_write(fh, b"x", u8, 6, b"ACGTZ", var.ctypes.data, bad.ctypes.data, 1) == -1      # an index outside the list
    assert L.flappie_variants_write(fh, b"x", u8, 5, b"ACGTZ", var[3:].ctypes.data, vc[:1].ctypes.data, 1) == -1      # a variant beyond the sequence
    libc.fclose(fh)
    a, b = float(np.float32(-3.14159274)), -2.5
    assert out.read_text() == ("read one\t1\tC\tZ\t12\t%.9g\t%.9g\t%.9g\n" % (a, b, a - b) + "read one\t2\t-\tAA\t7\t-1.25\t-inf\tinf\n" + "read one\t3\tTZ\t-\t0\t-inf\t-inf\t0\n"
                               + "read one\t6\t-\tT\t5\t-inf\t-4\t-inf\n" + "read one\t0\tA\tA\t9\t%.9g\t%.9g\t0\n" % (np.float32(-1e30), np.float32(-1e30)))
    assert "nan" not in out.read_text()


# ------------------------------------------------------------------------------------ the options
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    refs = tmp_path / "refs.fa"
    refs.write_text(">r1\nACGT\n")
    vars = tmp_path / "vars.tsv"
    vars.write_text("r1\t0\tA\tC\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--remap-variants=", "--remap-variants-out=", "--remap-variants-context=", "--remap-variants-all-paths"):
        assert any(re.match(r"^ {6}" + re.escape(opt), line) for line in r.stdout.split("\n")), opt      # long options only
    assert "1-23, default" in r.stdout and "10)" in r.stdout.split("--remap-variants-context=")[1][:200]
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--remap-variants" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out, table = tmp_path / "calls.tsv", tmp_path / "map.tsv"
    remap = ["--remap", str(refs), "--remap-out", str(table)]
    assert "--remap-variants goes with --remap" in refused(FLAPPIE, "--remap-variants", str(vars), "--remap-variants-out", str(out))
    assert "--remap-variants and --remap-variants-out go together" in refused(FLAPPIE, *remap, "--remap-variants", str(vars))
    for extra in (["--remap-variants-context", "3"], ["--remap-variants-all-paths"], ["--remap-variants-out", str(out)]):
        assert "go with --remap-variants" in refused(FLAPPIE, *remap, *extra), extra
        assert "go with --remap-variants" in refused(FLAPPIE, *extra), extra
    for bad in ("0", "24", "-1", "x", "3.5", ""):
        assert "--remap-variants-context must be a whole number from 1 to 23" in refused(
            FLAPPIE, *remap, "--remap-variants", str(vars), "--remap-variants-out", str(out), "--remap-variants-context", bad), bad
    assert "--remap-out" in refused(FLAPPIE, "--remap", str(refs), "--remap-variants", str(vars), "--remap-variants-out", str(out))
    for args in (["--remap-variants", str(vars)], ["--remap-variants-out", str(out)], ["--remap-variants-context", "3"], ["--remap-variants-all-paths"]):
        assert "--remap-variants is flappie's" in refused(RUNNIE, *args), args
    assert not out.exists() and not table.exists()


def test_library_exports_the_new_entries():
    lib = C.CDLL(LIBFFHIP)
    for name in ("ffhip_batch_set_remap_variants", "ffhip_batch_variant_calls", "ffhip_op_variants"):
        assert hasattr(lib, name), name
    host = C.CDLL(HOSTLIB)
    for name in ("flappie_variants_parse", "flappie_variants_read", "flappie_variants_free", "flappie_variants_of", "flappie_variants_write"):
        assert hasattr(host, name), name
    text = open(os.path.join(ROOT, "include", "ffhip.h")).read()
    assert re.search(r"#define\s+FFHIP_RUN_REMAP_VARIANTS\s+524288u", text)
    from flappie_amd import binding
    assert binding.RUN_REMAP_VARIANTS == 524288
    assert binding.VARIANT_DTYPE == V.VARIANT_DTYPE and binding.VARIANT_DTYPE.itemsize == 24
    assert binding.VARIANT_CALL_DTYPE == V.VARIANT_CALL_DTYPE and binding.VARIANT_CALL_DTYPE.itemsize == 16
    assert hasattr(binding.Batch, "set_remap_variants") and hasattr(binding.Batch, "variant_calls") and hasattr(binding, "op_variants")
    assert binding.make_variants([(3, 1, [2, 0])]).tobytes() == V.pack([(3, 1, [2, 0])]).tobytes()
