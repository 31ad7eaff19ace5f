"""flappie --truth-errors without a GPU: the restatement (errprofile_ref.py: the header's statement an op at a time, as the kernel has it) held to an independent
statement by truth position -- columns and gaps, 5-mers as slices, runs by a regular expression -- on a few hundred random alignments made to hit the limits (runs
of 16 and 17, 64 and 65 ops, 32 and 33 called letters); cases written down by hand; the host side (flappie_errprofile.c of libflappie_host.so: the table and the
summary) against the restatement on a hand-filled object; header, binding and library agree on the new calls and on the sections; every refusal the command line
makes before it opens a device.  Everything is integer- or byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import errprofile_ref as ER
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5

NEW_CALLS = ("ffhip_errprofile_create", "ffhip_errprofile_free", "ffhip_errprofile_reset", "ffhip_errprofile_words", "ffhip_errprofile_download",
             "ffhip_batch_set_errprofile", "ffhip_op_errprofile", "ffhip_op_errprofile_mapped", "ffhip_debug_errprofile_groups", "ffhip_debug_batch_clear_stretches")


def alignment_of(rng, truth, ins_rate=0.15, long_ins=0.02, err=0.2, edges=True):
    """(call, qual, truth, ops) of a random alignment to `truth` (codes 0 .. 3): a match's letter is the truth's (a C at random Z), a mismatch's another, an inserted
    letter the truth's neighbour's half the time; quality bytes over all of 0 .. 255"""
    ops, call = [], []
    given, truth = truth, ER.fold(truth)

    def insert(j):
        near = truth[min(j, len(truth) - 1)]
        call.append(int(near) if rng.random() < 0.5 else int(rng.integers(0, 4)))
        ops.append(2)
    if edges and rng.random() < 0.3:
        for _ in range(int(rng.integers(1, 4))):
            insert(0)
    for j, t in enumerate(truth):
        u = rng.random()
        if u < err / 2:
            ops.append(3)
        elif u < err:
            ops.append(1)
            call.append((int(t) + int(rng.integers(1, 4))) % 4)
        else:
            ops.append(0)
            call.append(int(t))
        if j + 1 < len(truth) or (edges and rng.random() < 0.3):
            if rng.random() < long_ins:
                for _ in range(int(rng.integers(20, 70))):
                    insert(j + 1)
            elif rng.random() < ins_rate:
                for _ in range(int(rng.integers(1, 4))):
                    insert(j + 1)
    s = "".join("Z" if c == 1 and rng.random() < 0.3 else "ACGT"[c] for c in call)
    qual = bytes(int(x) for x in rng.integers(0, 256, len(s)))
    return s, qual, np.array(given, np.uint8), np.array(ops, np.uint8)


def random_truth(rng, m):
    """m codes in runs: mostly short, some of 9 .. 20"""
    t = []
    while len(t) < m:
        r = int(rng.integers(9, 21)) if rng.random() < 0.06 else int(rng.choice((1, 1, 1, 2, 2, 3, 4, 5)))
        b = int(rng.integers(0, 4))
        if t and t[-1] == b:
            b = (b + 1) % 4
        t += [b] * r
    return t[:m]


def random_alignments(rng, count, max_m=260):
    out = []
    for it in range(count):
        m = int(rng.integers(1, 8)) if it % 7 == 0 else int(rng.integers(1, max_m))
        truth = random_truth(rng, m)
        if it % 5 == 0:
            truth = [4 if c == 1 and rng.random() < 0.5 else c for c in truth]      # Z in the truth
        out.append(alignment_of(rng, truth, err=(0.2, 0.5, 0.05)[it % 3]))
    return out


def run_case(r, ops_in_run, before=2, behind=2, letter=1, ins_letter=None, first_op=0):
    """a truth of `before` other letters, a run of r of `letter`, `behind` others, aligned with all matches but the run's first op (first_op) and with inserted
    letters so that the run's ops number ops_in_run: half ahead of its first op, the rest behind its last"""
    other = (letter + 1) % 4
    truth = [other] * before + [letter] * r + [other] * behind
    extra = ops_in_run - r
    f, b = extra // 2, extra - extra // 2
    il = letter if ins_letter is None else ins_letter
    ops = [0] * before + [2] * f + [first_op] + [0] * (r - 1) + [2] * b + [0] * behind
    call = [other] * before + [il] * f + ([] if first_op == 3 else [letter]) + [letter] * (r - 1) + [il] * b + [other] * behind
    s = "".join("ACGT"[c] for c in call)
    return s, bytes([40 + 33] * len(s)), np.array(truth, np.uint8), np.array(ops, np.uint8)


def hand_cases():
    """the limits, each once: (name, alignment)"""
    out = [("r16", run_case(16, 16)), ("r17", run_case(17, 17)), ("r17_last_but_one", run_case(17, 17, behind=1)), ("r18_to_the_end", run_case(18, 18, behind=0)),
           ("ops64", run_case(10, 64)), ("ops65", run_case(10, 65)), ("c32", run_case(16, 32)), ("c33", run_case(16, 33)), ("c_other_letter", run_case(5, 12, ins_letter=3)),
           ("run_at_the_start", run_case(4, 6, before=0)), ("run_at_the_end", run_case(4, 6, behind=0)), ("first_base_deleted", run_case(6, 9, first_op=3)),
           ("first_base_mismatch", run_case(6, 9, first_op=1))]
    for m in range(1, 6):                                        # the boundary of ctx
        out.append(("m%d" % m, ("ACGTA"[:m], bytes(range(30, 30 + m)), np.array([0, 1, 2, 3, 0][:m], np.uint8), np.zeros(m, np.uint8))))
    for j in (2, 3, 4):                                          # an insertion at j of a truth of 5: only j = 3 has a whole 5-mer round its centre j - 1
        ops = [0] * 5
        ops.insert(j, 2)
        out.append(("m5_ins%d" % j, ("ACGTA"[:j] + "T" + "ACGTA"[j:], b"!!!~~\x7f", np.array([0, 1, 2, 3, 0], np.uint8), np.array(ops, np.uint8))))
    out.append(("m6_ins", ("ACGTTAC", b"\x00 !~\x7f\xff5", np.array([0, 1, 2, 3, 0, 1], np.uint8), np.array([0, 0, 0, 2, 0, 0, 0], np.uint8))))
    out.append(("all_deleted", ("", b"", np.array([0, 0, 1, 4, 2, 2, 2, 3], np.uint8), np.full(8, 3, np.uint8))))
    out.append(("z", ("AZZGT", b"55555", np.array([0, 4, 4, 2, 3], np.uint8), np.zeros(5, np.uint8))))
    return out


# ------------------------------------------------------------------------------------ the two statements
def test_the_walk_by_ops_is_the_walk_by_truth_positions():
    rng = np.random.default_rng(1811)
    alns = random_alignments(rng, 400) + [a for _, a in hand_cases()]
    for mi in (0, 700):
        a, b = ER.ErrProfile(mi), ER.ErrProfile(mi)
        for aln in alns:
            a.add(*aln)
            b.brute(*aln)
            assert a.totals == b.totals and np.array_equal(a.counts, b.counts)
        t = a.totals
        if mi == 0:                                              # every limit is met
            assert t["reads"] > 100 and t["hp_long"] > 3 and t["hp_wide"] > 3 and t["edge_ins"] > 50 and t["ctx_sites"] > 10000 and t["hp_runs"] > 5000
        assert t["reads"] > 20 and (t["skipped"] > 100) == (mi > 0) and t["reads"] + t["skipped"] == len(alns)
        sec = a.sec
        assert int(sec["sub"].sum()) == t["match"] + t["mismatch"] + t["del"] and int(sec["ins"].sum()) == t["ins"] and int(sec["ctx"].sum()) == t["ctx_sites"]
        assert int(sec["qual"].sum()) == t["match"] + t["mismatch"] + t["ins"] and int(sec["hp"].sum()) == t["hp_runs"]
        assert sec["qual"][0].sum() > 0 and sec["qual"][93].sum() > 0 and sec["ctx"][:, 3].sum() > 0 and (mi > 0 or sec["hp"][:, :, 32].sum() > 0)


def test_the_limits_by_hand():
    def one(name):
        p = ER.ErrProfile()
        p.add(*dict(hand_cases())[name])
        return p
    hp = lambda p: [tuple(int(v) for v in x) for x in np.argwhere(p.sec["hp"])]
    assert hp(one("r16")) == [(1, 15, 16)] and one("r16").totals["hp_long"] == 0
    p = one("r17")
    assert hp(p) == [] and (p.totals["hp_long"], p.totals["hp_runs"]) == (1, 0)
    assert one("r17_last_but_one").totals["hp_long"] == 1
    p = one("r18_to_the_end")                                    # its first 17 letters stand inside the truth: long, although it goes on to the end
    assert (p.totals["hp_long"], p.totals["hp_runs"]) == (1, 0)
    p = ER.ErrProfile()
    p.add(*run_case(17, 17, behind=0))                           # the 17th letter is the last: it touches the end
    assert (p.totals["hp_long"], p.totals["hp_runs"]) == (0, 0)
    assert hp(one("ops64")) == [(1, 9, 32)] and one("ops64").totals["hp_wide"] == 0      # 10 matches and 54 inserted letters of the run's: 64 >= 32
    p = one("ops65")
    assert hp(p) == [] and (p.totals["hp_wide"], p.totals["hp_runs"]) == (1, 0)
    assert hp(one("c32")) == [(1, 15, 32)] and hp(one("c33")) == [(1, 15, 32)]
    assert hp(one("c_other_letter")) == [(1, 4, 5)]              # inserted T's beside a run of C: not the run's letter
    assert hp(one("run_at_the_start")) == [] and hp(one("run_at_the_end")) == []
    assert hp(one("first_base_deleted")) == [(1, 5, 5 + 3)] and hp(one("first_base_mismatch")) == [(1, 5, 5 + 3)]
    # ctx: nothing below m = 5; m = 5: the one centre
    for m in range(1, 5):
        assert one("m%d" % m).totals["ctx_sites"] == 0
    p = one("m5")
    assert p.totals["ctx_sites"] == 1 and int(p.sec["ctx"][int("01230", 4), 0]) == 1
    for j in (2, 3, 4):                                          # interior all three, but 3 <= j <= m - 2 is j = 3 alone
        p = one("m5_ins%d" % j)
        assert (p.totals["ctx_sites"], p.totals["ins"], p.totals["edge_ins"]) == (1 + (j == 3), 1, 0) and int(p.sec["ctx"][int("01230", 4), 3]) == (j == 3)
    p = one("m6_ins")
    assert p.totals["ctx_sites"] == 3 and int(p.sec["ctx"][int("01230", 4), 3]) == 1
    # qualities: bytes below '!' are 0, above '~' 93, taken as unsigned
    q = p.sec["qual"]
    assert int(q[0, 0]) == 3 and int(q[93, 0]) == 2 and int(q[93, 2]) == 1 and int(q[93].sum()) == 3 and int(q[ord("5") - 33, 0]) == 1
    p = one("all_deleted")
    assert p.totals["del"] == 8 and int(p.sec["sub"][:, 4].sum()) == 8 and int(p.sec["sub"][1, 4]) == 2 and int(p.sec["hp"][1, 1, 0]) == 1 and p.totals["hp_runs"] == 2
    p = one("z")
    assert int(p.sec["sub"][1, 1]) == 2 and int(p.sec["hp"][1, 1, 2]) == 1
    # below the identity: skipped, nothing else
    p = ER.ErrProfile(900)
    p.add("AAAA", b"!!!!", [0, 1, 0, 0], [0, 1, 0, 0])
    assert p.totals == dict({k: 0 for k in ER.TOTALS}, skipped=1) and not p.counts.any()


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    vp = C.c_void_p
    assert lib.ffhip_errprofile_create.argtypes == [vp, C.c_int] and lib.ffhip_errprofile_create.restype == vp
    assert lib.ffhip_errprofile_download.argtypes == [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    assert lib.ffhip_errprofile_words.restype == C.c_size_t and lib.ffhip_errprofile_words() == B.ERRPROFILE_WORDS == ER.WORDS == 6526      # (no device is touched)
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("ffhip_errprofile *ffhip_errprofile_create(ffhip_engine *eng, int min_identity);",
                  "void ffhip_errprofile_free(ffhip_errprofile *p);",
                  "int ffhip_errprofile_reset(ffhip_errprofile *p);",
                  "size_t ffhip_errprofile_words(void);",
                  "int ffhip_errprofile_download(ffhip_errprofile *p, uint64_t *counts /* [6514] */, ffhip_errprofile_totals *totals);",
                  "int ffhip_batch_set_errprofile(ffhip_batch *b, ffhip_errprofile *p);",
                  "int ffhip_op_errprofile(ffhip_engine *eng, ffhip_errprofile *p, const char *call, const char *qual, size_t n, const uint8_t *truth, size_t m, const uint8_t *ops, size_t nops);",
                  "typedef struct { uint64_t reads, skipped, match, mismatch, del, ins, edge_ins, ctx_sites, hp_runs, hp_long, hp_wide, reserved; } ffhip_errprofile_totals;"):
        assert proto in header, proto
    m = re.search(r"#define FFHIP_RUN_ERRPROFILE\s+\(UINT32_C\(1\) << (\d+)\)", header)
    assert m and int(m.group(1)) == 26 and (1 << 26) == B.RUN_ERRPROFILE == 2 * B.RUN_CONSENSUS      # the next free bit
    # the sections: the header's, the binding's and the restatement's, one behind the other
    assert B.ERRPROFILE_SECTIONS == ER.SECTIONS and B.ERRPROFILE_TOTALS == ER.TOTALS and len(ER.TOTALS) == 12
    at = 0
    for name, first, shape in ER.SECTIONS:
        assert first == at and re.search(r"#define FFHIP_ERRPROFILE_%s %d\n" % (name.upper(), first), header), name
        at += int(np.prod(shape))
    assert at == ER.TABLE_WORDS == B.ERRPROFILE_TABLE_WORDS and "#define FFHIP_ERRPROFILE_TABLE_WORDS %d\n" % at in header
    assert "#define FFHIP_ERRPROFILE_WORDS %d\n" % (at + 12) in header and 4 * at == 4 * (24 + 282 + 4096 + 2112)
    assert (B.ERRPROFILE_HP_MAX_RUN, B.ERRPROFILE_HP_MAX_CALLED, B.ERRPROFILE_HP_MAX_OPS) == (ER.HP_MAX_RUN, ER.HP_MAX_CALLED, ER.HP_MAX_OPS) == (16, 32, 64)
    for k, v in (("RUN", 16), ("CALLED", 32), ("OPS", 64)):
        assert "#define FFHIP_ERRPROFILE_HP_MAX_%s %d\n" % (k, v) in header
    assert [s[2] for s in ER.SECTIONS] == [(4, 5), (4,), (94, 3), (1024, 4), (4, ER.HP_MAX_RUN, ER.HP_MAX_CALLED + 1)]
    assert callable(B.ErrProfile) and callable(B.Batch.set_errprofile) and callable(B.op_errprofile) and callable(B.op_errprofile_mapped)
    assert all(callable(getattr(B.ErrProfile, n)) for n in ("download", "sections", "reset", "close"))
    H = C.CDLL(HOSTLIB)
    assert sorted(_declared_functions("flappie_errprofile.h")) == ["flappie_errprofile_summary_print", "flappie_errprofile_write"]
    assert all(hasattr(H, n) for n in _declared_functions("flappie_errprofile.h"))


# ------------------------------------------------------------------------------------ the host side
class Totals(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ER.TOTALS]


def test_the_writer_is_the_restatement(tmp_path):
    L = C.CDLL(HOSTLIB)
    L.flappie_errprofile_write.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.flappie_errprofile_summary_print.argtypes = [C.c_void_p, C.POINTER(Totals)]
    L.flappie_errprofile_summary_print.restype = None
    rng = np.random.default_rng(5)
    p = ER.ErrProfile()
    for aln in random_alignments(rng, 40):
        p.add(*aln)
    top = (1 << 64) - 1
    p.sec["sub"][2, 4] = top                                     # a counter at its largest value is written as it stands
    p.sec["ctx"][1023, 3] = top
    p.sec["ctx"][0] = (0, 0, 7, 0)
    p.sec["hp"][3, 15, 32] = top
    p.sec["hp"][0, 0, 0] = 5
    p.sec["qual"][93] = (1, top, 3)
    p.totals["hp_wide"] = top
    libc = C.CDLL(None)
    tsv, summ = tmp_path / "errors.tsv", tmp_path / "summary.txt"
    f = _cfile(libc, tsv)
    assert L.flappie_errprofile_write(f, p.counts.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    libc.fclose(f)
    assert L.flappie_errprofile_write(None, p.counts.ctypes.data_as(C.POINTER(C.c_uint64))) == -1 and L.flappie_errprofile_write(f, None) == -1
    got = tsv.read_text()
    assert got == "".join(ln + "\n" for ln in p.tsv_lines())
    lines = got.splitlines()
    assert [ln.split("\t")[0] for ln in lines[:118]] == ["sub"] * 20 + ["ins"] * 4 + ["qual"] * 94
    assert lines[14] == "sub\tG\t-\t18446744073709551615" and lines[20].startswith("ins\tA\t") and lines[24 + 93] == "qual\t93\t1\t18446744073709551615\t3"
    assert lines[118] == "ctx\tAAAAA\t0\t0\t7\t0" and "ctx\tTTTTT\t%d\t%d\t%d\t18446744073709551615" % tuple(int(v) for v in p.sec["ctx"][1023, :3]) in lines
    assert lines[-1] == "hp\tT\t16\t32\t18446744073709551615" and "hp\tA\t1\t0\t5" in lines
    assert re.fullmatch(r"[a-z]+(\t[ACGT-]+)?(\t\d+)+", lines[200]) and all("." not in ln and "e" not in ln.split("\t", 2)[2] for ln in lines)
    assert np.array_equal(ER.from_tsv(lines), p.counts)
    f = _cfile(libc, summ)
    t = Totals(*[p.totals[k] for k in ER.TOTALS])
    L.flappie_errprofile_summary_print(f, C.byref(t))
    libc.fclose(f)
    got = summ.read_text()
    assert got == "".join(ln + "\n" for ln in p.stderr_lines())
    assert got.splitlines()[0] == "errors\treads\t%d" % p.totals["reads"] and "errors\thp_wide\t18446744073709551615\n" in got and len(got.splitlines()) == 12


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--truth-errors=", "--truth-errors-min-identity="):
        assert opt in r.stdout, opt
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--truth-errors" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    hits, acc, errs = str(tmp_path / "hits.tsv"), str(tmp_path / "acc.tsv"), str(tmp_path / "errors.tsv")
    mapped = ["--map", str(fa), "--map-out", hits]
    aligned = mapped + ["--truth-from-map", "--truth-out", acc]
    truthed = ["--truth", str(fa), "--truth-out", acc]
    goes = "--truth-errors goes with --truth or --truth-from-map"
    assert goes in refused(FLAPPIE, "--truth-errors", errs)
    assert goes in refused(FLAPPIE, *mapped, "--truth-errors", errs)
    assert "--truth and --truth-out go together" in refused(FLAPPIE, "--truth", str(fa), "--truth-errors", errs)
    for mode in (aligned, truthed):
        assert "--truth-errors-min-identity goes with --truth-errors" in refused(FLAPPIE, *mode, "--truth-errors-min-identity", "900")
        for bad in ("-1", "1001", "90x", ""):
            assert "--truth-errors-min-identity must be a whole number from 0 to 1000" in refused(FLAPPIE, *mode, "--truth-errors", errs, "--truth-errors-min-identity", bad)
        assert "--truth-errors %s: cannot be written" % str(tmp_path / "no" / "errors.tsv") in refused(FLAPPIE, *mode, "--truth-errors", str(tmp_path / "no" / "errors.tsv"))
    for args in (["--truth-errors", errs], ["--truth-errors-min-identity", "900"]):
        assert "--truth-errors and --truth-errors-min-identity are flappie's" in refused(RUNNIE, *args)
    # both modes pass every check ahead of the device: with the files listed only, nothing is opened on a GPU and the table's file is there
    env = dict(os.environ, FLAPPIE_DEBUG="list_only")
    for mode in (aligned, truthed):
        r = subprocess.run([FLAPPIE, *mode, "--truth-errors", errs, "--truth-errors-min-identity", "900", str(tmp_path)], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 0, r.stderr
        assert os.path.exists(errs)
        os.remove(errs)
