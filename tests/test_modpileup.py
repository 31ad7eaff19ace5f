"""flappie --map-mods without a GPU: the restatement (modpileup_ref.py: the header's walk in signal order) held to a brute force that expands the alignment into
columns first and counts afterwards; the host side (flappie_modpileup.c of libflappie_host.so: the bedMethyl table, the histogram's file and the summary) against
the restatement's writer on hand-made counters; header, binding and library agree on the new calls; every refusal the command line makes before it opens a device
(all of them: each `errx` of --map-mods in flappie_cli.c stands ahead of flappie_hip_model, bar the one behind ffhip_modpileup_create, which repeats checks made
here and cannot be reached from the options).  Everything is integer- or byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_ref as R
import modpileup_ref as MP
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5
from test_map import Ref
from test_pileup import random_ops

NEW_CALLS = ("ffhip_modpileup_create", "ffhip_modpileup_free", "ffhip_modpileup_reset", "ffhip_modpileup_positions", "ffhip_modpileup_download",
             "ffhip_batch_set_modpileup", "ffhip_op_modpileup")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


# ------------------------------------------------------------------------------------ the restatement against brute force
def brute_force(refs, q, tstart, tend, call, ml, ops, lo, hi):
    """the alignment as a list of columns (forward position or None, call index or None), then every column looked at by itself:
    {(o, column, k, f): count}, sites, {byte: count}"""
    k, o = q >> 1, q & 1
    strand = refs[k] if not o else "".join(COMP[c] for c in reversed(refs[k]))      # what search q reads
    cols, j, i = [], tstart, 0
    for op in ops:
        cols.append((j if op != 2 else None, i if op != 3 else None))
        j += op != 2
        i += op != 3
    assert j == tend and i == len(call)
    counts, hist, sites = {}, {}, 0
    for y, i in cols:
        if y is None or strand[y] != "C":                      # a site: the strand the read lies on has a C there
            continue
        f = len(refs[k]) - 1 - y if o else y
        assert refs[k][f] == "CG"[o]
        sites += 1
        if i is None:
            col = "del"
        elif call[i] not in "CZ":
            col = "diff"
        else:
            hist[int(ml[i])] = hist.get(int(ml[i]), 0) + 1
            col = "mod" if ml[i] >= hi else ("canon" if ml[i] <= lo else "fail")
        counts[(o, col, k, f)] = counts.get((o, col, k, f), 0) + 1
    return counts, sites, hist


def hand_made(rng, refs, lo, hi):
    lens = [len(r) for r in refs]
    out = [(0, 0, 1, "Z", [hi], [0]), (1, 0, 1, "C", [lo], [1]), (0, 0, 1, "", [], [3]), (1, 0, 1, "GT", [3, 4], [2, 3, 2]), (2, 0, lens[1], "", [], [3] * lens[1])]
    for it in range(300):
        k = int(rng.integers(0, len(lens)))
        a = 0 if it % 4 == 0 else int(rng.integers(0, lens[k]))
        b = lens[k] if it % 4 == 1 else int(rng.integers(a + 1, lens[k] + 1))
        ops, n = random_ops(rng, b - a, weights=(0.6, 0.15, 0.1, 0.15), lead=it % 3 if it % 7 == 1 else 0, trail=it % 2 if it % 7 == 2 else 0)
        call = "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n))
        ml = rng.choice(np.array([0, lo, lo + 1, hi - 1, hi, 255, 128, 7], np.uint8), n)
        out.append((2 * k + int(rng.integers(0, 2)), a, b, call, ml, ops))
    return out


def test_the_signal_order_walk_against_columns_first():
    rng = np.random.default_rng(12)
    refs = ["C", R.random_seq(rng, 15), "C" * 16, "G" * 17, R.random_seq(rng, 33), R.random_seq(rng, 100), "ATTA" * 5]
    lens = [len(r) for r in refs]
    lo, hi = 60, 190
    p = MP.ModPileup(lens, refs, 0, lo, hi)
    want, sites, hist = {}, 0, np.zeros(256, np.uint64)
    seen = {"plus": 0, "minus": 0, "start0": 0, "endM": 0}
    alns = hand_made(rng, refs, lo, hi)
    for q, ts, te, call, ml, ops in alns:
        p.add(q, ts, te, call, ml, ops)
        c, s, h = brute_force(refs, q, ts, te, call, ml, ops, lo, hi)
        for key, v in c.items():
            want[key] = want.get(key, 0) + v
        sites += s
        for v, cnt in h.items():
            hist[v] += np.uint64(cnt)
        seen["minus" if q & 1 else "plus"] += 1
        seen["start0"] += ts == 0
        seen["endM"] += te == lens[q >> 1]
    assert min(seen.values()) >= 10, seen
    dense = np.zeros((10, p.P), np.uint32)
    for (o, col, k, f), v in want.items():
        dense[5 * o + MP.COLUMNS.index(col), p.off[k] + f] = v
    assert np.array_equal(p.counts, dense) and np.array_equal(p.hist, hist)
    t = p.totals
    assert t["reads"] == len(alns) and t["skipped"] == 0 and t["sites"] == sites == int(dense.sum()) and min(t[c] for c in MP.COLUMNS) > 0
    assert all(t[c] == int(dense[[i, 5 + i]].sum()) for i, c in enumerate(MP.COLUMNS)) and int(hist.sum()) == t["mod"] + t["canon"] + t["fail"]
    assert all(hist[v] > 0 for v in (0, lo, lo + 1, hi - 1, hi, 255))
    assert dense[:, p.off[6]:].sum() == 0 and dense[5:, p.off[2]:p.off[3]].sum() == 0 and dense[:5, p.off[3]:p.off[4]].sum() == 0      # no C or G; all C; all G
    # by hand: a read on the - strand of "ACGT" behind a record of 1: span [1, 3) of the reverse complement ACGT is forward [1, 3) walked from its right end, G first
    h = MP.ModPileup([1, 4], ["A", "ACGT"], 0, 50, 205)
    h.add(3, 1, 3, "ZAC", [205, 9, 50], [0, 2, 1])            # Z on the G at forward 2 (a site of the - strand): mod; A inserted; C on the C at forward 1: not a - site
    want = np.zeros((10, 5), np.uint32)
    want[5 + 0, 1 + 2] = 1
    assert np.array_equal(h.counts, want) and h.totals == dict(reads=1, skipped=0, sites=1, mod=1, canon=0, fail=0, diff=0, **{"del": 0}) and h.hist[205] == 1
    # the thresholds' edges, and the identity test at equality (3 matches of 4 columns)
    assert [h.classify(v) for v in (0, 50, 51, 204, 205, 255)] == ["canon", "canon", "fail", "fail", "mod", "mod"]
    for min_id, counted in ((750, 1), (751, 0)):
        x = MP.ModPileup([10], ["CCCCCCCCCC"], min_id, 50, 205)
        x.add(0, 2, 6, "CZA", [0, 255, 0], [0, 0, 3, 0])
        assert (x.totals["reads"], x.totals["skipped"], x.totals["sites"]) == (counted, 1 - counted, 4 * counted)
    x = MP.ModPileup([10], ["CCCCCCCCCC"], 900)
    mp, tr = {"status": 1, "q": 0, "tstart": 0, "tend": 3}, {"status": 1, "n": 3, "m": 3, "ops": np.array([0, 1, 0], np.uint8)}
    for a, b in ((mp, tr), (dict(mp, status=2), tr), (mp, dict(tr, status=2)), (mp, dict(tr, status=0))):
        x.add_read(a, b, "CCC", [1, 2, 3])
    assert x.totals["skipped"] == 1 and x.totals["reads"] == 0 and int(x.counts.sum()) == 0


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    vp = C.c_void_p
    assert lib.ffhip_modpileup_create.argtypes == [vp, vp, C.c_int, C.c_int, C.c_int] and lib.ffhip_modpileup_create.restype == vp
    assert lib.ffhip_modpileup_positions.restype == C.c_size_t
    assert lib.ffhip_op_modpileup.argtypes == [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("ffhip_modpileup *ffhip_modpileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity, int lo, int hi);",
                  "int ffhip_modpileup_download(ffhip_modpileup *p, uint32_t *counts /* [10][P] */, ffhip_modpileup_totals *totals, uint64_t *hist /* [256] */);",
                  "int ffhip_batch_set_modpileup(ffhip_batch *b, ffhip_modpileup *p);",
                  "int ffhip_op_modpileup(ffhip_engine *eng, ffhip_modpileup *p, int q, int tstart, int tend, const char *call, const uint8_t *ml, size_t n, "
                  "const uint8_t *ops, size_t nops);"):
        assert proto in header, proto
    m = re.search(r"#define FFHIP_RUN_MOD_PILEUP\s+\(1u << (\d+)\)", header)
    decimal = [int(v) for v in re.findall(r"#define FFHIP_RUN_[A-Z_0-9]+\s+(\d+)u", header)]
    assert m and (1 << int(m.group(1))) == B.RUN_MOD_PILEUP == 16777216 == 2 * max(decimal) == 2 * B.RUN_PILEUP      # the next free bit
    assert B.MODPILEUP_TOTALS == MP.TOTALS and len(B.MODPILEUP_TOTALS) == 8 and B.MODPILEUP_COLUMNS == MP.COLUMNS
    assert callable(B.ModPileup) and callable(B.Batch.set_modpileup) and callable(B.op_modpileup)
    H = C.CDLL(HOSTLIB)
    assert sorted(_declared_functions("flappie_modpileup.h")) == ["flappie_modpileup_hist_write", "flappie_modpileup_summary_print", "flappie_modpileup_write"]
    assert all(hasattr(H, n) for n in _declared_functions("flappie_modpileup.h"))


# ------------------------------------------------------------------------------------ the host side
class Totals(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in MP.TOTALS]


def test_the_table_the_histogram_and_the_summary_are_the_restatements(tmp_path):
    L = C.CDLL(HOSTLIB)
    L.flappie_map_ref_parse.restype = C.POINTER(Ref)
    L.flappie_map_ref_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_free.argtypes = [C.POINTER(Ref)]
    L.flappie_map_ref_free.restype = None
    L.flappie_modpileup_write.argtypes = [C.c_void_p, C.POINTER(Ref), C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    L.flappie_modpileup_hist_write.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.flappie_modpileup_summary_print.argtypes = [C.c_void_p, C.POINTER(Totals), C.c_ulonglong]
    L.flappie_modpileup_summary_print.restype = None
    # a record that begins with G and ends with C (no neighbour at either end), one in lower case, one of a single C, one CpG at a record's very ends
    records = ["GACGTCGGCATCCGAC", "ttcgacgcgta", "C", "CG"]
    names = ["chr1", "lower.2", "one", "cg"]
    text = ">chr1 first\n%s\n>lower.2\n%s\n>one\nC\n>cg\tx\nCG\n" % (records[0], records[1])
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_parse(text.encode(), err, 256)
    assert ref, err.value
    p = MP.ModPileup([len(r) for r in records], records)
    rng = np.random.default_rng(19)
    for k, rec in enumerate(p.refs):                          # hand-made counters: every site of either strand gets some, every third stays all 0
        for f, c in enumerate(rec):
            for o in (0, 1):
                if c == "CG"[o] and (f + o + k) % 3:
                    p.counts[5 * o:5 * o + 5, p.off[k] + f] = rng.integers(0, 4, 5)
    p.counts[0:2, p.off[0] + 2] = 0                           # Nvalid = 0 with fail > 0: 0.00
    p.counts[2, p.off[0] + 2] = 3
    p.counts[0:5, p.off[0] + 5] = (1, 2, 0, 0, 0)             # 33.33
    p.counts[0, p.off[1] + 2] = (1 << 32) - 1                 # a counter at its largest value is written as it stands
    p.counts[5:10, p.off[1] + 3] = ((1 << 32) - 1, 1, 0, 0, 0)      # ... and the sum of two of them under combine does not wrap
    p.counts[0:5, p.off[0]] = 7                               # not a site (the record begins with G, a - strand site): never written for +
    p.counts[5 + 3, p.off[0]] = 2                             # ... and written for - under the motif C only: no neighbour
    p.counts[1, p.off[0] + 15] = 2                            # the record ends with C: likewise
    p.counts[0, p.off[2]] = 1                                 # the record of a single C
    p.totals.update(reads=11, skipped=2, sites=99, mod=5, canon=4, fail=3, diff=2)
    p.totals["del"] = 1
    p.hist[:] = rng.integers(0, 1 << 40, 256).astype(np.uint64)
    p.hist[255] = np.uint64((1 << 64) - 1)
    libc = C.CDLL(None)
    flat = np.ascontiguousarray(p.counts)
    ptr = flat.ctypes.data_as(C.POINTER(C.c_uint32))
    got = {}
    for motif, combine in (("CG", False), ("C", False), ("CG", True)):
        bed = tmp_path / ("mods_%s_%d.bed" % (motif, combine))
        f = _cfile(libc, bed)
        rows = C.c_ulonglong(0)
        assert L.flappie_modpileup_write(f, ref, ptr, 0 if motif == "CG" else 1, int(combine), C.byref(rows)) == 0
        libc.fclose(f)
        text = bed.read_text()
        assert text == p.bed(names, motif, combine), (motif, combine)
        lines = [ln.split("\t") for ln in text.splitlines()]
        assert rows.value == len(lines) == p.stderr_lines(motif, combine)["rows"] > 0 and all(len(ln) == 18 for ln in lines)
        for ln in lines:
            assert ln[3] == "m" and ln[1] == ln[6] and ln[2] == ln[7] == str(int(ln[1]) + 1) and ln[8] == "255,0,0" and ln[13] == ln[17] == "0"
            assert int(ln[4]) == int(ln[9]) == int(ln[11]) + int(ln[12]) and ln[5] in ("." if combine else "+-")
            assert sum(int(ln[x]) for x in (11, 12, 14, 15, 16)) >= 1             # a row whose counters are all 0 is not written
        got[(motif, combine)] = lines
    cg, c, comb = got[("CG", False)], got[("C", False)], got[("CG", True)]
    key = lambda ln: (ln[0], int(ln[1]), ln[5])
    assert {key(ln) for ln in cg} < {key(ln) for ln in c}
    assert ("chr1", 0, "-") in {key(ln) for ln in c} and ("chr1", 0, "-") not in {key(ln) for ln in cg} and ("chr1", 0, "+") not in {key(ln) for ln in c}      # begins with G
    assert ("chr1", 15, "+") in {key(ln) for ln in c} and ("chr1", 15, "+") not in {key(ln) for ln in cg}                # ends with C
    assert not any(ln[0] == "one" for ln in cg) and any(ln[0] == "one" for ln in c)
    assert [ln for ln in cg if ln[0] == "chr1" and ln[1] == "2"][0][9:17] == ["0", "0.00", "0", "0", "0"] + [str(int(p.counts[4, 2])), "3", str(int(p.counts[3, 2]))]
    assert [ln for ln in cg if ln[0] == "chr1" and ln[1] == "5" and ln[5] == "+"][0][9:13] == ["3", "33.33", "1", "2"]
    assert any(ln[0] == "lower.2" for ln in cg)               # lower case is upper-cased
    low = [ln for ln in comb if ln[0] == "lower.2" and ln[1] == "2"][0]
    assert low[11] == str(2 * ((1 << 32) - 1)) and int(low[12]) == int(p.counts[1, p.off[1] + 2]) + 1
    assert len(comb) <= len([ln for ln in cg if ln[5] == "+"]) + len([ln for ln in cg if ln[5] == "-"]) and all(ln[5] == "." for ln in comb)
    f = _cfile(libc, tmp_path / "bad.bed")
    for bad in ((2, 0), (-1, 0), (1, 1)):                     # a motif that is neither; combine with the motif C
        assert L.flappie_modpileup_write(f, ref, ptr, bad[0], bad[1], None) == -1
    libc.fclose(f)
    assert (tmp_path / "bad.bed").read_text() == ""
    assert L.flappie_modpileup_write(None, ref, ptr, 0, 0, None) == -1
    hist = tmp_path / "hist.tsv"
    f = _cfile(libc, hist)
    assert L.flappie_modpileup_hist_write(f, p.hist.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    libc.fclose(f)
    assert hist.read_text() == p.hist_tsv() and hist.read_text().splitlines()[255] == "255\t18446744073709551615"
    summ = tmp_path / "summary.txt"
    f = _cfile(libc, summ)
    t = Totals(*[p.totals[k] for k in MP.TOTALS])
    L.flappie_modpileup_summary_print(f, C.byref(t), 17)
    libc.fclose(f)
    assert summ.read_text() == "".join("mods_pileup\t%s\t%d\n" % (k, v) for k, v in list(p.totals.items()) + [("rows", 17)])
    assert list(p.totals) == list(MP.TOTALS)
    L.flappie_map_ref_free(ref)


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all("--map-mods" + o in r.stdout for o in ("=", "-hi=", "-lo=", "-min-identity=", "-motif=", "-combine-strands", "-hist=")), r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--map-mods" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    hits, acc, bed, hist = (str(tmp_path / n) for n in ("hits.tsv", "acc.tsv", "mods.bed", "hist.tsv"))
    model = ["--model", "r941_5mC"]
    mapped = model + ["--map", str(fa), "--map-out", hits]
    aligned = mapped + ["--truth-from-map", "--truth-out", acc]
    assert "--map-mods goes with --truth-from-map" in refused(FLAPPIE, *model, "--map-mods", bed)
    assert "--map-mods goes with --truth-from-map" in refused(FLAPPIE, *mapped, "--map-mods", bed)
    assert "--truth-from-map goes with --map" in refused(FLAPPIE, *model, "--truth-from-map", "--truth-out", acc, "--map-mods", bed)
    assert "--truth-from-map and --truth-out go together" in refused(FLAPPIE, *mapped, "--truth-from-map", "--map-mods", bed)
    goes = "--map-mods-hi, --map-mods-lo, --map-mods-min-identity, --map-mods-motif, --map-mods-combine-strands and --map-mods-hist go with --map-mods"
    for sub in (["--map-mods-hi", "200"], ["--map-mods-lo", "20"], ["--map-mods-min-identity", "900"], ["--map-mods-motif", "C"], ["--map-mods-combine-strands"],
                ["--map-mods-hist", hist]):
        assert goes in refused(FLAPPIE, *aligned, *sub), sub
    for opt, top in (("hi", 255), ("lo", 255), ("min-identity", 1000)):
        for bad in ("-1", str(top + 1), "9x", ""):
            assert "--map-mods-%s must be a whole number from 0 to %d" % (opt, top) in refused(FLAPPIE, *aligned, "--map-mods", bed, "--map-mods-" + opt, bad), (opt, bad)
    for lo_hi, text in ((("--map-mods-lo", "205"), "--map-mods-lo (205) must be below --map-mods-hi (205)"), (("--map-mods-hi", "50"), "--map-mods-lo (50) must be below --map-mods-hi (50)"),
                        (("--map-mods-lo", "9", "--map-mods-hi", "8"), "--map-mods-lo (9) must be below --map-mods-hi (8)"), (("--map-mods-hi", "0"), "must be below")):
        assert text in refused(FLAPPIE, *aligned, "--map-mods", bed, *lo_hi), lo_hi
    for bad in ("GC", "cg", "CpG", ""):
        assert "--map-mods-motif is CG or C" in refused(FLAPPIE, *aligned, "--map-mods", bed, "--map-mods-motif", bad)
    assert "--map-mods-combine-strands goes with the motif CG" in refused(FLAPPIE, *aligned, "--map-mods", bed, "--map-mods-motif", "C", "--map-mods-combine-strands")
    # a model without a modified base: the wording of --modbase-tags
    native = ["--map", str(fa), "--map-out", hits, "--truth-from-map", "--truth-out", acc]
    tags = refused(FLAPPIE, "--modbase-tags")
    mods = refused(FLAPPIE, *native, "--map-mods", bed)
    assert "needs a model with a modified base (r941_5mC); \"r941_native\" has none" in mods and mods.split("--map-mods", 1)[1] == tags.split("--modbase-tags", 1)[1]
    assert "cannot be written" in refused(FLAPPIE, *aligned, "--map-mods", str(tmp_path / "no" / "mods.bed"))
    assert "cannot be written" in refused(FLAPPIE, *aligned, "--map-mods", bed, "--map-mods-hist", str(tmp_path / "no" / "hist.tsv"))
    os.remove(bed)                                            # (opened ahead of the histogram's file, which could not be)
    assert "--map-mods goes with --truth-from-map" in refused(FLAPPIE, *mapped, "--map-mods", bed, "--map-mods-hist", hist)
    assert not os.path.exists(bed) and not os.path.exists(hist)      # refused at option parsing: no file, no GPU
    for args in (["--map-mods", bed], ["--map-mods-hi", "200"], ["--map-mods-lo", "20"], ["--map-mods-min-identity", "900"], ["--map-mods-motif", "CG"],
                 ["--map-mods-combine-strands"], ["--map-mods-hist", hist]):
        assert "--map-mods and its --map-mods-* options are flappie's" in refused(RUNNIE, *args), args
