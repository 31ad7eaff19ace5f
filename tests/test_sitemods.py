"""flappie --remap-mods on the CPU: the restatement of include/ffhip.h "site mods" (sitemods_ref.py) against a brute-force enumeration of every monotone path on
tiny windows; the hypothesis coding; the window at its edges; the two invariants that tie the scores to remap; the option and its refusals; the library's new
entries.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import remap_ref as RR
import sitemods_ref as S
from test_cli import FLAPPIE, ROOT, RUNNIE, needs_hdf5

LIBFFHIP = os.path.join(ROOT, "flappie_amd", "libffhip.so")
NB = 5


def _scores(rng, N, scale=3.0):
    return (rng.standard_normal((N, 60)) * scale).astype(np.float32)


def _path(rng, N, L):
    rm = np.zeros(N, np.uint8)
    rm[rng.choice(N, L - 1, replace=False)] = 1
    return rm


def test_restatement_against_every_path_of_tiny_windows():
    rng = np.random.default_rng(11)
    seen = 0
    for trial in range(60):
        N = int(rng.integers(1, 10))
        L = int(rng.integers(1, min(N + 1, 6) + 1))
        codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L)
        rm = _path(rng, N, L)
        # sums of small dyadic fractions are exact in float32 in any order: the best path's score does not depend on the order of the adds
        T = (rng.integers(-64, 65, (N, 60)) / 8.0).astype(np.float32)
        st = S.starts(rm, L)
        for c in (0, 1, 2):
            for i in S.sites(codes):
                lo, hi, t0, t1 = S.window(st, L, i, c)
                if hi - lo + 1 > 4 or t1 - t0 > 7:
                    continue
                for letter in (S.CAN, S.MOD):
                    q = S.code_hypothesis(codes, i, letter, NB)
                    best, logsum = S.brute(T, q, lo, hi, t0, t1, NB)
                    got = S.score_best(T, q, lo, hi, t0, t1, NB)
                    assert got.dtype == np.float32 and got.tobytes() == best.tobytes(), (trial, c, i, letter, got, best)
                    assert abs(float(S.score_all(T, q, lo, hi, t0, t1, NB)) - logsum) <= 1e-9, (trial, c, i, letter)
                    seen += 1
    assert seen >= 200


def test_all_paths_never_gives_a_nan():
    T = np.full((6, 60), -1e30, np.float32)
    T[::2] = -np.inf
    codes, rm = np.array([1, 1, 4, 0], np.uint8), np.array([1, 0, 1, 0, 1, 0], np.uint8)
    with np.errstate(all="ignore"):
        for mode in (False, True):
            out = S.site_mods(T, NB, codes, rm, 3, mode)
            assert out["pos"].tolist() == [0, 1, 2] and not np.any(np.isnan(out["can"])) and not np.any(np.isnan(out["mod"]))


def test_hypothesis_coding_is_remaps_coding_of_the_edited_sequence():
    letters = {"A": 0, "C": 1, "G": 2, "T": 3, "Z": 4}
    assert S.code_hypothesis([1, 1, 1], 1, S.CAN, NB) == [1, 6, 1]          # C c C
    assert S.code_hypothesis([1, 1, 1], 1, S.MOD, NB) == [1, 4, 1]          # C Z C
    for text in ("CCC", "CZC", "ZZ", "CCCC", "ACCZCCA"):
        s = [letters[x] for x in text]
        assert S.sites(s) == [k for k, x in enumerate(text) if x in "CZ"]
        for i in S.sites(s):
            for letter in (S.CAN, S.MOD):
                edited = list(s)
                edited[i] = letter
                q = S.code_hypothesis(s, i, letter, NB)
                assert q == RR.flipflop_code(edited, NB), (text, i, letter)
                assert q[:i] == RR.flipflop_code(s, NB)[:i], (text, i, letter)          # the positions before i code as in s


def test_window_edges():
    # five bases over nine blocks: starts 0, 2, 3, 6, 8
    rm = np.array([0, 1, 1, 0, 0, 1, 0, 1, 0], np.uint8)
    st = S.starts(rm, 5)
    assert st == [0, 2, 3, 6, 8, 9]
    assert S.window(st, 5, 0, 1) == (0, 1, 0, 2)            # i = 0: block 2 is the move out of base 1
    assert S.window(st, 5, 4, 1) == (3, 4, 6, 9)            # i = L - 1: to the read's end
    assert S.window(st, 5, 2, 0) == (2, 2, 3, 5)            # c = 0: P = 1, the stays of base 2
    assert S.window(st, 5, 2, 31) == (0, 4, 0, 9)
    assert S.window(S.starts(np.zeros(4, np.uint8), 1), 1, 0, 15) == (0, 0, 0, 4)       # L = 1
    # L = N + 1: a base a block, the last base has none; n = P - 1 everywhere
    ones = np.ones(3, np.uint8)
    st = S.starts(ones, 4)
    for i in range(4):
        for c in (0, 1, 5):
            lo, hi, t0, t1 = S.window(st, 4, i, c)
            assert t1 - t0 == hi - lo
    rng = np.random.default_rng(2)
    T = _scores(rng, 3)
    out = S.site_mods(T, NB, np.array([1, 4, 1, 1], np.uint8), ones, 0)
    assert out["pos"].tolist() == [0, 1, 2, 3] and out["nblock"].tolist() == [0, 0, 0, 0]
    assert np.all(out["can"] == 0.0) and np.all(out["mod"] == 0.0)                      # P = 1, n = 0: the empty sum
    # a sequence without C or Z
    assert S.site_mods(T, NB, np.array([0, 2, 3], np.uint8), np.array([1, 0, 1], np.uint8), 15).size == 0
    assert S.SITE_MOD_DTYPE.itemsize == 16


def test_invariants_that_tie_the_scores_to_remap():
    rng = np.random.default_rng(5)
    n = 0
    for N in (1, 2, 7, 40, 90):
        for L in sorted({1, N + 1, int(rng.integers(1, N + 2)), int(rng.integers(1, min(N + 1, 30) + 1))}):
            codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L)
            T = _scores(rng, N)
            score, rm = RR.remap(T, codes, NB, L)                   # unbanded
            st = S.starts(rm, L)
            q = RR.flipflop_code(codes, NB)
            for c in (0, 1, 4, 31):
                out = S.site_mods(T, NB, codes, rm, c)
                for rec in out:
                    i = int(rec["pos"])
                    given = rec["can"] if codes[i] == S.CAN else rec["mod"]
                    lo, hi, t0, t1 = S.window(st, L, i, c)
                    assert rec["nblock"] == t1 - t0
                    if c >= L - 1:                                  # the whole read is the window: remap's own recursion
                        assert np.float32(given).tobytes() == np.float32(score).tobytes(), (N, L, c, i)
                    own, end = S.path_sum(T, q, rm, lo, t0, t1, NB)
                    assert end == hi and given >= own, (N, L, c, i, given, own)
                    n += 1
    assert n >= 100


@needs_hdf5
def test_option_and_its_refusals_without_gpu(tmp_path):
    refs = tmp_path / "refs.fa"
    refs.write_text(">r1\nACGT\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--remap-mods=", "--remap-mods-context=", "--remap-mods-all-paths"):
        assert opt in r.stdout, opt
        for line in r.stdout.split("\n"):                       # long options only
            if opt in line:
                assert re.match(r"^ {6}" + re.escape(opt), line), line
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--remap-mods" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out, table = tmp_path / "mods.tsv", tmp_path / "map.tsv"
    assert "--remap-mods goes with --remap" in refused(FLAPPIE, "--remap-mods", str(out))
    assert "--remap-mods" in refused(RUNNIE, "--remap-mods", str(out))
    assert "--remap-out" in refused(FLAPPIE, "--model", "r941_5mC", "--remap", str(refs), "--remap-mods", str(out))
    # a model without a modified base, in the words --modbase-tags uses
    tags = refused(FLAPPIE, "--modbase-tags")
    mods = refused(FLAPPIE, "--remap", str(refs), "--remap-out", str(table), "--remap-mods", str(out))
    assert "needs a model with a modified base" in tags and tags.split("needs a model")[1] == mods.split("needs a model")[1]
    for bad in ("-1", "32", "x", "3.5", ""):
        assert "--remap-mods-context must be a whole number from 0 to 31" in refused(
            FLAPPIE, "--model", "r941_5mC", "--remap", str(refs), "--remap-out", str(table), "--remap-mods", str(out), "--remap-mods-context", bad), bad
    assert "go with --remap-mods" in refused(FLAPPIE, "--remap-mods-context", "3")
    assert "go with --remap-mods" in refused(FLAPPIE, "--remap-mods-all-paths")
    assert not out.exists() and not table.exists()


def test_library_exports_the_new_entries():
    lib = C.CDLL(LIBFFHIP)
    for name in ("ffhip_batch_set_remap_mods", "ffhip_batch_site_mods", "ffhip_op_site_mods"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "ffhip.h")).read()
    assert re.search(r"#define\s+FFHIP_RUN_REMAP_MODS\s+262144u", text)
    from flappie_amd import binding
    assert binding.RUN_REMAP_MODS == 262144 and binding.SITE_MOD_DTYPE == S.SITE_MOD_DTYPE and binding.SITE_MOD_DTYPE.itemsize == 16
    assert hasattr(binding.Batch, "set_remap_mods") and hasattr(binding.Batch, "site_mods") and hasattr(binding, "op_site_mods")


def _windows(rng, N, L, c):
    codes = rng.choice(np.array([0, 1, 1, 4, 4, 2, 3], np.uint8), L)
    st = S.starts(_path(rng, N, L), L)
    for i in S.sites(codes):
        for letter in (S.CAN, S.MOD):
            yield (S.code_hypothesis(codes, i, letter, NB),) + S.window(st, L, i, c)


def _finite_and_neg_inf_scores(rng, N):
    for k in range(4):
        T = _scores(rng, N, 2.0)
        if k == 1:
            T = np.round(T * 4.0).astype(np.float32) / np.float32(4.0)      # ties
        elif k >= 2:
            T[rng.random(T.shape) < (0.02, 0.3)[k - 2]] = -np.inf
        yield T


def test_best_path_strict_compare_is_max_on_finite_and_neg_inf_scores():
    """include/ffhip.h "site mods": the rule is the strict compare of "variants"; on finite and -inf terms it is max(stay, move), the wording before"""
    def score_max(T, q, lo, hi, t0, t1):
        stay_idx, move_idx = S._indices(q, lo, hi, NB)
        X = np.full(hi - lo + 1, -np.inf, np.float32)
        X[0] = 0.0
        for t in range(t0, t1):
            move = np.full(X.size, -np.inf, np.float32)
            move[1:] = X[:-1] + T[t][move_idx[1:]]
            X = np.maximum(X + T[t][stay_idx], move)
        return np.float32(X[-1])
    rng = np.random.default_rng(41)
    n = neg = 0
    for T in _finite_and_neg_inf_scores(rng, 120):
        for c in (0, 3, 15):
            for q, lo, hi, t0, t1 in _windows(rng, 120, 50, c):
                a, b = S.score_best(T, q, lo, hi, t0, t1, NB), score_max(T, q, lo, hi, t0, t1)
                assert not np.isnan(a) and a.tobytes() == b.tobytes(), (c, lo, hi, a, b)
                n += 1
                neg += bool(np.isneginf(a))
    assert n >= 400 and 0 < neg < n, (n, neg)


def test_all_paths_ieee_rule_is_the_masked_rule_on_finite_and_neg_inf_scores():
    """include/ffhip.h "site mods": the all-paths rule as IEEE arithmetic gives, bit for bit, what the statement before gave (m = -inf masked ahead of the
    arithmetic) wherever the scores are finite or -inf -- and never a NaN there"""
    def score_masked(T, q, lo, hi, t0, t1):
        T = T.astype(np.float64)
        stay_idx, move_idx = S._indices(q, lo, hi, NB)
        X = np.full(hi - lo + 1, -np.inf, np.float64)
        X[0] = 0.0
        for t in range(t0, t1):
            stay = X + T[t][stay_idx]
            move = np.full(X.size, -np.inf, np.float64)
            move[1:] = X[:-1] + T[t][move_idx[1:]]
            m = np.maximum(stay, move)
            live = m > -np.inf
            d = np.zeros(X.size, np.float64)
            d[live] = np.abs(stay[live] - move[live])
            X = np.where(live, m + np.log1p(np.exp(-d)), -np.inf)
        return np.float64(X[-1])
    rng = np.random.default_rng(43)
    n = neg = 0
    for T in _finite_and_neg_inf_scores(rng, 120):
        for c in (0, 3, 15):
            for q, lo, hi, t0, t1 in _windows(rng, 120, 50, c):
                a, b = S.score_all(T, q, lo, hi, t0, t1, NB), score_masked(T, q, lo, hi, t0, t1)
                assert not np.isnan(a) and a.tobytes() == b.tobytes(), (c, lo, hi, a, b)
                n += 1
                neg += bool(np.isneginf(a))
    assert n >= 400 and 0 < neg < n, (n, neg)


def test_a_nan_is_seen_in_both_modes_and_the_two_best_path_rules_part_on_it():
    """with a NaN entry on a term the all-paths score is NaN (the statement before dropped it), and the strict compare keeps a NaN stay where max() also takes a
    NaN move: the rules differ, which is why the header names one"""
    rng = np.random.default_rng(47)
    T = _scores(rng, 300, 2.0)
    T[rng.random(T.shape) < 0.02] = np.nan
    nan_all = nan_best = fin_best = 0
    for q, lo, hi, t0, t1 in _windows(rng, 300, 120, 3):
        nan_all += bool(np.isnan(S.score_all(T, q, lo, hi, t0, t1, NB)))
        b = S.score_best(T, q, lo, hi, t0, t1, NB)
        nan_best += bool(np.isnan(b))
        fin_best += bool(np.isfinite(b))
    assert nan_all > 0 and nan_best > 0 and fin_best > 0, (nan_all, nan_best, fin_best)
