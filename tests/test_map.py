"""flappie --map without a GPU: the numpy restatement (map_ref.py) against a plain triple-loop DP on tiny cases, with ties of strand, record and column and the
start rule; the locality claim the segmented kernel rests on; the host side (the reference's parser, the turn to forward coordinates, the writers of hits.tsv and of
--map-records, the summary of libflappie_host.so) against the restatement on hand-made records; the CLI's refusals.  Everything is integer- or byte-exact.

The locality claim of include/ffhip.h "map": a search started fresh at column a has the exact d at every column j >= a + 2 L.  That holds, and with a column to
spare: an alignment that ends at j and starts before a spans more than j - a columns, and one of s columns costs at least s - L; at j = a + 2 L - 1 that is a cost of
at least L, which the empty match (start = j) has too.  So a + 2 L - 1 cannot differ -- every pattern and text of the exhaustive sweep below agrees.  Columns
before it can: the sweep counts them, and for L = 1 column a + 2 L - 2 = a itself does (D[1][a] = 1 whatever the letter before a)."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import map_ref as R
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5


def brute_row(p, y, anchored=False, fresh=0):
    """D[L][j], j = fresh .. len(y), by the recurrence as written; fresh = a: D[i][a] = i"""
    L, m = len(p), len(y)
    D = [[0] * (m + 1) for _ in range(L + 1)]
    for i in range(L + 1):
        D[i][fresh] = i
    for j in range(fresh, m + 1):
        D[0][j] = j - fresh if anchored else 0
    for i in range(1, L + 1):
        for j in range(fresh + 1, m + 1):
            D[i][j] = min(D[i - 1][j - 1] + (p[i - 1] != y[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D[L][fresh:]


def brute_edit(p, t):
    """the global edit distance"""
    return brute_row(p, t, anchored=True)[-1]


def brute_record(records, call, window, e):
    x = call.replace("Z", "C")
    n = len(x)
    if n == 0:
        return [0] * 16
    L, na = min(n, window), 1 if n <= window else 2
    ys = R.searches(records)
    an = []
    for p in ([x[:L], x[n - L:]] if na == 2 else [x[:L]]):
        rows = [brute_row(p, y) for y in ys]
        d, q, j = min((v, q, j) for q, r in enumerate(rows) for j, v in enumerate(r))
        second = min(min(r) for k, r in enumerate(rows) if k != q)
        start = max(i for i in range(j + 1) if brute_edit(p, ys[q][i:j]) == d)      # the largest i with ed(p, y[i:j]) = d
        an.append([q, start, j, d, second])
    if na == 1:
        an.append(list(an[0]))
    md = L * e // 1000
    status = 1
    if an[0][3] > md or an[1][3] > md:
        status = 2
    elif na == 2 and (an[0][0] != an[1][0] or an[0][1] >= an[1][2] or abs(an[1][2] - an[0][1] - n) > n * e // 1000):
        status = 3
    head = [status, n, na] + ([an[0][0], an[0][1], an[1][2]] if status == 1 else [0, 0, 0])
    return head + an[0] + an[1]


def test_restatement_against_the_plain_recurrence():
    rng = np.random.default_rng(1)
    for _ in range(150):
        p = R.random_seq(rng, int(rng.integers(1, 9)))
        ys = [R.random_seq(rng, int(rng.integers(1, 14))) for _ in range(int(rng.integers(1, 5)))]
        for anchored in (False, True):
            for g, y in zip(R.sweep(p, ys, anchored), ys):
                assert g.tolist() == brute_row(p, y, anchored), (p, y, anchored)
    seen = {"status": set(), "two": 0, "strand tie": 0, "record tie": 0, "column tie": 0, "start": 0}
    for it in range(250):
        alphabet = "AC" if it % 2 else "ACGT"                # (two letters: ties everywhere)
        records = [R.random_seq(rng, int(rng.integers(1, 16))).translate(str.maketrans("GT", alphabet[:2] if it % 2 else "GT")) for _ in range(int(rng.integers(1, 4)))]
        n = int(rng.integers(0, 13))
        call = R.random_seq(rng, n).translate(str.maketrans("GT", "ZA" if it % 2 else "GT"))
        if it % 3 == 0 and n:                                 # cut from the reference, so that some map
            y = R.searches(records)[int(rng.integers(0, 2 * len(records)))]
            call = (y + y)[:n]
        W, e = int(rng.choice([4, 6, 64])), int(rng.choice([0, 250, 500]))
        got, want = R.record(records, call, W, e), brute_record(records, call, W, e)
        assert R.raw(got).tolist() == want, (records, call, W, e)
        seen["status"].add(got["status"])
        seen["two"] += got["nanchor"] == 2
        if n:
            a = got["anchors"][0]
            rows = R.score_rows(records, call[:min(n, W)])
            seen["strand tie"] += int(rows[a["q"] ^ 1].min()) == a["dist"]
            seen["record tie"] += sum(int(r.min()) == a["dist"] for r in rows) > 2
            seen["column tie"] += int((rows[a["q"]] == a["dist"]).sum()) > 1
            seen["start"] += a["end"] - a["start"] != min(n, W)
    assert seen["status"] == {0, 1, 2, 3} and min(v for k, v in seen.items() if k != "status") >= 10, seen
    # the tie rule spelled out: the smallest q, then the leftmost end; the start is the LARGEST one of that distance
    assert R.place(["ACGT", "ACGT"], "CG") == {"q": 0, "start": 1, "end": 3, "dist": 0, "second": 0}
    assert R.place(["TTCGTT", "AACGAA"], "CG") == {"q": 0, "start": 2, "end": 4, "dist": 0, "second": 0}      # (CG is its own reverse complement: strand +)
    assert R.place(["GGCGAACGGG"], "CGA")["end"] == 5 and R.place(["CCCG"], "CG")["q"] == 0
    assert R.place(["CCCCAAAC"], "AAAA") == {"q": 0, "start": 4, "end": 7, "dist": 1, "second": 4}              # (AAA: start 4, not 3 with the C before it)
    assert R.place(["GGGGG"], "C") == {"q": 1, "start": 0, "end": 1, "dist": 0, "second": 1}


def test_locality_of_a_fresh_start():
    """every pattern of 1 .. 3 letters and every text of up to 7 over two letters, every fresh start"""
    differs = {1: 0, 2: 0, 3: 0}
    for L in (1, 2, 3):
        for p in map("".join, itertools.product("AC", repeat=L)):
            for m in range(1, 8):
                for y in map("".join, itertools.product("AC", repeat=m)):
                    exact = brute_row(p, y)
                    for a in range(m + 1):
                        fresh = brute_row(p, y, fresh=a)
                        for j in range(a, m + 1):
                            if j >= a + 2 * L - 1:
                                assert fresh[j - a] == exact[j], (p, y, a, j)       # (the header claims j >= a + 2 L)
                            else:
                                assert fresh[j - a] >= exact[j]
                                differs[L] += fresh[j - a] != exact[j]
    assert min(differs.values()) > 0, differs                 # ... and before that column it does differ
    # the restatement's fresh rows say the same on a longer case
    rng = np.random.default_rng(2)
    y = R.random_seq(rng, 400)
    p = R.edit(rng, y[150:190], 0.1)
    exact = R.sweep(p, [y])[0]
    for a in (0, 100, 151, 170, 399):
        fresh = R.fresh_row(p, y, a)
        assert np.array_equal(fresh[2 * len(p):], exact[a + 2 * len(p):]) and (fresh >= exact[a:]).all()
    assert not np.array_equal(R.fresh_row(p, y, 160)[:2 * len(p)], exact[160:160 + 2 * len(p)])
    # L = 1: the letter before a is out of a fresh search's sight at column a = a + 2 L - 2, and at no later one
    assert brute_row("A", "CAC")[2:] == [0, 1] and brute_row("A", "CAC", fresh=2) == [1, 1]


# ------------------------------------------------------------------------------------ the host side
class Ref(C.Structure):
    _fields_ = [("n", C.c_int), ("name", C.POINTER(C.c_char_p)), ("seq", C.POINTER(C.c_char_p)), ("len", C.POINTER(C.c_size_t))]


class Call(C.Structure):
    _fields_ = [("v", C.c_int32 * 16)]


class Summary(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("reads", "mapped", "unmapped", "discordant", "dist", "bases")]


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_map_ref_parse.restype = C.POINTER(Ref)
    L.flappie_map_ref_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_read.restype = C.POINTER(Ref)
    L.flappie_map_ref_read.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_free.argtypes = [C.POINTER(Ref)]
    L.flappie_map_ref_free.restype = None
    L.flappie_map_forward.argtypes = [C.POINTER(Ref), C.c_int, C.c_long, C.c_long, C.POINTER(C.c_int), C.c_char_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.flappie_map_write_line.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Call), C.POINTER(Ref)]
    L.flappie_map_write_record.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Call), C.POINTER(Ref)]
    L.flappie_map_summary_add.argtypes = [C.POINTER(Summary), C.POINTER(Call), C.c_int]
    L.flappie_map_summary_add.restype = None
    L.flappie_map_summary_print.argtypes = [C.c_void_p, C.POINTER(Summary)]
    L.flappie_map_summary_print.restype = None
    return L


def parse(L, text):
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_parse(text.encode() if text is not None else None, err, 256)
    return ref, err.value.decode()


REF_TEXT = ">lambda the control\nacgtAC\nGT\n\n>plasmid.2\tcircular\n  TTGA  \nCCa\r\n>x\nG\n"
REF_WANT = [("lambda", "ACGTACGT"), ("plasmid.2", "TTGACCA"), ("x", "G")]


def test_the_parser(L, tmp_path):
    ref, why = parse(L, REF_TEXT)
    assert ref and why == ""
    got = [(ref.contents.name[k].decode(), ref.contents.seq[k].decode(), ref.contents.len[k]) for k in range(ref.contents.n)]
    assert got == [(n, s, len(s)) for n, s in REF_WANT]
    L.flappie_map_ref_free(ref)
    for text, words in ((None, ["no reference"]), ("", ["empty"]), ("\n\n", ["empty"]), ("ACGT\n", ["in front of the first record"]), (">\nACGT\n", ["record 1", "no name"]),
                        (">a\n>b\nAC\n", ["record 1", "(a)", "no sequence"]), (">a\nAC\n>b\n", ["record 2", "(b)", "no sequence"]), (">a\nAC\n>b\nG\n>a\nT\n", ["record 3", "a", "twice"]),
                        (">a\nACGT\nACNT\n", ["record 1", "(a)", "position 6", "ACGT"]), (">a\nAC\n>b\nAR\n", ["record 2", "(b)", "position 1"]), (">a\nAC-GT\n", ["position 2"]),
                        (">a\nACGU\n", ["position 3"]), ("".join(">r%d\nA\n" % k for k in range(1025)), ["more than 1024 records"]),
                        (">a\n" + "ACGT" * (1 << 17) + "\n>b\n" + "G" * (1 << 19) + "\nT\n", ["record 2", "(b)", "position 524288", "1048576"])):
        ref, why = parse(L, text)
        assert not ref and all(w in why for w in words), (text[:40] if text else text, why)
    ref, why = parse(L, "".join(">r%d\nA\n" % k for k in range(1024)))
    assert ref and ref.contents.n == 1024
    L.flappie_map_ref_free(ref)
    ref, why = parse(L, ">a\n" + "\n".join(["acgt" * 64] * 2048) + "\n>b\n" + "G" * (1 << 19) + "\n")      # 2^20 in all
    assert ref and ref.contents.len[0] + ref.contents.len[1] == 1 << 20, why
    L.flappie_map_ref_free(ref)
    path = tmp_path / "ref.fa"
    path.write_text(REF_TEXT)
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_read(str(path).encode(), err, 256)
    assert ref and ref.contents.n == 3
    L.flappie_map_ref_free(ref)
    assert not L.flappie_map_ref_read(str(tmp_path / "missing.fa").encode(), err, 256) and b"cannot be read" in err.value
    (tmp_path / "nul.fa").write_bytes(b">a\nAC\0GT\n")
    assert not L.flappie_map_ref_read(str(tmp_path / "nul.fa").encode(), err, 256) and b"NUL" in err.value


def c_call(rec):
    c = Call()
    c.v[:] = R.raw(rec).tolist()
    return c


def test_the_coordinate_flip_and_the_writers(L, tmp_path):
    ref, _ = parse(L, REF_TEXT)
    records, names = [s for _, s in REF_WANT], [n for n, _ in REF_WANT]
    lens = [len(s) for s in records]
    for q in range(6):
        m = lens[q >> 1]
        for a in range(m + 1):
            for b in range(a, m + 1):
                k, o, fa, fb = C.c_int(-1), C.create_string_buffer(2), C.c_long(-1), C.c_long(-1)
                assert L.flappie_map_forward(ref, q, a, b, C.byref(k), o, C.byref(fa), C.byref(fb)) == 0
                assert (k.value, o.value[:1].decode(), fa.value, fb.value) == R.forward(q, a, b, lens)
                assert R.searches(records)[q][a:b] == (records[q >> 1][fa.value:fb.value] if q % 2 == 0 else R.revcomp(records[q >> 1][fa.value:fb.value]))
    for q, a, b in ((-1, 0, 1), (6, 0, 1), (0, -1, 2), (0, 3, 2), (0, 0, 9), (5, 0, 2)):
        assert L.flappie_map_forward(ref, q, a, b, None, None, None, None) == -1
    # hand-made records of every status, both strands, one anchor and two; and the restatement's own on calls cut from the reference
    an = lambda q, s, e, d, d2: dict(zip(R.ANCHOR_FIELDS, (q, s, e, d, d2)))      # noqa: E731
    zero = an(0, 0, 0, 0, 0)
    recs = [("none", dict(status=0, n=0, nanchor=0, q=0, tstart=0, tend=0, anchors=[zero, zero])),
            ("plus", dict(status=1, n=5, nanchor=1, q=0, tstart=2, tend=7, anchors=[an(0, 2, 7, 1, 3)] * 2)),
            ("minus", dict(status=1, n=6, nanchor=2, q=3, tstart=0, tend=6, anchors=[an(3, 0, 3, 0, 2), an(3, 4, 6, 1, 1)])),
            ("whole", dict(status=1, n=1, nanchor=1, q=5, tstart=0, tend=1, anchors=[an(5, 0, 1, 0, 0)] * 2)),
            ("over", dict(status=2, n=9, nanchor=1, q=0, tstart=0, tend=0, anchors=[an(2, 1, 6, 4, 4)] * 2)),
            ("apart", dict(status=3, n=9, nanchor=2, q=0, tstart=0, tend=0, anchors=[an(1, 0, 3, 0, 1), an(2, 2, 7, 1, 2)]))]
    for i, call in enumerate(("GTAC", "TGGTCAA", "C", "ACGTACGTTT")):
        recs.append(("cut%d" % i, R.record(records, call, 64, 250)))
    libc = C.CDLL(None)
    hits, fasta, summ = tmp_path / "hits.tsv", tmp_path / "recs.fa", tmp_path / "sum.txt"
    fh, ff, fs = _cfile(libc, hits), _cfile(libc, fasta), _cfile(libc, summ)
    s = Summary()
    for name, rec in recs:
        c = c_call(rec)
        assert L.flappie_map_write_line(fh, name.encode(), C.byref(c), ref) == 0
        assert L.flappie_map_write_record(ff, name.encode(), C.byref(c), ref) == (1 if rec["status"] == 1 else 0)
        L.flappie_map_summary_add(C.byref(s), C.byref(c), 64)
    bad = c_call(recs[1][1])
    bad.v[5] = 9                                              # tend beyond the record
    assert L.flappie_map_write_line(fh, b"bad", C.byref(bad), ref) == -1 and L.flappie_map_write_record(ff, b"bad", C.byref(bad), ref) == -1
    bad.v[0] = 4
    assert L.flappie_map_write_line(fh, b"bad", C.byref(bad), ref) == -1
    L.flappie_map_summary_print(fs, C.byref(s))
    for f in (fh, ff, fs):
        libc.fclose(f)
    want = [rec for _, rec in recs]
    assert hits.read_text() == "".join(R.hits_line(name, rec, names, lens) for name, rec in recs)
    assert hits.read_text().splitlines()[:6] == ["none\t0\t0\t0\t*\t*\t*\t*\t*\t0\t0\t0\t0", "plus\t1\t5\t1\tlambda\t+\t2\t7\t8\t1\t3\t1\t3", "minus\t1\t6\t2\tplasmid.2\t-\t1\t7\t7\t0\t2\t1\t1",
                                                 "whole\t1\t1\t1\tx\t-\t0\t1\t1\t0\t0\t0\t0", "over\t2\t9\t1\t*\t*\t*\t*\t*\t4\t4\t4\t4\tplasmid.2\t+\t1\t6\tplasmid.2\t+\t1\t6",
                                                 "apart\t3\t9\t2\t*\t*\t*\t*\t*\t0\t1\t1\t2\tlambda\t-\t5\t8\tplasmid.2\t+\t2\t7"]
    assert fasta.read_text() == "".join(R.record_text(name, rec, records) for name, rec in recs)
    assert fasta.read_text().startswith(">plus\nGTACG\n>minus\nTGGTCA\n>whole\nC\n")
    assert dict(line.split("\t")[1:] for line in summ.read_text().splitlines()) == R.summary(want, 64)
    assert all(line.startswith("map\t") for line in summ.read_text().splitlines())
    L.flappie_map_ref_free(ref)


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(REF_TEXT)
    opts = ("--map", "--map-out", "--map-window", "--map-max-error", "--map-records")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(opt + "=" in r.stdout for opt in opts), r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert not any(opt + "=" in r.stdout for opt in opts)

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out = str(tmp_path / "hits.tsv")
    for args in (["--map", str(fa)], ["--map-out", out], ["--map-window", "100"], ["--map-max-error", "100"], ["--map-records", out], ["--map", str(fa), "--map-out", out]):
        assert "--map is flappie's" in refused(RUNNIE, *args)
    assert "--map and --map-out go together" in refused(FLAPPIE, "--map", str(fa))
    for alone in (["--map-out", out], ["--map-window", "100"], ["--map-max-error", "100"], ["--map-records", out]):
        assert "go with --map" in refused(FLAPPIE, *alone)
    for bad in (["--map-window", "63"], ["--map-window", "4097"], ["--map-window", "x"], ["--map-max-error", "501"], ["--map-max-error", "-1"], ["--map-max-error", "2.5"]):
        assert "must be a whole number" in refused(FLAPPIE, "--map", str(fa), "--map-out", out, *bad)
    for what, text in (("empty", ""), ("N", ">a\nACGN\n"), ("twice", ">a\nAC\n>a\nGT\n"), ("no sequence", ">a\n>b\nAC\n")):
        bad = tmp_path / "bad.fa"
        bad.write_text(text)
        assert "bad.fa" in refused(FLAPPIE, "--map", str(bad), "--map-out", out), what
    assert "missing.fa" in refused(FLAPPIE, "--map", str(tmp_path / "missing.fa"), "--map-out", out)
    assert "cannot be written" in refused(FLAPPIE, "--map", str(fa), "--map-out", str(tmp_path / "no" / "dir.tsv"))
