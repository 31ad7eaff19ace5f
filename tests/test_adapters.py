"""flappie --adapters without a GPU: the numpy restatement (adapter_ref.py) against an independent brute force; the locality claim the segmented kernel rests on;
the host side (kit parser, tag formatter, trim, split, record writer of libflappie_host.so) against the restatement on hand-made records; the CLI's refusals.
Everything is integer- or byte-exact."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import adapter_ref as R
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, BasecallInfo, _cfile, needs_hdf5
from test_host_layer import RawTable

U8P = C.POINTER(C.c_uint8)


class Header(C.Structure):
    _fields_ = [("nhit", C.c_int32), ("len", C.c_int32), ("kept", C.c_int32), ("reserved", C.c_int32)]


class Hit(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("pattern", C.c_int16), ("orientation", C.c_uint8), ("dist", C.c_uint8), ("reserved", C.c_int32)]


class Kit(C.Structure):
    _fields_ = [("n", C.c_int), ("name", C.POINTER(C.c_char_p)), ("seq", C.POINTER(C.c_char_p))]


class Piece(C.Structure):
    _fields_ = [("a", C.c_size_t), ("b", C.c_size_t)]


class Out(C.Structure):
    _fields_ = [("head", C.POINTER(Header)), ("hits", C.POINTER(Hit)), ("kit", C.POINTER(Kit)), ("trim", C.c_bool), ("split", C.c_bool), ("window", C.c_int),
                ("min_length", C.c_size_t)]


def c_record(rec):
    hits = (Hit * 15)()
    for i, (s, e, k, o, d) in enumerate(rec["hits"]):
        hits[i] = Hit(s, e, k, o, d, 0)
    return Header(rec["nhit"], rec["len"], rec["kept"], 0), hits


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_adapter_kit_parse.restype = C.POINTER(Kit)
    L.flappie_adapter_kit_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_adapter_kit_read.restype = C.POINTER(Kit)
    L.flappie_adapter_kit_read.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_adapter_kit_free.argtypes = [C.POINTER(Kit)]
    L.flappie_adapter_kit_free.restype = None
    L.flappie_adapter_tags.restype = C.c_void_p
    L.flappie_adapter_tags.argtypes = [C.POINTER(Header), C.POINTER(Hit), C.POINTER(Kit)]
    L.flappie_adapter_trim.argtypes = [C.POINTER(Header), C.POINTER(Hit), C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.flappie_adapter_split.argtypes = [C.POINTER(Header), C.POINTER(Hit), C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(Piece), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    L.fprintf_format.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo]
    L.fprintf_adapter_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo, U8P, U8P, C.c_int, C.c_float, C.c_float,
                                         C.c_bool, C.c_void_p, C.c_void_p, C.c_bool, C.POINTER(Out), C.c_bool, C.POINTER(C.c_ulonglong)]
    L.fprintf_adapter_record.restype = None
    return L


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def brute_rows(p, x):
    """d[j] = the least distance of p to any substring of x that ends at j"""
    return [min(levenshtein(p, x[i:j]) for i in range(j + 1)) for j in range(len(x) + 1)]


def brute_hits(rows, md, reach):
    """a direct scan of the hit rule over python lists"""
    out = []
    for j in range(len(rows[0])):
        for q, d in enumerate(rows):
            if d[j] > md[q]:
                continue
            left = [d[t] for t in range(max(0, j - reach), j)]
            right = [d[t] for t in range(j + 1, min(len(d), j + reach + 1))]
            if all(v > d[j] for v in left) and all(v >= d[j] for v in right):
                out.append((j, q))
    return out


def test_restatement_against_brute_force_over_all_substrings():
    rng = np.random.default_rng(2)
    nhit = 0
    for t in range(150):
        two = rng.random() < 0.3                              # (a two-letter alphabet: repeats, ties, homopolymers)
        pats = [rand_seq(rng, int(rng.integers(1, 9)), "AC" if two else "ACGT") for _ in range(int(rng.integers(1, 4)))]
        x = rand_seq(rng, int(rng.integers(0, 30)), "ACZ" if two else "ACGTZ")
        plain = x.replace("Z", "C")
        d = R.score_rows(pats, x)
        sp = R.searches(pats)
        assert sp[1::2] == [R.revcomp(p) for p in pats] and d.shape == (2 * len(pats), len(x) + 1)
        rows = [brute_rows(p, plain) for p in sp]
        assert d.tolist() == rows, (pats, x)
        md = int(rng.integers(-1, 4))
        bound = R.bounds(pats, md)
        assert bound.tolist() == [(len(p) // 4 if md < 0 else min(md, len(p) - 1)) for p in sp]
        rec = R.record(pats, x, md)
        ends = brute_hits(rows, bound, R.R)
        assert rec["nhit"] == len(ends) and rec["len"] == len(x) and rec["kept"] == min(15, len(ends))
        assert [(e, 2 * k + o) for s, e, k, o, dd in rec["hits"]] == ends[:15], (pats, x)
        for s, e, k, o, dd in rec["hits"]:
            p = sp[2 * k + o]
            assert dd == rows[2 * k + o][e] and s == max(i for i in range(e + 1) if levenshtein(p, plain[i:e]) == dd), (pats, x, s, e)
            nhit += 1
    assert nhit > 100


def test_hit_rule_ties_homopolymers_and_short_calls():
    # a homopolymer run: every column from 4 on has distance 0 -- one hit, the leftmost, however long the run (every later column has its equal just before it)
    rec = R.record(["AAAA"], "C" + "A" * 40 + "C", 0)
    assert [(h[0], h[1], h[3]) for h in rec["hits"]] == [(1, 5, 0)]
    rec = R.record(["AAAA"], "C" + "A" * 100, 0)
    assert [(h[0], h[1]) for h in rec["hits"] if h[3] == 0] == [(1, 5)]
    # equal distances inside and outside R: two exact copies whose ends are 64 / 65 columns apart
    p = "ACGTTGCATGCA"
    for gap, want in ((64, 1), (65, 2)):
        x = "T" * 5 + p + "T" * (gap - len(p)) + p + "T" * 5
        rec = R.record([p], x, 0)
        fwd = [(h[0], h[1]) for h in rec["hits"] if h[3] == 0]
        assert len(fwd) == want and fwd[0] == (5, 5 + len(p)), (gap, fwd)
    # a smaller distance to the right within R beats a larger one to the left; beyond R both stand
    worse = p[:5] + "T" + p[6:]
    for gap, want in ((40, [0]), (80, [1, 0])):
        x = "GG" + worse + "G" * (gap - len(p)) + p + "GG"
        rec = R.record([p], x, 2)
        assert [h[4] for h in rec["hits"] if h[3] == 0] == want, (gap, rec)
    # ... and a smaller one to the LEFT within R removes the right one
    x = "GG" + p + "G" * (40 - len(p)) + worse + "GG"
    assert [h[4] for h in R.record([p], x, 2)["hits"] if h[3] == 0] == [0]
    # len < L, len = 0: the rows exist, column 0 holds L and is never a hit
    assert R.score_rows(["ACGTACGT"], "").tolist() == [[8], [8]] and R.record(["ACGTACGT"], "") == R.EMPTY
    rec = R.record(["ACGTACGT"], "ACGTAC", 2)
    assert rec["len"] == 6 and [(h[0], h[1], h[4]) for h in rec["hits"] if h[3] == 0] == [(0, 6, 2)]
    assert R.record(["ACGTACGT"], "ACGTAC", 1)["nhit"] == 0 and R.record(["ACGTACGT"], "ACGTAC", -1)["nhit"] == 2      # (its own reverse complement: both searches)
    # both orientations; the order (end, q); the cap at 15 with nhit counting all
    a, b = "ACCGTTAGGCAT", "TTGACCAGTACA"
    x = "".join("G" * 70 + (a if i % 2 == 0 else R.revcomp(b)) for i in range(20))
    rec = R.record([a, b], x, 0)
    assert rec["nhit"] == 20 and rec["kept"] == 15 and len(rec["hits"]) == 15
    assert [(h[2], h[3]) for h in rec["hits"]] == [(0, 0) if i % 2 == 0 else (1, 1) for i in range(15)]
    assert [h[1] for h in rec["hits"]] == sorted(h[1] for h in rec["hits"]) and R.raw_slots(rec).shape == (60,)
    pal = "ACGT"                                                  # a palindrome: both searches hit the same column, q = 0 first
    rec = R.record([pal], "GGGGACGTGGGG", 0)
    assert rec["hits"] == [(4, 8, 0, 0, 0), (4, 8, 0, 1, 0)]


def test_locality_a_fresh_start_is_exact_128_columns_on():
    rng = np.random.default_rng(5)
    ncol = 0
    for L in (1, 17, 40, 63, 64):
        pats = [rand_seq(rng, L), rand_seq(rng, max(1, L // 2))]
        for a in (100, 257):
            x = list(rand_seq(rng, a + 300))
            # planted matches that straddle a: copies with edits (insertions make them longer than L) that end a few columns either side of a + 128
            for k, at in enumerate((a - L // 2, a + 128 - 3 * L // 2, a + 126 - L)):
                p = list(pats[k % 2] if k < 2 else R.revcomp(pats[0]))
                for _ in range(min(L // 4, 6)):
                    p.insert(int(rng.integers(0, len(p))), "ACGT"[int(rng.integers(0, 4))])
                at = max(0, at)
                x[at:at + len(p)] = p
            x = "".join(x)
            full, fresh = R.score_rows(pats, x), R.score_rows(pats, x, start_at=a)
            assert np.array_equal(full[:, a + 128:], fresh[:, a + 128:]), (L, a)
            assert (fresh[:, a:] >= full[:, a:]).all() and (full <= np.repeat([len(p) for p in pats], 2)[:, None]).all()
            ncol += full.shape[1] - a - 128
        # the bound is tight enough to matter: a fresh start in the middle of an exact copy of the pattern is wrong just behind it
        x = "G" * 50 + pats[0] + "G" * 50
        if L >= 17:
            assert not np.array_equal(R.score_rows(pats, x)[:, 50 + L], R.score_rows(pats, x, start_at=50 + L // 2)[:, 50 + L])
    assert ncol > 1000


KIT_TEXT = "\n>ad01 first adapter\nacgtAC\nGTTT\n\n>ad02\nTTTTGGGG\n>ad03\tx\nA\n"
NAMES = ["ad01", "ad02", "ad03"]


def test_kit_parser_and_every_refusal(L, tmp_path):
    err = C.create_string_buffer(256)
    kit = L.flappie_adapter_kit_parse(KIT_TEXT.encode(), err, 256)
    assert kit and kit.contents.n == 3
    got = [(kit.contents.name[k].decode(), kit.contents.seq[k].decode()) for k in range(3)]
    assert got == [("ad01", "ACGTACGTTT"), ("ad02", "TTTTGGGG"), ("ad03", "A")] == R.parse_kit(KIT_TEXT)
    L.flappie_adapter_kit_free(kit)
    path = tmp_path / "kit.fa"
    path.write_text(KIT_TEXT.replace("\n", "\r\n"))
    kit = L.flappie_adapter_kit_read(str(path).encode(), err, 256)
    assert kit and kit.contents.n == 3 and kit.contents.seq[0] == b"ACGTACGTTT"
    L.flappie_adapter_kit_free(kit)
    full = "".join(">a%d\n%s\n" % (k, "ACGT" * 16) for k in range(32))
    kit = L.flappie_adapter_kit_parse(full.encode(), err, 256)
    assert kit and kit.contents.n == 32 and len(R.parse_kit(full)) == 32
    L.flappie_adapter_kit_free(kit)
    bad = {"empty": "", "blank": "\n\n", "too many": full + ">one_more\nA\n", "too long": ">a\n" + "A" * 65 + "\n", "too long over lines": ">a\n" + ("A" * 33 + "\n") * 2,
           "N": ">a\nACGN\n", "Z": ">a\nACGZ\n", "blank inside": ">a\nAC GT\n", "duplicate": ">a\nAC\n>b\nGT\n>a\nTT\n", "no sequence": ">a\n>b\nAC\n",
           "no sequence at the end": ">a\nAC\n>b\n", "no name": ">\nAC\n", "text first": "ACGT\n>a\nAC\n", "comma": ">a,b\nAC\n", "semicolon": ">a;b\nAC\n"}
    for what, text in bad.items():
        err.value = b""
        assert not L.flappie_adapter_kit_parse(text.encode(), err, 256), what
        assert err.value, what
        with pytest.raises(ValueError):
            R.parse_kit(text)
    assert not L.flappie_adapter_kit_read(str(tmp_path / "missing.fa").encode(), err, 256)


def _records(length=1000):
    """hand-made records of a call of `length` bases: none, front, rear, both, interior, several interior, overlapping, touching, crossing, overflow"""
    def H(*hits, nhit=None):                             # (a shorter call: the hits that lie within it, in (end, q) order as every record is)
        inside = sorted((h for h in hits if 0 <= h[0] < h[1] <= length), key=lambda h: (h[1], 2 * h[2] + h[3]))
        return {"nhit": len(inside) + (0 if nhit is None else nhit - len(hits)), "len": length, "kept": len(inside), "hits": inside}
    n = length
    return [H(),
            H((0, 28, 0, 0, 1)),
            H((n - 30, n - 2, 1, 1, 0)),
            H((3, 31, 0, 0, 2), (40, 50, 2, 0, 0), (n - 30, n - 2, 1, 1, 0)),
            H((2, 30, 0, 0, 0), (480, 508, 1, 1, 3), (n - 28, n, 0, 1, 0)),
            H((250, 278, 0, 0, 0), (500, 528, 1, 0, 1), (640, 668, 0, 1, 0)),
            H((300, 340, 0, 0, 0), (320, 350, 1, 0, 0), (350, 360, 2, 1, 0), (330, 700, 0, 1, 1)),      # overlapping, touching, one inside another (ordered by end)
            H((100, 160, 0, 0, 0), (155, 400, 1, 0, 0)),                                                  # a front hit's neighbour reaches into the interior
            H((0, 150, 0, 0, 0), (n - 150, n - 120, 1, 0, 0)),                                            # the largest window
            H((0, 120, 0, 0, 0), (60, 110, 1, 0, 0)),
            H(*[(50 * i + 200, 50 * i + 228, i % 3, i % 2, i % 4) for i in range(15)]),
            H(*[(50 * i + 200, 50 * i + 228, i % 3, i % 2, i % 4) for i in range(15)], nhit=16),
            H(*[(10 * i, 10 * i + 8, 0, 0, 0) for i in range(15)], nhit=40)]


def test_tags_trim_and_split_equal_the_restatement(L):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    err = C.create_string_buffer(256)
    kit = L.flappie_adapter_kit_parse(KIT_TEXT.encode(), err, 256)
    modes = {0: "whole", 1: "split", 2: "overflow"}
    seen = set()
    for length in (1000, 300, 160, 40):
        for rec in _records(length) + [{"nhit": 2, "len": length, "kept": 2, "hits": [(0, min(length, 30), 0, 0, 0), (max(0, length - 35), length, 1, 0, 0)]}]:
            head, hits = c_record(rec)
            p = L.flappie_adapter_tags(C.byref(head), hits, kit)
            assert p and C.string_at(p).decode() == R.tags(rec, NAMES), rec
            libc.free(p)
            for W in (150, 60, 0):
                a, b = C.c_size_t(99), C.c_size_t(99)
                crossed = L.flappie_adapter_trim(C.byref(head), hits, length, W, C.byref(a), C.byref(b))
                assert (a.value, b.value) == R.trim_range(rec, length, W), (rec, length, W)
                assert bool(crossed) == (R.trim_range(rec, length, W) == (0, 0) and length > 0 and rec["kept"] > 0)
                for M, clip in itertools.product((200, 25, 0), (None, (40, length - 17), (length // 2, length // 2 + 1))):
                    pieces, np_, nd = (Piece * 16)(), C.c_int(-1), C.c_int(-1)
                    cf, ct = clip if clip else (0, length)
                    mode = L.flappie_adapter_split(C.byref(head), hits, length, W, M, cf, ct, pieces, C.byref(np_), C.byref(nd))
                    want = R.split_pieces(rec, length, W, M, clip)
                    assert (modes[mode], [(pieces[i].a, pieces[i].b) for i in range(np_.value)], nd.value) == want, (rec, length, W, M, clip)
                    seen.add((want[0], len(want[1]) > 1, want[2] > 0))
    assert {("whole", False, False), ("split", True, False), ("split", True, True), ("split", False, True), ("overflow", False, False)} <= seen, seen
    # by hand
    r = _records()
    assert R.tags(r[0], NAMES) == "an:i:0\tah:Z:" and R.tags(r[3], NAMES) == "an:i:3\tah:Z:ad01,+,3,31,2;ad03,+,40,50,0;ad02,-,970,998,0;"
    assert R.trim_range(r[3], 1000) == (50, 970) and R.trim_range(r[3], 1000, 45) == (31, 970) and R.trim_range(r[4], 1000) == (30, 972)
    assert R.split_pieces(r[4], 1000) == ("split", [(30, 480), (508, 972)], 0) and R.split_pieces(r[4], 1000, M=460) == ("split", [(508, 972)], 1)
    assert R.split_pieces(r[6], 1000) == ("split", [(0, 300), (700, 1000)], 0) and R.split_pieces(r[3], 1000) == ("whole", [(50, 970)], 0)
    assert R.split_pieces(r[11], 1000)[0] == "overflow" and R.split_pieces(r[10], 1000)[0] == "split"
    assert R.combine_trims((10, 90), (20, 95), 100) == (20, 90) and R.combine_trims((0, 40), (60, 100), 100) == (0, 0) and R.combine_trims((0, 0), (0, 100), 100) == (0, 0)
    bad_head, bad_hits = c_record(dict(r[1], hits=[(0, 28, 3, 0, 1)]))
    assert not L.flappie_adapter_tags(C.byref(bad_head), bad_hits, kit)       # a pattern beyond the kit
    L.flappie_adapter_kit_free(kit)


def _write(L, libc, path, fn, *a):
    fp = _cfile(libc, path)
    fn(*a[:1], fp, *a[1:])
    libc.fclose(fp)
    return path.read_text()


def test_records_equal_the_restatement(L, tmp_path):
    libc = C.CDLL(None)
    err = C.create_string_buffer(256)
    kit = L.flappie_adapter_kit_parse(KIT_TEXT.encode(), err, 256)
    rng = np.random.default_rng(1)
    length = 1000
    call, qual = rand_seq(rng, length), "".join(chr(33 + int(v)) for v in rng.integers(0, 40, length))
    fmts = {0: "fasta", 1: "fastq", 2: "sam"}
    total = np.zeros(4, np.int64)
    for rec in _records(length):
        head, hits = c_record(rec)
        for reverse, uuid_first, (trim, split, W, M) in itertools.product((False, True), (True, False), ((False, False, 150, 200), (True, False, 150, 200), (True, False, 45, 200),
                                                                                                         (False, True, 150, 200), (True, True, 150, 460))):
            c, q = (call[::-1], qual[::-1]) if reverse else (call, qual)
            res = BasecallInfo(score=np.float32(-123.5), basecall=c.encode(), quality=q.encode(), basecall_length=len(c), nblock=400)
            res.rt = RawTable(uuid=b"u-1", n=4000, start=200, end=3990, raw=None)
            out = Out(C.pointer(head), hits, kit, trim, split, W, M)
            name = "u-1" if uuid_first else "a.fast5"
            for fmt in range(3):
                default = _write(L, libc, tmp_path / "d", L.fprintf_format, fmt, b"u-1", b"a.fast5", uuid_first, b"PRE_", res).split("\n")
                stats = (C.c_ulonglong * 4)()
                got = _write(L, libc, tmp_path / "t", L.fprintf_adapter_record, fmt, b"u-1", b"a.fast5", uuid_first, b"PRE_", res, None, None, 5, 0.0, 1.0, False,
                             None, None, False, C.byref(out), reverse, stats)
                want = R.records_text(fmts[fmt], default[0], call, qual, rec, NAMES, name, reverse=reverse, trim=trim, split=split, W=W, M=M)
                assert got == want, (rec, reverse, uuid_first, trim, split, fmt)
                mode, pieces, dropped, overflow = R.cuts(rec, length, trim, split, W, M)
                assert list(stats) == [int(mode == "split"), len(pieces) if mode == "split" else 0, dropped, int(overflow)], (rec, list(stats))
                total += np.array(list(stats))
                if mode == "split" and fmt == 1 and pieces:
                    first = got.split("\n")[0]
                    assert first.startswith("@PRE_%s:1  {" % name) and first.endswith("\tpi:Z:%s\tsp:B:i,%d,%d" % (name, pieces[0][0], pieces[0][1]))
    assert (total > 0).all(), total
    L.flappie_adapter_kit_free(kit)


@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    kit = tmp_path / "kit.fa"
    kit.write_text(KIT_TEXT)
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    opts = ("--adapters", "--adapter-max-dist", "--trim-adapters", "--adapter-window", "--split-reads", "--split-min-length")
    for opt in opts:
        assert opt in r.stdout, opt
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert not any(opt in r.stdout for opt in opts)

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    for args in (["--adapters", str(kit)], ["--trim-adapters"], ["--split-reads"], ["--adapter-window", "100"], ["--split-min-length", "10"], ["--adapter-max-dist", "2"]):
        assert "--adapters" in refused(RUNNIE, *args)
    refs = tmp_path / "refs.fa"
    refs.write_text(">r\nACGT\n")
    others = (["--emit-moves"], ["--modbase-tags", "--model", "r941_5mC"], ["--trace", str(tmp_path / "t.hdf5")])
    for other in others:
        assert "--trim-adapters" in refused(FLAPPIE, "--adapters", str(kit), "--trim-adapters", *other)
    for other in others + (["--remap", str(refs), "--remap-out", str(tmp_path / "m.tsv")], ["--truth", str(refs), "--truth-out", str(tmp_path / "a.tsv")]):
        assert "--split-reads" in refused(FLAPPIE, "--adapters", str(kit), "--split-reads", *other)
    assert not any((tmp_path / f).exists() for f in ("t.hdf5", "m.tsv", "a.tsv"))
    for alone in (["--trim-adapters"], ["--adapter-window", "100"], ["--adapter-max-dist", "3"], ["--split-reads"], ["--split-min-length", "100"]):
        assert "--adapters" in refused(FLAPPIE, *alone)
    assert "--adapter-window" in refused(FLAPPIE, "--adapters", str(kit), "--adapter-window", "100")
    assert "--split-min-length" in refused(FLAPPIE, "--adapters", str(kit), "--trim-adapters", "--split-min-length", "100")
    for bad in (["--adapter-max-dist", "-1"], ["--adapter-max-dist", "64"], ["--adapter-max-dist", "x"], ["--trim-adapters", "--adapter-window", "-1"], ["--split-reads", "--split-min-length", "-5"]):
        refused(FLAPPIE, "--adapters", str(kit), *bad)
    # a bad kit file: refused before any fast5 file or the GPU is touched
    texts = {"empty": "", "too many": "".join(">a%d\nACGT\n" % k for k in range(33)), "too long": ">a\n" + "A" * 65 + "\n", "N": ">a\nACGN\n", "duplicate": ">a\nAC\n>a\nGT\n",
             "comma": ">a,b\nACGT\n"}
    for what, text in texts.items():
        bad = tmp_path / "bad.fa"
        bad.write_text(text)
        assert "bad.fa" in refused(FLAPPIE, "--adapters", str(bad)), what
    assert "missing.fa" in refused(FLAPPIE, "--adapters", str(tmp_path / "missing.fa"))
