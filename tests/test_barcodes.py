"""flappie --barcodes on the CPU: the restatement (barcode_ref.py) against a brute-force minimum of the Levenshtein distance over all substrings; the kit parser,
the tag formatter, the trim and the record writer of libflappie_host.so (include/flappie_barcodes.h) against the restatement, byte for byte; the options'
refusals, which need no GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import barcode_ref as R
import modbase_ref as MR
import moves_ref as VR
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, BasecallInfo, _cfile, needs_hdf5
from test_host_layer import RawTable

U8P = C.POINTER(C.c_uint8)


class Call(C.Structure):
    _fields_ = [("best", C.c_int16), ("best_dist", C.c_uint8), ("second_dist", C.c_uint8), ("front_dist", C.c_uint8), ("rear_dist", C.c_uint8),
                ("ends", C.c_uint8), ("pad", C.c_uint8), ("front_end", C.c_int16), ("rear_end", C.c_int16), ("reserved", C.c_int32)]


class Kit(C.Structure):
    _fields_ = [("n", C.c_int), ("name", C.POINTER(C.c_char_p)), ("seq", C.POINTER(C.c_char_p)), ("lmin", C.c_int)]


def call_of(rec):
    return Call(**{k: rec[k] for k in R.FIELDS})


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(HOSTLIB)
    L.flappie_barcode_kit_parse.restype = C.POINTER(Kit)
    L.flappie_barcode_kit_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_barcode_kit_read.restype = C.POINTER(Kit)
    L.flappie_barcode_kit_read.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_barcode_kit_free.argtypes = [C.POINTER(Kit)]
    L.flappie_barcode_kit_free.restype = None
    L.flappie_barcode_tags.restype = C.c_void_p
    L.flappie_barcode_tags.argtypes = [C.POINTER(Call), C.POINTER(Kit)]
    L.flappie_barcode_trim.argtypes = [C.POINTER(Call), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.fprintf_format.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo]
    L.fprintf_barcode_record.argtypes = [C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool, C.c_char_p, BasecallInfo, U8P, U8P, C.c_int, C.c_float, C.c_float,
                                         C.c_bool, C.POINTER(Call), C.POINTER(Kit), C.c_bool, C.c_bool]
    return L


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def test_restatement_against_brute_force_over_all_substrings():
    rng = np.random.default_rng(2)
    n = 0
    for _ in range(400):
        p = "".join("ACGT"[i] for i in rng.integers(0, 4 if rng.random() < 0.7 else 2, rng.integers(1, 13)))
        x = "".join("ACGT"[i] for i in rng.integers(0, 4 if rng.random() < 0.7 else 2, rng.integers(0, 13)))
        # the least distance of p to any substring x[a:e], and the smallest end e among those that attain it (the empty substring ends at 0 .. m)
        best = min((levenshtein(p, x[a:e]), e) for e in range(len(x) + 1) for a in range(e + 1))
        assert R.infix(p, x) == best, (p, x)
        n += 1
    assert R.infix("ACGT", "") == (4, 0) and R.infix("A", "AAAA") == (0, 1) and R.infix("ACGT", "TTACGTACGT") == (0, 6)
    # windows: the rear is the front of the reverse complement, Z is read as C
    assert R.windows("AZGTT", 3) == ("ACG", "AAC") and R.windows("AC", 150) == ("AC", "GT") and R.windows("", 5) == ("", "")
    # the rules: the lowest index of the minimum, the runner-up among the others, both ends
    c = R.classify(["AACCGTTA", "AACCGTTA", "TTTTTTTT"], "AACCGTTACCCCCCCCCCCC", 150, 1, 3)
    assert c["best"] == -1 and c["best_dist"] == 0 and c["second_dist"] == 0 and c["front_dist"] == 0 and c["front_end"] == 8 and c["ends"] == 1
    c = R.classify(["AACCGTTA", "TTTTTTTT"], "AACCGTTACCCCCCCCCCCC", 150, 1, 3)
    assert c["best"] == 0 and c["second_dist"] >= 3 and R.category(c, 1) == "front"
    assert R.classify(["AACCGTTA", "TTTTTTTT"], "AACCGTTACCCCCCCCCCCC", 150, 1, 3, both_ends=True)["best"] == -1
    c = R.classify(["ACGTACGA"], "CCCCCCCCCCCCTCGTACGT", 150, 1, 3)
    assert c["best"] == 0 and c["second_dist"] == 255 and c["rear_dist"] == 0 and c["rear_end"] == 8 and c["ends"] == 2 and R.category(c, 1) == "rear"


KIT_TEXT = "\n>bc01 first sample\nacgtAC\nGTTT\n\n>bc02\nTTTTGGGG\n>bc03\tx\nA\n"


def test_kit_parser_and_every_refusal(L, tmp_path):
    err = C.create_string_buffer(256)
    kit = L.flappie_barcode_kit_parse(KIT_TEXT.encode(), err, 256)
    assert kit and kit.contents.n == 3 and kit.contents.lmin == 1
    got = [(kit.contents.name[k].decode(), kit.contents.seq[k].decode()) for k in range(3)]
    assert got == [("bc01", "ACGTACGTTT"), ("bc02", "TTTTGGGG"), ("bc03", "A")] == R.parse_kit(KIT_TEXT)
    L.flappie_barcode_kit_free(kit)
    path = tmp_path / "kit.fa"
    path.write_text(KIT_TEXT.replace("\n", "\r\n"))
    kit = L.flappie_barcode_kit_read(str(path).encode(), err, 256)
    assert kit and kit.contents.n == 3 and kit.contents.seq[0] == b"ACGTACGTTT"
    L.flappie_barcode_kit_free(kit)
    full = "".join(">b%d\n%s\n" % (k, "ACGT" * 32) for k in range(128))
    kit = L.flappie_barcode_kit_parse(full.encode(), err, 256)
    assert kit and kit.contents.n == 128 and kit.contents.lmin == 128
    L.flappie_barcode_kit_free(kit)
    bad = {"empty": "", "blank": "\n\n", "too many": full + ">one_more\nA\n", "too long": ">a\n" + "A" * 129 + "\n", "too long over lines": ">a\n" + ("A" * 65 + "\n") * 2,
           "N": ">a\nACGN\n", "Z": ">a\nACGZ\n", "blank inside": ">a\nAC GT\n", "duplicate": ">a\nAC\n>b\nGT\n>a\nTT\n", "no sequence": ">a\n>b\nAC\n",
           "no sequence at the end": ">a\nAC\n>b\n", "no name": ">\nAC\n", "text first": "ACGT\n>a\nAC\n"}
    for what, text in bad.items():
        err.value = b""
        assert not L.flappie_barcode_kit_parse(text.encode(), err, 256), what
        assert err.value, what
        with pytest.raises(ValueError):
            R.parse_kit(text)
    assert not L.flappie_barcode_kit_read(str(tmp_path / "missing.fa").encode(), err, 256)


def _records(n=3):
    rng = np.random.default_rng(4)
    out = [dict(best=1, best_dist=2, second_dist=9, front_dist=2, rear_dist=7, ends=1, front_end=5, rear_end=4),
           dict(best=0, best_dist=0, second_dist=255, front_dist=3, rear_dist=0, ends=3, front_end=3, rear_end=4),
           dict(best=2, best_dist=1, second_dist=6, front_dist=8, rear_dist=1, ends=2, front_end=0, rear_end=2),
           dict(best=-1, best_dist=7, second_dist=7, front_dist=7, rear_dist=9, ends=0, front_end=11, rear_end=3),
           dict(best=-1, best_dist=1, second_dist=2, front_dist=1, rear_dist=1, ends=3, front_end=6, rear_end=6),      # rejected by min_sep: nothing is cut
           dict(best=1, best_dist=1, second_dist=8, front_dist=1, rear_dist=1, ends=3, front_end=6, rear_end=5),       # the cuts meet
           dict(best=1, best_dist=1, second_dist=8, front_dist=1, rear_dist=1, ends=3, front_end=9, rear_end=9),       # the cuts cross
           dict(best=1, best_dist=1, second_dist=8, front_dist=1, rear_dist=1, ends=3, front_end=6, rear_end=4)]
    for _ in range(20):
        out.append(dict(best=int(rng.integers(-1, n)), best_dist=int(rng.integers(0, 129)), second_dist=int(rng.integers(0, 256)), front_dist=int(rng.integers(0, 129)),
                        rear_dist=int(rng.integers(0, 129)), ends=int(rng.integers(0, 4)), front_end=int(rng.integers(0, 257)), rear_end=int(rng.integers(0, 257))))
    return out


def test_tags_and_trim_equal_the_restatement(L):
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    err = C.create_string_buffer(256)
    kit = L.flappie_barcode_kit_parse(KIT_TEXT.encode(), err, 256)
    names = ["bc01", "bc02", "bc03"]
    for rec in _records():
        p = L.flappie_barcode_tags(C.byref(call_of(rec)), kit)
        assert p
        assert C.string_at(p).decode() == R.tags(rec, names), rec
        libc.free(p)
        for length in (0, 1, 10, 11, 12, 18, 300):
            a, b = C.c_size_t(99), C.c_size_t(99)
            crossed = L.flappie_barcode_trim(C.byref(call_of(rec)), length, C.byref(a), C.byref(b))
            want = R.trim_range(rec, length)
            assert (a.value, b.value) == want, (rec, length)
            lo = rec["front_end"] if rec["best"] >= 0 and rec["ends"] & 1 else 0
            cut = rec["rear_end"] if rec["best"] >= 0 and rec["ends"] & 2 else 0
            assert bool(crossed) == (lo + cut > 0 and lo + cut >= length), (rec, length)      # (an empty call that loses nothing is no crossing)
    assert R.tags(_records()[0], names) == "BC:Z:bc02\tbd:i:2\tbn:i:9\tbp:B:s,5,4"
    assert R.tags(_records()[3], names) == "BC:Z:unclassified\tbd:i:7\tbn:i:7\tbp:B:s,11,3"
    assert R.trim_range(_records()[0], 11) == (5, 11) and R.trim_range(_records()[1], 11) == (3, 7) and R.trim_range(_records()[2], 11) == (0, 9)
    assert R.trim_range(_records()[4], 11) == (0, 11) and R.trim_range(_records()[5], 11) == (0, 0) and R.trim_range(_records()[6], 11) == (0, 0)
    assert not L.flappie_barcode_tags(C.byref(call_of(dict(_records()[0], best=3))), kit)       # beyond the kit
    L.flappie_barcode_kit_free(kit)


def _write(L, libc, path, fn, *a):
    fp = _cfile(libc, path)
    fn(*a[:1], fp, *a[1:])
    libc.fclose(fp)
    return path.read_text()


def test_records_equal_the_restatement(L, tmp_path):
    libc = C.CDLL(None)
    err = C.create_string_buffer(256)
    kit = L.flappie_barcode_kit_parse(KIT_TEXT.encode(), err, 256)
    names = ["bc01", "bc02", "bc03"]
    call, qual = "ZACGTZCCAZT", "!#%+5?IJ+,-"
    ml = [201, 0, 3, 0, 0, 255, 0, 128, 0, 17, 0]
    mv = np.zeros(40, np.uint8)
    mv[[3, 4, 9, 10, 15, 20, 21, 30, 31, 35, 38]] = 1
    med, mad = np.float32(93.25), np.float32(12.625001)
    for rec in _records()[:8]:
        bc, tags = call_of(rec), R.tags(rec, names)
        for reverse in (False, True):
            for with_ml in (False, True):
                for with_mv in (False, True):
                    c, q, m = VR.oriented(call, qual, ml if with_ml else None, reverse)
                    res = BasecallInfo(score=np.float32(-123.5), basecall=c.encode(), quality=q.encode(), basecall_length=len(c), nblock=40)
                    res.rt = RawTable(uuid=b"u-1", n=4000, start=200, end=3990, raw=None)
                    mla = np.array(m, dtype=np.uint8) if with_ml else None
                    mlp = mla.ctypes.data_as(U8P) if with_ml else None
                    mvp = mv.ctypes.data_as(U8P) if with_mv else None
                    for fmt in range(3):
                        default = _write(L, libc, tmp_path / "d", L.fprintf_format, fmt, b"u-1", b"a.fast5", True, b"PRE_", res).split("\n")
                        got = _write(L, libc, tmp_path / "t", L.fprintf_barcode_record, fmt, b"u-1", b"a.fast5", True, b"PRE_", res, mlp, mvp, 5, med, mad, False,
                                     C.byref(bc), kit, False, reverse)
                        hdr, name = default[0][1:], default[0].split("\t")[0]
                        if with_mv:             # the move tags' record (MM / ML inside when given), the barcode tags behind its first line
                            args = (c, q, mv, 5, 4000, 200, med, mad, False, m)
                            base = VR.tagged_fasta(hdr, *args) if fmt == 0 else VR.tagged_fastq(hdr, *args) if fmt == 1 else VR.tagged_sam(name, *args)
                        elif with_ml:
                            base = MR.tagged_fasta(hdr, c, m) if fmt == 0 else MR.tagged_fastq(hdr, c, q, m) if fmt == 1 else MR.tagged_sam(name, c, q, m)
                        else:
                            base = ("\n".join(default[:2]) + "\n" if fmt == 0 else "\n".join(default[:4]) + "\n" if fmt == 1 else default[0] + "\n")
                        first, rest = base.split("\n", 1)
                        assert got == first + "\t" + tags + "\n" + rest, (rec, reverse, with_ml, with_mv, fmt)
                        assert got.split("\n")[0].split("\t")[-4:] == tags.split("\t")
                        if fmt == 2:
                            assert got.count("\n") == 1 and len(got.split("\t")) == 11 + 4 + (2 if with_ml else 0) + (7 if with_mv else 0)
            # the trim: SEQ and QUAL only, cut in signal order (a reversed record loses the same bases at its other ends)
            c, q, _ = VR.oriented(call, qual, None, reverse)
            res = BasecallInfo(score=np.float32(-123.5), basecall=c.encode(), quality=q.encode(), basecall_length=len(c), nblock=40)
            res.rt = RawTable(uuid=b"u-1", n=4000, start=200, end=3990, raw=None)
            a, b = R.trim_range(rec, len(call))
            seq, qs = call[a:b], qual[a:b]
            if reverse:
                seq, qs = seq[::-1], qs[::-1]
            for fmt in range(3):
                default = _write(L, libc, tmp_path / "d", L.fprintf_format, fmt, b"u-1", b"a.fast5", True, b"PRE_", res).split("\n")
                got = _write(L, libc, tmp_path / "t", L.fprintf_barcode_record, fmt, b"u-1", b"a.fast5", True, b"PRE_", res, None, None, 5, med, mad, False,
                             C.byref(bc), kit, True, reverse)
                if fmt == 0:
                    want = default[0] + "\t" + tags + "\n" + seq + "\n"
                elif fmt == 1:
                    want = default[0] + "\t" + tags + "\n" + seq + "\n+\n" + qs + "\n"
                else:
                    want = "\t".join(default[0].split("\t")[:9] + [seq, qs, tags]) + "\n"
                assert got == want, (rec, reverse, fmt)
    L.flappie_barcode_kit_free(kit)


@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    kit = tmp_path / "kit.fa"
    kit.write_text(KIT_TEXT)
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--barcodes", "--barcode-window", "--barcode-max-dist", "--barcode-min-sep", "--barcode-both-ends", "--trim-barcodes"):
        assert opt in r.stdout, opt
    assert "signal order" in r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--barcodes" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    assert "--barcodes" in refused(RUNNIE, "--barcodes", str(kit))
    for other in (["--emit-moves"], ["--modbase-tags", "--model", "r941_5mC"], ["--trace", str(tmp_path / "t.hdf5")]):
        assert "--trim-barcodes" in refused(FLAPPIE, "--barcodes", str(kit), "--trim-barcodes", *other)
    assert not (tmp_path / "t.hdf5").exists()
    for alone in (["--trim-barcodes"], ["--barcode-window", "100"], ["--barcode-max-dist", "3"], ["--barcode-min-sep", "2"], ["--barcode-both-ends"]):
        assert "--barcodes" in refused(FLAPPIE, *alone)
    for bad in (["--barcode-window", "0"], ["--barcode-window", "257"], ["--barcode-max-dist", "-1"], ["--barcode-max-dist", "256"], ["--barcode-min-sep", "256"]):
        refused(FLAPPIE, "--barcodes", str(kit), *bad)
    # a bad kit file: refused before any fast5 file or the GPU is touched
    texts = {"empty": "", "too many": "".join(">b%d\nACGT\n" % k for k in range(129)), "too long": ">a\n" + "A" * 129 + "\n", "N": ">a\nACGN\n", "duplicate": ">a\nAC\n>a\nGT\n"}
    for what, text in texts.items():
        bad = tmp_path / "bad.fa"
        bad.write_text(text)
        assert "bad.fa" in refused(FLAPPIE, "--barcodes", str(bad)), what
    assert "missing.fa" in refused(FLAPPIE, "--barcodes", str(tmp_path / "missing.fa"))
