"""flappie --remap-from-map without a GPU: the restatement (mapremap_ref.py) against remap_ref.py's own coding; the sizing rule against the library; header, binding
and library agree on the three new calls; the construction the GPU tests build their batches on meets what they ask of it; the line of map.tsv in the mode
(flappie_remap.c of libflappie_host.so) against the restatement; the command line's refusals.  Everything is integer- or byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import map_ref as R
import mapremap_ref as MR
import maptruth_ref as MT
import remap_ref as RR
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5

NEW_CALLS = ("ffhip_batch_set_remap_from_map", "ffhip_op_map_remap_code", "ffhip_debug_remap_from_map_form")


# ------------------------------------------------------------------------------------ the restatement
def test_the_restated_coding_is_remap_refs():
    """parity inside the run of equal letters is the recurrence of "remap": random stretches of both alphabets, with long runs, and every stretch of 1 .. 7 letters
    over two letters"""
    rng = np.random.default_rng(1)
    n = 0
    for nbase in (4, 5):
        for _ in range(200):
            m = int(rng.integers(1, 300))
            s = rng.integers(0, 4, m).astype(np.uint8)
            for _ in range(int(rng.integers(0, 4))):          # planted runs, up to three passes of a wave
                a = int(rng.integers(0, m))
                s[a:a + int(rng.integers(2, 200))] = s[a]
            assert MR.run_parity_code(s, nbase) == RR.flipflop_code(s, nbase)
            assert np.array_equal(MR.entries(s, nbase), MR.entries_by_remap_ref(s, nbase))
            n += 1
        for m in range(1, 8):
            for v in range(1 << m):
                s = [(v >> i) & 1 for i in range(m)]
                assert MR.run_parity_code(s, nbase) == RR.flipflop_code(s, nbase)
    assert n == 400
    e = MR.entries([2, 2, 2, 0], 4)                           # G G G A: flip, flop, flip, then A's flip
    assert [int(x) for x in e] == [RR.trans_lookup(2, 2, 4), RR.trans_lookup(6, 6, 4) | RR.trans_lookup(2, 6, 4) << 8, RR.trans_lookup(2, 2, 4) | RR.trans_lookup(6, 2, 4) << 8,
                                   RR.trans_lookup(0, 0, 4) | RR.trans_lookup(2, 0, 4) << 8]
    assert int(e.max()) < 1 << 16 and all((int(x) & 255) < 40 and (int(x) >> 8) < 40 for x in e)


def test_the_rule_on_small_records():
    records = ["ACGTTTGACCA", "GGGA"]
    ys = R.searches(records)
    for q, y in enumerate(ys):
        for a in range(len(y)):
            for b in range(a + 1, len(y) + 1):
                mp = {"status": 1, "q": q, "tstart": a, "tend": b}
                m = b - a
                for N in (m - 2, m - 1, m, m + 3):
                    if N < 1:
                        continue
                    status, L, ent = MR.remap_from_map(records, mp, N, 4)
                    if m <= N + 1:
                        assert (status, L) == (1, m) and np.array_equal(ent, MR.entries(MT.codes(y[a:b]), 4))
                    else:
                        assert (status, L, ent) == (2, m, None)
                for st in (0, 2, 3):
                    assert MR.remap_from_map(records, dict(mp, status=st), 100, 4) == (0, 0, None)
    assert np.array_equal(MR.sequence_of(records, {"status": 1, "q": 3, "tstart": 0, "tend": 4}), MT.codes("TCCC")) and MR.sequence_of(records, {"status": 2}) is None


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    assert lib.ffhip_batch_set_remap_from_map.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.ffhip_op_map_remap_code.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    assert lib.ffhip_debug_remap_from_map_form.argtypes == [C.c_int, C.c_int]
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("int ffhip_batch_set_remap_from_map(ffhip_batch *b, int on, int band);",
                  "int ffhip_op_map_remap_code(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, int nbase, int room, uint16_t *out /* end - start */, int *status, size_t *L);",
                  "int ffhip_debug_remap_from_map_form(int nblock, int band);"):
        assert proto in header, proto
    assert callable(B.Batch.set_remap_from_map) and callable(B.op_map_remap_code) and callable(B.remap_from_map_form)
    # the sizing rule needs no device: a read of N blocks takes the form of N + 1 positions
    for band in (0, 1, 31, 32, 127, 128, 511, 512, 2048, 2303):
        for N in (1, 2, 62, 63, 64, 254, 255, 256, 257, 1022, 1023, 1024, 4606, 4607, 4608, 20000, (1 << 30) - 1):
            want = int(lib.ffhip_debug_remap_form(N + 1, band))
            assert B.remap_from_map_form(N, band) == want and want >= 0, (N, band)
            if N + 1 <= 1 << 30:                              # ... which is never smaller than the form of any L the read can be mapped to
                assert all(int(lib.ffhip_debug_remap_form(L, band)) <= want for L in (1, 2, (N + 1) // 2, N, N + 1)), (N, band)
    assert [B.remap_from_map_form(N, 2048) for N in (63, 64, 255, 256, 1023, 1024)] == [0, 1, 1, 2, 2, 3]
    assert B.remap_from_map_form(0, 10) == -1 and B.remap_from_map_form(-5, 10) == -1 and B.remap_from_map_form(10, -1) == -1 and B.remap_from_map_form(1 << 30, 10) == -1
    H = C.CDLL(HOSTLIB)
    assert "flappie_remap_write_placed_line" in _declared_functions("flappie_remap.h") and hasattr(H, "flappie_remap_write_placed_line")


# ------------------------------------------------------------------------------------ the construction of the GPU tests
def test_the_reference_of_a_batchs_calls_meets_what_the_gpu_tests_ask():
    """test_mapremap_gpu.py builds its references from the batch's own calls (reference_of) and asserts that three reads in four are mapped and remapped, two or
    more on either strand, one or more not mapped; and that two or more reads take another kernel form in the one run than in the second of two.  Here, on random
    calls of the lengths its models give (about 0.9 bases a block at 5 samples a block, about 0.4 at 2), before any GPU time is spent."""
    from flappie_amd import binding as B
    lib = B.lib()
    for density, stride, rows, straddle in ((0.9, 5, 1300, (1285, 1331)), (0.42, 2, 2060, (1100, 1201))):
        rng = np.random.default_rng(int(100 * density))
        for shape in ("rows", "ragged"):
            samples = [rows] * 16 if shape == "rows" else [int(x) for x in rng.integers(*straddle, 4)] + [int(x) for x in rng.integers(1100, 2601, 15)]
            blocks = [(n + stride - 1) // stride for n in samples]
            calls = [MR.rand_seq(rng, int(density * N)) for N in blocks]
            recs = MR.reference_of(np.random.default_rng(23), calls)
            maps = [R.record(recs, c) for c in calls]
            remaps = []
            differ = 0
            for mp, N in zip(maps, blocks):
                status, L, _ = MR.remap_from_map(recs, mp, N, 4)
                remaps.append({"status": status, "L": L})
                differ += status == 1 and B.remap_from_map_form(N, 2048) != int(lib.ffhip_debug_remap_form(L, 2048))
            seen = MR.tally(maps, remaps)
            assert MR.tally_ok(seen), (density, shape, seen)
            assert differ >= 2, (density, shape, differ)
            assert all(mp["tend"] - mp["tstart"] <= N + 1 for mp, N in zip(maps, blocks) if mp["status"] == 1)
    assert not MR.tally_ok({"reads": 16, "mapped": 11, "plus": 6, "minus": 5, "not mapped": 5}) and not MR.tally_ok({"reads": 16, "mapped": 16, "plus": 8, "minus": 8, "not mapped": 0})
    assert not MR.tally_ok({"reads": 16, "mapped": 14, "plus": 13, "minus": 1, "not mapped": 2}) and MR.tally_ok({"reads": 16, "mapped": 12, "plus": 2, "minus": 10, "not mapped": 4})


# ------------------------------------------------------------------------------------ the host side
def test_the_line_of_map_tsv(tmp_path):
    L = C.CDLL(HOSTLIB)
    U8P = C.POINTER(C.c_uint8)
    L.flappie_remap_write_placed_line.restype = C.c_long
    L.flappie_remap_write_placed_line.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, U8P, C.c_float, C.c_char_p, C.c_char, C.c_long, C.c_long]
    L.flappie_remap_write_line.restype = C.c_long
    L.flappie_remap_write_line.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, U8P, C.c_float]
    names, lens = ["chrA", "plasmid.1"], [300, 40]
    rng = np.random.default_rng(7)
    libc = C.CDLL(None)
    out, plain = tmp_path / "map.tsv", tmp_path / "plain.tsv"
    fh, fp = _cfile(libc, out), _cfile(libc, plain)
    want, keep = [], []
    for i, (q, a, b) in enumerate(((0, 10, 30), (1, 10, 30), (2, 0, 40), (3, 5, 6), (1, 0, 300))):
        m = b - a
        N = m + int(rng.integers(0, 9)) if i != 4 else 100      # the last one: more bases than blocks + 1
        mp = {"status": 1, "q": q, "tstart": a, "tend": b}
        k, o, fa, fb = R.forward(q, a, b, lens)
        if m <= N + 1:
            rm = np.zeros(N, np.uint8)
            rm[rng.choice(N, m - 1, replace=False)] = 1
            rec = {"status": 1, "L": m, "nblock": N, "score": np.float32(-rng.random() * 100), "rm": rm}
        else:
            rm = np.zeros(1, np.uint8)
            rec = {"status": 2, "L": m, "nblock": N, "score": np.float32(0), "rm": None}
        keep.append(rm)
        name = ("read-%d" % i).encode()
        dev = L.flappie_remap_write_placed_line(fh, name, rec["status"], N, 5, 17 * i, m, 64, rm.ctypes.data_as(U8P), rec["score"], names[k].encode(), o.encode(), fa, fb)
        assert dev == (RR.starts_maxdev(rm, m)[1] if rec["status"] == 1 else 0)
        assert L.flappie_remap_write_line(fp, name, rec["status"], N, 5, 17 * i, m, 64, rm.ctypes.data_as(U8P), rec["score"]) == dev
        want.append(MR.map_tsv_line(name.decode(), rec, 5, 17 * i, 64, mp, names, lens))
    rm = np.array([0, 1, 0], np.uint8)
    for bad in ((b"x", 1, 3, 5, 0, 3, 8, rm.ctypes.data_as(U8P), 0.0, b"chrA", b"+", 0, 3),          # moves that do not fit L: nothing written
                (b"x", 1, 3, 5, 0, 2, 8, rm.ctypes.data_as(U8P), 0.0, b"chrA", b"*", 0, 2),          # no strand
                (b"x", 1, 3, 5, 0, 2, 8, rm.ctypes.data_as(U8P), 0.0, None, b"+", 0, 2),
                (b"x", 1, 3, 5, 0, 2, 8, rm.ctypes.data_as(U8P), 0.0, b"chrA", b"-", 5, 3)):
        assert L.flappie_remap_write_placed_line(fh, *bad) == -1
    libc.fclose(fh)
    libc.fclose(fp)
    text = out.read_text()
    assert text == "".join(want)
    rows, base = [ln.split("\t") for ln in text.splitlines()], [ln.split("\t") for ln in plain.read_text().splitlines()]
    assert all(len(f) == 14 and f[:10] == g for f, g in zip(rows, base)) and len(rows) == len(base) == 5      # the columns of --remap-out, then the place
    assert [f[10:] for f in rows] == [["chrA", "+", "10", "30"], ["chrA", "-", "270", "290"], ["plasmid.1", "+", "0", "40"], ["plasmid.1", "-", "34", "35"], ["chrA", "-", "0", "300"]]
    assert rows[4][1] == "2" and rows[4][7:10] == ["*", "*", "*"] and rows[0][1] == "1" and rows[0][9].startswith("0,")


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    vars_ = tmp_path / "vars.tsv"
    vars_.write_text("a\t1\tC\tT\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--remap-from-map" in r.stdout, r.stdout
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--remap-from-map" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr

    def accepted(*args):
        """the options pass; the run then finds no read (and no GPU is asked for before it has one)"""
        r = subprocess.run([FLAPPIE] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert not re.search(r"goes with|go together|does not go with|must be a whole number|flappie's", r.stderr), (args, r.stderr)
        return r

    hits, mp, ev, acc = str(tmp_path / "hits.tsv"), str(tmp_path / "map.tsv"), str(tmp_path / "events.tsv"), str(tmp_path / "acc.tsv")
    mapped = ["--map", str(fa), "--map-out", hits]
    mode = mapped + ["--remap-from-map", "--remap-out", mp]
    assert "--remap-from-map goes with --map" in refused(FLAPPIE, "--remap-from-map", "--remap-out", mp)
    assert "--remap-from-map and --remap-out go together" in refused(FLAPPIE, *mapped, "--remap-from-map")
    assert "--remap-from-map does not go with --remap:" in refused(FLAPPIE, *mode, "--remap", str(fa))
    assert "--remap-from-map does not go with --remap-mods" in refused(FLAPPIE, "--model", "r941_5mC", *mode, "--remap-mods", str(tmp_path / "mods.tsv"))
    assert "--remap-from-map does not go with --remap-variants" in refused(FLAPPIE, *mode, "--remap-variants", str(vars_), "--remap-variants-out", str(tmp_path / "calls.tsv"))
    assert "--remap-from-map does not go with --remap-variants" in refused(FLAPPIE, *mode, "--remap-variants-context", "5")
    assert "must be a whole number" in refused(FLAPPIE, *mode, "--remap-band", "2304")
    assert "cannot be written" in refused(FLAPPIE, *mapped, "--remap-from-map", "--remap-out", str(tmp_path / "no" / "map.tsv"))
    assert "--remap-events" in refused(FLAPPIE, *mode, "--remap-events", str(tmp_path / "no" / "events.tsv"))
    # what stands as it stood without the option
    assert "--remap and --remap-out go together" in refused(FLAPPIE, *mapped, "--remap-out", mp)
    assert "--remap-band goes with --remap" in refused(FLAPPIE, *mapped, "--remap-band", "100")
    assert "--remap-events goes with --remap" in refused(FLAPPIE, *mapped, "--remap-events", ev)
    # what goes with it
    accepted(*mode)
    accepted(*mode, "--remap-band", "0", "--remap-events", ev)
    accepted(*mode, "--remap-band", "2303", "--truth-from-map", "--truth-out", acc)
    assert "--remap-from-map is flappie's" in refused(RUNNIE, "--remap-from-map")
