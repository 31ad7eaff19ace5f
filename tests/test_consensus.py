"""flappie --map-consensus without a GPU: the restatement (consensus_ref.py: the header's walk in signal order) held to an independent forward-strand walk of the
read's SAM line, which takes an insertion's letters left to right -- what catches a wrong offset on the - strand; its planes 0 .. 4 held to the pileup's
restatement, strands summed; the call's rule on hostile counts, each cell written down by hand; the host side (flappie_consensus.c of libflappie_host.so: the FASTA
file, the table of changes and the summary) against the restatement on hand-made cells; header, binding and library agree on the new calls; every refusal the
command line makes before it opens a device.  Everything is integer- or byte-exact."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_ref as CR
import map_ref as R
import pileup_ref as PU
from test_cabi_and_model import _declared_functions
from test_cli import FLAPPIE, HOSTLIB, RUNNIE, _cfile, needs_hdf5
from test_map import Ref
from test_pileup import random_alignments

NEW_CALLS = ("ffhip_consensus_create", "ffhip_consensus_free", "ffhip_consensus_reset", "ffhip_consensus_positions", "ffhip_consensus_download",
             "ffhip_consensus_call", "ffhip_batch_set_consensus", "ffhip_op_consensus")


def long_run_alignments(rng, lens, count):
    """alignments whose insertion runs are long (up to 12 letters) and frequent, on both strands: where the forward offset and the eighth column matter"""
    out = []
    for it in range(count):
        k = int(rng.integers(0, len(lens)))
        Mk = lens[k]
        a = int(rng.integers(0, Mk))
        b = int(rng.integers(a + 1, Mk + 1))
        ops = [2] * int(rng.integers(0, 3) if it % 3 == 0 else 0)
        for j in range(b - a):
            ops.append((0, 1, 3)[int(rng.choice(3, p=(0.7, 0.15, 0.15)))])
            if rng.random() < 0.3:
                ops += [2] * int(rng.integers(1, 13))
        if it % 4 == 1 and ops[-1] != 2:
            ops += [2, 2]
        n = sum(1 for x in ops if x != 3)
        out.append((2 * k + it % 2, a, b, "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n)), np.array(ops, np.uint8)))
    return out


# ------------------------------------------------------------------------------------ the two walks
def test_the_signal_order_walk_is_the_forward_strand_walk():
    rng = np.random.default_rng(23)
    lens = [1, 15, 16, 17, 33, 100]
    alns = random_alignments(rng, lens, 300) + long_run_alignments(rng, lens, 300)
    alns += [(0, 0, 1, "A", [0]), (1, 0, 1, "GT", [2, 3, 2]), (10, 0, 100, "ACGT", [2, 2] + [3] * 100 + [2, 2]), (11, 99, 100, "TZ", [2, 0]), (11, 0, 1, "ZT", [0, 2]),
             (3, 2, 4, "ACG", [0, 2, 0]), (2, 2, 4, "ACG", [0, 2, 0]), (9, 3, 5, "A" + "ACGTACGTAC" + "G", [0] + [2] * 10 + [1]), (8, 3, 5, "A" + "ACGTACGTAC" + "G", [0] + [2] * 10 + [1])]
    assert all(set(int(x) for x in a[4]) <= {0, 1, 2, 3} for a in alns)
    a, b = CR.Consensus(lens), CR.Consensus(lens)
    runs = {0: set(), 1: set()}
    for q, ts, te, call, ops in alns:
        a.add(q, ts, te, call, ops)
        b.forward_add(q, ts, te, call, ops)
        for m in re.finditer("2+", "".join(str(int(x)) for x in ops)):
            runs[q & 1].add(len(m.group(0)))
    assert all({1, 2, 3, 7, 8, 9, 12} <= runs[o] for o in (0, 1)), runs
    assert a.totals == b.totals and np.array_equal(a.counts, b.counts)
    t = a.totals
    assert t["reads"] == len(alns) and t["skipped"] == 0 and min(t[k] for k in ("bases", "del", "ins_bases", "long_ins", "edge_ins")) > 0 and t["reserved"] == 0
    assert int(a.counts[:4].sum()) == t["bases"] and int(a.counts[4].sum()) == t["del"] and int(a.counts[5:].sum()) == t["ins_bases"]
    assert all(int(a.counts[5 + 4 * d:9 + 4 * d].sum()) > 0 for d in range(CR.MINOR))
    # by hand: a read on the - strand of a record of 5 behind a record of 1, span [1, 3) of the reverse complement = forward [2, 4), walked from its right end.
    # A at forward 3 as T; then ZG inserted between forward 2 and 3: in the gap behind 2, turned: G -> C at offset 0, Z -> G at offset 1; then G at forward 2 as C
    p = CR.Consensus([1, 5])
    p.add(3, 1, 3, "AZGG", [0, 2, 2, 1])
    want = np.zeros((CR.PLANES, 6), np.uint32)
    want[3, 1 + 3] = want[1, 1 + 2] = want[5 + 0 + 1, 1 + 2] = want[5 + 4 + 2, 1 + 2] = 1
    assert np.array_equal(p.counts, want) and p.totals == dict(reads=1, skipped=0, bases=2, ins_bases=2, long_ins=0, edge_ins=0, reserved=0, **{"del": 0})
    # ... and the same letters on the + strand keep their order
    p = CR.Consensus([1, 5])
    p.add(2, 2, 4, "AZGG", [0, 2, 2, 1])
    want = np.zeros((CR.PLANES, 6), np.uint32)
    want[0, 1 + 2] = want[2, 1 + 3] = want[5 + 0 + 1, 1 + 2] = want[5 + 4 + 2, 1 + 2] = 1
    assert np.array_equal(p.counts, want)
    # a run of 10 on either strand: the first eight FORWARD letters are kept, two are long
    for q, kept in ((8, "ACGTACGT"), (9, R.revcomp("ACGTACGTAC")[:8])):
        p = CR.Consensus(lens)
        p.add(q, 3, 5, "A" + "ACGTACGTAC" + "G", [0] + [2] * 10 + [1])
        gap = p.off[4] + (3 if q == 8 else 33 - 1 - 3 - 1)
        assert p.totals["ins_bases"] == 8 and p.totals["long_ins"] == 2
        assert [int(np.argmax(p.counts[5 + 4 * d:9 + 4 * d, gap])) for d in range(8)] == ["ACGT".index(c) for c in kept]
        assert int(p.counts[5:].sum()) == int(p.counts[5:, gap].sum()) == 8


def test_planes_0_to_4_are_the_pileup_with_its_strands_summed():
    rng = np.random.default_rng(29)
    lens = [7, 64, 130]
    for min_id in (0, 800):
        c, p = CR.Consensus(lens, min_id), PU.Pileup(lens, min_id)
        for q, ts, te, call, ops in random_alignments(rng, lens, 200):
            c.add(q, ts, te, call, ops)
            p.add(q, ts, te, call, ops)
        assert np.array_equal(c.counts[:5], p.counts[0, :5] + p.counts[1, :5])
        assert c.totals["reads"] == p.totals["reads"] > 0 and c.totals["skipped"] == p.totals["skipped"] and (min_id == 0 or c.totals["skipped"] > 0)
        assert c.totals["bases"] == p.totals["match"] + p.totals["mismatch"] and c.totals["del"] == p.totals["del"] and c.totals["edge_ins"] == p.totals["edge_ins"]
        assert c.totals["ins_bases"] + c.totals["long_ins"] == p.totals["ins"]
        # the gaps with an inserted letter at forward offset 0 are the gaps the pileup's column `ins` is not 0 at: every inner run has such a letter
        assert np.array_equal(c.counts[5:9].sum(axis=0) > 0, (p.counts[0, 5] + p.counts[1, 5]) > 0)
    # a read of a batch: both statuses 1, or nothing at all
    c = CR.Consensus([10], 900)
    mp = {"status": 1, "q": 0, "tstart": 0, "tend": 3}
    tr = {"status": 1, "n": 3, "m": 3, "ops": np.array([0, 1, 0], np.uint8)}
    c.add_read(mp, tr, "ACG")
    c.add_read(dict(mp, status=2), tr, "ACG")
    c.add_read(mp, dict(tr, status=0), "ACG")
    assert c.totals["skipped"] == 1 and c.totals["reads"] == 0 and int(c.counts.sum()) == 0


# ------------------------------------------------------------------------------------ the call on hostile counts
HOSTILE_REF = "ACGTTGCA" * 5
HOSTILE_MIN_DEPTH = 4


def columns_alignment(k, Mk, ref, a, cols, strand):
    """an alignment from forward columns: cols[x] = (letter or '-', inserted letters behind it) at forward position a + x; as the operator takes it, in signal order"""
    ops, seq = [], []
    for x, (c, ins) in enumerate(cols):
        ops.append(3 if c == "-" else 0 if c == ref[a + x] else 1)
        seq.append("" if c == "-" else c)
        ops += [2] * len(ins)
        seq.append(ins)
    seq, b = "".join(seq), a + len(cols)
    if strand == "+":
        return 2 * k, a, b, seq, np.array(ops, np.uint8)
    return 2 * k + 1, Mk - b, Mk - a, R.revcomp(seq), np.array(ops[::-1], np.uint8)


def hostile_alignments(k=0, Mk=len(HOSTILE_REF)):
    """five reads on alternating strands over HOSTILE_REF as record k, which put every edge of the call's rule somewhere (test_the_call_on_hostile_counts says where)"""
    ref = HOSTILE_REF
    spans = [(0, 40), (0, 40), (0, 40), (0, 34), (22, 30)]
    over = [
        {5: ("G", ""), 9: ("T", ""), 12: ("-", ""), 14: ("-", ""), 17: ("-", "GG"), 20: ("T", "A"), 24: ("A", "C"), 26: ("G", "T"), 27: ("T", "T"), 30: ("C", "ACGTACGTAC"), 36: ("T", "A")},
        {5: ("G", ""), 9: ("T", ""), 12: ("-", ""), 14: ("-", ""), 17: ("-", "GG"), 20: ("T", "A"), 24: ("A", "C"), 26: ("G", "T"), 27: ("T", "T"), 30: ("C", "ACGTACGTAC"), 36: ("T", "A")},
        {5: ("A", ""), 9: ("G", ""), 14: ("A", ""), 17: ("C", "GG"), 24: ("A", "C"), 27: ("T", "G"), 30: ("C", "ACGTACGTAC"), 36: ("T", "A")},
        {5: ("A", ""), 9: ("G", ""), 14: ("A", ""), 17: ("A", ""), 27: ("T", "G")},
        {},
    ]
    out = []
    for r, ((a, b), ov) in enumerate(zip(spans, over)):
        cols = [ov.get(x, (ref[x], "")) for x in range(a, b)]
        out.append(columns_alignment(k, Mk, ref, a, cols, "+-"[r % 2]))
    return out


HOSTILE_WANT = {       # position: (letters, what, depth)
    2: ("G", CR.SAME, 4),                   # depth exactly min_depth
    33: ("C", CR.SAME, 4), 34: ("g", CR.LOW, 3),      # ... and one below
    5: ("G", CR.SAME, 4),                   # A 2, G 2: the reference's G is among the tied
    9: ("G", CR.SUB, 4),                    # G 2, T 2 at a C: the first in A C G T
    12: ("T", CR.SAME, 4),                  # del 2, T 2 at a T
    14: ("A", CR.SUB, 4),                   # A 2, del 2 at a C: A stands ahead of del
    17: ("GG", CR.DEL | CR.INS, 4),         # del 2, C 1, A 1; GG behind it from 3 of 4: a deletion with an insertion behind it
    20: ("T", CR.SAME, 4),                  # an A behind it from 2 of 4: 2 t == depth, not written
    24: ("AC", CR.SAME | CR.INS, 5),        # a C behind it from 3 of 5: 2 t == depth + 1, written
    26: ("G", CR.SAME, 5),                  # 2 of 5
    27: ("TG", CR.SAME | CR.INS, 5),        # T 2, G 2 behind it: a column's tie goes to the first in A C G T
    30: ("CACGTACGT", CR.SAME | CR.INS, 4),  # ten letters from 3 of 4: eight columns all pass, n = 9, two letters a read are long
    36: ("t", CR.LOW, 3),                   # below the depth no insertion is looked at
}


def test_the_call_on_hostile_counts():
    c, f = CR.Consensus([len(HOSTILE_REF)]), CR.Consensus([len(HOSTILE_REF)])
    for aln in hostile_alignments():
        c.add(*aln)
        f.forward_add(*aln)
    assert np.array_equal(c.counts, f.counts) and c.totals == f.totals
    assert c.totals["long_ins"] == 6 and c.totals["edge_ins"] == 0 and c.totals["reads"] == 5
    g = 20
    assert int(c.counts[5:9, g].sum()) * 2 == int(c.depth()[g]) and int(c.counts[5:9, 24].sum()) * 2 == int(c.depth()[24]) + 1
    assert [int(x) for x in c.counts[:5, 5]] == [2, 0, 2, 0, 0] and [int(x) for x in c.counts[:5, 14]] == [2, 0, 0, 0, 2]
    cells = CR.call(c.counts, CR.ref_codes([HOSTILE_REF]), HOSTILE_MIN_DEPTH)
    for pos, (s, what, depth) in HOSTILE_WANT.items():
        got = (CR.letters(cells[pos]), int(cells[pos]["what"]), int(cells[pos]["depth"]))
        assert got == (s, what, depth) and int(cells[pos]["n"]) == len(s), (pos, got)
    plain = [x for x in range(40) if x not in HOSTILE_WANT]
    assert all(CR.letters(cells[x]) == (HOSTILE_REF[x] if x < 34 else HOSTILE_REF[x].lower()) for x in plain)
    # the depth decides alone: one more and one fewer
    assert CR.letters(CR.call(c.counts, CR.ref_codes([HOSTILE_REF]), 3)[34]) == "G" and CR.letters(CR.call(c.counts, CR.ref_codes([HOSTILE_REF]), 5)[2]) == "g"
    # a depth beyond 2^32 - 1 is saturated in the cell and still compared in full
    big = np.zeros((CR.PLANES, 1), np.uint32)
    big[0, 0] = big[1, 0] = big[5, 0] = CR.MASK
    cell = CR.call(big, [1], 1)[0]
    assert int(cell["depth"]) == CR.MASK and CR.letters(cell) == "C" and int(cell["what"]) == CR.SAME       # 2 t == depth: not written
    with pytest.raises(AssertionError):
        CR.call(big, [1], 0)


# ------------------------------------------------------------------------------------ the inputs of the end-to-end test restore the original
MARGIN = 300                                                 # what the end-to-end test leaves out at either end of a read's stretch
SHORTEST = 2 * MARGIN + 170                                  # the shortest call that holds the three planted differences inside the margins


def planted_reference(rng, calls, nrec=3):
    """The reference of the end-to-end test (tests/test_consensus_gpu.py): the calls themselves on alternating strands behind random flanks, in nrec records, and in
    every call's stretch -- at least MARGIN + 20 from its ends and 60 apart -- one substituted base, one base left out and one pair put in.  Returns (records,
    places), places[i] = (record, forward start, forward end, strand, y): y the call as the forward strand reads it, what a consensus has to give back."""
    parts, places = [[] for _ in range(nrec)], []
    for i, c in enumerate(calls):
        x = c.replace("Z", "C")
        y = x if i % 2 == 0 else R.revcomp(x)
        L = len(y)
        assert L >= SHORTEST, (i, L)
        p1 = MARGIN + 20 + int(rng.integers(0, L - SHORTEST + 1))
        p2, p3 = p1 + 60, p1 + 120
        other = "ACGT"[("ACGT".index(y[p1]) + 1 + int(rng.integers(0, 3))) % 4]
        stretch = y[:p1] + other + y[p1 + 1:p2] + y[p2 + 1:p3] + R.random_seq(rng, 2) + y[p3:]
        k = i % nrec
        flank = R.random_seq(rng, 200 + 31 * (i % 4))
        start = sum(len(x) for x in parts[k]) + len(flank)
        parts[k] += [flank, stretch]
        places.append((k, start, start + len(stretch), "+-"[i % 2], y))
    return ["".join(x) + R.random_seq(rng, 150) for x in parts], places


def restored(cells, off, places):
    """per read: (the consensus over its stretch without the margins, the call there)"""
    return [("".join(CR.letters(c) for c in cells[off[k] + a + MARGIN:off[k] + b - MARGIN]), y[MARGIN:len(y) - MARGIN]) for k, a, b, strand, y in places]


def test_the_end_to_end_inputs_restore_the_calls():
    """map_ref places every call on its stretch, truth_ref aligns it (the command line's default band, 512), three copies of every alignment go into the restatement,
    and the consensus at depth 3 over each stretch without MARGIN at either end is the call itself: the margin is enough for the anchors."""
    import truth_ref as T
    rng = np.random.default_rng(43)
    calls = [R.random_seq(rng, n) for n in (SHORTEST, 801, 1203, 1650)]
    calls[1] = calls[1][:400] + "Z" + calls[1][401:]
    records, places = planted_reference(np.random.default_rng(47), calls)
    lens = [len(r) for r in records]
    c = CR.Consensus(lens)
    ys = R.searches(records)
    for call, (k, a, b, strand, y) in zip(calls, places):
        mp = R.record(records, call)
        assert mp["status"] == 1 and R.forward(mp["q"], mp["tstart"], mp["tend"], lens) == (k, strand, a, b), (mp, k, a, b)
        tr = T.truth(call, ["ACGT".index(ch) for ch in ys[mp["q"]][mp["tstart"]:mp["tend"]]], 512)
        assert tr["status"] == 1 and (tr["n_mismatch"], tr["n_ins"], tr["n_del"]) == (1, 1, 2), tr
        for _ in range(3):
            c.add_read(mp, tr, call)
    cells = CR.call(c.counts, CR.ref_codes(records), 3)
    for got, want in restored(cells, c.off, places):
        assert got == want and len(want) >= 170
    tot = CR.stderr_lines(c.totals, cells)
    assert (tot["reads"], tot["sub"], tot["del"], tot["ins"]) == (12, 4, 8, 4) and tot["called"] == sum(b - a for k, a, b, s, y in places)
    # the flanks are below the depth: the reference's own letters in lower case
    assert CR.fasta(["a", "b", "c"], lens, cells).split("\n")[1][:70] == records[0][:70].lower()


# ------------------------------------------------------------------------------------ header, binding and library
def test_header_binding_and_library_agree_on_the_new_calls():
    from flappie_amd import binding as B
    declared = _declared_functions("ffhip.h")
    assert all(n in declared for n in NEW_CALLS), declared
    L = C.CDLL(B.library_path())
    assert all(hasattr(L, n) for n in NEW_CALLS)
    lib = B.lib()
    vp = C.c_void_p
    assert lib.ffhip_consensus_create.argtypes == [vp, vp, C.c_int] and lib.ffhip_consensus_create.restype == vp
    assert lib.ffhip_consensus_positions.restype == C.c_size_t and lib.ffhip_consensus_call.argtypes == [vp, C.c_int, vp]
    assert lib.ffhip_consensus_download.argtypes == [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    assert lib.ffhip_op_consensus.argtypes == [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    header = open(os.path.join(os.path.dirname(HOSTLIB), "..", "include", "ffhip.h")).read()
    for proto in ("ffhip_consensus *ffhip_consensus_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity);",
                  "void ffhip_consensus_free(ffhip_consensus *c);",
                  "int ffhip_consensus_reset(ffhip_consensus *c);",
                  "size_t ffhip_consensus_positions(const ffhip_consensus *c);",
                  "int ffhip_consensus_download(ffhip_consensus *c, uint32_t *counts /* [37][P] */, ffhip_consensus_totals *totals);",
                  "int ffhip_consensus_call(ffhip_consensus *c, int min_depth, ffhip_consensus_cell *cells /* [P] */);",
                  "int ffhip_batch_set_consensus(ffhip_batch *b, ffhip_consensus *c);",
                  "int ffhip_op_consensus(ffhip_engine *eng, ffhip_consensus *c, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops);",
                  "typedef struct { uint8_t n, what; char s[10]; uint32_t depth; } ffhip_consensus_cell;",
                  "#define FFHIP_CONSENSUS_PLANES 37", "#define FFHIP_CONSENSUS_MINOR 8"):
        assert proto in header, proto
    m = re.search(r"#define FFHIP_RUN_CONSENSUS\s+\(1u << (\d+)\)", header)
    assert m and int(m.group(1)) == 25 and (1 << 25) == B.RUN_CONSENSUS == 2 * B.RUN_MOD_PILEUP      # the next free bit
    shifted = [1 << int(v) for v in re.findall(r"#define FFHIP_RUN_[A-Z_0-9]+\s+\(1u << (\d+)\)", header)]
    assert shifted.count(B.RUN_CONSENSUS) == 1 and max(shifted) == B.RUN_CONSENSUS
    assert B.CONSENSUS_TOTALS == CR.TOTALS and len(B.CONSENSUS_TOTALS) == 8 and B.CONSENSUS_PLANES == CR.PLANES == 37 and B.CONSENSUS_MINOR == CR.MINOR == 8
    assert B.CONSENSUS_CELL == CR.CELL and CR.CELL.itemsize == 16
    assert (B.CONSENSUS_LOW, B.CONSENSUS_SAME, B.CONSENSUS_SUB, B.CONSENSUS_DEL, B.CONSENSUS_INS) == (CR.LOW, CR.SAME, CR.SUB, CR.DEL, CR.INS)
    assert re.search(r"FFHIP_CONSENSUS_LOW = 0, FFHIP_CONSENSUS_SAME = 1, FFHIP_CONSENSUS_SUB = 2, FFHIP_CONSENSUS_DEL = 3, FFHIP_CONSENSUS_INS = 4", header)
    assert callable(B.Consensus) and callable(B.Batch.set_consensus) and callable(B.op_consensus)
    assert all(callable(getattr(B.Consensus, n)) for n in ("download", "call", "reset", "close"))
    H = C.CDLL(HOSTLIB)
    assert sorted(_declared_functions("flappie_consensus.h")) == ["flappie_consensus_changes_write", "flappie_consensus_summary_print", "flappie_consensus_write"]
    assert all(hasattr(H, n) for n in _declared_functions("flappie_consensus.h"))


# ------------------------------------------------------------------------------------ the host side
class Totals(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in CR.TOTALS]


class Stats(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("positions", "called", "low_depth", "same", "sub", "del", "ins")]


def test_the_writers_are_the_restatements(tmp_path):
    L = C.CDLL(HOSTLIB)
    L.flappie_map_ref_parse.restype = C.POINTER(Ref)
    L.flappie_map_ref_parse.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.flappie_map_ref_free.argtypes = [C.POINTER(Ref)]
    L.flappie_map_ref_free.restype = None
    L.flappie_consensus_write.argtypes = [C.c_void_p, C.POINTER(Ref), C.c_void_p, C.POINTER(Stats)]
    L.flappie_consensus_changes_write.argtypes = [C.c_void_p, C.POINTER(Ref), C.c_void_p, C.POINTER(C.c_uint32)]
    L.flappie_consensus_summary_print.argtypes = [C.c_void_p, C.POINTER(Totals), C.POINTER(Stats)]
    L.flappie_consensus_summary_print.restype = None
    rng = np.random.default_rng(31)
    # the hostile record (a deletion with an insertion behind it, n = 9, lower case below the depth); a record whose every position is deleted: an EMPTY consensus;
    # a record in lower case of exactly 140 letters: two full lines and no third; one of 71 called positions: a line of 70 and a line of 1
    records = [HOSTILE_REF, "ACG", R.random_seq(rng, 140).lower(), R.random_seq(rng, 71)]
    names = ["hostile", "gone", "lower.2", "seventy-one"]
    text = ">hostile the first\n%s\n>gone\nACG\n>lower.2\tx\n%s\n>seventy-one\n%s\n" % (records[0], records[2], records[3])
    err = C.create_string_buffer(256)
    ref = L.flappie_map_ref_parse(text.encode(), err, 256)
    assert ref, err.value
    lens = [len(r) for r in records]
    c = CR.Consensus(lens)
    for aln in hostile_alignments():
        c.add(*aln)
    for _ in range(4):
        c.add(2, 0, 3, "", [3, 3, 3])
        c.add(6, 0, 71, records[3][:30] + "T" + records[3][30:40] + records[3][41:], [0] * 30 + [2] + [0] * 10 + [3] + [0] * 30)
    c.counts[0, c.off[3] + 5] = CR.MASK                       # a counter at its largest value: the depth saturates, the winner's count is written as it stands
    cells = CR.call(c.counts, CR.ref_codes(records), HOSTILE_MIN_DEPTH)
    assert all(int(cells[c.off[1] + x]["n"]) == 0 and int(cells[c.off[1] + x]["what"]) == CR.DEL for x in range(3))
    assert all(int(x["what"]) == CR.LOW for x in cells[c.off[2]:c.off[3]])
    libc = C.CDLL(None)
    fa, tsv, summ = tmp_path / "cons.fa", tmp_path / "changes.tsv", tmp_path / "summary.txt"
    raw = np.ascontiguousarray(cells)
    flat = np.ascontiguousarray(c.counts)
    st = Stats()
    f = _cfile(libc, fa)
    assert L.flappie_consensus_write(f, ref, raw.ctypes.data_as(C.c_void_p), C.byref(st)) == 0
    libc.fclose(f)
    assert L.flappie_consensus_write(None, ref, raw.ctypes.data_as(C.c_void_p), None) == -1
    got = fa.read_text()
    assert got == CR.fasta(names, lens, cells)
    lines = got.split("\n")
    # by hand: 9 C -> G, 14 C -> A, 17 deleted with GG behind it, AC at 24, TG at 27, C and eight inserted letters at 30, the last six below the depth
    assert lines[0] == ">hostile" and lines[1] == "ACGTTGCAA" + "G" + "GTTG" + "A" + "AA" + "GG" + "GTTGCA" + "AC" + "CG" + "TG" + "TG" + "CACGTACGT" + "AAC" + "gttgca"
    at = lines.index(">gone")
    assert lines[at + 1] == "" and lines[at + 2] == ">lower.2" and [len(x) for x in lines[at + 3:at + 6]] == [70, 70, len(">seventy-one")]
    assert lines[at + 3] + lines[at + 4] == records[2] and [len(x) for x in lines[at + 6:]] == [70, 1, 0]
    assert "".join(lines[at + 6:]) == records[3][:5] + "A" + records[3][6:30] + "T" + records[3][30:40] + records[3][41:]
    f = _cfile(libc, tsv)
    assert L.flappie_consensus_changes_write(f, ref, raw.ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    libc.fclose(f)
    assert L.flappie_consensus_changes_write(f, ref, raw.ctypes.data_as(C.c_void_p), None) == -1
    got = tsv.read_text()
    assert got == CR.changes(names, records, cells, c.counts)
    rows = [ln.split("\t") for ln in got.splitlines()]
    assert ["hostile", "17", "C", "GG", "4", "2", "3"] in rows and ["hostile", "9", "C", "G", "4", "2", "0"] in rows and ["gone", "1", "C", "-", "4", "4", "0"] in rows
    assert ["hostile", "30", "C", "CACGTACGT", "4", "4", "3"] in rows and ["seventy-one", "29", records[3][29], records[3][29] + "T", "4", "4", "4"] in rows
    assert ["seventy-one", "40", records[3][40], "-", "4", "4", "0"] in rows and all(len(r) == 7 for r in rows)
    if records[3][5] != "A":
        assert ["seventy-one", "5", records[3][5], "A", str(CR.MASK), str(CR.MASK), "0"] in rows
    assert not any(r[0] == "lower.2" for r in rows) and not any(r[:2] == ["hostile", "20"] for r in rows)
    want = CR.stderr_lines(c.totals, cells)
    assert [getattr(st, k) for k in ("positions", "called", "low_depth", "same", "sub", "del", "ins")] == [want[k] for k in ("positions", "called", "low_depth", "same", "sub", "del", "ins")]
    assert want["positions"] == c.P and want["low_depth"] == 6 + 140 and want["del"] == 1 + 3 + 1 and want["ins"] == 2 + 1 + 1 + 8 + 1 and want["long_ins"] == 6
    f = _cfile(libc, summ)
    t = Totals(*[c.totals[k] for k in CR.TOTALS])
    L.flappie_consensus_summary_print(f, C.byref(t), C.byref(st))
    libc.fclose(f)
    assert summ.read_text() == CR.stderr_text(c.totals, cells)
    L.flappie_map_ref_free(ref)


# ------------------------------------------------------------------------------------ the command line
@needs_hdf5
def test_options_and_their_refusals_without_gpu(tmp_path):
    fa = tmp_path / "ref.fa"
    fa.write_text(">a\nACGTACGTTGCA\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    for opt in ("--map-consensus=", "--map-consensus-changes=", "--map-consensus-min-depth=", "--map-consensus-min-identity="):
        assert opt in r.stdout, opt
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--map-consensus" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    hits, acc, cons, chg = str(tmp_path / "hits.tsv"), str(tmp_path / "acc.tsv"), str(tmp_path / "cons.fa"), str(tmp_path / "changes.tsv")
    mapped = ["--map", str(fa), "--map-out", hits]
    aligned = mapped + ["--truth-from-map", "--truth-out", acc]
    assert "--map-consensus goes with --truth-from-map" in refused(FLAPPIE, "--map-consensus", cons)
    assert "--map-consensus goes with --truth-from-map" in refused(FLAPPIE, *mapped, "--map-consensus", cons)
    goes = "--map-consensus-changes, --map-consensus-min-depth and --map-consensus-min-identity go with --map-consensus"
    for sub in (["--map-consensus-changes", chg], ["--map-consensus-min-depth", "5"], ["--map-consensus-min-identity", "900"]):
        assert goes in refused(FLAPPIE, *aligned, *sub)
    for bad in ("0", "-1", "65536", "3x", ""):
        assert "--map-consensus-min-depth must be a whole number from 1 to 65535" in refused(FLAPPIE, *aligned, "--map-consensus", cons, "--map-consensus-min-depth", bad)
    for bad in ("-1", "1001", "90x", ""):
        assert "--map-consensus-min-identity must be a whole number from 0 to 1000" in refused(FLAPPIE, *aligned, "--map-consensus", cons, "--map-consensus-min-identity", bad)
    assert "cannot be written" in refused(FLAPPIE, *aligned, "--map-consensus", str(tmp_path / "no" / "cons.fa"))
    assert "cannot be written" in refused(FLAPPIE, *aligned, "--map-consensus", cons, "--map-consensus-changes", str(tmp_path / "no" / "changes.tsv"))
    assert not os.path.exists(chg)
    for args in (["--map-consensus", cons], ["--map-consensus-changes", chg], ["--map-consensus-min-depth", "5"], ["--map-consensus-min-identity", "900"]):
        assert "--map-consensus and its --map-consensus-* options are flappie's" in refused(RUNNIE, *args)
