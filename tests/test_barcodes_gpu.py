"""flappie --barcodes on the GPU: the barcode records made by k_barcodes (include/ffhip.h FFHIP_RUN_BARCODES, ffhip_batch_barcode, ffhip_op_barcode_scores).

  * the operator's whole distance / end matrices equal the restatement (barcode_ref.py) at the word, carry, wave and window edges; the tie rules; the refusals;
  * on synthetic 8-state (H = 256, 384) and 10-state models every record equals the restatement on the batch's own calls, with a kit built from those calls --
    one read a row, ragged, packed, paired, launch per step, f32 re-run, --viterbi, with and without the move table and the 5mC bytes, both_ends on and off --
    and everything else the batch returns is bit for bit that of the same run without the flag;
  * a finished run with the flag makes exactly one more device-to-host copy call than the same run without;
  * the `flappie` binary's tagged and trimmed FASTQ / FASTA / SAM equal the restatement applied to its default output, and its summary adds up.
Everything is integer- or byte-exact: no tolerance anywhere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import barcode_ref as R

pytestmark = pytest.mark.gpu

PATTERN_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128)


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def mutate(rng, s, nedit):
    """nedit planted substitutions, insertions and deletions"""
    s = list(s)
    for _ in range(nedit):
        kind, at = rng.integers(0, 3), int(rng.integers(0, max(1, len(s))))
        if kind == 0 and s:
            s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
        elif kind == 1:
            s.insert(at, "ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 1:
            del s[at]
    return "".join(s)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def operator_kit(rng, full, n, W, lengths):
    """n patterns whose lengths run through `lengths`: random ones, and ones cut from the call and from the reverse complements of the calls the test searches,
    with 0 .. 6 planted edits"""
    plain = full.replace("Z", "C")
    sources = [plain, R.revcomp(plain), R.revcomp(plain[:W]), R.revcomp(plain[:W + 1])]
    kit = []
    for k in range(n):
        L = lengths[k % len(lengths)]
        if k % 3 == 0:
            p = rand_seq(rng, L)
        else:
            src = sources[k % len(sources)]
            a = int(rng.integers(0, max(1, min(W, len(src)) - L // 2)))
            p = mutate(rng, src[a:a + L] or "A", int(rng.integers(0, 7)))[:128] or "A"
        kit.append(p)
    return kit


def test_operator_matrices_at_every_edge(B, engine):
    rng = np.random.default_rng(11)
    full = rand_seq(rng, 1000, "ACGTZ")
    assert "Z" in full[:100] and "Z" in full[-100:]
    ncell = 0
    for W in (1, 150, 256):
        for n in (1, 63, 64, 65, 96, 128):
            lengths = PATTERN_LENGTHS if n != 64 else (1, 31, 32, 33, 63, 64)      # (a kit of 64-base patterns at most runs the one-word kernel)
            pats = operator_kit(rng, full, n, W, lengths)
            kit = B.Barcodes(engine, pats, W)
            for ln in sorted({0, 1, W - 1, W, W + 1, 1000}):
                call = full[:ln]
                dist, end = B.op_barcode_scores(engine, kit, call)
                wd, we = R.scores(pats, call, W)
                assert dist.shape == (2, n) and np.array_equal(dist, wd), (W, n, ln, np.argwhere(dist != wd)[:4])
                assert np.array_equal(end, we), (W, n, ln, np.argwhere(end != we)[:4])
                ncell += 2 * n
            kit.close()
    assert ncell > 10000


def test_operator_tie_rules_and_refusals(B, engine):
    # the smallest end of the minimum; an empty window gives dist = L, end = 0
    kit = B.Barcodes(engine, ["A", "ACGT", "TTTT"], 150)
    dist, end = B.op_barcode_scores(engine, kit, "AAAAACGTACGT")
    assert list(dist[0]) == [0, 0, 3] and list(end[0]) == [1, 8, 8] and list(end[1]) == [1, 4, 11], (dist, end)
    assert np.array_equal(np.stack([dist, end]), np.stack(R.scores(["A", "ACGT", "TTTT"], "AAAAACGTACGT", 150)))
    dist, end = B.op_barcode_scores(engine, kit, "")
    assert dist.tolist() == [[1, 4, 4], [1, 4, 4]] and end.tolist() == [[0, 0, 0], [0, 0, 0]]
    # Z is read as C, at the rear as well (complemented to G)
    dist, end = B.op_barcode_scores(engine, kit, "AZGT")
    assert dist[0][1] == 0 and dist[1][1] == 0
    with pytest.raises(B.FFHipError):
        B.op_barcode_scores(engine, kit, "ACGN")
    with pytest.raises(B.FFHipError):
        B.op_barcode_scores(engine, kit, "acgt")
    kit.close()
    for bad, W in (([], 150), (["A"] * 129, 150), ([""], 150), (["A" * 129], 150), (["acgt"], 150), (["ACGN"], 150), (["ACGZ"], 150), (["ACGT"], 0), (["ACGT"], 257)):
        with pytest.raises(B.FFHipError):
            B.Barcodes(engine, bad, W)
    B.Barcodes(engine, ["A" * 128] * 128, 256).close()


# ------------------------------------------------------------------------------------ batches
class Tally:
    def __init__(self):
        self.n = {"front": 0, "rear": 0, "max_dist": 0, "min_sep": 0}
        self.reads = 0

    def add(self, rec, max_dist):
        self.reads += 1
        self.n[R.category(rec, max_dist)] += 1


def planted_kit(rng, calls, long_pattern=False):
    """a kit from the run's own calls: fronts and reverse-complemented tails of some reads with planted edits, two near-identical patterns, random patterns"""
    good = [i for i, c in enumerate(calls) if len(c) >= 40]
    assert len(good) >= 8, [len(c) for c in calls]
    plain = [c.replace("Z", "C") for c in calls]
    L = 24
    kit = []
    for j, i in enumerate(good[:3]):                      # fronts, 0 / 2 / 4 edits
        kit.append(mutate(rng, plain[i][3:3 + L], 2 * j))
    for j, i in enumerate(good[3:6]):                     # tails, 0 / 2 / 4 edits
        kit.append(mutate(rng, R.revcomp(plain[i])[2:2 + L], 2 * j))
    twin = plain[good[6]][1:1 + L]                        # two near-identical patterns (one substitution apart), and the same pattern twice
    kit += [twin, twin[:10] + "ACGT"[("ACGT".index(twin[10]) + 1) % 4] + twin[11:]]
    dup = R.revcomp(plain[good[7]])[0:L]
    kit += [dup, dup]
    kit += [rand_seq(rng, L) for _ in range(3)]
    if long_pattern:                                      # a pattern of two words (the carry between them), cut from a front
        src = plain[good[0]]
        kit.append(mutate(rng, src[5:5 + 70], 3) if len(src) >= 80 else rand_seq(rng, 70))
    return kit


def _state(B, b, v, flags):
    path, qpath = b.path(v)
    st = dict(path=path, qpath=qpath.view(np.uint32), score=np.float32(b.score(v)).view(np.uint32), call=b.basecall(v), qual=b.quality(v))
    if not (flags & B.RUN_NO_TRACE):
        st["trace"] = b.trace(v)
    if flags & B.RUN_MOD_PROBS:
        st["ml"] = b.mod_probs(v)
    if flags & B.RUN_MOVES:
        st["mv"] = b.moves(v)
    return st


def _check_batches(B, engine, bs, nreads, flags, tally, where, W=150, params=((-1, -1, False), (4, 2, True)), long_pattern=False, temperature=1.0):
    """the batches (one, or a pair run together) without the flag; a kit from those calls; then with the flag: nothing else moves, and every record equals the
    restatement on the batch's own call"""
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
        for x in bs:
            x.finish()
    run(flags)
    before = [[_state(B, x, v, flags) for v in range(nreads[k])] for k, x in enumerate(bs)]
    with pytest.raises(B.FFHipError):
        bs[0].barcode(0)                                  # a run without the flag made none
    rng = np.random.default_rng(17)
    pats = planted_kit(rng, [st["call"] for st in before[0]], long_pattern)
    kit = B.Barcodes(engine, pats, W)
    for max_dist, min_sep, both in params:
        for x in bs:
            x.set_barcodes(kit, max_dist, min_sep, both)
        run(flags | B.RUN_BARCODES)
        md = R.default_max_dist(pats) if max_dist < 0 else max_dist
        ms = 3 if min_sep < 0 else min_sep
        for k, x in enumerate(bs):
            for v in range(nreads[k]):
                st, old = _state(B, x, v, flags), before[k][v]
                for key in st:
                    assert st[key] == old[key] if key in ("call", "qual") else np.array_equal(np.asarray(st[key]), np.asarray(old[key])), (where, k, v, key)
                want = R.classify(pats, st["call"], W, md, ms, both)
                got = x.barcode(v)
                assert got == want, (where, k, v, both, got, want)
                tally.add(got, md)
    for x in bs:
        x.set_barcodes(None)
    with pytest.raises(B.FFHipError):                     # no kit attached
        bs[0].run(temperature, flags | B.RUN_BARCODES)
    kit.close()


def _packed_batch(B, dm, rows, cap, nreads, rng, lo=600, hi=2000):
    lens = [int(x) for x in rng.integers(lo, hi + 1, nreads)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    pb = B.Batch(dm, rows, cap, max_reads=len(sigs))
    slot, off = pb.pack_plan(lens)
    assert min(slot) >= 0 and len(set(slot)) < len(slot), "every read placed, several to a row"
    pb.set_signals_packed(sigs, slot, off)
    return pb, len(sigs)


def _assert_tally(tally, reads):
    assert tally.reads >= reads, tally.reads
    assert all(v >= 1 for v in tally.n.values()), tally.n


@pytest.mark.parametrize("kind,hidden", [(M.NET_LSTM5, 256), (M.NET_LSTM5, 384), (M.NET_GRUMOD5, 256)])
def test_batch_records_rows_ragged_packed(B, engine, kind, hidden):
    tally = Tally()
    dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
    rng = np.random.default_rng(hidden + kind)
    extra = B.RUN_MOVES | (B.RUN_MOD_PROBS if kind == M.NET_GRUMOD5 else 0)
    # one read a row, all of one length
    b = B.Batch(dm, 16, 1500)
    b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
    _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE, tally, ("rows", kind, hidden), long_pattern=True)
    _check_batches(B, engine, [b], [16], extra, tally, ("rows + tags", kind, hidden), params=((-1, -1, False),))
    b.close()
    # ragged
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE, tally, ("ragged --viterbi", kind, hidden), W=40)
    b.close()
    # packed: default, launch per step, with the other tags
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    _check_batches(B, engine, [pb], [n], B.RUN_NO_TRACE, tally, ("packed", kind, hidden), long_pattern=True)
    _check_batches(B, engine, [pb], [n], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE | extra, tally, ("packed per step", kind, hidden), params=((5, 3, False),))
    pb.close()
    dm.close()
    _assert_tally(tally, 150)


def test_batch_records_paired_and_after_an_f32_rerun(B, engine):
    tally = Tally()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 16, 1500)
        b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
        pair.append(b)
    _check_batches(B, engine, pair, [16, 16], B.RUN_NO_TRACE, tally, "pair")
    for b in pair:
        b.close()
    pbs = [_packed_batch(B, dm, 16, 4000, 24, rng) for _ in range(2)]
    _check_batches(B, engine, [p[0] for p in pbs], [p[1] for p in pbs], B.RUN_NO_TRACE | B.RUN_MOVES, tally, "packed pair", params=((-1, -1, False),))
    for p in pbs:
        p[0].close()
    dm.close()
    # an outlier: the reads of its row come from the f32 re-run, and so do their records
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(4)
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in rng.integers(600, 2001, 16)]
    sigs[1][200] = 6.0e4
    b = B.Batch(dm, 16, 2000)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], 0, tally, "rerun rows")
    assert b.f32_reruns() == 1
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, engine, [pb], [16], B.RUN_MOVES, tally, "rerun packed", params=((-1, -1, False),))
    assert pb.f32_reruns() == sum(1 for k in range(16) if slot[k] == slot[1]) >= 1
    pb.close()
    dm.close()
    _assert_tally(tally, 100)


def _d2h_calls(B):
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, 1)
    return int(c[2]), int(c[3])


def test_exactly_one_more_copy_call(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(1)
    b = B.Batch(dm, 8, 2000)
    b.set_signals(rng.standard_normal((8, 2000)).astype(np.float32))
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    kit = B.Barcodes(engine, [rand_seq(rng, 24) for _ in range(12)])
    for x, nr in ((b, 8), (pb, n)):
        x.set_barcodes(kit)
        calls = {}
        for fl in (B.RUN_BARCODES, 0, B.RUN_BARCODES):          # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            x.run(1.0, B.RUN_NO_TRACE | fl)
            x.finish()
            calls[fl] = _d2h_calls(B)
        assert calls[B.RUN_BARCODES][0] == calls[0][0] + 1, calls
        assert calls[B.RUN_BARCODES][1] == calls[0][1] + 16 * nr, calls      # ... of 16 bytes a read
        assert set(x.barcode(0)) == set(R.FIELDS)
    kit.close()
    b.close()
    pb.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def _split_records(text, step):
    lines = text.split("\n")[:-1]
    return [lines[k:k + step] for k in range(0, len(lines), step)]


def _records(default, fmt):
    """name, call, qual, lines of every record of the default output"""
    out = []
    for rec in _split_records(default, {"fastq": 4, "fasta": 2, "sam": 2}[fmt]):
        if fmt == "sam":
            f = rec[0].split("\t")
            out.append((f[0], f[9], f[10], rec))
        else:
            out.append((rec[0][1:].split("  {")[0], rec[1], rec[3] if fmt == "fastq" else None, rec))
    return out


def _want(fmt, rec, call, qual, tags, keep=None):
    a, b = keep if keep is not None else (0, len(call))
    seq, q = call[a:b], (qual[a:b] if qual is not None else None)
    if fmt == "sam":
        f = rec[0].split("\t")
        return "\t".join(f[:9] + [seq, q]) + "\t" + tags + "\n"
    if fmt == "fasta":
        return rec[0] + "\t" + tags + "\n" + seq + "\n"
    return rec[0] + "\t" + tags + "\n" + seq + "\n+\n" + q + "\n"


def test_flappie_barcodes(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 24
    for i, n in enumerate(rng.integers(1500, 6000, nread)):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, extra=None):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default = {fmt: run(["--format", fmt])[0] for fmt in ("fastq", "fasta", "sam")}
    recs = _records(default["fastq"], "fastq")
    assert len(recs) == nread
    pats = planted_kit(np.random.default_rng(5), [r[1] for r in recs])
    names = ["bc%02d" % (k + 1) for k in range(len(pats))]
    kit = tmp_path / "kit.fa"
    kit.write_text("".join(">%s sample %d\n%s\n%s\n" % (nm, k, p[:10].lower(), p[10:]) for k, (nm, p) in enumerate(zip(names, pats))))
    md = R.default_max_dist(pats)
    cats = set()
    for opts, kw in (([], {}), (["--barcode-window", "60", "--barcode-max-dist", "4", "--barcode-min-sep", "2", "--barcode-both-ends"], dict(W=60, max_dist=4, min_sep=2, both_ends=True))):
        for fmt in ("fastq", "fasta", "sam"):
            tagged, err = run(["--format", fmt, "--barcodes", str(kit)] + opts)
            trimmed, _ = run(["--format", fmt, "--barcodes", str(kit), "--trim-barcodes"] + opts)
            step = {"fastq": 4, "fasta": 2, "sam": 1}[fmt]
            got, gott = _split_records(tagged, step), _split_records(trimmed, step)
            count = {}
            for k, (name, call, qual, rec) in enumerate(_records(default[fmt], fmt)):
                c = R.classify(pats, call, **kw)
                cats.add(R.category(c, kw.get("max_dist", md)))
                assert "\n".join(got[k]) + "\n" == _want(fmt, rec, call, qual, R.tags(c, names)), (fmt, name)
                assert "\n".join(gott[k]) + "\n" == _want(fmt, rec, call, qual, R.tags(c, names), R.trim_range(c, len(call))), (fmt, name)
                count[c["best"]] = count.get(c["best"], 0) + 1
            summary = dict(re.findall(r"^barcode\t(\S+)\t(\d+)$", err, re.M))
            assert list(summary) == names + ["unclassified"] and sum(int(v) for v in summary.values()) == nread, err
            assert all(int(summary[nm]) == count.get(k, 0) for k, nm in enumerate(names)) and int(summary["unclassified"]) == count.get(-1, 0), (summary, count)
    assert cats == {"front", "rear", "max_dist", "min_sep"}, cats
    # the tags describe the call in signal order under --reverse; SEQ and QUAL are reversed, and so is what the trim keeps
    fwd, _ = run(["--format", "fastq", "--barcodes", str(kit)])
    rev, _ = run(["--format", "fastq", "--barcodes", str(kit), "--reverse"])
    revt, _ = run(["--format", "fastq", "--barcodes", str(kit), "--reverse", "--trim-barcodes"])
    for (name, call, qual, rec), rr, rt in zip(recs, _split_records(rev, 4), _split_records(revt, 4)):
        c = R.classify(pats, call)
        a, b = R.trim_range(c, len(call))
        assert rr[0].split("\t")[1:] == R.tags(c, names).split("\t") and rr[1] == call[::-1] and rr[3] == qual[::-1], name
        assert rt[1] == call[a:b][::-1] and rt[3] == qual[a:b][::-1], name
    # no pipeline form changes a byte
    for dbg in ("no_pack", "pack_fail"):
        assert run(["--format", "fastq", "--barcodes", str(kit)], {"FLAPPIE_DEBUG": dbg})[0] == fwd, dbg
    assert run(["--format", "fastq"])[0] == default["fastq"]
