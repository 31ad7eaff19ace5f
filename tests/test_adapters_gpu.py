"""flappie --adapters on the GPU: the adapter records made by k_adapters (include/ffhip.h FFHIP_RUN_ADAPTERS, ffhip_batch_adapters, ffhip_op_adapter_scores,
ffhip_op_adapter_hits).

  * the operator's whole score rows equal the restatement (adapter_ref.py) at the word, wave and segment edges, Z in the call;
  * the operator's records equal the restatement when a copy of a pattern is planted so that its end lands on every column around the seams of the segments
    (S = FFHIP_ADAPTER_SEGMENT), for copies that span a seam, equal distances 64 and 65 columns apart, a better copy either side, both orientations, and 14, 15,
    16 and 40 hits in one call;
  * on synthetic 8-state (H = 256, 384) and 10-state models every record equals the restatement on the batch's own calls, with a kit cut from those calls -- one
    read a row, ragged, packed, paired, launch per step, f32 re-run, --viterbi, with and without barcodes and the move table -- and everything else the batch
    returns is bit for bit that of the same run without the flag;
  * a finished run with the flag makes exactly one more device-to-host copy call than the same run without;
  * the `flappie` binary's tagged, trimmed and split FASTQ / FASTA / SAM equal the restatement applied to its default output, and its summary adds up.
Everything is integer- or byte-exact: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

from flappie_amd import model as M
import adapter_ref as R
from test_barcodes_gpu import _d2h_calls, _packed_batch, _records, _split_records, _state, mutate, rand_seq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def same(got, want):
    return (got["nhit"], got["len"], got["kept"], got["hits"]) == (want["nhit"], want["len"], want["kept"], want["hits"])


def plant(rng, x, p, end, nedit):
    """x with a copy of p with nedit edits written so that it ENDS at column `end` (its last base is x[end - 1])"""
    c = mutate(rng, p, nedit)
    a = max(0, end - len(c))
    return x[:a] + c[len(c) - (end - a):] + x[end:]


# ------------------------------------------------------------------------------------ the operators
def test_score_rows_at_every_edge(B, engine):
    S = B.ADAPTER_SEGMENT
    assert S == B.lib().ffhip_adapter_segment() and S % 64 == 0
    rng = np.random.default_rng(11)
    full = rand_seq(rng, 5000, "ACGTZ")
    plain = full.replace("Z", "C")
    lengths = (1, 31, 32, 33, 63, 64)
    ncell = 0
    for n in (1, 31, 32):
        pats = []
        for k in range(n):                                    # random patterns, and ones cut from the call (either strand) around the seams with 0 .. 6 edits
            L = lengths[(k + n) % len(lengths)]
            if k % 3 == 2:
                p = rand_seq(rng, L)
            else:
                at = int(rng.choice([S, 2 * S, 4 * S, 100, 3000])) - int(rng.integers(0, L + 1))
                src = plain[max(0, at):max(0, at) + L]
                p = (mutate(rng, src if k % 2 else R.revcomp(src), int(rng.integers(0, 7))) or "A")[:64]
            pats.append(p)
        kit = B.Adapters(engine, pats)
        ref = R.score_rows(pats, full)                        # (a prefix's rows are a prefix of the rows)
        for ln in (0, 1, 63, 64, 65, S - 1, S, S + 1, 2 * S + 77, 5000):
            d = B.op_adapter_scores(engine, kit, full[:ln])
            assert d.shape == (2 * n, ln + 1) and np.array_equal(d, ref[:, :ln + 1]), (n, ln, np.argwhere(d != ref[:, :ln + 1])[:4])
            ncell += d.size
            got = B.op_adapter_hits(engine, kit, full[:ln])
            want = R.record(pats, full[:ln], d=ref[:, :ln + 1])
            assert same(got, want) and np.array_equal(got["raw"], R.raw_slots(want)), (n, ln, got, want)
        kit.close()
    assert ncell > 500000


def test_refusals(B, engine):
    kit = B.Adapters(engine, ["A", "ACGT", "TTTTGGGG"])
    assert B.op_adapter_scores(engine, kit, "").tolist() == [[1], [1], [4], [4], [8], [8]]
    assert B.op_adapter_hits(engine, kit, "AZGT")["hits"] == [(0, 1, 0, 0, 0), (3, 4, 0, 1, 0), (0, 4, 1, 0, 0), (0, 4, 1, 1, 0)]      # Z is read as C
    for call in ("ACGN", "acgt"):
        with pytest.raises(B.FFHipError):
            B.op_adapter_scores(engine, kit, call)
    kit.close()
    for bad in ([], ["A"] * 33, [""], ["A" * 65], ["acgt"], ["ACGN"], ["ACGZ"]):
        with pytest.raises(B.FFHipError):
            B.Adapters(engine, bad)
    B.Adapters(engine, ["A" * 64] * 32).close()


def test_hits_at_the_seams(B, engine):
    S = B.ADAPTER_SEGMENT
    rng = np.random.default_rng(3)
    p, other = rand_seq(rng, 40), rand_seq(rng, 33)
    pats = [other, p]
    kit = B.Adapters(engine, pats)
    nhit = 0
    spans = set()
    for seam in (S, 2 * S):
        base = rand_seq(rng, seam + 300)
        ends = list(range(seam - 200, seam + 201))
        calls = [plant(rng, base, p if e % 2 else R.revcomp(p), e, e % 7) for e in ends]      # one call a column, both orientations, 0 .. 6 edits
        want = R.records_many(pats, calls)
        for e, call, w in zip(ends, calls, want):
            got = B.op_adapter_hits(engine, kit, call)
            assert same(got, w) and np.array_equal(got["raw"], R.raw_slots(w)), (seam, e, got, w)
            assert any(h[2] == 1 and h[3] == (e + 1) % 2 and e - 40 < h[1] <= e + 6 for h in w["hits"]), (seam, e, w)      # (the planted copy is found: its edits may sit at its end)
            nhit += w["nhit"]
            spans |= {h[0] < seam < h[1] for h in w["hits"]}
    assert spans == {False, True} and nhit >= 802
    # equal distances 64 and 65 columns apart, a better copy within 64 columns on either side: at every offset of the pair across the seam
    worse = mutate(rng, p, 3)
    calls, kinds = [], []
    base = rand_seq(rng, S + 300)
    for first in range(S - 140, S + 41, 3):
        for kind, (gap, a, b) in enumerate(((64, p, p), (65, p, p), (50, worse, p), (50, p, worse))):
            x = plant(rng, base, a, first, 0)
            calls.append(plant(rng, x, b, first + gap, 0))
            kinds.append((kind, first))
    want = R.records_many(pats, calls)
    for (kind, first), call, w in zip(kinds, calls, want):
        got = B.op_adapter_hits(engine, kit, call)
        assert same(got, w), (kind, first, got, w)
        mine = [h for h in w["hits"] if h[2] == 1 and h[3] == 0 and first - 3 <= h[1] <= first + 68]
        assert len(mine) == (2 if kind == 1 else 1), (kind, first, w)
    # 14, 15, 16 and 40 hits in one call: the order and the cap, the hits spread over several segments and waves
    for count in (14, 15, 16, 40):
        x = rand_seq(rng, 70)
        for i in range(count):
            x += (p if i % 3 else R.revcomp(other)) + rand_seq(rng, 70 + i)
        got, w = B.op_adapter_hits(engine, kit, x), R.record(pats, x)
        assert same(got, w) and np.array_equal(got["raw"], R.raw_slots(w)), (count, got, w)
        assert w["nhit"] >= count and w["kept"] == min(15, w["nhit"]) and len(x) > 3 * S
    # a bound of one's own: max_dist 0 keeps the exact copies only, a large one is capped at L - 1
    x = plant(rng, plant(rng, rand_seq(rng, 2 * S), p, S + 5, 0), p, 300, 2)
    for md in (0, 1, 5, 63):
        got, w = B.op_adapter_hits(engine, kit, x, md), R.record(pats, x, md)
        assert same(got, w), (md, got, w)
    assert R.record(pats, x, 0)["nhit"] < R.record(pats, x, 5)["nhit"]
    kit.close()


# ------------------------------------------------------------------------------------ batches
def cut_kit(rng, calls):
    """a kit from the run's own calls: pieces of some reads from their fronts, middles and ends, as called and reverse-complemented, with planted edits; random ones"""
    plain = [c.replace("Z", "C") for c in calls]
    order = sorted(range(len(calls)), key=lambda i: -len(plain[i]))
    assert len(plain[order[5]]) >= 60, [len(c) for c in calls]
    kit = []
    for j, i in enumerate(order[:6]):
        c, L = plain[i], (24, 28, 40, 64, 33, 12)[j]
        at = (0, len(c) // 2, max(0, len(c) - L), len(c) // 3, 5, len(c) // 2)[j]
        piece = c[at:at + L]
        kit.append((mutate(rng, piece if j % 2 == 0 else R.revcomp(piece), j) or "A")[:64])
    kit += [rand_seq(rng, 28), rand_seq(rng, 6)]
    return kit


def _check_batches(B, engine, bs, nreads, flags, seen, where, max_dists=(-1, 3), temperature=1.0, barcodes=None):
    """the batches (one, or a pair run together) without the flag; a kit from those calls; then with the flag: nothing else moves, and every record equals the
    restatement on the batch's own call"""
    def run(fl):
        if len(bs) == 1:
            bs[0].run(temperature, fl)
        else:
            bs[0].run_pair(bs[1], temperature, fl)
        for x in bs:
            x.finish()
    if barcodes is not None:
        flags |= B.RUN_BARCODES
        for x in bs:
            x.set_barcodes(barcodes)
    run(flags)
    before = [[_state(B, x, v, flags) for v in range(nreads[k])] for k, x in enumerate(bs)]
    codes = [[x.barcode(v) for v in range(nreads[k])] for k, x in enumerate(bs)] if barcodes is not None else None
    with pytest.raises(B.FFHipError):
        bs[0].adapters(0)                                 # a run without the flag made none
    rng = np.random.default_rng(17)
    pats = cut_kit(rng, [st["call"] for st in before[0]])
    kit = B.Adapters(engine, pats)
    for max_dist in max_dists:
        for x in bs:
            x.set_adapters(kit, max_dist)
        run(flags | B.RUN_ADAPTERS)
        for k, x in enumerate(bs):
            for v in range(nreads[k]):
                st, old = _state(B, x, v, flags), before[k][v]
                for key in st:
                    assert st[key] == old[key] if key in ("call", "qual") else np.array_equal(np.asarray(st[key]), np.asarray(old[key])), (where, k, v, key)
                if codes is not None:
                    assert x.barcode(v) == codes[k][v], (where, k, v)
                want = R.record(pats, st["call"], max_dist)
                got = x.adapters(v)
                assert got == want, (where, k, v, max_dist, got, want)
                seen["reads"] += 1
                seen["hits"] += want["nhit"]
                seen["long"] += len(st["call"]) > B.ADAPTER_SEGMENT
                seen["minus"] += any(h[3] for h in want["hits"])
    for x in bs:
        x.set_adapters(None)
    with pytest.raises(B.FFHipError):                     # no kit attached
        bs[0].run(temperature, flags | B.RUN_ADAPTERS)
    kit.close()


def _tally():
    return {"reads": 0, "hits": 0, "long": 0, "minus": 0}


@pytest.mark.parametrize("kind,hidden", [(M.NET_LSTM5, 256), (M.NET_LSTM5, 384), (M.NET_GRUMOD5, 256)])
def test_batch_records_rows_ragged_packed(B, engine, kind, hidden):
    seen = _tally()
    dm = B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
    rng = np.random.default_rng(hidden + kind)
    extra = B.RUN_MOVES | (B.RUN_MOD_PROBS if kind == M.NET_GRUMOD5 else 0)
    bkit = B.Barcodes(engine, [rand_seq(rng, 24) for _ in range(5)])
    # one read a row, all of one length
    b = B.Batch(dm, 16, 1500)
    b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
    _check_batches(B, engine, [b], [16], B.RUN_NO_TRACE, seen, ("rows", kind, hidden))
    _check_batches(B, engine, [b], [16], extra, seen, ("rows + tags", kind, hidden), max_dists=(-1,), barcodes=bkit)
    b.close()
    # ragged, with reads whose calls take several segments
    sigs = [rng.standard_normal(int(n)).astype(np.float32) for n in list(rng.integers(600, 2001, 12)) + [9000, 12000, 7000, 5000]]
    b = B.Batch(dm, 16, 12000)
    b.set_signals_ragged(sigs)
    _check_batches(B, engine, [b], [16], B.RUN_VITERBI_ONLY | B.RUN_NO_TRACE, seen, ("ragged --viterbi", kind, hidden))
    b.close()
    # packed: default, launch per step, with the other tags
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    _check_batches(B, engine, [pb], [n], B.RUN_NO_TRACE, seen, ("packed", kind, hidden), max_dists=(-1,))
    _check_batches(B, engine, [pb], [n], B.RUN_STEPWISE_RNN | B.RUN_NO_TRACE | extra, seen, ("packed per step", kind, hidden), max_dists=(5,), barcodes=bkit)
    pb.close()
    bkit.close()
    dm.close()
    assert seen["reads"] >= 120 and seen["hits"] >= 30 and seen["long"] >= 4 and seen["minus"] >= 5, seen


def test_batch_records_paired_and_after_an_f32_rerun(B, engine):
    seen = _tally()
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    rng = np.random.default_rng(7)
    pair = []
    for k in range(2):
        b = B.Batch(dm, 16, 1500)
        b.set_signals(rng.standard_normal((16, 1500)).astype(np.float32))
        pair.append(b)
    _check_batches(B, engine, pair, [16, 16], B.RUN_NO_TRACE, seen, "pair", max_dists=(-1,))
    for b in pair:
        b.close()
    pbs = [_packed_batch(B, dm, 16, 4000, 24, rng) for _ in range(2)]
    _check_batches(B, engine, [p[0] for p in pbs], [p[1] for p in pbs], B.RUN_NO_TRACE | B.RUN_MOVES, seen, "packed pair", max_dists=(-1,))
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
    _check_batches(B, engine, [b], [16], 0, seen, "rerun rows", max_dists=(-1,))
    assert b.f32_reruns() == 1
    b.close()
    pb = B.Batch(dm, 16, 4000, max_reads=16)
    slot, off = pb.pack_plan([x.size for x in sigs])
    assert min(slot) >= 0
    pb.set_signals_packed(sigs, slot, off)
    _check_batches(B, engine, [pb], [16], B.RUN_MOVES, seen, "rerun packed", max_dists=(-1,))
    assert pb.f32_reruns() == sum(1 for k in range(16) if slot[k] == slot[1]) >= 1
    pb.close()
    dm.close()
    assert seen["reads"] >= 100 and seen["hits"] >= 20, seen


def test_exactly_one_more_copy_call(B, engine):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    rng = np.random.default_rng(1)
    b = B.Batch(dm, 8, 2000)
    b.set_signals(rng.standard_normal((8, 2000)).astype(np.float32))
    pb, n = _packed_batch(B, dm, 16, 4000, 24, rng)
    kit = B.Adapters(engine, [rand_seq(rng, 28) for _ in range(8)])
    for x, nr in ((b, 8), (pb, n)):
        x.set_adapters(kit)
        calls, held = {}, {}
        for fl in (B.RUN_ADAPTERS, 0, B.RUN_ADAPTERS):          # (the first run creates the buffers; the counts are taken from the later two)
            _d2h_calls(B)
            before = x.device_bytes() if fl and not held else None
            x.run(1.0, B.RUN_NO_TRACE | fl)
            x.finish()
            calls[fl] = _d2h_calls(B)
            if before is not None:
                held = {"grew": x.device_bytes() - before}
        assert calls[B.RUN_ADAPTERS][0] == calls[0][0] + 1, calls
        assert calls[B.RUN_ADAPTERS][1] == calls[0][1] + 256 * nr, calls      # ... of 256 bytes a read
        assert held["grew"] >= 256 * nr, held                                 # the device buffer is counted
        assert set(x.adapters(0)) == {"nhit", "len", "kept", "hits"}
    kit.close()
    b.close()
    pb.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary
def test_flappie_adapters(tmp_path):
    from test_cli import FAST5LIB, FLAPPIE, TOOL, synth_raw, write_fast5
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    reads = tmp_path / "reads"
    reads.mkdir()
    rng = np.random.default_rng(3)
    nread = 20
    for i, n in enumerate(list(rng.integers(3000, 9000, nread - 2)) + [20000, 30000]):
        write_fast5(reads / ("read_%02d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    env = dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path))

    def run(args, extra=None):
        r = subprocess.run([FLAPPIE, "--model", "r941_native", "--batch", "16"] + args + [str(reads)], env=dict(env, **(extra or {})), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, r.stderr

    default = {fmt: run(["--format", fmt])[0] for fmt in ("fastq", "fasta", "sam")}
    recs = _records(default["fastq"], "fastq")
    assert len(recs) == nread
    # The kit's sources in the order of the read ids.  The binary lists a directory as glob() finds it (GLOB_NOSORT, as the reference does), which is the file
    # system's order and not the same on every machine; the conditions below on what the kit cuts depend on which calls it was made from, so those are fixed.
    calls = [r[1] for r in sorted(recs, key=lambda r: r[0])]
    # a kit from the calls: fronts and ends of some reads (what a trim cuts), the middles of others (what a split cuts), one short pattern that occurs often
    plain = [c.replace("Z", "C") for c in calls]
    krng = np.random.default_rng(5)
    pats = [mutate(krng, plain[0][4:32], 1), mutate(krng, R.revcomp(plain[1][-30:-2]), 2), plain[2][len(plain[2]) // 2:len(plain[2]) // 2 + 40],
            mutate(krng, R.revcomp(plain[3][len(plain[3]) // 3:len(plain[3]) // 3 + 28]), 2), plain[4][:24], plain[4][-24:], plain[6][180:208], rand_seq(krng, 28)]
    assert min(len(c) for c in plain[:7]) >= 400, [len(c) for c in plain]
    names = ["ad%02d" % (k + 1) for k in range(len(pats))]
    kit = tmp_path / "kit.fa"
    kit.write_text("".join(">%s adapter %d\n%s\n%s\n" % (nm, k, p[:5].lower(), p[5:]) for k, (nm, p) in enumerate(zip(names, pats))))
    modes, tagged = set(), {}
    for opts, md, kw in (([], -1, {}), (["--trim-adapters"], -1, dict(trim=True)), (["--trim-adapters", "--adapter-window", "40", "--adapter-max-dist", "1"], 1, dict(trim=True, W=40)),
                         (["--split-reads", "--split-min-length", "150"], -1, dict(split=True, M=150)), (["--split-reads", "--trim-adapters", "--adapter-max-dist", "0"], 0, dict(split=True, trim=True)),
                         (["--split-reads", "--adapter-max-dist", "9"], 9, dict(split=True))):          # (nine edits: chance hits everywhere, more than 15 of them in a long read)
        for fmt in ("fastq", "fasta", "sam") if opts in ([], ["--trim-adapters"], ["--split-reads", "--split-min-length", "150"]) else ("fastq",):      # (every format for the tags, the plain trim and the split; FASTQ for the parameters)
            got, err = run(["--format", fmt, "--adapters", str(kit)] + opts)
            tagged[fmt] = got if not opts else tagged.get(fmt)
            want, count, stats, with_hit = "", [0] * len(pats), [0, 0, 0, 0], 0
            for name, call, qual, rec in _records(default[fmt], fmt):
                a = R.record(pats, call, md)
                want += R.records_text(fmt, rec[0], call, qual, a, names, name, **kw)
                mode, pieces, dropped, overflow = R.cuts(a, len(call), **kw)
                modes.add((mode, overflow, dropped > 0))
                for h in a["hits"]:
                    count[h[2]] += 1
                with_hit += a["nhit"] > 0
                stats = [stats[0] + (mode == "split"), stats[1] + (len(pieces) if mode == "split" else 0), stats[2] + dropped, stats[3] + overflow]
            assert got == want, (opts, fmt)
            assert dict(re.findall(r"^adapter\t(\S+)\t(\d+)$", err, re.M)) == {nm: str(c) for nm, c in zip(names, count)}, err
            summary = dict(re.findall(r"^adapters\t(\S+)\t(\d+)$", err, re.M))
            assert summary == {"reads_with_hit": str(with_hit), "split_reads": str(stats[0]), "pieces": str(stats[1]), "dropped_pieces": str(stats[2]), "overflow": str(stats[3])}, err
    assert {("one", False, False), ("split", False, False), ("one", True, False)} <= modes and any(m[2] for m in modes), modes
    # with --barcodes: the adapter tags behind the barcode tags, and the larger cut at each end wins
    import barcode_ref as BR
    bpats = [plain[0][2:26], R.revcomp(plain[1])[1:25], rand_seq(krng, 24)]
    bnames = ["bc01", "bc02", "bc03"]
    bkit = tmp_path / "bkit.fa"
    bkit.write_text("".join(">%s\n%s\n" % x for x in zip(bnames, bpats)))
    got, _ = run(["--format", "fastq", "--adapters", str(kit), "--barcodes", str(bkit), "--trim-barcodes", "--trim-adapters"])
    want, cut_by = "", set()
    for name, call, qual, rec in recs:
        a, c = R.record(pats, call), BR.classify(bpats, call)
        clip = BR.trim_range(c, len(call))
        want += R.records_text("fastq", rec[0], call, qual, a, names, name, extra_tags=BR.tags(c, bnames), trim=True, clip=clip)
        t, both = R.trim_range(a, len(call)), R.cuts(a, len(call), trim=True, clip=clip)[1][0]
        cut_by |= {("barcode", both[0] > t[0] or both[1] < t[1]), ("adapter", both[0] > clip[0] or both[1] < clip[1])}
    assert got == want
    assert {("barcode", True), ("adapter", True)} <= cut_by, cut_by
    # the tags describe the call in signal order under --reverse; SEQ and QUAL of every piece are reversed
    got, _ = run(["--format", "fastq", "--adapters", str(kit), "--split-reads", "--split-min-length", "150", "--reverse"])
    assert got == "".join(R.records_text("fastq", rec[0], call, qual, R.record(pats, call), names, name, reverse=True, split=True, M=150) for name, call, qual, rec in recs)
    # the other pipeline form changes no byte
    assert run(["--format", "fastq", "--adapters", str(kit)], {"FLAPPIE_DEBUG": "no_pack"})[0] == tagged["fastq"]
