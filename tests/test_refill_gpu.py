"""A batch object that is filled again is held to a fresh one: every feature, form and model.

`flappie` creates a few batch objects and fills them again for every chunk -- other reads, lengths and empty slots, other truths, sequences and variants,
sometimes other settings.  The expected value of such a run is exact: launches repeat bit for bit (test_repeat_launch_gpu.py) and a read's results do not depend
on where it stands (test_packed_gpu.py), so a refilled object returns what a FRESH object of the same constructor arguments returns after the same filling, the
same setter calls and the same run.  Every comparison here is byte equality of everything the object returns for every slot (refill_steps.state); an accessor
that refuses contributes its text, so a `valid` flag that outlives its run or a record of a slot that is empty now shows as a difference.

  * F1, F2, F3, F1 on one object (refill_steps.STEPS): one read a row, packed, packed on the launch-per-step kernels; the 4-base LSTM and the 5-base GRU model;
  * two row batches refilled and run as a pair; two objects in flight, refilled the way the CLI's pipeline refills them;
  * one pileup fed by the refilled object against one fed by fresh ones; the run-length model's run records; the device memory never falls;
  * the `flappie` binary over a directory in chunks of 16 reads and groups of 4 against one chunk: the same bytes, every feature; and the packed path;
  * tools/truth_bench.py runs to its end.
The conditions that keep the comparisons from being vacuous are asserted on the fresh objects' records only (Seen.check).  One is weaker than it could be:
map status 0 (a call of no bases) is asked of the LSTM trunk only, which gives one for the 19-sample read; the GRU model calls a base on every read here."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from flappie_amd import model as M
import refill_steps as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def B():
    from flappie_amd import binding
    return binding


@pytest.fixture(scope="module")
def engine(B):
    e = B.Engine(0)
    yield e
    e.close()


def _run(bs, fl):
    if len(bs) == 1:
        bs[0].run(1.0, fl)
    else:
        bs[0].run_pair(bs[1], 1.0, fl)
    for b in bs:
        b.finish()


def _plain_calls(B, dm, form, fills, nbase, extra=0):
    """the calls of every filling (groups of them) on a scratch object: the reference and the kits are made from them, once, up front"""
    calls = []
    b = S.make_batch(B, dm, form)
    for group in fills:
        for sigs in group:
            S.fill(b, form, sigs)
            _run([b], S.base_flags(B, nbase, extra))
            calls += list(S.calls_of(b).values())
    b.close()
    return calls


def _step(B, bs, form, step, sigs, shared, nbase, extra=0):
    """one step on the batch (or the pair): the signals, a run without feature flags for the calls, the inputs from those calls, the setters, the run with the
    flags, the finish.  Returns the inputs, one set a batch"""
    for b, sg in zip(bs, sigs):
        S.fill(b, form, sg)
    _run(bs, S.base_flags(B, nbase, extra))
    inps = [S.inputs(step, b, nbase, seed=k) for k, b in enumerate(bs)]
    for b, inp in zip(bs, inps):
        S.apply_setters(B, b, step, inp, shared, nbase)
    _run(bs, S.feature_flags(B, step, nbase, extra))
    return inps


class Seen:
    """what the FRESH objects' records show, step after step"""

    def __init__(self):
        self.steps, self.two, self.minus, self.neginf, self.reruns = [], 0, 0, 0, []

    def add(self, B, b, step, inp, fl):
        tf, rf = S.forms_of(B, b, step, inp)
        status = {"truth": [], "remap": [], "map": []}
        for v in range(b.nreads()):
            if b.read_nblock(v) == 0:
                continue
            m = b.map(v)
            for name, rec in (("truth", b.truth(v)), ("remap", b.remap(v)), ("map", m)):
                status[name].append(rec["status"])
            self.two += m["nanchor"] == 2
            self.minus += m["status"] == 1 and m["q"] & 1
            vc = b.variant_calls(v) if fl & B.RUN_REMAP_VARIANTS else None
            if vc is not None and vc.size:
                self.neginf += int(np.isneginf(vc["alt"][inp[2][v]["nref"] == 0]).sum())
        self.steps.append(dict(status=status, tf=tf, rf=rf))
        self.reruns.append(b.f32_reruns())

    def check(self, reruns, map0):
        print("seen:", [{k: np.bincount(v, minlength=4).tolist() for k, v in s["status"].items()} for s in self.steps], "truth forms", [sorted(set(s["tf"].values())) for s in self.steps],
              "remap forms", [sorted(set(s["rf"].values())) for s in self.steps], "two anchors", self.two, "minus", self.minus, "-inf insertions", self.neginf, "re-runs", self.reruns)
        for k, s in enumerate(self.steps):
            for name, st in s["status"].items():
                assert 2 * sum(x == 1 for x in st) >= len(st) > 0, ("at least half the reads have status 1", k, name, st)
        for name in ("truth", "remap", "map"):
            every = {x for s in self.steps for x in s["status"][name]}
            # WEAKER for map on the GRU model: map status 0 is a call of no bases.  The LSTM trunk gives one for F2's 19-sample read (the shortest legal read) under
            # either head; the GRU model calls a base on every read of these fillings (2 samples a block: 10 blocks), so statuses 1 and 2 are all that is asked there
            want = {0, 1, 2} if name != "map" or map0 else {1, 2}
            assert want <= every, (name, every)
        for key in ("tf", "rf"):
            assert len({f for s in self.steps for f in s[key].values()}) >= 2, ("two kernel forms", key)
        for a, b in zip(self.steps, self.steps[1:]):
            assert any(a[key][v] != b[key][v] for key in ("tf", "rf") for v in a[key] if v in b[key]), "a read changes its form between consecutive steps"
        assert self.two >= 1 and self.minus >= 1 and self.neginf >= 1, (self.two, self.minus, self.neginf)
        # the outlier of F2 sends its read (packed: its row) through the f32 re-run, and only there; the GRU trunk's convolution ends in tanh, so no sample
        # takes it out of the split format's range and its re-run counts are all zero: equal on both objects, which is all that is held there.  "lstm5mod", the
        # LSTM trunk under the 5-base head, is the model whose re-run carries site mods and 5mC bytes
        assert self.reruns == ([0, self.reruns[1], 0, 0] if reruns else [0, 0, 0, 0]) and (self.reruns[1] >= 1 or not reruns), self.reruns


CASES = [("rows", 0), ("packed", 0), ("packed", "RUN_STEPWISE_RNN")]


def _model(kind):
    """(model, nbase): H = 128; "lstm5mod" is the LSTM trunk under the GRU model's 5-base head (as tests/golden/make_result_copies.py has it)"""
    if kind != "lstm5mod":
        return M.synthetic_model(kind, 128, seed=1), 5 if kind == M.NET_GRUMOD5 else 4
    lstm, gru = M.synthetic_model(M.NET_LSTM5, 128, seed=1), M.synthetic_model(M.NET_GRUMOD5, 128, seed=1)
    return M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b), 5


# every form with the two models, and the rows form with the model whose f32 re-run carries the 5-base features
MODEL_CASES = [(f, e, k) for f, e in CASES for k in (M.NET_LSTM5, M.NET_GRUMOD5)] + [("rows", 0, "lstm5mod")]
MODEL_IDS = ["%s-%s" % (f + ("_stepwise" if e else ""), {M.NET_LSTM5: "lstm5", M.NET_GRUMOD5: "grumod5"}.get(k, k)) for f, e, k in MODEL_CASES]


@pytest.mark.parametrize("form,extra,kind", MODEL_CASES, ids=MODEL_IDS)
def test_refilled_batch_equals_a_fresh_one(B, engine, form, extra, kind):
    extra = getattr(B, extra) if extra else 0
    mdl, nbase = _model(kind)
    dm = B.DeviceModel(engine, mdl)
    fills = S.fillings(form, 11)
    shared = S.Shared(B, engine, _plain_calls(B, dm, form, [[f] for f in fills], nbase, extra))
    refilled = S.make_batch(B, dm, form)
    seen, held, first = Seen(), [], None
    for n, k in enumerate(S.SEQUENCE):
        step = S.STEPS[k]
        fresh = S.make_batch(B, dm, form)
        inp = _step(B, [fresh], form, step, [fills[step["fill"]]], shared, nbase, extra)[0]
        _step(B, [refilled], form, step, [fills[step["fill"]]], shared, nbase, extra)
        want, got = S.states(B, fresh, form), S.states(B, refilled, form)
        assert not S.differences(got, want), ("step", n, S.differences(got, want)[:8])
        assert refilled.f32_reruns() == fresh.f32_reruns(), ("step", n)
        for name in step["drop"]:                           # the features this step leaves out: refused on both objects
            live = next(v for v in range(fresh.nreads()) if fresh.read_nblock(v) > 0)
            for b in (fresh, refilled):
                with pytest.raises(B.FFHipError):
                    getattr(b, {"RUN_ADAPTERS": "adapters", "RUN_EVENTS": "events"}[name])(live)
        seen.add(B, fresh, step, inp, S.feature_flags(B, step, nbase, extra))
        held.append(refilled.device_bytes())
        fresh.close()
        if n == 0:
            first = got
    assert not S.differences(got, first), "the last F1 equals the first"
    # memory: never less, more after F3 than after F1 (a workspace grew after it had shrunk), and no more when the last step is repeated
    assert held == sorted(held) and held[2] > held[0], held
    _step(B, [refilled], form, S.STEPS[0], [fills[0]], shared, nbase, extra)
    assert refilled.device_bytes() == held[-1], (held, refilled.device_bytes())
    assert not S.differences(S.states(B, refilled, form), first)
    refilled.close()
    shared.close()
    dm.close()
    seen.check(reruns=(kind != M.NET_GRUMOD5), map0=(kind != M.NET_GRUMOD5))


LIGHT = tuple(n for n in S.FLIPFLOP if n not in ("transitions", "posterior", "trace"))


@pytest.mark.parametrize("form", ["pair", "pair256"])
def test_refilled_pair_equals_a_fresh_pair(B, engine, form):
    """pair: two row batches of 16 x 1500 at H = 384, the shape test_map_gpu.py gives ffhip_batch_run_pair -- which runs batches of one read tile one after the
    other (a paired layer launch takes 15 or 16 read tiles a batch: split_pair_ok), so `paired()` is held equal there and no more.  pair256: two batches of
    256 x 1000, whose layers do run as one launch; the big per-block arrays are left out of its states (LIGHT)"""
    nbase, big = 4, form == "pair256"
    names = LIGHT if big else S.FLIPFLOP
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 384, seed=2))
    fills = [S.fillings(form, 31), S.fillings(form, 32)]                     # one set a batch of the pair
    shared = S.Shared(B, engine, _plain_calls(B, dm, form, [[fills[0][k], fills[1][k]] for k in range(2)], nbase)[:64])
    pair = [S.make_batch(B, dm, form) for _ in range(2)]
    for k in (0, 1):
        step = S.STEPS[k]
        fresh = [S.make_batch(B, dm, form) for _ in range(2)]
        _step(B, fresh, form, step, [fills[0][k], fills[1][k]], shared, nbase)
        _step(B, pair, form, step, [fills[0][k], fills[1][k]], shared, nbase)
        assert all(b.paired() == big for b in fresh + pair), [b.paired() for b in fresh + pair]
        for j in range(2):
            want, got = S.states(B, fresh[j], form, names), S.states(B, pair[j], form, names)
            assert not S.differences(got, want), ("step", k, "batch", j, S.differences(got, want)[:8])
            assert pair[j].f32_reruns() == fresh[j].f32_reruns() == k, (k, j)          # F2's outlier, one read a batch
            live = [v for v in range(fresh[j].nreads()) if fresh[j].read_nblock(v)]
            assert 2 * sum(fresh[j].truth(v)["status"] == 1 for v in live) >= len(live) > 0
        for b in fresh:
            b.close()
    for b in pair:
        b.close()
    shared.close()
    dm.close()


@pytest.mark.parametrize("form", ["rows", "packed"])
def test_two_objects_in_flight_equal_the_serial_fresh_ones(B, engine, form):
    """The CLI's pipeline: run A(F1), run B(F2), finish A, fill A with F3 while B is not finished, run A, finish B, fill B ... for two rounds.  The setters stand
    where flappie_cli.c's batch_run has them -- behind the signals, in front of the run -- so the inputs come from the serial pass."""
    nbase = 4
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    fills = S.fillings(form, 21)
    shared = S.Shared(B, engine, _plain_calls(B, dm, form, [[f] for f in fills], nbase))
    want, inps, reruns = [], [], []
    for step in S.STEPS:
        fresh = S.make_batch(B, dm, form)
        inps.append(_step(B, [fresh], form, step, [fills[step["fill"]]], shared, nbase)[0])
        want.append(S.states(B, fresh, form))
        reruns.append(fresh.f32_reruns())
        fresh.close()
    assert reruns[1] >= 1 and reruns[0] == reruns[2] == 0, reruns
    jobs = [0, 1, 2, 0, 1, 2]                               # object j % 2 takes job j: A sees F1, F3, F2 and B sees F2, F1, F3
    objs = [S.make_batch(B, dm, form) for _ in range(2)]

    def submit(j):
        b, step = objs[j % 2], S.STEPS[jobs[j]]
        S.fill(b, form, fills[step["fill"]])
        S.apply_setters(B, b, step, inps[jobs[j]], shared, nbase)
        b.run(1.0, S.feature_flags(B, step, nbase))
    submit(0)
    submit(1)
    for j in range(len(jobs)):
        b = objs[j % 2]
        b.finish()
        got = S.states(B, b, form)
        assert not S.differences(got, want[jobs[j]]), ("job", j, S.differences(got, want[jobs[j]])[:8])
        assert b.f32_reruns() == reruns[jobs[j]], ("job", j)
        if j + 2 < len(jobs):
            submit(j + 2)                                   # (the other object is between its run and its finish)
    for b in objs:
        b.close()
    shared.close()
    dm.close()


def test_pileup_fed_by_a_refilled_batch_equals_one_fed_by_fresh_ones(B, engine):
    form, nbase = "rows", 4
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5, 128, seed=1))
    fills = S.fillings(form, 41)
    shared = S.Shared(B, engine, _plain_calls(B, dm, form, [[f] for f in fills], nbase))
    piles = [B.Pileup(engine, shared.ref, min_identity=930) for _ in range(2)]
    fl = S.base_flags(B, nbase) | B.RUN_MAP | B.RUN_TRUTH | B.RUN_PILEUP
    names = ("basecall", "map", "truth")
    refilled = S.make_batch(B, dm, form)
    for n, k in enumerate(S.SEQUENCE):
        step = S.STEPS[k]
        fresh = S.make_batch(B, dm, form)
        for b, pile in ((refilled, piles[0]), (fresh, piles[1])):
            S.fill(b, form, fills[step["fill"]])
            b.set_map(shared.ref, *step["map"])
            b.set_truth_from_map(True, step["truth_band"])
            b.set_pileup(pile)
            _run([b], fl)
        want, got = S.states(B, fresh, form, names), S.states(B, refilled, form, names)
        assert not S.differences(got, want), ("step", n, S.differences(got, want)[:8])
        assert refilled.f32_reruns() == fresh.f32_reruns() == (1 if k == 1 else 0)
        piles[1].download()                                 # (the fresh batch's accumulation is done before the batch goes)
        fresh.close()
    (ca, ta), (cb, tb) = piles[0].download(), piles[1].download()
    refilled.close()
    print("pileup totals", tb)
    assert ta == tb and np.array_equal(ca, cb)
    live = sum(1 for k in S.SEQUENCE for x in fills[S.STEPS[k]["fill"]] if x.size)
    assert tb["reads"] >= live // 2 and tb["skipped"] >= 1 and tb["reads"] + tb["skipped"] <= live, (tb, live)      # min_identity did set reads aside
    assert int(cb.sum()) > 0
    for p in piles:
        p.close()
    shared.close()
    dm.close()


def _rle_state(B, b, v, posterior):
    """a read of the run-length model: its qpath is NaN behind the first entry and has none there (decode_crf_runlength makes none), so entry 0 is left out"""
    out = {}
    for name, get in (("read_nblock", lambda: b.read_nblock(v)), ("score", lambda: np.float32(b.score(v))), ("path", lambda: b.path(v)[0]), ("qpath", lambda: b.path(v)[1][1:]),
                      ("transitions", lambda: b.transitions(v)), ("posterior", (lambda: b.posterior(v)) if posterior else (lambda: None)), ("rle_runs", lambda: b.rle_runs(v))):
        try:
            out[name] = S._blob(get())
        except B.FFHipError as e:
            out[name] = b"refused: " + str(e).encode()
    return out


@pytest.mark.parametrize("form", ["rows", "packed"])
def test_refilled_runlength_batch_equals_a_fresh_one(B, engine, form):
    dm = B.DeviceModel(engine, M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=2))
    fills = S.fillings(form, 51)
    refilled = S.make_batch(B, dm, form)
    first, held, nruns, reruns = None, [], 0, []
    for n, k in enumerate(S.SEQUENCE):
        step = S.STEPS[k]
        fl = 0
        for name in step["rle"]:
            fl |= getattr(B, name)
        fresh = S.make_batch(B, dm, form)
        for b in (fresh, refilled):
            S.fill(b, form, fills[step["fill"]])
            b.set_run_scale(step["scale"] or B.RLE_SCALE_DEFAULT)
            _run([b], fl)
        post = not fl & B.RUN_VITERBI_ONLY
        want, got = [[_rle_state(B, b, v, post) for v in S.slots(b, form)] for b in (fresh, refilled)]
        assert not S.differences(got, want), ("step", n, S.differences(got, want)[:8])
        assert refilled.f32_reruns() == fresh.f32_reruns()
        reruns.append(fresh.f32_reruns())
        live = [v for v in range(fresh.nreads()) if fresh.read_nblock(v) > 0]
        nruns += sum(fresh.rle_runs(v)["base"].size for v in live)
        assert (fresh.rle_runs(live[0])["shape"] is not None) == bool(fl & B.RUN_RLE_RECORDS)
        held.append(refilled.device_bytes())
        fresh.close()
        if n == 0:
            first = got
    assert not S.differences(got, first), "the last F1 equals the first"
    assert held == sorted(held), held
    assert nruns > 1000 and reruns[1] >= 1 and reruns[0] == reruns[2] == reruns[3] == 0, (nruns, reruns)
    refilled.close()
    dm.close()


# ------------------------------------------------------------------------------------ the binary across chunks
def _flappie(cli, model, batch, args, debug=None):
    from test_cli import FLAPPIE
    env = dict(cli["env"], **({"FLAPPIE_DEBUG": debug} if debug else {}))
    r = subprocess.run([FLAPPIE, "--model", model, "--batch", str(batch)] + args + [str(cli["reads"])], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout, r.stderr


def _batches(err):
    """(batches, packed ones) of a run, from the timing lines the binary prints"""
    m = re.search(r"^batches: (\d+) \((\d+) of them packed\)", err, re.M)
    assert m, err[-2000:]
    return int(m.group(1)), int(m.group(2))


def _write_reads(d, lens, seed):
    from test_cli import synth_raw, write_fast5
    reads = d / "reads"
    reads.mkdir()
    rng = np.random.default_rng(seed)
    for i, n in enumerate(lens):
        write_fast5(reads / ("read_%03d.fast5" % i), "uuid-%04d" % i, synth_raw(rng, int(n)))
    return reads


def _feature_files(d, calls, letters):
    """what the options read, made from the directory's own calls {name: call}: two kits, a reference of the calls with 5 % edits on alternating strands (four
    reads left out), truths (the calls with edits; one read without, one bad record), sequences (the calls; one read without, one bad record) and variants"""
    from test_barcodes_gpu import planted_kit
    rng = np.random.default_rng(5)
    names = sorted(calls)
    plain = {nm: calls[nm].replace("Z", "C") for nm in names}
    (d / "barcodes.fa").write_text("".join(">bc%02d\n%s\n" % (k + 1, p) for k, p in enumerate(planted_kit(rng, [calls[nm] for nm in names]))))
    ads = [S.mutate(rng, plain[names[0]][4:32], 1), S.mutate(rng, S.MR.revcomp(plain[names[1]][-30:-2]), 2), plain[names[2]][100:128], S.rand_seq(rng, 28)]
    (d / "adapters.fa").write_text("".join(">ad%02d\n%s\n" % (k + 1, p) for k, p in enumerate(ads)))
    recs = ["", "", ""]
    for i, nm in enumerate(names[:-4]):
        x = S.MR.edit(rng, plain[nm], 0.05)
        recs[i % 3] += S.rand_seq(rng, 100 + 31 * (i % 7)) + (x if i % 2 == 0 else S.MR.revcomp(x))
    (d / "ref.fa").write_text("".join(">rec%d\n%s\n" % (k, r + S.rand_seq(rng, 150)) for k, r in enumerate(recs)))
    (d / "truths.fa").write_text("".join(">%s\n%s\n" % (nm, "ACGNT" if i == 2 else S.MR.edit(rng, plain[nm], 0.08)) for i, nm in enumerate(names) if i != 1))
    (d / "seqs.fa").write_text("".join(">%s\n%s\n" % (nm, calls[nm][:3] + "N" + calls[nm][3:] if i == 4 else calls[nm]) for i, nm in enumerate(names) if i != 3))
    lines = ["# name\tpos\tref\talt"]
    for i, nm in enumerate(names):
        s = calls[nm]
        if i in (3, 4) or i % 5 == 0 or len(s) < 40:             # (no sequence, a bad one, and reads without variants)
            continue
        for p in sorted(int(x) for x in rng.choice(len(s) - 3, 5, replace=False)):
            kind = int(rng.integers(0, 4))
            ref, alt = ((s[p], letters[(letters.index(s[p]) + 1) % len(letters)]) if kind == 0 else ("-", s[p] * 12) if kind == 1 else (s[p:p + 2], "-") if kind == 2
                        else (s[p:p + 3], s[p:p + 3][::-1]))
            lines.append("%s\t%d\t%s\t%s" % (nm, p, ref, alt))
    (d / "vars.tsv").write_text("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """about 40 synthetic reads of 1500 .. 4000 samples, the two H = 128 models, and every file the feature options read, from a default run's calls"""
    from test_barcodes_gpu import _records
    from test_cli import FAST5LIB, FLAPPIE, TOOL
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    d = tmp_path_factory.mktemp("refill_cli")
    M.write_mdl(str(d / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=9, ident="r941native"))
    M.write_mdl(str(d / "flipflop_r941native5mC.h"), M.synthetic_model(M.NET_GRUMOD5, 128, seed=9, ident="r941native5mC"))
    out = {"dir": d, "reads": _write_reads(d, np.random.default_rng(3).integers(1500, 4000, 40), 4), "env": dict(os.environ, FLAPPIE_MODEL_DIR=str(d), FLAPPIE_CLI_TIMING="1")}
    for model, letters in (("r941_native", "ACGT"), ("r941_5mC", "ACGTZ")):
        sub = d / model
        sub.mkdir()
        recs = _records(_flappie(out, model, 64, ["--format", "fastq"])[0], "fastq")
        assert len(recs) == 40
        _feature_files(sub, {r[0]: r[1] for r in recs}, letters)
    return out


def _chunked_equals_one_chunk(cli, model, options, outputs, tag):
    """the option set with --batch 4 (chunks of 16 reads, groups of 4: the cached objects are filled again about ten times) and with --batch 64 (one chunk): the
    same stdout, the same bytes in every output file"""
    got = {}
    for batch in (4, 64):
        sub = cli["dir"] / ("%s_b%d" % (tag, batch))
        sub.mkdir()
        args = [str(cli["dir"] / model / a[1:]) if a.startswith("@") else str(sub / a[1:]) if a.startswith("=") else a for a in options]
        stdout, err = _flappie(cli, model, batch, args)
        got[batch] = (stdout, {name: (sub / name).read_bytes() for name in outputs}, _batches(err)[0])
    assert got[4][2] >= 10 > got[64][2] >= 1, (got[4][2], got[64][2])                # the chunked run did go in many batches
    assert got[4][0] == got[64][0] and got[4][0].count("\n") >= 40, tag
    for name in outputs:
        assert got[4][1][name] == got[64][1][name] and len(got[64][1][name]) > 0, (tag, name)
    return got[64]


def test_flappie_in_chunks_barcodes_adapters_map_pileup_polytail_remap_events(cli):
    stdout, files, _ = _chunked_equals_one_chunk(cli, "r941_native", [
        "--format", "sam", "--emit-moves", "--barcodes", "@barcodes.fa", "--adapters", "@adapters.fa", "--poly-tail", "--poly-tail-min-calls", "0", "--poly-tail-min-bases", "5",
        "--map", "@ref.fa", "--map-out", "=hits.tsv", "--map-records", "=recs.fa", "--truth-from-map", "--truth-out", "=acc.tsv", "--map-sam", "=aln.sam",
        "--map-pileup", "=pileup.tsv", "--map-pileup-min-identity", "900", "--remap", "@seqs.fa", "--remap-out", "=remap.tsv", "--remap-events", "=events.tsv"],
        ("hits.tsv", "recs.fa", "acc.tsv", "aln.sam", "pileup.tsv", "remap.tsv", "events.tsv"), "all")
    assert "mv:B:c" in stdout and "pt:i:" in stdout and files["acc.tsv"].count(b"\n") >= 20 and files["events.tsv"].count(b"\n") > 1000


def test_flappie_in_chunks_truth(cli):
    _, files, _ = _chunked_equals_one_chunk(cli, "r941_native", ["--format", "fastq", "--truth", "@truths.fa", "--truth-out", "=acc.tsv", "--truth-band", "64"], ("acc.tsv",), "truth")
    assert files["acc.tsv"].count(b"\n") >= 30


def test_flappie_in_chunks_5mC_mods_variants_moves_and_tags(cli):
    stdout, files, _ = _chunked_equals_one_chunk(cli, "r941_5mC", [
        "--format", "sam", "--emit-moves", "--modbase-tags", "--remap", "@seqs.fa", "--remap-out", "=remap.tsv", "--remap-mods", "=mods.tsv",
        "--remap-variants", "@vars.tsv", "--remap-variants-out", "=calls.tsv", "--remap-events", "=events.tsv"],
        ("remap.tsv", "mods.tsv", "calls.tsv", "events.tsv"), "5mC")
    assert "MM:Z:" in stdout and "ML:B:C" in stdout and "mv:B:c" in stdout and files["calls.tsv"].count(b"\n") >= 50 and files["mods.tsv"].count(b"\n") >= 100


def test_flappie_packed_path_in_chunks(tmp_path):
    """a directory of mixed lengths, as test_cli_packs_a_directory_of_mixed_lengths has it: the chunks go in packed batches, whose cached objects (pack_cache) are
    filled again chunk after chunk; with features on, against one chunk"""
    from test_barcodes_gpu import _records
    from test_cli import FAST5LIB, FLAPPIE, TOOL
    if not (os.path.exists(FLAPPIE) and os.path.exists(TOOL) and os.path.exists(FAST5LIB)):
        pytest.skip("libhdf5 not found when the host layer was built")
    M.write_mdl(str(tmp_path / "flipflop5_r941native.h"), M.synthetic_model(M.NET_LSTM5, 128, seed=1, ident="r941native"))
    rng = np.random.default_rng(2)
    lens = np.clip(np.exp(np.log(1200) + 0.9 * rng.standard_normal(140)), 700, 8000).astype(int)
    cli = {"dir": tmp_path, "reads": _write_reads(tmp_path, lens, 6), "env": dict(os.environ, FLAPPIE_MODEL_DIR=str(tmp_path), FLAPPIE_CLI_TIMING="1")}
    recs = _records(_flappie(cli, "r941_native", 64, ["--format", "fastq"])[0], "fastq")
    sub = tmp_path / "r941_native"
    sub.mkdir()
    _feature_files(sub, {r[0]: r[1] for r in recs}, "ACGT")
    got = {}
    for batch in (4, 64):
        out = tmp_path / ("b%d" % batch)
        out.mkdir()
        stdout, err = _flappie(cli, "r941_native", batch, ["--format", "sam", "--emit-moves", "--barcodes", str(sub / "barcodes.fa"), "--map", str(sub / "ref.fa"), "--map-out", str(out / "hits.tsv"),
                                                           "--truth-from-map", "--truth-out", str(out / "acc.tsv"), "--remap", str(sub / "seqs.fa"), "--remap-out", str(out / "remap.tsv"),
                                                           "--remap-events", str(out / "events.tsv")], debug="pack_log")
        made = len(re.findall(r"^packed batch object \(slot", err, re.M))
        packed = len(re.findall(r"^packed batch \d+ \(submitted", err, re.M))
        assert packed == _batches(err)[1], err[-2000:]
        got[batch] = (stdout, [(out / name).read_bytes() for name in ("hits.tsv", "acc.tsv", "remap.tsv", "events.tsv")], packed, made)
    # the chunked run took the packed path, in more than one chunk, and filled the objects it had made again
    assert got[4][2] >= 3 and got[4][2] > got[4][3] >= 1, got[4][2:]
    assert got[4][0] == got[64][0] and got[4][1] == got[64][1] and all(len(x) > 0 for x in got[64][1])


def test_truth_bench_runs_to_its_end():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "truth_bench.py"), "--steps", "2", "--warmup", "2", "--runs", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["aligned"] > 0 and out["paired"] is True, out
