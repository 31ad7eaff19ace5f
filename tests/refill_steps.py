"""What tests/test_refill_gpu.py applies to a batch object that is filled again and to a fresh one of the same shape: the fillings, the settings and flags of
every step, the per-read inputs built from a filling's own calls, the setter calls in the order `flappie` makes them (flappie_cli.c batch_run), and a read's
state -- everything the batch returns for it, as bytes.

A step is (filling, settings, flags).  STEPS holds three; the sequence on one object is SEQUENCE: F1, F2, F3 and F1 again with its own settings.
  * F1: every slot holds a read of 0.4 .. 1 of the capacity, one of exactly the capacity (packed: 24 reads).
  * F2: fewer and shorter: slots 0, 7 and the last are empty, the others hold 19 .. 800 samples (19 is the shortest legal read), one holds the capacity, one carries
    an outlier sample that sends it through the f32 re-run (packed: 5 reads, so rows without a read; the longest is 16 samples short of a row, which takes a dead
    block behind its last read).  Its inputs change status, form and size (inputs()).
  * F3: more and longer: 2/3 .. 1 of the capacity (packed: as many reads as the object takes), truth in the from-map mode.
No assertion here compares anything with a tolerance: a state is bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import map_ref as MR  # noqa: E402
import variants_ref as V  # noqa: E402
from make_annot_copies import _blob  # noqa: E402
from test_barcodes_gpu import mutate, rand_seq  # noqa: E402
from test_polytail_gpu import RUN_A, RUN_B  # noqa: E402
from test_variants_gpu import _variants  # noqa: E402

OUTLIER = 6.0e4
LETTERS = "ACGTZ"
SHAPES = {"rows": dict(nread=16, nsample=3000, max_reads=0), "packed": dict(nread=8, nsample=4000, max_reads=40), "pair": dict(nread=16, nsample=1500, max_reads=0),
          "pair256": dict(nread=256, nsample=1000, max_reads=0)}
EMPTY = (0, 7, -1)                 # F2's empty slots (one read a row): the first, an interior one, the last
SHORT_SEED = 11                    # the packed fillings of this seed hold the 19-sample read every F2 has (fillings())
SCALE_B = (1.1, 0.95, 1.3, 1.07)   # run-length model: another set of scale factors

# truth band, remap band, variants (context, all paths), site mods (context, all paths), map (window, max_error), barcodes (kit, max_dist, min_sep, both_ends),
# adapters (kit, max_dist), poly tail parameters, truth from map, the feature flags left out, the inputs that change status (inputs()); run-length model: flags, scale
STEPS = (
    dict(fill=0, truth_band=512, remap_band=2048, var=(10, False), mods=(15, False), map=(-1, -1), bc=(0, -1, -1, False), ad=(0, -1), pt=RUN_A, from_map=False,
         drop=(), special=False, rle=("RUN_RLE_RECORDS",), scale=None),
    dict(fill=1, truth_band=16, remap_band=8, var=(23, True), mods=(0, True), map=(64, 100), bc=(1, 6, 2, True), ad=(1, 5), pt=RUN_B, from_map=False,
         drop=("RUN_ADAPTERS", "RUN_EVENTS"), special=True, rle=("RUN_RLE_RUNS",), scale=SCALE_B),
    dict(fill=2, truth_band=1279, remap_band=2048, var=(1, False), mods=(31, False), map=(128, 200), bc=(0, -1, -1, False), ad=(0, -1), pt=dict(from_end=1, window=4),
         from_map=True, drop=(), special=False, rle=("RUN_RLE_RECORDS", "RUN_VITERBI_ONLY"), scale=None),
)
SEQUENCE = (0, 1, 2, 0)


def make_batch(B, dm, form):
    s = SHAPES[form]
    return B.Batch(dm, s["nread"], s["nsample"], max_reads=s["max_reads"])


def fillings(form, seed):
    """[F1, F2, F3]: a list of float32 signals each (an empty array: an empty slot)"""
    rng = np.random.default_rng(seed)
    cap = SHAPES[form]["nsample"]

    def sigs(lens):
        return [rng.standard_normal(int(n)).astype(np.float32) for n in lens]
    if form == "packed":
        f1 = sigs(rng.integers(400, 1401, 24))
        f2 = sigs([19, cap - 16, 700, 300, 500])
        f2[2][200] = OUTLIER
        f3 = sigs(rng.integers(300, 701, SHAPES[form]["max_reads"]))
        return [f1, f2, f3]
    nread = SHAPES[form]["nread"]
    l1 = [int(x) for x in rng.integers(2 * cap // 5, cap + 1, nread)]
    l1[5] = cap
    l2 = [int(x) for x in rng.integers(19, 801, nread)]
    l2[3], l2[9], l2[11] = 19, cap, 600
    for e in EMPTY:
        l2[e] = 0
    l3 = [int(x) for x in rng.integers(2 * cap // 3, cap + 1, nread)]
    f1, f2, f3 = sigs(l1), sigs(l2), sigs(l3)
    f2[11][200] = OUTLIER
    f2[3] = fillings("packed", SHORT_SEED)[1][0]           # the 19-sample read of the packed F2 (seed SHORT_SEED): the LSTM model calls no base on it
    return [f1, f2, f3]


def fill(b, form, sigs):
    if form == "packed":
        slot, off = b.pack_plan([x.size for x in sigs])
        assert min(slot) >= 0, "every read of the filling is placed"
        b.set_signals_packed(sigs, slot, off)
        return slot
    b.set_signals_ragged(sigs)
    return list(range(len(sigs)))


def slots(b, form):
    """every index the accessors are asked for: the object's slots, and for a packed object every read it could take (a read it held before and does not hold
    now is refused like an empty slot)"""
    return range(SHAPES[form]["max_reads"] or b.nread)


def base_flags(B, nbase, extra=0):
    """a run "without feature flags": the block's own sections only"""
    return extra | B.RUN_MOVES | (B.RUN_MOD_PROBS if nbase == 5 else 0)


def feature_flags(B, step, nbase, extra=0):
    fl = base_flags(B, nbase, extra) | B.RUN_BARCODES | B.RUN_ADAPTERS | B.RUN_MAP | B.RUN_POLYTAIL | B.RUN_TRUTH | B.RUN_REMAP | B.RUN_EVENTS | B.RUN_REMAP_VARIANTS
    if nbase == 5:
        fl |= B.RUN_REMAP_MODS
    for name in step["drop"]:
        fl &= ~getattr(B, name)
    return fl


def codes_of(call):
    return np.array([LETTERS.index(c) for c in call], np.uint8)


def calls_of(b):
    """{read: call} of the live reads of a finished batch"""
    return {v: b.basecall(v) for v in range(b.nreads()) if b.read_nblock(v) > 0}


def reference(rng, calls):
    """random filler and the calls with 5 % edits on alternating strands, in three records; every seventh call is left out (its read is not mapped)"""
    recs = ["", "", ""]
    for i, c in enumerate(calls):
        if i % 7 == 3 or not c:
            continue
        x = MR.edit(rng, c.replace("Z", "C"), 0.05)
        recs[i % 3] += rand_seq(rng, 60 + 37 * (i % 5)) + (x if i % 2 == 0 else MR.revcomp(x))
    return [r + rand_seq(rng, 200) for r in recs]


def kit_patterns(rng, calls):
    """two barcode kits (another number and length of patterns: 9 of 24 bases, 5 of 40 and 70: two words) and two adapter kits, cut from the longest calls"""
    good = [c.replace("Z", "C") for c in sorted(calls, key=len, reverse=True)[:8]]
    assert len(good) == 8 and len(good[-1]) >= 40, [len(c) for c in good]

    def cut(s, a, n, nedit):
        return (mutate(rng, s[a:a + n], nedit) or "ACGT")[:128]
    bc0 = [cut(p, 3, 24, j % 3) for j, p in enumerate(good[:4])] + [cut(MR.revcomp(p), 2, 24, j % 3) for j, p in enumerate(good[4:])] + [rand_seq(rng, 24)]
    bc1 = [cut(p, 0, 40, 2) for p in good[:3]] + [rand_seq(rng, 40), (good[3] + rand_seq(rng, 70))[:70]]
    ad0 = [cut(p, len(p) // 2, 12, 1)[:64] for p in good[:4]]
    ad1 = [cut(p, 10, 28, 2)[:64] for p in good[4:6]]
    return (bc0, bc1), (ad0, ad1)


class Shared:
    """the objects created once, up front: the reference from the calls of all fillings, two barcode kits, two adapter kits"""

    def __init__(self, B, engine, calls, seed=5):
        rng = np.random.default_rng(seed)
        self.records = reference(rng, calls)
        (bc0, bc1), (ad0, ad1) = kit_patterns(rng, calls)
        self.ref = B.MapRef(engine, self.records)
        self.bc = (B.Barcodes(engine, bc0, 150), B.Barcodes(engine, bc1, 60))
        self.ad = (B.Adapters(engine, ad0), B.Adapters(engine, ad1))

    def close(self):
        for x in self.bc + self.ad + (self.ref,):
            x.close()


def inputs(step, b, nbase, seed=0):
    """the per-read inputs of a step from the finished batch's own calls: (truths, sequences, variants), one entry a read of the batch.
    By default a read's truth is its call with 5 % edits, its sequence its call, its variants those of test_variants_gpu.  A `special` step (F2) has, among its
    live reads: a truth None, an empty one, one of one base, one four times the call; a sequence None, one of N + 2 codes (it cannot be mapped: status 2), one
    without C or Z (no sites); no variants for the first two reads and for those without a sequence"""
    n = b.nreads()
    live = [v for v in range(n) if b.read_nblock(v) > 0]
    rng = np.random.default_rng(100 + seed)
    truths, seqs, vars = [None] * n, [None] * n, [None] * n
    for v in live:
        call = b.basecall(v)
        q = codes_of(call) if call else np.array([1], np.uint8)
        seqs[v] = q
        truths[v] = codes_of(MR.edit(rng, call.replace("Z", "C"), 0.05) if call else "A")
    if step["special"]:
        assert len(live) >= 5
        one = min(live, key=b.read_nblock)                  # (the shortest read: a band of 16 leaves a truth of one base no path to a call of more than 32)
        a, e, four = [v for v in live if v != one][:3]
        truths[a], truths[e], truths[one], truths[four] = None, np.zeros(0, np.uint8), truths[one][:1], np.tile(seqs[four], 4)
        none, long, plain = live[-1], live[-2], live[-3]
        seqs[none] = None
        seqs[long] = rng.integers(0, nbase, b.read_nblock(long) + 2).astype(np.uint8)
        seqs[plain] = np.where((seqs[plain] == 1) | (seqs[plain] == 4), 0, seqs[plain]).astype(np.uint8)
    for v in live:
        if seqs[v] is not None and not (step["special"] and v in live[:2]):
            vars[v] = V.pack(_variants(np.random.default_rng(1000 + v), seqs[v], nbase, 3))
    return truths, seqs, vars


def apply_setters(B, b, step, inp, shared, nbase, pileup=None):
    """the setter calls of flappie_cli.c's batch_run, in its order, behind the signals and in front of the run"""
    truths, seqs, vars = inp
    kit, max_dist, min_sep, both = step["bc"]
    b.set_barcodes(shared.bc[kit], max_dist, min_sep, both)
    b.set_adapters(shared.ad[step["ad"][0]], step["ad"][1])
    b.set_map(shared.ref, *step["map"])
    b.set_polytail(**step["pt"])
    b.set_remap(seqs, step["remap_band"])
    if nbase == 5:
        b.set_remap_mods(*step["mods"])
    b.set_remap_variants(vars, *step["var"])
    if step["from_map"]:
        b.set_truth_from_map(True, step["truth_band"])
    else:
        b.set_truth(truths, step["truth_band"])
    if pileup is not None:
        b.set_pileup(pileup)


def forms_of(B, b, step, inp):
    """({read: truth form}, {read: remap form}): the kernel form every read with status 1 on the host's side takes in this step, as the library's own queries
    give it (ffhip_debug_truth_form of min(2 band + 1, blocks + 2), ffhip_debug_remap_form of the sequence's length and the band)"""
    truths, seqs, _ = inp
    tf, rf = {}, {}
    for v in range(b.nreads()):
        N = b.read_nblock(v)
        if N == 0:
            continue
        if step["from_map"] or (truths[v] is not None and truths[v].size):
            tf[v] = B.truth_form(min(2 * step["truth_band"] + 1, N + 2))
        if seqs[v] is not None and 1 <= seqs[v].size <= N + 1:
            rf[v] = int(B.lib().ffhip_debug_remap_form(int(seqs[v].size), int(step["remap_band"])))
    return tf, rf


FLIPFLOP = ("basecall", "quality", "score", "path", "read_nblock", "transitions", "posterior", "trace", "moves", "mod_probs", "barcode", "adapters", "map",
            "polytail", "truth", "remap", "events", "site_mods", "variant_calls")


def state(B, b, v, names=FLIPFLOP):
    """everything the batch returns for slot v, as bytes; an accessor that raises contributes the text of its error"""
    out = {}
    for name in names:
        try:
            out[name] = _blob(getattr(b, name)(v))
        except B.FFHipError as e:
            out[name] = b"refused: " + str(e).encode()
    return out


def states(B, b, form, names=FLIPFLOP):
    return [state(B, b, v, names) for v in slots(b, form)]


def differences(got, want):
    """[(slot, accessor)] where two lists of states differ"""
    assert len(got) == len(want)
    return [(v, k) for v, (g, w) in enumerate(zip(got, want)) for k in w if g[k] != w[k]]
