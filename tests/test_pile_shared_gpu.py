"""The four run-wide accumulators on the same alignments (include/ffhip.h "pileup", "mod pileup", "consensus", "error profile"; the kernels k_pileup, k_modpileup,
k_consensus and k_errprofile).  They take their reads through one gate and walk their ops with one scan (flappie_amd/csrc/ffhip_pile.hpp), so totals that name the
same thing in two objects are equal whatever each object does with an op.

The alignments: op counts at the wave and chunk edges of the scan (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513), each as all '=', all 'D', 'I' at both edges and a
seeded mix -- the kinds of test_pileup_gpu.operator_cases -- on both strands, at either end of a record of that test's reference, through ffhip_op_pileup,
ffhip_op_consensus, ffhip_op_errprofile_mapped and ffhip_op_modpileup into four fresh objects; once with min_identity 0 and once with one that skips some of the mixes.

The identities hold in pileup_ref.py, consensus_ref.py, errprofile_ref.py and modpileup_ref.py on the same alignments (the references are walked here too, which
takes no GPU: `identities` is applied to their totals first).  Integers: no tolerance."""
import numpy as np
import pytest

import consensus_ref as CO
import errprofile_ref as EP
import modpileup_ref as MP
import pileup_ref as PU
from test_barcodes_gpu import rand_seq
from test_pileup_gpu import LENS

pytestmark = pytest.mark.gpu

OP_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)
MIN_IDENTITY = 550                                             # per mille: a mix holds 55 % matches on average, so some mixes pass and some do not


def alignments(rng):
    """(kind, q, tstart, tend, call, qual, ml, ops): every op count in four kinds, on both strands, at either end of the shortest record that holds the span"""
    out = []
    for K in OP_COUNTS:
        mix = rng.choice(4, size=K, p=(0.55, 0.15, 0.15, 0.15)).astype(np.uint8)
        if (mix != 2).sum() == 0:
            mix[int(rng.integers(0, K))] = 0
        kinds = {"=": np.zeros(K, np.uint8), "D": np.full(K, 3, np.uint8), "mix": mix,
                 "I..I": np.array([2] + [0] * (K - 2) + [2], np.uint8) if K >= 3 else np.array([2, 0, 2], np.uint8)}      # (fewer than 3 ops: 'I' around one '=')
        for kind, ops in kinds.items():
            m, n = int((ops != 2).sum()), int((ops != 3).sum())
            k = min((k for k, Mk in enumerate(LENS) if Mk >= m), key=lambda k: LENS[k])
            for o in (0, 1):
                for at_end in (0, 1):
                    ts = LENS[k] - m if at_end else 0
                    call = "".join("ACGTZ"[int(x)] for x in rng.integers(0, 5, n))
                    qual = bytes(int(x) for x in rng.integers(33, 127, n))
                    ml = rng.integers(0, 256, n).astype(np.uint8)
                    out.append((kind, 2 * k + o, ts, ts + m, call, qual, ml, ops))
    return out


def identities(pu, co, ep, mo, where):
    """what must hold among the four objects' totals (dicts) after the same alignments"""
    for name in ("reads", "skipped"):
        assert pu[name] == co[name] == ep[name] == mo[name], (where, name, pu[name], co[name], ep[name], mo[name])
    for name in ("match", "mismatch", "del", "ins", "edge_ins"):
        assert pu[name] == ep[name], (where, name, pu[name], ep[name])
    assert co["bases"] == pu["match"] + pu["mismatch"] and co["del"] == pu["del"], (where, co, pu)
    assert co["ins_bases"] + co["long_ins"] == pu["ins"] and co["edge_ins"] == pu["edge_ins"], (where, co, pu)
    assert mo["del"] + mo["mod"] + mo["canon"] + mo["fail"] + mo["diff"] == mo["sites"], (where, mo)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(77)
    return [rand_seq(rng, m) for m in LENS], alignments(rng)


@pytest.mark.parametrize("min_identity", (0, MIN_IDENTITY))
def test_the_four_objects_agree_on_what_they_share(cases, min_identity):
    from flappie_amd import binding as B
    recs, aln = cases
    # the Python references first: the identities are theirs too, and the cases do what they are meant to
    w_pu, w_co, w_ep, w_mo = PU.Pileup(LENS, min_identity), CO.Consensus(LENS, min_identity), EP.ErrProfile(min_identity), MP.ModPileup(LENS, recs, min_identity)
    mixes_skipped = 0
    for kind, q, ts, te, call, qual, ml, ops in aln:
        before = w_pu.totals["skipped"]
        w_pu.add(q, ts, te, call, ops)
        w_co.add(q, ts, te, call, ops)
        w_ep.add(call, qual, EP.mapped_truth(recs, q, ts, te), ops)
        w_mo.add(q, ts, te, call, ml, ops)
        mixes_skipped += (w_pu.totals["skipped"] - before) if kind == "mix" else 0
    identities(w_pu.totals, w_co.totals, w_ep.totals, w_mo.totals, "references")
    n_mix = sum(1 for a in aln if a[0] == "mix")
    assert w_pu.totals["reads"] + w_pu.totals["skipped"] == len(aln) and (0 < mixes_skipped < n_mix if min_identity else w_pu.totals["skipped"] == 0)
    assert min(w_pu.totals[k] for k in ("match", "mismatch", "del", "ins", "edge_ins")) > 0 and w_mo.totals["sites"] > 0

    engine = B.Engine(0)
    ref = B.MapRef(engine, recs)
    pu, co, ep, mo = B.Pileup(engine, ref, min_identity), B.Consensus(engine, ref, min_identity), B.ErrProfile(engine, min_identity), B.ModPileup(engine, ref, min_identity)
    for kind, q, ts, te, call, qual, ml, ops in aln:
        B.op_pileup(engine, pu, q, ts, te, call, ops)
        B.op_consensus(engine, co, q, ts, te, call, ops)
        B.op_errprofile_mapped(engine, ep, ref, q, ts, te, call, qual, ops)
        B.op_modpileup(engine, mo, q, ts, te, call, ml, ops)
    t_pu, t_co, t_ep, t_mo = pu.download()[1], co.download()[1], ep.download()[1], mo.download()[1]
    identities(t_pu, t_co, t_ep, t_mo, "objects")
    assert t_pu["reads"] == w_pu.totals["reads"] and t_pu["skipped"] == w_pu.totals["skipped"], (t_pu, w_pu.totals)
    for obj in (pu, co, ep, mo, ref, engine):
        obj.close()
