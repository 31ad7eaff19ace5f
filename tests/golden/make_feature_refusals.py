#!/usr/bin/env python3
"""tests/golden/feature_refusals.json: what the host side of the per-read features (barcodes, adapters, map, poly tail, remap, events, site mods, variants,
truth, truth from map, pileup) answers to a call it refuses -- [case, return code, ffhip_last_error text] -- recorded from the release library of the commit
BEFORE that host code moved into flappie_amd/csrc/ffhip_features.hip and its repeated checks became one helper each.  tests/test_feature_refusals_gpu.py
replays the same calls (record() below) on the library of its tree and holds it to these codes and texts exactly.

This script runs in a built checkout of that parent (copied to its tests/golden/: it imports the flappie_amd beside it) and needs a GPU:
usage: PARENT/tests/golden/make_feature_refusals.py [OUT.json]
It records twice and writes nothing if the two differ.

Every FFHIP_EINVAL of the features' run fronts, device objects, setters, accessors and single-read operators is called once through the C ABI with a live
engine, on the smallest shapes the refusal tests of the suite use (the 4-base LSTM5 model at H = 128, the 5-base GRUMOD5 model at H = 64, the run-length model
at H = 128, one batch of 4 x 1000 samples each, a kit of one 8-base pattern, a reference of one 8-base record).  Left out: FFHIP_ENOMEM and FFHIP_EHIP; the
refusals that only reads of 10^5 blocks or lists of 2^30 entries in memory reach (a batch's sites or variants beyond 2^30, a mapped stretch's bound beyond the
longest truth, a batch's bounds beyond 2^32 - 1); and four texts of the fronts that no call reaches: remap's and truth's window that no kernel form holds (the
setters refuse the sequence or the band first), variants set for another number of reads (remap's row refuses its own count first, and new sequences detach the
variants), and truth from map without a reference (the map's row stands first and refuses).  Sequences and truths set for another number of reads are reached
with one packed batch of the 4-base model, 4 x 1000 samples, filled with two reads and then with three.  A length beyond a limit is passed as a number: the call refuses it before it reads.  A case named "x+y"
breaks rule x and rule y at once: which of the two answers is part of the record.  A call that returns a pointer is recorded as 0 (NULL) or 1.  An accessor
that returns FFHIP_EINVAL for a null output writes no text: the text recorded is then that of the case before, which the replay has in the same order."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flappie_amd import binding as B  # noqa: E402
from flappie_amd import model as M  # noqa: E402

u8p, f32p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int)


_KEEP = []      # the arrays behind the pointers handed out below, for the life of the process


def _u8(a):
    a = np.ascontiguousarray(a, np.uint8)
    _KEEP.append(a)
    return a, a.ctypes.data_as(u8p)


def _strs(seqs):
    return (C.c_char_p * max(1, len(seqs)))(*seqs)


def _mat(a, nr, stride=None):
    """an ffhip_mat over `a` [nc][stride] of nr rows a column"""
    a = np.ascontiguousarray(a, np.float32)
    return a, B.CFMat(a.ctypes.data_as(f32p), nr, a.shape[0], stride or a.shape[1], None, None)


def _variants(rows):
    v = np.zeros(len(rows), B.VARIANT_DTYPE)
    for i, (pos, nref, alt) in enumerate(rows):
        v[i]["pos"], v[i]["nref"], v[i]["nalt"] = pos, nref, len(alt)
        v[i]["alt"][:len(alt)] = alt
    return v


def record(engine):
    """[[case, return code, text]] on the library the binding has loaded"""
    L = B.lib()
    out = []

    def case(name, rc):
        out.append([name, int(rc), L.ffhip_last_error().decode()])

    def ptr(name, fn, *args):
        h = fn(*args)
        case(name, 1 if h else 0)
        return h

    eng2 = B.Engine(engine.device)
    e, e2 = engine.h, eng2.h
    dms = {k: B.DeviceModel(engine, M.synthetic_model(kind, hidden, seed=1))
           for k, (kind, hidden) in {"lstm4": (M.NET_LSTM5, 128), "gru5": (M.NET_GRUMOD5, 64), "rle": (M.NET_LSTM5_RLE, 128)}.items()}
    sig = np.random.default_rng(7).standard_normal((4, 1000)).astype(np.float32)
    bs = {}
    for k, dm in dms.items():
        bs[k] = B.Batch(dm, 4, 1000)
        bs[k].set_signals(sig)
        bs[k].run(1.0, 0)
        bs[k].finish()
    b4, b5, br = bs["lstm4"].h, bs["gru5"].h, bs["rle"].h
    kit, kit2 = B.Barcodes(engine, [b"ACGTACGT"]), B.Barcodes(eng2, [b"ACGTACGT"])
    ad, ad2 = B.Adapters(engine, [b"ACGTACGT"]), B.Adapters(eng2, [b"ACGTACGT"])
    ref, ref_b, ref2 = B.MapRef(engine, [b"ACGTTGCA"]), B.MapRef(engine, [b"TTGCAACG"]), B.MapRef(eng2, [b"ACGTTGCA"])
    pile, pile_b, pile2 = B.Pileup(engine, ref), B.Pileup(engine, ref_b), B.Pileup(eng2, ref2)
    FL = {k: getattr(B, "RUN_" + k) for k in ("NO_DECODE", "BARCODES", "ADAPTERS", "MAP", "POLYTAIL", "TRUTH", "REMAP", "EVENTS", "REMAP_MODS", "REMAP_VARIANTS", "PILEUP")}

    def run(name, b, flags):
        """a run the front refuses leaves the batch as it was; one it takes is finished"""
        rc = L.ffhip_batch_run(b, 1.0, flags)
        case(name, rc)
        if rc == 0:
            L.ffhip_batch_finish(b)

    # ---- device objects
    ptr("barcodes_upload: null engine", L.ffhip_barcodes_upload, None, 1, _strs([b"ACGT"]), 150)
    ptr("barcodes_upload: null kit", L.ffhip_barcodes_upload, e, 1, None, 150)
    ptr("barcodes_upload: no pattern", L.ffhip_barcodes_upload, e, 0, _strs([b"ACGT"]), 150)
    ptr("barcodes_upload: too many patterns", L.ffhip_barcodes_upload, e, 100000, _strs([b"ACGT"]), 150)
    ptr("barcodes_upload: window 0", L.ffhip_barcodes_upload, e, 1, _strs([b"ACGT"]), 0)
    ptr("barcodes_upload: window too wide", L.ffhip_barcodes_upload, e, 1, _strs([b"ACGT"]), 1 << 20)
    ptr("barcodes_upload: no pattern+window 0", L.ffhip_barcodes_upload, e, 0, _strs([b"ACGT"]), 0)
    ptr("barcodes_upload: empty pattern", L.ffhip_barcodes_upload, e, 2, _strs([b"ACGT", b""]), 150)
    ptr("barcodes_upload: null pattern", L.ffhip_barcodes_upload, e, 2, (C.c_char_p * 2)(b"ACGT", None), 150)
    ptr("barcodes_upload: long pattern", L.ffhip_barcodes_upload, e, 1, _strs([b"ACGT" * 100]), 150)
    ptr("barcodes_upload: letter N", L.ffhip_barcodes_upload, e, 2, _strs([b"ACGT", b"ACNT"]), 150)
    ptr("barcodes_upload: letter Z", L.ffhip_barcodes_upload, e, 1, _strs([b"ACGTZ"]), 150)
    ptr("barcodes_upload: lower case", L.ffhip_barcodes_upload, e, 1, _strs([b"acgt"]), 150)
    ptr("barcodes_upload: letter N+a later empty pattern", L.ffhip_barcodes_upload, e, 2, _strs([b"NCGT", b""]), 150)
    ptr("barcodes_upload: long pattern+letter N", L.ffhip_barcodes_upload, e, 1, _strs([b"N" + b"ACGT" * 100]), 150)
    ptr("adapters_upload: null engine", L.ffhip_adapters_upload, None, 1, _strs([b"ACGT"]))
    ptr("adapters_upload: null kit", L.ffhip_adapters_upload, e, 1, None)
    ptr("adapters_upload: no pattern", L.ffhip_adapters_upload, e, 0, _strs([b"ACGT"]))
    ptr("adapters_upload: too many patterns", L.ffhip_adapters_upload, e, 100000, _strs([b"ACGT"]))
    ptr("adapters_upload: empty pattern", L.ffhip_adapters_upload, e, 2, _strs([b"ACGT", b""]))
    ptr("adapters_upload: long pattern", L.ffhip_adapters_upload, e, 1, _strs([b"ACGT" * 100]))
    ptr("adapters_upload: letter N", L.ffhip_adapters_upload, e, 2, _strs([b"ACGT", b"ACGN"]))
    ptr("adapters_upload: letter Z", L.ffhip_adapters_upload, e, 1, _strs([b"ZACGT"]))
    ptr("adapters_upload: long pattern+letter N", L.ffhip_adapters_upload, e, 1, _strs([b"N" + b"ACGT" * 100]))
    ptr("map_ref_upload: null engine", L.ffhip_map_ref_upload, None, 1, _strs([b"ACGT"]))
    ptr("map_ref_upload: null reference", L.ffhip_map_ref_upload, e, 1, None)
    ptr("map_ref_upload: no record", L.ffhip_map_ref_upload, e, 0, _strs([b"ACGT"]))
    ptr("map_ref_upload: too many records", L.ffhip_map_ref_upload, e, 1 << 20, _strs([b"ACGT"]))
    ptr("map_ref_upload: empty record", L.ffhip_map_ref_upload, e, 2, _strs([b"ACGT", b""]))
    ptr("map_ref_upload: more than 2^20 bases", L.ffhip_map_ref_upload, e, 2, _strs([b"ACGT", b"A" * ((1 << 20) - 3)]))
    ptr("map_ref_upload: letter N", L.ffhip_map_ref_upload, e, 2, _strs([b"ACGT", b"ACGNT"]))
    ptr("map_ref_upload: letter Z", L.ffhip_map_ref_upload, e, 1, _strs([b"ACZGT"]))
    ptr("map_ref_upload: letter N+a later empty record", L.ffhip_map_ref_upload, e, 2, _strs([b"NCGT", b""]))
    ptr("pileup_create: null engine", L.ffhip_pileup_create, None, ref.h, 0)
    ptr("pileup_create: null reference", L.ffhip_pileup_create, e, None, 0)
    ptr("pileup_create: another engine's reference", L.ffhip_pileup_create, e, ref2.h, 0)
    ptr("pileup_create: min_identity 1001", L.ffhip_pileup_create, e, ref.h, 1001)
    ptr("pileup_create: another engine's reference+min_identity 1001", L.ffhip_pileup_create, e, ref2.h, 1001)
    case("pileup_reset: null", L.ffhip_pileup_reset(None))
    case("pileup_download: null", L.ffhip_pileup_download(None, None, None))

    # ---- the run fronts: nothing attached or set, then what a row of the table refuses
    for name in ("BARCODES", "ADAPTERS", "MAP", "POLYTAIL", "REMAP", "TRUTH"):
        run("run %s: nothing attached" % name, b4, FL[name])
        run("run %s: the run-length model" % name, br, FL[name])
        run("run %s: undecoded" % name, b4, FL[name] | FL["NO_DECODE"])
        run("run %s: the run-length model+undecoded" % name, br, FL[name] | FL["NO_DECODE"])
    for name in ("EVENTS", "REMAP_MODS", "REMAP_VARIANTS"):
        run("run %s: without REMAP" % name, b5, FL[name])
        run("run %s: without REMAP+the run-length model" % name, br, FL[name])
        run("run %s: REMAP with no sequences" % name, b5, FL[name] | FL["REMAP"])
    seq8, seq8p = _u8([0, 1, 2, 3, 0, 1, 2, 3])
    len8 = (C.c_size_t * 4)(8, 8, 8, 8)
    case("set_remap: sequences for the 4-base batch", L.ffhip_batch_set_remap(b4, 4, (u8p * 4)(seq8p, seq8p, seq8p, seq8p), len8, 16))
    run("run REMAP_MODS: a 4-base model", b4, FL["REMAP_MODS"] | FL["REMAP"])
    run("run REMAP_MODS: a 4-base model+undecoded: remap's row answers", b4, FL["REMAP_MODS"] | FL["REMAP"] | FL["NO_DECODE"])
    case("set_remap: the 4-base batch's cleared", L.ffhip_batch_set_remap(b4, 0, None, None, 0))
    run("run all: the pileup check precedes every row", b4, sum(FL.values()) & ~FL["NO_DECODE"])
    run("run all but PILEUP: the first row answers", b4, sum(FL.values()) & ~FL["NO_DECODE"] & ~FL["PILEUP"])
    for flags, name in ((FL["PILEUP"], "alone"), (FL["PILEUP"] | FL["TRUTH"], "without MAP"), (FL["PILEUP"] | FL["MAP"], "without TRUTH")):
        run("run PILEUP: " + name, b4, flags)
    PMT = FL["PILEUP"] | FL["MAP"] | FL["TRUTH"]
    run("run PILEUP: not from map", b4, PMT)
    case("set_truth_from_map: on", L.ffhip_batch_set_truth_from_map(b4, 1, 16))
    run("run TRUTH from map: without MAP", b4, FL["TRUTH"])
    run("run TRUTH from map: no reference", b4, FL["TRUTH"] | FL["MAP"])
    run("run PILEUP: no pileup", b4, PMT)
    case("set_pileup: another reference's", L.ffhip_batch_set_pileup(b4, pile_b.h))
    run("run PILEUP: no pileup's reference attached", b4, PMT)
    case("set_map: ok", L.ffhip_batch_set_map(b4, ref.h, -1, -1))
    run("run PILEUP: another reference's pileup", b4, PMT)
    case("set_pileup: detach", L.ffhip_batch_set_pileup(b4, None))
    case("set_truth_from_map: off", L.ffhip_batch_set_truth_from_map(b4, 0, 0))
    case("set_map: detach", L.ffhip_batch_set_map(b4, None, -1, -1))

    # ---- setters
    case("set_barcodes: null batch", L.ffhip_batch_set_barcodes(None, kit.h, -1, -1, 0))
    case("set_barcodes: another engine's kit", L.ffhip_batch_set_barcodes(b4, kit2.h, -1, -1, 0))
    case("set_barcodes: max_dist 256", L.ffhip_batch_set_barcodes(b4, kit.h, 256, -1, 0))
    case("set_barcodes: min_sep 256", L.ffhip_batch_set_barcodes(b4, kit.h, -1, 256, 0))
    case("set_barcodes: another engine's kit+max_dist 256", L.ffhip_batch_set_barcodes(b4, kit2.h, 256, -1, 0))
    case("set_adapters: null batch", L.ffhip_batch_set_adapters(None, ad.h, -1))
    case("set_adapters: another engine's kit", L.ffhip_batch_set_adapters(b4, ad2.h, -1))
    case("set_map: null batch", L.ffhip_batch_set_map(None, ref.h, -1, -1))
    case("set_map: another engine's reference", L.ffhip_batch_set_map(b4, ref2.h, -1, -1))
    case("set_map: window 63", L.ffhip_batch_set_map(b4, ref.h, 63, -1))
    case("set_map: window 4097", L.ffhip_batch_set_map(b4, ref.h, 4097, -1))
    case("set_map: max_error 501", L.ffhip_batch_set_map(b4, ref.h, -1, 501))
    case("set_map: window 63+max_error 501", L.ffhip_batch_set_map(b4, ref.h, 63, 501))
    case("set_map: another engine's reference+window 63", L.ffhip_batch_set_map(b4, ref2.h, 63, -1))
    pt = B._polytail_params({})
    case("set_polytail: null batch", L.ffhip_batch_set_polytail(None, C.byref(pt)))
    case("set_polytail: the run-length model", L.ffhip_batch_set_polytail(br, C.byref(pt)))
    for key, val in (("base", 4), ("from_end", 2), ("window", 0), ("window", 65), ("min_calls", 9), ("gap", 17), ("min_windows", 0), ("search", 0), ("min_bases", 0), ("max_sd", -1.0)):
        bad = B._polytail_params({key: val})
        case("set_polytail: %s %s" % (key, val), L.ffhip_batch_set_polytail(b4, C.byref(bad)))
    bad = B._polytail_params({"window": 0})
    case("set_polytail: the run-length model+window 0", L.ffhip_batch_set_polytail(br, C.byref(bad)))
    good, gp = _u8([0, 1, 2, 3, 0, 1, 2, 3])
    five, fp = _u8([0, 1, 4, 3])
    six, sp = _u8([0, 5, 6, 3])
    zlen = (C.c_size_t * 4)(8, 8, 8, 8)

    def seqs(*ps):
        return (u8p * 4)(*ps)

    for what, fn in (("remap", L.ffhip_batch_set_remap), ("truth", L.ffhip_batch_set_truth)):
        case("set_%s: null batch" % what, fn(None, 4, seqs(gp, gp, gp, gp), zlen, 16))
        case("set_%s: the run-length model" % what, fn(br, 4, seqs(gp, gp, gp, gp), zlen, 16))
        case("set_%s: no lengths" % what, fn(b4, 4, seqs(gp, gp, gp, gp), None, 16))
        case("set_%s: 3 reads for 4" % what, fn(b4, 3, seqs(gp, gp, gp, gp), zlen, 16))
        case("set_%s: band -1" % what, fn(b4, 4, seqs(gp, gp, gp, gp), zlen, -1))
        case("set_%s: band 100000" % what, fn(b4, 4, seqs(gp, gp, gp, gp), zlen, 100000))
        case("set_%s: 3 reads for 4+band -1" % what, fn(b4, 3, seqs(gp, gp, gp, gp), zlen, -1))
        case("set_%s: the run-length model+band -1" % what, fn(br, 4, seqs(gp, gp, gp, gp), zlen, -1))
        case("set_%s: a read too long" % what, fn(b4, 4, seqs(gp, gp, gp, gp), (C.c_size_t * 4)(8, 8, 1 << 40, 8), 16))
        case("set_%s: code 4 for a 4-base model" % what, fn(b4, 4, seqs(gp, gp, fp, gp), (C.c_size_t * 4)(8, 8, 4, 8), 16))
        case("set_%s: code 4 for a 5-base model" % what, fn(b5, 4, seqs(gp, gp, fp, gp), (C.c_size_t * 4)(8, 8, 4, 8), 16))
        case("set_%s: code 5 for a 5-base model" % what, fn(b5, 4, seqs(gp, gp, sp, gp), (C.c_size_t * 4)(8, 8, 4, 8), 16))
        case("set_%s: codes 5 and 6: the first answers" % what, fn(b4, 4, seqs(gp, sp, sp, gp), (C.c_size_t * 4)(8, 4, 4, 8), 16))
        case("set_%s: code 4+a later read too long" % what, fn(b4, 4, seqs(gp, fp, gp, gp), (C.c_size_t * 4)(8, 4, 1 << 40, 8), 16))
        case("set_%s: a read too long+code 4 in it" % what, fn(b4, 4, seqs(gp, fp, gp, gp), (C.c_size_t * 4)(8, 1 << 40, 8, 8), 16))
        case("set_%s: null reads and an empty one" % what, fn(b4, 4, seqs(None, gp, None, gp), (C.c_size_t * 4)(0, 0, 0, 8), 16))
        case("set_%s: clear" % what, fn(b4, 0, None, None, 0))
        case("set_%s: clear the 5-base batch's" % what, fn(b5, 0, None, None, 0))
    case("set_truth_from_map: null batch", L.ffhip_batch_set_truth_from_map(None, 1, 16))
    case("set_truth_from_map: the run-length model", L.ffhip_batch_set_truth_from_map(br, 1, 16))
    case("set_truth_from_map: band -1", L.ffhip_batch_set_truth_from_map(b4, 1, -1))
    case("set_truth_from_map: band 1280", L.ffhip_batch_set_truth_from_map(b4, 1, 1280))
    case("set_truth_from_map: the run-length model+band -1", L.ffhip_batch_set_truth_from_map(br, 1, -1))
    case("set_truth_from_map: off on the run-length model", L.ffhip_batch_set_truth_from_map(br, 0, -1))
    case("set_remap_mods: null batch", L.ffhip_batch_set_remap_mods(None, 15, 0))
    case("set_remap_mods: context -1", L.ffhip_batch_set_remap_mods(b5, -1, 0))
    case("set_remap_mods: context 100000", L.ffhip_batch_set_remap_mods(b5, 100000, 0))
    vs = _variants([(1, 1, [2])])
    vbad = _variants([(1, 1, [2]), (100, 1, [2]), (0, 0, [])])
    vp = lambda v: C.c_void_p(v.ctypes.data)      # noqa: E731
    nv = (C.c_size_t * 4)(1, 1, 1, 1)

    def vars_(*vv):
        return (C.c_void_p * 4)(*vv)

    case("set_remap_variants: null batch", L.ffhip_batch_set_remap_variants(None, 4, vars_(vp(vs), vp(vs), vp(vs), vp(vs)), nv, 10, 0))
    case("set_remap_variants: no sequences", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), vp(vs), vp(vs)), nv, 10, 0))
    case("set_remap: three of four reads", L.ffhip_batch_set_remap(b5, 4, seqs(gp, gp, None, gp), zlen, 16))
    case("set_remap_variants: no counts", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), vp(vs), vp(vs)), None, 10, 0))
    case("set_remap_variants: 3 reads for 4", L.ffhip_batch_set_remap_variants(b5, 3, vars_(vp(vs), vp(vs), vp(vs), vp(vs)), nv, 10, 0))
    case("set_remap_variants: context -1", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), None, vp(vs)), (C.c_size_t * 4)(1, 1, 0, 1), -1, 0))
    case("set_remap_variants: context 100000", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), None, vp(vs)), (C.c_size_t * 4)(1, 1, 0, 1), 100000, 0))
    case("set_remap_variants: 3 reads for 4+context -1", L.ffhip_batch_set_remap_variants(b5, 3, vars_(vp(vs), vp(vs), None, vp(vs)), nv, -1, 0))
    case("set_remap_variants: a count and no list", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), None, None, vp(vs)), (C.c_size_t * 4)(1, 1, 0, 1), 10, 0))
    case("set_remap_variants: too many", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), None, vp(vs)), (C.c_size_t * 4)(1, 1 << 40, 0, 1), 10, 0))
    case("set_remap_variants: a read with no sequence", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), vp(vs), vp(vs)), nv, 10, 0))
    case("set_remap_variants: pos beyond the sequence", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vbad), vp(vs), None, vp(vs)), (C.c_size_t * 4)(2, 1, 0, 1), 10, 0))
    case("set_remap_variants: both alleles empty", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vbad[2:]), None, vp(vs)), (C.c_size_t * 4)(1, 1, 0, 1), 10, 0))
    case("set_remap_variants: pos beyond the sequence+a later read with no sequence", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vbad), vp(vs), vp(vs), vp(vs)), (C.c_size_t * 4)(2, 1, 1, 1), 10, 0))
    run("run REMAP_VARIANTS: none set", b5, FL["REMAP"] | FL["REMAP_VARIANTS"])
    case("set_pileup: null batch", L.ffhip_batch_set_pileup(None, pile.h))
    case("set_pileup: the run-length model", L.ffhip_batch_set_pileup(br, pile.h))
    case("set_pileup: another engine's", L.ffhip_batch_set_pileup(b4, pile2.h))
    case("set_pileup: the run-length model+another engine's", L.ffhip_batch_set_pileup(br, pile2.h))

    # ---- a remap window no kernel form holds: refused by the setter; and what the fronts say of sequences and truths set for another number of reads cannot
    # be reached through the setters (they refuse it first), so the fronts' own count checks stay with the tests of packed batches that reach them
    wide, wp = _u8(np.zeros(20000, np.uint8))
    case("set_remap: a window of 20000 cells", L.ffhip_batch_set_remap(b4, 4, seqs(wp, gp, gp, gp), (C.c_size_t * 4)(20000, 8, 8, 8), 1 << 20))
    case("set_remap: code 4+a window of 20000 cells", L.ffhip_batch_set_remap(b4, 4, seqs(wp, fp, gp, gp), (C.c_size_t * 4)(20000, 4, 8, 8), 1 << 20))
    case("set_remap: clear again", L.ffhip_batch_set_remap(b4, 0, None, None, 0))

    # ---- between a run and its finish
    L.ffhip_batch_run(b5, 1.0, 0)
    case("set_polytail: between run and finish", L.ffhip_batch_set_polytail(b5, C.byref(pt)))
    case("set_remap_mods: between run and finish", L.ffhip_batch_set_remap_mods(b5, 15, 0))
    case("set_remap_mods: between run and finish+context -1", L.ffhip_batch_set_remap_mods(b5, -1, 0))
    case("set_remap_variants: between run and finish", L.ffhip_batch_set_remap_variants(b5, 4, vars_(vp(vs), vp(vs), None, vp(vs)), (C.c_size_t * 4)(1, 1, 0, 1), 10, 0))
    case("set_truth: between run and finish", L.ffhip_batch_set_truth(b5, 4, seqs(gp, gp, gp, gp), zlen, 16))
    case("set_truth: between run and finish+band -1", L.ffhip_batch_set_truth(b5, 4, seqs(gp, gp, gp, gp), zlen, -1))
    case("set_truth_from_map: between run and finish", L.ffhip_batch_set_truth_from_map(b5, 1, 16))
    case("set_truth_from_map: between run and finish+band -1", L.ffhip_batch_set_truth_from_map(b5, 1, -1))
    case("set_pileup: between run and finish", L.ffhip_batch_set_pileup(b5, pile.h))
    case("barcode: between run and finish", L.ffhip_batch_barcode(b5, 0, C.byref(B.CBarcodeCall())))
    L.ffhip_batch_finish(b5)

    # ---- accessors of a finished run that made none of the records
    hd, hits = B.CAdapterHeader(), C.POINTER(B.CAdapterHit)()
    anyp, n = C.c_void_p(), C.c_size_t()
    buf32 = C.cast(C.create_string_buffer(32), C.c_void_p)
    acc = (("barcode", lambda b, r, o=True, c=True: L.ffhip_batch_barcode(b, r, C.byref(B.CBarcodeCall()) if o else None)),
           ("adapters", lambda b, r, o=True, c=True: L.ffhip_batch_adapters(b, r, C.byref(hd) if o else None, C.byref(hits) if c else None)),
           ("map", lambda b, r, o=True, c=True: L.ffhip_batch_map(b, r, C.byref(B.CMapCall()) if o else None)),
           ("polytail", lambda b, r, o=True, c=True: L.ffhip_batch_polytail(b, r, buf32 if o else None)),
           ("remap", lambda b, r, o=True, c=True: L.ffhip_batch_remap(b, r, C.byref(B.CRemapCall()) if o else None)),
           ("truth", lambda b, r, o=True, c=True: L.ffhip_batch_truth(b, r, C.byref(B.CTruthCall()) if o else None)),
           ("events", lambda b, r, o=True, c=True: L.ffhip_batch_events(b, r, C.byref(anyp) if o else None, C.byref(n) if c else None)),
           ("site_mods", lambda b, r, o=True, c=True: L.ffhip_batch_site_mods(b, r, C.byref(anyp) if o else None, C.byref(n) if c else None)),
           ("variant_calls", lambda b, r, o=True, c=True: L.ffhip_batch_variant_calls(b, r, C.byref(anyp) if o else None, C.byref(n) if c else None)))
    for name, fn in acc:
        case(name + ": null batch", fn(None, 0))
        case(name + ": read 4 of 4", fn(b5, 4))
        case(name + ": read -1", fn(b5, -1))
        case(name + ": not made", fn(b5, 0))
        case(name + ": read 4 of 4+not made", fn(b5, 4))
        case(name + ": not made+no output", fn(b5, 0, False))
        case(name + ": not made+no second output", fn(b5, 0, True, False))
    # remap made, what goes with it not
    case("set_remap: four reads", L.ffhip_batch_set_remap(b5, 4, seqs(gp, gp, gp, gp), zlen, 16))
    run("run REMAP: taken", b5, FL["REMAP"])
    for name, fn in acc[6:]:
        case(name + ": remap made, they not", fn(b5, 0))

    # ---- a packed batch filled again with another number of reads: the fronts' own count checks (a setter holds the count to the batch's reads at its call)
    bp = B.Batch(dms["lstm4"], 4, 1000, max_reads=8)
    fill = [sig[0, :400], sig[1, :300], sig[2, :350]]
    bp.set_signals_packed(fill[:2], *bp.pack_plan([400, 300]))
    len2 = (C.c_size_t * 2)(8, 8)
    case("packed set_remap: two reads", L.ffhip_batch_set_remap(bp.h, 2, (u8p * 2)(gp, gp), len2, 16))
    case("packed set_truth: two reads", L.ffhip_batch_set_truth(bp.h, 2, (u8p * 2)(gp, gp), len2, 16))
    bp.set_signals_packed(fill, *bp.pack_plan([400, 300, 350]))
    run("packed run REMAP: sequences for two of three reads", bp.h, FL["REMAP"])
    run("packed run TRUTH: truths for two of three reads", bp.h, FL["TRUTH"])
    run("packed run REMAP+TRUTH: both counts wrong, truth's row stands first", bp.h, FL["REMAP"] | FL["TRUTH"])
    bp.close()

    # ---- single-read operators
    d32, d8 = (C.c_int32 * 64)(), (C.c_uint8 * 64)()
    case("op_barcode_scores: null engine", L.ffhip_op_barcode_scores(None, kit.h, b"ACGT", 4, d32, d32))
    case("op_barcode_scores: null kit", L.ffhip_op_barcode_scores(e, None, b"ACGT", 4, d32, d32))
    case("op_barcode_scores: another engine's kit", L.ffhip_op_barcode_scores(e, kit2.h, b"ACGT", 4, d32, d32))
    case("op_barcode_scores: no call", L.ffhip_op_barcode_scores(e, kit.h, None, 4, d32, d32))
    case("op_barcode_scores: no output", L.ffhip_op_barcode_scores(e, kit.h, b"ACGT", 4, None, d32))
    case("op_barcode_scores: len 2^40", L.ffhip_op_barcode_scores(e, kit.h, b"ACGT", 1 << 40, d32, d32))
    case("op_barcode_scores: letter N", L.ffhip_op_barcode_scores(e, kit.h, b"ACNT", 4, d32, d32))
    case("op_barcode_scores: a NUL", L.ffhip_op_barcode_scores(e, kit.h, b"AC\0T", 4, d32, d32))
    case("op_barcode_scores: lower case", L.ffhip_op_barcode_scores(e, kit.h, b"ACGTZacgt", 9, d32, d32))
    case("op_barcode_scores: letters N and X: the first answers", L.ffhip_op_barcode_scores(e, kit.h, b"ACGTZNXT", 8, d32, d32))
    case("op_barcode_scores: no output+letter N", L.ffhip_op_barcode_scores(e, kit.h, b"ACNT", 4, None, d32))
    case("op_adapter_scores: no output", L.ffhip_op_adapter_scores(e, ad.h, b"ACGT", 4, None))
    case("op_adapter_scores: no output+null engine", L.ffhip_op_adapter_scores(None, ad.h, b"ACGT", 4, None))
    case("op_adapter_scores: null engine", L.ffhip_op_adapter_scores(None, ad.h, b"ACGT", 4, d8))
    case("op_adapter_scores: null kit", L.ffhip_op_adapter_scores(e, None, b"ACGT", 4, d8))
    case("op_adapter_scores: another engine's kit", L.ffhip_op_adapter_scores(e, ad2.h, b"ACGT", 4, d8))
    case("op_adapter_scores: no call", L.ffhip_op_adapter_scores(e, ad.h, None, 4, d8))
    case("op_adapter_scores: len 2^40", L.ffhip_op_adapter_scores(e, ad.h, b"ACGT", 1 << 40, d8))
    case("op_adapter_scores: letter N", L.ffhip_op_adapter_scores(e, ad.h, b"ACGTZN", 6, d8))
    case("op_adapter_scores: a NUL", L.ffhip_op_adapter_scores(e, ad.h, b"\0CGT", 4, d8))
    case("op_adapter_scores: another engine's kit+letter N", L.ffhip_op_adapter_scores(e, ad2.h, b"ACNT", 4, d8))
    ahits = (B.CAdapterHit * 15)()
    case("op_adapter_hits: no header", L.ffhip_op_adapter_hits(e, ad.h, -1, b"ACGT", 4, None, ahits))
    case("op_adapter_hits: no hits", L.ffhip_op_adapter_hits(e, ad.h, -1, b"ACGT", 4, C.byref(hd), None))
    case("op_adapter_hits: letter N", L.ffhip_op_adapter_hits(e, ad.h, 1000, b"NCGT", 4, C.byref(hd), ahits))
    case("op_adapter_hits: no header+letter N", L.ffhip_op_adapter_hits(e, ad.h, -1, b"NCGT", 4, None, ahits))
    mc = B.CMapCall()
    case("op_map: no record", L.ffhip_op_map(e, ref.h, -1, -1, b"ACGT", 4, None))
    case("op_map: null engine", L.ffhip_op_map(None, ref.h, -1, -1, b"ACGT", 4, C.byref(mc)))
    case("op_map: null reference", L.ffhip_op_map(e, None, -1, -1, b"ACGT", 4, C.byref(mc)))
    case("op_map: another engine's reference", L.ffhip_op_map(e, ref2.h, -1, -1, b"ACGT", 4, C.byref(mc)))
    case("op_map: no call", L.ffhip_op_map(e, ref.h, -1, -1, None, 4, C.byref(mc)))
    case("op_map: len 2^40", L.ffhip_op_map(e, ref.h, -1, -1, b"ACGT", 1 << 40, C.byref(mc)))
    case("op_map: window 63", L.ffhip_op_map(e, ref.h, 63, -1, b"ACGT", 4, C.byref(mc)))
    case("op_map: max_error 501", L.ffhip_op_map(e, ref.h, -1, 501, b"ACGT", 4, C.byref(mc)))
    case("op_map: letter N", L.ffhip_op_map(e, ref.h, -1, -1, b"ACGN", 4, C.byref(mc)))
    case("op_map: a NUL", L.ffhip_op_map(e, ref.h, -1, -1, b"A\0GT", 4, C.byref(mc)))
    case("op_map: window 63+letter N", L.ffhip_op_map(e, ref.h, 63, -1, b"ACGN", 4, C.byref(mc)))
    case("op_map: max_error 501+letter N", L.ffhip_op_map(e, ref.h, -1, 501, b"NCGT", 4, C.byref(mc)))
    case("op_map: another engine's reference+window 63", L.ffhip_op_map(e, ref2.h, 63, -1, b"ACGT", 4, C.byref(mc)))
    case("op_map_scores: no output", L.ffhip_op_map_scores(e, ref.h, b"ACGT", 4, None))
    case("op_map_scores: no letters", L.ffhip_op_map_scores(e, ref.h, b"ACGT", 0, d32))
    case("op_map_scores: 4097 letters", L.ffhip_op_map_scores(e, ref.h, b"A" * 4097, 4097, d32))
    case("op_map_scores: letter N", L.ffhip_op_map_scores(e, ref.h, b"ACGN", 4, d32))
    case("op_map_scores: no letters+no output", L.ffhip_op_map_scores(e, ref.h, b"ACGT", 0, None))
    for what, fn in (("op_map_stretch", lambda q, s, t, eng=e, r=ref.h, o=d8: L.ffhip_op_map_stretch(eng, r, q, s, t, o)),
                     ("op_pileup", lambda q, s, t, eng=e, r=pile.h, o=d8: L.ffhip_op_pileup(eng, r, q, s, t, b"ACGT"[:max(0, t - s)], max(0, min(4, t - s)), o, max(0, min(4, t - s))))):
        case(what + ": null engine", fn(0, 0, 4, eng=None))
        case(what + ": null object", fn(0, 0, 4, r=None))
        case(what + ": another engine's object", fn(0, 0, 4, r=ref2.h if what == "op_map_stretch" else pile2.h))
        case(what + ": no output or ops", fn(0, 0, 4, o=None))
        case(what + ": search -1", fn(-1, 0, 4))
        case(what + ": search 2 of 2", fn(2, 0, 4))
        case(what + ": start -1", fn(0, -1, 4))
        case(what + ": end 9 of 8", fn(1, 0, 9))
        case(what + ": an empty span", fn(0, 4, 4))
        case(what + ": a reversed span", fn(1, 5, 3))
        case(what + ": search 2 of 2+end 9 of 8", fn(2, 0, 9))
        case(what + ": search -1+an empty span", fn(-1, 4, 4))
    ops, opp = _u8([0, 0, 0, 0])
    case("op_pileup: no call", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, None, 4, opp, 4))
    case("op_pileup: a call of 2^40", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACGT", 1 << 40, opp, 4))
    case("op_pileup: 2^40 ops", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACGT", 4, opp, 1 << 40))
    case("op_pileup: letter N", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACNT", 4, opp, 4))
    case("op_pileup: a NUL", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"AC\0T", 4, opp, 4))
    case("op_pileup: op 4", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACGT", 4, _u8([0, 4, 0, 0])[1], 4))
    case("op_pileup: the ops consume 3 of 4", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACGT", 4, opp, 3))
    case("op_pileup: an empty span+letter N", L.ffhip_op_pileup(e, pile.h, 0, 4, 4, b"ACNT", 4, opp, 4))
    case("op_pileup: search 2 of 2+letter N", L.ffhip_op_pileup(e, pile.h, 2, 0, 4, b"ACNT", 4, opp, 4))
    case("op_pileup: a call of 2^40+an empty span", L.ffhip_op_pileup(e, pile.h, 0, 4, 4, b"ACGT", 1 << 40, opp, 4))
    case("op_pileup: letter N+op 4", L.ffhip_op_pileup(e, pile.h, 0, 0, 4, b"ACNT", 4, _u8([0, 4, 0, 0])[1], 4))
    # scores of 8 blocks for either alphabet, a sequence of 4 bases, a path that moves 3 times
    rng = np.random.default_rng(11)
    t4, m4 = _mat(rng.standard_normal((8, 40)), 40)
    t5, m5 = _mat(rng.standard_normal((8, 60)), 60)
    t5odd, m5odd = _mat(rng.standard_normal((8, 62)), 60)
    t5one, m5one = _mat(rng.standard_normal((1, 60)), 60)
    s4, s4p = _u8([0, 1, 2, 3])
    s5, s5p = _u8([0, 1, 4, 1])
    rm_, rmp = _u8([0, 1, 0, 1, 0, 1, 0, 0])
    rm2, rm2p = _u8([0, 1, 0, 2, 0, 1, 0, 0])
    rm1, rm1p = _u8([0, 1, 0, 0, 0, 1, 0, 0])
    sc = C.c_float()
    case("op_remap: null engine", L.ffhip_op_remap(None, m4, 4, s4p, 4, 16, d8, C.byref(sc)))
    case("op_remap: no sequence", L.ffhip_op_remap(e, m4, 4, None, 4, 16, d8, C.byref(sc)))
    case("op_remap: no output", L.ffhip_op_remap(e, m4, 4, s4p, 4, 16, None, C.byref(sc)))
    case("op_remap: nbase 0", L.ffhip_op_remap(e, m4, 0, s4p, 4, 16, d8, C.byref(sc)))
    case("op_remap: nbase 5 for 40 rows", L.ffhip_op_remap(e, m4, 5, s4p, 4, 16, d8, C.byref(sc)))
    case("op_remap: a stride of 62", L.ffhip_op_remap(e, m5odd, 5, s4p, 4, 16, d8, C.byref(sc)))
    case("op_remap: band -1", L.ffhip_op_remap(e, m4, 4, s4p, 4, -1, d8, C.byref(sc)))
    case("op_remap: no bases", L.ffhip_op_remap(e, m4, 4, s4p, 0, 16, d8, C.byref(sc)))
    case("op_remap: 10 bases for 8 blocks", L.ffhip_op_remap(e, m4, 4, _u8([0, 1] * 5)[1], 10, 16, d8, C.byref(sc)))
    case("op_remap: code 4", L.ffhip_op_remap(e, m4, 4, s5p, 4, 16, d8, C.byref(sc)))
    case("op_remap: band -1+code 4", L.ffhip_op_remap(e, m4, 4, s5p, 4, -1, d8, C.byref(sc)))
    case("op_remap: 10 bases for 8 blocks+code 4", L.ffhip_op_remap(e, m4, 4, _u8([0, 4] * 5)[1], 10, 16, d8, C.byref(sc)))
    case("op_remap: nbase 5 for 40 rows+code 4", L.ffhip_op_remap(e, m4, 5, s5p, 4, 16, d8, C.byref(sc)))
    # (added with the status rule of "remap": scores that leave no finite path are the operator's one refusal that the kernel finds)
    tnan, mnan = _mat(np.full((8, 40), np.nan, np.float32), 40)
    case("op_remap: scores of NaN", L.ffhip_op_remap(e, mnan, 4, s4p, 4, 16, d8, C.byref(sc)))
    # 5000 blocks, 5000 bases and a band that does not narrow them: a window of 5000 cells, which no kernel form holds
    tw, mw = _mat(np.zeros((5000, 40), np.float32), 40)
    dw = (C.c_uint8 * 5000)()
    long_, longp = _u8(np.arange(5000) % 4)
    long4, long4p = _u8(np.where(np.arange(5000) == 4000, 4, np.arange(5000) % 4))
    case("op_remap: a window of 5000 cells", L.ffhip_op_remap(e, mw, 4, longp, 5000, 1 << 20, dw, C.byref(sc)))
    case("op_remap: code 4+a window of 5000 cells", L.ffhip_op_remap(e, mw, 4, long4p, 5000, 1 << 20, dw, C.byref(sc)))
    case("op_remap: band -1+a window of 5000 cells", L.ffhip_op_remap(e, mw, 4, longp, 5000, -1, dw, C.byref(sc)))
    sig8 = np.zeros(40, np.float32)
    path9 = (C.c_int * 9)(0, 0, 1, 1, 2, 2, 3, 3, 0)
    rec32 = C.cast(C.create_string_buffer(32), C.c_void_p)
    pt_op = lambda **kw: L.ffhip_op_polytail(kw.get("eng", e), kw.get("sig", sig8.ctypes.data_as(f32p)), kw.get("ns", 40), kw.get("stride", 5), kw.get("path", path9), kw.get("nb", 8),  # noqa: E731
                                             kw.get("nbase", 4), kw.get("params", C.byref(pt)), kw.get("out", rec32))
    case("op_polytail: no record", pt_op(out=None))
    case("op_polytail: null engine", pt_op(eng=None))
    case("op_polytail: no path", pt_op(path=None))
    case("op_polytail: no parameters", pt_op(params=None))
    case("op_polytail: no signal", pt_op(sig=None))
    case("op_polytail: stride 0", pt_op(stride=0))
    case("op_polytail: no blocks", pt_op(nb=0))
    case("op_polytail: nbase 3", pt_op(nbase=3))
    case("op_polytail: window 0", pt_op(params=C.byref(bad)))
    case("op_polytail: state 8 of a 4-base path", pt_op(path=(C.c_int * 9)(0, 0, 1, 8, 2, 2, 3, 3, 0)))
    case("op_polytail: state -1", pt_op(path=(C.c_int * 9)(0, 0, 1, 1, 2, 2, 3, 3, -1)))
    case("op_polytail: stride 0+window 0", pt_op(stride=0, params=C.byref(bad)))
    case("op_polytail: window 0+state 8", pt_op(params=C.byref(bad), path=(C.c_int * 9)(0, 0, 1, 8, 2, 2, 3, 3, 0)))
    case("op_polytail_windows: no outputs", L.ffhip_op_polytail_windows(e, sig8.ctypes.data_as(f32p), 40, 5, path9, 8, 4, C.byref(pt), None, None, None))
    ev = C.cast(C.create_string_buffer(16 * 16), C.c_void_p)
    ev_op = lambda **kw: L.ffhip_op_events(kw.get("eng", e), kw.get("sig", sig8.ctypes.data_as(f32p)), kw.get("ns", 40), kw.get("stride", 5), kw.get("rm", rmp), kw.get("nb", 8),  # noqa: E731
                                           kw.get("L", 4), kw.get("out", ev))
    case("op_events: null engine", ev_op(eng=None))
    case("op_events: no path", ev_op(rm=None))
    case("op_events: no output", ev_op(out=None))
    case("op_events: no signal", ev_op(sig=None))
    case("op_events: stride 0", ev_op(stride=0))
    case("op_events: no blocks", ev_op(nb=0))
    case("op_events: no bases", ev_op(L=0))
    case("op_events: 2^40 samples", ev_op(ns=1 << 40))
    case("op_events: a path byte of 2", ev_op(rm=rm2p))
    case("op_events: the path moves twice for 4 bases", ev_op(rm=rm1p))
    case("op_events: 5 bases for 3 moves", ev_op(L=5))
    case("op_events: a path byte of 2+too few moves", ev_op(rm=rm2p, L=7))
    case("op_events: stride 0+a path byte of 2", ev_op(stride=0, rm=rm2p))
    sm_out, nsite = C.cast(C.create_string_buffer(16 * 16), C.c_void_p), C.c_size_t()
    sm_op = lambda **kw: L.ffhip_op_site_mods(kw.get("eng", e), kw.get("t", m5), kw.get("nbase", 5), kw.get("codes", s5p), kw.get("L", 4), kw.get("rm", rmp), kw.get("nb", 8),  # noqa: E731
                                              kw.get("context", 15), 0, kw.get("out", sm_out), kw.get("n", C.byref(nsite)))
    vc_out = C.cast(C.create_string_buffer(16 * 16), C.c_void_p)
    va_op = lambda **kw: L.ffhip_op_variants(kw.get("eng", e), kw.get("t", m5), kw.get("nbase", 5), kw.get("codes", s5p), kw.get("L", 4), kw.get("rm", rmp), kw.get("nb", 8),  # noqa: E731
                                             kw.get("vars", vp(vs)), kw.get("nvar", 1), kw.get("context", 10), 0, kw.get("out", vc_out))
    for what, op in (("op_site_mods", sm_op), ("op_variants", va_op)):
        case(what + ": null engine", op(eng=None))
        case(what + ": nbase 3", op(nbase=3))
        case(what + ": nbase 4", op(nbase=4, t=m4, codes=s4p))
        case(what + ": 40 rows for 5 bases", op(t=m4))
        case(what + ": a stride of 62", op(t=m5odd))
        case(what + ": no sequence", op(codes=None))
        case(what + ": no path", op(rm=None))
        case(what + ": no output", op(out=None))
        case(what + ": context -1", op(context=-1))
        case(what + ": context 100000", op(context=100000))
        case(what + ": 7 blocks of path for 8 of scores", op(nb=7))
        case(what + ": no bases", op(L=0))
        case(what + ": a path byte of 2", op(rm=rm2p))
        case(what + ": the path moves twice for 4 bases", op(rm=rm1p))
        case(what + ": code 5", op(codes=_u8([0, 1, 5, 1])[1]))
        case(what + ": nbase 3+no sequence", op(nbase=3, codes=None))
        case(what + ": no sequence+context -1", op(codes=None, context=-1))
        case(what + ": context -1+7 blocks of path", op(context=-1, nb=7))
        case(what + ": 7 blocks of path+a path byte of 2", op(nb=7, rm=rm2p))
        case(what + ": a path byte of 2+code 5", op(rm=rm2p, codes=_u8([0, 1, 5, 1])[1]))
        case(what + ": too few moves+code 5", op(rm=rm1p, codes=_u8([0, 1, 5, 1])[1]))
        case(what + ": a path byte of 2 behind too few moves", op(rm=_u8([0, 1, 0, 0, 0, 0, 0, 2])[1]))
    case("op_site_mods: no count", sm_op(n=None))
    case("op_site_mods: no C or Z: taken", sm_op(codes=_u8([0, 2, 3, 0])[1]))
    case("op_variants: variants and no list", va_op(vars=None))
    case("op_variants: 2^40 variants", va_op(nvar=1 << 40))
    case("op_variants: pos beyond the sequence", va_op(vars=vp(vbad), nvar=2))
    case("op_variants: both alleles empty", va_op(vars=vp(vbad[2:]), nvar=1))
    case("op_variants: code 5+pos beyond the sequence", va_op(codes=_u8([0, 1, 5, 1])[1], vars=vp(vbad), nvar=2))
    case("op_variants: no variants: taken", va_op(vars=None, nvar=0, out=None))
    tc, tops = B.CTruthCall(), (C.c_uint8 * 64)()
    tr, trp = _u8([0, 1, 2, 3])
    tr5, tr5p = _u8([0, 1, 5, 3])
    tr_op = lambda **kw: L.ffhip_op_truth(kw.get("eng", e), kw.get("call", b"ACGT"), kw.get("n", 4), kw.get("truth", trp), kw.get("m", 4), kw.get("band", 16),  # noqa: E731
                                          kw.get("out", C.byref(tc)), kw.get("ops", tops))
    case("op_truth: null engine", tr_op(eng=None))
    case("op_truth: no record", tr_op(out=None))
    case("op_truth: no call", tr_op(call=None))
    case("op_truth: no truth", tr_op(truth=None))
    case("op_truth: no ops", tr_op(ops=None))
    case("op_truth: a call of 2^40", tr_op(n=1 << 40))
    case("op_truth: a truth of 2^40", tr_op(m=1 << 40))
    case("op_truth: band -1", tr_op(band=-1))
    case("op_truth: band 1280", tr_op(band=1280))
    case("op_truth: letter N", tr_op(call=b"ACNT"))
    case("op_truth: a NUL", tr_op(call=b"ACG\0"))
    case("op_truth: code 5", tr_op(truth=tr5p))
    case("op_truth: code 4: taken", tr_op(truth=_u8([0, 1, 4, 3])[1]))
    case("op_truth: a call of 2^40+band -1", tr_op(n=1 << 40, band=-1))
    case("op_truth: band -1+letter N", tr_op(band=-1, call=b"ACNT"))
    case("op_truth: letter N+code 5", tr_op(call=b"ACNT", truth=tr5p))
    case("op_truth: band 1280+code 5", tr_op(band=1280, truth=tr5p))

    assert len({row[0] for row in out}) == len(out), "a case name stands twice"
    for o in (pile, pile_b, pile2, kit, kit2, ad, ad2):
        o.close()
    for b in bs.values():
        b.close()
    for o in (ref, ref_b, ref2):
        o.close()
    for dm in dms.values():
        dm.close()
    eng2.close()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "feature_refusals.json")
    eng = B.Engine(0)
    table, again = record(eng), record(eng)
    eng.close()
    if table != again:
        for a, b in zip(table, again):
            if a != b:
                print("NOT REPRODUCIBLE", a, b)
        sys.exit(1)
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in table) + "\n]\n")
    print("wrote", path, "from", os.path.dirname(B.__file__), len(table), "cases,", sum(1 for r in table if r[1] not in (0, 1) or "taken" in r[0]), "answers")


if __name__ == "__main__":
    main()
