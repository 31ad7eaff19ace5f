"""ctypes binding of libffhip.so (the C-ABI of include/ffhip.h).

This is the Python mirror of the boundary used by tests/ and bench.py.  It contains no compute: if
the HIP library is missing or no gfx950 device is present it raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import numpy as np

from . import model as M

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

RUN_VITERBI_ONLY = 1
RUN_NO_TRACE = 2
RUN_NO_DECODE = 4
RUN_STEPWISE_RNN = 8
RUN_KEEP_ACTS = 16
RUN_UNFUSED_RNN = 32
RUN_F32_RNN = 64
RUN_FAST_GATES = 128
RUN_FAST_GATES2 = 256
RUN_EXACT_GATES = 512
RUN_RLE_RUNS = 1024       # run-length model: run bases + run-length estimates made on the device (Batch.rle_runs)
RUN_RLE_RECORDS = 2048    # ... and every run's shape, scale and dwell
RLE_SCALE_DEFAULT = (1.02, 1.04, 1.04, 1.02)      # decode_runnie.py's default --scale (A, C, G, T)
RUN_MOD_PROBS = 4096      # 5-base model: 5mC probabilities (SAM ML bytes) of the called bases made on the device (Batch.mod_probs)
RUN_MOVES = 8192          # flip-flop model: the move table (one byte a block, 1 where a base is emitted) made on the device (Batch.moves)
RUN_ADAPTERS = 1048576   # flip-flop model: one adapter record a read (a header and up to 15 hits) made on the device against the kit of Batch.set_adapters (Batch.adapters)
ADAPTER_SEGMENT = 512    # FFHIP_ADAPTER_SEGMENT (include/ffhip.h "adapters"): the columns one wave of k_adapters owns; checked against the library at load
ADAPTER_MAX_HITS = 15
RUN_MAP = 4194304        # flip-flop model: one map record a read (status, strand and record, span, either anchor's place) made on the device against the reference of Batch.set_map (Batch.map)
RUN_PILEUP = 8388608     # with RUN_MAP | RUN_TRUTH in the mode of Batch.set_truth_from_map: every aligned read's per-position counts added into the Pileup of Batch.set_pileup
PILEUP_TOTALS = ("reads", "skipped", "match", "mismatch", "del", "ins", "edge_ins", "reserved")      # ffhip_pileup_totals, eight uint64
RUN_MOD_PILEUP = 16777216  # with RUN_MAP | RUN_TRUTH | RUN_MOD_PROBS in the same mode: every aligned read's 5mC bytes classed per reference C into the ModPileup of Batch.set_modpileup
MODPILEUP_TOTALS = ("reads", "skipped", "sites", "mod", "canon", "fail", "diff", "del")      # ffhip_modpileup_totals, eight uint64
MODPILEUP_COLUMNS = ("mod", "canon", "fail", "diff", "del")
RUN_CONSENSUS = 33554432   # with RUN_MAP | RUN_TRUTH in the same mode: every aligned read's forward letters, deletions and inserted letters added per position into the Consensus of Batch.set_consensus
CONSENSUS_TOTALS = ("reads", "skipped", "bases", "del", "ins_bases", "long_ins", "edge_ins", "reserved")      # ffhip_consensus_totals, eight uint64
CONSENSUS_PLANES = 37    # FFHIP_CONSENSUS_PLANES: A C G T del, then A C G T of each of the CONSENSUS_MINOR insertion columns behind the position
CONSENSUS_MINOR = 8
CONSENSUS_LOW, CONSENSUS_SAME, CONSENSUS_SUB, CONSENSUS_DEL, CONSENSUS_INS = 0, 1, 2, 3, 4      # a cell's `what`: one of the first four, CONSENSUS_INS a bit beside it
CONSENSUS_CELL = np.dtype([("n", "u1"), ("what", "u1"), ("s", "S10"), ("depth", "<u4")])       # ffhip_consensus_cell, 16 bytes
RUN_ERRPROFILE = 67108864  # with RUN_TRUTH in either truth mode (truth from map: RUN_MAP too): every aligned read's ops classed into the ErrProfile of Batch.set_errprofile
ERRPROFILE_TOTALS = ("reads", "skipped", "match", "mismatch", "del", "ins", "edge_ins", "ctx_sites", "hp_runs", "hp_long", "hp_wide", "reserved")      # ffhip_errprofile_totals, twelve uint64
ERRPROFILE_SECTIONS = (("sub", 0, (4, 5)), ("ins", 20, (4,)), ("qual", 24, (94, 3)), ("ctx", 306, (1024, 4)), ("hp", 4402, (4, 16, 33)))      # name, FFHIP_ERRPROFILE_<NAME>, shape
ERRPROFILE_TABLE_WORDS = 6514   # FFHIP_ERRPROFILE_TABLE_WORDS: the sections together; the totals stand behind them
ERRPROFILE_WORDS = 6526         # FFHIP_ERRPROFILE_WORDS, ffhip_errprofile_words()
ERRPROFILE_HP_MAX_RUN, ERRPROFILE_HP_MAX_CALLED, ERRPROFILE_HP_MAX_OPS = 16, 32, 64
MAP_SEGMENT = 2048       # FFHIP_MAP_SEGMENT (include/ffhip.h "map"): the columns one task of k_map_scan owns; checked against the library at load
MAP_MAX_TOTAL = 1 << 20
MAP_MAX_ANCHOR = 4096
RUN_POLYTAIL = 2097152    # flip-flop model: one poly tail record a read made on the device from the Viterbi path and the signal with the parameters of Batch.set_polytail (Batch.polytail)
POLYTAIL_DTYPE = np.dtype([("status", np.int32), ("first", np.int32), ("count", np.int32), ("flat", np.int32), ("calls", np.int32),
                           ("level", np.float32), ("rate", np.float32), ("bases", np.float32)])      # ffhip_polytail (include/ffhip.h)
POLYTAIL_DEFAULTS = dict(base=0, from_end=0, window=8, min_calls=4, gap=2, min_windows=5, search=500, min_bases=20, max_sd=0.3)      # flappie --poly-tail's, at stride 5
RUN_BARCODES = 16384      # flip-flop model: one barcode record a read made on the device against the kit of Batch.set_barcodes (Batch.barcode)
RUN_REMAP = 32768         # flip-flop model: each read's signal mapped to the sequence of Batch.set_remap on the device (Batch.remap)
RUN_TRUTH = 65536         # flip-flop model: each read's call aligned to the truth of Batch.set_truth on the device (Batch.truth)
RUN_EVENTS = 131072       # with RUN_REMAP: first sample, count, mean and sd of every base of every mapped read, made on the device (Batch.events)
EVENT_DTYPE = np.dtype([("first", np.int32), ("count", np.int32), ("mean", np.float32), ("sd", np.float32)])      # ffhip_event (include/ffhip.h)
RUN_REMAP_MODS = 262144   # with RUN_REMAP, a model of the alphabet ACGTZ: the log scores with C and with Z at every C / Z of every mapped sequence, made on the device (Batch.site_mods)
SITE_MOD_DTYPE = np.dtype([("pos", np.int32), ("nblock", np.int32), ("can", np.float32), ("mod", np.float32)])      # ffhip_site_mod (include/ffhip.h)
RUN_REMAP_VARIANTS = 524288   # with RUN_REMAP: the log scores of every variant of Batch.set_remap_variants under the sequence as given and as edited, made on the device (Batch.variant_calls)
VARIANT_DTYPE = np.dtype([("pos", np.int32), ("nref", np.uint8), ("nalt", np.uint8), ("alt", np.uint8, (16,)), ("pad", np.uint8, (2,))])      # ffhip_variant (include/ffhip.h)
VARIANT_CALL_DTYPE = np.dtype([("index", np.int32), ("nblock", np.int32), ("ref", np.float32), ("alt", np.float32)])      # ffhip_variant_call (include/ffhip.h)
TRUTH_BAND_MAX = 1279     # the widest kernel form holds a window of 2 W + 1 <= 2560 cells
TRUTH_FIELDS = ("status", "n", "m", "dist", "n_match", "n_mismatch", "n_ins", "n_del", "maxdev")
# ffhip_debug_gate_math forms (include/ffhip.h)
GATE_FORMS = ("logistic_ref", "tanh_ref", "logistic_ref4_lean", "logistic_ref2_lean", "logistic_ref_lean", "tanh_ref_lean",
              "swish_act4", "tanh_act4", "logistic_hw1", "tanh_hw1", "logistic_hw2", "tanh_hw2")
NGROUP = 6
# ffhip_debug_batch_forms: kernel form ids (include/ffhip.h FFHIP_FORM_*)
FORMS = {1: "small<4,5>", 2: "small<16,20>", 3: "small<4>", 4: "small<16>", 5: "small<32>", 6: "mfma<true>", 7: "mfma<false>",
         8: "split_ws<10>", 9: "split<4,4>", 10: "split<2,2>", 11: "head<3>", 12: "head<4>", 13: "head_split<3>", 14: "head_split<4>"}
GROUP_NAMES = ("conv", "inproj", "recurrent", "head_crf", "posterior", "viterbi_assembly")


class FFHipError(RuntimeError):
    pass


class CMat(C.Structure):
    """`_Mat` of include/flappie_matrix.h"""
    _fields_ = [("nr", C.c_size_t), ("nrq", C.c_size_t), ("nc", C.c_size_t), ("stride", C.c_size_t),
                ("f", C.POINTER(C.c_float)), ("dev", C.c_void_p), ("dev_state", C.c_int)]


class CModelDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("nconv", C.c_int),
                ("conv_W", C.POINTER(CMat) * 3), ("conv_b", C.POINTER(CMat) * 3),
                ("conv_stride", C.c_int * 3),
                ("rnn_iW", C.POINTER(CMat) * 5), ("rnn_sW", C.POINTER(CMat) * 5),
                ("rnn_b", C.POINTER(CMat) * 5),
                ("FF_W", C.POINTER(CMat)), ("FF_b", C.POINTER(CMat))]


class CFMat(C.Structure):
    """`ffhip_mat` of include/ffhip.h, a plain host array (no device image)"""
    _fields_ = [("data", C.POINTER(C.c_float)), ("nr", C.c_size_t), ("nc", C.c_size_t), ("stride", C.c_size_t),
                ("dev", C.c_void_p), ("dev_state", C.c_void_p)]


class CRleRuns(C.Structure):
    """`ffhip_rle_runs` of include/ffhip.h"""
    _fields_ = [("nrun", C.c_size_t), ("length", C.c_ulonglong), ("failed", C.c_int),
                ("base", C.POINTER(C.c_uint8)), ("est", C.POINTER(C.c_int32)),
                ("shape", C.POINTER(C.c_float)), ("scale", C.POINTER(C.c_float)), ("dwell", C.POINTER(C.c_int32))]


class CBarcodeCall(C.Structure):
    """ffhip_barcode_call (include/ffhip.h): 16 bytes"""
    _fields_ = [("best", C.c_int16), ("best_dist", C.c_uint8), ("second_dist", C.c_uint8), ("front_dist", C.c_uint8), ("rear_dist", C.c_uint8),
                ("ends", C.c_uint8), ("pad", C.c_uint8), ("front_end", C.c_int16), ("rear_end", C.c_int16), ("reserved", C.c_int32)]


class CPolyTailParams(C.Structure):
    """ffhip_polytail_params (include/ffhip.h): 36 bytes"""
    _fields_ = [("base", C.c_int32), ("from_end", C.c_int32), ("window", C.c_int32), ("min_calls", C.c_int32), ("gap", C.c_int32), ("min_windows", C.c_int32),
                ("search", C.c_int32), ("min_bases", C.c_int32), ("max_sd", C.c_float)]


def _polytail_params(params: dict) -> CPolyTailParams:
    """POLYTAIL_DEFAULTS with `params` over them; min_calls follows a window given without it (half the window, rounded up)"""
    unknown = set(params) - set(POLYTAIL_DEFAULTS)
    if unknown:
        raise TypeError("no such poly tail parameter: " + ", ".join(sorted(unknown)))
    p = dict(POLYTAIL_DEFAULTS)
    if "window" in params and "min_calls" not in params:
        p["min_calls"] = (int(params["window"]) + 1) // 2
    p.update(params)
    return CPolyTailParams(*[int(p[k]) for k in list(POLYTAIL_DEFAULTS)[:8]], float(p["max_sd"]))


class CMapCall(C.Structure):
    """ffhip_map_call (include/ffhip.h): 64 bytes, sixteen int32"""
    _fields_ = [("v", C.c_int32 * 16)]


MAP_FIELDS = ("status", "n", "nanchor", "q", "tstart", "tend")
MAP_ANCHOR_FIELDS = ("q", "start", "end", "dist", "second")


def _map_record(rec) -> dict:
    """a map record as a dict: MAP_FIELDS, "anchors": two dicts of MAP_ANCHOR_FIELDS, "raw": the sixteen int32"""
    v = [int(x) for x in rec.v]
    out = dict(zip(MAP_FIELDS, v[:6]))
    out["anchors"] = [dict(zip(MAP_ANCHOR_FIELDS, v[6 + 5 * a:11 + 5 * a])) for a in range(2)]
    out["raw"] = np.array(v, np.int32)
    return out


class CAdapterHeader(C.Structure):
    """ffhip_adapter_header (include/ffhip.h): 16 bytes"""
    _fields_ = [("nhit", C.c_int32), ("len", C.c_int32), ("kept", C.c_int32), ("reserved", C.c_int32)]


class CAdapterHit(C.Structure):
    """ffhip_adapter_hit (include/ffhip.h): 16 bytes"""
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("pattern", C.c_int16), ("orientation", C.c_uint8), ("dist", C.c_uint8), ("reserved", C.c_int32)]


class CRemapCall(C.Structure):
    """ffhip_remap_call (include/ffhip.h)"""
    _fields_ = [("status", C.c_int), ("L", C.c_size_t), ("score", C.c_float), ("rm", C.POINTER(C.c_uint8)), ("nblock", C.c_size_t)]


class CTruthCall(C.Structure):
    """ffhip_truth_call (include/ffhip.h)"""
    _fields_ = [("status", C.c_int), ("n", C.c_size_t), ("m", C.c_size_t), ("dist", C.c_int), ("n_match", C.c_int), ("n_mismatch", C.c_int), ("n_ins", C.c_int),
                ("n_del", C.c_int), ("maxdev", C.c_int), ("nops", C.c_size_t), ("ops", C.POINTER(C.c_uint8))]


class CRawTable(C.Structure):
    """`raw_table` of include/flappie_structures.h"""
    _fields_ = [("uuid", C.c_char_p), ("n", C.c_size_t), ("start", C.c_size_t), ("end", C.c_size_t),
                ("raw", C.POINTER(C.c_float))]


class CDacRead(C.Structure):
    """`ffhip_dac_read` of include/ffhip.h"""
    _fields_ = [("dac", C.POINTER(C.c_int16)), ("n", C.c_size_t), ("offset", C.c_float), ("raw_unit", C.c_float)]


def library_path() -> str:
    # FFHIP_BINDING_LIBRARY: another build of the same C-ABI (tests only: tools/test_hooks/libffhip_resweep.so, the library whose layer kernels re-sweep on purpose)
    return os.environ.get("FFHIP_BINDING_LIBRARY") or os.path.join(_HERE, "libffhip.so")


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise FFHipError("libffhip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(path)
    vp = C.c_void_p
    L.ffhip_last_error.restype = C.c_char_p
    L.ffhip_version.restype = C.c_char_p
    L.ffhip_device_count.restype = C.c_int
    L.ffhip_engine_create.restype = vp
    L.ffhip_engine_create.argtypes = [C.c_int]
    L.ffhip_engine_destroy.argtypes = [vp]
    L.ffhip_engine_synchronize.argtypes = [vp]
    L.ffhip_engine_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ffhip_engine_set_profiling.argtypes = [vp, C.c_int]
    L.ffhip_model_upload.restype = vp
    L.ffhip_model_upload.argtypes = [vp, C.POINTER(CModelDesc)]
    L.ffhip_model_free.argtypes = [vp]
    for fn in ("ffhip_model_hidden", "ffhip_model_nparam", "ffhip_model_nbase", "ffhip_model_launch_reads"):
        getattr(L, fn).restype = C.c_size_t
        getattr(L, fn).argtypes = [vp]
    L.ffhip_model_nblock.restype = C.c_size_t
    L.ffhip_model_nblock.argtypes = [vp, C.c_size_t]
    L.ffhip_batch_create.restype = vp
    L.ffhip_batch_create.argtypes = [vp, vp, C.c_int, C.c_size_t]
    L.ffhip_batch_destroy.argtypes = [vp]
    L.ffhip_batch_nblock.restype = C.c_size_t
    L.ffhip_batch_nblock.argtypes = [vp]
    L.ffhip_batch_set_reads.argtypes = [vp, C.POINTER(CRawTable)]
    L.ffhip_batch_set_signals.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
    L.ffhip_batch_run.argtypes = [vp, C.c_float, C.c_uint]
    L.ffhip_batch_run_pair.argtypes = [vp, vp, C.c_float, C.c_uint]
    L.ffhip_batch_paired.argtypes = [vp]
    L.ffhip_batch_read_nblock.restype = C.c_size_t
    L.ffhip_batch_read_nblock.argtypes = [vp, C.c_int]
    L.ffhip_batch_set_signals_ragged.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t)]
    L.ffhip_prep_create.restype = vp
    L.ffhip_prep_create.argtypes = [vp, C.POINTER(CRawTable), C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_float]
    L.ffhip_prep_begin.restype = vp
    L.ffhip_prep_begin.argtypes = L.ffhip_prep_create.argtypes
    L.ffhip_prep_create_dac.restype = vp
    L.ffhip_prep_create_dac.argtypes = [vp, C.POINTER(CDacRead)] + L.ffhip_prep_create.argtypes[2:]
    L.ffhip_prep_begin_dac.restype = vp
    L.ffhip_prep_begin_dac.argtypes = L.ffhip_prep_create_dac.argtypes
    L.ffhip_prep_finish.argtypes = [vp]
    L.ffhip_prep_destroy.argtypes = [vp]
    L.ffhip_prep_range.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ffhip_prep_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ffhip_prep_get_signal.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_batch_set_prepared.argtypes = [vp, vp, C.POINTER(C.c_int)]
    # packed batches (several reads to a row)
    L.ffhip_model_pack_gap.restype = C.c_size_t
    L.ffhip_model_pack_gap.argtypes = [vp]
    L.ffhip_model_packable.argtypes = [vp]
    L.ffhip_pack_plan.argtypes = [vp, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ffhip_batch_create_packed.restype = vp
    L.ffhip_batch_create_packed.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int]
    L.ffhip_batch_set_prepared_packed.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ffhip_batch_set_signals_packed.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ffhip_batch_nreads.argtypes = [vp]
    L.ffhip_quantiles.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.c_size_t]
    L.ffhip_medmad_normalise.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ffhip_mad.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.ffhip_array_transform.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.c_float, C.c_float]
    L.ffhip_batch_finish.argtypes = [vp]
    L.ffhip_batch_basecall.restype = C.c_void_p
    L.ffhip_batch_basecall.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t)]
    L.ffhip_batch_quality.restype = C.c_void_p
    L.ffhip_batch_quality.argtypes = [vp, C.c_int]
    L.ffhip_batch_score.restype = C.c_float
    L.ffhip_batch_score.argtypes = [vp, C.c_int]
    L.ffhip_batch_get_path.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.ffhip_batch_get_transitions.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_batch_get_posterior.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_batch_get_trace.argtypes = [vp, C.c_int, C.POINTER(C.c_int32)]
    L.ffhip_batch_get_activation.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_batch_profile.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.ffhip_batch_f32_reruns.argtypes = [vp]
    L.ffhip_engine_f32_reruns.restype = C.c_ulonglong
    L.ffhip_engine_f32_reruns.argtypes = [vp]
    L.ffhip_debug_batch_keep_front.argtypes = [vp, C.c_int]
    L.ffhip_debug_batch_front.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_debug_batch_head_input.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ffhip_debug_batch_forms.argtypes = [vp, C.POINTER(C.c_int)]
    L.ffhip_debug_batch_device_bytes.restype = C.c_size_t
    L.ffhip_debug_batch_device_bytes.argtypes = [vp]
    L.ffhip_debug_result_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_size_t), C.c_int]
    L.ffhip_batch_set_run_scale.argtypes = [vp, C.POINTER(C.c_double)]
    L.ffhip_batch_rle_runs.argtypes = [vp, C.c_int, C.POINTER(CRleRuns)]
    L.ffhip_op_rle_runs.argtypes = [vp, CFMat, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int),
                                    C.POINTER(C.c_ulonglong)]
    L.ffhip_batch_mod_probs.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.ffhip_op_mod_probs.argtypes = [vp, CFMat, C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)]
    L.ffhip_batch_moves.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.ffhip_op_moves.argtypes = [vp, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_uint8)]
    L.ffhip_model_stride.restype = C.c_size_t
    L.ffhip_model_stride.argtypes = [vp]
    L.ffhip_barcodes_upload.restype = vp
    L.ffhip_barcodes_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.c_int]
    L.ffhip_barcodes_free.restype = None
    L.ffhip_barcodes_free.argtypes = [vp]
    L.ffhip_batch_set_barcodes.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.ffhip_batch_barcode.argtypes = [vp, C.c_int, C.POINTER(CBarcodeCall)]
    L.ffhip_op_barcode_scores.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.ffhip_adapters_upload.restype = vp
    L.ffhip_adapters_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p)]
    L.ffhip_adapters_free.restype = None
    L.ffhip_adapters_free.argtypes = [vp]
    L.ffhip_batch_set_adapters.argtypes = [vp, vp, C.c_int]
    L.ffhip_batch_adapters.argtypes = [vp, C.c_int, C.POINTER(CAdapterHeader), C.POINTER(C.POINTER(CAdapterHit))]
    L.ffhip_op_adapter_scores.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8)]
    L.ffhip_op_adapter_hits.argtypes = [vp, vp, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(CAdapterHeader), C.POINTER(CAdapterHit)]
    L.ffhip_adapter_segment.restype = C.c_int
    L.ffhip_adapter_segment.argtypes = []
    assert L.ffhip_adapter_segment() == ADAPTER_SEGMENT, "binding.py and libffhip.so disagree on FFHIP_ADAPTER_SEGMENT"
    L.ffhip_map_ref_upload.restype = vp
    L.ffhip_map_ref_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p)]
    L.ffhip_map_ref_free.restype = None
    L.ffhip_map_ref_free.argtypes = [vp]
    L.ffhip_batch_set_map.argtypes = [vp, vp, C.c_int, C.c_int]
    L.ffhip_batch_map.argtypes = [vp, C.c_int, C.POINTER(CMapCall)]
    L.ffhip_op_map_scores.argtypes = [vp, vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]
    L.ffhip_op_map.argtypes = [vp, vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(CMapCall)]
    L.ffhip_map_segment.restype = C.c_int
    L.ffhip_map_segment.argtypes = []
    assert L.ffhip_map_segment() == MAP_SEGMENT, "binding.py and libffhip.so disagree on FFHIP_MAP_SEGMENT"
    L.ffhip_batch_set_polytail.argtypes = [vp, C.POINTER(CPolyTailParams)]
    L.ffhip_batch_polytail.argtypes = [vp, C.c_int, vp]
    L.ffhip_op_polytail.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.POINTER(CPolyTailParams), vp]
    L.ffhip_op_polytail_windows.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.POINTER(CPolyTailParams),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
    L.ffhip_batch_set_remap.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t), C.c_int]
    L.ffhip_batch_remap.argtypes = [vp, C.c_int, C.POINTER(CRemapCall)]
    L.ffhip_op_remap.argtypes = [vp, CFMat, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_float)]
    L.ffhip_debug_remap_form.argtypes = [C.c_size_t, C.c_int]
    L.ffhip_batch_set_remap_from_map.argtypes = [vp, C.c_int, C.c_int]
    L.ffhip_op_map_remap_code.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.ffhip_debug_remap_from_map_form.argtypes = [C.c_int, C.c_int]
    L.ffhip_batch_events.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ffhip_op_events.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.c_size_t, vp]
    L.ffhip_batch_set_remap_mods.argtypes = [vp, C.c_int, C.c_int]
    L.ffhip_batch_site_mods.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ffhip_op_site_mods.argtypes = [vp, CFMat, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.c_int, vp, C.POINTER(C.c_size_t)]
    L.ffhip_batch_set_remap_variants.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_int, C.c_int]
    L.ffhip_batch_variant_calls.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ffhip_op_variants.argtypes = [vp, CFMat, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int, vp]
    L.ffhip_batch_set_truth.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t), C.c_int]
    L.ffhip_batch_truth.argtypes = [vp, C.c_int, C.POINTER(CTruthCall)]
    L.ffhip_op_truth.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.c_int, C.POINTER(CTruthCall), C.POINTER(C.c_uint8)]
    L.ffhip_debug_truth_form.argtypes = [C.c_size_t]
    L.ffhip_batch_set_truth_from_map.argtypes = [vp, C.c_int, C.c_int]
    L.ffhip_op_map_stretch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    L.ffhip_pileup_create.restype = vp
    L.ffhip_pileup_create.argtypes = [vp, vp, C.c_int]
    L.ffhip_pileup_free.restype = None
    L.ffhip_pileup_free.argtypes = [vp]
    L.ffhip_pileup_reset.argtypes = [vp]
    L.ffhip_pileup_positions.restype = C.c_size_t
    L.ffhip_pileup_positions.argtypes = [vp]
    L.ffhip_pileup_download.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.ffhip_batch_set_pileup.argtypes = [vp, vp]
    L.ffhip_op_pileup.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ffhip_modpileup_create.restype = vp
    L.ffhip_modpileup_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.ffhip_modpileup_free.restype = None
    L.ffhip_modpileup_free.argtypes = [vp]
    L.ffhip_modpileup_reset.argtypes = [vp]
    L.ffhip_modpileup_positions.restype = C.c_size_t
    L.ffhip_modpileup_positions.argtypes = [vp]
    L.ffhip_modpileup_download.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ffhip_batch_set_modpileup.argtypes = [vp, vp]
    L.ffhip_op_modpileup.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ffhip_consensus_create.restype = vp
    L.ffhip_consensus_create.argtypes = [vp, vp, C.c_int]
    L.ffhip_consensus_free.restype = None
    L.ffhip_consensus_free.argtypes = [vp]
    L.ffhip_consensus_reset.argtypes = [vp]
    L.ffhip_consensus_positions.restype = C.c_size_t
    L.ffhip_consensus_positions.argtypes = [vp]
    L.ffhip_consensus_download.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.ffhip_consensus_call.argtypes = [vp, C.c_int, vp]
    L.ffhip_batch_set_consensus.argtypes = [vp, vp]
    L.ffhip_op_consensus.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ffhip_errprofile_create.restype = vp
    L.ffhip_errprofile_create.argtypes = [vp, C.c_int]
    L.ffhip_errprofile_free.restype = None
    L.ffhip_errprofile_free.argtypes = [vp]
    L.ffhip_errprofile_reset.argtypes = [vp]
    L.ffhip_errprofile_words.restype = C.c_size_t
    L.ffhip_errprofile_words.argtypes = []
    L.ffhip_errprofile_download.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ffhip_batch_set_errprofile.argtypes = [vp, vp]
    L.ffhip_op_errprofile.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ffhip_op_errprofile_mapped.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]
    L.ffhip_debug_errprofile_groups.argtypes = [vp, C.c_int]
    L.ffhip_debug_batch_clear_stretches.argtypes = [vp]
    L.ffhip_debug_map_truth_bound.restype = C.c_longlong
    L.ffhip_debug_map_truth_bound.argtypes = [C.c_int, C.c_int]
    _LIB = L
    return L


SPLIT_FORMS = ("one_tile", "pair_tiles", "dense3", "dense256", "pack", "none")


def split_plan(kind: int, hidden: int, remaining: int, ncu: int, beside: int) -> dict:
    """ffhip_debug_split_plan: the layer launch the split-operand kernels take for `remaining` read tiles of a batch (no device, no engine; reads FFHIP_DEBUG)"""
    out = (C.c_int * 6)()
    _check(lib().ffhip_debug_split_plan(C.c_int(kind), C.c_int(hidden), C.c_int(remaining), C.c_int(ncu), C.c_int(beside), out))
    return {"form": SPLIT_FORMS[out[0]], "nrt": out[1], "ts": out[2], "workgroups": out[3], "per_cu": out[4], "fills_chip": out[5]}


RESULT_FIELDS = ("sat", "abort", "lens", "score", "bases", "quals", "nrun", "fail", "len", "base", "est", "shape", "scale", "dwell", "ml", "mv")
RESULT_SECTIONS = ("head", "core", "runs", "records", "mod", "moves")


def result_layout(nread: int, cap_reads: int, Tb: int, sections=()) -> dict:
    """ffhip_debug_result_layout: byte offset of every field and end of every section of a batch's result block that holds `sections` (names of RESULT_SECTIONS; no device, no engine)"""
    n = len(RESULT_FIELDS) + len(RESULT_SECTIONS)
    out = (C.c_size_t * n)()
    mask = sum(1 << RESULT_SECTIONS.index(s) for s in sections)
    _check(lib().ffhip_debug_result_layout(nread, cap_reads, Tb, mask, out, n))
    return {"field": dict(zip(RESULT_FIELDS, out[:len(RESULT_FIELDS)])), "end": dict(zip(RESULT_SECTIONS, out[len(RESULT_FIELDS):]))}


def split_pair_ok(kind: int, hidden: int, nrt: int, ncu: int) -> int:
    """ffhip_debug_split_pair_ok: two batches of nrt read tiles each may share paired layer launches (no device, no engine; reads FFHIP_DEBUG)"""
    return int(lib().ffhip_debug_split_pair_ok(C.c_int(kind), C.c_int(hidden), C.c_int(nrt), C.c_int(ncu)))


def _check(rc: int):
    if rc != 0:
        raise FFHipError("ffhip error %d: %s" % (rc, lib().ffhip_last_error().decode()))


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Engine:
    """One per GPU (ffhip_engine)."""

    def __init__(self, device: int = 0):
        self.h = lib().ffhip_engine_create(device)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())
        self.device = device

    def info(self):
        name = C.create_string_buffer(64)
        ncu, clk = C.c_int(), C.c_int()
        _check(lib().ffhip_engine_info(self.h, name, 64, C.byref(ncu), C.byref(clk)))
        return dict(arch=name.value.decode(), ncu=ncu.value, clock_khz=clk.value)

    def synchronize(self):
        _check(lib().ffhip_engine_synchronize(self.h))

    def f32_reruns(self) -> int:
        return int(lib().ffhip_engine_f32_reruns(self.h))

    def gate_math(self, form: str, x: np.ndarray) -> np.ndarray:
        """ffhip_debug_gate_math: the layer kernels' gate function `form` (GATE_FORMS) of every element of x, on the device"""
        x = np.ascontiguousarray(x, dtype=np.float32).ravel()
        out = np.empty_like(x)
        L = lib()
        L.ffhip_debug_gate_math.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]
        if x.size:
            _check(L.ffhip_debug_gate_math(self.h, GATE_FORMS.index(form), _fptr(x), _fptr(out), x.size))
        return out

    def set_profiling(self, on: bool):
        _check(lib().ffhip_engine_set_profiling(self.h, int(on)))

    def close(self):
        if self.h:
            lib().ffhip_engine_destroy(self.h)
            self.h = None


class DeviceModel:
    """Weights resident in HBM (ffhip_model), built from a flappie_amd.model.FlipflopModel."""

    def __init__(self, engine: Engine, mdl: M.FlipflopModel):
        self.engine = engine
        self.model = mdl
        keep = []

        def mk(mat: M.Mat):
            data = np.ascontiguousarray(mat.data, dtype=np.float32)
            cm = CMat(mat.nr, mat.nrq, mat.nc, mat.stride, _fptr(data), None, 0)
            keep.append((data, cm))
            return C.pointer(cm)

        d = CModelDesc()
        d.kind = mdl.kind
        d.nconv = len(mdl.convs)
        for i, cv in enumerate(mdl.convs):
            d.conv_W[i] = mk(cv.W)
            d.conv_b[i] = mk(cv.b)
            d.conv_stride[i] = cv.stride
        for i, r in enumerate(mdl.rnns):
            d.rnn_iW[i] = mk(r.iW)
            d.rnn_sW[i] = mk(r.sW)
            d.rnn_b[i] = mk(r.b)
        d.FF_W = mk(mdl.FF_W)
        d.FF_b = mk(mdl.FF_b)
        self.h = lib().ffhip_model_upload(engine.h, C.byref(d))
        del keep
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())

    @property
    def launch_reads(self) -> int:
        """reads per batch that keep every layer launch of this model full on this device (ffhip_model_launch_reads)"""
        return int(lib().ffhip_model_launch_reads(self.h))

    @property
    def stride(self) -> int:
        """samples a block: the product of the convolution strides (ffhip_model_stride)"""
        return int(lib().ffhip_model_stride(self.h))

    def close(self):
        if self.h:
            lib().ffhip_model_free(self.h)
            self.h = None


PREP_MEDMAD, PREP_DELTA, PREP_NONE = 0, 1, 2


class Prepared:
    """Raw reads trimmed and normalised on the device (ffhip_prep): trim_and_segment_raw + medmad_normalise_array."""

    def __init__(self, engine: "Engine", raws: List[np.ndarray], trim_start: int = 200, trim_end: int = 10,
                 varseg_chunk: int = 100, varseg_thresh: float = 0.0, mode: int = PREP_MEDMAD, delta: float = 0.0, begin_only: bool = False,
                 calibrations=None, ranges=None):
        """begin_only: ffhip_prep_begin (the work is enqueued, the call returns); `finish()` then waits -- ranges, statistics and signals are there after it.
        calibrations: one (offset, raw_unit) per read -- `raws` are then int16 DAC values, scaled to picoamperes on the device (ffhip_prep_create_dac /
        ffhip_prep_begin_dac).  varseg_chunk = 0 (either kind of input): no trimming at all, every read whole.
        ranges: one (start, end) per read of float samples -- raw_table's `start` and `end`, the stretch the preparation starts from (default: 0 and the read's length)"""
        self.engine = engine
        self.n = len(raws)
        if calibrations is not None:
            if len(calibrations) != self.n:
                raise ValueError("one (offset, raw_unit) per read")
            if ranges is not None:
                raise ValueError("DAC reads are prepared whole: no ranges")
            darr = (CDacRead * self.n)()
            keep = [np.ascontiguousarray(r, dtype=np.int16) for r in raws]
            for i, r in enumerate(keep):
                darr[i] = CDacRead(r.ctypes.data_as(C.POINTER(C.c_int16)), r.size, float(calibrations[i][0]), float(calibrations[i][1]))
            fn = lib().ffhip_prep_begin_dac if begin_only else lib().ffhip_prep_create_dac
            self.h = fn(engine.h, darr, self.n, trim_start, trim_end, varseg_chunk, varseg_thresh, mode, delta)
            if not self.h:
                raise FFHipError(lib().ffhip_last_error().decode())
            return
        arr = (CRawTable * self.n)()
        keep = [np.ascontiguousarray(r, dtype=np.float32) for r in raws]
        if ranges is not None and len(ranges) != self.n:
            raise ValueError("one (start, end) per read")
        for i, r in enumerate(keep):
            start, end = (0, r.size) if ranges is None else ranges[i]
            arr[i] = CRawTable(None, r.size, start, end, _fptr(r))
        fn = lib().ffhip_prep_begin if begin_only else lib().ffhip_prep_create
        self.h = fn(engine.h, arr, self.n, trim_start, trim_end, varseg_chunk, varseg_thresh, mode, delta)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())

    def finish(self):
        _check(lib().ffhip_prep_finish(self.h))

    def range(self, i: int):
        s, e = C.c_size_t(0), C.c_size_t(0)
        _check(lib().ffhip_prep_range(self.h, i, C.byref(s), C.byref(e)))
        return s.value, e.value

    def stats(self, i: int):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().ffhip_prep_stats(self.h, i, C.byref(a), C.byref(b)))
        return a.value, b.value

    def signal(self, i: int) -> np.ndarray:
        s, e = self.range(i)
        out = np.zeros(max(e - s, 0), dtype=np.float32)
        _check(lib().ffhip_prep_get_signal(self.h, i, _fptr(out)))
        return out

    def close(self):
        if self.h:
            lib().ffhip_prep_destroy(self.h)
            self.h = None


class Barcodes:
    """A barcode kit on the device (ffhip_barcodes): `seqs` are 1 .. 128 patterns over ACGT of 1 .. 128 bases, `window` the bases searched at each end of a call."""

    def __init__(self, engine: Engine, seqs, window: int = 150):
        self.engine = engine
        self.seqs = [x if isinstance(x, bytes) else str(x).encode() for x in seqs]
        self.n, self.window = len(self.seqs), int(window)
        arr = (C.c_char_p * max(1, self.n))(*self.seqs)
        self.h = lib().ffhip_barcodes_upload(engine.h, self.n, arr, self.window)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())

    def close(self):
        if self.h:
            lib().ffhip_barcodes_free(self.h)
            self.h = None


class Adapters:
    """An adapter kit on the device (ffhip_adapters): `seqs` are 1 .. 32 patterns over ACGT of 1 .. 64 bases, each searched as given and as its reverse complement."""

    def __init__(self, engine: Engine, seqs):
        self.engine = engine
        self.seqs = [x if isinstance(x, bytes) else str(x).encode() for x in seqs]
        self.n = len(self.seqs)
        arr = (C.c_char_p * max(1, self.n))(*self.seqs)
        self.h = lib().ffhip_adapters_upload(engine.h, self.n, arr)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())

    def close(self):
        if self.h:
            lib().ffhip_adapters_free(self.h)
            self.h = None


class MapRef:
    """A reference on the device (ffhip_map_ref): `seqs` are 1 .. 1024 records over ACGT of 1 or more bases, at most 2^20 together, each searched on both strands."""

    def __init__(self, engine: Engine, seqs):
        self.engine = engine
        self.seqs = [x if isinstance(x, bytes) else str(x).encode() for x in seqs]
        self.n = len(self.seqs)
        self.lens = [len(x) for x in self.seqs]
        arr = (C.c_char_p * max(1, self.n))(*self.seqs)
        self.h = lib().ffhip_map_ref_upload(engine.h, self.n, arr)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())

    def close(self):
        if self.h:
            lib().ffhip_map_ref_free(self.h)
            self.h = None


class _Pile:
    """What the run-wide accumulators share: an object of the library `_name` (ffhip_<_name>_create, _reset, _free and, for one that counts by a reference's
    positions, _positions), made from the arguments of create or FFHipError."""
    _name, _by_position = None, True

    def _create(self, engine: Engine, *args):
        self.engine = engine
        self.h = getattr(lib(), "ffhip_%s_create" % self._name)(engine.h, *args)
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())
        if self._by_position:
            self.positions = int(getattr(lib(), "ffhip_%s_positions" % self._name)(self.h))

    def reset(self):
        _check(getattr(lib(), "ffhip_%s_reset" % self._name)(self.h))

    def close(self):
        if self.h:
            getattr(lib(), "ffhip_%s_free" % self._name)(self.h)
            self.h = None


class Pileup(_Pile):
    """Per-position counts over all the reads of all the batches it is attached to (ffhip_pileup, include/ffhip.h "pileup"): 12 planes [strand][A C G T del ins]
    of P uint32 and eight uint64 totals on the device.  `min_identity` in per mille (0 .. 1000) is fixed here.  `ref` must outlive it, and it every batch it is attached to."""
    _name = "pileup"

    def __init__(self, engine: Engine, ref: MapRef, min_identity: int = 0):
        self.ref = ref
        self._create(engine, ref.h, int(min_identity))

    def download(self):
        """(counts uint32 [2][6][P], totals dict of PILEUP_TOTALS) once every accumulation enqueued by any batch is done (ffhip_pileup_download)"""
        counts = np.zeros((2, 6, self.positions), dtype=np.uint32)
        tot = np.zeros(len(PILEUP_TOTALS), dtype=np.uint64)
        _check(lib().ffhip_pileup_download(self.h, counts.ctypes.data_as(C.POINTER(C.c_uint32)), tot.ctypes.data_as(C.POINTER(C.c_uint64))))
        return counts, {k: int(v) for k, v in zip(PILEUP_TOTALS, tot)}


class ModPileup(_Pile):
    """Per reference C (- strand: G), how the aligned calls of all the batches it is attached to class their 5mC bytes (ffhip_modpileup, include/ffhip.h "mod pileup"):
    10 planes [strand][mod canon fail diff del] of P uint32, eight uint64 totals and a histogram of 256 uint64 on the device.  `min_identity` in per mille and the
    byte thresholds 0 <= lo < hi <= 255 (mod: ml >= hi, canon: ml <= lo) are fixed here.  `ref` must outlive it, and it every batch it is attached to."""
    _name = "modpileup"

    def __init__(self, engine: Engine, ref: MapRef, min_identity: int = 0, lo: int = 50, hi: int = 205):
        self.ref = ref
        self._create(engine, ref.h, int(min_identity), int(lo), int(hi))

    def download(self):
        """(counts uint32 [10][P], totals dict of MODPILEUP_TOTALS, hist uint64 [256]) once every accumulation enqueued by any batch is done (ffhip_modpileup_download)"""
        counts = np.zeros((10, self.positions), dtype=np.uint32)
        tot = np.zeros(len(MODPILEUP_TOTALS), dtype=np.uint64)
        hist = np.zeros(256, dtype=np.uint64)
        u64 = C.POINTER(C.c_uint64)
        _check(lib().ffhip_modpileup_download(self.h, counts.ctypes.data_as(C.POINTER(C.c_uint32)), tot.ctypes.data_as(u64), hist.ctypes.data_as(u64)))
        return counts, {k: int(v) for k, v in zip(MODPILEUP_TOTALS, tot)}, hist


class Consensus(_Pile):
    """Per reference position, the forward letters, deletions and inserted letters of the aligned calls of all the batches it is attached to (ffhip_consensus,
    include/ffhip.h "consensus"): 37 planes of P uint32 -- A C G T del, then A C G T of each of 8 insertion columns -- and eight uint64 totals on the device, and the
    consensus called from them there.  `min_identity` in per mille (0 .. 1000) is fixed here.  `ref` must outlive it, and it every batch it is attached to."""
    _name = "consensus"

    def __init__(self, engine: Engine, ref: MapRef, min_identity: int = 0):
        self.ref = ref
        self._create(engine, ref.h, int(min_identity))

    def download(self):
        """(counts uint32 [37][P], totals dict of CONSENSUS_TOTALS) once every accumulation enqueued by any batch is done (ffhip_consensus_download)"""
        counts = np.zeros((CONSENSUS_PLANES, self.positions), dtype=np.uint32)
        tot = np.zeros(len(CONSENSUS_TOTALS), dtype=np.uint64)
        _check(lib().ffhip_consensus_download(self.h, counts.ctypes.data_as(C.POINTER(C.c_uint32)), tot.ctypes.data_as(C.POINTER(C.c_uint64))))
        return counts, {k: int(v) for k, v in zip(CONSENSUS_TOTALS, tot)}

    def call(self, min_depth: int = 3) -> np.ndarray:
        """the consensus called on the device from the counters as they stand (ffhip_consensus_call): CONSENSUS_CELL [P], one 16-byte cell a position"""
        cells = np.zeros(self.positions, dtype=CONSENSUS_CELL)
        _check(lib().ffhip_consensus_call(self.h, int(min_depth), cells.ctypes.data_as(C.c_void_p)))
        return cells


class ErrProfile(_Pile):
    """By class, what the aligned calls of all the batches it is attached to got right and wrong (ffhip_errprofile, include/ffhip.h "error profile"): the tables
    sub[4][5], ins[4], qual[94][3], ctx[1024][4], hp[4][16][33] and twelve totals, all uint64 on the device.  `min_identity` in per mille (0 .. 1000) is fixed here.
    It belongs to no reference, serves either truth mode, and must outlive every batch it is attached to."""
    _name, _by_position = "errprofile", False

    def __init__(self, engine: Engine, min_identity: int = 0):
        self._create(engine, int(min_identity))

    def download(self):
        """(counts uint64 [ERRPROFILE_TABLE_WORDS], totals dict of ERRPROFILE_TOTALS) once every accumulation enqueued by any batch is done (ffhip_errprofile_download)"""
        counts = np.zeros(ERRPROFILE_TABLE_WORDS, dtype=np.uint64)
        tot = np.zeros(len(ERRPROFILE_TOTALS), dtype=np.uint64)
        _check(lib().ffhip_errprofile_download(self.h, counts.ctypes.data_as(C.POINTER(C.c_uint64)), tot.ctypes.data_as(C.POINTER(C.c_uint64))))
        return counts, {k: int(v) for k, v in zip(ERRPROFILE_TOTALS, tot)}

    @staticmethod
    def sections(counts) -> dict:
        """the flat counts as views by section: sub, ins, qual, ctx, hp (ERRPROFILE_SECTIONS)"""
        return {name: counts[at:at + int(np.prod(shape))].reshape(shape) for name, at, shape in ERRPROFILE_SECTIONS}

    def debug_groups(self, groups: int):
        """test hook (ffhip_debug_errprofile_groups): the most workgroups of the later launches; 0: the default"""
        _check(lib().ffhip_debug_errprofile_groups(self.h, int(groups)))


def _adapter_record(header, hits) -> dict:
    """a header and its hit slots as a dict: nhit, len, kept, hits = kept tuples (start, end, pattern, orientation, dist)"""
    kept = int(header.kept)
    return {"nhit": int(header.nhit), "len": int(header.len), "kept": kept,
            "hits": [(int(hits[i].start), int(hits[i].end), int(hits[i].pattern), int(hits[i].orientation), int(hits[i].dist)) for i in range(kept)]}


BARCODE_FIELDS = ("best", "best_dist", "second_dist", "front_dist", "rear_dist", "ends", "front_end", "rear_end")


class Batch:
    """`nread` reads of `nsample` samples (ffhip_batch)."""

    def __init__(self, dmodel: DeviceModel, nread: int, nsample: int, max_reads: int = 0):
        """max_reads > 0: a PACKED batch -- nread rows of nsample samples that take up to max_reads reads, several to a row (set_signals_packed / set_prepared_packed)"""
        self.dmodel = dmodel
        self.nread, self.nsample = nread, nsample
        self.h = (lib().ffhip_batch_create_packed(dmodel.engine.h, dmodel.h, nread, nsample, max_reads) if max_reads > 0
                  else lib().ffhip_batch_create(dmodel.engine.h, dmodel.h, nread, nsample))
        if not self.h:
            raise FFHipError(lib().ffhip_last_error().decode())
        self.nblock = int(lib().ffhip_batch_nblock(self.h))
        self.P = dmodel.model.nparam
        self.nstate = dmodel.model.nstate
        self._place = None          # where each read stands: [(row, first sample, samples)] (front / head_input)

    def set_signals(self, signals: np.ndarray):
        s = np.ascontiguousarray(signals, dtype=np.float32)
        assert s.shape == (self.nread, self.nsample), s.shape
        _check(lib().ffhip_batch_set_signals(self.h, _fptr(s), s.shape[1]))
        self._place = [(r, 0, self.nsample) for r in range(self.nread)]

    def set_signals_ragged(self, signals: List[np.ndarray]):
        """reads of different lengths (each <= the batch's nsample); results are then per-read sized"""
        assert len(signals) == self.nread
        ld = max(int(x.size) for x in signals)
        buf = np.zeros((self.nread, ld), dtype=np.float32)
        lens = (C.c_size_t * self.nread)()
        for i, x in enumerate(signals):
            buf[i, :x.size] = x
            lens[i] = x.size
        _check(lib().ffhip_batch_set_signals_ragged(self.h, _fptr(buf), ld, lens))
        self._place = [(r, 0, int(x.size)) for r, x in enumerate(signals)]

    def read_nblock(self, read: int) -> int:
        return int(lib().ffhip_batch_read_nblock(self.h, read))

    def set_reads(self, raws: List[np.ndarray], starts: List[int]):
        """raw_table path: raws[i][starts[i]:starts[i]+nsample] is read i."""
        arr = (CRawTable * self.nread)()
        keep = []
        for i, (r, st) in enumerate(zip(raws, starts)):
            r = np.ascontiguousarray(r, dtype=np.float32)
            keep.append(r)
            arr[i] = CRawTable(None, r.size, st, st + self.nsample, _fptr(r))
        _check(lib().ffhip_batch_set_reads(self.h, arr))

    def set_prepared(self, prep: "Prepared", reads: List[int]):
        """device-to-device: prepared reads `reads` (all of this batch's length) become the batch's input"""
        assert len(reads) == self.nread
        idx = (C.c_int * self.nread)(*reads)
        _check(lib().ffhip_batch_set_prepared(self.h, prep.h, idx))

    def pack_plan(self, nsamples: List[int]):
        """places (ffhip_pack_plan: longest first, each into the emptiest row) of reads of these lengths in this batch's rows: (slot, block offset) per read, slot -1 where a read did not fit"""
        n = len(nsamples)
        ns = (C.c_size_t * n)(*[int(x) for x in nsamples])
        slot, off = (C.c_int * n)(), (C.c_int * n)()
        placed = lib().ffhip_pack_plan(self.dmodel.h, self.nread, self.nsample, n, ns, slot, off)
        if placed < 0:
            raise FFHipError(lib().ffhip_last_error().decode())
        return list(slot), list(off)

    def set_signals_packed(self, signals: List[np.ndarray], slots: List[int], offs: List[int]):
        """read i stands in row slots[i] from block offs[i] on; results are then indexed by read"""
        n = len(signals)
        keep = [np.ascontiguousarray(x, dtype=np.float32) for x in signals]
        ptrs = (C.POINTER(C.c_float) * n)(*[_fptr(x) for x in keep])
        ns = (C.c_size_t * n)(*[x.size for x in keep])
        _check(lib().ffhip_batch_set_signals_packed(self.h, n, ptrs, ns, (C.c_int * n)(*slots), (C.c_int * n)(*offs)))
        st = self.dmodel.model.total_stride
        self._place = [(int(slots[i]), int(offs[i]) * st, int(keep[i].size)) for i in range(n)]

    def set_prepared_packed(self, prep: "Prepared", reads: List[int], slots: List[int], offs: List[int]):
        n = len(reads)
        _check(lib().ffhip_batch_set_prepared_packed(self.h, prep.h, n, (C.c_int * n)(*reads), (C.c_int * n)(*slots), (C.c_int * n)(*offs)))

    def nreads(self) -> int:
        return int(lib().ffhip_batch_nreads(self.h))

    def run(self, temperature: float = 1.0, flags: int = 0):
        _check(lib().ffhip_batch_run(self.h, temperature, flags))

    def run_pair(self, other: "Batch", temperature: float = 1.0, flags: int = 0):
        """this batch and `other` (same model, same shape) with the recurrent layers of both as one launch per layer"""
        _check(lib().ffhip_batch_run_pair(self.h, other.h, temperature, flags))

    def paired(self) -> bool:
        return bool(lib().ffhip_batch_paired(self.h))

    def finish(self):
        _check(lib().ffhip_batch_finish(self.h))

    def basecall(self, read: int) -> str:
        n = C.c_size_t()
        p = lib().ffhip_batch_basecall(self.h, read, C.byref(n))
        if not p:
            raise FFHipError(lib().ffhip_last_error().decode())
        return C.string_at(p, n.value).decode()

    def quality(self, read: int) -> str:
        p = lib().ffhip_batch_quality(self.h, read)
        if not p:
            raise FFHipError(lib().ffhip_last_error().decode())
        return C.string_at(p).decode()

    def score(self, read: int) -> float:
        return float(lib().ffhip_batch_score(self.h, read))

    def path(self, read: int):
        path = np.zeros(self.read_nblock(read) + 1, dtype=np.int32)
        qpath = np.zeros(self.read_nblock(read) + 1, dtype=np.float32)
        _check(lib().ffhip_batch_get_path(self.h, read, path.ctypes.data_as(C.POINTER(C.c_int)), _fptr(qpath)))
        return path, qpath

    def set_run_scale(self, factors):
        """the four run-length scale factors (A, C, G, T) of the batch's later runs (ffhip_batch_set_run_scale)"""
        f = np.ascontiguousarray(factors, dtype=np.float64)
        assert f.shape == (4,)
        _check(lib().ffhip_batch_set_run_scale(self.h, f.ctypes.data_as(C.POINTER(C.c_double))))

    def rle_runs(self, read: int) -> dict:
        """run records of a run with RUN_RLE_RUNS / RUN_RLE_RECORDS (ffhip_batch_rle_runs): base (0..3), est, failed, length, and shape / scale /
        dwell (None unless the records came down)"""
        r = CRleRuns()
        _check(lib().ffhip_batch_rle_runs(self.h, read, C.byref(r)))
        return _runs_dict(r.nrun, r.base, r.est, r.shape, r.scale, r.dwell, r.failed, r.length)

    def mod_probs(self, read: int) -> np.ndarray:
        """5mC probabilities of a run with RUN_MOD_PROBS (ffhip_batch_mod_probs): one uint8 a called base, aligned with basecall(read); 0 for A, G, T"""
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        _check(lib().ffhip_batch_mod_probs(self.h, read, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint8)

    def moves(self, read: int) -> np.ndarray:
        """move table of a run with RUN_MOVES (ffhip_batch_moves): one uint8 a block, 1 where the block's transition emits a base of basecall(read)"""
        p, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        _check(lib().ffhip_batch_moves(self.h, read, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint8)

    def set_barcodes(self, kit, max_dist: int = -1, min_sep: int = -1, both_ends: bool = False):
        """the kit and parameters of later runs with RUN_BARCODES (ffhip_batch_set_barcodes); max_dist < 0: floor(Lmin / 4), min_sep < 0: 3; kit None detaches"""
        _check(lib().ffhip_batch_set_barcodes(self.h, kit.h if kit is not None else None, int(max_dist), int(min_sep), int(bool(both_ends))))

    def set_adapters(self, kit, max_dist: int = -1):
        """the kit and bound of later runs with RUN_ADAPTERS (ffhip_batch_set_adapters); max_dist < 0: floor(L / 4) of each pattern; kit None detaches"""
        _check(lib().ffhip_batch_set_adapters(self.h, kit.h if kit is not None else None, int(max_dist)))

    def set_map(self, ref, window: int = -1, max_error: int = -1):
        """the reference, window and bound (per mille) of later runs with RUN_MAP (ffhip_batch_set_map); negative: the defaults 4096 and 250; ref None detaches"""
        _check(lib().ffhip_batch_set_map(self.h, ref.h if ref is not None else None, int(window), int(max_error)))

    def map(self, read: int) -> dict:
        """map record of a run with RUN_MAP (ffhip_batch_map): status, n, nanchor, q, tstart, tend, anchors = two dicts (q, start, end, dist, second), raw"""
        rec = CMapCall()
        _check(lib().ffhip_batch_map(self.h, read, C.byref(rec)))
        return _map_record(rec)

    def adapters(self, read: int) -> dict:
        """adapter record of a run with RUN_ADAPTERS (ffhip_batch_adapters): nhit, len, kept, hits = kept tuples (start, end, pattern, orientation, dist) by (end, q)"""
        h, hits = CAdapterHeader(), C.POINTER(CAdapterHit)()
        _check(lib().ffhip_batch_adapters(self.h, read, C.byref(h), C.byref(hits)))
        return _adapter_record(h, hits)

    def set_polytail(self, **params):
        """the parameters of later runs with RUN_POLYTAIL (ffhip_batch_set_polytail): the fields of POLYTAIL_DEFAULTS by name, the others at their defaults;
        set_polytail(detach=True) detaches"""
        if params.pop("detach", False):
            _check(lib().ffhip_batch_set_polytail(self.h, None))
            return
        p = _polytail_params(params)
        _check(lib().ffhip_batch_set_polytail(self.h, C.byref(p)))

    def polytail(self, read: int):
        """poly tail record of a run with RUN_POLYTAIL (ffhip_batch_polytail): a numpy record of POLYTAIL_DTYPE"""
        out = np.zeros((), POLYTAIL_DTYPE)
        _check(lib().ffhip_batch_polytail(self.h, read, out.ctypes.data_as(C.c_void_p)))
        return out

    def barcode(self, read: int) -> dict:
        """barcode record of a run with RUN_BARCODES (ffhip_batch_barcode): the fields of BARCODE_FIELDS as ints"""
        c = CBarcodeCall()
        _check(lib().ffhip_batch_barcode(self.h, read, C.byref(c)))
        return {f: int(getattr(c, f)) for f in BARCODE_FIELDS}

    def set_remap(self, seqs, band: int = 2048):
        """the sequences and band of later runs with RUN_REMAP (ffhip_batch_set_remap): one entry a read, None (no sequence) or codes 0 .. nbase - 1 in signal order; seqs None detaches"""
        if seqs is None:
            _check(lib().ffhip_batch_set_remap(self.h, 0, None, None, int(band)))
            return
        n = len(seqs)
        arrs = [None if q is None else np.ascontiguousarray(q, dtype=np.uint8) for q in seqs]
        ptrs = (C.POINTER(C.c_uint8) * max(1, n))()
        lens = (C.c_size_t * max(1, n))()
        dummy = np.zeros(1, np.uint8)
        for r, a in enumerate(arrs):
            if a is not None:
                ptrs[r] = (a if a.size else dummy).ctypes.data_as(C.POINTER(C.c_uint8))
                lens[r] = a.size
        _check(lib().ffhip_batch_set_remap(self.h, n, ptrs, lens, int(band)))

    def remap(self, read: int) -> dict:
        """remap record of a run with RUN_REMAP (ffhip_batch_remap): status, L, score (float32), rm (uint8 [nblock], None unless status is 1), nblock"""
        c = CRemapCall()
        _check(lib().ffhip_batch_remap(self.h, read, C.byref(c)))
        rm = np.ctypeslib.as_array(c.rm, shape=(c.nblock,)).copy() if c.status == 1 and c.nblock else None
        return {"status": int(c.status), "L": int(c.L), "score": np.float32(c.score), "rm": rm, "nblock": int(c.nblock)}

    def events(self, read: int):
        """events of a run with RUN_REMAP | RUN_EVENTS (ffhip_batch_events): a structured array (EVENT_DTYPE) of L entries, base after base; None unless the read's remap status is 1"""
        ev, n = C.c_void_p(), C.c_size_t()
        _check(lib().ffhip_batch_events(self.h, read, C.byref(ev), C.byref(n)))
        if not ev.value:
            return None
        return np.frombuffer(C.string_at(ev.value, n.value * EVENT_DTYPE.itemsize), dtype=EVENT_DTYPE).copy()

    def set_remap_mods(self, context: int = 15, all_paths: bool = False):
        """the context (0 .. 31 positions either side of a site) and the mode (best path, or all paths in fp64) of later runs with RUN_REMAP_MODS (ffhip_batch_set_remap_mods)"""
        _check(lib().ffhip_batch_set_remap_mods(self.h, int(context), 1 if all_paths else 0))

    def site_mods(self, read: int):
        """site mods of a run with RUN_REMAP | RUN_REMAP_MODS (ffhip_batch_site_mods): a structured array (SITE_MOD_DTYPE), one entry a C / Z of the read's sequence in increasing pos; None unless the read's remap status is 1"""
        sm, n = C.c_void_p(), C.c_size_t()
        _check(lib().ffhip_batch_site_mods(self.h, read, C.byref(sm), C.byref(n)))
        if not sm.value:
            return None
        return np.frombuffer(C.string_at(sm.value, n.value * SITE_MOD_DTYPE.itemsize), dtype=SITE_MOD_DTYPE).copy()

    def set_remap_variants(self, variants, context: int = 10, all_paths: bool = False):
        """the variants, the context (1 .. 23 positions either side of an edit) and the mode (best path, or all paths in fp64) of later runs with RUN_REMAP_VARIANTS
        (ffhip_batch_set_remap_variants; after set_remap): one entry a read, None or an array of VARIANT_DTYPE (make_variants); variants None detaches"""
        if variants is None:
            _check(lib().ffhip_batch_set_remap_variants(self.h, 0, None, None, int(context), 1 if all_paths else 0))
            return
        keep = [None if v is None else np.ascontiguousarray(v, dtype=VARIANT_DTYPE) for v in variants]
        n = len(keep)
        ptrs = (C.c_void_p * max(1, n))(*[None if v is None or v.size == 0 else v.ctypes.data for v in keep])
        lens = (C.c_size_t * max(1, n))(*[0 if v is None else v.size for v in keep])
        _check(lib().ffhip_batch_set_remap_variants(self.h, n, ptrs, lens, int(context), 1 if all_paths else 0))

    def variant_calls(self, read: int):
        """the records of a run with RUN_REMAP | RUN_REMAP_VARIANTS (ffhip_batch_variant_calls): a structured array (VARIANT_CALL_DTYPE), one entry a variant of the
        read's list in list order; None unless the read's remap status is 1"""
        vc, n = C.c_void_p(), C.c_size_t()
        _check(lib().ffhip_batch_variant_calls(self.h, read, C.byref(vc), C.byref(n)))
        if not vc.value:
            return None
        return np.frombuffer(C.string_at(vc.value, n.value * VARIANT_CALL_DTYPE.itemsize), dtype=VARIANT_CALL_DTYPE).copy()

    def set_truth(self, seqs, band: int = 512):
        """the truths and band of later runs with RUN_TRUTH (ffhip_batch_set_truth): one entry a read, None (no truth) or codes 0 .. nbase - 1 in signal order; seqs None detaches"""
        if seqs is None:
            _check(lib().ffhip_batch_set_truth(self.h, 0, None, None, int(band)))
            return
        n = len(seqs)
        arrs = [None if q is None else np.ascontiguousarray(q, dtype=np.uint8) for q in seqs]
        ptrs = (C.POINTER(C.c_uint8) * max(1, n))()
        lens = (C.c_size_t * max(1, n))()
        dummy = np.zeros(1, np.uint8)
        for r, a in enumerate(arrs):
            if a is not None:
                ptrs[r] = (a if a.size else dummy).ctypes.data_as(C.POINTER(C.c_uint8))
                lens[r] = a.size
        _check(lib().ffhip_batch_set_truth(self.h, n, ptrs, lens, int(band)))

    def set_remap_from_map(self, on: bool = True, band: int = 2048):
        """later runs with RUN_MAP | RUN_REMAP take each read's sequence from its map record (ffhip_batch_set_remap_from_map); it and set_remap replace each other"""
        _check(lib().ffhip_batch_set_remap_from_map(self.h, 1 if on else 0, int(band)))

    def set_truth_from_map(self, on: bool = True, band: int = 512):
        """later runs with RUN_MAP | RUN_TRUTH take each read's truth from its map record (ffhip_batch_set_truth_from_map); it and set_truth replace each other"""
        _check(lib().ffhip_batch_set_truth_from_map(self.h, 1 if on else 0, int(band)))

    def set_pileup(self, pileup):
        """the Pileup that later runs with RUN_MAP | RUN_TRUTH | RUN_PILEUP add to when they are finished (ffhip_batch_set_pileup); None detaches"""
        _check(lib().ffhip_batch_set_pileup(self.h, pileup.h if pileup is not None else None))

    def set_modpileup(self, modpileup):
        """the ModPileup that later runs with RUN_MAP | RUN_TRUTH | RUN_MOD_PROBS | RUN_MOD_PILEUP add to when they are finished (ffhip_batch_set_modpileup); None detaches"""
        _check(lib().ffhip_batch_set_modpileup(self.h, modpileup.h if modpileup is not None else None))

    def set_consensus(self, consensus):
        """the Consensus that later runs with RUN_MAP | RUN_TRUTH | RUN_CONSENSUS add to when they are finished (ffhip_batch_set_consensus); None detaches"""
        _check(lib().ffhip_batch_set_consensus(self.h, consensus.h if consensus is not None else None))

    def set_errprofile(self, errprofile):
        """the ErrProfile that later runs with RUN_TRUTH | RUN_ERRPROFILE add to when they are finished (ffhip_batch_set_errprofile); None detaches"""
        _check(lib().ffhip_batch_set_errprofile(self.h, errprofile.h if errprofile is not None else None))

    def debug_clear_stretches(self):
        """test hook (ffhip_debug_batch_clear_stretches): between a run in the mode of truth from map and its finish, zero the gathered stretches behind k_truth"""
        _check(lib().ffhip_debug_batch_clear_stretches(self.h))

    def truth(self, read: int) -> dict:
        """truth record of a run with RUN_TRUTH (ffhip_batch_truth): TRUTH_FIELDS as ints and ops (uint8 [dist + n_match] in path order, None unless status is 1)"""
        c = CTruthCall()
        _check(lib().ffhip_batch_truth(self.h, read, C.byref(c)))
        return _truth_dict(c, np.ctypeslib.as_array(c.ops, shape=(c.nops,)).copy() if c.status == 1 and c.nops else None)

    def transitions(self, read: int) -> np.ndarray:
        out = np.zeros((self.read_nblock(read), self.P), dtype=np.float32)
        _check(lib().ffhip_batch_get_transitions(self.h, read, _fptr(out)))
        return out

    def posterior(self, read: int) -> np.ndarray:
        out = np.zeros((self.read_nblock(read), self.P), dtype=np.float32)
        _check(lib().ffhip_batch_get_posterior(self.h, read, _fptr(out)))
        return out

    def trace(self, read: int) -> np.ndarray:
        out = np.zeros((self.read_nblock(read) + 1, self.nstate), dtype=np.int32)
        _check(lib().ffhip_batch_get_trace(self.h, read, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def activation(self, layer: int, read: int) -> np.ndarray:
        out = np.zeros((self.nblock, self.dmodel.model.hidden), dtype=np.float32)
        _check(lib().ffhip_batch_get_activation(self.h, layer, read, _fptr(out)))
        return out

    def rnn_path(self) -> int:
        """0 launch per step, 1 persistent recurrence + projection GEMM, 2 fused f32 layer kernel, 3 split-operand (fp16 x 2) layer kernel, 4 split-operand projection GEMM + recurrence-only split layer kernel"""
        L = lib()
        L.ffhip_batch_rnn_path.argtypes = [C.c_void_p]
        L.ffhip_batch_rnn_path.restype = C.c_int
        return int(L.ffhip_batch_rnn_path(self.h))

    # ---- debug read-outs (ffhip_debug_batch_*): the convolutions' and the head's own outputs and inputs; they change nothing a run launches
    def keep_front(self, on: bool = True):
        """from the next run on, keep the last convolution's output for front() (one device-to-device copy behind the convolution group)"""
        _check(lib().ffhip_debug_batch_keep_front(self.h, int(on)))

    def _span(self, layer: int, read: int):
        """(row, first column, columns) of `read` in the output of convolution `layer` (layer = nconv: the blocks)"""
        row, x0, n = self._place[read]
        convs = self.dmodel.model.convs
        before = int(np.prod([c.stride for c in convs[:layer + 1]])) if layer >= 0 else 1
        return row, x0 // before, -(-n // before)

    def front_row(self, layer: int, row: int) -> np.ndarray:
        """convolution `layer`'s output over the whole batch row, padding columns included: [Tout][filters]"""
        cv = self.dmodel.model.convs[layer]
        tout = self.nsample
        for c in self.dmodel.model.convs[:layer + 1]:
            tout = -(-tout // c.stride)
        out = np.zeros((tout, cv.W.nc), dtype=np.float32)
        _check(lib().ffhip_debug_batch_front(self.h, layer, row, _fptr(out)))
        return out

    def front(self, layer: int, read: int) -> np.ndarray:
        """convolution `layer`'s output for `read` alone (its columns of its row)"""
        row, c0, n = self._span(layer, read)
        return self.front_row(layer, row)[c0:c0 + n]

    def head_input_row(self, row: int) -> np.ndarray:
        """the last recurrent layer's output over the whole batch row, as the CRF head read it: [nblock][hidden]"""
        out = np.zeros((self.nblock, self.dmodel.model.hidden), dtype=np.float32)
        _check(lib().ffhip_debug_batch_head_input(self.h, row, _fptr(out)))
        return out

    def head_input(self, read: int) -> np.ndarray:
        row, c0, n = self._span(len(self.dmodel.model.convs) - 1, read)
        return self.head_input_row(row)[c0:c0 + n]

    def forms(self):
        """kernel forms of the last run: [form of each convolution], form of the head (names of FORMS)"""
        out = (C.c_int * 4)()
        _check(lib().ffhip_debug_batch_forms(self.h, out))
        nconv = len(self.dmodel.model.convs)
        return [FORMS.get(out[i], out[i]) for i in range(nconv)], FORMS.get(out[3], out[3])

    def device_bytes(self) -> int:
        """device memory the batch object holds (ffhip_debug_batch_device_bytes): its buffers, grown on first use by the paths its runs took"""
        return int(lib().ffhip_debug_batch_device_bytes(self.h))

    def f32_reruns(self) -> int:
        """reads of the last run that left the split operand format's range and were run again on the f32 path (ffhip_batch_finish)"""
        return int(lib().ffhip_batch_f32_reruns(self.h))

    def profile(self):
        ms = (C.c_float * NGROUP)()
        ln = (C.c_int * NGROUP)()
        _check(lib().ffhip_batch_profile(self.h, ms, ln))
        return {GROUP_NAMES[i]: dict(ms=float(ms[i]), launches=int(ln[i])) for i in range(NGROUP)}

    def close(self):
        if self.h:
            lib().ffhip_batch_destroy(self.h)
            self.h = None


def _runs_dict(n, base, est, shape, scale, dwell, failed, length) -> dict:
    def arr(p, dt):
        return None if not p else np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt)
    return dict(base=arr(base, np.uint8), est=arr(est, np.int32), shape=arr(shape, np.float32), scale=arr(scale, np.float32),
                dwell=arr(dwell, np.int32), failed=bool(failed), length=int(length))


def rle_runs_op(engine: Engine, param: np.ndarray, path: np.ndarray, factors=None, records: bool = True) -> dict:
    """ffhip_op_rle_runs: run records of ONE run-length matrix param [nblock][nparam] (the layout Batch.posterior returns) and its path (nblock
    entries, states 0 .. 2 nbase - 1); factors None: the defaults"""
    param = np.ascontiguousarray(param, dtype=np.float32)
    nblock, nparam = param.shape
    path = np.ascontiguousarray(path[:nblock], dtype=np.int32)
    assert path.shape == (nblock,)
    n = max(nblock, 1)
    base, est = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    shape, scale, dwell = (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)) if records else (None, None, None)
    f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)
    nrun, failed, length = C.c_size_t(), C.c_int(), C.c_ulonglong()

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))
    _check(lib().ffhip_op_rle_runs(engine.h, CFMat(_fptr(param), nparam, nblock, nparam), ptr(path, C.c_int), ptr(f, C.c_double), C.byref(nrun),
                                   ptr(base, C.c_uint8), ptr(est, C.c_int32), ptr(shape, C.c_float), ptr(scale, C.c_float), ptr(dwell, C.c_int32),
                                   C.byref(failed), C.byref(length)))
    k = nrun.value
    return dict(base=base[:k].copy(), est=est[:k].copy(), shape=None if shape is None else shape[:k].copy(), scale=None if scale is None else scale[:k].copy(),
                dwell=None if dwell is None else dwell[:k].copy(), failed=bool(failed.value), length=int(length.value))


def mod_probs_op(engine: Engine, logpost: np.ndarray, path: np.ndarray) -> np.ndarray:
    """ffhip_op_mod_probs: 5mC probabilities of ONE log posterior [nblock][60] (the layout Batch.posterior returns) and its path (the first nblock entries
    are used, states 0 .. 9): one uint8 a called base"""
    logpost = np.ascontiguousarray(logpost, dtype=np.float32)
    nblock, nparam = logpost.shape
    path = np.ascontiguousarray(path[:nblock], dtype=np.int32)
    assert path.shape == (nblock,)
    ml, n = np.zeros(max(nblock, 1), np.uint8), C.c_size_t()
    _check(lib().ffhip_op_mod_probs(engine.h, CFMat(_fptr(logpost), nparam, nblock, nparam), path.ctypes.data_as(C.POINTER(C.c_int)),
                                    ml.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n)))
    return ml[:n.value].copy()


def moves_op(engine: Engine, path: np.ndarray) -> np.ndarray:
    """ffhip_op_moves: the move table of ONE path of nblock + 1 entries: nblock uint8"""
    path = np.ascontiguousarray(path, dtype=np.int32)
    assert path.ndim == 1 and path.size >= 2
    mv = np.zeros(path.size - 1, np.uint8)
    _check(lib().ffhip_op_moves(engine.h, path.ctypes.data_as(C.POINTER(C.c_int)), path.size - 1, mv.ctypes.data_as(C.POINTER(C.c_uint8))))
    return mv


def op_barcode_scores(engine: Engine, kit: Barcodes, bases) -> tuple:
    """ffhip_op_barcode_scores: (dist, end), each int32 [2][n] (front, rear), of every pattern of the kit at both ends of ONE call (a str over ACGTZ, may be empty)"""
    b = bases if isinstance(bases, bytes) else str(bases).encode()
    dist, end = np.zeros((2, kit.n), np.int32), np.zeros((2, kit.n), np.int32)
    _check(lib().ffhip_op_barcode_scores(engine.h, kit.h, b, len(b), dist.ctypes.data_as(C.POINTER(C.c_int32)), end.ctypes.data_as(C.POINTER(C.c_int32))))
    return dist, end


def op_adapter_scores(engine: Engine, kit: Adapters, bases) -> np.ndarray:
    """ffhip_op_adapter_scores: the whole score rows uint8 [2 n][len + 1], row q = 2 k + orientation, of ONE call (a str over ACGTZ, may be empty)"""
    b = bases if isinstance(bases, bytes) else str(bases).encode()
    d = np.zeros((2 * kit.n, len(b) + 1), np.uint8)
    _check(lib().ffhip_op_adapter_scores(engine.h, kit.h, b, len(b), d.ctypes.data_as(C.POINTER(C.c_uint8))))
    return d


def op_adapter_hits(engine: Engine, kit: Adapters, bases, max_dist: int = -1) -> dict:
    """ffhip_op_adapter_hits: the record of ONE call, as Batch.adapters gives it; "raw": the 15 hit slots as 60 int32 (the slots no hit took are zero)"""
    b = bases if isinstance(bases, bytes) else str(bases).encode()
    h, hits = CAdapterHeader(), (CAdapterHit * ADAPTER_MAX_HITS)()
    _check(lib().ffhip_op_adapter_hits(engine.h, kit.h, int(max_dist), b, len(b), C.byref(h), hits))
    rec = _adapter_record(h, hits)
    rec["raw"] = np.frombuffer(bytes(hits), np.int32).copy()
    return rec


def op_map_scores(engine: Engine, ref: MapRef, pattern) -> list:
    """ffhip_op_map_scores: the whole score rows of ONE anchor (a str over ACGTZ of 1 .. 4096 letters): a list of 2 K int32 arrays, row q = 2 k + strand of m_k + 1 entries"""
    b = pattern if isinstance(pattern, bytes) else str(pattern).encode()
    d = np.zeros(2 * sum(m + 1 for m in ref.lens), np.int32)
    _check(lib().ffhip_op_map_scores(engine.h, ref.h, b, len(b), d.ctypes.data_as(C.POINTER(C.c_int32))))
    rows, at = [], 0
    for m in ref.lens:
        for _ in range(2):
            rows.append(d[at:at + m + 1])
            at += m + 1
    return rows


def op_map(engine: Engine, ref: MapRef, bases, window: int = -1, max_error: int = -1) -> dict:
    """ffhip_op_map: the record of ONE call (a str over ACGTZ, may be empty), as Batch.map gives it"""
    b = bases if isinstance(bases, bytes) else str(bases).encode()
    rec = CMapCall()
    _check(lib().ffhip_op_map(engine.h, ref.h, int(window), int(max_error), b, len(b), C.byref(rec)))
    return _map_record(rec)


def op_pileup(engine: Engine, pileup: Pileup, q: int, tstart: int, tend: int, call, ops):
    """ffhip_op_pileup: ONE alignment -- search q, span [tstart, tend), the call's letters (A C G T Z, signal order) and its ops (0 .. 3, path order) -- added into `pileup`"""
    s = call if isinstance(call, bytes) else str(call).encode()
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    _check(lib().ffhip_op_pileup(engine.h, pileup.h, int(q), int(tstart), int(tend), s, len(s), (o if o.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), o.size))


def op_consensus(engine: Engine, consensus: Consensus, q: int, tstart: int, tend: int, call, ops):
    """ffhip_op_consensus: ONE alignment -- search q, span [tstart, tend), the call's letters and its ops (0 .. 3) -- added into `consensus` by the kernel of the batches"""
    s = call if isinstance(call, bytes) else str(call).encode()
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    _check(lib().ffhip_op_consensus(engine.h, consensus.h, int(q), int(tstart), int(tend), s, len(s), (o if o.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), o.size))


def _errprofile_args(call, qual, ops):
    s = call if isinstance(call, bytes) else str(call).encode()
    qb = qual if isinstance(qual, bytes) else bytes(qual) if not isinstance(qual, str) else qual.encode("latin-1")
    if len(qb) != len(s):
        raise ValueError("a quality character a letter of the call")
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    return s, qb, o, (o if o.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8))


def op_errprofile(engine: Engine, errprofile: ErrProfile, call, qual, truth, ops):
    """ffhip_op_errprofile: ONE alignment -- the call's letters, its quality characters (bytes), the truth's codes 0 .. 4 and its ops (0 .. 3) -- added into `errprofile`"""
    s, qb, o, op = _errprofile_args(call, qual, ops)
    t = np.ascontiguousarray(truth, dtype=np.uint8)
    _check(lib().ffhip_op_errprofile(engine.h, errprofile.h, s, qb, len(s), (t if t.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), t.size, op, o.size))


def op_errprofile_mapped(engine: Engine, errprofile: ErrProfile, ref: MapRef, q: int, tstart: int, tend: int, call, qual, ops):
    """ffhip_op_errprofile_mapped: the same with the truth's letters from the span [tstart, tend) of search q of `ref`"""
    s, qb, o, op = _errprofile_args(call, qual, ops)
    _check(lib().ffhip_op_errprofile_mapped(engine.h, errprofile.h, ref.h, int(q), int(tstart), int(tend), s, qb, len(s), op, o.size))


def op_modpileup(engine: Engine, modpileup: ModPileup, q: int, tstart: int, tend: int, call, ml, ops):
    """ffhip_op_modpileup: ONE alignment -- search q, span [tstart, tend), the call's letters, its 5mC bytes (one a letter) and its ops (0 .. 3) -- added into `modpileup`"""
    s = call if isinstance(call, bytes) else str(call).encode()
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    u8 = C.POINTER(C.c_uint8)
    if ml is None:
        pm = None
    else:
        v = np.ascontiguousarray(ml, dtype=np.uint8)
        if v.size != len(s):
            raise ValueError("op_modpileup: %d 5mC bytes for a call of %d letters" % (v.size, len(s)))
        pm = (v if v.size else np.zeros(1, np.uint8)).ctypes.data_as(u8)
    _check(lib().ffhip_op_modpileup(engine.h, modpileup.h, int(q), int(tstart), int(tend), s, pm, len(s), (o if o.size else np.zeros(1, np.uint8)).ctypes.data_as(u8), o.size))


def op_map_stretch(engine: Engine, ref: MapRef, q: int, start: int, end: int) -> np.ndarray:
    """ffhip_op_map_stretch: y_q[start : end] of the reference as codes 0 .. 3 (uint8 [end - start]), gathered by the kernel of truth from map"""
    out = np.zeros(max(1, int(end) - int(start)), np.uint8)
    _check(lib().ffhip_op_map_stretch(engine.h, ref.h, int(q), int(start), int(end), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out[:int(end) - int(start)]


def op_map_remap_code(engine: Engine, ref: MapRef, q: int, start: int, end: int, nbase: int, room: int, fill: int = 0xffff) -> tuple:
    """ffhip_op_map_remap_code: (entries uint16 [end - start], status, L) of y_q[start : end] in remap's coding (stay | move << 8), made by the kernel of remap from
    map for an entry of `room` positions; with status 2 the entries are `fill`, what the output held before the call"""
    n = max(1, int(end) - int(start))
    out = np.full(n, fill, np.uint16)
    status, L = C.c_int(0), C.c_size_t(0)
    _check(lib().ffhip_op_map_remap_code(engine.h, ref.h, int(q), int(start), int(end), int(nbase), int(room), out.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(status), C.byref(L)))
    return out[:max(0, int(end) - int(start))], int(status.value), int(L.value)


def remap_from_map_form(nblock: int, band: int) -> int:
    """ffhip_debug_remap_from_map_form: the kernel form a read of `nblock` blocks takes in the mode of remap from map (-1: none)"""
    return int(lib().ffhip_debug_remap_from_map_form(int(nblock), int(band)))


def map_truth_bound(nblock: int, max_error: int) -> int:
    """ffhip_debug_map_truth_bound: the most bases a mapped call's stretch can have for a read of `nblock` blocks (-1: bad arguments)"""
    return int(lib().ffhip_debug_map_truth_bound(int(nblock), int(max_error)))


def op_remap(engine: Engine, trans: np.ndarray, nbase: int, codes, band: int = 2048) -> tuple:
    """ffhip_op_remap: (rm uint8 [nblock], score float32) of ONE read's transition scores `trans` [nblock][nstate (nbase + 1)] mapped to `codes` (0 .. nbase - 1, signal order);
    scores that leave no finite path (the batch's status 2) raise FFHipError with FFHIP_EINVAL"""
    t = np.ascontiguousarray(trans, dtype=np.float32)
    q = np.ascontiguousarray(codes, dtype=np.uint8)
    rm, score = np.zeros(t.shape[0], np.uint8), C.c_float(0.0)
    _check(lib().ffhip_op_remap(engine.h, CFMat(_fptr(t), t.shape[1], t.shape[0], t.shape[1]), int(nbase), (q if q.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), q.size, int(band),
                                rm.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(score)))
    return rm, np.float32(score.value)


def _polytail_inputs(signal, path):
    x = np.ascontiguousarray(signal, dtype=np.float32)
    pth = np.ascontiguousarray(path, dtype=np.int32)
    return x, pth, (x if x.size else np.zeros(1, np.float32)).ctypes.data_as(C.POINTER(C.c_float)), (pth if pth.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int))


def op_polytail(engine: Engine, signal, stride: int, path, nbase: int, **params):
    """ffhip_op_polytail: the poly tail record (POLYTAIL_DTYPE) of ONE read from its prepared signal (float32), the model's stride and its Viterbi path (nblock + 1 states)"""
    x, pth, xp, pp = _polytail_inputs(signal, path)
    p, out = _polytail_params(params), np.zeros((), POLYTAIL_DTYPE)
    _check(lib().ffhip_op_polytail(engine.h, xp, x.size, int(stride), pp, max(pth.size, 1) - 1, int(nbase), C.byref(p), out.ctypes.data_as(C.c_void_p)))
    return out


def op_polytail_windows(engine: Engine, signal, stride: int, path, nbase: int, **params) -> tuple:
    """ffhip_op_polytail_windows: (mu float64, q float64, flag uint8) of the NW windows of ONE read, inputs as for op_polytail"""
    x, pth, xp, pp = _polytail_inputs(signal, path)
    p = _polytail_params(params)
    nblock = max(pth.size, 1) - 1
    nw = min(nblock, x.size // max(int(stride), 1)) // max(int(p.window), 1)
    mu, q, flag = np.zeros(max(nw, 1)), np.zeros(max(nw, 1)), np.zeros(max(nw, 1), np.uint8)
    _check(lib().ffhip_op_polytail_windows(engine.h, xp, x.size, int(stride), pp, nblock, int(nbase), C.byref(p), mu.ctypes.data_as(C.POINTER(C.c_double)),
                                           q.ctypes.data_as(C.POINTER(C.c_double)), flag.ctypes.data_as(C.POINTER(C.c_uint8))))
    return mu[:nw], q[:nw], flag[:nw]


def op_events(engine: Engine, signal, stride: int, rm, L: int) -> np.ndarray:
    """ffhip_op_events: the events (EVENT_DTYPE, L entries) of ONE read from its prepared signal (float32), the model's stride and its remap path rm (uint8, a byte a block)"""
    x = np.ascontiguousarray(signal, dtype=np.float32)
    m = np.ascontiguousarray(rm, dtype=np.uint8)
    out = np.zeros(max(1, int(L)), EVENT_DTYPE)
    _check(lib().ffhip_op_events(engine.h, (x if x.size else np.zeros(1, np.float32)).ctypes.data_as(C.POINTER(C.c_float)), x.size, int(stride),
                                 (m if m.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), m.size, int(L), out.ctypes.data_as(C.c_void_p)))
    return out[:int(L)]


def op_site_mods(engine: Engine, trans: np.ndarray, nbase: int, codes, rm, context: int = 15, all_paths: bool = False, stride: int = 0) -> np.ndarray:
    """ffhip_op_site_mods: the site mods (SITE_MOD_DTYPE, one entry a C / Z of `codes`) of ONE read from its transition scores `trans` [nblock][nstate (nbase + 1)],
    its sequence and its remap path rm (uint8, a byte a block); stride > trans.shape[1]: the matrix is handed over with that many floats a block"""
    t = np.ascontiguousarray(trans, dtype=np.float32)
    nparam = t.shape[1] if t.ndim == 2 else 0
    if stride > nparam and t.ndim == 2:
        wide = np.full((t.shape[0], int(stride)), np.float32(np.nan))      # (the padding is never read)
        wide[:, :nparam] = t
        t = wide
    q = np.ascontiguousarray(codes, dtype=np.uint8)
    m = np.ascontiguousarray(rm, dtype=np.uint8)
    out, n = np.zeros(max(1, q.size), SITE_MOD_DTYPE), C.c_size_t(0)
    _check(lib().ffhip_op_site_mods(engine.h, CFMat(_fptr(t), nparam, t.shape[0], t.shape[1] if t.ndim == 2 else 0), int(nbase),
                                    (q if q.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), q.size,
                                    (m if m.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), m.size, int(context), 1 if all_paths else 0,
                                    out.ctypes.data_as(C.c_void_p), C.byref(n)))
    return out[:n.value]


def make_variants(variants) -> np.ndarray:
    """an array of VARIANT_DTYPE from (pos, nref, alt codes) triples"""
    out = np.zeros(len(variants), VARIANT_DTYPE)
    for i, (pos, nref, alt) in enumerate(variants):
        alt = np.asarray(alt, np.uint8).reshape(-1)
        out[i]["pos"], out[i]["nref"], out[i]["nalt"] = int(pos), int(nref), min(alt.size, 255)
        out[i]["alt"][:min(alt.size, 16)] = alt[:16]
    return out


def op_variants(engine: Engine, trans: np.ndarray, nbase: int, codes, rm, variants, context: int = 10, all_paths: bool = False, stride: int = 0) -> np.ndarray:
    """ffhip_op_variants: the records (VARIANT_CALL_DTYPE, one entry a variant) of ONE read from its transition scores `trans` [nblock][nstate (nbase + 1)], its
    sequence, its remap path rm (uint8, a byte a block) and its variants (VARIANT_DTYPE); stride > trans.shape[1]: the matrix is handed over with that many floats a block"""
    t = np.ascontiguousarray(trans, dtype=np.float32)
    nparam = t.shape[1] if t.ndim == 2 else 0
    if stride > nparam and t.ndim == 2:
        wide = np.full((t.shape[0], int(stride)), np.float32(np.nan))      # (the padding is never read)
        wide[:, :nparam] = t
        t = wide
    q = np.ascontiguousarray(codes, dtype=np.uint8)
    m = np.ascontiguousarray(rm, dtype=np.uint8)
    v = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE)
    out = np.zeros(max(1, v.size), VARIANT_CALL_DTYPE)
    _check(lib().ffhip_op_variants(engine.h, CFMat(_fptr(t), nparam, t.shape[0], t.shape[1] if t.ndim == 2 else 0), int(nbase),
                                   (q if q.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), q.size,
                                   (m if m.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), m.size,
                                   (v if v.size else np.zeros(1, VARIANT_DTYPE)).ctypes.data_as(C.c_void_p), v.size, int(context), 1 if all_paths else 0,
                                   out.ctypes.data_as(C.c_void_p)))
    return out[:v.size]


def _truth_dict(c, ops) -> dict:
    out = {f: int(getattr(c, f)) for f in TRUTH_FIELDS}
    out["ops"] = (np.zeros(0, np.uint8) if ops is None else ops) if c.status == 1 else None
    return out


def op_truth(engine: Engine, call, codes, band: int = 512) -> dict:
    """ffhip_op_truth: the record (TRUTH_FIELDS, ops) of ONE call (letters A C G T Z, str or bytes) aligned to `codes` (0 .. 4, signal order)"""
    s = call.encode() if isinstance(call, str) else bytes(call)
    q = np.ascontiguousarray(codes, dtype=np.uint8)
    ops, c = np.zeros(max(1, len(s) + q.size), np.uint8), CTruthCall()
    _check(lib().ffhip_op_truth(engine.h, s, len(s), (q if q.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8)), q.size, int(band), C.byref(c),
                                ops.ctypes.data_as(C.POINTER(C.c_uint8))))
    return _truth_dict(c, ops[:c.nops].copy())


def truth_form(window: int) -> int:
    """ffhip_debug_truth_form: the kernel form a window of that many cells takes (-1: none)"""
    return int(lib().ffhip_debug_truth_form(int(window)))


def basecall_reads(dmodel: DeviceModel, signals: np.ndarray, temperature: float = 1.0, flags: int = 0):
    """Convenience: one batch, returns list of (basecall, quality, score)."""
    b = Batch(dmodel, signals.shape[0], signals.shape[1])
    try:
        b.set_signals(signals)
        b.run(temperature, flags)
        b.finish()
        return [(b.basecall(i), b.quality(i), b.score(i)) for i in range(b.nread)]
    finally:
        b.close()
