/*  ffhip.h -- the C-ABI between flappie's C host code and the MI355X (gfx950) HIP engine.
 *
 *  This is the thin shim the north-star asks for: plain C, plain pointers and sizes, no C++ or
 *  torch types.  It is what the reference's host code would bind instead of calling into
 *  layers.c/decode.c one read at a time.  Each entry point names the reference interface it
 *  replaces (paths relative to /root/reference/src).
 *
 *  The reference has no batching (flappie.c:364-385 loops over files; one read = one forward
 *  pass).  A GPU cannot be filled one read at a time, so the unit of work here is a BATCH of reads
 *  that share one trimmed length (SURVEY.md section 8b "what the replacement must add").  Reads are
 *  never split or padded in time: the CRF normaliser and the recurrent state are whole-read
 *  quantities (layers.c:1089, :902-916), so results are identical to per-read evaluation.
 *
 *  Error convention (flappie_stdlib.h:37-45 RETURN_NULL_IF): functions returning pointers return
 *  NULL on failure; functions returning int return 0 on success and a negative FFHIP_E* code
 *  otherwise; nothing throws, nothing aborts.  ffhip_last_error() gives a static message.
 *
 *  Threading: an engine and everything created from it belong to one host thread (the reference
 *  is single threaded).  Use one engine per GPU.
 */
#ifndef FFHIP_H
#define FFHIP_H

#include <stddef.h>
#include <stdint.h>
#include "flappie_matrix.h"
#include "flappie_structures.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFHIP_OK          0
#define FFHIP_EINVAL     -1   /* bad argument / unsupported model shape */
#define FFHIP_ENOMEM     -2   /* host or device allocation failed      */
#define FFHIP_EHIP       -3   /* a HIP runtime call failed             */
#define FFHIP_ENODEV     -4   /* no usable gfx950 device               */
#define FFHIP_ETIMEOUT   -5   /* an in-kernel wait gave up (persistent recurrent kernel) */

typedef struct ffhip_engine ffhip_engine;
typedef struct ffhip_model ffhip_model;
typedef struct ffhip_batch ffhip_batch;

enum ffhip_net_kind {
    FFHIP_NET_LSTM5 = 0,    /* flipflop5_guppy_transitions, networks.c:539-586 */
    FFHIP_NET_GRUMOD5 = 1,  /* flipflop_guppy_transitions,  networks.c:450-489 */
    FFHIP_NET_LSTM5_RLE = 2 /* runlength5_guppy_transitions, networks.c:672-725: LSTM5 trunk, globalnorm_runlengthV2 head;
                             * decode = transpost_crf_runlength + decode_crf_runlength (runnie.c:262-276): results are the
                             * path (ffhip_batch_get_path, states 0..2*nbase-1), score and parameter/posterior matrices */
};

/* Host-side weight bundle.  Mirrors `guppy_stride5_model` (networks.c:181-215) and `guppy_model`
 * (networks.c:150-178): pointers to matrices in the .mdl layout, never owned by the engine. */
typedef struct {
    int kind;                         /* enum ffhip_net_kind */
    int nconv;                        /* 3 (LSTM5: swish after each) or 1 (GRUMOD5: tanh) */
    const_flappie_matrix conv_W[3];
    const_flappie_matrix conv_b[3];
    int conv_stride[3];
    const_flappie_matrix rnn_iW[5];   /* layer order B1,F2,B3,F4,B5 */
    const_flappie_matrix rnn_sW[5];
    const_flappie_matrix rnn_b[5];
    const_flappie_matrix FF_W;
    const_flappie_matrix FF_b;
} ffhip_model_desc;

/* flags for ffhip_batch_run */
#define FFHIP_RUN_VITERBI_ONLY   1u   /* `--viterbi`: decode the transitions, skip fwd/bwd (flappie.c:277-282) */
#define FFHIP_RUN_NO_TRACE       2u   /* skip exp + trace_from_posterior (flappie.c:299-300)                  */
#define FFHIP_RUN_NO_DECODE      4u   /* stop after calculate_transitions (networks.c:108-111)                */
#define FFHIP_RUN_STEPWISE_RNN   8u   /* force the launch-per-step recurrent kernels (debug / cross-check)    */
#define FFHIP_RUN_UNFUSED_RNN   32u   /* separate input-projection GEMM + recurrent kernel (cross-check)      */
#define FFHIP_RUN_F32_RNN       64u   /* f32-input MFMA recurrent kernel instead of the split-operand (two fp16 slices) one (cross-check) */
#define FFHIP_RUN_KEEP_ACTS     16u   /* keep every layer's activations for ffhip_batch_get_activation        */
/* (A read that left the default kernels' operand range and was evaluated again on the f32 kernels -- ffhip_batch_f32_reruns() -- returns
 * the f32 run's scores, path and calls; its KEPT ACTIVATIONS are not refreshed: they stay those of the first, discarded evaluation.) */
/* Gate activations of the split layer kernels (logistic, tanh; layers.c:979-1026 through util.h:319-337, sse_mathfun.h:225-301).  Since round 6 the DEFAULT is
 * the hardware form of FFHIP_RUN_FAST_GATES2: decided by measurement (profiles/r06_gates_*.txt: 8192 reads at the headline shape, 2048 at the two H = 256 shapes --
 * worst |dtrans| against the oracle 2.1e-5 with either form, reads called apart from the oracle 5 against the exact form's 6, and two evaluations of the reference's
 * own algorithm in two summation orders part on 8) and worth +4.4 % (112.6 against 107.8 Msamples/s on one box).  FFHIP_RUN_EXACT_GATES, or FFHIP_FAST_GATES=0 in
 * the environment, brings back the operation-for-operation replay of the reference's exp_ps and division. */
#define FFHIP_RUN_FAST_GATES   128u   /* gate activations through v_exp_f32 / v_rcp_f32 as they are (1 ulp each, the exponent rounded once) */
#define FFHIP_RUN_FAST_GATES2  256u   /* the same with the exponent of v_exp_f32 carried in two words and a Newton step behind v_rcp_f32: exp and the
                                       * reciprocal to ~1 ulp at every argument (the reference's cephes replay is no closer to the true functions); the default */
#define FFHIP_RUN_EXACT_GATES  512u   /* the reference's exp_ps polynomial and its division replayed bit for bit (the default of rounds 1-5) */
/* run records of the run-length model (FFHIP_NET_LSTM5_RLE, nbase 4; ffhip_batch_rle_runs below): made on the device behind the Viterbi and brought down in
 * ffhip_batch_finish's one copy of the result block */
#define FFHIP_RUN_RLE_RUNS    1024u   /* every run's base and run-length estimate, and per read the run count, expanded length and failure flag */
#define FFHIP_RUN_RLE_RECORDS 2048u   /* ... and every run's shape, scale and dwell as well (the whole .run record; 12 more bytes a block) */
/* 5mC probabilities of a flip-flop model with a modified base (nbase 5: A C G T Z, e.g. r941_5mC; ffhip_batch_mod_probs below): one byte a called base, made
 * on the device from the posterior behind the Viterbi and brought down in ffhip_batch_finish's one copy of the result block.  Path, scores, strings and trace are
 * those of the same run without the flag; under FFHIP_RUN_VITERBI_ONLY the forward-backward pass runs as well (for the probabilities only), and
 * ffhip_batch_get_posterior returns its posterior.  Another model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_MOD_PROBS   4096u
/* Move table of a flip-flop model (ffhip_batch_moves below): one byte a block, 1 where the block's transition emits a base of ffhip_batch_basecall, made on the
 * device from the Viterbi path (k_moves) and brought down in ffhip_batch_finish's one copy of the result block.  Everything else the run returns is that of the same
 * run without the flag.  The run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_MOVES       8192u
/* Barcode classification of a flip-flop model's calls (ffhip_batch_barcode below, "barcodes"): one 16-byte record a read, made on the device from the base strings
 * (k_barcodes) against the kit attached with ffhip_batch_set_barcodes.  The records are NOT part of the result block: they live in a small buffer of their own
 * (reads x 16 bytes) and come down in ONE extra copy, enqueued where the result block's copy is.  Everything else the run returns is that of the same run without the
 * flag.  No kit attached, the run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_BARCODES   16384u
/* Signal-to-sequence mapping of a flip-flop model's reads (ffhip_batch_remap below, "remap"): the best path of each read's transition scores through a sequence the
 * caller gave with ffhip_batch_set_remap, made on the device (k_remap) in the launch sequence of the decode.  Records and moves are NOT part of the result block:
 * they live in ONE buffer of their own (reads x 16 bytes, then a byte a block) and come down in ONE extra copy, enqueued where the result block's copy is.
 * Everything else the run returns is that of the same run without the flag.  No sequences set, the run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_REMAP      32768u
/* The call scored against a sequence the caller knows (ffhip_batch_truth below, "truth"): a banded global edit-distance alignment of each read's called letters to
 * the truth given with ffhip_batch_set_truth, with traceback, made on the device (k_truth) behind the call's assembly.  Records and ops are NOT part of the result
 * block: they live in ONE buffer of their own (reads x 48 bytes, then the ops) and come down in ONE extra copy, enqueued where the result block's copy is.
 * Everything else the run returns is that of the same run without the flag.  No truths set, the run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_TRUTH      65536u
/* With FFHIP_RUN_REMAP: the signal of every base of every mapped read (ffhip_batch_events below, "events"): first sample, sample count, mean and standard deviation,
 * made on the device (k_events) behind k_remap from the path it has just written and the signal the batch was given.  The events are NOT part of the result
 * block: they live in ONE buffer of their own (16 bytes a base, one read behind the other) and come down in ONE extra copy, enqueued where the remap buffer's copy
 * is.  Everything else the run returns is that of the same run without the flag.  Without FFHIP_RUN_REMAP: FFHIP_EINVAL; the run-length model and
 * FFHIP_RUN_NO_DECODE are refused as for remap. */
#define FFHIP_RUN_EVENTS     131072u
/* With FFHIP_RUN_REMAP, a model of the alphabet ACGTZ: at every C or Z of every mapped read's sequence, the log scores of the signal around it with C and with Z
 * at that position (ffhip_batch_site_mods below, "site mods"), made on the device (k_site_mods) behind k_remap from the transition scores, the coded sequences and
 * the path it has just written.  The records are NOT part of the result block: they live in ONE buffer of their own (16 bytes a site, one read behind the other)
 * and come down in ONE extra copy, enqueued where the remap buffer's copy is.  Everything else the run returns is that of the same run without the flag.  Without
 * FFHIP_RUN_REMAP, or on a model whose nbase is not 5: FFHIP_EINVAL; the run-length model and FFHIP_RUN_NO_DECODE are refused as for remap. */
#define FFHIP_RUN_REMAP_MODS 262144u
/* With FFHIP_RUN_REMAP, any flip-flop model (nbase 4 or 5): for every variant of ffhip_batch_set_remap_variants -- a short edit of a mapped read's sequence: a
 * substitution, an insertion or a deletion -- the log scores of the signal around it under the sequence as given (ref) and under the edited one (alt)
 * (ffhip_batch_variant_calls below, "variants"), made on the device (k_variants) behind k_remap from the transition scores, the coded sequences and the path it has
 * just written.  The records are NOT part of the result block: they live in ONE buffer of their own (16 bytes a variant, one read behind the other) and come down
 * in ONE extra copy, enqueued where the remap buffer's copy is.  Everything else the run returns -- events and site mods included -- is that of the same run
 * without the flag.  Without FFHIP_RUN_REMAP, or with no variants set: FFHIP_EINVAL; the run-length model and FFHIP_RUN_NO_DECODE are refused as for remap. */
#define FFHIP_RUN_REMAP_VARIANTS 524288u
/* Adapters and primers anywhere in a flip-flop model's calls (ffhip_batch_adapters below, "adapters"): one 256-byte record a read -- a header and up to 15 hits with
 * exact start and end -- made on the device from the base strings (k_adapters) against the kit attached with ffhip_batch_set_adapters.  The records are NOT part of
 * the result block: they live in a buffer of their own (reads x 256 bytes) and come down in ONE extra copy, enqueued where the result block's copy is.  Everything
 * else the run returns is that of the same run without the flag.  No kit attached, the run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_ADAPTERS   1048576u
/* The poly(A) tail of a flip-flop model's reads (ffhip_batch_polytail below, "poly tail"): one 32-byte record a read -- where the signal stays flat while the path
 * says the tail's base, and how many bases that is at the read's own speed -- made on the device (k_polytail) behind the decode from the Viterbi path and the signal
 * the batch was given, with the parameters of ffhip_batch_set_polytail.  It needs no FFHIP_RUN_REMAP.  The records are NOT part of the result block: they live in a
 * buffer of their own (reads x 32 bytes) and come down in ONE extra copy, enqueued where the result block's copy is.  Everything else the run returns is that of the
 * same run without the flag.  No parameters set, the run-length model, or FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_POLYTAIL   2097152u
/* Every call of a flip-flop model placed on a small reference (ffhip_batch_map below, "map"): one 64-byte record a read -- status, strand and record, the span, and
 * either anchor's own place, distance and runner-up -- made on the device from the base strings (k_map_scan, k_map_finish) against the reference attached with
 * ffhip_batch_set_map.  The records are NOT part of the result block: they live in a buffer of their own (reads x 64 bytes) and come down in ONE extra copy, enqueued
 * where the result block's copy is.  Everything else the run returns is that of the same run without the flag.  No reference attached, the run-length model, or
 * FFHIP_RUN_NO_DECODE with it: FFHIP_EINVAL. */
#define FFHIP_RUN_MAP        4194304u
/* With FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map: every aligned read's counts added, per reference position, into the pileup
 * attached with ffhip_batch_set_pileup ("pileup" below) -- on the device (k_pileup), as the last step of ffhip_batch_finish, from the records the caller reads.
 * Nothing comes down per read and the batch holds nothing new: the counters are the pileup's (ffhip_debug_batch_device_bytes does not change).  Everything the run
 * returns is that of the same run without the flag.  Without FFHIP_RUN_TRUTH, without FFHIP_RUN_MAP, outside the mode, with no pileup attached or with a pileup of
 * another reference than the batch's: FFHIP_EINVAL with a text that says which. */
#define FFHIP_RUN_PILEUP     8388608u
/* With FFHIP_RUN_MAP | FFHIP_RUN_TRUTH | FFHIP_RUN_MOD_PROBS in the mode of ffhip_batch_set_truth_from_map, a 5-base model: every aligned read's 5mC bytes classed and
 * added, per reference C (- strand: G), into the mod pileup attached with ffhip_batch_set_modpileup ("mod pileup" below) -- on the device (k_modpileup), as the last
 * step of ffhip_batch_finish, from the records, letters and bytes the caller reads.  Nothing comes down per read and the batch holds nothing new
 * (ffhip_debug_batch_device_bytes does not change); everything the run returns is that of the same run without the flag.  Without FFHIP_RUN_MAP, FFHIP_RUN_TRUTH or
 * FFHIP_RUN_MOD_PROBS, outside the mode, with no mod pileup attached or with one of another reference than the batch's: FFHIP_EINVAL with a text that says which.
 * FFHIP_RUN_PILEUP is neither required nor excluded. */
#define FFHIP_RUN_MOD_PILEUP (1u << 24)   /* 16777216: the bit behind FFHIP_RUN_PILEUP */
/* With FFHIP_RUN_MAP | FFHIP_RUN_TRUTH in the mode of ffhip_batch_set_truth_from_map: every aligned read's forward letters, deletions and INSERTED letters added, per
 * reference position, into the consensus attached with ffhip_batch_set_consensus ("consensus" below) -- on the device (k_consensus), as the last step of
 * ffhip_batch_finish, from the records and letters the caller reads.  Nothing comes down per read and the batch holds nothing new (ffhip_debug_batch_device_bytes
 * does not change); everything the run returns is that of the same run without the flag.  Without FFHIP_RUN_TRUTH, without FFHIP_RUN_MAP, outside the mode, with no
 * consensus attached or with one of another reference than the batch's: FFHIP_EINVAL with a text that says which.  FFHIP_RUN_PILEUP and FFHIP_RUN_MOD_PILEUP are
 * neither required nor excluded. */
#define FFHIP_RUN_CONSENSUS  (1u << 25)   /* 33554432: the bit behind FFHIP_RUN_MOD_PILEUP */
/* With FFHIP_RUN_TRUTH, in either truth mode (ffhip_batch_set_truth, or ffhip_batch_set_truth_from_map and then FFHIP_RUN_MAP as well): every aligned read's ops classed
 * -- which truth base was called as which, the quality of every called base, the truth 5-mer under every op, every homopolymer run's called length -- into the error
 * profile attached with ffhip_batch_set_errprofile ("error profile" below) -- on the device (k_errprofile), as the last step of ffhip_batch_finish, from the records,
 * letters and qualities the caller reads.  Nothing comes down per read and the batch holds nothing new (ffhip_debug_batch_device_bytes does not change); everything the
 * run returns is that of the same run without the flag.  Without FFHIP_RUN_TRUTH, in the mode of truth from map without FFHIP_RUN_MAP, with no error profile attached
 * or with one of another engine: FFHIP_EINVAL with a text that says which.  The run-length model and FFHIP_RUN_NO_DECODE are refused as for FFHIP_RUN_TRUTH.
 * FFHIP_RUN_PILEUP, FFHIP_RUN_MOD_PILEUP and FFHIP_RUN_CONSENSUS are neither required nor excluded. */
#define FFHIP_RUN_ERRPROFILE (UINT32_C(1) << 26)   /* 67108864: the bit behind FFHIP_RUN_CONSENSUS */

const char *ffhip_last_error(void);
const char *ffhip_version(void);

/* ---- engine: one per GPU ------------------------------------------------------------------ */
int ffhip_device_count(void);
ffhip_engine *ffhip_engine_create(int device);
void ffhip_engine_destroy(ffhip_engine *eng);
int ffhip_engine_synchronize(ffhip_engine *eng);
/* name, CU count, clock in kHz of the engine's device */
int ffhip_engine_info(const ffhip_engine *eng, char *name, size_t name_len, int *ncu, int *clock_khz);

/* ---- model: weights re-packed into MFMA fragment order and kept resident in HBM ------------ */
/* replaces the static model instances of networks.c:218-399 */
ffhip_model *ffhip_model_upload(ffhip_engine *eng, const ffhip_model_desc *desc);
void ffhip_model_free(ffhip_model *mdl);
size_t ffhip_model_hidden(const ffhip_model *mdl);
size_t ffhip_model_nparam(const ffhip_model *mdl);       /* nstate * (nbase + 1), rows of `trans` */
size_t ffhip_model_nbase(const ffhip_model *mdl);
size_t ffhip_model_stride(const ffhip_model *mdl);       /* samples a block: the product of the convolution strides (5 for the LSTM models, 2 for r941_5mC) */
size_t ffhip_model_launch_reads(const ffhip_model *mdl);  /* reads per batch that keep every layer launch of this model full on this device (MI355X: 1024 at 256 hidden units, 512 at 384, else 256) */
size_t ffhip_model_nblock(const ffhip_model *mdl, size_t nsample);   /* iceil chain, layers.c:204 */

/* ---- batch: `nread` reads of `nsample` samples each, workspace resident in HBM -------------- */
ffhip_batch *ffhip_batch_create(ffhip_engine *eng, const ffhip_model *mdl, int nread, size_t nsample);
void ffhip_batch_destroy(ffhip_batch *b);
size_t ffhip_batch_nblock(const ffhip_batch *b);

/* replaces features_from_raw (nnfeatures.c:15-28): copies raw[start..end) of every read to HBM.
 * `reads[i].end - reads[i].start` may be anything from the convolution window up to nsample: `nsample` is the
 * batch's CAPACITY.  When the lengths differ the batch is RAGGED: every read is evaluated whole and exactly as
 * if it were alone (its own right-edge convolution windows, recurrent state started at its own end for the
 * backward layers, its own block count in the CRF normaliser and the decoders); a read tile of 16 reads costs
 * what its longest member costs, so callers should sort reads by length.  Equal lengths take the uniform path. */
int ffhip_batch_set_reads(ffhip_batch *b, const raw_table *reads);
/* same from a packed host array signals[nread][ld], all reads nsample long */
int ffhip_batch_set_signals(ffhip_batch *b, const float *signals, size_t ld);
/* same, read r uses the first nsample[r] <= capacity samples of its row; nsample[r] == 0 leaves slot r empty
 * (no work, no results) so that one batch object can serve groups of fewer reads */
int ffhip_batch_set_signals_ragged(ffhip_batch *b, const float *signals, size_t ld, const size_t *nsample);
/* blocks of one read of the batch (ffhip_batch_nblock is the capacity's); sizes of that read's results:
 * path/qpath nblock+1, transitions/posterior nblock x nparam, trace (nblock+1) x nstate */
size_t ffhip_batch_read_nblock(const ffhip_batch *b, int read);

/* replaces calculate_transitions (networks.c:108) + transpost_crf_flipflop (decode.c:377) +
 * decode_crf_flipflop (decode.c:119) + change_positions / base+quality assembly
 * (flappie.c:284-292) + exp_activation_inplace / trace_from_posterior (flappie.c:299-300)
 * for the whole batch.  Asynchronous on the batch's stream; results stay in HBM. */
int ffhip_batch_run(ffhip_batch *b, float temperature, unsigned flags);
/* The same for TWO batches of one model and one shape (reads per batch, capacity), with the recurrent layers of both as ONE launch
 * per layer: at H = 384 a 256-read batch fills half of what the layer kernel's dense form carries (two workgroups per CU, 512
 * reads), so a pair runs its five layers in about the time one batch needs alone.  Each batch is still finished and read on its
 * own (ffhip_batch_finish).  Shapes or flags the paired launch does not take run one batch after the other, as two ffhip_batch_run calls. */
int ffhip_batch_run_pair(ffhip_batch *b0, ffhip_batch *b1, float temperature, unsigned flags);
/* 1 if the last run's layer launches were shared with another batch (ffhip_batch_run_pair took the paired path) */
int ffhip_batch_paired(const ffhip_batch *b);
/* copy the small results (calls, qualities, lengths, scores) to pinned host memory and wait */
int ffhip_batch_finish(ffhip_batch *b);

/* ---- results (valid after ffhip_batch_finish) ------------------------------------------------ */
/* basecall/quality: NUL-terminated, at most nblock chars.  Returned pointers stay owned by the batch. */
const char *ffhip_batch_basecall(const ffhip_batch *b, int read, size_t *length);
const char *ffhip_batch_quality(const ffhip_batch *b, int read);
float ffhip_batch_score(const ffhip_batch *b, int read);             /* decode_crf_flipflop return value */
/* on-demand device-to-host copies; out buffers are caller owned */
int ffhip_batch_get_path(ffhip_batch *b, int read, int *path /*[nblock+1]*/, float *qpath /*[nblock+1]*/);
int ffhip_batch_get_transitions(ffhip_batch *b, int read, float *out /*[nblock][nparam] packed*/);
int ffhip_batch_get_posterior(ffhip_batch *b, int read, float *out /*[nblock][nparam] packed, log*/);
int ffhip_batch_get_trace(ffhip_batch *b, int read, int32_t *out /*[nblock+1][nstate] packed*/);
/* debug taps used by the parity tests: activations after conv stack (layer -1) or after RNN layer l
 * (0..4) as dense [nblock][hidden] */
int ffhip_batch_get_activation(ffhip_batch *b, int layer, int read, float *out);
/* which recurrent implementation the last ffhip_batch_run used: 0 = one launch per step, 1 = persistent recurrence behind a
 * projection GEMM, 2 = fused f32-MFMA layer kernel, 3 = split-operand layer kernel (two fp16 slices per operand; hidden 128/256/384/512), 4 = split-operand projection GEMM +
 * recurrence-only split-operand layer kernel (LSTM, hidden 256/512 under FFHIP_RUN_UNFUSED_RNN) */
int ffhip_batch_rnn_path(const ffhip_batch *b);
/* debug read-outs of the kernels on either side of the recurrent stack (tests/test_front_head_fp64_gpu.py).  None changes a run's path, kernel forms or
 * launch shapes.
 * keep_front(b, on): from the next run on, one device-to-device copy right behind the convolution group keeps the last convolution's output (the split
 *   layout on the default path, fp32 otherwise); the thin convolutions' outputs stay in their buffers anyway.  Off: nothing is copied.
 * front(b, layer, row, out): the output of convolution `layer` in batch row `row` as dense fp32 [Tout_layer][filters], the whole row, padding columns
 *   included; split slices and fp16-slice intermediates are decoded as (h0 + h1) * 2^-e.  Needs a finished run with keep_front on.
 * head_input(b, row, out): the last recurrent layer's output as the CRF head read it, dense fp32 [nblock][hidden] of the whole row.
 * forms(b, out[4]): the kernel form each convolution launch (out[0 .. nconv-1]) and the head launch (out[3]) of the last run took: FFHIP_FORM_*, -1 none */
#define FFHIP_FORM_CONV_SMALL_4_5     1   /* k_conv_small<4, 5>: 1 -> 4 features, 5 taps               */
#define FFHIP_FORM_CONV_SMALL_16_20   2   /* k_conv_small<16, 20>: 4 -> 16 features, 5 taps             */
#define FFHIP_FORM_CONV_SMALL_4       3   /* k_conv_small<4>: generic, at most 4 filters                */
#define FFHIP_FORM_CONV_SMALL_16      4   /* k_conv_small<16>: generic, at most 16 filters              */
#define FFHIP_FORM_CONV_SMALL_32      5   /* k_conv_small<32>: generic, at most 32 filters              */
#define FFHIP_FORM_CONV_MFMA_VEC      6   /* k_conv_mfma<true>: f32 MFMA, input features a multiple of 4 */
#define FFHIP_FORM_CONV_MFMA_SCALAR   7   /* k_conv_mfma<false>                                         */
#define FFHIP_FORM_CONV_SPLIT_WS10    8   /* k_conv_split_ws<10>: split operands, weights stationary    */
#define FFHIP_FORM_CONV_SPLIT_4_4     9   /* k_conv_split<4, 4>                                         */
#define FFHIP_FORM_CONV_SPLIT_2_2    10   /* k_conv_split<2, 2>: the shape that fits beside another batch's layer launches */
#define FFHIP_FORM_HEAD_3            11   /* k_head<3>: f32 MFMA head, at most 48 outputs                */
#define FFHIP_FORM_HEAD_4            12   /* k_head<4>                                                  */
#define FFHIP_FORM_HEAD_SPLIT_3      13   /* k_head_split<3>: head on the last layer's split output     */
#define FFHIP_FORM_HEAD_SPLIT_4      14   /* k_head_split<4>                                            */
int ffhip_debug_batch_keep_front(ffhip_batch *b, int on);
int ffhip_debug_batch_front(ffhip_batch *b, int layer, int row, float *out);
int ffhip_debug_batch_head_input(ffhip_batch *b, int row, float *out);
int ffhip_debug_batch_forms(const ffhip_batch *b, int out[4]);
/* debug tap: `ntile` tiles of 16 reads x `hidden` values (hidden % 128 == 0) through the split activation layout of
 * the recurrent layer kernel and back; two fp16 slices of value * 2^12 hold 22 bits: |out - in| <= 2^-22 for |in| <= 1 (the bf16x3 build: bit for bit) */
int ffhip_debug_split_round_trip(ffhip_engine *eng, const float *in, float *out, size_t ntile, int hidden);
/* debug tap: the gate math of the persistent layer kernels (reciprocal by Newton steps instead of the division expansion,
 * floor instead of truncate/compare/subtract) against the reference-order arithmetic, on every fp32 mantissa at binary
 * exponent `exponent` (0..125); `steps` = Newton steps before the closing step (the kernels use 1).  Counts mismatching bit
 * patterns: 0 means bit-identical */
int ffhip_debug_lean_math_check(ffhip_engine *eng, int exponent, int steps, unsigned long long *mismatches);
/* debug tap: y[i] = f(x[i]) for the gate function `form` of the layer kernels, the same inline code they run:
 * 0 logistic_ref, 1 tanh_ref (the reference's exp_ps and division), 2 logistic_ref4_lean (four inputs a vector), 3 logistic_ref2_lean,
 * 4 logistic_ref_lean, 5 tanh_ref_lean, 6 / 7 apply_act4 swish / tanh, 8 / 9 logistic_hw / tanh_hw at level 1, 10 / 11 at level 2 */
int ffhip_debug_gate_math(ffhip_engine *eng, int form, const float *x, float *out, size_t n);

/* debug tap: every op_sel / op_sel_hi form of the packed-fp32 VALU instructions checked against the scalar
 * instructions in a loop on a stream of its own, so that it can run beside a batch's kernels; counts[4][16][2][4] mismatches by
 * instruction (add, mul, fma, v_pk_mov_b32: forms 0, 4, 8, 12 only), form (op_sel[0], op_sel[1], op_sel_hi[0], op_sel_hi[1] as a 4-bit number), result half, wave quarter */
int ffhip_debug_pk_probe(ffhip_engine *eng, int iters, int nwg, int ballast, unsigned *counts);

/* ---- flappie matrices with a device image -------------------------------------------------------
 * An ffhip_mat describes one flappie matrix (flappie_matrix.h:18-24: column-major, `nc` columns of `stride` = 4*ceil(nr/4) floats):
 * its HOST image `data` and, through `dev` / `dev_state`, the device image the matrix owns (the two members include/flappie_matrix.h
 * appends to `_Mat`; both may be NULL for a plain host array).  *dev_state: 0 = host only, 1 = host and device equal, 2 = the DEVICE
 * image is the current one (the host image is stale until flappie_matrix_sync()).  The operators below read the device image when
 * there is one (no upload), and leave their result on the device (state 2, no download) when the matrix they are given was produced
 * there -- see INTEGRATION.md section 3 for the rules and FLAPPIE_HOST_MATRICES=1 for the reference's host-only behaviour. */
typedef struct { float *data; size_t nr, nc, stride; void **dev; int *dev_state; } ffhip_mat;
/* buffers of device images come from (and go back to) a pool per device: no hipMalloc / hipFree per matrix */
void ffhip_dev_release(void *dev);
/* A matrix whose struct the caller may release with a plain free() (the reference's flappie.c:281 does that to the transition matrix):
 * `owner` (the struct's address) is remembered with its image; ffhip_dev_forget(owner) returns the image still recorded for that address
 * (NULL if none) and drops the record -- make_flappie_matrix calls it on every new struct, so an address handed out again returns the
 * orphaned buffer.  Any release of an image (ffhip_dev_release, an operator replacing a stale image) drops its record as well.  Thread-safe. */
void ffhip_dev_remember(const void *owner, void *dev);
void *ffhip_dev_forget(const void *owner);
/* the pool's books, for tests: {buffers it allocated and has not freed, of those in its free lists, remembered owners, buffers that sit
 * TWICE in a free list (must be 0: such a buffer would be handed to two matrices)} */
void ffhip_debug_pool_state(unsigned long long out[4]);
/* device image -> host image (the whole [nc][stride] image); synchronous */
int ffhip_dev_download(const void *dev, float *host, size_t nfloat);
/* host image -> a new device image (pool buffer); NULL on failure */
void *ffhip_dev_upload(const float *host, size_t nfloat);
/* 0: never keep device images (every operator uploads its inputs and downloads its result: the reference's semantics, FLAPPIE_HOST_MATRICES=1);
 * 1 (default): as described above */
void ffhip_set_matrix_policy(int device_images);
int ffhip_matrix_policy(void);
/* calls and bytes of host<->device copies this library has made since the last reset: {h2d calls, h2d bytes, d2h calls, d2h bytes,
 * largest single d2h in bytes} -- what tests/test_host_layer.py counts for the relinked flappie.c */
void ffhip_copy_counts(unsigned long long out[5], int reset);
/* the transition matrix of read `read` of a finished batch as a device image owned by `out` (device-to-device; out.dev / out.dev_state set) */
int ffhip_batch_transitions_to(ffhip_batch *b, int read, ffhip_mat out);
/* transpost_crf_flipflop / decode_crf_flipflop / trace_from_posterior on matrices with device images (decode.c:377-497, :119-204, :499-543) */
int ffhip_op_transpost(ffhip_engine *eng, ffhip_mat trans, int return_log, ffhip_mat post);
int ffhip_op_viterbi(ffhip_engine *eng, ffhip_mat scores, int combine_stays, int *path, float *qpath, float *score);
int ffhip_op_trace(ffhip_engine *eng, ffhip_mat post, int32_t *out);

/* ---- single-matrix decode entry points -------------------------------------------------------
 * Used by the reference-compatible wrappers in include/decode.h.  `trans` / `scores` / `post` are
 * host arrays in the reference's flappie_matrix image: `nblock` columns of `stride` floats, the
 * first `nparam` = nstate*(nbase+1) of each column meaningful. */
/* transpost_crf_flipflop (decode.c:377-497): log posterior (return_log != 0) or probabilities */
int ffhip_transpost(ffhip_engine *eng, const float *trans, size_t nblock, size_t nparam, size_t stride,
                    int return_log, float *post_out);
/* decode_crf_flipflop (decode.c:119-204): path[nblock+1], qpath[nblock+1] (qpath[0] = NAN) */
int ffhip_viterbi(ffhip_engine *eng, const float *scores, size_t nblock, size_t nparam, size_t stride,
                  int combine_stays, int *path, float *qpath, float *score);
/* trace_from_posterior (decode.c:499-543): `post` holds PROBABILITIES; out[nblock+1][nstate] packed */
int ffhip_trace(ffhip_engine *eng, const float *post, size_t nblock, size_t nparam, size_t stride, int32_t *out);

/* ---- layer operators on single matrices ---------------------------------------------------------
 * The reference's per-layer interface (layers.h:15-100, flappie_matrix.h:67-73) on the GPU, used by the
 * wrappers in include/layers.h, on ffhip_mat views (above).  Outputs must be allocated by the caller with the shape the
 * reference function would return; every call is synchronous.  Batch-of-one use of the same kernels the
 * batched pipeline runs. */
/* the flip-flop decoders of decode.h that flappie.c does not use (one wave per call, reference order):
 * argmax_decoder (decode.c:17-36): seq[nc] = row of the column maximum (-1 for the last row), *score = their sum in block order */
int ffhip_op_argmax_decoder(ffhip_engine *eng, ffhip_mat logpost, int *seq, float *score);
/* constrained_crf_flipflop (decode.c:209-270): post [nstate x nblock] per-state scores, path[nblock+1] */
int ffhip_op_constrained_flipflop(ffhip_engine *eng, ffhip_mat post, int *path, float *score);
/* posterior_crf_flipflop (decode.c:275-372) in log space: out [nstate x nblock+1] per-state forward + backward */
int ffhip_op_posterior_flipflop(ffhip_engine *eng, ffhip_mat trans, ffhip_mat out);

enum ffhip_activation {
    FFHIP_ACT_NONE = 0,
    FFHIP_ACT_SWISH = 1,        /* swish_activation_inplace, layers.c:24-33    */
    FFHIP_ACT_TANH = 2,         /* tanh_activation_inplace, layers.c:40-49     */
    FFHIP_ACT_EXP = 3,          /* exp_activation_inplace, layers.c:56-66      */
    FFHIP_ACT_LOG = 4,          /* log_activation_inplace, layers.c:73-81      */
    FFHIP_ACT_ELU = 5,          /* elu_activation_inplace, layers.c:88-96      */
    FFHIP_ACT_ROBUSTLOG = 6,    /* robustlog_activation_inplace, layers.c:109-124: log(p0 + p1*x) */
    FFHIP_ACT_SHIFT_SCALE = 7   /* shift_scale_matrix_inplace, flappie_matrix.c:625-633: (x - p0)/p1 */
};
/* element-wise over the whole image, pad lanes included (as the reference's SSE loops do) */
int ffhip_op_activation(ffhip_engine *eng, ffhip_mat C, int act, float p0, float p1);
/* residual_inplace (layers.c:338-353): Y += X */
int ffhip_op_add_inplace(ffhip_engine *eng, ffhip_mat Y, ffhip_mat X);
/* row_normalise_inplace / log_row_normalise_inplace (flappie_matrix.c:425-467) */
int ffhip_op_row_normalise(ffhip_engine *eng, ffhip_mat C, int log_space);
/* convolution (layers.c:189-276), including its strided right-edge behaviour; C is [W.nc x ceil(X.nc/stride)] */
int ffhip_op_convolution(ffhip_engine *eng, ffhip_mat X, ffhip_mat W, ffhip_mat b, size_t conv_stride, ffhip_mat C);
/* affine_map / affine_map2 (flappie_matrix.c:361-419): C = Wf^T Xf (+ Wb^T Xb) + b; pass Xb.data == NULL for one input */
int ffhip_op_affine(ffhip_engine *eng, ffhip_mat Xf, ffhip_mat Wf, ffhip_mat Xb, ffhip_mat Wb, ffhip_mat b, ffhip_mat C);
/* lstm_forward/backward (layers.c:877-976), grumod_forward/backward (layers.c:571-660); kind = enum ffhip_net_kind */
int ffhip_op_recurrent(ffhip_engine *eng, int kind, ffhip_mat Xa, ffhip_mat sW, int backward, ffhip_mat out);
/* lstm_step (layers.c:979-1026) / grumod_step (layers.c:664-715); `state` = LSTM cell state, updated in place */
int ffhip_op_recurrent_step(ffhip_engine *eng, int kind, ffhip_mat x, ffhip_mat h_prev, ffhip_mat sW, ffhip_mat state, ffhip_mat h_out);
/* sloika GRU: gru_forward/backward (layers.c:412-510; relu = 0) and gru_relu_forward/backward (layers.c:718-816; relu = 1);
 * X [3H x T] projected input, sW [H x 2H], sW2 [H x H].  One workgroup per call: no registered model uses these layers. */
int ffhip_op_gru(ffhip_engine *eng, int relu, ffhip_mat X, ffhip_mat sW, ffhip_mat sW2, int backward, ffhip_mat out);
/* gru_step (layers.c:513-568) / gru_relu_step (layers.c:819-874) */
int ffhip_op_gru_step(ffhip_engine *eng, int relu, ffhip_mat x, ffhip_mat istate, ffhip_mat sW, ffhip_mat sW2, ffhip_mat ostate);
/* crf_manystay_partition_function (layers.c:1035-1079) */
int ffhip_op_partition_function(ffhip_engine *eng, ffhip_mat S, double *logZ);
/* the same quantity by the batched pipeline's scaled linear-space recursion; requires |S| <= bound everywhere */
int ffhip_op_partition_function_scaled(ffhip_engine *eng, ffhip_mat S, float bound, double *logZ);
/* globalnorm_flipflop (layers.c:1082-1106) */
int ffhip_op_globalnorm_flipflop(ffhip_engine *eng, ffhip_mat X, ffhip_mat W, ffhip_mat b, float temperature, ffhip_mat C);

/* ---- run-length (runnie) head and decoders on single matrices ------------------------------------------
 * globalnorm_runlengthV2 (layers.c:1325-1358), runlengthV2_partition_function (layers.c:1255-1302),
 * transpost_crf_runlength (decode.c:1037-1159), decode_crf_runlength (decode.c:927-1013). */
int ffhip_op_globalnorm_runlength(ffhip_engine *eng, ffhip_mat X, ffhip_mat W, ffhip_mat b, float temperature, ffhip_mat C);
int ffhip_op_runlength_partition_function(ffhip_engine *eng, ffhip_mat S, double *logZ);
/* first-generation head: globalnorm_runlength (layers.c:1197-1228), runlength_partition_function (layers.c:1127-1174) */
int ffhip_op_globalnorm_runlength_v1(ffhip_engine *eng, ffhip_mat X, ffhip_mat W, ffhip_mat b, float temperature, ffhip_mat C);
int ffhip_op_runlength_partition_function_v1(ffhip_engine *eng, ffhip_mat S, double *logZ);
int ffhip_runlength_transpost(ffhip_engine *eng, ffhip_mat param, ffhip_mat post);
/* Run records (runnie.c:282-313) and run-length estimates (decode_runnie.py's run_estimate_modes), made on the device by k_rle_runs:
 *   a run starts at every block p with path[p] < nbase: base = path[p]; shape, scale = rows base, nbase + base of block p of the posterior (under --viterbi
 *   the transitions, the matrix runnie's .run writer reads); dwell = the next run's start - p, the last run's nblock - p; blocks before the first run count
 *   for nothing.  est = max(1, floor(s6 * factor[base])) in double, s6 = rint(scale * 1e6) / 1e6: the value Python reads back from the %f text of the scale.
 *   A read with a non-finite scale or an estimate >= 2^31 is `failed` (its estimates are not meaningful).  factor defaults to A, C, G, T = 1.02, 1.04, 1.04, 1.02.
 * ffhip_batch_set_run_scale: the four factors of a batch's later runs (a batch never set uses the defaults).
 * ffhip_batch_rle_runs: after ffhip_batch_finish of a run with FFHIP_RUN_RLE_RUNS (or _RECORDS); the arrays hold nrun entries, bases as 0 .. 3, and stay owned
 *   by the batch; shape / scale / dwell are NULL unless the run had FFHIP_RUN_RLE_RECORDS.  A flip-flop model's batch, or a run without the flag: FFHIP_EINVAL.
 * ffhip_op_rle_runs: the same on one [nparam x nblock] matrix (nbase 4) and its path (nblock entries, each 0 .. 2 nbase - 1); factor NULL: the defaults; the
 *   outputs are caller-owned arrays of nblock entries (shape, scale, dwell may be NULL). */
typedef struct {
    size_t nrun;                      /* runs of the read */
    unsigned long long length;        /* sum of est: the length of the expanded sequence */
    int failed;                       /* 1: a scale was not finite or an estimate reached 2^31 */
    const uint8_t *base;
    const int32_t *est;
    const float *shape, *scale;
    const int32_t *dwell;
} ffhip_rle_runs;
int ffhip_batch_set_run_scale(ffhip_batch *b, const double factor[4]);
int ffhip_batch_rle_runs(const ffhip_batch *b, int read, ffhip_rle_runs *out);
int ffhip_op_rle_runs(ffhip_engine *eng, ffhip_mat param, const int *path, const double *factor, size_t *nrun, uint8_t *base, int32_t *est,
                      float *shape, float *scale, int32_t *dwell, int *failed, unsigned long long *length);
/* 5mC probabilities (SAMv1 1.7 ML values), made on the device by k_mod_probs.  A called base is a change position pos (1 <= pos < nblock,
 * path[pos] != path[pos - 1]) -- the bases of ffhip_batch_basecall --; one whose state % 5 is 1 (C) or 4 (Z) gets, with x = exp(log posterior of block pos - 1),
 *   occ(j) = sum_{f < 10} x[10 j + f] + x[50 + j] + x[55 + j]      (flip j + flop j: column pos of the trace before its 255-scaling)
 *   p = occ(4) / (occ(1) + occ(4))  (0 if the denominator is 0 or not finite),   ml = min(255, floor(256 p));
 * every other called base gets 0.
 * ffhip_batch_mod_probs: after ffhip_batch_finish of a run with FFHIP_RUN_MOD_PROBS; *ml points at `length` bytes (the basecall's length), aligned with
 *   ffhip_batch_basecall's string and owned by the batch.  A run without the flag: FFHIP_EINVAL.
 * ffhip_op_mod_probs: the same on one [60 x nblock] log posterior (nbase 5) and its path (nblock entries, each 0 .. 9); ml: caller-owned, nblock bytes at
 *   least; *ncalled: the called bases (bytes written). */
int ffhip_batch_mod_probs(const ffhip_batch *b, int read, const uint8_t **ml, size_t *length);
int ffhip_op_mod_probs(ffhip_engine *eng, ffhip_mat logpost, const int *path, uint8_t *ml, size_t *ncalled);
/* Move table: where in the signal each called base sits (the mv tag of guppy --moves_out / dorado --emit-moves).  For a read of nblock blocks with the path
 * path[0 .. nblock]:
 *   move[b] = 1  iff  0 <= b <= nblock - 2 and path[b + 1] != path[b]   (b + 1 is a change position, decode.c:66-79);   move[nblock - 1] = 0 always
 *   (path[nblock] is never emitted).  Block b is the block whose transition enters the new state -- the block ffhip_op_mod_probs reads (pos - 1), column pos of
 *   the trace.  The ones number ffhip_batch_basecall's length, and the k-th one in signal order is the k-th character of the call.
 *   Block b stands for the samples [start + b * stride, start + (b + 1) * stride) of the raw signal, start the first sample the read was called from and
 *   stride = ffhip_model_stride (the product of the convolution strides: 5 for the LSTM models, 2 for r941_5mC), clipped to the read's end; no centring on
 *   the convolution window.
 * ffhip_batch_moves: after ffhip_batch_finish of a run with FFHIP_RUN_MOVES; *moves points at *nblock bytes (0 / 1) owned by the batch.  A run without the
 *   flag: FFHIP_EINVAL.
 * ffhip_op_moves: the kernel on one host path of nblock + 1 entries (nblock >= 1); moves: caller-owned, nblock bytes. */
int ffhip_batch_moves(const ffhip_batch *b, int read, const uint8_t **moves, size_t *nblock);
int ffhip_op_moves(ffhip_engine *eng, const int *path, size_t nblock, uint8_t *moves);
/* Barcodes: which sample a read belongs to.
 *   Kit: n patterns, 1 <= n <= 128, each a string over ACGT (upper case) of 1 .. 128 bases; anything else is refused.
 *   Windows of a call s of `len` bases (Z read as C) at window size W, 1 <= W <= 256: front = s[0 : min(W, len)], rear = revcomp(s)[0 : min(W, len)] -- both ends are
 *     the same search of the same patterns.
 *   Infix edit distance of a pattern p (L bases) in a window x (m bases), edlib's HW mode: D[0][j] = 0, D[i][0] = i,
 *     D[i][j] = min(D[i-1][j-1] + (p[i] != x[j]), D[i-1][j] + 1, D[i][j-1] + 1); dist = min_j D[L][j] over j = 0 .. m, end = the SMALLEST j that attains it
 *     (an empty window: dist = L, end = 0).
 *   Classification with max_dist, min_sep, both_ends: s_k = min(dist_front_k, dist_rear_k) (both_ends: their max); b = the smallest k of the minimal s_k;
 *     second = min over k != b of s_k (a kit of one pattern: 255); the read is classified to b iff s_b <= max_dist and second - s_b >= min_sep.
 *   The record: best = b or -1; and in every case best_dist = s_b, second_dist, front_dist / front_end / rear_dist / rear_end of pattern b, ends = bit 0 if
 *     front_dist <= max_dist, bit 1 if rear_dist <= max_dist.  An empty slot of a batch: best -1, all four distances 255.
 * ffhip_barcodes_upload: the kit's tables on the engine's device (NULL with a text on a bad kit); the kit must outlive the batches it is attached to.
 * ffhip_batch_set_barcodes: the kit and the parameters of the batch's later runs with FFHIP_RUN_BARCODES; max_dist < 0: floor(Lmin / 4), Lmin the kit's shortest
 *   pattern; min_sep < 0: 3; both at most 255.  kit == NULL detaches.
 * ffhip_batch_barcode: after ffhip_batch_finish of a run with the flag.  A run without it: FFHIP_EINVAL.
 * ffhip_op_barcode_scores: the kernel on one call of `len` characters of ACGTZ (len may be 0): the whole matrices dist[2][n], end[2][n], front first. */
typedef struct ffhip_barcodes ffhip_barcodes;
typedef struct { int16_t best; uint8_t best_dist, second_dist, front_dist, rear_dist, ends, pad; int16_t front_end, rear_end; int32_t reserved; } ffhip_barcode_call; /* 16 bytes */
ffhip_barcodes *ffhip_barcodes_upload(ffhip_engine *eng, int n, const char *const *seq, int window);
void ffhip_barcodes_free(ffhip_barcodes *kit);
int ffhip_batch_set_barcodes(ffhip_batch *b, const ffhip_barcodes *kit, int max_dist, int min_sep, int both_ends);
int ffhip_batch_barcode(const ffhip_batch *b, int read, ffhip_barcode_call *out);
int ffhip_op_barcode_scores(ffhip_engine *eng, const ffhip_barcodes *kit, const char *bases, size_t len, int32_t *dist /*[2][n]*/, int32_t *end /*[2][n]*/);
/* Adapters: every occurrence of a sequencing adapter or primer in a call, in both orientations, with exact start and end -- what trimming and read splitting need.
 *   Kit: n patterns, 1 <= n <= 32, each a string over ACGT (upper case) of 1 .. 64 bases; anything else is refused with a text.
 *   Searches: every pattern k is searched as given (orientation 0) and as its reverse complement (orientation 1), both on the call x of `len` bases in SIGNAL order,
 *     Z read as C.  The search index is q = 2 k + orientation: at most 64 searches.
 *   Score row of search q with (oriented) pattern p of L bases: the infix edit distance ending at column j, edlib's HW mode, exactly as for barcodes above:
 *     D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (p[i] != x[j]), D[i-1][j] + 1, D[i][j-1] + 1); d_q[j] = D[L][j], j = 0 .. len.
 *   Hit: with R = 64 and md_k the pattern's bound, column j is a hit end of search q iff d_q[j] <= md_k, and d_q[j] < d_q[j'] for every j' in [j - R, j) within
 *     [0, len], and d_q[j] <= d_q[j'] for every j' in (j, j + R] within [0, len]: the leftmost minimum within R columns either way, so a homopolymer run gives
 *     one hit, not one a column.  md_k = floor(L_k / 4) when max_dist < 0, else min(max_dist, L_k - 1).
 *   Start of a hit (q, j, d): the largest i with ed(p, x[i:j]) = d.  Equivalently: the reversed pattern against x[j-1], x[j-2], ... with an anchored start
 *     (D[0][c] = c), the first column c with D[L][c] = d; start = j - c, and c <= L + d <= 127.  The hit covers x[start : end], end = j.
 *   Record of a read, 256 bytes: the header { nhit, len, kept, reserved } and up to 15 hits { start, end, pattern, orientation, dist, reserved }, ordered by (end, q).
 *     nhit counts ALL hits of the read; kept = min(nhit, 15), and the first `kept` hits in that order are stored (the other slots are zero).  An empty slot of a
 *     batch: nhit = 0, len = 0.
 *   Locality (what the segmented kernel rests on): d_q[j] <= L, and an optimal match spans at most L + d <= 128 columns, so a search started fresh at column a
 *     (D[i][a] = i) has the exact d_q[j] for every j >= a + 128; and the hit rule looks 64 columns either way.  k_adapters cuts a call into segments of
 *     FFHIP_ADAPTER_SEGMENT columns -- segment g owns the hit ends in (g S, (g + 1) S] -- each worked by one wave from a fresh search 192 columns before it.
 * ffhip_adapters_upload: the kit's tables on the engine's device (NULL with a text on a bad kit); the kit must outlive the batches it is attached to.
 * ffhip_batch_set_adapters: the kit and the bound of the batch's later runs with FFHIP_RUN_ADAPTERS.  kit == NULL detaches.
 * ffhip_batch_adapters: after ffhip_batch_finish of a run with the flag: the read's header, and its hits in the batch's host buffer (valid until the batch's next
 *   run).  A run without the flag: FFHIP_EINVAL.
 * ffhip_op_adapter_scores: the kernel on one call of `len` characters of ACGTZ (len may be 0): the whole score rows d[2 n][len + 1], row q = 2 k + orientation.
 * ffhip_op_adapter_hits: likewise, the call's record: the header and all 15 hit slots. */
#define FFHIP_ADAPTER_SEGMENT 512
#define FFHIP_ADAPTER_MAX_HITS 15
typedef struct ffhip_adapters ffhip_adapters;
typedef struct { int32_t nhit, len, kept, reserved; } ffhip_adapter_header;                                            /* 16 bytes */
typedef struct { int32_t start, end; int16_t pattern; uint8_t orientation, dist; int32_t reserved; } ffhip_adapter_hit; /* 16 bytes */
int ffhip_adapter_segment(void);                /* FFHIP_ADAPTER_SEGMENT of the library as built */
ffhip_adapters *ffhip_adapters_upload(ffhip_engine *eng, int n, const char *const *seq);
void ffhip_adapters_free(ffhip_adapters *kit);
int ffhip_batch_set_adapters(ffhip_batch *b, const ffhip_adapters *kit, int max_dist);
int ffhip_batch_adapters(const ffhip_batch *b, int read, ffhip_adapter_header *header, const ffhip_adapter_hit **hits);
int ffhip_op_adapter_scores(ffhip_engine *eng, const ffhip_adapters *kit, const char *bases, size_t len, uint8_t *d /*[2 n][len + 1]*/);
int ffhip_op_adapter_hits(ffhip_engine *eng, const ffhip_adapters *kit, int max_dist, const char *bases, size_t len, ffhip_adapter_header *header, ffhip_adapter_hit *hits /*[15]*/);
/* Map: where on a small reference (the lambda control, a plasmid, a mitochondrion, a virus, an amplicon panel) a call lies, on either strand: the step from "a genome"
 * to "this read's own stretch of it, in signal order", which truth and remap take.  The call is the pattern here and the reference the text.
 *   Reference: K records, 1 <= K <= 1024, each a string over ACGT (upper case) of 1 or more bases, at most FFHIP_MAP_MAX_TOTAL = 2^20 bases together; anything else
 *     is refused with a text that names the record and the position.
 *   Searches: q = 2 k + o; the text y_q of m_k columns is record k as given (o = 0) or its reverse complement (o = 1).  A search never runs across records.
 *   Anchors of a call x of n bases (SIGNAL order, Z read as C) with window W, 64 <= W <= 4096 (default 4096): na = 1 if n <= W, else 2; the front anchor
 *     p_0 = x[0 : min(n, W)], the rear anchor p_1 = x[n - min(n, W) : n].  With na = 1 the rear anchor is the front one and one search is made.  An anchor has L
 *     bases, 1 <= L <= FFHIP_MAP_MAX_ANCHOR = 4096: at most 64 words of 64 rows.
 *   Score row of anchor a in search q: the infix edit distance exactly as for barcodes and adapters above: D[0][j] = 0, D[i][0] = i, unit costs;
 *     d_{a,q}[j] = D[L][j], j = 0 .. m_k.
 *   Best place of an anchor: the lexicographically smallest (d, q, j) over all searches and columns -- the distance minimal, among equals the smallest q, then
 *     the leftmost end j.  second = the minimum of d over all (q', j) with q' != q of the best place (with K = 1: the other strand).
 *   Start, as for adapters: the largest i with ed(p, y[i:j]) = d.  Equivalently: the reversed anchor against y[j-1], y[j-2], ... with an anchored start
 *     (D[0][c] = c), the first column c with D[L][c] = d; start = j - c, and c <= L + d <= 2 L.  The place covers y_q[start : end], end = j.
 *   Bound: md_a = floor(L_a e / 1000), e the maximal error in per mille, 0 <= e <= 500 (default 250); 64-bit integer arithmetic.
 *   Status: 0 no call (an empty slot of the batch, or n = 0); 1 mapped; 2 unmapped: some anchor's dist > md_a; 3 discordant: two anchors, both within their
 *     bounds, but their q differ, or start_0 >= end_1, or |(end_1 - start_0) - n| > floor(n e / 1000).
 *   Span, for status 1: tstart = start_0, tend = end_{na-1}, in the coordinates of y_q.  The forward-strand coordinates are the host's to make: [tstart, tend) for
 *     o = 0, [m_k - tend, m_k - tstart) for o = 1.
 *   Record (ffhip_map_call, 64 bytes, sixteen int32): status, n, nanchor, q, tstart, tend, then for each of two anchors { q, start, end, dist, second }.  With
 *     nanchor = 1 the rear slot repeats the front one.  Status 0 is all zeros apart from the status (which is 0 too); for status 2 and 3 the record's own q,
 *     tstart and tend are zero and the anchors' slots say why.
 *   Locality (what the segmented kernel rests on): d <= L, and an optimal match spans at most L + d <= 2 L columns, so a search started fresh at column a
 *     (D[i][a] = i) has the exact d at every column j >= a + 2 L.  k_map_scan cuts every search into segments of
 *     FFHIP_MAP_SEGMENT columns -- segment g owns the ends in (g S, (g + 1) S], the first one column 0 too -- each worked from a fresh search 2 L columns before
 *     it, or from the record's start if that is nearer.
 * ffhip_map_ref_upload: the reference as 2-bit codes and its task list on the engine's device (NULL with a text on a bad reference); it must outlive the batches
 *   it is attached to.
 * ffhip_batch_set_map: the reference, window and bound of the batch's later runs with FFHIP_RUN_MAP.  Negative values mean the defaults; ref == NULL detaches.
 * ffhip_batch_map: after ffhip_batch_finish of a run with the flag.  A run without the flag: FFHIP_EINVAL.
 * ffhip_op_map_scores: the scan kernel on ONE anchor of 1 .. 4096 letters of ACGTZ: the whole score rows, those of q = 0 .. 2 K - 1 one after another, m_k + 1
 *   entries each (twice the sum of m_k + 1 in all).
 * ffhip_op_map: likewise, the record of one call of any len >= 0. */
#define FFHIP_MAP_SEGMENT 2048
#define FFHIP_MAP_MAX_TOTAL 1048576
#define FFHIP_MAP_MAX_ANCHOR 4096
typedef struct ffhip_map_ref ffhip_map_ref;
typedef struct { int32_t q, start, end, dist, second; } ffhip_map_anchor;                                               /* 20 bytes */
typedef struct { int32_t status, n, nanchor, q, tstart, tend; ffhip_map_anchor anchor[2]; } ffhip_map_call;             /* 64 bytes */
int ffhip_map_segment(void);                    /* FFHIP_MAP_SEGMENT of the library as built */
ffhip_map_ref *ffhip_map_ref_upload(ffhip_engine *eng, int n, const char *const *seq);
void ffhip_map_ref_free(ffhip_map_ref *ref);
int ffhip_batch_set_map(ffhip_batch *b, const ffhip_map_ref *ref, int window, int max_error);
int ffhip_batch_map(const ffhip_batch *b, int read, ffhip_map_call *out);
int ffhip_op_map_scores(ffhip_engine *eng, const ffhip_map_ref *ref, const char *pattern, size_t len, int32_t *d /* 2 sum (m_k + 1) */);
int ffhip_op_map(ffhip_engine *eng, const ffhip_map_ref *ref, int window, int max_error, const char *bases, size_t len, ffhip_map_call *out);
/* Remap: the signal of a read mapped to a sequence the caller knows.
 *   Read: N >= 1 blocks with transition scores T[b][.], b = 0 .. N - 1, nparam = nstate (nbase + 1) floats a block -- exactly what ffhip_batch_get_transitions
 *     returns for that run.  Sequence: s of L bases as codes 0 .. nbase - 1 (the model's alphabet, ACGT or ACGTZ), in SIGNAL order (--reverse, RNA: the caller's business).
 *   Flip-flop coding: q_0 = s_0; q_i = s_i if s_i != s_{i-1}; otherwise q_i = s_i + nbase if q_{i-1} < nbase, else s_i.
 *   Path: p_0 .. p_N with p_0 = 0, p_N = L - 1, p_{b+1} - p_b in {0, 1}; it needs 1 <= L <= N + 1.  Its score is
 *     sum_b T[b][trans_lookup(q_{p_b}, q_{p_{b+1}}, nbase)] (decode.c:104-114: to < nbase ? to nstate + from : nbase nstate + from); a stay is from = to.
 *   Band: c(b) = floor(b (L - 1) / N) in 64-bit integers, b = 0 .. N; cell (b, i) is allowed iff 0 <= i <= L - 1 and |i - c(b)| <= W, W >= 0 the band half-width.
 *     The centre line is itself a path, so for finite scores every W has a solution; W >= L - 1 excludes nothing.
 *   Recursion, in float32: V_0[0] = 0, V_0[i > 0] = -inf.  For an allowed cell (b + 1, i): stay = V_b[i] + T[b][idx(q_i, q_i)], move = V_b[i-1] + T[b][idx(q_{i-1}, q_i)],
 *     a term being -inf where its source cell is not allowed or i = 0; V_{b+1}[i] = move if move > stay STRICTLY, else stay, and the cell's bit records which won.
 *     Each sum is one rounded add: no fused multiply-add, no re-association, no other arithmetic.  score = V_N[L - 1]; the traceback from (N, L - 1) follows the bits.
 *   Mapped: a read is mapped (status 1) iff score = V_N[L - 1] is FINITE.  A finite V was chosen from a finite source plus a finite entry, cells that are not allowed
 *     hold -inf and V_0 is finite at cell 0 alone: the bits under a finite score lead through allowed cells to (0, 0).  With a NaN or an infinity on the way no
 *     strict compare need have won and the bits need not describe a path, so a score that is NaN, +inf or -inf is status 2, "not mapped: the scores leave no finite
 *     path", whatever the bits say: the kernel tests the score once, ahead of the traceback, and follows no bit.  Such a read's record is that of every status 2
 *     read: { 2, L, 0, 0 }, no rm.
 *   Output per read: the score; rm[b] = p_{b+1} - p_b, b = 0 .. N - 1 (N bytes of 0 / 1 whose sum is L - 1); status 0 no sequence given, 1 mapped,
 *     2 not mapped (L > N + 1, L = 0, or a score that is not finite).
 *   What a caller derives: base i starts at block start[0] = 0, start[i] = 1 + (index of the i-th one); maxdev = max_b |p_b - c(b)| says whether the band was
 *     touched; block b stands for samples [trim_start + b stride, ...) as for ffhip_batch_moves.
 * ffhip_batch_set_remap: the sequences (copied, and coded, at the call) and the band of the batch's later runs with FFHIP_RUN_REMAP; nread = the batch's reads
 *   (ffhip_batch_nreads, so after the reads of a ragged or packed batch are set); codes[r] == NULL: read r has no sequence (status 0); len[r] == 0: status 2.  A code
 *   >= nbase, band < 0, the run-length model, or a read whose window min(2 band + 1, L) is more than 4608 cells (what the widest kernel form holds): FFHIP_EINVAL.
 *   codes == NULL detaches.  Not between a run and its finish.
 * ffhip_batch_remap: after ffhip_batch_finish of a run with the flag; rm points into the batch (nblock bytes, valid until the next run), NULL unless status is 1.
 * ffhip_op_remap: the kernel on ONE matrix of scores (nstate (nbase + 1) rows, a column a block) and one sequence; rm: caller-owned, nblock bytes.  L = 0 or
 *   L > nblock + 1, a code >= nbase, band < 0: FFHIP_EINVAL.  It has no status: scores that leave no finite path are FFHIP_EINVAL too, with a text that names the
 *   score; rm and *score are then left as they were.
 * The traceback workspace (a bit a cell of the window and block, in 64-bit words) is grown by the first run that needs it, sized from the batch's reads and the band,
 * freed with the batch and counted by ffhip_debug_batch_device_bytes; when it cannot be had: FFHIP_ENOMEM with the bytes in the text. */
typedef struct { int status; size_t L; float score; const uint8_t *rm; size_t nblock; } ffhip_remap_call;
int ffhip_batch_set_remap(ffhip_batch *b, int nread, const uint8_t *const *codes, const size_t *len, int band);
int ffhip_batch_remap(const ffhip_batch *b, int read, ffhip_remap_call *out);
int ffhip_op_remap(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, int band, uint8_t *rm /* nblock */, float *score);
/* the kernel form a sequence of L bases takes at this band: 0, 1 one wave (windows up to 64, 256 cells), 2, 3 a workgroup (up to 1024, 4608 cells); -1: none */
int ffhip_debug_remap_form(size_t L, int band);
/* Remap from map: each read's signal mapped to the stretch of the reference its call was mapped to, in ONE run -- the map record is on the device when k_map_finish
 * is done, the reference is resident as 2-bit codes and the transitions are where k_remap reads them, so nothing goes through the host (tests/mapremap_ref.py
 * restates this).  The stretch of a map record is that of "truth from map" below: y_q[tstart : tend] as codes 0 .. 3, m = tend - tstart bases, in the orientation of
 * the search q, which is signal order.  It is coded on the device by the flip-flop coding above, written without the recurrence:
 *     q_i = s_i + nbase ((i - runstart_i) & 1), runstart_i the first position of the run of equal letters that i lies in.
 *   The rule, for a read of N >= 1 blocks, room = N + 1 (a path needs L <= N + 1):
 *     map status 1, 1 <= m <= room, the record inside its reference record:  remap status 1, L = m: the recursion under "remap" on the stretch
 *     map status 1, m > room:                                                 remap status 2, L = m, nothing coded
 *     map status 0, 2 or 3:                                                    remap status 0, L = 0 -- a read without a sequence under ffhip_batch_set_remap
 *     (map status 1 with a record that does not lie in its reference record cannot occur; the kernel guards against it all the same: status 2, L = 0)
 *   Sizing: the host knows N and not m.  A read's share of the coded sequences is room entries, its kernel form that of room positions at the band
 *     (ffhip_debug_remap_from_map_form) and its workspace that form's at N blocks; with FFHIP_RUN_EVENTS it has room for room events, of which the L of its record
 *     are written and returned.  The form is therefore at least as large as the one the real L would take; the recursion is defined to the bit, so the bytes do not
 *     depend on the form.  The rooms of a batch's reads together must fit 32 bits (the list's offsets): otherwise FFHIP_EINVAL with a text.
 *   Everything else -- band, recursion, traceback, record, moves, events -- is that of "remap" and "events" with s the stretch: a read's remap record, moves and
 *     events are the same bytes as those of a second run given the stretch through ffhip_batch_set_remap with the same band.  That equality defines the feature.
 * ffhip_batch_set_remap_from_map: on = 1: the batch's later runs with FFHIP_RUN_MAP | FFHIP_RUN_REMAP take each read's sequence from its map record
 *   (k_map_remap_seq, one launch behind k_map_finish and ahead of k_remap, no copy and no wait); band 0 .. 2303 (any window of 2 band + 1 cells fits the widest kernel
 *   form), otherwise FFHIP_EINVAL.  on = 0 leaves the mode.  It and ffhip_batch_set_remap replace each other: the later call wins.  The run-length model, or a call
 *   between a run and its finish: FFHIP_EINVAL.  A run in this mode with FFHIP_RUN_REMAP but without FFHIP_RUN_MAP, or with no reference attached: FFHIP_EINVAL with a
 *   text that says which.  FFHIP_RUN_REMAP_MODS and FFHIP_RUN_REMAP_VARIANTS in this mode: FFHIP_EINVAL -- their site and variant lists are built on the host from
 *   sequences it does not have here.  ffhip_batch_remap and ffhip_batch_events are unchanged: L comes from the record.
 * ffhip_op_map_remap_code: the coding kernel on ONE span from host arguments, for an entry of `room` positions: *status and *L as the rule patches them, and with
 *   status 1 the end - start entries stay | move << 8 in out (untouched otherwise).  It refuses what ffhip_op_map_stretch refuses, and an nbase other than 4 or 5.
 * ffhip_debug_remap_from_map_form: the form a read of nblock blocks takes in this mode, ffhip_debug_remap_form(nblock + 1, band); no engine, no device. */
int ffhip_batch_set_remap_from_map(ffhip_batch *b, int on, int band);
int ffhip_op_map_remap_code(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, int nbase, int room, uint16_t *out /* end - start */, int *status, size_t *L);
int ffhip_debug_remap_from_map_form(int nblock, int band);
/* Events: the signal under every base of a mapped read -- what resquiggle tables, eventalign and comparisons of two samples' levels start from.
 *   Inputs: the read's prepared signal x[0 .. n - 1], float32 -- exactly what the batch was given with any ffhip_batch_set_* call, i.e. what the first convolution
 *     reads; the model's stride (samples a block); the read's N blocks and its remap path rm[0 .. N - 1] with its L, remap status 1.
 *   Spans: start[0] = 0, start[i] = 1 + (index of the i-th one in rm) as above, start[L] = N.  Base i covers the samples [s_i, e_i),
 *     s_i = min(start[i] stride, n), e_i = min(start[i + 1] stride, n), count_i = e_i - s_i.  count_i may be 0: with L = N + 1 the last base has no block, and the
 *     last block may lie past n where the chain of ceilings that gives N rounds up.
 *   Event of base i: the 16 bytes { int32 first = s_i; int32 count = count_i; float mean; float sd; }.  count = 0: mean = sd = 0.  Otherwise, in fp64 and in two
 *     passes, mean = (sum x_k) / count and sd = sqrt((sum (x_k - mean)^2) / count) over the span -- the population form -- each rounded to float32 once at the end.
 *     The order of the sums is the kernel's, and a function of the span's sample count only: a read's events are the same bytes in a one-read-a-row, ragged, packed,
 *     paired, launch-per-step or f32-rerun batch and from one run to the next.  No floating-point atomics, and no one-pass form with a sum of squares: a span of one
 *     repeated value has mean = that value and sd = 0.0 exactly.  first counts from the prepared signal's first sample (add the read's trim_start for raw samples).
 * ffhip_batch_events: after ffhip_batch_finish of a run with FFHIP_RUN_REMAP | FFHIP_RUN_EVENTS; *ev points into the batch (*L events, base after base, valid until
 *   the next run); *ev = NULL and *L = 0 unless the read's remap status is 1.
 * ffhip_op_events: the kernel on ONE read from host arrays: nsample samples (0 is allowed), nblock bytes of 0 / 1 and L; out: caller-owned, L events.
 *   sum rm != L - 1, a byte > 1, L = 0, stride < 1, nblock = 0 or more than 2^30 of either: FFHIP_EINVAL.
 * The events' buffer and its pinned mirror are sized at the front of every run with the flag from the L of ffhip_batch_set_remap, grown when a run needs more, freed
 * with the batch and counted by ffhip_debug_batch_device_bytes; when one cannot be had: FFHIP_ENOMEM with the bytes in the text. */
typedef struct { int32_t first, count; float mean, sd; } ffhip_event;      /* 16 bytes */
int ffhip_batch_events(const ffhip_batch *b, int read, const ffhip_event **ev, size_t *L);
int ffhip_op_events(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const uint8_t *rm, size_t nblock, size_t L, ffhip_event *out /* L */);
/* Site mods: at this C of my sequence, is this read methylated?  Per-read modified-base scoring against a reference: the mapping is kept, and around every C the
 * signal is scored twice through the model's transition scores, once with C and once with Z there.
 *   Inputs: a read of N >= 1 blocks with transition scores T[b][.] (what ffhip_batch_get_transitions returns); a model of nbase = 5 (codes A 0, C 1, G 2, T 3, Z 4);
 *     the sequence s of L codes of ffhip_batch_set_remap; the read's remap result with status 1, rm[0 .. N - 1], and from it start[0] = 0, start[i] = 1 + (index of
 *     the i-th one), start[L] = N as under "remap"; the context c, 0 <= c <= 31, and the mode, best-path or all-paths.
 *   Sites: every i with s_i in {1, 4}, in increasing i.  The given letter may be C or Z: both hypotheses are scored either way.
 *   Window of site i: lo = max(0, i - c), hi = min(L - 1, i + c), P = hi - lo + 1 (at most 63) positions; time runs from t0 = start[lo] to t1 = start[hi + 1] - 1
 *     if hi < L - 1 (block start[hi + 1] - 1 is the move out of hi: not part of the window), else t1 = N; n = t1 - t0.  The remap path itself passes from (t0, lo) to
 *     (t1, hi), so n >= P - 1 always; n may be 0 (P = 1).
 *   Hypotheses: s^can is s with s_i := 1, s^mod is s with s_i := 4; q^h is the flip-flop coding (the rule under "remap") of the WHOLE hypothesis sequence: the
 *     positions before i code as in s itself, those after i may change between flip and flop until the run of equal letters ends (CCC codes C c C, CZC codes C Z C).
 *   Recursion over all cells j = lo .. hi, no band, for t = t0 .. t1 - 1: X_t0[lo] = 0, X_t0[j > lo] = -inf; stay = X_t[j] + T[t][idx(q_j, q_j)],
 *     move = X_t[j-1] + T[t][idx(q_{j-1}, q_j)] (-inf for j = lo), idx = remap's trans_lookup.
 *     Best-path mode, in float32, each term ONE rounded add: X_{t+1}[j] = move if move > stay (a strict compare, the rule of "variants") else stay -- max(stay,
 *     move) on finite and -inf terms; a NaN stay is kept, a NaN move is not taken.  The score X_t1[hi] is reproducible to the bit.
 *     All-paths mode, in fp64 (T converted exactly), in IEEE arithmetic as written: m = move if move > stay else stay; X_{t+1}[j] = -inf if m == -inf, else
 *     m + log1p(exp(-|stay - move|)): from finite or -inf scores never a NaN.  A NaN entry, or +inf met by +inf, on a term gives NaN, and the reader sees it.  The
 *     score X_t1[hi] is rounded to float32 once.
 *   Output per site: the 16 bytes { int32 pos = i; int32 nblock = n; float can; float mod; }.  The log-likelihood ratio is can - mod and
 *     p(5mC) = 1 / (1 + exp(can - mod)): both are left to the reader.
 *   The order of operations depends on the window alone: a read's records are the same bytes in a one-read-a-row, ragged, packed, paired, launch-per-step or
 *     f32-rerun batch (there from the re-run's own transitions and path, as remap's record is) and from one run to the next, in both modes.
 * ffhip_batch_set_remap_mods: the context (0 .. 31; anything else FFHIP_EINVAL) and the mode of the batch's later runs with the flag; never called: 15 and
 *   best-path.  Not between a run and its finish.
 * ffhip_batch_site_mods: after ffhip_batch_finish of a run with FFHIP_RUN_REMAP | FFHIP_RUN_REMAP_MODS; *sm points into the batch (*nsite records in increasing
 *   pos, valid until the next run; a mapped sequence without C or Z: 0 records); *sm = NULL and *nsite = 0 unless the read's remap status is 1.
 * ffhip_op_site_mods: the kernel on ONE read from host arrays: the scores (60 rows, a column a block), L codes, nblock = trans.nc bytes of 0 / 1; out:
 *   caller-owned, room for every C and Z of codes (at most L records); *nsite: the records written.  nbase != 5, a code >= nbase, sum rm != L - 1, a byte > 1,
 *   L = 0, nblock = 0 or != trans.nc or more than 2^30, a context outside 0 .. 31: FFHIP_EINVAL.
 * The records' buffer and its pinned mirror, the workspace of starts (L + 1 int32 a read) and the lists of reads and sites are sized at the front of every run with
 * the flag from the sequences of ffhip_batch_set_remap, grown when a run needs more, freed with the batch and counted by ffhip_debug_batch_device_bytes; when one
 * cannot be had: FFHIP_ENOMEM with the bytes in the text. */
typedef struct { int32_t pos, nblock; float can, mod; } ffhip_site_mod;      /* 16 bytes */
int ffhip_batch_set_remap_mods(ffhip_batch *b, int context, int all_paths);
int ffhip_batch_site_mods(const ffhip_batch *b, int read, const ffhip_site_mod **sm, size_t *nsite);
int ffhip_op_site_mods(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, const uint8_t *rm, size_t nblock, int context, int all_paths,
                       ffhip_site_mod *out, size_t *nsite);
/* Variants: does this read support the reference allele or the alternative one?  The other half of per-read scoring against a reference: the computation of
 * "site mods" with two generalisations -- the two hypotheses may be any short edit of the sequence, not only C <-> Z, and they may differ in length.
 *   Inputs: a read of N >= 1 blocks with transition scores T[b][.]; nbase 4 or 5; the sequence s of L codes of ffhip_batch_set_remap; the read's remap result
 *     with status 1, its path rm and start[0 .. L], exactly as under "site mods"; a context c, 1 <= c <= 23; the mode, best-path or all-paths.
 *   A variant is { pos p, nref r, nalt k, alt[0 .. k - 1] }: 0 <= r <= 16, 0 <= k <= 16, r + k >= 1; 0 <= p, p + r <= L; every alt code < nbase;
 *     L - r + k >= 1.  The ref hypothesis is s itself; the alt hypothesis is s^alt = s[0:p] + alt + s[p+r:], of L - r + k codes.  r = 0 is a pure insertion in
 *     front of position p (p = L: behind the last base), k = 0 a pure deletion.  ref = alt letter for letter is allowed and gives two equal scores.
 *   Window: lo = max(0, p - c), hi = min(L - 1, p + r + c - 1); P_ref = hi - lo + 1 positions of s, P_alt = P_ref - r + k positions of s^alt; under the limits
 *     above both are between 1 and 62.  Blocks: t0 = start[lo]; t1 = start[hi + 1] - 1 if hi < L - 1 (block start[hi + 1] - 1 is the move out of hi), else N;
 *     n = t1 - t0.  BOTH hypotheses are scored over the same blocks t0 .. t1 - 1, each from its first window position at t0 to its last window position at t1:
 *     the ref hypothesis over positions lo .. hi of s, the alt hypothesis over positions lo .. lo + P_alt - 1 of s^alt.
 *   Coding: q^ref is remap's coding of s.  q^alt is the flip-flop coding (the rule under "remap") of the WHOLE s^alt: equal to q before p; behind the edit it may
 *     differ between flip and flop until a run of equal letters ends, and so may still differ at the window's last position.
 *   Recursion: that of "site mods", over each hypothesis's own P positions j = 0 .. P - 1: X_t0[0] = 0, X_t0[j > 0] = -inf; for t = t0 .. t1 - 1:
 *     stay = X_t[j] + T[t][idx(q_j, q_j)], move = X_t[j-1] + T[t][idx(q_{j-1}, q_j)] (-inf for j = 0), idx = remap's trans_lookup.
 *     Best-path mode, in float32, each term ONE rounded add: X_{t+1}[j] = move if move > stay (a strict compare) else stay; reproducible to the bit.
 *     All-paths mode, in fp64 (T converted exactly), in IEEE arithmetic as written: m = move if move > stay else stay; X_{t+1}[j] = -inf if m == -inf, else
 *     m + log1p(exp(-|stay - move|)): from finite or -inf scores never a NaN.  A NaN entry, or +inf met by +inf, on a term gives NaN, and the reader sees it.  The
 *     score is rounded to float32 once.
 *     The score is X_t1[P - 1].  A hypothesis with n < P - 1 has no path: its score is -inf, which comes out of the recursion and is no special case (the ref
 *     hypothesis always has one: the remap path itself).
 *   Output per variant: the 16 bytes { int32 index; int32 nblock = n; float ref; float alt; }; index is the variant's place in the read's list, and the records
 *     stand in list order.  The log-likelihood ratio ref - alt and any probability are left to the reader.
 *   The order of operations depends on the window and the variant alone: a read's records are the same bytes in a one-read-a-row, ragged, packed, paired,
 *     launch-per-step or f32-rerun batch (there from the re-run's own transitions and path, as remap's record is) and from one run to the next, in both modes.
 * ffhip_batch_set_remap_variants: one list a read (vars[r]: nvar[r] variants; nvar[r] = 0: none, vars[r] may be NULL), the context and the mode of the batch's
 *   later runs with the flag.  Called AFTER ffhip_batch_set_remap, because it validates against those L; the lists are copied.  vars = NULL detaches, and so does
 *   a later ffhip_batch_set_remap.  Not between a run and its finish.  FFHIP_EINVAL, with a text that names the read and the index: any limit above violated, a
 *   variant for a read without a sequence; also a context outside 1 .. 23, nread not the batch's, and a call with no sequences set.
 * ffhip_batch_variant_calls: after ffhip_batch_finish of a run with FFHIP_RUN_REMAP | FFHIP_RUN_REMAP_VARIANTS; *vc points into the batch (*nvar records in list
 *   order, valid until the next run); *vc = NULL and *nvar = 0 unless the read's remap status is 1.
 * ffhip_op_variants: the kernels on ONE read from host arrays: the scores (2 nbase (nbase + 1) rows, a column a block), L codes, nblock = trans.nc bytes of
 *   0 / 1, nvar variants; out: caller-owned, nvar records.  What ffhip_op_site_mods refuses (a code >= nbase, sum rm != L - 1, a byte > 1, L = 0, nblock = 0 or
 *   != trans.nc or more than 2^30), nbase other than 4 or 5, a context outside 1 .. 23 and every invalid variant: FFHIP_EINVAL.
 * The records' buffer and its pinned mirror, the workspace of starts (L + 1 int32 a read with variants) and the list of reads and variants are sized at the front
 * of every run with the flag, grown when a run needs more, freed with the batch and counted by ffhip_debug_batch_device_bytes; when one cannot be had:
 * FFHIP_ENOMEM with the bytes in the text. */
typedef struct { int32_t pos; uint8_t nref, nalt; uint8_t alt[16]; uint8_t pad[2]; } ffhip_variant;      /* 24 bytes */
typedef struct { int32_t index, nblock; float ref, alt; } ffhip_variant_call;                              /* 16 bytes */
int ffhip_batch_set_remap_variants(ffhip_batch *b, int nread, const ffhip_variant *const *vars, const size_t *nvar, int context, int all_paths);
int ffhip_batch_variant_calls(const ffhip_batch *b, int read, const ffhip_variant_call **vc, size_t *nvar);
int ffhip_op_variants(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, const uint8_t *rm, size_t nblock,
                      const ffhip_variant *vars, size_t nvar, int context, int all_paths, ffhip_variant_call *out /* nvar */);
/* Poly tail: how long a read's poly(A) tail is (pt:i of dorado, polya of nanopolish and tailfindr).  Over a homopolymer the signal is flat and the model sits in
 * one state for hundreds of blocks, so the call holds a handful of As; the length is in the signal: how long it stays flat while the path says the tail's base,
 * divided by how fast the rest of the read moves.
 *   Inputs for one read: the prepared signal x[0 .. n), float32 -- exactly what the first convolution reads; the model's stride S; the read's N >= 1 blocks; its
 *     Viterbi path path[0 .. N], states of the flip-flop model, and nbase.
 *   Parameters (ffhip_polytail_params, all int32 but the last): base t, 0 .. 3; from_end 0 (the tail is searched from the signal's start) or 1 (from its end);
 *     window K, 1 .. 64 blocks a window; min_calls, 0 .. K blocks of t a window needs; gap G, 0 .. 16 unflagged windows a tail may bridge; min_windows Wmin >= 1,
 *     the shortest interval kept; search R >= 1, the windows searched from the chosen end; min_bases >= 1, the called bases the rate needs; max_sd >= 0, float32,
 *     the flatness bound.
 *   1. Block base and moves: base_b = path[b + 1] % nbase, 4 (Z) read as 1 (C); mv[b] exactly as "Move table" above has it.
 *   2. Windows: NW = floor(min(N, floor(n / S)) / K); window w covers the samples [w K S, (w + 1) K S) and the blocks [w K, (w + 1) K).  A trailing partial
 *     window belongs to nothing.
 *   3. Window statistics, in fp64, two passes, each sum sequential in sample order, no fused multiply-add: a = sum x_k, mu = a / (K S), q = sum (x_k - mu)^2;
 *     flag_w = (q <= ((double)max_sd * (double)max_sd) * (double)(K S)) and #{b in w : base_b == t} >= min_calls.  No sqrt is taken.
 *   4. Candidates: flagged windows are merged across runs of at most G unflagged windows that lie between two flagged ones; a candidate [ws, we) is a maximal
 *     merged run, and starts and ends on a flagged window.
 *   5. The tail: of the candidates with we - ws >= Wmin that are in reach -- ws < R, or we > NW - R when from_end -- the longest; ties go to the smallest ws, or
 *     the largest we when from_end.  None: status 2.
 *   6. The record, with bs = ws K and be = we K: first = bs S; count = (be - bs) S; flat = the flagged windows in [ws, we);
 *     calls = #{b in [bs, be) : mv[b] == 1 and base_b == t}; level = the mean of mu_w over the interval's flagged windows, in fp64 in the kernel's own order,
 *     rounded to float32 once.
 *   7. Rate, from the far side of the tail (the transcript).  from_end 0: c = sum of mv[b] over b >= be, so = min(N S, n) - be S; from_end 1: c = sum of mv[b]
 *     over b < bs, so = bs S.  c < min_bases or so <= 0: status 3, the record keeps what step 6 gave and rate = bases = 0.  Otherwise status 1 with
 *     rate = (float)((double)so / (double)c) and bases = (float)(((double)count * (double)c) / (double)so): integers in, one rounded product, one rounded
 *     quotient, one rounding to float32.
 *   The record, 32 bytes: { int32 status, first, count, flat, calls; float level, rate, bases }.  An empty slot of a batch is all zero (status 0); status 2 is
 *     { 2, 0, ... }.  Every field except level is a function of the inputs alone: the same read gives the same bytes in a one-read-a-row, ragged, packed, paired,
 *     launch-per-step or f32-rerun batch and from one run to the next.  first counts from the prepared signal's first sample (add the read's trim_start for raw
 *     samples).
 * ffhip_batch_set_polytail: the parameters (copied) of the batch's later runs with FFHIP_RUN_POLYTAIL; NULL detaches.  A parameter out of range, the run-length
 *   model, or a call between a run and its finish: FFHIP_EINVAL with a text, and the batch is as it was.
 * ffhip_batch_polytail: after ffhip_batch_finish of a run with the flag.  A run without it: FFHIP_EINVAL.
 * ffhip_op_polytail: the kernel on ONE read from host arrays: nsample samples (0 is allowed), a path of nblock + 1 states; out: one record.
 * ffhip_op_polytail_windows: likewise, the NW windows' mu, q and flag (0 / 1), each caller-owned with room for NW entries: what holds the order of the sums to
 *   the bit.  Both: nblock = 0, stride < 1, nbase other than 4 or 5, a state >= 2 nbase, a parameter out of range, more than 2^30 of anything: FFHIP_EINVAL.
 * The records' buffer (fixed), the list of reads and the windows' workspace (9 bytes a window: mu and the flag bits) are made at the front of the first run with
 * the flag, the workspace grown when a run needs more, freed with the batch and counted by ffhip_debug_batch_device_bytes; when one cannot be had: FFHIP_ENOMEM
 * with the bytes in the text. */
typedef struct { int32_t base, from_end, window, min_calls, gap, min_windows, search, min_bases; float max_sd; } ffhip_polytail_params;      /* 36 bytes */
typedef struct { int32_t status, first, count, flat, calls; float level, rate, bases; } ffhip_polytail;                                      /* 32 bytes */
int ffhip_batch_set_polytail(ffhip_batch *b, const ffhip_polytail_params *params);
int ffhip_batch_polytail(const ffhip_batch *b, int read, ffhip_polytail *out);
int ffhip_op_polytail(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const int *path /* nblock + 1 */, size_t nblock, int nbase,
                      const ffhip_polytail_params *params, ffhip_polytail *out);
int ffhip_op_polytail_windows(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const int *path /* nblock + 1 */, size_t nblock, int nbase,
                              const ffhip_polytail_params *params, double *mu /* NW */, double *q /* NW */, uint8_t *flag /* NW */);
/* Truth: how close a call is to the sequence it should have been.
 *   Inputs: the call s of n >= 0 bases -- the batch's called letters in signal order, Z read as C (as the barcode search reads it); the truth t of m bases as codes
 *     0 .. nbase - 1, code 4 (Z) folded to 1 (C) for the comparison; the band half-width W >= 0.
 *   Cells: (j, i), j = 0 .. m truth bases and i = 0 .. n call bases consumed.  c(j) = floor(j n / m) in 64-bit integers; a cell is allowed iff |i - c(j)| <= W.
 *   Recursion, in integers over allowed cells only, a cell that is not allowed counting as +inf: D[0][0] = 0,
 *     D[j][i] = min(D[j-1][i-1] + (t_j != s_i), D[j-1][i] + 1, D[j][i-1] + 1); dist = D[m][n].
 *   Status: 0 no truth given; 1 aligned; 2 not aligned: m = 0, or D[m][n] is infinite (the band leaves no path).  n = 0 with m >= 1 is status 1: m deletions.
 *     (An empty slot of a batch -- a read of no blocks -- has no call at all, not a call of no bases: its truth is set aside, its record says status 0, and
 *     ffhip_batch_truth refuses the slot as every other result call does.)
 *   Traceback, defined on D alone so that no evaluation order can change it: from (m, n), at cell (j, i)
 *     1. the diagonal if j, i > 0, (j-1, i-1) is allowed and D[j-1][i-1] + (t_j != s_i) == D[j][i]: op '=' (0) or 'X' (1);
 *     2. else the deletion if j > 0, (j-1, i) is allowed and D[j-1][i] + 1 == D[j][i]: op 'D' (3);
 *     3. else the insertion: op 'I' (2).
 *   Output per read: status, n, m, dist; the four op counts (n_match + n_mismatch + n_ins = n, n_match + n_mismatch + n_del = m); maxdev = max |i - c(j)| over
 *     the path's cells (maxdev == W: widen the band); the ops in path order from (0, 0), one byte each, nops = dist + n_match of them.
 *   The band runs along the truth, so that the host, which knows m but not n, can size everything: the traceback workspace is two bits a cell of row and window
 *     (m rows of the chosen kernel form's cells), the window min(2 W + 1, nblock + 2) cells since n <= nblock + 1.  The kernel forms hold windows of 64, 256, 1280
 *     and 2560 cells, so W runs from 0 to 1279.  Call and truth: at most 2^24 bases each.
 * ffhip_batch_set_truth: the truths (copied at the call) and the band of the batch's later runs with FFHIP_RUN_TRUTH; nread = the batch's reads (ffhip_batch_nreads);
 *   codes[r] == NULL: read r has no truth (status 0); len[r] == 0: status 2.  A code >= nbase, band < 0 or > 1279 (a band the widest form cannot hold), the
 *   run-length model, or a call between a run and its finish: FFHIP_EINVAL, and the batch is as it was.  codes == NULL detaches.
 * ffhip_batch_truth: after ffhip_batch_finish of a run with the flag; ops points into the batch (nops bytes, valid until the next run), NULL unless status is 1.
 * ffhip_op_truth: the kernel on ONE pair; call: n letters of A C G T Z; ops: caller-owned, n + m bytes, of which the first out->nops are written; out->ops is NULL.
 *   A letter outside A C G T Z, a code > 4, a band outside 0 .. 1279: FFHIP_EINVAL.  m = 0 is status 2.
 * The traceback workspace and the buffer of records and ops are grown by the first run that needs them, sized from the truths' lengths, the reads' blocks and the
 * band, freed with the batch and counted by ffhip_debug_batch_device_bytes; when one cannot be had: FFHIP_ENOMEM with the bytes in the text. */
typedef struct {
    int status;
    size_t n, m;
    int dist, n_match, n_mismatch, n_ins, n_del, maxdev;
    size_t nops;
    const uint8_t *ops;
} ffhip_truth_call;
int ffhip_batch_set_truth(ffhip_batch *b, int nread, const uint8_t *const *codes, const size_t *len, int band);
int ffhip_batch_truth(const ffhip_batch *b, int read, ffhip_truth_call *out);
int ffhip_op_truth(ffhip_engine *eng, const char *call, size_t n, const uint8_t *truth, size_t m, int band, ffhip_truth_call *out, uint8_t *ops /* n + m */);
/* the kernel form a window of that many cells takes: 0, 1 one wave (up to 64, 256 cells), 2, 3 a workgroup (up to 1280, 2560 cells); -1: none */
int ffhip_debug_truth_form(size_t window);
/* Truth from map: each call aligned to the stretch of the reference it was mapped to, in ONE run -- the map record is on the device when k_map_finish is done, the
 * reference is resident as 2-bit codes and the call's letters are where k_truth reads them, so nothing goes through the host (tests/maptruth_ref.py restates this).
 *   Stretch of a map record with status 1, search q = 2 k + o and span [tstart, tend): y_q[tstart : tend], y_q record k as given (o = 0) or its reverse complement
 *     (o = 1), as codes 0 .. 3 (A C G T): m = tend - tstart bases.
 *   The truth of a read in this mode: map status 1 and 1 <= m <= bound: the stretch, and the truth status is what the recursion under "truth" gives (1 or 2).  Any
 *     other map status (0, 2, 3): no truth, truth status 0 -- a read without a truth under ffhip_batch_set_truth.  1 <= m with m > bound cannot occur (below); the
 *     kernel guards against it all the same and reports truth status 2.
 *   The bound: a mapped call of n bases has m <= n + floor(n e / 1000), e the batch's max_error.  One anchor: its place spans c <= L + d <= n + md columns.  Two
 *     anchors: the concordance rule itself.  n <= nblock + 1, so bound(N, e) = (N + 1) + floor((N + 1) e / 1000) for a read of N blocks, in 64-bit integers.  The host
 *     knows N and e and not n: a read's share of the truths is bound bases, its traceback workspace that of bound rows of its kernel form (the form follows from
 *     min(2 band + 1, N + 2) cells as under "truth") and its ops bound + N + 1 bytes.
 *   The price: the workspace is sized for bound rows and not for m.  At about 0.4 called bases a block, m is about 0.4 N and bound 1.25 N at the default e: roughly
 *     three to four times what exact sizing takes.  ffhip_debug_batch_device_bytes counts it; when it cannot be had: FFHIP_ENOMEM with the bytes in the text, as under
 *     "truth".  The bounds of a batch's reads together must fit 32 bits (the list's offsets), and one bound 2^24: otherwise FFHIP_EINVAL with a text.
 *   Everything else -- band, recursion, traceback rule, record, ops, the folding of Z -- is that of "truth" with t the stretch: a read's truth record and ops are the
 *     same bytes as those of a second run given the stretch through ffhip_batch_set_truth.  That equality defines the feature.
 * ffhip_batch_set_truth_from_map: on = 1: the batch's later runs with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH take each read's truth from its map record (k_map_stretch, one
 *   launch behind k_map_finish and ahead of k_truth, no copy and no wait); band as for ffhip_batch_set_truth (0 .. 1279, otherwise FFHIP_EINVAL).  on = 0 leaves the
 *   mode.  It and ffhip_batch_set_truth replace each other: the later call wins.  The run-length model, or a call between a run and its finish: FFHIP_EINVAL.  A run in
 *   this mode with FFHIP_RUN_TRUTH but without FFHIP_RUN_MAP, or with no reference attached: FFHIP_EINVAL with a text that says which.  ffhip_batch_truth is
 *   unchanged: m comes from the record.
 * ffhip_op_map_stretch: the gather kernel on ONE span from host arguments: y_q[start : end] as end - start codes.  q outside 0 .. 2 K - 1, start < 0, end > m_k or
 *   start >= end: FFHIP_EINVAL.
 * ffhip_debug_map_truth_bound: bound(nblock, max_error) as the library sizes by it (-1: nblock < 0 or max_error outside 0 .. 500); no engine, no device. */
int ffhip_batch_set_truth_from_map(ffhip_batch *b, int on, int band);
int ffhip_op_map_stretch(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, uint8_t *codes /* end - start */);
long long ffhip_debug_map_truth_bound(int nblock, int max_error);
/* Pileup: per reference position, how many aligned calls cover it and what they say there, added up over all the reads of all the batches it is attached to
 * (tests/pileup_ref.py restates this).  The first product here that is not a per-read record: integer adds commute, so the counters are the same bytes whatever
 * the batch size, packing, pairing or read order.
 *   A pileup belongs to one ffhip_map_ref of K records of M_k bases.  off_k = the sum of the lengths before record k, P = the sum of all (at most 2^20).
 *   Counters: 12 planes of P uint32, [strand o][column c][position]: o = 0 (+) or 1 (-); c = 0 .. 3 the base A C G T, 4 del, 5 ins.  Eight uint64 totals:
 *     reads, skipped, match, mismatch, del, ins, edge_ins, and one reserved word that stays 0.
 *   Which reads count: a read of a finished batch whose map record has status 1, whose truth record has status 1 and for which, in 64-bit integers,
 *     1000 n_match >= min_identity (n_match + n_mismatch + n_ins + n_del); min_identity in per mille, 0 .. 1000, fixed at creation.  A read with both statuses 1
 *     that fails the test adds 1 to `skipped` and nothing else; any other read adds nothing.
 *   What a counted read adds: q = 2 k + o and the span [tstart, tend) of its map record, m = tend - tstart; its call s of n letters in signal order (Z read as C,
 *     codes A 0, C 1, G 2, T 3); the K ops of its truth record.  reads += 1; then the ops from (0, 0), j the truth and i the call bases consumed so far:
 *       '=' (0) or 'X' (1): f = o ? M_k - 1 - (tstart + j) : tstart + j; base = o ? 3 - code(s_i) : code(s_i); count[o][base][off_k + f] += 1; match or mismatch
 *         += 1; j++, i++.
 *       'D' (3): f as above; count[o][4][off_k + f] += 1; del += 1; j++.
 *       'I' (2): 1 <= j <= m - 1: the inserted base lies between two aligned positions and is counted at the one to its LEFT on the forward strand:
 *         p = o ? M_k - 1 - tstart - j : tstart + j - 1; count[o][5][off_k + p] += 1; ins += 1.  j = 0 or j = m: an edge insertion, a clip in spirit:
 *         edge_ins += 1 and no plane changes.  Both: i++.
 *     An op's contribution depends on the op, j and i alone, so the kernel takes an op a thread with j and i from prefix counts.
 *   Counters wrap at 2^32 (the totals at 2^64); there is no guard.  Inserted letters are not kept.
 *   When: as the last step of a successful ffhip_batch_finish of a run with FFHIP_RUN_PILEUP -- behind the f32 re-runs of saturated reads, which patch the records,
 *     and in the innermost finish when the batch went again on the launch-per-step kernels -- so every read counts once, from the records ffhip_batch_map,
 *     ffhip_batch_truth and ffhip_batch_basecall return.  The kernel is enqueued on the batch's stream and nothing waits for it; the batch's next run is ordered
 *     behind it.  A batch's internal side batch never counts.
 * ffhip_pileup_create: zeroed counters on the engine's device; min_identity < 0 means 0, > 1000: NULL with a text.  The reference must outlive the pileup, and the
 *   pileup every batch it is attached to.
 * ffhip_pileup_free / _reset / _download wait for every accumulation enqueued against the pileup by any batch; download then makes one copy for the planes
 *   (counts: [12][P], may be NULL) and one for the totals (may be NULL).  ffhip_pileup_positions: P.
 * ffhip_batch_set_pileup: the pileup of the batch's later runs with FFHIP_RUN_PILEUP; NULL detaches.  A pileup of another engine, the run-length model, or a call
 *   between a run and its finish: FFHIP_EINVAL.
 * ffhip_op_pileup: the kernel on ONE alignment from host arguments, added into p.  q, tstart or tend outside the record (the rule of ffhip_op_map_stretch), a
 *   letter outside A C G T Z, an op above 3, or ops that do not consume exactly tend - tstart truth bases and n call bases: FFHIP_EINVAL, and nothing is added.
 *   The identity test applies: an alignment below min_identity adds 1 to `skipped`. */
typedef struct ffhip_pileup ffhip_pileup;
typedef struct { uint64_t reads, skipped, match, mismatch, del, ins, edge_ins, reserved; } ffhip_pileup_totals;      /* 64 bytes */
#define FFHIP_PILEUP_PLANES 12
ffhip_pileup *ffhip_pileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity);
void ffhip_pileup_free(ffhip_pileup *p);
int ffhip_pileup_reset(ffhip_pileup *p);
size_t ffhip_pileup_positions(const ffhip_pileup *p);
int ffhip_pileup_download(ffhip_pileup *p, uint32_t *counts /* [12][P] */, ffhip_pileup_totals *totals);
int ffhip_batch_set_pileup(ffhip_batch *b, ffhip_pileup *p);
int ffhip_op_pileup(ffhip_engine *eng, ffhip_pileup *p, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops);
/* Mod pileup: per reference C, how many aligned calls say "methylated", "not", or neither there, added up over all the reads of all the batches it is attached to
 * (tests/modpileup_ref.py restates this).  The pileup's twin over the 5mC bytes of ffhip_batch_mod_probs: integer adds only, the same bytes whatever the batch
 * size, packing, pairing or read order.
 *   A mod pileup belongs to one ffhip_map_ref of K records of M_k bases; off_k and P as the pileup's.
 *   Counters: 10 planes of P uint32, [strand o][column c][position]: c = 0 mod, 1 canon, 2 fail, 3 diff, 4 del.  Eight uint64 totals: reads, skipped, sites, mod,
 *     canon, fail, diff, del.  A histogram of 256 uint64: how many counted C / Z calls on a reference C had each byte -- to see the distribution and choose thresholds.
 *   Fixed at creation: min_identity in per mille by the pileup's rule (negative: 0; above 1000: refused), and two byte thresholds 0 <= lo < hi <= 255.
 *   Which reads count: the pileup's rule -- map status 1, truth status 1 and 1000 n_match >= min_identity (n_match + n_mismatch + n_ins + n_del) in 64-bit integers.
 *     A read with both statuses 1 that fails the test adds 1 to `skipped` and nothing else; any other read adds nothing.
 *   What a counted read adds: q = 2 k + o and the span [tstart, tend) of its map record, m = tend - tstart; its call s of n letters; its n bytes ml, aligned with s
 *     (ffhip_batch_mod_probs); the K ops of its truth record.  reads += 1; then the ops from (j, i) = (0, 0):
 *       '=' (0) or 'X' (1): f = o ? M_k - 1 - (tstart + j) : tstart + j.  The op is ON A SITE when the forward letter of record k at f is C (o = 0) or G (o = 1).
 *         On a site: sites += 1; s_i is C or Z: v = ml[i], hist[v] += 1, and the column is mod (v >= hi), canon (v <= lo) or fail (between); any other letter:
 *         diff.  count[o][column][off_k + f] += 1 and the total of the same name += 1.  Then j++, i++.  The class follows the call's LETTER, not the op code.
 *       'D' (3): f as above; on a site: sites += 1, column del.  j++.
 *       'I' (2): i++, and nothing else.
 *     An op's contribution depends on the op, j, i and the reference's letter alone, so the kernel takes an op a thread with j and i from prefix counts.
 *   Counters wrap at 2^32 (the totals and the histogram at 2^64); there is no guard.
 *   When: the last step of a successful ffhip_batch_finish of a run with FFHIP_RUN_MOD_PILEUP, where the pileup's stands: behind the f32 re-runs' patches (they patch
 *     the letters and the bytes too) and in the innermost finish of the time-out fallback.  A side batch never counts.  Its order against k_pileup is free.
 * ffhip_modpileup_create: zeroed counters; a bad min_identity or thresholds: NULL with a text.  The reference must outlive it, and it every batch it is attached to.
 * ffhip_modpileup_free / _reset / _download wait for every accumulation enqueued against it; each output of download may be NULL.  _positions: P.
 * ffhip_batch_set_modpileup: the mod pileup of the batch's later runs with the flag; NULL detaches.  One of another engine, a model whose alphabet is not ACGTZ, or a
 *   call between a run and its finish: FFHIP_EINVAL.
 * ffhip_op_modpileup: the kernel on ONE alignment from host arguments, added into p: ffhip_op_pileup's refusals, and ml NULL with n > 0; nothing is added by any.
 *   The ops may disagree with the letters.  The identity test applies. */
typedef struct ffhip_modpileup ffhip_modpileup;
typedef struct { uint64_t reads, skipped, sites, mod, canon, fail, diff, del; } ffhip_modpileup_totals;      /* 64 bytes */
#define FFHIP_MODPILEUP_PLANES 10
ffhip_modpileup *ffhip_modpileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity, int lo, int hi);
void ffhip_modpileup_free(ffhip_modpileup *p);
int ffhip_modpileup_reset(ffhip_modpileup *p);
size_t ffhip_modpileup_positions(const ffhip_modpileup *p);
int ffhip_modpileup_download(ffhip_modpileup *p, uint32_t *counts /* [10][P] */, ffhip_modpileup_totals *totals, uint64_t *hist /* [256] */);
int ffhip_batch_set_modpileup(ffhip_batch *b, ffhip_modpileup *p);
int ffhip_op_modpileup(ffhip_engine *eng, ffhip_modpileup *p, int q, int tstart, int tend, const char *call, const uint8_t *ml, size_t n, const uint8_t *ops, size_t nops);
/* Consensus: per reference position, the letters the aligned calls put there -- bases, deletions and what they INSERT behind it -- added up over all the reads of
 * all the batches it is attached to, and a consensus called from the sums (tests/consensus_ref.py restates this).  The pileup's second twin: integer adds only, the
 * same bytes whatever the batch size, packing, pairing or read order.  Strands are merged: everything is stored as forward-strand letters.
 *   A consensus belongs to one ffhip_map_ref of K records of M_k bases; off_k and P as the pileup's.
 *   Counters: FFHIP_CONSENSUS_PLANES = 37 planes of P uint32, [plane][position].  Planes 0 .. 4: A, C, G, T and del at the position.  Plane 5 + 4 d + base, d = 0 ..
 *     FFHIP_CONSENSUS_MINOR - 1: inserted base `base` at forward offset d in the gap behind the position (the pileup's placement: the gap belongs to the position
 *     to its left on the forward strand).  Eight uint64 totals: reads, skipped, bases, del, ins_bases, long_ins, edge_ins, reserved.
 *   Fixed at creation: min_identity in per mille by the pileup's rule (negative: 0; above 1000: refused).
 *   Which reads count: the pileup's rule -- map status 1, truth status 1 and 1000 n_match >= min_identity (n_match + n_mismatch + n_ins + n_del) in 64-bit integers.
 *     A read with both statuses 1 that fails the test adds 1 to `skipped` and nothing else; any other read adds nothing.
 *   What a counted read adds: q = 2 k + o and the span [tstart, tend) of its map record, m = tend - tstart; its call s of n letters (code: A 0, C and Z 1, G 2, T 3);
 *     the ops of its truth record.  reads += 1; then the ops in signal order from (j, i) = (0, 0):
 *       '=' (0) or 'X' (1): f = o ? M_k - 1 - (tstart + j) : tstart + j, base = o ? 3 - code(s_i) : code(s_i).  plane[base][off_k + f] += 1, bases += 1.  j++, i++.
 *       'D' (3): f as above.  plane[4][off_k + f] += 1, del += 1.  j++.
 *       a maximal run of l consecutive 'I' (2) at j: if j < 1 or j > m - 1 every letter of the run adds 1 to edge_ins and nothing else.  Otherwise the gap is
 *         p = o ? M_k - 1 - tstart - j : tstart + j - 1; the run's r-th letter in signal order is s_(i + r), its forward offset d = o ? l - 1 - r : r, its base as
 *         above.  d < 8: plane[5 + 4 d + base][off_k + p] += 1, ins_bases += 1; else long_ins += 1.  i += l.
 *     A letter's contribution depends on its op, j, i and at most 8 neighbouring ops alone, so the kernel takes an op a thread with j and i from prefix counts.
 *   Counters wrap at 2^32 (the totals at 2^64); there is no guard.
 *   When: the last step of a successful ffhip_batch_finish of a run with FFHIP_RUN_CONSENSUS, where the pileup's stands: behind the f32 re-runs' patches and in the
 *     innermost finish of the time-out fallback.  A side batch never counts.  Its order against k_pileup and k_modpileup is free.
 *   The call (ffhip_consensus_call, k_consensus_call): one 16-byte cell a position.  depth = the sum of planes 0 .. 4 in 64 bits (saturated to 2^32 - 1 in the cell).
 *     depth < min_depth: n = 1, s[0] the reference's letter in LOWER case, what = FFHIP_CONSENSUS_LOW, and no insertion is looked at.  Otherwise the winner is the
 *     largest of the five counts; a tie goes to the reference's letter if it is among the tied, else to the first in the order A, C, G, T, del.  what =
 *     FFHIP_CONSENSUS_SAME (the reference's letter), _SUB (another) or _DEL; a deletion writes no letter, the others the letter in upper case.  Then for d = 0, 1, ...
 *     while d < 8: t_d = the sum of column d's four counts; stop unless 2 t_d > depth; append the letter of the column's largest count (a tie: the first in A, C, G,
 *     T) and set the bit FFHIP_CONSENSUS_INS in `what`.  n = the letters written (0 .. 9); the bytes of s behind them are 0.  The consensus of a record is its cells'
 *     letters concatenated.
 * ffhip_consensus_create: zeroed counters; a bad min_identity: NULL with a text.  The reference must outlive it, and it every batch it is attached to.
 * ffhip_consensus_free / _reset / _download / ffhip_consensus_call wait for every accumulation enqueued against it; each output of download may be NULL.
 *   _positions: P.  ffhip_consensus_call: min_depth < 1 or cells NULL: FFHIP_EINVAL with a text.  It changes no counter and may be made again.
 * ffhip_batch_set_consensus: the consensus of the batch's later runs with the flag; NULL detaches.  One of another engine, the run-length model, or a call between
 *   a run and its finish: FFHIP_EINVAL.
 * ffhip_op_consensus: the kernel on ONE alignment from host arguments, added into c: ffhip_op_pileup's refusals; nothing is added by any.  The identity test applies. */
typedef struct ffhip_consensus ffhip_consensus;
typedef struct { uint64_t reads, skipped, bases, del, ins_bases, long_ins, edge_ins, reserved; } ffhip_consensus_totals;      /* 64 bytes */
typedef struct { uint8_t n, what; char s[10]; uint32_t depth; } ffhip_consensus_cell;      /* 16 bytes */
#define FFHIP_CONSENSUS_PLANES 37
#define FFHIP_CONSENSUS_MINOR 8
enum { FFHIP_CONSENSUS_LOW = 0, FFHIP_CONSENSUS_SAME = 1, FFHIP_CONSENSUS_SUB = 2, FFHIP_CONSENSUS_DEL = 3, FFHIP_CONSENSUS_INS = 4 /* a bit beside the others */ };
ffhip_consensus *ffhip_consensus_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity);
void ffhip_consensus_free(ffhip_consensus *c);
int ffhip_consensus_reset(ffhip_consensus *c);
size_t ffhip_consensus_positions(const ffhip_consensus *c);
int ffhip_consensus_download(ffhip_consensus *c, uint32_t *counts /* [37][P] */, ffhip_consensus_totals *totals);
int ffhip_consensus_call(ffhip_consensus *c, int min_depth, ffhip_consensus_cell *cells /* [P] */);
int ffhip_batch_set_consensus(ffhip_batch *b, ffhip_consensus *c);
int ffhip_op_consensus(ffhip_engine *eng, ffhip_consensus *c, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops);
/* Error profile: by CLASS instead of by position, what the aligned calls of all the reads of all the batches it is attached to got right and wrong
 * (tests/errprofile_ref.py restates this).  The pileup's sibling: integer adds only, the same bytes whatever the batch size, packing, pairing or read order.  It needs
 * no reference coordinates, so it serves a set truth (ffhip_batch_set_truth) as well as truth from map, and belongs to no reference.
 *   Inputs of one counted read: its call s of n letters in signal order (code: A 0, C and Z 1, G 2, T 3); its n quality characters Q, the bytes of ffhip_batch_basecall's
 *     quality string taken as unsigned, qv_i = clamp(Q_i - 33, 0, 93); its truth t of m codes in signal order, code 4 read as 1 -- the codes of ffhip_batch_set_truth or,
 *     in the mode of truth from map, y_q[tstart + j] of its MAP RECORD (read from the reference's letters, not from a kept copy of the stretch); the K ops of its truth
 *     record (0 '=', 1 'X', 2 'I', 3 'D').  (j, i) is the number of truth and call bases consumed before an op.  An 'I' op is INTERIOR iff 1 <= j <= m - 1, else an EDGE
 *     insertion.
 *   Which reads count: the pileup's rule -- truth status 1; in the mode of truth from map also map status 1 and tend - tstart == m; and 1000 n_match >= min_identity
 *     (n_match + n_mismatch + n_ins + n_del) in 64-bit integers.  A read with the statuses that fails the test adds 1 to `skipped` and nothing else; any other read adds
 *     nothing.  A counted read adds 1 to `reads`.
 *   Counters: FFHIP_ERRPROFILE_WORDS = 6526 uint64 in one flat array: the tables (FFHIP_ERRPROFILE_TABLE_WORDS = 6514) and the twelve totals behind them.
 *     sub[4][5] at FFHIP_ERRPROFILE_SUB: '=' / 'X' adds to sub[t_j][code(s_i)], 'D' to sub[t_j][4].
 *     ins[4] at FFHIP_ERRPROFILE_INS: an interior 'I' adds to ins[code(s_i)].
 *     qual[94][3] at FFHIP_ERRPROFILE_QUAL: '=' adds to qual[qv_i][0], 'X' to qual[qv_i][1], an interior 'I' to qual[qv_i][2].
 *     ctx[1024][4] at FFHIP_ERRPROFILE_CTX, with w(c) = sum over d = -2 .. 2 of 4^(2 - d) t_(c + d), defined for 2 <= c <= m - 3: an op that consumes t_j with such a j
 *       adds to ctx[w(j)][0 | 1 | 2] for '=', 'X', 'D'.  An interior 'I' at (j, i) belongs to the centre j - 1: with 3 <= j <= m - 2 it adds to ctx[w(j - 1)][3].
 *       Everything else adds nothing here.
 *     hp[4][16][33] at FFHIP_ERRPROFILE_HP: the maximal runs of equal letters of t, run [a, a + r) of letter b.  Only INTERIOR runs count: a >= 1 and a + r <= m - 1 (a
 *       run that touches an end of the truth has an unknown true length).  r > 16: hp_long += 1 and nothing else.  Otherwise let k_first and k_last be the ops that
 *       consume t_a and t_(a + r - 1), F the maximal block of consecutive 'I' ops ending at k_first - 1 and B the one starting at k_last + 1 (both gaps are interior by
 *       construction).  The run's ops are [k_first - |F|, k_last + |B|].  More than 64 of them: hp_wide += 1 and nothing else.  Otherwise c = the '=' ops in [k_first,
 *       k_last] + the 'I' ops among the run's ops whose letter is b; hp[b][r - 1][min(c, 32)] += 1 and hp_runs += 1.  Neighbouring runs differ in letter, so no inserted
 *       letter counts twice.
 *       One bounded walk decides this, so "r > 16" is read off the run's first 17 letters: a run with a >= 1 whose letters t_a .. t_(a + 16) are equal and whose 17th is
 *       not the truth's last (a + 17 <= m - 1) adds to hp_long, whether or not it goes on to the truth's end; a run that reaches the end within those 17 adds nothing.
 *     Totals (ffhip_errprofile_totals): reads, skipped, match, mismatch, del, ins (interior), edge_ins, ctx_sites (the ops that added to ctx), hp_runs, hp_long, hp_wide
 *       and one reserved word that stays 0.
 *   Counters wrap at 2^64.  Fixed at creation: min_identity in per mille by the pileup's rule (negative: 0; above 1000: refused).
 *   When: the last step of a successful ffhip_batch_finish of a run with FFHIP_RUN_ERRPROFILE, where the pileup's stands: behind the f32 re-runs' patches and in the
 *     innermost finish of the time-out fallback.  A side batch never counts.  Its order against the pileup's kernels is free.
 *   The limits 16, 64 and 32 come from reasoning about small references, whose longest homopolymers are about 10; no real read has been through them.
 * ffhip_errprofile_create: zeroed counters; a bad min_identity: NULL with a text.  It must outlive every batch it is attached to.
 * ffhip_errprofile_free / _reset / _download wait for every accumulation enqueued against it; each output of download may be NULL.  ffhip_errprofile_words: 6526.
 * ffhip_batch_set_errprofile: the error profile of the batch's later runs with the flag; NULL detaches.  One of another engine, the run-length model, or a call between
 *   a run and its finish: FFHIP_EINVAL.
 * ffhip_op_errprofile: the kernel on ONE alignment from host arrays, added into p: the call and its n quality characters, the truth's m codes (0 .. 4) and the ops.
 * ffhip_op_errprofile_mapped: the same with the truth's letters from the span [tstart, tend) of search q of `ref`.  Both refuse what ffhip_op_pileup refuses (a span
 *   or a truth of no base, letters other than A C G T Z, codes out of range, ops that do not consume exactly the call and the truth) and add nothing then.  The
 *   identity test applies.
 * ffhip_debug_errprofile_groups: a test hook -- the most workgroups of the object's later launches (0: the default, the device's compute units). */
typedef struct ffhip_errprofile ffhip_errprofile;
typedef struct { uint64_t reads, skipped, match, mismatch, del, ins, edge_ins, ctx_sites, hp_runs, hp_long, hp_wide, reserved; } ffhip_errprofile_totals;      /* 96 bytes */
#define FFHIP_ERRPROFILE_SUB 0
#define FFHIP_ERRPROFILE_INS 20
#define FFHIP_ERRPROFILE_QUAL 24
#define FFHIP_ERRPROFILE_CTX 306
#define FFHIP_ERRPROFILE_HP 4402
#define FFHIP_ERRPROFILE_TABLE_WORDS 6514
#define FFHIP_ERRPROFILE_WORDS 6526
#define FFHIP_ERRPROFILE_HP_MAX_RUN 16
#define FFHIP_ERRPROFILE_HP_MAX_CALLED 32
#define FFHIP_ERRPROFILE_HP_MAX_OPS 64
ffhip_errprofile *ffhip_errprofile_create(ffhip_engine *eng, int min_identity);
void ffhip_errprofile_free(ffhip_errprofile *p);
int ffhip_errprofile_reset(ffhip_errprofile *p);
size_t ffhip_errprofile_words(void);
int ffhip_errprofile_download(ffhip_errprofile *p, uint64_t *counts /* [6514] */, ffhip_errprofile_totals *totals);
int ffhip_batch_set_errprofile(ffhip_batch *b, ffhip_errprofile *p);
int ffhip_op_errprofile(ffhip_engine *eng, ffhip_errprofile *p, const char *call, const char *qual, size_t n, const uint8_t *truth, size_t m, const uint8_t *ops, size_t nops);
int ffhip_op_errprofile_mapped(ffhip_engine *eng, ffhip_errprofile *p, const ffhip_map_ref *ref, int q, int tstart, int tend, const char *call, const char *qual, size_t n,
                               const uint8_t *ops, size_t nops);
int ffhip_debug_errprofile_groups(ffhip_errprofile *p, int groups);
/* a test hook: between a run in the mode of truth from map and its finish, zero the stretches gathered for k_truth, behind k_truth on the batch's stream -- what a re-run
 * on the f32 path whose map record moved leaves stale.  Nothing the finish launches may read them; every record the run returns is unchanged */
int ffhip_debug_batch_clear_stretches(ffhip_batch *b);
int ffhip_runlength_viterbi(ffhip_engine *eng, ffhip_mat param, int *path /* nblock */, float *score);
/* decoders of the first-generation head on [4 nbase x nblock] matrices: decode_runlength (decode.c:694-767), posterior_runlength
 * (decode.c:793-892; post is [4 nbase x nblock + 1]), runlengths_mean (decode.c:576-603) */
int ffhip_runlength_v1_viterbi(ffhip_engine *eng, ffhip_mat param, int *path /* nblock: base entered, -1 = stay */, float *score);
int ffhip_runlength_v1_posterior(ffhip_engine *eng, ffhip_mat param, ffhip_mat post);
int ffhip_runlength_v1_mean(ffhip_engine *eng, ffhip_mat param, const int *path, int *runlength /* nblock */, size_t *seqlen);

/* ---- signal preparation on the GPU ------------------------------------------------------------------
 * trim_and_segment_raw (flappie_common.c:13-81) followed by medmad_normalise_array (util.c:198-212) or the
 * --delta transform (flappie.c:259-262) for a set of raw reads of any lengths, one workgroup per read; every
 * order statistic is an exact selection, so ranges and signals equal the reference's qsort-based ones.
 * The prepared signals stay in HBM; ffhip_batch_set_prepared feeds equal-length ones to a batch.
 * varseg_chunk == 0 (all four entries below): no trimming at all -- every read whole, trim_start / trim_end ignored --, then the mode's transform. */
typedef struct ffhip_prep ffhip_prep;
#define FFHIP_PREP_MEDMAD 0   /* medmad_normalise_array                                  */
#define FFHIP_PREP_DELTA  1   /* difference_array + shift_scale_array(0, delta)          */
#define FFHIP_PREP_NONE   2   /* trim only, samples copied                               */
#define FFHIP_PREP_DIFFERENCE  3   /* difference_array (util.c:416-427), ffhip_array_transform only  */
#define FFHIP_PREP_SHIFT_SCALE 4   /* shift_scale_array (util.c:214-223), ffhip_array_transform only */
ffhip_prep *ffhip_prep_create(ffhip_engine *eng, const raw_table *reads, int nread, size_t trim_start, size_t trim_end,
                              size_t varseg_chunk, float varseg_thresh, int mode, float delta);
/* the same in two halves: begin enqueues (uploads, kernel, the ranges' copies) and returns, finish waits -- a pipeline begins chunk k + 1 before it submits chunk k's
 * batches, and the preparation runs beside their convolutions.  One preparation may be pending at a time; ranges, statistics and signals are valid after finish. */
ffhip_prep *ffhip_prep_begin(ffhip_engine *eng, const raw_table *reads, int nread, size_t trim_start, size_t trim_end,
                             size_t varseg_chunk, float varseg_thresh, int mode, float delta);
/* The same two entries for reads that are still what the file holds: 16-bit DAC values and the read's calibration (a multi-read fast5 file's reads,
 * fast5_interface.h's fast5_dac_read).  Half the bytes are staged and uploaded; a kernel in front of the preparation writes the picoampere floats
 * (dac + offset) * raw_unit -- an add and a multiply, each rounded, as read_raw's loop does them -- and everything behind it is the float entries' bit for bit. */
typedef struct { const int16_t *dac; size_t n; float offset, raw_unit; } ffhip_dac_read;
ffhip_prep *ffhip_prep_create_dac(ffhip_engine *eng, const ffhip_dac_read *reads, int nread, size_t trim_start, size_t trim_end,
                                  size_t varseg_chunk, float varseg_thresh, int mode, float delta);
ffhip_prep *ffhip_prep_begin_dac(ffhip_engine *eng, const ffhip_dac_read *reads, int nread, size_t trim_start, size_t trim_end,
                                 size_t varseg_chunk, float varseg_thresh, int mode, float delta);
/* (a second preparation of either kind while one is begun and not finished fails with FFHIP_EINVAL: the engine's staging buffers are the pending one's) */
int ffhip_prep_finish(ffhip_prep *p);
void ffhip_prep_destroy(ffhip_prep *p);      /* waits for the copies ffhip_batch_set_prepared enqueued from it, not for the batches */
/* start >= end: the read was rejected (trim_and_segment_raw would have returned a NULL table) */
int ffhip_prep_range(const ffhip_prep *p, int read, size_t *start, size_t *end);
int ffhip_prep_stats(const ffhip_prep *p, int read, float *median, float *mad);      /* MEDMAD mode */
int ffhip_prep_get_signal(const ffhip_prep *p, int read, float *out /* end-start floats */);
/* device-to-device and asynchronous on the batch's stream (one gather launch; the call does not wait for the GPU) */
int ffhip_batch_set_prepared(ffhip_batch *b, const ffhip_prep *prep, const int *reads /* batch nread indices into prep (-1 = empty slot); lengths <= capacity */);

/* ---- packed batches: reads of ANY lengths, several to a row ---------------------------------------------------------------
 * The reference takes reads of any length one at a time (flappie.c:245-262, 334-385).  A batch above costs what its longest read costs -- a launch per
 * layer runs as many steps as that read has blocks whatever the others' lengths -- so a nanopore-like length mix (a long tail of 100 000-sample reads among
 * 5000-sample ones) fills a fraction of it.  A PACKED batch is `nslot` rows of `nsample` samples; a row holds one or more reads one behind the other, each
 * starting at a block offset of the caller's choice with at least ffhip_model_pack_gap() free blocks behind it.  Every read is still evaluated whole and
 * exactly as if it were alone (bit for bit what the one-read-a-row batch gives): the convolutions see zero padding either side of it, the recurrent
 * layers start from a zero state at its first block and, in the reverse layers, at its last; partition function, posterior, Viterbi, strings and trace
 * are per read.  Results are indexed by READ, 0 .. nread - 1 in the order of the set call.  The default path and the launch-per-step kernels (FFHIP_RUN_STEPWISE_RNN,
 * and the fall-back of ffhip_batch_finish when a persistent layer launch timed out) only: the 8- and 10-state flip-flop models and the run-length model
 * FFHIP_NET_LSTM5_RLE of nbase 4, with 128 .. 512 hidden units; no FFHIP_RUN_KEEP_ACTS / _F32_RNN / _UNFUSED_RNN; a temperature of at least 0.1 --
 * ffhip_batch_run says so otherwise.  A packed run-length batch gives per read what one read a row gives: path, qpath, score, transitions and posterior, and
 * no base / quality strings or trace.  ffhip_batch_run_pair takes packed batches too. */
int ffhip_model_packable(const ffhip_model *mdl);         /* 1: this model's default path takes packed batches on this device */
size_t ffhip_model_pack_gap(const ffhip_model *mdl);      /* free blocks a read of a packed row needs behind it */
/* plan of a packed batch: slot[i] / block_off[i] for every read (slot -1: it did not fit into nslot rows of nsample_cap samples); returns the reads placed.  Longest read first,
 * each into the row that holds least so far: a launch runs as long as its longest row, and this rule leaves all rows within a short read of total / nslot (first fit -- the
 * rule before round 6's third session, FFHIP_DEBUG=pack_first_fit -- fills row after row to nsample_cap: profiles/r06_pack_bench.txt, fill 0.93 -> 0.98) */
int ffhip_pack_plan(const ffhip_model *mdl, int nslot, size_t nsample_cap, int nread, const size_t *nsample, int *slot, int *block_off);
/* rows (a multiple of 16, <= want_rows) of a packed batch of nsample-sample rows whose workspace fits 36 % of the device's memory (two such objects are
 * alive in a pipeline): 512 rows of 200 000 samples are ~90 GB at 384 hidden units */
int ffhip_pack_rows(const ffhip_model *mdl, int want_rows, size_t nsample);
int ffhip_pack_rows_for(const ffhip_model *mdl, int want_rows, size_t nsample, int nobjects);      /* the same for a pipeline of nobjects objects (72 % / nobjects each) */
ffhip_batch *ffhip_batch_create_packed(ffhip_engine *eng, const ffhip_model *mdl, int nslot, size_t nsample, int max_reads);
int ffhip_batch_set_prepared_packed(ffhip_batch *b, const ffhip_prep *prep, int nread, const int *reads /* indices into prep */, const int *slot, const int *block_off);
int ffhip_batch_set_signals_packed(ffhip_batch *b, int nread, const float *const *signals, const size_t *nsample, const int *slot, const int *block_off);
int ffhip_batch_nreads(const ffhip_batch *b);             /* reads of the last set call (a packed batch: its reads, not its rows) */
/* quantilef (util.c:100-139): p[] in, quantiles out */
int ffhip_quantiles(ffhip_engine *eng, const float *x, size_t n, float *p, size_t np);
/* difference_array / shift_scale_array / both (FFHIP_PREP_DELTA) on one host array, in place */
int ffhip_array_transform(ffhip_engine *eng, float *x, size_t n, int mode, float shift, float scale);
/* madf (util.c:164-187): 1.4826 * median(|x - med|); med == NULL: about the array's own median */
int ffhip_mad(ffhip_engine *eng, const float *x, size_t n, const float *med, float *mad);
/* medmad_normalise_array (util.c:198-212) in place; optionally returns the median and MAD used */
int ffhip_medmad_normalise(ffhip_engine *eng, float *x, size_t n, float *median, float *mad);

/* ---- measurement ----------------------------------------------------------------------------- */
/* HIP-event timing of the kernel groups of one batch_run, on the stream they are launched on.
 * groups: 0 conv, 1 in-projection GEMMs, 2 recurrent, 3 head+CRF norm, 4 posterior, 5 viterbi+assembly */
#define FFHIP_NGROUP 6
int ffhip_engine_set_profiling(ffhip_engine *eng, int on);
int ffhip_batch_profile(const ffhip_batch *b, float ms[FFHIP_NGROUP], int launches[FFHIP_NGROUP]);
/* how often a batch of this engine was re-run on the launch-per-step kernels because a persistent layer launch timed out waiting for
 * its peer workgroups (another tenant on the GPU); each occurrence also warns on stderr once per process and sends the next 64 runs
 * to those kernels directly */
int ffhip_debug_fallback_count(const ffhip_engine *eng);
/* the rule that picks a layer launch of the split-operand kernels (needs no engine, touches no device): for a model of `kind` (0 LSTM, 1 GRUmod) and `hidden`
 * units with `remaining` read tiles (of 16 reads) of a batch still to launch on `ncu` compute units, `beside` != 0 when another batch is in flight,
 * out = { form (0 one tile a group, 1 a pair, 2 dense at 384, 3 dense at 256, 4 packed, 5 no kernel), read tiles the launch takes, tiles a group, workgroups,
 * workgroups of that kernel sharing a compute unit, 1 if the launch fills the chip (the next layer launch waits for it) }.  Reads FFHIP_DEBUG (no_dense, no_pack).
 * Returns FFHIP_OK, or FFHIP_EINVAL without `out` */
int ffhip_debug_split_plan(int kind, int hidden, int remaining, int ncu, int beside, int out[6]);
/* 1 if two batches of `nrt` read tiles each may share paired layer launches (ffhip_batch_run_pair), else 0; reads FFHIP_DEBUG (no_dense, no_pair); no engine, no device */
int ffhip_debug_split_pair_ok(int kind, int hidden, int nrt, int ncu);
/* where the fields of a batch's result block lie (the block ffhip_batch_finish brings down in one copy; needs no engine, touches no device): for a batch of `nread`
 * rows taking `cap_reads` reads (at least nread) of `Tb` blocks a row whose block holds `sections` (bit 2 run records' base and estimate, 3 their shape / scale /
 * dwell, 4 5mC bytes, 5 move table; head and core always), out = { byte offsets of sat, abort, lens, score, bases, quals, nrun, fail, len, base, est, shape, scale,
 * dwell, ml, mv; ends of the sections head, core, runs, records, mod, moves } -- 22 values, a section the block lacks where it would be added.
 * Returns FFHIP_OK, or FFHIP_EINVAL (no `out`, nout < 22, nread or Tb < 1) */
int ffhip_debug_result_layout(int nread, int cap_reads, int Tb, unsigned sections, size_t *out, int nout);
/* device memory the batch holds (its buffers, grown on first use by the paths its runs took): a packed batch's launch-per-step run adds less than one
 * activation buffer to what its default run holds -- the in-projection is computed a window of steps at a time */
size_t ffhip_debug_batch_device_bytes(const ffhip_batch *b);
/* Reads whose swish-convolution outputs left the range of the default path's operand format (two fp16 slices of value * 2^4: +-4094;
 * the reference's swish_activation_inplace, layers.c:24-33, has no bound): the producing kernels flag them, ffhip_batch_finish runs
 * them again through the all-f32 kernels (FFHIP_RUN_F32_RNN, no bound) and puts those results in place -- no read is returned
 * clamped.  The count of the batch's last run / of the engine's lifetime (the flappie binary prints the latter in its summary). */
int ffhip_batch_f32_reruns(const ffhip_batch *b);
unsigned long long ffhip_engine_f32_reruns(const ffhip_engine *eng);

#ifdef __cplusplus
}
#endif
#endif
