// ffhip_internal.hpp -- shared declarations between the HIP kernels and the host engine.
// gfx950 (MI355X) only.  Not part of the public boundary (include/ffhip.h is).
#pragma once
#include "ffhip_split.hpp"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// Head and decode kernels (remap and barcodes among them) run beside the NEXT batch's convolutions (run_front in ffhip_engine.hip, FFHIP_DEBUG=front_order=...) and the
// next layer launches wait for them: their waves go first on a shared SIMD (the convolutions stay at priority 0)
#ifndef FFHIP_DECODE_PRIO
#define FFHIP_DECODE_PRIO 2
#endif
#define FFHIP_DECODE_PRIO_SET() __builtin_amdgcn_s_setprio(FFHIP_DECODE_PRIO)

namespace ffhip {

// Development switches live in ONE environment variable: FFHIP_DEBUG=token[,token=value ...] (INTEGRATION.md section 6 lists them).
// dbg(token): nullptr when the token is absent, otherwise its value ("" for a bare token) -- what getenv gave when every switch
// had a variable of its own (rounds 1-4: 41 of them).  Looked up per call: tests flip switches between runs of one process.
// A token the library does not read is reported once on stderr (ffhip_engine.hip kDebugTokens).
const char *dbg(const char *token);

// ---------------------------------------------------------------------------------------------
// Data layouts in HBM (all fp32 unless noted).  B16 = ceil(nread/16) read tiles, Bp = 16*B16.
//
//  sample-major  S[r][pad + t][F]        conv inputs; `pad` zero rows before and after the T real
//                                        rows, read stride rs floats.  A window of `winlen` samples
//                                        is one contiguous vector of winlen*F floats.
//  tile-interleaved  A[t][rt][k/4][r16][k%4]
//                                        recurrent-stack activations (H features).  For one
//                                        (t, read tile) the 16 reads x 16 consecutive features are
//                                        1 KiB in exactly the lane order of an MFMA 16x16x4 f32
//                                        B-fragment quad: lane l=(kq=l>>4, r=l&15) holds float4
//                                        {k = 16*k16 + 4*kq + 0..3}.
//  D-fragment  X[t][rt][mt][lane][4]     gate pre-activations (Wi x + b).  Rows are permuted
//                                        unit-major/gate-minor (m = 4*u + g), so an MFMA output tile
//                                        (lane l: rows 4*(l>>4)+0..3, column l&15) gives every lane
//                                        the 4 gates of ONE hidden unit of ONE read.
//  weights  W[mt][k16][lane] float4      A-fragment order, lane l=(i=l&15, kq=l>>4) holds
//                                        W[16*mt + i][16*k16 + 4*kq + 0..3].
//  trans/post  T[r][blk][Ps]             Ps = 4*ceil(P/4): byte-identical to the reference's
//                                        flappie_matrix image of one read (column = block).
// ---------------------------------------------------------------------------------------------

constexpr int kSamplePad = 64;     // zero rows either side of a sample-major buffer
constexpr int kMaxState = 16;      // nstate <= 16 (nbase <= 8)
constexpr int kNoWindow = INT32_MIN;
constexpr int kZeroCol = INT32_MIN + 1;   // window-table entry of a column beyond a read's end in a ragged batch

struct SampleBuf {                 // sample-major activation buffer
    float *p;
    int F;                         // features per sample (exact, no padding)
    int T;                         // real samples
    size_t rs;                     // read stride in floats
    __host__ __device__ const float *row(int r, int t) const { return p + (size_t)r * rs + (size_t)(kSamplePad + t) * F; }
};

enum Act { ACT_NONE = 0, ACT_SWISH = 1, ACT_TANH = 2 };

// Packed batches (round 6; ffhip_batch_set_prepared_packed): several reads stand one behind the other in a slot (a row of the batch's buffers), so that a batch of reads
// of any lengths costs what its samples cost.  The convolutions, the layer kernels and the CRF head work on SLOTS (window tables / a live mask say where the reads are);
// everything per READ -- chains, Viterbi, assembly, trace -- takes the read's first row in the buffers of Tb rows a slot (b0) and of Tb + 1 rows a slot (b1).
// Both nullptr: one read a slot, read r is row r.
struct ReadMap {
    const int *b0 = nullptr, *b1 = nullptr;
    int nslot = 0;
    __device__ __forceinline__ size_t row0(int read, int TbS) const { return b0 ? (size_t)b0[read] : (size_t)read * (size_t)TbS; }
    __device__ __forceinline__ size_t row1(int read, int TbS) const { return b1 ? (size_t)b1[read] : (size_t)read * (size_t)(TbS + 1); }
};

// ---- kernel launchers (ffhip_kernels.hip) ----------------------------------------------------
// The launchers of the convolutions and of the CRF head return the kernel form they took (ffhip_debug_batch_forms; the numbering of include/ffhip.h)
enum KernelForm { kFormNone = -1, kFormConvSmall4x5 = 1, kFormConvSmall16x20, kFormConvSmall4, kFormConvSmall16, kFormConvSmall32, kFormConvMfmaVec, kFormConvMfmaScalar,
                  kFormConvSplitWs10, kFormConvSplit44, kFormConvSplit22, kFormHead3, kFormHead4, kFormHeadSplit3, kFormHeadSplit4 };
void launch_pack_signal(hipStream_t s, const float *src, size_t ld, SampleBuf dst, int nread);

// VALU convolution for the thin front layers; W dense taps [Fout][winlen][Fin]
int launch_conv_small(hipStream_t s, SampleBuf in, SampleBuf out, const float *W, const float *bias,
                       const int *x0a, const int *x0b, int Bp, int Tout, int winlen, int act, int ldp = 0,     // ldp: entries per read of a per-read window table (0 = shared)
                       const int *tin = nullptr,                                  // stride-1 layer of a ragged batch: per-read input lengths instead of a table
                       int split_exp = -100000,                                   // > -1000 (16 output features): write fp16 slices of value * 2^split_exp for launch_conv_split
                       unsigned *sat = nullptr,                                   // per-read word set to 1 when a value leaves the split format's range (ffhip_split.hpp: clamped there; the engine re-runs such a read on the f32 path)
                       const int *seg = nullptr);                                 // stride-1 layer of a packed batch: [Bp + 1] offsets, then every row's sorted read boundaries {start, end, ...} in columns

// MFMA convolution of the last conv layer: sample-major in, tile-interleaved out [Tout][B16][M/4][16][4]
int launch_conv_mfma(hipStream_t s, SampleBuf in, float *out, const float4 *Wp, const float *bias,
                      const int *x0a, const int *x0b, int B16, int Tout, int M, int K16, int act, int ldp = 0,
                      void *out_split = nullptr, int split_exp = 0, unsigned *sat = nullptr,      // out_split != nullptr: write the split layout of ffhip_rnn_split.hip (values * 2^split_exp) INSTEAD of `out` (M % 128 == 0)
                      int K = 0);      // values of a window (winlen * Fin; 0: 16 K16): the fragment's elements behind it read as zero

// the same convolution on split operands (16 input features): `in` holds fp16 slices (launch_conv_small with split_exp = kSplitExpX),
// Wp the split weight pack [M/16][ceil(winlen/2)][2][64] x 16 B scaled by 2^(acc_exp - kSplitExpX)
int launch_conv_split(hipStream_t s, SampleBuf in, float *out, const void *Wp, const float *bias, const int *x0a, const int *x0b,
                       int B16, int Tout, int M, int winlen, int act, int ldp, void *out_split, int split_exp, int acc_exp, int lean = 0, unsigned *sat = nullptr);      // lean: the <= 128-VGPR shape

// Xa = Wi^T x + b for every (t, read); in tile-interleaved, out D-fragment order
void launch_inproj(hipStream_t s, const float *in, float *xa, const float4 *Wp, const float *bias,
                   int ntile /*Tb*B16*/, int M /*rows, mult of 16*/, int K16);

// one recurrent step for all reads (launch-per-step path); live: a packed batch's mask [t][read tile] (tbs is not read then)
void launch_lstm_step(hipStream_t s, const float4 *sWp, const float *xa_t, const float *h_prev, float *h_out,
                      float *cstate, int B16, int H, int first, int t = 0, const int *tbs = nullptr, const unsigned *live = nullptr);
void launch_gru_step(hipStream_t s, const float4 *sWp, const float *xa_t, const float *h_prev, float *h_out,
                     int B16, int H, int first, int t = 0, const int *tbs = nullptr, const unsigned *live = nullptr);

// persistent recurrent layer (ffhip_rnn_persist.hip): one launch per layer and chunk of read tiles
bool persist_supported(int kind, int H, int ncu);
int persist_max_tiles(int kind, int H, int ncu, int fused);      // read tiles one launch can take (all workgroups co-resident)
bool launch_rnn_persist(hipStream_t s, int kind, const float4 *sWp, const float *xa, float *hout, unsigned *flags,
                        unsigned *abort_word, int Tb, int B16, int H, int rt0, int nrt, int backward, int mode,
                        const int *tbs = nullptr, const int *tbt = nullptr);      // ragged batch: blocks per read / max per tile
size_t persist_flag_words(int H, int nrt);
bool fused_supported(int kind, int H);
bool launch_lstm_fused(hipStream_t s, int kind, const float4 *sWp, const float4 *iWp, const float *bias, const float *xin, float *hout,
                       unsigned *flags, unsigned *abort_word, int Tb, int B16, int H, int rt0, int nrt, int backward, int mode,
                       const int *tbs = nullptr, const int *tbt = nullptr);
int persist_blocks_per_cu(int kind, int H);

// persistent recurrent layer on 16-bit MFMAs over split operands (ffhip_rnn_split.hip, format in ffhip_split.hpp): two fp16 slices a value, three products
// kept -- the accuracy of fp32 arithmetic at three matrix instructions a multiply-add block.  Activations in the SPLIT layout
// A[t][rt][k/32][slice][lane][8 x 16 bit]: 4 bytes a value (-DFFHIP_SPLIT_BF16X3, the cross-check build: three bf16 slices, six products, 6 bytes).
void launch_gather_rows(hipStream_t s, const float *const *src, const int *lens, float *dst, size_t row_stride, int nrow, const long long *dst_off = nullptr);
// packed batches: the strided convolution's window table / the layer kernels' live mask from per-read records (ffhip_kernels.hip)
void launch_pack_conv_table(hipStream_t s, const int4 *reads, int nread, int maxcols, int winlen, int stride, int Tmax, int *x0a, int *x0b, unsigned *overflow);
void launch_pack_live(hipStream_t s, const int4 *reads, int nread, int maxblocks, int B16, unsigned *live);
bool split_supported(int kind, int H);
// One layer launch of the split-operand kernels, decided in one place (split_plan): the kernel form, the read tiles it takes of the `remaining` ones of a
// batch, its grid, and whether it fills the chip.  `beside`: another batch is between run and finish.
enum SplitForm { kSplitOneTile, kSplitPairTiles, kSplitDense3, kSplitDense256, kSplitPack, kSplitNone };
// kSplitNone: no layer kernel for (kind, H).  For a kind 0 / 1 and an H of 128 .. 512 without one (GRUmod at 512) the other fields are still filled, with what a pair-form
// launch there would be -- the rules split_plan replaced answered for those shapes too, and tests/golden/split_plan_table.json holds their answers; all zero otherwise.
struct SplitPlan {
    SplitForm form;
    int nrt;                          // read tiles (of 16) this launch takes
    int ts, workgroups, per_cu;       // tiles a group, grid size, workgroups of this kernel that share a CU
    bool fills_chip;                  // 2 * workgroups > ncu * per_cu: a second such launch is not co-resident with this one
};
SplitPlan split_plan(int kind, int H, int remaining, int ncu, int beside);
size_t split_flag_words(int nrt);
size_t split_pack_offset(int H);           // 16-byte pieces in front of the gate-major weight pack of the packed GRUmod form
inline size_t split_bytes(size_t ntile, int H) { return ntile * (size_t)H * 32 * kSplitNS; }      // 16 reads x H x 2 B x slices
struct SplitLaunch {          // one batch's buffers and counts of a layer launch (scale_exp: the exponent S both products carry)
    const void *Wp; const float *bias; const void *xin; void *hout; float *hout_f32; unsigned *flags, *abort_word;
    int Tb, B16, rt0, nrt, backward, mode, scale_exp, fast_gates; const int *tbs, *tbt; unsigned epoch;
    const unsigned *live = nullptr;      // packed batch: bit r of word [t][read tile] = slot r holds a block of a read at step t (ffhip_rnn_split.hip SplitArgs)
};
bool split_pair_ok(int kind, int H, int nrt, int ncu);      // two batches of nrt read tiles each can share a layer launch: what launch_lstm_split_pair takes
bool launch_lstm_split_pair(hipStream_t s, int kind, int H, int ncu, const SplitLaunch &p0, const SplitLaunch &p1);
bool launch_lstm_split(hipStream_t s, int kind, int H, const SplitLaunch &l, const SplitPlan &p);      // l.nrt == p.nrt; false: kSplitNone
// recurrence-only layer kernel on split operands behind launch_inproj_split (LSTM, H = 256 / 512): xa as from launch_inproj_split
bool rnn_split_supported(int kind, int H);
int rnn_split_max_tiles(int ncu);      // read tiles (of 16) a launch takes: 32 workgroups per PAIR of tiles, one per CU
bool launch_rnn_split(hipStream_t s, const void *Wsplit, const float *xa, void *hout, float *hout_f32, unsigned *flags, unsigned *abort_word,
                      int Tb, int B16, int H, int rt0, int nrt, int backward, int mode, int scale_exp, const int *tbs = nullptr, const int *tbt = nullptr);
// input projection GEMM on split operands: in_split = activations in the split layout, Wp = the split weight pack (its first
// matrix is Wi), xa = D-fragment order like launch_inproj
void launch_inproj_split(hipStream_t s, const void *in_split, float *xa, const void *Wp, const float *bias, int ntile, int H, int scale_exp);
void launch_split_from_f32(hipStream_t s, const float *in, void *out, size_t ntile, int H, int act_exp, unsigned *sat = nullptr, int B16 = 1);      // tile-interleaved fp32 -> split of in * 2^act_exp
void launch_f32_from_split(hipStream_t s, const void *in, float *out, size_t ntile, int H, int act_exp);
void launch_lean_math_check(hipStream_t s, int exponent, int steps, unsigned long long *bad);      // adds the mismatch count to *bad
// the gate functions of ffhip_math.hpp one element at a time (ffhip_debug_gate_math): the numbering of include/ffhip.h
enum GateForm { kGateLogisticRef = 0, kGateTanhRef, kGateLogisticRef4Lean, kGateLogisticRef2Lean, kGateLogisticRefLean, kGateTanhRefLean, kGateSwishAct4,
                kGateTanhAct4, kGateLogisticHw1, kGateTanhHw1, kGateLogisticHw2, kGateTanhHw2, kGateForms };
void launch_gate_math(hipStream_t s, int form, const float *x, float *out, size_t n);

// the same head on the last layer's split output (ffhip_rnn_split.hip layout), weights as fp16 slices scaled by 2^(acc_exp - kSplitExpH)
int launch_head_split(hipStream_t s, const void *in_split, float *trans, const void *Wsplit, const float *bias,
                       int Tb, int B16, int nread, int P, int Ps, int Hc, float scale, int acc_exp, int raw, double *E = nullptr);
bool head_split_writes_E(int P);       // the head can leave exp(S - block max) for the linear-space chains (drops k_crf_exp)
// head: trans = tanh(W^T h + b) / (temperature/5)
int launch_head(hipStream_t s, const float *in, float *trans, const float4 *Wp, const float *bias,
                 int Tb, int B16, int nread, int P, int Ps, int K16, float scale, int raw = 0);      // raw = 1: W^T h + b only
// CRF partition function (fp64) + subtraction of (float)(logZ/Tb)
// logz: device buffer of nread doubles, receives the fp64 partition function per read; subtract = 0 leaves `trans` untouched
// tbs (optional, here and below): device array of the blocks of each read of a ragged batch; Tb is then the stride
void launch_crf_norm(hipStream_t s, float *trans, int nread, int Tb, int nbase, int Ps, double *logz, int subtract = 1, const int *tbs = nullptr);
// the same in linear space (fp64 scaled forward recursion); E = workspace of nread*Tb*crf_exp_stride(P) doubles,
// R = blocks between power-of-two rescalings (see crf_rescale_interval)
inline int crf_exp_stride(int P) { return (P + 1 + 7) & ~7; }
// per block the spread of alpha grows by at most exp(2*bound) (bound = max |score|) times nstate
inline int crf_rescale_interval(float bound) {
    const float bits = 2.0f * bound * 1.4427f + 4.0f;
    const int r = (int)(900.0f / bits);
    return r < 1 ? 0 : (r > 16 ? 16 : r);           // 0: range too wide for the linear form, use launch_crf_norm
}
void launch_crf_norm_linear(hipStream_t s, float *trans, double *E, int nread, int Tb, int nbase, int Ps, int R,
                            double *logz, int subtract = 1, const int *tbs = nullptr);
// forward/backward transition posteriors, log-normalised per block; fwd = workspace of 2*nread*(Tb+1)*kFwdRowBytes bytes
// E (optional, 8-state models): workspace of nread*Tb*crf_exp_stride(P) doubles, wide: nread ints -- with both the
// recursions run in linear space on exp(score - block max) (ffhip_decode.hip); reads whose scores span more than kFbRange per block keep the log-space kernel
void launch_transpost(hipStream_t s, const float *trans, float *post, float *fwd, int nread, int Tb, int nbase, int Ps, const int *tbs = nullptr,
                      double *E = nullptr, int *wide = nullptr);
constexpr size_t kFwdRowBytes = 10 * sizeof(double);   // per block and direction of the forward / backward workspace: kMaxState floats (log-space kernels) or up to 10 doubles (ffhip_decode.hip)
constexpr float kFbRange = 100.0f;       // max - min of a block's scores the scaled linear-space recursions take (fp64 range, scaling one pair of blocks behind)
// row_off / P_override: the run-length model's 32 transition scores sit behind 8 other rows of its 40-float blocks
void launch_crf_exp(hipStream_t s, const float *trans, double *E, int nread, int Tb, int nbase, int Ps, const int *tbs, int *wide, float limit, int row_off = 0, int P_override = 0);
// The run-length model's per-read kernels (nbase 4, stride 40).  nrow rows of Tb blocks (extents tbs) hold the head's output; the reads are nread = nrow reads a row
// (tbr = tbs) unless given: a packed batch's reads, their blocks tbr and their rows (map); gblk = the blocks per read the grids of the block-parallel kernels (k_rle_sub,
// k_rle_post8) are sized for -- Tb, or a packed batch's mean read: a longer read's workgroups stride over it.
void launch_rle_partition8x(hipStream_t s, const float *param, double *logz, int nread, int Tb, const int *tbs, ReadMap map = ReadMap());
void launch_rle_post8(hipStream_t s, const float *param, float *post, double *E, double *fwd, int nrow, int Tb, const int *tbs,
                      int nread = 0, const int *tbr = nullptr, ReadMap map = ReadMap(), int gblk = 0);
// ffhip_decode.hip: partition function (+ subtraction, flags & 1) and posterior (flags & 2) of 8- or 10-state reads from E in one launch; fwd = 2*nread*(Tb+1)*(2*nbase) doubles
void launch_crf_fb(hipStream_t s, int nbase, const double *E, float *trans, float *post, double *fwd, int nread, int Tb, double *logz, const int *tbs,
                    int flags, const int *wide, ReadMap map = ReadMap());
void launch_viterbi10x(hipStream_t s, const float *score_mat, uint8_t *tb, int *path, float *qpath, float *score, int nread, int Tb, const int *tbs, ReadMap map = ReadMap());
void launch_rle_viterbi8x(hipStream_t s, const float *param, uint8_t *tb, int *path, float *qpath, float *score, int nread, int Tb, const int *tbs, ReadMap map = ReadMap());
void launch_viterbi8x(hipStream_t s, const float *score_mat, uint8_t *tb, int *path, float *qpath, float *score, int nread, int Tb, const int *tbs, ReadMap map = ReadMap());
// Viterbi + traceback + qpath
void launch_viterbi(hipStream_t s, const float *score_mat, uint8_t *tb, int *path, float *qpath, float *score,
                    int nread, int Tb, int nbase, int Ps, const int *tbs = nullptr, ReadMap map = ReadMap());
// change positions -> base / quality strings
void launch_assemble(hipStream_t s, const int *path, const float *qpath, char *bases, char *quals, int *lens,
                     int nread, int Tb, int nbase, const int *tbs = nullptr, ReadMap map = ReadMap());
// 5mC probabilities of the called C / Z bases of a 5-base model (k_mod_probs): one byte a called base at the read's row of the (Tb + 1)-entry buffers
void launch_mod_probs(hipStream_t s, const float *post, const int *path, uint8_t *ml, int nread, int Tb, int Ps, const int *tbs = nullptr, ReadMap map = ReadMap());
// move table of the called bases (k_moves): one byte a block at the read's row of the (Tb + 1)-entry buffers, 1 where the block's transition emits a base
void launch_moves(hipStream_t s, const int *path, uint8_t *moves, int nread, int Tb, const int *tbs = nullptr, ReadMap map = ReadMap());
// barcode classification of the called reads (k_barcodes, ffhip_barcodes.hip): one 16-byte record a read (the layout of include/ffhip.h's ffhip_barcode_call) from the
// base strings and their lengths; dist_out / end_out, when given, take the whole [2][n] matrices of distances and end positions of read 0 (a launch of one read)
constexpr int kBarcodeMaxKit = 128, kBarcodeMaxLen = 128, kBarcodeMaxWindow = 256;
struct BarcodeKit {
    const unsigned long long *peq;      // [n][4][2]: bit i of word w of peq[k][c] = pattern k has base c (A C G T) at position 64 w + i
    const int *len;                     // [n]
    int n, window, words;               // patterns, bases of a window, 64-bit words the longest pattern takes (1 or 2)
};
void launch_barcodes(hipStream_t s, BarcodeKit kit, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map,
                     int max_dist, int min_sep, int both_ends, int *dist_out = nullptr, int *end_out = nullptr);
// adapters anywhere in the called reads (k_adapters, ffhip_adapters.hip; include/ffhip.h "adapters"): one 256-byte record a read -- a 16-byte header and up to 15
// hits of 16 bytes (ffhip_adapter_header, ffhip_adapter_hit) -- from the base strings and their lengths; d_out, when given, takes the whole score rows
// [2 n][len + 1] of read 0 (a launch of one read)
constexpr int kAdapterMaxKit = 32, kAdapterMaxLen = 64, kAdapterMaxHits = 15, kAdReach = 64, kAdSeg = 512;
constexpr size_t kAdapterRecBytes = 16 * (size_t)(kAdapterMaxHits + 1);
struct AdapterKit {
    const unsigned long long *peq;      // [2 n][4]: bit i of peq[q][c] = the oriented pattern of search q = 2 k + o has base c (A C G T) at position i
    const int *len;                     // [n]
    int n;
};
void launch_adapters(hipStream_t s, AdapterKit kit, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map,
                     int max_dist, uint8_t *d_out = nullptr);
// every call placed on a small reference (k_map_scan, k_map_finish, ffhip_map.hip; include/ffhip.h "map"): one 64-byte record a read (ffhip_map_call) from the base
// strings and their lengths.  `slots`: 2 nread ntask pairs of int32, the tasks' best (d, j); d_out, when given, takes the whole score rows of read 0's front anchor
// (a launch of one read)
constexpr int kMapMaxRecords = 1024, kMapMaxTotal = 1 << 20, kMapMaxAnchor = 4096, kMapSeg = 2048, kMapPad = 16, kMapWavesY = 128;
constexpr size_t kMapRecBytes = 64;
struct MapTask { int q, s, e, pad; };   // search q = 2 k + o, the ends (s, e] of record k's strand o (and 0, if s = 0)
struct MapRefView {
    const unsigned *words;              // the records' letters one behind the other, 2 bits a letter, 16 a word, kMapPad letters of padding before and behind
    const MapTask *tasks;               // [ntask], by (q, s)
    const int2 *recs;                   // [nrec]: { the record's first letter, its letters }
    const int *rowoff;                  // [2 nrec]: where search q's score row starts in d_out
    int ntask, nrec;
};
const char *map_invalid(int window, int max_error);      // nullptr, or what is wrong with the parameters (negative: the default)
void launch_map(hipStream_t s, const MapRefView &ref, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map, int window,
                int max_error, void *slots, int *d_out = nullptr);
// signal-to-sequence mapping (k_remap, ffhip_remap.hip; include/ffhip.h "remap"): per listed read one 16-byte record { status, L, score bits, end } at rec[read] and,
// for a mapped one, N bytes of 0 / 1 at the read's row of the (Tb + 1)-entry byte buffer `rm`.  A form is one instantiation of the kernel (0, 1: one wave; 2, 3: a
// workgroup): remap_form gives the smallest that holds a window of min(2 band + 1, L) cells, -1 when none does; a launch takes the reads of ONE form.
struct RemapRead {
    unsigned long long ws;              // the read's first 64-bit word in the traceback workspace (remap_ws_words(form, N) of them)
    unsigned seq;                       // its first entry in the coded sequences
    int L, status, read;                // bases; 0 no sequence, 1 to be mapped, 2 refused; the read's index in the batch
};
constexpr int kRemapForms = 4;
int remap_form(int L, int band);
int remap_max_window();
size_t remap_ws_words(int form, int nblock);
// the entries of a block's score row that position i of a sequence of codes 0 .. nbase - 1 reads: stay | move << 8 (host; the flip-flop coding of include/ffhip.h)
void remap_code(const uint8_t *codes, size_t L, int nbase, unsigned short *out);
void launch_remap(hipStream_t s, int form, const RemapRead *list, int count, const unsigned short *seq, const float *trans, int Ps, int band,
                  unsigned long long *ws, void *records, uint8_t *rm, int Tb, const int *tbs, ReadMap map);
// the call scored against a known sequence (k_truth, ffhip_truth.hip; include/ffhip.h "truth"): per listed read one record of kTruthRecInts int32
// { status, n, m, dist, matches, mismatches, insertions, deletions, maxdev, K, end, 0 } at rec[read] and, for an aligned one, its K op bytes RIGHT-aligned in the read's
// `cap` bytes of `ops` (the path's last op at [ops + cap - 1]; cap >= n + m).  A form is one instantiation of the kernel (0, 1: one wave; 2, 3: a workgroup):
// truth_form gives the smallest that holds a window of that many cells, -1 when none does; a launch takes the reads of ONE form.
struct TruthRead {
    unsigned long long ws;              // the read's first 64-bit word in the traceback workspace (truth_ws_words(form, m) of them)
    unsigned long long ops;             // its first byte in the ops buffer
    unsigned seq;                       // its first code in the truths
    int m, status, read, cap, room;     // bases; 0 no truth, 1 to be aligned, 2 refused; the read's index in the batch; its bytes of ops; truth from map: its share of
};                                      // the truths (the bound), which k_map_stretch fills -- it patches m and status; else 0
constexpr int kTruthForms = 4, kTruthRecInts = 12;
constexpr int kTruthMaxLen = 1 << 24;   // call and truth: the recursion's integers stay far below its +inf (1 << 29)
int truth_form(long long window);
int truth_max_window();
int truth_max_band();
size_t truth_ws_words(int form, int m);
void launch_truth(hipStream_t s, int form, const TruthRead *list, int count, const uint8_t *seq, const char *bases, const int *lens, int band,
                  unsigned long long *ws, int *records, uint8_t *ops, int Tb, const int *tbs, ReadMap map);
// truth from map (k_map_stretch, ffhip_map.hip; include/ffhip.h "truth from map"): for each of `count` entries of truth's list with status 1, from the map record at
// records[entry.read]: the stretch y_q[tstart : tend] as codes 0 .. 3 at seq + entry.seq, and entry.m and entry.status patched by the header's rule
void launch_map_stretch(hipStream_t s, const MapRefView &ref, const void *records, TruthRead *list, int count, uint8_t *seq);
// remap from map (k_map_remap_seq, ffhip_map.hip; include/ffhip.h "remap from map"): for each of `count` entries of remap's list with status 1, from the map record at
// records[entry.read]: the stretch y_q[tstart : tend] as remap_code's entries (stay | move << 8, alphabet of nbase) at seq + entry.seq, and entry.L and entry.status
// patched by the header's rule; an entry's room is the read's blocks (tbs[read], or Tb) + 1
void launch_map_remap_seq(hipStream_t s, const MapRefView &ref, const void *records, RemapRead *list, int count, unsigned short *seq, int nbase, int Tb, const int *tbs);
// The run-wide accumulators (ffhip_pile.hpp and the four files below).  What their launches take alike, a finished batch's (ffhip_features.hip pile_args) or one
// alignment's (pile_op): `count` entries of truth's list, the map records and the truth records (a read's at [entry.read]), the ops buffer (an entry's K op bytes
// right-aligned in its cap bytes) and the calls' letters (rows of Tb + 1, or as `map` says).  An entry's status is not read.  Atomics only.
struct PileArgs { const TruthRead *list; int count; const void *map_records; const int *truth_records; const uint8_t *ops; const char *bases; int Tb; ReadMap map; };
// ... and what the views of the three that count by reference position share: planes of P uint32 at counts, uint64 totals, the identity a read needs in per mille
struct PileView { unsigned *counts; unsigned long long *totals; size_t P; int min_identity; };
// pileup (k_pileup, ffhip_pileup.hip; include/ffhip.h "pileup"): the read's counts added into the 12 planes [strand][column][position] and the eight totals
// { reads, skipped, match, mismatch, del, ins, edge_ins, 0 }.  One launch, a workgroup an entry.
struct PileupView : PileView {};
constexpr int kPileupPlanes = 12, kPileupTotals = 8;
void launch_pileup(hipStream_t s, const MapRefView &ref, const PileArgs &a, const PileupView &pv);
// mod pileup (k_modpileup, ffhip_modpileup.hip; include/ffhip.h "mod pileup"): with the calls' 5mC bytes `ml` (rows as the letters'), the read's counts at the
// reference's C (- strand: G) positions added into the 10 planes [strand][mod canon fail diff del][position], the eight totals { reads, skipped, sites, mod, canon,
// fail, diff, del } and the 256 uint64 bins of the histogram of the counted bytes.  The reference's letters come from ref.words.  One launch, a workgroup an entry.
struct ModPileupView : PileView { unsigned long long *hist; int lo, hi; };
constexpr int kModPileupColumns = 5, kModPileupPlanes = 2 * kModPileupColumns, kModPileupTotals = 8, kModPileupBins = 256;
void launch_modpileup(hipStream_t s, const MapRefView &ref, const PileArgs &a, const uint8_t *ml, const ModPileupView &pv);
// consensus (k_consensus and k_consensus_call, ffhip_consensus.hip; include/ffhip.h "consensus"): the read's forward letters, deletions and inserted letters added
// into the 37 planes [plane][position] -- A C G T del, then A C G T of each of the 8 minor columns behind the position -- and the eight totals { reads, skipped,
// bases, del, ins_bases, long_ins, edge_ins, reserved }.  One launch, a workgroup an entry.  launch_consensus_call: a 16-byte ffhip_consensus_cell a position into
// `cells` (device memory), the reference's letters from ref.words.
struct ConsensusView : PileView {};
constexpr int kConsensusMinor = 8, kConsensusPlanes = 5 + 4 * kConsensusMinor, kConsensusTotals = 8;
enum { kConsensusLow = 0, kConsensusSame = 1, kConsensusSub = 2, kConsensusDel = 3, kConsensusIns = 4 };      // a cell's `what` (FFHIP_CONSENSUS_LOW ...: ffhip_consensus_call holds them equal)
void launch_consensus(hipStream_t s, const MapRefView &ref, const PileArgs &a, const ConsensusView &cv);
void launch_consensus_call(hipStream_t s, const MapRefView &ref, const ConsensusView &cv, unsigned min_depth, void *cells);
// error profile (k_errprofile, ffhip_errprofile.hip; include/ffhip.h "error profile"): with the calls' quality characters `quals` (rows as the letters') and the
// truths, the read's ops classed into kErrWords uint64 at ev.counts -- sub[4][5], ins[4], qual[94][3], ctx[1024][4], hp[4][16][33], then the twelve totals { reads,
// skipped, match, mismatch, del, ins, edge_ins, ctx_sites, hp_runs, hp_long, hp_wide, reserved }.  `ref` given: the mode of truth from map -- the map records are
// read and a truth letter comes from ref's words at the record's span; `seq` is not read.  `ref` null: a set truth -- a letter is seq[entry.seq + j] and no map
// record is read.  One launch of min(count, groups) workgroups, each taking every gridDim.x-th entry.
struct ErrProfileView { unsigned long long *counts; int min_identity; };
constexpr int kErrHpMaxRun = 16, kErrHpMaxCalled = 32, kErrHpMaxOps = 64;
constexpr int kErrAtSub = 0, kErrAtIns = 20, kErrAtQual = 24, kErrAtCtx = 306, kErrAtHp = 4402, kErrTableWords = 6514, kErrTotals = 12, kErrWords = kErrTableWords + kErrTotals;
void launch_errprofile(hipStream_t s, const MapRefView *ref, const PileArgs &a, int groups, const char *quals, const uint8_t *seq, const ErrProfileView &ev);
// the signal of every base of a mapped read (k_events, ffhip_events.hip; include/ffhip.h "events"): per listed read whose remap record at records[read] says
// { status 1, end 0 }, L events of 16 bytes { int32 first, count; float mean, sd } at events[out ..], from the read's samples sig[sig .. sig + n) and its bytes at the
// read's row of the (Tb + 1)-entry byte buffer `rm`; any other read writes nothing.  One form; the launch comes behind launch_remap on the same stream.
struct EventRead {
    unsigned long long sig;             // the read's first sample, in floats from `sig`
    unsigned long long out;             // its first event
    int n, L, read, pad;                // samples; the bases it has room for (a record with more writes nothing); the read's index in the batch
};
void launch_events(hipStream_t s, const EventRead *list, int count, const float *sig, int stride, const void *records, const uint8_t *rm, void *events,
                   int Tb, const int *tbs, ReadMap map);
// the poly(A) tail of a read (k_polytail, ffhip_polytail.hip; include/ffhip.h "poly tail"): per listed read the 32 bytes { int32 status, first, count, flat, calls;
// float level, rate, bases } at records[read], from the read's samples sig[sig .. sig + n) and its entries at the read's row of the (Tb + 1)-entry `path`; a read
// without blocks gets zeros.  wmu / wfl are the windows' workspace (a double and a byte a window, the read's first at `ws`; bit 0 of the byte is the flag); wq, when
// given, takes every window's q.  One form, one launch, behind the decode on the same stream.
struct PolyTailParams { int base, from_end, window, min_calls, gap, min_windows, search, min_bases; float max_sd; };      // include/ffhip.h's ffhip_polytail_params, byte for byte
struct PolyRead {
    unsigned long long sig;             // the read's first sample, in floats from `sig`
    unsigned long long ws;              // its first window in the workspace
    int n, read;                        // samples; the read's index in the batch
};
constexpr int kPolyTailMaxWindow = 64, kPolyTailMaxGap = 16;
constexpr size_t kPolyTailRecBytes = 32;
// nullptr when every parameter is in its range, else the range it leaves (a text for the error message)
const char *polytail_invalid(const PolyTailParams &p);
void launch_polytail(hipStream_t s, const PolyRead *list, int count, const float *sig, int stride, const int *path, int nbase, const PolyTailParams &p, void *records,
                     double *wmu, uint8_t *wfl, double *wq, int Tb, const int *tbs, ReadMap map);
// 5mC at every C / Z of a mapped sequence (k_site_starts + k_site_mods, ffhip_sitemods.hip; include/ffhip.h "site mods"), a model of nbase 5 only: per listed site
// whose read's remap record at records[read] says { status 1, end 0, L }, the 16 bytes { int32 pos, nblock; float can, mod } at out[site's index in `sites`], from
// the read's score rows, its coded sequence (remap_code) and its bytes at the read's row of the (Tb + 1)-entry byte buffer `rm`; any other read writes nothing.
// `starts` is the workspace of L + 1 int32 a listed read.  Two launches behind launch_remap on the same stream; all_paths picks the fp64 instantiation.
struct SiteRead {
    unsigned long long start;           // the read's first word in the workspace of starts
    unsigned seq;                       // its first entry in the coded sequences
    int L, read, pad;                   // the bases of its sequence; the read's index in the batch
};
struct SiteMod { int k, pos; };         // the site's read, as an index into the list of SiteRead; its position in the sequence
constexpr int kSiteModsMaxContext = 31; // a window of 2 c + 1 <= 63 positions: a lane a position
// the sites of one coded sequence, in increasing position (appended to *out with read index k when out is given); the count
size_t sitemods_sites(const unsigned short *coded, size_t L, int k, std::vector<SiteMod> *out);
void launch_site_mods(hipStream_t s, const SiteRead *list, int nread, const SiteMod *sites, int nsite, const unsigned short *seq, const float *trans, int Ps,
                      int context, int all_paths, const void *records, const uint8_t *rm, int *starts, void *out, int Tb, const int *tbs, ReadMap map);
// k_site_starts alone, for another list of reads and another workspace (ffhip_variants.hip launches it over its own): one launch, nread workgroups
void launch_site_starts(hipStream_t s, const SiteRead *list, int nread, const void *records, const uint8_t *rm, int *starts, int Tb, const int *tbs, ReadMap map);
// Ref against alt alleles of a mapped sequence (k_variants, ffhip_variants.hip; include/ffhip.h "variants"), nbase 4 or 5: per listed variant whose read's remap
// record at records[read] says { status 1, end 0, L }, the 16 bytes { int32 index, nblock; float ref, alt } at out[variant's place in `vars`], from the read's
// score rows, its coded sequence (remap_code), its starts (k_site_starts over `list`, launched here first) and the variant's 24 bytes; any other read writes
// nothing.  The reads' list has SiteRead's form.  Two launches behind launch_remap on the same stream; all_paths picks the fp64 instantiation.
struct Variant { int pos; uint8_t nref, nalt, alt[16], pad[2]; };      // include/ffhip.h's ffhip_variant, byte for byte
struct VarEntry { int k, index; Variant v; };           // the variant's read, as an index into the list of SiteRead; its place in the read's own list; the variant
constexpr int kVariantsMinContext = 1, kVariantsMaxContext = 23, kVariantsMaxAllele = 16;      // windows of 2 c + max(r, k) <= 62 positions: a lane a position
// nullptr when the variant keeps every limit of include/ffhip.h "variants" for a sequence of L codes, else the limit it breaks (a text for the error message)
const char *variant_invalid(const Variant &v, size_t L, int nbase);
void launch_variants(hipStream_t s, const SiteRead *list, int nread, const VarEntry *vars, int nvar, const unsigned short *seq, const float *trans, int Ps, int nbase,
                     int context, int all_paths, const void *records, const uint8_t *rm, int *starts, void *out, int Tb, const int *tbs, ReadMap map);
// exp + trace_from_posterior
void launch_trace(hipStream_t s, const float *post, int32_t *trace, int nread, int Tb, int nbase, int Ps, int is_log, const int *tbs = nullptr, ReadMap map = ReadMap());
void launch_exp_inplace(hipStream_t s, float *x, size_t n);
// run-length (runnie) head and decoders, ffhip_rle.hip: activation rows + runlengthV2 partition function + subtraction
// (a packed batch -- nread, tbr, map, gblk as for launch_rle_post8 -- needs nbase 4, stride 40)
void launch_rle_head_finish(hipStream_t s, float *param, double *logz, int nrow, int Tb, int nbase, int Ps, float temperature, const int *tbs = nullptr,
                            int nread = 0, const int *tbr = nullptr, ReadMap map = ReadMap(), int gblk = 0);
void launch_rle_partition(hipStream_t s, const float *param, double *logz, int nread, int Tb, int nbase, int Ps, const int *tbs = nullptr);
void launch_rle_transpost(hipStream_t s, const float *param, float *post, float *fwd, int nread, int Tb, int nbase, int Ps, const int *tbs = nullptr);
void launch_rle_viterbi(hipStream_t s, const float *param, uint8_t *tb, int *path, float *qpath, float *score, int nread, int Tb, int nbase, int Ps, const int *tbs = nullptr,
                        ReadMap map = ReadMap());      // map: a packed batch's reads (nbase 4, stride 40)
// run records + run-length estimates of a decoded run-length batch (k_rle_runs, nbase 4): per read nrun / fail / len (expanded length); per run, at the read's
// row of the (Tb + 1)-entry buffers, base and est, and shape / scale / dwell when those pointers are not null
struct RleRunScale { double f[4]; };
struct RleRunOut { uint8_t *base; int *est; float *shape, *scale; int *dwell; int *nrun, *fail; unsigned long long *len; };
void launch_rle_runs(hipStream_t s, const float *param, const int *path, int nread, int Tb, int nbase, int Ps, const int *tbs, ReadMap map,
                     const RleRunScale &sc, const RleRunOut &o);
// first-generation run-length decoders (decode.c:552-892) on one matrix of 4 nbase rows; tb: 8 bytes a block, fwd / bwd: 8 floats a block (+1)
void launch_rl1_viterbi(hipStream_t s, const float *param, uint8_t *tb, int *path, float *score, int nblk, int nbase, int Ps);
void launch_rl1_posterior(hipStream_t s, const float *param, float *post, float *fwd, float *bwd, int nblk, int nbase, int Ps);
void launch_rl1_mean(hipStream_t s, const float *param, const int *path, int *runlength, unsigned long long *seqlen, int nblk, int nbase, int Ps);
// tile-interleaved -> dense [Tb][H] of one read (debug tap)
void launch_untile(hipStream_t s, const float *act, float *dense, int read, int Tb, int B16, int H);

}  // namespace ffhip
