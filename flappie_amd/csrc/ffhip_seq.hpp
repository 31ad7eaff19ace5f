// ffhip_seq.hpp -- what the sequence kernels share, each written once: the letters' 2-bit codes and a reference's, one column of Myers' bit-vector recurrence, the 64-lane
// butterfly reductions, the flip-flop state coding of a coded position, and the two-hypothesis window recursion over a read's score rows.  Device code, except the
// state coding, which the host reads too.  Every result is an integer, or a float with a fixed order of operations: a kernel that calls these computes the same
// bytes wherever it stands.  Included by ffhip_adapters, _barcodes, _map, _truth, _pileup, _modpileup, _consensus, _errprofile, _polytail, _events, _remap, _sitemods and _variants.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "ffhip_internal.hpp"

namespace ffhip {

// ---- letters
__device__ __forceinline__ unsigned seq_code(char c) { return c == 'A' ? 0u : c == 'G' ? 2u : c == 'T' ? 3u : 1u; }      // C and Z: 1 (the call holds A C G T Z only)
// the letter at position g of a reference's 2-bit words (MapRefView::words: 16 letters a word, kMapPad letters of padding ahead of position 0)
__device__ __forceinline__ unsigned ref_letter(const unsigned *__restrict__ words, size_t g) {
    g += (size_t)kMapPad;
    return (words[g >> 4] >> (2 * (int)(g & 15))) & 3u;
}

// ---- Myers' bit-vector recurrence (J. ACM 46:395) in Hyyro's block form with a horizontal carry between words, as edlib's calculateBlock
// the match mask of the letter c among a word's four (all four read first: selects between registers, not branches around loads)
__device__ __forceinline__ unsigned long long myers_eq(const unsigned long long peq[4], unsigned c) {
    const unsigned long long a = peq[0], b = peq[1], g = peq[2], t = peq[3];
    return c == 0 ? a : c == 1 ? b : c == 2 ? g : t;
}

struct MyersH { unsigned long long Ph, Mh; };           // bit i: the horizontal difference of row i of the word is +1, is -1

// One column of one 64-bit word.  (pv, mv): the column as vertical differences, updated.  Eq: the column's match mask.  hin: the horizontal difference (-1, 0, +1)
// that enters at bit 0 -- 0 for a free start (D[0][j] = 0), +1 for an anchored one (D[0][j] = j), what left bit 63 of the word below otherwise; a constant folds
// away.  Returns the column's horizontal differences BEFORE the shift: the caller takes the bit of its last row, or bit 63 as the carry into the next word.
// Bits above a pattern's last row hold garbage that never reaches the rows below it (the addition carries upwards, the shifts move upwards).
__device__ __forceinline__ MyersH myers_step(unsigned long long &pv, unsigned long long &mv, unsigned long long Eq, int hin) {
    const unsigned long long neg = hin < 0 ? 1ull : 0ull, pos = hin > 0 ? 1ull : 0ull;
    const unsigned long long Xv = Eq | mv;
    Eq |= neg;
    const unsigned long long Xh = (((Eq & pv) + pv) ^ pv) | Eq;
    const MyersH h = { mv | ~(Xh | pv), pv & Xh };
    const unsigned long long Ph = (h.Ph << 1) | pos, Mh = (h.Mh << 1) | neg;
    pv = Mh | ~(Xv | Ph);
    mv = Ph & Xv;
    return h;
}
// the difference (-1, 0, +1) of the column at bit b
__device__ __forceinline__ int myers_diff(const MyersH &h, int b) { return (int)((h.Ph >> b) & 1ull) - (int)((h.Mh >> b) & 1ull); }

// ---- reductions over the wave's 64 lanes: an xor butterfly from 32 down to 1, every lane ends with the same value (a floating-point sum rounds in that order)
template <class T, class F>
__device__ __forceinline__ T wave_reduce(T v, F f) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = f(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) { return wave_reduce(v, [](int a, int o) { return o < a ? o : a; }); }
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) { return wave_reduce(v, [](unsigned long long a, unsigned long long o) { return o < a ? o : a; }); }
__device__ __forceinline__ long long wave_max(long long v) { return wave_reduce(v, [](long long a, long long o) { return o > a ? o : a; }); }
__device__ __forceinline__ int wave_sum(int v) { return wave_reduce(v, [](int a, int o) { return a + o; }); }
__device__ __forceinline__ double wave_sum(double v) { return wave_reduce(v, [](double a, double o) { return a + o; }); }

// ---- the flip-flop coding of a sequence over nbase letters: states 0 .. nbase - 1 are the flips, nbase .. 2 nbase - 1 the flops
// the entry of a block's score row for the step from -> to (trans_lookup, decode.c:104-114)
__host__ __device__ __forceinline__ int ff_lookup(int from, int to, int nbase) { return to < nbase ? to * 2 * nbase + from : 2 * nbase * nbase + from; }
// the state of a coded position (remap_code's low byte is ff_lookup(q, q))
template <int NB>
__host__ __device__ __forceinline__ int ff_state(unsigned short e) { const int st = e & 255; return st < 2 * NB * NB ? st / (2 * NB + 1) : st - 2 * NB * NB; }
// the state a letter takes behind state `prev` (prev < 0: the sequence's first position): the flop behind its own flip
template <int NB>
__host__ __device__ __forceinline__ int ff_next(int prev, int letter) { return (prev >= 0 && prev < NB && prev == letter) ? letter + NB : letter; }

// ---- the window recursion of two hypotheses over the blocks t0 .. t1 - 1 of a read's score rows T (Ps floats a row).  Lane j owns position j of the window of
// EITHER hypothesis h and reads two entries of a row: is[h] (stay: q_j -> q_j) and im[h] (move: q_{j-1} -> q_j; lane 0 has none).  X[h] starts as 0 in lane 0
// and -inf elsewhere and ends as the score of the paths from position 0 at block t0 to position j behind block t1 - 1: the best one (float32, one add a step and
// a strict compare) or all of them (ALL: fp64, log1p(exp())).  A step is, per hypothesis, one cross-lane move (the value of the lane below), two adds and the
// compare; the two hypotheses are independent chains and fill each other's latency.  The rows are read through the cache, kWinChunk blocks ahead of the chain in
// registers: no step waits for memory.  A hypothesis with fewer blocks than moves keeps -inf in its last lanes: no special case.
constexpr int kWinChunk = 8;            // blocks whose entries a lane holds ahead of the chain
template <bool ALL>
using win_real = typename std::conditional<ALL, double, float>::type;

template <bool ALL>
__device__ __forceinline__ void window_scores(const float *__restrict__ T, int Ps, int t0, int t1, const int (&is)[2], const int (&im)[2], int lane, win_real<ALL> (&X)[2]) {
    using real = win_real<ALL>;
    const real NEG = (real)-INFINITY;
    X[0] = X[1] = lane == 0 ? (real)0 : NEG;
    auto load = [&](int t, float (&a)[kWinChunk][4]) {                          // (t < t1; a block past the window's last reads the last again, unused)
#pragma unroll
        for (int u = 0; u < kWinChunk; u++) {
            const float *row = T + (size_t)min(t + u, t1 - 1) * Ps;
            a[u][0] = row[is[0]]; a[u][1] = row[im[0]]; a[u][2] = row[is[1]]; a[u][3] = row[im[1]];
        }
    };
    float cur[kWinChunk][4], nxt[kWinChunk][4];
    if (t0 < t1) load(t0, cur);
    for (int t = t0; t < t1; t += kWinChunk) {
        const bool more = t + kWinChunk < t1;
        if (more) load(t + kWinChunk, nxt);
#pragma unroll
        for (int u = 0; u < kWinChunk; u++) {
            if (t + u < t1) {                                                   // (uniform)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const real up = __shfl_up(X[h], 1, 64);
                    const real stay = X[h] + (real)cur[u][2 * h];
                    const real move = lane == 0 ? NEG : up + (real)cur[u][2 * h + 1];
                    const real m = move > stay ? move : stay;
                    if constexpr (ALL) X[h] = m == NEG ? NEG : m + log1p(exp(-fabs(stay - move)));
                    else X[h] = m;
                }
            }
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < kWinChunk; u++)
#pragma unroll
                for (int k = 0; k < 4; k++) cur[u][k] = nxt[u][k];
        }
    }
}

}  // namespace ffhip
