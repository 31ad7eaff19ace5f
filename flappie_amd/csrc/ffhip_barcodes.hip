// ffhip_barcodes.hip -- barcode classification of the called reads (FFHIP_RUN_BARCODES, include/ffhip.h "barcodes"): which sample a read belongs to.
//
// A kit is up to 128 patterns over ACGT of up to 128 bases.  A read's call s (Z read as C) gives two windows of min(W, len) bases: its front, and the front of
// its reverse complement.  Every pattern is searched in both by the infix edit distance (edlib's HW mode): D[0][j] = 0, D[i][0] = i, unit costs,
// dist = min_j D[L][j], end = the smallest j that attains it.  All of it is integer arithmetic: the results are exact.
//
// k_barcodes: one workgroup a read, 256 threads = 2 ends x 128 patterns, ONE PATTERN A LANE.  Myers' bit-vector recurrence (in Hyyro's form with
// a horizontal carry between words: myers_step, ffhip_seq.hpp) holds a column of the matrix as vertical differences in one 64-bit word a lane, two when the
// kit has a pattern longer than 64 (the carry out of bit 63 of the first enters the second).  The pattern's match masks Peq[4] stay in registers.  The window's
// characters are staged once in LDS as codes 0 .. 3, the rear window read from the call's end and complemented; the two waves of an end read the same
// character at every step (a broadcast), so lanes differ only in the bit that is their pattern's last row.  Bits above that row hold garbage that never
// reaches the rows below it (the addition carries upwards, the shifts move upwards).  A lane follows D[L][j] from D[L][0] = L through the horizontal
// differences at its top bit and keeps the first minimum.  The two distances of every pattern go through LDS to the first wave, which finds the minimum
// (lowest index first) and the runner-up by two butterfly reductions and writes the read's 16-byte record: nothing else leaves the kernel.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kBcThreads = 2 * kBarcodeMaxKit;
constexpr int kBcNone = 1000;                   // beyond every distance (<= 128): a lane without a pattern
static_assert(kBarcodeMaxKit == 128 && kBarcodeMaxLen == 128 && kBarcodeMaxWindow % 4 == 0, "two words a pattern, four waves a read, windows staged as whole words");

template <int NW>
__global__ void __launch_bounds__(kBcThreads)
k_barcodes(BarcodeKit kit, const char *__restrict__ bases, const int *__restrict__ lens, uint4 *__restrict__ rec, int TbS, const int *__restrict__ tbs, ReadMap map,
           int max_dist, int min_sep, int both_ends, int *__restrict__ dist_out, int *__restrict__ end_out) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ __attribute__((aligned(4))) uint8_t win[2][kBarcodeMaxWindow];
    __shared__ int sdist[2][kBarcodeMaxKit], send[2][kBarcodeMaxKit];
    const int read = blockIdx.x, tid = threadIdx.x;
    const int Tb = tbs ? tbs[read] : TbS;                // this read's blocks (uniform over the workgroup)
    if (Tb <= 0) {                                       // an empty slot: no call, no length to read -- best -1, every distance 255
        if (tid == 0) rec[read] = make_uint4(0xffffffffu, 0x0000ffffu, 0u, 0u);
        return;
    }
    const int len = lens[read] > 0 ? lens[read] : 0;
    const int m = len < kit.window ? len : kit.window;
    const char *bs = bases + map.row1(read, TbS);
    for (int j = tid; j < 2 * m; j += kBcThreads)        // front: s[j]; rear: the complement of s[len - 1 - j]
        if (j < m) win[0][j] = (uint8_t)seq_code(bs[j]);
        else win[1][j - m] = (uint8_t)(3u - seq_code(bs[len - 1 - (j - m)]));
    __syncthreads();
    const int end = tid / kBarcodeMaxKit, k = tid % kBarcodeMaxKit;      // waves 0, 1: the front; 2, 3: the rear
    const bool live = k < kit.n;
    unsigned long long peq[NW][4], pv[NW], mv[NW];
    const int L = live ? kit.len[k] : 1;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int w = 0; w < NW; w++) peq[w][c] = live ? kit.peq[((size_t)k * 4 + c) * 2 + w] : 0ull;
#pragma unroll
    for (int w = 0; w < NW; w++) { pv[w] = ~0ull; mv[w] = 0ull; }
    const int topw = (L - 1) >> 6, topb = (L - 1) & 63;
    int score = L, best = L, bend = 0;                   // D[L][0] = L
    const unsigned *w4 = reinterpret_cast<const unsigned *>(win[end]);
    for (int j0 = 0; j0 < m; j0 += 4) {
        const unsigned chars = __builtin_amdgcn_readfirstlane(w4[j0 >> 2]);      // four characters, the same in every lane of the wave
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (j0 + i >= m) break;
            const unsigned c = (chars >> (8 * i)) & 3u;
            int hin = 0, delta = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const MyersH h = myers_step(pv[w], mv[w], myers_eq(peq[w], c), hin);
                if (w == topw) delta = myers_diff(h, topb);
                hin = (int)(h.Ph >> 63) - (int)(h.Mh >> 63);
            }
            score += delta;
            if (score < best) { best = score; bend = j0 + i + 1; }      // the FIRST column of the minimum
        }
    }
    sdist[end][k] = live ? best : kBcNone;
    send[end][k] = bend;
    if (live && dist_out) { dist_out[end * kit.n + k] = best; end_out[end * kit.n + k] = bend; }      // the whole matrix (ffhip_op_barcode_scores)
    __syncthreads();
    if (tid >= 64) return;
    // s_k = min (both_ends: max) of the two distances; best = the lowest k of the minimum; second = the minimum over the others (255 for a kit of one)
    int s[2], key = kBcNone << 8;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int kk = tid + 64 * h, df = sdist[0][kk], dr = sdist[1][kk];
        s[h] = kk < kit.n ? (both_ends ? (df > dr ? df : dr) : (df < dr ? df : dr)) : kBcNone;
        const int kh = (s[h] << 8) | kk;
        key = kh < key ? kh : key;
    }
    key = wave_min(key);
    const int bi = key & 255, sb = key >> 8;
    int sec = kBcNone;
#pragma unroll
    for (int h = 0; h < 2; h++) if (tid + 64 * h != bi && s[h] < sec) sec = s[h];
    sec = wave_min(sec);
    if (sec >= kBcNone) sec = 255;
    if (tid == 0) {
        const int df = sdist[0][bi], dr = sdist[1][bi], ef = send[0][bi], er = send[1][bi];
        const bool classified = sb <= max_dist && sec - sb >= min_sep;
        const unsigned ends = (df <= max_dist ? 1u : 0u) | (dr <= max_dist ? 2u : 0u);
        // { int16 best; uint8 best_dist, second_dist | uint8 front_dist, rear_dist, ends, pad | int16 front_end, rear_end | int32 reserved }: ffhip_barcode_call
        rec[read] = make_uint4(((unsigned)(classified ? bi : -1) & 0xffffu) | ((unsigned)sb << 16) | ((unsigned)sec << 24),
                               (unsigned)df | ((unsigned)dr << 8) | (ends << 16), (unsigned)ef | ((unsigned)er << 16), 0u);
    }
}

void launch_barcodes(hipStream_t s, BarcodeKit kit, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map,
                     int max_dist, int min_sep, int both_ends, int *dist_out, int *end_out) {
    if (nread <= 0) return;
    uint4 *rec = (uint4 *)records;
    if (kit.words > 1) hipLaunchKernelGGL(k_barcodes<2>, dim3(nread), dim3(kBcThreads), 0, s, kit, bases, lens, rec, Tb, tbs, map, max_dist, min_sep, both_ends, dist_out, end_out);
    else hipLaunchKernelGGL(k_barcodes<1>, dim3(nread), dim3(kBcThreads), 0, s, kit, bases, lens, rec, Tb, tbs, map, max_dist, min_sep, both_ends, dist_out, end_out);
}

}  // namespace ffhip
