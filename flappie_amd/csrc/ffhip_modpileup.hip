// ffhip_modpileup.hip -- per reference C (on the - strand: G), how methylated the aligned calls say it is (FFHIP_RUN_MOD_PILEUP, include/ffhip.h "mod pileup"): the
// counters of a mod pileup object, which every finished batch it is attached to adds to.  Integer adds only, so the counters are the same bytes whatever the batch
// size, packing, pairing or read order.  The twin of ffhip_pileup.hip, whose shape it keeps.
//
// k_modpileup: one workgroup an entry of truth's read list, launched by ffhip_batch_finish behind everything that may still patch the read's records, letters and 5mC
// bytes (the f32 re-runs).  Which read counts, n, m, K, q and the span come from the truth and the map record as in k_pileup; the ops go a thread each in chunks of
// the workgroup's size, j and i from two wave ballots, the waves before through LDS, the chunks before in a running carry.  No thread walks ops.  New against
// k_pileup: the reference's letter at the op's position, one load from the 2-bit words the map searches (a word of padding ahead of the first record), and only a
// lane ON A SITE goes on -- to one load of the call's letter, one of its 5mC byte, one LDS add into the workgroup's histogram and one no-return add into a plane.
// The planes are [strand][column][position]: the lanes of a wave that hit one plane hit ascending words.  The totals are ballot popcounts kept by every wave, summed
// through LDS at the end and added with one 64-bit atomic each; the histogram's 256 bins likewise, a thread a bin, a bin that stayed 0 adds nothing.
// 256 threads, 1184 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kModPileupNT = 256, kModPileupNW = kModPileupNT / 64;
enum { MT_READS = 0, MT_SKIPPED, MT_SITES, MT_MOD, MT_CANON, MT_FAIL, MT_DIFF, MT_DEL };
static_assert(MT_DEL + 1 == kModPileupTotals && MT_MOD + kModPileupColumns == kModPileupTotals, "a column's total stands at MT_MOD + column");

__global__ void __launch_bounds__(kModPileupNT)
k_modpileup(const unsigned *__restrict__ words, const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec,
            const int *__restrict__ trec, const uint8_t *__restrict__ ops, const char *__restrict__ bases, const uint8_t *__restrict__ ml, int TbS, ReadMap map,
            ModPileupView pv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ int wj[2][kModPileupNW], wi[2][kModPileupNW];
    __shared__ unsigned wtot[kModPileupNW][1 + kModPileupColumns];
    __shared__ unsigned hist[256];
    static_assert(kModPileupNT == 256, "a thread a bin of the histogram");
    const TruthRead e = list[blockIdx.x];
    const int read = e.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int *rc = trec + (size_t)read * kTruthRecInts;
    const uint4 r0 = maprec[(size_t)read * 4], r1 = maprec[(size_t)read * 4 + 1];
    if (rc[0] != 1 || (int)r0.x != 1) return;                   // (every exit up to the loop is the whole workgroup's, and ahead of the first barrier)
    const int n = rc[1], m = rc[2], K = rc[9];
    const long long nm = rc[4], all = nm + rc[5] + rc[6] + rc[7];
    if (1000ll * nm < (long long)pv.min_identity * all) {
        if (tid == 0) atomicAdd(pv.totals + MT_SKIPPED, 1ull);
        return;
    }
    const int q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
    if (q < 0 || q >= 2 * nrec || K < 0 || K > e.cap || n < 0 || m < 1) return;      // (records that k_map_finish and k_truth do not write: nothing is counted)
    const int2 rk = recs[q >> 1];                                // { off_k, M_k }
    if (ts < 0 || te > rk.y || te - ts != m) return;
    const int o = q & 1, Mk = rk.y;
    const unsigned site_code = o ? 2u : 1u;                      // the forward letter of a site: C on the + strand, G on the - strand
    const size_t P = pv.P;
    unsigned *cnt = pv.counts + (size_t)o * kModPileupColumns * P + (size_t)rk.x;
    const uint8_t *op = ops + e.ops + (size_t)(e.cap - K);
    const size_t row = map.row1(read, TbS);
    const char *bs = bases + row;
    const uint8_t *mb = ml + row;
    const unsigned long long below = (1ull << lane) - 1ull;
    hist[tid] = 0u;                                              // (seen by all behind the first chunk's barrier, which stands ahead of its adds)
    int cj = 0, ci = 0;                                          // truth and call bases consumed by the chunks before
    unsigned t_site = 0, t_col[kModPileupColumns] = { 0, 0, 0, 0, 0 };      // this wave's share of the totals (the same in all its lanes)
    for (int k0 = 0, buf = 0; k0 < K; k0 += kModPileupNT, buf ^= 1) {
        const int k = k0 + tid;
        const bool live = k < K;
        const int code = live ? (int)op[k] : 4;
        const unsigned long long bt = __ballot(live && code != 2), bc = __ballot(live && code != 3);
        if (lane == 0) { wj[buf][wv] = __popcll(bt); wi[buf][wv] = __popcll(bc); }
        __syncthreads();                                         // (one a chunk: the next chunk writes the other half)
        int j = cj + __popcll(bt & below), i = ci + __popcll(bc & below);
#pragma unroll
        for (int w = 0; w < kModPileupNW; w++) {
            const int tj = wj[buf][w], ti = wi[buf][w];
            j += w < wv ? tj : 0; i += w < wv ? ti : 0;
            cj += tj; ci += ti;
        }
        const bool diag = code <= 1, del = code == 3;
        const int f = o ? Mk - 1 - (ts + j) : ts + j;
        bool site = false;
        if ((del || (diag && i < n)) && f >= 0 && f < Mk) {
            const size_t g = (size_t)kMapPad + (size_t)rk.x + (size_t)f;
            site = ((words[g >> 4] >> (2 * (int)(g & 15))) & 3u) == site_code;
        }
        int col = -1;
        if (site) {
            col = 4;
            if (diag) {
                col = 3;
                if (seq_code(bs[i]) == 1u) {                     // C or Z: the class follows the call's letter, not the op
                    const int v = (int)mb[i];
                    atomicAdd(&hist[v], 1u);
                    col = v >= pv.hi ? 0 : v <= pv.lo ? 1 : 2;
                }
            }
            atomicAdd(cnt + (size_t)col * P + (size_t)f, 1u);
        }
        t_site += __popcll(__ballot(site));
#pragma unroll
        for (int c = 0; c < kModPileupColumns; c++) t_col[c] += __popcll(__ballot(col == c));
    }
    if (lane == 0) {
        wtot[wv][0] = t_site;
#pragma unroll
        for (int c = 0; c < kModPileupColumns; c++) wtot[wv][1 + c] = t_col[c];
    }
    __syncthreads();
    if (const unsigned v = hist[tid]) atomicAdd(pv.hist + tid, (unsigned long long)v);
    if (tid < 1 + kModPileupColumns) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kModPileupNW; w++) v += wtot[w][tid];
        if (v) atomicAdd(pv.totals + MT_SITES + tid, v);
    } else if (tid == 1 + kModPileupColumns) atomicAdd(pv.totals + MT_READS, 1ull);
}

void launch_modpileup(hipStream_t s, const MapRefView &ref, const TruthRead *list, int count, const void *map_records, const int *truth_records, const uint8_t *ops,
                      const char *bases, const uint8_t *ml, int Tb, ReadMap map, const ModPileupView &pv) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_modpileup, dim3(count), dim3(kModPileupNT), 0, s, ref.words, ref.recs, ref.nrec, list, (const uint4 *)map_records, truth_records, ops, bases, ml,
                       Tb, map, pv);
}

}  // namespace ffhip
