// ffhip_pileup.hip -- per reference position, what the aligned calls say there (FFHIP_RUN_PILEUP, include/ffhip.h "pileup"): the counters of a pileup object, which
// every finished batch it is attached to adds to.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.
//
// k_pileup: one workgroup an entry of truth's read list, launched by ffhip_batch_finish behind everything that may still patch the read's records (the f32 re-runs).
// The truth RECORD says whether the read is counted (status, the four counts for the identity test) and gives n, m and K; the map record gives q and the span; the
// list entry gives only where the ops lie (K bytes right-aligned in its cap bytes).  The ops go a thread each in chunks of the workgroup's size: an op's place on
// the reference and in the call follows from j and i, the truth and call bases consumed before it -- the popcount of the lanes below in two wave ballots (op != I,
// op != D), the waves before through LDS, the chunks before in a running carry.  No thread walks ops.  A thread then adds 1 to at most one counter: the planes are
// [strand][column][position], so the lanes of a wave that hit one plane hit consecutive words.  The totals are ballot popcounts kept by every wave, summed through
// LDS at the end and added with one 64-bit atomic each.  256 threads, under 100 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kPileupNT = 256, kPileupNW = kPileupNT / 64;
enum { PT_READS = 0, PT_SKIPPED, PT_MATCH, PT_MISMATCH, PT_DEL, PT_INS, PT_EDGE_INS, PT_RESERVED };

__global__ void __launch_bounds__(kPileupNT)
k_pileup(const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec, const int *__restrict__ trec,
         const uint8_t *__restrict__ ops, const char *__restrict__ bases, int TbS, ReadMap map, PileupView pv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ int wj[2][kPileupNW], wi[2][kPileupNW];
    __shared__ unsigned wtot[kPileupNW][5];
    const TruthRead e = list[blockIdx.x];
    const int read = e.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int *rc = trec + (size_t)read * kTruthRecInts;
    const uint4 r0 = maprec[(size_t)read * 4], r1 = maprec[(size_t)read * 4 + 1];
    if (rc[0] != 1 || (int)r0.x != 1) return;                   // (every exit up to the loop is the whole workgroup's)
    const int n = rc[1], m = rc[2], K = rc[9];
    const long long nm = rc[4], all = nm + rc[5] + rc[6] + rc[7];
    if (1000ll * nm < (long long)pv.min_identity * all) {
        if (tid == 0) atomicAdd(pv.totals + PT_SKIPPED, 1ull);
        return;
    }
    const int q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
    if (q < 0 || q >= 2 * nrec || K < 0 || K > e.cap || n < 0 || m < 1) return;      // (records that k_map_finish and k_truth do not write: nothing is counted)
    const int2 rk = recs[q >> 1];                                // { off_k, M_k }
    if (ts < 0 || te > rk.y || te - ts != m) return;
    const int o = q & 1, Mk = rk.y;
    const size_t P = pv.P;
    unsigned *cnt = pv.counts + (size_t)o * 6 * P + (size_t)rk.x;
    const uint8_t *op = ops + e.ops + (size_t)(e.cap - K);
    const char *bs = bases + map.row1(read, TbS);
    const unsigned long long below = (1ull << lane) - 1ull;
    int cj = 0, ci = 0;                                          // truth and call bases consumed by the chunks before
    unsigned t_match = 0, t_mis = 0, t_del = 0, t_ins = 0, t_edge = 0;      // this wave's share of the totals (the same in all its lanes)
    for (int k0 = 0, buf = 0; k0 < K; k0 += kPileupNT, buf ^= 1) {
        const int k = k0 + tid;
        const bool live = k < K;
        const int code = live ? (int)op[k] : 4;
        const unsigned long long bt = __ballot(live && code != 2), bc = __ballot(live && code != 3);
        if (lane == 0) { wj[buf][wv] = __popcll(bt); wi[buf][wv] = __popcll(bc); }
        __syncthreads();                                         // (one a chunk: the next chunk writes the other half)
        int j = cj + __popcll(bt & below), i = ci + __popcll(bc & below);
#pragma unroll
        for (int w = 0; w < kPileupNW; w++) {
            const int tj = wj[buf][w], ti = wi[buf][w];
            j += w < wv ? tj : 0; i += w < wv ? ti : 0;
            cj += tj; ci += ti;
        }
        const bool diag = code <= 1, del = code == 3, ins = code == 2;
        const bool inner = ins && j >= 1 && j <= m - 1;
        t_match += __popcll(__ballot(code == 0)); t_mis += __popcll(__ballot(code == 1)); t_del += __popcll(__ballot(del));
        t_ins += __popcll(__ballot(inner)); t_edge += __popcll(__ballot(ins && !inner));
        int col = -1, f = 0;
        if (diag || del) {
            f = o ? Mk - 1 - (ts + j) : ts + j;
            const int c = (diag && i < n) ? (int)seq_code(bs[i]) : 0;      // C and Z: 1, as k_truth reads the call
            col = del ? 4 : (i < n ? (o ? 3 - c : c) : -1);
        } else if (inner) {
            f = o ? Mk - 1 - ts - j : ts + j - 1;
            col = 5;
        }
        if (col >= 0 && f >= 0 && f < Mk) atomicAdd(cnt + (size_t)col * P + (size_t)f, 1u);
    }
    if (lane == 0) { wtot[wv][0] = t_match; wtot[wv][1] = t_mis; wtot[wv][2] = t_del; wtot[wv][3] = t_ins; wtot[wv][4] = t_edge; }
    __syncthreads();
    if (tid < 5) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kPileupNW; w++) v += wtot[w][tid];
        if (v) atomicAdd(pv.totals + PT_MATCH + tid, v);
    } else if (tid == 5) atomicAdd(pv.totals + PT_READS, 1ull);
}

void launch_pileup(hipStream_t s, const MapRefView &ref, const TruthRead *list, int count, const void *map_records, const int *truth_records, const uint8_t *ops,
                   const char *bases, int Tb, ReadMap map, const PileupView &pv) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_pileup, dim3(count), dim3(kPileupNT), 0, s, ref.recs, ref.nrec, list, (const uint4 *)map_records, truth_records, ops, bases, Tb, map, pv);
}

}  // namespace ffhip
