// ffhip_pileup.hip -- per reference position, what the aligned calls say there (FFHIP_RUN_PILEUP, include/ffhip.h "pileup"): the counters of a pileup object, which
// every finished batch it is attached to adds to.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.
//
// k_pileup: one workgroup an entry of truth's read list, launched by ffhip_batch_finish.  Which read counts, where its ops lie and an op's j and i come from the gate
// and the scan that the accumulators share (ffhip_pile.hpp).  What is this file's: a thread adds 1 to at most one counter -- a match, mismatch or deletion to the
// column of the call's letter (or `del`) at the op's reference position, an inner insertion to the column `ins` of the position ahead of it.  The planes are
// [strand][column][position], so the lanes of a wave that hit one plane hit consecutive words.  The totals are ballot popcounts kept by every wave.
// 256 threads, 144 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
#include "ffhip_pile.hpp"

namespace ffhip {

enum { PT_READS = 0, PT_SKIPPED, PT_MATCH, PT_MISMATCH, PT_DEL, PT_INS, PT_EDGE_INS, PT_RESERVED };
constexpr int kPileupWaveTotals = PT_RESERVED - PT_MATCH;    // the totals a wave keeps: match .. edge_ins
static_assert(PT_RESERVED + 1 == kPileupTotals, "the totals of ffhip_pileup_totals");

__global__ void __launch_bounds__(kPileNT)
k_pileup(const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec, const int *__restrict__ trec,
         const uint8_t *__restrict__ ops, const char *__restrict__ bases, int TbS, ReadMap map, PileupView pv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ PileLds lds;
    __shared__ unsigned wtot[kPileNW][kPileupWaveTotals];
    PileRead r;
    const int gate = pile_gate(list[blockIdx.x], true, recs, nrec, maprec, trec, ops, TbS, map, pv.min_identity, r);      // (the whole workgroup's, ahead of the first barrier)
    if (gate == PILE_SKIPPED && threadIdx.x == 0) atomicAdd(pv.totals + PT_SKIPPED, 1ull);
    if (gate != PILE_COUNTED) return;
    const int n = r.n, m = r.m, o = r.o, Mk = r.Mk, ts = r.ts;
    const size_t P = pv.P;
    unsigned *cnt = pv.counts + (size_t)o * 6 * P + (size_t)r.off_k;
    const char *bs = bases + r.row;
    unsigned tw[kPileupWaveTotals] = { 0, 0, 0, 0, 0 };           // this wave's share of the totals (the same in all its lanes)
    PileScan scan;
    for (int k0 = 0; k0 < r.K; k0 += kPileNT) {
        const PileStep x = scan.step(lds, r.op, r.K, k0);
        const int code = x.code, j = x.j, i = x.i;
        const bool diag = code <= 1, del = code == 3, ins = code == 2;
        const bool inner = ins && j >= 1 && j <= m - 1;
        tw[PT_MATCH - PT_MATCH] += __popcll(__ballot(code == 0)); tw[PT_MISMATCH - PT_MATCH] += __popcll(__ballot(code == 1)); tw[PT_DEL - PT_MATCH] += __popcll(__ballot(del));
        tw[PT_INS - PT_MATCH] += __popcll(__ballot(inner)); tw[PT_EDGE_INS - PT_MATCH] += __popcll(__ballot(ins && !inner));
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
    pile_totals(wtot, tw, pv.totals + PT_MATCH, pv.totals + PT_READS, 1u);
}

void launch_pileup(hipStream_t s, const MapRefView &ref, const PileArgs &a, const PileupView &pv) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(k_pileup, dim3(a.count), dim3(kPileNT), 0, s, ref.recs, ref.nrec, a.list, (const uint4 *)a.map_records, a.truth_records, a.ops, a.bases, a.Tb, a.map, pv);
}

}  // namespace ffhip
