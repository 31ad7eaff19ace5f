// ffhip_modpileup.hip -- per reference C (on the - strand: G), how methylated the aligned calls say it is (FFHIP_RUN_MOD_PILEUP, include/ffhip.h "mod pileup"): the
// counters of a mod pileup object, which every finished batch it is attached to adds to.  Integer adds only, so the counters are the same bytes whatever the batch
// size, packing, pairing or read order.
//
// k_modpileup: one workgroup an entry of truth's read list, launched by ffhip_batch_finish behind everything that may still patch the read's records, letters and 5mC
// bytes.  Which read counts, where its ops lie and an op's j and i come from the gate and the scan that the accumulators share (ffhip_pile.hpp).  What is this
// file's: the reference's letter at the op's position, one load from the 2-bit words the map searches, and only a lane ON A SITE goes on -- to one load of the
// call's letter, one of its 5mC byte, one LDS add into the workgroup's histogram and one no-return add into a plane.  The planes are [strand][column][position]: the
// lanes of a wave that hit one plane hit ascending words.  The totals are ballot popcounts kept by every wave; the histogram's 256 bins leave beside them, a thread
// a bin with one 64-bit atomic, a bin that stayed 0 adds nothing.
// 256 threads, 1184 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
#include "ffhip_pile.hpp"

namespace ffhip {

enum { MT_READS = 0, MT_SKIPPED, MT_SITES, MT_MOD, MT_CANON, MT_FAIL, MT_DIFF, MT_DEL };
static_assert(MT_DEL + 1 == kModPileupTotals && MT_MOD + kModPileupColumns == kModPileupTotals, "a column's total stands at MT_MOD + column");

__global__ void __launch_bounds__(kPileNT)
k_modpileup(const unsigned *__restrict__ words, const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec,
            const int *__restrict__ trec, const uint8_t *__restrict__ ops, const char *__restrict__ bases, const uint8_t *__restrict__ ml, int TbS, ReadMap map,
            ModPileupView pv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ PileLds lds;
    __shared__ unsigned wtot[kPileNW][1 + kModPileupColumns];
    __shared__ unsigned hist[256];
    static_assert(kPileNT == 256, "a thread a bin of the histogram");
    PileRead r;
    const int gate = pile_gate(list[blockIdx.x], true, recs, nrec, maprec, trec, ops, TbS, map, pv.min_identity, r);      // (the whole workgroup's, ahead of the first barrier)
    if (gate == PILE_SKIPPED && threadIdx.x == 0) atomicAdd(pv.totals + MT_SKIPPED, 1ull);
    if (gate != PILE_COUNTED) return;
    const int tid = threadIdx.x, n = r.n, o = r.o, Mk = r.Mk, ts = r.ts;
    const unsigned site_code = o ? 2u : 1u;                      // the forward letter of a site: C on the + strand, G on the - strand
    const size_t P = pv.P;
    unsigned *cnt = pv.counts + (size_t)o * kModPileupColumns * P + (size_t)r.off_k;
    const char *bs = bases + r.row;
    const uint8_t *mb = ml + r.row;
    hist[tid] = 0u;                                              // (seen by all behind the first chunk's barrier, which stands ahead of its adds)
    unsigned tw[1 + kModPileupColumns] = { 0, 0, 0, 0, 0, 0 };    // this wave's share of the totals, sites and then a column each (the same in all its lanes)
    PileScan scan;
    for (int k0 = 0; k0 < r.K; k0 += kPileNT) {
        const PileStep x = scan.step(lds, r.op, r.K, k0);
        const int i = x.i;
        const bool diag = x.code <= 1, del = x.code == 3;
        const int f = o ? Mk - 1 - (ts + x.j) : ts + x.j;
        bool site = false;
        if ((del || (diag && i < n)) && f >= 0 && f < Mk) site = ref_letter(words, (size_t)r.off_k + (size_t)f) == site_code;
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
        tw[0] += __popcll(__ballot(site));
#pragma unroll
        for (int c = 0; c < kModPileupColumns; c++) tw[1 + c] += __popcll(__ballot(col == c));
    }
    pile_totals(wtot, tw, pv.totals + MT_SITES, pv.totals + MT_READS, 1u);
    if (const unsigned v = hist[tid]) atomicAdd(pv.hist + tid, (unsigned long long)v);      // (behind the exit's barrier: every add into hist is done)
}

void launch_modpileup(hipStream_t s, const MapRefView &ref, const PileArgs &a, const uint8_t *ml, const ModPileupView &pv) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(k_modpileup, dim3(a.count), dim3(kPileNT), 0, s, ref.words, ref.recs, ref.nrec, a.list, (const uint4 *)a.map_records, a.truth_records, a.ops, a.bases,
                       ml, a.Tb, a.map, pv);
}

}  // namespace ffhip
