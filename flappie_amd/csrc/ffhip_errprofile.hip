// ffhip_errprofile.hip -- the run's error profile (FFHIP_RUN_ERRPROFILE, include/ffhip.h "error profile"): which truth base is called as which, whether the qualities
// mean what they say, which 5-mers go wrong and how homopolymers come out -- the counters of an error profile object, which every finished batch it is attached to
// adds to.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.  The accumulator that is aggregated by
// class instead of by position, and so the one that serves a set truth as well as truth from map.
//
// k_errprofile: launched by ffhip_batch_finish where k_pileup is.  Which read counts, where its ops lie and an op's j and i come from the gate and the scan that the
// accumulators share (ffhip_pile.hpp), the gate in either truth mode.  What is this file's:
//   The tables live in LDS as uint32 histograms (kErrTableWords words, 26 KB), which the threads add to with LDS atomics.  A workgroup takes the list's entries
//   blockIdx.x, blockIdx.x + gridDim.x, ...: the histogram is zeroed once and flushed once, one 64-bit global atomic a NON-ZERO word -- and early whenever the ops
//   counted since the last flush would pass 2^31, so no word of it can wrap.  The totals are ballot popcounts kept by every wave and leave with the flush.
//   A truth letter comes from truth_letter(): the truths on the device for a set truth, the map record's span of the reference's 2-bit words in the mode of truth from
//   map -- NOT the stretch k_map_stretch wrote, which a re-run on the f32 path whose map record moved leaves stale.  Everything else is shared by the two modes.
//   Bounded walks: a ctx thread reads 5 truth letters.  The thread of the op that consumes a homopolymer run's first base reads its letter, the one before and at most
//   16 behind it, and then at most 64 op bytes of the run in the read's own contiguous ops -- back over the insertions ahead of the run, forward to the op of its
//   last base and over the insertions behind -- beside the byte that ends either block of insertions, and stops where the 65th would be needed.  No other thread
//   walks, and a run or a gap that straddles a wave, a chunk or the ops' ends needs no case of its own.
// 256 threads, 26272 bytes of LDS, no scratch.
#include "ffhip_pile.hpp"

namespace ffhip {

enum { ET_READS = 0, ET_SKIPPED, ET_MATCH, ET_MISMATCH, ET_DEL, ET_INS, ET_EDGE_INS, ET_CTX_SITES, ET_HP_RUNS, ET_HP_LONG, ET_HP_WIDE, ET_RESERVED };
constexpr int kErrWaveTotals = ET_RESERVED - ET_MATCH;       // the totals a wave keeps: match .. hp_wide
constexpr unsigned kErrFlushOps = 0x80000000u;               // a word of the LDS histogram takes at most one add an op
static_assert(ET_RESERVED + 1 == kErrTotals && kErrAtSub + 20 == kErrAtIns && kErrAtIns + 4 == kErrAtQual && kErrAtQual + 94 * 3 == kErrAtCtx &&
              kErrAtCtx + 1024 * 4 == kErrAtHp && kErrAtHp + 4 * kErrHpMaxRun * (kErrHpMaxCalled + 1) == kErrTableWords, "the sections stand one behind the other");

// where a read's truth letters come from: `seq` (codes 0 .. 4, 4 read as 1) or, when `words` is given, the letter dir * j from g of the reference's 2-bit words,
// complemented on the - strand
struct ErrTruth { const uint8_t *seq; const unsigned *words; long long g; int dir; };
__device__ __forceinline__ int truth_letter(const ErrTruth &t, int j) {
    if (t.words) {
        const int v = (int)ref_letter(t.words, (size_t)(t.g + (long long)t.dir * j));
        return t.dir < 0 ? 3 - v : v;
    }
    const int c = (int)t.seq[j];
    return c == 4 ? 1 : c & 3;
}

__global__ void __launch_bounds__(kPileNT)
k_errprofile(const unsigned *__restrict__ words, const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, int count, const uint4 *__restrict__ maprec,
             const int *__restrict__ trec, const uint8_t *__restrict__ ops, const char *__restrict__ bases, const char *__restrict__ quals,
             const uint8_t *__restrict__ seq, int TbS, ReadMap map, ErrProfileView ev) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ unsigned hist[kErrTableWords];
    __shared__ PileLds lds;
    __shared__ unsigned wtot[kPileNW][kErrWaveTotals];
    const int tid = threadIdx.x;
    const bool mapped = words != nullptr;
    for (int w = tid; w < kErrTableWords; w += kPileNT) hist[w] = 0u;      // (seen by all behind the first chunk's barrier, which stands ahead of its adds)
    unsigned tw[kErrWaveTotals];                                 // this wave's share of the totals since the last flush (the same in all its lanes)
#pragma unroll
    for (int x = 0; x < kErrWaveTotals; x++) tw[x] = 0u;
    unsigned n_reads = 0, n_skipped = 0, since = 0;              // the workgroup's reads, and the ops it has counted since the last flush (the same in all its threads)
    unsigned long long *totals = ev.counts + kErrTableWords;
    PileScan scan;                                               // (its half of the LDS words in turn runs on from read to read)
    // the flush: every thread calls it together.  One 64-bit atomic a non-zero word, and the word is zero again.
    auto flush = [&]() {
        pile_totals(wtot, tw, totals + ET_MATCH, totals + ET_READS, n_reads);      // (its barrier: every add into hist is done)
        if (tid == kErrWaveTotals + 1 && n_skipped) atomicAdd(totals + ET_SKIPPED, (unsigned long long)n_skipped);
        for (int w = tid; w < kErrTableWords; w += kPileNT)
            if (const unsigned v = hist[w]) { atomicAdd(ev.counts + w, (unsigned long long)v); hist[w] = 0u; }
#pragma unroll
        for (int x = 0; x < kErrWaveTotals; x++) tw[x] = 0u;
        n_reads = n_skipped = since = 0;
        __syncthreads();                                         // hist and wtot are free again
    };
    for (int ent = blockIdx.x; ent < count; ent += gridDim.x) {  // (every `continue` up to the chunks is the whole workgroup's)
        PileRead r;
        const int gate = pile_gate(list[ent], mapped, recs, nrec, maprec, trec, ops, TbS, map, ev.min_identity, r);
        if (gate == PILE_SKIPPED) n_skipped++;
        if (gate != PILE_COUNTED) continue;
        const int n = r.n, m = r.m, K = r.K;
        ErrTruth tr{ seq + list[ent].seq, nullptr, 0ll, 1 };
        if (mapped) {
            tr.words = words; tr.dir = r.o ? -1 : 1;
            tr.g = r.o ? (long long)r.off_k + r.Mk - 1 - r.ts : (long long)r.off_k + r.ts;      // the reference letter of y_q[tstart], as k_map_stretch
        }
        if (since + (unsigned)K > kErrFlushOps) flush();
        since += (unsigned)K;
        n_reads++;
        const uint8_t *op = r.op;
        const char *bs = bases + r.row, *qs = quals + r.row;
        scan.begin();
        for (int k0 = 0; k0 < K; k0 += kPileNT) {
            const PileStep x = scan.step(lds, op, K, k0);
            const int code = x.code, k = x.k, j = x.j, i = x.i;
            const bool has = i < n;
            const bool diag = code <= 1 && has && j < m, del = code == 3 && j < m, ins = code == 2 && has;
            const bool inner = ins && j >= 1 && j <= m - 1;
            bool site = false, run = false, lng = false, wide = false;
            if (diag || del) {
                const int t0 = truth_letter(tr, j);
                const int sc = diag ? (int)seq_code(bs[i]) : 4;  // C and Z: 1, as k_truth reads the call
                atomicAdd(&hist[kErrAtSub + 5 * t0 + sc], 1u);
                if (diag) {
                    const int qv = (int)(unsigned char)qs[i] - 33;
                    atomicAdd(&hist[kErrAtQual + 3 * (qv < 0 ? 0 : qv > 93 ? 93 : qv) + code], 1u);
                }
                int before = -1;                                 // t_(j - 1)
                if (j >= 2 && j <= m - 3) {
                    const int a2 = truth_letter(tr, j - 2);
                    before = truth_letter(tr, j - 1);
                    const int w = (((a2 * 4 + before) * 4 + t0) * 4 + truth_letter(tr, j + 1)) * 4 + truth_letter(tr, j + 2);
                    atomicAdd(&hist[kErrAtCtx + 4 * w + (del ? 2 : code)], 1u);
                    site = true;
                } else if (j >= 1) before = truth_letter(tr, j - 1);
                // the homopolymer run that starts here: interior runs only, so one at j = 0 is none
                if (j >= 1 && before != t0) {
                    int r = 1;
                    while (r <= kErrHpMaxRun && j + r < m && truth_letter(tr, j + r) == t0) r++;
                    if (j + r <= m - 1) {                        // (a run that reaches the truth's last base has an unknown length; r = 17: the 17th letter is not the last)
                        if (r > kErrHpMaxRun) lng = true;
                        else {
                            int nop = 1, c = code == 0 ? 1 : 0;
                            for (int kk = k - 1, ii = i - 1; kk >= 0 && op[kk] == 2; kk--, ii--) {      // F: the insertions that end ahead of the run's first op
                                if (++nop > kErrHpMaxOps) break;
                                c += (ii >= 0 && ii < n && (int)seq_code(bs[ii]) == t0) ? 1 : 0;
                            }
                            int kk = k + 1, ii = i + (code == 3 ? 0 : 1), left = r - 1;
                            for (; nop <= kErrHpMaxOps && kk < K && (left > 0 || op[kk] == 2); kk++) {   // to the op of the run's last base, then B behind it
                                const int o2 = (int)op[kk];
                                if (++nop > kErrHpMaxOps) break;
                                if (o2 == 2) { c += (ii < n && (int)seq_code(bs[ii]) == t0) ? 1 : 0; ii++; }
                                else { left--; c += o2 == 0 ? 1 : 0; ii += o2 == 3 ? 0 : 1; }
                            }
                            wide = nop > kErrHpMaxOps;
                            if (!wide) {
                                run = true;
                                atomicAdd(&hist[kErrAtHp + (t0 * kErrHpMaxRun + (r - 1)) * (kErrHpMaxCalled + 1) + (c > kErrHpMaxCalled ? kErrHpMaxCalled : c)], 1u);
                            }
                        }
                    }
                }
            } else if (inner) {
                atomicAdd(&hist[kErrAtIns + (int)seq_code(bs[i])], 1u);
                const int qv = (int)(unsigned char)qs[i] - 33;
                atomicAdd(&hist[kErrAtQual + 3 * (qv < 0 ? 0 : qv > 93 ? 93 : qv) + 2], 1u);
                if (j >= 3 && j <= m - 2) {                      // the gap belongs to the centre j - 1
                    int w = 0;
#pragma unroll
                    for (int d = -3; d <= 1; d++) w = w * 4 + truth_letter(tr, j + d);
                    atomicAdd(&hist[kErrAtCtx + 4 * w + 3], 1u);
                    site = true;
                }
            }
            tw[ET_MATCH - ET_MATCH] += __popcll(__ballot(diag && code == 0)); tw[ET_MISMATCH - ET_MATCH] += __popcll(__ballot(diag && code == 1));
            tw[ET_DEL - ET_MATCH] += __popcll(__ballot(del)); tw[ET_INS - ET_MATCH] += __popcll(__ballot(inner));
            tw[ET_EDGE_INS - ET_MATCH] += __popcll(__ballot(code == 2 && !inner)); tw[ET_CTX_SITES - ET_MATCH] += __popcll(__ballot(site));
            tw[ET_HP_RUNS - ET_MATCH] += __popcll(__ballot(run)); tw[ET_HP_LONG - ET_MATCH] += __popcll(__ballot(lng)); tw[ET_HP_WIDE - ET_MATCH] += __popcll(__ballot(wide));
        }
    }
    flush();
}

void launch_errprofile(hipStream_t s, const MapRefView *ref, const PileArgs &a, int groups, const char *quals, const uint8_t *seq, const ErrProfileView &ev) {
    if (a.count <= 0) return;
    const int grid = groups < 1 ? 1 : groups < a.count ? groups : a.count;
    hipLaunchKernelGGL(k_errprofile, dim3(grid), dim3(kPileNT), 0, s, ref ? ref->words : nullptr, ref ? ref->recs : nullptr, ref ? ref->nrec : 0, a.list, a.count,
                       (const uint4 *)a.map_records, a.truth_records, a.ops, a.bases, quals, seq, a.Tb, a.map, ev);
}

}  // namespace ffhip
