// ffhip_errprofile.hip -- the run's error profile (FFHIP_RUN_ERRPROFILE, include/ffhip.h "error profile"): which truth base is called as which, whether the qualities
// mean what they say, which 5-mers go wrong and how homopolymers come out -- the counters of an error profile object, which every finished batch it is attached to
// adds to.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.  The sibling of ffhip_pileup.hip that is
// aggregated by class instead of by position, and so the one that serves a set truth as well as truth from map.
//
// k_errprofile: launched by ffhip_batch_finish where k_pileup is.  Which read counts, n, m and K come from the truth record (and the map record in the mode of truth
// from map); the ops go a thread each in chunks of the workgroup's size, j and i from two wave ballots, the waves before through LDS, the chunks before in a running
// carry, as in k_pileup.  New against the siblings:
//   The tables live in LDS as uint32 histograms (kErrTableWords words, 26 KB), which the threads add to with LDS atomics.  A workgroup takes the list's entries
//   blockIdx.x, blockIdx.x + gridDim.x, ...: the histogram is zeroed once and flushed once, one 64-bit global atomic a NON-ZERO word -- and early whenever the ops
//   counted since the last flush would pass 2^31, so no word of it can wrap.  The totals are ballot popcounts kept by every wave and leave with the flush.
//   A truth letter comes from truth_letter(): the truths on the device for a set truth, the map record's span of the reference's 2-bit words in the mode of truth from
//   map -- NOT the stretch k_map_stretch wrote, which a re-run on the f32 path whose map record moved leaves stale.  Everything else is shared by the two modes.
//   Bounded walks: a ctx thread reads 5 truth letters.  The thread of the op that consumes a homopolymer run's first base reads its letter, the one before and at most
//   16 behind it, and then at most 64 op bytes of the run in the read's own contiguous ops -- back over the insertions ahead of the run, forward to the op of its
//   last base and over the insertions behind -- beside the byte that ends either block of insertions, and stops where the 65th would be needed.  No other thread
//   walks, and a run or a gap that straddles a wave, a chunk or the ops' ends needs no case of its own.
// 256 threads, no scratch.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kErrNT = 256, kErrNW = kErrNT / 64;
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
        const long long p = t.g + (long long)t.dir * j + kMapPad;
        const int v = (int)((t.words[p >> 4] >> (2 * (int)(p & 15))) & 3u);
        return t.dir < 0 ? 3 - v : v;
    }
    const int c = (int)t.seq[j];
    return c == 4 ? 1 : c & 3;
}

__global__ void __launch_bounds__(kErrNT)
k_errprofile(const unsigned *__restrict__ words, const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, int count, const uint4 *__restrict__ maprec,
             const int *__restrict__ trec, const uint8_t *__restrict__ ops, const char *__restrict__ bases, const char *__restrict__ quals,
             const uint8_t *__restrict__ seq, int TbS, ReadMap map, ErrProfileView ev) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ unsigned hist[kErrTableWords];
    __shared__ int wj[2][kErrNW], wi[2][kErrNW];
    __shared__ unsigned wtot[kErrNW][kErrWaveTotals];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool mapped = words != nullptr;
    for (int w = tid; w < kErrTableWords; w += kErrNT) hist[w] = 0u;      // (seen by all behind the first chunk's barrier, which stands ahead of its adds)
    unsigned tw[kErrWaveTotals];                                 // this wave's share of the totals since the last flush (the same in all its lanes)
#pragma unroll
    for (int x = 0; x < kErrWaveTotals; x++) tw[x] = 0u;
    unsigned n_reads = 0, n_skipped = 0, since = 0;              // the workgroup's reads, and the ops it has counted since the last flush (the same in all its threads)
    int buf = 0;                                                 // (runs on from read to read: a chunk's half of wj, wi is never the one before's)
    // the flush: every thread calls it together.  One 64-bit atomic a non-zero word, and the word is zero again.
    auto flush = [&]() {
        if (lane == 0) {
#pragma unroll
            for (int x = 0; x < kErrWaveTotals; x++) wtot[wv][x] = tw[x];
        }
        __syncthreads();                                         // every add into hist is done, wtot is written
        for (int w = tid; w < kErrTableWords; w += kErrNT)
            if (const unsigned v = hist[w]) { atomicAdd(ev.counts + w, (unsigned long long)v); hist[w] = 0u; }
        if (tid < kErrWaveTotals) {
            unsigned long long v = 0;
#pragma unroll
            for (int w = 0; w < kErrNW; w++) v += wtot[w][tid];
            if (v) atomicAdd(ev.counts + kErrTableWords + ET_MATCH + tid, v);
        } else if (tid == kErrWaveTotals) { if (n_reads) atomicAdd(ev.counts + kErrTableWords + ET_READS, (unsigned long long)n_reads); }
        else if (tid == kErrWaveTotals + 1) { if (n_skipped) atomicAdd(ev.counts + kErrTableWords + ET_SKIPPED, (unsigned long long)n_skipped); }
#pragma unroll
        for (int x = 0; x < kErrWaveTotals; x++) tw[x] = 0u;
        n_reads = n_skipped = since = 0;
        __syncthreads();                                         // hist and wtot are free again
    };
    for (int ent = blockIdx.x; ent < count; ent += gridDim.x) {  // (every `continue` up to the chunks is the whole workgroup's)
        const TruthRead e = list[ent];
        const int read = e.read;
        const int *rc = trec + (size_t)read * kTruthRecInts;
        if (rc[0] != 1) continue;
        uint4 r0 = make_uint4(1u, 0u, 0u, 0u), r1 = make_uint4(0u, 0u, 0u, 0u);
        if (mapped) { r0 = maprec[(size_t)read * 4]; r1 = maprec[(size_t)read * 4 + 1]; }
        if ((int)r0.x != 1) continue;
        const int n = rc[1], m = rc[2], K = rc[9];
        if (mapped && (int)r1.y - (int)r1.x != m) continue;      // (a record k_truth did not align to this span: nothing is counted)
        const long long nm = rc[4], all = nm + rc[5] + rc[6] + rc[7];
        if (1000ll * nm < (long long)ev.min_identity * all) { n_skipped++; continue; }
        if (K < 0 || K > e.cap || K > 2 * kTruthMaxLen || n < 0 || m < 1) continue;      // (records that k_truth does not write: nothing is counted)
        ErrTruth tr{ seq + e.seq, nullptr, 0ll, 1 };
        if (mapped) {
            const int q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
            if (q < 0 || q >= 2 * nrec) continue;
            const int2 rk = recs[q >> 1];                            // { off_k, M_k }
            if (ts < 0 || te > rk.y) continue;
            const int o = q & 1;
            tr.words = words; tr.dir = o ? -1 : 1;
            tr.g = o ? (long long)rk.x + rk.y - 1 - ts : (long long)rk.x + ts;      // the reference letter of y_q[tstart], as k_map_stretch
        } else if (m > e.m) continue;                            // (the truths hold e.m codes for this read)
        if (since + (unsigned)K > kErrFlushOps) flush();
        since += (unsigned)K;
        n_reads++;
        const uint8_t *op = ops + e.ops + (size_t)(e.cap - K);
        const size_t row = map.row1(read, TbS);
        const char *bs = bases + row, *qs = quals + row;
        int cj = 0, ci = 0;                                      // truth and call bases consumed by the chunks before
        for (int k0 = 0; k0 < K; k0 += kErrNT, buf ^= 1) {
            const int k = k0 + tid;
            const bool live = k < K;
            const int code = live ? (int)op[k] : 4;
            const unsigned long long bt = __ballot(live && code != 2), bc = __ballot(live && code != 3);
            if (lane == 0) { wj[buf][wv] = __popcll(bt); wi[buf][wv] = __popcll(bc); }
            __syncthreads();                                     // (one a chunk: the next chunk writes the other half)
            int j = cj + __popcll(bt & below), i = ci + __popcll(bc & below);
#pragma unroll
            for (int w = 0; w < kErrNW; w++) {
                const int tj = wj[buf][w], ti = wi[buf][w];
                j += w < wv ? tj : 0; i += w < wv ? ti : 0;
                cj += tj; ci += ti;
            }
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

void launch_errprofile(hipStream_t s, const MapRefView *ref, const TruthRead *list, int count, int groups, const void *map_records, const int *truth_records,
                       const uint8_t *ops, const char *bases, const char *quals, const uint8_t *seq, int Tb, ReadMap map, const ErrProfileView &ev) {
    if (count <= 0) return;
    const int grid = groups < 1 ? 1 : groups < count ? groups : count;
    hipLaunchKernelGGL(k_errprofile, dim3(grid), dim3(kErrNT), 0, s, ref ? ref->words : nullptr, ref ? ref->recs : nullptr, ref ? ref->nrec : 0, list, count,
                       (const uint4 *)map_records, truth_records, ops, bases, quals, seq, Tb, map, ev);
}

}  // namespace ffhip
