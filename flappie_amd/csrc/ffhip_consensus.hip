// ffhip_consensus.hip -- per reference position, the bases, the deletions and the INSERTED LETTERS the aligned calls put there (FFHIP_RUN_CONSENSUS, include/ffhip.h
// "consensus"): the counters of a consensus object, which every finished batch it is attached to adds to, and the kernel that calls a consensus from them at the
// run's end.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.  The second twin of ffhip_pileup.hip.
//
// k_consensus: one workgroup an entry of truth's read list, launched by ffhip_batch_finish where k_pileup is.  Which read counts, n, m, K, q and the span come from the
// truth and the map record as in k_pileup; the ops go a thread each in chunks of the workgroup's size, j and i from two wave ballots, the waves before through LDS,
// the chunks before in a running carry.  New against k_pileup: strands are merged into forward letters, and an insertion's thread needs its letter's FORWARD offset d
// in its run -- the I ops ahead of it in the run on the + strand, those behind it on the - strand -- and only whether d < 8.  So it reads up to 8 neighbouring op bytes
// in one direction, from the read's own contiguous ops, and stops at the first that is not I or at the ops' end: no thread walks more than 8 ops, and a run that
// straddles a wave, a chunk or the ops' ends needs no case of its own.  A thread then adds 1 to at most one counter; the planes are [plane][position], so the lanes
// of a wave that hit one plane hit consecutive words.  The totals are ballot popcounts kept by every wave, summed through LDS at the end and added with one 64-bit
// atomic each.  256 threads, 144 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
//
// k_consensus_call: one thread a position, once a run: the five counts' winner, then the insertion columns while a majority of the depth has one.  Integers only.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kConsensusNT = 256, kConsensusNW = kConsensusNT / 64;
enum { CT_READS = 0, CT_SKIPPED, CT_BASES, CT_DEL, CT_INS_BASES, CT_LONG_INS, CT_EDGE_INS, CT_RESERVED };
static_assert(CT_RESERVED + 1 == kConsensusTotals && 5 + 4 * kConsensusMinor == kConsensusPlanes, "the planes: A C G T del, then four a minor column");

__global__ void __launch_bounds__(kConsensusNT)
k_consensus(const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec, const int *__restrict__ trec,
            const uint8_t *__restrict__ ops, const char *__restrict__ bases, int TbS, ReadMap map, ConsensusView cv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ int wj[2][kConsensusNW], wi[2][kConsensusNW];
    __shared__ unsigned wtot[kConsensusNW][5];
    const TruthRead e = list[blockIdx.x];
    const int read = e.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int *rc = trec + (size_t)read * kTruthRecInts;
    const uint4 r0 = maprec[(size_t)read * 4], r1 = maprec[(size_t)read * 4 + 1];
    if (rc[0] != 1 || (int)r0.x != 1) return;                   // (every exit up to the loop is the whole workgroup's)
    const int n = rc[1], m = rc[2], K = rc[9];
    const long long nm = rc[4], all = nm + rc[5] + rc[6] + rc[7];
    if (1000ll * nm < (long long)cv.min_identity * all) {
        if (tid == 0) atomicAdd(cv.totals + CT_SKIPPED, 1ull);
        return;
    }
    const int q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
    if (q < 0 || q >= 2 * nrec || K < 0 || K > e.cap || n < 0 || m < 1) return;      // (records that k_map_finish and k_truth do not write: nothing is counted)
    const int2 rk = recs[q >> 1];                                // { off_k, M_k }
    if (ts < 0 || te > rk.y || te - ts != m) return;
    const int o = q & 1, Mk = rk.y;
    const size_t P = cv.P;
    unsigned *cnt = cv.counts + (size_t)rk.x;
    const uint8_t *op = ops + e.ops + (size_t)(e.cap - K);
    const char *bs = bases + map.row1(read, TbS);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int step = o ? 1 : -1;                                 // where the letters forward-AHEAD of an inserted letter stand among the ops
    int cj = 0, ci = 0;                                          // truth and call bases consumed by the chunks before
    unsigned t_base = 0, t_del = 0, t_ins = 0, t_long = 0, t_edge = 0;      // this wave's share of the totals (the same in all its lanes)
    for (int k0 = 0, buf = 0; k0 < K; k0 += kConsensusNT, buf ^= 1) {
        const int k = k0 + tid;
        const bool live = k < K;
        const int code = live ? (int)op[k] : 4;
        const unsigned long long bt = __ballot(live && code != 2), bc = __ballot(live && code != 3);
        if (lane == 0) { wj[buf][wv] = __popcll(bt); wi[buf][wv] = __popcll(bc); }
        __syncthreads();                                         // (one a chunk: the next chunk writes the other half)
        int j = cj + __popcll(bt & below), i = ci + __popcll(bc & below);
#pragma unroll
        for (int w = 0; w < kConsensusNW; w++) {
            const int tj = wj[buf][w], ti = wi[buf][w];
            j += w < wv ? tj : 0; i += w < wv ? ti : 0;
            cj += tj; ci += ti;
        }
        const bool diag = code <= 1, del = code == 3, ins = code == 2, has = i < n;
        const bool inner = ins && j >= 1 && j <= m - 1;
        int plane = -1, f = 0;
        bool lng = false;
        if (diag || del) {
            f = o ? Mk - 1 - (ts + j) : ts + j;
            if (del) plane = 4;
            else if (has) { const int c = (int)seq_code(bs[i]); plane = o ? 3 - c : c; }      // C and Z: 1, as k_truth reads the call
        } else if (inner && has) {
            f = o ? Mk - 1 - ts - j : ts + j - 1;
            int d = 0;                                           // the run's letters forward-ahead of this one: at most 8 op bytes read, all inside [0, K)
            for (int t = 1; t <= kConsensusMinor; t++) {
                const int kk = k + t * step;
                if (kk < 0 || kk >= K || op[kk] != 2) break;
                d++;
            }
            lng = d >= kConsensusMinor;
            if (!lng) { const int c = (int)seq_code(bs[i]); plane = 5 + 4 * d + (o ? 3 - c : c); }
        }
        const bool put = plane >= 0 && f >= 0 && f < Mk;
        if (put) atomicAdd(cnt + (size_t)plane * P + (size_t)f, 1u);
        t_base += __popcll(__ballot(put && plane < 4)); t_del += __popcll(__ballot(put && plane == 4)); t_ins += __popcll(__ballot(put && plane > 4));
        t_long += __popcll(__ballot(lng)); t_edge += __popcll(__ballot(ins && !inner));
    }
    if (lane == 0) { wtot[wv][0] = t_base; wtot[wv][1] = t_del; wtot[wv][2] = t_ins; wtot[wv][3] = t_long; wtot[wv][4] = t_edge; }
    __syncthreads();
    if (tid < 5) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kConsensusNW; w++) v += wtot[w][tid];
        if (v) atomicAdd(cv.totals + CT_BASES + tid, v);
    } else if (tid == 5) atomicAdd(cv.totals + CT_READS, 1ull);
}

// the call: a thread a position.  The cell is built in registers and leaves as one 16-byte store.
__global__ void __launch_bounds__(256)
k_consensus_call(const unsigned *__restrict__ words, const unsigned *__restrict__ counts, size_t P, unsigned min_depth, uint4 *__restrict__ cells) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const size_t gw = (size_t)kMapPad + g;
    const int rf = (int)((words[gw >> 4] >> (2 * (int)(gw & 15))) & 3u);
    unsigned c[5];
    unsigned long long depth = 0;
#pragma unroll
    for (int x = 0; x < 5; x++) { c[x] = counts[(size_t)x * P + g]; depth += c[x]; }
    unsigned long long s = 0;                                    // the ten letters, s[0] in the low byte, then s[8] and s[9]
    unsigned s_hi = 0, nl = 0, what = kConsensusLow;
    auto put = [&](unsigned ch) { if (nl < 8) s |= (unsigned long long)ch << (8 * nl); else s_hi |= ch << (8 * (nl - 8)); nl++; };
    constexpr unsigned kLower = 0x74676361u, kUpper = 0x54474341u;      // "acgt" and "ACGT", a letter a byte: no table, no indexed array (no scratch)
    if (depth < (unsigned long long)min_depth) put((kLower >> (8 * rf)) & 255u);
    else {
        int win = 0;
        unsigned cw = c[0], cr = c[0];
#pragma unroll
        for (int x = 1; x < 5; x++) {                            // the first of the largest in the order A C G T del ...
            if (c[x] > cw) { cw = c[x]; win = x; }
            if (x == rf) cr = c[x];
        }
        if (cr == cw) win = rf;                                  // ... unless the reference's letter is among them
        what = win == 4 ? kConsensusDel : win == rf ? kConsensusSame : kConsensusSub;
        if (win < 4) put((kUpper >> (8 * win)) & 255u);
        for (int d = 0; d < kConsensusMinor; d++) {
            unsigned long long t = 0;
            unsigned vb = 0;
            int b = 0;
#pragma unroll
            for (int x = 0; x < 4; x++) {                        // the column's total and the first of its largest in the order A C G T
                const unsigned v = counts[(size_t)(5 + 4 * d + x) * P + g];
                t += v;
                if (v > vb) { vb = v; b = x; }
            }
            if (!(2ull * t > depth)) break;
            put((kUpper >> (8 * b)) & 255u);
            what |= kConsensusIns;
        }
    }
    const unsigned w0 = nl | (what << 8) | ((unsigned)(s & 0xffffull) << 16);
    cells[g] = make_uint4(w0, (unsigned)(s >> 16), (unsigned)(s >> 48) | (s_hi << 16), depth > 0xffffffffull ? 0xffffffffu : (unsigned)depth);
}

void launch_consensus(hipStream_t s, const MapRefView &ref, const TruthRead *list, int count, const void *map_records, const int *truth_records, const uint8_t *ops,
                      const char *bases, int Tb, ReadMap map, const ConsensusView &cv) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_consensus, dim3(count), dim3(kConsensusNT), 0, s, ref.recs, ref.nrec, list, (const uint4 *)map_records, truth_records, ops, bases, Tb, map, cv);
}

void launch_consensus_call(hipStream_t s, const MapRefView &ref, const ConsensusView &cv, unsigned min_depth, void *cells) {
    if (cv.P == 0) return;
    hipLaunchKernelGGL(k_consensus_call, dim3((unsigned)((cv.P + 255) / 256)), dim3(256), 0, s, ref.words, cv.counts, cv.P, min_depth, (uint4 *)cells);
}

}  // namespace ffhip
