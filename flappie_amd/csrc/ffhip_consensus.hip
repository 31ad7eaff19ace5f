// ffhip_consensus.hip -- per reference position, the bases, the deletions and the INSERTED LETTERS the aligned calls put there (FFHIP_RUN_CONSENSUS, include/ffhip.h
// "consensus"): the counters of a consensus object, which every finished batch it is attached to adds to, and the kernel that calls a consensus from them at the
// run's end.  Integer adds only, so the counters are the same bytes whatever the batch size, packing, pairing or read order.
//
// k_consensus: one workgroup an entry of truth's read list, launched by ffhip_batch_finish where k_pileup is.  Which read counts, where its ops lie and an op's j and i
// come from the gate and the scan that the accumulators share (ffhip_pile.hpp).  What is this file's: strands are merged into forward letters, and an insertion's
// thread needs its letter's FORWARD offset d in its run -- the I ops ahead of it in the run on the + strand, those behind it on the - strand -- and only whether
// d < 8.  So it reads up to 8 neighbouring op bytes in one direction, from the read's own contiguous ops, and stops at the first that is not I or at the ops' end: no
// thread walks more than 8 ops, and a run that straddles a wave, a chunk or the ops' ends needs no case of its own.  A thread then adds 1 to at most one counter; the
// planes are [plane][position], so the lanes of a wave that hit one plane hit consecutive words.  The totals are ballot popcounts kept by every wave.
// 256 threads, 144 bytes of LDS, no scratch: it runs beside the next pair's layer launch as the decode does.
//
// k_consensus_call: one thread a position, once a run: the five counts' winner, then the insertion columns while a majority of the depth has one.  Integers only.
#include "ffhip_pile.hpp"

namespace ffhip {

enum { CT_READS = 0, CT_SKIPPED, CT_BASES, CT_DEL, CT_INS_BASES, CT_LONG_INS, CT_EDGE_INS, CT_RESERVED };
constexpr int kConsensusWaveTotals = CT_RESERVED - CT_BASES; // the totals a wave keeps: bases .. edge_ins
static_assert(CT_RESERVED + 1 == kConsensusTotals && 5 + 4 * kConsensusMinor == kConsensusPlanes, "the planes: A C G T del, then four a minor column");

__global__ void __launch_bounds__(kPileNT)
k_consensus(const int2 *__restrict__ recs, int nrec, const TruthRead *__restrict__ list, const uint4 *__restrict__ maprec, const int *__restrict__ trec,
            const uint8_t *__restrict__ ops, const char *__restrict__ bases, int TbS, ReadMap map, ConsensusView cv) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ PileLds lds;
    __shared__ unsigned wtot[kPileNW][kConsensusWaveTotals];
    PileRead r;
    const int gate = pile_gate(list[blockIdx.x], true, recs, nrec, maprec, trec, ops, TbS, map, cv.min_identity, r);      // (the whole workgroup's, ahead of the first barrier)
    if (gate == PILE_SKIPPED && threadIdx.x == 0) atomicAdd(cv.totals + CT_SKIPPED, 1ull);
    if (gate != PILE_COUNTED) return;
    const int n = r.n, m = r.m, K = r.K, o = r.o, Mk = r.Mk, ts = r.ts;
    const size_t P = cv.P;
    unsigned *cnt = cv.counts + (size_t)r.off_k;
    const uint8_t *op = r.op;
    const char *bs = bases + r.row;
    const int step = o ? 1 : -1;                                 // where the letters forward-AHEAD of an inserted letter stand among the ops
    unsigned tw[kConsensusWaveTotals] = { 0, 0, 0, 0, 0 };        // this wave's share of the totals (the same in all its lanes)
    PileScan scan;
    for (int k0 = 0; k0 < K; k0 += kPileNT) {
        const PileStep x = scan.step(lds, op, K, k0);
        const int code = x.code, k = x.k, j = x.j, i = x.i;
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
        tw[CT_BASES - CT_BASES] += __popcll(__ballot(put && plane < 4)); tw[CT_DEL - CT_BASES] += __popcll(__ballot(put && plane == 4));
        tw[CT_INS_BASES - CT_BASES] += __popcll(__ballot(put && plane > 4)); tw[CT_LONG_INS - CT_BASES] += __popcll(__ballot(lng));
        tw[CT_EDGE_INS - CT_BASES] += __popcll(__ballot(ins && !inner));
    }
    pile_totals(wtot, tw, cv.totals + CT_BASES, cv.totals + CT_READS, 1u);
}

// the call: a thread a position.  The cell is built in registers and leaves as one 16-byte store.
__global__ void __launch_bounds__(256)
k_consensus_call(const unsigned *__restrict__ words, const unsigned *__restrict__ counts, size_t P, unsigned min_depth, uint4 *__restrict__ cells) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= P) return;
    const int rf = (int)ref_letter(words, g);
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

void launch_consensus(hipStream_t s, const MapRefView &ref, const PileArgs &a, const ConsensusView &cv) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(k_consensus, dim3(a.count), dim3(kPileNT), 0, s, ref.recs, ref.nrec, a.list, (const uint4 *)a.map_records, a.truth_records, a.ops, a.bases, a.Tb, a.map, cv);
}

void launch_consensus_call(hipStream_t s, const MapRefView &ref, const ConsensusView &cv, unsigned min_depth, void *cells) {
    if (cv.P == 0) return;
    hipLaunchKernelGGL(k_consensus_call, dim3((unsigned)((cv.P + 255) / 256)), dim3(256), 0, s, ref.words, cv.counts, cv.P, min_depth, (uint4 *)cells);
}

}  // namespace ffhip
