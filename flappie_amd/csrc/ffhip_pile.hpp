// ffhip_pile.hpp -- what the run-wide accumulators' kernels share, each written once: k_pileup, k_modpileup, k_consensus and k_errprofile (ffhip_pileup, _modpileup,
// _consensus and _errprofile.hip).  Each of them takes entries of truth's read list behind everything that may still patch a read's records (the f32 re-runs), asks
// the GATE whether the read is counted, walks its ops with the SCAN, classes every op into a counter of its own -- the one part that differs, and all that stands in
// its file -- and leaves its totals through the EXIT.  Integer adds only.  Device code.
//
// The gate.  The truth RECORD says whether the read is counted (status, the four counts for the identity test) and gives n, m and K; the map record gives q and the
// span; the list entry gives only where the ops lie (K bytes right-aligned in its cap bytes) and, for a set truth, how many codes the truths hold for the read.
// The identity test stands ahead of the tests of q, K and the span.  For `skipped` that order is immaterial: a record of status 1 beside a map record of status 1
// passes those tests always.  k_truth writes status 1 with the m of its list entry, which k_map_stretch patched to tend - tstart of the very map record -- status 1,
// q and the span inside its reference record, or the entry is refused and k_truth writes status 2 -- and with a K of at most n + m <= cap; the f32 re-run replaces
// a read's map record and truth record together, from one side run that made them the same way; and the single-alignment operators (ffhip_features.hip pile_op)
// build both records from one span that span_check has held to the reference.  So the tests behind the identity test only keep a kernel inside its buffers when
// it is handed records that no kernel of the library wrote.
//
// The scan.  The ops go a thread each in chunks of the workgroup's size: an op's place on the reference and in the call follows from j and i, the truth and call
// bases consumed before it -- the popcount of the lanes below in two wave ballots (op != I, op != D), the waves before through LDS, the chunks before in a running
// carry.  No thread walks ops.  One barrier a chunk: the next chunk writes the other half of the LDS words, and the half in turn runs on from read to read.
#pragma once
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kPileNT = 256, kPileNW = kPileNT / 64;

// ---- the gate
enum { PILE_NOT_COUNTED = 0, PILE_SKIPPED, PILE_COUNTED };
struct PileRead {
    int read, n, m, K;                  // the read's index in the batch; call bases, truth bases, ops
    int o, Mk, off_k, ts;               // mapped: the strand, the reference record's letters and first letter, the span's start on strand o (else 0)
    const uint8_t *op;                  // the K ops
    size_t row;                         // where the read's letters (qualities, 5mC bytes) start in their buffers
};
// mapped: the mode of truth from map (the map record at maprec[read] is read and held against recs); else a set truth of e.m codes, and neither is read.
// Every thread of the workgroup gets the same answer; `r` is filled when it is PILE_COUNTED.
__device__ __forceinline__ int pile_gate(const TruthRead &e, bool mapped, const int2 *__restrict__ recs, int nrec, const uint4 *__restrict__ maprec,
                                         const int *__restrict__ trec, const uint8_t *__restrict__ ops, int TbS, const ReadMap &map, int min_identity, PileRead &r) {
    const int read = e.read;
    const int *rc = trec + (size_t)read * kTruthRecInts;
    uint4 r0 = make_uint4(1u, 0u, 0u, 0u), r1 = make_uint4(0u, 0u, 0u, 0u);
    if (mapped) { r0 = maprec[(size_t)read * 4]; r1 = maprec[(size_t)read * 4 + 1]; }
    if (rc[0] != 1 || (int)r0.x != 1) return PILE_NOT_COUNTED;
    const int n = rc[1], m = rc[2], K = rc[9];
    const long long nm = rc[4], all = nm + rc[5] + rc[6] + rc[7];
    if (1000ll * nm < (long long)min_identity * all) return PILE_SKIPPED;
    if (K < 0 || K > e.cap || K > 2 * kTruthMaxLen || n < 0 || m < 1) return PILE_NOT_COUNTED;      // (records that k_map_finish and k_truth do not write: nothing is counted)
    r.o = r.Mk = r.off_k = r.ts = 0;
    if (mapped) {
        const int q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
        if (q < 0 || q >= 2 * nrec) return PILE_NOT_COUNTED;
        const int2 rk = recs[q >> 1];                            // { off_k, M_k }
        if (ts < 0 || te > rk.y || te - ts != m) return PILE_NOT_COUNTED;
        r.o = q & 1; r.Mk = rk.y; r.off_k = rk.x; r.ts = ts;
    } else if (m > e.m) return PILE_NOT_COUNTED;                 // (the truths hold e.m codes for this read)
    r.read = read; r.n = n; r.m = m; r.K = K;
    r.op = ops + e.ops + (size_t)(e.cap - K);
    r.row = map.row1(read, TbS);
    return PILE_COUNTED;
}

// ---- the scan
struct alignas(16) PileLds { int wj[2][kPileNW], wi[2][kPileNW]; };      // a kernel's __shared__ words of it (a chunk's four of either: one 16-byte read)
struct PileStep { bool live; int code, k, j, i; };                // the thread's op of a chunk: is there one, its code (none: 4), its index, the truth and call bases before it
struct PileScan {
    int buf = 0, cj = 0, ci = 0;                                 // the half of the LDS words in turn; truth and call bases consumed by the read's chunks before
    __device__ __forceinline__ void begin() { cj = ci = 0; }      // a new read
    // the chunk of the ops [k0, k0 + kPileNT): every thread of the workgroup calls it together
    __device__ __forceinline__ PileStep step(PileLds &s, const uint8_t *__restrict__ op, int K, int k0) {
        const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
        const unsigned long long below = (1ull << lane) - 1ull;
        PileStep x;
        x.k = k0 + tid;
        x.live = x.k < K;
        x.code = x.live ? (int)op[x.k] : 4;
        const unsigned long long bt = __ballot(x.live && x.code != 2), bc = __ballot(x.live && x.code != 3);
        if (lane == 0) { s.wj[buf][wv] = __popcll(bt); s.wi[buf][wv] = __popcll(bc); }
        __syncthreads();                                         // (one a chunk: the next chunk writes the other half)
        x.j = cj + __popcll(bt & below); x.i = ci + __popcll(bc & below);
#pragma unroll
        for (int w = 0; w < kPileNW; w++) {
            const int tj = s.wj[buf][w], ti = s.wi[buf][w];
            x.j += w < wv ? tj : 0; x.i += w < wv ? ti : 0;
            cj += tj; ci += ti;
        }
        buf ^= 1;
        return x;
    }
};

// ---- the totals' exit: tw are a wave's ballot popcounts (the same in all its lanes).  Every thread of the workgroup calls it together: the waves' counts are summed
// through LDS and added to base[0 .. N) with one 64-bit atomic each that is not zero, and the next thread adds the workgroup's reads.
template <int N>
__device__ __forceinline__ void pile_totals(unsigned (&wtot)[kPileNW][N], const unsigned (&tw)[N], unsigned long long *base, unsigned long long *reads, unsigned n_reads) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
#pragma unroll
        for (int x = 0; x < N; x++) wtot[tid >> 6][x] = tw[x];
    }
    __syncthreads();                                             // every add of the workgroup into LDS is done, wtot is written
    if (tid < N) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kPileNW; w++) v += wtot[w][tid];
        if (v) atomicAdd(base + tid, v);
    } else if (tid == N) { if (n_reads) atomicAdd(reads, (unsigned long long)n_reads); }
}

}  // namespace ffhip
