// ffhip_adapters.hip -- adapters and primers anywhere in the called reads (FFHIP_RUN_ADAPTERS, include/ffhip.h "adapters"): every occurrence, both orientations, with
// exact start and end.
//
// A kit is up to 32 patterns over ACGT of up to 64 bases; search q = 2 k + o is pattern k as given (o = 0) or its reverse complement (o = 1) on the call in signal
// order, Z read as C.  d_q[j] = D[L][j] of the infix edit distance (D[0][j] = 0, D[i][0] = i, unit costs); column j is a hit end iff d_q[j] <= md_k and it is the
// leftmost minimum of d_q within 64 columns either way; the hit's start is the largest i with ed(p, x[i:j]) = d_q[j].  All of it is integer arithmetic: exact.
//
// k_adapters: one workgroup a read, four waves, ONE SEARCH A LANE.  A lane holds its search's column as vertical differences in one 64-bit word (Myers' recurrence
// in Hyyro's form: myers_step, ffhip_seq.hpp) and the four match masks of its oriented pattern in registers, and follows d at bit L - 1.  A call of 50 000 bases must not be
// one wave's chain, so the text is cut into SEGMENTS of kAdSeg = FFHIP_ADAPTER_SEGMENT columns: segment g owns the hit ends j in (g S, (g + 1) S].  The waves take
// the segments in turn, four a ROUND.  The wave of a segment starts a fresh search (D[i][a] = i) 192 columns before it: d_q[j] <= L and an optimal match spans at
// most L + d <= 128 columns, so the fresh search is exact from column a + 128 on, which leaves 64 exact columns before the segment for the hit rule; it runs on
// 64 columns past the segment for the rule's other side.
//   text: staged a round at a time in LDS as 2-bit codes, 16 a word, zero beyond the call; a wave reads one word for 16 columns (the same address in every lane).
//   d:    the d bytes do NOT go through LDS.  The layer kernels of the NEXT batch are resident while a batch is decoded -- two workgroups of 79 KB of LDS on every
//         CU -- and a kernel that wants more than the 5 KB they leave waits for them to end and holds the next launch up (measured: DESIGN.md section 5).  d moves
//         by -1, 0 or +1 a column, so a lane keeps the last 128 horizontal differences as two bits a column in four 64-bit registers, and beside d of the current
//         column t the value d[t - 64].  Only when that is <= md -- rare -- are the 64 columns before it and the 64 behind it rebuilt from the differences and
//         tested.  A lane has at most one hit in 64 columns (of two, the left must be <= the right and the right < the left).
//   start: for a hit only -- the reversed pattern (the masks bit-reversed) against x[j-1], x[j-2], ... with an anchored start (D[0][c] = c: a carry of +1 into
//         bit 0 of every column), until D[L][c] = d: start = j - c.
//   order: a wave walks the hit columns of a tile in ascending order (a wave minimum of the lanes' lowest hit column) and ranks the lanes of one column by a
//         ballot: its segment's hits leave in (end, q) order into 15 slots of LDS, with the segment's count.  Behind a barrier every thread forms the same prefix
//         over the round's four counts and the read's running total, and 60 threads store the hits that fall into the record's 15 slots: one 16-byte store a hit,
//         one for the header.  No atomics.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kAdWaves = 4, kAdThreads = 64 * kAdWaves;
constexpr int kAdTile = 64;                                      // columns a candidate mask covers
constexpr int kAdWarm = 192;                                     // a fresh search starts this far before its segment: 128 to be exact, 64 for the hit rule
constexpr int kAdText = kAdWaves * kAdSeg + kAdWarm + kAdReach;  // characters staged a round
static_assert(kAdSeg % kAdTile == 0 && kAdWarm % kAdTile == 0 && kAdReach == kAdTile && kAdWarm >= 128 + kAdReach, "whole tiles; exact d 64 columns before a segment");
static_assert(kAdReach == 64, "the differences of 64 columns a word: one word pair behind the tested column, one before it");
static_assert(kAdText % 16 == 0 && kAdapterMaxKit * 2 == 64 && kAdapterMaxLen == 64 && kAdapterMaxHits == 15, "a search a lane, a pattern a word, a record of 16 stores");

// the hit rule at column j with d[j] = v0: (bp, bm) hold the differences d[j - i] - d[j - i - 1] at bit i (the columns before), (ap, am) the differences
// d[j + 64 - i] - d[j + 63 - i] at bit i (the columns behind): strictly below the 64 columns before, not above the 64 behind, within [0, len]
__device__ __forceinline__ bool ad_is_hit(int v0, int j, int len, unsigned long long bp, unsigned long long bm, unsigned long long ap, unsigned long long am) {
    bool ok = true;
    int v = v0;
    for (int i = 0; i < kAdReach && j - 1 - i >= 0; i++) {        // d[j - 1 - i]
        v -= (int)((bp >> i) & 1ull) - (int)((bm >> i) & 1ull);
        if (v <= v0) ok = false;
    }
    v = v0;
    for (int i = kAdReach - 1; i >= 0 && j + kAdReach - i <= len; i--) {      // d[j + 64 - i]
        v += (int)((ap >> i) & 1ull) - (int)((am >> i) & 1ull);
        if (v < v0) ok = false;
    }
    return ok;
}

// start of the hit (j, d): the reversed pattern against x[j - 1], x[j - 2], ... from an anchored start, until D[L][c] = d
__device__ __forceinline__ int ad_start(const unsigned long long peq[4], int L, int j, int d, const unsigned *text, int t0) {
    unsigned long long rp[4], pv = ~0ull, mv = 0ull;
#pragma unroll
    for (int c = 0; c < 4; c++) rp[c] = __brevll(peq[c]) >> (64 - L);
    int score = L, c = 0;
    while (score != d && c < j && c < 2 * kAdapterMaxLen) {
        const int idx = j - 1 - c - t0;
        const unsigned ch = (text[idx >> 4] >> (2 * (idx & 15))) & 3u;
        score += myers_diff(myers_step(pv, mv, myers_eq(rp, ch), 1), L - 1);      // D[0][c] = c: +1 enters at bit 0
        c++;
    }
    return j - c;
}

template <bool SCORES>
__global__ void __launch_bounds__(kAdThreads)
k_adapters(AdapterKit kit, const char *__restrict__ bases, const int *__restrict__ lens, uint4 *__restrict__ rec, int TbS, const int *__restrict__ tbs, ReadMap map,
           int max_dist, uint8_t *__restrict__ d_out) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ unsigned text[kAdText / 16];
    __shared__ uint4 shit[kAdWaves][kAdapterMaxHits];
    __shared__ int scnt[kAdWaves];
    const int read = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint4 *out = rec + (size_t)read * (kAdapterMaxHits + 1);
    const int Tb = tbs ? tbs[read] : TbS;                // this read's blocks (uniform over the workgroup)
    if (Tb <= 0) {                                       // an empty slot: no call, no length to read -- nhit 0, len 0
        if (tid <= kAdapterMaxHits) out[tid] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int len = lens[read] > 0 ? lens[read] : 0;
    const char *bs = bases + map.row1(read, TbS);
    const bool live = lane < 2 * kit.n;
    const int L = live ? kit.len[lane >> 1] : 1;
    const int md = max_dist < 0 ? L / 4 : (max_dist < L - 1 ? max_dist : L - 1);
    unsigned long long peq[4];
#pragma unroll
    for (int c = 0; c < 4; c++) peq[c] = live ? kit.peq[(size_t)lane * 4 + c] : 0ull;
    const int topb = L - 1;
    uint8_t *drow = (SCORES && d_out && live) ? d_out + (size_t)lane * ((size_t)len + 1) : nullptr;      // the whole score rows (ffhip_op_adapter_scores)
    if (drow && wave == 0) drow[0] = (uint8_t)L;         // D[L][0] = L (never a hit: md < L)
    const int nseg = (len + kAdSeg - 1) / kAdSeg, nround = (nseg + kAdWaves - 1) / kAdWaves;
    int total = 0;                                       // the read's hits so far: the same in every thread
    for (int r = 0; r < nround; r++) {
        const int t0 = r * kAdWaves * kAdSeg - kAdWarm;  // the first staged character (negative in round 0: zero there, and never read)
        for (int w = tid; w < kAdText / 16; w += kAdThreads) {
            unsigned v = 0u;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int i = t0 + 16 * w + e;
                if (i >= 0 && i < len) v |= seq_code(bs[i]) << (2 * e);
            }
            text[w] = v;
        }
        __syncthreads();
        const int a = (r * kAdWaves + wave) * kAdSeg;    // this wave's segment: characters a .. a + S - 1, hit ends a + 1 .. a + S
        int cnt = 0;                                     // its hits
        if (a < len) {
            unsigned long long pv = ~0ull, mv = 0ull;
            unsigned long long hp0 = 0ull, hm0 = 0ull, hp1 = 0ull, hm1 = 0ull;      // the differences of the last 64 columns (bit 0: the newest), and of the 64 before them
            int score = L, lag = L;                      // D[L][.] = L where the fresh search starts, and before it
            for (int k = (a == 0 ? 0 : -kAdWarm / kAdTile); k <= kAdSeg / kAdTile; k++) {
                const int c0 = a + k * kAdTile;          // the tile's first character
                if (c0 - kAdTile >= len) break;          // neither this tile nor the one before it holds a column
                const bool owned = k >= 0 && k < kAdSeg / kAdTile, test = k >= 1 && live;      // (the columns tested in this tile are the tile's before it)
                int hitj = 0x7fffffff, hitd = 0;
#pragma unroll 1
                for (int g = 0; g < kAdTile / 16; g++) {
                    const unsigned chars = __builtin_amdgcn_readfirstlane(text[(c0 - t0 + 16 * g) >> 4]);      // 16 characters, the same in every lane
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const unsigned c = (chars >> (2 * i)) & 3u;
                        const MyersH h = myers_step(pv, mv, myers_eq(peq, c), 0);      // D[0][j] = 0: nothing enters at bit 0
                        const unsigned long long up = (h.Ph >> topb) & 1ull, dn = (h.Mh >> topb) & 1ull;
                        score += (int)up - (int)dn;
                        hp1 = (hp1 << 1) | (hp0 >> 63); hm1 = (hm1 << 1) | (hm0 >> 63);
                        hp0 = (hp0 << 1) | up; hm0 = (hm0 << 1) | dn;
                        lag += (int)(hp1 & 1ull) - (int)(hm1 & 1ull);      // d[t - 64], t = c0 + 16 g + i + 1 this column
                        const int t = c0 + 16 * g + i + 1;
                        if (SCORES) { if (drow && owned && t <= len) drow[t] = (uint8_t)score; }
                        if (test && lag <= md && t - kAdReach <= len && ad_is_hit(lag, t - kAdReach, len, hp1, hm1, hp0, hm0)) { hitj = t - kAdReach; hitd = lag; }
                    }
                }
                for (;;) {                               // the hit columns of the tile before in ascending order, the lanes of a column in theirs: (end, q)
                    const int cm = wave_min(hitj);
                    if (cm == 0x7fffffff) break;
                    const bool mine = hitj == cm;
                    const unsigned long long bal = __ballot(mine);
                    if (mine) {
                        hitj = 0x7fffffff;
                        const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull));
                        if (pos < kAdapterMaxHits) {
                            const int start = ad_start(peq, L, cm, hitd, text, t0);
                            shit[wave][pos] = make_uint4((unsigned)start, (unsigned)cm, (unsigned)(lane >> 1) | ((unsigned)(lane & 1) << 16) | ((unsigned)hitd << 24), 0u);
                        }
                    }
                    cnt += __popcll(bal);
                }
            }
        }
        if (lane == 0) scnt[wave] = cnt;
        __syncthreads();
        // the round's four counts: every thread forms the same prefix; 60 threads store the hits that fall into the record's 15 slots
        int before = total, sum = 0;
#pragma unroll
        for (int w = 0; w < kAdWaves; w++) { const int c = scnt[w]; if (w < tid / kAdapterMaxHits) before += c; sum += c; }
        if (tid < kAdWaves * kAdapterMaxHits) {
            const int w = tid / kAdapterMaxHits, i = tid % kAdapterMaxHits;
            if (i < scnt[w] && before + i < kAdapterMaxHits) out[1 + before + i] = shit[w][i];
        }
        total += sum;
        __syncthreads();                                 // the next round stages its text and hits over these
    }
    const int kept = total < kAdapterMaxHits ? total : kAdapterMaxHits;
    if (tid == 0) out[0] = make_uint4((unsigned)total, (unsigned)len, (unsigned)kept, 0u);
    else if (tid <= kAdapterMaxHits && tid - 1 >= kept) out[tid] = make_uint4(0u, 0u, 0u, 0u);      // the slots no hit took
}

void launch_adapters(hipStream_t s, AdapterKit kit, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map,
                     int max_dist, uint8_t *d_out) {
    if (nread <= 0) return;
    if (d_out) hipLaunchKernelGGL(k_adapters<true>, dim3(nread), dim3(kAdThreads), 0, s, kit, bases, lens, (uint4 *)records, Tb, tbs, map, max_dist, d_out);
    else hipLaunchKernelGGL(k_adapters<false>, dim3(nread), dim3(kAdThreads), 0, s, kit, bases, lens, (uint4 *)records, Tb, tbs, map, max_dist, d_out);
}

}  // namespace ffhip
