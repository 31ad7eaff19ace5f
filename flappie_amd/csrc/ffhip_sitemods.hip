// ffhip_sitemods.hip -- 5mC at every C of a mapped sequence (FFHIP_RUN_REMAP_MODS, include/ffhip.h "site mods"): around every position i of the sequence that holds C
// or Z, the blocks the mapping gave to the bases i - c .. i + c are scored twice through the transition scores, once with C and once with Z at i, every path of the
// window's blocks through the window's bases allowed.  A few hundred small, independent dynamic programmes a read: wide parallel work on data that is resident when
// k_remap is done (the scores, the coded sequences, the path's bytes).
//
// k_site_starts: one workgroup a listed read; start[0 .. L] (the block every base starts at, start[L] = N) from a prefix count of the path's bytes -- a ballot and a
//   population count in a wave, four wave totals through LDS -- into the read's L + 1 words of the workspace.  A read whose remap record is not { status 1, end 0 }
//   writes nothing.
// k_site_mods<ALL>: one wave a site, kSmWaves sites a workgroup, no barrier and no LDS.  Lane j owns position lo + j of the window (P <= 63 positions) and carries the
//   value of BOTH hypotheses in registers.  The hypothesis' flip-flop states come from the coding of s that the batch holds: positions before i keep theirs, position
//   i takes the letter with the flip or flop that q_{i-1} leaves it, and the positions behind it are recoded one after the other, in a loop that is uniform in the
//   wave and ends where the coding meets that of s again (the end of the run of equal letters).  A lane then knows the (at most) four entries of a block's score row
//   it reads: stay and move of either hypothesis, and window_scores (ffhip_seq.hpp) runs both through the window's blocks: best path in float32, all paths in fp64.
//   The order of operations depends on the window alone: the same read gives the same bytes wherever it stands in a batch.  No atomics, no scratch.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kSmNT = 256;              // threads of either kernel's workgroup
constexpr int kSmWaves = kSmNT / 64;    // sites a workgroup
constexpr int kSmNbase = 5;             // the model with a modified base: ACGTZ

size_t sitemods_sites(const unsigned short *coded, size_t L, int k, std::vector<SiteMod> *out) {
    size_t n = 0;
    for (size_t i = 0; i < L; i++) {
        const int letter = ff_state<kSmNbase>(coded[i]) % kSmNbase;
        if (letter != 1 && letter != 4) continue;
        if (out) out->push_back(SiteMod{ k, (int)i });
        n++;
    }
    return n;
}

__global__ void __launch_bounds__(kSmNT)
k_site_starts(const SiteRead *__restrict__ list, const uint4 *__restrict__ rec, const uint8_t *__restrict__ rm, int *__restrict__ starts, int TbS,
              const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    __shared__ int wsum[2][kSmWaves];
    const SiteRead sr = list[blockIdx.x];
    const int read = sr.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint4 rc = rec[read];
    const int N = tbs ? tbs[read] : TbS, L = sr.L;
    if (rc.x != 1u || rc.w != 0u || (int)rc.y != L || L < 1 || N < 1) return;      // not mapped: nothing is written
    const uint8_t *m = rm + map.row1(read, TbS);
    int *st = starts + sr.start;
    if (tid == 0) { st[0] = 0; st[L] = N; }
    int ones = 0;                                                               // ones in front of this round
    for (int b0 = 0, par = 0; b0 < N; b0 += kSmNT, par ^= 1) {
        const int b = b0 + tid;
        const bool one = b < N && m[b] != 0;
        const unsigned long long bal = __ballot(one);
        if (lane == 0) wsum[par][wv] = __popcll(bal);
        __syncthreads();                                                        // (two sets of totals: one barrier a round)
        int before = ones, total = 0;
#pragma unroll
        for (int w = 0; w < kSmWaves; w++) { const int c = wsum[par][w]; before += w < wv ? c : 0; total += c; }
        const int k = before + __popcll(bal & ((1ull << lane) - 1ull)) + 1;
        if (one && k < L) st[k] = b + 1;
        ones += total;
    }
}

template <bool ALL>
__global__ void __launch_bounds__(kSmNT)
k_site_mods(const SiteRead *__restrict__ list, const SiteMod *__restrict__ sites, int nsite, const unsigned short *__restrict__ seq, const float *__restrict__ trans,
            int Ps, int ctx, const uint4 *__restrict__ rec, const int *__restrict__ starts, int4 *__restrict__ out, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    const int lane = threadIdx.x & 63, site = blockIdx.x * kSmWaves + (threadIdx.x >> 6);
    if (site >= nsite) return;                                                  // (a whole wave: the kernel has no barrier)
    const SiteMod sm = sites[site];
    const SiteRead sr = list[sm.k];
    const int read = sr.read, L = sr.L, i = sm.pos;
    const uint4 rc = rec[read];
    const int N = tbs ? tbs[read] : TbS;
    if (rc.x != 1u || rc.w != 0u || (int)rc.y != L || L < 1 || N < 1 || i < 0 || i >= L) return;
    const int lo = max(0, i - ctx), hi = min(L - 1, i + ctx), P = hi - lo + 1;  // (ctx <= 31: P <= 63)
    const int *st = starts + sr.start;
    const int t0 = min(max(st[lo], 0), N);
    const int t1 = min(max(hi < L - 1 ? st[hi + 1] - 1 : N, t0), N);           // (a path's starts give t0 <= t1 <= N; anything else reads no row outside the read)
    const unsigned short *sq = seq + sr.seq;
    const float *T = trans + map.row0(read, TbS) * (size_t)Ps;

    // ---- the states of both hypotheses at this lane's position
    const int pos = lo + lane;
    const int q0 = lane < P ? ff_state<kSmNbase>(sq[pos]) : 0;                            // the coding of s itself
    const int qb = i > 0 ? ff_state<kSmNbase>(sq[i - 1]) : -1;
    int q[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        int prev = ff_next<kSmNbase>(qb, h ? 4 : 1);
        int mine = pos == i ? prev : q0;
        for (int p = i + 1; p <= hi; p++) {                                     // (uniform in the wave)
            const int orig = __shfl(q0, p - lo, 64);
            const int now = ff_next<kSmNbase>(prev, orig % kSmNbase);
            if (now == orig) break;                                             // the coding of s from here on
            mine = pos == p ? now : mine;
            prev = now;
        }
        q[h] = mine;
    }
    int is[2], im[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int below = __shfl_up(q[h], 1, 64);
        is[h] = ff_lookup(q[h], q[h], kSmNbase);
        im[h] = lane > 0 ? ff_lookup(below, q[h], kSmNbase) : 0;
    }

    win_real<ALL> X[2];
    window_scores<ALL>(T, Ps, t0, t1, is, im, lane, X);
    if (lane == P - 1) out[site] = make_int4(i, t1 - t0, __float_as_int((float)X[0]), __float_as_int((float)X[1]));
}

void launch_site_starts(hipStream_t s, const SiteRead *list, int nread, const void *records, const uint8_t *rm, int *starts, int Tb, const int *tbs, ReadMap map) {
    if (nread <= 0) return;
    hipLaunchKernelGGL(k_site_starts, dim3(nread), dim3(kSmNT), 0, s, list, (const uint4 *)records, rm, starts, Tb, tbs, map);
}

void launch_site_mods(hipStream_t s, const SiteRead *list, int nread, const SiteMod *sites, int nsite, const unsigned short *seq, const float *trans, int Ps,
                      int context, int all_paths, const void *records, const uint8_t *rm, int *starts, void *out, int Tb, const int *tbs, ReadMap map) {
    if (nread <= 0 || nsite <= 0) return;
    const uint4 *rec = (const uint4 *)records;
    hipLaunchKernelGGL(k_site_starts, dim3(nread), dim3(kSmNT), 0, s, list, rec, rm, starts, Tb, tbs, map);
    const dim3 grid((nsite + kSmWaves - 1) / kSmWaves);
    if (all_paths) hipLaunchKernelGGL((k_site_mods<true>), grid, dim3(kSmNT), 0, s, list, sites, nsite, seq, trans, Ps, context, rec, starts, (int4 *)out, Tb, tbs, map);
    else hipLaunchKernelGGL((k_site_mods<false>), grid, dim3(kSmNT), 0, s, list, sites, nsite, seq, trans, Ps, context, rec, starts, (int4 *)out, Tb, tbs, map);
}

}  // namespace ffhip
