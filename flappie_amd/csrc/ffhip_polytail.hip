// ffhip_polytail.hip -- the poly(A) tail of every read (FFHIP_RUN_POLYTAIL, include/ffhip.h "poly tail"): where the signal stays flat while the Viterbi path says the
// tail's base, and how many bases that is at the speed of the rest of the read.  Both inputs are on the device when the decode is done: the read's prepared signal
// (what the first convolution read) and its path; what leaves is one 32-byte record a read.
//
// k_polytail: one workgroup of kPtNT threads a listed read; a read without blocks gets the all-zero record.
//   1. The windows, a round of threads at a time.  A round's samples come to LDS with coalesced loads (a window a row, the pitch odd so that the lanes' walks fall on
//      different banks), its blocks' bases beside them as bytes; a thread then walks its own window in index order: the sum, the mean, the squared distances -- fp64,
//      two passes, no sqrt -- and the count of the tail's base.  A round is min(kPtNT, kPtSamples / pitch) windows: 4 KB of samples, so that the workgroup finds room
//      on a CU beside the next batch's layer kernel.  A window wider than that is walked in memory, kPtNT windows a round.  mu and the flag go to the read's
//      workspace (9 bytes a window).
//   2. The candidates, two scans over the flags, kPtNT windows a round, ballots inside a wave and wave values through LDS across it, a carry across rounds.
//      Backwards, the next flagged window behind w (a min-scan): a flagged window ENDS a merged run iff there is none within gap + 1.  Forwards, the last flagged
//      window in front of w (a max-scan): a flagged window STARTS one iff there is none within gap + 1; and the last start at or in front of w (a max-scan again).
//      An end at w closes the candidate [start, w + 1): every thread keeps the best of its own -- (length, then the tie rule) as one 64-bit key -- and one
//      butterfly and four wave values give the workgroup's.
//   3. The sums over the winner's ranges: flagged windows, mu over them (the one floating-point reduction: a thread's windows in order, a butterfly, the four wave
//      sums in order), the tail's moves, the moves on the far side.  Thread 0 writes the record as two 16-byte stores.
//   Every integer field and rate and bases are functions of the read alone; level's order is a function of the winner's windows alone.  No atomics.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kPtNT = 256;              // threads of a workgroup: windows a round of the scans
constexpr int kPtSamples = 1024;        // floats of LDS a round's windows share

const char *polytail_invalid(const PolyTailParams &p) {
    if (p.base < 0 || p.base > 3) return "base is one of 0 .. 3 (A C G T)";
    if (p.from_end != 0 && p.from_end != 1) return "from_end is 0 or 1";
    if (p.window < 1 || p.window > kPolyTailMaxWindow) return "window is 1 .. 64 blocks";
    if (p.min_calls < 0 || p.min_calls > p.window) return "min_calls is 0 .. window";
    if (p.gap < 0 || p.gap > kPolyTailMaxGap) return "gap is 0 .. 16 windows";
    if (p.min_windows < 1) return "min_windows is at least 1";
    if (p.search < 1) return "search is at least 1 window";
    if (p.min_bases < 1) return "min_bases is at least 1";
    if (!(p.max_sd >= 0.0f) || !(p.max_sd <= 3.0e38f)) return "max_sd is a finite number >= 0";
    return nullptr;
}

__device__ __forceinline__ int pt_base(int state, int nbase) { const int c = state % nbase; return c == 4 ? 1 : c; }

__global__ void __launch_bounds__(kPtNT)
k_polytail(const PolyRead *__restrict__ list, const float *__restrict__ sig, int stride, const int *__restrict__ path, int nbase, PolyTailParams p,
           uint4 *__restrict__ out, double *__restrict__ wmu, uint8_t *__restrict__ wfl, double *__restrict__ wq, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    constexpr int NWV = kPtNT / 64, NONE = 0x7fffffff;
    __shared__ float xs[kPtSamples];
    __shared__ uint8_t bsh[kPtSamples];
    __shared__ int wa[2][NWV], wb[2][NWV], isum[3][NWV];
    __shared__ long long wkey[NWV];
    __shared__ double dsum[NWV];
    const PolyRead pr = list[blockIdx.x];
    const int read = pr.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = tbs ? tbs[read] : TbS, n = pr.n, K = p.window, S = stride, t = p.base;
    uint4 *rec = out + 2 * (size_t)read;
    if (N < 1) {                                                                 // an empty slot: status 0
        if (tid == 0) { rec[0] = make_uint4(0u, 0u, 0u, 0u); rec[1] = make_uint4(0u, 0u, 0u, 0u); }
        return;
    }
    const int *pth = path + map.row1(read, TbS);                                // entries 0 .. N
    const float *x = sig + pr.sig;
    double *mus = wmu + pr.ws, *qs = wq ? wq + pr.ws : nullptr;
    uint8_t *fl = wfl + pr.ws;
    const int NW = min(N, n / S) / K;
    const int KS = NW > 0 ? K * S : 1;                                          // (NW > 0: K S <= n)

    // ---- 1. mu, q and the flag of every window
    {
        const int pitch = KS | 1;
        const int WR = pitch <= kPtSamples ? min(kPtNT, kPtSamples / pitch) : 0; // 0: a window does not fit, the threads walk memory
        const int step = WR ? WR : kPtNT;
        const double thr = ((double)p.max_sd * (double)p.max_sd) * (double)KS;
        for (int w0 = 0; w0 < NW; w0 += step) {
            const int nw = min(step, NW - w0);
            if (WR) {
                const float *src = x + (size_t)w0 * KS;
                for (int i = tid; i < nw * KS; i += kPtNT) { const int r = i / KS; xs[r * pitch + (i - r * KS)] = src[i]; }
                const int *ps = pth + (size_t)w0 * K + 1;
                for (int i = tid; i < nw * K; i += kPtNT) bsh[i] = (uint8_t)pt_base(ps[i], nbase);
                __syncthreads();
            }
            if (tid < nw) {
                const int w = w0 + tid;
                double a = 0.0, q = 0.0, mu;
                int calls = 0;
                if (WR) {
                    const float *xp = xs + tid * pitch;
                    for (int k = 0; k < KS; k++) a = a + (double)xp[k];
                    mu = a / (double)KS;
                    for (int k = 0; k < KS; k++) { const double d = (double)xp[k] - mu; q = q + d * d; }
                    for (int k = 0; k < K; k++) calls += bsh[tid * K + k] == t;
                } else {
                    const float *xp = x + (size_t)w * KS;
                    for (int k = 0; k < KS; k++) a = a + (double)xp[k];
                    mu = a / (double)KS;
                    for (int k = 0; k < KS; k++) { const double d = (double)xp[k] - mu; q = q + d * d; }
                    for (int k = 0; k < K; k++) calls += pt_base(pth[(size_t)w * K + k + 1], nbase) == t;
                }
                mus[w] = mu;
                if (qs) qs[w] = q;
                fl[w] = (uint8_t)(q <= thr && calls >= p.min_calls);
            }
            if (WR) __syncthreads();                                            // xs[], bsh[] change hands
        }
    }
    __threadfence();                                                            // every thread's flags, before any thread reads them back
    __syncthreads();

    // ---- 2a. backwards: bit 1 of a flagged window's byte = it ends a merged run
    const int rounds = (NW + kPtNT - 1) / kPtNT;
    {
        int carry = NONE;                                                       // the first flagged window behind this round
        for (int r = rounds - 1, par = 0; r >= 0; r--, par ^= 1) {
            const int w = r * kPtNT + tid;
            const bool f = w < NW && (fl[w] & 1);
            const unsigned long long bal = __ballot(f);
            if (lane == 0) wa[par][wv] = bal ? r * kPtNT + wv * 64 + __ffsll((long long)bal) - 1 : NONE;
            __syncthreads();                                                    // (two sets of values: one barrier a round)
            int behind = carry, first = carry;                                  // behind: in the waves behind this one; first: in the round
#pragma unroll
            for (int k = NWV - 1; k >= 0; k--) { const int v = wa[par][k]; if (v != NONE) { first = v; if (k > wv) behind = v; } }
            const unsigned long long hi = bal & ~((2ull << lane) - 1ull);
            const int next = hi ? r * kPtNT + wv * 64 + __ffsll((long long)hi) - 1 : behind;
            if (f) fl[w] = (uint8_t)(1 | ((next == NONE || next - w - 1 > p.gap) ? 2 : 0));
            carry = first;
        }
    }
    __threadfence();
    __syncthreads();

    // ---- 2b. forwards: the starts, every end's start, the best candidate
    long long best = -1;
    {
        int cprev = -1, cstart = -1;                                            // the last flagged window, the last start, in front of this round
        for (int r = 0, par = 0; r < rounds; r++, par ^= 1) {
            const int w = r * kPtNT + tid, wbase = r * kPtNT + wv * 64;
            const int byte = w < NW ? fl[w] : 0;
            const bool f = byte & 1;
            const unsigned long long bal = __ballot(f);
            if (lane == 0) wa[par][wv] = bal ? wbase + 63 - __clzll((long long)bal) : -1;
            __syncthreads();
            int front = cprev, last = cprev;                                    // front: in the waves in front of this one; last: in the round
#pragma unroll
            for (int k = 0; k < NWV; k++) { const int v = wa[par][k]; if (v >= 0) { last = v; if (k < wv) front = v; } }
            const unsigned long long lo = bal & ((1ull << lane) - 1ull);
            const int prev = lo ? wbase + 63 - __clzll((long long)lo) : front;
            const bool st = f && (prev < 0 || w - prev - 1 > p.gap);
            const unsigned long long sbal = __ballot(st);
            if (lane == 0) wb[par][wv] = sbal ? wbase + 63 - __clzll((long long)sbal) : -1;
            __syncthreads();
            int sfront = cstart, slast = cstart;
#pragma unroll
            for (int k = 0; k < NWV; k++) { const int v = wb[par][k]; if (v >= 0) { slast = v; if (k < wv) sfront = v; } }
            const unsigned long long slo = sbal & ((2ull << lane) - 1ull);
            const int ws = slo ? wbase + 63 - __clzll((long long)slo) : sfront;
            if (byte & 2) {                                                     // the candidate [ws, w + 1)
                const int we = w + 1, len = we - ws;
                const bool reach = p.from_end ? (long long)we > (long long)NW - (long long)p.search : ws < p.search;
                if (ws >= 0 && len >= p.min_windows && reach) {
                    const long long key = ((long long)len << 32) | (long long)(p.from_end ? we : NONE - ws);
                    best = key > best ? key : best;
                }
            }
            cprev = last;
            cstart = slast;
        }
    }
    best = wave_max(best);
    if (lane == 0) wkey[wv] = best;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NWV; k++) best = wkey[k] > best ? wkey[k] : best;
    if (best < 0) {                                                             // (uniform) no candidate: status 2
        if (tid == 0) { rec[0] = make_uint4(2u, 0u, 0u, 0u); rec[1] = make_uint4(0u, 0u, 0u, 0u); }
        return;
    }

    // ---- 3. the record
    const int len = (int)(best >> 32), tie = (int)(best & 0xffffffffll);
    const int ws = p.from_end ? tie - len : NONE - tie, we = ws + len, bs = ws * K, be = we * K;
    int flat = 0, calls = 0, c = 0;
    double lv = 0.0;
    for (int w = ws + tid; w < we; w += kPtNT) if (fl[w] & 1) { flat++; lv = lv + mus[w]; }
    for (int b = bs + tid; b < be; b += kPtNT) calls += b < N - 1 && pth[b + 1] != pth[b] && pt_base(pth[b + 1], nbase) == t;
    for (int b = (p.from_end ? 0 : be) + tid; b < (p.from_end ? bs : N); b += kPtNT) c += b < N - 1 && pth[b + 1] != pth[b];
    flat = wave_sum(flat); calls = wave_sum(calls); c = wave_sum(c); lv = wave_sum(lv);
    if (lane == 0) { isum[0][wv] = flat; isum[1][wv] = calls; isum[2][wv] = c; dsum[wv] = lv; }
    __syncthreads();
    if (tid == 0) {
        flat = calls = c = 0; lv = 0.0;
#pragma unroll
        for (int k = 0; k < NWV; k++) { flat += isum[0][k]; calls += isum[1][k]; c += isum[2][k]; lv = lv + dsum[k]; }
        const long long total = (long long)N * S < (long long)n ? (long long)N * S : (long long)n;
        const long long so = p.from_end ? (long long)bs * S : total - (long long)be * S;
        const int count = (be - bs) * S;
        const float level = (float)(lv / (double)flat);
        const bool rated = c >= p.min_bases && so > 0;
        const float rate = rated ? (float)((double)so / (double)c) : 0.0f;
        const float bases = rated ? (float)(((double)count * (double)c) / (double)so) : 0.0f;
        rec[0] = make_uint4(rated ? 1u : 3u, (unsigned)(bs * S), (unsigned)count, (unsigned)flat);
        rec[1] = make_uint4((unsigned)calls, __float_as_uint(level), __float_as_uint(rate), __float_as_uint(bases));
    }
}

void launch_polytail(hipStream_t s, const PolyRead *list, int count, const float *sig, int stride, const int *path, int nbase, const PolyTailParams &p, void *records,
                     double *wmu, uint8_t *wfl, double *wq, int Tb, const int *tbs, ReadMap map) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_polytail, dim3(count), dim3(kPtNT), 0, s, list, sig, stride, path, nbase, p, (uint4 *)records, wmu, wfl, wq, Tb, tbs, map);
}

}  // namespace ffhip
