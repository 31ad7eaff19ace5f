// ffhip_events.hip -- the signal of every base of a mapped read (FFHIP_RUN_EVENTS, include/ffhip.h "events"): where the base starts, how many samples the pore dwelt
// on it, their mean and their spread.  Both inputs are on the device when k_remap is done: the read's prepared signal (what the first convolution read) and the path's
// bytes rm[]; what is left is a segmented reduction, 4 bytes a sample in and 16 bytes a base out.
//
// k_events: one workgroup of kEvNT threads a listed read; a read whose remap record is not { status 1, end 0 } writes nothing.
//   1. The starts.  Block b closes base p_b when rm[b] = 1, so the k-th one (k = 1 ..) at block b says start[k] = b + 1: an exclusive prefix sum of rm, kEvNT blocks a
//      round -- a ballot and a population count inside a wave, four wave totals through LDS.  start[k] waits in the `first` field of event k, in memory the read owns.
//   2. The events, kEvNT bases a round.  The round's kEvNT + 1 starts come to LDS BEFORE any event of the round is written (base i's end is base i + 1's start), and
//      a round writes only its own events: the next round's starts are still in place.  A thread owns a base.  Spans of up to kEvLane samples it reduces alone, sample
//      after sample.  Longer spans are taken by the base's whole wave, one after the other: lane l adds samples l, l + 64, ... and a butterfly of xor-shuffles adds the
//      lanes (a + b = b + a: every lane holds the same sum), so a base that holds thousands of blocks costs its wave count / 64 rounds, not its thread count rounds.
//   Both passes are fp64 -- the mean, then the squared distances from it -- and each result is rounded to float32 once.  The order of every sum is a function of the
//   span's sample count alone: the same read gives the same bytes wherever it stands in a batch.  No atomics; a span of one repeated value has sd 0.0 exactly.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"
#include <math.h>

namespace ffhip {

constexpr int kEvNT = 256;              // threads of a workgroup: blocks a round of the scan, bases a round of the events
constexpr int kEvLane = 32;             // samples a thread reduces alone; a longer span is its wave's

__global__ void __launch_bounds__(kEvNT)
k_events(const EventRead *__restrict__ list, const float *__restrict__ sig, int stride, const uint4 *__restrict__ rec, const uint8_t *__restrict__ rm,
         int4 *__restrict__ out, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    constexpr int NWV = kEvNT / 64;
    __shared__ int wsum[2][NWV];
    __shared__ int st[kEvNT + 1];
    const EventRead er = list[blockIdx.x];
    const int read = er.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint4 rc = rec[read];
    const int N = tbs ? tbs[read] : TbS, L = (int)rc.y, n = er.n;
    if (rc.x != 1u || rc.w != 0u || L < 1 || L > er.L || N < 1) return;        // not mapped (or more bases than the host gave it room for): nothing is written
    const uint8_t *m = rm + map.row1(read, TbS);
    const float *x = sig + er.sig;
    int4 *ev = out + er.out;

    // ---- 1. start[k], k = 1 .. L - 1, into ev[k].x
    if (tid == 0) ev[0].x = 0;
    int ones = 0;                                                               // ones in front of this round
    for (int b0 = 0, par = 0; b0 < N; b0 += kEvNT, par ^= 1) {
        const int b = b0 + tid;
        const bool one = b < N && m[b] != 0;
        const unsigned long long bal = __ballot(one);
        if (lane == 0) wsum[par][wv] = __popcll(bal);
        __syncthreads();                                                        // (two sets of totals: one barrier a round)
        int before = ones, total = 0;
#pragma unroll
        for (int w = 0; w < NWV; w++) { const int c = wsum[par][w]; before += w < wv ? c : 0; total += c; }
        const int k = before + __popcll(bal & ((1ull << lane) - 1ull)) + 1;
        if (one && k < L) ev[k].x = b + 1;
        ones += total;
    }
    __threadfence();                                                            // every thread's starts, before any thread reads them back
    __syncthreads();

    // ---- 2. the events
    for (int i0 = 0; i0 < L; i0 += kEvNT) {
        const int nb = min(kEvNT, L - i0);
        for (int j = tid; j <= nb; j += kEvNT) st[j] = i0 + j < L ? min(max(ev[i0 + j].x, 0), N) : N;
        __syncthreads();
        int s = 0, cnt = 0;
        if (tid < nb) {
            const long long a = (long long)st[tid] * stride, e = (long long)max(st[tid + 1], st[tid]) * stride;
            s = (int)(a < n ? a : n);
            cnt = (int)(e < n ? e : n) - s;
        }
        double mean = 0.0, sd = 0.0;
        if (cnt > 0 && cnt <= kEvLane) {
            const float *p = x + s;
            double a = 0.0, q = 0.0;
            for (int k = 0; k < cnt; k++) a = a + (double)p[k];
            mean = a / (double)cnt;
            for (int k = 0; k < cnt; k++) { const double d = (double)p[k] - mean; q = q + d * d; }
            sd = sqrt(q / (double)cnt);
        }
        unsigned long long wide = __ballot(cnt > kEvLane);
        while (wide) {                                                          // (uniform in the wave)
            const int j = __ffsll((long long)wide) - 1;
            wide &= wide - 1ull;
            const int sj = __shfl(s, j, 64), cj = __shfl(cnt, j, 64);
            const float *p = x + sj;
            double a = 0.0, q = 0.0;
            for (int k = lane; k < cj; k += 64) a = a + (double)p[k];
            const double mu = wave_sum(a) / (double)cj;
            for (int k = lane; k < cj; k += 64) { const double d = (double)p[k] - mu; q = q + d * d; }
            const double dev = sqrt(wave_sum(q) / (double)cj);
            if (lane == j) { mean = mu; sd = dev; }
        }
        if (tid < nb) ev[i0 + tid] = make_int4(s, cnt, __float_as_int((float)mean), __float_as_int((float)sd));
        __syncthreads();                                                        // st[] changes hands
    }
}

void launch_events(hipStream_t s, const EventRead *list, int count, const float *sig, int stride, const void *records, const uint8_t *rm, void *events,
                   int Tb, const int *tbs, ReadMap map) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_events, dim3(count), dim3(kEvNT), 0, s, list, sig, stride, (const uint4 *)records, rm, (int4 *)events, Tb, tbs, map);
}

}  // namespace ffhip
