// ffhip_truth.hip -- the call scored against a sequence the caller knows (FFHIP_RUN_TRUTH, include/ffhip.h "truth"): a banded global edit-distance alignment with
// traceback, one read a workgroup, behind k_assemble on the decode's stream.
//
// Cell (j, i): j = 0 .. m truth bases and i = 0 .. n call bases consumed; allowed iff |i - c(j)| <= W, c(j) = floor(j n / m).  In integers
//   D[j][i] = min(D[j-1][i-1] + (t_j != s_i), D[j-1][i] + 1, D[j][i-1] + 1),
// include/ffhip.h holds the whole statement and tests/truth_ref.py restates it.  Rows run in sequence (the band runs along the truth, whose length the host knows), a
// row's cells in parallel: with a_i = min(diagonal, deletion), the insertion chain D[j][i] = min(a_i, D[j][i-1] + 1) is i + prefix-min(a_k - k) over the row's allowed
// cells, which are contiguous -- K values a lane in sequence, the lanes' totals by a DPP scan across the wave, the waves' totals through LDS.
//
// k_truth<NT, K>: NT threads a read, K consecutive cells a thread in registers, S = NT K slots; slot s of row j is cell lo(j) + s, lo(j) = clamp(c(j) - W, 0,
// n + 1 - min(2 W + 1, n + 1)).  The window may advance by any number of cells a row (n > m), so a finished row is handed to the next through LDS, which reads it
// `lo(j) - lo(j-1)` slots further on, guarded by the band of the row before.  NT = 64 is ONE wave: its LDS operations are in order, and no barrier stands in the
// per-row chain; the workgroup forms have two a row (the waves' totals, the row).  The truth comes through LDS in chunks of at most 64 rows, fewer where the call is
// much the longer, so that the call's letters a chunk can reach fit a ring in LDS; the next chunk's truth and the ring's new letters are loaded into registers
// while this chunk is worked, so no row waits for HBM.  What bounds a row is the chain LDS read -> min -> scan -> LDS write.
// The row's decisions -- the op the traceback takes INTO each cell, two bits: 0 '=', 1 'X', 2 'I', 3 'D', by include/ffhip.h's rule on D alone -- leave as whole
// 64-bit ballot words, 2 K a wave and row, at [row - 1][wave][register][bit plane] of the read's workspace.  Traceback: the same workgroup, behind a fence, brings
// the words back through LDS in chunks of rows; thread 0 follows them from (m, n) and writes the op bytes downwards from the end of the read's bytes, so that they
// stand in path order and end at the last byte; the counts, maxdev and K go to the read's record.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"
#include <algorithm>

namespace ffhip {

constexpr int kTruthCR = 64;            // truth bases a chunk, at most (<= 64: one lane each prefetches the next chunk)
constexpr int kTruthTbWords = 2048;     // 64-bit words of decisions a chunk of the traceback stages in LDS
constexpr int kTruthInf = 1 << 29, kTruthBig = (1 << 30) - 1;
static const int kTruthNT[kTruthForms] = { 64, 64, 256, 512 }, kTruthK[kTruthForms] = { 1, 4, 5, 5 };

int truth_form(long long window) {
    for (int f = 0; f < kTruthForms; f++) if (window <= (long long)kTruthNT[f] * kTruthK[f]) return f;
    return -1;
}
int truth_max_window() { return kTruthNT[kTruthForms - 1] * kTruthK[kTruthForms - 1]; }
int truth_max_band() { return (truth_max_window() - 1) / 2; }
size_t truth_ws_words(int form, int m) { return (size_t)m * (size_t)(kTruthNT[form] / 64 * kTruthK[form] * 2); }

// inclusive prefix minimum over the wave's 64 lanes: four shifts inside each row of 16 lanes, then lane 15 and lane 31 broadcast to the rows behind them
__device__ __forceinline__ int tr_wave_scan_min(int v, int lane) {
    int t;
    t = __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false); if ((lane & 15) >= 1) v = min(t, v);      // row_shr:1
    t = __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false); if ((lane & 15) >= 2) v = min(t, v);      // row_shr:2
    t = __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false); if ((lane & 15) >= 4) v = min(t, v);      // row_shr:4
    t = __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false); if ((lane & 15) >= 8) v = min(t, v);      // row_shr:8
    t = __builtin_amdgcn_update_dpp(v, v, 0x142, 0xf, 0xf, false); if ((lane & 31) >= 16) v = min(t, v);     // row_bcast:15
    t = __builtin_amdgcn_update_dpp(v, v, 0x143, 0xf, 0xf, false); if (lane >= 32) v = min(t, v);            // row_bcast:31
    return v;
}

template <int NT>
__device__ __forceinline__ void tr_row_sync() {
    if constexpr (NT > 64) __syncthreads();
    else {                              // one wave: its LDS operations execute in order; only the compiler has to keep them so
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

constexpr int tr_ring(int S) { int r = 64; while (r < 2 * S) r *= 2; return r; }

template <int NT, int K>
__global__ void __launch_bounds__(NT)
k_truth(const TruthRead *__restrict__ list, const uint8_t *__restrict__ seq, const char *__restrict__ bases, const int *__restrict__ lens, int band,
        unsigned long long *__restrict__ ws, int *__restrict__ rec, uint8_t *__restrict__ ops, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    constexpr int S = NT * K, NWV = NT / 64, WPR = NWV * K * 2, R = tr_ring(S), PF = R / NT, TR = kTruthTbWords / WPR;
    static_assert(kTruthCR <= NT && R % NT == 0 && TR >= 1, "a lane prefetches one truth base and whole shares of the ring");
    __shared__ int rowv[2][S];
    __shared__ uint8_t ring[R];
    __shared__ uint8_t tq[2][kTruthCR];
    __shared__ int wtot[NWV];
    __shared__ unsigned long long tbw[kTruthTbWords];
    __shared__ int fin;
    const TruthRead tr = list[blockIdx.x];
    const int read = tr.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Tb = tbs ? tbs[read] : TbS, m = tr.m;
    int n = Tb > 0 ? lens[read] : 0;
    n = n > 0 ? n : 0;
    int *rc = rec + (size_t)read * kTruthRecInts;
    const int W = band, Wd = 2 * W + 1 < n + 1 ? 2 * W + 1 : n + 1;
    int status = tr.status;
    if (status == 1 && (m < 1 || Wd > S || n > tr.cap - m || n > kTruthMaxLen)) status = 2;      // (the last three: the host sized form and bytes so that they cannot be)
    if (status != 1) {
        if (tid < kTruthRecInts) rc[tid] = tid == 0 ? status : tid == 1 ? n : tid == 2 ? m : 0;
        return;
    }
    const char *bs = bases + map.row1(read, TbS);
    const uint8_t *tt = seq + tr.seq;
    unsigned long long *tw = ws + tr.ws;
    const int q = n / m, r = n - q * m;
    const int RC = min(kTruthCR, 1 + (R - S) / (q + 1));       // rows a chunk: the window's lower edge moves by at most (RC - 1)(q + 1) <= R - S cells in it
    const int lo_max = n + 1 - Wd;
    auto lof = [&](int c) { return min(max(c - W, 0), lo_max); };
    auto cof = [&](int j) { return (int)(((long long)j * n) / m); };
    // the cells whose letters the chunk of rows [j0, j0 + RC) reads: [*a, *b), at most R of them
    auto reach = [&](int j0, int *a, int *b) { const int j1 = min(j0 + RC, m + 1); *a = lof(cof(j0)); *b = min(n + 1, lof(cof(j1 - 1)) + S); };

    int have;                                                   // the ring holds the letter of every cell below it that a later row can read (cell i: s_i at i mod R)
    {
        int a, b;
        reach(1, &a, &b);
        for (int i = a + tid; i < b; i += NT) ring[i & (R - 1)] = i > 0 ? (uint8_t)seq_code(bs[i - 1]) : (uint8_t)0;
        have = b;
        if (tid < min(RC, m)) { const int t = tt[tid]; tq[0][tid] = (uint8_t)(t == 4 ? 1 : t); }
    }
    int lo = 0, alo = 0, ahi = min(W, n), c = 0, acc = 0;
#pragma unroll
    for (int k = 0; k < K; k++) { const int s = tid * K + k; rowv[0][s] = s <= ahi ? s : kTruthInf; }      // row 0: D[0][i] = i
    __syncthreads();

    for (int j0 = 1, buf = 0; j0 <= m; j0 += RC, buf ^= 1) {
        const int j1 = min(j0 + RC, m + 1);
        // the next chunk's share, into registers
        int na = 0, nb = 0;
        if (j1 <= m) { reach(j1, &na, &nb); na = max(na, have); }
        uint8_t pf[PF];
#pragma unroll
        for (int x = 0; x < PF; x++) { const int i = na + tid + x * NT; pf[x] = (i < nb && i > 0) ? (uint8_t)seq_code(bs[i - 1]) : (uint8_t)0; }
        const int tnext = (j1 <= m && tid < min(RC, m + 1 - j1)) ? tt[j1 - 1 + tid] : 0;

        for (int j = j0; j < j1; j++) {
            const int lo_p = lo, alo_p = alo, ahi_p = ahi;
            c += q; acc += r;
            if (acc >= m) { acc -= m; c++; }                    // c = c(j)
            lo = lof(c); alo = max(c - W, 0); ahi = min(c + W, n);
            const int tj = tq[buf][j - j0];
            const int *pr = rowv[(j - 1) & 1];
            const int i0 = lo + tid * K, p0 = i0 - lo_p;        // my first cell, and its slot in the row before
            int pv[K + 1];                                      // D[j-1][i0 - 1 .. i0 + K - 1], +inf where the row before does not allow the cell
#pragma unroll
            for (int k = 0; k <= K; k++) {
                const int i = i0 + k - 1, p = p0 + k - 1;
                const int v = pr[min(max(p, 0), S - 1)];
                pv[k] = (i >= alo_p && i <= ahi_p) ? v : kTruthInf;
            }
            int cost[K], pm[K], run = kTruthBig;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int i = i0 + k;
                cost[k] = ring[i & (R - 1)] != tj ? 1 : 0;
                const int a = (i >= alo && i <= ahi) ? min(pv[k] + cost[k], pv[k + 1] + 1) : kTruthInf;
                run = min(run, a - i);
                pm[k] = run;
            }
            const int incl = tr_wave_scan_min(run, lane);
            int excl = __shfl_up(incl, 1, 64);
            excl = lane == 0 ? kTruthBig : excl;
            if constexpr (NT > 64) {
                if (lane == 63) wtot[wv] = incl;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NWV - 1; w++) { const int t = wtot[w]; excl = w < wv ? min(excl, t) : excl; }
            }
            unsigned long long mine = 0ull;
            int *pw = rowv[j & 1];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int i = i0 + k;
                int d = i + min(excl, pm[k]);
                d = (i >= alo && i <= ahi && d < kTruthInf / 2) ? d : kTruthInf;
                const int op = pv[k] + cost[k] == d ? cost[k] : pv[k + 1] + 1 == d ? 3 : 2;
                pw[tid * K + k] = d;
                const unsigned long long b0 = __ballot(op & 1), b1 = __ballot(op & 2);
                mine = lane == 2 * k ? b0 : lane == 2 * k + 1 ? b1 : mine;
            }
            if (lane < 2 * K) tw[(size_t)(j - 1) * WPR + wv * 2 * K + lane] = mine;
            tr_row_sync<NT>();
        }
#pragma unroll
        for (int x = 0; x < PF; x++) { const int i = na + tid + x * NT; if (i < nb) ring[i & (R - 1)] = pf[x]; }
        if (j1 <= m) { have = nb > have ? nb : have; if (tid < min(RC, m + 1 - j1)) tq[buf ^ 1][tid] = (uint8_t)(tnext == 4 ? 1 : tnext); }
        __syncthreads();
    }
    if (tid == 0) fin = rowv[m & 1][n - lo];
    __threadfence();                                            // the words of every wave, before any thread reads them back
    __syncthreads();
    const int dist = fin;
    if (dist >= kTruthInf / 2) {                                // the band leaves no path
        if (tid < kTruthRecInts) rc[tid] = tid == 0 ? 2 : tid == 1 ? n : tid == 2 ? m : 0;
        return;
    }
    __syncthreads();                                            // (fin is written again below)

    // ---- traceback: thread 0's state; c = c(j), acc = (j n) mod m
    int j = m, i = n, pos = tr.cap, cnt[4] = { 0, 0, 0, 0 }, maxdev = 0, bad = 0;
    c = n; acc = 0;
    uint8_t *op = ops + tr.ops;
    for (int jt = m; jt >= 1; ) {
        const int jlo = max(1, jt - TR + 1), nw = (jt - jlo + 1) * WPR;
        for (int x = tid; x < nw; x += NT) tbw[x] = tw[(size_t)(jlo - 1) * WPR + x];
        __syncthreads();
        if (tid == 0) {
            while (j >= jlo && !bad) {
                const int slot = i - lof(c);
                if (slot < 0 || slot >= S || pos <= 0) { bad = 1; break; }
                const int th = slot / K, kk = slot - th * K, at = (j - jlo) * WPR + (th >> 6) * 2 * K + 2 * kk, sh = th & 63;
                const int code = (int)((tbw[at] >> sh) & 1ull) | ((int)((tbw[at + 1] >> sh) & 1ull) << 1);
                op[--pos] = (uint8_t)code;
                cnt[0] += code == 0; cnt[1] += code == 1; cnt[2] += code == 2; cnt[3] += code == 3;
                if (code != 2) { j--; c -= q; acc -= r; if (acc < 0) { acc += m; c--; } }
                if (code != 3) i--;
                if (i < 0) { bad = 1; break; }
                const int dev = i > c ? i - c : c - i;
                maxdev = dev > maxdev ? dev : maxdev;
            }
            fin = bad ? 0 : j;
        }
        __syncthreads();
        jt = fin;
    }
    if (tid == 0) {
        while (i > 0 && !bad && j == 0) {                      // row 0: insertions
            if (pos <= 0) { bad = 1; break; }
            op[--pos] = (uint8_t)2;
            cnt[2]++;
            i--;
            maxdev = i > maxdev ? i : maxdev;
        }
        rc[0] = 1; rc[1] = n; rc[2] = m; rc[3] = dist;
        rc[4] = cnt[0]; rc[5] = cnt[1]; rc[6] = cnt[2]; rc[7] = cnt[3];
        rc[8] = maxdev; rc[9] = tr.cap - pos;
        rc[10] = bad ? -1 : i + j;                              // the cell the traceback came out at: 0 for a path
        rc[11] = 0;
    }
}

void launch_truth(hipStream_t s, int form, const TruthRead *list, int count, const uint8_t *seq, const char *bases, const int *lens, int band,
                  unsigned long long *ws, int *records, uint8_t *ops, int Tb, const int *tbs, ReadMap map) {
    if (count <= 0) return;
#define FFHIP_TRUTH_FORM(NT_, K_) hipLaunchKernelGGL((k_truth<NT_, K_>), dim3(count), dim3(NT_), 0, s, list, seq, bases, lens, band, ws, records, ops, Tb, tbs, map)
    switch (form) {
    case 0: FFHIP_TRUTH_FORM(64, 1); break;
    case 1: FFHIP_TRUTH_FORM(64, 4); break;
    case 2: FFHIP_TRUTH_FORM(256, 5); break;
    default: FFHIP_TRUTH_FORM(512, 5); break;
    }
#undef FFHIP_TRUTH_FORM
}

}  // namespace ffhip
