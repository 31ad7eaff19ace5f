// ffhip_remap.hip -- constrained Viterbi of a read's transition scores against a GIVEN sequence (FFHIP_RUN_REMAP, include/ffhip.h "remap"): which blocks of
// the signal belong to which base of a sequence the caller already knows.
//
// The sequence s of L bases is flip-flop coded (q_i: a repeated base alternates between its flip and its flop state), a path p_0 = 0 .. p_N = L - 1 steps by 0 or 1
// a block, and its score is the sum of the entries ff_lookup(q_from, q_to) (ffhip_seq.hpp) of the blocks' score rows.  Cell (b, i) is allowed iff
// |i - c(b)| <= W, c(b) = floor(b (L - 1) / N).  V_{b+1}[i] = move if move > stay (strictly) else stay, each ONE float32 add; include/ffhip.h holds the whole
// statement and tests/remap_ref.py restates it.  The host codes the sequence when it copies it (remap_code): what reaches the device is, per position, the two
// entries a block's row is read at -- stay (q_i -> q_i) in the low byte, move (q_{i-1} -> q_i) in the high byte.
//
// k_remap<NT, K>: one workgroup of NT threads a read, K cells a thread in registers, S = NT K slots.  Cell i lives in slot i mod S for as long as it is inside the
// live window [lo, lo + S), lo = clamp(c(b) - W, 0, L - min(2 W + 1, L)): the window advances by at most one cell a block, and the one slot that falls out of it
// behind takes the cell that enters in front (value -inf, entries from the LDS ring of the sequence).  A thread's K slots are consecutive, so a step needs ONE
// value from the thread below: a cross-lane move inside a wave, and between waves the last lane's value through two LDS words and the step's one barrier.  The
// one-wave forms (NT = 64) have no barrier in that per-step chain (each chunk still ends in one, and the traceback has two a chunk).  Blocks run in sequence: the score rows come through LDS in chunks of <= 48 blocks, the next chunk (and the
// sequence entries the window will reach in it) loaded into registers while this one is worked, so that no step waits for HBM; what bounds a step is the
// dependent chain cross-lane move -> add -> compare (-> barrier), as for the other chains of the decode.
// The step's decisions leave as whole 64-bit words: one ballot a register, K words a wave, at [block][wave][register] of the read's traceback workspace.
// Traceback: the same workgroup, behind a fence, brings the words back in chunks of 256 / K blocks (the chunk before prefetched in registers); thread 0
// follows the bits from cell L - 1 -- the bit of cell i is bit (i mod S) / K mod 64 of word [wave][(i mod S) mod K] -- and the chunk's bytes go out together.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"
#include <math.h>
#include <algorithm>

namespace ffhip {

constexpr int kRemapChunk = 2048;       // floats of score rows a chunk stages in LDS
constexpr int kRemapCB = 48;            // blocks a chunk, at most (<= 64: a thread prefetches at most one sequence entry a chunk)
static const int kRemapNT[kRemapForms] = { 64, 64, 256, 512 }, kRemapK[kRemapForms] = { 1, 4, 4, 9 };

int remap_form(int L, int band) {
    const long long wd = std::min<long long>(2ll * band + 1, L);
    for (int f = 0; f < kRemapForms; f++) if (wd <= (long long)kRemapNT[f] * kRemapK[f]) return f;
    return -1;
}
int remap_max_window() { return kRemapNT[kRemapForms - 1] * kRemapK[kRemapForms - 1]; }
size_t remap_ws_words(int form, int nblock) { return (size_t)nblock * (size_t)(kRemapNT[form] / 64 * kRemapK[form]); }

void remap_code(const uint8_t *codes, size_t L, int nbase, unsigned short *out) {
    int prev = 0;
    for (size_t i = 0; i < L; i++) {
        const int s = codes[i];
        const int q = (i > 0 && s == codes[i - 1] && prev < nbase) ? s + nbase : s;
        out[i] = (unsigned short)(ff_lookup(q, q, nbase) | ((i > 0 ? ff_lookup(prev, q, nbase) : 0) << 8));
        prev = q;
    }
}

template <int NT, int K>
__global__ void __launch_bounds__(NT)
k_remap(const RemapRead *__restrict__ list, const unsigned short *__restrict__ seq, const float *__restrict__ trans, int Ps, int band,
        unsigned long long *__restrict__ ws, uint4 *__restrict__ rec, uint8_t *__restrict__ rm, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    constexpr int S = NT * K, NWV = NT / 64, WPS = NWV * K, QR = S + 2 * kRemapCB + 8, PF = kRemapChunk / NT, TBS = 256 / K, TPF = (TBS * WPS + NT - 1) / NT;
    static_assert(kRemapChunk % NT == 0 && kRemapCB <= 64, "a thread prefetches whole shares of a chunk");
    __shared__ float tch[2][kRemapChunk];
    __shared__ unsigned short qs[QR];
    __shared__ float edge[2][NWV];
    __shared__ unsigned long long tbw[2][TBS * WPS];
    __shared__ uint8_t rmc[TBS];
    __shared__ float fscore;
    const RemapRead rr = list[blockIdx.x];
    const int read = rr.read, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = tbs ? tbs[read] : TbS, L = rr.L;
    int status = rr.status;
    if (status == 1 && (N < 1 || L < 1 || L > N + 1)) status = 2;
    if (status != 1) {
        if (tid == 0) rec[read] = make_uint4((unsigned)status, (unsigned)L, 0u, 0u);
        return;
    }
    const float *T = trans + map.row0(read, TbS) * (size_t)Ps;
    uint8_t *out = rm + map.row1(read, TbS);
    unsigned long long *tw = ws + rr.ws;
    const unsigned short *sq = seq + rr.seq;
    const int W = band < L ? band : L, Wd = 2 * W + 1 < L ? 2 * W + 1 : L;      // (W >= L - 1 excludes nothing: W = L says the same without overflow)
    const int CB = min(kRemapChunk / Ps, kRemapCB);
    const float NEG = -INFINITY;
    auto lof = [&](int b) { const int c = (int)(((long long)b * (L - 1)) / N); return min(max(c - W, 0), L - Wd); };
    auto need = [&](int b0) { return min(L, lof(min(b0 + CB, N)) + S + 1); };      // the sequence entries the window can reach in the chunk that starts at b0

    int qhi = need(0);
    for (int i = tid; i < qhi; i += NT) qs[i] = sq[i];                              // (<= S + CB + 1 < QR: no wrap yet)
    { const int n0 = min(CB, N) * Ps; for (int j = tid; j < n0; j += NT) tch[0][j] = T[j]; }
    __syncthreads();

    float V[K];
    int idx[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int slot = tid * K + k;
        V[k] = slot == 0 ? 0.0f : NEG;
        idx[k] = slot < L ? qs[slot] : 0;
    }
    int lo = 0, lo_mod = 0, c = 0, acc = 0;
    for (int b0 = 0, buf = 0; b0 < N; b0 += CB, buf ^= 1) {
        const int nb = min(CB, N - b0), nxt0 = b0 + CB;
        const int nn = nxt0 < N ? min(CB, N - nxt0) * Ps : 0;
        float pf[PF];
#pragma unroll
        for (int j = 0; j < PF; j++) { const int e = tid + j * NT; pf[j] = e < nn ? T[(size_t)nxt0 * Ps + e] : 0.0f; }
        const int need_next = nxt0 < N ? need(nxt0) : qhi;
        const unsigned short qpf = qhi + tid < need_next ? sq[qhi + tid] : (unsigned short)0;
        const float *tc = tch[buf];
        for (int bl = 0; bl < nb; bl++) {
            const int b = b0 + bl;
            acc += L - 1;
            if (acc >= N) { acc -= N; c++; }                        // c = c(b + 1)
            const int lo_new = min(max(c - W, 0), L - Wd);
            // the value below every slot, before any slot changes hands
            float up = __shfl(V[K - 1], (lane + 63) & 63, 64);
            if constexpr (NT > 64) {
                if (lane == 63) edge[b & 1][wv] = V[K - 1];
                __syncthreads();
                if (lane == 0) up = edge[b & 1][(wv + NWV - 1) % NWV];
            }
            float nbv[K];
            nbv[0] = up;
#pragma unroll
            for (int k = 1; k < K; k++) nbv[k] = V[k - 1];
            if (lo_new != lo) {                                     // slot lo mod S: cell lo leaves, cell lo + S enters
                const int cell = lo + S;
#pragma unroll
                for (int k = 0; k < K; k++)
                    if (tid * K + k == lo_mod) { V[k] = NEG; idx[k] = cell < L ? qs[cell % QR] : 0; }
                lo = lo_new;
                lo_mod = lo_mod + 1 == S ? 0 : lo_mod + 1;
            }
            const int a_lo = max(c - W, 0) - lo, a_hi = min(c + W, L - 1) - lo;
            const float *tr = tc + bl * Ps;
            unsigned long long mine = 0ull;
#pragma unroll
            for (int k = 0; k < K; k++) {
                int d = tid * K + k - lo_mod;
                d = d < 0 ? d + S : d;                              // the cell is lo + d
                const float stay = V[k] + tr[idx[k] & 255];
                const float move = (lo + d == 0) ? NEG : nbv[k] + tr[idx[k] >> 8];
                const bool win = move > stay;
                V[k] = (d >= a_lo && d <= a_hi) ? (win ? move : stay) : NEG;
                const unsigned long long bal = __ballot(win);
                mine = lane == k ? bal : mine;
            }
            if (lane < K) tw[(size_t)b * WPS + wv * K + lane] = mine;
        }
#pragma unroll
        for (int j = 0; j < PF; j++) { const int e = tid + j * NT; if (e < nn) tch[buf ^ 1][e] = pf[j]; }
        if (qhi + tid < need_next) qs[(qhi + tid) % QR] = qpf;
        qhi = need_next;
        __syncthreads();
    }
    {
        const int slot = (L - 1) % S;
#pragma unroll
        for (int k = 0; k < K; k++) if (tid * K + k == slot) fscore = V[k];
    }
    __threadfence();                                                // the words of every wave, before any thread reads them back
    __syncthreads();
    // A score that is not finite (a NaN or an infinity on the way: no strict compare need have won) leaves bits that describe no path: not mapped, status 2, and
    // no traceback.  A finite one was chosen, block by block, from a finite source plus a finite entry, so its bits lead through allowed cells to cell 0.
    if (!(fabsf(fscore) < INFINITY)) {                              // (uniform: one LDS word)
        if (tid == 0) rec[read] = make_uint4(2u, (unsigned)L, 0u, 0u);
        return;
    }

    // ---- traceback
    int th = ((L - 1) % S) / K, kk = ((L - 1) % S) % K, p = L - 1;   // (thread 0's: the slot of cell p as thread and register)
    int e1 = N, buf = 0;
    {
        const int e0 = max(0, e1 - TBS), n = (e1 - e0) * WPS;
        for (int j = tid; j < n; j += NT) tbw[0][j] = tw[(size_t)e0 * WPS + j];
    }
    __syncthreads();
    while (e1 > 0) {
        const int e0 = max(0, e1 - TBS), f1 = e0, f0 = max(0, f1 - TBS), nn = (f1 - f0) * WPS;
        unsigned long long tpf[TPF];
#pragma unroll
        for (int j = 0; j < TPF; j++) { const int e = tid + j * NT; tpf[j] = e < nn ? tw[(size_t)f0 * WPS + e] : 0ull; }
        if (tid == 0) {
            for (int t = e1 - e0 - 1; t >= 0; t--) {
                const unsigned long long w = tbw[buf][t * WPS + (th >> 6) * K + kk];
                const int bit = (int)((w >> (th & 63)) & 1ull);
                rmc[t] = (uint8_t)bit;
                if (bit) {
                    p--;
                    if (--kk < 0) { kk = K - 1; if (--th < 0) th = NT - 1; }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TPF; j++) { const int e = tid + j * NT; if (e < nn) tbw[buf ^ 1][e] = tpf[j]; }
        __syncthreads();
        for (int t = tid; t < e1 - e0; t += NT) out[e0 + t] = rmc[t];
        __syncthreads();
        e1 = e0; buf ^= 1;
    }
    // { int32 status, L; float score; int32 end }: end = the cell the traceback came out at, 0 for a path
    if (tid == 0) rec[read] = make_uint4(1u, (unsigned)L, __float_as_uint(fscore), (unsigned)p);
}

void launch_remap(hipStream_t s, int form, const RemapRead *list, int count, const unsigned short *seq, const float *trans, int Ps, int band,
                  unsigned long long *ws, void *records, uint8_t *rm, int Tb, const int *tbs, ReadMap map) {
    if (count <= 0) return;
    uint4 *rec = (uint4 *)records;
#define FFHIP_REMAP_FORM(NT_, K_) hipLaunchKernelGGL((k_remap<NT_, K_>), dim3(count), dim3(NT_), 0, s, list, seq, trans, Ps, band, ws, rec, rm, Tb, tbs, map)
    switch (form) {
    case 0: FFHIP_REMAP_FORM(64, 1); break;
    case 1: FFHIP_REMAP_FORM(64, 4); break;
    case 2: FFHIP_REMAP_FORM(256, 4); break;
    default: FFHIP_REMAP_FORM(512, 9); break;
    }
#undef FFHIP_REMAP_FORM
}

}  // namespace ffhip
