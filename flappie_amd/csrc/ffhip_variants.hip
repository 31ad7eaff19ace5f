// ffhip_variants.hip -- ref against alt alleles of a mapped sequence (FFHIP_RUN_REMAP_VARIANTS, include/ffhip.h "variants"): around every variant -- a short edit
// { pos p, nref r, nalt k, alt[] } of the sequence s a read was mapped to -- the blocks the mapping gave to the bases p - c .. p + r + c - 1 are scored twice through
// the transition scores, once through those bases of s and once through the bases the edit puts in their place, every path of the window's blocks through a
// hypothesis's bases allowed.  The recursion is k_site_mods' (window_scores, ffhip_seq.hpp); the hypotheses are more general: the edit is any substitution,
// insertion or deletion of up to 16 letters, so the two may differ in LENGTH, and the alphabet has 4 or 5 letters.  The starts come from k_site_starts, launched here over this
// feature's own list of reads into its own workspace.
//
// k_variants<ALL>: one wave a variant, kVrWaves variants a workgroup, no barrier and no LDS.  Lane j owns window position j of EACH hypothesis -- position lo + j
//   of s and position lo + j of s^alt -- and carries both values in registers; P_ref and P_alt are at most 62.  The ref states are the coding of s the batch
//   holds.  Lane j's alt letter is s[lo + j] in front of p, alt[lo + j - p] inside the edit (the variant's 24 bytes) and s[lo + j - k + r] behind it; the alt
//   states are those of s in front of p, and from p on they are coded one after the other from the state of q[p - 1], in a loop that is uniform in the wave and
//   ends, behind the edit, where the coding meets that of s again (the end of a run of equal letters) or at the window's last position.  A lane then knows the
//   (at most) four entries of a block's score row it reads: stay and move of either hypothesis, and window_scores (ffhip_seq.hpp) runs both through the window's
//   blocks: best path in float32, all paths in fp64.  A hypothesis with fewer blocks than moves keeps -inf in its last lane: no special case.  The two results sit in
//   lanes P_ref - 1 and P_alt - 1; the alt one is brought to lane P_ref - 1, which writes the record as one 16-byte store.
//   The order of operations depends on the window and the variant alone: the same read gives the same bytes wherever it stands in a batch.  No atomics, no scratch.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

constexpr int kVrNT = 256;              // threads of the workgroup
constexpr int kVrWaves = kVrNT / 64;    // variants a workgroup
static_assert(2 * kVariantsMaxContext + kVariantsMaxAllele <= 64, "a lane a window position");

const char *variant_invalid(const Variant &v, size_t L, int nbase) {
    if (v.nref > kVariantsMaxAllele || v.nalt > kVariantsMaxAllele) return "an allele is longer than 16";
    if (v.nref + v.nalt < 1) return "ref and alt are both empty";
    if (v.pos < 0 || (size_t)v.pos + v.nref > L) return "pos + nref lies beyond the sequence";
    for (int i = 0; i < v.nalt; i++) if (v.alt[i] >= nbase) return "an alt code is not a base of the model";
    if (L - v.nref + v.nalt < 1) return "the edit leaves no base";
    return nullptr;
}

template <bool ALL, int NB>
__global__ void __launch_bounds__(kVrNT)
k_variants(const SiteRead *__restrict__ list, const VarEntry *__restrict__ vars, int nvar, const unsigned short *__restrict__ seq, const float *__restrict__ trans,
           int Ps, int ctx, const uint4 *__restrict__ rec, const int *__restrict__ starts, int4 *__restrict__ out, int TbS, const int *__restrict__ tbs, ReadMap map) {
    FFHIP_DECODE_PRIO_SET();
    const int lane = threadIdx.x & 63, vi = blockIdx.x * kVrWaves + (threadIdx.x >> 6);
    if (vi >= nvar) return;                                                     // (a whole wave: the kernel has no barrier)
    const int4 head = *(const int4 *)(vars + vi);                               // { k, index, pos, nref | nalt << 8 | alt[0 .. 1] << 16 }
    const SiteRead sr = list[head.x];
    const int read = sr.read, L = sr.L, p = head.z, r = head.w & 255, k = (head.w >> 8) & 255;
    const uint4 rc = rec[read];
    const int N = tbs ? tbs[read] : TbS;
    if (rc.x != 1u || rc.w != 0u || (int)rc.y != L || L < 1 || N < 1) return;
    if (ctx < kVariantsMinContext || ctx > kVariantsMaxContext || r > kVariantsMaxAllele || k > kVariantsMaxAllele || r + k < 1 || p < 0 || p > L - r || L - r + k < 1) return;
    const int lo = max(0, p - ctx), hi = min(L - 1, p + r + ctx - 1), Pr = hi - lo + 1, Pa = Pr - r + k;      // (1 <= Pr, Pa <= 2 ctx + 16 <= 62)
    const int *st = starts + sr.start;
    const int t0 = min(max(st[lo], 0), N);
    const int t1 = min(max(hi < L - 1 ? st[hi + 1] - 1 : N, t0), N);           // (a path's starts give t0 <= t1 <= N; anything else reads no row outside the read)
    const unsigned short *sq = seq + sr.seq;
    const float *T = trans + map.row0(read, TbS) * (size_t)Ps;

    // ---- the states of both hypotheses at this lane's position
    const int a = lo + lane;                                                    // this lane's position, in s and in s^alt
    const int q0 = lane < Pr ? ff_state<NB>(sq[a]) : 0;                         // the coding of s itself
    const int myalt = lane < k ? vars[vi].v.alt[lane] : 0;                      // the alt allele, a letter a lane
    const int inside = __shfl(myalt, (a - p) & 63, 64);
    const int behind = __shfl(q0, (lane - k + r) & 63, 64);                     // the state of s at the position that stands here behind the edit
    const int la = a < p ? q0 % NB : a < p + k ? inside : behind % NB;          // this lane's alt letter
    int qa = lane >= Pa ? 0 : a < p ? q0 : behind;
    {
        int prev = p > 0 ? ff_state<NB>(sq[p - 1]) : -1;
        for (int x = p; x < lo + Pa; x++) {                                     // (uniform in the wave)
            const int now = ff_next<NB>(prev, __shfl(la, x - lo, 64));
            if (x >= p + k && now == __shfl(q0, x - k + r - lo, 64)) break;     // the coding of s from here on
            qa = a == x ? now : qa;
            prev = now;
        }
    }
    const int q[2] = { q0, qa };
    int is[2], im[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int below = __shfl_up(q[h], 1, 64);
        is[h] = ff_lookup(q[h], q[h], NB);
        im[h] = lane > 0 ? ff_lookup(below, q[h], NB) : 0;
    }

    win_real<ALL> X[2];
    window_scores<ALL>(T, Ps, t0, t1, is, im, lane, X);
    const float ref = (float)X[0], alt = __shfl((float)X[1], Pa - 1, 64);
    if (lane == Pr - 1) out[vi] = make_int4(head.y, t1 - t0, __float_as_int(ref), __float_as_int(alt));
}

void launch_variants(hipStream_t s, const SiteRead *list, int nread, const VarEntry *vars, int nvar, const unsigned short *seq, const float *trans, int Ps, int nbase,
                     int context, int all_paths, const void *records, const uint8_t *rm, int *starts, void *out, int Tb, const int *tbs, ReadMap map) {
    if (nread <= 0 || nvar <= 0 || (nbase != 4 && nbase != 5)) return;
    static_assert(sizeof(VarEntry) == 32 && offsetof(VarEntry, v) == 8 && offsetof(Variant, nref) == 4 && offsetof(Variant, alt) == 6, "k_variants reads an entry's first 16 bytes as one int4");
    const uint4 *rec = (const uint4 *)records;
    launch_site_starts(s, list, nread, records, rm, starts, Tb, tbs, map);
    const dim3 grid((nvar + kVrWaves - 1) / kVrWaves), block(kVrNT);
#define FFHIP_VR_LAUNCH(ALL, NB) hipLaunchKernelGGL((k_variants<ALL, NB>), grid, block, 0, s, list, vars, nvar, seq, trans, Ps, context, rec, starts, (int4 *)out, Tb, tbs, map)
    if (nbase == 5) { if (all_paths) FFHIP_VR_LAUNCH(true, 5); else FFHIP_VR_LAUNCH(false, 5); }
    else { if (all_paths) FFHIP_VR_LAUNCH(true, 4); else FFHIP_VR_LAUNCH(false, 4); }
#undef FFHIP_VR_LAUNCH
}

}  // namespace ffhip
