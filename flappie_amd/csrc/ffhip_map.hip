// ffhip_map.hip -- every call placed on a small reference (FFHIP_RUN_MAP, include/ffhip.h "map"): the call is the pattern, the reference the text, both strands.
//
// A reference is K records over ACGT, on the device once as 2-bit codes (A 0, C 1, G 2, T 3), 16 a word, one record behind the other with a word of padding at either
// end; search q = 2 k + o reads record k as given (o = 0) or backwards and complemented (o = 1, 3 - code) from the same words.  An anchor is the first or the last
// min(n, W) letters of a call in signal order, Z read as C: L <= 4096 rows, so up to 64 words of 64 rows.  d_{a,q}[j] = D[L][j] of the infix edit distance
// (D[0][j] = 0, D[i][0] = i, unit costs).  All of it is integer arithmetic: exact.
//
// k_map_scan: Myers' recurrence in Hyyro's block form (myers_step, ffhip_seq.hpp) over MANY words.  Word w of an anchor is worked by lane w of a LANE GROUP of G lanes, G the
// next power of two >= ceil(L / 64): a wave holds 64 / G tasks.  Lane w is one column behind lane w - 1: at step t it works column t - w, and the horizontal
// difference (-1, 0, +1) that left word w - 1 at that column a step ago enters it through a lane shuffle, the column's letter with it (two bits more of the same
// word) -- only lane 0 of a group reads the reference, 16 letters a load, the next load under way while these are worked.  Nothing goes through LDS or memory.
//   task:  (read, anchor, segment of one search's text).  The reference's task list is built at upload: search q cut into segments of kMapSeg = FFHIP_MAP_SEGMENT
//          columns; segment g owns the ends j in (g S, (g + 1) S], the first one j = 0 too.  A task starts fresh (D[i][a] = i) at a = max(0, g S - 2 L): d <= L and
//          an optimal match spans at most L + d <= 2 L columns, so it is exact from a + 2 L on.  The tasks of a (read, anchor) are dealt to gridDim.y waves.
//   best:  the last word's lane follows d at bit (L - 1) % 64 and keeps the smallest d of the owned columns, the leftmost of equals; it leaves (d, j) in the task's
//          own slot of the workspace.  No atomics.
// k_map_finish: one wave a read.  Tasks are listed by (q, segment), so the smallest (d, task) IS the smallest (d, q, j): a wave minimum over the slots; `second` is a
//   wave minimum of d over the tasks of the other searches.  The start: the reversed anchor against y[j-1], y[j-2], ... with an anchored start (+1 enters word 0
//   at every column), the same lane pipeline with one group of 64 lanes, until D[L][c] = d; c <= 2 L.  Then the bound, the pairing rule, and the record as four
//   16-byte stores.
// k_map_stretch (include/ffhip.h "truth from map"): one wave an entry of truth's read list, behind k_map_finish: the mapped read's stretch of the reference as codes
//   where k_truth reads its truth, and the entry's length and status patched.  Its own comment stands in front of it.
// k_map_remap_seq (include/ffhip.h "remap from map"): the same for an entry of remap's read list, the stretch in remap's flip-flop coding where k_remap reads its sequence.
#include "ffhip_internal.hpp"
#include "ffhip_seq.hpp"

namespace ffhip {

static_assert(kMapMaxAnchor == 64 * 64 && (kMapSeg % 16) == 0 && kMapPad == 16, "an anchor is at most a wave of words; letters are read 16 a word");

// 16 letters of a strand as 2-bit codes, the first in bits 0-1: those at g, g + 1, ... (dir > 0) or g, g - 1, ... (dir < 0) of the reference, complemented if comp.
// g - 15 >= -kMapPad and g + 15 < total + kMapPad: the words hold a word of padding either side (map_ref_upload).
__device__ __forceinline__ unsigned map_chunk(const unsigned *__restrict__ words, long long g, int dir, bool comp) {
    const long long p = (dir > 0 ? g : g - 15) + kMapPad;
    const unsigned long long two = (unsigned long long)words[p >> 4] | ((unsigned long long)words[(p >> 4) + 1] << 32);
    unsigned v = (unsigned)(two >> (2 * (int)(p & 15)));
    if (dir < 0) { v = __brev(v); v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1); }      // the letters in reverse order, each letter's two bits as they were
    return comp ? ~v : v;
}

// the match masks of word w of an anchor p of L letters (rev: of the reversed anchor)
__device__ __forceinline__ void map_masks(const char *__restrict__ p, int L, int w, bool rev, unsigned long long peq[4]) {
    peq[0] = peq[1] = peq[2] = peq[3] = 0ull;
    for (int i = 0; i < 64; i++) {
        const int r = 64 * w + i;
        if (r >= L) break;
        const unsigned c = seq_code(p[rev ? L - 1 - r : r]);
        const unsigned long long bit = 1ull << i;
        peq[0] |= c == 0 ? bit : 0ull; peq[1] |= c == 1 ? bit : 0ull; peq[2] |= c == 2 ? bit : 0ull; peq[3] |= c == 3 ? bit : 0ull;
    }
}

__device__ __forceinline__ int map_anchor_len(int n, int window) { return n < window ? n : window; }

template <bool SCORES>
__global__ void __launch_bounds__(64)
k_map_scan(MapRefView ref, const char *__restrict__ bases, const int *__restrict__ lens, int TbS, const int *__restrict__ tbs, ReadMap map, int window,
           int2 *__restrict__ slots, int *__restrict__ d_out) {
    FFHIP_DECODE_PRIO_SET();
    const int read = blockIdx.x >> 1, anchor = blockIdx.x & 1, lane = threadIdx.x;
    const int Tb = tbs ? tbs[read] : TbS;
    if (Tb <= 0) return;                                 // an empty slot: no call (k_map_finish writes its record)
    const int n = lens[read] > 0 ? lens[read] : 0;
    if (n == 0 || (anchor == 1 && n <= window)) return;  // no call, or the rear anchor is the front one
    const int L = map_anchor_len(n, window), nw = (L + 63) >> 6;
    int G = 1;
    while (G < nw) G <<= 1;
    const int w = lane & (G - 1), per_wave = 64 / G, top = (L - 1) & 63;
    const char *p = bases + map.row1(read, TbS) + (anchor ? n - L : 0);
    unsigned long long peq[4];
    map_masks(p, L, w, false, peq);
    const bool last = w == nw - 1, idle = w >= nw;
    int2 *myslots = slots + (size_t)blockIdx.x * ref.ntask;
    for (int task0 = blockIdx.y * per_wave; task0 < ref.ntask; task0 += gridDim.y * per_wave) {      // (uniform over the wave)
        const int task = task0 + lane / G;
        const bool have = task < ref.ntask && !idle;
        const MapTask tk = have ? ref.tasks[task] : MapTask{ 0, 0, 0, 0 };
        const int2 rc = have ? ref.recs[tk.q >> 1] : make_int2(0, 1);      // { first letter, letters }
        const int a = have ? (tk.s - 2 * L > 0 ? tk.s - 2 * L : 0) : 0;     // the fresh start
        const int ncol = have ? tk.e - a : 0;                               // letters a .. e - 1, ends a + 1 .. e
        const int o = tk.q & 1, dir = o ? -1 : 1;
        const long long g0 = o ? (long long)rc.x + rc.y - 1 - a : (long long)rc.x + a;      // the reference letter of column a
        int *drow = (SCORES && have && last) ? d_out + ref.rowoff[tk.q] : nullptr;
        unsigned long long pv = ~0ull, mv = 0ull;
        int score = L, bd = tk.s == 0 ? L : 0x7fffffff, bj = 0;             // d[0] = L belongs to the first segment
        if (SCORES) { if (drow && tk.s == 0) drow[0] = L; }
        int carry = 1;                                   // what this lane hands on: (difference + 1) | letter << 2
        unsigned cur = (have && w == 0 && ncol > 0) ? map_chunk(ref.words, g0, dir, o) : 0u;
        const int nstep = have ? ncol + w : 0;           // this lane's steps: t = w .. ncol + w - 1
        for (int t0 = 0; __any(t0 < nstep); t0 += 16) {
            const unsigned nxt = (have && w == 0 && t0 + 16 < ncol) ? map_chunk(ref.words, g0 + (long long)dir * (t0 + 16), dir, o) : 0u;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int t = t0 + i, col = t - w;
                const int in = __shfl_up(carry, 1, G);  // lane w - 1's column t - w of a step ago (lane 0 of a group: its own, not used)
                if (have && col >= 0 && col < ncol) {
                    const unsigned c = w == 0 ? (cur >> (2 * i)) & 3u : (unsigned)in >> 2;
                    const int hin = w == 0 ? 0 : (in & 3) - 1;
                    const int hout = myers_diff(myers_step(pv, mv, myers_eq(peq, c), hin), last ? top : 63);      // what leaves the word, or its last row
                    carry = (hout + 1) | (int)(c << 2);
                    if (last) {
                        score += hout;
                        const int j = a + col + 1;
                        if (j > tk.s) {
                            if (score < bd) { bd = score; bj = j; }
                            if (SCORES) { if (drow) drow[j] = score; }
                        }
                    }
                }
            }
            cur = nxt;
        }
        if (have && last) myslots[task] = make_int2(bd, bj);
    }
}

// start of the place (q, j, d) of the anchor p of L letters: the reversed anchor against y_q[j-1], y_q[j-2], ... from an anchored start, until D[L][c] = d; one
// wave, lane w the word w.  The same in every lane.
__device__ __forceinline__ int map_start(const MapRefView &ref, const char *__restrict__ p, int L, int q, int j, int d, int lane) {
    const int nw = (L + 63) >> 6, top = (L - 1) & 63, w = lane;
    const bool last = w == nw - 1, idle = w >= nw;
    unsigned long long peq[4], pv = ~0ull, mv = 0ull;
    map_masks(p, L, w, true, peq);
    const int2 rc = ref.recs[q >> 1];
    const int o = q & 1, dir = o ? 1 : -1;               // y_q backwards: the record backwards (o = 0), or forwards and complemented
    const long long g0 = o ? (long long)rc.x + rc.y - j : (long long)rc.x + j - 1;
    const int ncol = j < 2 * L ? j : 2 * L;
    int score = L, carry = 1, found = d == L ? 0 : -1;   // (c = 0: D[L][0] = L)
    unsigned cur = (w == 0 && ncol > 0) ? map_chunk(ref.words, g0, dir, o) : 0u;
    for (int t0 = 0; t0 < ncol + nw - 1 && !__any(found >= 0); t0 += 16) {
        const unsigned nxt = (w == 0 && t0 + 16 < ncol) ? map_chunk(ref.words, g0 + (long long)dir * (t0 + 16), dir, o) : 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int t = t0 + i, col = t - w;
            const int in = __shfl_up(carry, 1, 64);
            if (!idle && col >= 0 && col < ncol) {
                const unsigned c = w == 0 ? (cur >> (2 * i)) & 3u : (unsigned)in >> 2;
                const int hin = w == 0 ? 1 : (in & 3) - 1;
                const int hout = myers_diff(myers_step(pv, mv, myers_eq(peq, c), hin), last ? top : 63);      // what leaves the word, or its last row
                carry = (hout + 1) | (int)(c << 2);
                if (last) {
                    score += hout;
                    if (score == d && found < 0) found = col + 1;
                }
            }
        }
        cur = nxt;
    }
    const int c = __shfl(found, nw - 1, 64);
    return j - (c < 0 ? ncol : c);                       // (c < 0 cannot be: ed(p, y[i:j]) = d for some i >= j - 2 L)
}

__global__ void __launch_bounds__(64)
k_map_finish(MapRefView ref, const char *__restrict__ bases, const int *__restrict__ lens, int TbS, const int *__restrict__ tbs, ReadMap map, int window, int max_error,
             const int2 *__restrict__ slots, uint4 *__restrict__ rec) {
    FFHIP_DECODE_PRIO_SET();
    const int read = blockIdx.x, lane = threadIdx.x;
    uint4 *out = rec + (size_t)read * 4;
    const int Tb = tbs ? tbs[read] : TbS;
    const int n = Tb > 0 && lens[read] > 0 ? lens[read] : 0;
    if (n == 0) {                                        // an empty slot, or no call
        if (lane < 4) out[lane] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int na = n <= window ? 1 : 2, L = map_anchor_len(n, window);
    const int md = (int)((long long)L * max_error / 1000);
    const char *x = bases + map.row1(read, TbS);
    int aq[2], as[2], ae[2], ad[2], a2[2];
    for (int a = 0; a < na; a++) {
        const int2 *sl = slots + ((size_t)read * 2 + a) * ref.ntask;
        unsigned long long key = ~0ull;
        for (int t = lane; t < ref.ntask; t += 64) {
            const unsigned long long k = ((unsigned long long)(unsigned)sl[t].x << 32) | (unsigned)t;
            key = k < key ? k : key;
        }
        key = wave_min(key);
        const int bt = (int)(unsigned)key, d = (int)(key >> 32), q = ref.tasks[bt].q, j = sl[bt].y;
        unsigned long long k2 = ~0ull;
        for (int t = lane; t < ref.ntask; t += 64)
            if (ref.tasks[t].q != q) { const unsigned long long k = (unsigned long long)(unsigned)sl[t].x; k2 = k < k2 ? k : k2; }
        k2 = wave_min(k2);
        aq[a] = q; ae[a] = j; ad[a] = d; a2[a] = (int)k2;
        as[a] = map_start(ref, x + (a ? n - L : 0), L, q, j, d, lane);
    }
    if (na == 1) { aq[1] = aq[0]; as[1] = as[0]; ae[1] = ae[0]; ad[1] = ad[0]; a2[1] = a2[0]; }
    int status = 1;
    if (ad[0] > md || ad[1] > md) status = 2;
    else if (na == 2) {
        const long long span = (long long)ae[1] - as[0], off = span > n ? span - n : n - span;
        if (aq[0] != aq[1] || as[0] >= ae[1] || off > (long long)n * max_error / 1000) status = 3;
    }
    const bool ok = status == 1;
    if (lane == 0) out[0] = make_uint4((unsigned)status, (unsigned)n, (unsigned)na, ok ? (unsigned)aq[0] : 0u);
    else if (lane == 1) out[1] = make_uint4(ok ? (unsigned)as[0] : 0u, ok ? (unsigned)ae[1] : 0u, (unsigned)aq[0], (unsigned)as[0]);
    else if (lane == 2) out[2] = make_uint4((unsigned)ae[0], (unsigned)ad[0], (unsigned)a2[0], (unsigned)aq[1]);
    else if (lane == 3) out[3] = make_uint4((unsigned)as[1], (unsigned)ae[1], (unsigned)ad[1], (unsigned)a2[1]);
}

// k_map_stretch (include/ffhip.h "truth from map"): one wave an entry of truth's read list, all forms' entries in one launch, behind k_map_finish and ahead of the
// k_truth launches.  A read whose map record says status 1 gets its stretch y_q[tstart : tend] as codes 0 .. 3 at seq + entry.seq, m = tend - tstart of them, read
// with map_chunk in the orientation of q as the scan reads it; a lane takes one letter of 64 a pass, so a pass is one store of 64 bytes in a row.  Lane 0 then
// patches the entry's m and status in the list, which k_truth reads.  entry.room is the read's share of `seq` (the bound): m > room, or a record that does not lie
// in its reference record, is status 2 and writes no code.  An entry of status 0 (an empty slot) is left as it is.  Integers only, no atomics.
__global__ void __launch_bounds__(64)
k_map_stretch(MapRefView ref, const uint4 *__restrict__ rec, TruthRead *__restrict__ list, uint8_t *__restrict__ seq) {
    FFHIP_DECODE_PRIO_SET();
    const int lane = threadIdx.x;
    TruthRead *e = list + blockIdx.x;
    const TruthRead tr = *e;                             // (read whole before lane 0 patches it)
    if (tr.status != 1) return;                          // an empty slot
    const uint4 *r = rec + (size_t)tr.read * 4;
    const uint4 r0 = r[0], r1 = r[1];
    const int mstatus = (int)r0.x, q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y, room = tr.room;
    int status = 0, m = 0;
    if (mstatus == 1) {
        status = 2;
        if (q >= 0 && q < 2 * ref.nrec) {
            const int2 rc = ref.recs[q >> 1];                // { first letter, letters }
            if (ts >= 0 && ts < te && te <= rc.y) {
                m = te - ts;
                if (m <= room) {
                    status = 1;
                    const int o = q & 1, dir = o ? -1 : 1;
                    const long long g0 = o ? (long long)rc.x + rc.y - 1 - ts : (long long)rc.x + ts;      // the reference letter of y_q[tstart]
                    uint8_t *out = seq + tr.seq;
                    for (int i = lane; i < m; i += 64) {
                        const unsigned v = map_chunk(ref.words, g0 + (long long)dir * (i & ~15), dir, o);
                        out[i] = (uint8_t)((v >> (2 * (i & 15))) & 3u);
                    }
                }
            }
        }
    }
    if (lane == 0) { e->m = m; e->status = status; }
}

void launch_map_stretch(hipStream_t s, const MapRefView &ref, const void *records, TruthRead *list, int count, uint8_t *seq) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_map_stretch, dim3(count), dim3(64), 0, s, ref, (const uint4 *)records, list, seq);
}

// k_map_remap_seq (include/ffhip.h "remap from map"): k_map_stretch's twin for remap, one wave an entry of remap's read list, all forms' entries in one launch, behind
// k_map_finish and ahead of the k_remap launches.  A read whose map record says status 1 gets its stretch y_q[tstart : tend] in remap's coding at seq + entry.seq, m =
// tend - tstart entries of 16 bits: stay (q_i -> q_i) | move (q_{i-1} -> q_i) << 8, byte for byte what remap_code makes on the host.  q_i = s_i + nbase * ((i -
// runstart_i) & 1).  A lane takes one letter of 64 a pass.  One ballot of s_i != s_{i-1} marks the pass's run starts, and the highest mark at or below a lane is its
// own; with no mark there the run began in an earlier pass, and its start comes with the carry (the last run start, letter and q of the pass before: the same in every
// lane).  q_{i-1} is one cross-lane move, or the carry for lane 0.  Lane 0 then patches the entry's L and status, which k_remap reads.  The room of an entry is the
// N + 1 positions a path of the read's N blocks can hold: m > room is status 2 with L = m and no entry written, as is a record that does not lie in its reference
// record (L = 0); a read the map did not place is status 0.  An entry of status 0 (an empty slot) is left as it is.  Integers only, no atomics, no LDS.
__global__ void __launch_bounds__(64)
k_map_remap_seq(MapRefView ref, const uint4 *__restrict__ rec, RemapRead *__restrict__ list, unsigned short *__restrict__ seq, int nbase, int TbS, const int *__restrict__ tbs) {
    FFHIP_DECODE_PRIO_SET();
    const int lane = threadIdx.x;
    RemapRead *e = list + blockIdx.x;
    const RemapRead rr = *e;                             // (read whole before lane 0 patches it)
    if (rr.status != 1) return;                          // an empty slot
    const uint4 *r = rec + (size_t)rr.read * 4;
    const uint4 r0 = r[0], r1 = r[1];
    const int mstatus = (int)r0.x, q = (int)r0.w, ts = (int)r1.x, te = (int)r1.y;
    const int N = tbs ? tbs[rr.read] : TbS;
    const long long room = (long long)N + 1;
    int status = 0, m = 0;
    if (mstatus == 1) {
        status = 2;
        if (q >= 0 && q < 2 * ref.nrec) {
            const int2 rc = ref.recs[q >> 1];                // { first letter, letters }
            if (ts >= 0 && ts < te && te <= rc.y) {
                m = te - ts;
                if (m <= room) {
                    status = 1;
                    const int o = q & 1, dir = o ? -1 : 1;
                    const long long g0 = o ? (long long)rc.x + rc.y - 1 - ts : (long long)rc.x + ts;      // the reference letter of y_q[tstart]
                    unsigned short *out = seq + rr.seq;
                    int c_start = 0, c_s = -1, c_q = 0;      // the carry: nothing stands in front of position 0
                    for (int i0 = 0; i0 < m; i0 += 64) {     // (uniform over the wave)
                        const int i = i0 + lane;
                        const bool have = i < m;
                        int s = 0;
                        if (have) {
                            const unsigned v = map_chunk(ref.words, g0 + (long long)dir * (i & ~15), dir, o);
                            s = (int)((v >> (2 * (i & 15))) & 3u);
                        }
                        const int below = __shfl_up(s, 1, 64);
                        const int sp = lane == 0 ? c_s : below;
                        const unsigned long long marks = __ballot(have && s != sp);
                        const unsigned long long mine = marks & (~0ull >> (63 - lane));      // the marks at or below this lane
                        const int start = mine ? i0 + 63 - __clzll((long long)mine) : c_start;
                        const int qi = s + nbase * ((i - start) & 1);
                        const int qb = __shfl_up(qi, 1, 64);
                        const int qp = lane == 0 ? c_q : qb;
                        if (have) out[i] = (unsigned short)(ff_lookup(qi, qi, nbase) | ((i > 0 ? ff_lookup(qp, qi, nbase) : 0) << 8));
                        c_start = marks ? i0 + 63 - __clzll((long long)marks) : c_start;      // (a full pass, or the last one: lane 63's letter is real wherever it is read)
                        c_s = __shfl(s, 63, 64);
                        c_q = __shfl(qi, 63, 64);
                    }
                }
            }
        }
    }
    if (lane == 0) { e->L = m; e->status = status; }
}

void launch_map_remap_seq(hipStream_t s, const MapRefView &ref, const void *records, RemapRead *list, int count, unsigned short *seq, int nbase, int Tb, const int *tbs) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_map_remap_seq, dim3(count), dim3(64), 0, s, ref, (const uint4 *)records, list, seq, nbase, Tb, tbs);
}

const char *map_invalid(int window, int max_error) {
    if (window >= 0 && (window < 64 || window > kMapMaxAnchor)) return "window is 64 .. 4096 bases";
    if (max_error > 500) return "max_error is 0 .. 500 per mille";
    return nullptr;
}

void launch_map(hipStream_t s, const MapRefView &ref, const char *bases, const int *lens, void *records, int nread, int Tb, const int *tbs, ReadMap map, int window,
                int max_error, void *slots, int *d_out) {
    if (nread <= 0) return;
    const dim3 grid(2 * nread, ref.ntask < kMapWavesY ? ref.ntask : kMapWavesY);
    if (d_out) hipLaunchKernelGGL(k_map_scan<true>, grid, dim3(64), 0, s, ref, bases, lens, Tb, tbs, map, window, (int2 *)slots, d_out);
    else hipLaunchKernelGGL(k_map_scan<false>, grid, dim3(64), 0, s, ref, bases, lens, Tb, tbs, map, window, (int2 *)slots, d_out);
    hipLaunchKernelGGL(k_map_finish, dim3(nread), dim3(64), 0, s, ref, bases, lens, Tb, tbs, map, window, max_error, (const int2 *)slots, (uint4 *)records);
}

}  // namespace ffhip
