// ffhip_results.hpp -- the result block of a batch, described once (host only, no kernels; included by ffhip_engine.hip).
// What ffhip_batch_finish brings to the host is ONE block on the device and one pinned block on the host, moved in a single copy.  The two tables below are its
// whole description, fields (kResFields) and sections (kResSections): layout, growth, the bytes a run copies, every pointer and the f32 re-run's patching read them.
// To add a per-block byte section -- the move table is the example -- one writes
//   its field row     { "mv", RS_MOVES, 1, PER_BLOCK, PATCH_BLOCKS }
//   its section row   { "moves", RS_CORE, RS_MOD, FFHIP_RUN_MOVES, false, 0, 0, <the two error texts> }
//   its kernel call   launch_moves(.., b->res.on_dev<uint8_t>(RF_MV), ..)      (run_back)
//   its accessor      ffhip_batch_moves: b->res.on_host<uint8_t>(RF_MV) + read_row1(b, read)
// and nothing in the re-run, the growth or the copy size.
#pragma once
#include <algorithm>
#include <string.h>

#include "ffhip_host.hpp"

namespace ffhip {

enum ResSec { RS_HEAD, RS_CORE, RS_RUNS, RS_RECORDS, RS_MOD, RS_MOVES, RS_COUNT, RS_NONE = RS_COUNT };
enum ResField { RF_SAT, RF_ABORT, RF_LENS, RF_SCORE, RF_BASES, RF_QUALS, RF_NRUN, RF_FAIL, RF_LEN, RF_BASE, RF_EST, RF_SHAPE, RF_SCALE, RF_DWELL, RF_ML, RF_MV, RF_COUNT };
// entries of a field: a word per padded row (Bp), one 256-byte cell, one per read (cap_reads), one per row of the (Tb + 1)-row buffers (nread * (Tb + 1))
enum ResExtent { PER_ROW, ONE_CELL, PER_READ, PER_BLOCK };
// what the f32 re-run puts back for a read of nb blocks: nothing, its nb + 1 entries (a PER_READ field: its one entry), or nb entries
enum ResPatch { PATCH_NONE, PATCH_READ, PATCH_BLOCKS };

struct ResFieldRow { const char *name; ResSec sec; int elem; ResExtent ext; ResPatch patch; };      // (rows in ResField order: a section's fields lie in it one behind the other)
constexpr ResFieldRow kResFields[RF_COUNT] = {
    { "sat",   RS_HEAD,    4, PER_ROW,   PATCH_NONE },      // reads beyond the split format's range (a word a row)
    { "abort", RS_HEAD,    4, ONE_CELL,  PATCH_NONE },      // [0] abort word, [1] development counter, [2] packed convolution table overflow
    { "lens",  RS_CORE,    4, PER_READ,  PATCH_READ },
    { "score", RS_CORE,    4, PER_READ,  PATCH_READ },
    { "bases", RS_CORE,    1, PER_BLOCK, PATCH_READ },
    { "quals", RS_CORE,    1, PER_BLOCK, PATCH_READ },
    { "nrun",  RS_RUNS,    4, PER_READ,  PATCH_READ },
    { "fail",  RS_RUNS,    4, PER_READ,  PATCH_READ },
    { "len",   RS_RUNS,    8, PER_READ,  PATCH_READ },
    { "base",  RS_RUNS,    1, PER_BLOCK, PATCH_READ },
    { "est",   RS_RUNS,    4, PER_BLOCK, PATCH_READ },
    { "shape", RS_RECORDS, 4, PER_BLOCK, PATCH_READ },
    { "scale", RS_RECORDS, 4, PER_BLOCK, PATCH_READ },
    { "dwell", RS_RECORDS, 4, PER_BLOCK, PATCH_READ },
    { "ml",    RS_MOD,     1, PER_BLOCK, PATCH_READ },
    { "mv",    RS_MOVES,   1, PER_BLOCK, PATCH_BLOCKS },
};

// A section starts where `behind` ends -- or where `behind_held` ends, if the block holds that one.  `flags`: the run flags that ask for it; `always`: part of
// every block.  Which models may ask: the run-length model or the flip-flop models (`rle`), with `nbase` bases (0: any); model_text answers another model,
// undecoded_text FFHIP_RUN_NO_DECODE beside the flag.
struct ResSectionRow { const char *name; ResSec behind, behind_held; unsigned flags; bool always, rle; int nbase; const char *model_text, *undecoded_text; };
constexpr char kResRunsText[] = "run records: a decoded run of the run-length model (nbase 4) only";
constexpr ResSectionRow kResSections[RS_COUNT] = {
    { "head",    RS_NONE, RS_NONE, 0, true, false, 0, nullptr, nullptr },      // all a run without a decode brings down
    { "core",    RS_HEAD, RS_NONE, 0, true, false, 0, nullptr, nullptr },
    { "runs",    RS_CORE, RS_NONE, FFHIP_RUN_RLE_RUNS | FFHIP_RUN_RLE_RECORDS, false, true, 4, kResRunsText, kResRunsText },
    { "records", RS_RUNS, RS_NONE, FFHIP_RUN_RLE_RECORDS, false, true, 4, kResRunsText, kResRunsText },
    { "mod",     RS_CORE, RS_NONE, FFHIP_RUN_MOD_PROBS, false, false, 5, "5mC probabilities: a flip-flop model with a modified base (nbase 5) only",
      "5mC probabilities need a decoded run (FFHIP_RUN_NO_DECODE is set)" },
    { "moves",   RS_CORE, RS_MOD,  FFHIP_RUN_MOVES, false, false, 0, "move table: a flip-flop model only (the run-length model's run records carry dwells)",
      "the move table needs a decoded run (FFHIP_RUN_NO_DECODE is set)" },
};
// (runs and mod both start behind the core: a batch has one model and they ask for different ones -- `rle` -- so no block ever holds both)
constexpr unsigned res_bit(ResSec s) { return 1u << s; }
constexpr unsigned kResAlways = res_bit(RS_HEAD) | res_bit(RS_CORE);

// the sections a run with these flags fills, among those the block holds
inline unsigned res_sections_of(unsigned flags, unsigned held) {
    if (flags & FFHIP_RUN_NO_DECODE) return res_bit(RS_HEAD);
    unsigned v = kResAlways;
    for (int s = 0; s < RS_COUNT; s++) if (flags & kResSections[s].flags) v |= res_bit((ResSec)s);
    return v & (held | kResAlways);
}

// offsets in bytes of every field and the end of every section, for a block that holds the sections `held` (those it lacks: where they would be added)
struct ResLayout {
    size_t field[RF_COUNT], end[RS_COUNT];
    size_t end_of(unsigned sections) const { size_t n = 0; for (int s = 0; s < RS_COUNT; s++) if (sections & (1u << s)) n = std::max(n, end[s]); return n; }
};
inline ResLayout result_layout(int Bp, int cap_reads, int nread, int Tb, unsigned held) {
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };      // every part is 256-aligned
    const size_t count[4] = { (size_t)Bp, 0, (size_t)cap_reads, (size_t)nread * ((size_t)Tb + 1) };
    ResLayout o{};
    for (int s = 0; s < RS_COUNT; s++) {
        const ResSectionRow &sec = kResSections[s];
        size_t at = s == RS_HEAD ? 0 : o.end[(sec.behind_held != RS_NONE && (held & res_bit(sec.behind_held))) ? sec.behind_held : sec.behind];
        for (int f = 0; f < RF_COUNT; f++) {
            if (kResFields[f].sec != s) continue;
            o.field[f] = at;
            at += kResFields[f].ext == ONE_CELL ? 256 : up(count[kResFields[f].ext] * (size_t)kResFields[f].elem);
        }
        o.end[s] = at;
    }
    return o;
}

// The block itself: device half, pinned host half, what both hold now (`cap` bytes, the sections `held`) and where everything lies (`at`).
struct ResultBlock {
    int Bp = 0, cap_reads = 0, nread = 0, Tb = 0;
    unsigned char *dev = nullptr, *host = nullptr;
    size_t cap = 0;
    unsigned held = 0;
    ResLayout at{};

    template <class T> T *on_dev(ResField f) const { return (T *)(dev + at.field[f]); }
    template <class T> T *on_host(ResField f) const { return (T *)(host + at.field[f]); }

    int create(int Bp_, int cap_reads_, int nread_, int Tb_, hipStream_t stream) { Bp = Bp_; cap_reads = cap_reads_; nread = nread_; Tb = Tb_; return hold(kResAlways, stream); }      // a new batch: the sections every block has
    // the block with section s as well, grown on the first run that asks for it (a section that comes to lie in front of one the block holds moves that one back:
    // results are rewritten by every run).  Nothing is marked before the grow has succeeded: a failure leaves the block as it was.
    int ensure(ResSec s, hipStream_t stream) { return (held & res_bit(s)) ? FFHIP_OK : hold(held | res_bit(s), stream); }
    // the prefix a finished run with these flags brings down: the smallest that covers the sections it filled (so a block that holds ml copies it with moves alone)
    size_t copy_bytes(unsigned flags) const { return at.end_of(res_sections_of(flags, held)); }
    void release() { if (dev) hipFree(dev); if (host) hipHostFree(host); dev = host = nullptr; cap = 0; held = 0; }

private:
    int hold(unsigned sections, hipStream_t stream) {
        const ResLayout o = result_layout(Bp, cap_reads, nread, Tb, sections);
        if (int rc = grow(o.end_of(sections), stream)) return rc;
        held = sections; at = o;
        return FFHIP_OK;
    }
    // both halves grown to `need` bytes, their contents kept (a packed batch's set-up writes into the block before the run), the rest zero
    int grow(size_t need, hipStream_t stream) {
        if (cap >= need) return FFHIP_OK;
        HIP_TRY(hipStreamSynchronize(stream), FFHIP_EHIP);
        unsigned char *d = nullptr, *h = nullptr;
        if (hipMalloc((void **)&d, need) != hipSuccess) return set_err(FFHIP_ENOMEM, "hipMalloc of %zu bytes failed", need);
        if (hipHostMalloc((void **)&h, need) != hipSuccess) { hipFree(d); return set_err(FFHIP_ENOMEM, "pinned host allocation failed"); }
        memset(h + cap, 0, need - cap);
        if (cap) memcpy(h, host, cap);
        if (hipMemsetAsync(d + cap, 0, need - cap, stream) != hipSuccess ||
            (cap && hipMemcpyAsync(d, dev, cap, hipMemcpyDeviceToDevice, stream) != hipSuccess) || hipStreamSynchronize(stream) != hipSuccess) {
            hipFree(d); hipHostFree(h); return set_err(FFHIP_EHIP, "copy of the result block failed");
        }
        release();
        dev = d; host = h; cap = need;
        return FFHIP_OK;
    }
};

}  // namespace ffhip
