// ffhip_features.hip -- host side of the per-read features (barcodes, adapters, map, poly tail, remap, events, site mods, variants, truth, truth from map, pileup, mod pileup, consensus):
// each feature's share of a batch's run (ffhip_annot.hpp), its device objects, setters and accessors (include/ffhip.h), and its single-read operator ffhip_op_*.
// No kernel lives here (theirs are ffhip_barcodes.hip ... ffhip_variants.hip) and none is launched from here but through their launch_* functions, so the Makefile
// compiles this file as C++.  ffhip_engine.hip reaches it through ffhip_annot.hpp only.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "ffhip_batch.hpp"

// ---- each check once: what a setter, a run's front and a single-read operator all ask is asked here; where their texts differ, the caller words its own refusal
static size_t bad_letter(const char *s, size_t len) { size_t i = 0; while (i < len && s[i] && strchr("ACGTZ", s[i])) i++; return i; }      // the first character of a call that is not one of ACGTZ, or len
static size_t bad_code(const uint8_t *c, size_t len, int nbase) { size_t i = 0; while (i < len && c[i] < nbase) i++; return i; }         // the first code that is no base of nbase, or len
static int acgt_index(char c) { const char *at = strchr("ACGT", c); return at ? (int)(at - "ACGT") : -1; }                                // a pattern's or a reference's letter (never NUL)
// a kit's patterns, n of 1 .. maxlen letters of ACGT each: their lengths, and enter(k, i, c, L) for letter i, of index c, of pattern k of L letters
template <class Enter> static bool kit_patterns(const char *who, int n, const char *const *seq, int maxlen, int *len, Enter enter) {
    for (int k = 0; k < n; k++) {
        const size_t L = seq[k] ? strnlen(seq[k], (size_t)maxlen + 1) : 0;
        if (L < 1 || L > (size_t)maxlen) { set_err(FFHIP_EINVAL, "%s %d: a pattern has 1 .. %d bases", who, k, maxlen); return false; }
        for (size_t i = 0; i < L; i++) {
            const int c = acgt_index(seq[k][i]);
            if (c < 0) { set_err(FFHIP_EINVAL, "%s %d: character %zu is not one of ACGT", who, k, i); return false; }
            enter((size_t)k, i, (size_t)c, L);
        }
        len[k] = (int)L;
    }
    return true;
}
static int path_check(const char *who, const uint8_t *rm, size_t nblock, size_t L) {       // a move path: nblock bytes of 0 or 1 that move L - 1 times
    size_t ones = 0;
    for (size_t i = 0; i < nblock; i++) {
        if (rm[i] > 1) return set_err(FFHIP_EINVAL, "%s: block %zu of the path is %d (0 or 1)", who, i, (int)rm[i]);
        ones += rm[i];
    }
    return ones != L - 1 ? set_err(FFHIP_EINVAL, "%s: the path moves %zu times, a sequence of %zu bases takes %zu", who, ones, L, L - 1) : FFHIP_OK;
}
static int truth_band_check(const char *who, int band) {
    if (band >= 0 && band <= truth_max_band()) return FFHIP_OK;
    return set_err(FFHIP_EINVAL, "%s: the band half-width is %d (0 .. %d: the widest kernel form holds a window of %d cells)", who, band, truth_max_band(), truth_max_window());
}
static int span_check(const char *who, const ffhip_map_ref *ref, int q, int start, int end) {      // q is a search of the reference, [start, end) a span of its record
    if (q < 0 || q >= 2 * ref->view.nrec) return set_err(FFHIP_EINVAL, "%s: search %d is not one of 0 .. %d", who, q, 2 * ref->view.nrec - 1);
    const int mk = ref->rec_len[(size_t)q >> 1];
    return start < 0 || end > mk || start >= end ? set_err(FFHIP_EINVAL, "%s: [%d, %d) is not a span of 1 or more of the record's %d bases", who, start, end, mk) : FFHIP_OK;
}
static bool trans_ok(const ffhip_mat &t, int nbase) { return view_ok(t) && t.nr == (size_t)(2 * nbase * (nbase + 1)) && t.stride % 4 == 0 && t.stride <= 2048; }      // scores as remap, site mods and variants take them
static void truth_unpack(const int rec[kTruthRecInts], ffhip_truth_call *out) {      // a truth record as k_truth wrote it; the ops are the caller's
    out->status = rec[0]; out->n = (size_t)rec[1]; out->m = (size_t)rec[2]; out->dist = rec[3];
    out->n_match = rec[4]; out->n_mismatch = rec[5]; out->n_ins = rec[6]; out->n_del = rec[7];
    out->maxdev = rec[8]; out->nops = (size_t)rec[9]; out->ops = nullptr;
}
// where read r's first sample stands in sbuf[0], in floats (st: total_stride)
static size_t signal_at(const ffhip_batch *b, int r, int st) { return (b->packed ? (size_t)b->v_slot[r] * b->sbuf[0].rs + (size_t)b->v_off[r] * st : (size_t)r * b->sbuf[0].rs) + kSamplePad; }
static PolyTailParams polytail_params(const ffhip_polytail_params *params) { PolyTailParams p; memcpy(&p, params, sizeof p); return p; }      // the kernel's view of them
// what a negative parameter stands for, to a batch's setter and to the single-read operator
static int barcodes_max_dist(const ffhip_barcodes *kit, int d) { return d < 0 ? kit->lmin / 4 : d; }
static int barcodes_min_sep(int v) { return v < 0 ? 3 : v; }
static int adapters_max_dist(int d) { return d < 0 ? -1 : std::min(d, kAdapterMaxLen - 1); }
static void map_defaults(int *window, int *max_error) { if (*window < 0) *window = kMapMaxAnchor; if (*max_error < 0) *max_error = 250; }
static int op_done(hipStream_t s) {      // an operator's end: its kernels have run, and whether they ran
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    HIP_TRY(hipGetLastError(), FFHIP_EHIP);
    return FFHIP_OK;
}
// A device object's buffers: each allocated and -- host != nullptr -- filled; at the first failure all are given back (dev_free: as at the object's end), the text set
struct DevBuf { void **dev; const void *host; size_t bytes; };
static void dev_free(std::initializer_list<void **> bufs) { for (void **p : bufs) { if (*p) hipFree(*p); *p = nullptr; } }
static int dev_fill(const char *what, std::initializer_list<DevBuf> bufs) {
    int rc = FFHIP_OK;
    for (auto u = bufs.begin(); u != bufs.end() && !rc; u++) {
        if (hipMalloc(u->dev, u->bytes) != hipSuccess) { *u->dev = nullptr; rc = set_err(FFHIP_ENOMEM, "device allocation failed"); }
        else if (u->host && hipMemcpy(*u->dev, u->host, u->bytes, hipMemcpyHostToDevice) != hipSuccess) rc = set_err(FFHIP_EHIP, "upload of the %s failed", what);
    }
    if (rc) for (const DevBuf &u : bufs) dev_free({ u.dev });
    return rc;
}

// ---- the per-read products outside the result block (ffhip_annot.hpp).  Per feature: its share of the front (prepare: checks of its own, lists, workspaces, room
// for the records), its share of the back (launch), what a finished run brings down (bytes) and where a read's record lies (spans); kAnnots, the table, at the end.
static void span1(AnnotSpan out[2], size_t at, size_t bytes) { out[0] = AnnotSpan{ at, bytes }; out[1] = AnnotSpan{}; }
// barcodes, adapters, the map and the poly tail: one record of REC bytes a read
template <size_t REC> static size_t fixed_bytes(const ffhip_batch *b) { return (size_t)batch_nreads(b) * REC; }
template <size_t REC> static void fixed_spans(const ffhip_batch *, int r, AnnotSpan out[2]) { span1(out, (size_t)r * REC, REC); }

static_assert(sizeof(ffhip_barcode_call) == 16, "k_barcodes writes a record as one 16-byte store");
static int barcodes_prepare(ffhip_batch *b) {
    if (!b->bc.kit) return set_err(FFHIP_EINVAL, "barcodes: no kit is attached to the batch (ffhip_batch_set_barcodes)");
    return b->bc.rec.fixed(b, (size_t)b->cap_reads * sizeof(ffhip_barcode_call), "barcodes: the reads' records");
}
static void barcodes_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // from the strings and lengths k_assemble has just written
    launch_barcodes(b->stream, b->bc.kit->kit, b->bases(), b->lens(), b->bc.rec.dev, batch_nreads(b), b->Tb, tbr, rmap, b->bc.max_dist, b->bc.min_sep, b->bc.both);
    b->launches[5]++;
    b->bc.valid = 1;
}

static_assert(sizeof(ffhip_adapter_header) == 16 && sizeof(ffhip_adapter_hit) == 16 && FFHIP_ADAPTER_SEGMENT == kAdSeg && FFHIP_ADAPTER_MAX_HITS == kAdapterMaxHits,
              "k_adapters writes a header and a hit as one 16-byte store each");
static int adapters_prepare(ffhip_batch *b) {
    if (!b->ad.kit) return set_err(FFHIP_EINVAL, "adapters: no kit is attached to the batch (ffhip_batch_set_adapters)");
    return b->ad.rec.fixed(b, (size_t)b->cap_reads * kAdapterRecBytes, "adapters: the reads' records");
}
static void adapters_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // likewise
    launch_adapters(b->stream, b->ad.kit->kit, b->bases(), b->lens(), b->ad.rec.dev, batch_nreads(b), b->Tb, tbr, rmap, b->ad.max_dist);
    b->launches[5]++;
    b->ad.valid = 1;
}

static_assert(sizeof(ffhip_map_call) == kMapRecBytes && FFHIP_MAP_SEGMENT == kMapSeg && FFHIP_MAP_MAX_TOTAL == kMapMaxTotal && FFHIP_MAP_MAX_ANCHOR == kMapMaxAnchor,
              "k_map_finish writes a record as four 16-byte stores");
static int map_prepare(ffhip_batch *b) {
    ffhip_batch::Map &f = b->map;
    if (!f.ref) return set_err(FFHIP_EINVAL, "map: no reference is attached to the batch (ffhip_batch_set_map)");
    if (int rc = f.rec.fixed(b, (size_t)b->cap_reads * kMapRecBytes, "map: the reads' records")) return rc;
    return dgrow(b, &f.ws, &f.ws_cap, (size_t)b->cap_reads * 2 * (size_t)f.ref->view.ntask * 8, "map: the tasks' slots");
}
static void map_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // from the strings and lengths, as barcodes and adapters
    ffhip_batch::Map &f = b->map;
    launch_map(b->stream, f.ref->view, b->bases(), b->lens(), f.rec.dev, batch_nreads(b), b->Tb, tbr, rmap, f.window, f.max_error, f.ws);
    b->launches[5] += 2;
    f.valid = 1;
}

// Poly tail, the front's share: every read's samples (the addresses events_prepare gives) and its first window in the workspace, which grows here
static_assert(sizeof(ffhip_polytail) == kPolyTailRecBytes && sizeof(ffhip_polytail_params) == sizeof(PolyTailParams) && sizeof(PolyRead) == 24,
              "k_polytail writes a record as two 16-byte stores; the parameters and the reads' list are copied as they stand");
static int polytail_prepare(ffhip_batch *b) {
    ffhip_batch::PolyTail &f = b->pt;
    if (!f.set) return set_err(FFHIP_EINVAL, "poly tail: no parameters are set for the batch (ffhip_batch_set_polytail)");
    const int nR = batch_nreads(b), st = total_stride(b->mdl);
    if (int rc = f.rec.fixed(b, (size_t)b->cap_reads * kPolyTailRecBytes, "poly tail: the reads' records")) return rc;
    if (int rc = f.list.grow(b, b->stream, (size_t)b->cap_reads * sizeof(PolyRead), "poly tail: the reads' list")) return rc;
    PolyRead *list = (PolyRead *)f.list.host;
    size_t at = 0;
    for (int r = 0; r < nR; r++) {
        list[r] = PolyRead{ signal_at(b, r, st), at, b->hT[r], r };
        at += (size_t)(std::min(b->hTb[r], b->hT[r] / st) / f.p.window);
    }
    if (int rc = dgrow(b, (void **)&f.ws, &f.ws_cap, std::max<size_t>(at, 1) * 9, "poly tail: the windows' workspace")) return rc;
    f.windows = at;
    return nR > 0 ? f.list.copy_up((size_t)nR * sizeof(PolyRead), b->stream) : FFHIP_OK;
}
static void polytail_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // from the path the decode has just written and the signal the convolutions read
    ffhip_batch::PolyTail &f = b->pt;
    launch_polytail(b->stream, (const PolyRead *)f.list.dev, batch_nreads(b), b->sbuf[0].p, total_stride(b->mdl), b->path, b->mdl->nbase, polytail_params(&f.p), f.rec.dev,
                    (double *)f.ws, f.ws + 8 * f.windows, nullptr, b->Tb, tbr, rmap);
    b->launches[5]++;
    f.valid = 1;
}

// Remap and truth list their reads a kernel form each, one form behind the other: the pinned image and its upload, and the walk over the forms, a launch each
static_assert(kRemapForms == kTruthForms, "one packing for both");
template <class Read> static int forms_upload(ffhip_batch *b, Annot &f, const std::vector<Read> (&per)[kRemapForms], int (&count)[kRemapForms], int nR) {
    size_t at = 0;
    for (int k = 0; k < kRemapForms; k++) {
        count[k] = (int)per[k].size();
        if (!per[k].empty()) memcpy((Read *)f.list.host + at, per[k].data(), per[k].size() * sizeof(Read));
        at += per[k].size();
    }
    return nR > 0 ? f.list.copy_up((size_t)nR * sizeof(Read), b->stream) : FFHIP_OK;
}
template <class Launch> static void forms_launch(ffhip_batch *b, Annot &f, const int (&count)[kRemapForms], Launch launch) {
    size_t at = 0;
    for (int k = 0; k < kRemapForms; k++) {
        if (count[k] > 0) { launch(k, at, count[k]); b->launches[5]++; }
        at += (size_t)count[k];
    }
    f.valid = 1;
}

// Remap, the front's share: buffers on first use, every read's status, kernel form and place in the workspace, the lists a form each, their upload.
static_assert(sizeof(RemapRead) == 24, "the reads' list is copied as it stands");
// the sequence's positions the host sizes read r by: its sequence's, or -- remap from map, where no length is known here -- the N + 1 a path of its N blocks can hold
static int remap_room(const ffhip_batch *b, int r) { return b->rmp.from_map ? (b->hTb[r] >= 1 ? b->hTb[r] + 1 : 0) : (int)b->rmp.seq[r].size(); }
static bool remap_mappable(const ffhip_batch *b, int r) {      // this read's sequence can be mapped (from the map: it may have one)
    const int N = b->hTb[r], L = remap_room(b, r);
    return (b->rmp.from_map || b->rmp.state[r] == 1) && N >= 1 && L >= 1 && L <= N + 1;
}
static size_t remap_bytes(const ffhip_batch *b) { return remap_moves_at(b) + (size_t)b->nread * ((size_t)b->Tb + 1); }
// The two modes differ in where a read's length and status come from, as truth's do.  A set sequence has its own.  From the map every read of N >= 1 blocks is listed
// with L = 0 and status 1 for k_map_remap_seq to patch; its share of the sequences (dseq grows here in this mode), its kernel form and its workspace are those of
// N + 1 positions, the most a path of N blocks can hold.
static int remap_prepare(ffhip_batch *b) {
    ffhip_batch::Remap &f = b->rmp;
    const int nR = batch_nreads(b);
    const bool fm = f.from_map != 0;
    if (fm) {
        if (!(b->run_flags & FFHIP_RUN_MAP)) return set_err(FFHIP_EINVAL, "remap from map: the run does not make the map records (FFHIP_RUN_REMAP goes with FFHIP_RUN_MAP in this mode)");
        if (!b->map.ref) return set_err(FFHIP_EINVAL, "remap from map: no reference is attached to the batch (ffhip_batch_set_map)");
        if (b->run_flags & FFHIP_RUN_REMAP_MODS)
            return set_err(FFHIP_EINVAL, "remap from map: site mods are listed on the host from sequences it does not have in this mode (FFHIP_RUN_REMAP_MODS goes with ffhip_batch_set_remap)");
        if (b->run_flags & FFHIP_RUN_REMAP_VARIANTS)
            return set_err(FFHIP_EINVAL, "remap from map: variants are validated on the host against sequences it does not have in this mode (FFHIP_RUN_REMAP_VARIANTS goes with ffhip_batch_set_remap)");
    } else {
        if (!f.set) return set_err(FFHIP_EINVAL, "remap: no sequences are set for the batch (ffhip_batch_set_remap)");
        if ((int)f.seq.size() != nR) return set_err(FFHIP_EINVAL, "remap: sequences were set for %zu reads, the batch holds %d", f.seq.size(), nR);
    }
    if (int rc = f.rec.fixed(b, remap_bytes(b), "remap: the records and moves")) return rc;
    if (int rc = f.list.grow(b, b->stream, (size_t)b->cap_reads * sizeof(RemapRead), "remap: the reads' list")) return rc;
    std::vector<RemapRead> per[kRemapForms];
    size_t ws = 0, seq = 0;
    for (int r = 0; r < nR; r++) {
        const int L = remap_room(b, r);
        if (fm && seq + (size_t)L > (size_t)0xffffffffu)
            return set_err(FFHIP_EINVAL, "remap from map: the reads' rooms come to more than 2^32 - 1 positions together (read %d: %d), which the list's 32-bit offsets cannot hold", r, L);
        RemapRead rr{ ws, (unsigned)seq, fm ? 0 : L, fm ? (L > 0 ? 1 : 0) : f.state[r], r };
        int form = 0;
        if (rr.status == 1 && !remap_mappable(b, r)) rr.status = 2;
        if (rr.status == 1) {
            form = remap_form(L, f.band);
            if (form < 0) return set_err(FFHIP_EINVAL, "remap: read %d's window of min(2 band + 1, L) cells is more than %d", r, remap_max_window());
            ws += remap_ws_words(form, b->hTb[r]);
        }
        seq += (size_t)L;
        per[form].push_back(rr);
    }
    if (fm) if (int rc = dgrow(b, (void **)&f.dseq, &f.dseq_cap, (seq ? seq : 1) * sizeof(unsigned short), "remap from map: the sequences")) return rc;
    if (int rc = dgrow(b, (void **)&f.ws, &f.ws_cap, ws * 8, "remap: the traceback workspace")) return rc;
    return forms_upload(b, f, per, f.count, nR);
}
static void remap_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {           // from the transitions, whatever the path was decoded from
    ffhip_batch::Remap &f = b->rmp;
    if (f.from_map) {                                       // every form's entries in one launch, behind k_map_finish (map's row stands ahead of remap's in kAnnots)
        launch_map_remap_seq(b->stream, b->map.ref->view, b->map.rec.dev, (RemapRead *)f.list.dev, batch_nreads(b), f.dseq, b->mdl->nbase, b->Tb, tbr);
        b->launches[5]++;
    }
    forms_launch(b, f, f.count, [&](int form, size_t at, int n) {
        launch_remap(b->stream, form, (const RemapRead *)f.list.dev + at, n, f.dseq, b->trans, b->mdl->Ps, f.band, f.ws, f.rec.dev, f.rec.dev + remap_moves_at(b), b->Tb, tbr, rmap);
    });
}
static void remap_spans(const ffhip_batch *b, int r, AnnotSpan out[2]) {           // the record, and the moves of the read's blocks (not the entry behind them)
    out[0] = AnnotSpan{ (size_t)r * 16, 16 };
    out[1] = AnnotSpan{ remap_moves_at(b) + read_row1(b, r), (size_t)b->hTb[r] };
}

// Truth from map: the most bases a stretch of a call of a read of N blocks can have, with max_error e per mille (include/ffhip.h "truth from map")
static long long map_truth_bound(long long N, long long e) { return (N + 1) + (N + 1) * e / 1000; }
// Truth, the front's share: as remap's.  The ops' bytes follow from the truths and the reads' blocks, so records and ops grow here.  The two modes differ in where
// a read's length and status come from.  A set truth has its own.  From the map no truth's length is known here, so every read of N > 0 blocks is listed with
// m = 0 and status 1 for k_map_stretch to patch, and its share of the truths (dseq grows here in this mode), its workspace and its ops are those of bound(N, e).
static_assert(sizeof(TruthRead) == 40, "the reads' list is copied as it stands");
static int truth_prepare(ffhip_batch *b) {
    ffhip_batch::Truth &f = b->tru;
    const int nR = batch_nreads(b);
    const bool fm = f.from_map != 0;
    if (fm) {
        if (!(b->run_flags & FFHIP_RUN_MAP)) return set_err(FFHIP_EINVAL, "truth from map: the run does not make the map records (FFHIP_RUN_TRUTH goes with FFHIP_RUN_MAP in this mode)");
        if (!b->map.ref) return set_err(FFHIP_EINVAL, "truth from map: no reference is attached to the batch (ffhip_batch_set_map)");
    } else {
        if (!f.set) return set_err(FFHIP_EINVAL, "truth: no truths are set for the batch (ffhip_batch_set_truth)");
        if ((int)f.seq.size() != nR) return set_err(FFHIP_EINVAL, "truth: truths were set for %zu reads, the batch holds %d", f.seq.size(), nR);
    }
    if (int rc = f.list.grow(b, b->stream, (size_t)b->cap_reads * sizeof(TruthRead), "truth: the reads' list")) return rc;
    std::vector<TruthRead> per[kTruthForms];
    std::vector<size_t> off((size_t)nR + 1, 0);
    size_t ws = 0, seq = 0, ops = 0;
    for (int r = 0; r < nR; r++) {
        const int N = b->hTb[r];
        const long long len = !fm ? (long long)f.seq[r].size() : N > 0 ? map_truth_bound(N, b->map.max_error) : 0;      // the truth's bases, or their bound
        const int status = N <= 0 ? 0 : fm ? 1 : f.state[r];
        if (fm && len > kTruthMaxLen) return set_err(FFHIP_EINVAL, "truth from map: read %d's stretch may have %lld bases (at most %d)", r, len, kTruthMaxLen);
        if (fm && seq + (size_t)len > (size_t)0xffffffffu)
            return set_err(FFHIP_EINVAL, "truth from map: the reads' bounds come to more than 2^32 - 1 bases together (read %d: %lld), which the list's 32-bit offsets cannot hold", r, len);
        const int cap = status == 1 ? (int)len + N + 1 : 0;
        TruthRead tr{ ws, ops, (unsigned)seq, fm ? 0 : (int)len, status, r, cap, fm ? (int)len : 0 };
        int form = 0;
        if (tr.status == 1) {
            form = truth_form(std::min<long long>(2ll * f.band + 1, (long long)N + 2));
            if (form < 0) return set_err(FFHIP_EINVAL, "truth: read %d's window of min(2 band + 1, blocks + 2) cells is more than %d", r, truth_max_window());
            ws += truth_ws_words(form, (int)len);
        }
        off[r] = ops;
        seq += (size_t)len; ops += (size_t)cap;
        per[form].push_back(tr);
    }
    off[nR] = ops;
    if (fm) if (int rc = dgrow(b, (void **)&f.dseq, &f.dseq_cap, seq ? seq : 1, "truth from map: the truths")) return rc;
    if (int rc = dgrow(b, (void **)&f.ws, &f.ws_cap, ws * 8, "truth: the traceback workspace")) return rc;
    if (int rc = f.rec.grow(b, b->stream, truth_ops_at(b) + ops, "truth: the records and ops")) return rc;
    f.off = std::move(off);
    return forms_upload(b, f, per, f.count, nR);
}
static void truth_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {           // from the strings and lengths k_assemble has just written
    ffhip_batch::Truth &f = b->tru;
    if (f.from_map) {                                       // every form's entries in one launch, behind k_map_finish (map's row stands ahead of truth's in kAnnots)
        launch_map_stretch(b->stream, b->map.ref->view, b->map.rec.dev, (TruthRead *)f.list.dev, batch_nreads(b), f.dseq);
        b->launches[5]++;
    }
    forms_launch(b, f, f.count, [&](int form, size_t at, int n) {
        launch_truth(b->stream, form, (const TruthRead *)f.list.dev + at, n, f.dseq, b->bases(), b->lens(), f.band, f.ws, (int *)f.rec.dev, f.rec.dev + truth_ops_at(b), b->Tb, tbr, rmap);
    });
}
static size_t truth_bytes(const ffhip_batch *b) { return truth_ops_at(b) + (b->tru.off.empty() ? 0 : b->tru.off.back()); }
static void truth_spans(const ffhip_batch *b, int r, AnnotSpan out[2]) {
    out[0] = AnnotSpan{ (size_t)r * kTruthRecInts * 4, (size_t)kTruthRecInts * 4 };
    out[1] = AnnotSpan{ truth_ops_at(b) + b->tru.off[r], b->tru.off[r + 1] - b->tru.off[r] };
}

// Events, site mods and variants: 16-byte records, a read's one behind the other from its offset
static_assert(sizeof(ffhip_event) == 16 && sizeof(ffhip_site_mod) == 16 && sizeof(ffhip_variant_call) == 16, "their kernels write a record as one 16-byte store");
template <auto F> static size_t perbase_bytes(const ffhip_batch *b) { return (b->*F).total() * 16; }
template <auto F> static void perbase_spans(const ffhip_batch *b, int r, AnnotSpan out[2]) { const ffhip_batch::PerBase &f = b->*F; span1(out, f.off[r] * 16, (f.off[r + 1] - f.off[r]) * 16); }

// Events, the front's share, behind remap's: every read's place in the one buffer, from the L of its sequence, and where its samples stand (the addresses
// rerun_on_f32_path reads them at); the buffer and its mirror grow here.  A read remap_prepare refuses has no room and no entry.
static_assert(sizeof(EventRead) == 32, "the reads' list is copied as it stands");
static int events_prepare(ffhip_batch *b) {
    ffhip_batch::PerBase &f = b->evt;
    const int nR = batch_nreads(b), st = total_stride(b->mdl);
    if (int rc = f.list.grow(b, b->stream, (size_t)b->cap_reads * sizeof(EventRead), "events: the reads' list")) return rc;
    std::vector<size_t> off((size_t)nR + 1, 0);
    std::vector<EventRead> list;
    size_t at = 0;
    for (int r = 0; r < nR; r++) {
        const int L = remap_room(b, r);                      // (remap from map: room for N + 1 events; k_events writes the L of remap's record and leaves the rest alone)
        off[r] = at;
        if (!remap_mappable(b, r)) continue;
        list.push_back(EventRead{ signal_at(b, r, st), at, b->hT[r], L, r, 0 });
        at += (size_t)L;
    }
    off[nR] = at;
    if (int rc = f.rec.grow(b, b->stream, std::max<size_t>(at, 1) * sizeof(ffhip_event), "events: the reads' events")) return rc;
    f.off = std::move(off);
    f.reads = (int)list.size();
    if (list.empty()) return FFHIP_OK;
    memcpy(f.list.host, list.data(), list.size() * sizeof(EventRead));
    return f.list.copy_up(list.size() * sizeof(EventRead), b->stream);
}
static void events_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {          // from the path k_remap has just written and the signal the convolutions read
    if (b->evt.reads > 0) {
        launch_events(b->stream, (const EventRead *)b->evt.list.dev, b->evt.reads, b->sbuf[0].p, total_stride(b->mdl), b->rmp.rec.dev, b->rmp.rec.dev + remap_moves_at(b),
                      b->evt.rec.dev, b->Tb, tbr, rmap);
        b->launches[5]++;
    }
    b->evt.valid = 1;
}

// Site mods and variants, the front's share, behind remap's: the reads that can be mapped and have an entry (a C or Z; a variant), their entries one read behind the
// other (an entry's place in its list is its record's place in the buffer), every listed read's L + 1 words of starts; buffers, mirrors and workspace grow here.
// entries_of(r, k, &ent) appends read r's entries as those of listed read k and says whether there are any.  The two lists are one pinned image and one upload:
// the entries in front of the reads (entries_first) or behind them.  A read remap_prepare refuses has no entry.
struct SitesText { const char *name, *noun, *records, *starts, *lists; };
template <class Entry, class EntriesOf> static int sites_prepare(ffhip_batch *b, ffhip_batch::Sites &f, bool entries_first, const SitesText &t, EntriesOf entries_of) {
    const int nR = batch_nreads(b);
    std::vector<size_t> off((size_t)nR + 1, 0);
    std::vector<SiteRead> list;
    std::vector<Entry> ent;
    size_t words = 0, seq = 0;
    for (int r = 0; r < nR; r++) {
        const int L = (int)b->rmp.seq[r].size();
        off[r] = ent.size();
        if (remap_mappable(b, r) && entries_of(r, (int)list.size(), &ent)) {
            list.push_back(SiteRead{ words, (unsigned)seq, L, r, 0 });
            words += (size_t)L + 1;
        }
        seq += (size_t)L;
    }
    off[nR] = ent.size();
    if (ent.size() > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "%s: %zu %s in one batch", t.name, ent.size(), t.noun);
    const size_t lb = list.size() * sizeof(SiteRead), eb = ent.size() * sizeof(Entry);
    if (int rc = f.rec.grow(b, b->stream, std::max<size_t>(ent.size(), 1) * 16, t.records)) return rc;
    if (int rc = dgrow(b, (void **)&f.start, &f.start_cap, std::max<size_t>(words, 1) * 4, t.starts)) return rc;
    if (int rc = f.list.grow(b, b->stream, std::max<size_t>(lb + eb, 8), t.lists)) return rc;
    f.off = std::move(off);
    f.reads = (int)list.size();
    if (ent.empty()) return FFHIP_OK;
    memcpy(f.list.host + (entries_first ? eb : 0), list.data(), lb);
    memcpy(f.list.host + (entries_first ? 0 : lb), ent.data(), eb);
    return f.list.copy_up(lb + eb, b->stream);
}

static_assert(sizeof(SiteRead) == 24 && sizeof(SiteMod) == 8, "the lists are copied as they stand");
static int sitemods_prepare(ffhip_batch *b) {
    static const SitesText t{ "site mods", "sites", "site mods: the sites' records", "site mods: the workspace of starts", "site mods: the lists of reads and sites" };
    return sites_prepare<SiteMod>(b, b->smd, false, t, [&](int r, int k, std::vector<SiteMod> *out) { return sitemods_sites(b->rmp.seq[r].data(), b->rmp.seq[r].size(), k, out) > 0; });
}
static void sitemods_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // from that path, the transitions and the coded sequences
    ffhip_batch::Sites &f = b->smd;
    if (f.total() > 0) {
        launch_site_mods(b->stream, (const SiteRead *)f.list.dev, f.reads, (const SiteMod *)(f.list.dev + (size_t)f.reads * sizeof(SiteRead)), (int)f.total(), b->rmp.dseq, b->trans,
                         b->mdl->Ps, f.context, f.all, b->rmp.rec.dev, b->rmp.rec.dev + remap_moves_at(b), f.start, f.rec.dev, b->Tb, tbr, rmap);
        b->launches[5] += 2;
    }
    f.valid = 1;
}

// (the variants stand in front of the reads: an entry is read as 16-byte words)
static_assert(sizeof(VarEntry) == 32 && sizeof(Variant) == sizeof(ffhip_variant) && sizeof(ffhip_variant) == 24, "the lists are copied as they stand");
static int variants_prepare(ffhip_batch *b) {
    static const SitesText t{ "variants", "variants", "variants: the variants' records", "variants: the workspace of starts", "variants: the list of variants and reads" };
    const int nR = batch_nreads(b);
    if (b->var.set.empty()) return set_err(FFHIP_EINVAL, "variants: none are set for the batch (ffhip_batch_set_remap_variants)");
    if ((int)b->var.set.size() != nR) return set_err(FFHIP_EINVAL, "variants: lists were set for %zu reads, the batch holds %d", b->var.set.size(), nR);
    return sites_prepare<VarEntry>(b, b->var, true, t, [&](int r, int k, std::vector<VarEntry> *out) {
        for (size_t i = 0; i < b->var.set[r].size(); i++) {
            VarEntry e{ k, (int)i, {} };
            memcpy(&e.v, &b->var.set[r][i], sizeof e.v);
            out->push_back(e);
        }
        return !b->var.set[r].empty();
    });
}
static void variants_launch(ffhip_batch *b, const int *tbr, ReadMap rmap) {        // (likewise)
    ffhip_batch::Variants &f = b->var;
    if (f.total() > 0) {
        launch_variants(b->stream, (const SiteRead *)(f.list.dev + f.total() * sizeof(VarEntry)), f.reads, (const VarEntry *)f.list.dev, (int)f.total(), b->rmp.dseq, b->trans,
                        b->mdl->Ps, b->mdl->nbase, f.context, f.all, b->rmp.rec.dev, b->rmp.rec.dev + remap_moves_at(b), f.start, f.rec.dev, b->Tb, tbr, rmap);
        b->launches[5] += 2;
    }
    f.valid = 1;
}

// The table, in launch order (ffhip_batch::annot has the same): the map stands ahead of truth, which in its from-map mode reads the records k_map_finish has just written; truth reads the strings as barcodes and adapters do; the poly tail reads the path and the signal; events, site mods and variants read what
// k_remap has just written
const AnnotRow ffhip::kAnnots[ffhip_batch::AN_COUNT] = {
    { FFHIP_RUN_BARCODES, nullptr, 0, "barcodes: a flip-flop model only (the run-length model has no base strings)", "barcodes need a decoded run (FFHIP_RUN_NO_DECODE is set)",
      barcodes_prepare, barcodes_launch, fixed_bytes<sizeof(ffhip_barcode_call)>, fixed_spans<sizeof(ffhip_barcode_call)> },
    { FFHIP_RUN_ADAPTERS, nullptr, 0, "adapters: a flip-flop model only (the run-length model has no base strings)", "adapters need a decoded run (FFHIP_RUN_NO_DECODE is set)",
      adapters_prepare, adapters_launch, fixed_bytes<kAdapterRecBytes>, fixed_spans<kAdapterRecBytes> },
    { FFHIP_RUN_MAP, nullptr, 0, "map: a flip-flop model only (the run-length model has no base strings)", "map needs a decoded run (FFHIP_RUN_NO_DECODE is set)",
      map_prepare, map_launch, fixed_bytes<kMapRecBytes>, fixed_spans<kMapRecBytes> },
    { FFHIP_RUN_POLYTAIL, nullptr, 0, "poly tail: a flip-flop model only (the run-length model's path is not one of bases)", "poly tail needs a decoded run (FFHIP_RUN_NO_DECODE is set)",
      polytail_prepare, polytail_launch, fixed_bytes<kPolyTailRecBytes>, fixed_spans<kPolyTailRecBytes> },
    { FFHIP_RUN_TRUTH, nullptr, 0, "truth: a flip-flop model only (the run-length model's call is a list of runs)", "truth needs a decoded run (FFHIP_RUN_NO_DECODE is set)",
      truth_prepare, truth_launch, truth_bytes, truth_spans },
    { FFHIP_RUN_REMAP, nullptr, 0, "remap: a flip-flop model only (the run-length model's scores are not transitions between bases)", "remap needs a decoded run (FFHIP_RUN_NO_DECODE is set)",
      remap_prepare, remap_launch, remap_bytes, remap_spans },
    { FFHIP_RUN_EVENTS, "events: the signal of a mapped read's bases needs the mapping (FFHIP_RUN_EVENTS goes with FFHIP_RUN_REMAP)", 0, nullptr, nullptr,
      events_prepare, events_launch, perbase_bytes<&ffhip_batch::evt>, perbase_spans<&ffhip_batch::evt> },
    { FFHIP_RUN_REMAP_MODS, "site mods: the scores of a mapped sequence's C positions need the mapping (FFHIP_RUN_REMAP_MODS goes with FFHIP_RUN_REMAP)", 5,
      "site mods: the model has no modified base (FFHIP_RUN_REMAP_MODS takes a model of the alphabet ACGTZ)", nullptr, sitemods_prepare, sitemods_launch, perbase_bytes<&ffhip_batch::smd>, perbase_spans<&ffhip_batch::smd> },
    { FFHIP_RUN_REMAP_VARIANTS, "variants: the scores of a mapped sequence's alleles need the mapping (FFHIP_RUN_REMAP_VARIANTS goes with FFHIP_RUN_REMAP)", 0, nullptr, nullptr,
      variants_prepare, variants_launch, perbase_bytes<&ffhip_batch::var>, perbase_spans<&ffhip_batch::var> },
};
// the front's share of them all: may this run ask, then the feature's own preparations
int ffhip::annots_prepare(ffhip_batch *b, unsigned flags) {
    const ffhip_model *m = b->mdl;
    for (int i = 0; i < ffhip_batch::AN_COUNT; i++) {
        const AnnotRow &row = kAnnots[i];
        b->annot(i).valid = 0;
        if (!(flags & row.flag)) continue;
        if (row.remap_text && !(flags & FFHIP_RUN_REMAP)) return set_err(FFHIP_EINVAL, "%s", row.remap_text);
        if (row.model_text && (m->kind == FFHIP_NET_LSTM5_RLE || (row.nbase && m->nbase != row.nbase))) return set_err(FFHIP_EINVAL, "%s", row.model_text);
        if (row.undecoded_text && (flags & FFHIP_RUN_NO_DECODE)) return set_err(FFHIP_EINVAL, "%s", row.undecoded_text);
        if (int rc = row.prepare(b)) return rc;
    }
    return FFHIP_OK;
}
// ---- the run-wide accumulators (include/ffhip.h "pileup", "mod pileup", "consensus", "error profile"): no record, no buffer of the batch's, so no row above.
// One row an accumulator.  The front's share: may this run ask -- the flag's companions in the order their refusals are reported, then the mode of truth from map
// and the reference (the error profile serves either mode and belongs to no reference: it asks for the map in that mode only, and for the batch's engine)
struct PileRow {
    unsigned flag;
    const char *name, *goes, *setter;
    struct { unsigned flag; const char *makes; } with[3];
    bool by_position;
    const ffhip_pile *(*attached)(const ffhip_batch *);
};
static const PileRow kPiles[] = {
    { FFHIP_RUN_PILEUP, "pileup", "(FFHIP_RUN_PILEUP goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)", "ffhip_batch_set_pileup",
      { { FFHIP_RUN_TRUTH, "truth records" }, { FFHIP_RUN_MAP, "map records" } }, true, [](const ffhip_batch *b) -> const ffhip_pile * { return b->pile; } },
    { FFHIP_RUN_MOD_PILEUP, "mod pileup", "(FFHIP_RUN_MOD_PILEUP goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH | FFHIP_RUN_MOD_PROBS)", "ffhip_batch_set_modpileup",
      { { FFHIP_RUN_MAP, "map records" }, { FFHIP_RUN_TRUTH, "truth records" }, { FFHIP_RUN_MOD_PROBS, "5mC probabilities" } }, true,
      [](const ffhip_batch *b) -> const ffhip_pile * { return b->modpile; } },
    { FFHIP_RUN_CONSENSUS, "consensus", "(FFHIP_RUN_CONSENSUS goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)", "ffhip_batch_set_consensus",
      { { FFHIP_RUN_TRUTH, "truth records" }, { FFHIP_RUN_MAP, "map records" } }, true, [](const ffhip_batch *b) -> const ffhip_pile * { return b->cons; } },
    { FFHIP_RUN_ERRPROFILE, "error profile", "(FFHIP_RUN_ERRPROFILE goes with FFHIP_RUN_TRUTH)", "ffhip_batch_set_errprofile",
      { { FFHIP_RUN_TRUTH, "truth records" } }, false, [](const ffhip_batch *b) -> const ffhip_pile * { return b->errp; } },
};
int ffhip::piles_check(const ffhip_batch *b, unsigned flags) {
    for (const PileRow &row : kPiles) {
        if (!(flags & row.flag)) continue;
        for (const auto &w : row.with)
            if (w.flag && !(flags & w.flag)) return set_err(FFHIP_EINVAL, "%s: the run does not make the %s %s", row.name, w.makes, row.goes);
        if (!row.by_position && b->tru.from_map && !(flags & FFHIP_RUN_MAP))
            return set_err(FFHIP_EINVAL, "%s: the run does not make the map records (in the mode of truth from map FFHIP_RUN_ERRPROFILE goes with FFHIP_RUN_MAP | FFHIP_RUN_TRUTH)", row.name);
        if (row.by_position && !b->tru.from_map) return set_err(FFHIP_EINVAL, "%s: the batch is not in the mode of truth from map (ffhip_batch_set_truth_from_map)", row.name);
        const ffhip_pile *p = row.attached(b);
        if (!p) return set_err(FFHIP_EINVAL, "%s: no %s is attached to the batch (%s)", row.name, row.name, row.setter);
        if (row.by_position && p->ref != b->map.ref) return set_err(FFHIP_EINVAL, "%s: the attached %s belongs to another reference than the batch's map reference", row.name, row.name);
        if (!row.by_position && p->eng != b->eng) return set_err(FFHIP_EINVAL, "%s: the attached %s belongs to another engine", row.name, row.name);
    }
    return FFHIP_OK;
}
// ... and the finish's: the records, ops and letters are final (ffhip_batch_finish), so every listed read is counted once, on the batch's stream, unwaited for
static PileArgs pile_args(const ffhip_batch *b) {
    return { (const TruthRead *)b->tru.list.dev, batch_nreads(b), b->map.rec.dev, (const int *)b->tru.rec.dev, b->tru.rec.dev + truth_ops_at(b), b->bases(), b->Tb,
             b->packed ? ReadMap{ b->d_vb0, b->d_vb1, b->nread } : ReadMap() };
}
static void pile_mark(ffhip_pile *p, const ffhip_batch *b) {     // work against it was enqueued on the batch's stream (pile_wait)
    for (int i = 0; i < b->eng->nstreams; i++) if (b->eng->streams[i] == b->stream) p->used[i] = true;
}
void ffhip::pileup_launch(ffhip_batch *b) {
    launch_pileup(b->stream, b->pile->ref->view, pile_args(b), b->pile->view);
    pile_mark(b->pile, b);
}
void ffhip::modpileup_launch(ffhip_batch *b) {
    launch_modpileup(b->stream, b->modpile->ref->view, pile_args(b), b->res.on_dev<uint8_t>(RF_ML), b->modpile->view);
    pile_mark(b->modpile, b);
}
void ffhip::consensus_launch(ffhip_batch *b) {
    launch_consensus(b->stream, b->cons->ref->view, pile_args(b), b->cons->view);
    pile_mark(b->cons, b);
}
void ffhip::errprofile_launch(ffhip_batch *b) {                  // (in the mode of truth from map it takes the batch's own reference)
    launch_errprofile(b->stream, b->tru.from_map ? &b->map.ref->view : nullptr, pile_args(b), b->errp->groups, b->quals(), b->tru.dseq, b->errp->view);
    pile_mark(b->errp, b);
}
// the copies of a finished run beside the block's: one a feature the run made, if it has a byte to bring
int ffhip::annots_copy_down(ffhip_batch *b) {
    for (int i = 0; i < ffhip_batch::AN_COUNT; i++)
        if (const size_t n = b->annot(i).valid ? kAnnots[i].bytes(b) : 0)
            if (int rc = b->annot(i).rec.copy_down(n, b->stream)) return rc;
    return FFHIP_OK;
}

// the accessor of barcodes, the map and the poly tail (feature f), whose public record is the kernel's: made in this run, then read's record as it stands
template <class F, class Rec> static int fixed_record(const ffhip_batch *b, int read, F ffhip_batch::*feature, const char *unmade, Rec *out) {
    if (!results_ok(b, read) || !out) return FFHIP_EINVAL;
    const Annot &f = b->*feature;
    if (!f.valid || !f.rec.host) return set_err(FFHIP_EINVAL, "%s", unmade);
    memcpy(out, f.rec.host + (size_t)read * sizeof *out, sizeof *out);
    return FFHIP_OK;
}

// ---- barcodes (include/ffhip.h "barcodes"; the kernel: ffhip_barcodes.hip)
extern "C" ffhip_barcodes *ffhip_barcodes_upload(ffhip_engine *eng, int n, const char *const *seq, int window) {
    if (!eng || !seq) { set_err(FFHIP_EINVAL, "null engine or kit"); return nullptr; }
    if (n < 1 || n > kBarcodeMaxKit) { set_err(FFHIP_EINVAL, "a barcode kit holds 1 .. %d patterns, not %d", kBarcodeMaxKit, n); return nullptr; }
    if (window < 1 || window > kBarcodeMaxWindow) { set_err(FFHIP_EINVAL, "the barcode window is 1 .. %d bases, not %d", kBarcodeMaxWindow, window); return nullptr; }
    std::vector<unsigned long long> peq((size_t)n * 8, 0ull);
    std::vector<int> len(n, 0);
    int lmin = kBarcodeMaxLen, lmax = 0;
    if (!kit_patterns("barcode", n, seq, kBarcodeMaxLen, len.data(), [&](size_t k, size_t i, size_t c, size_t L) {
            peq[(k * 4 + c) * 2 + i / 64] |= 1ull << (i % 64);
            lmin = std::min(lmin, (int)L); lmax = std::max(lmax, (int)L);
        })) return nullptr;
    hipSetDevice(eng->device);
    ffhip_barcodes *kit = new ffhip_barcodes();
    kit->eng = eng; kit->lmin = lmin;
    if (dev_fill("barcode kit", { { &kit->d_peq, peq.data(), peq.size() * 8 }, { &kit->d_len, len.data(), len.size() * 4 } })) { delete kit; return nullptr; }
    kit->kit = BarcodeKit{ (const unsigned long long *)kit->d_peq, (const int *)kit->d_len, n, window, lmax > 64 ? 2 : 1 };
    return kit;
}
extern "C" void ffhip_barcodes_free(ffhip_barcodes *kit) {
    if (!kit) return;
    hipSetDevice(kit->eng->device);
    dev_free({ &kit->d_peq, &kit->d_len });
    delete kit;
}
extern "C" int ffhip_batch_set_barcodes(ffhip_batch *b, const ffhip_barcodes *kit, int max_dist, int min_sep, int both_ends) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (!kit) { b->bc.kit = nullptr; return FFHIP_OK; }
    if (kit->eng != b->eng) return set_err(FFHIP_EINVAL, "the barcode kit belongs to another engine");
    if (max_dist > 255 || min_sep > 255) return set_err(FFHIP_EINVAL, "barcodes: max_dist and min_sep are at most 255");
    b->bc.kit = kit;
    b->bc.max_dist = barcodes_max_dist(kit, max_dist);
    b->bc.min_sep = barcodes_min_sep(min_sep);
    b->bc.both = both_ends ? 1 : 0;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_barcode(const ffhip_batch *b, int read, ffhip_barcode_call *out) {
    return fixed_record(b, read, &ffhip_batch::bc, "barcode records were not made in this run (FFHIP_RUN_BARCODES)", out);
}

// ---- adapters (include/ffhip.h "adapters"; the kernel: ffhip_adapters.hip)
extern "C" int ffhip_adapter_segment(void) { return kAdSeg; }
extern "C" ffhip_adapters *ffhip_adapters_upload(ffhip_engine *eng, int n, const char *const *seq) {
    if (!eng || !seq) { set_err(FFHIP_EINVAL, "null engine or kit"); return nullptr; }
    if (n < 1 || n > kAdapterMaxKit) { set_err(FFHIP_EINVAL, "an adapter kit holds 1 .. %d patterns, not %d", kAdapterMaxKit, n); return nullptr; }
    std::vector<unsigned long long> peq((size_t)n * 8, 0ull);       // [2 n][4]: as given, then the reverse complement
    std::vector<int> len(n, 0);
    if (!kit_patterns("adapter", n, seq, kAdapterMaxLen, len.data(), [&](size_t k, size_t i, size_t c, size_t L) {
            peq[(2 * k) * 4 + c] |= 1ull << i;
            peq[(2 * k + 1) * 4 + (3 - c)] |= 1ull << (L - 1 - i);
        })) return nullptr;
    hipSetDevice(eng->device);
    ffhip_adapters *kit = new ffhip_adapters();
    kit->eng = eng;
    if (dev_fill("adapter kit", { { &kit->d_peq, peq.data(), peq.size() * 8 }, { &kit->d_len, len.data(), len.size() * 4 } })) { delete kit; return nullptr; }
    kit->kit = AdapterKit{ (const unsigned long long *)kit->d_peq, (const int *)kit->d_len, n };
    return kit;
}
extern "C" void ffhip_adapters_free(ffhip_adapters *kit) {
    if (!kit) return;
    hipSetDevice(kit->eng->device);
    dev_free({ &kit->d_peq, &kit->d_len });
    delete kit;
}
extern "C" int ffhip_batch_set_adapters(ffhip_batch *b, const ffhip_adapters *kit, int max_dist) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (!kit) { b->ad.kit = nullptr; return FFHIP_OK; }
    if (kit->eng != b->eng) return set_err(FFHIP_EINVAL, "the adapter kit belongs to another engine");
    b->ad.kit = kit;
    b->ad.max_dist = adapters_max_dist(max_dist);
    return FFHIP_OK;
}
extern "C" int ffhip_batch_adapters(const ffhip_batch *b, int read, ffhip_adapter_header *header, const ffhip_adapter_hit **hits) {
    if (!results_ok(b, read) || !header || !hits) return FFHIP_EINVAL;
    if (!b->ad.valid || !b->ad.rec.host) return set_err(FFHIP_EINVAL, "adapter records were not made in this run (FFHIP_RUN_ADAPTERS)");
    const uint8_t *rec = b->ad.rec.host + (size_t)read * kAdapterRecBytes;
    memcpy(header, rec, sizeof *header);
    *hits = (const ffhip_adapter_hit *)(rec + sizeof *header);
    return FFHIP_OK;
}

// ---- map (include/ffhip.h "map"; the kernels: ffhip_map.hip)
extern "C" int ffhip_map_segment(void) { return kMapSeg; }
extern "C" ffhip_map_ref *ffhip_map_ref_upload(ffhip_engine *eng, int n, const char *const *seq) {
    if (!eng || !seq) { set_err(FFHIP_EINVAL, "null engine or reference"); return nullptr; }
    if (n < 1 || n > kMapMaxRecords) { set_err(FFHIP_EINVAL, "a reference holds 1 .. %d records, not %d", kMapMaxRecords, n); return nullptr; }
    std::vector<int2> recs(n);
    std::vector<int> rowoff((size_t)2 * n);
    std::vector<MapTask> tasks;
    size_t total = 0, entries = 0;
    for (int k = 0; k < n; k++) {
        const size_t m = seq[k] ? strnlen(seq[k], (size_t)kMapMaxTotal + 1) : 0;
        if (m < 1) { set_err(FFHIP_EINVAL, "reference record %d: position 0: a record has 1 or more bases", k); return nullptr; }
        if (total + m > (size_t)kMapMaxTotal) {
            set_err(FFHIP_EINVAL, "reference record %d: position %zu: the records hold at most %d bases together", k, (size_t)kMapMaxTotal - total, kMapMaxTotal);
            return nullptr;
        }
        recs[k] = make_int2((int)total, (int)m);
        total += m;
        for (int o = 0; o < 2; o++) {
            rowoff[2 * k + o] = (int)entries;
            entries += m + 1;
            for (size_t s = 0; s < m; s += kMapSeg) tasks.push_back(MapTask{ 2 * k + o, (int)s, (int)std::min(m, s + kMapSeg), 0 });
        }
    }
    std::vector<unsigned> words((total + 2 * kMapPad + 15) / 16 + 2, 0u);
    for (int k = 0; k < n; k++)
        for (int i = 0; i < recs[k].y; i++) {
            const int c = acgt_index(seq[k][i]);
            if (c < 0) { set_err(FFHIP_EINVAL, "reference record %d: position %d: the character is not one of ACGT", k, i); return nullptr; }
            const size_t g = (size_t)kMapPad + recs[k].x + i;
            words[g >> 4] |= (unsigned)c << (2 * (g & 15));
        }
    hipSetDevice(eng->device);
    ffhip_map_ref *ref = new ffhip_map_ref();
    ref->eng = eng;
    ref->score_entries = entries;
    for (int k = 0; k < n; k++) ref->rec_len.push_back(recs[k].y);
    if (dev_fill("reference", { { &ref->d_words, words.data(), words.size() * 4 }, { &ref->d_tasks, tasks.data(), tasks.size() * sizeof(MapTask) },
                                { &ref->d_recs, recs.data(), recs.size() * sizeof(int2) }, { &ref->d_rowoff, rowoff.data(), rowoff.size() * 4 } })) { delete ref; return nullptr; }
    ref->view = MapRefView{ (const unsigned *)ref->d_words, (const MapTask *)ref->d_tasks, (const int2 *)ref->d_recs, (const int *)ref->d_rowoff, (int)tasks.size(), n };
    return ref;
}
extern "C" void ffhip_map_ref_free(ffhip_map_ref *ref) {
    if (!ref) return;
    hipSetDevice(ref->eng->device);
    dev_free({ &ref->d_words, &ref->d_tasks, &ref->d_recs, &ref->d_rowoff });
    delete ref;
}
extern "C" int ffhip_batch_set_map(ffhip_batch *b, const ffhip_map_ref *ref, int window, int max_error) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (!ref) { b->map.ref = nullptr; return FFHIP_OK; }
    if (ref->eng != b->eng) return set_err(FFHIP_EINVAL, "the reference belongs to another engine");
    if (const char *why = map_invalid(window, max_error)) return set_err(FFHIP_EINVAL, "map: %s", why);
    map_defaults(&window, &max_error);
    b->map.ref = ref;
    b->map.window = window;
    b->map.max_error = max_error;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_map(const ffhip_batch *b, int read, ffhip_map_call *out) {
    return fixed_record(b, read, &ffhip_batch::map, "map records were not made in this run (FFHIP_RUN_MAP)", out);
}

// ---- poly tail (include/ffhip.h "poly tail"; the kernel: ffhip_polytail.hip)
extern "C" int ffhip_batch_set_polytail(ffhip_batch *b, const ffhip_polytail_params *params) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "poly tail: the batch is between a run and its finish");
    if (!params) { b->pt.set = false; return FFHIP_OK; }
    if (b->mdl->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "poly tail: a flip-flop model only (the run-length model's path is not one of bases)");
    const PolyTailParams p = polytail_params(params);
    if (const char *why = polytail_invalid(p)) return set_err(FFHIP_EINVAL, "poly tail: %s", why);
    b->pt.p = *params;
    b->pt.set = true;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_polytail(const ffhip_batch *b, int read, ffhip_polytail *out) {
    return fixed_record(b, read, &ffhip_batch::pt, "poly tail records were not made in this run (FFHIP_RUN_POLYTAIL)", out);
}

// ---- remap (include/ffhip.h "remap"; the kernel: ffhip_remap.hip)
// new sequences of a batch (remap's coded ones, the truths): flattened, the device buffer grown to them, uploaded
template <class T> static int seq_adopt(ffhip_batch *b, const std::vector<std::vector<T>> &seq, T **dseq, size_t *cap, const char *what) {
    size_t total = 0;
    for (const auto &q : seq) total += q.size();
    hipSetDevice(b->eng->device);
    HIP_TRY(hipStreamSynchronize(b->stream), FFHIP_EHIP);
    if (int rc = dgrow(b, (void **)dseq, cap, (total ? total : 1) * sizeof(T), what)) return rc;
    std::vector<T> flat;
    flat.reserve(total);
    for (const auto &q : seq) flat.insert(flat.end(), q.begin(), q.end());
    if (total) HIP_TRY(hipMemcpy(*dseq, flat.data(), total * sizeof(T), hipMemcpyHostToDevice), FFHIP_EHIP);
    return FFHIP_OK;
}
int ffhip::remap_adopt(ffhip_batch *b, std::vector<std::vector<unsigned short>> &&seq, std::vector<signed char> &&state, int band) {
    if (int rc = seq_adopt(b, seq, &b->rmp.dseq, &b->rmp.dseq_cap, "remap: the sequences")) return rc;
    b->rmp.seq = std::move(seq); b->rmp.state = std::move(state);
    b->rmp.band = band; b->rmp.set = 1; b->rmp.from_map = 0;
    b->var.set.clear();                                     // (variants are validated against the sequences: new sequences detach them)
    return FFHIP_OK;
}
extern "C" int ffhip_batch_set_remap(ffhip_batch *b, int nread, const uint8_t *const *codes, const size_t *len, int band) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (!codes) { b->rmp.set = 0; b->rmp.from_map = 0; b->rmp.seq.clear(); b->rmp.state.clear(); b->var.set.clear(); return FFHIP_OK; }
    const ffhip_model *m = b->mdl;
    if (m->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "remap: a flip-flop model only (the run-length model's scores are not transitions between bases)");
    if (!len || nread != batch_nreads(b)) return set_err(FFHIP_EINVAL, "remap: sequences for %d reads, the batch holds %d", nread, batch_nreads(b));
    if (band < 0) return set_err(FFHIP_EINVAL, "remap: the band half-width is %d (>= 0)", band);
    std::vector<std::vector<unsigned short>> seq((size_t)nread);
    std::vector<signed char> state((size_t)nread, 0);
    for (int r = 0; r < nread; r++) {
        if (!codes[r]) continue;
        if (len[r] > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "remap: read %d's sequence has %zu bases", r, len[r]);
        state[r] = len[r] ? 1 : 2;
        if (const size_t i = bad_code(codes[r], len[r], m->nbase); i < len[r])
            return set_err(FFHIP_EINVAL, "remap: read %d, position %zu: code %d is not a base of the model (0 .. %d)", r, i, (int)codes[r][i], m->nbase - 1);
        if (remap_form((int)len[r], band) < 0 && len[r]) return set_err(FFHIP_EINVAL, "remap: read %d's window of min(2 band + 1, L) cells is more than %d", r, remap_max_window());
        seq[r].resize(len[r]);
        remap_code(codes[r], len[r], m->nbase, seq[r].data());
    }
    return remap_adopt(b, std::move(seq), std::move(state), band);
}
// remap from map (include/ffhip.h "remap from map"; the kernel: k_map_remap_seq, ffhip_map.hip)
extern "C" int ffhip_batch_set_remap_from_map(ffhip_batch *b, int on, int band) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "remap from map: the batch is between a run and its finish");
    if (!on) { b->rmp.from_map = 0; return FFHIP_OK; }
    if (b->mdl->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "remap from map: a flip-flop model only (the run-length model's scores are not transitions between bases)");
    if (band < 0 || 2 * band + 1 > remap_max_window())
        return set_err(FFHIP_EINVAL, "remap from map: the band half-width is %d (0 .. %d: the widest kernel form holds a window of %d cells)", band, (remap_max_window() - 1) / 2, remap_max_window());
    b->rmp.seq.clear(); b->rmp.state.clear(); b->var.set.clear();      // (the two ways of giving sequences replace each other; variants are validated against set ones)
    b->rmp.set = 0; b->rmp.from_map = 1; b->rmp.band = band;
    return FFHIP_OK;
}
// A mapped read's traceback ends at position 0; and the accessor of everything made from the mapping (events, site mods, variants: feature f): made in this run,
// then the read's remap record, and its records in f -- or "nothing", which is the answer for a status other than 1
static int remap_end_check(int read, const int rec[4]) {
    return rec[0] == 1 && rec[3] != 0 ? set_err(FFHIP_EHIP, "remap: read %d's traceback ended at position %d, not 0", read, rec[3]) : FFHIP_OK;
}
template <class T, class F> static int mapped_records(const ffhip_batch *b, int read, F ffhip_batch::*feature, const char *unmade, int rec[4], const T **out, size_t *n) {
    if (!results_ok(b, read) || !out || !n) return FFHIP_EINVAL;
    const ffhip_batch::PerBase &f = b->*feature;
    if (!f.valid || !b->rmp.valid || !f.rec.host) return set_err(FFHIP_EINVAL, "%s", unmade);
    memcpy(rec, b->rmp.rec.host + (size_t)read * 16, 16);
    *out = nullptr; *n = 0;
    if (int rc = remap_end_check(read, rec)) return rc;
    if (rec[0] == 1) { *out = (const T *)f.rec.host + f.off[read]; *n = f.off[read + 1] - f.off[read]; }
    return FFHIP_OK;
}
extern "C" int ffhip_batch_remap(const ffhip_batch *b, int read, ffhip_remap_call *out) {
    if (!results_ok(b, read) || !out) return FFHIP_EINVAL;
    if (!b->rmp.valid || !b->rmp.rec.host) return set_err(FFHIP_EINVAL, "remap records were not made in this run (FFHIP_RUN_REMAP)");
    int rec[4];
    memcpy(rec, b->rmp.rec.host + (size_t)read * 16, 16);
    out->status = rec[0]; out->L = (size_t)rec[1];
    memcpy(&out->score, &rec[2], 4);
    out->nblock = (size_t)b->hTb[read];
    out->rm = rec[0] == 1 ? b->rmp.rec.host + remap_moves_at(b) + read_row1(b, read) : nullptr;
    return remap_end_check(read, rec);
}

// ---- events (include/ffhip.h "events"; the kernel: ffhip_events.hip)
extern "C" int ffhip_batch_events(const ffhip_batch *b, int read, const ffhip_event **ev, size_t *L) {
    int rec[4];
    if (int rc = mapped_records(b, read, &ffhip_batch::evt, "events were not made in this run (FFHIP_RUN_REMAP | FFHIP_RUN_EVENTS)", rec, ev, L)) return rc;
    if (rec[0] == 1 && b->rmp.from_map && rec[1] >= 1 && (size_t)rec[1] <= *L) *L = (size_t)rec[1];      // (remap from map: what is held is the room, and the record's L the events)
    if (rec[0] != 1 || (size_t)rec[1] == *L) return FFHIP_OK;
    const size_t held = *L;
    *ev = nullptr; *L = 0;
    return set_err(FFHIP_EHIP, "events: read %d was mapped to %d bases, its events hold %zu", read, rec[1], held);
}

// ---- site mods (include/ffhip.h "site mods"; the kernels: ffhip_sitemods.hip)
extern "C" int ffhip_batch_set_remap_mods(ffhip_batch *b, int context, int all_paths) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "site mods: the batch is running (ffhip_batch_finish first)");
    if (context < 0 || context > kSiteModsMaxContext) return set_err(FFHIP_EINVAL, "site mods: the context is %d (0 .. %d)", context, kSiteModsMaxContext);
    b->smd.context = context; b->smd.all = all_paths ? 1 : 0;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_site_mods(const ffhip_batch *b, int read, const ffhip_site_mod **sm, size_t *nsite) {
    int rec[4];
    return mapped_records(b, read, &ffhip_batch::smd, "site mods were not made in this run (FFHIP_RUN_REMAP | FFHIP_RUN_REMAP_MODS)", rec, sm, nsite);
}

// ---- variants (include/ffhip.h "variants"; the kernel: ffhip_variants.hip)
extern "C" int ffhip_batch_set_remap_variants(ffhip_batch *b, int nread, const ffhip_variant *const *vars, const size_t *nvar, int context, int all_paths) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "variants: the batch is running (ffhip_batch_finish first)");
    if (!vars) { b->var.set.clear(); return FFHIP_OK; }
    if (!b->rmp.set) return set_err(FFHIP_EINVAL, "variants: no sequences are set for the batch (ffhip_batch_set_remap comes first)");
    if (!nvar || nread != batch_nreads(b) || (size_t)nread != b->rmp.seq.size()) return set_err(FFHIP_EINVAL, "variants: lists for %d reads, the batch holds %d", nread, batch_nreads(b));
    if (context < kVariantsMinContext || context > kVariantsMaxContext) return set_err(FFHIP_EINVAL, "variants: the context is %d (%d .. %d)", context, kVariantsMinContext, kVariantsMaxContext);
    std::vector<std::vector<ffhip_variant>> set((size_t)nread);
    for (int r = 0; r < nread; r++) {
        if (!nvar[r]) continue;
        if (!vars[r]) return set_err(FFHIP_EINVAL, "variants: read %d has %zu variants and no list", r, nvar[r]);
        if (nvar[r] > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "variants: read %d has %zu variants", r, nvar[r]);
        if (b->rmp.state[r] != 1) return set_err(FFHIP_EINVAL, "variants: read %d, index 0: the read has no sequence", r);
        for (size_t i = 0; i < nvar[r]; i++) {
            Variant v;
            memcpy(&v, &vars[r][i], sizeof v);
            if (const char *why = variant_invalid(v, b->rmp.seq[r].size(), b->mdl->nbase))
                return set_err(FFHIP_EINVAL, "variants: read %d, index %zu: %s (pos %d, nref %d, nalt %d, a sequence of %zu codes)", r, i, why, (int)v.pos, (int)v.nref, (int)v.nalt, b->rmp.seq[r].size());
        }
        set[r].assign(vars[r], vars[r] + nvar[r]);
    }
    b->var.set = std::move(set);
    b->var.context = context; b->var.all = all_paths ? 1 : 0;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_variant_calls(const ffhip_batch *b, int read, const ffhip_variant_call **vc, size_t *nvar) {
    int rec[4];
    return mapped_records(b, read, &ffhip_batch::var, "variants were not scored in this run (FFHIP_RUN_REMAP | FFHIP_RUN_REMAP_VARIANTS)", rec, vc, nvar);
}

// ---- truth (include/ffhip.h "truth"; the kernel: ffhip_truth.hip)
int ffhip::truth_adopt(ffhip_batch *b, std::vector<std::vector<uint8_t>> &&seq, std::vector<signed char> &&state, int band) {
    if (int rc = seq_adopt(b, seq, &b->tru.dseq, &b->tru.dseq_cap, "truth: the truths")) return rc;
    b->tru.seq = std::move(seq); b->tru.state = std::move(state);
    b->tru.band = band; b->tru.set = 1; b->tru.from_map = 0;
    return FFHIP_OK;
}
extern "C" int ffhip_batch_set_truth(ffhip_batch *b, int nread, const uint8_t *const *codes, const size_t *len, int band) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "truth: the batch is between a run and its finish");
    if (!codes) { b->tru.set = 0; b->tru.from_map = 0; b->tru.seq.clear(); b->tru.state.clear(); return FFHIP_OK; }
    const ffhip_model *m = b->mdl;
    if (m->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "truth: a flip-flop model only (the run-length model's call is a list of runs)");
    if (!len || nread != batch_nreads(b)) return set_err(FFHIP_EINVAL, "truth: truths for %d reads, the batch holds %d", nread, batch_nreads(b));
    if (int rc = truth_band_check("truth", band)) return rc;
    std::vector<std::vector<uint8_t>> seq((size_t)nread);
    std::vector<signed char> state((size_t)nread, 0);
    for (int r = 0; r < nread; r++) {
        if (!codes[r]) continue;
        if (len[r] > (size_t)kTruthMaxLen) return set_err(FFHIP_EINVAL, "truth: read %d's truth has %zu bases (at most %d)", r, len[r], kTruthMaxLen);
        state[r] = len[r] ? 1 : 2;
        if (const size_t i = bad_code(codes[r], len[r], m->nbase); i < len[r])
            return set_err(FFHIP_EINVAL, "truth: read %d, position %zu: code %d is not a base of the model (0 .. %d)", r, i, (int)codes[r][i], m->nbase - 1);
        seq[r].assign(codes[r], codes[r] + len[r]);
    }
    return truth_adopt(b, std::move(seq), std::move(state), band);
}
// truth from map (include/ffhip.h "truth from map"; the kernel: k_map_stretch, ffhip_map.hip)
extern "C" int ffhip_batch_set_truth_from_map(ffhip_batch *b, int on, int band) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "truth from map: the batch is between a run and its finish");
    if (!on) { b->tru.from_map = 0; return FFHIP_OK; }
    if (b->mdl->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "truth from map: a flip-flop model only (the run-length model's call is a list of runs)");
    if (int rc = truth_band_check("truth from map", band)) return rc;
    b->tru.seq.clear(); b->tru.state.clear();               // (the two ways of giving truths replace each other)
    b->tru.set = 0; b->tru.from_map = 1; b->tru.band = band;
    return FFHIP_OK;
}
// ---- the run-wide accumulators' objects (the kernels: ffhip_pileup, _modpileup, _consensus and _errprofile.hip).  What every one of them does alike:
static int pile_wait(ffhip_pile *p) {                            // every accumulation enqueued against it, by any batch, is done
    hipSetDevice(p->eng->device);
    for (int i = 0; i < p->eng->nstreams; i++)
        if (p->used[i]) { HIP_TRY(hipStreamSynchronize(p->eng->streams[i]), FFHIP_EHIP); p->used[i] = false; }
    return FFHIP_OK;
}
static int pile_zero(ffhip_pile *p, void *a, size_t abytes, void *b, size_t bbytes) {      // its two allocations (b may be none)
    hipStream_t s = p->eng->streams[0];
    HIP_TRY(hipMemsetAsync(a, 0, abytes, s), FFHIP_EHIP);
    if (b) HIP_TRY(hipMemsetAsync(b, 0, bbytes, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    return FFHIP_OK;
}
template <class Obj> static void pile_free(Obj *p, std::initializer_list<void **> bufs) {
    pile_wait(p);
    dev_free(bufs);
    delete p;
}
// attaching one to a batch: `slot` of the batch takes it (nullptr: none).  acgtz: a model with the modified base, else any flip-flop model
template <class Obj> static int pile_attach(ffhip_batch *b, Obj *p, Obj *ffhip_batch::*slot, const char *name, bool acgtz) {
    if (!b) return set_err(FFHIP_EINVAL, "null batch");
    if (b->ran && !b->finished) return set_err(FFHIP_EINVAL, "%s: the batch is between a run and its finish", name);
    if (!p) { b->*slot = nullptr; return FFHIP_OK; }
    if (acgtz && (b->mdl->kind == FFHIP_NET_LSTM5_RLE || b->mdl->nbase != 5)) return set_err(FFHIP_EINVAL, "%s: the model has no modified base (a model of the alphabet ACGTZ)", name);
    if (b->mdl->kind == FFHIP_NET_LSTM5_RLE) return set_err(FFHIP_EINVAL, "%s: a flip-flop model only (the run-length model's call is a list of runs)", name);
    if (p->eng != b->eng) return set_err(FFHIP_EINVAL, "%s: the %s belongs to another engine", name, name);
    b->*slot = p;
    return FFHIP_OK;
}
// ... and the three that count by a reference's positions: `planes` planes of P uint32 and `words` uint64 behind view.totals
struct PileKind { const char *name; int planes, words; };
static const PileKind kPileupKind = { "pileup", kPileupPlanes, kPileupTotals }, kModPileupKind = { "mod pileup", kModPileupPlanes, kModPileupTotals + kModPileupBins },
                      kConsensusKind = { "consensus", kConsensusPlanes, kConsensusTotals };
static int pile_zero(ffhip_pile *p, const PileView &v, const PileKind &k) { return pile_zero(p, v.counts, (size_t)k.planes * v.P * 4, v.totals, (size_t)k.words * 8); }
template <class Obj> static Obj *pile_create(const PileKind &k, ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity) {
    if (!eng || !ref || ref->eng != eng) { set_err(FFHIP_EINVAL, "%s: a reference of this engine", k.name); return nullptr; }
    if (min_identity > 1000) { set_err(FFHIP_EINVAL, "%s: min_identity is %d per mille (0 .. 1000)", k.name, min_identity); return nullptr; }
    hipSetDevice(eng->device);
    Obj *p = new Obj();
    p->eng = eng; p->ref = ref;
    size_t P = 0;
    for (int m : ref->rec_len) P += (size_t)m;
    p->view.P = P; p->view.min_identity = min_identity < 0 ? 0 : min_identity;
    const size_t bytes = (size_t)k.planes * P * 4, words = (size_t)k.words * 8;
    if (dev_fill(k.name, { { (void **)&p->view.counts, nullptr, bytes }, { (void **)&p->view.totals, nullptr, words } })) {
        set_err(FFHIP_ENOMEM, "%s: the counters take %zu bytes of device memory, which could not be had", k.name, bytes + words);
        delete p;
        return nullptr;
    }
    if (pile_zero(p, p->view, k) != FFHIP_OK) { pile_free(p, { (void **)&p->view.counts, (void **)&p->view.totals }); return nullptr; }
    return p;
}
// the planes and the first uint64 behind view.totals, once every accumulation is done
static int pile_download(ffhip_pile *p, const PileView &v, const PileKind &k, uint32_t *counts, void *totals, size_t totals_bytes) {
    if (int rc = pile_wait(p)) return rc;
    if (counts) HIP_TRY(hipMemcpy(counts, v.counts, (size_t)k.planes * v.P * 4, hipMemcpyDeviceToHost), FFHIP_EHIP);
    if (totals) HIP_TRY(hipMemcpy(totals, v.totals, totals_bytes, hipMemcpyDeviceToHost), FFHIP_EHIP);
    return FFHIP_OK;
}
// ---- pileup (include/ffhip.h "pileup"; the kernel: ffhip_pileup.hip)
extern "C" ffhip_pileup *ffhip_pileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity) { return pile_create<ffhip_pileup>(kPileupKind, eng, ref, min_identity); }
extern "C" void ffhip_pileup_free(ffhip_pileup *p) { if (p) pile_free(p, { (void **)&p->view.counts, (void **)&p->view.totals }); }
extern "C" int ffhip_pileup_reset(ffhip_pileup *p) {
    if (!p) return set_err(FFHIP_EINVAL, "null pileup");
    if (int rc = pile_wait(p)) return rc;
    return pile_zero(p, p->view, kPileupKind);
}
extern "C" size_t ffhip_pileup_positions(const ffhip_pileup *p) { return p ? p->view.P : 0; }
extern "C" int ffhip_pileup_download(ffhip_pileup *p, uint32_t *counts, ffhip_pileup_totals *totals) {
    if (!p) return set_err(FFHIP_EINVAL, "null pileup");
    static_assert(sizeof(ffhip_pileup_totals) == kPileupTotals * 8, "the totals come down as they stand");
    return pile_download(p, p->view, kPileupKind, counts, totals, sizeof *totals);
}
extern "C" int ffhip_batch_set_pileup(ffhip_batch *b, ffhip_pileup *p) { return pile_attach(b, p, &ffhip_batch::pile, "pileup", false); }
// ---- mod pileup (include/ffhip.h "mod pileup"; the kernel: ffhip_modpileup.hip): the totals and the histogram are one allocation, view.hist behind view.totals
extern "C" ffhip_modpileup *ffhip_modpileup_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity, int lo, int hi) {
    if (eng && ref && ref->eng == eng && min_identity <= 1000 && (lo < 0 || lo >= hi || hi > 255)) {      // (behind the refusals that pile_create words)
        set_err(FFHIP_EINVAL, "mod pileup: the thresholds are lo %d and hi %d (0 <= lo < hi <= 255)", lo, hi);
        return nullptr;
    }
    ffhip_modpileup *p = pile_create<ffhip_modpileup>(kModPileupKind, eng, ref, min_identity);
    if (p) { p->view.lo = lo; p->view.hi = hi; p->view.hist = p->view.totals + kModPileupTotals; }
    return p;
}
extern "C" void ffhip_modpileup_free(ffhip_modpileup *p) { if (p) pile_free(p, { (void **)&p->view.counts, (void **)&p->view.totals }); }
extern "C" int ffhip_modpileup_reset(ffhip_modpileup *p) {
    if (!p) return set_err(FFHIP_EINVAL, "null mod pileup");
    if (int rc = pile_wait(p)) return rc;
    return pile_zero(p, p->view, kModPileupKind);
}
extern "C" size_t ffhip_modpileup_positions(const ffhip_modpileup *p) { return p ? p->view.P : 0; }
extern "C" int ffhip_modpileup_download(ffhip_modpileup *p, uint32_t *counts, ffhip_modpileup_totals *totals, uint64_t *hist) {
    if (!p) return set_err(FFHIP_EINVAL, "null mod pileup");
    static_assert(sizeof(ffhip_modpileup_totals) == kModPileupTotals * 8 && FFHIP_MODPILEUP_PLANES == kModPileupPlanes, "the totals come down as they stand");
    if (int rc = pile_download(p, p->view, kModPileupKind, counts, totals, sizeof *totals)) return rc;
    if (hist) HIP_TRY(hipMemcpy(hist, p->view.hist, (size_t)kModPileupBins * 8, hipMemcpyDeviceToHost), FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" int ffhip_batch_set_modpileup(ffhip_batch *b, ffhip_modpileup *p) { return pile_attach(b, p, &ffhip_batch::modpile, "mod pileup", true); }
// ---- consensus (include/ffhip.h "consensus"; the kernels: ffhip_consensus.hip)
extern "C" ffhip_consensus *ffhip_consensus_create(ffhip_engine *eng, const ffhip_map_ref *ref, int min_identity) { return pile_create<ffhip_consensus>(kConsensusKind, eng, ref, min_identity); }
extern "C" void ffhip_consensus_free(ffhip_consensus *c) { if (c) pile_free(c, { (void **)&c->view.counts, (void **)&c->view.totals }); }
extern "C" int ffhip_consensus_reset(ffhip_consensus *c) {
    if (!c) return set_err(FFHIP_EINVAL, "null consensus");
    if (int rc = pile_wait(c)) return rc;
    return pile_zero(c, c->view, kConsensusKind);
}
extern "C" size_t ffhip_consensus_positions(const ffhip_consensus *c) { return c ? c->view.P : 0; }
extern "C" int ffhip_consensus_download(ffhip_consensus *c, uint32_t *counts, ffhip_consensus_totals *totals) {
    if (!c) return set_err(FFHIP_EINVAL, "null consensus");
    static_assert(sizeof(ffhip_consensus_totals) == kConsensusTotals * 8 && FFHIP_CONSENSUS_PLANES == kConsensusPlanes && FFHIP_CONSENSUS_MINOR == kConsensusMinor,
                  "the totals come down as they stand");
    return pile_download(c, c->view, kConsensusKind, counts, totals, sizeof *totals);
}
// the call: one launch over the planes as they stand, the cells through a buffer that lives for the call
extern "C" int ffhip_consensus_call(ffhip_consensus *c, int min_depth, ffhip_consensus_cell *cells) {
    if (!c || !cells) return set_err(FFHIP_EINVAL, "null consensus or cells");
    static_assert(sizeof(ffhip_consensus_cell) == 16, "a cell is one 16-byte store of k_consensus_call");
    static_assert(FFHIP_CONSENSUS_LOW == kConsensusLow && FFHIP_CONSENSUS_SAME == kConsensusSame && FFHIP_CONSENSUS_SUB == kConsensusSub &&
                  FFHIP_CONSENSUS_DEL == kConsensusDel && FFHIP_CONSENSUS_INS == kConsensusIns, "the kernel's codes are the header's");
    if (min_depth < 1) return set_err(FFHIP_EINVAL, "consensus: min_depth is %d (1 or more: a position nobody covers has no winner)", min_depth);
    if (int rc = pile_wait(c)) return rc;
    const size_t bytes = c->view.P * sizeof *cells;
    void *d_cells = nullptr;
    if (dev_fill("consensus cells", { { &d_cells, nullptr, bytes } })) return set_err(FFHIP_ENOMEM, "consensus: the cells take %zu bytes of device memory, which could not be had", bytes);
    hipStream_t s = c->eng->streams[0];
    launch_consensus_call(s, c->ref->view, c->view, (unsigned)min_depth, d_cells);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cells, d_cells, bytes, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    dev_free({ &d_cells });
    HIP_TRY(e, FFHIP_EHIP);
    HIP_TRY(e2, FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" int ffhip_batch_set_consensus(ffhip_batch *b, ffhip_consensus *c) { return pile_attach(b, c, &ffhip_batch::cons, "consensus", false); }
// ---- error profile (include/ffhip.h "error profile"; the kernel: ffhip_errprofile.hip): one allocation, by class and of no reference
extern "C" ffhip_errprofile *ffhip_errprofile_create(ffhip_engine *eng, int min_identity) {
    if (!eng) { set_err(FFHIP_EINVAL, "error profile: an engine"); return nullptr; }
    if (min_identity > 1000) { set_err(FFHIP_EINVAL, "error profile: min_identity is %d per mille (0 .. 1000)", min_identity); return nullptr; }
    hipSetDevice(eng->device);
    ffhip_errprofile *p = new ffhip_errprofile();
    p->eng = eng;
    p->view.min_identity = min_identity < 0 ? 0 : min_identity;
    p->groups = std::max(1, eng->prop.multiProcessorCount);
    if (dev_fill("error profile", { { (void **)&p->view.counts, nullptr, (size_t)kErrWords * 8 } })) {
        set_err(FFHIP_ENOMEM, "error profile: the counters take %zu bytes of device memory, which could not be had", (size_t)kErrWords * 8);
        delete p;
        return nullptr;
    }
    if (ffhip_errprofile_reset(p) != FFHIP_OK) { ffhip_errprofile_free(p); return nullptr; }
    return p;
}
extern "C" void ffhip_errprofile_free(ffhip_errprofile *p) { if (p) pile_free(p, { (void **)&p->view.counts }); }
extern "C" int ffhip_errprofile_reset(ffhip_errprofile *p) {
    if (!p) return set_err(FFHIP_EINVAL, "null error profile");
    if (int rc = pile_wait(p)) return rc;
    return pile_zero(p, p->view.counts, (size_t)kErrWords * 8, nullptr, 0);
}
extern "C" size_t ffhip_errprofile_words(void) { return (size_t)kErrWords; }
extern "C" int ffhip_errprofile_download(ffhip_errprofile *p, uint64_t *counts, ffhip_errprofile_totals *totals) {
    if (!p) return set_err(FFHIP_EINVAL, "null error profile");
    static_assert(sizeof(ffhip_errprofile_totals) == kErrTotals * 8 && FFHIP_ERRPROFILE_WORDS == kErrWords && FFHIP_ERRPROFILE_TABLE_WORDS == kErrTableWords &&
                  FFHIP_ERRPROFILE_SUB == kErrAtSub && FFHIP_ERRPROFILE_INS == kErrAtIns && FFHIP_ERRPROFILE_QUAL == kErrAtQual && FFHIP_ERRPROFILE_CTX == kErrAtCtx &&
                  FFHIP_ERRPROFILE_HP == kErrAtHp && FFHIP_ERRPROFILE_HP_MAX_RUN == kErrHpMaxRun && FFHIP_ERRPROFILE_HP_MAX_CALLED == kErrHpMaxCalled &&
                  FFHIP_ERRPROFILE_HP_MAX_OPS == kErrHpMaxOps, "the counters come down as they stand, in the header's sections");
    if (int rc = pile_wait(p)) return rc;
    if (counts) HIP_TRY(hipMemcpy(counts, p->view.counts, (size_t)kErrTableWords * 8, hipMemcpyDeviceToHost), FFHIP_EHIP);
    if (totals) HIP_TRY(hipMemcpy(totals, p->view.counts + kErrTableWords, sizeof *totals, hipMemcpyDeviceToHost), FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" int ffhip_batch_set_errprofile(ffhip_batch *b, ffhip_errprofile *p) { return pile_attach(b, p, &ffhip_batch::errp, "error profile", false); }
// test hook: the most workgroups of the object's later launches (0: the engine's compute units again), so that a workgroup's walk over several reads can be held
// to one read a workgroup
extern "C" int ffhip_debug_errprofile_groups(ffhip_errprofile *p, int groups) {
    if (!p || groups < 0) return set_err(FFHIP_EINVAL, "error profile: an object and 0 or more workgroups");
    p->groups = groups ? groups : std::max(1, p->eng->prop.multiProcessorCount);
    return FFHIP_OK;
}
// test hook: between a run in the mode of truth from map and its finish, the stretches k_map_stretch gathered for k_truth are zeroed behind k_truth, on the batch's
// stream -- what a re-run on the f32 path whose map record moved leaves stale.  Whatever the finish launches must not read them
extern "C" int ffhip_debug_batch_clear_stretches(ffhip_batch *b) {
    if (!b || !b->ran || b->finished || !b->tru.from_map || !b->tru.dseq) return set_err(FFHIP_EINVAL, "clear stretches: a batch in the mode of truth from map, between a run and its finish");
    hipSetDevice(b->eng->device);
    HIP_TRY(hipMemsetAsync(b->tru.dseq, 0, b->tru.dseq_cap, b->stream), FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" long long ffhip_debug_map_truth_bound(int nblock, int max_error) {
    return (nblock < 0 || max_error < 0 || max_error > 500) ? -1 : map_truth_bound(nblock, max_error);
}
extern "C" int ffhip_batch_truth(const ffhip_batch *b, int read, ffhip_truth_call *out) {
    if (!results_ok(b, read) || !out) return FFHIP_EINVAL;
    if (!b->tru.valid || !b->tru.rec.host) return set_err(FFHIP_EINVAL, "truth records were not made in this run (FFHIP_RUN_TRUTH)");
    int rec[kTruthRecInts];
    memcpy(rec, b->tru.rec.host + (size_t)read * sizeof rec, sizeof rec);
    truth_unpack(rec, out);
    if (rec[0] == 1) {
        const size_t cap = b->tru.off[read + 1] - b->tru.off[read];
        if (rec[10] != 0 || out->nops > cap) return set_err(FFHIP_EHIP, "truth: read %d's traceback ended %d cells from (0, 0)", read, rec[10]);
        out->ops = b->tru.rec.host + truth_ops_at(b) + b->tru.off[read + 1] - out->nops;
    }
    return FFHIP_OK;
}

extern "C" int ffhip_debug_remap_form(size_t L, int band) { return (L < 1 || L > ((size_t)1 << 30) || band < 0) ? -1 : remap_form((int)L, band); }
extern "C" int ffhip_debug_remap_from_map_form(int nblock, int band) {      // the form a read of nblock blocks takes in the mode of remap from map: that of its room
    return (nblock < 1 || nblock >= (1 << 30) || band < 0) ? -1 : remap_form(nblock + 1, band);
}
extern "C" int ffhip_debug_truth_form(size_t window) { return (window < 1 || window > ((size_t)1 << 30)) ? -1 : truth_form((long long)window); }

// distances and end positions of every pattern of a kit at both ends of one call (k_barcodes; include/ffhip.h "barcodes")
extern "C" int ffhip_op_barcode_scores(ffhip_engine *eng, const ffhip_barcodes *kit, const char *bases, size_t len, int32_t *dist, int32_t *end) {
    OP_ENTER(eng);
    if (!kit || kit->eng != eng || (!bases && len) || !dist || !end || len > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "bad barcode score arguments (a kit of this engine, a call of len characters, two outputs of 2 n entries)");
    if (const size_t i = bad_letter(bases, len); i < len) return set_err(FFHIP_EINVAL, "barcode scores: character %zu of the call is not one of ACGTZ", i);
    const int n = kit->kit.n, ilen = (int)len;
    char *d_bases = (char *)(len ? tmp.upload(bases, len, s) : tmp.get(4));
    int *d_len = (int *)tmp.upload(&ilen, 4, s);
    int *d_out = (int *)tmp.get((size_t)4 * n * 4);
    void *d_rec = tmp.get(16);
    if (!d_bases || !d_len || !d_out || !d_rec) OP_NOMEM();
    launch_barcodes(s, kit->kit, d_bases, d_len, d_rec, 1, ilen > 0 ? ilen : 1, nullptr, ReadMap(), barcodes_max_dist(kit, -1), barcodes_min_sep(-1), 0, d_out, d_out + 2 * n);
    HIP_TRY(hipMemcpyAsync(dist, d_out, (size_t)2 * n * 4, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipMemcpyAsync(end, d_out + 2 * n, (size_t)2 * n * 4, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    return FFHIP_OK;
}

// the kernel of the adapter search on one call (k_adapters; include/ffhip.h "adapters"): the whole score rows, or the call's record
static int op_adapters(ffhip_engine *eng, const ffhip_adapters *kit, int max_dist, const char *bases, size_t len, uint8_t *d, ffhip_adapter_header *header, ffhip_adapter_hit *hits) {
    OP_ENTER(eng);
    if (!kit || kit->eng != eng || (!bases && len) || len > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "bad adapter arguments (a kit of this engine, a call of len characters, the outputs)");
    if (const size_t i = bad_letter(bases, len); i < len) return set_err(FFHIP_EINVAL, "adapters: character %zu of the call is not one of ACGTZ", i);
    const int n = kit->kit.n, ilen = (int)len;
    const size_t dbytes = d ? (size_t)2 * n * (len + 1) : 0;
    char *d_bases = (char *)(len ? tmp.upload(bases, len, s) : tmp.get(4));
    int *d_len = (int *)tmp.upload(&ilen, 4, s);
    uint8_t *d_d = d ? (uint8_t *)tmp.get(dbytes) : nullptr;
    uint8_t *d_rec = (uint8_t *)tmp.get(kAdapterRecBytes);
    if (!d_bases || !d_len || (d && !d_d) || !d_rec) OP_NOMEM();
    launch_adapters(s, kit->kit, d_bases, d_len, d_rec, 1, ilen > 0 ? ilen : 1, nullptr, ReadMap(), max_dist, d_d);
    if (d) HIP_TRY(hipMemcpyAsync(d, d_d, dbytes, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (header) HIP_TRY(hipMemcpyAsync(header, d_rec, 16, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (hits) HIP_TRY(hipMemcpyAsync(hits, d_rec + 16, kAdapterRecBytes - 16, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" int ffhip_op_adapter_scores(ffhip_engine *eng, const ffhip_adapters *kit, const char *bases, size_t len, uint8_t *d) {
    if (!d) return set_err(FFHIP_EINVAL, "adapter scores: an output of 2 n (len + 1) bytes");
    return op_adapters(eng, kit, -1, bases, len, d, nullptr, nullptr);
}
extern "C" int ffhip_op_adapter_hits(ffhip_engine *eng, const ffhip_adapters *kit, int max_dist, const char *bases, size_t len, ffhip_adapter_header *header, ffhip_adapter_hit *hits) {
    if (!header || !hits) return set_err(FFHIP_EINVAL, "adapter hits: a header and room for 15 hits");
    return op_adapters(eng, kit, adapters_max_dist(max_dist), bases, len, nullptr, header, hits);
}

// the kernels of the map on one call (k_map_scan, k_map_finish; include/ffhip.h "map"): the whole score rows of its front anchor, or the call's record
static int op_map(ffhip_engine *eng, const ffhip_map_ref *ref, int window, int max_error, const char *bases, size_t len, int32_t *d, ffhip_map_call *out) {
    OP_ENTER(eng);
    if (!ref || ref->eng != eng || (!bases && len) || len > (size_t)1 << 30) return set_err(FFHIP_EINVAL, "bad map arguments (a reference of this engine, a call of len characters, the output)");
    if (const char *why = map_invalid(window, max_error)) return set_err(FFHIP_EINVAL, "map: %s", why);
    if (const size_t i = bad_letter(bases, len); i < len) return set_err(FFHIP_EINVAL, "map: character %zu of the call is not one of ACGTZ", i);
    map_defaults(&window, &max_error);
    const int ilen = (int)len;
    const size_t dbytes = d ? ref->score_entries * 4 : 0;
    char *d_bases = (char *)(len ? tmp.upload(bases, len, s) : tmp.get(4));
    int *d_len = (int *)tmp.upload(&ilen, 4, s);
    int *d_d = d ? (int *)tmp.get(dbytes) : nullptr;
    void *d_slots = tmp.get((size_t)2 * ref->view.ntask * 8);
    uint8_t *d_rec = (uint8_t *)tmp.get(kMapRecBytes);
    if (!d_bases || !d_len || (d && !d_d) || !d_slots || !d_rec) OP_NOMEM();
    launch_map(s, ref->view, d_bases, d_len, d_rec, 1, ilen > 0 ? ilen : 1, nullptr, ReadMap(), window, max_error, d_slots, d_d);
    if (d) HIP_TRY(hipMemcpyAsync(d, d_d, dbytes, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (out) HIP_TRY(hipMemcpyAsync(out, d_rec, kMapRecBytes, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    return FFHIP_OK;
}
extern "C" int ffhip_op_map_scores(ffhip_engine *eng, const ffhip_map_ref *ref, const char *pattern, size_t len, int32_t *d) {
    if (!d) return set_err(FFHIP_EINVAL, "map scores: an output of twice the sum of m_k + 1 entries");
    if (len < 1 || len > (size_t)kMapMaxAnchor) return set_err(FFHIP_EINVAL, "map scores: an anchor has 1 .. %d letters, not %zu", kMapMaxAnchor, len);
    return op_map(eng, ref, kMapMaxAnchor, -1, pattern, len, d, nullptr);
}
extern "C" int ffhip_op_map(ffhip_engine *eng, const ffhip_map_ref *ref, int window, int max_error, const char *bases, size_t len, ffhip_map_call *out) {
    if (!out) return set_err(FFHIP_EINVAL, "map: a record to fill");
    return op_map(eng, ref, window, max_error, bases, len, nullptr, out);
}

// the gather of truth from map on one span from host arguments (k_map_stretch; include/ffhip.h "truth from map"): a record and a list entry made here
extern "C" int ffhip_op_map_stretch(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, uint8_t *codes) {
    OP_ENTER(eng);
    if (!ref || ref->eng != eng || !codes) return set_err(FFHIP_EINVAL, "bad map stretch arguments (a reference of this engine, an output of end - start bytes)");
    if (int rc = span_check("map stretch", ref, q, start, end)) return rc;
    const int m = end - start;
    ffhip_map_call rec;
    memset(&rec, 0, sizeof rec);
    rec.status = 1; rec.nanchor = 1; rec.q = q; rec.tstart = start; rec.tend = end;
    const TruthRead tr{ 0ull, 0ull, 0u, 0, 1, 0, 0, m };
    void *d_rec = tmp.upload(&rec, sizeof rec, s);
    TruthRead *d_list = (TruthRead *)tmp.upload(&tr, sizeof tr, s);
    uint8_t *d_seq = (uint8_t *)tmp.get((size_t)m);
    if (!d_rec || !d_list || !d_seq) OP_NOMEM();
    launch_map_stretch(s, ref->view, d_rec, d_list, 1, d_seq);
    TruthRead got;
    HIP_TRY(hipMemcpyAsync(&got, d_list, sizeof got, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipMemcpyAsync(codes, d_seq, (size_t)m, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (int rc = op_done(s)) return rc;
    if (got.status != 1 || got.m != m) return set_err(FFHIP_EHIP, "map stretch: the kernel left status %d and %d bases for a span of %d", got.status, got.m, m);
    return FFHIP_OK;
}

// the coding of remap from map on one span from host arguments (k_map_remap_seq; include/ffhip.h "remap from map"): a record and a list entry made here, the
// entry's room given as the blocks of a batch of one read.  *status and *L are what the kernel patched; out holds L entries when *status is 1 and is untouched otherwise
extern "C" int ffhip_op_map_remap_code(ffhip_engine *eng, const ffhip_map_ref *ref, int q, int start, int end, int nbase, int room, uint16_t *out, int *status, size_t *L) {
    OP_ENTER(eng);
    if (!ref || ref->eng != eng || !out || !status || !L) return set_err(FFHIP_EINVAL, "bad map remap code arguments (a reference of this engine, an output of end - start entries, a status and a length)");
    if (nbase != 4 && nbase != 5) return set_err(FFHIP_EINVAL, "map remap code: an alphabet of 4 or 5 bases, not %d", nbase);
    if (room < 0 || room > (1 << 30)) return set_err(FFHIP_EINVAL, "map remap code: a room of 0 .. 2^30 positions, not %d", room);
    if (int rc = span_check("map remap code", ref, q, start, end)) return rc;
    const int m = end - start;
    ffhip_map_call rec;
    memset(&rec, 0, sizeof rec);
    rec.status = 1; rec.nanchor = 1; rec.q = q; rec.tstart = start; rec.tend = end;
    const RemapRead rr{ 0ull, 0u, 0, 1, 0 };
    void *d_rec = tmp.upload(&rec, sizeof rec, s);
    RemapRead *d_list = (RemapRead *)tmp.upload(&rr, sizeof rr, s);
    unsigned short *d_seq = (unsigned short *)tmp.get((size_t)std::max(room, 1) * 2);
    if (!d_rec || !d_list || !d_seq) OP_NOMEM();
    launch_map_remap_seq(s, ref->view, d_rec, d_list, 1, d_seq, nbase, room - 1, nullptr);
    RemapRead got;
    HIP_TRY(hipMemcpyAsync(&got, d_list, sizeof got, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (int rc = op_done(s)) return rc;
    if (got.L != m || (got.status != 1 && got.status != 2) || (got.status == 1) != (m <= room))
        return set_err(FFHIP_EHIP, "map remap code: the kernel left status %d and %d bases for a span of %d in a room of %d", got.status, got.L, m, room);
    if (got.status == 1) {
        HIP_TRY(hipMemcpyAsync(out, d_seq, (size_t)m * 2, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
        if (int rc = op_done(s)) return rc;
    }
    *status = got.status; *L = (size_t)got.L;
    return FFHIP_OK;
}

// one alignment from host arguments added into an accumulator: the checks of all four, then a map record, a truth record and a list entry made here, and the ops and
// the call on the device -- what a launch takes (PileArgs)
static int pile_op(const char *who, TmpDev &tmp, hipStream_t s, const ffhip_map_ref *ref, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops, PileArgs *out) {
    if (ref) { if (int rc = span_check(who, ref, q, tstart, tend)) return rc; }      // (no reference: the error profile of a given truth, [0, m))
    else if (tstart != 0 || tend < 1) return set_err(FFHIP_EINVAL, "%s: a truth of 1 or more bases", who);
    if (n > (size_t)kTruthMaxLen || nops > (size_t)2 * kTruthMaxLen) return set_err(FFHIP_EINVAL, "%s: a call of %zu bases and %zu ops (at most %d bases)", who, n, nops, kTruthMaxLen);
    if (const size_t i = bad_letter(call, n); i < n) return set_err(FFHIP_EINVAL, "%s: position %zu of the call: '%c' is not one of A C G T Z", who, i, call[i]);
    const size_t m = (size_t)(tend - tstart);
    size_t cnt[4] = { 0, 0, 0, 0 };
    for (size_t k = 0; k < nops; k++) {
        if (ops[k] > 3) return set_err(FFHIP_EINVAL, "%s: op %zu: code %d is not one of 0 .. 3", who, k, (int)ops[k]);
        cnt[ops[k]]++;
    }
    if (cnt[0] + cnt[1] + cnt[3] != m || cnt[0] + cnt[1] + cnt[2] != n)
        return set_err(FFHIP_EINVAL, "%s: the ops consume %zu truth and %zu call bases, the span has %zu and the call %zu", who, cnt[0] + cnt[1] + cnt[3], cnt[0] + cnt[1] + cnt[2], m, n);
    ffhip_map_call mrec;
    memset(&mrec, 0, sizeof mrec);
    mrec.status = 1; mrec.n = (int)n; mrec.nanchor = 1; mrec.q = q; mrec.tstart = tstart; mrec.tend = tend;
    const int trec[kTruthRecInts] = { 1, (int)n, (int)m, (int)(cnt[1] + cnt[2] + cnt[3]), (int)cnt[0], (int)cnt[1], (int)cnt[2], (int)cnt[3], 0, (int)nops, 0, 0 };
    const TruthRead tr{ 0ull, 0ull, 0u, (int)m, 1, 0, (int)nops, 0 };
    *out = { (const TruthRead *)tmp.upload(&tr, sizeof tr, s), 1, tmp.upload(&mrec, sizeof mrec, s), (const int *)tmp.upload(trec, sizeof trec, s),
             (const uint8_t *)tmp.upload(ops, nops, s), (const char *)tmp.upload(n ? call : "", n ? n : 1, s), n > 0 ? (int)n : 1, ReadMap() };
    if (!out->list || !out->map_records || !out->truth_records || !out->ops || !out->bases) OP_NOMEM();
    return FFHIP_OK;
}
extern "C" int ffhip_op_pileup(ffhip_engine *eng, ffhip_pileup *p, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops) {
    OP_ENTER(eng);
    if (!p || p->eng != eng || (n && !call) || !ops) return set_err(FFHIP_EINVAL, "bad pileup arguments (a pileup of this engine, a call of n letters, nops ops)");
    PileArgs d;
    if (int rc = pile_op("pileup", tmp, s, p->ref, q, tstart, tend, call, n, ops, nops, &d)) return rc;
    launch_pileup(s, p->ref->view, d, p->view);
    return op_done(s);
}
extern "C" int ffhip_op_consensus(ffhip_engine *eng, ffhip_consensus *c, int q, int tstart, int tend, const char *call, size_t n, const uint8_t *ops, size_t nops) {
    OP_ENTER(eng);
    if (!c || c->eng != eng || (n && !call) || !ops) return set_err(FFHIP_EINVAL, "bad consensus arguments (a consensus of this engine, a call of n letters, nops ops)");
    PileArgs d;
    if (int rc = pile_op("consensus", tmp, s, c->ref, q, tstart, tend, call, n, ops, nops, &d)) return rc;
    launch_consensus(s, c->ref->view, d, c->view);
    return op_done(s);
}
// ... into an error profile (k_errprofile): with a reference the truth's letters are its span's, else the m codes given
static int errprofile_op(ffhip_engine *eng, ffhip_errprofile *p, const ffhip_map_ref *ref, int q, int tstart, int tend, const char *call, const char *qual, size_t n,
                         const uint8_t *truth, const uint8_t *ops, size_t nops) {
    OP_ENTER(eng);
    if (!p || p->eng != eng || (n && (!call || !qual)) || !ops || (ref ? ref->eng != eng : !truth))
        return set_err(FFHIP_EINVAL, "bad error profile arguments (an error profile of this engine, a call of n letters with its n quality characters, a truth or a reference of this engine, nops ops)");
    PileArgs d;
    if (int rc = pile_op("error profile", tmp, s, ref, q, tstart, tend, call, n, ops, nops, &d)) return rc;
    const size_t m = (size_t)(tend - tstart);
    if (!ref) if (const size_t j = bad_code(truth, m, 5); j < m) return set_err(FFHIP_EINVAL, "error profile: position %zu of the truth: code %d is not one of 0 .. 4", j, (int)truth[j]);
    const char *d_qual = (const char *)tmp.upload(n ? qual : "", n ? n : 1, s);
    const uint8_t *d_truth = ref ? nullptr : (const uint8_t *)tmp.upload(truth, m, s);
    if (!d_qual || (!ref && !d_truth)) OP_NOMEM();
    launch_errprofile(s, ref ? &ref->view : nullptr, d, 1, d_qual, d_truth, p->view);
    return op_done(s);
}
extern "C" int ffhip_op_errprofile(ffhip_engine *eng, ffhip_errprofile *p, const char *call, const char *qual, size_t n, const uint8_t *truth, size_t m, const uint8_t *ops, size_t nops) {
    if (m > (size_t)kTruthMaxLen) return set_err(FFHIP_EINVAL, "error profile: a truth of %zu bases (at most %d)", m, kTruthMaxLen);
    return errprofile_op(eng, p, nullptr, 0, 0, (int)m, call, qual, n, truth, ops, nops);
}
extern "C" int ffhip_op_errprofile_mapped(ffhip_engine *eng, ffhip_errprofile *p, const ffhip_map_ref *ref, int q, int tstart, int tend, const char *call, const char *qual, size_t n,
                                          const uint8_t *ops, size_t nops) {
    if (!ref) return set_err(FFHIP_EINVAL, "error profile: a reference of this engine");
    return errprofile_op(eng, p, ref, q, tstart, tend, call, qual, n, nullptr, ops, nops);
}
extern "C" int ffhip_op_modpileup(ffhip_engine *eng, ffhip_modpileup *p, int q, int tstart, int tend, const char *call, const uint8_t *ml, size_t n, const uint8_t *ops, size_t nops) {
    OP_ENTER(eng);
    if (!p || p->eng != eng || (n && (!call || !ml)) || !ops)
        return set_err(FFHIP_EINVAL, "bad mod pileup arguments (a mod pileup of this engine, a call of n letters with its n 5mC bytes, nops ops)");
    PileArgs d;
    if (int rc = pile_op("mod pileup", tmp, s, p->ref, q, tstart, tend, call, n, ops, nops, &d)) return rc;
    const uint8_t zero = 0;
    const uint8_t *d_ml = (const uint8_t *)tmp.upload(n ? ml : &zero, n ? n : 1, s);
    if (!d_ml) OP_NOMEM();
    launch_modpileup(s, p->ref->view, d, d_ml, p->view);
    return op_done(s);
}

// one matrix of transition scores mapped to one sequence (k_remap; include/ffhip.h "remap")
extern "C" int ffhip_op_remap(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, int band, uint8_t *rm, float *score) {
    OP_ENTER(eng);
    if (!codes || !rm || !score || nbase < 1 || 2 * nbase > kMaxState || !trans_ok(trans, nbase) || trans.nc > (size_t)1 << 30)
        return set_err(FFHIP_EINVAL, "bad remap arguments (scores of 2 nbase (nbase + 1) rows, a sequence, outputs of nblock bytes and one float)");
    const size_t N = trans.nc;
    if (band < 0) return set_err(FFHIP_EINVAL, "remap: the band half-width is %d (>= 0)", band);
    if (L < 1 || L > N + 1) return set_err(FFHIP_EINVAL, "remap: a sequence of %zu bases has no path through %zu blocks (1 <= L <= nblock + 1)", L, N);
    if (const size_t i = bad_code(codes, L, nbase); i < L) return set_err(FFHIP_EINVAL, "remap: position %zu: code %d is not a base (0 .. %d)", i, (int)codes[i], nbase - 1);
    const int form = remap_form((int)L, band);
    if (form < 0) return set_err(FFHIP_EINVAL, "remap: the window of min(2 band + 1, L) cells is more than %d", remap_max_window());
    std::vector<unsigned short> coded(L);
    remap_code(codes, L, nbase, coded.data());
    const RemapRead rr{ 0ull, 0u, (int)L, 1, 0 };
    float *d_t = mat_in(tmp, trans, s);
    unsigned short *d_seq = (unsigned short *)tmp.upload(coded.data(), L * sizeof(unsigned short), s);
    RemapRead *d_list = (RemapRead *)tmp.upload(&rr, sizeof rr, s);
    const size_t ws_bytes = remap_ws_words(form, (int)N) * 8;
    unsigned long long *d_ws = (unsigned long long *)tmp.get(ws_bytes);
    uint8_t *d_rm = (uint8_t *)tmp.get(N + 1);
    void *d_rec = tmp.get(16);
    if (!d_ws) return set_err(FFHIP_ENOMEM, "remap: the traceback workspace takes %zu bytes of device memory, which could not be had", ws_bytes);
    if (!d_t || !d_seq || !d_list || !d_rm || !d_rec) OP_NOMEM();
    launch_remap(s, form, d_list, 1, d_seq, d_t, (int)trans.stride, band, d_ws, d_rec, d_rm, (int)N, nullptr, ReadMap());
    int rec[4];
    HIP_TRY(hipMemcpyAsync(rec, d_rec, 16, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    // (L and N were checked above: the kernel's only status 2 is the score's, a property of the input and no failure of the device)
    if (rec[0] == 2) return set_err(FFHIP_EINVAL, "remap: the score V_N[L - 1] is not finite: the scores leave no finite path (a NaN or an infinity among the entries it reads, or sums past float32)");
    if (rec[0] != 1 || rec[3] != 0) return set_err(FFHIP_EHIP, "remap: status %d, traceback ended at position %d", rec[0], rec[3]);
    HIP_TRY(hipMemcpyAsync(rm, d_rm, N, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    memcpy(score, &rec[2], 4);
    return FFHIP_OK;
}

// the poly tail of one read from its signal and its Viterbi path (k_polytail; include/ffhip.h "poly tail"): the record, or the windows' values
static int op_polytail(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const int *path, size_t nblock, int nbase, const ffhip_polytail_params *params,
                       ffhip_polytail *out, double *mu, double *q, uint8_t *flag) {
    OP_ENTER(eng);
    if (!path || !params || (nsample && !signal)) return set_err(FFHIP_EINVAL, "bad poly tail arguments (a signal, a path of nblock + 1 states, the parameters, the outputs)");
    if (stride < 1 || nblock < 1 || nblock > (size_t)1 << 30 || nsample > (size_t)1 << 30 || (nbase != 4 && nbase != 5))
        return set_err(FFHIP_EINVAL, "poly tail: stride %d, %zu blocks, %zu samples, nbase %d (a stride >= 1, 1 .. 2^30 blocks, at most 2^30 samples, nbase 4 or 5)", stride, nblock, nsample, nbase);
    const PolyTailParams p = polytail_params(params);
    if (const char *why = polytail_invalid(p)) return set_err(FFHIP_EINVAL, "poly tail: %s", why);
    for (size_t i = 0; i <= nblock; i++) if (path[i] < 0 || path[i] >= 2 * nbase) return set_err(FFHIP_EINVAL, "poly tail: entry %zu of the path is %d (a state, 0 .. %d)", i, path[i], 2 * nbase - 1);
    const size_t NW = std::min(nblock, nsample / (size_t)stride) / (size_t)p.window, room = NW ? NW : 1;
    const PolyRead pr{ 0ull, 0ull, (int)nsample, 0 };
    const float none = 0.0f;
    float *d_x = (float *)tmp.upload(nsample ? signal : &none, (nsample ? nsample : 1) * sizeof(float), s);
    int *d_path = (int *)tmp.upload(path, (nblock + 1) * 4, s);
    PolyRead *d_list = (PolyRead *)tmp.upload(&pr, sizeof pr, s);
    double *d_mu = (double *)tmp.get(room * 8), *d_q = (double *)tmp.get(room * 8);
    uint8_t *d_fl = (uint8_t *)tmp.get(room), *d_rec = (uint8_t *)tmp.get(kPolyTailRecBytes);
    if (!d_x || !d_path || !d_list || !d_mu || !d_q || !d_fl || !d_rec) OP_NOMEM();
    launch_polytail(s, d_list, 1, d_x, stride, d_path, nbase, p, d_rec, d_mu, d_fl, d_q, (int)nblock, nullptr, ReadMap());
    if (out) HIP_TRY(hipMemcpyAsync(out, d_rec, kPolyTailRecBytes, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (mu && NW) {
        HIP_TRY(hipMemcpyAsync(mu, d_mu, NW * 8, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
        HIP_TRY(hipMemcpyAsync(q, d_q, NW * 8, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
        HIP_TRY(hipMemcpyAsync(flag, d_fl, NW, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    }
    HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP);
    if (mu) for (size_t w = 0; w < NW; w++) flag[w] &= 1;       // (bit 1 is the scan's: the window ends a candidate)
    return FFHIP_OK;
}
extern "C" int ffhip_op_polytail(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const int *path, size_t nblock, int nbase,
                                 const ffhip_polytail_params *params, ffhip_polytail *out) {
    if (!out) return set_err(FFHIP_EINVAL, "poly tail: an output record");
    return op_polytail(eng, signal, nsample, stride, path, nblock, nbase, params, out, nullptr, nullptr, nullptr);
}
extern "C" int ffhip_op_polytail_windows(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const int *path, size_t nblock, int nbase,
                                         const ffhip_polytail_params *params, double *mu, double *q, uint8_t *flag) {
    if (!mu || !q || !flag) return set_err(FFHIP_EINVAL, "poly tail windows: three outputs of NW entries");
    return op_polytail(eng, signal, nsample, stride, path, nblock, nbase, params, nullptr, mu, q, flag);
}

// the events of one read from its signal and its path (k_events; include/ffhip.h "events")
extern "C" int ffhip_op_events(ffhip_engine *eng, const float *signal, size_t nsample, int stride, const uint8_t *rm, size_t nblock, size_t L, ffhip_event *out) {
    OP_ENTER(eng);
    if (!rm || !out || (nsample && !signal)) return set_err(FFHIP_EINVAL, "bad events arguments (a signal, a path of nblock bytes and L events of output)");
    if (stride < 1 || nblock < 1 || L < 1 || nblock > (size_t)1 << 30 || nsample > (size_t)1 << 30)
        return set_err(FFHIP_EINVAL, "events: stride %d, %zu blocks, %zu samples and %zu bases (a stride >= 1, 1 .. 2^30 blocks, at most 2^30 samples, L >= 1)", stride, nblock, nsample, L);
    if (int rc = path_check("events", rm, nblock, L)) return rc;
    const EventRead er{ 0ull, 0ull, (int)nsample, (int)L, 0, 0 };
    const unsigned rec[4] = { 1u, (unsigned)L, 0u, 0u };
    const float none = 0.0f;
    float *d_x = (float *)tmp.upload(nsample ? signal : &none, (nsample ? nsample : 1) * sizeof(float), s);
    uint8_t *d_rm = (uint8_t *)tmp.upload(rm, nblock, s);
    EventRead *d_list = (EventRead *)tmp.upload(&er, sizeof er, s);
    void *d_rec = tmp.upload(rec, sizeof rec, s);
    void *d_ev = tmp.get(L * sizeof(ffhip_event));
    if (!d_ev) return set_err(FFHIP_ENOMEM, "events: the events take %zu bytes of device memory, which could not be had", L * sizeof(ffhip_event));
    if (!d_x || !d_rm || !d_list || !d_rec) OP_NOMEM();
    launch_events(s, d_list, 1, d_x, stride, d_rec, d_rm, d_ev, (int)nblock, nullptr, ReadMap());
    HIP_TRY(hipMemcpyAsync(out, d_ev, L * sizeof(ffhip_event), hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    return op_done(s);
}

// Site mods and variants of one read, what their operators share.  check: the path and the codes, behind the operator's own checks of its arguments, and the
// sequence coded.  upload, once the operator has its entries (the sites; the variants) and there are any: scores, sequence, path, a list of this one read, the
// entries, a record of status 1, and room for the starts and a 16-byte record an entry.  download: the records, and whether the kernels ran.
namespace {
struct SiteOp {
    std::vector<unsigned short> coded;
    SiteRead sr{}; unsigned rec[4] = { 1u, 0u, 0u, 0u };          // (the asynchronous uploads read them: they live as long as the call)
    float *d_t = nullptr; unsigned short *d_seq = nullptr; uint8_t *d_rm = nullptr; SiteRead *d_list = nullptr; void *d_ent = nullptr, *d_rec = nullptr, *d_out = nullptr; int *d_start = nullptr;
    int check(const char *who, int nbase, const uint8_t *codes, size_t L, const uint8_t *rm, size_t nblock) {
        if (int rc = path_check(who, rm, nblock, L)) return rc;
        if (const size_t i = bad_code(codes, L, nbase); i < L) return set_err(FFHIP_EINVAL, "%s: position %zu: code %d is not a base (0 .. %d)", who, i, (int)codes[i], nbase - 1);
        coded.resize(L);
        remap_code(codes, L, nbase, coded.data());
        return FFHIP_OK;
    }
    int upload(const char *who, TmpDev &tmp, hipStream_t s, const ffhip_mat &trans, const uint8_t *rm, size_t nblock, const void *ent, size_t ent_bytes, size_t nent) {
        const size_t L = coded.size();
        sr = SiteRead{ 0ull, 0u, (int)L, 0, 0 };
        rec[1] = (unsigned)L;
        d_t = mat_in(tmp, trans, s);
        d_seq = (unsigned short *)tmp.upload(coded.data(), L * sizeof(unsigned short), s);
        d_rm = (uint8_t *)tmp.upload(rm, nblock, s);
        d_list = (SiteRead *)tmp.upload(&sr, sizeof sr, s);
        d_ent = tmp.upload(ent, ent_bytes, s);
        d_rec = tmp.upload(rec, sizeof rec, s);
        d_start = (int *)tmp.get((L + 1) * 4);
        d_out = tmp.get(nent * 16);
        if (!d_start || !d_out) return set_err(FFHIP_ENOMEM, "%s: the records and starts take %zu bytes of device memory, which could not be had", who, nent * 16 + (L + 1) * 4);
        if (!d_t || !d_seq || !d_rm || !d_list || !d_ent || !d_rec) OP_NOMEM();
        return FFHIP_OK;
    }
    int download(hipStream_t s, void *out, size_t nent) const {
        HIP_TRY(hipMemcpyAsync(out, d_out, nent * 16, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
        return op_done(s);
    }
};
}  // namespace

// the site mods of one read from its scores, its sequence and its path (k_site_starts + k_site_mods; include/ffhip.h "site mods")
extern "C" int ffhip_op_site_mods(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, const uint8_t *rm, size_t nblock, int context, int all_paths,
                                  ffhip_site_mod *out, size_t *nsite) {
    OP_ENTER(eng);
    if (nbase != 5) return set_err(FFHIP_EINVAL, "site mods: nbase is %d (a model of the alphabet ACGTZ: 5)", nbase);
    if (!codes || !rm || !out || !nsite || !trans_ok(trans, nbase))
        return set_err(FFHIP_EINVAL, "bad site mods arguments (scores of 2 nbase (nbase + 1) rows, a sequence, a path of nblock bytes, records and their count)");
    if (context < 0 || context > kSiteModsMaxContext) return set_err(FFHIP_EINVAL, "site mods: the context is %d (0 .. %d)", context, kSiteModsMaxContext);
    if (nblock < 1 || nblock != trans.nc || L < 1 || nblock > (size_t)1 << 30)
        return set_err(FFHIP_EINVAL, "site mods: %zu blocks of path, %zu of scores and %zu bases (the same 1 .. 2^30 blocks, L >= 1)", nblock, trans.nc, L);
    SiteOp o;
    if (int rc = o.check("site mods", nbase, codes, L, rm, nblock)) return rc;
    std::vector<SiteMod> sites;
    *nsite = sitemods_sites(o.coded.data(), L, 0, &sites);
    if (sites.empty()) return FFHIP_OK;
    if (int rc = o.upload("site mods", tmp, s, trans, rm, nblock, sites.data(), sites.size() * sizeof(SiteMod), sites.size())) return rc;
    launch_site_mods(s, o.d_list, 1, (const SiteMod *)o.d_ent, (int)sites.size(), o.d_seq, o.d_t, (int)trans.stride, context, all_paths ? 1 : 0, o.d_rec, o.d_rm, o.d_start, o.d_out,
                     (int)nblock, nullptr, ReadMap());
    return o.download(s, out, sites.size());
}

// the variants of one read from its scores, its sequence and its path (k_site_starts + k_variants; include/ffhip.h "variants")
extern "C" int ffhip_op_variants(ffhip_engine *eng, ffhip_mat trans, int nbase, const uint8_t *codes, size_t L, const uint8_t *rm, size_t nblock,
                                 const ffhip_variant *vars, size_t nvar, int context, int all_paths, ffhip_variant_call *out) {
    OP_ENTER(eng);
    if (nbase != 4 && nbase != 5) return set_err(FFHIP_EINVAL, "variants: nbase is %d (4 or 5)", nbase);
    if (!codes || !rm || (nvar && (!vars || !out)) || !trans_ok(trans, nbase))
        return set_err(FFHIP_EINVAL, "bad variants arguments (scores of 2 nbase (nbase + 1) rows, a sequence, a path of nblock bytes, variants and room for their records)");
    if (context < kVariantsMinContext || context > kVariantsMaxContext) return set_err(FFHIP_EINVAL, "variants: the context is %d (%d .. %d)", context, kVariantsMinContext, kVariantsMaxContext);
    if (nblock < 1 || nblock != trans.nc || L < 1 || nblock > (size_t)1 << 30 || nvar > (size_t)1 << 30)
        return set_err(FFHIP_EINVAL, "variants: %zu blocks of path, %zu of scores, %zu bases and %zu variants (the same 1 .. 2^30 blocks, L >= 1)", nblock, trans.nc, L, nvar);
    SiteOp o;
    if (int rc = o.check("variants", nbase, codes, L, rm, nblock)) return rc;
    std::vector<VarEntry> list(nvar);
    for (size_t i = 0; i < nvar; i++) {
        list[i].k = 0; list[i].index = (int)i;
        memcpy(&list[i].v, &vars[i], sizeof(Variant));
        if (const char *why = variant_invalid(list[i].v, L, nbase))
            return set_err(FFHIP_EINVAL, "variants: read 0, index %zu: %s (pos %d, nref %d, nalt %d, a sequence of %zu codes)", i, why, (int)vars[i].pos, (int)vars[i].nref, (int)vars[i].nalt, L);
    }
    if (!nvar) return FFHIP_OK;
    if (int rc = o.upload("variants", tmp, s, trans, rm, nblock, list.data(), nvar * sizeof(VarEntry), nvar)) return rc;
    launch_variants(s, o.d_list, 1, (const VarEntry *)o.d_ent, (int)nvar, o.d_seq, o.d_t, (int)trans.stride, nbase, context, all_paths ? 1 : 0, o.d_rec, o.d_rm, o.d_start, o.d_out,
                    (int)nblock, nullptr, ReadMap());
    return o.download(s, out, nvar);
}

// one call aligned to one truth (k_truth; include/ffhip.h "truth")
extern "C" int ffhip_op_truth(ffhip_engine *eng, const char *call, size_t n, const uint8_t *truth, size_t m, int band, ffhip_truth_call *out, uint8_t *ops) {
    OP_ENTER(eng);
    if (!out || (n && !call) || (m && !truth) || ((n + m) && !ops)) return set_err(FFHIP_EINVAL, "bad truth arguments (a call, a truth, a record and n + m bytes of ops)");
    if (n > (size_t)kTruthMaxLen || m > (size_t)kTruthMaxLen) return set_err(FFHIP_EINVAL, "truth: a call of %zu and a truth of %zu bases (at most %d each)", n, m, kTruthMaxLen);
    if (int rc = truth_band_check("truth", band)) return rc;
    if (const size_t i = bad_letter(call, n); i < n) return set_err(FFHIP_EINVAL, "truth: position %zu of the call: '%c' is not one of A C G T Z", i, call[i]);
    if (const size_t i = bad_code(truth, m, 5); i < m) return set_err(FFHIP_EINVAL, "truth: position %zu of the truth: code %d is not a base (0 .. 4)", i, (int)truth[i]);
    const int form = truth_form(std::min<long long>(2ll * band + 1, (long long)n + 1));
    const int ni = (int)n, cap = (int)(n + m);
    const TruthRead tr{ 0ull, 0ull, 0u, (int)m, m ? 1 : 2, 0, cap, 0 };
    char *d_call = (char *)tmp.upload(n ? call : "", n ? n : 1, s);
    uint8_t *d_seq = (uint8_t *)tmp.upload(m ? truth : (const uint8_t *)"", m ? m : 1, s);
    int *d_len = (int *)tmp.upload(&ni, 4, s);
    TruthRead *d_list = (TruthRead *)tmp.upload(&tr, sizeof tr, s);
    const size_t ws_bytes = truth_ws_words(form, (int)m) * 8;
    unsigned long long *d_ws = (unsigned long long *)tmp.get(ws_bytes ? ws_bytes : 8);
    uint8_t *d_ops = (uint8_t *)tmp.get(cap ? cap : 1);
    int *d_rec = (int *)tmp.get(kTruthRecInts * 4);
    if (!d_ws) return set_err(FFHIP_ENOMEM, "truth: the traceback workspace takes %zu bytes of device memory, which could not be had", ws_bytes);
    if (!d_call || !d_seq || !d_len || !d_list || !d_ops || !d_rec) OP_NOMEM();
    // (Tb = max(n, 1): a read of no blocks is an empty slot to the kernel, which then reads no length)
    launch_truth(s, form, d_list, 1, d_seq, d_call, d_len, band, d_ws, d_rec, d_ops, ni > 0 ? ni : 1, nullptr, ReadMap());
    int rec[kTruthRecInts];
    std::vector<uint8_t> got((size_t)cap);
    HIP_TRY(hipMemcpyAsync(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (cap) HIP_TRY(hipMemcpyAsync(got.data(), d_ops, (size_t)cap, hipMemcpyDeviceToHost, s), FFHIP_EHIP);
    if (int rc = op_done(s)) return rc;
    truth_unpack(rec, out);
    if (rec[0] == 1) {
        if (rec[10] != 0 || rec[9] < 0 || rec[9] > cap) return set_err(FFHIP_EHIP, "truth: the traceback ended %d cells from (0, 0)", rec[10]);
        memcpy(ops, got.data() + cap - rec[9], (size_t)rec[9]);
    }
    return FFHIP_OK;
}
