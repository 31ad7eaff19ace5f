// ffhip_annot.hpp -- the per-read products of a batch that live OUTSIDE its result block, described once (host only, no kernels; included by ffhip_batch.hpp).
// Barcodes, adapters, the map, the poly tail, truth, remap, events, site mods and variants each bring their records to the host in a buffer and a copy of their own.  Such a buffer is a
// Mirrored (below), a feature is a struct of its own in ffhip_batch that starts as an Annot, and kAnnots (ffhip_features.hip, behind the features' functions) has one
// row a feature, in launch order.  To add a per-read product outside the block one writes
//   its struct        struct Thing : Annot { <parameters, lists, workspaces, per-read offsets> } thing;      (ffhip_batch in ffhip_batch.hpp, and its place in ffhip_batch::annot)
// and in ffhip_features.hip
//   its two functions thing_prepare (run_front: lists, workspaces, room in `rec`), thing_launch (run_back: the kernel)
//   its two layouts   thing_bytes (what a finished run brings down), thing_spans (where a read's record lies in `rec`: at most two pieces)
//   its row           { FFHIP_RUN_THING, <the text without FFHIP_RUN_REMAP, or nullptr>, <nbase, the model's text>, <the undecoded text>, the four functions }
//   its setter, accessor and operator   ffhip_batch_set_thing, ffhip_batch_thing: b->thing.rec.host + ..., ffhip_op_thing; each check through its one helper ("each check once")
// and nothing in ffhip_engine.hip, whose front, back, finish, f32 re-run, rehearsal and destroy reach the features through the declarations at the end of this file only.
#pragma once
#include <string.h>

#include "ffhip_host.hpp"

struct ffhip_batch;

namespace ffhip {

// the batch's device allocator (ffhip_engine.hip): a buffer the batch owns and counts (zero: filled on the batch's stream), and one that grows -- the old one is
// given back first, once the batch's stream has drained
void *dalloc(ffhip_batch *b, size_t bytes, bool zero);
int dgrow(ffhip_batch *b, void **p, size_t *cap, size_t need, const char *what);

// A device buffer of the batch and its pinned host mirror.  The device half belongs to the batch's allocator (ffhip_batch_destroy frees it with the rest), the
// host half to this.  Room comes in exactly two ways; `what` names the buffer in the text of a failure, as "remap: the records and moves".
struct Mirrored {
    uint8_t *dev = nullptr, *host = nullptr;
    size_t dev_cap = 0, host_cap = 0;

    // `bytes` on first use, both halves zero (a read without blocks may never be written by its kernel and must read as zeros); it never grows
    int fixed(ffhip_batch *b, size_t bytes, const char *what) {
        if (!dev) {
            if (!(dev = (uint8_t *)dalloc(b, bytes, true))) return set_err(FFHIP_ENOMEM, "%s takes %zu bytes of device memory, which could not be had", what, bytes);
            dev_cap = bytes;
        }
        return host ? FFHIP_OK : pin(bytes, what);
    }
    // at least `need` bytes: a buffer that is too small is given back once the stream has drained (a run that was never finished may still read it) and a new one
    // taken, the device half as it comes, the host half zero.  Nothing is kept.
    int grow(ffhip_batch *b, hipStream_t s, size_t need, const char *what) {
        if (int rc = dgrow(b, (void **)&dev, &dev_cap, need, what)) return rc;
        if (host && need <= host_cap) return FFHIP_OK;
        if (host) { HIP_TRY(hipStreamSynchronize(s), FFHIP_EHIP); release(); }
        return pin(need, what);
    }
    int copy_down(size_t n, hipStream_t s) const { HIP_TRY(hipMemcpyAsync(host, dev, n, hipMemcpyDeviceToHost, s), FFHIP_EHIP); return FFHIP_OK; }
    int copy_up(size_t n, hipStream_t s) const { HIP_TRY(hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, s), FFHIP_EHIP); return FFHIP_OK; }
    void release() { if (host) hipHostFree(host); host = nullptr; host_cap = 0; }

private:
    int pin(size_t bytes, const char *what) {
        if (hipHostMalloc((void **)&host, bytes, hipHostMallocDefault) != hipSuccess) {
            host = nullptr;
            return set_err(FFHIP_ENOMEM, "%s take %zu bytes of pinned host memory, which could not be had", what, bytes);
        }
        host_cap = bytes;
        memset(host, 0, bytes);
        return FFHIP_OK;
    }
};

// what every feature's struct starts with: its records, the list its front uploads for its kernel (if it has one), and whether the last run made the records
struct Annot { Mirrored rec, list; int valid = 0; };

// a piece of a read's record in `rec`
struct AnnotSpan { size_t at = 0, bytes = 0; };

// One row a feature.  The front clears `valid`, and for a run with `flag`: refuses it without FFHIP_RUN_REMAP (remap_text; nullptr: the feature stands alone),
// on the run-length model or -- nbase != 0 -- a flip-flop model of another alphabet (model_text; nullptr: any model remap takes) and undecoded (undecoded_text;
// nullptr: remap's row has asked), then calls prepare.  The back calls launch, which sets `valid`.  A finished run brings bytes() of `rec` down, if any; the f32
// re-run puts a read's spans() back, both halves.
struct AnnotRow {
    unsigned flag;
    const char *remap_text;
    int nbase;
    const char *model_text, *undecoded_text;
    int (*prepare)(ffhip_batch *);
    void (*launch)(ffhip_batch *, const int *tbr, ReadMap rmap);
    size_t (*bytes)(const ffhip_batch *);
    void (*spans)(const ffhip_batch *, int read, AnnotSpan out[2]);
};

// ---- what ffhip_engine.hip asks of ffhip_features.hip: the table (ffhip_batch::AN_COUNT rows), the front's and the finish's share of all features and of the
// run-wide accumulators, and rerun_on_f32_path's way of handing its side batch the re-run reads' sequences and truths
FFHIP_LOCAL extern const AnnotRow kAnnots[];
FFHIP_LOCAL int annots_prepare(ffhip_batch *b, unsigned flags);
FFHIP_LOCAL int annots_copy_down(ffhip_batch *b);
FFHIP_LOCAL int piles_check(const ffhip_batch *b, unsigned flags);
FFHIP_LOCAL void pileup_launch(ffhip_batch *b);
FFHIP_LOCAL void modpileup_launch(ffhip_batch *b);
FFHIP_LOCAL void consensus_launch(ffhip_batch *b);
FFHIP_LOCAL void errprofile_launch(ffhip_batch *b);
FFHIP_LOCAL int remap_adopt(ffhip_batch *b, std::vector<std::vector<unsigned short>> &&seq, std::vector<signed char> &&state, int band);
FFHIP_LOCAL int truth_adopt(ffhip_batch *b, std::vector<std::vector<uint8_t>> &&seq, std::vector<signed char> &&state, int band);

}  // namespace ffhip
