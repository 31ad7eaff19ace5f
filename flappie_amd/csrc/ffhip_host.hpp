// ffhip_host.hpp -- host-side helpers shared by ffhip_engine.hip, ffhip_features.hip and ffhip_layers.hip (not public).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <vector>

#include "../../include/ffhip.h"
#include "ffhip_internal.hpp"

constexpr int kEngineStreams = 4;

struct ffhip_engine {
    int device = 0;
    hipDeviceProp_t prop;
    hipStream_t streams[kEngineStreams] = {};      // batches take them in turn (FFHIP_DEBUG=streams=2..4)
    int nstreams = kEngineStreams, next_stream = 0;
    int profiling = 0;
    // Persistent recurrent kernels spin on their peers: every workgroup of a launch must be resident.
    // Two batches (streams) may run such kernels at the same time only if both fit; otherwise the
    // launches are chained through this event.
    hipEvent_t persist_done = nullptr;
    hipEvent_t head_done = nullptr; int head_done_rec = 0;      // behind the CRF head of the last batch run: a packed batch's set-up waits for it (ffhip_engine.hip apply_packed)
    int persist_chained = 0;
    hipEvent_t batch_done = nullptr;     // end of the last submitted batch (any stream): see run_front, "whole batches one after the other"
    int batch_done_rec = 0;
    hipEvent_t done_ring[4] = { nullptr, nullptr, nullptr, nullptr };      // end of the decode of the last four submitted batches (before their copies to the host)
    unsigned done_head = 0;
    int persist_last_half = 0;  // the engine's last persistent launch left room for a twin of its size: only then may the next half-chip launch run beside it
    // A persistent layer kernel whose workgroups are not all resident (another tenant on the GPU, e.g. a second flappie
    // process) gives up through its bounded waits (abort word).  ffhip_batch_finish then re-runs the batch on the
    // launch-per-step kernels, which need no co-residency, and the next `stepwise_batches` runs go there directly:
    // co-tenancy becomes a slowdown, not FFHIP_ETIMEOUT.
    int stepwise_batches = 0;
    int fallbacks = 0;          // how often that happened (ffhip_debug_fallback_count)
    unsigned long long f32_reruns = 0;      // reads that left the split format's range and were run again on the f32 path (ffhip_engine_f32_reruns)
    int in_flight = 0;          // batches between ffhip_batch_run and ffhip_batch_finish: kernels of a batch submitted beside another
                                // take the shapes that fit next to a resident layer launch (k_conv_split<2, 2>)
    // Signal preparation (ffhip_prep.hip) runs on a stream of its own -- beside the batches, not queued behind one of them -- and
    // keeps its buffers: a pinned staging area (one packed upload per chunk instead of one per read), the kernel's scratch, and a
    // pool of output buffers handed to ffhip_prep objects (hipMalloc / hipFree per chunk would synchronise the device each time).
    hipStream_t prep_stream = nullptr;
    void *prep_pin = nullptr;
    size_t prep_pin_cap = 0;
    void *prep_scratch[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };      // raw floats, chunk MADs, tables, statistics + calibrations, DAC values
    size_t prep_scratch_cap[5] = { 0, 0, 0, 0, 0 };
    ffhip_prep *prep_pending = nullptr;             // the one preparation begun and not finished (these buffers are its)
    std::vector<std::pair<void *, size_t>> prep_pool;       // free output buffers (pointer, bytes)
    double rehearsal_busy_until = 0.0;                      // FFHIP_DEBUG_HOST_REHEARSAL_MSPS (ffhip_engine.hip): when the emulated GPU is free again
};

struct ffhip_prep;

// a barcode kit on the device (ffhip_barcodes_upload; the kernel's view of it is BarcodeKit)
struct ffhip_barcodes {
    ffhip_engine *eng = nullptr;
    ffhip::BarcodeKit kit{};
    int lmin = 0;                       // the shortest pattern: the default max_dist is lmin / 4
    void *d_peq = nullptr, *d_len = nullptr;
};

// an adapter kit on the device (ffhip_adapters_upload; the kernel's view of it is AdapterKit)
struct ffhip_adapters {
    ffhip_engine *eng = nullptr;
    ffhip::AdapterKit kit{};
    void *d_peq = nullptr, *d_len = nullptr;
};

// a reference on the device (ffhip_map_ref_upload; the kernels' view of it is MapRefView): the coded letters, the records' table, the task list, the score rows' starts
struct ffhip_map_ref {
    ffhip_engine *eng = nullptr;
    ffhip::MapRefView view{};
    void *d_words = nullptr, *d_tasks = nullptr, *d_recs = nullptr, *d_rowoff = nullptr;
    size_t score_entries = 0;           // of all 2 K score rows together: the sum of m_k + 1, twice
    std::vector<int> rec_len;           // [nrec]: the records' letters, on the host (ffhip_op_map_stretch checks its span against them)
};

// a run-wide accumulator on the device: counters which the batches it is attached to add to on their own streams -- `used` says which of the engine's streams hold
// such work that nothing has waited for yet.  ref: the reference whose positions it counts by (the error profile: none)
struct ffhip_pile {
    ffhip_engine *eng = nullptr;
    const ffhip_map_ref *ref = nullptr;
    bool used[kEngineStreams] = {};
};
// a pileup (ffhip_pileup_create; the kernel's view of it is PileupView): 12 planes of P uint32 and eight uint64 totals
struct ffhip_pileup : ffhip_pile { ffhip::PileupView view{}; };
// a mod pileup (ffhip_modpileup_create; the kernel's view of it is ModPileupView): 10 planes of P uint32, and eight uint64 totals with the 256 uint64 bins of the
// histogram behind them in one allocation
struct ffhip_modpileup : ffhip_pile { ffhip::ModPileupView view{}; };
// a consensus (ffhip_consensus_create; the kernels' view of it is ConsensusView): 37 planes of P uint32 and eight uint64 totals
struct ffhip_consensus : ffhip_pile { ffhip::ConsensusView view{}; };
// an error profile (ffhip_errprofile_create; the kernel's view of it is ErrProfileView): kErrWords uint64, the tables and the twelve totals behind them.
// groups: the most workgroups of a launch (the engine's compute units; ffhip_debug_errprofile_groups sets another)
struct ffhip_errprofile : ffhip_pile { ffhip::ErrProfileView view{}; int groups = 1; };

// a function or table one file of the library defines for another and the library does not export
#define FFHIP_LOCAL __attribute__((visibility("hidden")))

namespace ffhip {

int set_err(int code, const char *fmt, ...);        // records the thread's last error text, returns `code`

#define HIP_TRY(expr, ret)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            ffhip::set_err(FFHIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return ret;                                                                             \
        }                                                                                           \
    } while (0)

// W(row m, k) accessor -> A-fragment order [Mt][K16][64 lanes][4]; rows/cols beyond the matrix are 0
template <class F>
static std::vector<float> pack_afrag(int Mt, int K16, F w) {
    std::vector<float> out((size_t)Mt * K16 * 256, 0.0f);
    for (int mt = 0; mt < Mt; mt++)
        for (int k16 = 0; k16 < K16; k16++)
            for (int lane = 0; lane < 64; lane++) {
                const int i = lane & 15, kq = lane >> 4;
                for (int e = 0; e < 4; e++)
                    out[(((size_t)mt * K16 + k16) * 64 + lane) * 4 + e] = w(mt * 16 + i, k16 * 16 + kq * 4 + e);
            }
    return out;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// strided-convolution column plan (layers.c:216-271 restated in index space); returns Tout, <0 on failure
int build_conv_plan(int T, int winlen, int s, std::vector<int> &a, std::vector<int> &bq);

// Process-wide pool of device buffers (power-of-two size classes from 4 KiB): the device images that flappie matrices own and
// the scratch of the single-matrix calls.  hipMalloc / hipFree per call cost more than the kernels of a one-read call, and hipFree
// synchronises the device.  A buffer goes back only when no enqueued work uses it (the single-matrix calls are synchronous).
void *pool_get(size_t bytes);
void pool_put(void *p);
void pool_trim(int device);           // hipFree every unused buffer of that device (its last engine is destroyed)
void pool_engine_born(int device);
bool pool_engine_gone(int device);    // true: it was the device's last engine
int pool_default_device();
int pool_device_of(const void *p);    // -1: not a pool buffer
void pool_state(unsigned long long out[4]);
#ifdef FFHIP_TEST_HOOKS
double rehearsal_rate();              // test hook FFHIP_DEBUG_HOST_REHEARSAL_MSPS (ffhip_engine.hip; the `make hooks` build only); <= 0: off
bool rehearsal_nogpu();
#else
static inline double rehearsal_rate() { return 0.0; }      // the release library: no hook, the code behind it folds away
static inline bool rehearsal_nogpu() { return false; }
#endif
void image_remember(const void *owner, void *dev);
void *image_forget(const void *owner);

// every host<->device copy of the library goes through these: ffhip_copy_counts (include/ffhip.h)
hipError_t counted_memcpy_async(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s);
hipError_t counted_memcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind);
hipError_t counted_memcpy_2d_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s);
#define hipMemcpyAsync(...) ::ffhip::counted_memcpy_async(__VA_ARGS__)
#define hipMemcpy(...) ::ffhip::counted_memcpy(__VA_ARGS__)
#define hipMemcpy2DAsync(...) ::ffhip::counted_memcpy_2d_async(__VA_ARGS__)

// scratch device allocations of one single-matrix call
struct TmpDev {
    std::vector<void *> p;
    ~TmpDev() { for (void *q : p) pool_put(q); }
    void *get(size_t bytes) {
        void *d = pool_get(bytes ? bytes : 4);
        if (d) p.push_back(d);
        return d;
    }
    void *upload(const void *host, size_t bytes, hipStream_t s) {
        void *d = get(bytes);
        if (d && hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
        return d;
    }
};

// ---- device images of flappie matrices (include/ffhip.h, "flappie matrices with a device image")
int matrix_policy();
static inline bool mat_has_dev(const ffhip_mat &m) { return m.dev && m.dev_state && *m.dev && *m.dev_state >= 1 && matrix_policy() != 0; }
// the image an operator READS: the matrix's device image when it has one, an uploaded copy of the host image otherwise
static inline float *mat_in(TmpDev &t, const ffhip_mat &m, hipStream_t s) {
    if (mat_has_dev(m)) return (float *)*m.dev;
    return (float *)t.upload(m.data, m.nc * m.stride * sizeof(float), s);
}
// the image an operator WRITES: `lazy` (the result stays on the device, the matrix owns the buffer) or scratch to be downloaded
static inline float *mat_out(TmpDev &t, const ffhip_mat &m, bool lazy) {
    const size_t bytes = m.nc * m.stride * sizeof(float);
    if (lazy && m.dev && m.dev_state) {
        if (!*m.dev) *m.dev = pool_get(bytes);
        return (float *)*m.dev;
    }
    return (float *)t.get(bytes);
}
// after the kernels that wrote `d` were enqueued on s: mark the device image current (lazy) or download it
static inline hipError_t mat_done(const ffhip_mat &m, float *d, bool lazy, hipStream_t s) {
    if (lazy && m.dev && m.dev_state && d == (float *)*m.dev) { *m.dev_state = 2; return hipSuccess; }
    if (m.dev && m.dev_state && *m.dev && d != (float *)*m.dev) { pool_put(*m.dev); *m.dev = nullptr; *m.dev_state = 0; }      // a reused output: its old device image is stale
    return hipMemcpyAsync(m.data, d, m.nc * m.stride * sizeof(float), hipMemcpyDeviceToHost, s);
}

// how every single-matrix and single-read operator starts, and what it says when its scratch could not be had
#define OP_ENTER(eng_)                                                     \
    if (!(eng_)) return set_err(FFHIP_EINVAL, "null engine");              \
    hipSetDevice((eng_)->device);                                          \
    hipStream_t s = (eng_)->streams[0];                                    \
    TmpDev tmp
#define OP_NOMEM() return set_err(FFHIP_ENOMEM, "device allocation failed")

static inline bool view_ok(const ffhip_mat &m) { return m.data && m.nr > 0 && m.nc > 0 && m.stride >= m.nr; }

static inline bool flipflop_dims(size_t nparam, size_t stride, int *nbase) {
    const int nb = (int)roundf((-1.0f + sqrtf(1.0f + 2.0f * (float)nparam)) / 2.0f);
    if (nb < 1 || (size_t)(2 * nb * (nb + 1)) != nparam || 2 * nb > kMaxState || nparam > 64 || stride < nparam) return false;
    *nbase = nb;
    return true;
}

// device address and length of a prepared read's kept samples (ffhip_prep.hip); nullptr if rejected
const float *prep_device_signal(const struct ::ffhip_prep *p, int read, size_t *len);
void prep_mark_used(const struct ::ffhip_prep *p, hipStream_t s);      // an asynchronous reader of the prepared signals was enqueued on s

}  // namespace ffhip
