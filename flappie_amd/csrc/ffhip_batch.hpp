// ffhip_batch.hpp -- the resident model and the batch as ffhip_engine.hip (the runs) and ffhip_features.hip (the per-read features) see them: types and inline accessors, no behaviour (host only, not public).
#pragma once
#include "ffhip_results.hpp"
#include "ffhip_annot.hpp"

using namespace ffhip;      // (both files that include this say so themselves: the types below were written in ffhip_engine.hip's scope and moved as they stood)

// ------------------------------------------------------------------------------------ model
struct ConvDev {
    int Fin = 0, Fout = 0, winlen = 0, stride = 1;
    float *taps = nullptr;      // [Fout][winlen][Fin]   (VALU layers)
    float *bias = nullptr;      // [Fout] or [Mpad] for the MFMA layer
    float4 *Wp = nullptr;       // A-fragment order     (last layer)
    int K16 = 0, Mpad = 0;
    void *Wsplit = nullptr;     // last layer with 16 input features: fp16 slices in 16x16x32 A order for k_conv_split (ffhip_split.hpp)
    int split_S = 0;            // exponent its accumulators carry: weight exponent + kSplitExpX
};
struct RnnDev {
    float4 *iWp = nullptr, *sWp = nullptr;
    float *bias = nullptr;      // [4*Hp] permuted rows
    int Kin16 = 0;
    void *Wsplit = nullptr;     // both matrices as 16-bit slices in MFMA 16x16x32 A order (ffhip_rnn_split.hip, ffhip_split.hpp), or nullptr
    int split_S = 0;            // the power-of-two exponent both products of this layer carry: sw(Wi) + e(x) = sw(sW) + e(h)
};

struct ffhip_model {
    ffhip_engine *eng = nullptr;
    int kind = 0, cell = 0, nconv = 0, G = 4;
    int H = 0, Hp = 0;          // hidden units, padded to a multiple of 16
    int P = 0, Ps = 0, nbase = 0, nstate = 0;
    int act = ACT_SWISH;
    ConvDev conv[3];
    RnnDev rnn[5];
    float4 *FFp = nullptr;
    float *FFb = nullptr;
    void *FFsplit = nullptr;    // the head's weights as fp16 slices in 16x16x32 A order (k_head_split: reads the last layer's split output)
    int FF_split_S = 0;         // exponent its accumulators carry: weight exponent + kSplitExpH
    std::vector<void *> owned;
};

// ------------------------------------------------------------------------------------ a run's path (decided by plan_run, ffhip_engine.hip)
struct RunPath {
    bool keep = false, persist = false, fused = false;           // FFHIP_RUN_KEEP_ACTS; one launch per layer (and chunk of read tiles); the f32 layer kernel with the projection inside
    bool proj_split = false, split = false, split2 = false;      // projections on split operands; ModelPath::split; H = 512 (and FFHIP_RUN_UNFUSED_RNN at H = 256):
                                                                 // projection GEMM + recurrence-only layer kernel, both on split operands
    bool conv_split = false, conv_f16 = false;                   // the last convolution writes the split layout / runs on split operands (its predecessor writes fp16 slices)
    bool split_head = false, packable = false;                   // the CRF head reads the last layer's split output (k_head_split: no fp32 copy of it); a packed batch may take the run
    bool post_done = false, head_e = false, rle_post8 = false;   // 8- / 10-state flip-flop models, a block's scores spanning at most kFbRange: ONE pair of fp64 linear-space chains
                                                                 // per read gives logZ, the normalised scores and the posterior (k_crf_fb); head_e: their input exp(S - block max)
                                                                 // comes from the split head's epilogue; rle_post8: the run-length model's posterior from such chains (k_rle_post8)
    int R = 0, gates = 2, persist_mode = 0, rnn_path = 0;       // rescaling interval of the linear-space CRF normalisation (0: log space); gate_level; hand-off of the persistent
                                                                 // layer kernels (0: write-through where a group spans XCDs); ffhip_batch_rnn_path
};

// ------------------------------------------------------------------------------------ batch
struct ConvPlan { int Tin = 0, Tout = 0; int *x0a = nullptr, *x0b = nullptr; };

struct ffhip_batch {
    ffhip_engine *eng = nullptr;
    const ffhip_model *mdl = nullptr;
    hipStream_t stream = nullptr;
    int nread = 0, B16 = 0, Bp = 0;
    int T = 0, Tb = 0;                  // capacity: samples / blocks of the longest read the batch can take
    ConvPlan plan[3];
    // ragged batch (reads of different lengths, all <= T): per-read window tables, block counts and tile maxima
    bool ragged = false;
    std::vector<int> hT, hTb;           // samples / blocks of each read
    // host images of the tables below: they stay alive here so that their uploads can be asynchronous on the batch's stream (a
    // synchronous copy or a stream synchronisation in the set-up path waits for compute slots the other batch's layer launches hold)
    // (pinned: an asynchronous copy from pageable memory is staged by the runtime and may block the caller)
    struct Pinned {
        void *p = nullptr; size_t cap = 0;
        void *get(size_t bytes) {
            if (cap >= bytes && p) return p;
            if (p) hipHostFree(p);
            p = nullptr; cap = 0;
            if (hipHostMalloc(&p, bytes + bytes / 4 + 64, hipHostMallocDefault) != hipSuccess) return nullptr;
            cap = bytes + bytes / 4 + 64;
            return p;
        }
        ~Pinned() { if (p) hipHostFree(p); }
    };
    Pinned h_tin[3], h_ta[3], h_tq[3], h_tbs, h_tbt, h_glen, h_gsrc, h_rehearsal;
    int *d_tbs = nullptr, *d_tbt = nullptr;
    int *rag_x0a[3] = { nullptr, nullptr, nullptr }, *rag_x0b[3] = { nullptr, nullptr, nullptr };
    int *rag_tin[3] = { nullptr, nullptr, nullptr };       // stride-1 thin layers: per-read input lengths replace the table
    // Packed batch (ffhip_batch_set_*_packed): the `nread` rows of the buffers are SLOTS, each holding one or more reads one behind the other with a gap of
    // ffhip_model_pack_gap() blocks; results are indexed by READ (0 .. nvirt - 1, the order of the set call).  hT / hTb hold the reads' lengths then.
    int res_copied = 0;                 // the result block's copy to the host is already enqueued (a packed batch: behind its decode, in ffhip_batch_run)
    int cap_reads = 0;                  // the per-read result arrays (lens, score, logZ) take this many reads (>= nread)
    bool packed = false;
    int nvirt = 0;
    std::vector<int> v_slot, v_off;     // slot and first block of every read
    int *d_vb0 = nullptr, *d_vb1 = nullptr, *d_vtb = nullptr;      // per read: first row in Tb-row / (Tb + 1)-row buffers, blocks
    unsigned *d_live = nullptr;         // [Tb][B16]: bit r = slot 16 rt + r holds a block of a read at step t (the layer kernels' reset mask)
    int *rag_seg[3] = { nullptr, nullptr, nullptr };       // stride-1 thin layers of a packed batch: read boundaries per row (k_conv_small `seg`)
    size_t rag_seg_cap[3] = { 0, 0, 0 };
    long long *d_goff = nullptr;        // destination of every read's signal (floats from sbuf[0].p + kSamplePad)
    int4 *d_prd = nullptr;             // per read records for the device-side table / mask builders: [conv table | live mask] x cap_reads
    Pinned h_vb0, h_vb1, h_vtb, h_prd, h_seg[3], h_goff;
    SampleBuf sbuf[3];                  // sbuf[0] = signal, sbuf[l] = output of conv l-1
    float *act[2] = { nullptr, nullptr };
    void *actS[2] = { nullptr, nullptr };      // the same two buffers in the split-operand layout (ffhip_rnn_split.hip), allocated on first use
    float *keep[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    float *xa = nullptr, *cstate = nullptr;
    float *fa[2] = { nullptr, nullptr };       // the fp32 activations of the run in progress: act[], or -- a packed batch's launch-per-step run -- the memory of actS[]
    float *xa_win = nullptr;            // the launch-per-step run's in-projection, kStepWindow steps of it (run_layers); allocated on first use
    void *split_win = nullptr;          // ... and its input in the split layout
    size_t dev_bytes = 0;               // what dalloc holds for the batch (ffhip_debug_batch_device_bytes: this and the result block)
    float *trans = nullptr, *post = nullptr, *fwd = nullptr;
    double *crf_logz = nullptr;         // fp64 partition function per read
    double *crf_e = nullptr;            // exp(score - block max), workspace of the linear-space partition function
    uint8_t *tb = nullptr;
    int *path = nullptr; float *qpath = nullptr;
    int32_t *trace = nullptr;
    unsigned split_epoch = 0;           // launch counter of the split layer kernel (its check-in words are never cleared)
    int counted = 0;                    // this batch is in the engine's in_flight count (between run and finish)
    const float **d_gsrc = nullptr; int *d_glen = nullptr;              // ffhip_batch_set_prepared: source rows of the gather
    unsigned *pflags = nullptr;         // persistent-kernel XCC ids (the abort word: pabort() below)
    // reads with a value beyond the split format's range (ffhip_split.hpp: the swish convolutions' outputs are clamped at +-4094 there, the
    // reference's are unbounded, layers.c:24-33): one word per read, set by the producers of that format, looked at by ffhip_batch_finish,
    // which runs such reads again on the f32 path (`side`) and puts their results in place
    double rehearsal_done_at = 0.0;     // FFHIP_DEBUG_HOST_REHEARSAL_MSPS: when the emulated GPU is done with this batch
    ffhip_batch *side = nullptr;        // 16 slots of this batch's capacity, created when the first read needs it
    bool is_side = false;
    int reruns = 0;                     // reads of the last run that took that way
    int persist_concurrent_ok = 0;      // two such batches fit on the chip at once
    float *scratch = nullptr;           // dense [Tb][H] for debug taps
    // The small results, brought to the host by ffhip_batch_finish in one copy: the result block (ffhip_results.hpp), and thin views of its head and core fields
    ResultBlock res;
    unsigned *sat() const { return res.on_dev<unsigned>(RF_SAT); }
    unsigned *pabort() const { return res.on_dev<unsigned>(RF_ABORT); }
    int *lens() const { return res.on_dev<int>(RF_LENS); }
    float *score() const { return res.on_dev<float>(RF_SCORE); }
    char *bases() const { return res.on_dev<char>(RF_BASES); }
    char *quals() const { return res.on_dev<char>(RF_QUALS); }
    unsigned *h_sat() const { return res.on_host<unsigned>(RF_SAT); }
    unsigned *h_abort() const { return res.on_host<unsigned>(RF_ABORT); }
    int *h_lens() const { return res.on_host<int>(RF_LENS); }
    unsigned res_made = 0;              // sections of the block the last run filled (res_bit)
    // The per-read products OUTSIDE the result block (ffhip_annot.hpp): each a struct of its own that starts with its records (`rec`: a device buffer and its pinned
    // mirror, created or grown by the front of the first run that asks, one copy of their own beside the block's), its uploaded list if it has one, and `valid`
    // (the last run made them).  annot(i) is feature i of kAnnots.
    // Barcode records (FFHIP_RUN_BARCODES, k_barcodes): 16 bytes a read, cap_reads of them
    struct Barcodes : Annot { const ffhip_barcodes *kit = nullptr; int max_dist = 0, min_sep = 3, both = 0; } bc;
    // Adapter records (FFHIP_RUN_ADAPTERS, k_adapters): 256 bytes a read, cap_reads of them
    struct Adapters : Annot { const ffhip_adapters *kit = nullptr; int max_dist = -1; } ad;
    // Map records (FFHIP_RUN_MAP, k_map_scan and k_map_finish): 64 bytes a read, cap_reads of them; the tasks' slots (8 bytes a task of either anchor of every read),
    // taken by the front of the first run that asks
    struct Map : Annot { const ffhip_map_ref *ref = nullptr; int window = kMapMaxAnchor, max_error = 250; void *ws = nullptr; size_t ws_cap = 0; } map;
    // Poly tail records (FFHIP_RUN_POLYTAIL, k_polytail): 32 bytes a read, cap_reads of them; the reads' list, written by the front of every run that asks; the
    // windows' workspace (a double and a byte a window of every read, `windows` of them in this run), grown when a run needs more
    struct PolyTail : Annot { ffhip_polytail_params p{}; bool set = false; uint8_t *ws = nullptr; size_t ws_cap = 0, windows = 0; } pt;
    // Remap (FFHIP_RUN_REMAP, k_remap): the coded sequences of ffhip_batch_set_remap on the host and (dseq) on the device; cap_reads 16-byte records and, behind them,
    // a byte a block in the layout of the (Tb + 1)-entry buffers; the reads' list and the traceback workspace, both written by the front of every run that asks.
    // from_map (ffhip_batch_set_remap_from_map): no sequences on the host -- k_map_remap_seq codes each mapped read's stretch into dseq and patches the list, and
    // everything is sized from the read's blocks N: N + 1 positions
    struct Remap : Annot {
        std::vector<std::vector<unsigned short>> seq;       // per read: stay | move << 8 of every position (remap_code)
        std::vector<signed char> state;                      // per read: 0 no sequence, 1 a sequence, 2 refused at the call (L = 0)
        int set = 0, band = 0, from_map = 0;
        unsigned short *dseq = nullptr; size_t dseq_cap = 0;
        unsigned long long *ws = nullptr; size_t ws_cap = 0;
        int count[kRemapForms] = { 0, 0, 0, 0 };
    } rmp;
    // Truth (FFHIP_RUN_TRUTH, k_truth): the truths of ffhip_batch_set_truth on the host and (dseq) on the device; cap_reads 48-byte records and, behind them,
    // m + blocks + 1 bytes of ops a read with a truth; the reads' list and the traceback workspace as for remap.  from_map (ffhip_batch_set_truth_from_map): no
    // truths on the host -- k_map_stretch writes each mapped read's into dseq and patches the list, and everything is sized from the bound (map_truth_bound)
    struct Truth : Annot {
        std::vector<std::vector<uint8_t>> seq;               // per read: codes 0 .. nbase - 1
        std::vector<signed char> state;                      // per read: 0 no truth, 1 a truth, 2 an empty one
        std::vector<size_t> off;                             // per read: its first byte of ops behind the records, and (one more entry) the end
        int set = 0, band = 0, from_map = 0;
        uint8_t *dseq = nullptr; size_t dseq_cap = 0;
        unsigned long long *ws = nullptr; size_t ws_cap = 0;
        int count[kTruthForms] = { 0, 0, 0, 0 };
    } tru;
    // Events (FFHIP_RUN_EVENTS with FFHIP_RUN_REMAP, k_events): 16 bytes a base of every read with a sequence that can be mapped, one read behind the other
    // Site mods (FFHIP_RUN_REMAP_MODS with FFHIP_RUN_REMAP, k_site_mods): 16 bytes a C / Z of every such read; the workspace of starts (L + 1 int32 a listed read);
    // the lists are the reads, then the sites
    // Variants (FFHIP_RUN_REMAP_VARIANTS with FFHIP_RUN_REMAP, k_variants): 16 bytes a variant of every such read; a workspace of starts of its own; the lists are
    // the variants, then the reads; `set`: the lists of ffhip_batch_set_remap_variants (copied; empty: the feature is detached)
    struct PerBase : Annot {                                 // records of 16 bytes, a read's one behind the other
        std::vector<size_t> off;                             // per read: its first record, and (one more entry) the end
        int reads = 0;                                       // the reads in the list
        size_t total() const { return off.empty() ? 0 : off.back(); }
    } evt;
    struct Sites : PerBase { int *start = nullptr; size_t start_cap = 0; int context, all = 0; explicit Sites(int c) : context(c) {} } smd{ 15 };
    struct Variants : Sites { std::vector<std::vector<ffhip_variant>> set; Variants() : Sites(10) {} } var;
    // Pileup (FFHIP_RUN_PILEUP, k_pileup): the engine-level object the batch's finished runs add to; nothing of it is the batch's
    ffhip_pileup *pile = nullptr;
    ffhip_modpileup *modpile = nullptr;                      // (FFHIP_RUN_MOD_PILEUP, k_modpileup: likewise)
    ffhip_consensus *cons = nullptr;                         // (FFHIP_RUN_CONSENSUS, k_consensus: likewise)
    ffhip_errprofile *errp = nullptr;                        // (FFHIP_RUN_ERRPROFILE, k_errprofile: likewise; it belongs to no reference)
    enum { AN_COUNT = 9 };
    Annot &annot(int i) { Annot *const a[AN_COUNT] = { &bc, &ad, &map, &pt, &tru, &rmp, &evt, &smd, &var }; return *a[i]; }       // (the order of kAnnots: launch order)
    RleRunScale run_scale{ { 1.02, 1.04, 1.04, 1.02 } };      // decode_runnie.py's default --scale
    std::vector<void *> owned;
    unsigned last_flags = 0;
    float last_temperature = 1.0f;
    int ran = 0, finished = 0;
    int final_act = 0;                  // which act[] holds the last recurrent layer's output
    RunPath run_path;                   // the run's path, decided at its front (plan_run)
    int rnn_path = 0;                   // what the last run used: 0 launch per step, 1 persistent recurrence behind a projection GEMM, 2 fused f32 layer kernel, 3 split-operand layer kernel, 4 split-operand projection GEMM + recurrence-only layer kernel
    hipEvent_t ev[FFHIP_NGROUP + 1];
    int have_ev = 0;
    int launches[FFHIP_NGROUP];
    hipEvent_t lev[5][3];
    hipEvent_t pair_ev = nullptr;       // ffhip_batch_run_pair: orders the two streams around the paired layer launches
    int run_cur = 0;                    // which of act[] / actS[] holds the current activations between the phases of a run
    unsigned run_flags = 0;
    int paired_last = 0;                // the last run's layers were one launch with another batch's
    ffhip_batch *prof_mate = nullptr;   // second batch of a profiled pair: the batch whose lev[][] events bracket the paired launches (two event records
                                        // per launch instead of six: each is a packet between two layer launches, ~5 us of idle chip)
    ffhip_batch *prof_ref = nullptr;    // ... and the first batch's way back, so that either can go first
    int profiled = 0;
    // debug read-outs (ffhip_debug_batch_keep_front / _front / _head_input / _forms): none of them changes what a run launches
    bool keep_front = false;            // the next runs copy the last convolution's output to front_keep
    void *front_keep = nullptr;         // [Tb][B16] tiles in the split layout (front_exp: values * 2^front_exp) or fp32 tile-interleaved (front_exp < -1000)
    int front_kept = 0, front_exp = -100000, front_f16 = -1;       // the last run kept it; the thin layer whose output was fp16 slices (-1: none)
    int forms[4] = { -1, -1, -1, -1 };  // kernel forms of the last run's convolution launches and its head launch (KernelForm)
};

static inline int batch_nreads(const ffhip_batch *b) { return b->packed ? b->nvirt : b->nread; }
// behind the cap_reads records of remap's and truth's buffers: where the moves and the ops start
static inline size_t remap_moves_at(const ffhip_batch *b) { return (size_t)b->cap_reads * 16; }
static inline size_t truth_ops_at(const ffhip_batch *b) { return (size_t)b->cap_reads * kTruthRecInts * 4; }
static inline size_t read_row1(const ffhip_batch *b, int read) { return b->packed ? (size_t)b->v_slot[read] * (b->Tb + 1) + b->v_off[read] : (size_t)read * (b->Tb + 1); }      // a read's first row in the buffers of Tb + 1 rows a slot
static inline int total_stride(const ffhip_model *m) { int st = 1; for (int l = 0; l < m->nconv; l++) st *= m->conv[l].stride; return st; }
FFHIP_LOCAL bool results_ok(const ffhip_batch *b, int read);      // what every accessor of a finished batch asks first (ffhip_engine.hip): false with the error text set
