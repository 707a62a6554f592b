// Internal declarations shared by the HIP translation units of libsir_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "sir_hip.h"

void sir_set_error(const char* fmt, ...);

#define SIR_WAVE 64               // CDNA wavefront width (hard-coded, see cdna guide section 1)
#define SIR_NFFT 1024
#define SIR_HOP 512
#define SIR_NFREQ 513
#define SIR_MAX_MELS 64

// kernels (or kernel groups) of the path, for sir_profile_*
enum SirKernelId {
    SIR_K_FEAT_FRAMES = 0, SIR_K_FEAT_NORM, SIR_K_PREP, SIR_K_CONV1, SIR_K_CONV2, SIR_K_CONV3,
    SIR_K_GEMM_IH0, SIR_K_GRU0, SIR_K_GEMM_IH1, SIR_K_GRU1, SIR_K_ATTN, SIR_K_FC,
    // training step (model_train_fwd.hip, train_loss_optim.hip, model_train_bwd.hip): forward groups, loss, backward groups, optimizer
    SIR_K_T_PREP, SIR_K_T_CONV1, SIR_K_T_CONV2, SIR_K_T_BN2, SIR_K_T_CONV3, SIR_K_T_BN3, SIR_K_T_GEMM_IH0, SIR_K_T_GRU0,
    SIR_K_T_DROPOUT, SIR_K_T_GEMM_IH1, SIR_K_T_GRU1, SIR_K_T_HEAD, SIR_K_CE,
    SIR_K_B_HEAD, SIR_K_B_GRU1, SIR_K_B_DW1, SIR_K_B_DX1, SIR_K_B_GRU0, SIR_K_B_DW0, SIR_K_B_DX0,
    SIR_K_B_BN3, SIR_K_B_WGRAD3, SIR_K_B_DGRAD3, SIR_K_B_BN2, SIR_K_B_WGRAD2, SIR_K_B_DGRAD2, SIR_K_B_CONV1, SIR_K_ADAM,
    // training recipe (appended: the ids above keep their meaning): batch mixing, gradient norm / clip, clipped Adam
    SIR_K_MIX, SIR_K_GRAD_SUMSQ, SIR_K_GRAD_CLIP, SIR_K_ADAM_CLIPPED,
    // sir_adam_step_ex with decoupled weight decay and / or the EMA shadow on (appended), without / with clipping
    SIR_K_ADAM_EX, SIR_K_ADAM_EX_CLIPPED,
    // utterance segmentation of long recordings (vad.hip, appended): chunk energy, state machine (count + bases + table), clip gather
    SIR_K_VAD_ENERGY, SIR_K_VAD_SEGMENT, SIR_K_VAD_GATHER,
    SIR_K_COUNT,        // what sir_profile_kernel_count() returns: the ids of the paths every caller runs
    // Extended ids (SIR_PROFILE_EXTRA_IDS of them, include/sir_hip.h), appended BEHIND the count: kernels that run only when a caller
    // asks for something optional.  Callers that walk [0, count) -- the benchmark's roofline table, its per-kernel FLOP / byte
    // tables -- never see them; sir_profile_kernel_name and sir_profile_collect serve them to callers that ask for count + extra.
    // Gradient of the training step with respect to its input features (sir_model_train_bwd_x): conv1's data gradient
    SIR_K_B_CONV1_DGRAD = SIR_K_COUNT,
    SIR_K_COUNT_ALL
};
static_assert(SIR_K_COUNT_ALL - SIR_K_COUNT == SIR_PROFILE_EXTRA_IDS, "include/sir_hip.h: SIR_PROFILE_EXTRA_IDS");

// Bits of the handle's device status word (sir_handle::status).  A kernel raises one with a relaxed agent-scope fetch_or;
// api.hip check_status_impl reads and clears the word and turns the bits into an error.  include/sir_hip.h documents several
// by number: the values are part of the contract and never move.
enum SirStatusBit : unsigned int {
    SIR_STATUS_GRU_TIMEOUT   = 1u,      // a GRU recurrence's exchange spin timed out (gru_quad_kernel.h, gru_bwd_quad_kernel.h)
    SIR_STATUS_CE_LABEL      = 2u,      // cross-entropy label outside [0, C) that is not -100 (ce_loss_rows.h)
    SIR_STATUS_GATHER_INDEX  = 4u,      // sir_gather_features: index outside the store (frontend.hip)
    SIR_STATUS_CONV_WEIGHT   = 8u,      // transformed conv weight outside the f16x3 range (conv_wino2_f16x3_kernel.h)
    SIR_STATUS_PERTURB       = 16u,     // sir_wave_perturb: pitch / tempo outside its range (perturb.hip)
    SIR_STATUS_MIX_PERM      = 32u,     // sir_mix_features: permutation entry outside the batch (frontend.hip)
    SIR_STATUS_RAGGED_LENGTH = 64u,     // ragged forward: a length outside [8, t_frames] (infer_tables.h, train_workspace.h)
    SIR_STATUS_VAD_ROW       = 128u,    // sir_vad_gather: a table row outside the batch (clip_gather.h)
    SIR_STATUS_REVERB        = 256u,    // sir_wave_reverb_mix: bad index, bank length or snr_db (reverb.hip)
    SIR_STATUS_EVAL_LABEL    = 512u,    // sir_eval_accumulate* / sir_temperature_fit: label outside [0, C) that is not -100 (evaluate.hip)
    SIR_STATUS_STREAM_ROW    = 1024u,   // sir_stream_gather: an impossible table row (clip_gather.h)
    SIR_STATUS_GRU_WEIGHT    = 2048u,   // GRU weight not finite or outside +-65504 (f16_split.h)
    SIR_STATUS_ACT_RANGE     = 4096u,   // training activation beyond the backward's exact range (train_fwd_kernels.h)
    SIR_STATUS_BN_PARAM      = 8192u,   // conv1 weight / BatchNorm parameter not finite (model_kernels.h)
    SIR_STATUS_DECODE_TUPLE  = 16384u,  // sir_decode_slots: a tuple-table byte outside its slot's [0, C_g) (slots_decode.hip)
};

// Slot heads (include/sir_hip.h "slot heads"): one logit row as up to kMaxSlots softmax segments.  Passed to kernels by
// value; the loss (slots.hip) and the evaluation (evaluate.hip) extend it with their own per-slot arrays.
constexpr int kMaxSlots = 8;
struct SlotTable {
    int n;
    int start[kMaxSlots], size[kMaxSlots];           // first column and width of segment g
};

struct SirProfRec { int id; hipEvent_t e0, e1; };
static inline size_t sir_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// bytes per sample of a waveform argument, 0 for a wave_dtype that is neither SIR_WAVE_F32 nor SIR_WAVE_I16
static inline size_t sir_wave_elem_bytes(int wave_dtype) { return wave_dtype == SIR_WAVE_F32 ? 4 : wave_dtype == SIR_WAVE_I16 ? 2 : 0; }
// a wave_dtype that sir_wave_elem_bytes accepted, as a type: calls f once with a value of the element type (its type is the tag:
// `[&](auto tag) { using T = decltype(tag); return impl<T>((const T*)wave, ...); }`) and returns what f returns
template <typename F>
static inline int sir_wave_dispatch(int wave_dtype, F&& f) { return wave_dtype == SIR_WAVE_I16 ? f((short)0) : f(0.0f); }

// polyphase resampling filter of one (orig_freq, new_freq) pair (frontend.hip), device tables
struct sir_resample_table {
    int orig_freq, new_freq;    // as passed by the caller
    int orig, nw, width, L;     // gcd-reduced rates, torchaudio's `width`, taps kept per phase
    float* taps;                // [nw][L]
    int* first;                 // [nw] index (in torchaudio's kernel row) of the first kept tap
};

struct sir_handle {
    // event profiling state (host only)
    int prof_mode;      // 0 off, 1 every kernel, 2 only prof_only
    int prof_only;
    std::vector<SirProfRec> prof_pending;
    std::vector<hipEvent_t> prof_free;
    // prepared-weight cache key (sir_model_set_weights_version)
    unsigned long long weights_version;
    // one entry per workspace that holds prepared weights (several streams may alternate workspaces)
    struct PrepEntry { const void* ws; unsigned long long version; long long key; };
    PrepEntry prep[4];
    int prep_next;
    sir_feature_config cfg;
    int device;
    // feature tables (device)
    float2* tw512;      // exp(-2*pi*i*j/512),  j = 0..511
    float2* tw1024;     // exp(-2*pi*i*k/1024), k = 0..512
    float* window;      // [1024]
    float* melw;        // compact filter weights: filter after filter, taps ascending in frequency (mel_nnz floats)
    int4* mel_desc;     // [64] per slot, filters sorted by tap count: {filter (-1 = unused), first FFT bin, taps, offset into melw}
    int mel_nnz;
    // front-end geometry.  `general` = anything but n_fft 1024 / hop 512 / win_length 1024: sir_features_fwd then runs the general
    // launch pair (features_gen.hip: feat_gen_frames_kernel + feat_gen_norm_kernel) with the tables below, and `window` holds n_fft
    // floats, the win_length window centred between zeros.  The specialised kernels keep their SIR_NFFT / SIR_HOP constants.
    int win_length;
    bool general;
    float2* gen_twn;    // general path: exp(-2*pi*i*k/(n_fft/2)), k = 0 .. n_fft/2 - 1 (the packed transform's twiddles)
    float2* gen_tw2n;   // general path: exp(-2*pi*i*k/n_fft),     k = 0 .. n_fft/2 - 1 (the untangle twiddles)
    // the filterbank transposed for sir_features_bwd: per FFT bin the (at most) two filters that cover it, {filter, weight, filter,
    // weight} (int, float, int, float; weight 0 = none), [513]; mel_max_cover = filters on the busiest bin (the kernel serves <= 2)
    void* mel_taps;
    int mel_max_cover;
    std::vector<sir_resample_table> resample_tables;   // built on first use of a rate pair
    // device word set to 1 by a GRU recurrence kernel whose inter-workgroup exchange timed out (its results are then
    // invalid); zeroed at creation, read and cleared by sir_check_status / sir_profile_collect
    unsigned int* status;
    // Cluster kernels (the GRU recurrences) need every workgroup of a cluster resident at once; dispatch order
    // guarantees that within ONE launch, but two such launches on different streams interleave their dispatch and, once
    // their workgroups outnumber the CUs, can fill the chip with partial clusters that wait for each other for ever (seen
    // with 2 processes x 2 streams on one GPU: spin time-outs).  Launches of cluster kernels issued through this handle are
    // therefore chained: one on another stream first waits for the previous one's completion event (sir_cluster_enter).
    hipEvent_t cluster_done;
    hipStream_t cluster_stream;        // stream of the latest cluster launch (compared, never dereferenced)
    bool cluster_pending, cluster_seen, cluster_multi;
    int cluster_run;                   // chained mode: launches in a row that came from cluster_stream
    // kernels whose dynamic-LDS opt-in has been made (sir_lds_opt_in), per handle = per device (a process-wide static would
    // skip the second device of a process that drives several)
    std::vector<const void*> lds_opted;
    float* zero_page;                  // 4 KB of zeros: DMA source of the second-generation Winograd kernel's out-of-image pixels
    int num_cus;                       // persistent kernels launch one workgroup per CU
    // Exchange-granule buffers of the cluster kernels (GRU recurrences).  They are OWNED by the handle (hipMalloc), one per
    // (launch stream, kernel kind): nothing but that kernel ever writes them, so a granule found there is always one of its
    // own from an earlier launch and the launch epoch in its tag tells it apart.  (They used to be carved out of the caller's
    // workspace at a batch-dependent offset: a launch at another batch size, or any other tenant of that memory, could leave
    // arbitrary bits where the 16-bit tag of the forward kernel is polled.)  Launches on one stream are ordered, launches on
    // different streams get different buffers.  A buffer is zeroed when it is new or must cover more bytes than the
    // previous launch on it wrote -- not before every launch (4.8 us each, 4 per training step / 2 per inference batch,
    // serialised in front of a latency-bound kernel).
    struct XbufEntry { hipStream_t st; int kind; void* p; size_t cap, bytes; unsigned epoch; unsigned long long used; };
    XbufEntry xbufs[16];
    unsigned long long xbuf_clock;
    unsigned long long xbuf_evictions;   // LRU evictions so far (each costs a device-synchronising hipFree + hipMalloc on the launch path)
    // second stream of the training backward (model_train_bwd.hip): the off-chain weight-gradient launches; created on first use.
    // ev: 0 fork behind the GRU part, 1 / 2 dz3 / dz2 ready, 3 join, 4 / 5 GRU layer 0 / 1 BPTT done
    hipStream_t bwd_side;
    hipEvent_t bwd_ev[6];
};

// granule buffer + launch epoch for a cluster kernel launched on `st`; allocates / grows / zeroes the buffer when needed.
// `kind` separates kernels with different granule formats (gru_quad_kernel.h / gru_bwd_quad_kernel.h).
static inline int sir_xbuf_acquire(sir_handle* h, hipStream_t st, int kind, size_t bytes, unsigned mask, void** xbuf, unsigned* epoch) {
    sir_handle::XbufEntry* e = nullptr;
    for (auto& x : h->xbufs)
        if (x.p && x.st == st && x.kind == kind) e = &x;
    if (!e) {                                             // free slot, else the least recently used one
        e = &h->xbufs[0];
        for (auto& x : h->xbufs) {
            if (!x.p) { e = &x; break; }
            if (x.used < e->used) e = &x;
        }
        if (e->p) {                                       // hipFree waits for the device: no launch can still be using it
            ++h->xbuf_evictions;                          // (more than 16 live (stream, kind) pairs: every launch then frees + allocates)
            if (hipFree(e->p) != hipSuccess) { sir_set_error("exchange buffer: hipFree of an evicted buffer failed"); return SIR_EHIP; }
            e->p = nullptr;
        }
        e->st = st; e->kind = kind; e->cap = 0; e->bytes = 0; e->epoch = 0;
    }
    if (bytes > e->cap) {
        if (e->p && hipFree(e->p) != hipSuccess) { sir_set_error("exchange buffer: hipFree before growing failed"); return SIR_EHIP; }
        e->p = nullptr; e->cap = 0; e->bytes = 0;
        const size_t cap = sir_align_up(bytes, (size_t)1 << 20);
        if (hipMalloc(&e->p, cap) != hipSuccess) { e->p = nullptr; sir_set_error("exchange buffer: hipMalloc of %zu bytes failed", cap); return SIR_EHIP; }
        e->cap = cap;
    }
    // new buffer, or more clusters than the PREVIOUS launch on it wrote: the extra granules are older than one epoch (after a
    // run of 128 smaller batches they would carry the current epoch again) -- zero.  Otherwise every granule that will be
    // polled was written by the previous launch, whose epoch differs.
    if (bytes > e->bytes && hipMemsetAsync(e->p, 0, bytes, st) != hipSuccess) { sir_set_error("exchange buffer: hipMemsetAsync failed"); return SIR_EHIP; }
    e->bytes = bytes;
    e->epoch = (e->epoch + 1) & mask;
    e->used = ++h->xbuf_clock;
    *epoch = e->epoch;
    *xbuf = e->p;
    return SIR_OK;
}

// bracket of a cluster-kernel launch (see sir_handle::cluster_done).  The completion event costs the stream a ~6 us bubble
// per launch (the next kernel waits for the marker packet), so it is only recorded while launches really come from more
// than one stream: a handle starts in single-stream mode, the first launch from a second stream drains the device once
// and switches to chained mode, 64 launches in a row from one stream switch back.
static inline int sir_cluster_enter(sir_handle* h, hipStream_t st) {
    if (!h->cluster_multi) {
        if (h->cluster_seen && h->cluster_stream != st) {
            if (hipDeviceSynchronize() != hipSuccess) return SIR_EHIP;
            h->cluster_multi = true;
            h->cluster_pending = false;
            h->cluster_run = 0;
        }
        return SIR_OK;
    }
    if (h->cluster_pending && h->cluster_stream != st)
        if (hipStreamWaitEvent(st, h->cluster_done, 0) != hipSuccess) return SIR_EHIP;
    return SIR_OK;
}
static inline int sir_cluster_leave(sir_handle* h, hipStream_t st) {
    if (h->cluster_multi) {
        if (hipEventRecord(h->cluster_done, st) != hipSuccess) return SIR_EHIP;
        h->cluster_pending = true;
        h->cluster_run = (h->cluster_stream == st) ? h->cluster_run + 1 : 0;
        if (h->cluster_run >= 64) { h->cluster_multi = false; h->cluster_pending = false; }
    }
    h->cluster_stream = st;
    h->cluster_seen = true;
    return SIR_OK;
}

int sir_check_hip(hipError_t e, const char* what);

#define SIR_HIP_TRY(expr)                                   \
    do {                                                    \
        int _rc = sir_check_hip((expr), #expr);             \
        if (_rc != SIR_OK) return _rc;                      \
    } while (0)
#define SIR_KCHECK() SIR_HIP_TRY(hipGetLastError())
#define SIR_TRY(expr)                                       \
    do {                                                    \
        int _rc = (expr);                                   \
        if (_rc != SIR_OK) return _rc;                      \
    } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for `kernel`, once per handle; called at the kernel's launch site.  A linear
// search is enough: the host path launches <= ~20 kernels that need the opt-in.
static inline int sir_lds_opt_in(sir_handle* h, const void* kernel, int bytes) {
    for (const void* k : h->lds_opted)
        if (k == kernel) return SIR_OK;
    SIR_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    h->lds_opted.push_back(kernel);
    return SIR_OK;
}

// RAII: records a HIP event pair on `st` around the launches issued while it is alive
struct SirProfScope {
    sir_handle* h; int id; hipStream_t st; hipEvent_t e0, e1; bool on;
    SirProfScope(sir_handle* h_, int id_, hipStream_t st_) : h(h_), id(id_), st(st_), e0(nullptr), e1(nullptr) {
        on = h->prof_mode == 1 || (h->prof_mode == 2 && h->prof_only == id);
        if (!on) return;
        hipEvent_t ev[2];
        for (int i = 0; i < 2; ++i) {
            if (!h->prof_free.empty()) { ev[i] = h->prof_free.back(); h->prof_free.pop_back(); }
            else if (hipEventCreate(&ev[i]) != hipSuccess) { on = false; return; }
        }
        e0 = ev[0]; e1 = ev[1];
        (void)hipEventRecord(e0, st);
    }
    ~SirProfScope() {
        if (!on) return;
        (void)hipEventRecord(e1, st);
        h->prof_pending.push_back(SirProfRec{id, e0, e1});
    }
};

// frontend.hip: the handle's table for a rate pair (orig_freq != new_freq), built, uploaded and cached on first use
// (host-synchronous, two small hipMallocs owned by the handle); later calls only look it up.  false: the build failed.
bool sir_get_resample_table(sir_handle* h, int orig_freq, int new_freq, sir_resample_table* out);

// slots.hip: the slot-layout rules of include/sir_hip.h; fills start[8] / size[8], or sets `who`'s error and returns false
bool sir_slots_check_layout(const char* who, const int32_t* slot_sizes, int n_slots, int num_classes, int* start, int* size);

// model_train_fwd.hip
size_t sir_train_workspace_bytes_impl(int batch, int t_frames);

// features_gen.hip (feat_lds.h: FeatGenLds)
size_t sir_features_gen_lds_bytes(int n_fft, int mel_nnz);   // dynamic LDS the general frames kernel needs on such a handle
#define SIR_LDS_BYTES (160 * 1024)                            // per workgroup on gfx950
// (the general launch pair behind sir_features_launch, and its dB slab: the workspace)
size_t sir_features_gen_slab_bytes(const sir_handle* h, int batch, int max_len);
int sir_features_gen_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
                            int max_len, float* out, int t_pad, float* db_out, void* workspace, const sir_augment* aug,
                            hipStream_t stream);
// features_fwd.hip, features_bwd.hip
int sir_features_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride,
                        const int32_t* lengths, int batch, int max_len, float* out, int t_pad,
                        float* db_out, void* workspace, size_t workspace_bytes, const sir_augment* aug,
                        hipStream_t stream);
int sir_features_bwd_launch(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths,
                            int batch, int max_len, const float* db, const float* dout, int t_pad, const sir_augment* aug,
                            float* dwave, int64_t dwave_stride, hipStream_t stream);

// GRU recurrences (gru_quad.hip: forward and BPTT, clusters of four workgroups on the matrix cores).  Both write h->status if an
// exchange spin times out.  nlive (forward, optional): per-utterance step count past which gi rows come from utterance B, or -- `ragged` --
// past which the utterance's h is held and nothing of it is read or written (gru_quad_kernel.h)
int sir_launch_gru_quad(sir_handle* h, hipStream_t st, bool save, const float* gi, const float* whh0, const float* whh1, const float* bhh0,
                        const float* bhh1, float* y, int B, int S, float* gates,
                        unsigned short* yplanes = nullptr, const void* wfrag0 = nullptr, const void* wfrag1 = nullptr,
                        const int* nlive = nullptr, bool ragged = false);
void sir_prep_whh_quad(sir_handle* h, hipStream_t st, const float* whh, void* frag);     // -> GRU_FRAG_BYTES (gru_frag_prep.h)
int sir_launch_gru_bwd_quad(sir_handle* h, hipStream_t st, const float* dy, const float* gates, const float* y, const float* whh0,
                            const float* whh1, float* dgi, float* dgh, float* bsum_i, float* bsum_h, int B, int S,
                            const void* wfrag0 = nullptr, const void* wfrag1 = nullptr, const int* nlive = nullptr);
