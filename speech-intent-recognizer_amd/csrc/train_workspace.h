// The training step's workspace, declared ONCE: the slot table below generates the slot enum (whose values are the published indices of
// sir_model_train_workspace_offsets, include/sir_hip.h), the byte layout, the typed pointers and carve().  With it the pieces both
// directions of the step need: the shape (TDims), the GRU weight-gradient split plan, argument checks.  Host code, except for the
// three constants at the top that kernels of both directions share with the layout.
#pragma once
#include "model_kernels.h"       // C1_PROWS / C1_PCOLS (model_shape.h, sir_internal.h)
#include "gemm_tn_common.h"      // TN_* tile sizes
#include "gru_frag_prep.h"       // GRU_FRAG_BYTES
#include "workspace_slots.h"     // the slot generators; WS_DIR* / WCB_* sub-buffer sizes, prep_blocks

constexpr int C1_NMOM = 54;      // conv1 input moments (layout: train_fwd_kernels.h), forward -> backward through TB_C1M
__host__ __device__ constexpr int c1_r_index(int t, int u) { return 9 + t * 9 - t * (t - 1) / 2 + (u - t); }   // t <= u
constexpr int WGR_PARTS = 16;    // partial sums of the two-pass nine-tap weight-gradient reduce (train_bwd_kernels.h), behind the slabs in TB_SLAB

// K splits of the four-job weight-gradient launch of one GRU layer (gemm_tn2_f16x3_kernel<true>) and its slab floats
static inline void tn_dw_plan(int tokens, int in_sz, int* tiles, int* kchunk, int* nsplit, size_t* slab_floats) {
    const int t = 2 * ((768 / TN2_BM) * ((in_sz + TN_BN - 1) / TN_BN) + (768 / TN2_BM) * 1);
    int ks = 256 / t;
    ks = ks < 1 ? 1 : (ks > 16 ? 16 : ks);
    const int kc = (((tokens + ks - 1) / ks) + TN_BK - 1) / TN_BK * TN_BK;
    const int ns = (tokens + kc - 1) / kc;
    *tiles = t; *kchunk = kc; *nsplit = ns;
    *slab_floats = (size_t)ns * 2 * 768 * ((size_t)in_sz + 256);
}

// the layer-input gradient dX = dG [W; W_reverse] of a layer whose 128-row tiles would leave CUs idle (layer 1: 6400 x 512 = 100
// tiles) runs as TWO K halves on 128-row tiles (wave tile 64 x 64) plus an ordered add, instead of 64-row tiles (wave tile 64 x 32)
static inline bool dx_splitk(int tokens, int in_sz) {
    const int nt = ((tokens + TN2_BM - 1) / TN2_BM) * ((in_sz + TN_BN - 1) / TN_BN);
    return nt < 160 && 2 * nt >= 96;
}

struct TDims : SirDims {
    SirConvPlan conv;
    int c1gx, c1gy;          // conv1 grids (ceil over un-pooled odd columns)
    int c2gx, c3gx, c3fx;      // c3fx: conv3 FORWARD grid (16x8-pixel tiles); c3gx: conv3 data-gradient grid (16x16)
    int c2wx;                  // conv2 FORWARD grid: Winograd blocks of two tile columns (4 pixels)
    int wg2_blocks, wg3_blocks;  // workgroups (= slabs) of the nine-tap weight-gradient fallback: one image each
    int ksplits, kchunk;
};

static inline bool make_tdims(int batch, int t, TDims* d) {
    if (!sir_make_dims(batch, t, d)) return false;
    d->conv = sir_conv_plan(d, false);
    d->c1gx = ((t + 1) / 2 + C1_PCOLS - 1) / C1_PCOLS;
    d->c1gy = (32 + C1_PROWS - 1) / C1_PROWS;
    d->c2gx = (d->wp1 + 7) / 8;
    d->c2wx = ((d->wp1 + 1) / 2 + 1) / 2;
    d->c3gx = (d->wp2 + 15) / 16;
    d->c3fx = (d->wp2 + 7) / 8;
    d->wg2_blocks = d->wg3_blocks = batch;
    const int K = batch * d->S;
    d->ksplits = K >= 2048 ? 8 : (K >= 256 ? 2 : 1);
    d->kchunk = ((K + d->ksplits - 1) / d->ksplits + 31) / 32 * 32;
    return true;
}

// per-(task, tile column) statistics of the producer / consumer Winograd kernel (or per-workgroup ones of the fallback kernels), the
// conv1 partials and the BatchNorm backward partials share TB_STATS: float2 elements
static inline size_t tws_stats_elems(const TDims& d) {
    const size_t B = d.B;
    size_t st = (size_t)d.c1gx * d.c1gy * B * 32;                       // conv1 partials (float2)
    size_t s2 = (size_t)d.c2wx * B * 64, s3 = (size_t)d.c3fx * B * 128;
    if ((size_t)4 * 1024 * 64 > s2) s2 = (size_t)4 * 1024 * 64;         // (4 blocks per workgroup, at most 1024 workgroups = CUs)
    if ((size_t)4 * 1024 * 128 > s3) s3 = (size_t)4 * 1024 * 128;
    if (s2 > st) st = s2;
    if (s3 > st) st = s3;
    const size_t bw = (size_t)(B * 16 * d.wp1 / 64 + 64) * 128;          // bn backward partials, generous
    if (bw > st) st = bw;
    return st;
}

// floats of TB_SLAB (side = false: every split-K / weight-gradient slab of the backward + the partial sums of the two-pass wgrad
// reduce) or of TB_SLAB2 (side = true: the GRU weight-gradient slabs alone)
static inline size_t tws_slab_floats(const TDims& d, bool side) {
    const size_t B = d.B, S = d.S;
    size_t gru = 0, dx = 0;
    for (int in_sz : {1024, 512}) {                       // slabs of the four-job GRU weight-gradient launch (size independent of the batch)
        int t_, kc_, ns_;
        size_t need;
        tn_dw_plan(d.B * d.S, in_sz, &t_, &kc_, &ns_, &need);
        if (need > gru) gru = need;
        if (dx_splitk((int)(d.B * d.S), in_sz) && (size_t)2 * B * S * in_sz > dx) dx = (size_t)2 * B * S * in_sz;
    }
    if (side) return gru > 64 ? gru : 64;
    size_t slab = (size_t)d.wg3_blocks * 9 * 128 * 64;
    const size_t s_w2 = (size_t)d.wg2_blocks * 9 * 64 * 32, s_g = (size_t)d.ksplits * 768 * 1024;
    if (s_w2 > slab) slab = s_w2;
    if (s_g > slab) slab = s_g;
    if (gru > slab) slab = gru;
    if (dx > slab) slab = dx;
    if ((size_t)64 * 16 * 128 * 64 > slab) slab = (size_t)64 * 16 * 128 * 64;      // Winograd weight-gradient slabs: 64 strips of conv3, 128 of conv2
    return slab + (size_t)WGR_PARTS * 16 * 128 * 64;
}

// ---- the slot table: X(slot, pointer member, element type, element count) ----------------------------------------------------------
// One line per slot, in layout order; the enum value TB_<slot> is the slot's published index.  Counts are expressions of
// `d` (TDims) with B = d.B and S = d.S as size_t.  Every slot starts on a 256-byte boundary.
#define SIR_TRAIN_SLOTS(X)                                                                                                             \
    X(A1, a1, float, B * 32 * d.wp1 * 32)        /* conv1 block output (pooled), NHWC */                                               \
    X(Z2, z2, float, B * 32 * d.wp1 * 64)        /* conv2 raw output */                                                                \
    X(A2, a2, float, B * 16 * d.wp2 * 64)        /* conv2 block output */                                                              \
    X(Z3, z3, float, B * 16 * d.wp2 * 128)       /* conv3 raw output */                                                                \
    X(X0, x0, float, B * S * 1024)               /* conv3 block output in the GRU layout = layer 0 input */                            \
    X(GI, gi, float, B * S * 1536)               /* input projection of the layer that is running */                                   \
    X(G0, g0, float, B * S * 2048)               /* saved gates of layer 0 */                                                          \
    X(G1, g1, float, B * S * 2048)               /* saved gates of layer 1 */                                                          \
    X(Y0, y0, float, B * S * 512)                /* layer 0 output */                                                                  \
    X(Y0D, y0d, float, B * S * 512)              /* layer 0 output behind the dropout */                                               \
    X(Y1, y1, float, B * S * 512)                /* layer 1 output */                                                                  \
    X(CTX, ctx, float, B * 512)                  /* attention-pooled context */                                                        \
    X(BN, bn, float, 4 * 224)                    /* [4][224]: scale, shift, mean, invstd (bn1|bn2|bn3 channel ranges 0,32,96) */       \
    X(BNB, bnb, float, 2 * 224)                  /* [2][224]: mean dy, mean dy*xhat (backward) */                                      \
    X(STATS, stats, float2, tws_stats_elems(d))  /* partials of the BN forward / backward reductions */                                \
    X(WP2, reserved0, float, 64)                 /* reserved (a slot of a removed kernel generation: keeps the indices and offsets behind it) */ \
    X(WP3, reserved1, float, 64)                 /* reserved (a slot of a removed kernel generation: keeps the indices and offsets behind it) */ \
    X(WHT, wht, float, 4 * GRU_FRAG_BYTES / sizeof(float))   /* W_hh of 2 layers x 2 directions as resident fragments, forward */      \
    X(WR4, wr4, float, 4 * GRU_FRAG_BYTES / sizeof(float))   /* the same for the backward recurrence */                                \
    X(WP2T, reserved2, float, 64)                /* reserved (a slot of a removed kernel generation: keeps the indices and offsets behind it) */ \
    X(WP3T, reserved3, float, 64)                /* reserved (a slot of a removed kernel generation: keeps the indices and offsets behind it) */ \
    X(DY1, dy1, float, B * S * 512)              /* gradient of layer 1 output */                                                      \
    X(DY0, dy0, float, B * S * 512)              /* gradient of layer 0 output */                                                      \
    X(DGI, dgi, float, B * S * 1536)             /* gate gradients of layer 0, input side */                                           \
    X(DGH, dgh, float, B * S * 1536)             /* gate gradients of layer 0, hidden side */                                          \
    X(DX0, dx0, float, B * S * 1024)             /* gradient of x0 */                                                                  \
    X(DZ3, dz3, float, B * 16 * d.wp2 * 128)     /* gradient of z3 */                                                                  \
    X(DA2, da2, float, B * 16 * d.wp2 * 64)      /* gradient of a2 */                                                                  \
    X(DZ2, dz2, float, B * 32 * d.wp1 * 64)      /* gradient of z2 */                                                                  \
    X(DA1, da1, float, B * 32 * d.wp1 * 32)      /* gradient of a1 */                                                                  \
    X(SMALL, small, float, B * 512 + B + 64 + (size_t)d.c1gx * d.c1gy * B * 352)   /* daw_part [B][512], dab_part [B], conv1 backward partials (32 x 11 per block) */ \
    X(SLAB, slab, float, tws_slab_floats(d, false))          /* split-K / wgrad partial slabs */                                       \
    X(XS, xs, unsigned short, B * S * 1024 * 2)  /* f16x2 planes (f16_split.h) of the forward GEMM A operand [2][B*S][1024] */         \
    X(WS, ws, unsigned short, 2 * WS_DIR0 + 2 * WS_DIR1)     /* f16x2 planes of W_ih: wsl0 [2 directions] WS_DIR0, wsl1 [2] WS_DIR1 */ \
    X(WCB, wcb, unsigned short, 3 * (WCB_W2 + WCB_W3 + WCB_W2 + WCB_W3 + WCB_W3_TAPS))   /* conv weights, 3 planes each: wcb2, wcb3 (forward), wcb2t, wcb3t (data gradient), wcb3d */ \
    X(C1M, c1m, double, C1_NMOM)                 /* conv1 input moments (conv1_moments_kernel), forward -> backward */                 \
    X(DGI1, dgi1, float, B * S * 1536)           /* gate gradients of layer 1 (TB_DGI / TB_DGH hold layer 0's): layer 1's */          \
    X(DGH1, dgh1, float, B * S * 1536)           /*   weight-gradient GEMM may run after layer 0's BPTT */                             \
    X(SLAB2, slab2, float, tws_slab_floats(d, true))         /* GRU weight-gradient slabs when that GEMM runs on the side stream */ \
    X(BSC, bsc, float, 2 + 2 * B)                /* the backward's loss scale, pairs {scale, 1 / scale}: pair 0 the call's, pair 1 + b utterance b's */ \
    X(RAG, rag, int, 4 * B)                      /* ragged step: [4][B] validated frames, W1, W2, S_b of every clip (ragged_widths_kernel) */

#define SIR_TRAIN_SLOT_ENUM(id, member, type, count) TB_##id,
enum TrainBuf { SIR_TRAIN_SLOTS(SIR_TRAIN_SLOT_ENUM) TB_COUNT };

// byte offset of every slot; returns the workspace size
static inline size_t tws_layout(const TDims& d, size_t* off) {
    const size_t B = d.B, S = d.S;
    size_t pos = 0;
    SIR_TRAIN_SLOTS(SIR_SLOT_OFFSET)
    return pos;
}

struct TPtrs {
    SIR_TRAIN_SLOTS(SIR_SLOT_MEMBER)
    unsigned short *wsl0, *wsl1;                        // sub-buffers of ws
    unsigned short *wcb2, *wcb3, *wcb2t, *wcb3t, *wcb3d;   // sub-buffers of wcb (wcb3d: only for shapes the Winograd kernel does not cover)
};

static inline TPtrs carve(void* ws, const size_t* off) {
    char* b = (char*)ws;
    TPtrs p;
    SIR_TRAIN_SLOTS(SIR_SLOT_CARVE)
    p.wsl0 = p.ws; p.wsl1 = p.wsl0 + 2 * WS_DIR0;
    p.wcb2 = p.wcb; p.wcb3 = p.wcb2 + 3 * WCB_W2;
    p.wcb2t = p.wcb3 + 3 * WCB_W3; p.wcb3t = p.wcb2t + 3 * WCB_W2;
    p.wcb3d = p.wcb3t + 3 * WCB_W3;
    return p;
}

// Ragged step (sir_model_train_fwd_ragged / sir_model_train_bwd_ragged): the widths of clip b from the GIVEN frames[b], as the tables of
// the ragged inference call take them (infer_tables.h) -- fw = frames[b], or 0 where it lies outside [8, T]; W1 = fw / 2, W2 = fw / 4,
// S_b = fw / 8 -- into TB_RAG as [4][B].  A clip of width 0 has no column, no step and NaN logits; it raises bit 6 of the status word
// (status == NULL, the backward: the forward has raised it already).  Nothing else reads `frames`: whatever it holds, every width the
// kernels see lies inside the buffers.
struct RagPtrs { const int *fw, *w1, *w2, *sb; };
static inline RagPtrs rag_ptrs(const int* rag, int B) { return RagPtrs{rag, rag + B, rag + 2 * (size_t)B, rag + 3 * (size_t)B}; }
static __global__ __launch_bounds__(256) void ragged_widths_kernel(const int* __restrict__ frames, int B, int T, int* __restrict__ rag,
                                                                    unsigned int* __restrict__ status) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int f = frames[b];
    const bool ok = f >= 8 && f <= T;
    const int fw = ok ? f : 0;
    rag[b] = fw; rag[B + b] = fw >> 1; rag[2 * (size_t)B + b] = fw >> 2; rag[3 * (size_t)B + b] = fw >> 3;
    if (!ok && status) __hip_atomic_fetch_or(status, SIR_STATUS_RAGGED_LENGTH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static const sir_train_config kTrainAllLive = {{0, 0, 0}};      // what a NULL sir_train_config means: nothing frozen

static inline int check_common(const char* who, sir_handle* h, const sir_model_weights* w, int batch, int t, void* ws, size_t bytes,
                               TDims* d, size_t* off) {
    if (!h || !w || !ws) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    if (!make_tdims(batch, t, d)) { sir_set_error("%s: unsupported shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", who, batch, t); return SIR_EINVAL; }
    if (h->cfg.n_mels != 64) { sir_set_error("%s: the model is wired for 64 mels", who); return SIR_EUNSUPPORTED; }
    if (w->num_classes < 1 || w->num_classes > 64) { sir_set_error("%s: num_classes=%d", who, w->num_classes); return SIR_EINVAL; }
    const size_t need = tws_layout(*d, off);
    if (bytes < need) { sir_set_error("%s: workspace %zu < %zu", who, bytes, need); return SIR_ENOMEM; }
    if (((uintptr_t)ws & 255) != 0) { sir_set_error("%s: workspace must be 256-byte aligned", who); return SIR_EINVAL; }
    return SIR_OK;
}

// The ragged step (`frames` given) takes every BatchNorm on its running statistics: refused otherwise, before anything is launched
// or written.  `what`: "result" (forward) or "gradient" (backward).
static inline int check_ragged_frozen(const char* who, const sir_train_config* cfg, const char* what) {
    if (cfg && cfg->bn_frozen[0] && cfg->bn_frozen[1] && cfg->bn_frozen[2]) return SIR_OK;
    sir_set_error("%s: lengths (frames per clip) need every BatchNorm on its frozen running statistics "
                  "(bn_frozen = {1, 1, 1}): with batch statistics a clip has no %s of its own", who, what);
    return SIR_EUNSUPPORTED;
}

// Loss scale of the backward (a power of two, exact in fp32 both ways): head_bwd_kernel multiplies d(loss)/d(GRU output) by it and
// every kernel that writes a PARAMETER gradient behind it multiplies by its inverse, so that the intermediate gradients -- 1e-5 to
// 1e-7 at batch 256 unscaled -- sit around 2^-4 .. 2^4: inside fp16's normal range for the f16x3 contractions of the backward
// (f16_split.h).  The STATIC scale, 2^8 x batch (rounded up to a power of two), makes the scaled d(logits) (softmax - onehot) x 2^8
// whatever the batch.  That holds for a mean cross-entropy far from convergence only: below 2^-14 the split keeps an absolute
// 2^-36, so a batch whose softmax - onehot is 2^-24 would lose all but 8 bits.  bwd_scale_kernel (train_bwd_kernels.h) therefore
// reads max |dlogits| at the head of every backward and writes the scale the kernels use into TB_BSC: the static one while the scaled
// maximum stays within [2^5, 2^10), else the power of two that brings it back to [2^7, 2^8) -- any finite dlogits, 2^-24 or 2^16
// times the usual, gives the same relative accuracy (tests/test_operand_range_gpu.py).  Results are bit-identical to the unscaled
// backward wherever the arithmetic is fp32 or bf16x6 (scaling by 2^k commutes with every rounding there).
// A gradient that enters at the embedding (sir_model_train_bwd_emb) takes part in that maximum as |demb| * 2^5: it is added to
// dctx = dlogits fc_w, which at the reference head's initialisation is about |dlogits| * 2^-4.5 (bwd_scale_kernel has the reason).
inline int sir_bwd_loss_scale_exp(int batch) {
    int k = 8;
    while ((1 << (k - 8)) < batch && k < 24) ++k;
    return k;
}
inline float sir_bwd_loss_scale(int batch) { return (float)(1u << sir_bwd_loss_scale_exp(batch)); }

inline int grid_for(size_t n, int per_block = 256, int cap = 8192) {
    size_t g = (n + per_block - 1) / per_block;
    return (int)(g > (size_t)cap ? cap : (g < 1 ? 1 : g));
}
