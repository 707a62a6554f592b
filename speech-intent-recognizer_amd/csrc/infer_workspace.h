// The inference workspace, declared ONCE: the slot table below generates the slot enum (whose values are the published indices of
// sir_model_workspace_offsets, include/sir_hip.h), the byte layout, the typed pointers and carve(); the table list below it does the
// same for the int sub-tables inside the WS_PAD slot (published by sir_model_infer_table_offsets).  With them the shape (Dims).
// Host code; the table kernels (infer_tables.h) take Dims by value.
#pragma once
#include "model_shape.h"
#include "workspace_slots.h"
#include "gru_frag_prep.h"       // GRU_FRAG_BYTES

struct Dims : SirDims {
    int tw2, tw3, k2max, k3max;     // Winograd tile columns of conv2 / conv3, and 4-column task columns per utterance
};

static inline bool make_dims(int batch, int t_frames, Dims* d) {
    if (!sir_make_dims(batch, t_frames, d)) return false;
    d->tw2 = (d->wp1 + 1) / 2; d->tw3 = (d->wp2 + 1) / 2; d->k2max = (d->tw2 + 3) / 4; d->k3max = (d->tw3 + 3) / 4;
    return true;
}

// ---- the int sub-tables of WS_PAD: X(member, ints, alignment in ints) -------------------------------------------------------------
// One line per table, in layout order; `n` = B + 1 (the batch + the template utterance).  A padded call fills them from the scan
// (pad_extent_kernel, pad_tables_kernel); a ragged call puts the validated frames[B] in e0's place, d1 = W1, d3 = S_b and the tight
// lists (ragged_tables_kernel).
#define SIR_INFER_TABLES(X)                                                                                                            \
    X(e0, B, 1)                            /* E0[B]: 1 + last frame column with any bit set */                                         \
    X(d1, n, 1)                            /* conv1 columns per utterance */                                                           \
    X(d3, n, 1)                            /* GRU steps that see data, per utterance */                                                \
    X(gap2, 1 + n * d.k2max, 1)            /* unused: where conv2's task list lay when a task was one word (keeps the offsets behind it) */ \
    X(gap3, 1 + n * d.k3max, 1)            /* unused: the same of conv3's */                                                           \
    X(rows, 1 + n * d.S, 1)                /* layer-0 projection row list: count, then u * S + s ascending */                          \
    X(tab2, 2 + 2 * n * d.k2max, 2)        /* conv2 task list (Wino2Geo::ctab): {count, -}, then two words per task, read as int2 */   \
    X(tab3, 2 + 2 * n * d.k3max, 2)        /* conv3 task list */                                                                       \
    X(record, 2, 1)                        /* {rows read, tile chosen} of the latest row-list projection (ops.proj_tile_record) */     \
    X(nonfinite, B, 1)                     /* 1 where an utterance holds a NaN or an infinity: pad_extent_kernel -> the head kernel */

#define SIR_TABLE_OFFSET(member, ints, align) pos = sir_align_up(pos, align); t.member = pos; pos += (ints);
#define SIR_TABLE_OFFSET_MEMBER(member, ints, align) size_t member;
#define SIR_TABLE_MEMBER(member, ints, align) int* member;
#define SIR_TABLE_CARVE(member, ints, align) p.t.member = p.pad + tabs.member;

struct ITabs { SIR_INFER_TABLES(SIR_TABLE_OFFSET_MEMBER) size_t count; };      // int offsets inside WS_PAD, and the slot's ints
struct ITabPtrs { SIR_INFER_TABLES(SIR_TABLE_MEMBER) };

static inline ITabs itab_layout(const Dims& d) {
    const size_t B = d.B, n = B + 1;
    size_t pos = 0;
    ITabs t;
    SIR_INFER_TABLES(SIR_TABLE_OFFSET)
    t.count = pos;
    return t;
}

// ---- the slot table: X(slot, pointer member, element type, element count) ----------------------------------------------------------
// One line per slot, in layout order; the enum value WS_<slot> is the slot's published index.  Counts are expressions of `d` (Dims)
// with B = d.B, S = d.S and n = B + 1 (activation buffers: the batch + the template utterance, index B) as size_t.
#define SIR_INFER_SLOTS(X)                                                                                                             \
    X(A1, a1, float, n * 32 * d.wp1 * 32)        /* conv1 out  NHWC [n][32][T/2][32] */                                                \
    X(A2, a2, float, n * 16 * d.wp2 * 64)        /* conv2 out  NHWC [n][16][T/4][64] */                                                \
    X(X0, x0, float, n * S * 1024)               /* conv3 out = GRU input [n][S][1024], feature = c*8 + h */                           \
    X(GI, gi, float, n * S * 1536)               /* input projections of the current GRU layer [n*S][1536] */                          \
    X(Y0, y0, float, B * S * 512)                /* GRU layer 0 output [B][S][512] */                                                  \
    X(Y1, y1, float, B * S * 512)                /* GRU layer 1 output [B][S][512] */                                                  \
    X(CTX, ctx, float, B * 512)                  /* attention-pooled context [B][512] */                                               \
    X(PAD, pad, int, itab_layout(d).count)       /* pad-skip tables: SIR_INFER_TABLES above */                                         \
    X(XZ, xz, float, (size_t)64 * d.T)           /* all-zero feature row [64][T] of the template utterance (zeroed by pad_tables_kernel on every call) */ \
    X(BN, bn, float, 2 * 224)                    /* folded BN: scale[224] then shift[224] (channels of bn1|bn2|bn3) */                 \
    X(WHT, wht, unsigned char, 4 * GRU_FRAG_BYTES)   /* W_hh fragments of the recurrence kernel, [4 (layer, direction)][GRU_FRAG_BYTES] */ \
    X(XS, xs, unsigned short, n * S * 1024 * 2)  /* f16x2 planes (f16_split.h) of the current GEMM A operand, [2][n*S][1024] fp16 */   \
    X(WS, ws, unsigned short, 2 * WS_DIR0 + 2 * WS_DIR1)     /* f16x2 planes of W_ih: wsl0 [2 directions] WS_DIR0, wsl1 [2] WS_DIR1 */ \
    X(WCB, wcb, unsigned short, 3 * (WCB_W2 + WCB_W3 + WCB_W3_TAPS))   /* conv weights, 3 planes each: wcb2, wcb3 (16 Winograd frequencies per (cout, cin)), wcb3d (9 taps) */ \
    X(GXB, reserved0, char, 0)                   /* reserved (the exchange granules of the GRU clusters live in handle-owned buffers, sir_xbuf_acquire): keeps the index */ \
    X(GFL, reserved1, char, 0)                   /* reserved: keeps the index */

#define SIR_INFER_SLOT_ENUM(id, member, type, count) WS_##id,
enum WsBuf { SIR_INFER_SLOTS(SIR_INFER_SLOT_ENUM) WS_COUNT };

// byte offset of every slot; returns the workspace size
static inline size_t iws_layout(const Dims& d, size_t* off) {
    const size_t B = d.B, S = d.S, n = B + 1;
    size_t pos = 0;
    SIR_INFER_SLOTS(SIR_SLOT_OFFSET)
    return pos;
}

struct IPtrs {
    SIR_INFER_SLOTS(SIR_SLOT_MEMBER)
    ITabPtrs t;                                  // sub-tables of pad
    float *bns, *bnt;                            // sub-buffers of bn: scale, shift
    unsigned char* whh[4];                       // sub-buffers of wht: (layer, direction)
    unsigned short *wsl0[2], *wsl1[2];           // sub-buffers of ws: layer 0 / layer 1, by direction
    unsigned short *wcb2, *wcb3, *wcb3d;         // sub-buffers of wcb (wcb3d: only for shapes the Winograd kernel does not cover)
};

static inline IPtrs carve(void* ws, const size_t* off, const Dims& d) {
    char* b = (char*)ws;
    IPtrs p;
    SIR_INFER_SLOTS(SIR_SLOT_CARVE)
    const ITabs tabs = itab_layout(d);
    SIR_INFER_TABLES(SIR_TABLE_CARVE)
    p.bns = p.bn; p.bnt = p.bns + 224;
    for (int i = 0; i < 4; ++i) p.whh[i] = p.wht + i * GRU_FRAG_BYTES;
    for (int dir = 0; dir < 2; ++dir) { p.wsl0[dir] = p.ws + dir * WS_DIR0; p.wsl1[dir] = p.ws + 2 * WS_DIR0 + dir * WS_DIR1; }
    p.wcb2 = p.wcb; p.wcb3 = p.wcb2 + 3 * WCB_W2; p.wcb3d = p.wcb3 + 3 * WCB_W3;
    return p;
}
