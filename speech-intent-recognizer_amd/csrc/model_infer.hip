// sir_model_infer: eval-mode CNNAudioGRU.forward + argmax (models/models.py:41-68, scripts/evaluate.py:82-83)
// as a fixed sequence of hand-written kernels on one stream.  See model_kernels.h for the kernels.
//
// Pad skip.  Features are zero-padded to a fixed frame count (bench / pipeline: 200 frames for 94 real ones at 3 s).  A conv
// output whose receptive field sees only trailing all-+0.0 frame columns does not depend on the utterance: it equals what an
// all-zero utterance of the same width produces at that position.  So one extra "template" utterance (index B, fed from an
// all-zero feature row in the workspace) rides along at full width through conv1-3 and the layer-0 input projection, and for
// every real utterance only the columns that some non-template GRU step depends on are computed:
//   E0  = 1 + last frame column with any bit set (pad_extent_kernel; -0.0, NaN, denormals count as data)
//   d3  = min(S, (E0 + 14) / 8)   GRU steps s < d3 see data (conv3 output s reads frame columns >= 8 s - 7)
//   d2  = min(wp2, 2 d3 + 1), d1 = min(wp1, 2 d2 + 1)   columns of conv2 / conv1 those steps read
// conv1 stores pooled columns < d1; conv2 / conv3 run over a compacted list of 4-tile-column tasks (Wino2Geo::ctab), at most
// ceil(d / 4) of them per utterance (a last task with idle tile slots hosts columns of the template or of the next utterance:
// "Leftover packing" below); the layer-0 input projection runs over a row list (steps s < d3 of each utterance + the template's S
// rows) and the layer-0 recurrence reads the template's gi row for steps s >= d3.  Columns past the computed ones
// are left unwritten in a1 / a2 / x0 / xs / gi.  The conv fallback kernels (shapes the Winograd kernel does not cover) keep the
// full path.
//
// Ragged (sir_model_infer_ragged): the UN-PADDED function -- utterance b is computed as if it were alone in a batch of its own width
// frames[b] (scripts/test_tts_samples.py:83-96 feeds each file at its own length).  The same tables, given rather than scanned: no
// template utterance, W1 = frames / 2 columns of conv1, ceil((frames / 4) / 4) and ceil((frames / 8) / 4) task columns of conv2 /
// conv3, S_b = frames / 8 projection rows and GRU steps.  Every stage takes its right edge at the utterance's own width: conv1 reads
// frame columns >= frames[b] as zeros, the Winograd kernels source map columns past the width from the zero page and store no pooled
// column past half of it, both input projections run over the row list, the recurrences hold h while t >= S_b and the attention
// softmax runs over t < S_b.  On the conv fallback kernels the maps are masked to zero past the width by a pass of their own.
#include "f16x3_kernels.h"
#include "conv_fwd.h"
#include "gru_frag_prep.h"

namespace {

enum WsBuf {
    WS_A1 = 0,   // conv1 out  NHWC [B][32][T/2][32]
    WS_A2,       // conv2 out  NHWC [B][16][T/4][64]
    WS_X0,       // conv3 out = GRU input [B][S][1024], feature = c*8 + h
    WS_GI,       // input projections of the current GRU layer [B*S][1536]
    WS_Y0,       // GRU layer 0 output [B][S][512]
    WS_Y1,       // GRU layer 1 output [B][S][512]
    WS_CTX,      // attention-pooled context [B][512]
    WS_PAD,      // pad-skip tables (int): E0[B], conv1 columns d1[B + 1], GRU steps d3[B + 1], conv2 / conv3 task-column lists,
                 // layer-0 projection row list.  Ragged: validated frames[B] in E0's place, d1 = W1, d3 = S_b, the tight lists.
                 // Behind the tables: what the latest row-list projection read and chose, {rows, tile} (ops.proj_tile_record)
    WS_XZ,       // all-zero feature row [64][T] of the template utterance (zeroed by pad_tables_kernel on every call)
    WS_BN,       // folded BN: scale[224] then shift[224] (channels of bn1|bn2|bn3)
    WS_WHT,      // W_hh fragments of the recurrence kernel, [4 (layer, direction)][GRU_FRAG_BYTES]
    WS_XS,       // f16x2 planes (f16_split.h) of the current GEMM A operand, [2][B*S][1024] fp16
    WS_WS,       // f16x2 planes of W_ih: l0 [2 directions][2][768][1024], l1 [2][2][768][512]
    WS_WCB,      // bf16x3 planes of the conv2 / conv3 weights
    WS_GXB,      // (unused: the exchange granules of the GRU clusters live in handle-owned buffers, sir_xbuf_acquire)
    WS_GFL,      // (unused)
    WS_COUNT
};

struct Dims : SirDims {
    int tw2, tw3, k2max, k3max;     // Winograd tile columns of conv2 / conv3, and 4-column task columns per utterance
};

bool make_dims(int batch, int t_frames, Dims* d) {
    if (!sir_make_dims(batch, t_frames, d)) return false;
    d->tw2 = (d->wp1 + 1) / 2; d->tw3 = (d->wp2 + 1) / 2; d->k2max = (d->tw2 + 3) / 4; d->k3max = (d->tw3 + 3) / 4;
    return true;
}

// int offsets inside WS_PAD
struct PadTabs { size_t e0, d1, d3, tab2, tab3, rows, count; };     // (count: the tables' ints; behind them the projection's record, 2 ints,
                                                                     // and behind that one non-finite flag per utterance, B ints)
PadTabs pad_tabs(const Dims& d) {
    PadTabs t;
    const size_t n = (size_t)d.B + 1;
    // (e0, d1, d3 and the row list keep the places they had when a task was one word; the task lists, two words per task and
    // 8-byte aligned, follow the row list)
    t.e0 = 0; t.d1 = d.B; t.d3 = t.d1 + n; t.rows = t.d3 + n + 1 + n * d.k2max + 1 + n * d.k3max;
    t.tab2 = t.rows + 1 + n * d.S; t.tab2 += t.tab2 & 1;
    t.tab3 = t.tab2 + 2 + 2 * n * d.k2max;
    t.count = t.tab3 + 2 + 2 * n * d.k3max;
    return t;
}

void ws_sizes(const Dims& d, size_t* bytes) {
    const size_t B = d.B + 1;       // activation buffers: the batch + the template utterance (index B)
    bytes[WS_A1] = B * 32 * d.wp1 * 32 * 4;
    bytes[WS_A2] = B * 16 * d.wp2 * 64 * 4;
    bytes[WS_X0] = B * d.S * 1024 * 4;
    bytes[WS_GI] = B * d.S * 1536 * 4;
    bytes[WS_Y0] = (size_t)d.B * d.S * 512 * 4;
    bytes[WS_Y1] = (size_t)d.B * d.S * 512 * 4;
    bytes[WS_CTX] = (size_t)d.B * 512 * 4;
    bytes[WS_PAD] = (pad_tabs(d).count + 2 + (size_t)d.B) * 4;  // + {row count read, tile chosen} of the latest row-list projection + the flags
    bytes[WS_XZ] = (size_t)64 * d.T * 4;
    bytes[WS_BN] = (size_t)2 * 224 * 4;
    bytes[WS_WHT] = 4 * GRU_FRAG_BYTES;                         // W_hh as the resident f16x2 MFMA fragments of the recurrence kernel
    bytes[WS_XS] = B * d.S * 1024 * 2 * 2;
    bytes[WS_WS] = ((size_t)2 * 2 * 768 * 1024 + (size_t)2 * 2 * 768 * 512) * 2;
    bytes[WS_WCB] = ((size_t)3 * 32 * 16 * 64 + (size_t)3 * 64 * 16 * 128 + (size_t)3 * 64 * 9 * 128) * 2;   // conv2, conv3: 16 Winograd frequencies per (cout, cin); conv3 again with 9 taps for the direct kernel (shapes the Winograd kernel does not cover)
    bytes[WS_GXB] = 0;
    bytes[WS_GFL] = 0;
}

size_t ws_layout(const Dims& d, size_t* off) {
    size_t bytes[WS_COUNT], pos = 0;
    ws_sizes(d, bytes);
    for (int i = 0; i < WS_COUNT; ++i) {
        off[i] = pos;
        pos += sir_align_up(bytes[i], 256);
    }
    return pos;
}

// E0[b] = 1 + the last frame column of utterance b with any bit set in any of the 64 mel rows, 0 if none (bits, not values:
// -0.0, NaN and denormals are data).  nonfinite[b] = 1 if any of its features is a NaN or an infinity (exponent bits all set), else 0:
// the head kernel turns such a row into NaNs, which the ReLU / max-pool of the conv kernels (fmaxf) would not carry there.
// frames != NULL (ragged): only the columns below frames[b] are looked at (none if that length is invalid) and e0 is not written.
static __global__ __launch_bounds__(256) void pad_extent_kernel(const float* __restrict__ x, int T, int* __restrict__ e0,
                                                                 const int* __restrict__ frames, int* __restrict__ nonfinite) {
    const unsigned* xb = reinterpret_cast<const unsigned*>(x) + (size_t)blockIdx.x * 64 * T;
    int last = -1, cols = T;
    if (frames) { const int f = frames[blockIdx.x]; cols = f >= 8 && f <= T ? f : 0; }
    unsigned nf = 0;                                          // the largest magnitude seen, as bits
    for (int c = threadIdx.x; c < cols; c += 256) {
        unsigned acc = 0;
#pragma unroll 32
        for (int r = 0; r < 64; ++r) {
            const unsigned v = xb[(size_t)r * T + c];
            acc |= v;
            nf = max(nf, v & 0x7fffffffu);
        }
        if (acc) last = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o));
    const bool wave_nf = __ballot(nf >= 0x7f800000u) != 0;    // exponent bits all set: an infinity or a NaN
    __shared__ int wl[4], wn[4];
    if ((threadIdx.x & 63) == 0) { wl[threadIdx.x >> 6] = last; wn[threadIdx.x >> 6] = wave_nf ? 1 : 0; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (e0) e0[blockIdx.x] = max(max(wl[0], wl[1]), max(wl[2], wl[3])) + 1;
        nonfinite[blockIdx.x] = wn[0] | wn[1] | wn[2] | wn[3];
    }
}

// Leftover packing of the conv2 / conv3 task lists (Wino2Geo::ctab).  Image u, having given its first g columns away, lists its
// other r = c - g columns from tile column g on, four to a task; the last task holds l = r mod 4 of them.  A last task with l = 1 can
// host a guest segment of up to 2 tile columns of another image, one with l = 2 of 1 (pk_cap); l = 3 cannot (2 nA + 2 <= 2 sB).
// Guests are taken, in the order of the hosts,
//   1. from the template's columns (ascending) while it has any left -- a host takes min(capacity, left) of them;
//   2. after that from the head of the NEXT image: min(capacity, that image's need) columns, which that image then does not list itself
//      (so its own leftover changes: the hand-overs chain).
// What the template has left it lists itself, last.  The guest sits in the task's LAST slots: sB = 4 - nB.
// A list never grows by this: image u lists ceil((c - g) / 4) <= ceil(c / 4) tasks, so (B + 1) * kmax still bounds it.
__device__ __forceinline__ int pk_cap(int r) { const int l = r & 3; return l == 1 ? 2 : l == 2 ? 1 : 0; }
// columns that an image of need c, g of them given away, takes from a next image of need cn (rule 2)
__device__ __forceinline__ int pk_take(int c, int g, int cn) { return g <= c ? min(pk_cap(c - g), cn) : 0; }
// the hand-over as a function g_in -> g_out on {0, 1, 2}, two bits per value, so that a chain of them composes (and scans)
constexpr int PK_ID = 0 | 1 << 2 | 2 << 4;
__device__ __forceinline__ int pk_fn(int c, int cn) { return pk_take(c, 0, cn) | pk_take(c, 1, cn) << 2 | pk_take(c, 2, cn) << 4; }
__device__ __forceinline__ int pk_then(int f, int g) {       // f first, then g
    int r = 0;
#pragma unroll
    for (int x = 0; x < 3; ++x) r |= ((g >> (2 * ((f >> (2 * x)) & 3))) & 3) << (2 * x);
    return r;
}
// the tasks of one image in one list: first tile column base + g, r columns; the last task hosts nB columns from gB (nB = 0: no guest)
__device__ __forceinline__ void pk_emit(int* __restrict__ tab, int o, int base, int g, int r, int gB, int nB) {
    const int k = (r + 3) >> 2;
    for (int t = 0; t < k; ++t) {
        reinterpret_cast<int2*>(tab)[1 + o + t] = make_int2((base + g + 4 * t) << 2 | (min(4, r - 4 * t) - 1),
                                                            t == k - 1 && nB > 0 ? gB << 2 | (2 - nB) << 1 | (nB - 1) : -1);
    }
}

// prefix sums over `nu` utterances of what `need(u, c1, c2, c3)` demands (columns of conv1 / conv2 / conv3) -> conv1 columns d1o, GRU
// steps d3o, the compacted task lists of conv2 / conv3 (Wino2Geo::ctab) and the projection's row list (u * S + s for s < c3,
// ascending).  PACK: utterance nu - 1 is the template and leftovers are packed (above); else the lists carry no guests.  One workgroup
// of 1024 threads; deterministic (three scans: guest capacities and rows, hand-overs, task counts -- each a shuffle scan inside the
// waves and a fold over the 16 wave totals, two barriers).
template <bool PACK, typename Need>
__device__ __forceinline__ void pad_tables_emit(const Dims& d, int nu, Need need, int* __restrict__ d1o, int* __restrict__ d3o,
                                                int* __restrict__ tab2, int* __restrict__ tab3, int* __restrict__ prow) {
    const int tid = threadIdx.x;
    const int per = (nu + 1023) / 1024, u0 = min(nu, tid * per), u1 = min(nu, u0 + per);
    const int nr = PACK ? nu - 1 : nu;                        // real utterances
    __shared__ int wt[3][16];
    // exclusive prefixes (in place) and totals of three values per thread under the associative `op` (earlier operand first)
    auto scan = [&](auto op, int id, int& a, int& b, int& c, int& ta, int& tb, int& tc) {
        const int ln = tid & 63, wv = tid >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int xa = __shfl_up(a, o), xb = __shfl_up(b, o), xc = __shfl_up(c, o);
            if (ln >= o) { a = op(xa, a); b = op(xb, b); c = op(xc, c); }
        }
        __syncthreads();                                      // (the totals of the scan before have been read)
        if (ln == 63) { wt[0][wv] = a; wt[1][wv] = b; wt[2][wv] = c; }
        __syncthreads();
        int pa = id, pb = id, pc = id;
        ta = id; tb = id; tc = id;
        for (int w = 0; w < 16; ++w) {
            const int va = wt[0][w], vb = wt[1][w], vc = wt[2][w];
            if (w < wv) { pa = op(pa, va); pb = op(pb, vb); pc = op(pc, vc); }
            ta = op(ta, va); tb = op(tb, vb); tc = op(tc, vc);
        }
        const int xa = __shfl_up(a, 1), xb = __shfl_up(b, 1), xc = __shfl_up(c, 1);
        a = ln ? op(pa, xa) : pa; b = ln ? op(pb, xb) : pb; c = ln ? op(pc, xc) : pc;
    };
    auto add = [](int a, int b) { return a + b; };
    int c1, c2, c3, n1, n2, n3;
    // 1. guest capacities of the hosts as long as the template feeds them (no hand-over, g = 0), and projection rows
    int q2_0 = 0, q3_0 = 0, orw0 = 0, cap2, cap3, nrow;
    for (int u = u0; u < u1; ++u) { need(u, c1, c2, c3); orw0 += c3; if (PACK && u < nr) { q2_0 += pk_cap(c2); q3_0 += pk_cap(c3); } }
    scan(add, 0, q2_0, q3_0, orw0, cap2, cap3, nrow);
    int t2 = 0, t3 = 0, gt2 = 0, gt3 = 0;                     // the template's need and what the hosts take of it
    if (PACK) { need(nr, c1, t2, t3); gt2 = min(t2, cap2); gt3 = min(t3, cap3); }
    // 2. hand-overs: host u takes from the template while columns of it are left (capacity prefix q < t), from image u + 1 after
    int g2 = 0, g3 = 0;
    if (PACK) {
        int f2 = PK_ID, f3 = PK_ID, fx = PK_ID, q2 = q2_0, q3 = q3_0, x2, x3, xx;
        for (int u = u0; u < min(u1, nr); ++u) {
            need(u, c1, c2, c3);
            n2 = n3 = 0;
            if (u + 1 < nr) need(u + 1, n1, n2, n3);
            f2 = pk_then(f2, q2 < t2 ? 0 : pk_fn(c2, n2)); f3 = pk_then(f3, q3 < t3 ? 0 : pk_fn(c3, n3));
            q2 += pk_cap(c2); q3 += pk_cap(c3);
        }
        scan([](int a, int b) { return pk_then(a, b); }, PK_ID, f2, f3, fx, x2, x3, xx);
        g2 = f2 & 3; g3 = f3 & 3;                             // (the first image is handed nothing: f(0))
    }
    // 3. task counts.  walk(emit): this thread's utterances with their hand-overs, counting or writing
    auto walk = [&](bool emit, int& o2, int& o3, int orw) {
        int q2 = q2_0, q3 = q3_0, h2 = g2, h3 = g3;
        for (int u = u0; u < u1; ++u) {
            need(u, c1, c2, c3);
            int b2 = 0, b3 = 0, m2 = 0, m3 = 0, x2 = 0, x3 = 0;   // guest: first column, count; hand-over to the next image
            if (PACK && u < nr) {
                n2 = n3 = 0;
                if (u + 1 < nr) need(u + 1, n1, n2, n3);
                if (q2 < t2) { b2 = nr * d.tw2 + q2; m2 = min(pk_cap(c2), t2 - q2); } else { b2 = (u + 1) * d.tw2; m2 = x2 = pk_take(c2, h2, n2); }
                if (q3 < t3) { b3 = nr * d.tw3 + q3; m3 = min(pk_cap(c3), t3 - q3); } else { b3 = (u + 1) * d.tw3; m3 = x3 = pk_take(c3, h3, n3); }
                q2 += pk_cap(c2); q3 += pk_cap(c3);
            } else if (PACK) { h2 = gt2; h3 = gt3; }            // the template lists what is left of it
            const int r2 = c2 - h2, r3 = c3 - h3;
            if (emit) {
                d1o[u] = c1; d3o[u] = c3;
                pk_emit(tab2, o2, u * d.tw2, h2, r2, b2, m2);
                pk_emit(tab3, o3, u * d.tw3, h3, r3, b3, m3);
                for (int s = 0; s < c3; ++s) prow[1 + orw + s] = u * d.S + s;
            }
            o2 += (r2 + 3) >> 2; o3 += (r3 + 3) >> 2; orw += c3;
            h2 = x2; h3 = x3;
        }
    };
    int o2 = 0, o3 = 0, ox = 0, nt2, nt3, ntx;
    walk(false, o2, o3, 0);
    scan(add, 0, o2, o3, ox, nt2, nt3, ntx);
    walk(true, o2, o3, orw0);
    if (tid == 0) { tab2[0] = nt2; tab3[0] = nt3; prow[0] = nrow; }
}

// one workgroup: demanded columns per utterance from E0 (see the head of this file; utterance B = the template, full width),
// prefix sums over the batch -> compacted, leftover-packed task lists of conv2 / conv3 (Wino2Geo::ctab), the layer-0 projection's row list
// (u * S + s for s < d3[u], ascending; the template's S rows last), and the template's zero features
static __global__ __launch_bounds__(1024) void pad_tables_kernel(const int* __restrict__ e0, Dims d, int* __restrict__ d1o, int* __restrict__ d3o,
                                                                 int* __restrict__ tab2, int* __restrict__ tab3, int* __restrict__ prow,
                                                                 float* __restrict__ xz) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 64 * d.T; i += 1024) xz[i] = 0.0f;
    auto need = [&](int u, int& c1, int& c2, int& c3) {
        if (u == d.B) { c1 = d.wp1; c2 = d.wp2; c3 = d.S; return; }
        c3 = min(d.S, (e0[u] + 14) / 8);
        c2 = min(d.wp2, 2 * c3 + 1);
        c1 = min(d.wp1, 2 * c2 + 1);
    };
    pad_tables_emit<true>(d, d.B + 1, need, d1o, d3o, tab2, tab3, prow);
}

// Ragged: the same tables from the GIVEN lengths, B utterances, no template.  fw[b] = frames[b], or 0 where it is outside [8, T]:
// such an utterance gets no column, no row and no step (its logits become NaN in attention_pool_ragged_kernel) and raises bit 6 of
// the handle's status word.  Widths follow from fw alone: W1 = fw / 2 (conv1 out), W2 = fw / 4 (conv2 out), S_b = fw / 8.
static __global__ __launch_bounds__(1024) void ragged_tables_kernel(const int* __restrict__ frames, Dims d, int* __restrict__ fw, int* __restrict__ d1o,
                                                                    int* __restrict__ d3o, int* __restrict__ tab2, int* __restrict__ tab3,
                                                                    int* __restrict__ prow, unsigned int* __restrict__ status) {
    bool bad = false;
    for (int u = threadIdx.x; u < d.B; u += 1024) {
        const int f0 = frames[u], f = f0 >= 8 && f0 <= d.T ? f0 : 0;
        fw[u] = f;
        bad |= f == 0;
    }
    if (bad) __hip_atomic_fetch_or(status, 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                                          // fw is read back below by other threads of this (one) workgroup
    auto need = [&](int u, int& c1, int& c2, int& c3) {
        const int f = fw[u];
        c1 = f >> 1; c2 = f >> 2; c3 = f >> 3;
    };
    pad_tables_emit<false>(d, d.B, need, d1o, d3o, tab2, tab3, prow);     // (guest-free: the ragged kernel form reads no guest word)
}

// Ragged on the conv fallback kernels (they run at full width): map columns >= fw[b] >> sh of image b become zeros -- the image edge
// the next conv reads, and no stale workspace bits behind it.  a: NHWC [B][H][W][C], grid (H, B).
static __global__ __launch_bounds__(256) void ragged_mask_kernel(float* __restrict__ a, const int* __restrict__ fw, int sh, int H, int W, int C) {
    const int b = blockIdx.y, r = blockIdx.x, w0 = min(W, fw[b] >> sh);
    float4* row = reinterpret_cast<float4*>(a + (((size_t)b * H + r) * W + w0) * C);
    const int n4 = (W - w0) * (C / 4);
    for (int i = threadIdx.x; i < n4; i += 256) row[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace

extern "C" size_t sir_model_workspace_bytes(const sir_handle* h, int batch, int t_frames, int train) {
    (void)h;
    if (train) return sir_train_workspace_bytes_impl(batch, t_frames);
    Dims d;
    if (!make_dims(batch, t_frames, &d)) return 0;
    size_t off[WS_COUNT];
    return ws_layout(d, off);
}

extern "C" int sir_model_workspace_offsets(const sir_handle* h, int batch, int t_frames, int train, size_t* offsets,
                                           int n) {
    (void)h; (void)train;
    Dims d;
    if (!make_dims(batch, t_frames, &d) || !offsets) {
        sir_set_error("sir_model_workspace_offsets: bad shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", batch, t_frames);
        return SIR_EINVAL;
    }
    size_t off[WS_COUNT];
    ws_layout(d, off);
    for (int i = 0; i < n && i < WS_COUNT; ++i) offsets[i] = off[i];
    return WS_COUNT;
}

// frames == nullptr: the padded function with the pad skip (sir_model_infer); else the ragged one (head of this file)
static int model_infer_impl(const char* who, sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, int batch,
                            int t_frames, float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!h || !w || !feats || !logits || !workspace) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    Dims d;
    if (!make_dims(batch, t_frames, &d)) {
        sir_set_error("%s: unsupported shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", who, batch, t_frames);
        return SIR_EINVAL;
    }
    if (h->cfg.n_mels != 64) { sir_set_error("%s: the model is wired for 64 mels (models.py:23)", who); return SIR_EUNSUPPORTED; }
    if (w->num_classes < 1 || w->num_classes > 64) { sir_set_error("%s: num_classes=%d", who, w->num_classes); return SIR_EINVAL; }
    size_t off[WS_COUNT];
    const size_t need = ws_layout(d, off);
    if (workspace_bytes < need) { sir_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need); return SIR_ENOMEM; }
    if (((uintptr_t)workspace & 255) != 0) { sir_set_error("%s: workspace must be 256-byte aligned", who); return SIR_EINVAL; }
    const bool ragged = frames != nullptr;
    hipStream_t st = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* a1 = (float*)(ws + off[WS_A1]);
    float* a2 = (float*)(ws + off[WS_A2]);
    float* x0 = (float*)(ws + off[WS_X0]);
    float* gi = (float*)(ws + off[WS_GI]);
    float* y0 = (float*)(ws + off[WS_Y0]);
    float* y1 = (float*)(ws + off[WS_Y1]);
    float* ctx = (float*)(ws + off[WS_CTX]);
    float* bns = (float*)(ws + off[WS_BN]);
    float* bnt = bns + 224;
    float* wht = (float*)(ws + off[WS_WHT]);
    unsigned short* xs = (unsigned short*)(ws + off[WS_XS]);
    unsigned short* wsl0 = (unsigned short*)(ws + off[WS_WS]);
    unsigned short* wsl1 = wsl0 + (size_t)2 * 2 * 768 * 1024;
    unsigned short* wcb2 = (unsigned short*)(ws + off[WS_WCB]);
    unsigned short* wcb3 = wcb2 + (size_t)3 * 32 * 16 * 64;       // Winograd form
    unsigned short* wcb3d = wcb3 + (size_t)3 * 64 * 16 * 128;     // direct form (fallback)
    const int B = d.B, S = d.S;
    const PadTabs pt = pad_tabs(d);
    int* const ptab = (int*)(ws + off[WS_PAD]);
    float* const xz = (float*)(ws + off[WS_XZ]);
    // tile rule of the row-list projections (f16x3_kernels.h): CU time instead of latency while launches alternate between streams.
    // Read once per call (the recurrence launches below may flip it)
    const bool proj_throughput = h->cluster_multi;
    int* const proj_rec = ptab + pt.count;
    int* const nonfinite = proj_rec + 2;                        // [B]: pad_extent_kernel -> the head kernel

    // conv2 / conv3 as Winograd F(2x2, 3x3) -- the 2x2 output tile is the pooling window -- on the producer / consumer kernel
    // (conv_wino2_f16x3_kernel.h); shapes it does not cover (batch x map beyond 32-bit offsets) keep the bf16x6 fallback kernels.
    // The pad skip (head of this file) runs with the Winograd kernels, over the batch + the template utterance.
    const SirConvPlan cp = sir_conv_plan(&d, true);             // (true: the template utterance)
    const bool w2 = cp.fwd_wino;
    const int BT = w2 ? B + 1 : B;                                // utterances through conv1-3 and the layer-0 projection
    // (ragged: no template utterance is computed, but the plan, the plane stride of xs and the table offsets stay those of the
    // padded call -- and so does the prepared-weight key: a ragged and a padded call may alternate on one workspace)

    // ---- weight preparation -------------------------------------------------------------
    // skipped when the caller vouches (sir_model_set_weights_version) that the weights are the ones prepared
    // into this very workspace by the previous call
    const long long prep_key = ((long long)B << 32) | (unsigned)d.T;
    sir_handle::PrepEntry* pe = nullptr;
    for (auto& e : h->prep)
        if (e.ws == workspace) pe = &e;
    const bool reuse_prep = pe && h->weights_version != 0 && pe->version == h->weights_version && pe->key == prep_key;
    if (!reuse_prep) {
        SirProfScope prof(h, SIR_K_PREP, st);
        const int bn_c[3] = {32, 64, 128}, bn_o[3] = {0, 32, 96};
        for (int i = 0; i < 3; ++i)
            hipLaunchKernelGGL(prep_bn_kernel, dim3(1), dim3(128), 0, st, w->bn_w[i], w->bn_b[i], w->bn_mean[i], w->bn_var[i],
                               bns + bn_o[i], bnt + bn_o[i], bn_c[i], i == 0 ? w->conv_w[0] : (const float*)nullptr, i == 0 ? 288 : 0, h->status);
        for (int i = 0; i < 4; ++i) sir_prep_whh_quad(h, st, w->gru_w_hh[i], (unsigned char*)wht + (size_t)i * GRU_FRAG_BYTES);
        // (the weight planes are prepared in the arithmetic of the kernel that will read them: f16x3 for the second-generation
        // Winograd kernel's forward stages, bf16x3 for the first-generation / direct fallbacks)
        if (w2) hipLaunchKernelGGL(prep_conv_w_wino_f16x3_kernel, dim3((32 * 16 * 64 + 255) / 256), dim3(256), 0, st, w->conv_w[1], wcb2, 32, 64, h->status);
        else hipLaunchKernelGGL(prep_conv_w_wino_bf16x3_kernel, dim3((32 * 16 * 64 + 255) / 256), dim3(256), 0, st, w->conv_w[1], wcb2, 32, 64);
        if (w2) hipLaunchKernelGGL(prep_conv_w_wino_f16x3_kernel, dim3((64 * 16 * 128 + 255) / 256), dim3(256), 0, st, w->conv_w[2], wcb3, 64, 128, h->status);
        else hipLaunchKernelGGL(prep_conv_w_wino_bf16x3_kernel, dim3((64 * 16 * 128 + 255) / 256), dim3(256), 0, st, w->conv_w[2], wcb3, 64, 128);
        hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3((64 * 9 * 128 + 255) / 256), dim3(256), 0, st, w->conv_w[2], wcb3d, 64, 128);
        for (int dir = 0; dir < 2; ++dir) {
            hipLaunchKernelGGL(split2h_weights_kernel, dim3(384), dim3(256), 0, st, w->gru_w_ih[dir], 1024, wsl0 + (size_t)dir * 2 * 768 * 1024, (size_t)768, 1024, h->status);
            hipLaunchKernelGGL(split2h_weights_kernel, dim3(192), dim3(256), 0, st, w->gru_w_ih[2 + dir], 512, wsl1 + (size_t)dir * 2 * 768 * 512, (size_t)768, 512, h->status);
        }
        if (!pe) { pe = &h->prep[h->prep_next]; h->prep_next = (h->prep_next + 1) % 4; }
        pe->ws = workspace; pe->version = h->weights_version; pe->key = prep_key;
    }
    SIR_KCHECK();

    // ---- CNN stack: conv + folded BN + ReLU + 2x2 max-pool per launch ------------------------------
    {
        SirProfScope prof(h, SIR_K_CONV1, st);
        if (ragged) {                                             // tables from the given lengths; conv1 at each utterance's own width
            hipLaunchKernelGGL(pad_extent_kernel, dim3(B), dim3(256), 0, st, feats, d.T, (int*)nullptr, (const int*)frames, nonfinite);
            hipLaunchKernelGGL(ragged_tables_kernel, dim3(1), dim3(1024), 0, st, (const int*)frames, d, ptab + pt.e0, ptab + pt.d1, ptab + pt.d3,
                               ptab + pt.tab2, ptab + pt.tab3, ptab + pt.rows, h->status);
            hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_ragged_kernel, conv1_grid(B, d.wp1), dim3(256), 0, st, feats,
                               w->conv_w[0], bns, bnt, a1, 64, d.T, 32, d.wp1, (const int*)(ptab + pt.d1), (const int*)(ptab + pt.e0));
            // (fallback path only: the mask of conv1's map is counted with conv1, that of conv2's map with conv2 in sir_profile_*)
            if (!w2) hipLaunchKernelGGL(ragged_mask_kernel, dim3(32, B), dim3(256), 0, st, a1, (const int*)(ptab + pt.e0), 1, 32, d.wp1, 32);
        } else {
        // (the scan also flags non-finite features for the head kernel: it runs on the fallback path too, where nothing reads e0)
        hipLaunchKernelGGL(pad_extent_kernel, dim3(B), dim3(256), 0, st, feats, d.T, ptab + pt.e0, (const int*)nullptr, nonfinite);
        if (w2) {                                                 // pad-skip tables (the scan and this: two small launches, counted with conv1)
            hipLaunchKernelGGL(pad_tables_kernel, dim3(1), dim3(1024), 0, st, (const int*)(ptab + pt.e0), d, ptab + pt.d1, ptab + pt.d3,
                               ptab + pt.tab2, ptab + pt.tab3, ptab + pt.rows, xz);
        }
        hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_kernel, conv1_grid(BT, d.wp1), dim3(256), 0, st, feats,
                           w->conv_w[0], bns, bnt, a1, 64, d.T, 32, d.wp1, (const float*)xz, B, w2 ? (const int*)(ptab + pt.d1) : (const int*)nullptr);
        }
    }
    // (the lists' capacity and the grid bound, (B + 1) * kmax tasks: no image lists more than ceil(need / 4) <= kmax tasks, packed or
    // not -- pad_tables_emit)
    {
        SirProfScope prof(h, SIR_K_CONV2, st);
        if (ragged) {
            SIR_TRY((conv_fwd<32, 64, 0, true>(h, st, w2, cp.geo2, B, a1, wcb2, nullptr, bns + 32, bnt + 32, a2, nullptr, ptab + pt.tab2, (B + 1) * d.k2max,
                                               ptab + pt.e0, 1)));
            if (!w2) hipLaunchKernelGGL(ragged_mask_kernel, dim3(16, B), dim3(256), 0, st, a2, (const int*)(ptab + pt.e0), 2, 16, d.wp2, 64);
        } else
        SIR_TRY((conv_fwd<32, 64, 0>(h, st, w2, cp.geo2, BT, a1, wcb2, nullptr, bns + 32, bnt + 32, a2, nullptr, ptab + pt.tab2, (B + 1) * d.k2max)));
    }
    {
        // conv3 stores straight into the GRU input layout [B][S][c*8+h] (models.py:55-57) and writes the f16x2 planes of
        // the first input projection's A operand beside it
        SirProfScope prof(h, SIR_K_CONV3, st);
        if (ragged)
            SIR_TRY((conv_fwd<64, 128, 1, true>(h, st, w2, cp.geo3, B, a2, wcb3, wcb3d, bns + 96, bnt + 96, x0, (float2*)xs, ptab + pt.tab3, (B + 1) * d.k3max,
                                                ptab + pt.e0, 2)));
        else
        SIR_TRY((conv_fwd<64, 128, 1>(h, st, w2, cp.geo3, BT, a2, wcb3, wcb3d, bns + 96, bnt + 96, x0, (float2*)xs, ptab + pt.tab3, (B + 1) * d.k3max)));
    }
    SIR_KCHECK();

    // ---- 2-layer bidirectional GRU ----------------------------------------------------------
    const int M = B * S;
    {
        // pad skip: only the rows the recurrence reads (the row list of pad_tables_kernel: steps s < d3 of every utterance and the
        // template's S rows), on a tile the compacted count fills the chip with; the other gi rows are left unwritten
        SirProfScope prof(h, SIR_K_GEMM_IH0, st);
        if (w2 || ragged)                                         // (ragged: the rows s < S_b of every utterance, on either conv path)
            SIR_TRY(launch_gemm_nt_f16x3_gather(h, st, (const unsigned short*)xs, (const unsigned short*)wsl0,
                                                    (const unsigned short*)(wsl0 + (size_t)2 * 768 * 1024), w->gru_b_ih[0], w->gru_b_ih[1], gi, 1536,
                                                    (const int*)(ptab + pt.rows), BT * S, 768, 1024, proj_throughput, proj_rec));
        else
            SIR_TRY(launch_gemm_nt_f16x3(h, st, (const unsigned short*)xs, (const unsigned short*)wsl0,
                                             (const unsigned short*)(wsl0 + (size_t)2 * 768 * 1024), w->gru_b_ih[0], w->gru_b_ih[1], gi, 1536, M, 768, 1024));
    }
    {
        SirProfScope prof(h, SIR_K_GRU0, st);
        // layer 0 also writes the f16x2 planes of ITS output: the A operand of the layer-1 projection
        SIR_TRY(sir_launch_gru_quad(h, st, false, gi, w->gru_w_hh[0], w->gru_w_hh[1], w->gru_b_hh[0], w->gru_b_hh[1], y0, B, S, nullptr,
                                    xs, wht, (unsigned char*)wht + GRU_FRAG_BYTES, w2 || ragged ? (const int*)(ptab + pt.d3) : (const int*)nullptr, ragged));
    }
    {
        SirProfScope prof(h, SIR_K_GEMM_IH1, st);
        if (ragged)                                               // the same row list: layer 0 wrote y0's planes for exactly these rows
            SIR_TRY(launch_gemm_nt_f16x3_gather(h, st, (const unsigned short*)xs, (const unsigned short*)wsl1,
                                                    (const unsigned short*)(wsl1 + (size_t)2 * 768 * 512), w->gru_b_ih[2], w->gru_b_ih[3], gi, 1536,
                                                    (const int*)(ptab + pt.rows), M, 768, 512, proj_throughput, proj_rec));
        else
        SIR_TRY(launch_gemm_nt_f16x3(h, st, (const unsigned short*)xs, (const unsigned short*)wsl1,
                                         (const unsigned short*)(wsl1 + (size_t)2 * 768 * 512), w->gru_b_ih[2], w->gru_b_ih[3], gi, 1536, M, 768, 512));
    }
    {
        SirProfScope prof(h, SIR_K_GRU1, st);
        SIR_TRY(sir_launch_gru_quad(h, st, false, gi, w->gru_w_hh[2], w->gru_w_hh[3], w->gru_b_hh[2], w->gru_b_hh[3], y1, B, S, nullptr,
                                    nullptr, (unsigned char*)wht + 2 * GRU_FRAG_BYTES, (unsigned char*)wht + 3 * GRU_FRAG_BYTES,
                                    ragged ? (const int*)(ptab + pt.d3) : (const int*)nullptr, ragged));
    }
    SIR_KCHECK();

    // ---- attention pooling + classifier head ------------------------------------------------
    {
        SirProfScope prof(h, SIR_K_ATTN, st);
        if (ragged)
            hipLaunchKernelGGL(attention_pool_ragged_kernel, dim3(B), dim3(256), 0, st, y1, w->attn_w, w->attn_b, ctx, S, w->fc_w, w->fc_b,
                               w->num_classes, logits, (long long*)argmax, (const int*)(ptab + pt.d3), (const int*)nonfinite);
        else
        hipLaunchKernelGGL(attention_pool_kernel, dim3(B), dim3(256), 0, st, y1, w->attn_w, w->attn_b, ctx, S, w->fc_w, w->fc_b,
                           w->num_classes, logits, (long long*)argmax, (const int*)nonfinite, (const double*)nullptr);
    }
    SIR_KCHECK();
    return SIR_OK;
}

extern "C" int sir_model_infer(sir_handle* h, const sir_model_weights* w, const float* feats, int batch, int t_frames,
                               float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream_) {
    return model_infer_impl("sir_model_infer", h, w, feats, nullptr, batch, t_frames, logits, argmax, workspace, workspace_bytes, stream_);
}

extern "C" int sir_model_infer_ragged(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, int batch,
                                      int t_frames, float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
    if (!frames) { sir_set_error("sir_model_infer_ragged: NULL frames"); return SIR_EINVAL; }
    return model_infer_impl("sir_model_infer_ragged", h, w, feats, frames, batch, t_frames, logits, argmax, workspace, workspace_bytes, stream_);
}
