// The device code that builds the inference tables (the WS_PAD slot, infer_workspace.h) ahead of the model's kernels; launched by
// model_infer.hip, whose head comment says what the model's kernels do with them.
//
// Pad skip (sir_model_infer).  Per utterance, from the features alone:
//   E0  = 1 + last frame column with any bit set (pad_extent_kernel; -0.0, NaN, denormals count as data)
//   d3  = min(S, (E0 + 14) / 8)   GRU steps s < d3 see data (conv3 output s reads frame columns >= 8 s - 7)
//   d2  = min(wp2, 2 d3 + 1), d1 = min(wp1, 2 d2 + 1)   columns of conv2 / conv1 those steps read
// and for the template utterance (index B) the full widths.  From these pad_tables_kernel lists, for conv2 / conv3, 4-tile-column
// tasks (Wino2Geo::ctab), at most ceil(d / 4) of them per utterance (a last task with idle tile slots hosts columns of the template
// or of the next utterance: "Leftover packing" below), and for the layer-0 input projection the rows s < d3 of each utterance + the
// template's S rows.
//
// Ragged (sir_model_infer_ragged).  The same tables, given rather than scanned (ragged_tables_kernel): no template utterance,
// W1 = frames / 2 columns of conv1, ceil((frames / 4) / 4) and ceil((frames / 8) / 4) task columns of conv2 / conv3, S_b = frames / 8
// projection rows and GRU steps.  On the conv fallback kernels the maps are masked to zero past the width by a pass of their own
// (ragged_mask_kernel).
#pragma once
#include "infer_workspace.h"

namespace {

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
    if (bad) __hip_atomic_fetch_or(status, SIR_STATUS_RAGGED_LENGTH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
