// Embeddings and the prototype head (include/sir_hip.h: sir_proto_state_bytes, sir_proto_reset, sir_proto_accumulate,
// sir_proto_finalize, sir_proto_score; DESIGN.md section 4 "Embeddings and the prototype head").
//
// An embedding is the 512-float attention-pooled context of an utterance (sir_model_embed).  Everything here reads a 512-float row
// the same way: ONE WAVE OWNS A ROW, lane l holds its elements 8 l .. 8 l + 7 (two 16-byte loads).  A row's sum of squares is
// formed in double -- the lane's eight squares in element order, then the xor butterfly over the 64 lanes (32, 16, ... 1: every
// lane ends with the same bits) -- so it depends on nothing but the row, and so does the unit vector e / sqrt(sumsq), the quotient
// taken in double.  sir_proto_accumulate and sir_proto_score share that code (row_norm, unit_elem: unit_rows.h).
//
// The bank (caller-owned device state): a 64-byte header {int32 n_classes, int32 0, int64 skipped}, int64 count[P], double
// sum[P][512].  sir_proto_accumulate runs one wave per CLASS: the wave walks the labels of the batch in row order (64 labels per
// load, a ballot, the set bits in ascending order) and adds the unit vectors of its own rows to its own sum -- a sequential chain
// in row order per class, no floating atomic -- so the state after a set of rows does not depend on how the rows were cut into
// calls.  The skipped rows are counted by a second launch, one wave per row, with an integer atomic.
//
// sir_proto_score: a workgroup of sixteen waves owns R batch rows (4, 2 or 1: the most that still gives every CU a workgroup)
// and ALL prototypes.  Every wave holds the R unit vectors in registers (8 VGPRs each) and takes prototypes w, w + 16, ...: two
// 16-byte loads per lane fetch the prototype's row coalesced, the lane forms its 8-term partial of each of the R dot products
// (fma chain in element order), and the R x 64 partials are reduced by a transposing butterfly -- R = 4: after the xor-32 step a
// lane keeps two of the four sums, after xor-16 one, then xor 8, 4, 2, 1: 7 cross-lane moves per prototype instead of 24 --
// whose tree is the same for every sum and every R.  A dot product is therefore a function of the two rows alone: the same
// bits whatever the row's position in the batch, the batch size, R or the wave that took the prototype (sixteen waves share the prototypes; four prototype rows per wave are in flight).  The
// similarities of the R rows go to LDS ([R][P] floats); then wave r < R finishes row r: class maxima by integer atomic max in LDS on the order-preserving integer image of the float (a maximum does not depend on the
// order it is taken in), k rank scans over the classes as in slots_decode.hip (the best class strictly after the previous
// winner in the order: descending score, ascending class), the softmax denominator over the present classes summed in double in
// a fixed lane-strided order, and the nearest prototype.  fp32 FMAs were chosen over the f16x3 matrix-core split: at one pass
// over the prototypes per workgroup the FMAs are a minority of the instructions beside the loads and the butterfly (DESIGN.md
// section 4 has the measurements).
#include <cmath>
#include <climits>
#include "sir_internal.h"
#include "row_softmax.h"   // kMaxRows
#include "unit_rows.h"     // kDim, kMaxProtos, load_row8, row_norm, unit_elem, wave_sum_f64
#include "wave_fft.h"      // wave_fence

namespace {

constexpr int kHeaderBytes = 64;
constexpr int kScoreWaves = 16;                      // its waves: at the largest bank one workgroup fills a CU's LDS, and the loads
constexpr int kScoreDepth = 4;                       // in flight are all that hides the latency: 16 waves x 4 prototype rows = 128 KB
constexpr int kScoreThreads = kScoreWaves * SIR_WAVE;
constexpr int kSkipWaves = 4;                        // rows (= waves) per workgroup of proto_skipped_kernel
constexpr int kNoClass = 0x7fffffff;

struct ProtoHeader { int n_classes, zero; long long skipped; };

inline size_t state_bytes_of(int P) { return (size_t)kHeaderBytes + (size_t)P * 8 + (size_t)P * kDim * 8; }
__host__ __device__ inline long long* state_count(void* state) { return (long long*)((char*)state + kHeaderBytes); }
__host__ __device__ inline double* state_sum(void* state, int P) { return (double*)((char*)state + kHeaderBytes + (size_t)P * 8); }

// ---- the bank -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void proto_reset_kernel(void* state, int P, const uint8_t* __restrict__ mask) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ProtoHeader* hd = (ProtoHeader*)state;
        hd->n_classes = P;
        hd->zero = 0;
        if (!mask) hd->skipped = 0;
    }
    long long* count = state_count(state);
    double* sum = state_sum(state, P);
    for (int p = blockIdx.x; p < P; p += gridDim.x) {                                    // workgroup-uniform
        if (mask && !mask[p]) continue;
        if (threadIdx.x == 0) count[p] = 0;
        for (int c = threadIdx.x; c < kDim; c += blockDim.x) sum[(size_t)p * kDim + c] = 0.0;
    }
}

// one wave per class: its rows in ascending order, one sequential chain per sum element
__global__ __launch_bounds__(SIR_WAVE) void proto_accumulate_kernel(void* state, int P, const float* __restrict__ emb,
                                                                     const long long* __restrict__ labels, int B) {
    const int p = blockIdx.x, lane = threadIdx.x;
    double* sum = state_sum(state, P) + (size_t)p * kDim + 8 * lane;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long n = 0;
    bool loaded = false;
    for (int b0 = 0; b0 < B; b0 += SIR_WAVE) {
        const int b = b0 + lane;
        unsigned long long mine = __ballot(b < B && labels[b] == (long long)p);
        while (mine) {                                                                   // wave-uniform
            const int row = b0 + __ffsll((long long)mine) - 1;
            mine &= mine - 1;
            float e[8];
            load_row8(emb + (size_t)row * kDim, lane, e);
            double norm;
            if (!row_norm(e, norm)) continue;
            if (!loaded) {
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = sum[i];
                loaded = true;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += unit_elem(e[i], norm);
            ++n;
        }
    }
    if (loaded) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sum[i] = acc[i];
        if (lane == 0) state_count(state)[p] += n;
    }
}

// one wave per row: the rows sir_proto_accumulate leaves out
__global__ __launch_bounds__(kSkipWaves * SIR_WAVE) void proto_skipped_kernel(void* state, int P, const float* __restrict__ emb,
                                                                         const long long* __restrict__ labels, int B) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    unsigned long long n = 0;
    for (int b = blockIdx.x * kSkipWaves + wave; b < B; b += gridDim.x * kSkipWaves) {   // wave-uniform
        const long long l = labels[b];
        bool skip = l < 0 || l >= (long long)P;
        if (!skip) {
            float e[8];
            load_row8(emb + (size_t)b * kDim, lane, e);
            double norm;
            skip = !row_norm(e, norm);
        }
        n += skip ? 1 : 0;
    }
    if (lane == 0 && n) atomicAdd((unsigned long long*)&((ProtoHeader*)state)->skipped, n);
}

// one wave per class: protos[p] = fp32(sum[p] / ||sum[p]||) in double; an empty class, a zero or a non-finite sum: zeros, live 0
__global__ __launch_bounds__(SIR_WAVE) void proto_finalize_kernel(void* state, int P, float* __restrict__ protos, uint8_t* __restrict__ live) {
#pragma clang fp contract(off)
    const int p = blockIdx.x, lane = threadIdx.x;
    const double* sum = state_sum(state, P) + (size_t)p * kDim + 8 * lane;
    double v[8], ss = 0.0;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = sum[i];
        bad = bad || (__double2hiint(v[i]) & 0x7ff00000) == 0x7ff00000;
        ss += v[i] * v[i];
    }
    ss = wave_sum_f64(ss);
    const double norm = sqrt(ss);
    const bool ok = state_count(state)[p] > 0 && __ballot(bad) == 0ull && ss > 0.0 && (__double2hiint(norm) & 0x7ff00000) != 0x7ff00000;
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = ok ? (float)(v[i] / norm) : 0.0f;
    float4* out = reinterpret_cast<float4*>(protos + (size_t)p * kDim) + 2 * lane;
    out[0] = make_float4(o[0], o[1], o[2], o[3]);
    out[1] = make_float4(o[4], o[5], o[6], o[7]);
    if (lane == 0) live[p] = ok ? 1 : 0;
}

// ---- scoring ---------------------------------------------------------------------------------------------------------------
// the order-preserving integer image of a float (no NaN comes here): a < b as floats => ord(a) < ord(b); -0.0 sits just below +0.0
__device__ __forceinline__ int float_ord(float x) { const int i = __float_as_int(x); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float ord_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }
constexpr int kAbsent = INT_MIN;                     // no live prototype of the class (float_ord never returns it: it is -NaN's image)

// the better of two (score, class) pairs: larger score, then lower class; kNoClass = no candidate
__device__ __forceinline__ void keep_better_class(float& s, int& c, float s2, int c2) {
    const bool take = c2 != kNoClass && (c == kNoClass || s2 > s || (s2 == s && c2 < c));
    if (take) { s = s2; c = c2; }
}

struct ScoreOut {
    float* sims;           // [B][P] or NULL
    int* topk_class;       // [B][k]
    float* topk_sim;       // [B][k]
    float* topk_prob;      // [B][k]
    int* nearest;          // [B] or NULL
};

__host__ __device__ inline size_t score_lds_bytes(int rows, int P, int NC) { return ((size_t)rows * P + P + (size_t)rows * NC) * 4; }

// The transposing butterfly over the wave: R sums per lane in, sum r out in the lanes with lane / (64 / R) == r.  While more than
// one sum is left a step keeps half of them (the lower half in the lanes whose bit is clear) and sends the other half across;
// every sum goes through the same tree -- lanes paired at distance 32, 16, 8, 4, 2, 1 -- so its bits do not depend on R or r.
template <int R>
__device__ __forceinline__ float transpose_sum(const float (&v)[R], int lane) {
    static_assert(R == 1 || R == 2 || R == 4, "rows per workgroup");
    float c;
    if constexpr (R == 4) {
        const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
        float a0 = hi32 ? v[2] : v[0], a1 = hi32 ? v[3] : v[1];
        const float g0 = hi32 ? v[0] : v[2], g1 = hi32 ? v[1] : v[3];
        a0 += __shfl_xor(g0, 32);
        a1 += __shfl_xor(g1, 32);
        c = hi16 ? a1 : a0;
        const float g = hi16 ? a0 : a1;
        c += __shfl_xor(g, 16);
    } else if constexpr (R == 2) {
        const bool hi32 = (lane & 32) != 0;
        c = hi32 ? v[1] : v[0];
        const float g = hi32 ? v[0] : v[1];
        c += __shfl_xor(g, 32);
        c += __shfl_xor(c, 16);
    } else {
        c = v[0];
        c += __shfl_xor(c, 32);
        c += __shfl_xor(c, 16);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) c += __shfl_xor(c, off);
    return c;
}

// kRows batch rows per workgroup.  The host picks the largest of 4, 2, 1 that still gives every CU a workgroup: four rows share
// one pass over the prototypes and one butterfly, but a batch of 256 in groups of four would leave three CUs in four idle.
template <int kRows>
__global__ __launch_bounds__(kScoreThreads) void proto_score_kernel(const float* __restrict__ emb, int B, const float* __restrict__ protos,
                                                                       const uint8_t* __restrict__ live, const int* __restrict__ pclass,
                                                                       int P, int NC, const float* __restrict__ scale, int k, ScoreOut o) {
    extern __shared__ float s_proto[];
    float* s_sim = s_proto;                                                              // [kRows][P]
    int* s_cls = reinterpret_cast<int*>(s_proto + (size_t)kRows * P);                    // [P]: the prototype's class, -1: takes no part
    int* s_max = s_cls + P;                                                              // [kRows][NC]: float_ord of the class maximum
    const int tid = threadIdx.x, lane = tid & (SIR_WAVE - 1), wave = tid / SIR_WAVE;
    const int b0 = blockIdx.x * kRows;

    for (int p = tid; p < P; p += kScoreThreads) {
        int c = pclass ? pclass[p] : p;
        if (c < 0 || c >= NC || (live && !live[p])) c = -1;
        s_cls[p] = c;
    }
    for (int i = tid; i < kRows * NC; i += kScoreThreads) s_max[i] = kAbsent;

    // the kRows unit vectors, in every wave's registers (rows past the batch: zeros, never stored)
    float u[kRows][8];
    bool ok[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        float e[8];
        const bool in = b0 + r < B;                                                      // wave-uniform
        if (in) load_row8(emb + (size_t)(b0 + r) * kDim, lane, e);
        else {
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = 0.0f;
        }
        double norm;
        ok[r] = row_norm(e, norm);
#pragma unroll
        for (int i = 0; i < 8; ++i) u[r][i] = ok[r] ? (float)unit_elem(e[i], norm) : 0.0f;
    }

    // similarities: wave w takes prototypes w, w + kScoreWaves, ..., kScoreDepth of them per round with all their loads issued first
    constexpr int kLanesPerRow = SIR_WAVE / kRows;
    for (int p0 = wave; p0 < P; p0 += kScoreDepth * kScoreWaves) {                       // wave-uniform
        float q[kScoreDepth][8];
#pragma unroll
        for (int j = 0; j < kScoreDepth; ++j) {
            const int pj = p0 + j * kScoreWaves;
            load_row8(protos + (size_t)(pj < P ? pj : P - 1) * kDim, lane, q[j]);        // (past the end: the last row again, not stored)
        }
#pragma unroll
        for (int j = 0; j < kScoreDepth; ++j) {
            const int p = p0 + j * kScoreWaves;
            float v[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                float acc = u[r][0] * q[j][0];
#pragma unroll
                for (int i = 1; i < 8; ++i) acc = fmaf(u[r][i], q[j][i], acc);
                v[r] = acc;
            }
            const float c = transpose_sum<kRows>(v, lane);
            if ((lane & (kLanesPerRow - 1)) == 0 && p < P) s_sim[(size_t)(lane / kLanesPerRow) * P + p] = c;
        }
    }
    __syncthreads();

    // wave r < kRows finishes row r (no barrier below: a wave touches only its own slabs of s_sim and s_max)
    const int r = wave, b = b0 + r;
    if (r >= kRows || b >= B) return;
    bool row_ok = false;
#pragma unroll
    for (int j = 0; j < kRows; ++j) row_ok = j == r ? ok[j] : row_ok;
    const float nan = __builtin_nanf("");
    if (!row_ok) {
        if (o.sims)
            for (int p = lane; p < P; p += SIR_WAVE) o.sims[(size_t)b * P + p] = nan;
        if (lane < k) { o.topk_class[(size_t)b * k + lane] = -1; o.topk_sim[(size_t)b * k + lane] = nan; o.topk_prob[(size_t)b * k + lane] = nan; }
        if (o.nearest && lane == 0) o.nearest[b] = -1;
        return;
    }
    const float* sim = s_sim + (size_t)r * P;
    int* cmax = s_max + (size_t)r * NC;
    for (int p = lane; p < P; p += SIR_WAVE) {
        const float s = sim[p];
        if (o.sims) o.sims[(size_t)b * P + p] = s;
        const int c = s_cls[p];
        if (c >= 0 && s == s) atomicMax(&cmax[c], float_ord(s));                         // (a NaN prototype takes no part)
    }
    wave_fence();

    const float beta = scale ? scale[0] : 1.0f;
    float best_s = 0.0f, top_s = 0.0f;
    int best_c = kNoClass, top_c = kNoClass;
    double den = 0.0;
    for (int rank = 0; rank < k; ++rank) {                                               // wave-uniform
        if (rank == 0 || best_c != kNoClass) {
            const float ps = best_s;
            const int pc = best_c;
            best_c = kNoClass;
            for (int c = lane; c < NC; c += SIR_WAVE) {
                const int m = cmax[c];
                if (m == kAbsent) continue;
                const float s = ord_float(m);
                if (rank == 0 || s < ps || (s == ps && c > pc)) keep_better_class(best_s, best_c, s, c);   // ascending c: a tie keeps the lower class
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) keep_better_class(best_s, best_c, __shfl_xor(best_s, off), __shfl_xor(best_c, off));
            best_s = __shfl(best_s, 0);
            best_c = __shfl(best_c, 0);
        }
        if (rank == 0) {
            top_s = best_s;
            top_c = best_c;
            if (top_c != kNoClass) {
                // softmax of beta * s over the present classes: d = (s - max s) * beta as row_softmax forms it, the sum in double,
                // lane-strided in class order then the butterfly
                double part = 0.0;
                for (int c = lane; c < NC; c += SIR_WAVE) {
                    const int m = cmax[c];
                    if (m != kAbsent) part += (double)expf((ord_float(m) - top_s) * beta);
                }
                den = wave_sum_f64(part);
            }
        }
        if (lane == 0) {
            const size_t at = (size_t)b * k + rank;
            if (best_c == kNoClass) { o.topk_class[at] = -1; o.topk_sim[at] = 0.0f; o.topk_prob[at] = 0.0f; }
            else {
                o.topk_class[at] = best_c;
                o.topk_sim[at] = best_s;
                o.topk_prob[at] = (float)((double)expf((best_s - top_s) * beta) / den);
            }
        }
    }
    if (o.nearest) {                                                                     // the first prototype of the rank-0 class at its score
        int np = kNoClass;
        if (top_c != kNoClass)
            for (int p = lane; p < P; p += SIR_WAVE)
                if (np == kNoClass && s_cls[p] == top_c && sim[p] == top_s) np = p;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const int n2 = __shfl_xor(np, off); np = n2 < np ? n2 : np; }
        if (lane == 0) o.nearest[b] = np == kNoClass ? -1 : np;
    }
}

// the header on the host: accumulate / finalize / a masked reset refuse a state that sir_proto_reset did not lay out for n_classes
int header_ok(const char* who, const void* state, int n_classes, hipStream_t st) {
    ProtoHeader hd;
    SIR_HIP_TRY(hipMemcpyAsync(&hd, state, sizeof(hd), hipMemcpyDeviceToHost, st));
    SIR_HIP_TRY(hipStreamSynchronize(st));
    if (hd.n_classes != n_classes) {
        sir_set_error("%s: the state's header holds n_classes=%d, the call says %d (sir_proto_reset lays a state out)", who, hd.n_classes, n_classes);
        return SIR_EINVAL;
    }
    return SIR_OK;
}

int state_args_ok(const char* who, const sir_handle* h, const void* state, size_t state_bytes, int n_classes) {
    if (!h || !state) { sir_set_error("%s: NULL argument (h and state are required)", who); return SIR_EINVAL; }
    if (n_classes < 1 || n_classes > kMaxProtos) { sir_set_error("%s: n_classes=%d outside [1, %d]", who, n_classes, kMaxProtos); return SIR_EINVAL; }
    if ((uintptr_t)state & 15u) { sir_set_error("%s: the state must be 16-byte aligned", who); return SIR_EINVAL; }
    const size_t need = state_bytes_of(n_classes);
    if (state_bytes < need) { sir_set_error("%s: state of %zu bytes, %zu needed", who, state_bytes, need); return SIR_EINVAL; }
    return SIR_OK;
}

}  // namespace

extern "C" size_t sir_proto_state_bytes(int n_classes) {
    return n_classes < 1 || n_classes > kMaxProtos ? 0 : state_bytes_of(n_classes);
}

extern "C" int sir_proto_reset(sir_handle* h, void* state, size_t state_bytes, int n_classes, const uint8_t* mask, void* stream) {
    const char* who = "sir_proto_reset";
    SIR_TRY(state_args_ok(who, h, state, state_bytes, n_classes));
    if (mask) SIR_TRY(header_ok(who, state, n_classes, (hipStream_t)stream));
    hipLaunchKernelGGL(proto_reset_kernel, dim3(n_classes < 1024 ? n_classes : 1024), dim3(256), 0, (hipStream_t)stream, state, n_classes, mask);
    return sir_check_hip(hipGetLastError(), "sir_proto_reset kernel");
}

extern "C" int sir_proto_accumulate(sir_handle* h, void* state, size_t state_bytes, int n_classes, const float* emb, const int64_t* labels,
                                    int batch, void* stream) {
    const char* who = "sir_proto_accumulate";
    SIR_TRY(state_args_ok(who, h, state, state_bytes, n_classes));
    if (!emb || !labels) { sir_set_error("%s: NULL argument (emb and labels are required)", who); return SIR_EINVAL; }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: batch=%d outside [1, 2^30]", who, batch); return SIR_EINVAL; }
    if (((uintptr_t)emb & 15u) || ((uintptr_t)labels & 7u)) { sir_set_error("%s: emb must be 16-byte aligned, labels 8-byte aligned", who); return SIR_EINVAL; }
    SIR_TRY(header_ok(who, state, n_classes, (hipStream_t)stream));
    hipLaunchKernelGGL(proto_accumulate_kernel, dim3(n_classes), dim3(SIR_WAVE), 0, (hipStream_t)stream, state, n_classes, emb,
                       (const long long*)labels, batch);
    const int rows_blocks = (batch + kSkipWaves - 1) / kSkipWaves;
    hipLaunchKernelGGL(proto_skipped_kernel, dim3(rows_blocks < 4096 ? rows_blocks : 4096), dim3(kSkipWaves * SIR_WAVE), 0, (hipStream_t)stream, state,
                       n_classes, emb, (const long long*)labels, batch);
    return sir_check_hip(hipGetLastError(), "sir_proto_accumulate kernels");
}

extern "C" int sir_proto_finalize(sir_handle* h, void* state, size_t state_bytes, int n_classes, float* protos, uint8_t* live, void* stream) {
    const char* who = "sir_proto_finalize";
    SIR_TRY(state_args_ok(who, h, state, state_bytes, n_classes));
    if (!protos || !live) { sir_set_error("%s: NULL argument (protos and live are required)", who); return SIR_EINVAL; }
    if ((uintptr_t)protos & 15u) { sir_set_error("%s: protos must be 16-byte aligned", who); return SIR_EINVAL; }
    SIR_TRY(header_ok(who, state, n_classes, (hipStream_t)stream));
    hipLaunchKernelGGL(proto_finalize_kernel, dim3(n_classes), dim3(SIR_WAVE), 0, (hipStream_t)stream, state, n_classes, protos, live);
    return sir_check_hip(hipGetLastError(), "sir_proto_finalize kernel");
}

extern "C" int sir_proto_score(sir_handle* h, const float* emb, int batch, const float* protos, const uint8_t* live, const int32_t* proto_class,
                               int n_protos, int n_classes, const float* scale, int k, float* sims, int32_t* topk_class, float* topk_sim,
                               float* topk_prob, int32_t* nearest, void* stream) {
    const char* who = "sir_proto_score";
    if (!h || !emb || !protos || !topk_class || !topk_sim || !topk_prob) {
        sir_set_error("%s: NULL argument (h, emb, protos, topk_class, topk_sim and topk_prob are required)", who);
        return SIR_EINVAL;
    }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: batch=%d outside [1, 2^30]", who, batch); return SIR_EINVAL; }
    if (n_protos < 1 || n_protos > kMaxProtos) { sir_set_error("%s: n_protos=%d outside [1, %d]", who, n_protos, kMaxProtos); return SIR_EINVAL; }
    if (n_classes < 1 || n_classes > n_protos) { sir_set_error("%s: n_classes=%d outside [1, n_protos=%d]", who, n_classes, n_protos); return SIR_EINVAL; }
    if (!proto_class && n_classes != n_protos) {
        sir_set_error("%s: without proto_class a prototype's class is its row: n_classes=%d must equal n_protos=%d", who, n_classes, n_protos);
        return SIR_EINVAL;
    }
    if (k < 1 || k > 8) { sir_set_error("%s: k=%d outside [1, 8]", who, k); return SIR_EINVAL; }
    if (((uintptr_t)emb | (uintptr_t)protos) & 15u) { sir_set_error("%s: emb and protos must be 16-byte aligned", who); return SIR_EINVAL; }
    const uintptr_t bits = (uintptr_t)proto_class | (uintptr_t)scale | (uintptr_t)sims | (uintptr_t)topk_class | (uintptr_t)topk_sim |
                           (uintptr_t)topk_prob | (uintptr_t)nearest;
    if (bits & 3u) { sir_set_error("%s: pointers must be 4-byte aligned", who); return SIR_EINVAL; }
    const ScoreOut o{sims, (int*)topk_class, topk_sim, topk_prob, (int*)nearest};
    // rows per workgroup: the most that still leaves no CU without a workgroup (the results do not depend on it)
    const int cus = h->num_cus > 0 ? h->num_cus : 256;
    const int rows = (batch + 3) / 4 >= cus ? 4 : (batch + 1) / 2 >= cus ? 2 : 1;
    const dim3 grid((batch + rows - 1) / rows), block(kScoreThreads);
    const size_t lds = score_lds_bytes(rows, n_protos, n_classes);
    const int lds_max = (int)score_lds_bytes(rows, kMaxProtos, kMaxProtos);
    const int* pclass = (const int*)proto_class;
    if (rows == 4) {
        SIR_TRY(sir_lds_opt_in(h, (const void*)proto_score_kernel<4>, lds_max));
        hipLaunchKernelGGL(proto_score_kernel<4>, grid, block, lds, (hipStream_t)stream, emb, batch, protos, live, pclass, n_protos, n_classes, scale, k, o);
    } else if (rows == 2) {
        SIR_TRY(sir_lds_opt_in(h, (const void*)proto_score_kernel<2>, lds_max));
        hipLaunchKernelGGL(proto_score_kernel<2>, grid, block, lds, (hipStream_t)stream, emb, batch, protos, live, pclass, n_protos, n_classes, scale, k, o);
    } else {
        SIR_TRY(sir_lds_opt_in(h, (const void*)proto_score_kernel<1>, lds_max));
        hipLaunchKernelGGL(proto_score_kernel<1>, grid, block, lds, (hipStream_t)stream, emb, batch, protos, live, pclass, n_protos, n_classes, scale, k, o);
    }
    return sir_check_hip(hipGetLastError(), "sir_proto_score kernel");
}
