// The ascent / projection step of an L-infinity adversary on a feature batch (include/sir_hip.h: sir_adv_step).
//
// One launch, grid (column tiles of 64 frames, batch).  A workgroup of 256 threads owns ALL n_mels rows of its column tile, so
// "is this frame column of x0 all +0.0" is decided on chip: every thread keeps its x0 values in registers, ORs their bit patterns
// per column, the row groups combine through 1 KB of LDS, and the same registers then feed the step -- x0 is read from HBM once.
// Three reads (x0, x, g) and one write per element; nothing else touches memory.
//   16-byte form (t % 4 == 0, every pointer 16-byte aligned): a thread owns 4 consecutive frames of 4 rows (16 column quads x
//       16 row groups; a wave reads 4 rows x 256 contiguous bytes per instruction);
//   element form (any t >= 1): a thread owns 1 frame of 16 rows (64 columns x 4 row groups; a wave reads one 256-byte row segment).
// Values travel as bit patterns: a kept element is a select between two 32-bit words, never an arithmetic result, so -0.0 and
// NaN payloads of x0 survive.  Every arithmetic step is its own fp32 rounding (add_rn / sub_rn / mul_rn below: no contraction).
#include "sir_internal.h"

// One rounding per operation.  The HIP headers define __fadd_rn / __fsub_rn / __fmul_rn as plain operators that carry the
// translation unit's default contraction permission, so after inlining hipcc still fuses __fadd_rn(x0, __fmul_rn(eps, r)) into one
// v_fma_f32 (seen in the assembly: the random start was ONE rounding).  The operators below are compiled with contraction off,
// which the default -ffp-contract=fast-honor-pragmas honours; the kernel's assembly holds no fma.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }

constexpr int kAdvThreads = 256;
constexpr int kAdvCols = 64;             // frames per column tile

// the 24-bit uniform of train_fwd_kernels.h dropout_keep: hash of (seed, element index), >> 40, * 2^-24
__device__ __forceinline__ float adv_uniform(unsigned long long seed, size_t idx) {
    unsigned long long x = seed ^ (idx * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (float)(unsigned)(x >> 40) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ float adv_project(float y, float x0, float eps) {
    const float lo = sub_rn(x0, eps), hi = add_rn(x0, eps);
    return fminf(fmaxf(y, lo), hi);
}

template <int V>
__device__ __forceinline__ void adv_load(const unsigned int* p, unsigned int (&v)[V]) {
    if constexpr (V == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = *p;
    }
}

template <int V>
__device__ __forceinline__ void adv_store(unsigned int* p, const unsigned int (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}

// x and out may be the same buffer (in-place iterate): a thread reads its own elements of x before it writes them, and no other
// thread touches them -- hence no __restrict__ on those two.
template <int V>
__global__ __launch_bounds__(kAdvThreads) void adv_step_kernel(const unsigned int* __restrict__ x0, const unsigned int* x,
                                                               const unsigned int* __restrict__ g, const int* __restrict__ active,
                                                               int batch, int n_mels, int t, float eps, float alpha, int keep_zero,
                                                               unsigned long long seed, unsigned int* out) {
    constexpr int CG = kAdvCols / V;            // column groups of a tile (V frames each)
    constexpr int RG = kAdvThreads / CG;        // row groups
    constexpr int ROWS = SIR_MAX_MELS / RG;     // rows of one thread: rg, rg + RG, ...
    __shared__ unsigned int col_or[RG][kAdvCols];
    const int cg = threadIdx.x % CG, rg = threadIdx.x / CG;
    const int j0 = blockIdx.x * kAdvCols + cg * V;
    const bool in_t = j0 < t;                   // (16-byte form: t % 4 == 0, so j0 < t covers j0 + 3)
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const bool live = active == nullptr || active[b] != 0;          // workgroup-uniform
        const size_t row0 = (size_t)b * n_mels;
        unsigned int a[ROWS][V];
        unsigned int seen[V];
#pragma unroll
        for (int e = 0; e < V; ++e) seen[e] = 0u;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int m = rg + k * RG;
#pragma unroll
            for (int e = 0; e < V; ++e) a[k][e] = 0u;
            if (in_t && m < n_mels) adv_load<V>(x0 + (row0 + m) * t + j0, a[k]);
#pragma unroll
            for (int e = 0; e < V; ++e) seen[e] |= a[k][e];
        }
        bool kept[V];
#pragma unroll
        for (int e = 0; e < V; ++e) kept[e] = false;
        if (keep_zero && live) {                                         // workgroup-uniform: both barriers are reached by all
#pragma unroll
            for (int e = 0; e < V; ++e) col_or[rg][cg * V + e] = seen[e];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < V; ++e) {
                unsigned int o = 0u;
#pragma unroll
                for (int r = 0; r < RG; ++r) o |= col_or[r][cg * V + e];
                kept[e] = o == 0u;                                       // every row holds bit pattern 0 (+0.0; -0.0 is data)
            }
            __syncthreads();                                             // before the next row of the batch overwrites col_or
        }
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const int m = rg + k * RG;
            if (!(in_t && m < n_mels)) continue;
            const size_t at = (row0 + m) * t + j0;
            unsigned int res[V];
            if (!live) {
#pragma unroll
                for (int e = 0; e < V; ++e) res[e] = a[k][e];
            } else if (g != nullptr) {
                unsigned int xv[V], gv[V];
                adv_load<V>(x + at, xv);
                adv_load<V>(g + at, gv);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float gf = __uint_as_float(gv[e]);
                    const float step = gf > 0.0f ? alpha : (gf < 0.0f ? -alpha : 0.0f);   // a NaN gradient compares false twice: 0
                    const float y = add_rn(__uint_as_float(xv[e]), step);
                    const float r = adv_project(y, __uint_as_float(a[k][e]), eps);
                    res[e] = kept[e] ? a[k][e] : __float_as_uint(r);
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float u = adv_uniform(seed, at + e);
                    const float r = sub_rn(mul_rn(2.0f, u), 1.0f);                  // exact: u is a multiple of 2^-24 in [0, 1)
                    const float x0f = __uint_as_float(a[k][e]);
                    const float y = add_rn(x0f, mul_rn(eps, r));
                    res[e] = kept[e] ? a[k][e] : __float_as_uint(adv_project(y, x0f, eps));
                }
            }
            adv_store<V>(out + at, res);
        }
    }
}

// [p, p + bytes) and [q, q + bytes) share a byte
bool adv_overlap(const void* p, const void* q, size_t bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" int sir_adv_step(sir_handle* h, const float* x0, const float* x, const float* g, const int32_t* active,
                            int batch, int n_mels, int t, const sir_adv_config* cfg, uint64_t start_seed,
                            float* out, void* stream) {
    if (!h || !x0 || !out || !cfg) { sir_set_error("sir_adv_step: NULL argument (h, x0, out and cfg are required)"); return SIR_EINVAL; }
    if (batch < 1 || t < 1 || n_mels < 1 || n_mels > SIR_MAX_MELS) {
        sir_set_error("sir_adv_step: bad sizes (batch %d, n_mels %d, t %d: batch and t >= 1, n_mels in [1, %d])", batch, n_mels, t, SIR_MAX_MELS);
        return SIR_EINVAL;
    }
    if (!(cfg->eps >= 0.0f)) { sir_set_error("sir_adv_step: eps must be >= 0 and not NaN"); return SIR_EINVAL; }
    if (g == nullptr && x != nullptr) { sir_set_error("sir_adv_step: x given without g (a random start is drawn around x0 alone)"); return SIR_EINVAL; }
    if (g != nullptr) {
        if (x == nullptr) { sir_set_error("sir_adv_step: a gradient step needs the iterate x (pass x0 for the first step)"); return SIR_EINVAL; }
        if (!(cfg->alpha >= 0.0f)) { sir_set_error("sir_adv_step: alpha must be >= 0 and not NaN"); return SIR_EINVAL; }
    }
    const size_t bytes = (size_t)batch * n_mels * t * sizeof(float);
    if (adv_overlap(out, x0, bytes) || (g && adv_overlap(out, g, bytes)) || (x && out != x && adv_overlap(out, x, bytes))) {
        sir_set_error("sir_adv_step: out must not alias x0 or g, and may alias x only as the same buffer (in place)");
        return SIR_EINVAL;
    }
    const uintptr_t bits = (uintptr_t)x0 | (uintptr_t)x | (uintptr_t)g | (uintptr_t)out;
    if ((bits & 3u) || (((uintptr_t)active) & 3u)) { sir_set_error("sir_adv_step: pointers must be 4-byte aligned"); return SIR_EINVAL; }
    const dim3 grid((unsigned)((t + kAdvCols - 1) / kAdvCols), (unsigned)(batch < 65535 ? batch : 65535));
    const unsigned int* x0u = reinterpret_cast<const unsigned int*>(x0);
    const unsigned int* xu = reinterpret_cast<const unsigned int*>(x);
    const unsigned int* gu = reinterpret_cast<const unsigned int*>(g);
    unsigned int* outu = reinterpret_cast<unsigned int*>(out);
    if ((t & 3) == 0 && (bits & 15u) == 0)
        hipLaunchKernelGGL(adv_step_kernel<4>, grid, dim3(kAdvThreads), 0, (hipStream_t)stream, x0u, xu, gu, (const int*)active, batch, n_mels, t,
                           cfg->eps, cfg->alpha, cfg->keep_zero_columns, (unsigned long long)start_seed, outu);
    else
        hipLaunchKernelGGL(adv_step_kernel<1>, grid, dim3(kAdvThreads), 0, (hipStream_t)stream, x0u, xu, gu, (const int*)active, batch, n_mels, t,
                           cfg->eps, cfg->alpha, cfg->keep_zero_columns, (unsigned long long)start_seed, outu);
    return sir_check_hip(hipGetLastError(), "adv_step_kernel");
}
