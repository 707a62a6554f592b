// The cosine-proxy (normalised-softmax, AM-softmax / CosFace-style) loss on the utterance embeddings and its gradients
// (include/sir_hip.h: sir_proxy_loss_workspace_bytes, sir_proxy_loss; DESIGN.md section 4 "Training the embedding").
//
//   u_b = e_b / ||e_b||, q_k = p_k / ||p_k||  (norms and quotients in double: unit_rows.h, the code of the prototype head)
//   z_bk = scale (<u_b, q_k> - margin [k = y_b]);  loss = mean over the rows with a label of -log softmax(z_b)[y_b]
//   dz = (softmax - onehot) grad_scale / n_valid
//   du_b = scale sum_k dz_bk q_k,  demb_b = (du_b - <du_b, u_b> u_b) / ||e_b||
//   dq_k = scale sum_b dz_bk u_b,  dproxies_k = (dq_k - <dq_k, q_k> q_k) / ||p_k||
//
// Four launches, only kernels, nothing allocates, no floating atomic, every sum in a fixed order:
//   proxy_unit_kernel   one wave per row of emb and of proxies: the fp32 unit vector and the double norm into the workspace; one
//                       more workgroup counts the rows with a label (integers: no order to fix).
//   proxy_row_kernel    one workgroup of eight waves per batch row.  Every wave holds u_b (8 VGPRs) and takes proxies w, w + 8, ...:
//                       the similarity is proto_score_kernel's -- the lane's 8-term fma chain in element order, then the xor
//                       butterfly 32 .. 1 -- so it carries that kernel's bits.  The logits go to LDS; the softmax denominator is
//                       summed in double (thread-strided in class order, the butterfly, the eight waves in order); dz goes to LDS
//                       and to the workspace; a second pass over the proxies adds dz_bk q_k per wave in ascending k, the eight
//                       waves' partials are added in wave order, and wave 0 projects in double.
//   proxy_col_kernel    one wave per proxy: its column of dz (64 rows per load, broadcast lane by lane) times the unit rows, ONE chain
//                       in ascending row order as proto_accumulate_kernel's, then the projection in double.  A zero dz adds nothing
//                       and is selected away, so that an ignored row's embedding (a NaN, say) cannot travel.
//   proxy_reduce_kernel the row losses added in double in a fixed tree, divided by n_valid (none: 0 / 0 = NaN, as sir_ce_loss).
// A row's dz, loss and demb depend on the row, the proxies and n_valid alone: the same bits at any position and batch size.
// fp32 FMAs, not the f16x3 matrix-core split, for the reason DESIGN.md gives for sir_proto_score.
#include <cmath>
#include "sir_internal.h"
#include "row_softmax.h"   // kMaxRows
#include "unit_rows.h"     // kDim, kMaxProtos, load_row8, row_norm, unit_elem, wave_sum_f64

namespace {

constexpr int kUnitWaves = 4;                        // rows (= waves) per workgroup of proxy_unit_kernel and proxy_col_kernel
constexpr int kRowWaves = 8;
constexpr int kRowThreads = kRowWaves * SIR_WAVE;
constexpr int kRowDepth = 4;                         // proxy rows in flight per wave
constexpr size_t kAlign = 256;

struct ProxyWs {
    int* nvalid;           // [1] (+ padding)
    double* enorm;         // [B]
    double* pnorm;         // [P]
    float* row_loss;       // [B]
    float* U;              // [B][512]
    float* Q;              // [P][512]
    float* dz;             // [B][P]
};

inline size_t up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
inline size_t ws_layout(int B, int P, size_t (&off)[7]) {
    size_t at = 0;
    off[0] = at; at += up(sizeof(int));
    off[1] = at; at += up((size_t)B * 8);
    off[2] = at; at += up((size_t)P * 8);
    off[3] = at; at += up((size_t)B * 4);
    off[4] = at; at += up((size_t)B * kDim * 4);
    off[5] = at; at += up((size_t)P * kDim * 4);
    off[6] = at; at += up((size_t)B * P * 4);
    return at;
}

__device__ __forceinline__ void store_row8(float* __restrict__ row, int lane, const float (&o)[8]) {
    float4* out = reinterpret_cast<float4*>(row) + 2 * lane;
    out[0] = make_float4(o[0], o[1], o[2], o[3]);
    out[1] = make_float4(o[4], o[5], o[6], o[7]);
}

// out = (d - <d, v> v) / norm: the part of d at right angles to the unit row v, in double (the lane's eight products in element
// order, then the butterfly)
__device__ __forceinline__ void project_row8(const float (&d)[8], const float (&v)[8], double norm, float (&o)[8]) {
#pragma clang fp contract(off)
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += (double)d[i] * (double)v[i];
    t = wave_sum_f64(t);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)(((double)d[i] - t * (double)v[i]) / norm);
}

// waves [0, B): rows of emb; waves [B, B + P): rows of proxies; the last workgroup: n_valid
__global__ __launch_bounds__(kUnitWaves * SIR_WAVE) void proxy_unit_kernel(const float* __restrict__ emb, const float* __restrict__ proxies,
                                                                           const long long* __restrict__ labels, int B, int P, ProxyWs ws) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ int cnt[kUnitWaves * SIR_WAVE];
        int nv = 0;
        for (int b = threadIdx.x; b < B; b += kUnitWaves * SIR_WAVE) nv += labels[b] != -100ll ? 1 : 0;
        cnt[threadIdx.x] = nv;
        __syncthreads();
        for (int o = kUnitWaves * SIR_WAVE / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) ws.nvalid[0] = cnt[0];
        return;
    }
    const long long g = (long long)blockIdx.x * kUnitWaves + wave;                       // wave-uniform
    if (g >= (long long)B + P) return;
    const bool is_emb = g < B;
    const size_t r = is_emb ? (size_t)g : (size_t)(g - B);
    float e[8], o[8];
    load_row8((is_emb ? emb : proxies) + r * kDim, lane, e);
    double norm;
    const bool ok = row_norm(e, norm);
    // (a row with a NaN or an infinity or of norm zero has no direction: NaN, which the loss then shows)
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = ok ? (float)unit_elem(e[i], norm) : nan;
    store_row8((is_emb ? ws.U : ws.Q) + r * kDim, lane, o);
    if (lane == 0) (is_emb ? ws.enorm : ws.pnorm)[r] = ok ? norm : (double)nan;
}

__global__ __launch_bounds__(kRowThreads) void proxy_row_kernel(const long long* __restrict__ labels, int B, int P, float scale, float margin,
                                                                float grad_scale, ProxyWs ws, int want_dz, float* __restrict__ demb,
                                                                unsigned int* status) {
    __shared__ float s_z[kMaxProtos];                                                    // logits, then exp, then dz
    __shared__ float s_part[kRowWaves * kDim];
    __shared__ double s_den[kRowWaves];
    __shared__ float s_mx[kRowWaves];
    const int tid = threadIdx.x, lane = tid & (SIR_WAVE - 1), wave = tid / SIR_WAVE;
    const int b = blockIdx.x;
    const long long yl = labels[b];
    const bool ignored = yl == -100ll;
    const bool bad = !ignored && (yl < 0 || yl >= (long long)P);
    if (ignored || bad) {                                                                // workgroup-uniform, before any barrier
        // -100: out of the loss, the gradients and the divisor.  Any other label outside [0, P): the loss NaN and the status bit of
        // sir_ce_loss (SIR_EINVAL at the next sir_check_status); nothing is read out of bounds and the row has no gradient.
        if (want_dz)
            for (int k = tid; k < P; k += kRowThreads) ws.dz[(size_t)b * P + k] = 0.0f;
        if (demb && tid < kDim / 4) reinterpret_cast<float4*>(demb + (size_t)b * kDim)[tid] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tid == 0) {
            ws.row_loss[b] = bad ? __builtin_nanf("") : 0.0f;
            if (bad) __hip_atomic_fetch_or(status, SIR_STATUS_CE_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    const int y = (int)yl;
    float u[8];
    load_row8(ws.U + (size_t)b * kDim, lane, u);

    // the logits: wave w takes proxies w, w + kRowWaves, ..., kRowDepth of them per round with all their loads issued first
    for (int p0 = wave; p0 < P; p0 += kRowDepth * kRowWaves) {                           // wave-uniform
        float q[kRowDepth][8];
#pragma unroll
        for (int j = 0; j < kRowDepth; ++j) {
            const int pj = p0 + j * kRowWaves;
            load_row8(ws.Q + (size_t)(pj < P ? pj : P - 1) * kDim, lane, q[j]);          // (past the end: the last row again, not stored)
        }
#pragma unroll
        for (int j = 0; j < kRowDepth; ++j) {
            const int p = p0 + j * kRowWaves;
            float acc = u[0] * q[j][0];
#pragma unroll
            for (int i = 1; i < 8; ++i) acc = fmaf(u[i], q[j][i], acc);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
            if (lane == 0 && p < P) s_z[p] = scale * (acc - (p == y ? margin : 0.0f));
        }
    }
    __syncthreads();
    const float zy = s_z[y];
    float mx = -INFINITY;
    for (int k = tid; k < P; k += kRowThreads) mx = fmaxf(mx, s_z[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) s_mx[wave] = mx;
    __syncthreads();
    mx = s_mx[0];
#pragma unroll
    for (int w = 1; w < kRowWaves; ++w) mx = fmaxf(mx, s_mx[w]);
    // the denominator in double: thread-strided in class order, the butterfly, the waves in order
    double part = 0.0;
    for (int k = tid; k < P; k += kRowThreads) {
        const float e = expf(s_z[k] - mx);
        s_z[k] = e;
        part += (double)e;
    }
    part = wave_sum_f64(part);
    if (lane == 0) s_den[wave] = part;
    __syncthreads();
    double den = s_den[0];
#pragma unroll
    for (int w = 1; w < kRowWaves; ++w) den += s_den[w];
    if (tid == 0) ws.row_loss[b] = (float)(log(den) - (double)(zy - mx));
    const float gs = grad_scale / (float)ws.nvalid[0];
    for (int k = tid; k < P; k += kRowThreads) {
        const float d = ((float)((double)s_z[k] / den) - (k == y ? 1.0f : 0.0f)) * gs;
        s_z[k] = d;
        if (want_dz) ws.dz[(size_t)b * P + k] = d;
    }
    if (!demb) return;                                                                   // workgroup-uniform
    __syncthreads();

    // du = scale sum_k dz_k q_k: per wave its proxies in ascending k, then the waves in order
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int p0 = wave; p0 < P; p0 += kRowDepth * kRowWaves) {                           // wave-uniform
        float q[kRowDepth][8];
#pragma unroll
        for (int j = 0; j < kRowDepth; ++j) {
            const int pj = p0 + j * kRowWaves;
            load_row8(ws.Q + (size_t)(pj < P ? pj : P - 1) * kDim, lane, q[j]);
        }
#pragma unroll
        for (int j = 0; j < kRowDepth; ++j) {
            const int p = p0 + j * kRowWaves;
            if (p < P) {                                                                 // wave-uniform
                const float d = s_z[p];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(d, q[j][i], acc[i]);
            }
        }
    }
    store_row8(s_part + wave * kDim, lane, acc);
    __syncthreads();
    if (wave != 0) return;
    float du[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float s = s_part[8 * lane + i];
#pragma unroll
        for (int w = 1; w < kRowWaves; ++w) s += s_part[w * kDim + 8 * lane + i];
        du[i] = scale * s;
    }
    project_row8(du, u, ws.enorm[b], o);
    store_row8(demb + (size_t)b * kDim, lane, o);
}

__global__ __launch_bounds__(kUnitWaves * SIR_WAVE) void proxy_col_kernel(int B, int P, float scale, ProxyWs ws, float* __restrict__ dproxies) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const int k = blockIdx.x * kUnitWaves + wave;                                        // wave-uniform
    if (k >= P) return;
    float q[8];
    load_row8(ws.Q + (size_t)k * kDim, lane, q);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int b0 = 0; b0 < B; b0 += SIR_WAVE) {
        const int bb = b0 + lane;
        const float dv = bb < B ? ws.dz[(size_t)bb * P + k] : 0.0f;
        const int n = B - b0 < SIR_WAVE ? B - b0 : SIR_WAVE;
        for (int j0 = 0; j0 < n; j0 += 4) {                                              // four unit rows in flight
            float d[4], ur[4][8];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = j0 + jj;                                                   // (< 64; past the batch: dz reads as zero)
                d[jj] = __shfl(dv, j);
                const int row = b0 + j < B ? b0 + j : B - 1;
                load_row8(ws.U + (size_t)row * kDim, lane, ur[jj]);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = d[jj] != 0.0f ? fmaf(d[jj], ur[jj][i], acc[i]) : acc[i];
        }
    }
    float dq[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) dq[i] = scale * acc[i];
    project_row8(dq, q, ws.pnorm[k], o);
    store_row8(dproxies + (size_t)k * kDim, lane, o);
}

__global__ __launch_bounds__(256) void proxy_reduce_kernel(int B, ProxyWs ws, float* __restrict__ loss) {
    __shared__ double red[256];
    double a = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) a += (double)ws.row_loss[b];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)ws.nvalid[0]);
}

}  // namespace

extern "C" size_t sir_proxy_loss_workspace_bytes(int batch, int n_proxies) {
    if (batch < 1 || batch > kMaxRows || n_proxies < 1 || n_proxies > kMaxProtos) return 0;
    size_t off[7];
    return ws_layout(batch, n_proxies, off);
}

extern "C" int sir_proxy_loss(sir_handle* h, const float* emb, const float* proxies, const int64_t* labels, int batch, int n_proxies,
                              float scale, float margin, float* loss, float* demb, float* dproxies, float grad_scale, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const char* who = "sir_proxy_loss";
    if (!h || !emb || !proxies || !labels || !loss || !workspace) {
        sir_set_error("%s: NULL argument (h, emb, proxies, labels, loss and workspace are required)", who);
        return SIR_EINVAL;
    }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: batch=%d outside [1, 2^30]", who, batch); return SIR_EINVAL; }
    if (n_proxies < 1 || n_proxies > kMaxProtos) { sir_set_error("%s: n_proxies=%d outside [1, %d]", who, n_proxies, kMaxProtos); return SIR_EINVAL; }
    if (!(scale > 0.0f) || std::isinf(scale)) { sir_set_error("%s: scale=%g must be positive and finite", who, (double)scale); return SIR_EINVAL; }
    if (!(margin >= 0.0f) || std::isinf(margin)) { sir_set_error("%s: margin=%g must be finite and >= 0", who, (double)margin); return SIR_EINVAL; }
    if (((uintptr_t)emb | (uintptr_t)proxies | (uintptr_t)demb | (uintptr_t)dproxies | (uintptr_t)workspace) & 15u) {
        sir_set_error("%s: emb, proxies, demb, dproxies and workspace must be 16-byte aligned", who);
        return SIR_EINVAL;
    }
    if (((uintptr_t)labels & 7u) || ((uintptr_t)loss & 3u)) { sir_set_error("%s: labels must be 8-byte aligned, loss 4-byte aligned", who); return SIR_EINVAL; }
    size_t off[7];
    const size_t need = ws_layout(batch, n_proxies, off);
    if (workspace_bytes < need) { sir_set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need); return SIR_EINVAL; }
    char* base = (char*)workspace;
    const ProxyWs ws{(int*)(base + off[0]), (double*)(base + off[1]), (double*)(base + off[2]), (float*)(base + off[3]),
                     (float*)(base + off[4]), (float*)(base + off[5]), (float*)(base + off[6])};
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)batch + n_proxies;
    hipLaunchKernelGGL(proxy_unit_kernel, dim3((unsigned)((rows + kUnitWaves - 1) / kUnitWaves + 1)), dim3(kUnitWaves * SIR_WAVE), 0, st, emb, proxies,
                       (const long long*)labels, batch, n_proxies, ws);
    hipLaunchKernelGGL(proxy_row_kernel, dim3(batch), dim3(kRowThreads), 0, st, (const long long*)labels, batch, n_proxies, scale, margin, grad_scale,
                       ws, dproxies ? 1 : 0, demb, h->status);
    if (dproxies)
        hipLaunchKernelGGL(proxy_col_kernel, dim3((n_proxies + kUnitWaves - 1) / kUnitWaves), dim3(kUnitWaves * SIR_WAVE), 0, st, batch, n_proxies,
                           scale, ws, dproxies);
    hipLaunchKernelGGL(proxy_reduce_kernel, dim3(1), dim3(256), 0, st, batch, ws, loss);
    return sir_check_hip(hipGetLastError(), "sir_proxy_loss kernels");
}
