// Slot heads, the loss (include/sir_hip.h: sir_ce_loss_slots): one logit row as several independent softmax segments, the
// weighted sum of their soft-target cross-entropies and its gradient.  (sir_classify_slots and sir_eval_accumulate_slots sit
// with their single-head relatives in evaluate.hip, whose row helpers they share.)
//
// The contract is bit identity, per slot, with sir_ce_loss_soft on a contiguous copy of the segment, so the kernel below is
// ce_loss_kernel (train_loss_optim_kernels.h) run once per slot by ONE workgroup of 256 threads: the same thread-per-row map,
// the same per-row expressions in the same order on a register array of the same length (32 for widths <= 32, else 64), the
// same two LDS trees.  Only the addressing differs: a row's segment starts at logits + b * num_classes + start_g and its labels
// at labels + b * n_slots + g.  The row arithmetic is restated here rather than shared so that ce_loss_kernel and the code
// generated for it stay untouched.  Slots run one after the other: the total is then one thread's fp32 sum in slot order,
// with no scratch buffer and no second launch.
#include <cmath>
#include "sir_internal.h"

namespace {

constexpr int kMaxSlots = 8;
constexpr unsigned int kStatusBadCeLabel = 2u;       // api.hip check_status_impl, as ce_loss_kernel

struct CeSlotTable {
    int n;
    int start[kMaxSlots], size[kMaxSlots];
    float gs[kMaxSlots], w[kMaxSlots];               // grad_scale * w_g (fp32 product), w_g
};

// this thread's rows of one slot -> its partial of the slot's loss sum; writes the slot's segment of dlogits
template <int CMAX, bool SOFT>
__device__ __forceinline__ float ce_slot_rows(const float* __restrict__ logits, const long long* __restrict__ labels,
                                              const long long* __restrict__ labels_b, const float* __restrict__ lam, float eps,
                                              int B, int NC, int G, int g, int start, int C, float nvalid, float grad_scale,
                                              float* __restrict__ dlogits, unsigned int* status) {
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* r = logits + (size_t)b * NC + start;
        const long long yl = labels[(size_t)b * G + g];
        const bool ignored = yl == -100ll;
        const bool bad = !ignored && (yl < 0 || yl >= (long long)C);
        if (bad) __hip_atomic_fetch_or(status, kStatusBadCeLabel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int y = (bad || ignored) ? 0 : (int)yl;
        if constexpr (SOFT) {
            const long long yl2 = (labels_b && !ignored) ? labels_b[(size_t)b * G + g] : yl;
            const bool bad2 = !ignored && (yl2 < 0 || yl2 >= (long long)C);
            if (bad2) __hip_atomic_fetch_or(status, kStatusBadCeLabel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int y2 = (bad2 || ignored) ? 0 : (int)yl2;
            const float lm = (labels_b && lam) ? lam[b] : 1.0f;
            const float wa = (1.0f - eps) * lm, wb = (1.0f - eps) * (1.0f - lm), u = eps / (float)C;
            float v[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) v[c] = c < C ? r[c] : 0.0f;
            const float ra = r[y], rb = r[y2];
            float mx = v[0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c) if (c < C) mx = fmaxf(mx, v[c]);
            float den = 0.0f, dsum = 0.0f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) if (c < C) { const float d = v[c] - mx; dsum += d; v[c] = expf(d); den += v[c]; }
            const float row = logf(den) - (wa * (ra - mx) + wb * (rb - mx) + u * dsum);
            acc += (bad || bad2) ? __builtin_nanf("") : (ignored ? 0.0f : row);
            if (dlogits) {
                const float inv = 1.0f / den, gs = ignored ? 0.0f : grad_scale / nvalid;
                float* dr = dlogits + (size_t)b * NC + start;
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) {
                        const float q = u + (c == y ? wa : 0.0f) + (c == y2 ? wb : 0.0f);
                        dr[c] = ignored ? 0.0f : (v[c] * inv - q) * gs;
                    }
            }
            continue;
        }
        float v[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) v[c] = c < C ? r[c] : 0.0f;
        const float ry = r[y];
        float mx = v[0];
#pragma unroll
        for (int c = 1; c < CMAX; ++c) if (c < C) mx = fmaxf(mx, v[c]);
        float den = 0.0f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) if (c < C) { v[c] = expf(v[c] - mx); den += v[c]; }
        const float lse = mx + logf(den);
        acc += bad ? __builtin_nanf("") : (ignored ? 0.0f : lse - ry);
        if (dlogits) {
            const float inv = 1.0f / den, gs = ignored ? 0.0f : grad_scale / nvalid;
            float* dr = dlogits + (size_t)b * NC + start;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) dr[c] = ignored ? 0.0f : (v[c] * inv - (c == y ? 1.0f : 0.0f)) * gs;
        }
    }
    return acc;
}

template <bool SOFT>
__global__ __launch_bounds__(256) void ce_loss_slots_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                            const long long* __restrict__ labels_b, const float* __restrict__ lam,
                                                            float eps, CeSlotTable tab, int B, int NC, float* __restrict__ loss,
                                                            float* __restrict__ slot_loss, float* __restrict__ dlogits,
                                                            unsigned int* status) {
    __shared__ float red[256];
    __shared__ int cnt[256];
    const int G = tab.n;
    float total = 0.0f;                                                                  // thread 0's alone is used
    for (int g = 0; g < G; ++g) {                                                        // uniform over the workgroup
        const int start = tab.start[g], C = tab.size[g];
        int nv = 0;
        for (int b = threadIdx.x; b < B; b += 256) nv += labels[(size_t)b * G + g] != -100ll ? 1 : 0;
        cnt[threadIdx.x] = nv;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
            __syncthreads();
        }
        const float nvalid = (float)cnt[0];
        const float acc = C <= 32 ? ce_slot_rows<32, SOFT>(logits, labels, labels_b, lam, eps, B, NC, G, g, start, C, nvalid, tab.gs[g], dlogits, status)
                                  : ce_slot_rows<64, SOFT>(logits, labels, labels_b, lam, eps, B, NC, G, g, start, C, nvalid, tab.gs[g], dlogits, status);
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
#pragma clang fp contract(off)                                                           // a rounded product, then a rounded sum: no fma
            const float sl = red[0] / nvalid;
            if (slot_loss) slot_loss[g] = sl;
            const float term = tab.w[g] * sl;
            total = total + term;
        }
        __syncthreads();                                                                 // red / cnt are rewritten by the next slot
    }
    if (threadIdx.x == 0) loss[0] = total;
}

}  // namespace

// The layout rules of include/sir_hip.h ("slot heads"); fills start[] / size[] (arrays of 8).  false: `who`'s error is set.
bool sir_slots_check_layout(const char* who, const int32_t* slot_sizes, int n_slots, int num_classes, int* start, int* size) {
    if (!slot_sizes) { sir_set_error("%s: slot_sizes is NULL", who); return false; }
    if (n_slots < 1 || n_slots > kMaxSlots) { sir_set_error("%s: n_slots=%d outside [1, %d]", who, n_slots, kMaxSlots); return false; }
    if (num_classes < 1 || num_classes > 64) { sir_set_error("%s: num_classes=%d outside [1, 64]", who, num_classes); return false; }
    long long sum = 0;
    for (int g = 0; g < n_slots; ++g) {
        if (slot_sizes[g] < 1 || slot_sizes[g] > 64) { sir_set_error("%s: slot %d has width %d (1..64)", who, g, (int)slot_sizes[g]); return false; }
        start[g] = (int)sum;
        size[g] = slot_sizes[g];
        sum += slot_sizes[g];
    }
    if (sum != num_classes) { sir_set_error("%s: the slot widths add up to %lld, num_classes is %d", who, sum, num_classes); return false; }
    return true;
}

extern "C" int sir_ce_loss_slots(sir_handle* h, const float* logits, const int64_t* labels_a, const int64_t* labels_b, const float* lam,
                                 float label_smoothing, const int32_t* slot_sizes, const float* slot_weights, int n_slots, int batch,
                                 int num_classes, float* loss, float* slot_loss, float* dlogits, float grad_scale, void* stream_) {
    const char* who = "sir_ce_loss_slots";
    if (!h || !logits || !labels_a || !loss) { sir_set_error("%s: NULL argument (h, logits, labels_a and loss are required)", who); return SIR_EINVAL; }
    if (batch < 1) { sir_set_error("%s: bad shape batch=%d", who, batch); return SIR_EINVAL; }
    CeSlotTable tab;
    if (!sir_slots_check_layout(who, slot_sizes, n_slots, num_classes, tab.start, tab.size)) return SIR_EINVAL;
    if (!(label_smoothing >= 0.0f && label_smoothing < 1.0f)) { sir_set_error("%s: label_smoothing %g outside [0, 1)", who, (double)label_smoothing); return SIR_EINVAL; }
    tab.n = n_slots;
    for (int g = 0; g < n_slots; ++g) {
        const float w = slot_weights ? slot_weights[g] : 1.0f;
        if (!(w >= 0.0f) || std::isinf(w)) { sir_set_error("%s: slot_weights[%d] = %g must be finite and >= 0", who, g, (double)w); return SIR_EINVAL; }
        tab.w[g] = w;
        tab.gs[g] = grad_scale * w;
    }
    if ((((uintptr_t)logits | (uintptr_t)lam | (uintptr_t)loss | (uintptr_t)slot_loss | (uintptr_t)dlogits) & 3u) ||
        (((uintptr_t)labels_a | (uintptr_t)labels_b) & 7u)) {
        sir_set_error("%s: float pointers must be 4-byte aligned, labels 8-byte aligned", who);
        return SIR_EINVAL;
    }
    const hipStream_t st = (hipStream_t)stream_;
    const long long* la = (const long long*)labels_a;
    const long long* lb = (const long long*)labels_b;
    SirProfScope prof(h, SIR_K_CE, st);
    if (labels_b != nullptr || label_smoothing != 0.0f)
        hipLaunchKernelGGL(ce_loss_slots_kernel<true>, dim3(1), dim3(256), 0, st, logits, la, lb, lam, label_smoothing, tab, batch,
                           num_classes, loss, slot_loss, dlogits, h->status);
    else
        hipLaunchKernelGGL(ce_loss_slots_kernel<false>, dim3(1), dim3(256), 0, st, logits, la, lb, lam, label_smoothing, tab, batch,
                           num_classes, loss, slot_loss, dlogits, h->status);
    SIR_KCHECK();
    return SIR_OK;
}
