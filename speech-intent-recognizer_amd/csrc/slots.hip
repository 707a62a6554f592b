// Slot heads, the loss (include/sir_hip.h: sir_ce_loss_slots): one logit row as several independent softmax segments, the
// weighted sum of their soft-target cross-entropies and its gradient.  (sir_classify_slots and sir_eval_accumulate_slots sit
// with their single-head relatives in evaluate.hip, where either form of a call wraps the same per-segment function.)
//
// The contract is bit identity, per slot, with sir_ce_loss_soft on a contiguous copy of the segment.  It holds by construction:
// the kernel below runs ce_loss_kernel's body (ce_loss_rows.h: the valid-row count, the row arithmetic on a register array of
// 32 floats for widths <= 32, else 64, the LDS sum) once per slot in ONE workgroup of 256 threads, with the segment's
// addressing -- a row's segment starts at logits + b * num_classes + start_g, its labels are labels + b * n_slots + g.
// Slots run one after the other: the total is then one thread's fp32 sum in slot order, with no scratch buffer and no
// second launch.
#include <cmath>
#include "ce_loss_rows.h"

namespace {

struct CeSlotTable : SlotTable {
    float gs[kMaxSlots], w[kMaxSlots];               // grad_scale * w_g (fp32 product), w_g
};

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
        const float nvalid = ce_valid_rows(labels, B, G, g, cnt);
        const float acc = C <= 32 ? ce_rows<32, SOFT>(logits, labels, labels_b, lam, eps, B, NC, start, G, g, C, nvalid, tab.gs[g], dlogits, status)
                                  : ce_rows<64, SOFT>(logits, labels, labels_b, lam, eps, B, NC, start, G, g, C, nvalid, tab.gs[g], dlogits, status);
        const float sum = ce_block_sum(acc, red);
        if (threadIdx.x == 0) {
#pragma clang fp contract(off)                                                           // a rounded product, then a rounded sum: no fma
            const float sl = sum / nvalid;
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
