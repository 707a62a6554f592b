// What follows the forward pass, on the device (include/sir_hip.h: sir_classify, sir_eval_accumulate, sir_temperature_fit, and
// the slot-head forms sir_classify_slots, sir_eval_accumulate_slots).
//
// One logit row is G independent softmax segments (SlotTable, sir_internal.h), lane j of a segment holding class start_g + j,
// and a single head is the segment that is the whole row.  The work on a segment is written once, as a device function that
// takes the segment's addressing (classify_segment, eval_accumulate_segment, eval_finish_block); the single-head kernel and
// the slot kernel of a call are thin __global__ wrappers around it.  So each slot's results carry the bits of the single-head
// call on a contiguous copy of the segment by construction.  (The slot kernels on a one-slot table would serve a single head
// with the same bits; they measured 8 % / 3 % slower at batch 256 -- DESIGN.md section 4 "Slot heads" -- hence the wrappers.)
//
// A row has at most 64 classes, so ONE WAVE OWNS A ROW, one lane per class: the row maximum and the softmax denominator are
// xor-butterfly reductions over the 64 lanes (every lane ends with the same bits: each level adds the same two values in both
// partners, and fp32 addition commutes), and a class's rank is counted, not sorted for -- lane c walks the C logits of its row
// (a readlane per class, the index is wave-uniform) and counts those that beat its own: larger, or equal with a lower index.
// The classes of rank < k are the top-k in order, rank 0 is the first maximum, and the rank of the label's lane answers "is
// the label among the first j + 1" for all eight j at once.
//   sir_classify*       : grid-stride over rows, 4 waves per workgroup; slot form: the wave of a row walks its slots and
//                         multiplies the rank-0 probabilities in slot order (the joint probability).
//   sir_eval_accumulate*: launch 1, grid (workgroups, G), up to 64 workgroups of 16 waves per slot: workgroup (x, g) takes
//                         segment g and column g of the labels into slot state g (global wave w takes rows w, w + waves,
//                         ...).  Counters and the workgroup's confusion counts are gathered in LDS (integer atomics) and
//                         flushed once, one global integer atomic per non-zero word.  The two floating sums have a fixed
//                         order: per-wave doubles in row order, added in wave order into the workgroup's partial, which
//                         goes to a scratch area behind the state's fields; the last launch, one workgroup per block of
//                         the state, adds the partials in workgroup order.  Slot form only: between the two, the joint
//                         block -- the same wave / row map once more, the wave of a row walks its slots.
//   sir_temperature_fit : per Newton step a reduction launch (<= 256 workgroups of 16 waves, global wave g takes rows g,
//                         g + waves, ...; per-workgroup partials in the workspace) and a one-thread update launch.
#include <cmath>
#include "sir_internal.h"
#include "row_softmax.h"  // row_softmax, wave_max, kClsWaves, classify_blocks
#include "wave_fft.h"      // wave_sum

namespace {

constexpr int kEvalWaves = 16;                       // waves of the accumulate / fit workgroups
constexpr int kEvalThreads = kEvalWaves * SIR_WAVE;
constexpr int kFitMaxBlocks = 256;
constexpr int kEvalMaxBlocks = 64;                   // workgroups of sir_eval_accumulate = partial rows of the state's scratch area
constexpr int kFitHeader = 64;                       // workspace: {float beta, float nll at beta = 1} then the partials

struct EvalSlotTable : SlotTable {
    long long base[kMaxSlots + 1];                   // 8-byte word offset of slot state g in the state; [n]: the joint block
};

// One segment of one row in its wave: the C logits at logits + at -> their probabilities at probs + at (probs NULL: not wanted)
// and the segment's k top-k entries at topk_idx / topk_prob + out.  A finite segment multiplies `joint` by its rank-0
// probability, another one clears `all_finite`.
__device__ __forceinline__ void classify_segment(const float* __restrict__ logits, size_t at, int lane, int C, float beta, int k,
                                                 float* __restrict__ probs, int* __restrict__ topk_idx, float* __restrict__ topk_prob,
                                                 size_t out, float& joint, bool& all_finite) {
    const float nan = __builtin_nanf("");
    const float l = lane < C ? logits[at + lane] : 0.0f;
    const RowSoftmax r = row_softmax(l, lane, C, beta);
    const float p = r.e / r.den;
    if (r.finite) {
        if (lane < C) {
            if (probs) probs[at + lane] = p;
            if (r.rank < k) { topk_idx[out + r.rank] = lane; topk_prob[out + r.rank] = p; }
        } else if (lane < k) { topk_idx[out + lane] = -1; topk_prob[out + lane] = 0.0f; }   // ranks >= C (sir_classify has k <= C)
        const unsigned long long top = __ballot(lane < C && r.rank == 0);              // exactly one lane
        const int pred = top ? __ffsll((long long)top) - 1 : 0;
        joint *= __shfl(p, pred);
    } else {
        all_finite = false;
        if (lane < C && probs) probs[at + lane] = nan;
        if (lane < k) { topk_idx[out + lane] = -1; topk_prob[out + lane] = nan; }
    }
}

// a single head: the segment is the row (and nothing reads the joint probability)
__global__ __launch_bounds__(kClsWaves * SIR_WAVE) void classify_kernel(const float* __restrict__ logits, int B, int C,
                                                                         const float* __restrict__ inv_t, int k, float* __restrict__ probs,
                                                                         int* __restrict__ topk_idx, float* __restrict__ topk_prob) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const float beta = inv_t ? inv_t[0] : 1.0f;
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {      // wave-uniform
        float joint = 1.0f;
        bool all_finite = true;
        classify_segment(logits, (size_t)b * C, lane, C, beta, k, probs, topk_idx, topk_prob, (size_t)b * k, joint, all_finite);
    }
}

// topk_idx / topk_prob are [B][G][k], joint_prob [B] or NULL: the wave of a row walks its slots, the rank-0 probabilities are
// multiplied in slot order
__global__ __launch_bounds__(kClsWaves * SIR_WAVE) void classify_slots_kernel(const float* __restrict__ logits, int B, int NC, SlotTable tab,
                                                                               const float* __restrict__ inv_t, int k, float* __restrict__ probs,
                                                                               int* __restrict__ topk_idx, float* __restrict__ topk_prob,
                                                                               float* __restrict__ joint_prob) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const float nan = __builtin_nanf("");
    const int G = tab.n;
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {      // wave-uniform
        float joint = 1.0f;
        bool all_finite = true;
        for (int g = 0; g < G; ++g) {
            const int start = tab.start[g], C = tab.size[g];
            const float beta = inv_t ? inv_t[g] : 1.0f;
            classify_segment(logits, (size_t)b * NC + start, lane, C, beta, k, probs, topk_idx, topk_prob, ((size_t)b * G + g) * k, joint,
                             all_finite);
        }
        if (joint_prob && lane == 0) joint_prob[b] = all_finite ? joint : nan;
    }
}

// offsets into the evaluation state, in 8-byte words (include/sir_hip.h)
struct EvalLayout {
    int n, topk, nll, bin_count, bin_correct, bin_conf, ignored, nonfinite, scratch, words;
};
__host__ __device__ inline EvalLayout eval_layout(int C, int M) {
    EvalLayout o;
    o.n = C * C; o.topk = o.n + 1; o.nll = o.topk + 8; o.bin_count = o.nll + 1; o.bin_correct = o.bin_count + M;
    o.bin_conf = o.bin_correct + M; o.ignored = o.bin_conf + M; o.nonfinite = o.ignored + 1; o.scratch = o.nonfinite + 1;
    o.words = o.scratch + kEvalMaxBlocks * (M + 1);         // scratch: per workgroup {nll partial, bin_conf partial[M]}
    return o;
}

// how a row is treated, wave-uniform: 0 counted, 1 ignored (label -100), 2 label outside [0, C), 3 non-finite row
__device__ __forceinline__ int row_kind(long long y, int C, bool finite) {
    if (y == -100ll) return 1;
    if (y < 0 || y >= (long long)C) return 2;
    return finite ? 0 : 3;
}

// offsets into the joint block, in 8-byte words
struct JointLayout {
    int n, exact, slots_correct, nll, bin_count, bin_correct, bin_conf, excluded, scratch, words;
};
__host__ __device__ inline JointLayout joint_layout(int M) {
    JointLayout o;
    o.n = 0; o.exact = 1; o.slots_correct = 2; o.nll = 11; o.bin_count = 12; o.bin_correct = o.bin_count + M;
    o.bin_conf = o.bin_correct + M; o.excluded = o.bin_conf + M; o.scratch = o.excluded + 1;
    o.words = o.scratch + kEvalMaxBlocks * (M + 1);
    return o;
}

// The tail the accumulate kernels share, behind the barrier that follows the rows: thread m < M adds bin m's per-wave sums in
// wave order into the workgroup's partial row (part[1 + m]; the scratch area starts `scratch` words into the block) and flushes
// the bin's two counters, thread 64 does the same for the NLL (part[0]).
__device__ __forceinline__ void eval_flush_bins(unsigned long long* state, int scratch, int bin_count, int bin_correct, int M,
                                                const double (*s_conf)[64], const double* s_nll, const unsigned int* s_bin_count,
                                                const unsigned int* s_bin_correct) {
    const int t = threadIdx.x;
    double* part = reinterpret_cast<double*>(state + scratch) + (size_t)blockIdx.x * (M + 1);
    if (t < M) {
        double c = 0.0;
        for (int w = 0; w < kEvalWaves; ++w) c += s_conf[w][t];
        part[1 + t] = c;
        if (s_bin_count[t]) atomicAdd(&state[bin_count + t], (unsigned long long)s_bin_count[t]);
        if (s_bin_correct[t]) atomicAdd(&state[bin_correct + t], (unsigned long long)s_bin_correct[t]);
    } else if (t == 64) {
        double c = 0.0;
        for (int w = 0; w < kEvalWaves; ++w) c += s_nll[w];
        part[0] = c;
    }
}

// Workgroup blockIdx.x of gridDim.x over one segment of the rows -- logits + b * row_stride + start, C wide, its label
// labels[b * label_stride + label_col] -- into the single-head state at `state`.  A single head is (C, 0, 1, 0).
__device__ __forceinline__ void eval_accumulate_segment(const float* __restrict__ logits, const long long* __restrict__ labels, int B,
                                                        int row_stride, int start, int label_stride, int label_col, int C, float beta, int M,
                                                        unsigned long long* state, unsigned int* status) {
    __shared__ double s_conf[kEvalWaves][64];
    __shared__ double s_nll[kEvalWaves];
    __shared__ unsigned int s_bin_count[64], s_bin_correct[64], s_topk[8], s_misc[3];      // misc: n, ignored, non-finite
    __shared__ unsigned int s_cm[64 * 64];                                              // this workgroup's confusion counts, [C][C]
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const EvalLayout o = eval_layout(C, M);
    s_conf[wave][lane] = 0.0;
    for (int i = threadIdx.x; i < C * C; i += kEvalThreads) s_cm[i] = 0u;
    if (threadIdx.x < 64) { s_bin_count[threadIdx.x] = 0u; s_bin_correct[threadIdx.x] = 0u; }
    if (threadIdx.x < 8) s_topk[threadIdx.x] = 0u;
    if (threadIdx.x < 3) s_misc[threadIdx.x] = 0u;
    __syncthreads();
    double nll = 0.0;                                                                   // the same value on every lane of the wave
    // the next row's logit and label are loaded before this row's arithmetic: the wave's rows are one dependent chain
    // otherwise, a memory latency each
    const int first_row = blockIdx.x * kEvalWaves + wave, stride = gridDim.x * kEvalWaves;
    float l_next = (first_row < B && lane < C) ? logits[(size_t)first_row * row_stride + start + lane] : 0.0f;
    long long y_next = first_row < B ? labels[(size_t)first_row * label_stride + label_col] : 0ll;
    for (int b = first_row; b < B; b += stride) {                                       // wave-uniform
        const float l = l_next;
        const long long y = y_next;
        const int nb = b + stride;
        if (nb < B) {
            l_next = lane < C ? logits[(size_t)nb * row_stride + start + lane] : 0.0f;
            y_next = labels[(size_t)nb * label_stride + label_col];
        }
        const RowSoftmax r = row_softmax(l, lane, C, beta);
        const int kind = row_kind(y, C, r.finite);
        if (kind != 0) {
            if (lane == 0) {
                if (kind == 1) atomicAdd(&s_misc[1], 1u);
                else if (kind == 3) atomicAdd(&s_misc[2], 1u);
                else __hip_atomic_fetch_or(status, SIR_STATUS_EVAL_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            continue;
        }
        const int yi = (int)y;
        const int rank_y = __shfl(r.rank, yi);
        const float dy = __shfl(r.d, yi);
        const unsigned long long top = __ballot(lane < C && r.rank == 0);              // exactly one lane
        const int pred = top ? __ffsll((long long)top) - 1 : 0;                        // (a finite row always has a rank 0)
        const float pmax = __shfl(r.e, pred) / r.den;
        int bin = (int)floorf(pmax * (float)M);
        bin = bin < M - 1 ? bin : M - 1;
        bin = bin > 0 ? bin : 0;                                                        // (a NaN beta must not index outside the bins)
        nll += (double)(log1pf(r.rest) - dy);
        if (lane == 0) {
            s_conf[wave][bin] += (double)pmax;                                          // this wave's rows, in row order
            atomicAdd(&s_misc[0], 1u);
            atomicAdd(&s_bin_count[bin], 1u);
            if (pred == yi) atomicAdd(&s_bin_correct[bin], 1u);
            atomicAdd(&s_cm[yi * C + pred], 1u);
        }
        if (lane < 8 && rank_y <= lane) atomicAdd(&s_topk[lane], 1u);
    }
    if (lane == 0) s_nll[wave] = nll;
    __syncthreads();
    const int t = threadIdx.x;
    for (int i = t; i < C * C; i += kEvalThreads)
        if (s_cm[i]) atomicAdd(&state[i], (unsigned long long)s_cm[i]);
    eval_flush_bins(state, o.scratch, o.bin_count, o.bin_correct, M, s_conf, s_nll, s_bin_count, s_bin_correct);
    if (t >= 128 && t < 136) {
        if (s_topk[t - 128]) atomicAdd(&state[o.topk + (t - 128)], (unsigned long long)s_topk[t - 128]);
    } else if (t == 192) {
        if (s_misc[0]) atomicAdd(&state[o.n], (unsigned long long)s_misc[0]);
        if (s_misc[1]) atomicAdd(&state[o.ignored], (unsigned long long)s_misc[1]);
        if (s_misc[2]) atomicAdd(&state[o.nonfinite], (unsigned long long)s_misc[2]);
    }
}

// a single head: the segment is the row
__global__ __launch_bounds__(kEvalThreads) void eval_accumulate_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                       int B, int C, const float* __restrict__ inv_t, int M,
                                                                       unsigned long long* state, unsigned int* status) {
    eval_accumulate_segment(logits, labels, B, C, 0, 1, 0, C, inv_t ? inv_t[0] : 1.0f, M, state, status);
}

// grid (workgroups, G): workgroup (x, g) is eval_accumulate_kernel's workgroup x on segment g and column g of the labels, into
// slot state g
__global__ __launch_bounds__(kEvalThreads) void eval_slots_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                  int B, int NC, EvalSlotTable tab, const float* __restrict__ inv_t, int M,
                                                                  unsigned long long* state_all, unsigned int* status) {
    const int g = blockIdx.y;
    eval_accumulate_segment(logits, labels, B, NC, tab.start[g], tab.n, g, tab.size[g], inv_t ? inv_t[g] : 1.0f, M, state_all + tab.base[g],
                            status);
}

// the joint block: a row counts iff every slot has a label in [0, C_g) and a finite segment (the status word is raised by
// eval_slots_kernel, which sees the same labels)
__global__ __launch_bounds__(kEvalThreads) void eval_joint_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                  int B, int NC, EvalSlotTable tab, const float* __restrict__ inv_t, int M,
                                                                  unsigned long long* state_all) {
    __shared__ double s_conf[kEvalWaves][64];
    __shared__ double s_nll[kEvalWaves];
    __shared__ unsigned int s_bin_count[64], s_bin_correct[64], s_right[kMaxSlots + 1], s_misc[3];   // misc: n, exact, excluded
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const int G = tab.n;
    unsigned long long* state = state_all + tab.base[G];
    const JointLayout o = joint_layout(M);
    s_conf[wave][lane] = 0.0;
    if (threadIdx.x < 64) { s_bin_count[threadIdx.x] = 0u; s_bin_correct[threadIdx.x] = 0u; }
    if (threadIdx.x <= kMaxSlots) s_right[threadIdx.x] = 0u;
    if (threadIdx.x < 3) s_misc[threadIdx.x] = 0u;
    __syncthreads();
    double nll = 0.0;                                                                   // the same value on every lane of the wave
    const int stride = gridDim.x * kEvalWaves;
    for (int b = blockIdx.x * kEvalWaves + wave; b < B; b += stride) {                  // wave-uniform
        float joint = 1.0f;
        double row_nll = 0.0;
        int right = 0;
        bool counted = true;
        for (int g = 0; g < G; ++g) {                                                   // every branch below is wave-uniform
            const int start = tab.start[g], C = tab.size[g];
            const float beta = inv_t ? inv_t[g] : 1.0f;
            const float l = lane < C ? logits[(size_t)b * NC + start + lane] : 0.0f;
            const long long y = labels[(size_t)b * G + g];
            const RowSoftmax r = row_softmax(l, lane, C, beta);
            if (row_kind(y, C, r.finite) != 0) { counted = false; break; }
            const int yi = (int)y;
            const float dy = __shfl(r.d, yi);
            const unsigned long long top = __ballot(lane < C && r.rank == 0);
            const int pred = top ? __ffsll((long long)top) - 1 : 0;
            joint *= __shfl(r.e, pred) / r.den;
            row_nll += (double)(log1pf(r.rest) - dy);
            right += pred == yi ? 1 : 0;
        }
        if (!counted) {
            if (lane == 0) atomicAdd(&s_misc[2], 1u);
            continue;
        }
        int bin = (int)floorf(joint * (float)M);
        bin = bin < M - 1 ? bin : M - 1;
        bin = bin > 0 ? bin : 0;                                                        // (a NaN beta must not index outside the bins)
        nll += row_nll;
        if (lane == 0) {
            s_conf[wave][bin] += (double)joint;                                         // this wave's rows, in row order
            atomicAdd(&s_misc[0], 1u);
            atomicAdd(&s_bin_count[bin], 1u);
            atomicAdd(&s_right[right], 1u);
            if (right == G) { atomicAdd(&s_misc[1], 1u); atomicAdd(&s_bin_correct[bin], 1u); }
        }
    }
    if (lane == 0) s_nll[wave] = nll;
    __syncthreads();
    const int t = threadIdx.x;
    eval_flush_bins(state, o.scratch, o.bin_count, o.bin_correct, M, s_conf, s_nll, s_bin_count, s_bin_correct);
    if (t >= 128 && t <= 128 + kMaxSlots) {
        if (s_right[t - 128]) atomicAdd(&state[o.slots_correct + (t - 128)], (unsigned long long)s_right[t - 128]);
    } else if (t == 192) {
        if (s_misc[0]) atomicAdd(&state[o.n], (unsigned long long)s_misc[0]);
        if (s_misc[1]) atomicAdd(&state[o.exact], (unsigned long long)s_misc[1]);
        if (s_misc[2]) atomicAdd(&state[o.excluded], (unsigned long long)s_misc[2]);
    }
}

// Adds the workgroups' partials to the two floating fields of one block of the state (a slot state or the joint block; its
// scratch area, NLL and bin_conf at the given word offsets), in workgroup order: thread 0 the NLL, thread 1 + m bin m
__device__ __forceinline__ void eval_finish_block(unsigned long long* state, int scratch, int nll, int bin_conf, int M, int blocks) {
    const int t = threadIdx.x;
    if (t > M) return;
    const double* part = reinterpret_cast<const double*>(state + scratch);
    double c = 0.0;
    for (int b = 0; b < blocks; ++b) c += part[(size_t)b * (M + 1) + t];
    double* dst = reinterpret_cast<double*>(state + (t == 0 ? nll : bin_conf + (t - 1)));
    *dst += c;
}
__global__ __launch_bounds__(128) void eval_finish_kernel(unsigned long long* state, int C, int M, int blocks) {
    const EvalLayout o = eval_layout(C, M);
    eval_finish_block(state, o.scratch, o.nll, o.bin_conf, M, blocks);
}
// workgroup g: slot state g < n, or the joint block
__global__ __launch_bounds__(128) void eval_slots_finish_kernel(unsigned long long* state_all, EvalSlotTable tab, int M, int blocks) {
    const int g = blockIdx.x;
    int scratch, nll, bin_conf;
    if (g < tab.n) { const EvalLayout o = eval_layout(tab.size[g], M); scratch = o.scratch; nll = o.nll; bin_conf = o.bin_conf; }
    else { const JointLayout o = joint_layout(M); scratch = o.scratch; nll = o.nll; bin_conf = o.bin_conf; }
    eval_finish_block(state_all + tab.base[g], scratch, nll, bin_conf, M, blocks);
}

// layout check + word offsets of the G + 1 blocks; returns the state's size in 8-byte words, 0 with `who`'s error set
size_t slot_table(const char* who, const int32_t* slot_sizes, int n_slots, int num_classes, int n_bins, EvalSlotTable* tab) {
    if (!sir_slots_check_layout(who, slot_sizes, n_slots, num_classes, tab->start, tab->size)) return 0;
    tab->n = n_slots;
    long long words = 0;
    for (int g = 0; g < n_slots; ++g) {
        tab->base[g] = words;
        if (n_bins >= 1 && n_bins <= 64) words += eval_layout(tab->size[g], n_bins).words;
    }
    tab->base[n_slots] = words;
    if (n_bins >= 1 && n_bins <= 64) words += joint_layout(n_bins).words;
    return (size_t)words;
}

inline int eval_blocks(int batch) {
    const int b = (batch + kEvalWaves - 1) / kEvalWaves;
    return b > kEvalMaxBlocks ? kEvalMaxBlocks : b;
}

inline int fit_blocks(int n_rows) {
    const int b = (n_rows + 63) / 64;
    return b < 1 ? 1 : (b > kFitMaxBlocks ? kFitMaxBlocks : b);
}

// partial[block] = {sum f_i, sum g_i, sum h_i, rows} over the block's rows at *beta_ptr (NULL: 1):
// f_i = logsumexp(beta l) - beta l_y, g_i = E_p[l] - l_y, h_i = Var_p(l)
__global__ __launch_bounds__(kEvalThreads) void fit_reduce_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                  int N, int C, const float* __restrict__ beta_ptr,
                                                                  double* __restrict__ partials, unsigned int* status) {
    __shared__ double s_part[kEvalWaves][4];
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const float beta = beta_ptr ? beta_ptr[0] : 1.0f;
    double f = 0.0, g = 0.0, hs = 0.0, cnt = 0.0;                                        // the same values on every lane
    const int stride = gridDim.x * kEvalWaves;
    for (int b = blockIdx.x * kEvalWaves + wave; b < N; b += stride) {                  // wave-uniform
        const bool on = lane < C;
        const float l = on ? logits[(size_t)b * C + lane] : 0.0f;
        const long long y = labels[b];
        const bool finite = __ballot(on && is_nonfinite(l)) == 0ull;
        const int kind = row_kind(y, C, finite);
        if (kind != 0) {
            if (kind == 2 && lane == 0) __hip_atomic_fetch_or(status, SIR_STATUS_EVAL_LABEL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const float m = wave_max(on ? l : -INFINITY);
        const float c = l - m;                                                           // centred logit: the moments below are of c
        const float e = on ? expf(c * beta) : 0.0f;
        const unsigned long long at_max = __ballot(on && l == m);
        const int first = __ffsll((long long)at_max) - 1;
        const float rest = wave_sum(lane == first ? 0.0f : e);                           // as row_softmax
        const float den = 1.0f + rest;
        const float mean = wave_sum(e * c) / den;
        const float dc = c - mean;
        const float var = wave_sum(e * dc * dc) / den;
        const float cy = __shfl(c, (int)y);
        f += (double)(log1pf(rest) - cy * beta);
        g += (double)(mean - cy);
        hs += (double)var;
        cnt += 1.0;
    }
    if (lane == 0) { s_part[wave][0] = f; s_part[wave][1] = g; s_part[wave][2] = hs; s_part[wave][3] = cnt; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double c = 0.0;
        for (int w = 0; w < kEvalWaves; ++w) c += s_part[w][threadIdx.x];
        partials[(size_t)blockIdx.x * 4 + threadIdx.x] = c;
    }
}

// One thread.  step >= 0: the Newton update after the reduction at the current beta (step 0: beta = 1, and f(1) is kept).
// step < 0: the reduction was the closing one at the fitted beta -> out.
__global__ void fit_update_kernel(const double* __restrict__ partials, int blocks, int step, int iters, float* hdr, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double F = 0.0, G = 0.0, H = 0.0, n = 0.0;
    for (int i = 0; i < blocks; ++i) { F += partials[4 * i]; G += partials[4 * i + 1]; H += partials[4 * i + 2]; n += partials[4 * i + 3]; }
    const double f = F / n;                                                             // no rows: 0 / 0 = NaN
    if (step < 0) {
        const float beta = iters > 0 ? hdr[0] : 1.0f;
        out[0] = beta;
        out[1] = iters > 0 ? hdr[1] : (float)f;
        out[2] = (float)f;
        return;
    }
    const double beta = step > 0 ? (double)hdr[0] : 1.0;
    if (step == 0) hdr[1] = (float)f;
    const double g = G / n, h = H / n;
    double b = beta - g / fmax(h, 1e-12);
    b = fmin(fmax(b, 0.5 * beta), 2.0 * beta);
    b = fmin(fmax(b, 1.0 / 64.0), 64.0);
    if (!(g == g) || !(h == h)) b = beta;                                               // a NaN step keeps beta
    hdr[0] = (float)b;
}

}  // namespace

extern "C" int sir_classify(sir_handle* h, const float* logits, int batch, int num_classes, const float* inv_temperature, int k,
                            float* probs, int32_t* topk_idx, float* topk_prob, void* stream) {
    if (!h || !logits || !topk_idx || !topk_prob) { sir_set_error("sir_classify: NULL argument (h, logits, topk_idx and topk_prob are required)"); return SIR_EINVAL; }
    if (batch < 1 || batch > kMaxRows || num_classes < 1 || num_classes > 64) { sir_set_error("sir_classify: bad shape batch=%d (1..2^30) num_classes=%d (1..64)", batch, num_classes); return SIR_EINVAL; }
    if (k < 1 || k > 8 || k > num_classes) { sir_set_error("sir_classify: k=%d outside [1, min(8, num_classes=%d)]", k, num_classes); return SIR_EINVAL; }
    const uintptr_t bits = (uintptr_t)logits | (uintptr_t)inv_temperature | (uintptr_t)probs | (uintptr_t)topk_idx | (uintptr_t)topk_prob;
    if (bits & 3u) { sir_set_error("sir_classify: pointers must be 4-byte aligned"); return SIR_EINVAL; }
    hipLaunchKernelGGL(classify_kernel, dim3(classify_blocks(batch)), dim3(kClsWaves * SIR_WAVE), 0, (hipStream_t)stream, logits, batch,
                       num_classes, inv_temperature, k, probs, (int*)topk_idx, topk_prob);
    return sir_check_hip(hipGetLastError(), "classify_kernel");
}

extern "C" size_t sir_eval_state_bytes(int num_classes, int n_bins) {
    if (num_classes < 1 || num_classes > 64 || n_bins < 1 || n_bins > 64) return 0;
    return (size_t)eval_layout(num_classes, n_bins).words * 8;
}

extern "C" int sir_eval_accumulate(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                                   const float* inv_temperature, int n_bins, void* state, size_t state_bytes, void* stream) {
    if (!h || !logits || !labels || !state) { sir_set_error("sir_eval_accumulate: NULL argument"); return SIR_EINVAL; }
    if (batch < 1 || batch > kMaxRows || num_classes < 1 || num_classes > 64) { sir_set_error("sir_eval_accumulate: bad shape batch=%d (1..2^30) num_classes=%d (1..64)", batch, num_classes); return SIR_EINVAL; }
    if (n_bins < 1 || n_bins > 64) { sir_set_error("sir_eval_accumulate: n_bins=%d outside [1, 64]", n_bins); return SIR_EINVAL; }
    if ((((uintptr_t)logits | (uintptr_t)inv_temperature) & 3u) || (((uintptr_t)labels | (uintptr_t)state) & 7u)) {
        sir_set_error("sir_eval_accumulate: logits / inv_temperature must be 4-byte aligned, labels / state 8-byte aligned");
        return SIR_EINVAL;
    }
    const size_t need = sir_eval_state_bytes(num_classes, n_bins);
    if (state_bytes < need) { sir_set_error("sir_eval_accumulate: state of %zu bytes, %zu needed", state_bytes, need); return SIR_ENOMEM; }
    const int blocks = eval_blocks(batch);
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(blocks), dim3(kEvalThreads), 0, (hipStream_t)stream, logits, (const long long*)labels, batch,
                       num_classes, inv_temperature, n_bins, (unsigned long long*)state, h->status);
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, (unsigned long long*)state, num_classes, n_bins, blocks);
    return sir_check_hip(hipGetLastError(), "sir_eval_accumulate kernels");
}

extern "C" size_t sir_temperature_fit_workspace_bytes(int n_rows) {
    if (n_rows < 1 || n_rows > (1 << 22)) return 0;
    return (size_t)kFitHeader + (size_t)fit_blocks(n_rows) * 4 * sizeof(double);
}

extern "C" int sir_temperature_fit(sir_handle* h, const float* logits, const int64_t* labels, int n_rows, int num_classes, int iters,
                                   float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !logits || !labels || !out || !workspace) { sir_set_error("sir_temperature_fit: NULL argument"); return SIR_EINVAL; }
    if (n_rows < 1 || n_rows > (1 << 22) || num_classes < 1 || num_classes > 64) {
        sir_set_error("sir_temperature_fit: bad shape n_rows=%d (1..2^22) num_classes=%d (1..64)", n_rows, num_classes);
        return SIR_EINVAL;
    }
    if (iters < 0 || iters > 1000) { sir_set_error("sir_temperature_fit: iters=%d outside [0, 1000]", iters); return SIR_EINVAL; }
    if ((((uintptr_t)logits | (uintptr_t)out) & 3u) || (((uintptr_t)labels | (uintptr_t)workspace) & 7u)) {
        sir_set_error("sir_temperature_fit: logits / out must be 4-byte aligned, labels / workspace 8-byte aligned");
        return SIR_EINVAL;
    }
    const size_t need = sir_temperature_fit_workspace_bytes(n_rows);
    if (workspace_bytes < need) { sir_set_error("sir_temperature_fit: workspace of %zu bytes, %zu needed", workspace_bytes, need); return SIR_ENOMEM; }
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = fit_blocks(n_rows);
    float* hdr = (float*)workspace;
    double* partials = (double*)((char*)workspace + kFitHeader);
    for (int step = 0; step <= iters; ++step) {
        hipLaunchKernelGGL(fit_reduce_kernel, dim3(blocks), dim3(kEvalThreads), 0, st, logits, (const long long*)labels, n_rows, num_classes,
                           step > 0 ? hdr : (const float*)nullptr, partials, h->status);
        hipLaunchKernelGGL(fit_update_kernel, dim3(1), dim3(1), 0, st, partials, blocks, step < iters ? step : -1, iters, hdr, out);
    }
    return sir_check_hip(hipGetLastError(), "sir_temperature_fit kernels");
}

extern "C" int sir_classify_slots(sir_handle* h, const float* logits, int batch, int num_classes, const int32_t* slot_sizes, int n_slots,
                                  const float* inv_temperature, int k, float* probs, int32_t* topk_idx, float* topk_prob, float* joint_prob,
                                  void* stream) {
    const char* who = "sir_classify_slots";
    if (!h || !logits || !topk_idx || !topk_prob) { sir_set_error("%s: NULL argument (h, logits, topk_idx and topk_prob are required)", who); return SIR_EINVAL; }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: bad shape batch=%d (1..2^30)", who, batch); return SIR_EINVAL; }
    SlotTable tab;
    if (!sir_slots_check_layout(who, slot_sizes, n_slots, num_classes, tab.start, tab.size)) return SIR_EINVAL;
    tab.n = n_slots;
    if (k < 1 || k > 8) { sir_set_error("%s: k=%d outside [1, 8]", who, k); return SIR_EINVAL; }
    const uintptr_t bits = (uintptr_t)logits | (uintptr_t)inv_temperature | (uintptr_t)probs | (uintptr_t)topk_idx | (uintptr_t)topk_prob |
                           (uintptr_t)joint_prob;
    if (bits & 3u) { sir_set_error("%s: pointers must be 4-byte aligned", who); return SIR_EINVAL; }
    hipLaunchKernelGGL(classify_slots_kernel, dim3(classify_blocks(batch)), dim3(kClsWaves * SIR_WAVE), 0, (hipStream_t)stream, logits, batch,
                       num_classes, tab, inv_temperature, k, probs, (int*)topk_idx, topk_prob, joint_prob);
    return sir_check_hip(hipGetLastError(), "classify_slots_kernel");
}

extern "C" size_t sir_eval_slots_state_bytes(const int32_t* slot_sizes, int n_slots, int n_bins) {
    if (!slot_sizes || n_slots < 1 || n_slots > kMaxSlots || n_bins < 1 || n_bins > 64) return 0;
    long long sum = 0;
    for (int g = 0; g < n_slots; ++g) sum += slot_sizes[g] >= 1 && slot_sizes[g] <= 64 ? slot_sizes[g] : 65;
    if (sum > 64) return 0;
    EvalSlotTable tab;
    return slot_table("sir_eval_slots_state_bytes", slot_sizes, n_slots, (int)sum, n_bins, &tab) * 8;
}

extern "C" int sir_eval_accumulate_slots(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                                         const int32_t* slot_sizes, int n_slots, const float* inv_temperature, int n_bins, void* state,
                                         size_t state_bytes, void* stream) {
    const char* who = "sir_eval_accumulate_slots";
    if (!h || !logits || !labels || !state) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: bad shape batch=%d (1..2^30)", who, batch); return SIR_EINVAL; }
    if (n_bins < 1 || n_bins > 64) { sir_set_error("%s: n_bins=%d outside [1, 64]", who, n_bins); return SIR_EINVAL; }
    EvalSlotTable tab;
    const size_t need = slot_table(who, slot_sizes, n_slots, num_classes, n_bins, &tab) * 8;
    if (!need) return SIR_EINVAL;
    if ((((uintptr_t)logits | (uintptr_t)inv_temperature) & 3u) || (((uintptr_t)labels | (uintptr_t)state) & 7u)) {
        sir_set_error("%s: logits / inv_temperature must be 4-byte aligned, labels / state 8-byte aligned", who);
        return SIR_EINVAL;
    }
    if (state_bytes < need) { sir_set_error("%s: state of %zu bytes, %zu needed", who, state_bytes, need); return SIR_ENOMEM; }
    const hipStream_t st = (hipStream_t)stream;
    const int blocks = eval_blocks(batch);
    unsigned long long* words = (unsigned long long*)state;
    hipLaunchKernelGGL(eval_slots_kernel, dim3(blocks, n_slots), dim3(kEvalThreads), 0, st, logits, (const long long*)labels, batch, num_classes,
                       tab, inv_temperature, n_bins, words, h->status);
    hipLaunchKernelGGL(eval_joint_kernel, dim3(blocks), dim3(kEvalThreads), 0, st, logits, (const long long*)labels, batch, num_classes, tab,
                       inv_temperature, n_bins, words);
    hipLaunchKernelGGL(eval_slots_finish_kernel, dim3(n_slots + 1), dim3(128), 0, st, words, tab, n_bins, blocks);
    return sir_check_hip(hipGetLastError(), "sir_eval_accumulate_slots kernels");
}
