// Slot heads, joint decoding (include/sir_hip.h: sir_decode_slots): the k best label TUPLES of a logit row read as several
// softmax segments -- over a table of the tuples that exist (constrained), or over the whole product space (unconstrained).
//
// The map is classify_slots_kernel's: ONE WAVE OWNS A ROW, kClsWaves rows per workgroup, grid-stride over the rows.  Per slot the
// wave forms row_softmax (row_softmax.h -- the function sir_classify_slots and sir_eval_accumulate_slots stand on) and from it
// the log-probabilities lp_g[c] = d_c - log1pf(rest_g): the fp32 terms of sir_eval_accumulate_slots' joint NLL, negated.  A
// tuple's score is s_t = lp_0[t_0] + lp_1[t_1] + ... in fp32, slot order, no fma (there is no product to fuse: the pragma
// below keeps the subtraction that forms lp away from the product inside d).
//
// Constrained: the row's <= 64 log-probabilities go to the wave's slab of LDS; the table (uint8 [n][8], one 64-bit load per
// tuple, <= 32 KB, read by every wave: it lives in L2) is scanned lane-strided, t = lane, lane + 64, ...  The table is read
// ONCE per row: scan 0 leaves every score in the wave's slab (n floats behind the log-probabilities, NaN for a tuple that is not
// valid; 4 x (64 + 4096) floats = 65 KB per workgroup at the largest table, dynamic LDS sized by the table), and the later scans
// read LDS only -- recomputing cost a dependent L2 load per tuple and scan, 108 us against 46 us at 4096 rows x batch 256.
// A lane reads back only what it wrote itself, so the scans need no barrier between them.  The scans:
//   scan 0     : scores into LDS; every lane keeps its best (score, row); a wave argmax gives rank 0, whose score is the
//                maximum M.  It also writes tuple_logp and raises the status word for a table byte >= C_g.
//   sum        : every lane adds expf(s_t - M) over its tuples in scan order, the lanes' sums are added by the xor butterfly
//                (fixed order: bit-reproducible); L = M + logf(sum).
//   scan r > 0 : the best (score, row) that comes strictly AFTER rank r - 1 in the order (descending score, ascending row).  The
//                order is total, so "after the previous winner" is the whole memory of the earlier ranks: no per-lane lists,
//                no dynamically indexed registers, no scratch.
// A tuple with a byte >= C_g is never eligible and takes no part in the sum; its LDS index is clamped into the slot, so no lane
// reads outside the row's log-probabilities whatever the table holds.
//
// Unconstrained: staged merging, exact for sums over independent lists (fp32 addition is monotone: a >= b => a + c >= b + c
// after rounding).  Lane i < n_part holds the i-th best partial tuple over slots 0 .. g - 1 (score, mixed-radix index, packed
// labels); lane j < min(k, C_g) holds slot g's rank-j label, sir_classify's ranking.  Lane 8 i + j is candidate (partial i,
// label j) -- at most 64 -- and a candidate's rank is counted as row_softmax counts a class's: the candidates that beat it,
// by a larger score or an equal one in a lower lane (partial rank major, slot rank minor).  The candidates of rank < k move to
// lanes 0 .. k - 1 and go on.
#include <cmath>
#include "row_softmax.h"

namespace {

constexpr int kMaxTuples = 4096;
constexpr int kNoRow = 0x7fffffff;
constexpr int kScanDepth = 8;                        // table loads a lane issues back to back in scan 0

// floats of a wave's LDS slab: the row's 64 log-probabilities, then one score per tuple
__host__ __device__ inline int decode_slab_floats(int n_tuples) { return 64 + (n_tuples + 63) / 64 * 64; }

struct DecodeOut {
    int* index;            // [B][k]
    int* labels;           // [B][k][G]
    float* logp;           // [B][k]
    float* prob;           // [B][k]
    float* mass;           // [B] or NULL
    float* tuple_logp;     // [B][n_tuples] or NULL
};

__device__ __forceinline__ float slot_logp(const RowSoftmax& r) {
#pragma clang fp contract(off)                                                           // d's product stays a rounded product
    return r.d - log1pf(r.rest);
}

// rank `rank` of row b: table row / mixed-radix index `index` (-1: no such rank), its labels packed one byte per slot
__device__ __forceinline__ void write_rank(const DecodeOut& o, int b, int k, int G, int rank, int lane, int index,
                                           unsigned long long packed, float logp, float prob) {
    const size_t at = (size_t)b * k + rank;
    if (lane == 0) { o.index[at] = index; o.logp[at] = logp; o.prob[at] = prob; }
    if (lane < G) o.labels[at * G + lane] = index < 0 ? -1 : (int)((packed >> (8 * lane)) & 0xffull);
}

// a row with a NaN or an infinity in some segment: every output of the row is -1 / NaN
__device__ __forceinline__ void write_nonfinite_row(const DecodeOut& o, int b, int k, int G, int lane, int n_tuples) {
    const float nan = __builtin_nanf("");
    if (lane < k) { o.index[(size_t)b * k + lane] = -1; o.logp[(size_t)b * k + lane] = nan; o.prob[(size_t)b * k + lane] = nan; }
    for (int i = lane; i < k * G; i += SIR_WAVE) o.labels[(size_t)b * k * G + i] = -1;
    if (o.mass && lane == 0) o.mass[b] = nan;
    if (o.tuple_logp)
        for (int t = lane; t < n_tuples; t += SIR_WAVE) o.tuple_logp[(size_t)b * n_tuples + t] = nan;
}

// the better of two (score, row) pairs: larger score, then lower row; kNoRow = no candidate
__device__ __forceinline__ void keep_better(float& s, int& t, float s2, int t2) {
    const bool take = t2 != kNoRow && (t == kNoRow || s2 > s || (s2 == s && t2 < t));
    if (take) { s = s2; t = t2; }
}

// score of table entry `w` from the wave's log-probabilities; false: some byte g < G is >= C_g (the score is then -inf)
__device__ __forceinline__ bool tuple_score(const SlotTable& tab, const float* lp, unsigned long long w, float& s) {
#pragma clang fp contract(off)
    bool ok = true;
    float acc = 0.0f;
    for (int g = 0; g < tab.n; ++g) {                                                    // wave-uniform trip count
        const int c = (int)((w >> (8 * g)) & 0xffull), C = tab.size[g];
        ok = ok && c < C;
        const float v = lp[tab.start[g] + (c < C ? c : C - 1)];                          // always inside the row's segment g
        acc = g == 0 ? v : acc + v;
    }
    s = ok ? acc : -INFINITY;
    return ok;
}

__global__ __launch_bounds__(kClsWaves * SIR_WAVE) void decode_table_kernel(const float* __restrict__ logits, int B, int NC, SlotTable tab,
                                                                             const float* __restrict__ inv_t,
                                                                             const unsigned long long* __restrict__ tuples, int n_tuples, int k,
                                                                             DecodeOut o, unsigned int* status) {
    extern __shared__ float s_decode[];                                                   // per wave: lp[64], score[n rounded up to 64]
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const int G = tab.n;
    float* lp = s_decode + (size_t)wave * decode_slab_floats(n_tuples);
    float* sc = lp + 64;
    const float nan = __builtin_nanf("");
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {      // wave-uniform
        bool finite = true;
        wave_fence();                                                                    // the previous row's reads are done
        for (int g = 0; g < G; ++g) {
            const int start = tab.start[g], C = tab.size[g];
            const float l = lane < C ? logits[(size_t)b * NC + start + lane] : 0.0f;
            const RowSoftmax r = row_softmax(l, lane, C, inv_t ? inv_t[g] : 1.0f);
            finite = finite && r.finite;
            if (lane < C) lp[start + lane] = slot_logp(r);
        }
        wave_fence();
        if (!finite) { write_nonfinite_row(o, b, k, G, lane, n_tuples); continue; }

        // scan 0: rank 0, all scores, the table check
        float best_s = 0.0f;
        int best_t = kNoRow;
        bool bad = false;
        for (int t0 = lane; t0 < n_tuples; t0 += kScanDepth * SIR_WAVE) {
            // kScanDepth table loads in flight before the first is used: a wave alone on its SIMD pays an L2 latency per
            // dependent load otherwise
            unsigned long long w[kScanDepth];
#pragma unroll
            for (int j = 0; j < kScanDepth; ++j) {
                const int t = t0 + j * SIR_WAVE;
                w[j] = t < n_tuples ? tuples[t] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < kScanDepth; ++j) {
                const int t = t0 + j * SIR_WAVE;
                if (t < n_tuples) {
                    float s;
                    const bool ok = tuple_score(tab, lp, w[j], s);
                    bad = bad || !ok;
                    sc[t] = ok ? s : nan;
                    if (o.tuple_logp) o.tuple_logp[(size_t)b * n_tuples + t] = s;
                    if (ok) keep_better(best_s, best_t, s, t);                           // ascending t: an equal score keeps the lower row
                }
            }
        }
        if (__ballot(bad) != 0ull && lane == 0)
            __hip_atomic_fetch_or(status, SIR_STATUS_DECODE_TUPLE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) keep_better(best_s, best_t, __shfl_xor(best_s, off), __shfl_xor(best_t, off));
        best_s = __shfl(best_s, 0);                                                      // (a NaN beta: the lanes may disagree)
        best_t = __shfl(best_t, 0);

        // L = logsumexp over the valid tuples = M + log(sum exp(s - M)), M = rank 0's score
        const float M = best_s;
        float L = -INFINITY;
        if (best_t != kNoRow && M > -INFINITY) {
            float part = 0.0f;
#pragma unroll 8
            for (int t = lane; t < n_tuples; t += SIR_WAVE) {                            // (unrolled: the LDS reads go out together)
                const float s = sc[t];
                if (s == s) part += expf(s - M);
            }
            L = M + logf(wave_sum(part));
        }
        if (o.mass && lane == 0) o.mass[b] = expf(L);

        for (int r = 0; r < k; ++r) {                                                    // wave-uniform
            if (r > 0 && best_t != kNoRow) {                                             // the best entry after (best_s, best_t) in the order
                const float ps = best_s;
                const int pt = best_t;
                best_t = kNoRow;
#pragma unroll 8
                for (int t = lane; t < n_tuples; t += SIR_WAVE) {
                    const float s = sc[t];                                               // (NaN, a tuple that is not valid: never eligible)
                    if (s < ps || (s == ps && t > pt)) keep_better(best_s, best_t, s, t);
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) keep_better(best_s, best_t, __shfl_xor(best_s, off), __shfl_xor(best_t, off));
                best_s = __shfl(best_s, 0);
                best_t = __shfl(best_t, 0);
            }
            if (best_t == kNoRow) { write_rank(o, b, k, G, r, lane, -1, 0ull, -INFINITY, 0.0f); continue; }
            write_rank(o, b, k, G, r, lane, best_t, tuples[best_t], best_s, L > -INFINITY ? expf(best_s - L) : 0.0f);
        }
    }
}

__global__ __launch_bounds__(kClsWaves * SIR_WAVE) void decode_product_kernel(const float* __restrict__ logits, int B, int NC, SlotTable tab,
                                                                               const float* __restrict__ inv_t, int k, DecodeOut o) {
    const int lane = threadIdx.x & (SIR_WAVE - 1), wave = threadIdx.x / SIR_WAVE;
    const int G = tab.n;
    for (int b = blockIdx.x * kClsWaves + wave; b < B; b += gridDim.x * kClsWaves) {      // wave-uniform
        bool finite = true;
        int n_part = 0;                                                                  // partial tuples held, lanes 0 .. n_part - 1
        float part_s = 0.0f;
        int part_i = 0;
        unsigned long long part_l = 0ull;
        for (int g = 0; g < G; ++g) {
            const int start = tab.start[g], C = tab.size[g];
            const float l = lane < C ? logits[(size_t)b * NC + start + lane] : 0.0f;
            const RowSoftmax r = row_softmax(l, lane, C, inv_t ? inv_t[g] : 1.0f);
            finite = finite && r.finite;
            const float mine = slot_logp(r);
            // lane j < kk: the slot's rank-j label and its log-probability
            const int kk = k < C ? k : C;
            float slot_s = 0.0f;
            int slot_c = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned long long m = __ballot(lane < C && r.rank == j);          // one lane on a finite row
                const int src = m ? __ffsll((long long)m) - 1 : 0;
                const float v = __shfl(mine, src);
                if (lane == j) { slot_s = v; slot_c = src; }
            }
            if (g == 0) {
                n_part = kk;
                part_s = slot_s;
                part_i = slot_c;
                part_l = (unsigned long long)slot_c;
                continue;
            }
            // candidate (i, j) in lane 8 i + j
            const int i = lane >> 3, j = lane & 7;
            const bool on = i < n_part && j < kk;
            const float ps = __shfl(part_s, i), ss = __shfl(slot_s, j);
            const int pi = __shfl(part_i, i), sc = __shfl(slot_c, j);
            const unsigned long long pl = ((unsigned long long)(unsigned)__shfl((int)(part_l >> 32), i) << 32) |
                                          (unsigned long long)(unsigned)__shfl((int)(part_l & 0xffffffffull), i);
            float cand_s;
            {
#pragma clang fp contract(off)
                cand_s = ps + ss;
            }
            const int cand_i = pi * C + sc;
            const unsigned long long cand_l = pl | ((unsigned long long)sc << (8 * g));
            int rank = 0;
            for (int q = 0; q < SIR_WAVE; ++q) {
                const float sq = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand_s), q));
                const bool onq = (q >> 3) < n_part && (q & 7) < kk;                      // wave-uniform
                rank += (onq && (sq > cand_s || (sq == cand_s && q < lane))) ? 1 : 0;
            }
            const int total = n_part * kk;
            const int n_next = k < total ? k : total;
            float ns = 0.0f;
            int ni = 0;
            unsigned long long nl = 0ull;
            int found = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned long long m = __ballot(on && rank == q);
                const int src = m ? __ffsll((long long)m) - 1 : 0;
                const float vs = __shfl(cand_s, src);
                const int vi = __shfl(cand_i, src);
                const int lo = __shfl((int)(cand_l & 0xffffffffull), src), hi = __shfl((int)(cand_l >> 32), src);
                if (lane == q) { ns = vs; ni = vi; nl = ((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo; }
                found += (m != 0ull && q < n_next && found == q) ? 1 : 0;                // ranks present without a hole (a NaN beta leaves holes)
            }
            n_part = found;
            part_s = ns; part_i = ni; part_l = nl;
        }
        if (!finite) { write_nonfinite_row(o, b, k, G, lane, 0); continue; }
        for (int r = 0; r < k; ++r) {                                                    // wave-uniform
            if (r >= n_part) { write_rank(o, b, k, G, r, lane, -1, 0ull, -INFINITY, 0.0f); continue; }
            const float s = __shfl(part_s, r);
            const int idx = __shfl(part_i, r);
            const unsigned long long pl = ((unsigned long long)(unsigned)__shfl((int)(part_l >> 32), r) << 32) |
                                          (unsigned long long)(unsigned)__shfl((int)(part_l & 0xffffffffull), r);
            write_rank(o, b, k, G, r, lane, idx, pl, s, expf(s));
        }
        if (o.mass && lane == 0) o.mass[b] = 1.0f;
    }
}

}  // namespace

extern "C" int sir_decode_slots(sir_handle* h, const float* logits, int batch, int num_classes, const int32_t* slot_sizes, int n_slots,
                                const float* inv_temperature, const uint8_t* tuples, int n_tuples, int k, int32_t* best_index,
                                int32_t* best_labels, float* best_logp, float* best_prob, float* valid_mass, float* tuple_logp, void* stream) {
    const char* who = "sir_decode_slots";
    if (!h || !logits || !best_index || !best_labels || !best_logp || !best_prob) {
        sir_set_error("%s: NULL argument (h, logits, best_index, best_labels, best_logp and best_prob are required)", who);
        return SIR_EINVAL;
    }
    if (batch < 1 || batch > kMaxRows) { sir_set_error("%s: bad shape batch=%d (1..2^30)", who, batch); return SIR_EINVAL; }
    SlotTable tab;
    if (!sir_slots_check_layout(who, slot_sizes, n_slots, num_classes, tab.start, tab.size)) return SIR_EINVAL;
    tab.n = n_slots;
    if (k < 1 || k > 8) { sir_set_error("%s: k=%d outside [1, 8]", who, k); return SIR_EINVAL; }
    if (tuples) {
        if (n_tuples < 1 || n_tuples > kMaxTuples) { sir_set_error("%s: n_tuples=%d outside [1, %d]", who, n_tuples, kMaxTuples); return SIR_EINVAL; }
        if ((uintptr_t)tuples & 7u) { sir_set_error("%s: the tuple table must be 8-byte aligned", who); return SIR_EINVAL; }
    } else {
        if (n_tuples != 0) { sir_set_error("%s: n_tuples=%d without a table (unconstrained decoding takes 0)", who, n_tuples); return SIR_EINVAL; }
        if (tuple_logp) { sir_set_error("%s: tuple_logp needs a tuple table", who); return SIR_EINVAL; }
    }
    const uintptr_t bits = (uintptr_t)logits | (uintptr_t)inv_temperature | (uintptr_t)best_index | (uintptr_t)best_labels |
                           (uintptr_t)best_logp | (uintptr_t)best_prob | (uintptr_t)valid_mass | (uintptr_t)tuple_logp;
    if (bits & 3u) { sir_set_error("%s: pointers must be 4-byte aligned", who); return SIR_EINVAL; }
    const DecodeOut o{(int*)best_index, (int*)best_labels, best_logp, best_prob, valid_mass, tuple_logp};
    const dim3 grid(classify_blocks(batch)), block(kClsWaves * SIR_WAVE);
    if (tuples) {
        const size_t lds = (size_t)kClsWaves * decode_slab_floats(n_tuples) * sizeof(float);
        SIR_TRY(sir_lds_opt_in(h, (const void*)decode_table_kernel, (int)(kClsWaves * decode_slab_floats(kMaxTuples) * sizeof(float))));
        hipLaunchKernelGGL(decode_table_kernel, grid, block, lds, (hipStream_t)stream, logits, batch, num_classes, tab, inv_temperature,
                           (const unsigned long long*)tuples, n_tuples, k, o, h->status);
    } else
        hipLaunchKernelGGL(decode_product_kernel, grid, block, 0, (hipStream_t)stream, logits, batch, num_classes, tab, inv_temperature, k, o);
    return sir_check_hip(hipGetLastError(), "sir_decode_slots kernel");
}
