// The clip gather of sir_vad_gather and sir_stream_gather: rows of a segment table cut out of their source as zero-tailed
// float rows.  A streamed clip must equal the batch clip bit for bit, so the kernel, its launch and the output size rules exist
// once, here; the two entry points differ only in the source policy they pass by value:
//   LinearClips  whole recordings in HBM: rows of 3 x int32 {recording, first, end}, bad rows raise SIR_STATUS_VAD_ROW
//   RingClips    per-stream rings:        rows of 4 x int64 {stream, first, end, flags}, position p of a stream at ring offset
//                                         p mod (R * c), bad rows raise SIR_STATUS_STREAM_ROW
// A policy names its row type and status bit and supplies row(s), bad(row), group(row, col) -- the address of the 16 source
// bytes that start at clip column col -- and one(row, i), the sample at clip column i.
#pragma once
#include "wave_block.h"
#include "wave_sample.h"

namespace {

template <typename T> struct LinearClips {
    // a 16-byte group is loaded whole only where the launch's VEC flag vouches for the alignment of wave and stride
    static constexpr bool kAligned = false;
    static constexpr unsigned int kBadRow = SIR_STATUS_VAD_ROW;
    struct Row { int src, start, end; };
    const T* wave; long long stride; int n_rec; const int* table;
    __device__ __forceinline__ Row row(int s) const { return Row{table[s * 3LL + 0], table[s * 3LL + 1], table[s * 3LL + 2]}; }
    __device__ __forceinline__ bool bad(const Row& r) const {
        return r.src < 0 || r.src >= n_rec || r.start < 0 || r.end < r.start || (long long)r.end > stride;
    }
    __device__ __forceinline__ const T* group(const Row& r, int col) const { return wave + (long long)r.src * stride + r.start + col; }
    __device__ __forceinline__ T one(const Row& r, int i) const { return *group(r, i); }
};

template <typename T> struct RingClips {
    // the ring is 16-byte aligned and R * c is a multiple of the vector width: a group that starts at a multiple of the
    // vector width never straddles the wrap
    static constexpr bool kAligned = true;
    static constexpr unsigned int kBadRow = SIR_STATUS_STREAM_ROW;
    struct Row { long long src, start, end; };
    const T* ring; long long RC; int S; const long long* table;
    __device__ __forceinline__ Row row(int s) const { return Row{table[s * 4LL + 0], table[s * 4LL + 1], table[s * 4LL + 2]}; }
    __device__ __forceinline__ bool bad(const Row& r) const {
        return r.src < 0 || r.src >= S || r.start < 0 || r.end < r.start || r.end - r.start > RC;
    }
    __device__ __forceinline__ const T* group(const Row& r, int col) const { return ring + r.src * RC + (r.start + col) % RC; }
    __device__ __forceinline__ T one(const Row& r, int i) const { return *group(r, i); }
};

// grid (table row, column block); a thread moves 16 source bytes (8 i16 / 4 f32 samples) and zero-fills behind the clip.
// VEC: the output rows are 16-byte aligned (and, for a source that is not kAligned, the source rows too).
template <typename T, bool VEC, typename Src>
__global__ __launch_bounds__(kThreads) void clip_gather_kernel(Src src, const int* __restrict__ total, int seg_cap, float* __restrict__ out,
                                                               long long out_stride, int max_clip, int* __restrict__ out_lengths,
                                                               unsigned int* __restrict__ status) {
    constexpr int V = 16 / (int)sizeof(T);
    const int s = blockIdx.x;
    int n_valid = total[0];
    n_valid = n_valid < 0 ? 0 : (n_valid > seg_cap ? seg_cap : n_valid);
    const bool head = blockIdx.y == 0 && threadIdx.x == 0;
    if (s >= n_valid) {                                     // not a row of the table: length 0, the output row stays as it is
        if (head) out_lengths[s] = 0;
        return;
    }
    const typename Src::Row r = src.row(s);
    const bool bad = src.bad(r);
    const int len = bad ? 0 : (int)(r.end - r.start < max_clip ? r.end - r.start : max_clip);
    if (head) {
        out_lengths[s] = len;
        if (bad) __hip_atomic_fetch_or(status, Src::kBadRow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int col = (blockIdx.y * kThreads + threadIdx.x) * V;
    if (col >= max_clip) return;
    float v[V];
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = 0.0f;
    if (col < len) {
        if ((VEC || Src::kAligned) && (r.start % V) == 0 && col + V <= len) {
            alignas(16) T t[V];
            *reinterpret_cast<int4*>(t) = *reinterpret_cast<const int4*>(src.group(r, col));
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = to_f32<T>(t[e]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (col + e < len) v[e] = to_f32<T>(src.one(r, col + e));
        }
    }
    float* dst = out + (long long)s * out_stride + col;
    if (VEC && col + V <= max_clip) {
#pragma unroll
        for (int e = 0; e < V; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(v[e], v[e + 1], v[e + 2], v[e + 3]);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (col + e < max_clip) dst[e] = v[e];
    }
}

// the output-side size rules of both entry points (the last: the grid's y extent at 4 floats per thread)
bool clip_gather_sizes_ok(int seg_cap, int max_clip_len, int64_t out_stride) {
    return seg_cap > 0 && max_clip_len > 0 && out_stride >= max_clip_len && ((long long)max_clip_len + kThreads * 4 - 1) / (kThreads * 4) <= 65535;
}

// src_vec: the source rows are 16-byte aligned (always true of a kAligned source)
template <typename T, typename Src>
int clip_gather_launch(sir_handle* h, const Src& src, bool src_vec, const int32_t* total, int seg_cap, float* out, int64_t out_stride,
                       int max_clip_len, int32_t* out_lengths, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const bool vec = src_vec && (uintptr_t)out % 16 == 0 && out_stride % 4 == 0;
    const dim3 grid(seg_cap, (max_clip_len + kThreads * V - 1) / (kThreads * V));
    const auto kernel = vec ? clip_gather_kernel<T, true, Src> : clip_gather_kernel<T, false, Src>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, src, total, seg_cap, out, (long long)out_stride, max_clip_len, out_lengths, h->status);
    return sir_check_hip(hipGetLastError(), "clip_gather_kernel");
}

}  // namespace
