// Pieces shared by the two energy detectors: vad.hip (whole recordings resident in HBM) and stream.hip (live streams fed
// push by push).  A chunk must get the same energy bits whichever of the two judges it, so the accumulator, the sub-wave read
// pattern and the reduction order exist once, here; so do the rules of a sir_vad_config.  (The clip gather: clip_gather.h.)
#pragma once
#include "wave_block.h"

namespace {

__device__ __forceinline__ int clamp_len(int len, int max_len) { return len < 0 ? 0 : (len > max_len ? max_len : len); }

// ---- chunk energy ----------------------------------------------------------------------------------------------------------
// A chunk is read by a sub-wave of LPC lanes, 16 bytes per lane and step, 64 samples per step (chunk_size is a multiple of 64):
// i16 -> 8 lanes x 8 samples, 8 chunks per pass of a wave; f32 -> 16 lanes x 4 samples, 4 chunks per pass.  Reduction order (fixed):
//   i16: exact integer sum of |s| (<= 4096 * 32768 = 2^27), e = (float)((double)S / (count * 32768.0))
//   f32: lane: four accumulators, one per vector component, each a chain over the steps; (a0 + a1) + (a2 + a3); xor butterfly
//        over the 16 lanes (distance 1, 2, 4, 8: the same bits in every lane, fp add commutes); e = sum / (float)count.
//        Additions on the longest path: chunk_size / 64 (chain) + 2 + 4 (tree).
// Samples behind the chunk's count enter as +0 (no rounding); a vector load is issued only where all its samples exist.
template <typename T> struct Acc;
template <> struct Acc<short> {
    int s = 0;
    __device__ __forceinline__ void add_vec(const void* p) {
        const int4 v = *reinterpret_cast<const int4*>(p);
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lo = (int)(short)(w[i] & 0xffff), hi = w[i] >> 16;
            s += (lo < 0 ? -lo : lo) + (hi < 0 ? -hi : hi);
        }
    }
    __device__ __forceinline__ void add_one(int, short x) { const int v = x; s += v < 0 ? -v : v; }
    __device__ __forceinline__ float finish(int lpc, int count) {
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) s += __shfl_xor(s, m);
        (void)lpc;
        return (float)((double)s / ((double)count * 32768.0));
    }
};
template <> struct Acc<float> {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    __device__ __forceinline__ void add_vec(const void* p) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        a[0] = __fadd_rn(a[0], fabsf(v.x)); a[1] = __fadd_rn(a[1], fabsf(v.y));
        a[2] = __fadd_rn(a[2], fabsf(v.z)); a[3] = __fadd_rn(a[3], fabsf(v.w));
    }
    __device__ __forceinline__ void add_one(int e, float x) {
        const float v = fabsf(x);                            // e is a compile-time constant after unrolling
        if (e == 0) a[0] = __fadd_rn(a[0], v);
        else if (e == 1) a[1] = __fadd_rn(a[1], v);
        else if (e == 2) a[2] = __fadd_rn(a[2], v);
        else a[3] = __fadd_rn(a[3], v);
    }
    __device__ __forceinline__ float finish(int, int count) {
        float s = __fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[2], a[3]));
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) s = __fadd_rn(s, __shfl_xor(s, m));
        return __fdiv_rn(s, (float)count);
    }
};

// One lane's share of one chunk: `p` is the lane's first sample (chunk + sl * V, sl = the lane's index in its sub-wave), `left`
// the samples of the chunk at or behind it (count - sl * V), `steps` = chunk_size / 64.
template <typename T, bool VEC>
__device__ __forceinline__ void chunk_accumulate(Acc<T>& acc, const T* p, int left, int steps) {
    constexpr int V = 16 / (int)sizeof(T);      // samples per 16-byte load
#pragma unroll 4
    for (int s = 0; s < steps; ++s, p += 64, left -= 64) {
        if (VEC && left >= V) {
            acc.add_vec(p);
        } else if (left > 0) {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (e < left) acc.add_one(e, p[e]);
        }
    }
}

// ---- block scans -----------------------------------------------------------------------------------------------------------
// inclusive scans over the 256 threads of the block: wave scan by shuffles, the four wave totals through LDS
__device__ __forceinline__ int wave_incl_add(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}
// exclusive prefix sum of v over the block; *total = the block's sum.  `sh` holds kWaves ints and is free again on return.
__device__ __forceinline__ int block_excl_add(int v, int* sh, int* total) {
    const int incl = wave_incl_add(v);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) sh[wv] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) { const int t = sh[i]; if (i < wv) off += t; tot += t; }
    __syncthreads();
    *total = tot;
    return off + incl - v;
}

// ---- config rules (host) ---------------------------------------------------------------------------------------------------
bool chunk_ok(int c) { return c >= 64 && c <= 4096 && c % 64 == 0; }

// the rules of a sir_vad_config, for sir_vad_segment and sir_stream_*; a failure is reported in who's name (NULL: silently)
bool vad_config_ok(const char* who, const sir_vad_config& v) {
    if (!chunk_ok(v.chunk_size)) {
        if (who) sir_set_error("%s: chunk_size %d is not a multiple of 64 in [64, 4096]", who, v.chunk_size);
        return false;
    }
    if (!(v.threshold >= 0.0f) || v.silence_chunks < 0 || v.prior_chunks < 0) {
        if (who) sir_set_error("%s: bad config (threshold %g must be >= 0 and not NaN, silence_chunks %d and prior_chunks %d >= 0)", who,
                               (double)v.threshold, v.silence_chunks, v.prior_chunks);
        return false;
    }
    return true;
}

}  // namespace
