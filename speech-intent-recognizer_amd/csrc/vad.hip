// Utterance segmentation of long recordings (sir_vad_segment, sir_vad_gather): the energy detector of the reference's
// continuous-audio recogniser (scripts/testing.py:38-133) for a whole batch of recordings resident in HBM.
//
//   1. vad_energy_kernel   one read of every sample: mean |x| per chunk -> packed speech flags (and, optionally, the energies)
//   2. vad_segment_kernel  the listener's state machine in its data-parallel form, one workgroup per recording, run twice:
//                          <false> counts the segments, vad_base_kernel turns the counts into base rows, <true> writes the table
//   3. clip_gather_kernel  cuts the segments out as zero-tailed float rows (clip_gather.h, shared with sir_stream_gather)
//
// The state machine (testing.py:84-133) only ever looks at `last`, the index of the latest speech chunk:
//   trigger at i : speech_i and (no speech chunk before i, or i - last_before(i) > n_stop)
//   end at j     : last_upto(j) == j - n_stop          (n_stop == 0: every speech chunk ends its own segment)
// `last` is a prefix maximum, the k-th trigger pairs with the k-th end, so prefix sums of the two flag kinds number the rows.
// No atomics anywhere on the numbering path: the table order is part of the contract and every output is bit-reproducible.
#include "clip_gather.h"
#include "vad_common.h"

#include <math.h>

namespace {


// ---- 1. chunk energy -------------------------------------------------------------------------------------------------------
// One wave owns one 32-bit flag word = 32 consecutive chunks of one recording.  The accumulator, the sub-wave read pattern and the
// reduction order are those of vad_common.h (shared with the live-stream detector, stream.hip).
// Samples behind the recording's length enter as +0 (no rounding); a vector load is issued only where all its samples exist.

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void vad_energy_kernel(const T* __restrict__ wave, long long stride, const int* __restrict__ lengths,
                                                              long long n_tasks, int max_len, int c, float threshold, int max_chunks,
                                                              int wpr, float* __restrict__ energy_out, unsigned int* __restrict__ flags) {
    constexpr int V = 16 / (int)sizeof(T);      // samples per 16-byte load
    constexpr int LPC = 64 / V;                 // lanes per chunk
    constexpr int CPP = SIR_WAVE / LPC;         // chunks per pass of the wave
    const long long task = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (task >= n_tasks) return;                // wave-uniform
    const int r = (int)(task / wpr), w = (int)(task - (long long)r * wpr);
    const int lane = threadIdx.x & 63, sub = lane / LPC, sl = lane - sub * LPC;
    const int len = clamp_len(lengths[r], max_len);
    const int nch = (int)(((long long)len + c - 1) / c);
    const T* row = wave + (long long)r * stride;
    float* erow = energy_out ? energy_out + (size_t)r * max_chunks : nullptr;
    unsigned int word = 0;
    if (w * 32 < nch) {                         // wave-uniform
        const int steps = c / 64;
        for (int pass = 0; pass < 32 / CPP; ++pass) {
            const int k = w * 32 + pass * CPP + sub;
            Acc<T> acc;
            int count = 1;
            if (k < nch) {
                const long long begin = (long long)k * c;
                const long long rest = (long long)len - begin;
                count = rest < c ? (int)rest : c;
                chunk_accumulate<T, VEC>(acc, row + begin + sl * V, count - sl * V, steps);
            }
            const float e = acc.finish(LPC, count);               // every lane takes part in the butterfly
            const bool live = k < nch;
            const bool speech = live && e > threshold;            // strict, in float (testing.py:44-47); NaN is silence
            const unsigned long long b = __ballot(speech);
#pragma unroll
            for (int j = 0; j < CPP; ++j) word |= (unsigned int)((b >> (j * LPC)) & 1ull) << (pass * CPP + j);
            if (erow && sl == 0 && k < max_chunks) erow[k] = live ? e : 0.0f;
        }
    } else if (erow) {
        const int k = w * 32 + lane;
        if (lane < 32 && k < max_chunks) erow[k] = 0.0f;
    }
    if (lane == 0) flags[(size_t)r * wpr + w] = word;
}

// ---- 2. segmentation -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_incl_max(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v = o > v ? o : v; }
    return v;
}
// exclusive prefix maximum (identity -1); *total = the block's maximum
__device__ __forceinline__ int block_excl_max(int v, int* sh, int* total) {
    const int incl = wave_incl_max(v);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) sh[wv] = incl;
    __syncthreads();
    int off = -1, tot = -1;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) { const int t = sh[i]; if (i < wv) off = t > off ? t : off; tot = t > tot ? t : tot; }
    __syncthreads();
    int prev = __shfl_up(incl, 1);
    if ((threadIdx.x & 63) == 0) prev = -1;
    *total = tot;
    return prev > off ? prev : off;
}

// One thread walks the 32 chunks of its flag word from the `last` the prefix maximum hands it.  on_trigger(i) / on_end(j) are
// called in chunk order.  A silent word holds at most one event, the end at last + n_stop.
template <typename FT, typename FE>
__device__ __forceinline__ void walk_word(unsigned int bits, int w, int n, int last, int n_stop, FT on_trigger, FE on_end) {
    const int i0 = w * 32;
    if (i0 >= n) return;
    const int i1 = n - i0 < 32 ? n : i0 + 32;
    if (bits == 0) {
        if (last >= 0) {
            const long long j = (long long)last + n_stop;
            if (j >= i0 && j < i1) on_end((int)j);
        }
        return;
    }
    for (int i = i0; i < i1; ++i) {
        if ((bits >> (i - i0)) & 1u) {
            if (last < 0 || (long long)i - last > n_stop) on_trigger(i);
            last = i;
        }
        if (last >= 0 && (long long)i - last == n_stop) on_end(i);
    }
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void vad_segment_kernel(const unsigned int* __restrict__ flags, const int* __restrict__ lengths,
                                                               int max_len, int c, int wpr, int n_stop, int prior, int flush,
                                                               int* __restrict__ seg_count, const int* __restrict__ base,
                                                               int* __restrict__ table, int seg_cap) {
    __shared__ int sh[kWaves];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int len = clamp_len(lengths[r], max_len);
    const int n = (int)(((long long)len + c - 1) / c);
    const int nwords = (n + 31) / 32;
    const long long row0 = WRITE ? (long long)base[r] : 0;
    // segments of this recording: WRITE reads the count its own <false> run left (a trigger without an end is dropped by it)
    const int count = WRITE ? seg_count[r] : 0;
    int carry_last = -1, carry_t = 0, carry_e = 0;      // block-uniform: state behind the tiles done so far
    for (int tile = 0; tile < nwords; tile += kThreads) {
        const int w = tile + tid;
        const unsigned int bits = w < nwords ? flags[(size_t)r * wpr + w] : 0u;
        const int mine = bits ? w * 32 + 31 - __clz((int)bits) : -1;
        int tile_last;
        int last = block_excl_max(mine, sh, &tile_last);
        last = last > carry_last ? last : carry_last;
        int nt = 0, ne = 0;
        walk_word(bits, w, n, last, n_stop, [&](int) { ++nt; }, [&](int) { ++ne; });
        int tot_t, tot_e;
        const int off_t = block_excl_add(nt, sh, &tot_t);
        const int off_e = block_excl_add(ne, sh, &tot_e);
        if (WRITE) {
            int kt = carry_t + off_t, ke = carry_e + off_e;
            walk_word(bits, w, n, last, n_stop,
                      [&](int i) {
                          const long long row = row0 + kt;
                          if (kt < count && row < seg_cap) {
                              const int first = prior >= 1 ? (i - prior + 1 > 0 ? i - prior + 1 : 0) : i;
                              table[row * 3 + 0] = r;
                              table[row * 3 + 1] = first * c;
                          }
                          ++kt;
                      },
                      [&](int j) {
                          const long long row = row0 + ke;
                          if (row < seg_cap) {
                              const long long e = ((long long)j + 1) * c;
                              table[row * 3 + 2] = e < len ? (int)e : len;
                          }
                          ++ke;
                      });
        }
        carry_last = tile_last > carry_last ? tile_last : carry_last;
        carry_t += tot_t;
        carry_e += tot_e;
    }
    // an utterance still open when the recording stops: the reference drops it; flush_tail ends it at the recording's length
    const bool open = carry_last >= 0 && (long long)carry_last + n_stop >= n;
    if (tid == 0) {
        if (!WRITE) {
            seg_count[r] = carry_e + ((open && flush) ? 1 : 0);
        } else if (open && flush) {
            const long long row = row0 + carry_e;
            if (row < seg_cap) table[row * 3 + 2] = len;
        }
    }
}

// base[r] = sum of seg_count[0..r), total[0] = the sum of all: one block, a contiguous slice per thread
__global__ __launch_bounds__(kThreads) void vad_base_kernel(const int* __restrict__ seg_count, int n_rec, int* __restrict__ base,
                                                            int* __restrict__ total) {
    __shared__ int sh[kWaves];
    const int per = (n_rec + kThreads - 1) / kThreads;
    const int b = threadIdx.x * per, e = b + per < n_rec ? b + per : n_rec;
    int s = 0;
    for (int i = b; i < e; ++i) s += seg_count[i];
    int tot;
    int run = block_excl_add(s, sh, &tot);
    for (int i = b; i < e; ++i) { base[i] = run; run += seg_count[i]; }
    if (threadIdx.x == 0) total[0] = tot;
}

struct WsLayout { int wpr, max_chunks; size_t flags_off, base_off, total; };

WsLayout ws_layout(int n_rec, int max_len, int c) {
    WsLayout w;
    w.max_chunks = (int)(((long long)max_len + c - 1) / c);
    w.wpr = (w.max_chunks + 31) / 32;
    w.flags_off = 0;
    w.base_off = sir_align_up((size_t)n_rec * w.wpr * sizeof(unsigned int), 256);
    w.total = sir_align_up(w.base_off + (size_t)n_rec * sizeof(int), 256);
    return w;
}

template <typename T>
int segment_impl(sir_handle* h, const T* wave, int64_t wave_stride, const int32_t* lengths, int n_rec, int max_len, const sir_vad_config* cfg,
                 float* energy_out, int32_t* seg_count, int32_t* seg_table, int seg_cap, int32_t* total, void* workspace, hipStream_t st) {
    const WsLayout w = ws_layout(n_rec, max_len, cfg->chunk_size);
    unsigned int* flags = (unsigned int*)((char*)workspace + w.flags_off);
    int* base = (int*)((char*)workspace + w.base_off);
    const long long n_tasks = (long long)n_rec * w.wpr;
    const unsigned int blocks = (unsigned int)((n_tasks + kWaves - 1) / kWaves);
    const bool vec = (uintptr_t)wave % 16 == 0 && ((long long)wave_stride * (long long)sizeof(T)) % 16 == 0;
    {
        SirProfScope prof(h, SIR_K_VAD_ENERGY, st);
        if (vec)
            hipLaunchKernelGGL((vad_energy_kernel<T, true>), dim3(blocks), dim3(kThreads), 0, st, wave, (long long)wave_stride, lengths, n_tasks,
                               max_len, cfg->chunk_size, cfg->threshold, w.max_chunks, w.wpr, energy_out, flags);
        else
            hipLaunchKernelGGL((vad_energy_kernel<T, false>), dim3(blocks), dim3(kThreads), 0, st, wave, (long long)wave_stride, lengths, n_tasks,
                               max_len, cfg->chunk_size, cfg->threshold, w.max_chunks, w.wpr, energy_out, flags);
        SIR_TRY(sir_check_hip(hipGetLastError(), "vad_energy_kernel"));
    }
    SirProfScope prof(h, SIR_K_VAD_SEGMENT, st);
    const int flush = cfg->flush_tail != 0 ? 1 : 0;
    hipLaunchKernelGGL(vad_segment_kernel<false>, dim3(n_rec), dim3(kThreads), 0, st, flags, lengths, max_len, cfg->chunk_size, w.wpr,
                       cfg->silence_chunks, cfg->prior_chunks, flush, seg_count, (const int*)nullptr, (int*)nullptr, 0);
    SIR_TRY(sir_check_hip(hipGetLastError(), "vad_segment_kernel (count)"));
    hipLaunchKernelGGL(vad_base_kernel, dim3(1), dim3(kThreads), 0, st, seg_count, n_rec, base, total);
    SIR_TRY(sir_check_hip(hipGetLastError(), "vad_base_kernel"));
    if (seg_cap > 0) {
        hipLaunchKernelGGL(vad_segment_kernel<true>, dim3(n_rec), dim3(kThreads), 0, st, flags, lengths, max_len, cfg->chunk_size, w.wpr,
                           cfg->silence_chunks, cfg->prior_chunks, flush, seg_count, base, seg_table, seg_cap);
        SIR_TRY(sir_check_hip(hipGetLastError(), "vad_segment_kernel (write)"));
    }
    return SIR_OK;
}

}  // namespace

extern "C" int sir_vad_stop_chunks(int sample_rate, int chunk_size, double silence_limit) {
    if (sample_rate <= 0 || chunk_size <= 0 || !(silence_limit >= 0.0) || isinf(silence_limit)) return -1;
    // the listener's own test (testing.py:110-111), `silence_chunks * (chunk_size / sample_rate) >= silence_limit`, in double as
    // Python evaluates it: start a little below the quotient and walk up to the first count that passes
    const double per = (double)chunk_size / (double)sample_rate;
    const double guess = floor(silence_limit / per) - 2.0;
    if (guess > 1.0e9) return -1;
    int n = guess > 0.0 ? (int)guess : 0;
    while ((double)n * per < silence_limit) ++n;
    return n;
}

extern "C" size_t sir_vad_workspace_bytes(const sir_handle* h, int n_rec, int max_len, int chunk_size) {
    if (!h || n_rec <= 0 || max_len <= 0 || !chunk_ok(chunk_size)) return 0;
    return ws_layout(n_rec, max_len, chunk_size).total;
}

extern "C" int sir_vad_segment(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int n_rec,
                               int max_len, const sir_vad_config* cfg, float* energy_out, int32_t* seg_count, int32_t* seg_table, int seg_cap,
                               int32_t* total, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !wave || !lengths || !cfg || !seg_count || !total || !workspace || (seg_cap > 0 && !seg_table)) {
        sir_set_error("sir_vad_segment: NULL argument");
        return SIR_EINVAL;
    }
    if (!sir_wave_elem_bytes(wave_dtype)) { sir_set_error("sir_vad_segment: bad wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (n_rec <= 0 || max_len <= 0 || wave_stride < max_len || seg_cap < 0) {
        sir_set_error("sir_vad_segment: bad sizes (n_rec %d, max_len %d, wave_stride %lld, seg_cap %d)", n_rec, max_len, (long long)wave_stride, seg_cap);
        return SIR_EINVAL;
    }
    if (!vad_config_ok("sir_vad_segment", *cfg)) return SIR_EINVAL;
    const size_t need = sir_vad_workspace_bytes(h, n_rec, max_len, cfg->chunk_size);
    if ((long long)n_rec * ws_layout(n_rec, max_len, cfg->chunk_size).wpr / kWaves >= (1ll << 31) - 1) {      // the energy kernel's grid
        sir_set_error("sir_vad_segment: batch too large (n_rec %d, max_len %d)", n_rec, max_len);
        return SIR_EINVAL;
    }
    if ((uintptr_t)workspace % 16 != 0) { sir_set_error("sir_vad_segment: workspace must be 16-byte aligned"); return SIR_EINVAL; }
    if (workspace_bytes < need) {
        sir_set_error("sir_vad_segment: workspace of %zu bytes, %zu needed", workspace_bytes, need);
        return SIR_ENOMEM;
    }
    return sir_wave_dispatch(wave_dtype, [&](auto tag) {
        using T = decltype(tag);
        return segment_impl<T>(h, (const T*)wave, wave_stride, lengths, n_rec, max_len, cfg, energy_out, seg_count, seg_table, seg_cap, total,
                               workspace, (hipStream_t)stream);
    });
}

extern "C" int sir_vad_gather(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, int n_rec, const int32_t* seg_table,
                              const int32_t* total, int seg_cap, float* out, int64_t out_stride, int max_clip_len, int32_t* out_lengths,
                              void* stream) {
    if (!h || !wave || !seg_table || !total || !out || !out_lengths) { sir_set_error("sir_vad_gather: NULL argument"); return SIR_EINVAL; }
    if (!sir_wave_elem_bytes(wave_dtype)) { sir_set_error("sir_vad_gather: bad wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (n_rec <= 0 || wave_stride <= 0 || !clip_gather_sizes_ok(seg_cap, max_clip_len, out_stride)) {
        sir_set_error("sir_vad_gather: bad sizes (n_rec %d, wave_stride %lld, seg_cap %d, max_clip_len %d, out_stride %lld)", n_rec,
                      (long long)wave_stride, seg_cap, max_clip_len, (long long)out_stride);
        return SIR_EINVAL;
    }
    SirProfScope prof(h, SIR_K_VAD_GATHER, (hipStream_t)stream);
    return sir_wave_dispatch(wave_dtype, [&](auto tag) {
        using T = decltype(tag);
        const LinearClips<T> src{(const T*)wave, (long long)wave_stride, n_rec, seg_table};
        const bool src_vec = (uintptr_t)wave % 16 == 0 && ((long long)wave_stride * (long long)sizeof(T)) % 16 == 0;
        return clip_gather_launch<T>(h, src, src_vec, total, seg_cap, out, out_stride, max_clip_len, out_lengths, (hipStream_t)stream);
    });
}
