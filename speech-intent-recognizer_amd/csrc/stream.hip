// Live streams (sir_stream_reset, sir_stream_push, sir_stream_gather): the energy detector of the reference's continuous-audio
// recogniser (scripts/testing.py:38-133) for S streams that arrive piece by piece, with the listener's state carried from one
// push to the next in a caller-owned device buffer.  The parallel axis is streams x new chunks, not the chunks of one long
// recording as in vad.hip.
//
//   1. stream_append_kernel   copies the new samples of every stream into its ring (chunk k at ring offset (k mod R) * c)
//   2. stream_energy_kernel   one sub-wave per chunk that this push completes: mean |x| -> one flag byte (and, optionally, the energy)
//   3. stream_segment_kernel  one thread per stream walks its new chunks through the listener's state machine; rows are numbered
//                             across streams by block scans with a base carried over tiles of 256 streams; the state is committed
//   4. clip_gather_kernel     cuts the rows of the table out of the rings as zero-tailed float rows, wrap-aware (clip_gather.h,
//                             the kernel of sir_vad_gather with the ring as its source)
//
// Kernels 1 and 2 only read the per-stream counters; kernel 3 is the one that moves them.  No atomics on the numbering path.
//
// State buffer (256-byte aligned sections, in this order):
//   StreamState [S]          32 bytes per stream: n, j, first (int64), recording, silence (int32)
//   ring        [S][R * c]   samples in the push dtype
//   flags       [S][K]       one byte per chunk the latest push judged, K = ceil(max_in / c) + 1
#include "clip_gather.h"
#include "stream_common.h"
#include "vad_common.h"

#include <math.h>

namespace {

constexpr int kMaxChunks = 1 << 20;                   // bound of max_utt_chunks and ring_chunks: every byte count stays far below 2^63

struct StreamState { long long n, j, first; int recording, silence; };
static_assert(sizeof(StreamState) == 32, "state layout (include/sir_hip.h, DESIGN.md section 4)");

struct Layout { int per, K; long long RC; size_t ring_off, flags_off, total; };

// ---- 1. append -------------------------------------------------------------------------------------------------------------
// grid (stream, column block).  A thread owns one 16-byte group of the DESTINATION: the ring is 16-byte aligned and R * c is a
// multiple of the vector width, so a group never straddles the wrap; the source is read with one vector load where its address
// allows and sample by sample otherwise.  The groups at the two ends of the push are partial and go sample by sample.
template <typename T>
__global__ __launch_bounds__(kThreads) void stream_append_kernel(const T* __restrict__ in, long long in_stride, int in_width, int max_in,
                                                                 const int* __restrict__ in_lengths, const StreamState* __restrict__ state,
                                                                 T* __restrict__ ring, long long RC) {
    constexpr int V = 16 / (int)sizeof(T);
    const int s = blockIdx.x;
    const int m = new_samples(in_lengths[s], in_width, max_in);
    const long long d0 = state[s].n % RC;
    const int a = (int)(d0 % V);
    const long long t0 = ((long long)blockIdx.y * kThreads + threadIdx.x) * V - a;    // first new sample of this group (may be < 0)
    if (t0 >= m) return;
    const T* src = in + (long long)s * in_stride;
    T* dst = ring + (long long)s * RC + (d0 + t0) % RC;                              // d0 + t0 >= d0 - a >= 0, a multiple of V
    if (t0 >= 0 && t0 + V <= m) {
        alignas(16) T t[V];
        if ((uintptr_t)(src + t0) % 16 == 0) {
            *reinterpret_cast<int4*>(t) = *reinterpret_cast<const int4*>(src + t0);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) t[e] = src[t0 + e];
        }
        *reinterpret_cast<int4*>(dst) = *reinterpret_cast<const int4*>(t);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
            if (t0 + e >= 0 && t0 + e < m) dst[e] = src[t0 + e];
    }
}

// ---- 2. energy -------------------------------------------------------------------------------------------------------------
// One sub-wave per chunk slot k < K of a stream: chunk j + k is judged if the push completed it, or if the stream closes and it is
// the trailing partial chunk.  A chunk is contiguous and 16-byte aligned in the ring, so the vector path of vad_common.h serves it.
template <typename T>
__global__ __launch_bounds__(kThreads) void stream_energy_kernel(const StreamState* __restrict__ state, const int* __restrict__ in_lengths,
                                                                 const unsigned char* __restrict__ close, const T* __restrict__ ring,
                                                                 long long RC, int R, int c, int K, int in_width, int max_in,
                                                                 float threshold, long long n_tasks, int gps,
                                                                 float* __restrict__ energy_out, unsigned char* __restrict__ flags) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int LPC = 64 / V;
    constexpr int CPP = SIR_WAVE / LPC;
    const long long task = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (task >= n_tasks) return;                // wave-uniform
    const int s = (int)(task / gps), grp = (int)(task - (long long)s * gps);
    const int lane = threadIdx.x & 63, sub = lane / LPC, sl = lane - sub * LPC;
    const int k = grp * CPP + sub;
    const StreamState st = state[s];
    const long long n_new = st.n + new_samples(in_lengths[s], in_width, max_in);
    const long long chunk = st.j + k, begin = chunk * c;
    const bool full = begin + c <= n_new;
    const bool partial = !full && begin < n_new && close != nullptr && close[s] != 0;
    const bool live = k < K && (full || partial);
    Acc<T> acc;
    int count = 1;
    if (live) {
        count = full ? c : (int)(n_new - begin);
        const T* p = ring + (long long)s * RC + (chunk % R) * c;
        chunk_accumulate<T, true>(acc, p + sl * V, count - sl * V, c / 64);
    }
    const float e = acc.finish(LPC, count);                       // every lane takes part in the butterfly
    const bool speech = live && e > threshold;                    // strict, in float (testing.py:44-47); NaN is silence
    if (sl == 0 && k < K) {
        flags[(size_t)s * K + k] = speech ? 1 : 0;
        if (energy_out) energy_out[(size_t)s * K + k] = live ? e : 0.0f;
    }
}

// ---- 3. state machine ------------------------------------------------------------------------------------------------------
// The listener's loop (testing.py:84-133) over the chunks this push judged, from the carried state `st`.  emit(row of this stream,
// first sample, end sample, flags) is called in time order; returns the number of rows.  The forced cut makes the prefix-maximum
// form of vad_segment_kernel inapplicable, and a push brings at most K chunks.
template <typename F>
__device__ __forceinline__ int walk_stream(const unsigned char* __restrict__ fl, int nj, long long n_new, int c, int prior, int n_stop,
                                           int max_utt, bool flush, StreamState& st, F emit) {
    int rows = 0;
    for (int k = 0; k < nj; ++k) {
        const long long i = st.j + k;
        const bool speech = fl[k] != 0;
        if (!st.recording && speech) {
            st.recording = 1;
            st.silence = 0;
            st.first = prior >= 1 ? (i - prior + 1 > 0 ? i - prior + 1 : 0) : i;
        }
        if (st.recording) {
            st.silence = speech ? 0 : st.silence + 1;
            int flag = -1;
            if (st.silence >= n_stop) flag = 0;
            else if (i - st.first + 1 >= max_utt) flag = SIR_STREAM_FORCED;
            if (flag >= 0) {
                const long long e = (i + 1) * c;
                emit(rows++, st.first * c, e < n_new ? e : n_new, flag);
                st.recording = 0;
            }
        }
    }
    if (flush && st.recording) emit(rows++, st.first * c, n_new, SIR_STREAM_FLUSHED);
    return rows;
}

// One workgroup; thread t of tile T owns stream T * 256 + t.  Each thread walks twice from the same carried state: once to count
// its rows, once -- behind the block scan that numbers them -- to write them; then it commits the state.
__global__ __launch_bounds__(kThreads) void stream_segment_kernel(StreamState* __restrict__ state, const int* __restrict__ in_lengths,
                                                                  const unsigned char* __restrict__ close,
                                                                  const unsigned char* __restrict__ flags, int S, int c, int K, int in_width,
                                                                  int max_in, int prior, int n_stop, int max_utt, int flush_tail,
                                                                  long long* __restrict__ table, int seg_cap, int* __restrict__ total) {
    __shared__ int sh[kWaves];
    long long base = 0;                                             // block-uniform: rows of the tiles done so far
    for (int tile = 0; tile < S; tile += kThreads) {
        const int s = tile + threadIdx.x;
        const bool active = s < S;
        StreamState st0 = {0, 0, 0, 0, 0};
        long long n_new = 0;
        int nj = 0, nfull = 0;
        bool closing = false;
        if (active) {
            st0 = state[s];
            n_new = st0.n + new_samples(in_lengths[s], in_width, max_in);
            closing = close != nullptr && close[s] != 0;
            nfull = (int)(n_new / c - st0.j);
            nj = nfull + ((closing && n_new % c != 0) ? 1 : 0);
            nj = nj < K ? nj : K;                                   // cannot bind while j == n / c holds; keeps the flag reads in bounds
        }
        const unsigned char* fl = flags + (size_t)(active ? s : 0) * K;
        const bool flush = closing && flush_tail != 0;
        StreamState st = st0;
        const int mine = walk_stream(fl, nj, n_new, c, prior, n_stop, max_utt, flush, st, [](int, long long, long long, int) {});
        int tot;
        const long long row0 = base + block_excl_add(mine, sh, &tot);
        if (active) {
            st = st0;
            walk_stream(fl, nj, n_new, c, prior, n_stop, max_utt, flush, st, [&](int r, long long a, long long b, int flag) {
                const long long row = row0 + r;
                if (row < seg_cap) {
                    long long* t = table + row * 4;
                    t[0] = s; t[1] = a; t[2] = b; t[3] = flag;
                }
            });
            if (closing) {
                st = StreamState{0, 0, 0, 0, 0};
            } else {
                st.n = n_new;
                st.j = st0.j + nfull;
            }
            state[s] = st;
        }
        base += tot;
    }
    if (threadIdx.x == 0) total[0] = (int)base;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// everything but ring_chunks: what the size helpers need
bool base_ok(const sir_stream_config* cfg, const char* who) {
    if (!cfg) { if (who) sir_set_error("%s: NULL config", who); return false; }
    const sir_vad_config& v = cfg->vad;
    if (!vad_config_ok(who, v)) return false;
    if (!sir_wave_elem_bytes(cfg->wave_dtype)) {
        if (who) sir_set_error("%s: bad wave_dtype %d", who, cfg->wave_dtype);
        return false;
    }
    if (!stream_limits_ok(who, cfg->n_streams, cfg->max_in)) return false;
    if (cfg->max_utt_chunks <= v.prior_chunks || cfg->max_utt_chunks > kMaxChunks) {
        if (who) sir_set_error("%s: max_utt_chunks %d must be above prior_chunks %d and at most %d", who, cfg->max_utt_chunks, v.prior_chunks,
                               kMaxChunks);
        return false;
    }
    return true;
}

int chunks_per_push(const sir_stream_config* cfg) { return (cfg->max_in + cfg->vad.chunk_size - 1) / cfg->vad.chunk_size; }

bool config_ok(const sir_stream_config* cfg, const char* who) {
    if (!base_ok(cfg, who)) return false;
    const int need = cfg->max_utt_chunks + chunks_per_push(cfg) + 2;
    if (cfg->ring_chunks < need || cfg->ring_chunks > 2 * kMaxChunks) {
        if (who) sir_set_error("%s: ring_chunks %d must be in [%d, %d] (max_utt_chunks + ceil(max_in / chunk_size) + 2 at the least)", who,
                               cfg->ring_chunks, need, 2 * kMaxChunks);
        return false;
    }
    return true;
}

Layout layout(const sir_stream_config* cfg) {
    Layout l;
    l.per = chunks_per_push(cfg);
    l.K = l.per + 1;
    l.RC = (long long)cfg->ring_chunks * cfg->vad.chunk_size;
    const size_t esz = sir_wave_elem_bytes(cfg->wave_dtype);
    l.ring_off = sir_align_up((size_t)cfg->n_streams * sizeof(StreamState), 256);
    l.flags_off = sir_align_up(l.ring_off + (size_t)cfg->n_streams * (size_t)l.RC * esz, 256);    // < 2^16 * 2^33 * 4
    l.total = sir_align_up(l.flags_off + (size_t)cfg->n_streams * l.K, 256);
    return l;
}

template <typename T>
int push_impl(void* state, const sir_stream_config* cfg, const T* in, int64_t in_stride, int in_width, const int32_t* in_lengths,
              const uint8_t* close, float* energy_out, int64_t* seg_table, int seg_cap, int32_t* total, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int CPP = SIR_WAVE / (64 / V);
    const Layout l = layout(cfg);
    StreamState* ss = (StreamState*)state;
    T* ring = (T*)((char*)state + l.ring_off);
    unsigned char* flags = (unsigned char*)state + l.flags_off;
    const int S = cfg->n_streams, c = cfg->vad.chunk_size;
    const int width = in_width < cfg->max_in ? in_width : cfg->max_in;
    const int groups = (width + V - 1) / V + 1;                    // destination groups a push can touch (misaligned start: one more)
    hipLaunchKernelGGL(stream_append_kernel<T>, dim3(S, (groups + kThreads - 1) / kThreads), dim3(kThreads), 0, st, in, (long long)in_stride,
                       in_width, cfg->max_in, in_lengths, ss, ring, l.RC);
    SIR_TRY(sir_check_hip(hipGetLastError(), "stream_append_kernel"));
    const int gps = (l.K + CPP - 1) / CPP;
    const long long n_tasks = (long long)S * gps;
    hipLaunchKernelGGL(stream_energy_kernel<T>, dim3((unsigned int)((n_tasks + kWaves - 1) / kWaves)), dim3(kThreads), 0, st, ss, in_lengths,
                       close, ring, l.RC, cfg->ring_chunks, c, l.K, in_width, cfg->max_in, cfg->vad.threshold, n_tasks, gps, energy_out, flags);
    SIR_TRY(sir_check_hip(hipGetLastError(), "stream_energy_kernel"));
    hipLaunchKernelGGL(stream_segment_kernel, dim3(1), dim3(kThreads), 0, st, ss, in_lengths, close, flags, S, c, l.K, in_width, cfg->max_in,
                       cfg->vad.prior_chunks, cfg->vad.silence_chunks, cfg->max_utt_chunks, cfg->vad.flush_tail != 0 ? 1 : 0,
                       (long long*)seg_table, seg_cap, total);
    return sir_check_hip(hipGetLastError(), "stream_segment_kernel");
}

}  // namespace

extern "C" int sir_stream_min_ring_chunks(const sir_stream_config* cfg) {
    if (!base_ok(cfg, nullptr)) return -1;
    return cfg->max_utt_chunks + chunks_per_push(cfg) + 2;
}

extern "C" int sir_stream_max_rows(const sir_stream_config* cfg) {
    if (!base_ok(cfg, nullptr)) return -1;
    const long long rows = (long long)cfg->n_streams * (chunks_per_push(cfg) + 2);
    return rows > 0x7fffffffll ? -1 : (int)rows;
}

extern "C" size_t sir_stream_state_bytes(const sir_handle* h, const sir_stream_config* cfg) {
    if (!h || !config_ok(cfg, nullptr)) return 0;
    return layout(cfg).total;
}

extern "C" int sir_stream_reset(sir_handle* h, void* state, size_t state_bytes, const sir_stream_config* cfg, const uint8_t* mask,
                                void* stream) {
    if (!h || !state || !cfg) { sir_set_error("sir_stream_reset: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_reset")) return SIR_EINVAL;
    SIR_TRY(state_ok("sir_stream_reset", state, state_bytes, layout(cfg).total));
    return stream_reset_launch((StreamState*)state, mask, cfg->n_streams, (hipStream_t)stream);
}

extern "C" int sir_stream_push(sir_handle* h, void* state, size_t state_bytes, const sir_stream_config* cfg, const void* in, int64_t in_stride,
                               int in_width, const int32_t* in_lengths, const uint8_t* close, float* energy_out, int64_t* seg_table,
                               int seg_cap, int32_t* total, void* stream) {
    if (!h || !state || !cfg || !in || !in_lengths || !seg_table || !total) { sir_set_error("sir_stream_push: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_push")) return SIR_EINVAL;
    if (!push_sizes_ok("sir_stream_push", in_width, cfg->max_in, in_stride)) return SIR_EINVAL;
    const long long rows = (long long)cfg->n_streams * (chunks_per_push(cfg) + 2);
    if (rows > 0x7fffffffll || seg_cap < rows) {
        sir_set_error("sir_stream_push: seg_cap %d is below sir_stream_max_rows = %lld (nothing was launched, the state has not moved)", seg_cap,
                      rows);
        return SIR_EINVAL;
    }
    SIR_TRY(state_ok("sir_stream_push", state, state_bytes, layout(cfg).total));
    return sir_wave_dispatch(cfg->wave_dtype, [&](auto tag) {
        using T = decltype(tag);
        return push_impl<T>(state, cfg, (const T*)in, in_stride, in_width, in_lengths, close, energy_out, seg_table, seg_cap, total,
                            (hipStream_t)stream);
    });
}

extern "C" int sir_stream_gather(sir_handle* h, const void* state, size_t state_bytes, const sir_stream_config* cfg, const int64_t* seg_table,
                                 const int32_t* total, int seg_cap, float* out, int64_t out_stride, int max_clip_len, int32_t* out_lengths,
                                 void* stream) {
    if (!h || !state || !cfg || !seg_table || !total || !out || !out_lengths) { sir_set_error("sir_stream_gather: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_gather")) return SIR_EINVAL;
    if (!clip_gather_sizes_ok(seg_cap, max_clip_len, out_stride)) {
        sir_set_error("sir_stream_gather: bad sizes (seg_cap %d, max_clip_len %d, out_stride %lld)", seg_cap, max_clip_len, (long long)out_stride);
        return SIR_EINVAL;
    }
    const Layout l = layout(cfg);
    SIR_TRY(state_ok("sir_stream_gather", state, state_bytes, l.total));
    return sir_wave_dispatch(cfg->wave_dtype, [&](auto tag) {
        using T = decltype(tag);
        const RingClips<T> src{(const T*)((const char*)state + l.ring_off), l.RC, cfg->n_streams, (const long long*)seg_table};
        return clip_gather_launch<T>(h, src, true, total, seg_cap, out, out_stride, max_clip_len, out_lengths, (hipStream_t)stream);
    });
}
