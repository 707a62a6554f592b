// Stream input (sir_stream_input_reset, sir_stream_input_push): the stage in front of sir_stream_push for callers whose audio is
// not PCM at the handle's rate -- 8 kHz G.711 telephony first of all.  S independent streams, each decoded (mu-law / A-law bytes,
// int16, float32: decode of wave_sample.h) and rate-converted push by push with sir_resample's own table (frontend.hip) and its
// geometry and fmaf chain (resample_fir.h, one copy for both): the concatenated outputs of a stream are bit for bit what
// sir_resample gives for the whole decoded stream, however it was cut.
//
//   1. sin_emit_kernel     grid (output block of 256, stream): a thread computes one output of this push.  Chain positions
//                          below the stream's n come from its history ring, the rest from the push row, decoded on load.
//   2. sin_commit_kernel   one workgroup per stream: writes the push's last samples into the ring and moves the counters.
//   (equal rates: sin_copy_kernel alone decodes the row and moves n.)
//
// Kernel 1 only reads the state, kernel 2 is the one that moves it; both derive the emitted count E(n) of include/sir_hip.h from
// the table's first[] (a minimum over the nw phases, no assumption that need(j) grows with j).  No atomics, no LDS beyond the
// four words of that block minimum.
//
// State buffer (256-byte aligned sections, in this order):
//   InState [S]      16 bytes per stream: n samples received, outputs emitted (int64), both since the last close / reset
//   ring    [S][H]   float32, decoded sample i of a stream at offset i mod H, H = 2 (2 width + orig); absent when the rates are equal
// Why H is enough: an output j not yet emitted at n has q(j) >= q(j0), j0 = E(n), and need(j0) > n, so its first chain position
// q(j) orig + first[p] - width > n - first[p0] - L + first[p] >= n - (K - 1) - K with K = 2 width + orig >= L, first[] in [0, K).
#include "resample_fir.h"
#include "stream_common.h"
#include "wave_sample.h"

namespace {

struct InState { long long n, emitted; };
static_assert(sizeof(InState) == 16, "state layout (include/sir_hip.h, DESIGN.md section 4)");

// the rate pair's geometry (the one sir_resample's table is built from) and the history ring's length H
struct Geo : ResampleGeo { int H; bool copy; };
struct Layout { size_t ring_off, total; };

Geo geometry(const sir_stream_input_config* cfg) {
    const ResampleGeo r = resample_geometry(cfg->in_rate, cfg->out_rate);
    const bool copy = cfg->in_rate == cfg->out_rate;
    return Geo{r, copy ? 0 : 2 * r.K, copy};
}

// ---- E(n): outputs a stream of n samples has emitted ----------------------------------------------------------------------------
// Phase p fails first at q_p = the smallest q >= 0 with q orig + first[p] - width + L > n; E(n) = min over p of q_p nw + p.  A closing
// stream emits everything: ceil(nw n / orig).  Every thread of the workgroup calls this (two barriers) and gets the same value.
__device__ __forceinline__ long long emitted_at(long long n, bool closing, const int* __restrict__ first, int orig, int nw, int width, int L,
                                                long long* sh) {
    if (closing) return (n * nw + orig - 1) / orig;
    long long best = 0x7fffffffffffffffll;
    for (int p = threadIdx.x; p < nw; p += kThreads) {
        const long long d = n - (first[p] - width + L);
        const long long q = d < 0 ? 0 : d / orig + 1;
        const long long j = q * nw + p;
        best = j < best ? j : best;
    }
#pragma unroll
    for (int o = SIR_WAVE / 2; o > 0; o >>= 1) {
        const long long other = __shfl_xor(best, o, SIR_WAVE);
        best = other < best ? other : best;
    }
    __syncthreads();                                              // a caller may have read sh from an earlier call
    if ((threadIdx.x & (SIR_WAVE - 1)) == 0) sh[threadIdx.x / SIR_WAVE] = best;
    __syncthreads();
    best = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = sh[w] < best ? sh[w] : best;
    return best;
}

// ---- 1. emit ---------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kThreads) void sin_emit_kernel(const typename WaveElem<DT>::type* __restrict__ in, long long in_stride, int in_width,
                                                            int max_in, const int* __restrict__ in_lengths,
                                                            const unsigned char* __restrict__ close, const InState* __restrict__ state,
                                                            const float* __restrict__ ring, int H, const float* __restrict__ taps,
                                                            const int* __restrict__ first, int orig, int nw, int width, int L,
                                                            float* __restrict__ out, long long out_stride, int max_out,
                                                            int* __restrict__ out_lengths) {
    __shared__ long long sh[kWaves];
    const int s = blockIdx.y;
    const int m = new_samples(in_lengths[s], in_width, max_in);
    const bool closing = close != nullptr && close[s] != 0;
    const bool head = blockIdx.x == 0 && threadIdx.x == 0;
    if (m == 0 && !closing) {                                     // workgroup-uniform: the stream is untouched
        if (head) out_lengths[s] = 0;
        return;
    }
    const InState st = state[s];
    const long long n1 = st.n + m;
    const long long e1 = emitted_at(n1, closing, first, orig, nw, width, L, sh);
    long long cnt = e1 - st.emitted;
    cnt = cnt < 0 ? 0 : (cnt > max_out ? max_out : cnt);          // cannot bind (sir_stream_input_max_out); keeps the stores in bounds
    if (head) out_lengths[s] = (int)cnt;
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= (int)cnt) return;
    const long long q0 = st.emitted / nw;
    const int kk = (int)(st.emitted - q0 * nw) + k;                // < nw + max_out
    const int dq = kk / nw, p = kk - dq * nw;
    const long long base = (q0 + dq) * orig + first[p] - width;   // first chain position of output st.emitted + k
    const int rel = (int)(base - st.n);                           // in (-H, m + orig + width]: relative to the push row
    const int h0 = (int)(st.n % H);
    const int lo = st.n < H ? -(int)st.n : -H;                    // positions below 0 are zeros; below n - H nothing is asked for
    const typename WaveElem<DT>::type* row = in + (long long)s * in_stride;
    const float* hist = ring + (long long)s * H;
    out[(long long)s * out_stride + k] = fir_chain(taps + (size_t)p * L, L, [&](int l) {
        const int r = rel + l;
        float v = 0.0f;
        if (r >= 0) {
            if (r < m) v = decode<DT>(row[r]);                    // at or behind n1: the zero tail of a closing stream
        } else if (r >= lo) {
            int idx = h0 + r;
            idx += idx < 0 ? H : 0;
            v = hist[idx];
        }
        return v;
    });
}

// ---- 2. commit -------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kThreads) void sin_commit_kernel(const typename WaveElem<DT>::type* __restrict__ in, long long in_stride, int in_width,
                                                              int max_in, const int* __restrict__ in_lengths,
                                                              const unsigned char* __restrict__ close, InState* __restrict__ state,
                                                              float* __restrict__ ring, int H, const int* __restrict__ first, int orig, int nw,
                                                              int width, int L) {
    __shared__ long long sh[kWaves];
    const int s = blockIdx.x;
    const int m = new_samples(in_lengths[s], in_width, max_in);
    const bool closing = close != nullptr && close[s] != 0;
    if (m == 0 && !closing) return;
    const InState st = state[s];
    if (closing) {                                                // workgroup-uniform
        __syncthreads();                                          // every thread has read st
        if (threadIdx.x == 0) state[s] = InState{0, 0};           // the ring needs no clearing: nothing below position 0 is read
        return;
    }
    const long long n1 = st.n + m;
    const long long e1 = emitted_at(n1, false, first, orig, nw, width, L, sh);     // (its barriers: every thread has read st)
    const int h0 = (int)(st.n % H);
    const typename WaveElem<DT>::type* row = in + (long long)s * in_stride;
    float* hist = ring + (long long)s * H;
    for (int t = (m > H ? m - H : 0) + threadIdx.x; t < m; t += kThreads) hist[(h0 + t) % H] = decode<DT>(row[t]);
    if (threadIdx.x == 0) state[s] = InState{n1, e1};
}

// ---- equal rates: decode / copy ----------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kThreads) void sin_copy_kernel(const typename WaveElem<DT>::type* __restrict__ in, long long in_stride, int in_width,
                                                            int max_in, const int* __restrict__ in_lengths,
                                                            const unsigned char* __restrict__ close, InState* __restrict__ state,
                                                            float* __restrict__ out, long long out_stride, int* __restrict__ out_lengths) {
    const int s = blockIdx.y;
    const int m = new_samples(in_lengths[s], in_width, max_in);
    if (blockIdx.x == 0 && threadIdx.x == 0) {                    // the only reader and writer of this stream's counters
        out_lengths[s] = m;
        const bool closing = close != nullptr && close[s] != 0;
        if (closing) state[s] = InState{0, 0};
        else if (m > 0) { const long long n1 = state[s].n + m; state[s] = InState{n1, n1}; }
    }
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k < m) out[(long long)s * out_stride + k] = decode<DT>(in[(long long)s * in_stride + k]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool dtype_ok(int dt) { return dt == SIR_WAVE_F32 || dt == SIR_WAVE_I16 || dt == SIR_WAVE_ULAW || dt == SIR_WAVE_ALAW; }

bool config_ok(const sir_stream_input_config* cfg, const char* who) {
    if (!cfg) { if (who) sir_set_error("%s: NULL config", who); return false; }
    if (!dtype_ok(cfg->in_dtype)) { if (who) sir_set_error("%s: bad in_dtype %d", who, cfg->in_dtype); return false; }
    if (cfg->in_rate <= 0 || cfg->out_rate <= 0) {
        if (who) sir_set_error("%s: bad rates (%d -> %d Hz)", who, cfg->in_rate, cfg->out_rate);
        return false;
    }
    return stream_limits_ok(who, cfg->n_streams, cfg->max_in);
}

// ceil(nw (max_in + 3 width + 2 orig) / orig) + 1 (include/sir_hip.h); -1 when it does not fit an int
long long max_out_of(const sir_stream_input_config* cfg, const Geo& g) {
    if (g.copy) return cfg->max_in;
    const long long span = (long long)cfg->max_in + 3ll * g.width + 2ll * g.orig;
    const long long v = ((long long)g.nw * span + g.orig - 1) / g.orig + 1;
    return v > 0x7fffffffll ? -1 : v;
}

Layout layout(const sir_stream_input_config* cfg, const Geo& g) {
    Layout l;
    l.ring_off = sir_align_up((size_t)cfg->n_streams * sizeof(InState), 256);
    l.total = l.ring_off + sir_align_up((size_t)cfg->n_streams * (size_t)g.H * sizeof(float), 256);
    return l;
}

// the handle's table of the pair.  Its orig / nw / width are g's by construction (resample_geometry); that the kept taps fit the
// history ring, 1 <= L <= K, is a property of the filter and is checked
int table_of(sir_handle* h, const sir_stream_input_config* cfg, const Geo& g, sir_resample_table* t, const char* who) {
    if (!sir_get_resample_table(h, cfg->in_rate, cfg->out_rate, t)) {
        sir_set_error("%s: could not build the %d -> %d Hz filter table", who, cfg->in_rate, cfg->out_rate);
        return SIR_EHIP;
    }
    if (t->L < 1 || t->L > g.K) {
        sir_set_error("%s: the %d -> %d Hz table (orig %d, new %d, width %d) keeps L = %d taps, outside [1, %d]", who, cfg->in_rate, cfg->out_rate,
                      t->orig, t->nw, t->width, t->L, g.K);
        return SIR_EUNSUPPORTED;
    }
    return SIR_OK;
}

template <int DT>
int push_impl(void* state, const sir_stream_input_config* cfg, const Geo& g, const sir_resample_table* t, const void* in_v, int64_t in_stride,
              int in_width, const int32_t* in_lengths, const uint8_t* close, float* out, int64_t out_stride, int max_out,
              int32_t* out_lengths, hipStream_t st) {
    typedef typename WaveElem<DT>::type T;
    const T* in = (const T*)in_v;
    InState* ss = (InState*)state;
    const int S = cfg->n_streams;
    if (g.copy) {
        hipLaunchKernelGGL(sin_copy_kernel<DT>, dim3((in_width + kThreads - 1) / kThreads, S), dim3(kThreads), 0, st, in, (long long)in_stride,
                           in_width, cfg->max_in, in_lengths, close, ss, out, (long long)out_stride, out_lengths);
        return sir_check_hip(hipGetLastError(), "sin_copy_kernel");
    }
    float* ring = (float*)((char*)state + layout(cfg, g).ring_off);
    hipLaunchKernelGGL(sin_emit_kernel<DT>, dim3((max_out + kThreads - 1) / kThreads, S), dim3(kThreads), 0, st, in, (long long)in_stride, in_width,
                       cfg->max_in, in_lengths, close, (const InState*)ss, (const float*)ring, g.H, (const float*)t->taps, (const int*)t->first,
                       t->orig, t->nw, t->width, t->L, out, (long long)out_stride, max_out, out_lengths);
    SIR_TRY(sir_check_hip(hipGetLastError(), "sin_emit_kernel"));
    hipLaunchKernelGGL(sin_commit_kernel<DT>, dim3(S), dim3(kThreads), 0, st, in, (long long)in_stride, in_width, cfg->max_in, in_lengths, close,
                       ss, ring, g.H, (const int*)t->first, t->orig, t->nw, t->width, t->L);
    return sir_check_hip(hipGetLastError(), "sin_commit_kernel");
}

}  // namespace

extern "C" int sir_stream_input_max_out(const sir_stream_input_config* cfg) {
    if (!config_ok(cfg, nullptr)) return -1;
    return (int)max_out_of(cfg, geometry(cfg));
}

extern "C" size_t sir_stream_input_state_bytes(const sir_handle* h, const sir_stream_input_config* cfg) {
    if (!h || !config_ok(cfg, nullptr)) return 0;
    const Geo g = geometry(cfg);
    if (max_out_of(cfg, g) < 0) return 0;
    return layout(cfg, g).total;
}

extern "C" int sir_stream_input_reset(sir_handle* h, void* state, size_t state_bytes, const sir_stream_input_config* cfg, const uint8_t* mask,
                                      void* stream) {
    if (!h || !state || !cfg) { sir_set_error("sir_stream_input_reset: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_input_reset")) return SIR_EINVAL;
    const Geo g = geometry(cfg);
    if (max_out_of(cfg, g) < 0) { sir_set_error("sir_stream_input_reset: the outputs of one push do not fit an int"); return SIR_EINVAL; }
    SIR_TRY(state_ok("sir_stream_input_reset", state, state_bytes, layout(cfg, g).total));
    if (!g.copy) {                                                // the one place a table is built: pushes only look it up
        sir_resample_table t;
        SIR_TRY(table_of(h, cfg, g, &t, "sir_stream_input_reset"));
    }
    return stream_reset_launch((InState*)state, mask, cfg->n_streams, (hipStream_t)stream);
}

extern "C" int sir_stream_input_push(sir_handle* h, void* state, size_t state_bytes, const sir_stream_input_config* cfg, const void* in,
                                     int64_t in_stride, int in_width, const int32_t* in_lengths, const uint8_t* close, float* out,
                                     int64_t out_stride, int32_t* out_lengths, void* stream) {
    if (!h || !state || !cfg || !in || !in_lengths || !out || !out_lengths) { sir_set_error("sir_stream_input_push: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_input_push")) return SIR_EINVAL;
    if (!push_sizes_ok("sir_stream_input_push", in_width, cfg->max_in, in_stride)) return SIR_EINVAL;
    const Geo g = geometry(cfg);
    const long long max_out = max_out_of(cfg, g);
    if (max_out < 0) { sir_set_error("sir_stream_input_push: the outputs of one push do not fit an int"); return SIR_EINVAL; }
    if (out_stride < max_out) {
        sir_set_error("sir_stream_input_push: out_stride %lld is below sir_stream_input_max_out = %lld (nothing was launched, the state has "
                      "not moved)", (long long)out_stride, max_out);
        return SIR_EINVAL;
    }
    SIR_TRY(state_ok("sir_stream_input_push", state, state_bytes, layout(cfg, g).total));
    sir_resample_table t{};
    if (!g.copy) SIR_TRY(table_of(h, cfg, g, &t, "sir_stream_input_push"));
    hipStream_t st = (hipStream_t)stream;
    switch (cfg->in_dtype) {
    case SIR_WAVE_F32:
        return push_impl<SIR_WAVE_F32>(state, cfg, g, &t, in, in_stride, in_width, in_lengths, close, out, out_stride, (int)max_out, out_lengths, st);
    case SIR_WAVE_I16:
        return push_impl<SIR_WAVE_I16>(state, cfg, g, &t, in, in_stride, in_width, in_lengths, close, out, out_stride, (int)max_out, out_lengths, st);
    case SIR_WAVE_ULAW:
        return push_impl<SIR_WAVE_ULAW>(state, cfg, g, &t, in, in_stride, in_width, in_lengths, close, out, out_stride, (int)max_out, out_lengths, st);
    default:
        return push_impl<SIR_WAVE_ALAW>(state, cfg, g, &t, in, in_stride, in_width, in_lengths, close, out, out_stride, (int)max_out, out_lengths, st);
    }
}
