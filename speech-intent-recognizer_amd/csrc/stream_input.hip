// Stream input (sir_stream_input_reset, sir_stream_input_push): the stage in front of sir_stream_push for callers whose audio is
// not PCM at the handle's rate -- 8 kHz G.711 telephony first of all.  S independent streams, each decoded (mu-law / A-law bytes,
// int16, float32) and rate-converted push by push with sir_resample's own table (frontend.hip) and its fmaf chain, tap for tap:
// the concatenated outputs of a stream are bit for bit what sir_resample gives for the whole decoded stream, however it was cut.
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
#include "sir_internal.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SIR_WAVE;
constexpr int kMaxStreams = 65535;
constexpr int kMaxIn = 1 << 24;

struct InState { long long n, emitted; };
static_assert(sizeof(InState) == 16, "state layout (include/sir_hip.h, DESIGN.md section 4)");

struct Geo { int orig, nw, width, K, H; bool copy; };
struct Layout { size_t ring_off, total; };

int gcd_int(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

// gcd-reduced rates and torchaudio's `width`, the expressions of frontend.hip's build_table (checked against the table at reset / push)
Geo geometry(const sir_stream_input_config* cfg) {
    Geo g;
    const int d = gcd_int(cfg->in_rate, cfg->out_rate);
    g.orig = cfg->in_rate / d;
    g.nw = cfg->out_rate / d;
    g.copy = cfg->in_rate == cfg->out_rate;
    const double base = (g.orig < g.nw ? g.orig : g.nw) * 0.99;
    g.width = (int)ceil(6 * (double)g.orig / base);
    g.K = 2 * g.width + g.orig;
    g.H = g.copy ? 0 : 2 * g.K;
    return g;
}

__host__ __device__ __forceinline__ int new_samples(int len, int in_width, int max_in) {
    const int cap = in_width < max_in ? in_width : max_in;
    return len < 0 ? 0 : (len > cap ? cap : len);
}

// ---- decoding: one element of the push row -> float32 (include/sir_hip.h) ---------------------------------------------------
template <int DT> struct Elem;
template <> struct Elem<SIR_WAVE_F32> { typedef float type; };
template <> struct Elem<SIR_WAVE_I16> { typedef short type; };
template <> struct Elem<SIR_WAVE_ULAW> { typedef unsigned char type; };
template <> struct Elem<SIR_WAVE_ALAW> { typedef unsigned char type; };

template <int DT>
__device__ __forceinline__ float decode(typename Elem<DT>::type x) {
    if constexpr (DT == SIR_WAVE_F32) {
        return x;
    } else if constexpr (DT == SIR_WAVE_I16) {
        return (float)x * (1.0f / 32768.0f);
    } else if constexpr (DT == SIR_WAVE_ULAW) {
        const int u = ~(int)x & 0xFF;
        const int t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7);
        return (float)((u & 0x80) ? 0x84 - t : t - 0x84) * (1.0f / 32768.0f);
    } else {
        const int a = (int)x ^ 0x55, e = (a >> 4) & 7, m = a & 0x0F;
        const int t = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8;
        return (float)((a & 0x80) ? t : -t) * (1.0f / 32768.0f);
    }
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
__global__ __launch_bounds__(kThreads) void sin_emit_kernel(const typename Elem<DT>::type* __restrict__ in, long long in_stride, int in_width,
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
    const typename Elem<DT>::type* row = in + (long long)s * in_stride;
    const float* hist = ring + (long long)s * H;
    const float* tp = taps + (size_t)p * L;
    float acc = 0.0f;
    for (int l = 0; l < L; ++l) {
        const int r = rel + l;
        float v = 0.0f;
        if (r >= 0) {
            if (r < m) v = decode<DT>(row[r]);                    // at or behind n1: the zero tail of a closing stream
        } else if (r >= lo) {
            int idx = h0 + r;
            idx += idx < 0 ? H : 0;
            v = hist[idx];
        }
        acc = fmaf(tp[l], v, acc);
    }
    out[(long long)s * out_stride + k] = acc;
}

// ---- 2. commit -------------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kThreads) void sin_commit_kernel(const typename Elem<DT>::type* __restrict__ in, long long in_stride, int in_width,
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
    const typename Elem<DT>::type* row = in + (long long)s * in_stride;
    float* hist = ring + (long long)s * H;
    for (int t = (m > H ? m - H : 0) + threadIdx.x; t < m; t += kThreads) hist[(h0 + t) % H] = decode<DT>(row[t]);
    if (threadIdx.x == 0) state[s] = InState{n1, e1};
}

// ---- equal rates: decode / copy ----------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(kThreads) void sin_copy_kernel(const typename Elem<DT>::type* __restrict__ in, long long in_stride, int in_width,
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

__global__ __launch_bounds__(kThreads) void sin_reset_kernel(InState* __restrict__ state, const unsigned char* __restrict__ mask, int S) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s < S && (mask == nullptr || mask[s] != 0)) state[s] = InState{0, 0};
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
    if (cfg->n_streams < 1 || cfg->n_streams > kMaxStreams || cfg->max_in < 1 || cfg->max_in > kMaxIn) {
        if (who) sir_set_error("%s: bad sizes (n_streams %d must be in [1, %d], max_in %d in [1, %d])", who, cfg->n_streams, kMaxStreams,
                               cfg->max_in, kMaxIn);
        return false;
    }
    return true;
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

int state_ok(const void* state, size_t state_bytes, const sir_stream_input_config* cfg, const Geo& g, const char* who) {
    if ((uintptr_t)state % 256 != 0) { sir_set_error("%s: state must be 256-byte aligned", who); return SIR_EINVAL; }
    const size_t need = layout(cfg, g).total;
    if (state_bytes < need) { sir_set_error("%s: state of %zu bytes, %zu needed", who, state_bytes, need); return SIR_ENOMEM; }
    return SIR_OK;
}

// the handle's table of the pair; it must be the geometry the state was sized for
int table_of(sir_handle* h, const sir_stream_input_config* cfg, const Geo& g, sir_resample_table* t, const char* who) {
    if (!sir_get_resample_table(h, cfg->in_rate, cfg->out_rate, t)) {
        sir_set_error("%s: could not build the %d -> %d Hz filter table", who, cfg->in_rate, cfg->out_rate);
        return SIR_EHIP;
    }
    if (t->orig != g.orig || t->nw != g.nw || t->width != g.width || t->L < 1 || t->L > g.K) {
        sir_set_error("%s: the %d -> %d Hz table (orig %d, new %d, width %d, L %d) does not have the expected geometry", who, cfg->in_rate,
                      cfg->out_rate, t->orig, t->nw, t->width, t->L);
        return SIR_EUNSUPPORTED;
    }
    return SIR_OK;
}

template <int DT>
int push_impl(void* state, const sir_stream_input_config* cfg, const Geo& g, const sir_resample_table* t, const void* in_v, int64_t in_stride,
              int in_width, const int32_t* in_lengths, const uint8_t* close, float* out, int64_t out_stride, int max_out,
              int32_t* out_lengths, hipStream_t st) {
    typedef typename Elem<DT>::type T;
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
    SIR_TRY(state_ok(state, state_bytes, cfg, g, "sir_stream_input_reset"));
    if (!g.copy) {                                                // the one place a table is built: pushes only look it up
        sir_resample_table t;
        SIR_TRY(table_of(h, cfg, g, &t, "sir_stream_input_reset"));
    }
    hipLaunchKernelGGL(sin_reset_kernel, dim3((cfg->n_streams + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                       (InState*)state, mask, cfg->n_streams);
    return sir_check_hip(hipGetLastError(), "sin_reset_kernel");
}

extern "C" int sir_stream_input_push(sir_handle* h, void* state, size_t state_bytes, const sir_stream_input_config* cfg, const void* in,
                                     int64_t in_stride, int in_width, const int32_t* in_lengths, const uint8_t* close, float* out,
                                     int64_t out_stride, int32_t* out_lengths, void* stream) {
    if (!h || !state || !cfg || !in || !in_lengths || !out || !out_lengths) { sir_set_error("sir_stream_input_push: NULL argument"); return SIR_EINVAL; }
    if (!config_ok(cfg, "sir_stream_input_push")) return SIR_EINVAL;
    if (in_width < 1 || in_width > cfg->max_in || in_stride < in_width) {
        sir_set_error("sir_stream_input_push: bad sizes (in_width %d must be in [1, max_in %d], in_stride %lld >= in_width)", in_width,
                      cfg->max_in, (long long)in_stride);
        return SIR_EINVAL;
    }
    const Geo g = geometry(cfg);
    const long long max_out = max_out_of(cfg, g);
    if (max_out < 0) { sir_set_error("sir_stream_input_push: the outputs of one push do not fit an int"); return SIR_EINVAL; }
    if (out_stride < max_out) {
        sir_set_error("sir_stream_input_push: out_stride %lld is below sir_stream_input_max_out = %lld (nothing was launched, the state has "
                      "not moved)", (long long)out_stride, max_out);
        return SIR_EINVAL;
    }
    SIR_TRY(state_ok(state, state_bytes, cfg, g, "sir_stream_input_push"));
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
