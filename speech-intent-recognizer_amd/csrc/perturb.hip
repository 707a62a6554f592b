// Waveform pitch / tempo perturbation ahead of the feature path (reference: scripts/augment.py:30-80, pitch_shift and
// speed_change, which run sox `pitch c` + `rate sr` and `tempo f` + `rate sr` on one clip at a time on the host).
//
// Tempo T(x, f) restates sox 14.4's `tempo` effect (default profile, linear search): WSOLA with segment S, search W,
// overlap O and hop H = S - O samples derived from the sample rate by sox's formulas (1312 / 235 / 192 / 1120 at 16 kHz).
// z = W/2 zeros, x[0:L], zeros.  Segment j starts its search at p_j = int(f j H + .5) (p_0 = 0) and picks
//     off_j = argmin_i sum_m (z[p_j + i + m] - ob[m])^2,  i in [0, W), m in [0, O)   (first minimum; off_0 = W/2)
// then emits H samples: the O-sample linear cross-fade of the previous tail `ob` into z[q .. q+O) (q = p_j + off_j; segment
// 0 emits z[q .. q+O) as it is), then z[q+O .. q+H); the new tail is z[q+H .. q+S).  Output j covers [j H, (j+1) H); the
// result is the first int(L/f + .5) samples.  Pitch P(x, c) = T(x, 1/d), d = 2^(c/1200), resampled back to L samples at the
// fractional positions n d with the library's own windowed-sinc filter (sinc_interp_hann, width 6, rolloff 0.99 -- the
// filter of sir_resample, NOT sox's `rate`):  y[n] = sum_k s[k] h(n d - k),  h(u) = b sinc(b u) cos(pi b u / 12)^2 for
// |b u| < 6, b = 0.99 min(1, 1/d).  Speed V(x, f) = T(x, f) (the reference's `rate sr` after `tempo` is a no-op).
//
// Chain per utterance, in the reference's order (augment.py:119-133): shift (read index, as sir_features_fwd), pitch, speed.
// Noise and the features follow in sir_features_fwd.  Cents 0 / factor 1 are the identity (a copy), not WSOLA at 1.
//
// Kernels: wsola_kernel = one 256-thread workgroup per utterance (each utterance is a sequential chain of segments: segment
// j's tail `ob` depends on off_{j-1}; utterances are independent).  Per segment every thread owns one search candidate (two
// where W > 256, above 17.4 kHz) and sums its O squared differences from LDS; the thread's own comparison, a wave-shuffle
// and an LDS argmin all break ties toward the lower index.  The segment's
// whole source window z[p_j .. p_j + W + S) (1547 samples at 16 kHz) sits in one of two LDS buffers: the next segment's
// window does not depend on the search (p_{j+1} is known), so its global loads are issued before the search and land in
// the other buffer after it -- no load latency on the chain.  pitch_resample_kernel = a gather of ~14 taps per output
// sample over the whole grid; sin(pi b (fr + i)) and the Hann term are expanded by angle addition around the nearest
// integer position (fr in [-0.5, 0.5]) with per-utterance cos / sin tables of the integer offsets i, so that a tap costs a
// few FMAs and one reciprocal instead of two transcendental calls.
#include <math.h>
#include <stdint.h>
#include "sir_internal.h"
#include "wave_sample.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRate = 24000;        // largest sample rate whose WSOLA window fits the buffers below (the prefetch
constexpr int kMaxRegion = 2368;       // registers of a larger one spill); W + S at 24 kHz = 352 + 1968, rounded up to 64
constexpr int kMaxO = 288;             // O at 24 kHz
constexpr int kPer = (kMaxRegion + kThreads - 1) / kThreads;
constexpr float kMaxCents = 200.0f;    // |pitch| bound: sizes the workspace of the stretched signal
constexpr double kMaxStretch = 1.1224620483093730;    // 2^(200/1200)
constexpr float kMinTempo = 0.5f, kMaxTempo = 2.0f;
constexpr int kTab = 8;                // |n d - k| < 6 / b <= 6.81 at 200 cents, and |fr| <= 0.5: offsets i in [-7, 7]

enum { kModeCents = 0, kModeTempo = 1, kModeCopy = 2 };

struct Geom { int S, W, O, H; };

Geom geom_for(int sr) {                // sox tempo.c, default profile: segment 82 ms, search 14.68 ms, overlap 12 ms
    Geom g;
    g.S = (int)(sr * 82.0 / 1000.0 + .5);
    g.W = (int)(sr * 14.68 / 1000.0 + .5);
    double ov = sr * 12.0 / 1000.0 + 4.5;
    g.O = ((int)(ov > 16.0 ? ov : 16.0)) & ~7;
    if (2 * g.O > g.S) g.O -= 8;
    g.H = g.S - g.O;
    return g;
}

// the row's factor; false = outside the accepted range (row zeroed, status flagged)
__device__ __forceinline__ bool row_factor(int mode, const float* factor, int b, double* f) {
    *f = 1.0;
    if (mode == kModeCents) {
        const float c = factor[b];
        if (!(fabsf(c) <= kMaxCents)) return false;
        if (c != 0.0f) *f = 1.0 / exp2((double)c / 1200.0);
    } else if (mode == kModeTempo) {
        const float t = factor[b];
        if (!(t >= kMinTempo && t <= kMaxTempo)) return false;
        *f = (double)t;
    }
    return true;
}

// One tempo pass.  src rows: [batch][src_stride] (WT = float or PCM16), row length min(lengths[b], max_len), read shifted
// by shift[b] (optional).  dst rows: [batch][dst_stride] f32, [0, Nc) written, [Nc, cap) zeroed, Nc = min(int(L/f+.5), cap).
// guard_cents (optional; the speed pass behind a pitch pass): a row whose cents the pitch pass rejected stays rejected here
// (zeroed, length 0), whatever its tempo.
template <typename WT>
__global__ __launch_bounds__(kThreads) void wsola_kernel(const WT* __restrict__ src, long long src_stride, const int* __restrict__ lengths,
                                                         int max_len, const int* __restrict__ shift, int mode,
                                                         const float* __restrict__ factor, float* __restrict__ dst, long long dst_stride,
                                                         int cap, int vec, int* __restrict__ dst_len, int* __restrict__ offsets,
                                                         int max_segments, int pass, unsigned int* __restrict__ status, int S, int W,
                                                         int O, int H, const float* __restrict__ guard_cents) {
    __shared__ float reg[2][kMaxRegion];     // source windows z[p_j .. p_j + W + S), double-buffered over j
    __shared__ float ob[2][kMaxO];           // tail of the previous segment, double-buffered over j
    __shared__ float rv[kThreads / SIR_WAVE];
    __shared__ int ri[kThreads / SIR_WAVE];

    const int b = blockIdx.x, tid = threadIdx.x;
    int L = lengths ? lengths[b] : max_len;
    L = L < 0 ? 0 : (L > max_len ? max_len : L);
    const int sh = shift ? shift[b] : 0;
    const WT* x = src + (size_t)b * src_stride;
    float* y = dst + (size_t)b * dst_stride;

    double f;
    if (!row_factor(mode, factor, b, &f) || (guard_cents && !(fabsf(guard_cents[b]) <= kMaxCents))) {
        if (tid == 0) {
            __hip_atomic_fetch_or(status, SIR_STATUS_PERTURB, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (dst_len) dst_len[b] = 0;
        }
        for (int i = tid; i < cap; i += kThreads) y[i] = 0.0f;
        return;
    }
    // shifted sample i of the clip (x_s[i] = x[i - shift] inside [0, L))
    auto xs = [&](int i) -> float {
        const int s = i - sh;
        return (i >= 0 && i < L && s >= 0 && s < L) ? to_f32<WT>(x[s]) : 0.0f;
    };
    if (f == 1.0) {                                          // effect not drawn: the (shifted) clip as it is
        const int n = L < cap ? L : cap;
        if (tid == 0 && dst_len) dst_len[b] = n;
        for (int i = tid; i < cap; i += kThreads) y[i] = i < n ? xs(i) : 0.0f;
        return;
    }

    const int N = (int)((double)L / f + 0.5);
    const int Nc = N < cap ? N : cap;
    if (tid == 0 && dst_len) dst_len[b] = Nc;
    for (int i = Nc + tid; i < cap; i += kThreads) y[i] = 0.0f;
    const int nseg = (Nc + H - 1) / H;
    const int R = W + S, hw = W / 2;
    const float invO = 1.0f / (float)O;

    for (int r = 0; r < kPer; ++r) {                         // window of segment 0 (p_0 = 0)
        const int e = tid + kThreads * r;
        if (e < R) reg[0][e] = xs(e - hw);
    }
    __syncthreads();

    for (int j = 0; j < nseg; ++j) {
        const int cur = j & 1;
        const bool more = j + 1 < nseg;
        float pre[kPer];
        if (more) {                                          // next window: issued now, stored after the search
            const int pn = (int)(f * (double)(j + 1) * (double)H + 0.5);
#pragma unroll
            for (int r = 0; r < kPer; ++r) {
                const int e = tid + kThreads * r;
                pre[r] = e < R ? xs(pn + e - hw) : 0.0f;
            }
        }
        int off = hw;
        if (j > 0) {
            float best = INFINITY;
            int bi = W;                                      // sentinel: loses to every candidate
            const float* o = ob[cur];
            for (int i = tid; i < W; i += kThreads) {
                const float* zr = &reg[cur][i];
                float acc = 0.0f;
#pragma unroll 8
                for (int m = 0; m < O; ++m) {
                    const float d = zr[m] - o[m];
                    acc = fmaf(d, d, acc);
                }
                if (acc < best) { best = acc; bi = i; }
            }
#pragma unroll
            for (int s = SIR_WAVE / 2; s > 0; s >>= 1) {
                const float ov = __shfl_xor(best, s);
                const int oi = __shfl_xor(bi, s);
                if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            if ((tid & (SIR_WAVE - 1)) == 0) { rv[tid / SIR_WAVE] = best; ri[tid / SIR_WAVE] = bi; }
            __syncthreads();
            best = rv[0]; bi = ri[0];
#pragma unroll
            for (int w = 1; w < kThreads / SIR_WAVE; ++w)
                if (rv[w] < best || (rv[w] == best && ri[w] < bi)) { best = rv[w]; bi = ri[w]; }
            off = bi < W ? bi : 0;                           // no finite cost at all (NaN / inf input): candidate 0
        }
        if (tid == 0 && offsets && j < max_segments) offsets[((size_t)b * 2 + pass) * max_segments + j] = off;

        const float* zq = &reg[cur][off];                    // z[q ..], q = p_j + off; q + S <= p_j + W - 1 + S
        const float* oc = ob[cur];
        const bool fade = j > 0;
        const int base = j * H;
        const int cnt = Nc - base < H ? Nc - base : H;
        auto val = [&](int m) -> float {
            if (fade && m < O) { const float w = (float)m * invO; return oc[m] * (1.0f - w) + zq[m] * w; }
            return zq[m];
        };
        if (vec && cnt == H) {                               // 16-byte stores (H % 4 == 0, rows 16-byte aligned)
            for (int t = tid; t < H / 4; t += kThreads) {
                const int m = 4 * t;
                *reinterpret_cast<float4*>(y + base + m) = make_float4(val(m), val(m + 1), val(m + 2), val(m + 3));
            }
        } else {
            for (int m = tid; m < cnt; m += kThreads) y[base + m] = val(m);
        }
        for (int m = tid; m < O; m += kThreads) ob[cur ^ 1][m] = zq[H + m];
        if (more) {
#pragma unroll
            for (int r = 0; r < kPer; ++r) {
                const int e = tid + kThreads * r;
                if (e < R) reg[cur ^ 1][e] = pre[r];
            }
        }
        __syncthreads();
    }
}

// Pitch resample: s (the pitch pass's stretched rows, s_len[b] samples) -> y[n] = sum_k s[k] h(n d - k), n < min(L, cap),
// zero to cap.  Rows with 0 cents copy s (which is then the shifted clip); rows outside the cents range are zero.
__global__ __launch_bounds__(kThreads) void pitch_resample_kernel(const float* __restrict__ s, long long s_stride, const int* __restrict__ s_len,
                                                                  const int* __restrict__ lengths, int max_len, const float* __restrict__ cents,
                                                                  float* __restrict__ dst, long long dst_stride, int cap,
                                                                  int* __restrict__ dst_len) {
    __shared__ float4 tab[2 * kTab + 1];     // i in [-kTab, kTab]: cos(pi b i), sin(pi b i), cos(pi b i / 6), sin(pi b i / 6)
    const int b = blockIdx.y;
    const int n = blockIdx.x * kThreads + threadIdx.x;
    int L = lengths ? lengths[b] : max_len;
    L = L < 0 ? 0 : (L > max_len ? max_len : L);
    const float c = cents[b];
    const bool bad = !(fabsf(c) <= kMaxCents);
    const int n_out = bad ? 0 : (L < cap ? L : cap);
    if (n == 0 && dst_len) dst_len[b] = n_out;
    const float* sr = s + (size_t)b * s_stride;
    float* y = dst + (size_t)b * dst_stride;
    if (bad || c == 0.0f) {                                  // uniform per block
        if (n < cap) y[n] = n < n_out ? sr[n] : 0.0f;
        return;
    }
    const double d = exp2((double)c / 1200.0);
    const double bd = 0.99 * (d > 1.0 ? 1.0 / d : 1.0);
    if (threadIdx.x < 2 * kTab + 1) {
        const double i = (double)((int)threadIdx.x - kTab);
        tab[threadIdx.x] = make_float4((float)cospi(bd * i), (float)sinpi(bd * i), (float)cospi(bd * i / 6.0), (float)sinpi(bd * i / 6.0));
    }
    __syncthreads();
    if (n >= cap) return;
    float acc = 0.0f;
    if (n < n_out) {
        const int Ls = s_len[b];
        const double R = 6.0 / bd;
        const double pos = (double)n * d;
        const double kd = rint(pos);
        const int k0 = (int)kd;
        const float fr = (float)(pos - kd);
        int kmin = (int)ceil(pos - R), kmax = (int)floor(pos + R);
        kmin = kmin < 0 ? 0 : kmin;
        kmax = kmax > Ls - 1 ? Ls - 1 : kmax;
        kmin = kmin < k0 - kTab ? k0 - kTab : kmin;          // (never binds: |k0 - k| <= 7)
        kmax = kmax > k0 + kTab ? k0 + kTab : kmax;
        const float bf = (float)bd;
        float sa, ca, s6, c6;
        sincospif(bf * fr, &sa, &ca);
        sincospif(bf * fr * (1.0f / 6.0f), &s6, &c6);
        const float kPi = 3.14159265358979323846f;
        for (int k = kmin; k <= kmax; ++k) {
            const int i = k0 - k;                            // n d - k = fr + i
            const float4 t4 = tab[i + kTab];
            const float t = bf * (fr + (float)i);
            const float sn = sa * t4.x + ca * t4.y;          // sin(pi b fr + pi b i)
            const float sinc = t == 0.0f ? 1.0f : sn * __builtin_amdgcn_rcpf(kPi * t);
            const float win = 0.5f + 0.5f * (c6 * t4.z - s6 * t4.w);    // cos(pi t / 12)^2 = (1 + cos(pi t / 6)) / 2
            acc = fmaf(sr[k], bf * sinc * win, acc);
        }
    }
    y[n] = acc;
}

struct WsLayout { size_t s_off, y_off, slen_off, total; long long s_stride, y_stride; };

WsLayout ws_layout(int batch, int max_len) {
    WsLayout w;
    w.s_stride = (long long)sir_align_up((size_t)(max_len * kMaxStretch + 1.0) + 4, 64);
    w.y_stride = (long long)sir_align_up((size_t)max_len, 64);
    w.s_off = 0;
    w.y_off = sir_align_up(w.s_off + (size_t)batch * w.s_stride * sizeof(float), 256);
    w.slen_off = sir_align_up(w.y_off + (size_t)batch * w.y_stride * sizeof(float), 256);
    w.total = sir_align_up(w.slen_off + (size_t)batch * sizeof(int), 256);
    return w;
}

template <typename WT>
void launch_wsola(hipStream_t st, const WT* src, long long src_stride, const int* lengths, int max_len, const int* shift, int mode,
                  const float* factor, float* dst, long long dst_stride, int cap, int vec, int* dst_len, int* offsets, int max_segments,
                  int pass, unsigned int* status, const Geom& g, int batch, const float* guard_cents = nullptr) {
    hipLaunchKernelGGL(wsola_kernel<WT>, dim3(batch), dim3(kThreads), 0, st, src, src_stride, lengths, max_len, shift, mode, factor, dst,
                       dst_stride, cap, vec, dst_len, offsets, max_segments, pass, status, g.S, g.W, g.O, g.H, guard_cents);
}

template <typename WT>
int perturb_impl(sir_handle* h, const WT* wave, int64_t wave_stride, const int32_t* lengths, int batch, int max_len, const int32_t* shift,
                 const float* pitch_cents, const float* tempo, float* out, int64_t out_stride, int max_out_len, int32_t* out_lengths,
                 int32_t* offsets_out, int max_segments, void* workspace, hipStream_t st) {
    const Geom g = geom_for(h->cfg.sample_rate);
    const int out_vec = ((uintptr_t)out % 16 == 0 && out_stride % 4 == 0 && g.H % 4 == 0) ? 1 : 0;
    if (!pitch_cents) {
        launch_wsola<WT>(st, wave, (long long)wave_stride, lengths, max_len, shift, tempo ? kModeTempo : kModeCopy, tempo, out,
                         (long long)out_stride, max_out_len, out_vec, out_lengths, offsets_out, max_segments, 1, h->status, g, batch);
        return sir_check_hip(hipGetLastError(), "wsola_kernel");
    }
    const WsLayout w = ws_layout(batch, max_len);
    char* ws = (char*)workspace;
    float* s = (float*)(ws + w.s_off);
    float* yb = (float*)(ws + w.y_off);
    int* slen = (int*)(ws + w.slen_off);
    const int ws_vec = g.H % 4 == 0 ? 1 : 0;                 // workspace rows: 256-byte aligned base, strides % 64 == 0
    launch_wsola<WT>(st, wave, (long long)wave_stride, lengths, max_len, shift, kModeCents, pitch_cents, s, w.s_stride, (int)w.s_stride,
                     ws_vec, slen, offsets_out, max_segments, 0, h->status, g, batch);
    int rc = sir_check_hip(hipGetLastError(), "wsola_kernel (pitch)");
    if (rc != SIR_OK) return rc;
    float* rdst = tempo ? yb : out;
    const long long rstride = tempo ? w.y_stride : (long long)out_stride;
    const int rcap = tempo ? (int)w.y_stride : max_out_len;
    hipLaunchKernelGGL(pitch_resample_kernel, dim3((rcap + kThreads - 1) / kThreads, batch), dim3(kThreads), 0, st, (const float*)s,
                       w.s_stride, (const int*)slen, lengths, max_len, pitch_cents, rdst, rstride, rcap, tempo ? nullptr : out_lengths);
    rc = sir_check_hip(hipGetLastError(), "pitch_resample_kernel");
    if (rc != SIR_OK || !tempo) return rc;
    launch_wsola<float>(st, yb, w.y_stride, lengths, max_len, nullptr, kModeTempo, tempo, out, (long long)out_stride, max_out_len, out_vec,
                        out_lengths, offsets_out, max_segments, 1, h->status, g, batch, pitch_cents);
    return sir_check_hip(hipGetLastError(), "wsola_kernel (speed)");
}

}  // namespace

extern "C" int sir_perturb_out_len(int length, float tempo) {
    if (length < 0 || !(tempo > 0.0f)) return -1;
    if (tempo == 1.0f) return length;
    return (int)((double)length / (double)tempo + 0.5);
}

extern "C" size_t sir_perturb_workspace_bytes(const sir_handle* h, int batch, int max_len) {
    if (!h || batch <= 0 || max_len <= 0) return 0;
    return ws_layout(batch, max_len).total;
}

extern "C" int sir_wave_perturb(sir_handle* h, const void* wave, int wave_dtype, int64_t wave_stride, const int32_t* lengths, int batch,
                                int max_len, const int32_t* shift, const float* pitch_cents, const float* tempo, float* out,
                                int64_t out_stride, int max_out_len, int32_t* out_lengths, int32_t* offsets_out, int max_segments,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !wave || !out) { sir_set_error("sir_wave_perturb: NULL argument"); return SIR_EINVAL; }
    if (batch <= 0 || batch > 65535 || max_len <= 0 || max_out_len <= 0 || wave_stride < max_len || out_stride < max_out_len) {
        sir_set_error("sir_wave_perturb: bad sizes (batch %d, max_len %d, wave_stride %lld, max_out_len %d, out_stride %lld)", batch,
                      max_len, (long long)wave_stride, max_out_len, (long long)out_stride);
        return SIR_EINVAL;
    }
    if (!sir_wave_elem_bytes(wave_dtype)) { sir_set_error("sir_wave_perturb: bad wave_dtype %d", wave_dtype); return SIR_EINVAL; }
    if (offsets_out && max_segments <= 0) { sir_set_error("sir_wave_perturb: offsets_out needs max_segments > 0"); return SIR_EINVAL; }
    const int sr = h->cfg.sample_rate;
    const Geom g = sr > 0 ? geom_for(sr) : Geom{0, 0, 0, 0};
    if (sr < 8000 || sr > kMaxRate || g.W + g.S > kMaxRegion || g.O > kMaxO || g.W < 1 || g.H < g.O) {
        sir_set_error("sir_wave_perturb: sample rate %d Hz is outside [8000, %d]", sr, kMaxRate);
        return SIR_EUNSUPPORTED;
    }
    if (pitch_cents) {
        const size_t need = ws_layout(batch, max_len).total;
        if (!workspace || workspace_bytes < need || (uintptr_t)workspace % 256 != 0) {
            sir_set_error("sir_wave_perturb: workspace of %zu bytes at %p, need %zu bytes, 256-byte aligned", workspace_bytes, workspace, need);
            return SIR_ENOMEM;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (offsets_out)
        SIR_HIP_TRY(hipMemsetAsync(offsets_out, 0xff, (size_t)batch * 2 * max_segments * sizeof(int32_t), st));   // -1 = unused
    return sir_wave_dispatch(wave_dtype, [&](auto tag) {
        using WT = decltype(tag);
        return perturb_impl<WT>(h, (const WT*)wave, wave_stride, lengths, batch, max_len, shift, pitch_cents, tempo, out, out_stride, max_out_len,
                                out_lengths, offsets_out, max_segments, workspace, st);
    });
}
