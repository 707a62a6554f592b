// Standalone timing/consistency harness of the bf16x6 convolution kernels (developer tool, not part
// of the library): random NHWC input and weights at the batch-256 shapes of conv2 / conv3, both
// kernel generations, HIP-event timing, bitwise comparison, timing-only knock-outs.
//   build: make -C speech-intent-recognizer_amd/csrc tools     run (GPU box): lib/bench_conv
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "../../speech-intent-recognizer_amd/csrc/bf16x6_kernels.h"
#include "legacy_kernels.h"
#include "../../speech-intent-recognizer_amd/csrc/conv_wino_bf16x6_kernel.h"
#include "../../speech-intent-recognizer_amd/csrc/conv_wino2_f16x3_kernel.h"
#include "conv_direct_f16x3_kernel.h"

#define CK_(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1); } } while (0)

// the library keeps the Winograd kernel's geometry in its conv plan and opts in to the dynamic LDS through its handle; the harness
// does both here, per instantiation (`attr_done`)
template <int CIN, int COUT, int OUT_MODE, int DBG = 0, int PRIO = 3>
static hipError_t launch_conv_wino2(hipStream_t st, bool* attr_done, const float* x, const unsigned short* wpb, const float* scale, const float* shift,
                                    float* out, int B, int H, int W, float2* stats, const float* zeros) {
    Wino2Geo g;
    if (!wino2_geo(B, H, W, CIN > COUT ? CIN : COUT, &g)) return hipErrorInvalidValue;
    if (!*attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)conv3x3_wino2_f16x3_kernel<CIN, COUT, OUT_MODE, DBG, PRIO>, hipFuncAttributeMaxDynamicSharedMemorySize, W2_LDS_BYTES);
        if (e != hipSuccess) return e;
        *attr_done = true;
    }
    return launch_conv_wino2<CIN, COUT, OUT_MODE, DBG, PRIO>(st, g, x, wpb, scale, shift, out, stats, zeros);
}

template <typename F>
static float time_us(hipStream_t st, int reps, F launch) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 40; ++i) launch();      // long warm-up: the clocks ramp over the first milliseconds of load
    hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) launch();
    hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    CK_(hipGetLastError());
    return ms * 1000.0f / reps;
}

template <int CIN, int COUT, int PR, int PC, int OUT_MODE>
static void run(const char* name, int B, int H, int W) {
    const int Hp = H / 2, Wp = W / 2, reps = 60;
    const size_t nx = (size_t)B * H * W * CIN, nw = (size_t)COUT * CIN * 9;
    const size_t nout = OUT_MODE == 2 ? (size_t)B * H * W * COUT : (size_t)B * Hp * Wp * COUT;   // raw mode writes every pixel
    std::vector<float> hx(nx), hw(nw), hs(COUT), ht(COUT);
    srand(7);
    for (auto& v : hx) v = rand() / (float)RAND_MAX * 2.0f - 0.3f;
    for (auto& v : hw) v = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    for (int c = 0; c < COUT; ++c) { hs[c] = 0.5f + rand() / (float)RAND_MAX; ht[c] = rand() / (float)RAND_MAX - 0.5f; }
    float *dx, *dw, *ds, *dt, *o1, *o2;
    unsigned short* wpb;
    CK_(hipMalloc(&dx, nx * 4)); CK_(hipMalloc(&dw, nw * 4)); CK_(hipMalloc(&ds, COUT * 4)); CK_(hipMalloc(&dt, COUT * 4));
    CK_(hipMalloc(&o1, nout * 4)); CK_(hipMalloc(&o2, nout * 4)); CK_(hipMalloc(&wpb, nw * 6));
    CK_(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
    CK_(hipMemcpy(ds, hs.data(), COUT * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dt, ht.data(), COUT * 4, hipMemcpyHostToDevice));
    hipStream_t st; CK_(hipStreamCreate(&st));
    hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3((CIN * 9 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpb, CIN, COUT);
    const dim3 grid((W + 4 * PC - 1) / (4 * PC), (H + 8 * PR - 1) / (8 * PR), B);
    const double gf = 2.0 * B * H * W * (double)COUT * CIN * 9 * 1e-9;
    CK_(hipMemset(o1, 0, nout * 4)); CK_(hipMemset(o2, 0, nout * 4));
    float t1 = 0.0f;
    if constexpr ((PR * PC) % 4 == 0) {
        constexpr size_t lds = conv_bf16x6_lds_bytes(PR, PC);
        t1 = time_us(st, reps, [&] {
            hipLaunchKernelGGL((conv3x3_bf16x6_kernel<CIN, COUT, PR, PC, OUT_MODE, (PR * PC) / 4>), grid, dim3(256), lds, st, (const float*)dx, (const unsigned short*)wpb,
                               (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, (float2*)nullptr); });
    } else {
        // no gen-1 kernel for this tile: the consistency check is against the 4x2-patch channel-split kernel
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, 4, 2, OUT_MODE, 0>), dim3((W + 7) / 8, (H + 31) / 32, B), dim3(256), conv_ns_lds_bytes(4, 2), st,
                           (const float*)dx, (const unsigned short*)wpb, (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, (float2*)nullptr);
    }
    constexpr size_t lds_ns = conv_ns_lds_bytes(PR, PC);       // the product kernel's half-major, unpadded LDS image
    float t2 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, OUT_MODE, 0>), grid, dim3(256), lds_ns, st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    CK_(hipStreamSynchronize(st));
    std::vector<float> h1(nout), h2(nout);
    CK_(hipMemcpy(h1.data(), o1, nout * 4, hipMemcpyDeviceToHost)); CK_(hipMemcpy(h2.data(), o2, nout * 4, hipMemcpyDeviceToHost));
    double d = 0, mx = 0;
    for (size_t i = 0; i < nout; ++i) { d = fmax(d, fabs((double)h1[i] - h2[i])); mx = fmax(mx, fabs(h1[i])); }
    printf("%s: B=%d %dx%d %d->%d  %.2f GF  grid %dx%dx%d\n", name, B, H, W, CIN, COUT, gf, grid.x, grid.y, grid.z);
    printf("  gen1 (pixels split over waves)   %8.1f us  %7.1f TF\n", t1, gf * 1e3 / t1);
    printf("  gen2 (channels split over waves) %8.1f us  %7.1f TF   max |gen1 - gen2| = %.3e (max |out| %.2f)\n", t2, gf * 1e3 / t2, d, mx);
    float t3 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, OUT_MODE, 1>), grid, dim3(256), lds_ns, st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    float t4 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, OUT_MODE, 2>), grid, dim3(256), lds_ns, st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    float t5 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, OUT_MODE, 3>), grid, dim3(256), lds_ns, st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    auto variant = [&](auto minb, auto pipe, auto db) {
        constexpr int DBv = decltype(db)::value;
        constexpr size_t ldsv = conv_ns_lds_bytes(PR, PC, DBv ? 2 : 1);
        auto kfn = conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, OUT_MODE, 0, decltype(minb)::value, decltype(pipe)::value, DBv>;
        if (ldsv > 64 * 1024) CK_(hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsv));
        CK_(hipMemsetAsync(o2, 0, nout * 4, st));
        const float t = time_us(st, reps, [&] {
            hipLaunchKernelGGL(kfn, grid, dim3(256), ldsv, st,
                               (const float*)dx, (const unsigned short*)wpb, (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
        if (DBv) {                                              // the double-buffered variants are new code: compare bitwise with o1
            CK_(hipStreamSynchronize(st));
            CK_(hipMemcpy(h2.data(), o2, nout * 4, hipMemcpyDeviceToHost));
            size_t bad = 0;
            for (size_t i = 0; i < nout; ++i) bad += h1[i] != h2[i];
            if (bad) printf("  !! double-buffered variant differs from the reference output in %zu values\n", bad);
        }
        return t;
    };
    using std::integral_constant;
    using I0 = integral_constant<int, 0>; using I1 = integral_constant<int, 1>; using I2 = integral_constant<int, 2>;
    using I3 = integral_constant<int, 3>; using I4 = integral_constant<int, 4>;
    constexpr bool L4 = PR * PC * COUT <= 512;
    printf("  workgroups/CU (LDS %zu B per buffer):\n", lds_ns);
    printf("    plain                       2: %.1f  3: %.1f", variant(I2{}, I0{}, I0{}), variant(I3{}, I0{}, I0{}));
    if (L4) printf("  4: %.1f", variant(I4{}, I0{}, I0{}));
    printf("\n    fragments pipelined         2: %.1f  3: %.1f", variant(I2{}, I1{}, I0{}), variant(I3{}, I1{}, I0{}));
    if (L4) printf("  4: %.1f", variant(I4{}, I1{}, I0{}));
    printf("\n    double-buffered staging     2: %.1f  3: %.1f", variant(I2{}, I0{}, I1{}), variant(I3{}, I0{}, I1{}));
    if (L4) printf("  4: %.1f", variant(I4{}, I0{}, I1{}));
    printf("\n    both                        2: %.1f  3: %.1f", variant(I2{}, I1{}, I1{}), variant(I3{}, I1{}, I1{}));
    if (L4) printf("  4: %.1f", variant(I4{}, I1{}, I1{}));
    printf(" us\n");
    printf("  gen2 knock-outs (timing only): weights once %.1f us, tile staged once %.1f us, both %.1f us\n", t3, t4, t5);
    hipFree(dx); hipFree(dw); hipFree(ds); hipFree(dt); hipFree(o1); hipFree(o2); hipFree(wpb);
}

// Winograd F(2x2, 3x3) conv2 against the direct kernel: same input, same weights, pooled BN + ReLU output and raw output
static void run_wino(int B, int H, int W) {
    constexpr int CIN = 32, COUT = 64;
    const int Hp = H / 2, Wp = W / 2, reps = 60;
    const size_t nx = (size_t)B * H * W * CIN, nw = (size_t)COUT * CIN * 9, npool = (size_t)B * Hp * Wp * COUT, nraw = (size_t)B * H * W * COUT;
    std::vector<float> hx(nx), hw(nw), hs(COUT), ht(COUT);
    srand(11);
    for (auto& v : hx) v = rand() / (float)RAND_MAX * 2.0f - 0.3f;
    for (auto& v : hw) v = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    for (int c = 0; c < COUT; ++c) { hs[c] = 0.5f + rand() / (float)RAND_MAX; ht[c] = rand() / (float)RAND_MAX - 0.5f; }
    float *dx, *dw, *ds, *dt, *o1, *o2;
    unsigned short *wpb, *wpw;
    float2 *st1, *st2;
    CK_(hipMalloc(&dx, nx * 4)); CK_(hipMalloc(&dw, nw * 4)); CK_(hipMalloc(&ds, COUT * 4)); CK_(hipMalloc(&dt, COUT * 4));
    CK_(hipMalloc(&o1, nraw * 4)); CK_(hipMalloc(&o2, nraw * 4)); CK_(hipMalloc(&wpb, nw * 6)); CK_(hipMalloc(&wpw, (size_t)COUT * CIN * 16 * 6));
    const dim3 gd((W + 7) / 8, (H + 31) / 32, B), gw(((W + 1) / 2 + 1) / 2, (H + 31) / 32, B);
    CK_(hipMalloc(&st1, (size_t)gd.x * gd.y * B * COUT * 8)); CK_(hipMalloc(&st2, (size_t)gw.x * gw.y * B * COUT * 8));
    CK_(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
    CK_(hipMemcpy(ds, hs.data(), COUT * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dt, ht.data(), COUT * 4, hipMemcpyHostToDevice));
    hipStream_t st; CK_(hipStreamCreate(&st));
    hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3((CIN * 9 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpb, CIN, COUT);
    hipLaunchKernelGGL(prep_conv_w_wino_bf16x3_kernel, dim3((CIN * 16 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpw, CIN, COUT);
    printf("conv2 as Winograd F(2x2,3x3): B=%d %dx%d %d->%d  grid %dx%dx%d (direct: %dx%dx%d)\n", B, H, W, CIN, COUT, gw.x, gw.y, gw.z, gd.x, gd.y, gd.z);
    auto compare = [&](const char* what, size_t n, bool is_stats) {
        std::vector<float> h1(n), h2(n);
        CK_(hipStreamSynchronize(st));
        CK_(hipMemcpy(h1.data(), o1, n * 4, hipMemcpyDeviceToHost)); CK_(hipMemcpy(h2.data(), o2, n * 4, hipMemcpyDeviceToHost));
        double d = 0, mx = 0, sq = 0;
        for (size_t i = 0; i < n; ++i) { d = fmax(d, fabs((double)h1[i] - h2[i])); mx = fmax(mx, fabs(h1[i])); sq += (double)h1[i] * h1[i]; }
        printf("  %-28s max |direct - winograd| = %.3e  (max |out| %.3f, rms %.3f)\n", what, d, mx, sqrt(sq / n));
        (void)is_stats;
    };
    // pooled BN + ReLU output
    CK_(hipMemsetAsync(o1, 0, nraw * 4, st)); CK_(hipMemsetAsync(o2, 0, nraw * 4, st));
    const float t1 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, 4, 2, 0, 0, 3, 0>), gd, dim3(256), conv_ns_lds_bytes(4, 2), st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, (float2*)nullptr); });
    const float t2 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 2>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dx, (const unsigned short*)wpw,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    const double gf = 2.0 * B * H * W * (double)COUT * CIN * 9 * 1e-9;
    const float t2b = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 3>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dx, (const unsigned short*)wpw,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
    if (B >= 64) {
        // the same launches over FOUR rotating inputs (4 x 105 MB: more than the 256 MB MALL holds), as inside the model where every
        // launch reads activations the previous kernel just wrote: the timings above re-read one input that stays cached
        float* dxr[4];
        for (int k = 0; k < 4; ++k) { CK_(hipMalloc(&dxr[k], nx * 4)); CK_(hipMemcpyAsync(dxr[k], dx, nx * 4, hipMemcpyDeviceToDevice, st)); }
        int rot = 0;
        const float r1 = time_us(st, reps, [&] {
            hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, 4, 2, 0, 0, 3, 0>), gd, dim3(256), conv_ns_lds_bytes(4, 2), st, (const float*)dxr[rot++ & 3], (const unsigned short*)wpb,
                               (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, (float2*)nullptr); });
        const float r2 = time_us(st, reps, [&] {
            hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 3, 0>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dxr[rot++ & 3], (const unsigned short*)wpw,
                               (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
        const float r3 = time_us(st, reps, [&] {
            hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 3, 1>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dxr[rot++ & 3], (const unsigned short*)wpw,
                               (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
        const float r4 = time_us(st, reps, [&] {
            hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 2, 1>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dxr[rot++ & 3], (const unsigned short*)wpw,
                               (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
        printf("  rotating inputs:   direct %.1f us   winograd %.1f us, with the XCD-aware block order %.1f us (2 workgroups/CU: %.1f us)\n", r1, r2, r3, r4);
        auto ko = [&](auto kc) {
            return time_us(st, reps, [&] {
                hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 0, 3, 1, decltype(kc)::value>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dxr[rot++ & 3],
                                   (const unsigned short*)wpw, (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, (float2*)nullptr); });
        };
        using std::integral_constant;
        printf("  winograd knock-outs (timing only): no loads %.1f, no transform/split/LDS writes %.1f, no MFMAs %.1f, no stores %.1f, loads+transform %.1f, all but MFMA %.1f, all %.1f us\n",
               ko(integral_constant<int, 1>{}), ko(integral_constant<int, 2>{}), ko(integral_constant<int, 4>{}), ko(integral_constant<int, 8>{}),
               ko(integral_constant<int, 3>{}), ko(integral_constant<int, 11>{}), ko(integral_constant<int, 15>{}));
        printf("  more knock-outs: weights loaded once %.1f, weights once + no patch loads %.1f, weights once + no loads + no transform %.1f us\n",
               ko(integral_constant<int, 16>{}), ko(integral_constant<int, 17>{}), ko(integral_constant<int, 19>{}));
        for (int k = 0; k < 4; ++k) (void)hipFree(dxr[k]);
    }
    printf("  BN + ReLU + pool:  direct %.1f us (%.1f TF)   winograd %.1f us (%.1f TF algorithmic); at 3 workgroups/CU: %.1f us\n", t1, gf * 1e3 / t1, t2, gf * 1e3 / t2, t2b);
    compare("pooled output", npool, false);
    // raw output + statistics
    CK_(hipMemsetAsync(o1, 0, nraw * 4, st)); CK_(hipMemsetAsync(o2, 0, nraw * 4, st));
    const float t3 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, 4, 2, 2, 0, 3, 0>), gd, dim3(256), conv_ns_lds_bytes(4, 2), st, (const float*)dx, (const unsigned short*)wpb,
                           (const float*)nullptr, (const float*)nullptr, o1, H, W, Hp, Wp, st1); });
    const float t4 = time_us(st, reps, [&] {
        hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, 2>), gw, dim3(256), WINO_LDS_BYTES, st, (const float*)dx, (const unsigned short*)wpw,
                           (const float*)nullptr, (const float*)nullptr, o2, H, W, Hp, Wp, st2); });
    printf("  raw + statistics:  direct %.1f us   winograd %.1f us\n", t3, t4);
    compare("raw output", nraw, false);
    {   // channel statistics: totals over the workgroups
        const size_t n1 = (size_t)gd.x * gd.y * B, n2 = (size_t)gw.x * gw.y * B;
        std::vector<float2> s1(n1 * COUT), s2(n2 * COUT);
        CK_(hipMemcpy(s1.data(), st1, s1.size() * 8, hipMemcpyDeviceToHost)); CK_(hipMemcpy(s2.data(), st2, s2.size() * 8, hipMemcpyDeviceToHost));
        double worst = 0;
        for (int c = 0; c < COUT; ++c) {
            double a = 0, aq = 0, bsum = 0, bq = 0;
            for (size_t k = 0; k < n1; ++k) { a += s1[k * COUT + c].x; aq += s1[k * COUT + c].y; }
            for (size_t k = 0; k < n2; ++k) { bsum += s2[k * COUT + c].x; bq += s2[k * COUT + c].y; }
            worst = fmax(worst, fmax(fabs(a - bsum) / (fabs(a) + 1.0), fabs(aq - bq) / (fabs(aq) + 1.0)));
        }
        printf("  channel statistics: worst relative difference of (sum, sum of squares) = %.3e\n", worst);
    }
    (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(ds); (void)hipFree(dt); (void)hipFree(o1); (void)hipFree(o2); (void)hipFree(wpb); (void)hipFree(wpw);
    (void)hipFree(st1); (void)hipFree(st2);
}

// `bench_conv loop [seconds]`: the product conv2 launch back to back, for sampling clocks and power from outside
// (rocm-smi --showclocks --showpower in a second shell) -- is the kernel running at the power cap?
static void load_loop(double seconds) {
    const int B = 256, H = 32, W = 100, CIN = 32, COUT = 64;
    const size_t nx = (size_t)B * H * W * CIN, nw = (size_t)COUT * CIN * 9, nout = (size_t)B * (H / 2) * (W / 2) * COUT;
    float *dx, *dw, *ds, *dt, *o;
    unsigned short* wpb;
    CK_(hipMalloc(&dx, nx * 4)); CK_(hipMalloc(&dw, nw * 4)); CK_(hipMalloc(&ds, COUT * 4)); CK_(hipMalloc(&dt, COUT * 4));
    CK_(hipMalloc(&o, nout * 4)); CK_(hipMalloc(&wpb, nw * 6));
    std::vector<float> hx(nx), hw(nw);
    for (auto& v : hx) v = rand() / (float)RAND_MAX * 2.0f - 0.3f;
    for (auto& v : hw) v = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    CK_(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
    CK_(hipMemset(ds, 0, COUT * 4)); CK_(hipMemset(dt, 0, COUT * 4));
    hipStream_t st; CK_(hipStreamCreate(&st));
    hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3((CIN * 9 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpb, CIN, COUT);
    const dim3 grid((W + 7) / 8, 1, B);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    double elapsed = 0;
    while (elapsed < seconds) {
        hipEventRecord(e0, st);
        for (int i = 0; i < 1000; ++i)
            hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<32, 64, 4, 2, 0, 0, 3, 0>), grid, dim3(256), conv_ns_lds_bytes(4, 2), st, (const float*)dx,
                               (const unsigned short*)wpb, (const float*)ds, (const float*)dt, o, H, W, H / 2, W / 2, (float2*)nullptr);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float ms = 0; hipEventElapsedTime(&ms, e0, e1);
        elapsed += ms * 1e-3;
        printf("conv2 x1000: %.1f us per launch (t = %.2f s)\n", ms, elapsed);
        fflush(stdout);
    }
}

// Second-generation Winograd kernel (conv_wino2_f16x3_kernel.h) against the direct kernel: same input, same weights.
//   MODE 0: pooled NHWC, 1: pooled GRU layout + f16x2 planes, 2: raw + statistics, 3: raw (data gradient: DGRAD weights)
template <int CIN, int COUT, int PR, int PC, int MODE, bool DGRAD, int MINB>
static void run_wino2(const char* name, int B, int H, int W, int reps = 60) {
    const int Hp = H / 2, Wp = W / 2;
    const size_t nx = (size_t)B * H * W * CIN, nw = (size_t)COUT * CIN * 9;
    const bool raw = MODE >= 2;
    const size_t nout = raw ? (size_t)B * H * W * COUT : (size_t)B * Hp * Wp * COUT;
    std::vector<float> hx(nx), hw(nw), hs(COUT), ht(COUT);
    srand(13);
    for (auto& v : hx) v = rand() / (float)RAND_MAX * 2.0f - 0.3f;
    for (auto& v : hw) v = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    for (int c = 0; c < COUT; ++c) { hs[c] = 0.5f + rand() / (float)RAND_MAX; ht[c] = rand() / (float)RAND_MAX - 0.5f; }
    float *dx, *dw, *ds, *dt, *o1, *o2;
    unsigned short *wpb, *wpw, *pl1 = nullptr, *pl2 = nullptr;
    Wino2Geo geo;
    if (!wino2_geo(B, H, W, CIN > COUT ? CIN : COUT, &geo)) { printf("%s: unsupported shape\n", name); return; }
    const dim3 gd((W + 4 * PC - 1) / (4 * PC), (H + 8 * PR - 1) / (8 * PR), B);
    float2 *st1 = nullptr, *st2 = nullptr;
    CK_(hipMalloc(&dx, nx * 4)); CK_(hipMalloc(&dw, nw * 4)); CK_(hipMalloc(&ds, COUT * 4)); CK_(hipMalloc(&dt, COUT * 4));
    CK_(hipMalloc(&o1, nout * 4)); CK_(hipMalloc(&o2, nout * 4)); CK_(hipMalloc(&wpb, nw * 6)); CK_(hipMalloc(&wpw, (size_t)COUT * CIN * 16 * 6));
    if (MODE == 1) { CK_(hipMalloc(&pl1, nout * 6)); CK_(hipMalloc(&pl2, nout * 6)); CK_(hipMemset(pl1, 0, nout * 6)); CK_(hipMemset(pl2, 0, nout * 6)); }
    if (MODE == 2) { CK_(hipMalloc(&st1, (size_t)gd.x * gd.y * B * COUT * 8)); CK_(hipMalloc(&st2, wino2_stat_blocks(B, H, W, 256) * COUT * 8)); }
    CK_(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
    CK_(hipMemcpy(ds, hs.data(), COUT * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dt, ht.data(), COUT * 4, hipMemcpyHostToDevice));
    hipStream_t st; CK_(hipStreamCreate(&st));
    // forward: weights [COUT][CIN][3][3]; data gradient: the layer's weights are [CIN][COUT][3][3] (forward cout = this CIN).
    // The direct kernel takes bf16x3 planes, the Winograd kernel (f16x3 arithmetic) f16x3 planes.
    unsigned int* dstat; CK_(hipMalloc(&dstat, 256)); CK_(hipMemset(dstat, 0, 256));
    if (DGRAD) {
        hipLaunchKernelGGL(prep_conv_wT_bf16x3_kernel, dim3((CIN * 9 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpb, COUT, CIN);
        hipLaunchKernelGGL(prep_conv_wT_wino_f16x3_kernel, dim3((CIN * 16 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpw, COUT, CIN, dstat);
    } else {
        hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3((CIN * 9 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpb, CIN, COUT);
        hipLaunchKernelGGL(prep_conv_w_wino_f16x3_kernel, dim3((CIN * 16 * COUT + 255) / 256), dim3(256), 0, st, (const float*)dw, wpw, CIN, COUT, dstat);
    }
    CK_(hipMemsetAsync(o1, 0, nout * 4, st)); CK_(hipMemsetAsync(o2, 0, nout * 4, st));
    constexpr int DM = MODE == 3 ? 2 : MODE;              // the direct kernel's raw mode
    constexpr int DB = (PR * PC <= 8 && MINB == 2) ? 1 : 0;
    bool attr = false;
    float* dzero; CK_(hipMalloc(&dzero, 4096)); CK_(hipMemset(dzero, 0, 4096));       // zero page of the DMA (>= CIN + 4 floats)
    auto direct = [&](const float* in) {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, PR, PC, DM, 0, MINB, 1, DB>), gd, dim3(256), conv_ns_lds_bytes(PR, PC, DB ? 2 : 1), st, in,
                           (const unsigned short*)wpb, (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, MODE == 1 ? (float2*)pl1 : st1); };
    auto wino2 = [&](const float* in) {
        CK_((launch_conv_wino2<CIN, COUT, MODE>(st, &attr, in, wpw, ds, dt, o2, B, H, W, MODE == 1 ? (float2*)pl2 : st2, dzero))); };
    direct(dx); wino2(dx);
    CK_(hipStreamSynchronize(st));
    {
        std::vector<float> h1(nout), h2(nout);
        CK_(hipMemcpy(h1.data(), o1, nout * 4, hipMemcpyDeviceToHost)); CK_(hipMemcpy(h2.data(), o2, nout * 4, hipMemcpyDeviceToHost));
        double d = 0, mx = 0, sq = 0; size_t bad = 0, first = (size_t)-1;
        for (size_t i = 0; i < nout; ++i) {
            const double e = fabs((double)h1[i] - h2[i]);
            if (e > 1e-4) { ++bad; if (first == (size_t)-1) first = i; }
            d = fmax(d, e); mx = fmax(mx, fabs(h1[i])); sq += (double)h1[i] * h1[i];
        }
        printf("%s: B=%d %dx%d %d->%d mode %d, %d tasks x %d\n  max |direct - wino2| = %.3e (max |out| %.3f, rms %.3f), %zu elements off by > 1e-4", name, B, H, W, CIN, COUT,
               MODE, geo.NS, COUT / 64, d, mx, sqrt(sq / nout), bad);
        if (bad) printf(" (first at %zu: %.6f vs %.6f)", first, h1[first], h2[first]);
        printf("\n");
        if (MODE == 1) {
            std::vector<unsigned short> p1(nout * 3), p2(nout * 3);
            CK_(hipMemcpy(p1.data(), pl1, nout * 6, hipMemcpyDeviceToHost)); CK_(hipMemcpy(p2.data(), pl2, nout * 6, hipMemcpyDeviceToHost));
            // planes of slightly different floats differ in their low parts: compare the reconstructed values
            double dp = 0;
            for (size_t i = 0; i < nout; ++i) {
                auto f = [](unsigned short u) { _Float16 hv; memcpy(&hv, &u, 2); return (double)(float)hv; };
                dp = fmax(dp, fabs(f(p1[i]) + f(p1[nout + i]) / 2048.0 - f(p2[i]) - f(p2[nout + i]) / 2048.0));
            }
            printf("  f16x2 planes (hi + lo / 2^11) of the following GEMM's operand: max difference %.3e\n", dp);
        }
        if (MODE == 2) {
            const size_t n1 = (size_t)gd.x * gd.y * B, n2 = wino2_stat_blocks(B, H, W, 256);
            std::vector<float2> s1(n1 * COUT), s2(n2 * COUT);
            CK_(hipMemcpy(s1.data(), st1, s1.size() * 8, hipMemcpyDeviceToHost)); CK_(hipMemcpy(s2.data(), st2, s2.size() * 8, hipMemcpyDeviceToHost));
            double worst = 0;
            for (int c = 0; c < COUT; ++c) {
                double a = 0, aq = 0, b2 = 0, bq = 0;
                for (size_t k = 0; k < n1; ++k) { a += s1[k * COUT + c].x; aq += s1[k * COUT + c].y; }
                for (size_t k = 0; k < n2; ++k) { b2 += s2[k * COUT + c].x; bq += s2[k * COUT + c].y; }
                worst = fmax(worst, fmax(fabs(a - b2) / fmax(1.0, fabs(a)), fabs(aq - bq) / fmax(1.0, fabs(aq))));
            }
            printf("  channel statistics: worst relative difference of (sum, sum of squares) = %.3e\n", worst);
        }
    }
    if (B >= 64) {
        float* dxr[4];
        for (int k = 0; k < 4; ++k) { CK_(hipMalloc(&dxr[k], nx * 4)); CK_(hipMemcpyAsync(dxr[k], dx, nx * 4, hipMemcpyDeviceToDevice, st)); }
        int rot = 0;
        const float t1 = time_us(st, reps, [&] { direct(dxr[rot++ & 3]); });
        const float t2 = time_us(st, reps, [&] { wino2(dxr[rot++ & 3]); });
        const double gf = 2.0 * B * H * W * (double)COUT * CIN * 9 * 1e-9;
        bool atp[3] = {false, false, false};
        const float tp1 = time_us(st, reps, [&] { CK_((launch_conv_wino2<CIN, COUT, MODE, 0, 1>(st, &atp[0], dxr[rot++ & 3], wpw, ds, dt, o2, B, H, W, MODE == 1 ? (float2*)pl2 : st2, dzero))); });
        const float tp2 = time_us(st, reps, [&] { CK_((launch_conv_wino2<CIN, COUT, MODE, 0, 3>(st, &atp[1], dxr[rot++ & 3], wpw, ds, dt, o2, B, H, W, MODE == 1 ? (float2*)pl2 : st2, dzero))); });
        printf("  rotating inputs: direct %.1f us (%.1f TF)   wino2 %.1f us (%.1f TF algorithmic); producers at s_setprio 1: %.1f, 3: %.1f us\n", t1, gf * 1e3 / t1, t2, gf * 1e3 / t2, tp1, tp2);
        for (int k = 0; k < 4; ++k) (void)hipFree(dxr[k]);
        // phase stamps of workgroup 0, second task (cycles relative to the first stamp): group A | group B
        bool attr2 = false;
        for (int rep = 0; rep < 3; ++rep)
            CK_((launch_conv_wino2<CIN, COUT, MODE, 1>(st, &attr2, dx, wpw, ds, dt, o2, B, H, W, MODE == 1 ? (float2*)pl2 : st2, dzero)));
        CK_(hipStreamSynchronize(st));
        {
            auto ko = [&](auto kc) {
                bool at = false;
                return time_us(st, reps, [&] { CK_((launch_conv_wino2<CIN, COUT, MODE, decltype(kc)::value>(st, &at, dx, wpw, ds, dt, o2, B, H, W, MODE == 1 ? (float2*)pl2 : st2, dzero))); });
            };
            using std::integral_constant;
            printf("  knock-outs (timing only, one cached input): full %.1f, no DMA %.1f, no transform %.1f, no MFMA %.1f, no epilogue %.1f, no transform+MFMA %.1f, only barriers+epilogue %.1f us\n",
                   ko(integral_constant<int, 32>{}), ko(integral_constant<int, 2>{}), ko(integral_constant<int, 4>{}), ko(integral_constant<int, 8>{}), ko(integral_constant<int, 16>{}),
                   ko(integral_constant<int, 12>{}), ko(integral_constant<int, 14>{}));
            printf("  more: weights loaded once %.1f, weights once + only barriers/epilogue %.1f, weights once + no epilogue %.1f us\n",
                   ko(integral_constant<int, 64>{}), ko(integral_constant<int, 78>{}), ko(integral_constant<int, 80>{}));
        }
        long long hs_[2][32];
        CK_(hipMemcpyFromSymbol(hs_, HIP_SYMBOL(w2_dbg_stamps), sizeof(hs_)));
        {
            long long hf_[8][8];
            CK_(hipMemcpyFromSymbol(hf_, HIP_SYMBOL(w2_dbg_fine), sizeof(hf_)));
            printf("  producer wave 0, steps 8..15, cycles from the step's top: DMA issued | raw patches read | V written | DMA wait over | barrier passed\n   ");
            for (int k = 0; k < 8; ++k) printf(" [%lld %lld %lld %lld %lld]", hf_[k][1] - hf_[k][0], hf_[k][2] - hf_[k][0], hf_[k][3] - hf_[k][0], hf_[k][4] - hf_[k][0], hf_[k][5] - hf_[k][0]);
            printf("\n");
        }
        for (int g = 0; g < 2; ++g) {
            printf("  stamps group %c:", g ? 'B' : 'A');
            for (int k = 0; k < 2 * (2 * (CIN / 16) + 1) + 5 && k < 32; ++k) printf(" %lld", hs_[g][k] - hs_[0][0]);
            printf("\n");
        }
    }
    hipFree(dx); hipFree(dw); hipFree(ds); hipFree(dt); hipFree(o1); hipFree(o2); hipFree(wpb); hipFree(wpw); hipFree(dstat);
    if (pl1) hipFree(pl1); if (pl2) hipFree(pl2); if (st1) hipFree(st1); if (st2) hipFree(st2);
    fflush(stdout);
}

// Round 4 experiment: the DIRECT convolution on the f16x3 arithmetic (conv_direct_f16x3_kernel.h: NT x MT register tile per wave) against the
// direct bf16x6 kernel (results) -- what a convolution without the Winograd input transform costs on the fp16 pipe.
template <int CIN, int COUT, int PR, int PC, int MODE, bool DGRAD, int NT, int MINB, int RPR, int RPC, int WR = 3, bool AH2 = true, int NW = 4>
static void run_direct16(const char* name, int B, int H, int W, int reps = 60) {
    const int Hp = H / 2, Wp = W / 2;
    const size_t nx = (size_t)B * H * W * CIN, nw = (size_t)COUT * CIN * 9;
    const size_t nout = MODE == 2 ? (size_t)B * H * W * COUT : (size_t)B * Hp * Wp * COUT;
    std::vector<float> hx(nx), hw(nw), hs(COUT), ht(COUT);
    srand(13);
    for (auto& v : hx) v = rand() / (float)RAND_MAX * 2.0f - 0.3f;
    for (auto& v : hw) v = (rand() / (float)RAND_MAX - 0.5f) * 0.2f;
    for (int c = 0; c < COUT; ++c) { hs[c] = 0.5f + rand() / (float)RAND_MAX; ht[c] = rand() / (float)RAND_MAX - 0.5f; }
    float *dx, *dw, *ds, *dt, *o1, *o2;
    unsigned short *wpb, *wph;
    float2 *st1 = nullptr, *st2 = nullptr;
    const dim3 gr((W + 4 * RPC - 1) / (4 * RPC), (H + 8 * RPR - 1) / (8 * RPR), B);     // the bf16x6 reference launch
    const dim3 gd((W + 4 * PC - 1) / (4 * PC), (H + 8 * PR - 1) / (8 * PR), B);
    CK_(hipMalloc(&dx, nx * 4)); CK_(hipMalloc(&dw, nw * 4)); CK_(hipMalloc(&ds, COUT * 4)); CK_(hipMalloc(&dt, COUT * 4));
    CK_(hipMalloc(&o1, nout * 4)); CK_(hipMalloc(&o2, nout * 4)); CK_(hipMalloc(&wpb, nw * 6)); CK_(hipMalloc(&wph, nw * 4));
    if (MODE == 2) { CK_(hipMalloc(&st1, (size_t)gr.x * gr.y * B * COUT * 8)); CK_(hipMalloc(&st2, (size_t)gd.x * gd.y * B * COUT * 8)); }
    CK_(hipMemcpy(dx, hx.data(), nx * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));
    CK_(hipMemcpy(ds, hs.data(), COUT * 4, hipMemcpyHostToDevice)); CK_(hipMemcpy(dt, ht.data(), COUT * 4, hipMemcpyHostToDevice));
    hipStream_t st; CK_(hipStreamCreate(&st));
    const dim3 pg((CIN * 9 * COUT + 255) / 256);
    if (DGRAD) {
        hipLaunchKernelGGL(prep_conv_wT_bf16x3_kernel, pg, dim3(256), 0, st, (const float*)dw, wpb, COUT, CIN);
        hipLaunchKernelGGL(prep_conv_wT_f16x3_kernel, pg, dim3(256), 0, st, (const float*)dw, wph, COUT, CIN, (unsigned int*)nullptr);
    } else {
        hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, pg, dim3(256), 0, st, (const float*)dw, wpb, CIN, COUT);
        hipLaunchKernelGGL(prep_conv_w_f16x3_kernel, pg, dim3(256), 0, st, (const float*)dw, wph, CIN, COUT, (unsigned int*)nullptr);
    }
    CK_(hipMemsetAsync(o1, 0, nout * 4, st)); CK_(hipMemsetAsync(o2, 0, nout * 4, st));
    constexpr size_t lds = conv_d16_lds_bytes(PR, PC);
    auto d16 = [&](auto kn, const float* in) {
        constexpr int KN = decltype(kn)::value;
        static bool attr = false;
        if (!attr && lds > 65536) {
            CK_(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_f16x3_direct_kernel<CIN, COUT, PR, PC, MODE, NT, MINB, KN, WR, AH2, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr = true;
        }
        hipLaunchKernelGGL((conv3x3_f16x3_direct_kernel<CIN, COUT, PR, PC, MODE, NT, MINB, KN, WR, AH2, NW>), gd, dim3(64 * NW), lds, st, in, (const unsigned short*)wph,
                           (const float*)ds, (const float*)dt, o2, H, W, Hp, Wp, st2);
    };
    using std::integral_constant;
    hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, RPR, RPC, MODE, 0, 2, 1, 0>), gr, dim3(256), conv_ns_lds_bytes(RPR, RPC), st, (const float*)dx, (const unsigned short*)wpb,
                       (const float*)ds, (const float*)dt, o1, H, W, Hp, Wp, st1);
    d16(integral_constant<int, 0>{}, dx);
    CK_(hipStreamSynchronize(st));
    CK_(hipGetLastError());
    std::vector<float> h1(nout), h2(nout);
    CK_(hipMemcpy(h1.data(), o1, nout * 4, hipMemcpyDeviceToHost)); CK_(hipMemcpy(h2.data(), o2, nout * 4, hipMemcpyDeviceToHost));
    double d = 0, mx = 0; size_t bad = 0;
    for (size_t i = 0; i < nout; ++i) { const double e = fabs((double)h1[i] - h2[i]); d = fmax(d, e); mx = fmax(mx, fabs(h1[i])); bad += e > 1e-4; }
    printf("%s: B=%d %dx%d %d->%d mode %d, tile %dx%d, NT %d, %d waves, weight ring %d, hi sets %d, LDS %zu\n  max |direct bf16x6 - direct f16x3| = %.3e (max |out| %.3f), %zu elements off by > 1e-4\n", name, B, H, W, CIN, COUT,
           MODE, 8 * PR, 4 * PC, NT, NW, WR, AH2 ? 2 : 1, lds, d, mx, bad);
    if (MODE == 2) {
        const size_t n1 = (size_t)gr.x * gr.y * B, n2 = (size_t)gd.x * gd.y * B;
        std::vector<float2> s1(n1 * COUT), s2(n2 * COUT);
        CK_(hipMemcpy(s1.data(), st1, s1.size() * 8, hipMemcpyDeviceToHost)); CK_(hipMemcpy(s2.data(), st2, s2.size() * 8, hipMemcpyDeviceToHost));
        double worst = 0;
        for (int c = 0; c < COUT; ++c) {
            double a = 0, aq = 0, b2 = 0, bq = 0;
            for (size_t k = 0; k < n1; ++k) { a += s1[k * COUT + c].x; aq += s1[k * COUT + c].y; }
            for (size_t k = 0; k < n2; ++k) { b2 += s2[k * COUT + c].x; bq += s2[k * COUT + c].y; }
            worst = fmax(worst, fmax(fabs(a - b2) / fmax(1.0, fabs(a)), fabs(aq - bq) / fmax(1.0, fabs(aq))));
        }
        printf("  channel statistics: worst relative difference of (sum, sum of squares) = %.3e\n", worst);
    }
    if (B >= 64) {
        float* dxr[4];
        for (int k = 0; k < 4; ++k) { CK_(hipMalloc(&dxr[k], nx * 4)); CK_(hipMemcpyAsync(dxr[k], dx, nx * 4, hipMemcpyDeviceToDevice, st)); }
        int rot = 0;
        const double gf = 2.0 * B * H * W * (double)COUT * CIN * 9 * 1e-9;
        const float t = time_us(st, reps, [&] { d16(integral_constant<int, 0>{}, dxr[rot++ & 3]); });
        printf("  rotating inputs: %.1f us (%.1f TF algorithmic); knock-outs: weights once %.1f, tile staged once %.1f, no MFMA %.1f, no stores %.1f, no MFMA + no stores %.1f us\n", t, gf * 1e3 / t,
               time_us(st, reps, [&] { d16(integral_constant<int, 1>{}, dxr[rot++ & 3]); }), time_us(st, reps, [&] { d16(integral_constant<int, 2>{}, dxr[rot++ & 3]); }),
               time_us(st, reps, [&] { d16(integral_constant<int, 4>{}, dxr[rot++ & 3]); }), time_us(st, reps, [&] { d16(integral_constant<int, 8>{}, dxr[rot++ & 3]); }),
               time_us(st, reps, [&] { d16(integral_constant<int, 12>{}, dxr[rot++ & 3]); }));
        for (int k = 0; k < 4; ++k) (void)hipFree(dxr[k]);
    }
    (void)hipFree(dx); (void)hipFree(dw); (void)hipFree(ds); (void)hipFree(dt); (void)hipFree(o1); (void)hipFree(o2); (void)hipFree(wpb); (void)hipFree(wph);
    if (st1) (void)hipFree(st1); if (st2) (void)hipFree(st2);
    fflush(stdout);
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "direct16") {
        const bool small = argc > 2 && std::string(argv[2]) == "small";
        if (!small) {
            run_direct16<64, 128, 2, 2, 1, false, 2, 2, 2, 2>("conv3 GRU layout", 256, 16, 50);
            run_direct16<64, 128, 2, 2, 1, false, 2, 2, 2, 2, 2, false, 2>("conv3 GRU layout", 256, 16, 50);
            run_direct16<64, 128, 2, 2, 1, false, 2, 2, 2, 2, 3, false, 2>("conv3 GRU layout", 256, 16, 50);
            run_direct16<64, 128, 2, 4, 1, false, 2, 2, 2, 2, 2, false, 4>("conv3 GRU layout", 256, 16, 50);
            run_direct16<64, 128, 2, 2, 2, false, 2, 2, 2, 2, 2, false, 2>("conv3 raw", 256, 16, 50);
            run_direct16<32, 64, 4, 2, 0, false, 2, 2, 4, 2, 2, false, 2>("conv2 pooled", 256, 32, 100);
            run_direct16<32, 64, 4, 2, 2, false, 2, 2, 4, 2, 2, false, 2>("conv2 raw", 256, 32, 100);
            run_direct16<128, 64, 2, 4, 2, true, 2, 2, 2, 4, 2, false, 2>("conv3 data gradient", 256, 16, 50);
            run_direct16<64, 32, 4, 2, 2, true, 1, 2, 4, 2, 2, false, 2>("conv2 data gradient", 256, 32, 100);
        }
        run_direct16<64, 128, 2, 2, 1, false, 2, 2, 2, 2, 2, false, 2>("conv3 GRU layout, ragged", 3, 16, 23);
        run_direct16<64, 128, 2, 2, 2, false, 2, 2, 2, 2, 2, false, 2>("conv3 raw, ragged", 1, 16, 15);
        run_direct16<32, 64, 4, 2, 0, false, 2, 2, 4, 2, 2, false, 2>("conv2 pooled, ragged", 3, 32, 47);
        run_direct16<128, 64, 2, 4, 2, true, 2, 2, 2, 4, 2, false, 2>("conv3 data gradient, ragged", 5, 16, 23);
        run_direct16<64, 32, 4, 2, 2, true, 1, 2, 4, 2, 2, false, 2>("conv2 data gradient, ragged", 3, 32, 47);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "wino2") {
        const bool small = argc > 2 && std::string(argv[2]) == "small";
        if (!small) {
            run_wino2<32, 64, 4, 2, 0, false, 3>("conv2 pooled", 256, 32, 100);
            run_wino2<32, 64, 4, 2, 2, false, 3>("conv2 raw + stats", 256, 32, 100);
            run_wino2<64, 128, 2, 2, 1, false, 2>("conv3 GRU layout + planes", 256, 16, 50);
            run_wino2<64, 128, 2, 2, 2, false, 2>("conv3 raw + stats", 256, 16, 50);
            run_wino2<128, 64, 2, 4, 3, true, 2>("conv3 data gradient", 256, 16, 50);
            run_wino2<64, 32, 4, 2, 3, true, 4>("conv2 data gradient", 256, 32, 100);
        }
        run_wino2<32, 64, 4, 2, 0, false, 3>("conv2 pooled, ragged", 3, 32, 47);
        run_wino2<32, 64, 4, 2, 2, false, 3>("conv2 raw, ragged", 5, 32, 47);
        run_wino2<64, 128, 2, 2, 1, false, 2>("conv3 GRU layout, ragged", 3, 16, 23);
        run_wino2<64, 128, 2, 2, 2, false, 2>("conv3 raw, ragged", 1, 16, 15);
        run_wino2<128, 64, 2, 4, 3, true, 2>("conv3 data gradient, ragged", 5, 16, 23);
        run_wino2<64, 32, 4, 2, 3, true, 4>("conv2 data gradient, ragged", 3, 32, 47);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "loop") { load_loop(argc > 2 ? atof(argv[2]) : 3.0); return 0; }
    if (argc > 1 && std::string(argv[1]) == "wino") { run_wino(256, 32, 100); run_wino(3, 32, 47); return 0; }
    run<64, 128, 2, 4, 1>("conv3", 256, 16, 50);
    run<64, 128, 2, 2, 1>("conv3, 16x8-pixel tile (4 patches per wave)", 256, 16, 50);
    run<32, 64, 4, 2, 0>("conv2", 256, 32, 100);
    run<32, 64, 2, 5, 0>("conv2, 16x20-pixel tile (5 patches per wave, 10 tiles per utterance)", 256, 32, 100);
    run<128, 64, 2, 4, 2>("conv3 data gradient", 256, 16, 50);
    run<64, 32, 4, 2, 2>("conv2 data gradient", 256, 32, 100);
    return 0;
}
