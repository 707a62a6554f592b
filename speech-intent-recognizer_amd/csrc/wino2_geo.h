// Launch geometry of the producer / consumer Winograd kernel (conv_wino2_f16x3_kernel.h) and the shape test that decides
// whether a map runs on it.  Host code only: model_shape.h builds the conv plan from it.
#pragma once
#include <stddef.h>

// Exact unsigned division by a launch-time constant (the round-up method: q = (t + ((n - t) >> 1)) >> sh with t = mulhi(m, n); a shift for
// powers of two).  A hardware-free 32-bit division costs ~25 vector instructions on this ISA; the producers' per-task address set-up held ten
// of them -- ~1000 of the ~8000 cycles of a two-chunk task on the kernel's critical waves (fine-grained stamps in
// profiles/r04/bench_conv_wino2_f16x3.txt).  The device side is w2_div (conv_wino2_f16x3_kernel.h).
struct W2Div { unsigned m; int sh; int pow2; unsigned d; };
static inline W2Div w2_div_make(unsigned d) {
    W2Div r{0u, 0, 0, d};
    if ((d & (d - 1)) == 0) { r.pow2 = 1; while ((1u << r.sh) < d) ++r.sh; return r; }
    int l = 0;
    while ((1ull << l) < d) ++l;                             // ceil(log2 d)
    r.m = (unsigned)((((1ull << l) - d) << 32) / d + 1);
    r.sh = l - 1;
    return r;
}

struct Wino2Geo {
    int H, W;            // input = output map (pixels)
    int TW;              // tile columns per image = ceil(W / 2)
    int NG;              // tile columns of the batch = B * TW
    int RBN;             // 8-row tile blocks per image = (H / 2) / 8
    int NS;              // spatial tasks = RBN * ceil(NG / 4)
    int Hp, Wp;          // pooled map (OUT_MODE 0 / 1)
    int B;
    W2Div dTW, d2TW, dRBN;   // divisions by TW, 2 TW, RBN (all operands are non-negative)
    // nullptr: tile columns are numbered across the whole batch (above).  Otherwise a COMPACTED task list in device memory
    // (inference pad skip, model_infer.hip): ctab[0] = number of task columns n, NS = RBN * n, ctab[1] unused, and two words per task column k < n
    // (ctab is 8-byte aligned: the kernel loads the pair at once):
    //   ctab[2 + 2 k] = gA << 2 | (nA - 1)     segment A: nA = 1..4 tile columns of ONE image from gA = img * TW + tx0 (any tx0), in
    //                                          tile slots 0 .. nA - 1
    //   ctab[3 + 2 k] = -1, or gB << 2 | (sB - 2) << 1 | (nB - 1)
    //                                          guest segment B: nB = 1..2 tile columns of ANOTHER image from gB, in tile slots
    //                                          sB .. sB + nB - 1 (sB = 2 or 3, sB + nB <= 4)
    // Tile slot k reads patch columns 2 k .. 2 k + 3 of the task's 10-column raw patch, so the segments' patch columns must be
    // disjoint: 2 nA + 2 <= 2 sB ([1 | idle | 2], [1 | idle | idle | 1], [2 | idle | 1]).  Every patch column is sourced from the
    // image of its own segment (or the zero page outside that image); slots between the segments and past a segment's count
    // compute garbage that is neither stored nor counted, and a segment never runs past its image's TW.  The RAGGED form reads
    // the first word only (its lists carry no guests).
    const int* ctab;
    // un-padded batch inference (the kernel's RAGGED form; needs ctab): image b is wtab[b] >> wsh pixel columns wide.  nullptr otherwise.
    const int* wtab;
    int wsh;
};
// false: shape outside what the kernel covers (whole 8-tile-row blocks, 32-bit element offsets) -- the caller keeps the
// first-generation / direct kernel for it
static inline bool wino2_geo(int B, int H, int W, int cmax, Wino2Geo* g) {
    g->B = B; g->H = H; g->W = W; g->TW = (W + 1) / 2; g->NG = B * g->TW; g->RBN = H / 16; g->ctab = nullptr; g->wtab = nullptr; g->wsh = 0;
    g->NS = g->RBN * ((g->NG + 3) / 4); g->Hp = H / 2; g->Wp = W / 2;
    g->dTW = w2_div_make((unsigned)g->TW); g->d2TW = w2_div_make(2u * (unsigned)g->TW); g->dRBN = w2_div_make((unsigned)(g->RBN > 0 ? g->RBN : 1));
    return H % 16 == 0 && W >= 1 && B >= 1 && (size_t)B * H * W * cmax < ((size_t)1 << 31) && (size_t)g->NG * 2 < ((size_t)1 << 30);
}
// statistics blocks of OUT_MODE 2: one per (workgroup, transform-row wave); `max_wg` as passed to launch_conv_wino2
static inline size_t wino2_stat_blocks(int B, int H, int W, int max_wg) {
    const size_t ns = (size_t)(H / 16) * (((size_t)B * ((W + 1) / 2) + 3) / 4);
    return (ns < (size_t)max_wg ? ns : (size_t)max_wg) * 4;
}
