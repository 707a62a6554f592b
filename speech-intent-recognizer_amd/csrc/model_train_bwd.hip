// Training step of CNNAudioGRU on MI355X, backward (sir_model_train_bwd and its split / fine-tuning / input-gradient forms): what is wanted
// (BwdPlan), then head -> GRU layer 1 -> GRU layer 0 -> conv3 -> conv2 -> conv1, one function per stage.
#define SIR_NO_STANDALONE_KERNELS       // (the backward launches none of them: model_kernels.h)
#include "train_bwd_kernels.h"
#include "conv_wino2_f16x3_kernel.h"
#include "wgrad_bf16x6_kernel.h"
#include "gemm_tn2_f16x3_kernel.h"
#include "wgrad_wino_f16x3_kernel.h"

namespace {

// Weight gradient of a conv stage (CIN -> COUT forward channels, H x W map) into dw, on stream st: the Winograd kernel
// (16 products per tile and channel pair instead of 36, wgrad_wino_f16x3_kernel.h) + strip sum + G^T . G, or the nine-tap fallback,
// one slab per image, + its two-pass reduce
template <int CIN, int COUT>
int conv_wgrad(sir_handle* h, hipStream_t st, bool wino, int B, int H, int W, const float* dz, const float* a, float* slab, float* dw, const float* bsc) {
    if (wino) {
        using Cfg = WgwCfg<CIN, COUT>;
        const int strips = wgrad_wino_strips(B, H, W, Cfg::TPS, Cfg::groups, h->num_cus);
        SIR_TRY(sir_lds_opt_in(h, (const void*)conv_wgrad_wino_f16x3_kernel<CIN, COUT>, (int)Cfg::lds_bytes));
        hipLaunchKernelGGL((conv_wgrad_wino_f16x3_kernel<CIN, COUT>), dim3(Cfg::groups * strips), dim3(WGW_THREADS), Cfg::lds_bytes, st, dz, a, slab, B, H, W);
        float* part = slab + (size_t)strips * 16 * COUT * CIN;
        hipLaunchKernelGGL(wgrad_wino_sum_kernel, dim3((16 * COUT * CIN / 4 + 255) / 256), dim3(256), 0, st, (const float*)slab, strips, 16 * COUT * CIN / 4, part);
        hipLaunchKernelGGL(wgrad_wino_finish_kernel, dim3((COUT * CIN + 255) / 256), dim3(256), 0, st, (const float*)part, CIN, COUT, dw, bsc);
        return SIR_OK;
    }
    const size_t ldsx = wgrad_x6_lds_bytes(CIN, COUT, W);
    // (sir_model_train_bwd_x refuses such a shape before its first launch)
    if (!wgrad_x6_fits(CIN, COUT, W)) { sir_set_error("sir_model_train_bwd: t_frames too large for the weight-gradient tile"); return SIR_EUNSUPPORTED; }
    SIR_TRY(sir_lds_opt_in(h, (const void*)conv_wgrad_bf16x6_kernel<CIN, COUT>, 160 * 1024));
    // one workgroup and one slab per image (H rows; its four k-split waves add up in LDS)
    hipLaunchKernelGGL((conv_wgrad_bf16x6_kernel<CIN, COUT>), dim3(B), dim3(512), ldsx, st, dz, a, slab, H, W, H);
    float* part = slab + (size_t)B * 9 * COUT * CIN;
    hipLaunchKernelGGL(wgrad_reduce_partial_kernel, dim3((9 * COUT * CIN / 4 + 255) / 256, WGR_PARTS), dim3(256), 0, st, (const float*)slab, B, 9 * COUT * CIN / 4, part);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((9 * COUT * CIN + 255) / 256), dim3(256), 0, st, (const float*)part, WGR_PARTS, CIN, COUT, dw, bsc);
    return SIR_OK;
}

// Data gradient of a conv stage = a CIN -> COUT convolution (forward COUT -> CIN) with the flipped / transposed taps, raw output: the
// Winograd kernel on the weights PREP_CONV_WT_WINO_F16X3 built, or the stage's fallback on the form train_prep_kernel built for it
// (conv3: first-generation Winograd, blocks of 8 x 4 tiles for the 16-row map; conv2: direct)
template <int CIN, int COUT>
int conv_dgrad(sir_handle* h, hipStream_t st, bool wino, const Wino2Geo& geo, const float* dz, const unsigned short* wt, float* da) {
    static_assert((CIN == 128 && COUT == 64) || (CIN == 64 && COUT == 32), "conv3 or conv2");
    const int H = geo.H, W = geo.W, B = geo.B;
    if (wino) {
        SIR_TRY(sir_lds_opt_in(h, (const void*)conv3x3_wino2_f16x3_kernel<CIN, COUT, 3, 0, 3>, W2_LDS_BYTES));
        SIR_HIP_TRY((launch_conv_wino2<CIN, COUT, 3>(st, geo, dz, wt, (const float*)nullptr, (const float*)nullptr, da, (float2*)nullptr, h->zero_page, h->num_cus)));
    } else if constexpr (CIN == 128) {
        hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<128, 64, 2, 3, 1, 0, 4>), dim3(((W + 1) / 2 + 3) / 4, 1, B), dim3(256), WINO_LDS_BYTES, st,
                           dz, wt, (const float*)nullptr, (const float*)nullptr, da, H, W, H / 2, W / 2, (float2*)nullptr);
    } else {
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<64, 32, 4, 2, 2, 0, 4>), dim3((W + 7) / 8, 1, B), dim3(256), conv_ns_lds_bytes(4, 2), st,
                           dz, wt, (const float*)nullptr, (const float*)nullptr, da, H, W, H / 2, W / 2, (float2*)nullptr);
    }
    return SIR_OK;
}

// What is wanted (a NULL gradient pointer = frozen parameter) and how far down the chain has to run.  A launch that writes wanted
// and unwanted gradients gets NULL for the unwanted ones: the kernels test the pointer at the store.
struct BwdPlan {
    bool fc, attn;                  // head: fc weight or bias / attention weight or bias
    bool gru_w[2], gru_b[2];        // per GRU layer: any weight matrix / any bias
    bool gb[3], blk[3];             // per conv block: gamma or beta / those or the conv weight
    bool cnn;                       // anything in the CNN, the gradient of the input features (sir_model_train_bwd_x) included
    bool head, bptt[2];             // stages that run: the head, the BPTT of layer 0 / 1 (something trainable in it or below it)
    bool dz3, da2, dz2, da1;        // gradients of the CNN chain that somebody reads
};

// dx: d(loss)/d(features) is wanted -- the data chain then runs to the bottom whatever `g` holds
BwdPlan bwd_plan(const sir_model_grads& g, bool dx) {
    BwdPlan w;
    w.fc = g.fc_w || g.fc_b;
    w.attn = g.attn_w || g.attn_b;
    for (int l = 0; l < 2; ++l) {
        w.gru_w[l] = g.gru_w_ih[2 * l] || g.gru_w_ih[2 * l + 1] || g.gru_w_hh[2 * l] || g.gru_w_hh[2 * l + 1];
        w.gru_b[l] = g.gru_b_ih[2 * l] || g.gru_b_ih[2 * l + 1] || g.gru_b_hh[2 * l] || g.gru_b_hh[2 * l + 1];
    }
    for (int i = 0; i < 3; ++i) { w.gb[i] = g.bn_w[i] || g.bn_b[i]; w.blk[i] = g.conv_w[i] || w.gb[i]; }
    w.cnn = w.blk[0] || w.blk[1] || w.blk[2] || dx;
    w.bptt[0] = w.gru_w[0] || w.gru_b[0] || w.cnn;
    w.bptt[1] = w.gru_w[1] || w.gru_b[1] || w.gru_w[0] || w.gru_b[0] || w.cnn;
    w.head = w.fc || w.attn || w.bptt[1];
    w.dz3 = g.conv_w[2] || w.blk[1] || w.blk[0] || dx;
    w.da2 = w.blk[1] || w.blk[0] || dx;
    w.dz2 = g.conv_w[1] || w.blk[0] || dx;
    w.da1 = w.blk[0] || dx;
    return w;
}

// One backward call: arguments, workspace, plan, and the two streams.
// Two-stream form (A/B in profiles/r04/ab_bwd_streams.txt): the launches that nothing downstream waits for -- the GRU weight
// gradients of both layers and the two convolution weight gradients, with their slab reduces -- go to `side`, a stream owned by the
// handle.  Each GRU weight-gradient GEMM forks right behind ITS layer's BPTT: layer 1's then runs beside layer 0's BPTT, which keeps
// one workgroup on half of the CUs (gru_bwd_quad_kernel.h) and leaves the rest idle.  Each convolution weight gradient forks behind
// the BatchNorm backward that produces its dz.  One join before the call returns.  The chain dX -> BN3 -> dgrad3 -> BN2 -> dgrad2 ->
// conv1 stays on the caller's stream.  In the split form (SIR_BWD_HEAD_GRU / SIR_BWD_CNN, data parallel) the first half joins before
// it returns -- its gradients are reduced next.  While every kernel is being timed (sir_profile_enable mode 1) the backward stays on
// one stream -- per-kernel times of overlapped launches would say nothing about the kernels -- and side == st.
struct Bwd {
    sir_handle* h;
    hipStream_t st, side;           // the caller's stream; the stream of the weight gradients
    bool two;                       // side is a stream of its own
    const sir_model_weights* w; const sir_model_grads* g; const sir_train_config* cfg;
    const float* demb;              // d(loss)/d(ctx) [B][512] that enters beside dlogits fc_w (sir_model_train_bwd_emb), or NULL
    const float *feats, *dlogits, *y0in;      // y0in: what GRU layer 1 read (layer 0's output, behind the dropout if there is one)
    float* dfeats;                  // d(loss)/d(feats) [B][64][T], or NULL: not wanted
    float dropout_p; uint64_t dropout_seed;
    TPtrs p; TDims d; BwdPlan want;
    const float* bsc;               // TB_BSC: this call's loss scale and its inverse, written by bwd_scale_kernel (pair 0; pair 1 + b: utterance b's)
    bool row_scaled;                // every utterance on a scale of its own (the data-only backward under frozen statistics)
    float *scale, *shift, *smean, *sinv, *mdy, *mdyx;      // the [224]-channel BatchNorm arrays (bn1 | bn2 | bn3 at 0, 32, 96) in p.bn, p.bnb
    bool forked, side_marked;       // side has work of this call / its last launch is marked by event 3 (sir_handle::bwd_ev)
    bool ragged; RagPtrs rg;        // sir_model_train_bwd_ragged: the clips' own widths (TB_RAG, rewritten from `frames` at the head of the call)

    int fork(int ev) {              // side continues behind what st holds now
        if (!two) return SIR_OK;
        forked = true;
        SIR_HIP_TRY(hipEventRecord(h->bwd_ev[ev], st));
        SIR_HIP_TRY(hipStreamWaitEvent(side, h->bwd_ev[ev], 0));
        return SIR_OK;
    }
    int mark_side() {               // marks what is (so far) the side stream's last launch
        if (!two) return SIR_OK;
        SIR_HIP_TRY(hipEventRecord(h->bwd_ev[3], side));
        side_marked = true;
        return SIR_OK;
    }
    int join() {                    // st waits for the marked launch: every gradient is final on the caller's stream
        if (two && side_marked) SIR_HIP_TRY(hipStreamWaitEvent(st, h->bwd_ev[3], 0));
        return SIR_OK;
    }
};

// ---- head: fc + attention pooling ----------------------------------------------------------------------------------------
int bwd_head(Bwd& c) {
    const int B = c.d.B, S = c.d.S, C = c.w->num_classes;
    float* daw_part = c.p.small;
    float* dab_part = c.p.small + (size_t)B * 512;
    if (c.want.head) {
        SirProfScope prof(c.h, SIR_K_B_HEAD, c.st);
        hipLaunchKernelGGL(bwd_scale_kernel, dim3(c.row_scaled ? (B + 15) / 16 : 1), dim3(1024), 0, c.st, c.dlogits, B, C, sir_bwd_loss_scale_exp(B),
                           c.row_scaled ? 1 : 0, c.p.bsc, c.ragged ? c.rg.sb : (const int*)nullptr, c.demb);
        // (workgroups [B, B + 2 C) are the fc weight / bias gradient: left out when fc is frozen)
        hipLaunchKernelGGL(head_bwd_kernel, dim3(B + (c.want.fc ? 2 * C : 0)), dim3(256), 0, c.st, c.dlogits, c.w->fc_w, (const float*)c.p.y1, c.w->attn_w,
                           c.w->attn_b, (const float*)c.p.ctx, c.p.dy1, daw_part, dab_part, c.g->fc_w, c.g->fc_b, B, S, C, c.bsc, c.row_scaled ? 1 : 0,
                           c.ragged ? c.rg.sb : (const int*)nullptr, c.demb);
        if (c.want.attn)
            hipLaunchKernelGGL(head_colsum_kernel, dim3(9), dim3(256), 0, c.st, (const float*)daw_part, (const float*)dab_part, B, c.g->attn_w, c.g->attn_b);
    }
    SIR_KCHECK();
    return SIR_OK;
}

// all four weight-gradient GEMMs of a GRU layer (2 directions x {W_ih, W_hh}) in one launch + the slab reduce
int bwd_gru_dw(Bwd& c, int layer, hipStream_t s_) {
    const TPtrs& p = c.p;
    const int M = c.d.B * c.d.S;
    const float* dgi_l = layer ? p.dgi1 : p.dgi;
    const float* dgh_l = layer ? p.dgh1 : p.dgh;
    const float* yout = layer ? p.y1 : p.y0;
    const float* xin = layer ? c.y0in : p.x0;
    const int in_sz = layer ? 512 : 1024;
    SirProfScope prof(c.h, layer ? SIR_K_B_DW1 : SIR_K_B_DW0, s_);
    TnJobs jb{};
    float* outs[4];
    size_t sizes[4];
    jb.njobs = 4;
    jb.zeros = c.h->zero_page;
    int tiles = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const int gi_idx = 2 * layer + dir;
        const int ja = 2 * dir, jh = 2 * dir + 1;
        jb.A[ja] = dgi_l + dir * 768; jb.lda[ja] = 1536; jb.B[ja] = xin; jb.ldb[ja] = in_sz; jb.N[ja] = in_sz; jb.shift[ja] = 0;
        outs[ja] = c.g->gru_w_ih[gi_idx];
        jb.A[jh] = dgh_l + dir * 768; jb.lda[jh] = 1536; jb.B[jh] = yout + dir * 256; jb.ldb[jh] = 512; jb.N[jh] = 256;
        jb.shift[jh] = dir ? 1 : -1;
        outs[jh] = c.g->gru_w_hh[gi_idx];
    }
    for (int j = 0; j < 4; ++j) {
        jb.tile0[j] = tiles;
        tiles += (768 / TN2_BM) * ((jb.N[j] + TN_BN - 1) / TN_BN);
        sizes[j] = (size_t)768 * jb.N[j];
    }
    jb.tile0[4] = tiles;
    int tiles_chk, kchunk, nsplit;
    size_t need;
    tn_dw_plan(M, in_sz, &tiles_chk, &kchunk, &nsplit, &need);
    size_t pos = 0;
    for (int j = 0; j < 4; ++j) {
        jb.slab[j] = (c.two ? p.slab2 : p.slab) + pos;
        jb.slab_stride[j] = sizes[j];
        pos += sizes[j] * nsplit;
    }
    // (f16x3: the gate gradients carry the loss scale)
    SIR_TRY(sir_lds_opt_in(c.h, (const void*)gemm_tn2_f16x3_kernel<true>, (int)tn2_lds_bytes(true)));
    hipLaunchKernelGGL(gemm_tn2_f16x3_kernel<true>, dim3(tiles, nsplit), dim3(TN2_THREADS), tn2_lds_bytes(true), s_, jb, 768, M, kchunk, c.d.S);
    SlabJobs sj{};
    for (int j = 0; j < 4; ++j) { sj.src[j] = jb.slab[j]; sj.out[j] = outs[j]; sj.n[j] = outs[j] ? sizes[j] : 0; }     // (n = 0: a frozen matrix is not reduced)
    hipLaunchKernelGGL(slab_reduce_jobs_kernel, dim3(grid_for(sizes[0]), 4), dim3(256), 0, s_, sj, nsplit, c.bsc);
    return SIR_OK;
}

// gradient wrt the input of a GRU layer: dgi [M][1536] x [W_ih; W_ih_reverse] [1536][in]
int bwd_gru_dx(Bwd& c, int layer) {
    const TPtrs& p = c.p;
    const int M = c.d.B * c.d.S, in_sz = layer ? 512 : 1024;
    const bool drop = layer == 1 && c.dropout_p > 0.0f;
    SirProfScope prof(c.h, layer ? SIR_K_B_DX1 : SIR_K_B_DX0, c.st);
    float* dxin = layer ? p.dy0 : p.dx0;
    TnJobs jn{};
    jn.njobs = 1;
    jn.zeros = c.h->zero_page;
    if (drop) { jn.drop_p = c.dropout_p; jn.drop_seed = c.dropout_seed; }   // dy0 = mask * d(y0d)
    jn.A[0] = layer ? p.dgi1 : p.dgi; jn.lda[0] = 1536;
    jn.B[0] = c.w->gru_w_ih[2 * layer]; jn.B2[0] = c.w->gru_w_ih[2 * layer + 1]; jn.brows[0] = 768; jn.ldb[0] = in_sz;
    jn.N[0] = in_sz; jn.shift[0] = 0;
    jn.slab[0] = dxin; jn.slab_stride[0] = 0;
    jn.tile0[0] = 0;
    const int ntn = (in_sz + TN_BN - 1) / TN_BN;
    int ntiles = ((M + TN_BM - 1) / TN_BM) * ntn;
    if (dx_splitk(M, in_sz)) {
        jn.drop_p = 0.0f;                                // (the dropout mask is applied by the add)
        jn.slab[0] = p.slab; jn.slab_stride[0] = (size_t)M * in_sz;
        jn.tile0[1] = ntiles;
        SIR_TRY(sir_lds_opt_in(c.h, (const void*)gemm_tn2_f16x3_kernel<false>, (int)tn2_lds_bytes(false)));
        hipLaunchKernelGGL(gemm_tn2_f16x3_kernel<false>, dim3(ntiles, 2), dim3(TN2_THREADS), tn2_lds_bytes(false), c.st, jn, M, 1536, 768, 1);
        hipLaunchKernelGGL(dx_halves_add_kernel, dim3(grid_for((size_t)M * in_sz / 4)), dim3(256), 0, c.st, (const float*)p.slab, (size_t)M * in_sz / 4,
                           dxin, drop ? c.dropout_p : 0.0f, (unsigned long long)c.dropout_seed);
    } else if (ntiles < 160) {                           // too few 128-row tiles to fill the CUs: 64-row tiles
        ntiles = ((M + 63) / 64) * ntn;
        jn.tile0[1] = ntiles;
        SIR_TRY(sir_lds_opt_in(c.h, (const void*)gemm_tn2_f16x3_kernel<false, 0, 64>, (int)tn2_lds_bytes(false, 64)));
        hipLaunchKernelGGL((gemm_tn2_f16x3_kernel<false, 0, 64>), dim3(ntiles, 1), dim3(TN2_THREADS), tn2_lds_bytes(false, 64), c.st, jn, M, 1536, 1536, 1);
    } else {
        jn.tile0[1] = ntiles;
        SIR_TRY(sir_lds_opt_in(c.h, (const void*)gemm_tn2_f16x3_kernel<false>, (int)tn2_lds_bytes(false)));
        hipLaunchKernelGGL(gemm_tn2_f16x3_kernel<false>, dim3(ntiles, 1), dim3(TN2_THREADS), tn2_lds_bytes(false), c.st, jn, M, 1536, 1536, 1);
    }
    return SIR_OK;
}

// ---- one GRU layer: BPTT, bias gradients, weight gradients (side stream), input gradient -------------------------------------
int bwd_gru_layer(Bwd& c, int layer) {
    const TPtrs& p = c.p;
    const BwdPlan& want = c.want;
    const int B = c.d.B, S = c.d.S, M = B * S;
    float* bsum_i = p.slab;                              // [B][1536] x2, consumed before the slabs are used
    float* bsum_h = p.slab + (size_t)B * 1536;
    {   SirProfScope prof(c.h, layer ? SIR_K_B_GRU1 : SIR_K_B_GRU0, c.st);
        SIR_TRY(sir_launch_gru_bwd_quad(c.h, c.st, layer ? p.dy1 : p.dy0, layer ? p.g1 : p.g0, layer ? p.y1 : p.y0, c.w->gru_w_hh[2 * layer],
                                        c.w->gru_w_hh[2 * layer + 1], layer ? p.dgi1 : p.dgi, layer ? p.dgh1 : p.dgh, bsum_i, bsum_h, B, S,
                                        (const char*)p.wr4 + (size_t)(2 * layer) * GRU_FRAG_BYTES, (const char*)p.wr4 + (size_t)(2 * layer + 1) * GRU_FRAG_BYTES,
                                        c.ragged ? c.rg.sb : (const int*)nullptr));
        // bias gradients first: bsum_* alias the slab area used below
        if (want.gru_b[layer])
            hipLaunchKernelGGL(gru_bias_colsum_kernel, dim3(24, 2), dim3(256), 0, c.st, (const float*)bsum_i, (const float*)bsum_h, B,
                               c.g->gru_b_ih[2 * layer], c.g->gru_b_ih[2 * layer + 1], c.g->gru_b_hh[2 * layer], c.g->gru_b_hh[2 * layer + 1], c.bsc);
    }
    // Layer 0's saved gates and outputs (65 MB) were written early in the forward and have left the 256 MB last-level cache by now;
    // layer 1's are still there, and layer 0's BPTT -- a latency chain whose polls share the L2 channels with its input misses --
    // pays 16-26 us for the difference (profiles/r04/ab_bptt.txt).  A read-and-drop pass on the side stream, beside layer 1's dX on
    // the caller's, brings them back: step -28 .. -40 us.  The same for the raw conv outputs ahead of the BatchNorm backward was
    // measured and LOSES (those kernels are bandwidth-bound: the reads are only moved earlier).
    const bool touch = c.two && layer == 1 && want.bptt[0];     // (the prefetch belongs to layer 0's BPTT, not to layer 1's weight gradient)
    if (want.gru_w[layer] || touch) {                    // (layer 0's GEMM queues behind layer 1's on the side stream: they share the slabs)
        SIR_TRY(c.fork(4 + layer));
        if (touch)
            hipLaunchKernelGGL(cache_touch_kernel, dim3(256), dim3(256), 0, c.side, (const float4*)p.g0, (size_t)M * 2048 / 4, (const float4*)p.y0,
                               (size_t)M * 512 / 4, p.small);
        if (want.gru_w[layer]) SIR_TRY(bwd_gru_dw(c, layer, c.side));
    }
    if (!(layer ? want.bptt[0] : want.cnn)) return SIR_OK;     // nobody reads this layer's input gradient
    SIR_TRY(bwd_gru_dx(c, layer));
    SIR_KCHECK();
    return SIR_OK;
}

// ---- conv3 / conv2 block: BatchNorm + ReLU + pool backward -> dz, weight gradient (side stream), data gradient ------------------
struct ConvBlock {
    int i, ch;                      // index of the block's conv / BatchNorm parameters (1 = conv2, 2 = conv3); its first BatchNorm channel
    int H, W, Wp;                   // rows and columns of the conv output z, columns of the pooled map
    const float *z, *da, *a_in;     // raw conv output; gradient of the pooled output; the conv's input
    float *dz, *da_in;              // gradient of z; gradient of the conv's input
    const unsigned short* wt;       // data-gradient form of the weights
    const Wino2Geo* geo;
    bool wgrad_wino, dgrad_wino, need_dz, need_da_in;
    int nblk, ev;                   // workgroups (= partial sums) of the reduce launch; fork event of the weight gradient
    bool last_on_side;              // no weight gradient follows this block's on the side stream
    int prof_bn, prof_wgrad, prof_dgrad;
    const int* wlim;                // ragged step: columns of the pooled map that belong to each clip (`da` counts as zero behind them), else NULL
};

// CIN -> COUT: the forward's channels.  GRU_IN: `da` is in the GRU layout (conv3).  reduce(): launches the block's partial sums of
// dy and dy * xhat from the POOLED activations and their gradient -- dy = da wherever a > 0 and xhat at the routed maximum is
// (a - beta) / gamma -- instead of the four times larger raw conv output.
template <int CIN, int COUT, bool GRU_IN, class Reduce>
int bwd_conv_block(Bwd& c, const ConvBlock& k, Reduce reduce) {
    const int B = c.d.B, Hp = k.H / 2;
    const bool frozen = c.cfg->bn_frozen[k.i] != 0, gb = c.want.gb[k.i];
    float *scale = c.scale + k.ch, *shift = c.shift + k.ch;
    const int dz_grid = grid_for((size_t)B * Hp * ((k.W + 1) / 2) * (COUT / 4));
    // frozen statistics: the pooled sums feed only dgamma / dbeta (same kernel: xhat = (a - beta) / gamma holds for the running
    // statistics too, and the small-gamma path reads the folded arrays), and dz waits for no reduce at all
    if (!frozen || gb || k.need_dz) {
        SirProfScope prof(c.h, k.prof_bn, c.st);
        if (!frozen || gb) reduce();
        if (frozen) {
            if (gb)
                hipLaunchKernelGGL(bn_bwd_finalize_frozen_kernel, dim3(COUT), dim3(256), 0, c.st, (const float2*)c.p.stats, k.nblk, COUT, c.g->bn_w[k.i],
                                   c.g->bn_b[k.i], c.bsc);
            if (k.need_dz && k.wlim)
                hipLaunchKernelGGL((bn_bwd_dz_kernel<GRU_IN, true, true>), dim3(dz_grid), dim3(256), 0, c.st, k.z, k.da, scale, shift, (const float*)nullptr,
                                   (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, k.dz, B, k.H, k.W, COUT, Hp, k.Wp, k.wlim);
            else if (k.need_dz)
                hipLaunchKernelGGL((bn_bwd_dz_kernel<GRU_IN, true>), dim3(dz_grid), dim3(256), 0, c.st, k.z, k.da, scale, shift, (const float*)nullptr,
                                   (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, k.dz, B, k.H, k.W, COUT, Hp, k.Wp, (const int*)nullptr);
        } else {
            hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(COUT), dim3(256), 0, c.st, (const float2*)c.p.stats, k.nblk, COUT, (double)B * k.H * k.W,
                               c.g->bn_w[k.i], c.g->bn_b[k.i], c.mdy + k.ch, c.mdyx + k.ch, c.bsc);
            if (k.need_dz)
                hipLaunchKernelGGL(bn_bwd_dz_kernel<GRU_IN>, dim3(dz_grid), dim3(256), 0, c.st, k.z, k.da, scale, shift, c.smean + k.ch, c.sinv + k.ch,
                                   c.mdy + k.ch, c.mdyx + k.ch, k.dz, B, k.H, k.W, COUT, Hp, k.Wp, (const int*)nullptr);
        }
    }
    if (c.g->conv_w[k.i]) {
        SIR_TRY(c.fork(k.ev));
        {   SirProfScope prof(c.h, k.prof_wgrad, c.side);
            SIR_TRY((conv_wgrad<CIN, COUT>(c.h, c.side, k.wgrad_wino, B, k.H, k.W, k.dz, k.a_in, c.p.slab, c.g->conv_w[k.i], c.bsc)));
        }
        if (k.last_on_side) SIR_TRY(c.mark_side());
    }
    if (k.need_da_in) {
        // data gradient = a COUT -> CIN convolution with the flipped / transposed taps, raw output (train_prep_kernel of the forward built k.wt)
        SirProfScope prof(c.h, k.prof_dgrad, c.st);
        SIR_TRY((conv_dgrad<COUT, CIN>(c.h, c.st, k.dgrad_wino, *k.geo, k.dz, k.wt, k.da_in)));      // (dz carries the loss scale: inside fp16's range)
    }
    SIR_KCHECK();
    return SIR_OK;
}

int bwd_conv3(Bwd& c) {
    const TPtrs& p = c.p;
    const TDims& d = c.d;
    const int rows = d.B * d.wp3, rpb = 16;
    ConvBlock k{2, 96, 16, d.wp2, d.wp3, p.z3, p.dx0, p.a2, p.dz3, p.da2, p.wcb3t, &d.conv.geo3, d.conv.wgrad3_wino, d.conv.dgrad3_wino,
                c.want.dz3, c.want.da2, (rows + rpb - 1) / rpb, 1, !c.g->conv_w[1], SIR_K_B_BN3, SIR_K_B_WGRAD3, SIR_K_B_DGRAD3,
                c.ragged ? c.rg.sb : (const int*)nullptr};     // (dx0 is zero behind S_b already: the projection's rows do not spill)
    return bwd_conv_block<64, 128, true>(c, k, [&] {
        hipLaunchKernelGGL(bn_bwd_reduce_pooled_gru_kernel, dim3(k.nblk), dim3(256), 0, c.st, (const float*)p.x0, (const float*)p.dx0,
                           (const float*)p.z3, c.w->bn_w[2], c.w->bn_b[2], c.scale + 96, c.shift + 96, c.smean + 96, c.sinv + 96, p.stats, rows, 16, d.wp2, d.wp3, rpb);
    });
}

int bwd_conv2(Bwd& c) {
    const TPtrs& p = c.p;
    const TDims& d = c.d;
    const int ppb = 64;
    const size_t npix = (size_t)d.B * 16 * d.wp2;
    ConvBlock k{1, 32, 32, d.wp1, d.wp2, p.z2, p.da2, p.a1, p.dz2, p.da1, p.wcb2t, &d.conv.geo2, d.conv.wgrad2_wino, d.conv.dgrad2_wino,
                c.want.dz2, c.want.da1, (int)((npix + ppb - 1) / ppb), 2, true, SIR_K_B_BN2, SIR_K_B_WGRAD2, SIR_K_B_DGRAD2,
                c.ragged ? c.rg.w2 : (const int*)nullptr};
    return bwd_conv_block<32, 64, false>(c, k, [&] {
        hipLaunchKernelGGL(bn_bwd_reduce_pooled_kernel, dim3(k.nblk), dim3(256), 0, c.st, (const float*)p.a2, (const float*)p.da2,
                           (const float*)p.z2, c.w->bn_w[1], c.w->bn_b[1], c.scale + 32, c.shift + 32, c.smean + 32, c.sinv + 32, p.stats, d.B, 32,
                           d.wp1, 64, 16, d.wp2, ppb, k.wlim);
    });
}

// ---- conv1 block: ONE recompute pass: (sum dy, sum dy*xhat, sum dy*x_tap) per channel; the mean terms of dz = s (dy - m1 - xhat m2)
// and with them the rest of dW1 are closed forms in the input moments of the forward (conv1_bwd_finalize_kernel, in double) ------
// With dfeats (sir_model_train_bwd_x) the block's data gradient follows: conv1_bwd_data_kernel, the last link of the chain.
int bwd_conv1(Bwd& c) {
    const TPtrs& p = c.p;
    const TDims& d = c.d;
    const sir_model_grads* g = c.g;
    const int B = d.B, T = d.T;
    const bool frozen = c.cfg->bn_frozen[0] != 0;
    // the reduce pass feeds the three parameter gradients and, with live statistics, the two means of the data gradient's dz
    if (c.want.blk[0] || (c.dfeats && !frozen)) {
        float* c1part = p.small + (size_t)B * 512 + B + 64;
        SirProfScope prof(c.h, SIR_K_B_CONV1, c.st);
        const dim3 g1(d.c1gx, d.c1gy, B);
        const int nblk = d.c1gx * d.c1gy * B;
        if (c.ragged)
            hipLaunchKernelGGL((conv1_bwd_kernel<2, true>), g1, dim3(256), 0, c.st, c.feats, c.w->conv_w[0], (const float*)p.da1, c.scale, c.shift,
                               c.smean, c.sinv, (const float*)nullptr, (const float*)nullptr, c1part, 64, T, 32, d.wp1, c.rg.w1, c.rg.fw);
        else
            hipLaunchKernelGGL(conv1_bwd_kernel<2>, g1, dim3(256), 0, c.st, c.feats, c.w->conv_w[0], (const float*)p.da1, c.scale, c.shift,
                               c.smean, c.sinv, (const float*)nullptr, (const float*)nullptr, c1part, 64, T, 32, d.wp1, (const int*)nullptr, (const int*)nullptr);
        float* c1tmp = (float*)p.stats;           // [128][352] partial column sums, then [352] totals behind them
        float* c1tot = c1tmp + 128 * 352;
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((352 + 63) / 64, 128), dim3(256), 0, c.st, (const float*)c1part, nblk, 352, 352, c1tmp);
        hipLaunchKernelGGL(colsum_kernel, dim3((352 + 63) / 64), dim3(256), 0, c.st, (const float*)c1tmp, 128, 352, 352, c1tot);
        if (frozen)                                          // frozen statistics: plain sums, no input moments
            hipLaunchKernelGGL(conv1_bwd_finalize_frozen_kernel, dim3(1), dim3(320), 0, c.st, (const float*)c1tot, (const float*)c.scale, g->bn_w[0], g->bn_b[0],
                               g->conv_w[0], c.bsc);
        else                                                 // (the means go to bn1's channels of TB_BNB, which nothing else uses)
            hipLaunchKernelGGL(conv1_bwd_finalize_kernel, dim3(1), dim3(320), 0, c.st, (const float*)c1tot, (const double*)p.c1m,
                               c.w->conv_w[0], c.scale, c.smean, c.sinv, (double)B * 64 * T, g->bn_w[0], g->bn_b[0], g->conv_w[0], c.bsc,
                               c.dfeats ? c.mdy : (float*)nullptr, c.dfeats ? c.mdyx : (float*)nullptr);
    }
    if (c.dfeats) {
        // data gradient: dz1 recomputed per tile, transposed 3x3 convolution onto the features (conv1_bwd_data_kernel)
        SirProfScope prof(c.h, SIR_K_B_CONV1_DGRAD, c.st);
        const dim3 gd((T + C1D_TW - 1) / C1D_TW, (64 + C1D_TH - 1) / C1D_TH, B);
        if (c.ragged)                                        // (frozen: the entry point insists)
            hipLaunchKernelGGL((conv1_bwd_data_kernel<true, true>), gd, dim3(256), 0, c.st, c.feats, c.w->conv_w[0], (const float*)p.da1, c.scale, c.shift,
                               (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, c.dfeats, 64, T, 32, d.wp1, c.bsc,
                               c.row_scaled ? 1 : 0, c.rg.w1, c.rg.fw);
        else if (frozen)
            hipLaunchKernelGGL(conv1_bwd_data_kernel<true>, gd, dim3(256), 0, c.st, c.feats, c.w->conv_w[0], (const float*)p.da1, c.scale, c.shift,
                               (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, c.dfeats, 64, T, 32, d.wp1, c.bsc, c.row_scaled ? 1 : 0,
                               (const int*)nullptr, (const int*)nullptr);
        else
            hipLaunchKernelGGL(conv1_bwd_data_kernel<false>, gd, dim3(256), 0, c.st, c.feats, c.w->conv_w[0], (const float*)p.da1, c.scale, c.shift,
                               c.smean, c.sinv, (const float*)c.mdy, (const float*)c.mdyx, c.dfeats, 64, T, 32, d.wp1, c.bsc, c.row_scaled ? 1 : 0,
                               (const int*)nullptr, (const int*)nullptr);
    }
    SIR_KCHECK();
    return SIR_OK;
}

}  // namespace

extern "C" int sir_model_train_bwd(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                                   int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                                   const sir_model_grads* g, void* workspace, size_t workspace_bytes, void* stream_) {
    return sir_model_train_bwd_part(h, w, feats, dlogits, batch, t_frames, dropout_p, dropout_seed, g, workspace, workspace_bytes, SIR_BWD_ALL, stream_);
}

extern "C" int sir_model_train_bwd_part(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                                        int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                                        const sir_model_grads* g, void* workspace, size_t workspace_bytes, int part, void* stream_) {
    return sir_model_train_bwd_cfg(h, w, feats, dlogits, batch, t_frames, dropout_p, dropout_seed, nullptr, g, workspace, workspace_bytes, part, stream_);
}

extern "C" int sir_model_train_bwd_cfg(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                                       int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                                       const sir_train_config* cfg, const sir_model_grads* g, void* workspace,
                                       size_t workspace_bytes, int part, void* stream_) {
    return sir_model_train_bwd_x(h, w, feats, dlogits, batch, t_frames, dropout_p, dropout_seed, cfg, g, nullptr, workspace, workspace_bytes, part, stream_);
}

// frames == NULL: the padded step; else the ragged one (sir_model_train_bwd_ragged: every BatchNorm frozen, the caller has checked)
// demb == NULL: no gradient enters at the embedding (the four entry points of before)
static int train_bwd_impl(const char* who, sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, const float* dlogits,
                          const float* demb, int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                          const sir_train_config* cfg, const sir_model_grads* g, float* dfeats, void* workspace,
                          size_t workspace_bytes, int part, void* stream_) {
    if (part != SIR_BWD_ALL && part != SIR_BWD_HEAD_GRU && part != SIR_BWD_CNN) {
        sir_set_error("sir_model_train_bwd_part: unknown part %d", part);
        return SIR_EINVAL;
    }
    Bwd c{};
    size_t off[TB_COUNT];
    int rc = check_common(who, h, w, batch, t_frames, workspace, workspace_bytes, &c.d, off);
    if (rc != SIR_OK) return rc;
    if (!feats || !dlogits || !g) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    if ((uintptr_t)demb & 15u) { sir_set_error("%s: demb must be 16-byte aligned", who); return SIR_EINVAL; }
    if (dfeats && (((uintptr_t)dfeats & 3) != 0 || dfeats == feats)) {
        sir_set_error("sir_model_train_bwd_x: dfeats must be a float buffer of its own");
        return SIR_EINVAL;
    }
    c.want = bwd_plan(*g, dfeats != nullptr);
    // A wanted conv2 / conv3 weight gradient whose Winograd gate is closed runs on the nine-tap kernel, which holds one whole map row:
    // refused here, for either half of a split call, before anything is launched or written (a frozen conv weight launches neither)
    if ((g->conv_w[1] && !c.d.conv.wgrad2_wino && !wgrad_x6_fits(32, 64, c.d.wp1)) ||
        (g->conv_w[2] && !c.d.conv.wgrad3_wino && !wgrad_x6_fits(64, 128, c.d.wp2))) {
        sir_set_error("sir_model_train_bwd: batch=%d t_frames=%d: the conv2 / conv3 weight gradient of a stage beyond 32-bit offsets takes map rows "
                      "of at most %d / %d columns (t_frames <= 257 / 259)", batch, t_frames, wgrad_x6_max_w(64), wgrad_x6_max_w(128));
        return SIR_EUNSUPPORTED;
    }
    if (!h->bwd_side) {                                      // (first use: the only allocating step, as for the exchange buffers)
        SIR_HIP_TRY(hipStreamCreateWithFlags(&h->bwd_side, hipStreamNonBlocking));
        for (auto& e : h->bwd_ev) SIR_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    c.h = h; c.w = w; c.g = g; c.cfg = cfg; c.feats = feats; c.dlogits = dlogits; c.demb = demb; c.dfeats = dfeats;
    c.dropout_p = dropout_p; c.dropout_seed = dropout_seed;
    c.st = (hipStream_t)stream_;
    c.two = h->bwd_side != nullptr && h->prof_mode != 1;
    c.side = c.two ? h->bwd_side : c.st;
    c.p = carve(workspace, off);
    c.bsc = c.p.bsc;
    // rows on scales of their own: only where no gradient sums over the batch -- every BatchNorm on its running statistics and no
    // parameter gradient wanted (sir_amd.explain, a crafting pass of an adversary under frozen statistics)
    c.row_scaled = dfeats && cfg->bn_frozen[0] && cfg->bn_frozen[1] && cfg->bn_frozen[2] && !c.want.fc && !c.want.attn && !c.want.gru_w[0] &&
                   !c.want.gru_w[1] && !c.want.gru_b[0] && !c.want.gru_b[1] && !c.want.blk[0] && !c.want.blk[1] && !c.want.blk[2];
    c.scale = c.p.bn; c.shift = c.p.bn + 224; c.smean = c.p.bn + 448; c.sinv = c.p.bn + 672;
    c.mdy = c.p.bnb; c.mdyx = c.p.bnb + 224;
    c.y0in = dropout_p > 0.0f ? c.p.y0d : c.p.y0;
    c.ragged = frames != nullptr;
    c.rg = rag_ptrs(c.p.rag, c.d.B);
    if (c.ragged)                                            // (either half of a split call; no status: the forward has reported a bad length)
        hipLaunchKernelGGL(ragged_widths_kernel, dim3((c.d.B + 255) / 256), dim3(256), 0, c.st, (const int*)frames, c.d.B, c.d.T, c.p.rag,
                           (unsigned int*)nullptr);

    if (part != SIR_BWD_CNN) {
        SIR_TRY(bwd_head(c));
        if (c.want.bptt[1]) SIR_TRY(bwd_gru_layer(c, 1));
        if (c.want.bptt[0]) SIR_TRY(bwd_gru_layer(c, 0));
        // the GRU gradients are final on the caller's stream once it has waited for this mark (the conv chain below does not depend
        // on them, but the data-parallel caller of the split form reduces them next)
        if (c.forked) SIR_TRY(c.mark_side());
        if (part == SIR_BWD_HEAD_GRU) return c.join();
    }
    if (!c.want.cnn) {                                       // whole CNN frozen, no input gradient: the chain ended at layer 0's BPTT
        SIR_KCHECK();
        return c.join();
    }
    // (SIR_BWD_CNN of the split form: the side stream starts behind the first half)
    if (g->conv_w[1] || g->conv_w[2]) SIR_TRY(c.fork(0));
    SIR_TRY(bwd_conv3(c));
    if (c.want.da2) SIR_TRY(bwd_conv2(c));
    if (c.want.da1) SIR_TRY(bwd_conv1(c));
    return c.join();
}

extern "C" int sir_model_train_bwd_x(sir_handle* h, const sir_model_weights* w, const float* feats, const float* dlogits,
                                     int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                                     const sir_train_config* cfg, const sir_model_grads* g, float* dfeats, void* workspace,
                                     size_t workspace_bytes, int part, void* stream_) {
    return train_bwd_impl("sir_model_train_bwd", h, w, feats, nullptr, dlogits, nullptr, batch, t_frames, dropout_p, dropout_seed, cfg ? cfg : &kTrainAllLive, g,
                          dfeats, workspace, workspace_bytes, part, stream_);
}

extern "C" int sir_model_train_bwd_ragged(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames,
                                          const float* dlogits, int batch, int t_frames, float dropout_p, uint64_t dropout_seed,
                                          const sir_train_config* cfg, const sir_model_grads* g, float* dfeats, void* workspace,
                                          size_t workspace_bytes, int part, void* stream_) {
    if (int rc = check_ragged_frozen("sir_model_train_bwd_ragged", cfg, "gradient")) return rc;
    if (!frames) { sir_set_error("sir_model_train_bwd_ragged: NULL frames"); return SIR_EINVAL; }
    return train_bwd_impl("sir_model_train_bwd_ragged", h, w, feats, frames, dlogits, nullptr, batch, t_frames, dropout_p, dropout_seed, cfg, g, dfeats,
                          workspace, workspace_bytes, part, stream_);
}

// The superset of the forms above: frames == NULL is sir_model_train_bwd_x (cfg == NULL: every BatchNorm live), else
// sir_model_train_bwd_ragged; demb == NULL is exactly that call.
extern "C" int sir_model_train_bwd_emb(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames,
                                       const float* dlogits, const float* demb, int batch, int t_frames, float dropout_p,
                                       uint64_t dropout_seed, const sir_train_config* cfg, const sir_model_grads* g, float* dfeats,
                                       void* workspace, size_t workspace_bytes, int part, void* stream_) {
    if (frames) {
        if (int rc = check_ragged_frozen("sir_model_train_bwd_emb", cfg, "gradient")) return rc;
    }
    return train_bwd_impl("sir_model_train_bwd_emb", h, w, feats, frames, dlogits, demb, batch, t_frames, dropout_p, dropout_seed,
                          cfg ? cfg : &kTrainAllLive, g, dfeats, workspace, workspace_bytes, part, stream_);
}
