// Training step of CNNAudioGRU on MI355X, forward: batch-statistics BatchNorm (or the frozen running ones), saved activations for
// the backward (sir_model_train_fwd), and the workspace queries.  With sir_ce_loss, sir_model_train_bwd and sir_adam_step
// (train_loss_optim.hip, model_train_bwd.hip) it replaces the body of train_epoch (scripts/train.py:90-107: forward, criterion,
// loss.backward(), optimizer.step()).
#include "f16x3_kernels.h"
#include "train_fwd_kernels.h"
#include "conv_fwd.h"

size_t sir_train_workspace_bytes_impl(int batch, int t_frames) {
    TDims d;
    if (!make_tdims(batch, t_frames, &d)) return 0;
    size_t off[TB_COUNT];
    return tws_layout(d, off);
}

extern "C" int sir_model_train_workspace_offsets(const sir_handle* h, int batch, int t_frames, size_t* offsets, int n) {
    (void)h;
    TDims d;
    if (!make_tdims(batch, t_frames, &d) || !offsets) {
        sir_set_error("sir_model_train_workspace_offsets: bad shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", batch, t_frames);
        return SIR_EINVAL;
    }
    size_t off[TB_COUNT];
    tws_layout(d, off);
    for (int i = 0; i < n && i < TB_COUNT; ++i) offsets[i] = off[i];
    return TB_COUNT;
}

extern "C" int sir_model_train_fwd(sir_handle* h, const sir_model_weights* w, float* const bn_running_mean[3],
                                   float* const bn_running_var[3], const float* feats, int batch, int t_frames,
                                   float bn_momentum, float dropout_p, uint64_t dropout_seed, float* logits, void* workspace, size_t workspace_bytes, void* stream_) {
    return sir_model_train_fwd_cfg(h, w, bn_running_mean, bn_running_var, feats, batch, t_frames, bn_momentum, dropout_p, dropout_seed,
                                   nullptr, logits, workspace, workspace_bytes, stream_);
}

// frames == NULL: the padded step.  Else the ragged one (sir_model_train_fwd_ragged; every BatchNorm frozen -- the caller has checked):
// clip b alone at its own width frames[b].  conv1 takes its right edge there (the ragged inference kernel); each block's BN + ReLU +
// pool kernel writes zeros behind the clip's new width, so conv2 / conv3 and the layer-0 projection run unchanged, at full width, on
// maps whose columns behind a clip are the zeros its own padding would be; the recurrences hold h for t >= S_b and store no row
// there (the rows are zeroed: ragged_zero_tail_kernel says who reads them); the attention softmax runs over t < S_b.
static int train_fwd_impl(const char* who, sir_handle* h, const sir_model_weights* w, float* const bn_running_mean[3],
                          float* const bn_running_var[3], const float* feats, const int32_t* frames, int batch, int t_frames,
                          float bn_momentum, float dropout_p, uint64_t dropout_seed, const sir_train_config* cfg,
                          float* logits, void* workspace, size_t workspace_bytes, void* stream_) {
    const bool ragged = frames != nullptr;
    TDims d;
    size_t off[TB_COUNT];
    int rc = check_common(who, h, w, batch, t_frames, workspace, workspace_bytes, &d, off);
    if (rc != SIR_OK) return rc;
    if (!feats || !logits || !bn_running_mean || !bn_running_var) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    for (int i = 0; ragged && i < 3; ++i)
        if (!bn_running_mean[i] || !bn_running_var[i]) { sir_set_error("%s: NULL running statistics", who); return SIR_EINVAL; }
    if (dropout_p < 0.0f || dropout_p >= 1.0f) { sir_set_error("%s: dropout_p=%f", who, dropout_p); return SIR_EINVAL; }
    hipStream_t st = (hipStream_t)stream_;
    TPtrs p = carve(workspace, off);
    const int B = d.B, S = d.S, T = d.T;
    const RagPtrs rg = rag_ptrs(p.rag, B);
    float *scale = p.bn, *shift = p.bn + 224, *smean = p.bn + 448, *sinv = p.bn + 672;

    // conv2 / conv3 forward and both data gradients run on the producer / consumer Winograd kernel (conv_wino2_f16x3_kernel.h);
    // shapes it does not cover keep the first-generation / direct kernels (the plan: model_shape.h).
    const SirConvPlan& cp = d.conv;
    const bool w2 = cp.fwd_wino;
    {   // all weight re-layouts of this step, the backward's included (the weights do not change before it runs)
        SirProfScope prof(h, SIR_K_T_PREP, st);
        PrepJobs pj{};
        int nj = 0, blocks = 0;
        auto add = [&](PrepKind kind, const float* src, void* dst, int a, int b, int nblk) {
            pj.kind[nj] = kind; pj.src[nj] = src; pj.dst[nj] = dst; pj.a[nj] = a; pj.b[nj] = b; pj.block0[nj] = blocks;
            blocks += nblk; ++nj;
        };
        pj.status = h->status;
        // (f16x3 planes for the second-generation Winograd kernel, bf16x3 planes for the first-generation / direct fallbacks)
        add(w2 ? PREP_CONV_W_WINO_F16X3 : PREP_CONV_W_WINO_BF16X3, w->conv_w[1], p.wcb2, 32, 64, prep_blocks(WCB_W2));       // conv2 forward: Winograd frequencies
        add(w2 ? PREP_CONV_W_WINO_F16X3 : PREP_CONV_W_WINO_BF16X3, w->conv_w[2], p.wcb3, 64, 128, prep_blocks(WCB_W3));     // conv3 forward: Winograd frequencies
        if (!w2) add(PREP_CONV_W_BF16X3, w->conv_w[2], p.wcb3d, 64, 128, prep_blocks(WCB_W3_TAPS));
        // conv2 data gradient (64 -> 32): the second-generation Winograd kernel (its transform feeds only 32 outputs -- on bf16x6 that
        // lost to the direct kernel, on f16x3 with half the matrix products it wins: profiles/r04/bench_conv_f16x3.txt), else direct
        if (cp.dgrad2_wino) add(PREP_CONV_WT_WINO_F16X3, w->conv_w[1], p.wcb2t, 32, 64, prep_blocks(WCB_W2));
        else add(PREP_CONV_WT_BF16X3, w->conv_w[1], p.wcb2t, 32, 64, prep_blocks(WCB_W2_TAPS));
        // conv3 data gradient: Winograd frequencies of the flipped taps
        add(cp.dgrad3_wino ? PREP_CONV_WT_WINO_F16X3 : PREP_CONV_WT_WINO_BF16X3, w->conv_w[2], p.wcb3t, 64, 128, prep_blocks(WCB_W3));
        for (int dir = 0; dir < 2; ++dir) {
            add(PREP_SPLIT2H, w->gru_w_ih[dir], p.wsl0 + dir * WS_DIR0, 1024, 768, WS_DIR0_BLOCKS);
            add(PREP_SPLIT2H, w->gru_w_ih[2 + dir], p.wsl1 + dir * WS_DIR1, 512, 768, WS_DIR1_BLOCKS);
        }
        for (int i = 0; i < 4; ++i) {                        // W_hh (layer i / 2, direction i % 2) as the recurrences' resident fragments
            add(PREP_WHH_QUAD, w->gru_w_hh[i], (char*)p.wht + (size_t)i * GRU_FRAG_BYTES, 0, 0, GQ_FRAG_THREADS / 256);
            add(PREP_WHH_BWD_QUAD, w->gru_w_hh[i], (char*)p.wr4 + (size_t)i * GRU_FRAG_BYTES, 0, 0, BQ_FRAG_THREADS / 256);
        }
        pj.block0[nj] = blocks;
        pj.njobs = nj;
        static_assert(PREP_MAX_JOBS >= 18, "job table");
        hipLaunchKernelGGL(train_prep_kernel, dim3(blocks), dim3(256), 0, st, pj);
    }
    SIR_KCHECK();

    // conv1 block: statistics pass (recompute), finalize, then the fused conv+BN+ReLU+pool pass
    {   SirProfScope prof(h, SIR_K_T_CONV1, st);
        // conv1's BatchNorm statistics come from 54 moments of the INPUT (z_c = sum_t w_c[t] x_t: sums and sums of squares
        // of z are bilinear in the taps), so conv1 itself runs once, fused with BN + ReLU + pool
        if (cfg->bn_frozen[0]) {                      // frozen statistics: no moments (the frozen conv1 backward needs none either)
            hipLaunchKernelGGL(bn_fold_running_kernel, dim3(1), dim3(64), 0, st, w->bn_w[0], w->bn_b[0], (const float*)bn_running_mean[0],
                               (const float*)bn_running_var[0], 32, scale, shift, smean, sinv, w->conv_w[0], 288, h->status);
        } else {
            const int tiles = d.c1gx * d.c1gy;
            int per_img = (2048 + B - 1) / B;             // workgroups per image: >= 2048 in all when the batch allows it
            per_img = per_img < 1 ? 1 : (per_img > tiles ? tiles : per_img);
            hipLaunchKernelGGL(conv1_moments_kernel, dim3(per_img, B), dim3(256), 0, st, feats, (float*)p.stats, 64, T, d.c1gx, d.c1gy);
            hipLaunchKernelGGL(conv1_moments_reduce_kernel, dim3(C1_NMOM), dim3(256), 0, st, (const float*)p.stats, per_img * B, p.c1m);
            hipLaunchKernelGGL(conv1_bn_from_moments_kernel, dim3(1), dim3(64), 0, st, (const double*)p.c1m, w->conv_w[0],
                               (double)B * 64 * T, w->bn_w[0], w->bn_b[0], bn_running_mean[0], bn_running_var[0], bn_momentum, scale, shift, smean, sinv, h->status);
        }
        if (ragged) {
            hipLaunchKernelGGL(ragged_widths_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const int*)frames, B, T, p.rag, h->status);
            hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_ragged_kernel, conv1_grid(B, d.wp1), dim3(256), 0, st,
                               feats, w->conv_w[0], scale, shift, p.a1, 64, T, 32, d.wp1, rg.w1, rg.fw);
            hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(32, B), dim3(256), 0, st, p.a1, rg.w1, 32, d.wp1, 32, 1);
        } else
            hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_kernel, conv1_grid(B, d.wp1), dim3(256), 0, st,
                               feats, w->conv_w[0], scale, shift, p.a1, 64, T, 32, d.wp1, (const float*)nullptr, B, (const int*)nullptr);
    }
    // conv2 block: raw conv + partial statistics on MFMA, finalize, BN+ReLU+pool
    {
        {   SirProfScope prof(h, SIR_K_T_CONV2, st);
            SIR_TRY((conv_fwd<32, 64, 2>(h, st, w2, cp.geo2, B, p.a1, p.wcb2, nullptr, nullptr, nullptr, p.z2, p.stats)));
        }
        SirProfScope prof(h, SIR_K_T_BN2, st);
        if (cfg->bn_frozen[1])                        // (the convolution's partial statistics are simply not read)
            hipLaunchKernelGGL(bn_fold_running_kernel, dim3(1), dim3(64), 0, st, w->bn_w[1], w->bn_b[1], (const float*)bn_running_mean[1],
                               (const float*)bn_running_var[1], 64, scale + 32, shift + 32, smean + 32, sinv + 32, (const float*)nullptr, 0, h->status);
        else
            hipLaunchKernelGGL(bn_finalize_kernel, dim3(64), dim3(256), 0, st, (const float2*)p.stats, w2 ? (int)wino2_stat_blocks(B, 32, d.wp1, h->num_cus) : d.c2wx * B, 64,
                               (double)B * 32 * d.wp1, w->bn_w[1], w->bn_b[1], bn_running_mean[1], bn_running_var[1], bn_momentum,
                               scale + 32, shift + 32, smean + 32, sinv + 32, h->status);
        if (ragged)
            hipLaunchKernelGGL((bn_relu_pool_kernel<false, true>), dim3(grid_for((size_t)B * 16 * d.wp2 * 16)), dim3(256), 0, st, p.z2,
                               scale + 32, shift + 32, p.a2, B, 32, d.wp1, 64, 16, d.wp2, 256.0f, h->status, rg.w2);
        else
            hipLaunchKernelGGL(bn_relu_pool_kernel<false>, dim3(grid_for((size_t)B * 16 * d.wp2 * 16)), dim3(256), 0, st, p.z2,
                               scale + 32, shift + 32, p.a2, B, 32, d.wp1, 64, 16, d.wp2, 256.0f, h->status, (const int*)nullptr);
    }
    {
        {   SirProfScope prof(h, SIR_K_T_CONV3, st);
            SIR_TRY((conv_fwd<64, 128, 2>(h, st, w2, cp.geo3, B, p.a2, p.wcb3, p.wcb3d, nullptr, nullptr, p.z3, p.stats)));
        }
        SirProfScope prof(h, SIR_K_T_BN3, st);
        if (cfg->bn_frozen[2])
            hipLaunchKernelGGL(bn_fold_running_kernel, dim3(1), dim3(128), 0, st, w->bn_w[2], w->bn_b[2], (const float*)bn_running_mean[2],
                               (const float*)bn_running_var[2], 128, scale + 96, shift + 96, smean + 96, sinv + 96, (const float*)nullptr, 0, h->status);
        else
            hipLaunchKernelGGL(bn_finalize_kernel, dim3(128), dim3(256), 0, st, (const float2*)p.stats, w2 ? (int)wino2_stat_blocks(B, 16, d.wp2, h->num_cus) : d.c3fx * B, 128,
                               (double)B * 16 * d.wp2, w->bn_w[2], w->bn_b[2], bn_running_mean[2], bn_running_var[2], bn_momentum,
                               scale + 96, shift + 96, smean + 96, sinv + 96, h->status);
        if (ragged)
            hipLaunchKernelGGL((bn_relu_pool_kernel<true, true>), dim3(grid_for((size_t)B * 8 * d.wp3 * 32)), dim3(256), 0, st, p.z3,
                               scale + 96, shift + 96, p.x0, B, 16, d.wp2, 128, 8, d.wp3, 512.0f, h->status, rg.sb);
        else
            hipLaunchKernelGGL(bn_relu_pool_kernel<true>, dim3(grid_for((size_t)B * 8 * d.wp3 * 32)), dim3(256), 0, st, p.z3,
                               scale + 96, shift + 96, p.x0, B, 16, d.wp2, 128, 8, d.wp3, 512.0f, h->status, (const int*)nullptr);
    }
    SIR_KCHECK();

    const int M = B * S;
    {   SirProfScope prof(h, SIR_K_T_GEMM_IH0, st);
        hipLaunchKernelGGL(split2h_kernel, dim3(2048), dim3(256), 0, st, (const float*)p.x0, 1024, p.xs, (size_t)M, 1024);
        SIR_TRY(launch_gemm_nt_f16x3(h, st, (const unsigned short*)p.xs, (const unsigned short*)p.wsl0,
                                     (const unsigned short*)(p.wsl0 + WS_DIR0), w->gru_b_ih[0], w->gru_b_ih[1], p.gi, 1536, M, 768, 1024));
    }
    {   SirProfScope prof(h, SIR_K_T_GRU0, st);
        if (ragged) hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(S, B), dim3(256), 0, st, p.y0, rg.sb, S, 512, 1, 0);
        SIR_TRY(sir_launch_gru_quad(h, st, true, p.gi, w->gru_w_hh[0], w->gru_w_hh[1], w->gru_b_hh[0], w->gru_b_hh[1], p.y0, B, S, p.g0, nullptr,
                                    (const char*)p.wht, (const char*)p.wht + GRU_FRAG_BYTES, ragged ? rg.sb : nullptr, ragged));
    }
    const float* y0in = p.y0;
    {   SirProfScope prof(h, SIR_K_T_GEMM_IH1, st);
        if (dropout_p > 0.0f) {                                   // dropout + the f16x2 planes of its output in one pass
            hipLaunchKernelGGL(dropout_split2h_kernel, dim3(2048), dim3(256), 0, st, (const float*)p.y0, p.y0d, p.xs, (size_t)M * 512,
                               dropout_p, (unsigned long long)dropout_seed);
            y0in = p.y0d;
        } else {
            hipLaunchKernelGGL(split2h_kernel, dim3(2048), dim3(256), 0, st, y0in, 512, p.xs, (size_t)M, 512);
        }
        SIR_TRY(launch_gemm_nt_f16x3(h, st, (const unsigned short*)p.xs, (const unsigned short*)p.wsl1,
                                     (const unsigned short*)(p.wsl1 + WS_DIR1), w->gru_b_ih[2], w->gru_b_ih[3], p.gi, 1536, M, 768, 512));
    }
    {   SirProfScope prof(h, SIR_K_T_GRU1, st);
        if (ragged) hipLaunchKernelGGL(ragged_zero_tail_kernel, dim3(S, B), dim3(256), 0, st, p.y1, rg.sb, S, 512, 1, 0);
        SIR_TRY(sir_launch_gru_quad(h, st, true, p.gi, w->gru_w_hh[2], w->gru_w_hh[3], w->gru_b_hh[2], w->gru_b_hh[3], p.y1, B, S, p.g1, nullptr,
                                    (const char*)p.wht + 2 * GRU_FRAG_BYTES, (const char*)p.wht + 3 * GRU_FRAG_BYTES, ragged ? rg.sb : nullptr, ragged));
    }
    SirProfScope prof_head(h, SIR_K_T_HEAD, st);
    if (ragged) {                                            // (ctx is saved for the backward; a clip of width 0: NaN logits)
        hipLaunchKernelGGL(attention_pool_ragged_kernel, dim3(B), dim3(256), 0, st, p.y1, w->attn_w, w->attn_b, p.ctx, S, w->fc_w,
                           w->fc_b, w->num_classes, logits, (long long*)nullptr, rg.sb, (const int*)nullptr);
        SIR_KCHECK();
        return SIR_OK;
    }
    // live bn1 statistics: the sum of the squared features (a moment of conv1_moments_kernel) is finite only if every feature is; if
    // it is not, every row's logits are NaN -- batch statistics carry one bad feature into all of them (ReLU / max-pool drop NaNs)
    hipLaunchKernelGGL(attention_pool_kernel, dim3(B), dim3(256), 0, st, p.y1, w->attn_w, w->attn_b, p.ctx, S, w->fc_w,
                       w->fc_b, w->num_classes, logits, (long long*)nullptr, (const int*)nullptr,
                       cfg->bn_frozen[0] ? (const double*)nullptr : (const double*)p.c1m + c1_r_index(4, 4));
    SIR_KCHECK();
    return SIR_OK;
}

extern "C" int sir_model_train_fwd_cfg(sir_handle* h, const sir_model_weights* w, float* const bn_running_mean[3],
                                       float* const bn_running_var[3], const float* feats, int batch, int t_frames,
                                       float bn_momentum, float dropout_p, uint64_t dropout_seed, const sir_train_config* cfg,
                                       float* logits, void* workspace, size_t workspace_bytes, void* stream_) {
    return train_fwd_impl("sir_model_train_fwd", h, w, bn_running_mean, bn_running_var, feats, nullptr, batch, t_frames, bn_momentum, dropout_p,
                          dropout_seed, cfg ? cfg : &kTrainAllLive, logits, workspace, workspace_bytes, stream_);
}

extern "C" int sir_model_train_fwd_ragged(sir_handle* h, const sir_model_weights* w, const float* const bn_running_mean[3],
                                          const float* const bn_running_var[3], const float* feats, const int32_t* frames, int batch,
                                          int t_frames, float dropout_p, uint64_t dropout_seed, const sir_train_config* cfg,
                                          float* logits, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int rc = check_ragged_frozen("sir_model_train_fwd_ragged", cfg, "result")) return rc;
    if (!frames) { sir_set_error("sir_model_train_fwd_ragged: NULL frames"); return SIR_EINVAL; }
    // (frozen blocks read the running statistics and never write them: bn_fold_running_kernel)
    return train_fwd_impl("sir_model_train_fwd_ragged", h, w, (float* const*)bn_running_mean, (float* const*)bn_running_var, feats, frames,
                          batch, t_frames, 0.0f, dropout_p, dropout_seed, cfg, logits, workspace, workspace_bytes, stream_);
}
