// sir_model_infer: eval-mode CNNAudioGRU.forward + argmax (models/models.py:41-68, scripts/evaluate.py:82-83)
// as a fixed sequence of hand-written kernels on one stream.  See model_kernels.h for the kernels, infer_workspace.h for the
// workspace they run in and infer_tables.h for the tables (E0, d1, d3, task lists, row list) that the first launches build.
//
// Pad skip.  Features are zero-padded to a fixed frame count (bench / pipeline: 200 frames for 94 real ones at 3 s).  A conv
// output whose receptive field sees only trailing all-+0.0 frame columns does not depend on the utterance: it equals what an
// all-zero utterance of the same width produces at that position.  So one extra "template" utterance (index B, fed from an
// all-zero feature row in the workspace) rides along at full width through conv1-3 and the layer-0 input projection, and for
// every real utterance only the columns that some non-template GRU step depends on are computed:
// conv1 stores pooled columns < d1; conv2 / conv3 run over a compacted list of 4-tile-column tasks; the layer-0 input projection
// runs over a row list (steps s < d3 of each utterance + the template's S rows) and the layer-0 recurrence reads the template's gi
// row for steps s >= d3.  Columns past the computed ones are left unwritten in a1 / a2 / x0 / xs / gi.  The conv fallback kernels
// (shapes the Winograd kernel does not cover) keep the full path.
//
// Ragged (sir_model_infer_ragged): the UN-PADDED function -- utterance b is computed as if it were alone in a batch of its own width
// frames[b] (scripts/test_tts_samples.py:83-96 feeds each file at its own length).  Every stage takes its right edge at the
// utterance's own width: conv1 reads frame columns >= frames[b] as zeros, the Winograd kernels source map columns past the width from
// the zero page and store no pooled column past half of it, both input projections run over the row list, the recurrences hold h
// while t >= S_b and the attention softmax runs over t < S_b.  On the conv fallback kernels the maps are masked to zero past the width.
#include "f16x3_kernels.h"
#include "conv_fwd.h"
#include "infer_tables.h"

extern "C" size_t sir_model_workspace_bytes(const sir_handle* h, int batch, int t_frames, int train) {
    (void)h;
    if (train) return sir_train_workspace_bytes_impl(batch, t_frames);
    Dims d;
    if (!make_dims(batch, t_frames, &d)) return 0;
    size_t off[WS_COUNT];
    return iws_layout(d, off);
}

extern "C" int sir_model_workspace_offsets(const sir_handle* h, int batch, int t_frames, int train, size_t* offsets,
                                           int n) {
    (void)h; (void)train;
    Dims d;
    if (!make_dims(batch, t_frames, &d) || !offsets) {
        sir_set_error("sir_model_workspace_offsets: bad shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", batch, t_frames);
        return SIR_EINVAL;
    }
    size_t off[WS_COUNT];
    iws_layout(d, off);
    for (int i = 0; i < n && i < WS_COUNT; ++i) offsets[i] = off[i];
    return WS_COUNT;
}

extern "C" int sir_model_infer_table_offsets(const sir_handle* h, int batch, int t_frames, size_t* offsets, int n) {
    (void)h;
    Dims d;
    if (!make_dims(batch, t_frames, &d) || !offsets) {
        sir_set_error("sir_model_infer_table_offsets: bad shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", batch, t_frames);
        return SIR_EINVAL;
    }
    const ITabs t = itab_layout(d);
    const size_t v[] = {t.e0, t.d1, t.d3, t.rows, t.tab2, t.tab3, t.record, t.nonfinite, t.count, (size_t)WS_PAD};
    const int nv = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < nv; ++i) offsets[i] = v[i];
    return nv;
}

// sir_model_embed's export: emb[b] = ctx[b] (workspace slot 6, untouched), all-NaN for a row whose logits the head kernel makes NaN --
// a non-finite feature in the utterance (nonfinite: pad_extent_kernel) or a rejected ragged length (slen[b] < 1; slen NULL: padded)
static __global__ __launch_bounds__(128) void embed_export_kernel(const float* __restrict__ ctx, const int* __restrict__ nonfinite,
                                                                  const int* __restrict__ slen, float* __restrict__ emb) {
    const int b = blockIdx.x;
    const bool bad = nonfinite[b] != 0 || (slen && slen[b] < 1);
    const float qnan = __builtin_nanf("");
    const float4 v = reinterpret_cast<const float4*>(ctx + (size_t)b * 512)[threadIdx.x];
    reinterpret_cast<float4*>(emb + (size_t)b * 512)[threadIdx.x] = bad ? make_float4(qnan, qnan, qnan, qnan) : v;
}

// frames == nullptr: the padded function with the pad skip (sir_model_infer); else the ragged one (head of this file).
// emb != nullptr (sir_model_embed): the context rows are exported behind the head, and logits may then be NULL (no classifier)
static int model_infer_impl(const char* who, sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, int batch,
                            int t_frames, float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream_,
                            float* emb = nullptr) {
    if (!h || !w || !feats || (!logits && !emb) || !workspace) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    if (emb && (((uintptr_t)emb & 15) != 0)) { sir_set_error("%s: emb must be 16-byte aligned", who); return SIR_EINVAL; }
    Dims d;
    if (!make_dims(batch, t_frames, &d)) {
        sir_set_error("%s: unsupported shape batch=%d t_frames=%d (need " SIR_SHAPE_LIMITS ")", who, batch, t_frames);
        return SIR_EINVAL;
    }
    if (h->cfg.n_mels != 64) { sir_set_error("%s: the model is wired for 64 mels (models.py:23)", who); return SIR_EUNSUPPORTED; }
    if (w->num_classes < 1 || w->num_classes > 64) { sir_set_error("%s: num_classes=%d", who, w->num_classes); return SIR_EINVAL; }
    size_t off[WS_COUNT];
    const size_t need = iws_layout(d, off);
    if (workspace_bytes < need) { sir_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need); return SIR_ENOMEM; }
    if (((uintptr_t)workspace & 255) != 0) { sir_set_error("%s: workspace must be 256-byte aligned", who); return SIR_EINVAL; }
    const bool ragged = frames != nullptr;
    hipStream_t st = (hipStream_t)stream_;
    const IPtrs p = carve(workspace, off, d);
    const ITabPtrs& t = p.t;
    const int B = d.B, S = d.S;
    // tile rule of the row-list projections (f16x3_kernels.h): CU time instead of latency while launches alternate between streams.
    // Read once per call (the recurrence launches below may flip it)
    const bool proj_throughput = h->cluster_multi;

    // conv2 / conv3 as Winograd F(2x2, 3x3) -- the 2x2 output tile is the pooling window -- on the producer / consumer kernel
    // (conv_wino2_f16x3_kernel.h); shapes it does not cover (batch x map beyond 32-bit offsets) keep the bf16x6 fallback kernels.
    // The pad skip (head of this file) runs with the Winograd kernels, over the batch + the template utterance.
    const SirConvPlan cp = sir_conv_plan(&d, true);             // (true: the template utterance)
    const bool w2 = cp.fwd_wino;
    const int BT = w2 ? B + 1 : B;                                // utterances through conv1-3 and the layer-0 projection
    // (ragged: no template utterance is computed, but the plan, the plane stride of xs and the table offsets stay those of the
    // padded call -- and so does the prepared-weight key: a ragged and a padded call may alternate on one workspace)

    // ---- weight preparation -------------------------------------------------------------
    // skipped when the caller vouches (sir_model_set_weights_version) that the weights are the ones prepared
    // into this very workspace by the previous call
    const long long prep_key = ((long long)B << 32) | (unsigned)d.T;
    sir_handle::PrepEntry* pe = nullptr;
    for (auto& e : h->prep)
        if (e.ws == workspace) pe = &e;
    const bool reuse_prep = pe && h->weights_version != 0 && pe->version == h->weights_version && pe->key == prep_key;
    if (!reuse_prep) {
        SirProfScope prof(h, SIR_K_PREP, st);
        const int bn_c[3] = {32, 64, 128}, bn_o[3] = {0, 32, 96};
        for (int i = 0; i < 3; ++i)
            hipLaunchKernelGGL(prep_bn_kernel, dim3(1), dim3(128), 0, st, w->bn_w[i], w->bn_b[i], w->bn_mean[i], w->bn_var[i],
                               p.bns + bn_o[i], p.bnt + bn_o[i], bn_c[i], i == 0 ? w->conv_w[0] : (const float*)nullptr, i == 0 ? 288 : 0, h->status);
        for (int i = 0; i < 4; ++i) sir_prep_whh_quad(h, st, w->gru_w_hh[i], p.whh[i]);
        // (the weight planes are prepared in the arithmetic of the kernel that will read them: f16x3 for the second-generation
        // Winograd kernel's forward stages, bf16x3 for the first-generation / direct fallbacks)
        if (w2) hipLaunchKernelGGL(prep_conv_w_wino_f16x3_kernel, dim3(prep_blocks(WCB_W2)), dim3(256), 0, st, w->conv_w[1], p.wcb2, 32, 64, h->status);
        else hipLaunchKernelGGL(prep_conv_w_wino_bf16x3_kernel, dim3(prep_blocks(WCB_W2)), dim3(256), 0, st, w->conv_w[1], p.wcb2, 32, 64);
        if (w2) hipLaunchKernelGGL(prep_conv_w_wino_f16x3_kernel, dim3(prep_blocks(WCB_W3)), dim3(256), 0, st, w->conv_w[2], p.wcb3, 64, 128, h->status);
        else hipLaunchKernelGGL(prep_conv_w_wino_bf16x3_kernel, dim3(prep_blocks(WCB_W3)), dim3(256), 0, st, w->conv_w[2], p.wcb3, 64, 128);
        hipLaunchKernelGGL(prep_conv_w_bf16x3_kernel, dim3(prep_blocks(WCB_W3_TAPS)), dim3(256), 0, st, w->conv_w[2], p.wcb3d, 64, 128);
        for (int dir = 0; dir < 2; ++dir) {
            hipLaunchKernelGGL(split2h_weights_kernel, dim3(WS_DIR0_BLOCKS), dim3(256), 0, st, w->gru_w_ih[dir], 1024, p.wsl0[dir], (size_t)768, 1024, h->status);
            hipLaunchKernelGGL(split2h_weights_kernel, dim3(WS_DIR1_BLOCKS), dim3(256), 0, st, w->gru_w_ih[2 + dir], 512, p.wsl1[dir], (size_t)768, 512, h->status);
        }
        if (!pe) { pe = &h->prep[h->prep_next]; h->prep_next = (h->prep_next + 1) % 4; }
        pe->ws = workspace; pe->version = h->weights_version; pe->key = prep_key;
    }
    SIR_KCHECK();

    // ---- CNN stack: conv + folded BN + ReLU + 2x2 max-pool per launch ------------------------------
    {
        SirProfScope prof(h, SIR_K_CONV1, st);
        // the scan (ragged: below frames[b] only, and e0 holds the validated frames instead).  It also flags non-finite features for
        // the head kernel: it runs on the fallback path too, where nothing reads e0
        hipLaunchKernelGGL(pad_extent_kernel, dim3(B), dim3(256), 0, st, feats, d.T, ragged ? nullptr : t.e0, (const int*)frames, t.nonfinite);
        if (ragged) {                                             // tables from the given lengths; conv1 at each utterance's own width
            hipLaunchKernelGGL(ragged_tables_kernel, dim3(1), dim3(1024), 0, st, (const int*)frames, d, t.e0, t.d1, t.d3, t.tab2, t.tab3, t.rows, h->status);
            hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_ragged_kernel, conv1_grid(B, d.wp1), dim3(256), 0, st, feats,
                               w->conv_w[0], p.bns, p.bnt, p.a1, 64, d.T, 32, d.wp1, t.d1, t.e0);
            // (fallback path only: the mask of conv1's map is counted with conv1, that of conv2's map with conv2 in sir_profile_*)
            if (!w2) hipLaunchKernelGGL(ragged_mask_kernel, dim3(32, B), dim3(256), 0, st, p.a1, t.e0, 1, 32, d.wp1, 32);
        } else {
            // pad-skip tables (the scan and this: two small launches, counted with conv1)
            if (w2) hipLaunchKernelGGL(pad_tables_kernel, dim3(1), dim3(1024), 0, st, t.e0, d, t.d1, t.d3, t.tab2, t.tab3, t.rows, p.xz);
            hipLaunchKernelGGL(conv1_mfma_bn_relu_pool_kernel, conv1_grid(BT, d.wp1), dim3(256), 0, st, feats,
                               w->conv_w[0], p.bns, p.bnt, p.a1, 64, d.T, 32, d.wp1, p.xz, B, w2 ? t.d1 : nullptr);
        }
    }
    // (the lists' capacity and the grid bound, (B + 1) * kmax tasks: no image lists more than ceil(need / 4) <= kmax tasks, packed or
    // not -- pad_tables_emit)
    {
        SirProfScope prof(h, SIR_K_CONV2, st);
        if (ragged) {
            SIR_TRY((conv_fwd<32, 64, 0, true>(h, st, w2, cp.geo2, B, p.a1, p.wcb2, nullptr, p.bns + 32, p.bnt + 32, p.a2, nullptr, t.tab2, (B + 1) * d.k2max,
                                               t.e0, 1)));
            if (!w2) hipLaunchKernelGGL(ragged_mask_kernel, dim3(16, B), dim3(256), 0, st, p.a2, t.e0, 2, 16, d.wp2, 64);
        } else
            SIR_TRY((conv_fwd<32, 64, 0>(h, st, w2, cp.geo2, BT, p.a1, p.wcb2, nullptr, p.bns + 32, p.bnt + 32, p.a2, nullptr, t.tab2, (B + 1) * d.k2max)));
    }
    {
        // conv3 stores straight into the GRU input layout [B][S][c*8+h] (models.py:55-57) and writes the f16x2 planes of
        // the first input projection's A operand beside it
        SirProfScope prof(h, SIR_K_CONV3, st);
        if (ragged)
            SIR_TRY((conv_fwd<64, 128, 1, true>(h, st, w2, cp.geo3, B, p.a2, p.wcb3, p.wcb3d, p.bns + 96, p.bnt + 96, p.x0, (float2*)p.xs, t.tab3, (B + 1) * d.k3max,
                                                t.e0, 2)));
        else
            SIR_TRY((conv_fwd<64, 128, 1>(h, st, w2, cp.geo3, BT, p.a2, p.wcb3, p.wcb3d, p.bns + 96, p.bnt + 96, p.x0, (float2*)p.xs, t.tab3, (B + 1) * d.k3max)));
    }
    SIR_KCHECK();

    // ---- 2-layer bidirectional GRU ----------------------------------------------------------
    const int M = B * S;
    // steps of its own per utterance: layer 0 reads the template's gi row behind them (pad skip), a ragged call holds h there
    const int* const nlive0 = w2 || ragged ? t.d3 : nullptr;
    const int* const nlive1 = ragged ? t.d3 : nullptr;
    {
        // pad skip: only the rows the recurrence reads (the row list of pad_tables_kernel: steps s < d3 of every utterance and the
        // template's S rows), on a tile the compacted count fills the chip with; the other gi rows are left unwritten
        SirProfScope prof(h, SIR_K_GEMM_IH0, st);
        if (w2 || ragged)                                         // (ragged: the rows s < S_b of every utterance, on either conv path)
            SIR_TRY(launch_gemm_nt_f16x3_gather(h, st, p.xs, p.wsl0[0], p.wsl0[1], w->gru_b_ih[0], w->gru_b_ih[1], p.gi, 1536,
                                                t.rows, BT * S, 768, 1024, proj_throughput, t.record));
        else
            SIR_TRY(launch_gemm_nt_f16x3(h, st, p.xs, p.wsl0[0], p.wsl0[1], w->gru_b_ih[0], w->gru_b_ih[1], p.gi, 1536, M, 768, 1024));
    }
    {
        SirProfScope prof(h, SIR_K_GRU0, st);
        // layer 0 also writes the f16x2 planes of ITS output: the A operand of the layer-1 projection
        SIR_TRY(sir_launch_gru_quad(h, st, false, p.gi, w->gru_w_hh[0], w->gru_w_hh[1], w->gru_b_hh[0], w->gru_b_hh[1], p.y0, B, S, nullptr,
                                    p.xs, p.whh[0], p.whh[1], nlive0, ragged));
    }
    {
        SirProfScope prof(h, SIR_K_GEMM_IH1, st);
        if (ragged)                                               // the same row list: layer 0 wrote y0's planes for exactly these rows
            SIR_TRY(launch_gemm_nt_f16x3_gather(h, st, p.xs, p.wsl1[0], p.wsl1[1], w->gru_b_ih[2], w->gru_b_ih[3], p.gi, 1536,
                                                t.rows, M, 768, 512, proj_throughput, t.record));
        else
            SIR_TRY(launch_gemm_nt_f16x3(h, st, p.xs, p.wsl1[0], p.wsl1[1], w->gru_b_ih[2], w->gru_b_ih[3], p.gi, 1536, M, 768, 512));
    }
    {
        SirProfScope prof(h, SIR_K_GRU1, st);
        SIR_TRY(sir_launch_gru_quad(h, st, false, p.gi, w->gru_w_hh[2], w->gru_w_hh[3], w->gru_b_hh[2], w->gru_b_hh[3], p.y1, B, S, nullptr,
                                    nullptr, p.whh[2], p.whh[3], nlive1, ragged));
    }
    SIR_KCHECK();

    // ---- attention pooling + classifier head ------------------------------------------------
    {
        SirProfScope prof(h, SIR_K_ATTN, st);
        if (ragged)
            hipLaunchKernelGGL(attention_pool_ragged_kernel, dim3(B), dim3(256), 0, st, p.y1, w->attn_w, w->attn_b, p.ctx, S, w->fc_w, w->fc_b,
                               w->num_classes, logits, (long long*)argmax, t.d3, t.nonfinite);
        else
            hipLaunchKernelGGL(attention_pool_kernel, dim3(B), dim3(256), 0, st, p.y1, w->attn_w, w->attn_b, p.ctx, S, w->fc_w, w->fc_b,
                               w->num_classes, logits, (long long*)argmax, t.nonfinite, nullptr);
        if (emb)
            hipLaunchKernelGGL(embed_export_kernel, dim3(B), dim3(128), 0, st, p.ctx, t.nonfinite, ragged ? t.d3 : (const int*)nullptr, emb);
    }
    SIR_KCHECK();
    return SIR_OK;
}

extern "C" int sir_model_infer(sir_handle* h, const sir_model_weights* w, const float* feats, int batch, int t_frames,
                               float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream_) {
    return model_infer_impl("sir_model_infer", h, w, feats, nullptr, batch, t_frames, logits, argmax, workspace, workspace_bytes, stream_);
}

extern "C" int sir_model_infer_ragged(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, int batch,
                                      int t_frames, float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes,
                                      void* stream_) {
    if (!frames) { sir_set_error("sir_model_infer_ragged: NULL frames"); return SIR_EINVAL; }
    return model_infer_impl("sir_model_infer_ragged", h, w, feats, frames, batch, t_frames, logits, argmax, workspace, workspace_bytes, stream_);
}

extern "C" int sir_model_embed(sir_handle* h, const sir_model_weights* w, const float* feats, const int32_t* frames, int batch, int t_frames,
                               float* emb, float* logits, int64_t* argmax, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!emb) { sir_set_error("sir_model_embed: NULL emb"); return SIR_EINVAL; }
    if (argmax && !logits) { sir_set_error("sir_model_embed: argmax needs logits"); return SIR_EINVAL; }
    return model_infer_impl("sir_model_embed", h, w, feats, frames, batch, t_frames, logits, argmax, workspace, workspace_bytes, stream_, emb);
}
