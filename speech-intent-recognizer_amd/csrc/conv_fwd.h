// Host launcher of one forward conv stage (conv2: 32 -> 64 channels on 32-row maps, conv3: 64 -> 128 on 16-row maps), shared by
// model_infer.hip and model_train_fwd.hip: the Winograd f16x3 kernel, or the bf16x6 fallback of that stage.
#pragma once
#include "conv_wino2_f16x3_kernel.h"

// OUT_MODE as in conv_wino2_f16x3_kernel.h (0 / 1: inference, BN + ReLU + pool; 2: training, raw output + statistics in `stats`).
// `geo`: the plan's geometry of this stage (its batch includes the template utterance when the plan has one); `nb`: utterances the
// fallback computes.  ctab / ncol_max: compacted task columns of the inference pad skip (Winograd only).  RAGGED (Winograd only): image b
// is wtab[b] >> wsh columns wide (conv_wino2_f16x3_kernel.h); the fallbacks run at full width on a map the caller has masked.
template <int CIN, int COUT, int OUT_MODE, bool RAGGED = false>
static inline int conv_fwd(sir_handle* h, hipStream_t st, bool wino, const Wino2Geo& geo, int nb, const float* x, const unsigned short* w_wino,
                           const unsigned short* w_fallback, const float* scale, const float* shift, float* out, float2* stats,
                           const int* ctab = nullptr, int ncol_max = 0, const int* wtab = nullptr, int wsh = 0) {
    static_assert((CIN == 32 && COUT == 64) || (CIN == 64 && COUT == 128), "conv2 or conv3");
    const int H = geo.H, W = geo.W;
    if (wino) {
        SIR_TRY(sir_lds_opt_in(h, (const void*)conv3x3_wino2_f16x3_kernel<CIN, COUT, OUT_MODE, 0, 3, RAGGED>, W2_LDS_BYTES));
        SIR_HIP_TRY((launch_conv_wino2<CIN, COUT, OUT_MODE, 0, 3, RAGGED>(st, geo, x, w_wino, scale, shift, out, stats, h->zero_page, h->num_cus, ctab,
                                                                         ncol_max, wtab, wsh)));
    } else if constexpr (CIN == 32) {     // first-generation Winograd kernel (64 output channels), blocks of two tile columns
        hipLaunchKernelGGL((conv3x3_wino_bf16x6_kernel<CIN, COUT, OUT_MODE == 2 ? 2 : 0>), dim3(((W + 1) / 2 + 1) / 2, 1, nb), dim3(256), WINO_LDS_BYTES, st,
                           x, w_wino, scale, shift, out, H, W, H / 2, W / 2, OUT_MODE == 2 ? stats : (float2*)nullptr);
    } else {                    // direct kernel on its nine-tap weights, 16 x 8-pixel tiles
        hipLaunchKernelGGL((conv3x3_bf16x6_ns_kernel<CIN, COUT, 2, 2, OUT_MODE, 0, 2, 1, 1>), dim3((W + 7) / 8, 1, nb), dim3(256), conv_ns_lds_bytes(2, 2, 2), st,
                           x, w_fallback, scale, shift, out, H, W, H / 2, W / 2, stats);
    }
    return SIR_OK;
}
