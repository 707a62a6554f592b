// Shape of one model call -- the map sizes shared by inference and training -- and the conv plan: which of the conv2 / conv3
// stages run on their Winograd kernels and which on the shape fallbacks.  Decided once per call, here and nowhere else: the weight
// preparation, the forward and backward launches and the workspace sizing all read the same plan, so the forward's prepared weights
// are in the form the backward will launch.  Host code only.
#pragma once
#include "wino2_geo.h"

constexpr int ATT_MAX_S = 256;      // GRU steps the attention kernels hold in LDS (model_kernels.h, train_bwd_kernels.h)
// what sir_make_dims accepts, for the refusal messages: S = t_frames / 8 in [1, ATT_MAX_S] (2055 / 8 = 256, 2056 / 8 = 257)
#define SIR_SHAPE_LIMITS "8 <= t_frames <= 2055 (at most 256 GRU steps), batch <= 65535"

// conv stage `conv` (2 or 3) runs on its Winograd kernel (second-generation forward / data gradient, Winograd weight gradient) if
// `shape_ok` -- else on the first-generation / direct fallback.  Test-only SIR_CONV_FALLBACK: 1 = conv2's stages do not fit, 2 = none do.
bool sir_conv_stage_fits(int conv, bool shape_ok);

struct SirConvPlan {
    bool fwd_wino;                      // conv2 AND conv3 forward (the forward needs both maps to fit)
    bool dgrad2_wino, dgrad3_wino;      // data gradients
    bool wgrad2_wino, wgrad3_wino;      // weight gradients
    Wino2Geo geo2, geo3;                // the forward's launch geometry (batch + template utterance); the data gradients' too when there is none
};

// (plain ints only: the table kernels of infer_tables.h take an extension of this struct, Dims of infer_workspace.h, by value)
struct SirDims {
    int B, T, wp1, wp2, wp3, S;         // batch, frames, map widths behind conv1 / conv2 / conv3, GRU steps
};

static inline bool sir_make_dims(int batch, int t_frames, SirDims* d) {
    d->B = batch; d->T = t_frames;
    d->wp1 = t_frames / 2; d->wp2 = d->wp1 / 2; d->wp3 = d->wp2 / 2; d->S = d->wp3;
    return batch > 0 && d->S >= 1 && d->S <= ATT_MAX_S && batch <= 65535;
}

// `template_utt`: one extra all-zero utterance rides through the forward convolutions (inference pad skip, model_infer.hip)
static inline SirConvPlan sir_conv_plan(const SirDims* d, bool template_utt) {
    SirConvPlan p;
    const int batch = d->B, bf = batch + (template_utt ? 1 : 0);
    const bool ok2 = wino2_geo(bf, 32, d->wp1, 64, &p.geo2), ok3 = wino2_geo(bf, 16, d->wp2, 128, &p.geo3);
    p.fwd_wino = sir_conv_stage_fits(2, ok2) && sir_conv_stage_fits(3, ok3);
    Wino2Geo g;                         // the backward runs on the batch alone
    p.dgrad2_wino = sir_conv_stage_fits(2, wino2_geo(batch, 32, d->wp1, 64, &g));
    p.dgrad3_wino = sir_conv_stage_fits(3, wino2_geo(batch, 16, d->wp2, 128, &g));
    // the weight-gradient kernels address dz in BYTES through 32-bit buffer offsets: a tighter bound than wino2_geo's element count
    p.wgrad2_wino = sir_conv_stage_fits(2, (size_t)batch * 32 * d->wp1 * 64 * 4 < ((size_t)1 << 31));
    p.wgrad3_wino = sir_conv_stage_fits(3, (size_t)batch * 16 * d->wp2 * 128 * 4 < ((size_t)1 << 31));
    return p;
}
