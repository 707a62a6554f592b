// Training step of CNNAudioGRU on MI355X, loss and optimizer: cross-entropy with hard or mixed / smoothed targets (sir_ce_loss,
// sir_ce_loss_soft), the global gradient norm and clip (sir_grad_norm), multi-tensor Adam and its variants (sir_adam_step,
// sir_adam_step_clipped, sir_adam_step_ex).
#include <cmath>
#include "train_loss_optim_kernels.h"

// sir_ce_loss and sir_ce_loss_soft share one kernel template; a hard target (no second label, no smoothing) takes the
// instantiation sir_ce_loss has always launched, so the two entry points agree bit for bit there.
static int ce_loss_launch(sir_handle* h, const char* who, const float* logits, const int64_t* labels, const int64_t* labels_b,
                          const float* lam, float eps, int batch, int num_classes, float* loss, float* dlogits, float grad_scale, hipStream_t st) {
    if (!h || !logits || !labels || !loss) { sir_set_error("%s: NULL argument", who); return SIR_EINVAL; }
    if (batch < 1 || num_classes < 1 || num_classes > 64) { sir_set_error("%s: bad shape batch=%d num_classes=%d (1..64)", who, batch, num_classes); return SIR_EINVAL; }
    if (!(eps >= 0.0f && eps < 1.0f)) { sir_set_error("%s: label_smoothing %g outside [0, 1)", who, (double)eps); return SIR_EINVAL; }
    const long long* la = (const long long*)labels;
    const long long* lb = (const long long*)labels_b;
    const bool soft = labels_b != nullptr || eps != 0.0f;
    SirProfScope prof(h, SIR_K_CE, st);
#define SIR_CE_LAUNCH(CMAX, SOFT) \
    hipLaunchKernelGGL((ce_loss_kernel<CMAX, SOFT>), dim3(1), dim3(256), 0, st, logits, la, batch, num_classes, loss, dlogits, grad_scale, \
                       h->status, lb, lam, eps)
    if (num_classes <= 32) { if (soft) SIR_CE_LAUNCH(32, true); else SIR_CE_LAUNCH(32, false); }
    else                   { if (soft) SIR_CE_LAUNCH(64, true); else SIR_CE_LAUNCH(64, false); }
#undef SIR_CE_LAUNCH
    SIR_KCHECK();
    return SIR_OK;
}

extern "C" int sir_ce_loss(sir_handle* h, const float* logits, const int64_t* labels, int batch, int num_classes,
                           float* loss, float* dlogits, float grad_scale, void* stream_) {
    return ce_loss_launch(h, "sir_ce_loss", logits, labels, nullptr, nullptr, 0.0f, batch, num_classes, loss, dlogits, grad_scale, (hipStream_t)stream_);
}

extern "C" int sir_ce_loss_soft(sir_handle* h, const float* logits, const int64_t* labels_a, const int64_t* labels_b,
                                const float* lam, float label_smoothing, int batch, int num_classes, float* loss, float* dlogits, float grad_scale, void* stream_) {
    return ce_loss_launch(h, "sir_ce_loss_soft", logits, labels_a, labels_b, lam, label_smoothing, batch, num_classes, loss, dlogits, grad_scale, (hipStream_t)stream_);
}

// ---- tensor tables: a block of 256 threads per SIR_ADAM_CHUNK elements, tensor after tensor ------------------------------------
// Fills the kernel argument of the Adam launches and returns its block count, or -1 with the error of entry point `who` set.
// `sh` (sir_adam_step_ex alone) with `ema`, which may be NULL: the shadow table too, under that entry point's stricter checks.
static int adam_table(const char* who, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                      float* const* exp_avg_sq, float* const* ema, const int64_t* sizes, int step, AdamTensors* ts, AdamShadow* sh) {
    if (n_tensors < 1 || n_tensors > SIR_ADAM_MAX_TENSORS || step < 1) { sir_set_error("%s: n_tensors=%d step=%d", who, n_tensors, step); return -1; }
    int blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (sh) {
            if (sizes[i] < 0) { sir_set_error("%s: size %d is negative", who, i); return -1; }
            if (ema && (!ema[i] || ema[i] == params[i])) { sir_set_error("%s: shadow %d is NULL or aliases its parameter", who, i); return -1; }
            sh->e[i] = ema ? ema[i] : nullptr;
        }
        ts->p[i] = params[i]; ts->g[i] = grads[i]; ts->m[i] = exp_avg[i]; ts->v[i] = exp_avg_sq[i]; ts->n[i] = sizes[i];
        ts->first_block[i] = blocks;
        blocks += (int)((sizes[i] + SIR_ADAM_CHUNK - 1) / SIR_ADAM_CHUNK);
    }
    if (sh)
        for (int i = n_tensors; i < SIR_ADAM_MAX_TENSORS; ++i) sh->e[i] = nullptr;
    ts->first_block[n_tensors] = blocks;
    ts->count = n_tensors;
    return blocks;
}

// The same for the gradient-norm launches; `ts` NULL: only the block count (sir_grad_norm_partials).  -1: bad count or size.
static int grad_table(int n_tensors, float* const* grads, const int64_t* sizes, GradTensors* ts) {
    if (!sizes || n_tensors < 1 || n_tensors > SIR_ADAM_MAX_TENSORS) return -1;
    long long blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (sizes[i] < 0) return -1;
        if (ts) { ts->g[i] = grads[i]; ts->n[i] = sizes[i]; ts->first_block[i] = (int)blocks; }
        blocks += (sizes[i] + SIR_ADAM_CHUNK - 1) / SIR_ADAM_CHUNK;
    }
    if (!(blocks > 0 && blocks < (1ll << 30))) return -1;
    if (ts) { ts->first_block[n_tensors] = (int)blocks; ts->count = n_tensors; }
    return (int)blocks;
}

extern "C" int sir_adam_step(sir_handle* h, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const int64_t* sizes, int step, float lr, float beta1, float beta2, float eps, float weight_decay, void* stream_) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !sizes) { sir_set_error("sir_adam_step: NULL argument"); return SIR_EINVAL; }
    AdamTensors ts;
    const int blocks = adam_table("sir_adam_step", n_tensors, params, grads, exp_avg, exp_avg_sq, nullptr, sizes, step, &ts, nullptr);
    if (blocks < 0) return SIR_EINVAL;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    SirProfScope prof(h, SIR_K_ADAM, (hipStream_t)stream_);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, ts, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2));
    SIR_KCHECK();
    return SIR_OK;
}

// ---- global gradient norm, clipping, clipped Adam ---------------------------------------------------------------------
extern "C" int sir_grad_norm_partials(int n_tensors, const int64_t* sizes) { return grad_table(n_tensors, nullptr, sizes, nullptr); }

extern "C" int sir_grad_norm(sir_handle* h, int n_tensors, float* const* grads, const int64_t* sizes, float max_norm,
                             float* partials, int partials_floats, float* out2, int scale_in_place, void* stream_) {
    if (!h || !grads || !sizes || !partials) { sir_set_error("sir_grad_norm: NULL argument"); return SIR_EINVAL; }
    GradTensors ts;
    const int blocks = grad_table(n_tensors, grads, sizes, &ts);
    if (blocks < 0) { sir_set_error("sir_grad_norm: n_tensors=%d (1..%d) or a bad size", n_tensors, SIR_ADAM_MAX_TENSORS); return SIR_EINVAL; }
    if (partials_floats < blocks) { sir_set_error("sir_grad_norm: partials holds %d floats, %d needed", partials_floats, blocks); return SIR_ENOMEM; }
    if (scale_in_place && !out2) { sir_set_error("sir_grad_norm: scale_in_place needs out2"); return SIR_EINVAL; }
    if (out2 && !(max_norm > 0.0f)) { sir_set_error("sir_grad_norm: max_norm %g must be > 0", (double)max_norm); return SIR_EINVAL; }
    for (int i = 0; i < n_tensors; ++i)
        if (!grads[i] && sizes[i] > 0) { sir_set_error("sir_grad_norm: NULL gradient %d", i); return SIR_EINVAL; }
    hipStream_t st = (hipStream_t)stream_;
    {   SirProfScope prof(h, SIR_K_GRAD_SUMSQ, st);
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, ts, partials);
        SIR_KCHECK();
    }
    if (!out2) return SIR_OK;
    SirProfScope prof(h, SIR_K_GRAD_CLIP, st);
    if (scale_in_place)
        hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(256), 0, st, ts, (const float*)partials, blocks, max_norm, out2);
    else
        hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partials, blocks, max_norm, out2);
    SIR_KCHECK();
    return SIR_OK;
}

extern "C" int sir_adam_step_clipped(sir_handle* h, int n_tensors, float* const* params, const float* const* grads,
                                     float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes, int step, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, const float* partials,
                                     int n_partials, float max_norm, float* out2, void* stream_) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !sizes || !partials || !out2) { sir_set_error("sir_adam_step_clipped: NULL argument"); return SIR_EINVAL; }
    AdamTensors ts;
    const int blocks = adam_table("sir_adam_step_clipped", n_tensors, params, grads, exp_avg, exp_avg_sq, nullptr, sizes, step, &ts, nullptr);
    if (blocks < 0) return SIR_EINVAL;
    if (!(max_norm > 0.0f) || n_partials < 1) { sir_set_error("sir_adam_step_clipped: max_norm %g must be > 0, n_partials %d >= 1", (double)max_norm, n_partials); return SIR_EINVAL; }
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    SirProfScope prof(h, SIR_K_ADAM_CLIPPED, (hipStream_t)stream_);
    hipLaunchKernelGGL(adam_multi_clipped_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, ts, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)sqrt(bc2), partials, n_partials, max_norm, out2);
    SIR_KCHECK();
    return SIR_OK;
}

// ---- every variant of the optimizer step behind one call ---------------------------------------------------------------
template <bool CLIP>
static void launch_adam_ex(bool decoupled, bool ema, int blocks, hipStream_t st, const AdamTensors& ts, const AdamShadow& sh,
                           const sir_adam_config* c, float decay_f, float bc1, float bc2_sqrt, const float* partials, int n_partials, float* out2) {
#define SIR_ADAM_EX_LAUNCH(D, E)                                                                                               \
    hipLaunchKernelGGL((adam_multi_ex_kernel<CLIP, D, E>), dim3(blocks), dim3(256), 0, st, ts, sh, c->lr, c->beta1, c->beta2,    \
                       c->eps, c->weight_decay, decay_f, c->ema_decay, bc1, bc2_sqrt, partials, n_partials, c->max_norm, out2)
    if (decoupled && ema) SIR_ADAM_EX_LAUNCH(true, true);
    else if (decoupled) SIR_ADAM_EX_LAUNCH(true, false);
    else SIR_ADAM_EX_LAUNCH(false, true);
#undef SIR_ADAM_EX_LAUNCH
}

extern "C" int sir_adam_step_ex(sir_handle* h, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                float* const* exp_avg_sq, float* const* ema, const int64_t* sizes, int step,
                                const sir_adam_config* cfg, const float* partials, int n_partials, float* out2, void* stream_) {
    if (!h || !params || !grads || !exp_avg || !exp_avg_sq || !sizes || !cfg) { sir_set_error("sir_adam_step_ex: NULL argument"); return SIR_EINVAL; }
    const float fl[7] = {cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, cfg->max_norm, cfg->ema_decay};
    for (float f : fl)
        if (f != f) { sir_set_error("sir_adam_step_ex: NaN in the configuration"); return SIR_EINVAL; }
    if (!(cfg->ema_decay >= 0.0f && cfg->ema_decay < 1.0f)) { sir_set_error("sir_adam_step_ex: ema_decay %g outside [0, 1)", (double)cfg->ema_decay); return SIR_EINVAL; }
    const bool use_ema = cfg->ema_decay > 0.0f, clip = cfg->max_norm > 0.0f, decoupled = cfg->decoupled != 0;
    if (use_ema != (ema != nullptr)) { sir_set_error("sir_adam_step_ex: `ema` must be given exactly when ema_decay > 0"); return SIR_EINVAL; }
    if (cfg->max_norm < 0.0f) { sir_set_error("sir_adam_step_ex: max_norm %g must be >= 0", (double)cfg->max_norm); return SIR_EINVAL; }
    if (clip && (!partials || !out2 || n_partials < 1)) { sir_set_error("sir_adam_step_ex: max_norm > 0 needs partials, n_partials >= 1 and out2"); return SIR_EINVAL; }
    if (!decoupled && !use_ema)              // nothing new asked for: the existing launches, bit for bit
        return clip ? sir_adam_step_clipped(h, n_tensors, params, grads, exp_avg, exp_avg_sq, sizes, step, cfg->lr, cfg->beta1, cfg->beta2,
                                            cfg->eps, cfg->weight_decay, partials, n_partials, cfg->max_norm, out2, stream_)
                    : sir_adam_step(h, n_tensors, params, grads, exp_avg, exp_avg_sq, sizes, step, cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, stream_);
    AdamTensors ts;
    AdamShadow sh;
    const int blocks = adam_table("sir_adam_step_ex", n_tensors, params, grads, exp_avg, exp_avg_sq, use_ema ? ema : nullptr, sizes, step, &ts, &sh);
    if (blocks < 0) return SIR_EINVAL;
    if (blocks < 1) return SIR_OK;           // every tensor empty
    const double bc1 = 1.0 - pow((double)cfg->beta1, step), bc2 = 1.0 - pow((double)cfg->beta2, step);
    const float decay_f = (float)(1.0 - (double)cfg->lr * (double)cfg->weight_decay);
    hipStream_t st = (hipStream_t)stream_;
    SirProfScope prof(h, clip ? SIR_K_ADAM_EX_CLIPPED : SIR_K_ADAM_EX, st);
    if (clip) launch_adam_ex<true>(decoupled, use_ema, blocks, st, ts, sh, cfg, decay_f, (float)bc1, (float)sqrt(bc2), partials, n_partials, out2);
    else launch_adam_ex<false>(decoupled, use_ema, blocks, st, ts, sh, cfg, decay_f, (float)bc1, (float)sqrt(bc2), nullptr, 0, nullptr);
    SIR_KCHECK();
    return SIR_OK;
}
