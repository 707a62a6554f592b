// Launcher of the quad-workgroup MFMA GRU recurrence (gru_quad_kernel.h).
#include <stdlib.h>
#include "gru_quad_kernel.h"
#include "gru_bwd_quad_kernel.h"

int sir_launch_gru_quad(sir_handle* h, hipStream_t st, bool save, const float* gi, const float* whh0, const float* whh1, const float* bhh0,
                        const float* bhh1, float* y, int B, int S, float* gates, unsigned short* yplanes, const void* wfrag0,
                        const void* wfrag1, const int* nlive, bool ragged) {
    if (ragged && !nlive) { sir_set_error("gru_quad: the ragged form needs the step counts"); return SIR_EINVAL; }
    if (S >= 511) { sir_set_error("gru_quad: %d steps exceed the 9-bit step field of the granule tag", S); return SIR_EUNSUPPORTED; }
    if (!wfrag0 || !wfrag1) { sir_set_error("gru_quad: the prepared W_hh fragments are required (sir_prep_whh_quad / train_prep_kernel)"); return SIR_EINVAL; }
    const int clusters = ((B + GQ_NU - 1) / GQ_NU) * 2;
    const dim3 grid(4 * (unsigned)clusters);
    // SIR_GRU_DBG: timing knock-outs and fault injection of gru_quad_kernel (see its `dbg` comment); 0 in production
    static const int dbg0 = getenv("SIR_GRU_DBG") ? atoi(getenv("SIR_GRU_DBG")) : 0;
    const int dbg = (dbg0 & ~(31 << 8)) | ((((dbg0 >> 8) & 31) ? ((dbg0 >> 8) & 31) : GQ_POLL_DELAY) << 8);
    // gate arithmetic and global accesses in the coalesced thread layout (ROLES) for the gate-saving (training) form, whose five 16-byte
    // stores per lane and step were fully exposed (layer 0: 79.5 -> 71.4 us); not for the inference form, where the extra barrier costs
    // more than its one to three stores (71.6 -> 74.7 us).  profiles/r04/ab_gq_roles.txt
    typedef void (*kern_t)(const float*, const float*, const float*, const float*, const float*, float*, int, int, float*, unsigned long long*,
                           unsigned int*, int, unsigned, unsigned short*, const uint4*, const uint4*, const int*);
    // (save && ragged: the ragged training step)
    const kern_t kern = save ? (ragged ? gru_quad_kernel<true, true, true> : gru_quad_kernel<true, true>)
                             : ragged ? gru_quad_kernel<false, false, true> : gru_quad_kernel<false, false>;
    SIR_TRY(sir_lds_opt_in(h, (const void*)kern, (int)GQ_LDS_BYTES));
    // the launch is chained with the handle's other cluster launches (sir_cluster_enter); leave runs whenever enter succeeded
    SIR_TRY(sir_cluster_enter(h, st));
    unsigned epoch = 0;
    void* xbuf = nullptr;
    int rc = sir_xbuf_acquire(h, st, 1, (size_t)clusters * GQ_XBUF_PER_CLUSTER, 127u, &xbuf, &epoch);
    if (rc == SIR_OK) {
        hipLaunchKernelGGL(kern, grid, dim3(GQ_THREADS), GQ_LDS_BYTES, st, gi, whh0, whh1, bhh0, bhh1, y, B, S, gates,
                           (unsigned long long*)xbuf, h->status, dbg, epoch, yplanes, (const uint4*)wfrag0, (const uint4*)wfrag1, nlive);
        rc = sir_check_hip(hipGetLastError(), "gru_quad_kernel");
    }
    const int rc_leave = sir_cluster_leave(h, st);
    return rc != SIR_OK ? rc : rc_leave;
}

// inference-side preparation of one direction's resident fragments (GRU_FRAG_BYTES)
void sir_prep_whh_quad(sir_handle* h, hipStream_t st, const float* whh, void* frag) {
    hipLaunchKernelGGL(prep_whh_quad_kernel, dim3(GQ_FRAG_THREADS / 256), dim3(256), 0, st, whh, (uint4*)frag, h->status);
}

// BPTT on the matrix cores, clusters of four workgroups x 16 utterances (gru_bwd_quad_kernel.h)
int sir_launch_gru_bwd_quad(sir_handle* h, hipStream_t st, const float* dy, const float* gates, const float* y, const float* whh0,
                            const float* whh1, float* dgi, float* dgh, float* bsum_i, float* bsum_h, int B, int S, const void* wfrag0,
                            const void* wfrag1, const int* nlive) {
    // nlive != NULL: the ragged form (steps of its own per utterance; see the kernel)
    typedef void (*kern_t)(const float*, const float*, const float*, const float*, const float*, float*, float*, float*, float*, int, int,
                           unsigned long long*, unsigned int*, unsigned, int, const uint4*, const uint4*, const int*);
    const kern_t kern = nlive ? gru_bwd_quad_kernel<true> : gru_bwd_quad_kernel<false>;
    if (S >= 65535) { sir_set_error("gru_bwd_quad: %d steps exceed the 16-bit step field of the granule tag", S); return SIR_EUNSUPPORTED; }
    if (!wfrag0 || !wfrag1) { sir_set_error("gru_bwd_quad: the prepared W_hh fragments are required (train_prep_kernel)"); return SIR_EINVAL; }
    const int clusters = ((B + GQ_NU - 1) / GQ_NU) * 2;
    const int dbg = GQ_POLL_DELAY << 8;                      // (`dbg` of gru_bwd_quad_kernel: no knock-outs, the first poll's delay)
    SIR_TRY(sir_lds_opt_in(h, (const void*)kern, (int)BQ_LDS_BYTES));
    SIR_TRY(sir_cluster_enter(h, st));
    unsigned epoch = 0;
    void* xbuf = nullptr;
    int rc = sir_xbuf_acquire(h, st, 3, (size_t)clusters * BQ_XBUF_PER_CLUSTER, 0xFFFFu, &xbuf, &epoch);
    if (rc == SIR_OK) {
        hipLaunchKernelGGL(kern, dim3(4 * (unsigned)clusters), dim3(GQ_THREADS), BQ_LDS_BYTES, st, dy, gates, y, whh0, whh1, dgi, dgh,
                           bsum_i, bsum_h, B, S, (unsigned long long*)xbuf, h->status, epoch, dbg, (const uint4*)wfrag0, (const uint4*)wfrag1, nlive);
        rc = sir_check_hip(hipGetLastError(), "gru_bwd_quad_kernel");
    }
    const int rc_leave = sir_cluster_leave(h, st);
    return rc != SIR_OK ? rc : rc_leave;
}
