// Shared pieces of the token-reduction ("TN") GEMMs of the GRU backward (gemm_tn2_f16x3_kernel.h) and of the convolution weight
// gradients that are built the same way (wgrad_wino_f16x3_kernel.h, wgrad_bf16x6_kernel.h): tile sizes, the swizzled k-major LDS
// image and its transposed reads, the job table.
//
//   dW[m][n] = sum_tok A[tok][m] * B[tok (+shift)][n]       A = dgi / dgh slice [tokens][768], B = layer input or h_prev
// Both operands are token-major in memory, i.e. TRANSPOSED with respect to what a 16-bit MFMA wants (eight consecutive
// k = tokens per lane).  The transposition is done by the LDS hardware on the way OUT: a 32-token stage is written in its natural
// [token][column] order -- thread = (token, 4 columns) reads a float4 (lanes along the columns: 512-byte coalesced rows), splits
// it into the operand planes and issues ONE ds_write_b64 per plane -- and the MFMA fragments are fetched with
// ds_read_b64_tr_b16 (gfx950), which hands lane i column i of a 4-token x 16-column block: two of them make the lane's eight
// consecutive tokens.  64-byte chunks of a row are XOR-swizzled with the token index so that the four rows of a transposed read
// fall on the four quarters of the bank line (conflict-free reads AND stores).
// One launch covers up to four jobs (both directions x {W_ih, W_hh} of a layer): blockIdx.x walks the 128 x 256 output
// tiles of all jobs, blockIdx.y the K splits; every (tile, split) writes its partial to the job's slab z (deterministic
// slab_reduce afterwards).
//   seq / shift: row tok of B is taken from row tok + shift of the same length-`seq` sequence, zero outside it (the
//   h_{t-1} / h_{t+1} operand of the W_hh gradient).
#pragma once
#include "bf16x6_kernels.h"

constexpr int TN_BM = 128, TN_BN = 256, TN_BK = 32;
constexpr int TN2_BM = 128;                                   // (gemm_tn2_f16x3_kernel.h; here because the workspace sizing reads it too)
constexpr int TN_ROWB = TN_BK * 2 + 16;                      // k-contiguous image (A of dX): 80 B per row, 5 sixteen-byte slots (odd -> conflict-free b128 reads)
// k-major image of an operand given as [k][x] (x contiguous): per plane 32 rows of 2 X bytes, 64-byte chunks swizzled
constexpr size_t tn_lds_bytes(bool a_km, int bm) {
    return (size_t)3 * (a_km ? TN_BK * bm * 2 : bm * TN_ROWB) + (size_t)3 * TN_BK * TN_BN * 2;
}

// byte offset of element (row k, byte xb of the row) in a k-major image with XW-byte rows.  The four rows k0 .. k0+3 of a
// transposed read (k0 a multiple of 4) put their 64-byte chunk on four different quarters of the 256-byte bank line:
//   XW >= 256: chunk c -> c ^ (k & 3);   XW = 128: chunk c -> c ^ ((k >> 1) & 1)   (rows k and k + 2 share a line half)
template <int XW>
__device__ __forceinline__ int tn_kmaj_off(int k, int xb) {
    const int key = XW == 128 ? ((k >> 1) & 1) : (k & 3);
    return k * XW + ((((xb >> 6) ^ key)) << 6) + (xb & 63);
}
typedef short tn_v4i16 __attribute__((ext_vector_type(4)));
// eight consecutive k of one column as an MFMA fragment: two hardware-transposed reads (k .. k+3 and k+4 .. k+7), XW-byte rows
template <int XW>
__device__ __forceinline__ bf16x8 tn_tr_fragment(const unsigned char* p) {
    struct { tn_v4i16 lo, hi; } f;
    f.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_v4i16 __attribute__((address_space(3)))*)(p));
    f.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tn_v4i16 __attribute__((address_space(3)))*)(p + 4 * XW));
    return __builtin_bit_cast(bf16x8, f);
}

// keep mask of the inter-layer dropout (same function as train_fwd_kernels.h dropout_keep; the dX GEMM of layer 1 applies the
// dropout BACKWARD in its epilogue: its output IS d(dropout(y0)), and y0's gradient is that times the mask / (1 - p))
__device__ __forceinline__ bool tn_dropout_keep(unsigned long long seed, size_t idx, float p) {
    unsigned long long x = seed ^ (idx * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return (float)(unsigned)(x >> 40) * (1.0f / 16777216.0f) >= p;
}

struct TnJobs {
    const float* A[4]; const float* B[4]; float* slab[4];   // slab[j] + z * slab_stride[j] receives split z of job j
    const float* B2[4]; int brows[4];                        // rows k >= brows[j] of B come from B2[j] (two stacked matrices); 0 = off
    int lda[4], ldb[4], N[4], shift[4];
    size_t slab_stride[4];
    int tile0[5];                                            // first tile index of each job (prefix sums), tile0[njobs] = total
    int njobs;
    float drop_p;                                            // > 0: out[m][n] *= keep(drop_seed, m * N + n) / (1 - drop_p)
    unsigned long long drop_seed;
    const float* zeros;                                      // >= 256 zero floats (the handle's zero page): B rows that must read as zero (gemm_tn2)
};
