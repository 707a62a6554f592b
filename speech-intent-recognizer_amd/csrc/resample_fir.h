// The two things sir_resample (frontend.hip) and sir_stream_input_push (stream_input.hip) must agree on for a streamed
// conversion to give sir_resample's bits: the geometry of a rate pair and the chain that turns L taps into one output.
#pragma once
#include <math.h>
#include "sir_internal.h"

namespace {

constexpr int kLowpassWidth = 6;        // torchaudio's "sinc_interp_hann" defaults
constexpr double kRolloff = 0.99;

// gcd-reduced rates, the filter's cutoff base = min(orig, nw) * rolloff, torchaudio's `width`, and K = 2 width + orig, the
// length of torchaudio's kernel row: a phase's kept taps [first, first + L) lie inside [0, K)
struct ResampleGeo { int orig, nw, width, K; double base; };

int gcd_int(int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; }

ResampleGeo resample_geometry(int orig_freq, int new_freq) {
    ResampleGeo g;
    const int d = gcd_int(orig_freq, new_freq);
    g.orig = orig_freq / d;
    g.nw = new_freq / d;
    g.base = (g.orig < g.nw ? g.orig : g.nw) * kRolloff;
    g.width = (int)ceil(kLowpassWidth * (double)g.orig / g.base);
    g.K = 2 * g.width + g.orig;
    return g;
}

// one output: acc = fmaf(tp[l], sample(l), acc) for l = 0 .. L - 1, from acc = 0; sample(l) is the input at chain position l
template <typename F>
__device__ __forceinline__ float fir_chain(const float* __restrict__ tp, int L, F sample) {
    float acc = 0.0f;
    for (int l = 0; l < L; ++l) acc = fmaf(tp[l], sample(l), acc);
    return acc;
}

}  // namespace
