// A stored waveform sample as a float on the device: the only place where that conversion is written down.  By element type
// (to_f32<T>: float as it is, PCM16 dequantised as s / 32768; sir_wave_elem_bytes of sir_internal.h is the host side) for the
// stages that take SIR_WAVE_F32 / SIR_WAVE_I16, and by dtype tag (WaveElem<DT>, decode<DT>) for the stream input, which also
// takes G.711 bytes.  The feature kernels' packed two-samples-per-word reads (feat_common.h, features_gen.hip) are their own layout.
#pragma once
#include <hip/hip_runtime.h>
#include "sir_hip.h"

namespace {

__device__ __forceinline__ float pcm16_to_f32(int s) { return (float)s * (1.0f / 32768.0f); }

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<short>(short v) { return pcm16_to_f32(v); }

// element type of a SIR_WAVE_* dtype
template <int DT> struct WaveElem;
template <> struct WaveElem<SIR_WAVE_F32> { typedef float type; };
template <> struct WaveElem<SIR_WAVE_I16> { typedef short type; };
template <> struct WaveElem<SIR_WAVE_ULAW> { typedef unsigned char type; };
template <> struct WaveElem<SIR_WAVE_ALAW> { typedef unsigned char type; };

// one element of dtype DT -> float32 (include/sir_hip.h): G.711 bytes expand to their 14 / 13-bit PCM value on the int16 scale
template <int DT>
__device__ __forceinline__ float decode(typename WaveElem<DT>::type x) {
    if constexpr (DT == SIR_WAVE_F32 || DT == SIR_WAVE_I16) {
        return to_f32(x);
    } else if constexpr (DT == SIR_WAVE_ULAW) {
        const int u = ~(int)x & 0xFF;
        const int t = (((u & 0x0F) << 3) + 0x84) << ((u >> 4) & 7);
        return pcm16_to_f32((u & 0x80) ? 0x84 - t : t - 0x84);
    } else {
        const int a = (int)x ^ 0x55, e = (a >> 4) & 7, m = a & 0x0F;
        const int t = e ? ((m << 4) + 0x108) << (e - 1) : (m << 4) + 8;
        return pcm16_to_f32((a & 0x80) ? t : -t);
    }
}

}  // namespace
