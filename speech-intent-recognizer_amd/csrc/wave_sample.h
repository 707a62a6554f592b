// A waveform sample as a float on the device: float as it is, PCM16 dequantised as s / 32768 (SIR_WAVE_F32 / SIR_WAVE_I16;
// sir_wave_elem_bytes of sir_internal.h is the host side).  The one definition for the feature, reverb and perturbation kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace {

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<short>(short v) { return (float)v * (1.0f / 32768.0f); }

}  // namespace
