// What the two live-stream stages share (stream.hip: sir_stream_*, stream_input.hip: sir_stream_input_*): the limits of a
// stream set, the samples a push brings, the checks of a push and of the caller-owned state buffer, and the masked reset.
#pragma once
#include "wave_block.h"

namespace {

constexpr int kMaxStreams = 65535;
constexpr int kMaxIn = 1 << 24;

// samples of a stream's row that a push takes: its length clamped to [0, min(in_width, max_in)]
__host__ __device__ __forceinline__ int new_samples(int len, int in_width, int max_in) {
    const int cap = in_width < max_in ? in_width : max_in;
    return len < 0 ? 0 : (len > cap ? cap : len);
}

// config rule; a failure is reported in who's name (NULL: silently)
bool stream_limits_ok(const char* who, int n_streams, int max_in) {
    if (n_streams >= 1 && n_streams <= kMaxStreams && max_in >= 1 && max_in <= kMaxIn) return true;
    if (who) sir_set_error("%s: bad sizes (n_streams %d must be in [1, %d], max_in %d in [1, %d])", who, n_streams, kMaxStreams, max_in, kMaxIn);
    return false;
}

bool push_sizes_ok(const char* who, int in_width, int max_in, int64_t in_stride) {
    if (in_width >= 1 && in_width <= max_in && in_stride >= in_width) return true;
    sir_set_error("%s: bad sizes (in_width %d must be in [1, max_in %d], in_stride %lld >= in_width)", who, in_width, max_in, (long long)in_stride);
    return false;
}

// need: the bytes the stage's layout asks for
int state_ok(const char* who, const void* state, size_t state_bytes, size_t need) {
    if ((uintptr_t)state % 256 != 0) { sir_set_error("%s: state must be 256-byte aligned", who); return SIR_EINVAL; }
    if (state_bytes < need) { sir_set_error("%s: state of %zu bytes, %zu needed", who, state_bytes, need); return SIR_ENOMEM; }
    return SIR_OK;
}

// State{} is a stream that has received nothing; mask NULL: every stream
template <typename State>
__global__ __launch_bounds__(kThreads) void stream_reset_kernel(State* __restrict__ state, const unsigned char* __restrict__ mask, int S) {
    const int s = blockIdx.x * kThreads + threadIdx.x;
    if (s < S && (mask == nullptr || mask[s] != 0)) state[s] = State{};
}

template <typename State>
int stream_reset_launch(State* state, const uint8_t* mask, int S, hipStream_t st) {
    hipLaunchKernelGGL(stream_reset_kernel<State>, dim3((S + kThreads - 1) / kThreads), dim3(kThreads), 0, st, state, mask, S);
    return sir_check_hip(hipGetLastError(), "stream_reset_kernel");
}

}  // namespace
