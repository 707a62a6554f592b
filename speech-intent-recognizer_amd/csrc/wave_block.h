// Workgroup shape of the segmentation and live-stream kernels (vad.hip, stream.hip, stream_input.hip and the headers they share)
#pragma once
#include "sir_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / SIR_WAVE;

}  // namespace
