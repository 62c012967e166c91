// quantize_dev.h -- what the kernels that produce u8 codes share: the corpus kernels of kernels_u8.h and kernels_gemm_i8.h
// (api.hip) and the row ingest of kernels_mutate_u8.h (mutate_u8.hip). A __forceinline__ device function only: no kernel lives here.
#pragma once

#include "common.h"

namespace innr {

// quantize_u8 (scalar.rs:212-225): clamp(round((v - offset) * (255/alpha)), 0, 255); round = half away from zero
__device__ __forceinline__ uint8_t quantize_one(float v, float offset, float inv_alpha) {
    const float r = __builtin_roundf(ex::mul(ex::sub(v, offset), inv_alpha));
    if (r != r) return 0;  // NaN `as u8` == 0
    return (uint8_t)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

}  // namespace innr
