// rows_dev.h -- what the kernels that move whole vectors by index share: the gathers of kernels_rows.h (rows.hip) and the
// scatter of kernels_mutate.h (mutate.hip). Constants and a __forceinline__ device function only: no kernel lives here.
#pragma once

#include "common.h"

namespace innr {

constexpr int kRowsTile = 32;               // indices and dimensions per LDS tile of the store gather and scatter
constexpr uint32_t kRowsNone = 0xFFFFFFFFu;  // local index of a slot with nothing to load (N < 2^32 - 1: never a vector)

// global index -> local, kRowsNone (and *bad) when it is not this batch's
__device__ __forceinline__ uint32_t rows_local(uint64_t g, uint64_t base, uint32_t N, uint32_t* bad) {
    if (g < base || g - base >= (uint64_t)N) {
        *bad = 1u;
        return kRowsNone;
    }
    return (uint32_t)(g - base);
}

}  // namespace innr
