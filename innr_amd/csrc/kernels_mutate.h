// kernels_mutate.h -- the kernels of innr_batch_update_rows (mutate.hip): the write direction of kernels_rows.h.
//   update_check_kernel      the indices of a call against the batch's range and against each other (a bitmap, atomicOr)
//   scatter_rows_pdx_kernel  row-major rows into the dimension-major store V[d*ldN + i], transposed through LDS
// The scatter is a copy: values move as 32-bit words, so a NaN keeps sign and payload and a denormal stays one. Appending and
// removing rows need no kernel of their own: transpose_rows_kernel and the selection's count and gather (api.hip) serve them.
#pragma once

#include "rows_dev.h"

namespace innr {

// The mirror of gather_rows_pdx_kernel (innr_batch_update_rows): V[d*ldN + idx[j] - base] = in[j*D + d], j < n, d < D, through the
// same tile. Here the loads run along d (whole cache lines of the input rows) and the stores along the indices, so that sorted or
// clustered indices write whole lines of a dimension row. mutate.hip has validated the indices (update_check_kernel) before this
// runs; the kernel checks each again before it forms an address -- an index outside sets *bad and writes nothing. Distinct indices
// (the validation's other half) mean that no two threads write one word. Dimensions are masked with d < D: rows D .. Dpad of the
// store stay zero. The grid strides over the tiles in both directions.
__global__ __launch_bounds__(256) void scatter_rows_pdx_kernel(uint32_t* __restrict__ V, size_t ldN, uint32_t N, uint32_t D,
                                                               uint64_t base, const uint64_t* __restrict__ idx, size_t n,
                                                               const uint32_t* __restrict__ in, uint32_t* __restrict__ bad) {
    __shared__ uint32_t tile[kRowsTile][kRowsTile + 1];
    __shared__ uint32_t loc[kRowsTile];
    const uint32_t tx = threadIdx.x, ty = threadIdx.y;
    const size_t ntile_i = (n + kRowsTile - 1) / kRowsTile;
    const uint32_t ntile_d = (D + kRowsTile - 1) / kRowsTile;
    for (size_t ti = blockIdx.x; ti < ntile_i; ti += gridDim.x) {
        const size_t j0 = ti * kRowsTile;
        if (ty == 0) loc[tx] = j0 + tx < n ? rows_local(idx[j0 + tx], base, N, bad) : kRowsNone;
        __syncthreads();
        const uint32_t local = loc[tx];
        for (uint32_t td = blockIdx.y; td < ntile_d; td += gridDim.y) {
            const uint32_t d0 = td * kRowsTile;
#pragma unroll
            for (int r = 0; r < kRowsTile; r += 8) {
                const size_t j = j0 + ty + r;
                tile[ty + r][tx] = (j < n && d0 + tx < D) ? in[j * D + d0 + tx] : 0u;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kRowsTile; r += 8) {
                const uint32_t d = d0 + ty + r;
                if (local != kRowsNone && d < D) V[(size_t)d * ldN + local] = tile[tx][ty + r];
            }
            __syncthreads();  // the tile (and, after the last one, loc) is written again
        }
    }
}

// The index validation of innr_batch_update_rows: every idx[j], j < n, against [base, base + N) and against the other indices of
// the call. bits: one bit per vector of the batch (ceil(N / 32) words, zeroed by the caller once per CALL -- the host entry point
// runs this once per staging round on the same bitmap); an index whose bit is already set occurs twice. flag (4 words + 2 x 64
// bits, zeroed per call): [0] an index outside the range was seen, [1] a duplicate; one offending index of each kind at
// flag64[1] / flag64[2] (whichever thread wrote last: any of them serves the message). Grid-strided, one index per thread and step.
__global__ __launch_bounds__(256) void update_check_kernel(const uint64_t* __restrict__ idx, size_t n, uint64_t base, uint32_t N,
                                                           uint32_t* __restrict__ bits, uint32_t* __restrict__ flag) {
    unsigned long long* flag64 = reinterpret_cast<unsigned long long*>(flag);
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += step) {
        const uint64_t g = idx[j];
        if (g < base || g - base >= (uint64_t)N) {
            flag[0] = 1u;
            flag64[1] = g;
            continue;
        }
        const uint32_t l = (uint32_t)(g - base), bit = 1u << (l & 31);
        if (atomicOr(&bits[l >> 5], bit) & bit) {
            flag[1] = 1u;
            flag64[2] = g;
        }
    }
}

}  // namespace innr
