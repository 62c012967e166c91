// kernels_mutate_u8.h -- the kernels of the entry points that change a u8 code batch in place (mutate_u8.hip):
//   scatter_rows_u8_pdx_kernel  row-major code rows into the dimension-major code store C8[d*ldN + i], transposed through LDS
//   quantize_rows_u8_kernel     row-major f32 rows into row-major code rows, quantize_u8 per value (quantize_dev.h)
// Appending and removing need no kernel of their own: transpose_rows_u8_kernel and the selection's count and gather (api.hip)
// serve them, and the indices of an update are validated by update_check_kernel (mutate.hip).
#pragma once

#include "quantize_dev.h"
#include "rows_dev.h"

namespace innr {

// The byte twin of scatter_rows_pdx_kernel (innr_batch_update_codes): C8[d*ldN + idx[j] - base] = in[j*D + d], j < n, d < D, through
// a tile of kRowsTile indices x kRowsTile dimensions. The loads run along d, the stores along the indices. mutate_u8.hip has
// validated the indices (update_check_kernel) before this runs; the kernel checks each again before it forms an address -- an
// index outside sets *bad and writes nothing. Dimensions are masked with d < D: rows D .. Dpad of the store stay zero. The grid
// strides over the tiles in both directions.
// EVERY STORE IS ONE BYTE. Four neighbouring vectors share a dword of a dimension row, and the other three may be written by
// another lane, wave or block of this launch, or not be named by the call at all: a read-modify-write of the dword would race
// with the first and overwrite the second. (Distinct indices -- the validation's other half -- mean that no two threads write
// one byte.) Wider stores for sorted indices were not tried: an update is bound by its host round trips.
// The tile's rows are 36 bytes apart: the transposed read of lane tx is at dword 9 tx + const, an odd stride over the banks.
constexpr int kRowsTileU8Pitch = kRowsTile + 4;
__global__ __launch_bounds__(256) void scatter_rows_u8_pdx_kernel(uint8_t* __restrict__ C8, size_t ldN, uint32_t N, uint32_t D,
                                                                  uint64_t base, const uint64_t* __restrict__ idx, size_t n,
                                                                  const uint8_t* __restrict__ in, uint32_t* __restrict__ bad) {
    __shared__ uint8_t tile[kRowsTile][kRowsTileU8Pitch];
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
                tile[ty + r][tx] = (j < n && d0 + tx < D) ? in[j * D + d0 + tx] : (uint8_t)0;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kRowsTile; r += 8) {
                const uint32_t d = d0 + ty + r;
                if (local != kRowsNone && d < D) C8[(size_t)d * ldN + local] = tile[tx][ty + r];
            }
            __syncthreads();  // the tile (and, after the last one, loc) is written again
        }
    }
}

// innr_batch_append_quantized / _update_quantized: out[t] = quantize_u8(in[t]) for the `total` = n*D contiguous values of row-major
// rows, four per thread and step. D need be no multiple of 4 and `in` only 4-byte aligned: the values in front of the first
// 16-byte boundary of `in` (at most 3) and behind the last whole group of four (at most 3) are done one by one, the groups between
// with one 16-byte load each; a group's four codes go out as one dword where `out` is aligned there, else byte by byte.
// Grid-strided.
__global__ __launch_bounds__(256) void quantize_rows_u8_kernel(const float* __restrict__ in, size_t total, float offset, float inv_alpha,
                                                               uint8_t* __restrict__ out) {
    const size_t head = std::min<size_t>(total, ((16u - (uint32_t)(reinterpret_cast<uintptr_t>(in) & 15u)) & 15u) >> 2);
    const size_t nvec = (total - head) / 4;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    const bool out4 = (reinterpret_cast<uintptr_t>(out + head) & 3u) == 0;
    for (size_t g = tid; g < nvec; g += step) {
        const float4 v = *reinterpret_cast<const float4*>(in + head + 4 * g);
        const uint32_t q0 = quantize_one(v.x, offset, inv_alpha), q1 = quantize_one(v.y, offset, inv_alpha);
        const uint32_t q2 = quantize_one(v.z, offset, inv_alpha), q3 = quantize_one(v.w, offset, inv_alpha);
        uint8_t* o = out + head + 4 * g;
        if (out4) {
            *reinterpret_cast<uint32_t*>(o) = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
        } else {
            o[0] = (uint8_t)q0;
            o[1] = (uint8_t)q1;
            o[2] = (uint8_t)q2;
            o[3] = (uint8_t)q3;
        }
    }
    const size_t tail0 = head + 4 * nvec;
    const size_t nends = head + (total - tail0);  // <= 6
    for (size_t s = tid; s < nends; s += step) {
        const size_t t = s < head ? s : tail0 + (s - head);
        out[t] = quantize_one(in[t], offset, inv_alpha);
    }
}

}  // namespace innr
