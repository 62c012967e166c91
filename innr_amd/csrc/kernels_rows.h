// kernels_rows.h -- search by stored vector (innr_batch_gather_rows / innr_batch_knn_rows, rows.hip): reading vectors of the
// corpus back as row-major rows, and taking a query's own index out of its result. DESIGN.md 4.5f.
//   gather_rows_pdx_kernel   rows out of the dimension-major store V[d*ldN + i], transposed through LDS
//   gather_rows_copy_kernel  rows out of the row-major copy rows[i*Dr + d] (INNR_COPY_ROWS) where the batch has built one
//   strip_self_kernel        [Q][kk] staged results -> [Q][kk - 1] without the entry whose index is the query's own
// The gathers are copies: values move as 32-bit words, so a NaN keeps sign and payload and a denormal stays one. Both check
// every index against [base, base + N) before they form an address from it: an index outside sets *bad, reads nothing and
// writes zeros (rows.hip reports it at the end of the call). Both give the same bits.
#pragma once

#include "rows_dev.h"  // kRowsTile, kRowsNone, rows_local: shared with the scatter of kernels_mutate.h

namespace innr {

// out[j*D + d] = V[d*ldN + idx[j] - base], j < n, d < D. A block of 32 x 8 threads owns tiles of 32 indices x 32 dimensions: for
// the loads threadIdx.x runs along the indices (consecutive indices: whole cache lines of a dimension row), for the stores along
// d (whole cache lines of the output rows); in between the tile lies in LDS, padded to 33 words a row so that both the row-wise
// writes and the column-wise reads touch 32 different banks. Dimensions are masked with d < D, not with the padded row count:
// rows D .. Dpad of a prefix view hold the parent's next dimensions. The grid strides over the tiles in both directions.
__global__ __launch_bounds__(256) void gather_rows_pdx_kernel(const uint32_t* __restrict__ V, size_t ldN, uint32_t N, uint32_t D,
                                                              uint64_t base, const uint64_t* __restrict__ idx, size_t n,
                                                              uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
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
                const uint32_t d = d0 + ty + r;
                tile[ty + r][tx] = (local != kRowsNone && d < D) ? V[(size_t)d * ldN + local] : 0u;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kRowsTile; r += 8) {
                const size_t j = j0 + ty + r;
                if (j < n && d0 + tx < D) out[j * D + d0 + tx] = tile[tx][ty + r];
            }
            __syncthreads();  // the tile (and, after the last one, loc) is written again
        }
    }
}

// the same from the row-major copy: one wave per row, the grid strides over the rows. vec: D % 4 == 0 and `out` is 16-byte
// aligned, so every output row is (the copy's rows always are: Dr is a multiple of 4) -- 16 bytes per lane and access.
__global__ __launch_bounds__(256) void gather_rows_copy_kernel(const uint32_t* __restrict__ rows, uint32_t Dr, uint32_t N, uint32_t D,
                                                               uint64_t base, const uint64_t* __restrict__ idx, size_t n,
                                                               uint32_t* __restrict__ out, uint32_t* __restrict__ bad, int vec) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * 4;
    for (size_t j = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += nwaves) {
        const uint32_t local = rows_local(idx[j], base, N, bad);
        uint32_t* dst = out + j * D;
        if (local == kRowsNone) {
            for (uint32_t d = lane; d < D; d += 64) dst[d] = 0u;
            continue;
        }
        const uint32_t* src = rows + (size_t)local * Dr;
        if (vec) {
            const uint4* s4 = reinterpret_cast<const uint4*>(src);
            uint4* d4 = reinterpret_cast<uint4*>(dst);
            for (uint32_t v = lane; v < D / 4; v += 64) d4[v] = s4[v];
        } else {
            for (uint32_t d = lane; d < D; d += 64) dst[d] = src[d];
        }
    }
}

// One wave per query over its kk staged entries (best first): p = the position of the entry whose index is self[q], kk - 1 when
// there is none (the dot metric; duplicates with lower indices) -- exactly one entry goes. The other kk - 1 keep their order.
__global__ __launch_bounds__(256) void strip_self_kernel(const uint64_t* __restrict__ st_idx, const float* __restrict__ st_score,
                                                         uint32_t kk, const uint64_t* __restrict__ self, uint32_t Q,
                                                         uint64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;  // (a whole wave leaves: the ballots below see full waves only)
    const uint64_t me = self[q];
    const uint64_t* si = st_idx + (size_t)q * kk;
    const float* ss = st_score + (size_t)q * kk;
    uint32_t p = kk - 1;
    for (uint32_t s = 0; s < kk; s += 64) {
        const unsigned long long hit = __ballot(s + lane < kk && si[s + lane] == me);
        if (hit) {
            p = s + (uint32_t)__ffsll((long long)hit) - 1;
            break;
        }
    }
    uint64_t* oi = out_idx + (size_t)q * (kk - 1);
    float* os = out_score + (size_t)q * (kk - 1);
    for (uint32_t e = lane; e + 1 < kk; e += 64) {
        const uint32_t from = e < p ? e : e + 1;
        oi[e] = si[from];
        os[e] = ss[from];
    }
}

}  // namespace innr
