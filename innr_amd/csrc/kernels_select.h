// kernels_select.h -- the selection behind innr_batch_knn_filtered_multi (batch_knn_filtered, batch.rs:820-882, for Q queries):
// the vectors that pass the caller's mask, gathered in index order into a compact dimension-major batch of their own, which
// any kNN engine then searches; the results' indices are mapped back to the parent's.
//
// A vector's exact score depends on that vector and the query only, and the gather keeps index order, so "ties go to the lower
// index" is the same rule in compact and in parent indices: the search on the selection returns the parent's filtered answer bit
// for bit. Chunks of kSelChunk consecutive vectors (one wave, a lane owns 4 of them, like the scan kernels) are the unit of the
// count, the scan of the counts (exclusive_scan_kernel, kernels_ext.h) and the gather.
#pragma once

#include "common.h"

namespace innr {

constexpr int kSelChunk = 64 * 4;  // vectors per chunk: 64 lanes x 4
constexpr uint32_t kSelSlab = 64;  // dimension rows per gather block (blockIdx.y); more where D would need > 65535 slabs

// The passing vectors of the lanes below `lane` in the wave (returned) and of the whole wave (*chunk_total). m4: one 0/1 byte per
// vector of the lane's 4 (byte c = vector c). Every lane of the wave must call this (ballots).
__device__ __forceinline__ uint32_t sel_pass_below(uint32_t m4, int lane, uint32_t* chunk_total) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t below = 0, total = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long b = __ballot((m4 >> (8 * c)) & 1u);
        below += (uint32_t)__popcll(b & lt);
        total += (uint32_t)__popcll(b);
    }
    *chunk_total = total;
    return below;
}

// 1. The caller's mask (N bytes, mask[i] != 0 <=> pass; any alignment) folded to 0/1 into nm[0, ldN) (zero beyond N), the passing
//    vectors per chunk, and -- old != null: the normalised mask of the cached selection -- *diff = 1 on any difference.
//    Grid: ceil(nchunks / 4) blocks of 256 threads, one wave per chunk.
__global__ __launch_bounds__(256) void select_mask_kernel(const uint8_t* __restrict__ mask, uint32_t N, size_t nchunks,
                                                          uint8_t* __restrict__ nm, const uint8_t* __restrict__ old,
                                                          uint32_t* __restrict__ chunk_count, uint32_t* __restrict__ diff) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t ch = (size_t)blockIdx.x * 4 + w;
    if (ch >= nchunks) return;  // wave-uniform
    const size_t col = ch * kSelChunk + (size_t)lane * 4;
    uint32_t m4 = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (col + c < N && mask[col + c]) m4 |= 1u << (8 * c);
    *reinterpret_cast<uint32_t*>(nm + col) = m4;
    if (old && *reinterpret_cast<const uint32_t*>(old + col) != m4) *diff = 1u;
    uint32_t total;
    (void)sel_pass_below(m4, lane, &total);
    if (lane == 0) chunk_count[ch] = total;
}

// 2. The gather (the hot path): S[d * ldS + rank(i)] = V[d * ldN + i] for every passing i and d in this block's slab of rows
//    (d < D only: rows D..Dpad of the selection keep the zeros alloc_batch wrote), map[rank(i)] = i (blocks with blockIdx.y == 0).
//    rank(i) = chunk_off[chunk] + the passing vectors before i in its chunk. A lane whose 4 vectors all fail issues no load: a
//    sparse or clustered mask reads only the cache lines it needs. Grid: (ceil(nchunks / 4), max(1, ceil(D / slab))), 256 threads.
__global__ __launch_bounds__(256) void select_gather_kernel(const float* __restrict__ V, size_t ldN, uint32_t D,
                                                            const uint8_t* __restrict__ nm, const uint32_t* __restrict__ chunk_off,
                                                            size_t nchunks, float* __restrict__ S, size_t ldS,
                                                            uint32_t* __restrict__ map, uint32_t slab) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t ch = (size_t)blockIdx.x * 4 + w;
    if (ch >= nchunks) return;  // wave-uniform
    const size_t col = ch * kSelChunk + (size_t)lane * 4;
    const uint32_t m4 = *reinterpret_cast<const uint32_t*>(nm + col);
    uint32_t total;
    const uint32_t r0 = chunk_off[ch] + sel_pass_below(m4, lane, &total);
    if (m4 == 0) return;
    uint32_t r[4];
    {
        uint32_t r_ = r0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = r_;
            r_ += (m4 >> (8 * c)) & 1u;
        }
    }
    if (blockIdx.y == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((m4 >> (8 * c)) & 1u) map[r[c]] = (uint32_t)(col + c);
    }
    const uint32_t d0 = blockIdx.y * slab;
    const uint32_t d1 = (d0 < D && slab < D - d0) ? d0 + slab : D;
    const float* src = V + col;
#pragma unroll 8
    for (uint32_t d = d0; d < d1; ++d) {
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)d * ldN);
        float* dst = S + (size_t)d * ldS;
        if (m4 & 0x1u) dst[r[0]] = v.x;
        if (m4 & 0x100u) dst[r[1]] = v.y;
        if (m4 & 0x10000u) dst[r[2]] = v.z;
        if (m4 & 0x1000000u) dst[r[3]] = v.w;
    }
}

// 3. The results of a search on the selection, in place: idx[t] = base + map[idx[t]] for t < n (a selection index >= npass cannot
//    come out of an engine; it is left as it is).
__global__ __launch_bounds__(256) void select_remap_kernel(uint64_t* __restrict__ idx, size_t n, const uint32_t* __restrict__ map,
                                                           uint32_t npass, uint64_t base) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const uint64_t j = idx[t];
    if (j < npass) idx[t] = base + map[j];
}

}  // namespace innr
