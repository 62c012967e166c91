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

// 2b. The gather of a u8 code batch (innr_batch_knn_u8_filtered): S[d * ldS + rank(i)] = C8[d * ldN + i], map[rank(i)] = i, with the
//    chunks, counts and offsets of the f32 gather (a code batch's ldN is a multiple of 1024, hence of kSelChunk): a lane owns one
//    dword of 4 codes per row and loads it only if one of them passes; a chunk with no passing vector returns before any load.
//    The survivors of a chunk are one contiguous run [chunk_off, chunk_off + total) of every destination row.
//    The wave compacts kSelU8Rows rows' passing bytes in LDS at the run's own alignment (lo = chunk_off % 4: both row strides are
//    multiples of 4, so every row of S has it) and writes the run as whole dwords; only the dwords at the two ragged ends, which
//    the neighbouring chunks' runs share, go out byte by byte (never a byte outside the run). One byte store per passing code
//    instead -- the f32 gather's form -- was measured and lost at every selectivity.
//    Grid: as select_gather_kernel.
// rows per LDS round: that many loads in flight per lane (the gather is bound by the latency of its rounds, not by bandwidth:
// DESIGN.md 4.5e has 4 against 16 rows); 16 rows are 16.5 KiB of LDS a block
constexpr int kSelU8Rows = 16;
constexpr int kSelU8Stage = (kSelChunk + 4 + 4) / 4;  // dwords per staged row: 3 + 256 bytes at most, rounded up (66)

__global__ __launch_bounds__(256) void select_gather_u8_kernel(const uint8_t* __restrict__ C8, size_t ldN, uint32_t D,
                                                               const uint8_t* __restrict__ nm, const uint32_t* __restrict__ chunk_off,
                                                               size_t nchunks, uint8_t* __restrict__ S, size_t ldS,
                                                               uint32_t* __restrict__ map, uint32_t slab) {
    __shared__ uint32_t stage[4][kSelU8Rows][kSelU8Stage];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t ch = (size_t)blockIdx.x * 4 + w;
    if (ch >= nchunks) return;  // wave-uniform
    const size_t col = ch * kSelChunk + (size_t)lane * 4;
    const uint32_t m4 = *reinterpret_cast<const uint32_t*>(nm + col);
    uint32_t total;
    const uint32_t below = sel_pass_below(m4, lane, &total);
    if (total == 0) return;  // wave-uniform
    const uint32_t base = chunk_off[ch];
    uint32_t r[4];  // rank within the chunk
    {
        uint32_t r_ = below;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = r_;
            r_ += (m4 >> (8 * c)) & 1u;
        }
    }
    if (blockIdx.y == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((m4 >> (8 * c)) & 1u) map[base + r[c]] = (uint32_t)(col + c);
    }
    const uint32_t d0 = blockIdx.y * slab;
    const uint32_t d1 = (d0 < D && slab < D - d0) ? d0 + slab : D;
    const uint8_t* src = C8 + col;
    const uint32_t lo = base & 3u, hi = lo + total;  // the run's bytes within its staged row: [lo, hi), hi <= 259
    const uint32_t ndw = (hi + 3) / 4;               // <= 65: lane 0 takes dword 64 as well
    uint8_t* S0 = S + (base - lo);                   // dword-aligned in every row
    for (uint32_t d = d0; d < d1; d += kSelU8Rows) {
        uint32_t v[kSelU8Rows];
#pragma unroll
        for (int u = 0; u < kSelU8Rows; ++u) {
            v[u] = 0;
            if (m4 && d + u < d1) v[u] = *reinterpret_cast<const uint32_t*>(src + (size_t)(d + u) * ldN);
        }
#pragma unroll
        for (int u = 0; u < kSelU8Rows; ++u) {
            uint8_t* st = reinterpret_cast<uint8_t*>(stage[w][u]) + lo;
            if (m4 & 0x1u) st[r[0]] = (uint8_t)v[u];
            if (m4 & 0x100u) st[r[1]] = (uint8_t)(v[u] >> 8);
            if (m4 & 0x10000u) st[r[2]] = (uint8_t)(v[u] >> 16);
            if (m4 & 0x1000000u) st[r[3]] = (uint8_t)(v[u] >> 24);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < kSelU8Rows; ++u) {
            if (d + u >= d1) break;
            uint8_t* row = S0 + (size_t)(d + u) * ldS;
            for (uint32_t j = (uint32_t)lane; j < ndw; j += 64) {
                const uint32_t word = stage[w][u][j];
                const uint32_t b0 = 4 * j;
                if (b0 >= lo && b0 + 4 <= hi) {
                    *reinterpret_cast<uint32_t*>(row + b0) = word;
                } else {
#pragma unroll
                    for (uint32_t c = 0; c < 4; ++c)
                        if (b0 + c >= lo && b0 + c < hi) row[b0 + c] = (uint8_t)(word >> (8 * c));
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the next round overwrites the staged rows
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
