// kernels_adaptive.h -- batch_knn_adaptive (src/batch.rs:441-564) on the device: the kernels between the warm-up scan and the
// final sort. The reference is one sequential loop over (dimension, vector); DESIGN.md 4.5d restates it as phases a GPU can run
// and adaptive.hip drives them:
//   warm-up distances (the exact engine's scan over the first W rows)  ->  threshold (radix select, sort_full.hip)
//   -> flag and compact (step 4)  ->  per segment of <= 32 dimensions: accumulate + death dimension + histogram, the ordered cut,
//   compact  ->  once exactly k vectors live: finish  ->  sort the survivors.
// Every compaction keeps list order = index order: per-chunk counts, an exclusive scan of them (exclusive_scan_kernel, launched
// from api.hip) and a scatter to "own position minus the killed before me". No workgroup waits on another: what one phase decides
// reaches the next through AdaptiveState in device memory. Every index gathered with comes from this call's own compaction (< N),
// every loop is bounded by a dimension count or the list length.
#pragma once

#include "common.h"

namespace innr {

constexpr uint32_t kAdpBins = 33;      // death dimensions of one segment (a segment has at most 32; one bin to spare)
constexpr uint32_t kAdpNoDeath = 255;  // death[] of a vector that never exceeded the threshold in the segment
constexpr int kAdpChunk = 256;         // list entries per workgroup = per count of the compactions

struct AdaptiveState {
    float thr;         // the pruning threshold of the current phase
    uint32_t cutdim;   // ordered cut: vectors that died before this dimension of the segment are killed ...
    uint32_t cutrank;  // ... and the first `cutrank` (in list order) of those that died in it
    uint32_t killed;   // vectors the cut kills
    uint32_t total[2]; // totals of the compactions' scans ([0]: flagged vectors of step 4)
    uint32_t pad[2];
    uint32_t hist[kAdpBins];  // deaths per dimension of the segment
};

// thr = the k-th best distance of a sort's output (composites, best first; sort_full.hip), times `scale` (1.0f: exact, no rounding)
__global__ void adaptive_threshold_kernel(const uint64_t* __restrict__ sorted, size_t k, float scale, AdaptiveState* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) st->thr = ex::mul(pref_score(cand_pref(sorted[k - 1]), true), scale);
}

// step 4's predicate: fl(dist * scale) > fl(thr * 1.5f); false for a NaN on either side
__device__ __forceinline__ bool adaptive_flagged(float dist, float scale, float thr) {
    return ex::mul(dist, scale) > ex::mul(thr, 1.5f);
}

// wave ballot of `p` -> this thread's count of set lanes before it in its workgroup of 256 (sh: 4 words of LDS) and the
// workgroup's total. Every thread of the workgroup must call it.
__device__ __forceinline__ uint32_t adaptive_block_rank(bool p, uint32_t* sh, uint32_t* block_total) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(p);
    if (lane == 0) sh[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < w; ++j) before += sh[j];
    *block_total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();  // sh may be reused
    return before;
}

// step 4, pass 1: flagged vectors per chunk of 256
__global__ __launch_bounds__(kAdpChunk) void adaptive_flag_count_kernel(const float* __restrict__ dist, uint32_t N, float scale,
                                                                        const AdaptiveState* __restrict__ st,
                                                                        uint32_t* __restrict__ chunk_count) {
    __shared__ uint32_t sh[4];
    const uint32_t i = blockIdx.x * kAdpChunk + threadIdx.x;
    const bool f = i < N && adaptive_flagged(dist[i], scale, st->thr);
    uint32_t total;
    (void)adaptive_block_rank(f, sh, &total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// step 4, pass 2: the first `cap` flagged vectors in index order are killed; vector i, if it lives, goes to list position
// i - (killed before it) = i - min(flagged before it, cap).
__global__ __launch_bounds__(kAdpChunk) void adaptive_flag_scatter_kernel(const float* __restrict__ dist, uint32_t N, float scale,
                                                                          const AdaptiveState* __restrict__ st,
                                                                          const uint32_t* __restrict__ chunk_off, uint32_t cap,
                                                                          uint32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                                          uint32_t out_n) {
    __shared__ uint32_t sh[4];
    const uint32_t i = blockIdx.x * kAdpChunk + threadIdx.x;
    const float dv = i < N ? dist[i] : 0.0f;
    const bool f = i < N && adaptive_flagged(dv, scale, st->thr);
    uint32_t total;
    const uint32_t before = chunk_off[blockIdx.x] + adaptive_block_rank(f, sh, &total);
    if (i >= N || (f && before < cap)) return;
    const uint32_t pos = i - (before < cap ? before : cap);
    if (pos < out_n) {
        out_idx[pos] = i;
        out_dist[pos] = dv;
    }
}

// One dimension of one live vector: dist = fl(dist + fl(diff * diff)), diff = fl(q - v) -- scan_dim's arithmetic (kernels_scan.h)
__device__ __forceinline__ float adaptive_step(float acc, float q, float v) {
    const float diff = ex::sub_keepnan(q, v);
    return ex::mad2(acc, diff, diff);
}

// The corpus column of a list entry. The list is this call's own compaction, so the entry is below N; the clamp only keeps a
// gather inside the corpus should that ever not hold.
__device__ __forceinline__ uint32_t adaptive_column(uint32_t i, uint32_t N) { return i < N ? i : N - 1; }

// A segment [s0, s1] (<= 32 dimensions, constant threshold) while more than k vectors live: one lane per live vector gathers
// V[d * ldN + idx], accumulates in dimension order, records the first dimension after which its distance exceeded the threshold
// (death[j] = d - s0, kAdpNoDeath if none; a NaN distance or threshold never compares greater) and counts it in the histogram.
// The loads of a lane hit a different cache line per dimension (64 B fetched per 4 B used): groups of 8 are issued together.
__global__ __launch_bounds__(kAdpChunk) void adaptive_segment_kernel(const float* __restrict__ V, size_t ldN,
                                                                     const float* __restrict__ q, uint32_t s0, uint32_t s1,
                                                                     const uint32_t* __restrict__ idx, float* __restrict__ dist,
                                                                     uint32_t n, uint32_t N, AdaptiveState* st,
                                                                     uint8_t* __restrict__ death) {
    __shared__ uint32_t h[kAdpBins];
    if (threadIdx.x < kAdpBins) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t j = blockIdx.x * kAdpChunk + threadIdx.x;
    if (j < n) {
        const float thr = st->thr;
        const float* p = V + adaptive_column(idx[j], N);
        float acc = dist[j];
        uint32_t dd = kAdpNoDeath;
        uint32_t d = s0;
#pragma unroll 1
        for (; d + 8 <= s1 + 1; d += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(d + u) * ldN];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc = adaptive_step(acc, q[d + u], v[u]);
                if (dd == kAdpNoDeath && acc > thr) dd = d + u - s0;
            }
        }
        for (; d <= s1; ++d) {
            acc = adaptive_step(acc, q[d], p[(size_t)d * ldN]);
            if (dd == kAdpNoDeath && acc > thr) dd = d - s0;
        }
        dist[j] = acc;
        death[j] = (uint8_t)dd;
        if (dd < kAdpBins) atomicAdd(&h[dd], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kAdpBins && h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// The ordered cut: deaths are applied in (dimension, list position) order until `need` = |L| - k vectors are gone. The dimension
// where the cumulative histogram reaches `need` is cut at a rank; with fewer deaths than `need` all of them are applied.
__global__ void adaptive_cut_kernel(AdaptiveState* st, uint32_t need) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t cum = 0, cutdim = kAdpBins, cutrank = 0, killed = 0;
    for (uint32_t b = 0; b < kAdpBins; ++b) {
        const uint32_t c = st->hist[b];
        if (cum + c >= need) {
            cutdim = b;
            cutrank = need - cum;
            killed = need;
            break;
        }
        cum += c;
        killed = cum;
    }
    st->cutdim = cutdim;
    st->cutrank = cutrank;
    st->killed = killed;
}

// the cut's compaction, pass 1: per chunk, the vectors that died before the cut dimension and those that died in it
__global__ __launch_bounds__(kAdpChunk) void adaptive_cut_count_kernel(const uint8_t* __restrict__ death, uint32_t n,
                                                                       const AdaptiveState* __restrict__ st,
                                                                       uint32_t* __restrict__ cnt_lt, uint32_t* __restrict__ cnt_eq) {
    __shared__ uint32_t sh[4];
    const uint32_t j = blockIdx.x * kAdpChunk + threadIdx.x;
    const uint32_t dd = j < n ? death[j] : kAdpNoDeath, cutdim = st->cutdim;
    uint32_t lt, eq;
    (void)adaptive_block_rank(dd < cutdim, sh, &lt);
    (void)adaptive_block_rank(dd == cutdim, sh, &eq);
    if (threadIdx.x == 0) {
        cnt_lt[blockIdx.x] = lt;
        cnt_eq[blockIdx.x] = eq;
    }
}

// ... pass 2: entry j is killed if it died before the cut dimension, or in it among the first cutrank; a survivor moves to
// j - (killed before it), with its full segment distance
__global__ __launch_bounds__(kAdpChunk) void adaptive_cut_scatter_kernel(const uint8_t* __restrict__ death,
                                                                         const uint32_t* __restrict__ idx,
                                                                         const float* __restrict__ dist, uint32_t n,
                                                                         const AdaptiveState* __restrict__ st,
                                                                         const uint32_t* __restrict__ off_lt,
                                                                         const uint32_t* __restrict__ off_eq,
                                                                         uint32_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                                         uint32_t out_n) {
    __shared__ uint32_t sh[4];
    const uint32_t j = blockIdx.x * kAdpChunk + threadIdx.x;
    const uint32_t dd = j < n ? death[j] : kAdpNoDeath, cutdim = st->cutdim, cutrank = st->cutrank;
    uint32_t t;
    const uint32_t lt_before = off_lt[blockIdx.x] + adaptive_block_rank(dd < cutdim, sh, &t);
    const uint32_t eq_before = off_eq[blockIdx.x] + adaptive_block_rank(dd == cutdim, sh, &t);
    if (j >= n || dd < cutdim || (dd == cutdim && eq_before < cutrank)) return;
    const uint32_t pos = j - (lt_before + (eq_before < cutrank ? eq_before : cutrank));
    if (pos < out_n) {
        out_idx[pos] = idx[j];
        out_dist[pos] = dist[j];
    }
}

// Exactly k vectors live: nothing is pruned any more (the reference's guard alive_count > k), the dimensions [d0, D) only
// accumulate. One lane per vector; the order of the additions is the reference's, the loads go out eight at a time.
__global__ __launch_bounds__(kAdpChunk) void adaptive_finish_kernel(const float* __restrict__ V, size_t ldN, const float* __restrict__ q,
                                                                    uint32_t d0, uint32_t D, const uint32_t* __restrict__ idx,
                                                                    float* __restrict__ dist, uint32_t n, uint32_t N) {
    const uint32_t j = blockIdx.x * kAdpChunk + threadIdx.x;
    if (j >= n) return;
    const float* p = V + adaptive_column(idx[j], N);
    float acc = dist[j];
    uint32_t d = d0;
#pragma unroll 1
    for (; d + 8 <= D; d += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(d + u) * ldN];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = adaptive_step(acc, q[d + u], v[u]);
    }
    for (; d < D; ++d) acc = adaptive_step(acc, q[d], p[(size_t)d * ldN]);
    dist[j] = acc;
}

// The sorted survivors (composites [~ord(dist) | ~list position], best first: list order is index order, so this is the
// reference's stable sort) -> the caller's indices and the distances' own bits.
__global__ __launch_bounds__(256) void adaptive_emit_kernel(const uint64_t* __restrict__ sorted, uint32_t k,
                                                            const uint32_t* __restrict__ idx, uint32_t n, uint64_t index_base,
                                                            uint64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= k) return;
    const uint64_t key = sorted[r];
    const uint32_t pos = cand_idx(key);
    out_idx[r] = index_base + (pos < n ? idx[pos] : 0u);
    out_score[r] = pref_score(cand_pref(key), true);
}

// D == 0 (batch.rs:458-463): indices 0 .. k-1, scores 0.0
__global__ __launch_bounds__(256) void adaptive_iota_kernel(size_t total, size_t k, uint64_t index_base, uint64_t* __restrict__ out_idx,
                                                            float* __restrict__ out_score) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    out_idx[t] = index_base + t % k;
    out_score[t] = 0.0f;
}

}  // namespace innr
