// kernels_ext.h -- the remaining L2 helpers of src/batch.rs: per-dimension variance (:572-592) and the
// order-preserving survivor compaction behind batch_l2_squared_pruning (:320-365).
#pragma once

#include "common.h"

namespace innr {

// batch_dimension_variance (batch.rs:572-592): per dimension d, SEQUENTIALLY over i = 0..N-1 (the order is part
// of the result): mean = sum(x)/n, var = sum((x-mean)*(x-mean))/n, both sums folded from -0.0 like
// <f32 as Sum>::sum. One lane per dimension: a serial dependency chain is what the reference computes, so the
// only parallelism is across dimensions; float4 loads keep each lane on its own cache lines. One-time per batch.
__global__ __launch_bounds__(64) void dimension_variance_kernel(const float* __restrict__ V, size_t ldN, uint32_t N,
                                                                uint32_t D, float* __restrict__ var) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const float* row = V + (size_t)d * ldN;
    if (N <= 1) {  // batch.rs:573-575
        var[d] = 0.0f;
        return;
    }
    const float nf = (float)N;
    float s = -0.0f;
    const uint32_t n4 = N / 4;
    const float4* r4 = reinterpret_cast<const float4*>(row);
#pragma unroll 4
    for (uint32_t i = 0; i < n4; ++i) {
        const float4 v = r4[i];
        s = ex::add(ex::add(ex::add(ex::add(s, v.x), v.y), v.z), v.w);
    }
    for (uint32_t i = n4 * 4; i < N; ++i) s = ex::add(s, row[i]);
    const float mean = ex::div(s, nf);
    float acc = -0.0f;
#pragma unroll 4
    for (uint32_t i = 0; i < n4; ++i) {
        const float4 v = r4[i];
        // (sub_keepnan: a NaN mean -- a column that holds a NaN -- keeps its sign, like the reference's x - mean on the host ISAs;
        // variance_order sorts by total_cmp, which puts +NaN first and -NaN last)
        const float a = ex::sub_keepnan(v.x, mean), b = ex::sub_keepnan(v.y, mean), c = ex::sub_keepnan(v.z, mean),
                    e = ex::sub_keepnan(v.w, mean);
        acc = ex::mad2(ex::mad2(ex::mad2(ex::mad2(acc, a, a), b, b), c, c), e, e);
    }
    for (uint32_t i = n4 * 4; i < N; ++i) {
        const float a = ex::sub_keepnan(row[i], mean);
        acc = ex::mad2(acc, a, a);
    }
    var[d] = ex::div(acc, nf);
}

// batch_l2_squared_pruning survivors (batch.rs:339-364): a vector is dropped the first time its partial sum
// exceeds `threshold`; partial sums of squares are monotone (also in f32), so the survivors are exactly the
// vectors whose FULL distance is not > threshold (NaN survives: `dist > threshold` is false), reported in index
// order with their full distance. Pass 1 counts per 256-vector chunk, pass 2 (after an exclusive scan of the
// counts) scatters in order.
__global__ __launch_bounds__(256) void prune_count_kernel(const float* __restrict__ dist, uint32_t N, float threshold,
                                                          uint32_t* __restrict__ chunk_count) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = (i < N) && !(dist[i] > threshold);
    const unsigned long long m = __ballot(keep);
    __shared__ uint32_t wc[4];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// single-workgroup exclusive scan of `n` counts (n <= a few 100k): offsets[i] = sum(counts[0..i)), total -> *total
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(const uint32_t* __restrict__ counts, uint32_t n,
                                                               uint32_t* __restrict__ offsets,
                                                               uint32_t* __restrict__ total) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t b = threadIdx.x * per, e = (b + per < n) ? b + per : n;
    uint32_t s = 0;
    for (uint32_t i = b; i < e; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the partials
        uint32_t v = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = (threadIdx.x == 0) ? 0 : part[threadIdx.x - 1];
    for (uint32_t i = b; i < e; ++i) {
        offsets[i] = run;
        run += counts[i];
    }
    if (threadIdx.x == 1023) *total = part[1023];
}

__global__ __launch_bounds__(256) void prune_scatter_kernel(const float* __restrict__ dist, uint32_t N, float threshold,
                                                            const uint32_t* __restrict__ chunk_offset, uint64_t index_base,
                                                            uint64_t* __restrict__ out_idx, float* __restrict__ out_dist,
                                                            uint32_t cap) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const float dv = (i < N) ? dist[i] : 0.0f;
    const bool keep = (i < N) && !(dv > threshold);
    const unsigned long long m = __ballot(keep);
    __shared__ uint32_t wc[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wc[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t base = chunk_offset[blockIdx.x];
    for (int j = 0; j < w; ++j) base += wc[j];
    if (keep) {
        const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (pos < cap) {
            out_idx[pos] = index_base + i;
            out_dist[pos] = dv;
        }
    }
}

// ---- range search (innr_batch_range_search): the scans, and the finish of the queries a collect pass served -----------------
// Per query (one workgroup each), in place: cnt[q][0..n) survivors per chunk -> their exclusive prefix, cnt[q][n] = tot[q] = the
// query's total. 32-bit: a query has at most N < 2^32 survivors.
__global__ __launch_bounds__(1024) void range_chunk_scan_kernel(uint32_t* __restrict__ cnt, size_t ldc, uint32_t n,
                                                                 uint32_t* __restrict__ tot) {
    __shared__ uint32_t part[1024];
    uint32_t* row = cnt + (size_t)blockIdx.x * ldc;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t b = threadIdx.x * per < n ? threadIdx.x * per : n, e = (b + per < n) ? b + per : n;
    uint32_t s = 0;
    for (uint32_t i = b; i < e; ++i) s += row[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan of the partials
        const uint32_t v = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = (threadIdx.x == 0) ? 0 : part[threadIdx.x - 1];
    for (uint32_t i = b; i < e; ++i) {
        const uint32_t c = row[i];
        row[i] = run;
        run += c;
    }
    if (threadIdx.x == 1023) {
        row[n] = part[1023];
        tot[blockIdx.x] = part[1023];
    }
}

// The 64-bit scan over the totals of one chunk of nq <= 4096 queries (single workgroup): off[0] is the running base the chunk
// before left (the first chunk's: 0), off[j + 1] = off[0] + tot[0] + ... + tot[j], so off[nq] carries the base on.
__global__ __launch_bounds__(1024) void range_offsets_kernel(const uint32_t* __restrict__ tot, uint32_t nq, uint64_t* __restrict__ off) {
    __shared__ uint64_t part[1024];
    const uint32_t per = (nq + 1023) / 1024;
    const uint32_t b = threadIdx.x * per < nq ? threadIdx.x * per : nq, e = (b + per < nq) ? b + per : nq;
    uint64_t s = 0;
    for (uint32_t i = b; i < e; ++i) s += tot[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t v = (threadIdx.x >= o) ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = off[0] + ((threadIdx.x == 0) ? 0 : part[threadIdx.x - 1]);
    for (uint32_t i = b; i < e; ++i) {
        run += tot[i];
        off[i + 1] = run;
    }
}

// A collect pass (MODE 2 of the GEMM filter, thresholds from seed_thresholds_kernel) left query q's candidates in its list and
// their exact composites in keys[q][0..ccnt[q]). The list holds every survivor only if it did not overflow and the filter's error
// bound held for the query: bad[q] = 1 otherwise (list past `cap`; no finite collect threshold, seed[q] == 0; a query norm outside
// {0} + [1e-12, 1e18], where the approximate scores may overflow or lose products to flushing) and the exact scan finishes it.
// For the others the exact predicate marks each survivor in the query's bitmap over the corpus (bit i % 32 of word i / 32) and
// counts it in its CHUNK-vector chunk. A corpus index occurs once per list, and OR / ADD do not depend on the order of arrival.
// CHUNK: the vectors per count of the exact scan that shares cnt (256: range_scan_kernel, 1024: range_scan_u8_kernel).
// QNORM = false (a code corpus on the int8 filter): no norm window -- a constant that overflows already makes the query's bound
// non-finite, hence its seed 0 -- and qnorm is not read; a query without a finite collect threshold was closed before the launch
// (seed[q] = 0xFFFFFFFF, range_close_unbounded_kernel) and is bad like one whose seed is still 0.
template <bool L2, int CHUNK = 256, bool QNORM = true>
__global__ __launch_bounds__(256) void range_mark_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ccnt, uint32_t cap,
                                                          const float* __restrict__ thr, const uint32_t* __restrict__ seed,
                                                          const float* __restrict__ qnorm, uint32_t* __restrict__ bitmap, size_t ldb,
                                                          uint32_t* __restrict__ cnt, size_t ldc, uint32_t* __restrict__ bad) {
    static_assert(CHUNK == 256 || CHUNK == 1024, "the chunk of the f32 scans or of the u8 scans");
    constexpr int SH = CHUNK == 256 ? 8 : 10;
    const uint32_t q = blockIdx.y;
    const uint32_t n = ccnt[q];
    bool fb;
    if constexpr (QNORM) {
        const float qn = qnorm[q];
        fb = n > cap || seed[q] == 0u || !(qn == 0.0f || (qn >= 1e-12f && qn <= 1e18f));
    } else {
        fb = n > cap || seed[q] == 0u || seed[q] == 0xFFFFFFFFu;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) bad[q] = fb ? 1u : 0u;
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (fb || slot >= n) return;
    const uint64_t key = keys[(size_t)q * cap + slot];
    const float s = pref_score(cand_pref(key), L2), t = thr[q];
    if (L2 ? (s > t) : (s < t)) return;
    const uint32_t i = cand_idx(key), bit = 1u << (i & 31);
    const uint32_t old = atomicOr(bitmap + (size_t)q * ldb + (i >> 5), bit);
    if (!(old & bit)) atomicAdd(cnt + (size_t)q * ldc + (i >> SH), 1u);
}

// The collect thresholds of a code corpus (seed_thresholds_u8_kernel) before the launch: a query without a finite one (seed 0: a
// NaN or infinite threshold, a NaN / inf query, an unusable query scale) would collect the whole corpus through the survivors'
// path only to be discarded. It is closed the way padding queries are -- the largest key, nothing is ever admitted -- and
// range_mark_kernel<.., false> hands it to the exact scan.
__global__ void range_close_unbounded_kernel(uint32_t* __restrict__ seed, uint32_t nq) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nq && seed[j] == 0u) seed[j] = 0xFFFFFFFFu;
}

// ... and after the scans each marked candidate goes to its place in index order: the query's offset, its chunk's prefix, the
// marked vectors of the chunk below it (popcounts of the bitmap). Only positions < outcap are written.
template <int CHUNK = 256>
__global__ __launch_bounds__(256) void range_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ccnt, uint32_t cap,
                                                             bool l2, const uint32_t* __restrict__ bitmap, size_t ldb,
                                                             const uint32_t* __restrict__ pref, size_t ldc, const uint32_t* __restrict__ bad,
                                                             const uint64_t* __restrict__ qoff, uint64_t index_base,
                                                             uint64_t* __restrict__ out_idx, float* __restrict__ out_score, uint64_t outcap) {
    static_assert(CHUNK == 256 || CHUNK == 1024, "the chunk of the f32 scans or of the u8 scans");
    constexpr int SH = CHUNK == 256 ? 8 : 10;
    constexpr uint32_t W = CHUNK / 32;  // bitmap words per chunk
    const uint32_t q = blockIdx.y;
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (bad[q] || slot >= ccnt[q]) return;
    const uint64_t key = keys[(size_t)q * cap + slot];
    const uint32_t i = cand_idx(key), bit = 1u << (i & 31);
    const uint32_t* words = bitmap + (size_t)q * ldb + ((i >> SH) * W);  // the chunk's words
    const uint32_t w = (i >> 5) & (W - 1);
    if (!(words[w] & bit)) return;
    uint32_t rank = (uint32_t)__popc(words[w] & (bit - 1u));
    for (uint32_t u = 0; u < w; ++u) rank += (uint32_t)__popc(words[u]);
    const uint64_t pos = qoff[q] + pref[(size_t)q * ldc + (i >> SH)] + rank;
    if (pos < outcap) {
        out_idx[pos] = index_base + i;
        out_score[pos] = pref_score(cand_pref(key), l2);
    }
}

}  // namespace innr
