// kernels_scan.h -- the bit-exact scan: batch_dot_into / batch_l2_squared_into / batch_cosine_into
// (src/batch.rs:284-297, 250-266, 705-728) for up to QB queries per corpus pass.
//
// HBM-bound design (roofline: 4*N*D bytes per pass): one lane owns 4 consecutive corpus
// vectors and keeps their QB accumulators in registers; a wave reads each dimension row as one coalesced
// 1 KiB float4 access (the PDX layout makes lane i's element of row d contiguous with lane i+1's).
// Each lane walks d = 0..D-1 in the reference's order with fl(acc + fl(q*v)) (ex::mad2), so outputs are
// bit-identical to the Rust loops -- which also means the reference's N-long accumulator array that is
// re-streamed D times on the CPU (8*N*D bytes of extra traffic) never exists here.
#pragma once

#include "common.h"
#include "topk_dev.h"

namespace innr {

constexpr int kScanThreads = 256;          // 4 waves
constexpr int kScanChunk = 64 * 4;         // vectors per wave step (64 lanes x float4)

// one dimension d of 4 vectors against QB queries
template <int QB, bool L2>
__device__ __forceinline__ void scan_dim(float (&acc)[QB][4], const float4& v, const float* __restrict__ Qm, size_t ldq, uint32_t d) {
#pragma unroll
    for (int j = 0; j < QB; ++j) {
        const float q = Qm[(size_t)j * ldq + d];  // wave-uniform -> scalar load
        if (L2) {  // batch.rs:262-263: diff = q_d - v_d; dist += diff*diff
            const float d0 = ex::sub_keepnan(q, v.x), d1 = ex::sub_keepnan(q, v.y), d2 = ex::sub_keepnan(q, v.z),
                        d3 = ex::sub_keepnan(q, v.w);
            acc[j][0] = ex::mad2(acc[j][0], d0, d0);
            acc[j][1] = ex::mad2(acc[j][1], d1, d1);
            acc[j][2] = ex::mad2(acc[j][2], d2, d2);
            acc[j][3] = ex::mad2(acc[j][3], d3, d3);
        } else {  // batch.rs:294: prod += q_d * v_d
            acc[j][0] = ex::mad2(acc[j][0], q, v.x);
            acc[j][1] = ex::mad2(acc[j][1], q, v.y);
            acc[j][2] = ex::mad2(acc[j][2], q, v.z);
            acc[j][3] = ex::mad2(acc[j][3], q, v.w);
        }
    }
}

// acc[j][c] for QB queries x 4 vectors starting at column `col` (col % 4 == 0, col + 3 < ldN).
// ORD: walk the dimensions in the order given by `order[0..D)` (batch_knn_reordered, batch.rs:640-648).
// Groups of kScanGroup dimensions, ALL their loads issued at the top of the iteration and awaited one by one: left to the
// scheduler (a plain 8-fold unroll), the 4- and 8-query instantiations came out as load -> vmcnt(0) -> multiply, one
// dimension after the other, each round trip covered only by the other waves of the SIMD (kernels_u8.h has the same shape
// and the measurements behind it).
constexpr int kScanGroup = 8;
template <int QB, bool L2, bool ORD = false>
__device__ __forceinline__ void scan_accumulate(const float* __restrict__ V, size_t ldN, uint32_t D, size_t col,
                                                const float* __restrict__ Qm, size_t ldq, float (&acc)[QB][4],
                                                const uint32_t* __restrict__ order = nullptr) {
#pragma unroll
    for (int j = 0; j < QB; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
    const float4* p = reinterpret_cast<const float4*>(V + col);
    const size_t stride = ldN / 4;
    constexpr int U = kScanGroup;
    uint32_t t = 0;
#pragma unroll 1
    for (; t + U <= D; t += U) {
        float4 v[U];
        uint32_t dd[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            dd[u] = (ORD && order) ? order[t + u] : t + u;
            v[u] = p[(size_t)dd[u] * stride];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) scan_dim<QB, L2>(acc, v[u], Qm, ldq, dd[u]);
    }
    for (; t < D; ++t) {
        const uint32_t d = (ORD && order) ? order[t] : t;
        const float4 v = p[(size_t)d * stride];
        scan_dim<QB, L2>(acc, v, Qm, ldq, d);
    }
}

// batch.rs:716-727 epilogue for one value: whole output 0 if ||q|| < eps; 0 if ||v|| <= eps
__device__ __forceinline__ float cosine_epilogue(float dot, float qn, float vn) {
    if (qn < INNR_NORM_EPSILON) return 0.0f;
    return (vn > INNR_NORM_EPSILON) ? ex::div(dot, ex::mul(qn, vn)) : 0.0f;
}

// ---- materialising variant: out[j*ldo + i] for all i (innr_batch_scores) -----------------------------
// ORD: dimensions walked in `order` (batch_knn_reordered beyond the candidate lists: all scores, then a full sort)
template <int QB, bool L2, bool COS, bool ORD = false>
__global__ __launch_bounds__(kScanThreads) void scan_scores_kernel(const float* __restrict__ V, size_t ldN,
                                                                    uint32_t D, const float* __restrict__ Qm,
                                                                    size_t ldq, const float* __restrict__ norms,
                                                                    const float* __restrict__ qnorm,
                                                                    float* __restrict__ out, size_t ldo,
                                                                    const uint32_t* __restrict__ order = nullptr) {
    const size_t nchunks = ldN / kScanChunk;
    const size_t wave = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * kScanThreads) >> 6;
    const int lane = threadIdx.x & 63;
    for (size_t ch = wave; ch < nchunks; ch += nwaves) {
        const size_t col = ch * kScanChunk + (size_t)lane * 4;
        float acc[QB][4];
        scan_accumulate<QB, L2, ORD>(V, ldN, D, col, Qm, ldq, acc, order);
        float4 vn = make_float4(0, 0, 0, 0);
        if (COS) vn = *reinterpret_cast<const float4*>(norms + col);
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            float4 o = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
            if (COS) {
                const float qn = qnorm[j];
                o.x = cosine_epilogue(o.x, qn, vn.x);
                o.y = cosine_epilogue(o.y, qn, vn.y);
                o.z = cosine_epilogue(o.z, qn, vn.z);
                o.w = cosine_epilogue(o.w, qn, vn.w);
            }
            *reinterpret_cast<float4*>(out + (size_t)j * ldo + col) = o;
        }
    }
}

// ---- fused top-k variant: exact scores -> threshold filter -> per-wave candidate lists ---------------
// Wave `slot` owns chunks [slot*cps, (slot+1)*cps) and lists[slot][0..QB). See topk_dev.h.
// R = list capacity / 64 (compile-time so only ONE compaction width is instantiated per kernel: the dynamic
// dispatch cost 150-196 VGPRs and capped the scan at 2-3 waves/SIMD, far too few to cover HBM latency).
// EXT: the L2 variants of the reference -- `mask` (batch_knn_filtered's predicate evaluated per index,
// batch.rs:839: only passing vectors are scored/admitted) and `order` (batch_knn_reordered's dimension order).
template <int QB, bool L2, bool COS, int R, bool EXT = false>
__global__ __launch_bounds__(kScanThreads) void scan_filter_kernel(
    const float* __restrict__ V, size_t ldN, uint32_t N, uint32_t D, const float* __restrict__ Qm, size_t ldq,
    const float* __restrict__ norms, const float* __restrict__ qnorm, uint64_t* __restrict__ lists,
    uint32_t* __restrict__ counts, uint32_t qstride, uint32_t KP, uint32_t chunks_per_slot,
    uint32_t* __restrict__ errflag, const uint8_t* __restrict__ mask = nullptr,
    const uint32_t* __restrict__ order = nullptr, uint32_t nvalid = 0xFFFFFFFFu) {
    constexpr uint32_t cap = 64 * R;
    __shared__ uint32_t s_cnt[kScanThreads / 64][QB];
    __shared__ uint32_t s_thr[kScanThreads / 64][QB];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t slot = (size_t)blockIdx.x * (kScanThreads / 64) + w;
    if (lane < QB) {
        s_cnt[w][lane] = 0;
        s_thr[w][lane] = 0;  // pref 0 = no threshold: everything is admitted
    }
    __builtin_amdgcn_wave_barrier();
    // blockIdx.y = query group: QB consecutive queries each; lists/counts are indexed [slot][query of the launch]
    // (qstride = queries in the launch). Small corpora put all their query groups into one launch.
    const uint32_t qoff = blockIdx.y * QB;
    Qm += (size_t)qoff * ldq;
    if (COS) qnorm += qoff;
    const size_t nchunks = ldN / kScanChunk;
    size_t ch0 = slot * chunks_per_slot, ch1 = ch0 + chunks_per_slot;
    if (ch1 > nchunks) ch1 = nchunks;
    uint64_t* my_lists = lists + (slot * (size_t)qstride + qoff) * cap;
    for (size_t ch = ch0; ch < ch1; ++ch) {
        const size_t col = ch * kScanChunk + (size_t)lane * 4;
        float acc[QB][4];
        scan_accumulate<QB, L2, EXT>(V, ldN, D, col, Qm, ldq, acc, order);
        uint32_t pass4 = 0x01010101u;  // per-vector predicate bytes (EXT: from the caller's mask)
        if (EXT && mask) pass4 = (col + 3 < N) ? *reinterpret_cast<const uint32_t*>(mask + col)
                                               : ((col < N ? mask[col] : 0u) | ((col + 1 < N ? mask[col + 1] : 0u) << 8) |
                                                  ((col + 2 < N ? mask[col + 2] : 0u) << 16));
        float vn[4] = {0, 0, 0, 0};
        if (COS) {
            const float4 t = *reinterpret_cast<const float4*>(norms + col);
            vn[0] = t.x; vn[1] = t.y; vn[2] = t.z; vn[3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            const uint32_t thr = __hip_atomic_load(&s_thr[w][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            const float qn = COS ? qnorm[j] : 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const size_t i = col + c;
                float s = acc[j][c];
                if (COS) s = cosine_epilogue(s, qn, vn[c]);
                const uint32_t pref = score_pref<L2>(s);
                // qoff + j >= nvalid: a zero row padding a ragged query tail (knn_exact_range) -- its scores all tie, nothing is kept
                if (i < N && pref >= thr && ((pass4 >> (8 * c)) & 0xffu) && qoff + j < nvalid)
                    cand_append(my_lists + (size_t)j * cap, &s_cnt[w][j], cap, cand_make(pref, (uint32_t)i), errflag);
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1  // one copy of the compaction code, not QB inlined copies (register pressure)
        for (int j = 0; j < QB; ++j) {
            const uint32_t c = __builtin_amdgcn_readfirstlane(
                __hip_atomic_load(&s_cnt[w][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
            if (c > cap - kBurst) {  // wave-uniform (scalar branch)
                uint32_t t;
                const uint32_t keep = wave_compact<R>(my_lists + (size_t)j * cap, c, KP, &t);
                if (lane == 0) {
                    s_cnt[w][j] = keep;
                    s_thr[w][j] = t;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    // leave at most KP entries per list (bounds the select kernel's work), then publish the counts
#pragma unroll 1
    for (int j = 0; j < QB; ++j) {
        uint32_t c = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&s_cnt[w][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
        if (c > KP) {
            uint32_t t;
            c = wave_compact<R>(my_lists + (size_t)j * cap, c, KP, &t);
        }
        if (lane == 0) counts[slot * qstride + qoff + j] = c;
    }
}

// ---- range search: every vector within a per-query threshold, in index order (innr_batch_range_search) ---------------
// The predicate of batch_l2_squared_pruning (batch.rs:351) per query: squared L2 keeps !(dist > thr), dot / cosine keep
// !(score < thr), so a NaN score survives either way. Two launches of the same arithmetic around a scan of the counts:
//   EMIT = false: cnt[row][ch] = survivors of query `row` in the 256-vector chunk ch (every chunk is written);
//   EMIT = true : cnt holds each row's exclusive prefix over the chunks, the row's total at [nchunks]. A chunk where no query
//     of the group has a survivor is skipped before its corpus rows are read (wave-uniform test), the others are scored again
//     and survivor i lands at qoff[row] + cnt[row][ch] + (survivors of the chunk below i); only positions < cap are written.
// Query groups of QB on blockIdx.y. The last group of a ragged batch is moved back to end on the last query (nq >= QB): the
// queries it shares with the group before are scored twice and written by the earlier group only, so no row is read past nq.
// qmap: cnt / qoff row of local query q (null: q itself) -- the queries of a batch that the exact path finishes.
template <int QB, bool L2, bool COS, bool EMIT>
__global__ __launch_bounds__(kScanThreads) void range_scan_kernel(
    const float* __restrict__ V, size_t ldN, uint32_t N, uint32_t D, const float* __restrict__ Qm, size_t ldq,
    const float* __restrict__ norms, const float* __restrict__ qnorm, const float* __restrict__ thr,
    const uint32_t* __restrict__ qmap, uint32_t nq, uint32_t* __restrict__ cnt, size_t ldc,
    const uint64_t* __restrict__ qoff, uint64_t index_base, uint64_t* __restrict__ out_idx, float* __restrict__ out_score,
    uint64_t cap) {
    const uint32_t g0 = blockIdx.y * QB;                      // first query this group writes
    const uint32_t qb0 = g0 + QB <= nq ? g0 : nq - QB;        // first query it scores
    Qm += (size_t)qb0 * ldq;
    uint32_t row[QB];
#pragma unroll
    for (int j = 0; j < QB; ++j) row[j] = qmap ? qmap[qb0 + j] : qb0 + j;
    const size_t nchunks = ldN / kScanChunk;
    const size_t wave = ((size_t)blockIdx.x * kScanThreads + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * kScanThreads) >> 6;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (size_t ch = wave; ch < nchunks; ch += nwaves) {
        if (EMIT) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < QB; ++j)
                if (qb0 + j >= g0) any |= cnt[row[j] * ldc + ch + 1] != cnt[row[j] * ldc + ch];
            if (!any) continue;
        }
        const size_t col = ch * kScanChunk + (size_t)lane * 4;
        float acc[QB][4];
        scan_accumulate<QB, L2>(V, ldN, D, col, Qm, ldq, acc);
        float vn[4] = {0, 0, 0, 0};
        if (COS) {
            const float4 t = *reinterpret_cast<const float4*>(norms + col);
            vn[0] = t.x; vn[1] = t.y; vn[2] = t.z; vn[3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            if (qb0 + j < g0) continue;  // scored for the group before (wave-uniform)
            const float t = thr[qb0 + j];
            const float qn = COS ? qnorm[qb0 + j] : 0.0f;
            float s[4];
            bool keep[4];
            unsigned long long m[4];
            uint32_t total = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s[c] = COS ? cosine_epilogue(acc[j][c], qn, vn[c]) : acc[j][c];
                keep[c] = col + c < N && (L2 ? !(s[c] > t) : !(s[c] < t));
                m[c] = __ballot(keep[c]);
                total += (uint32_t)__popcll(m[c]);
            }
            if (!EMIT) {
                if (lane == 0) cnt[row[j] * ldc + ch] = total;
            } else if (total) {
                uint64_t pos = qoff[row[j]] + cnt[row[j] * ldc + ch];
#pragma unroll
                for (int c = 0; c < 4; ++c) pos += (uint32_t)__popcll(m[c] & below);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (keep[c]) {
                        if (pos < cap) {
                            out_idx[pos] = index_base + col + c;
                            out_score[pos] = s[c];
                        }
                        ++pos;
                    }
                }
            }
        }
    }
}

}  // namespace innr
