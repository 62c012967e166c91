// adaptive.hip -- innr_batch_knn_adaptive / _dev (include/innr_hip.h): batch_knn_adaptive (src/batch.rs:441-564) on the device,
// over the kernels of kernels_adaptive.h. A translation unit of its own; it borrows the exact engine's scan and the exclusive scan
// from api.hip and the radix select + sort from sort_full.hip through api_internal.h. DESIGN.md 4.5d has the restatement of the
// reference's sequential loop that the phases below follow, step by step.
#include "api_internal.h"
#include "kernels_adaptive.h"

namespace {

struct AdaptiveBufs {
    AdaptiveState* st;
    uint32_t *cnt[2], *off[2];  // per-chunk counts and their exclusive scans
    uint32_t* idx[2];           // the live list, ascending corpus indices; a compaction writes the other copy
    float* dist[2];
    uint8_t* death;
};

constexpr size_t kStateBytes = 256;
static_assert(sizeof(AdaptiveState) <= kStateBytes, "AdaptiveState outgrew its slot");

// the k-th smallest of dist[0, n) (total_cmp), times scale -> st->thr; leaves the best k composites sorted at keys + N
innr_status kth_threshold(innr_ctx* c, const float* dist, size_t n, size_t k, size_t N, float scale, AdaptiveState* st) {
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    INNR_HIP_CHECK(full_sort_scores(dist, n, true, keys, keys + N, c->sort_tmp.p, c->sort_tmp.bytes, c->stream, nullptr, k));
    adaptive_threshold_kernel<<<1, 64, 0, c->stream>>>(keys + N, k, scale, st);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// One query. *alive_after_warmup: |L| after step 4. Leaves k results at d_out_idx / d_out_score.
innr_status adaptive_one(innr_batch* b, const float* dq, size_t k, size_t W, uint64_t* d_out_idx, float* d_out_score,
                         uint32_t* alive_after_warmup, float* warm_ms) {
    innr_ctx* c = b->ctx;
    const size_t N = b->N, D = b->D;
    const float scale = (float)D / (float)W;  // batch.rs:484
    const uint32_t nch = (uint32_t)((N + kAdpChunk - 1) / kAdpChunk);
    AdaptiveBufs w;
    {
        char* p = c->adp_scan.as<char>();
        w.st = reinterpret_cast<AdaptiveState*>(p);
        uint32_t* u = reinterpret_cast<uint32_t*>(p + kStateBytes);
        w.cnt[0] = u, w.cnt[1] = u + nch, w.off[0] = u + 2 * (size_t)nch, w.off[1] = u + 3 * (size_t)nch;
    }
    float* warm = c->scores.as<float>();
    // steps 2-3: warm-up distances of every vector, the threshold from their k-th smallest
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    INNR_TRY(l2_prefix_scores(b, dq, W, warm));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_TRY(kth_threshold(c, warm, N, k, N, scale, w.st));
    // step 4: flag, count, and -- once the host knows how long the list gets -- compact
    adaptive_flag_count_kernel<<<nch, kAdpChunk, 0, c->stream>>>(warm, (uint32_t)N, scale, w.st, w.cnt[0]);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_TRY(exclusive_scan_u32(c, w.cnt[0], nch, w.off[0], &w.st->total[0]));
    uint32_t flagged = 0;
    INNR_HIP_CHECK(copy_out(c, &flagged, &w.st->total[0], sizeof(flagged)));
    INNR_HIP_CHECK(ctx_sync(c));
    {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) *warm_ms += ms;
    }
    const uint32_t cap = (uint32_t)(N - k);
    uint32_t n = (uint32_t)N - std::min(flagged, cap);
    *alive_after_warmup = n;
    {
        const size_t n4 = round_up(n, 64);  // (keeps every array 256-byte aligned)
        INNR_TRY(c->adp_list.ensure(n4 * 17));
        char* p = c->adp_list.as<char>();
        w.idx[0] = reinterpret_cast<uint32_t*>(p), w.idx[1] = reinterpret_cast<uint32_t*>(p + n4 * 4);
        w.dist[0] = reinterpret_cast<float*>(p + n4 * 8), w.dist[1] = reinterpret_cast<float*>(p + n4 * 12);
        w.death = reinterpret_cast<uint8_t*>(p + n4 * 16);
    }
    adaptive_flag_scatter_kernel<<<nch, kAdpChunk, 0, c->stream>>>(warm, (uint32_t)N, scale, w.st, w.off[0], cap, w.idx[0], w.dist[0], n);
    INNR_HIP_CHECK(hipGetLastError());
    int cur = 0;
    // steps 6-9: the remaining dimensions in segments that end on a multiple of 32 (or on the last dimension)
    for (size_t s0 = W; s0 < D;) {
        const uint32_t lch = (n + kAdpChunk - 1) / kAdpChunk;
        if (n == k) {  // step 8 for every remaining segment at once: nothing is pruned any more, thresholds no longer matter
            adaptive_finish_kernel<<<lch, kAdpChunk, 0, c->stream>>>(b->V, b->ldN, dq, (uint32_t)s0, (uint32_t)D, w.idx[cur], w.dist[cur], n,
                                                                      (uint32_t)N);
            INNR_HIP_CHECK(hipGetLastError());
            break;
        }
        const size_t s1 = std::min(round_up(s0, 32), D - 1);
        INNR_HIP_CHECK(hipMemsetAsync(w.st->hist, 0, sizeof(w.st->hist), c->stream));
        adaptive_segment_kernel<<<lch, kAdpChunk, 0, c->stream>>>(b->V, b->ldN, dq, (uint32_t)s0, (uint32_t)s1, w.idx[cur], w.dist[cur], n,
                                                                   (uint32_t)N, w.st, w.death);
        adaptive_cut_kernel<<<1, 64, 0, c->stream>>>(w.st, n - (uint32_t)k);
        INNR_HIP_CHECK(hipGetLastError());
        uint32_t killed = 0;
        INNR_HIP_CHECK(copy_out(c, &killed, &w.st->killed, sizeof(killed)));
        INNR_HIP_CHECK(ctx_sync(c));
        if (killed) {
            const uint32_t m = n - killed;
            adaptive_cut_count_kernel<<<lch, kAdpChunk, 0, c->stream>>>(w.death, n, w.st, w.cnt[0], w.cnt[1]);
            INNR_HIP_CHECK(hipGetLastError());
            INNR_TRY(exclusive_scan_u32(c, w.cnt[0], lch, w.off[0], &w.st->total[0]));
            INNR_TRY(exclusive_scan_u32(c, w.cnt[1], lch, w.off[1], &w.st->total[1]));
            adaptive_cut_scatter_kernel<<<lch, kAdpChunk, 0, c->stream>>>(w.death, w.idx[cur], w.dist[cur], n, w.st, w.off[0], w.off[1],
                                                                           w.idx[cur ^ 1], w.dist[cur ^ 1], m);
            INNR_HIP_CHECK(hipGetLastError());
            cur ^= 1;
            n = m;
        }
        // step 9 (only where a later segment can still prune with it)
        if (s1 % 32 == 0 && s1 + 1 < D && n > k) INNR_TRY(kth_threshold(c, w.dist[cur], n, k, N, 1.0f, w.st));
        s0 = s1 + 1;
    }
    // step 10: the survivors by (distance, index), the first k
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    INNR_HIP_CHECK(full_sort_scores(w.dist[cur], n, true, keys, keys + N, c->sort_tmp.p, c->sort_tmp.bytes, c->stream, nullptr, k));
    adaptive_emit_kernel<<<(unsigned)((k + 255) / 256), 256, 0, c->stream>>>(keys + N, (uint32_t)k, w.idx[cur], n, b->index_base, d_out_idx,
                                                                          d_out_score);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// the checks both entry points share, in the reference's order (batch.rs:447-463); *work = false: nothing left to do
innr_status adaptive_check(innr_batch* b, size_t Q, size_t D, size_t k, size_t warmup_dims, size_t* out_k, innr_knn_stats* stats,
                           bool* work) {
    *work = false;
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->engine = INNR_KNN_EXACT;
    }
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !out_k) {
        set_error("bad batch/out_k");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // batch.rs:447
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    if (warmup_dims == 0) {  // batch.rs:448
        set_error("warmup_dims must be > 0");
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    *work = !(b->N == 0 || k == 0 || Q == 0);  // batch.rs:450-455
    return INNR_OK;
}

}  // namespace

innr_status innr_batch_knn_adaptive_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, size_t warmup_dims,
                                        uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats) {
    bool work = false;
    INNR_TRY(adaptive_check(b, Q, D, k, warmup_dims, out_k, stats, &work));
    if (!work) return INNR_OK;
    if ((!d_queries && D) || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    const size_t N = b->N, kout = std::min(k, N);  // batch.rs:457
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    uint32_t kept = 0;
    float warm_ms = 0.0f;
    if (D == 0) {  // batch.rs:458-463
        const size_t total = Q * kout;
        adaptive_iota_kernel<<<(unsigned)((total + 255) / 256), 256, 0, c->stream>>>(total, kout, b->index_base, d_out_idx, d_out_score);
        INNR_HIP_CHECK(hipGetLastError());
        kept = (uint32_t)N;
    } else {
        const size_t W = std::min(warmup_dims, D);  // batch.rs:464
        const size_t nch = (N + kAdpChunk - 1) / kAdpChunk;
        size_t tmp_bytes = 0;
        INNR_HIP_CHECK(full_sort_scratch_bytes(N, &tmp_bytes));
        INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
        INNR_TRY(c->sort_keys.ensure((N + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
        INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        INNR_TRY(c->adp_scan.ensure(kStateBytes + 4 * nch * sizeof(uint32_t)));
        for (size_t q = 0; q < Q; ++q) {
            uint32_t alive = 0;
            INNR_TRY(adaptive_one(b, d_queries + q * D, kout, W, d_out_idx + q * kout, d_out_score + q * kout, &alive, &warm_ms));
            kept = std::max(kept, alive);
        }
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    *out_k = kout;
    if (stats) {
        stats->candidates_kept = kept;
        stats->gemm_ms = warm_ms;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}

innr_status innr_batch_knn_adaptive(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, size_t warmup_dims,
                                    uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    bool work = false;
    INNR_TRY(adaptive_check(b, Q, D, k, warmup_dims, out_k, stats, &work));
    if (!work) return INNR_OK;
    if ((!queries && D) || !out_idx || !out_score) return INNR_E_BAD_ARG;
    return knn_from_host(b->ctx, queries, Q, D, std::min(k, b->N), out_idx, out_score, out_k, [&](const float* dQ, uint64_t* di, float* ds) {
        return innr_batch_knn_adaptive_dev(b, dQ, Q, D, k, warmup_dims, di, ds, out_k, stats);
    });
}
