// rows.hip -- search by stored vector (include/innr_hip.h): innr_batch_gather_rows[_dev], VerticalBatch::extract_vector
// (batch.rs:217) for many vectors at once, and innr_batch_knn_rows[_dev], innr_batch_knn with the queries taken from the batch
// itself. A translation unit of its own over the kernels of kernels_rows.h; the search itself is the public innr_batch_knn_dev
// (the context's lock is recursive), so engine choice and results are that call's. DESIGN.md 4.5f.
// Workspace: the context's rows_* buffers and nothing else -- the inner search uses most of the others.
#include "api_internal.h"
#include "kernels_rows.h"

namespace {

constexpr size_t kRowsRound = 4096;                  // queries per round of innr_batch_knn_rows
constexpr size_t kRowsWorkspace = (size_t)256 << 20; // a round's gathered rows + staged result stay within this
constexpr size_t kRowsFlagBytes = 256;               // rows_flag: word 0 = an index outside the batch was seen

innr_status need_f32(const innr_batch* b) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: a code row is not an f32 vector)");
        return INNR_E_BAD_ARG;
    }
    return INNR_OK;
}

innr_status bad_index(const innr_batch* b, const char* who) {
    set_error("%s: an index lies outside this batch's range [%llu, %llu)", who, (unsigned long long)b->index_base,
              (unsigned long long)(b->index_base + b->N));
    return INNR_E_BAD_ARG;
}

// the host entry points check before they move anything
innr_status check_host_indices(const innr_batch* b, const uint64_t* idx, size_t n, const char* who) {
    for (size_t j = 0; j < n; ++j)
        if (idx[j] < b->index_base || idx[j] - b->index_base >= b->N) return bad_index(b, who);
    return INNR_OK;
}

innr_status clear_flag(innr_ctx* c) {
    INNR_TRY(c->rows_flag.ensure(kRowsFlagBytes));
    INNR_HIP_CHECK(hipMemsetAsync(c->rows_flag.p, 0, kRowsFlagBytes, c->stream));
    return INNR_OK;
}

// the flag, read once at the end of a call (synchronises the stream)
innr_status check_flag(innr_ctx* c, const innr_batch* b, const char* who) {
    uint32_t bad = 0;
    INNR_HIP_CHECK(copy_out(c, &bad, c->rows_flag.p, sizeof(bad)));
    INNR_HIP_CHECK(ctx_sync(c));
    return bad ? bad_index(b, who) : INNR_OK;
}

// n rows (n > 0, D > 0) to d_out[n][D]: from the row-major copy when the batch has one, else from the store. Never builds the copy.
innr_status launch_gather(innr_batch* b, const uint64_t* d_idx, size_t n, float* d_out) {
    innr_ctx* c = b->ctx;
    uint32_t* bad = c->rows_flag.as<uint32_t>();
    uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
    const CorpusCopy& rc = b->copy[kCopyRows];
    if (rc.p && !c->tune.no_rows_copy) {
        const int vec = b->D % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 16 == 0;
        const unsigned nb = (unsigned)std::min<size_t>((n + 3) / 4, (size_t)c->num_cus * 64);
        gather_rows_copy_kernel<<<nb, 256, 0, c->stream>>>(reinterpret_cast<const uint32_t*>(rc.p), rc.nk, (uint32_t)b->N, (uint32_t)b->D,
                                                            b->index_base, d_idx, n, out, bad, vec);
    } else {
        const size_t ti = (n + kRowsTile - 1) / kRowsTile, td = (b->D + kRowsTile - 1) / kRowsTile;
        const dim3 grid((unsigned)std::min<size_t>(ti, 1u << 20), (unsigned)std::min<size_t>(td, 1024));
        gather_rows_pdx_kernel<<<grid, dim3(kRowsTile, 8), 0, c->stream>>>(reinterpret_cast<const uint32_t*>(b->V), b->ldN, (uint32_t)b->N,
                                                                           (uint32_t)b->D, b->index_base, d_idx, n, out, bad);
    }
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// what the kNN entry points share. *work = false: *out_k is final. kin: the inner call's k; kk = min(kin, N) entries come back
// per query, kp of them reach the caller.
struct RowsPlan {
    size_t kin, kk, kp, round;
};
innr_status knn_rows_check(innr_batch* b, int metric, size_t Q, size_t k, int exclude_self, size_t* out_k, innr_knn_stats* stats,
                           RowsPlan* p, bool* work) {
    *work = false;
    INNR_TRY(need_f32(b));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !metric_ok(metric) || !out_k) {
        set_error("bad batch/metric/out_k");
        return INNR_E_BAD_ARG;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0) return INNR_OK;
    p->kin = exclude_self && k != SIZE_MAX ? k + 1 : k;
    p->kk = std::min(p->kin, b->N);
    p->kp = exclude_self ? std::min(k, b->N - 1) : p->kk;
    if (p->kp == 0) return INNR_OK;  // exclude_self on a batch of one vector
    // a query's share of a round's workspace: its gathered row and, with exclude_self, (k + 1) staged entries of 12 bytes
    const size_t row_bytes = b->D * sizeof(float);
    const size_t stage_bytes = !exclude_self ? 0 : (p->kin > kRowsWorkspace / 12 ? kRowsWorkspace : p->kin * 12);
    p->round = std::max<size_t>(1, std::min(kRowsRound, kRowsWorkspace / std::max<size_t>(row_bytes + stage_bytes, 1)));
    *work = true;
    return INNR_OK;
}

}  // namespace

innr_status innr_batch_gather_rows_dev(innr_batch* b, const uint64_t* d_idx, size_t n, float* d_out) {
    INNR_TRY(need_f32(b));
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    if (n == 0 || b->D == 0) return INNR_OK;
    if (!d_idx || !d_out) {
        set_error("gather_rows: null indices / output");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(clear_flag(c));
    INNR_TRY(launch_gather(b, d_idx, n, d_out));
    return check_flag(c, b, "gather_rows");
}

innr_status innr_batch_gather_rows(innr_batch* b, const uint64_t* idx, size_t n, float* out) {
    INNR_TRY(need_f32(b));
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    if (n == 0 || b->D == 0) return INNR_OK;
    if (!idx || !out) {
        set_error("gather_rows: null indices / output");
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(check_host_indices(b, idx, n, "gather_rows"));
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(clear_flag(c));
    // in rounds, so that a long list does not need its whole output on the device at once
    const size_t D = b->D, round = std::max<size_t>(1, std::min(n, kRowsWorkspace / (D * sizeof(float) + sizeof(uint64_t))));
    const size_t idx_bytes = round_up(round * sizeof(uint64_t), 256);
    INNR_TRY(c->rows_io.ensure(idx_bytes + round * D * sizeof(float)));
    uint64_t* d_idx = c->rows_io.as<uint64_t>();
    float* d_out = reinterpret_cast<float*>(c->rows_io.as<char>() + idx_bytes);
    for (size_t j0 = 0; j0 < n; j0 += round) {
        const size_t r = std::min(round, n - j0);
        INNR_HIP_CHECK(copy_in(c, d_idx, idx + j0, r * sizeof(uint64_t)));
        INNR_TRY(launch_gather(b, d_idx, r, d_out));
        INNR_HIP_CHECK(copy_out(c, out + j0 * D, d_out, r * D * sizeof(float)));
        if (j0 + r < n) INNR_HIP_CHECK(ctx_sync(c));  // the buffers are used again
    }
    return check_flag(c, b, "gather_rows");
}

innr_status innr_batch_knn_rows_dev(innr_batch* b, int metric, const uint64_t* d_idx, size_t Q, size_t k, int exclude_self, int engine,
                                    uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats) {
    RowsPlan p{};
    bool work = false;
    INNR_TRY(knn_rows_check(b, metric, Q, k, exclude_self, out_k, stats, &p, &work));
    if (!work) return INNR_OK;
    if (!d_idx || !d_out_idx || !d_out_score) {
        set_error("knn_rows: null indices / outputs");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(clear_flag(c));
    INNR_HIP_CHECK(hipEventRecord(c->ev[4], c->stream));
    const size_t D = b->D, round = std::min(p.round, Q);
    INNR_TRY(c->rows_q.ensure(std::max<size_t>(round * D * sizeof(float), 16)));
    uint64_t* st_idx = nullptr;
    float* st_score = nullptr;
    if (exclude_self) {
        const size_t idx_bytes = round_up(round * p.kk * sizeof(uint64_t), 256);
        INNR_TRY(c->rows_stage.ensure(idx_bytes + round * p.kk * sizeof(float)));
        st_idx = c->rows_stage.as<uint64_t>();
        st_score = reinterpret_cast<float*>(c->rows_stage.as<char>() + idx_bytes);
    }
    innr_knn_stats sum{};
    for (size_t q0 = 0; q0 < Q; q0 += round) {
        const size_t r = std::min(round, Q - q0);
        if (D) INNR_TRY(launch_gather(b, d_idx + q0, r, c->rows_q.as<float>()));
        innr_knn_stats st{};
        size_t got = 0;
        INNR_TRY(innr_batch_knn_dev(b, metric, c->rows_q.as<float>(), r, D, p.kin, engine, exclude_self ? st_idx : d_out_idx + q0 * p.kk,
                                    exclude_self ? st_score : d_out_score + q0 * p.kk, &got, &st));
        if (got != p.kk) {
            set_error("knn_rows: the inner search returned %zu results per query, not %zu", got, p.kk);
            return INNR_E_HIP;
        }
        if (exclude_self) {
            strip_self_kernel<<<(unsigned)((r + 3) / 4), 256, 0, c->stream>>>(st_idx, st_score, (uint32_t)p.kk, d_idx + q0, (uint32_t)r,
                                                                              d_out_idx + q0 * p.kp, d_out_score + q0 * p.kp);
            INNR_HIP_CHECK(hipGetLastError());
        }
        sum.engine = st.engine;
        sum.queries_fallback += st.queries_fallback;
        sum.candidates_kept = std::max(sum.candidates_kept, st.candidates_kept);
        sum.gemm_ms += st.gemm_ms;
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[5], c->stream));
    INNR_TRY(check_flag(c, b, "knn_rows"));
    *out_k = p.kp;
    if (stats) {
        *stats = sum;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[4], c->ev[5]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}

innr_status innr_batch_knn_rows(innr_batch* b, int metric, const uint64_t* idx, size_t Q, size_t k, int exclude_self, int engine,
                                uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    RowsPlan p{};
    bool work = false;
    INNR_TRY(knn_rows_check(b, metric, Q, k, exclude_self, out_k, stats, &p, &work));
    if (!work) return INNR_OK;
    if (!idx || !out_idx || !out_score) {
        set_error("knn_rows: null indices / outputs");
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(check_host_indices(b, idx, Q, "knn_rows"));
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    // [Q] indices in, [Q][kp] indices and scores out
    const size_t in_bytes = round_up(Q * sizeof(uint64_t), 256), oi_bytes = round_up(Q * p.kp * sizeof(uint64_t), 256);
    INNR_TRY(c->rows_io.ensure(in_bytes + oi_bytes + Q * p.kp * sizeof(float)));
    uint64_t* d_idx = c->rows_io.as<uint64_t>();
    uint64_t* d_oi = reinterpret_cast<uint64_t*>(c->rows_io.as<char>() + in_bytes);
    float* d_os = reinterpret_cast<float*>(c->rows_io.as<char>() + in_bytes + oi_bytes);
    INNR_HIP_CHECK(copy_in(c, d_idx, idx, Q * sizeof(uint64_t)));
    INNR_TRY(innr_batch_knn_rows_dev(b, metric, d_idx, Q, k, exclude_self, engine, d_oi, d_os, out_k, stats));
    INNR_HIP_CHECK(copy_out(c, out_idx, d_oi, Q * p.kp * sizeof(uint64_t)));
    INNR_HIP_CHECK(copy_out(c, out_score, d_os, Q * p.kp * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}
