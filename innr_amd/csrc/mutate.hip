// mutate.hip -- changing a resident f32 batch in place (include/innr_hip.h): innr_batch_append_rows / innr_batch_update_rows /
// innr_batch_keep_rows[_dev]. DESIGN.md 4.5g. A translation unit of its own over the kernels of kernels_mutate.h; the kernels
// api.hip owns (transpose_rows_kernel, the selection's count and gather) are reached through its launchers (api_internal.h).
// Each call either leaves the batch exactly as it was or ends in invalidate_derived (api.hip), the one list of what a batch
// derives from its store: the store is the only thing these functions write themselves.
// u8 code batches are refused here and changed by mutate_u8.hip, which shares this unit's index validation (launch_update_check).
// Workspace: the context's rows_io (staged rows and indices), rows_flag, rows_bits, rows_map; keep: flt_in / flt_mask / flt_scan.
#include "api_internal.h"
#include "kernels_mutate.h"

namespace {

constexpr size_t kStageBytes = (size_t)256 << 20;  // a host entry point's staged rows and indices stay within this
constexpr size_t kFlagBytes = 256;                 // rows_flag: UpdateFlag at its head (word 0 also: the scatter's own range check)

innr_status clear_flag(innr_ctx* c) {
    INNR_TRY(c->rows_flag.ensure(kFlagBytes));
    INNR_HIP_CHECK(hipMemsetAsync(c->rows_flag.p, 0, kFlagBytes, c->stream));
    return INNR_OK;
}

innr_status need_mutable(const innr_batch* b, const char* who) {
    if (!b) {
        set_error("%s: batch is null", who);
        return INNR_E_BAD_ARG;
    }
    if (!b->V) {
        set_error("%s needs an f32 batch (got a u8 code batch)", who);
        return INNR_E_BAD_ARG;
    }
    if (b->is_view) {
        set_error("%s: a prefix view cannot be changed (change its parent, with no view alive)", who);
        return INNR_E_BAD_ARG;
    }
    return INNR_OK;
}

innr_status need_dim(const innr_batch* b, size_t D, const char* who) {
    if (D != b->D) {
        set_error("%s: rows of dimension %zu for a batch of dimension %zu", who, D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    return INNR_OK;
}

// rows per staging round of a host entry point: what fits the 256 MiB bound, at most the option mutate_round, at least one
size_t stage_round(const innr_ctx* c, size_t n, size_t row_bytes) {
    size_t r = std::max<size_t>(1, kStageBytes / std::max<size_t>(row_bytes, 1));
    if (c->tune.mutate_round > 0) r = std::min(r, (size_t)c->tune.mutate_round);
    return std::min(n, r);
}

// rows[n][D] into columns col0 .. col0 + n of the store V: device rows at once, host rows staged through c->rows_io
innr_status put_rows(innr_ctx* c, const float* rows, bool host, size_t n, size_t D, float* V, size_t ldN, size_t col0) {
    if (D == 0) return INNR_OK;
    if (!host) {
        INNR_HIP_CHECK(transpose_rows_into(c, rows, n, D, V, ldN, col0));
        return INNR_OK;
    }
    const size_t round = stage_round(c, n, D * sizeof(float));
    INNR_TRY(c->rows_io.ensure(round * D * sizeof(float)));
    for (size_t i0 = 0; i0 < n; i0 += round) {
        const size_t r = std::min(round, n - i0);
        INNR_HIP_CHECK(copy_in(c, c->rows_io.p, rows + i0 * D, r * D * sizeof(float)));
        INNR_HIP_CHECK(transpose_rows_into(c, c->rows_io.as<float>(), r, D, V, ldN, col0 + i0));
        if (i0 + r < n) INNR_HIP_CHECK(ctx_sync(c));  // the buffer is used again
    }
    return INNR_OK;
}

// b takes nb's store and vector count; nb, with b's old store, is freed (the stream is synchronised)
void take_store(innr_batch* b, innr_batch* nb) {
    std::swap(b->V, nb->V);
    std::swap(b->ldN, nb->ldN);
    std::swap(b->corpus_bytes, nb->corpus_bytes);
    b->N = nb->N;
    innr_batch_free(nb);
}

innr_status append_rows(innr_batch* b, const float* rows, size_t n, size_t D, bool host) {
    INNR_TRY(need_mutable(b, "append_rows"));
    INNR_TRY(need_dim(b, D, "append_rows"));
    if (n == 0) return INNR_OK;
    if (!rows && D) {
        set_error("append_rows: rows is null");
        return INNR_E_BAD_ARG;
    }
    if (n >= kMaxBatchN || b->N >= kMaxBatchN - n) {
        set_error("append_rows: %zu + %zu vectors are too many for u32 device indices", b->N, n);
        return INNR_E_UNSUPPORTED;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const size_t N = b->N;
    if (N + n <= b->ldN) {
        // into the zero padding, in place
        const innr_status st = [&]() -> innr_status {
            INNR_TRY(put_rows(c, rows, host, n, D, b->V, b->ldN, N));
            INNR_HIP_CHECK(ctx_sync(c));
            return INNR_OK;
        }();
        if (st != INNR_OK) {  // the padding as it was (N has not moved)
            if (D) (void)hipMemset2DAsync(b->V + N, b->ldN * sizeof(float), 0, n * sizeof(float), D, c->stream);
            (void)hipStreamSynchronize(c->stream);
            return st;
        }
        b->N = N + n;
        invalidate_derived(b);
        return INNR_OK;
    }
    innr_batch* nb = nullptr;
    INNR_TRY(alloc_batch(c, N + n, D, &nb));  // zeroed: the dimension rows D .. Dpad and the columns >= N + n included
    const innr_status st = [&]() -> innr_status {
        if (N && D)
            INNR_HIP_CHECK(hipMemcpy2DAsync(nb->V, nb->ldN * sizeof(float), b->V, b->ldN * sizeof(float), N * sizeof(float), D,
                                            hipMemcpyDeviceToDevice, c->stream));
        INNR_TRY(put_rows(c, rows, host, n, D, nb->V, nb->ldN, N));
        INNR_HIP_CHECK(ctx_sync(c));
        return INNR_OK;
    }();
    if (st != INNR_OK) {
        innr_batch_free(nb);
        return st;
    }
    take_store(b, nb);
    invalidate_derived(b);
    return INNR_OK;
}

innr_status launch_scatter(innr_batch* b, const uint64_t* d_idx, const float* d_rows, size_t n) {
    innr_ctx* c = b->ctx;
    const size_t ti = (n + kRowsTile - 1) / kRowsTile, td = (b->D + kRowsTile - 1) / kRowsTile;
    const dim3 grid((unsigned)std::min<size_t>(ti, 1u << 20), (unsigned)std::min<size_t>(td, 1024));
    scatter_rows_pdx_kernel<<<grid, dim3(kRowsTile, 8), 0, c->stream>>>(reinterpret_cast<uint32_t*>(b->V), b->ldN, (uint32_t)b->N,
                                                                        (uint32_t)b->D, b->index_base, d_idx, n,
                                                                        reinterpret_cast<const uint32_t*>(d_rows),
                                                                        c->rows_flag.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

innr_status update_rows(innr_batch* b, const uint64_t* idx, const float* rows, size_t n, size_t D, bool host) {
    INNR_TRY(need_mutable(b, "update_rows"));
    INNR_TRY(need_dim(b, D, "update_rows"));
    if (n == 0) return INNR_OK;
    if (!idx || (!rows && D)) {
        set_error("update_rows: null indices / rows");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    // pass 1: every index of the call, before anything is written
    const size_t bits_bytes = std::max<size_t>((b->N + 31) / 32 * sizeof(uint32_t), 16);
    INNR_TRY(c->rows_bits.ensure(bits_bytes));
    INNR_HIP_CHECK(hipMemsetAsync(c->rows_bits.p, 0, bits_bytes, c->stream));
    INNR_TRY(clear_flag(c));
    const size_t round = host ? stage_round(c, n, D * sizeof(float) + sizeof(uint64_t)) : n;
    const size_t idx_bytes = round_up(round * sizeof(uint64_t), 256);
    uint64_t* st_idx = nullptr;
    float* st_rows = nullptr;
    if (host) {
        INNR_TRY(c->rows_io.ensure(idx_bytes + round * D * sizeof(float)));
        st_idx = c->rows_io.as<uint64_t>();
        st_rows = reinterpret_cast<float*>(c->rows_io.as<char>() + idx_bytes);
        for (size_t j0 = 0; j0 < n; j0 += round) {
            const size_t r = std::min(round, n - j0);
            INNR_HIP_CHECK(copy_in(c, st_idx, idx + j0, r * sizeof(uint64_t)));
            INNR_TRY(launch_update_check(b, st_idx, r));
            if (j0 + r < n) INNR_HIP_CHECK(ctx_sync(c));  // the buffer is used again
        }
    } else {
        INNR_TRY(launch_update_check(b, idx, n));
    }
    UpdateFlag f{};
    static_assert(sizeof(UpdateFlag) == 24 && sizeof(UpdateFlag) <= kFlagBytes, "update_check_kernel's flag layout");
    INNR_HIP_CHECK(copy_out(c, &f, c->rows_flag.p, sizeof(f)));
    INNR_HIP_CHECK(ctx_sync(c));
    if (f.outside) {
        set_error("update_rows: index %llu lies outside this batch's range [%llu, %llu)", (unsigned long long)f.outside_idx,
                  (unsigned long long)b->index_base, (unsigned long long)(b->index_base + b->N));
        return INNR_E_BAD_ARG;
    }
    if (f.twice) {
        set_error("update_rows: index %llu occurs more than once in one call (duplicate indices are refused)",
                  (unsigned long long)f.twice_idx);
        return INNR_E_BAD_ARG;
    }
    if (D == 0) return INNR_OK;  // nothing to write
    // pass 2: the writes (the scatter checks the range once more; rows_flag word 0 is clean here)
    const innr_status st = [&]() -> innr_status {
        if (host) {
            for (size_t j0 = 0; j0 < n; j0 += round) {
                const size_t r = std::min(round, n - j0);
                INNR_HIP_CHECK(copy_in(c, st_idx, idx + j0, r * sizeof(uint64_t)));
                INNR_HIP_CHECK(copy_in(c, st_rows, rows + j0 * D, r * D * sizeof(float)));
                INNR_TRY(launch_scatter(b, st_idx, st_rows, r));
                if (j0 + r < n) INNR_HIP_CHECK(ctx_sync(c));
            }
        } else {
            INNR_TRY(launch_scatter(b, idx, rows, n));
        }
        uint32_t bad = 0;  // set only if the indices changed under the call
        INNR_HIP_CHECK(copy_out(c, &bad, c->rows_flag.p, sizeof(bad)));
        INNR_HIP_CHECK(ctx_sync(c));
        if (bad) {
            set_error("update_rows: the indices changed between the check and the writes (rows of valid indices were written)");
            return INNR_E_BAD_ARG;
        }
        return INNR_OK;
    }();
    if (st != INNR_OK) (void)hipStreamSynchronize(c->stream);
    invalidate_derived(b);  // also after a failure in pass 2: rows may have been written
    return st;
}

innr_status keep_rows(innr_batch* b, const uint8_t* mask, size_t* out_n, bool host) {
    INNR_TRY(need_mutable(b, "keep_rows"));
    if (out_n) *out_n = b->N;
    if (b->N == 0) return INNR_OK;
    if (!mask) {
        set_error("keep_rows: mask is null");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const uint8_t* d_mask = mask;
    if (host) {
        INNR_TRY(c->flt_in.ensure(b->N));
        INNR_HIP_CHECK(hipMemcpyAsync(c->flt_in.p, mask, b->N, hipMemcpyHostToDevice, c->stream));
        d_mask = c->flt_in.as<uint8_t>();
    }
    size_t npass = 0;
    INNR_TRY(count_mask(b, d_mask, &npass));  // (synchronises)
    if (npass == b->N) return INNR_OK;        // every row stays: nothing changes, nothing is dropped
    innr_batch* nb = nullptr;
    INNR_TRY(alloc_batch(c, npass, b->D, &nb));
    const innr_status st = [&]() -> innr_status {
        if (npass && b->D) {
            INNR_TRY(c->rows_map.ensure(npass * sizeof(uint32_t)));
            INNR_TRY(gather_passing(b, nb->V, nb->ldN, c->rows_map.as<uint32_t>()));
        }
        INNR_HIP_CHECK(ctx_sync(c));
        return INNR_OK;
    }();
    if (st != INNR_OK) {
        innr_batch_free(nb);
        return st;
    }
    take_store(b, nb);
    invalidate_derived(b);
    if (out_n) *out_n = b->N;
    return INNR_OK;
}

}  // namespace

// (declared in api_internal.h: the code batches' update shares the validation kernel, mutate_u8.hip)
innr_status innr::launch_update_check(innr_batch* b, const uint64_t* d_idx, size_t n) {
    innr_ctx* c = b->ctx;
    const unsigned nb = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)c->num_cus * 8);
    update_check_kernel<<<nb, 256, 0, c->stream>>>(d_idx, n, b->index_base, (uint32_t)b->N, c->rows_bits.as<uint32_t>(),
                                                   c->rows_flag.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

innr_status innr_batch_append_rows(innr_batch* b, const float* rows, size_t n, size_t D) { return append_rows(b, rows, n, D, true); }
innr_status innr_batch_append_rows_dev(innr_batch* b, const float* d_rows, size_t n, size_t D) {
    return append_rows(b, d_rows, n, D, false);
}
innr_status innr_batch_update_rows(innr_batch* b, const uint64_t* idx, const float* rows, size_t n, size_t D) {
    return update_rows(b, idx, rows, n, D, true);
}
innr_status innr_batch_update_rows_dev(innr_batch* b, const uint64_t* d_idx, const float* d_rows, size_t n, size_t D) {
    return update_rows(b, d_idx, d_rows, n, D, false);
}
innr_status innr_batch_keep_rows(innr_batch* b, const uint8_t* mask, size_t* out_n) { return keep_rows(b, mask, out_n, true); }
innr_status innr_batch_keep_rows_dev(innr_batch* b, const uint8_t* d_mask, size_t* out_n) { return keep_rows(b, d_mask, out_n, false); }
