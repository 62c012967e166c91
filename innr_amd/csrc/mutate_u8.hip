// mutate_u8.hip -- changing a resident u8 code batch in place (include/innr_hip.h): innr_batch_append_codes / _update_codes /
// _keep_codes and the variants fed f32 rows, innr_batch_append_quantized / _update_quantized, each with its _dev twin.
// DESIGN.md 4.5h. A translation unit of its own over the two kernels of kernels_mutate_u8.h; the kernels other units own
// (transpose_rows_u8_kernel, the selection's count and gather: api.hip; update_check_kernel: mutate.hip) are reached through
// their launchers (api_internal.h). Each call either leaves the batch exactly as it was or ends in invalidate_derived (api.hip),
// the one list of what a batch derives from its store: the store is the only thing these functions write themselves.
// Workspace: the context's rows_io (a round's staged indices | codes | f32 rows), rows_flag, rows_bits, rows_map; keep: flt_in /
// flt_mask / flt_scan.
#include "api_internal.h"
#include "kernels_mutate_u8.h"

namespace {

constexpr size_t kStageBytes = (size_t)256 << 20;  // a round's staged indices, codes and f32 rows stay within this
constexpr size_t kFlagBytes = 256;                 // rows_flag: UpdateFlag at its head (word 0 also: the scatter's own range check)

innr_status need_code_batch(const innr_batch* b, const char* who) {
    if (!b) {
        set_error("%s: batch is null", who);
        return INNR_E_BAD_ARG;
    }
    if (!b->C8) {
        set_error("%s needs a u8 code batch (got an f32 batch: innr_batch_append_rows and its kin change one)", who);
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

innr_status need_room(const innr_batch* b, size_t n, const char* who) {
    if (n >= kMaxBatchNU8 || b->N >= kMaxBatchNU8 - n) {
        set_error("%s: %zu + %zu vectors are too many for a code batch (u32 device indices)", who, b->N, n);
        return INNR_E_UNSUPPORTED;
    }
    return INNR_OK;
}

// The rows of a call as they arrive: codes or f32 rows (exactly one is set), on the host or on the device.
struct Source {
    const uint8_t* codes;
    const float* rows;
    bool host;
    bool null() const { return !codes && !rows; }
};

// One round of a call in c->rows_io: [indices | codes | f32 rows], each part only where the call needs it. A call whose codes are
// on the device already runs as one round with nothing staged.
struct Rounds {
    size_t round = 0;          // rows per round
    uint64_t* idx = nullptr;   // staged indices (host update)
    uint8_t* codes = nullptr;  // staged or quantised codes
    float* rows = nullptr;     // staged f32 rows (host, quantised)
};

innr_status plan_rounds(innr_ctx* c, const Source& s, bool with_idx, size_t n, size_t D, Rounds* out) {
    const bool stage_idx = with_idx && s.host, stage_codes = s.host || s.rows, stage_rows = s.host && s.rows;
    Rounds r;
    r.round = n;
    if (stage_idx || stage_codes) {
        const size_t row_bytes = (stage_idx ? sizeof(uint64_t) : 0) + (stage_codes ? D : 0) + (stage_rows ? D * sizeof(float) : 0);
        size_t m = std::max<size_t>(1, kStageBytes / std::max<size_t>(row_bytes, 1));
        if (c->tune.mutate_round > 0) m = std::min(m, (size_t)c->tune.mutate_round);
        r.round = std::min(n, m);
        const size_t idx_bytes = stage_idx ? round_up(r.round * sizeof(uint64_t), 256) : 0;
        const size_t code_bytes = stage_codes ? round_up(std::max<size_t>(r.round * D, 1), 256) : 0;
        const size_t rows_bytes = stage_rows ? r.round * D * sizeof(float) : 0;
        INNR_TRY(c->rows_io.ensure(idx_bytes + code_bytes + rows_bytes));
        char* p = c->rows_io.as<char>();
        if (stage_idx) r.idx = reinterpret_cast<uint64_t*>(p);
        if (stage_codes) r.codes = reinterpret_cast<uint8_t*>(p + idx_bytes);
        if (stage_rows) r.rows = reinterpret_cast<float*>(p + idx_bytes + code_bytes);
    }
    *out = r;
    return INNR_OK;
}

// the device codes of rows [i0, i0 + m) of the call: where they are, or staged / quantised into the round's buffers
innr_status round_codes(innr_batch* b, const Source& s, const Rounds& r, size_t i0, size_t m, const uint8_t** d_codes) {
    innr_ctx* c = b->ctx;
    const size_t D = b->D;
    if (s.codes) {
        if (!s.host) {
            *d_codes = s.codes + i0 * D;
            return INNR_OK;
        }
        INNR_HIP_CHECK(copy_in(c, r.codes, s.codes + i0 * D, m * D));
        *d_codes = r.codes;
        return INNR_OK;
    }
    const float* d_rows = s.rows + i0 * D;
    if (s.host) {
        INNR_HIP_CHECK(copy_in(c, r.rows, s.rows + i0 * D, m * D * sizeof(float)));
        d_rows = r.rows;
    }
    const size_t total = m * D;
    const unsigned nb = (unsigned)std::min<size_t>((total / 4 + 255) / 256 + 1, (size_t)c->num_cus * 16);
    // 255.0f / alpha in f32 on the host, as innr_batch_quantize_u8 and innr_batch_generate_u8 pass it (scalar.rs:213); no check on alpha
    quantize_rows_u8_kernel<<<nb, 256, 0, c->stream>>>(d_rows, total, b->offset, 255.0f / b->alpha, r.codes);
    INNR_HIP_CHECK(hipGetLastError());
    *d_codes = r.codes;
    return INNR_OK;
}

// the rows of the call into columns col0 .. col0 + n of the store C8, round by round
innr_status put_codes(innr_batch* b, const Source& s, size_t n, uint8_t* C8, size_t ldN, size_t col0) {
    innr_ctx* c = b->ctx;
    const size_t D = b->D;
    if (D == 0) return INNR_OK;
    Rounds r;
    INNR_TRY(plan_rounds(c, s, false, n, D, &r));
    for (size_t i0 = 0; i0 < n; i0 += r.round) {
        const size_t m = std::min(r.round, n - i0);
        const uint8_t* d_codes = nullptr;
        INNR_TRY(round_codes(b, s, r, i0, m, &d_codes));
        INNR_HIP_CHECK(transpose_codes_into(c, d_codes, m, D, C8, ldN, col0 + i0));
        if (s.host && i0 + m < n) INNR_HIP_CHECK(ctx_sync(c));  // the pinned area and the caller's pages are read until here
    }
    return INNR_OK;
}

// b takes nb's store and vector count; nb, with b's old store, is freed (the stream is synchronised)
void take_store(innr_batch* b, innr_batch* nb) {
    std::swap(b->C8, nb->C8);
    std::swap(b->ldN, nb->ldN);
    std::swap(b->corpus_bytes, nb->corpus_bytes);
    b->N = nb->N;
    innr_batch_free(nb);
}

innr_status append(innr_batch* b, const Source& s, size_t n, size_t D, const char* who) {
    INNR_TRY(need_code_batch(b, who));
    INNR_TRY(need_dim(b, D, who));
    if (n == 0) return INNR_OK;
    if (s.null() && D) {
        set_error("%s: rows is null", who);
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(need_room(b, n, who));
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const size_t N = b->N;
    if (N + n <= b->ldN) {
        // into the zero padding, in place
        const innr_status st = [&]() -> innr_status {
            INNR_TRY(put_codes(b, s, n, b->C8, b->ldN, N));
            INNR_HIP_CHECK(ctx_sync(c));
            return INNR_OK;
        }();
        if (st != INNR_OK) {  // the padding as it was (N has not moved)
            if (D) (void)hipMemset2DAsync(b->C8 + N, b->ldN, 0, n, D, c->stream);
            (void)hipStreamSynchronize(c->stream);
            return st;
        }
        b->N = N + n;
        invalidate_derived(b);
        return INNR_OK;
    }
    innr_batch* nb = nullptr;
    INNR_TRY(alloc_batch_u8(c, N + n, D, b->alpha, b->offset, &nb));  // zeroed: rows D .. Dpad and the columns >= N + n included
    const innr_status st = [&]() -> innr_status {
        if (N && D)  // the old D x N block: a pitched copy, the pitches are the two stores' widths in bytes
            INNR_HIP_CHECK(hipMemcpy2DAsync(nb->C8, nb->ldN, b->C8, b->ldN, N, D, hipMemcpyDeviceToDevice, c->stream));
        INNR_TRY(put_codes(b, s, n, nb->C8, nb->ldN, N));
        INNR_HIP_CHECK(ctx_sync(c));
        return INNR_OK;
    }();
    if (st != INNR_OK) {
        (void)hipStreamSynchronize(c->stream);
        innr_batch_free(nb);
        return st;
    }
    take_store(b, nb);
    invalidate_derived(b);
    return INNR_OK;
}

innr_status launch_scatter(innr_batch* b, const uint64_t* d_idx, const uint8_t* d_codes, size_t n) {
    innr_ctx* c = b->ctx;
    const size_t ti = (n + kRowsTile - 1) / kRowsTile, td = (b->D + kRowsTile - 1) / kRowsTile;
    const dim3 grid((unsigned)std::min<size_t>(ti, 1u << 20), (unsigned)std::min<size_t>(td, 1024));
    scatter_rows_u8_pdx_kernel<<<grid, dim3(kRowsTile, 8), 0, c->stream>>>(b->C8, b->ldN, (uint32_t)b->N, (uint32_t)b->D, b->index_base,
                                                                           d_idx, n, d_codes, c->rows_flag.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

innr_status update(innr_batch* b, const uint64_t* idx, const Source& s, size_t n, size_t D, const char* who) {
    INNR_TRY(need_code_batch(b, who));
    INNR_TRY(need_dim(b, D, who));
    if (n == 0) return INNR_OK;
    if (!idx || (s.null() && D)) {
        set_error("%s: null indices / rows", who);
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(need_room(b, n, who));  // (more indices than that cannot be distinct ones of this batch either)
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    // pass 1: every index of the call, before anything is written
    const size_t bits_bytes = std::max<size_t>((b->N + 31) / 32 * sizeof(uint32_t), 16);
    INNR_TRY(c->rows_bits.ensure(bits_bytes));
    INNR_HIP_CHECK(hipMemsetAsync(c->rows_bits.p, 0, bits_bytes, c->stream));
    INNR_TRY(c->rows_flag.ensure(kFlagBytes));
    INNR_HIP_CHECK(hipMemsetAsync(c->rows_flag.p, 0, kFlagBytes, c->stream));
    Rounds r;
    INNR_TRY(plan_rounds(c, s, true, n, D, &r));
    if (s.host) {
        for (size_t j0 = 0; j0 < n; j0 += r.round) {
            const size_t m = std::min(r.round, n - j0);
            INNR_HIP_CHECK(copy_in(c, r.idx, idx + j0, m * sizeof(uint64_t)));
            INNR_TRY(launch_update_check(b, r.idx, m));
            if (j0 + m < n) INNR_HIP_CHECK(ctx_sync(c));  // the buffer is used again
        }
    } else {
        INNR_TRY(launch_update_check(b, idx, n));
    }
    UpdateFlag f{};
    static_assert(sizeof(UpdateFlag) == 24 && sizeof(UpdateFlag) <= kFlagBytes, "update_check_kernel's flag layout");
    INNR_HIP_CHECK(copy_out(c, &f, c->rows_flag.p, sizeof(f)));
    INNR_HIP_CHECK(ctx_sync(c));
    if (f.outside) {
        set_error("%s: index %llu lies outside this batch's range [%llu, %llu)", who, (unsigned long long)f.outside_idx,
                  (unsigned long long)b->index_base, (unsigned long long)(b->index_base + b->N));
        return INNR_E_BAD_ARG;
    }
    if (f.twice) {
        set_error("%s: index %llu occurs more than once in one call (duplicate indices are refused)", who,
                  (unsigned long long)f.twice_idx);
        return INNR_E_BAD_ARG;
    }
    if (D == 0) return INNR_OK;  // nothing to write
    // pass 2: the writes (the scatter checks the range once more; rows_flag word 0 is clean here)
    const innr_status st = [&]() -> innr_status {
        for (size_t j0 = 0; j0 < n; j0 += r.round) {
            const size_t m = std::min(r.round, n - j0);
            const uint64_t* d_idx = idx + j0;
            if (s.host) {
                INNR_HIP_CHECK(copy_in(c, r.idx, idx + j0, m * sizeof(uint64_t)));
                d_idx = r.idx;
            }
            const uint8_t* d_codes = nullptr;
            INNR_TRY(round_codes(b, s, r, j0, m, &d_codes));
            INNR_TRY(launch_scatter(b, d_idx, d_codes, m));
            if (s.host && j0 + m < n) INNR_HIP_CHECK(ctx_sync(c));
        }
        uint32_t bad = 0;  // set only if the indices changed under the call
        INNR_HIP_CHECK(copy_out(c, &bad, c->rows_flag.p, sizeof(bad)));
        INNR_HIP_CHECK(ctx_sync(c));
        if (bad) {
            set_error("%s: the indices changed between the check and the writes (rows of valid indices were written)", who);
            return INNR_E_BAD_ARG;
        }
        return INNR_OK;
    }();
    if (st != INNR_OK) (void)hipStreamSynchronize(c->stream);
    invalidate_derived(b);  // also after a failure in pass 2: rows may have been written
    return st;
}

innr_status keep(innr_batch* b, const uint8_t* mask, size_t* out_n, bool host) {
    const char* who = "keep_codes";
    INNR_TRY(need_code_batch(b, who));
    if (out_n) *out_n = b->N;
    if (b->N == 0) return INNR_OK;
    if (!mask) {
        set_error("%s: mask is null", who);
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
    INNR_TRY(alloc_batch_u8(c, npass, b->D, b->alpha, b->offset, &nb));
    const innr_status st = [&]() -> innr_status {
        if (npass && b->D) {
            INNR_TRY(c->rows_map.ensure(npass * sizeof(uint32_t)));
            INNR_TRY(gather_passing_u8(b, nb->C8, nb->ldN, c->rows_map.as<uint32_t>()));
        }
        INNR_HIP_CHECK(ctx_sync(c));
        return INNR_OK;
    }();
    if (st != INNR_OK) {
        (void)hipStreamSynchronize(c->stream);
        innr_batch_free(nb);
        return st;
    }
    take_store(b, nb);
    invalidate_derived(b);
    if (out_n) *out_n = b->N;
    return INNR_OK;
}

}  // namespace

innr_status innr_batch_append_codes(innr_batch* b, const uint8_t* codes, size_t n, size_t D) {
    return append(b, Source{codes, nullptr, true}, n, D, "append_codes");
}
innr_status innr_batch_append_codes_dev(innr_batch* b, const uint8_t* d_codes, size_t n, size_t D) {
    return append(b, Source{d_codes, nullptr, false}, n, D, "append_codes");
}
innr_status innr_batch_update_codes(innr_batch* b, const uint64_t* idx, const uint8_t* codes, size_t n, size_t D) {
    return update(b, idx, Source{codes, nullptr, true}, n, D, "update_codes");
}
innr_status innr_batch_update_codes_dev(innr_batch* b, const uint64_t* d_idx, const uint8_t* d_codes, size_t n, size_t D) {
    return update(b, d_idx, Source{d_codes, nullptr, false}, n, D, "update_codes");
}
innr_status innr_batch_keep_codes(innr_batch* b, const uint8_t* mask, size_t* out_n) { return keep(b, mask, out_n, true); }
innr_status innr_batch_keep_codes_dev(innr_batch* b, const uint8_t* d_mask, size_t* out_n) { return keep(b, d_mask, out_n, false); }
innr_status innr_batch_append_quantized(innr_batch* b, const float* rows, size_t n, size_t D) {
    return append(b, Source{nullptr, rows, true}, n, D, "append_quantized");
}
innr_status innr_batch_append_quantized_dev(innr_batch* b, const float* d_rows, size_t n, size_t D) {
    return append(b, Source{nullptr, d_rows, false}, n, D, "append_quantized");
}
innr_status innr_batch_update_quantized(innr_batch* b, const uint64_t* idx, const float* rows, size_t n, size_t D) {
    return update(b, idx, Source{nullptr, rows, true}, n, D, "update_quantized");
}
innr_status innr_batch_update_quantized_dev(innr_batch* b, const uint64_t* d_idx, const float* d_rows, size_t n, size_t D) {
    return update(b, d_idx, Source{nullptr, d_rows, false}, n, D, "update_quantized");
}
