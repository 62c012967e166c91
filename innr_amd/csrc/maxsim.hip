// maxsim.hip -- maxsim over a document corpus: the innr_docs handle and every innr_maxsim_* / innr_docs_* entry point
// (include/innr_hip.h) over the kernels of kernels_maxsim.h. A translation unit of its own; the rest of the library reaches it
// through the C ABI and maxsim_topk_impl (api_internal.h).
#include <stdio.h>

#include <memory>

#include "api_internal.h"
#include "kernels_maxsim.h"

// kernel_of(Inst) of the recorded maxsim families (api_internal.h: Inst, launch_kernel)
template <int COS, int NQ, int MULTI> constexpr auto kernel_of(Inst<kLaunchMsScan, COS, NQ, MULTI>) { return &maxsim_scan_kernel<COS != 0, NQ, MULTI != 0>; }
template <int COS, int NB, int NQ> constexpr auto kernel_of(Inst<kLaunchMsTile, COS, NB, NQ>) { return &maxsim_mfma_tile_kernel<COS != 0, NB, NQ>; }
template <int COS> constexpr auto kernel_of(Inst<kLaunchMsGeneric, COS>) { return &maxsim_mfma_kernel<COS != 0>; }
template <int COS, int NQ, int MULTI> constexpr auto kernel_of(Inst<kLaunchMsRerank, COS, NQ, MULTI>) { return &maxsim_rerank_kernel<COS != 0, NQ, MULTI != 0>; }

// ---- maxsim over a document corpus (maxsim.rs) -------------------------------------------------------------
static innr_status alloc_docs(innr_ctx* ctx, size_t ndocs, size_t T, size_t dim, innr_docs** out) {
    if (!ctx || !out) return INNR_E_BAD_ARG;
    if (ndocs >= 0xFFFFFFFFull || dim > 1024 || T > 65535) {
        set_error("maxsim corpus limits: docs < 2^32, dim <= 1024, T <= 65535 (got %zu, %zu, %zu)", ndocs, dim, T);
        return INNR_E_UNSUPPORTED;
    }
    INNR_ENTER(ctx);
    innr_docs* d = new (std::nothrow) innr_docs();
    if (!d) return INNR_E_OOM;
    d->ctx = ctx;
    d->ndocs = ndocs;
    d->T = T;
    d->dim = dim;
    const size_t bytes = std::max<size_t>(ndocs * T * dim, 1) * sizeof(float);
    hipError_t e = hipMalloc((void**)&d->tok, bytes);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for document tokens failed: %s", bytes, hipGetErrorString(e));
        delete d;
        return INNR_E_OOM;
    }
    d->tok_bytes = bytes;
    *out = d;
    return INNR_OK;
}

innr_status innr_maxsim_upload(innr_ctx* ctx, const float* tokens, const uint32_t* doc_len, size_t ndocs, size_t T,
                               size_t dim, innr_docs** out) {
    if ((!tokens && ndocs * T * dim) || !ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_docs* d = nullptr;
    INNR_TRY(alloc_docs(ctx, ndocs, T, dim, &d));
    hipError_t e = hipSuccess;
    if (ndocs * T * dim) e = hipMemcpy(d->tok, tokens, ndocs * T * dim * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && doc_len && ndocs) {
        e = hipMalloc((void**)&d->doc_len, ndocs * sizeof(uint32_t));
        if (e == hipSuccess) d->doc_len_bytes = ndocs * sizeof(uint32_t);
        if (e == hipSuccess) e = hipMemcpy(d->doc_len, doc_len, ndocs * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        set_error("maxsim upload failed: %s", hipGetErrorString(e));
        innr_docs_free(d);
        return INNR_E_HIP;
    }
    *out = d;
    return INNR_OK;
}

innr_status innr_maxsim_generate(innr_ctx* ctx, size_t ndocs, size_t T, size_t dim, uint64_t seed, uint64_t row0,
                                 innr_docs** out) {
    if (!ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_docs* d = nullptr;
    INNR_TRY(alloc_docs(ctx, ndocs, T, dim, &d));
    const size_t ntok = ndocs * T;
    if (ntok && dim) {
        generate_tokens_kernel<<<(unsigned)((ntok + 255) / 256), 256, 0, ctx->stream>>>(d->tok, ntok, (uint32_t)dim, seed, row0);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("maxsim generate failed: %s", hipGetErrorString(e));
            innr_docs_free(d);
            return INNR_E_HIP;
        }
    }
    *out = d;
    return INNR_OK;
}

void innr_docs_free(innr_docs* d) {
    if (!d) return;
    CtxGuard _guard(d->ctx);
    if (d->ctx) {
        (void)hipSetDevice(d->ctx->device);
        (void)ctx_sync(d->ctx);
    }
    if (d->tok) (void)hipFree(d->tok);
    if (d->doc_len) (void)hipFree(d->doc_len);
    if (d->tok_inv) (void)hipFree(d->tok_inv);
    delete d;
}

size_t innr_docs_count(const innr_docs* d) { return d ? d->ndocs : 0; }

innr_status innr_docs_shape(const innr_docs* d, size_t* ndocs, size_t* T, size_t* dim, int* has_doc_len) {
    if (!d) return INNR_E_BAD_ARG;
    if (ndocs) *ndocs = d->ndocs;
    if (T) *T = d->T;
    if (dim) *dim = d->dim;
    if (has_doc_len) *has_doc_len = d->doc_len ? 1 : 0;
    return INNR_OK;
}

// tokens[docs*T*dim] (the layout innr_maxsim_upload takes) and, when the corpus has them, doc_len[docs]
innr_status innr_docs_download(innr_docs* d, float* tokens, uint32_t* doc_len) {
    if (!d || (!tokens && d->ndocs * d->T * d->dim)) return INNR_E_BAD_ARG;
    INNR_ENTER(d->ctx);
    const size_t n = d->ndocs * d->T * d->dim;
    if (n) INNR_HIP_CHECK(hipMemcpyAsync(tokens, d->tok, n * sizeof(float), hipMemcpyDeviceToHost, d->ctx->stream));
    if (doc_len && d->doc_len && d->ndocs)
        INNR_HIP_CHECK(hipMemcpyAsync(doc_len, d->doc_len, d->ndocs * sizeof(uint32_t), hipMemcpyDeviceToHost, d->ctx->stream));
    INNR_HIP_CHECK(ctx_sync(d->ctx));
    return INNR_OK;
}

innr_status innr_docs_set_index_base(innr_docs* d, uint64_t base) {
    if (!d) return INNR_E_BAD_ARG;
    d->index_base = base;
    return INNR_OK;
}

innr_status innr_docs_memory(const innr_docs* d, uint64_t* corpus_bytes, uint64_t* derived) {
    if (!d) {
        set_error("corpus is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(d->ctx);
    if (corpus_bytes) *corpus_bytes = d->tok_bytes + d->doc_len_bytes;
    if (derived) *derived = d->tok_inv_bytes;
    return INNR_OK;
}

// ---- query staging: tokens zero-padded to a multiple of kMsQ in c->q_row, exact squared norms in c->q_norm (cosine)
static innr_status maxsim_stage_query(innr_docs* d, int cosine, const float* qtok, size_t Tq) {
    innr_ctx* c = d->ctx;
    const size_t dim = d->dim, Tq_pad = round_up(Tq, kMsQ);
    INNR_TRY(c->q_row.ensure(Tq_pad * dim * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(2 * Tq_pad * sizeof(float)));  // [Tq_pad] squared norms, [Tq_pad] 1/norm (MFMA engine)
    INNR_HIP_CHECK(hipMemsetAsync(c->q_row.p, 0, Tq_pad * dim * sizeof(float), c->stream));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, qtok, Tq * dim * sizeof(float)));
    if (cosine) {
        query_token_sq_kernel<<<(unsigned)((Tq_pad + 63) / 64), 64, 0, c->stream>>>(c->q_row.as<float>(), (uint32_t)Tq_pad,
                                                                                   (uint32_t)dim, c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
    }
    return INNR_OK;
}

// exact engine over `nslots` documents (all of them, or the ones listed in doc_ids) -> out[slot]; query staged
static innr_status maxsim_scan_exact(innr_docs* d, int cosine, size_t Tq, const uint32_t* doc_ids, size_t nslots, float* out) {
    innr_ctx* c = d->ctx;
    const size_t dim = d->dim;
    uint32_t Tp = 1;
    while (Tp < d->T && Tp < 64) Tp <<= 1;
    const uint32_t docs_per_wave = 64 / Tp;
    const size_t nwaves_needed = (nslots + docs_per_wave - 1) / docs_per_wave;
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((nwaves_needed + 3) / 4, (size_t)c->num_cus * 2));
    const size_t qpk_floats = (size_t)kMsQ * std::max<size_t>(dim, 8) * 4;
    INNR_TRY(c->q_kmajor.ensure((qpk_floats + kMsQ) * sizeof(float)));  // packed query (either engine) + sqrt of the pass' squared norms
    float* qpk = c->q_kmajor.as<float>();
    float* saa = qpk + qpk_floats;
    for (size_t p0 = 0; p0 < Tq; p0 += kMsQ) {
        const uint32_t nq = (uint32_t)std::min<size_t>(kMsQ, Tq - p0);
        const float* qp = c->q_row.as<float>() + p0 * dim;
        const float* aa = c->q_norm.as<float>() + p0;
        if (cosine) sqrt_kernel<<<1, kMsQ, 0, c->stream>>>(aa, nq, saa);
        // (every instantiation has a row in tests/test_gpu_kernel_variants.py: MS_SCAN)
        dispatch([&](auto cosv, auto nqv, auto multi) {
            const unsigned npk = (unsigned)(dim / 4) * nqv * 4;
            if (npk) maxsim_pack_query_kernel<<<(npk + 255) / 256, 256, 0, c->stream>>>(qp, (uint32_t)nqv, (uint32_t)dim, qpk);
            launch_kernel(c, Inst<kLaunchMsScan, cosv, nqv, multi>(), {blocks, kMsThreads}, d->tok, d->doc_len, (uint32_t)nslots,
                          (uint32_t)d->T, Tp, (uint32_t)dim, qp, qpk, nq, cosine ? aa : nullptr, out, out, p0 == 0, doc_ids,
                          cosine ? saa : nullptr);
        }, flag(cosine), one_of<8, 16, 32>(nq <= 8 ? 8 : (nq <= 16 ? 16 : 32)), flag(d->T > 64));
        INNR_HIP_CHECK(hipGetLastError());
    }
    return INNR_OK;
}

// exact scores of every document into c->scores (device); q tokens uploaded from the host
static innr_status maxsim_scores_dev(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim) {
    innr_ctx* c = d->ctx;
    if (dim != d->dim) {  // maxsim.rs:103-110
        set_error("dimension mismatch (doc): query dim %zu, document dim %zu", dim, d->dim);
        return INNR_E_DIM_MISMATCH;
    }
    INNR_TRY(c->scores.ensure(std::max<size_t>(d->ndocs, 1) * sizeof(float)));
    float* out = c->scores.as<float>();
    if (Tq == 0 || d->T == 0 || d->ndocs == 0) {  // maxsim.rs:97-99: empty query or empty documents -> 0.0
        INNR_HIP_CHECK(hipMemsetAsync(out, 0, std::max<size_t>(d->ndocs, 1) * sizeof(float), c->stream));
        return INNR_OK;
    }
    INNR_TRY(maxsim_stage_query(d, cosine, qtok, Tq));
    return maxsim_scan_exact(d, cosine, Tq, nullptr, d->ndocs, out);
}

innr_status innr_maxsim_scores(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, float* out) {
    if (!d || (!out && d->ndocs) || (!qtok && Tq * dim)) return INNR_E_BAD_ARG;
    INNR_ENTER(d->ctx);
    INNR_TRY(maxsim_scores_dev(d, cosine, qtok, Tq, dim));
    if (d->ndocs) {
        INNR_HIP_CHECK(copy_out(d->ctx, out, d->ctx->scores.p, d->ndocs * sizeof(float)));
        INNR_HIP_CHECK(ctx_sync(d->ctx));
    }
    return INNR_OK;
}

// top-KP of the dense score array c->scores -> c->sel / c->sel_cnt (order: score desc, document index asc -- the
// caller's stable sort in the reference example, examples/maxsim_colbert.rs:186-187)
static innr_status maxsim_select(innr_docs* d, uint32_t KP, const float* sc) {
    innr_ctx* c = d->ctx;
    const uint32_t cap = exact_cap(KP);
    const size_t nchunks = (d->ndocs + 255) / 256;
    size_t nslots = round_up(cap_scan_slots(c, std::min<size_t>(nchunks, (size_t)c->num_cus * 8)), 4);
    const uint32_t cps = (uint32_t)((nchunks + nslots - 1) / nslots);
    INNR_TRY(c->lists.ensure(nslots * cap * sizeof(uint64_t)));
    INNR_TRY(c->counts.ensure(nslots * sizeof(uint32_t)));
    const unsigned nb = (unsigned)(nslots / 4);
    uint64_t* lists = c->lists.as<uint64_t>();
    uint32_t* counts = c->counts.as<uint32_t>();
    uint32_t* err = c->flags.as<uint32_t>();
    dispatch([&](auto rr) {
        record_scan(c, kScanDense, 1, INNR_METRIC_DOT, rr, false, cps, nslots, 1);
        dense_filter_kernel<rr><<<nb, 256, 0, c->stream>>>(sc, (uint32_t)d->ndocs, lists, counts, KP, cps, err);
    }, rr_scan(cap));
    INNR_HIP_CHECK(hipGetLastError());
    return run_select(c, lists, counts, (uint32_t)nslots, 1, cap, KP, 1);
}

// per-token 1/norm and the corpus-wide maximum token norm, computed once per corpus (MFMA engine)
static innr_status maxsim_ensure_token_norms(innr_docs* d) {
    if (d->tok_inv) return INNR_OK;
    innr_ctx* c = d->ctx;
    const size_t ntok = d->ndocs * d->T;
    hipError_t e = hipMalloc((void**)&d->tok_inv, (ntok + 64) * sizeof(float));  // + slack: tiles read 4-float groups past T
    if (e != hipSuccess) {
        d->tok_inv = nullptr;
        set_error("hipMalloc(%zu bytes) for token norms failed: %s", ntok * sizeof(float), hipGetErrorString(e));
        return INNR_E_OOM;
    }
    d->tok_inv_bytes = (ntok + 64) * sizeof(float);
    INNR_TRY(c->misc.ensure(4096));
    INNR_HIP_CHECK(hipMemsetAsync(c->misc.p, 0, 4, c->stream));
    maxsim_token_norms_kernel<<<(unsigned)((ntok + 255) / 256), 256, 0, c->stream>>>(d->tok, ntok, (uint32_t)d->dim, d->tok_inv,
                                                                                     c->misc.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t bits = 0;
    INNR_HIP_CHECK(copy_out(c, &bits, c->misc.p, 4));
    INNR_HIP_CHECK(ctx_sync(c));
    memcpy(&d->max_norm, &bits, 4);
    return INNR_OK;
}

static bool maxsim_mfma_eligible(const innr_docs* d, size_t Tq) {
    return d->T > 16 && d->dim % 8 == 0 && d->dim >= 8 && d->dim <= 512 && Tq > 0 && d->ndocs > 0;
}

// MFMA engine: approximate scores of every document (c->scores), top-KP by approximate score, exact re-score of
// those KP documents, proof. Results in c->out_idx / c->out_score; *proven = false -> the caller redoes it exactly.
// error bound of the approximate document score: per (token, query token) pair the MFMA fma chain and
// the reference's mul-then-add 4-way sum differ by <= (2 dim + 8) u |q_j| |d_i|; the max over tokens is 1-Lipschitz; the
// two Tq-term sums (tree here, sequential there) add <= 2 Tq u sum_j |best_j|. Returns false when no finite bound exists.
static bool maxsim_error_bound(const innr_docs* d, int cosine, const float* qtok, size_t Tq, float* E) {
    const size_t dim = d->dim;
    double qsum = 0.0;
    for (size_t j = 0; j < Tq; ++j) {
        double ss = 0.0;
        for (size_t e = 0; e < dim; ++e) ss += (double)qtok[j * dim + e] * (double)qtok[j * dim + e];
        qsum += std::sqrt(ss);
    }
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double Ed = cosine ? 1.05 * (2.0 * dim + 32.0 + 2.0 * Tq) * u * (double)Tq
                             : 1.05 * (2.0 * dim + 8.0 + 2.0 * Tq) * u * (double)d->max_norm * qsum;
    if (!(Ed - Ed == 0.0) || Ed > 3.0e38) return false;
    *E = (float)(Ed * 1.0000002);
    return true;
}

// Approximate scores of `nqr` queries (1, 2 or 4; more than one only with <= 32 tokens each and a tile-unrolled dim)
// for every document: c->scores[qi * ndocs + doc]. Query qi = qtoks[qi], Tqs[qi] tokens.
static innr_status maxsim_approx(innr_docs* d, int cosine, const float* const* qtoks, const size_t* Tqs, int nqr) {
    innr_ctx* c = d->ctx;
    const size_t dim = d->dim;
    size_t Tq_pad = 0;
    for (int qi = 0; qi < nqr; ++qi) Tq_pad = std::max(Tq_pad, round_up(Tqs[qi], kMsQ));
    const size_t rows = (size_t)nqr * Tq_pad;  // query qi occupies rows [qi*Tq_pad, (qi+1)*Tq_pad), zero padded
    INNR_TRY(c->q_row.ensure(rows * dim * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(2 * rows * sizeof(float)));
    INNR_HIP_CHECK(hipMemsetAsync(c->q_row.p, 0, rows * dim * sizeof(float), c->stream));
    for (int qi = 0; qi < nqr; ++qi)
        INNR_HIP_CHECK(copy_in(c, c->q_row.as<float>() + (size_t)qi * Tq_pad * dim, qtoks[qi], Tqs[qi] * dim * sizeof(float)));
    float* qscale = c->q_norm.as<float>() + rows;
    if (cosine) {
        query_token_sq_kernel<<<(unsigned)((rows + 63) / 64), 64, 0, c->stream>>>(c->q_row.as<float>(), (uint32_t)rows,
                                                                                 (uint32_t)dim, c->q_norm.as<float>());
        maxsim_query_scale_kernel<<<(unsigned)((rows + 63) / 64), 64, 0, c->stream>>>(c->q_norm.as<float>(), (uint32_t)rows, qscale);
        INNR_HIP_CHECK(hipGetLastError());
    }
    INNR_TRY(c->scores.ensure((size_t)nqr * d->ndocs * sizeof(float)));
    INNR_TRY(c->q_kmajor.ensure((size_t)nqr * kMsQ * std::max<size_t>(dim, 8) * sizeof(float) * 4));
    // [0,8K) norm scratch, [8K,16K) candidate ids / exact scores (maxsim_post), [16K,..) per-pass token counts: 16 bytes
    // per pass of kMsQ query tokens -- sized from the pass count, a long query must not run into its neighbours
    const size_t npass = Tq_pad / kMsQ;
    INNR_TRY(c->misc.ensure(16384 + npass * 16 + 64));
    float* qB = c->q_kmajor.as<float>();
    float* approx = c->scores.as<float>();
    const size_t qb_stride = dim * 32;  // floats per packed query: [dim/8][64][4]
    const size_t lds = (size_t)nqr * qb_stride * sizeof(float);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((d->ndocs + 3) / 4, (size_t)c->num_cus * 8));
    const bool tiled = dim % 32 == 0 && dim <= 128 && !d->ctx->tune.maxsim_generic;
    uint32_t* nq_dev = reinterpret_cast<uint32_t*>(static_cast<char*>(c->misc.p) + 16384);  // token counts, 4 per pass
    for (size_t p0 = 0; p0 < Tq_pad; p0 += kMsQ) {
        uint32_t nq_host[4] = {0, 0, 0, 0};
        for (int qi = 0; qi < nqr; ++qi) {
            nq_host[qi] = Tqs[qi] > p0 ? (uint32_t)std::min<size_t>(kMsQ, Tqs[qi] - p0) : 0u;
            maxsim_pack_mfma_kernel<<<(unsigned)((dim * 32 + 255) / 256), 256, 0, c->stream>>>(
                c->q_row.as<float>() + ((size_t)qi * Tq_pad + p0) * dim, (uint32_t)dim, qB + (size_t)qi * qb_stride);
        }
        INNR_HIP_CHECK(copy_in(c, nq_dev + 4 * (p0 / kMsQ), nq_host, sizeof(nq_host)));
        const uint32_t* nqp = nq_dev + 4 * (p0 / kMsQ);
        const float* tok_inv = cosine ? d->tok_inv : nullptr;
        const float* qsc = cosine ? qscale + p0 : nullptr;
        // (every instantiation has a row in tests/test_gpu_kernel_variants.py: MS_TILE, MS_GENERIC)
        if (tiled) {  // NB = dim / 32 K-blocks; four, two or one query a pass
            dispatch([&](auto cosv, auto nb, auto nqv) {
                launch_kernel(c, Inst<kLaunchMsTile, cosv, nb, nqv>(), {blocks, kMsThreads, lds, (uint32_t)nqr}, d->tok, d->doc_len, tok_inv,
                              (uint32_t)d->ndocs, (uint32_t)d->T, qB, nqp, qsc, approx, approx, p0 == 0);
            }, flag(cosine), one_of<1, 2, 3, 4>(dim / 32), one_of<4, 2, 1>(nqr));
        } else if (nqr != 1) {
            set_error("internal: multi-query maxsim needs the tile-unrolled kernel");
            return INNR_E_UNSUPPORTED;
        } else {
            dispatch([&](auto cosv) {
                launch_kernel(c, Inst<kLaunchMsGeneric, cosv>(), {blocks, kMsThreads, lds}, d->tok, d->doc_len, tok_inv, (uint32_t)d->ndocs,
                              (uint32_t)d->T, (uint32_t)dim, qB, nq_host[0], qsc, approx, approx, p0 == 0);
            }, flag(cosine));
        }
        INNR_HIP_CHECK(hipGetLastError());
    }
    return INNR_OK;
}

// Second half of the MFMA engine for ONE query: top-KP of its approximate scores, exact re-score of those documents,
// final order + proof. Results at c->out_idx / c->out_score + out_off; *proven = false -> the caller redoes it exactly.
static innr_status maxsim_post(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t kout, float E,
                               const float* approx, size_t out_off, bool* proven, uint32_t* kp_out) {
    innr_ctx* c = d->ctx;
    const uint32_t KP = pick_kp(kout, 16);
    *kp_out = KP;
    INNR_TRY(maxsim_select(d, KP, approx));
    INNR_TRY(c->misc.ensure(16384));  // KP <= 256: ids + exact scores fit behind the first 8 KiB
    uint32_t* ids = reinterpret_cast<uint32_t*>(static_cast<char*>(c->misc.p) + 8192);
    float* exact = reinterpret_cast<float*>(ids + KP);
    maxsim_cand_ids_kernel<<<(KP + 255) / 256, 256, 0, c->stream>>>(c->sel.as<uint64_t>(), c->sel_cnt.as<uint32_t>(), KP, ids);
    INNR_HIP_CHECK(hipGetLastError());
    const size_t ncand = std::min<size_t>(KP, d->ndocs);
    INNR_TRY(maxsim_stage_query(d, cosine, qtok, Tq));  // the exact engine reads the query from c->q_row / c->q_norm
    INNR_TRY(maxsim_scan_exact(d, cosine, Tq, ids, ncand, exact));
    uint32_t* flag = c->flags.as<uint32_t>() + 64;
    maxsim_finish_kernel<<<1, 256, 0, c->stream>>>(c->sel.as<uint64_t>(), c->sel_cnt.as<uint32_t>(), exact, (uint32_t)kout,
                                                   (uint32_t)d->ndocs, E, d->index_base, c->out_idx.as<uint64_t>() + out_off,
                                                   c->out_score.as<float>() + out_off, flag);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t ok = 0;
    INNR_HIP_CHECK(copy_out(c, &ok, flag, 4));
    INNR_HIP_CHECK(ctx_sync(c));
    *proven = ok != 0;
    return INNR_OK;
}

// exact engine for one query: all-document scores -> top-k at c->out_idx / c->out_score + out_off
static innr_status maxsim_topk_exact(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t kout, size_t out_off,
                                     uint32_t* kp_out) {
    innr_ctx* c = d->ctx;
    INNR_TRY(maxsim_scores_dev(d, cosine, qtok, Tq, d->dim));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    if (kout > INNR_MAX_K) {  // more results than a candidate list holds: sort all document scores (cf. knn_full_sort)
        size_t tmp_bytes = 0;
        INNR_HIP_CHECK(full_sort_scratch_bytes(d->ndocs, &tmp_bytes));
        INNR_TRY(c->sort_keys.ensure((d->ndocs + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
        INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        uint64_t* keys = c->sort_keys.as<uint64_t>();
        INNR_HIP_CHECK(full_sort_scores(c->scores.as<float>(), d->ndocs, false, keys, keys + d->ndocs, c->sort_tmp.p, tmp_bytes,
                                        c->stream, nullptr, kout));
        INNR_TRY(emit_results(c, keys + d->ndocs, 0, 1, kout, false, d->index_base, c->out_idx.as<uint64_t>() + out_off,
                              c->out_score.as<float>() + out_off));
        *kp_out = (uint32_t)d->ndocs;
        return INNR_OK;
    }
    const uint32_t KP = pick_kp(kout, 0);
    *kp_out = KP;
    INNR_TRY(maxsim_select(d, KP, c->scores.as<float>()));
    return emit_results(c, c->sel.as<uint64_t>(), KP, 1, kout, false, d->index_base, c->out_idx.as<uint64_t>() + out_off,
                        c->out_score.as<float>() + out_off);
}

// to_host == false (the sharded call): the result stays on the device, at c->out_idx / c->out_score [*out_k]
namespace innr {
innr_status maxsim_topk_impl(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, size_t k, int engine,
                             uint64_t* out_doc, float* out_score, size_t* out_k, innr_knn_stats* stats, bool to_host) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!d || !out_k || (!qtok && Tq * dim)) return INNR_E_BAD_ARG;
    if (engine != INNR_KNN_AUTO && engine != INNR_KNN_EXACT && engine != INNR_KNN_MFMA) return INNR_E_BAD_ARG;
    *out_k = 0;
    innr_ctx* c = d->ctx;
    INNR_ENTER(c);
    if (dim != d->dim && Tq && d->T) {
        set_error("dimension mismatch (doc): query dim %zu, document dim %zu", dim, d->dim);
        return INNR_E_DIM_MISMATCH;
    }
    if (d->ndocs == 0 || k == 0) return INNR_OK;
    const size_t kout = std::min(k, d->ndocs);  // beyond INNR_MAX_K: the exact engine sorts all document scores
    if (to_host && (!out_doc || !out_score)) return INNR_E_BAD_ARG;
    const bool eligible = maxsim_mfma_eligible(d, Tq) && kout <= INNR_MAX_K && pick_kp(kout, 16) <= 256;
    if (engine == INNR_KNN_MFMA && !eligible) {
        set_error("maxsim MFMA engine needs T > 16, dim %% 8 == 0, 8 <= dim <= 512, a non-empty query and k <= 240");
        return INNR_E_UNSUPPORTED;
    }
    const bool use_mfma = engine == INNR_KNN_MFMA || (engine == INNR_KNN_AUTO && eligible && d->ndocs >= 4096);
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    bool proven = false;
    uint32_t KP = 0;
    int used = INNR_KNN_EXACT;
    float scan_ms = 0.0f;
    INNR_TRY(c->out_idx.ensure(kout * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(kout * sizeof(float)));
    if (use_mfma) {
        float E = 0.0f;
        INNR_TRY(maxsim_ensure_token_norms(d));
        // a non-finite token somewhere, or no finite bound: nothing can be proven, go straight to the exact engine
        if ((d->max_norm - d->max_norm == 0.0f) && maxsim_error_bound(d, cosine, qtok, Tq, &E)) {
            INNR_TRY(maxsim_approx(d, cosine, &qtok, &Tq, 1));
            INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
            INNR_TRY(maxsim_post(d, cosine, qtok, Tq, kout, E, c->scores.as<float>(), 0, &proven, &KP));
        }
        if (proven) {
            used = INNR_KNN_MFMA;
            (void)hipEventElapsedTime(&scan_ms, c->ev[2], c->ev[3]);
        }
    }
    if (!proven) {
        INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
        INNR_TRY(maxsim_topk_exact(d, cosine, qtok, Tq, kout, 0, &KP));
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
    INNR_TRY(check_errflag(c));
    if (to_host) {
        INNR_HIP_CHECK(copy_out(c, out_doc, c->out_idx.p, kout * sizeof(uint64_t)));
        INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, kout * sizeof(float)));
    }
    INNR_HIP_CHECK(ctx_sync(c));
    *out_k = kout;
    if (stats) {
        stats->engine = used;
        stats->candidates_kept = KP;
        stats->queries_fallback = (use_mfma && !proven) ? 1u : 0u;
        float ms = 0.0f;
        if (used == INNR_KNN_MFMA) stats->gemm_ms = scan_ms;  // the approximate scan kernel(s)
        else if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) stats->gemm_ms = ms;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}
}  // namespace innr

innr_status innr_maxsim_topk(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, size_t k, int engine,
                             uint64_t* out_doc, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    return maxsim_topk_impl(d, cosine, qtok, Tq, dim, k, engine, out_doc, out_score, out_k, stats, true);
}

// Several queries against the same corpus in one call (an addition: the reference scores one (query, document) pair
// per call). Queries are taken 4 (then 2, then 1) per corpus pass on the MFMA engine, which turns the scan from
// HBM-bound into MFMA-bound; every query's result is the same as innr_maxsim_topk's.
// qtoks: Q queries of Tq_stride*dim floats each, query i using its first tq[i] tokens (tq == NULL: all Tq_stride).
innr_status innr_maxsim_topk_multi(innr_docs* d, int cosine, const float* qtoks, size_t Q, const uint32_t* tq,
                                   size_t Tq_stride, size_t dim, size_t k, int engine, uint64_t* out_doc, float* out_score,
                                   size_t* out_k, innr_knn_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!d || !out_k || (!qtoks && Q * Tq_stride * dim)) return INNR_E_BAD_ARG;
    if (engine != INNR_KNN_AUTO && engine != INNR_KNN_EXACT && engine != INNR_KNN_MFMA) return INNR_E_BAD_ARG;
    *out_k = 0;
    innr_ctx* c = d->ctx;
    INNR_ENTER(c);
    if (dim != d->dim && Tq_stride && d->T) {
        set_error("dimension mismatch (doc): query dim %zu, document dim %zu", dim, d->dim);
        return INNR_E_DIM_MISMATCH;
    }
    if (d->ndocs == 0 || k == 0 || Q == 0) return INNR_OK;
    const size_t kout = std::min(k, d->ndocs);
    if (!out_doc || !out_score) return INNR_E_BAD_ARG;
    std::vector<size_t> Tqs(Q);
    size_t tq_max = 0, tq_min = Tq_stride;
    for (size_t i = 0; i < Q; ++i) {
        Tqs[i] = tq ? std::min<size_t>(tq[i], Tq_stride) : Tq_stride;
        tq_max = std::max(tq_max, Tqs[i]);
        tq_min = std::min(tq_min, Tqs[i]);
    }
    const bool eligible = tq_min > 0 && maxsim_mfma_eligible(d, tq_min) && kout <= INNR_MAX_K && pick_kp(kout, 16) <= 256;
    if (engine == INNR_KNN_MFMA && !eligible) {
        set_error("maxsim MFMA engine needs T > 16, dim %% 8 == 0, 8 <= dim <= 512, non-empty queries and k <= 240");
        return INNR_E_UNSUPPORTED;
    }
    bool use_mfma = engine == INNR_KNN_MFMA || (engine == INNR_KNN_AUTO && eligible && d->ndocs >= 4096);
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    INNR_TRY(c->out_idx.ensure(Q * kout * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(Q * kout * sizeof(float)));
    if (use_mfma) {
        INNR_TRY(maxsim_ensure_token_norms(d));
        if (!(d->max_norm - d->max_norm == 0.0f)) use_mfma = false;  // a non-finite token: nothing can be proven
    }
    // groups of 4 / 2 queries share a corpus pass when the tile-unrolled kernel applies and every query fits one pass
    const bool groupable = use_mfma && dim % 32 == 0 && dim <= 128 && tq_max <= (size_t)kMsQ && !d->ctx->tune.maxsim_generic;
    std::vector<uint8_t> done(Q, 0);
    uint32_t KP = 0, nfallback = 0;
    float scan_ms = 0.0f;
    for (size_t i = 0; use_mfma && i < Q;) {
        const int g = !groupable ? 1 : (Q - i >= 4 ? 4 : (Q - i >= 2 ? 2 : 1));
        const float* ptrs[4];
        size_t tqs[4];
        float E[4];
        bool bounded = true;
        for (int j = 0; j < g; ++j) {
            ptrs[j] = qtoks + (i + j) * Tq_stride * dim;
            tqs[j] = Tqs[i + j];
            bounded = bounded && maxsim_error_bound(d, cosine, ptrs[j], tqs[j], &E[j]);
        }
        if (bounded) {
            INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
            INNR_TRY(maxsim_approx(d, cosine, ptrs, tqs, g));
            INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
            for (int j = 0; j < g; ++j) {
                bool proven = false;
                INNR_TRY(maxsim_post(d, cosine, ptrs[j], tqs[j], kout, E[j], c->scores.as<float>() + (size_t)j * d->ndocs,
                                     (i + j) * kout, &proven, &KP));
                done[i + j] = proven ? 1 : 0;
            }
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) scan_ms += ms;
        }
        i += g;
    }
    for (size_t i = 0; i < Q; ++i) {  // exact engine: unproven queries, or everything when the MFMA engine is off
        if (done[i]) continue;
        if (use_mfma) ++nfallback;
        INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
        INNR_TRY(maxsim_topk_exact(d, cosine, qtoks + i * Tq_stride * dim, Tqs[i], kout, i * kout, &KP));
        if (!use_mfma) {
            INNR_HIP_CHECK(ctx_sync(c));
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) scan_ms += ms;
        }
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
    INNR_TRY(check_errflag(c));
    INNR_HIP_CHECK(copy_out(c, out_doc, c->out_idx.p, Q * kout * sizeof(uint64_t)));
    INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, Q * kout * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    *out_k = kout;
    if (stats) {
        stats->engine = use_mfma ? INNR_KNN_MFMA : INNR_KNN_EXACT;
        stats->candidates_kept = KP;
        stats->queries_fallback = nfallback;
        stats->gemm_ms = scan_ms;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}

// slots and document ids are 32-bit in the re-rank kernels; its pack and norms launches have one thread per packed float / token
static innr_status maxsim_rerank_fits(size_t Q, size_t kc, size_t Tq_stride, size_t dim) {
    const size_t stride_pad = round_up(std::max<size_t>(Tq_stride, 1), kMsQ);
    if (kc > 0xFFFFFF00ull / Q || Tq_stride > 0xFFFFFFFFull || stride_pad > ((size_t)0x7fffffff * 256) / (Q * (ms_rerank_blk(dim) / kMsQ))) {
        set_error("maxsim rerank: %zu queries x %zu candidates (x %zu query tokens) is beyond one launch", Q, kc, Tq_stride);
        return INNR_E_UNSUPPORTED;
    }
    return INNR_OK;
}

// Second stage for multi-vector corpora (an addition, the document-side twin of innr_batch_rerank): exact maxsim /
// maxsim_cosine of query j against ITS kc candidate documents, best min(k, kc) per query. Every candidate is scored
// exactly, once (maxsim_rerank_kernel: the corpus scan's arithmetic over all Q*kc pairs in one launch per 32-token pass);
// there is no approximate stage and nothing to prove. Queries as in innr_maxsim_topk_multi, candidates as in innr_batch_rerank.
innr_status innr_maxsim_rerank_dev(innr_docs* d, int cosine, const float* d_qtoks, size_t Q, const uint32_t* tq, size_t Tq_stride,
                                   size_t dim, const uint64_t* d_cand, size_t kc, size_t k, uint64_t* d_out_doc, float* d_out_score,
                                   size_t* out_k) {
    if (!d || !out_k) return INNR_E_BAD_ARG;
    *out_k = 0;
    if (dim != d->dim) {  // maxsim.rs:103-110
        set_error("dimension mismatch (doc): query dim %zu, document dim %zu", dim, d->dim);
        return INNR_E_DIM_MISMATCH;
    }
    if (d->ndocs == 0 || Q == 0 || k == 0 || kc == 0) return INNR_OK;
    if (!d_cand || !d_out_doc || !d_out_score) return INNR_E_BAD_ARG;
    INNR_TRY(maxsim_rerank_fits(Q, kc, Tq_stride, dim));
    std::unique_ptr<uint32_t[]> tqv(new (std::nothrow) uint32_t[Q]);
    if (!tqv) return INNR_E_OOM;
    size_t tq_max = 0;
    for (size_t i = 0; i < Q; ++i) {
        tqv[i] = (uint32_t)(tq ? std::min<size_t>(tq[i], Tq_stride) : Tq_stride);
        tq_max = std::max<size_t>(tq_max, tqv[i]);
    }
    if (!d_qtoks && tq_max * dim) return INNR_E_BAD_ARG;
    const size_t npass = std::max<size_t>((tq_max + kMsQ - 1) / kMsQ, 1), blk = ms_rerank_blk(dim);
    const size_t kout = std::min(k, kc);
    innr_ctx* c = d->ctx;
    INNR_ENTER(c);
    size_t tmp_bytes = 0;
    INNR_HIP_CHECK(segmented_sort_scratch_bytes(Q, kc, &tmp_bytes));
    INNR_TRY(c->sort_keys.ensure((2 * Q * kc + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
    INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    INNR_TRY(c->misc.ensure(Q * sizeof(uint32_t) + 64));
    INNR_TRY(c->q_kmajor.ensure(Q * npass * blk * sizeof(float)));
    if (cosine) INNR_TRY(c->q_norm.ensure(std::max<size_t>(2 * Q * Tq_stride, 1) * sizeof(float)));
    if (npass > 1) INNR_TRY(c->scores.ensure(Q * kc * sizeof(float)));
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    uint32_t* bad = c->flags.as<uint32_t>() + 65;  // set by the kernel for a candidate outside the corpus
    uint32_t* d_tq = c->misc.as<uint32_t>();
    INNR_HIP_CHECK(copy_in(c, d_tq, tqv.get(), Q * sizeof(uint32_t)));
    float* qpk = c->q_kmajor.as<float>();
    float* aa = cosine ? c->q_norm.as<float>() : nullptr;
    float* saa = cosine ? aa + Q * Tq_stride : nullptr;
    if (tq_max && d->T) {
        maxsim_rerank_pack_kernel<<<(unsigned)((Q * npass * blk + 255) / 256), 256, 0, c->stream>>>(
            d_qtoks, d_tq, (uint32_t)Q, (uint32_t)Tq_stride, (uint32_t)dim, (uint32_t)npass, (uint32_t)tq_max, qpk);
        if (cosine)
            maxsim_rerank_norms_kernel<<<(unsigned)((Q * Tq_stride + 255) / 256), 256, 0, c->stream>>>(
                d_qtoks, d_tq, (uint32_t)Q, (uint32_t)Tq_stride, (uint32_t)dim, aa, saa);
        INNR_HIP_CHECK(hipGetLastError());
    }
    uint32_t Tp = 1;
    while (Tp < d->T && Tp < 64) Tp <<= 1;
    const uint32_t docs_per_wave = 64 / Tp;
    const size_t units = Q * ((kc + docs_per_wave - 1) / docs_per_wave);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((units + 3) / 4, (size_t)c->num_cus * 2));
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    float* partial = c->scores.as<float>();
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    for (size_t pass = 0; pass < npass; ++pass) {
        // (every instantiation has a row in tests/test_gpu_kernel_variants.py: MS_RERANK)
        dispatch([&](auto cosv, auto nqv, auto multi) {
            launch_kernel(c, Inst<kLaunchMsRerank, cosv, nqv, multi>(), {blocks, kMsThreads, 0, (uint32_t)Q}, d->tok, d->doc_len,
                          (uint32_t)d->ndocs, (uint32_t)d->T, Tp, (uint32_t)dim, d_qtoks, (uint32_t)Tq_stride, d_tq, qpk, (uint32_t)npass,
                          (uint32_t)pass, aa, saa, d_cand, (uint32_t)Q, (uint32_t)kc, d->index_base, partial, keys, bad);
        }, flag(cosine), one_of<8, 16, 32>(ms_pass_nq((uint32_t)tq_max, (uint32_t)pass)), flag(d->T > 64));
        INNR_HIP_CHECK(hipGetLastError());
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_HIP_CHECK(segmented_topk_keys(keys, keys + Q * kc, Q, kc, kout, keys + 2 * Q * kc, c->sort_tmp.p, c->stream));
    INNR_TRY(emit_results(c, keys + Q * kc, kc, Q, kout, false, d->index_base, d_out_doc, d_out_score));
    uint32_t hbad = 0;  // the call's one host read
    INNR_HIP_CHECK(copy_out(c, &hbad, bad, 4));
    INNR_HIP_CHECK(ctx_sync(c));
    if (c->tune.trace) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess)
            fprintf(stderr, "innr: maxsim_rerank Q=%zu kc=%zu passes=%zu: scan kernels %.4f ms\n", Q, kc, npass, ms);
    }
    if (hbad) {
        set_error("maxsim rerank: a candidate index lies outside this corpus' range [%llu, %llu)", (unsigned long long)d->index_base,
                  (unsigned long long)(d->index_base + d->ndocs));
        return INNR_E_BAD_ARG;
    }
    *out_k = kout;
    return INNR_OK;
}

innr_status innr_maxsim_rerank(innr_docs* d, int cosine, const float* qtoks, size_t Q, const uint32_t* tq, size_t Tq_stride, size_t dim,
                               const uint64_t* cand, size_t kc, size_t k, uint64_t* out_doc, float* out_score, size_t* out_k) {
    if (!d || !out_k) return INNR_E_BAD_ARG;
    *out_k = 0;
    if (dim != d->dim) {
        set_error("dimension mismatch (doc): query dim %zu, document dim %zu", dim, d->dim);
        return INNR_E_DIM_MISMATCH;
    }
    if (d->ndocs == 0 || Q == 0 || k == 0 || kc == 0) return INNR_OK;
    if (!cand || !out_doc || !out_score) return INNR_E_BAD_ARG;
    INNR_TRY(maxsim_rerank_fits(Q, kc, Tq_stride, dim));  // before anything of the caller's is read
    const size_t qfloats = Q * Tq_stride * dim;
    if (!qtoks && qfloats) {
        bool needed = !tq;
        for (size_t i = 0; tq && i < Q; ++i) needed = needed || tq[i] != 0;
        if (needed) return INNR_E_BAD_ARG;
    }
    innr_ctx* c = d->ctx;
    INNR_ENTER(c);
    const size_t kout = std::min(k, kc);
    INNR_TRY(c->q_row.ensure(std::max<size_t>(qfloats, 1) * sizeof(float)));
    INNR_TRY(c->out_idx.ensure(Q * (kout + kc) * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(Q * kout * sizeof(float)));
    uint64_t* d_cand = c->out_idx.as<uint64_t>() + Q * kout;
    if (qtoks && qfloats) INNR_HIP_CHECK(copy_in(c, c->q_row.p, qtoks, qfloats * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, d_cand, cand, Q * kc * sizeof(uint64_t)));
    INNR_TRY(innr_maxsim_rerank_dev(d, cosine, c->q_row.as<float>(), Q, tq, Tq_stride, dim, d_cand, kc, k, c->out_idx.as<uint64_t>(), c->out_score.as<float>(), out_k));
    INNR_HIP_CHECK(copy_out(c, out_doc, c->out_idx.p, Q * kout * sizeof(uint64_t)));
    INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, Q * kout * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}
