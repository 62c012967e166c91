/*
 * innr_hip.h -- C ABI of the MI355X-native (gfx950 / CDNA4) batch k-NN scan behind innr's API.
 *
 * This is the drop-in boundary for ONE path of arclabs561/innr: batch::VerticalBatch +
 * batch_dot / batch_l2_squared / batch_cosine / batch_norms / batch_knn_* (src/batch.rs),
 * scalar::batch_knn_u8 (src/scalar.rs) and maxsim (src/maxsim.rs). The reference has no FFI of
 * its own (pure Rust, zero deps); these entry points are what a Rust `extern "C"` shim for that
 * path binds -- each one cites the reference interface it replaces. INTEGRATION.md shows the shim.
 *
 * Conventions
 *   - plain pointers and sizes, no C++/torch types; every function returns an innr_status
 *     (0 = ok, <0 = error) and never throws or aborts across the ABI. innr_last_error() returns a
 *     thread-local message for the last failure.
 *   - the reference reports misuse by panicking (assert_eq! on dimension mismatch, batch.rs:251,285,
 *     386,743,778); the ABI returns INNR_E_DIM_MISMATCH and the host shim turns it into that panic.
 *   - host buffers are caller-owned and only read/written during the call. `_dev` variants take
 *     DEVICE pointers (hipMalloc'ed / torch tensors on the ctx's device), run on the ctx stream and
 *     return after the result is complete on that stream.
 *   - indices are reported as uint64 (Rust usize); on device they are u32 (N < 2^32 - 1 per shard)
 *     plus a 64-bit per-shard base (innr_batch_set_index_base) for range-partitioned corpora.
 *   - results are deterministic: same inputs => same bits (tests/integration.rs:134-151).
 *   - NaN. A NaN in the INPUT keeps its sign through every entry point (total_cmp ranks -NaN below -inf and +NaN above
 *     +inf, so the sign decides where such a vector lands). A NaN that an invalid operation GENERATES -- inf * 0 in a dot
 *     product, inf / inf in a cosine -- has the sign the ISA gives it, and the reference inherits its host's: x86 produces
 *     0xFFC00000 (sign bit set), aarch64 0x7FC00000. gfx950 produces 0xFFC00000 like x86 (measured, tools/nan_probe.py), and this
 *     ABI guarantees it on every engine: a generated NaN is 0xFFC00000 and ranks LAST in batch_knn_dot / batch_knn_cosine (below
 *     -inf), as on the reference's x86 hosts (tests/test_gpu_exact.py::test_generated_nan_sign_and_rank_are_pinned).
 *   - there is NO CPU fallback inside this library. If no GPU is present, innr_ctx_create fails.
 */
#ifndef INNR_HIP_H
#define INNR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int innr_status;
#define INNR_OK 0
#define INNR_E_DIM_MISMATCH (-1) /* reference: assert_eq!(query.len(), batch.dimension) panics */
#define INNR_E_BAD_ARG (-2)
#define INNR_E_OOM (-3)
#define INNR_E_HIP (-4)
#define INNR_E_RCCL (-5)
#define INNR_E_UNSUPPORTED (-6) /* documented limit of this build (e.g. k > INNR_MAX_K) */

/* metric selector: which reference function family a scan/kNN call reproduces */
#define INNR_METRIC_DOT 0    /* batch_dot / batch_knn_dot            batch.rs:270-297, 742-764 (higher = better) */
#define INNR_METRIC_L2SQ 1   /* batch_l2_squared / batch_knn         batch.rs:236-266, 385-411 (lower = better)  */
#define INNR_METRIC_COSINE 2 /* batch_cosine / batch_knn_cosine      batch.rs:690-728, 777-800 (higher = better) */

/* kNN engine selector */
#define INNR_KNN_AUTO 0  /* MFMA GEMM for query batches, exact scan for small batches */
#define INNR_KNN_EXACT 1 /* bit-exact VALU scan in the reference's arithmetic order (HBM-bound) */
#define INNR_KNN_MFMA 2  /* f32 MFMA GEMM + fused top-k filter + exact re-score (MFMA-bound) */
#define INNR_KNN_MFMA_BF16 3 /* the same with the FILTER on the bf16 matrix pipe (16x the f32 MFMA rate) over a K-packed bf16
                              * copy of the corpus built on first use (+ N*D*2 bytes of HBM). Results are unchanged -- the
                              * candidates are re-scored in the reference's f32 order and the answer is proven against the
                              * bf16 error bound, unproven queries are redone exactly. Every metric with k <= 48 (cosine: a copy
                              * of the normalised rows; squared L2: a copy with |v|^2 in six more K columns); other calls are
                              * served by INNR_KNN_MFMA (innr_knn_stats.engine tells). INNR_KNN_AUTO picks a low-precision filter
                              * (this one, or INNR_KNN_MFMA_I8 where it applies) for >= 128 queries when the copy exists or fits. */

#define INNR_KNN_MFMA_I8 4 /* the filter on the INTEGER matrix pipe (v_mfma_i32_32x32x32_i8: twice the bf16 MFMA rate, 32x the f32 one).
                            * innr_batch_knn_u8[_dev]: over a K-packed signed copy of the codes built on first use (+ N*D bytes of
                            * HBM), the f32 query as a 14-bit fixed-point value -- its high int8 limb on the matrix pipe, the low
                            * limb bounded in the filter and computed exactly for the survivors (lists of 256: a 16-bit value, both
                            * limbs on the pipe). Needs alpha > 0 and D <= 65535; otherwise INNR_KNN_MFMA serves the call.
                            * INNR_KNN_AUTO picks it on large code corpora from two queries on once the copy exists (from four -- or
                            * with the fourth smaller call -- when it has to be built and fits): up to 128 queries cost one pass
                            * over the copy.
                            * innr_batch_knn[_dev] on an F32 batch (dot, cosine, squared L2 -- whose copy carries |v|^2 as two 8-bit
                            * limbs in up to 121 more dimensions; k <= INNR_MAX_K): the corpus scalar-quantised once with a
                            * single (offset, alpha) -- quantize_u8 with the corpus' own range, the first stage of the two-stage
                            * pipeline of scalar.rs:366-368 -- filtered on the integer pipe, re-scored on the f32 corpus and
                            * PROVEN against (alpha / 510) |q|_1 + the query's quantisation; unproven queries redone on the f32
                            * engine. Results unchanged in every case (stats->engine tells which engine ran). */

#define INNR_MAX_K 240 /* largest k the candidate-list engines hold (k + margin <= 256). Every kNN entry point accepts
                        * any k, like the reference: beyond INNR_MAX_K innr_batch_knn[_dev], innr_batch_knn_u8[_dev],
                        * innr_batch_knn_filtered / _reordered compute all N scores and sort them on the device, one query
                        * at a time (the reference's own algorithm, batch.rs:754-763), and so does innr_maxsim_topk[_multi]
                        * with its document scores; innr_batch_rerank* sorts candidate lists longer than 256. */

typedef struct innr_ctx innr_ctx;     /* one GPU: device id, stream, workspace. One per process/GPU. */
typedef struct innr_batch innr_batch; /* device-resident VerticalBatch (PDX, dimension-major) + cached norms */

/* what a kNN call did (optional out-parameter; all fields written) */
typedef struct innr_knn_stats {
    int engine;                 /* INNR_KNN_EXACT, INNR_KNN_MFMA, INNR_KNN_MFMA_BF16 or INNR_KNN_MFMA_I8 actually used */
    uint32_t queries_fallback;  /* MFMA engine: queries whose margin proof failed and were redone exactly */
    uint32_t candidates_kept;   /* k' = candidates per query kept before the exact re-score */
    float gemm_ms;              /* device time of the dominant kernel (HIP events on the ctx stream) */
    float total_ms;             /* device time of the whole call */
} innr_knn_stats;

/* ---- context ------------------------------------------------------------------------------ */
innr_status innr_ctx_create(int device, innr_ctx** out);
void innr_ctx_destroy(innr_ctx* ctx);
/* run on the caller's HIP stream (hipStream_t as void*), e.g. torch's current stream, so the library's kernels
 * are ordered with the caller's own device work; NULL = the device's legacy default stream. Without this call
 * the ctx uses a private non-blocking stream (every host-pointer entry point synchronises it before returning). */
innr_status innr_ctx_set_stream(innr_ctx* ctx, void* hip_stream);
innr_status innr_ctx_synchronize(innr_ctx* ctx);
/* Tuning / experiment switches of a context (no reference counterpart: innr has no configuration). Their defaults are read from
 * the environment ONCE, in innr_ctx_create (INNR_<NAME IN CAPITALS>); no call reads the environment afterwards. Names:
 * gemm_waves, gemm_blocks_per_cu, gemm_qt_group, gemm_seed_n, gemm_no_seed, gemm_no_kp_retry, i8_two_limb, no_auto_bf16,
 * no_auto_i8, u8_no_i8, rescore_all, maxsim_generic, no_k_rule, no_completion, no_rows_copy, i8_slices_per_cu, i8_no_small, i8_no_small4, i8_small_max_q, i8_small_free, trace, fail_local_search (a test
 * switch of the sharded calls), filter_keep_selection (default 1; 0: innr_batch_knn_filtered_multi and innr_batch_knn_u8_filtered
 * free their selection at the end of every call), copy_budget_mib (default -1 = unlimited: the copy budget, in MiB, of every batch created from now on, see
 * innr_batch_set_copy_budget), scan_max_slots (default 0 = fill the chip: the most wave slots an exact scan is cut into, rounded
 * up to a multiple of 4, so that a wave owns several chunks of a small corpus), mutate_round (default 0 = what fits 256 MiB: the
 * most rows a staging round of innr_batch_append_rows / innr_batch_update_rows and their u8 twins carries; a test switch), range_u8_i8_min_n (default
 * 65536: the fewest vectors of a code batch whose innr_batch_range_search_u8 calls the int8 collect pass serves) -- DESIGN.md lists what each one does. None of them changes a result. Unknown name: INNR_E_BAD_ARG. */
innr_status innr_ctx_set_option(innr_ctx* ctx, const char* name, long value);
innr_status innr_ctx_get_option(innr_ctx* ctx, const char* name, long* value);
const char* innr_last_error(void);
const char* innr_version(void);

/* ---- VerticalBatch (batch.rs:88-220) -------------------------------------------------------- */
/* data = VerticalBatch::data() (batch.rs:212): dimension-major, data[d*N + i] */
innr_status innr_batch_upload_colmajor(innr_ctx* ctx, const float* data, size_t N, size_t D, innr_batch** out);
/* rows = what from_rows/from_slices/from_flat receive (batch.rs:103,138,167): row-major [N*D];
 * the row-major -> dimension-major transpose runs on the device */
innr_status innr_batch_upload_rowmajor(innr_ctx* ctx, const float* rows, size_t N, size_t D, innr_batch** out);
/* synthetic corpus generated on the device (the bench: 30 GB cannot cross PCIe per run). Row i of the batch is
 * row (row0 + i) of the chosen stream, so range-partitioned shards of one logical corpus agree across GPUs.
 *   INNR_GEN_EXAMPLE_LCG: generate_embedding(D, seed + row) (examples/batch_demo.rs:167-170, 233-242) -- the
 *       reference example's generator; a one-parameter family of vectors, kept for the C1 plumbing shape.
 *   INNR_GEN_UNIFORM: i.i.d. uniform[-1,1), the distribution of the reference's criterion inputs
 *       (benches/batch.rs:11-21); stream = splitmix64 of the element index (oracle: orc_generate_uniform_rows). */
#define INNR_GEN_EXAMPLE_LCG 0
#define INNR_GEN_UNIFORM 1
innr_status innr_batch_generate(innr_ctx* ctx, size_t N, size_t D, int generator, uint64_t seed, uint64_t row0,
                                innr_batch** out);
void innr_batch_free(innr_batch* b);
/* introspection (cf. backend.rs:40-67): the engine INNR_KNN_AUTO resolves to for a Q-query call on this batch */
int innr_batch_auto_engine(const innr_batch* b, size_t Q);
size_t innr_batch_num_vectors(const innr_batch* b); /* batch.rs:199 */
size_t innr_batch_dimension(const innr_batch* b);   /* batch.rs:204 */
/* copy the dimension-major data back (VerticalBatch::data(), batch.rs:212): out[D*N] */
innr_status innr_batch_download_colmajor(innr_batch* b, float* out);
/* range-partitioned corpus: reported index = base + local index */
innr_status innr_batch_set_index_base(innr_batch* b, uint64_t base);

/* ---- one query x N scans (bit-identical to the reference's loops) --------------------------- */
/* batch_dot_into / batch_l2_squared_into / batch_cosine_into (batch.rs:284,250,705).
 * q: [D]; out: [N]. COSINE: `norms` = the caller's batch_norms() result [N] as in the reference
 * signature (batch.rs:690), or NULL to use the norms cached on the device. */
innr_status innr_batch_scores(innr_batch* b, int metric, const float* q, size_t D, const float* norms, float* out);
/* batch_norms_into (batch.rs:672): out[N] */
innr_status innr_batch_norms(innr_batch* b, float* out);

/* ---- kNN ------------------------------------------------------------------------------------ */
/* batch_knn_dot / batch_knn_cosine / batch_knn for Q queries at once (Q = 1 is the reference call).
 * queries: row-major [Q*D]. Writes k' = min(k, N) results per query, best first, to
 * out_idx[q*k' + r], out_score[q*k' + r]; *out_k = k'. k == 0 or N == 0 => *out_k = 0 (batch.rs:745).
 * Ordering: DOT/COSINE score descending by f32::total_cmp, ties -> lower index (stable sort,
 * batch.rs:757,793); L2SQ distance ascending, ties -> lower index (TopK keeps earlier ids, topk.rs:101).
 * Scores are bit-identical to the reference's portable loops in every engine. */
innr_status innr_batch_knn(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, size_t k,
                           int engine, uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* same, queries and outputs resident on the device (out arrays sized Q*min(k,N)) */
innr_status innr_batch_knn_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D, size_t k,
                               int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k,
                               innr_knn_stats* stats);

/* ---- scalar-quantised corpus: asymmetric f32 query x u8 codes (src/scalar.rs) ------------------------------ */
/* A &[QuantizedU8] (scalar.rs:171-174: N separately allocated Vec<u8>) becomes one device-resident code array.
 * codes: row-major packed [N*D] (document i's bytes at codes + i*D); alpha/offset = the collection's
 * QuantizationParams (scalar.rs:44-49). The result is an innr_batch that only the *_u8 entry points accept. */
innr_status innr_batch_upload_u8(innr_ctx* ctx, const uint8_t* codes, size_t N, size_t D, float alpha, float offset,
                                 innr_batch** out);
/* synthetic codes on the device: row i = quantize_u8(uniform row (row0+i) of stream `seed`, params) (scalar.rs:212) */
innr_status innr_batch_generate_u8(innr_ctx* ctx, size_t N, size_t D, uint64_t seed, uint64_t row0, float alpha,
                                   float offset, innr_batch** out);
/* codes back to the host, dimension-major out[d*N + i] */
innr_status innr_batch_download_u8(innr_batch* b, uint8_t* out);
/* ... and in again from that order (persistence: a saved code corpus is its data[d*N + i] behind a small header, like
 * VerticalBatch::data() for the f32 store, batch.rs:208-214) */
innr_status innr_batch_upload_u8_colmajor(innr_ctx* ctx, const uint8_t* data, size_t N, size_t D, float alpha, float offset,
                                          innr_batch** out);
/* asymmetric_dot_u8_precomputed for every document (scalar.rs:284-300; the map inside batch_knn_u8 :384-388):
 * out[i] = (alpha/255)*mixed_dot(q, codes_i) + offset*sum(q), bit-identical to the portable path. */
innr_status innr_batch_scores_u8(innr_batch* b, const float* q, size_t D, float* out);
/* batch_knn_u8 (scalar.rs:370-393) for Q queries: top-k by asymmetric dot, descending, ties -> lower index.
 * Same conventions as innr_batch_knn (k' = min(k,N); empty corpus or k == 0 -> *out_k = 0 before any check). */
innr_status innr_batch_knn_u8(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, int engine,
                              uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
innr_status innr_batch_knn_u8_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, int engine,
                                  uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats);
/* batch_knn_u8 (scalar.rs:370-393) over the vectors that pass a mask, for each of Q queries (an addition: the code-batch twin of
 * innr_batch_knn_filtered_multi). mask: N bytes, mask[i] != 0 <=> the vector takes part, one mask for every query. Writes
 * k' = min(k, number passing) results per query to out_idx[q*k' + r], out_score[q*k' + r] (arrays sized Q*min(k,N)): top k' by
 * asymmetric dot, descending by total_cmp, ties to the lower index, indices into this batch plus its index base, scores with the
 * bits of innr_batch_scores_u8; *out_k = k'. Any k is accepted (beyond INNR_MAX_K: the masked full sort).
 * Order of the checks: a null batch, an f32 batch or a null out_k: INNR_E_BAD_ARG; N == 0 or k == 0: *out_k = 0 (before the
 * dimension check, as in innr_batch_knn_u8, scalar.rs:376-378); D != the batch's: INNR_E_DIM_MISMATCH; Q == 0: *out_k = 0; a null
 * mask: INNR_E_BAD_ARG; null queries / outputs with work to do: INNR_E_BAD_ARG; no passing vector: *out_k = 0.
 * Engines: INNR_KNN_EXACT scans this batch's codes with the mask applied. Every other engine, INNR_KNN_AUTO included, runs on a
 * SELECTION: the passing vectors' codes gathered on the device, in index order, into a code batch of their own with this batch's
 * alpha and offset, searched by innr_batch_knn_u8_dev with the caller's engine (innr_knn_stats.engine tells which engine ran
 * there; the selection builds its own int8 copy when that engine wants one), the indices then mapped back; results are
 * bit-identical either way. A mask that passes every vector searches this batch itself. On a prefix view only the view's rows
 * are gathered. Memory: the batch keeps the selection of its last mask -- round_up(npass, 1024) * round_up(D, 32) bytes of codes,
 * round_up(N, 1024) + 4*npass bytes of mask and map, plus the selection's own copies -- counted as INNR_COPY_SELECTION and against
 * the copy budget; a call with the same mask (compared on the device after folding to 0/1) reuses it, a different mask replaces
 * it, innr_batch_free and innr_batch_release_copies(INNR_COPY_SELECTION) free it, the option filter_keep_selection = 0 frees it
 * at the end of every call. A selection that does not fit, or that the budget does not admit, leaves the call to the masked exact
 * scan. stats->total_ms covers the whole call (mask, selection build, search).
 * Out of scope: a mask per query, the adaptive k-NN on codes (the reference's is squared L2 on f32), a sharded variant. */
innr_status innr_batch_knn_u8_filtered(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, const uint8_t* mask,
                                       int engine, uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* same, queries, mask and outputs resident on the device (innr_batch_knn_dev's conventions) */
innr_status innr_batch_knn_u8_filtered_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, const uint8_t* d_mask,
                                           int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats);
/* Range search on codes: innr_batch_range_search's contract with the one metric of a code batch (an addition). A vector survives
 * for query j iff !(score < thresholds[j]), score with the bits of innr_batch_scores_u8: a NaN score or threshold survives. The
 * result layout is innr_batch_range_search's: out_offsets of Q + 1 64-bit entries, each query's entries in ascending index order,
 * indices = index base + local index, only global positions < cap written, cap == 0 a count-only call (out_idx / out_score may
 * then be null), *out_total > cap still INNR_OK.
 * Order of the checks: a null or f32 batch: INNR_E_BAD_ARG; D != the batch's: INNR_E_DIM_MISMATCH; a null out_offsets or
 * out_total: INNR_E_BAD_ARG; N == 0 or Q == 0: all-zero offsets; null thresholds, queries or outputs with work to do:
 * INNR_E_BAD_ARG.
 * Engines: INNR_KNN_EXACT scans the corpus in the reference's arithmetic, up to eight queries per pass: one pass counts the
 * survivors per 1024-vector chunk, a second one -- which skips every chunk without survivors -- writes them. The other known
 * values (INNR_KNN_MFMA, _BF16, _I8, and INNR_KNN_AUTO from a measured batch size on) take the collect path: one pass of the int8
 * matrix-pipe filter over the batch's int8 copy (INNR_COPY_I8_DOT, the one innr_batch_knn_u8 builds: reported, released and
 * budgeted as there) collects every vector whose approximate score is within the filter's error bound of the query's threshold,
 * those are re-scored exactly and the exact predicate decides. A query without a finite collect threshold (a NaN or infinite
 * threshold, a NaN / inf query, a query with no usable scale) and a query with more than 65536 collected vectors are finished by
 * the exact scan (stats->queries_fallback counts them). Results are bit-identical either way. The collect path serves a call only
 * if innr_batch_knn_u8's rules for the int8 engine hold (alpha > 0, finite params, D <= 65535; a prefix view: a length that is a
 * multiple of 32), the batch has at least range_u8_i8_min_n vectors (a context option, default 65536 -- it binds explicit
 * requests too: below it a tile launch plus re-score costs more than the scans) and the int8 copy exists or can be built: on an
 * explicit request whenever the copy budget admits it, under INNR_KNN_AUTO only with room to spare (free memory >= twice the copy
 * + 8 GiB) and from kRangeU8AutoQ0 queries on (api.hip; a tuning constant, not part of this contract). Otherwise, and for unknown
 * engine values, the exact scan serves the whole call and nothing counts as a fallback.
 * stats->engine = INNR_KNN_MFMA_I8 if a collect pass ran, else INNR_KNN_EXACT; queries_fallback = queries the exact scan finished
 * after a collect pass; candidates_kept = the longest collected list (at most 65536); gemm_ms = device time of the collect
 * launches (exact scan: of the scans); total_ms of the whole call. The host-memory entry point stages results as
 * innr_batch_range_search does (a count pass first where min(cap, Q*N) results would need more than 256 MiB).
 * Memory: the call works in rounds of at most 4096 queries whose workspace stays within 2 GiB (per query N/256 bytes of counts; on
 * the collect path N/8 bytes of bitmap and 768 KiB of lists and keys more).
 * Out of scope: a sharded variant; the filtered / selection variant of range search; bf16 / int8 collect modes of the f32
 * innr_batch_range_search. */
innr_status innr_batch_range_search_u8(innr_batch* b, const float* queries, size_t Q, size_t D, const float* thresholds, int engine,
                                       uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                       innr_knn_stats* stats);
/* same, queries, thresholds, out_offsets, out_idx and out_score resident on the device; the call synchronises with the host */
innr_status innr_batch_range_search_u8_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, const float* d_thresholds,
                                           int engine, uint64_t* d_out_offsets, uint64_t* d_out_idx, float* d_out_score, size_t cap,
                                           size_t* out_total, innr_knn_stats* stats);
/* quantize_u8 (scalar.rs:212-225) on the host (one-time ingest step): out[i] =
 * clamp(round((v[i]-offset)*255/alpha), 0, 255), round = half away from zero */
void innr_quantize_u8(const float* values, size_t n, float alpha, float offset, uint8_t* out);
/* mixed_dot_u8_f32 for one pair (scalar.rs:314-358, portable loop), host function like the other pairwise ones */
float innr_mixed_dot_u8_f32(const float* a, const uint8_t* b, size_t n);

/* corpus ingest on the device: codes of a resident f32 batch, out = quantize_u8 of every value (scalar.rs:212-225);
 * the new batch inherits the index base. */
innr_status innr_batch_quantize_u8(innr_batch* f32_batch, float alpha, float offset, innr_batch** out);
/* The range QuantizationParams::fit (scalar.rs:68-87) scans for, of a resident f32 batch: global min / max of the non-NaN
 * values; *out_any = 0 when the batch holds none. The host side finishes `fit` exactly like the reference: no values at all
 * -> {alpha 1, offset 0} (:69-74); otherwise from_range(min(f32::MAX, *out_min), max(f32::MIN, *out_max)) -- the reference's
 * scan starts from (f32::MAX, f32::MIN) and `fit` has no min > max guard, so a non-empty ALL-NaN corpus gives
 * from_range(f32::MAX, f32::MIN) = {alpha 1.0, offset 3.4028235e38}, not {1, 0} (innr_amd/scalar.py fit_batch, rust shim
 * scalar::fit_batch). The order of the reference's sequential scan decides between -0.0 and +0.0; here -0.0 < +0.0. */
innr_status innr_batch_minmax(innr_batch* f32_batch, float* out_min, float* out_max, int* out_any);
/* QuantizationParams::fit_quantile's range (scalar.rs:104-139) of a resident f32 batch: the values at the reference's two
 * ranks (its own f32 index arithmetic, :131-134) of the FINITE values sorted by total_cmp, found by a radix select on the
 * device (five corpus streams, no sort). quantile >= 1: the plain min/max of fit() (:118-120). *out_any = 0: no finite value
 * (alpha 1, offset 0). quantile outside (0, 1] is the reference's panic: INNR_E_DIM_MISMATCH with that message. */
innr_status innr_batch_quantile_range(innr_batch* f32_batch, float quantile, float* out_lo, float* out_hi, int* out_any);

/* ---- maxsim over a document corpus (src/maxsim.rs:96-194; caller shape examples/maxsim_colbert.rs:159-193) ---- */
typedef struct innr_docs innr_docs; /* device-resident token embeddings of `docs` documents, T tokens x dim each */
/* tokens: [docs*T*dim] row-major (document, token, dim); doc_len[docs] = valid tokens per document (<= T) or NULL */
innr_status innr_maxsim_upload(innr_ctx* ctx, const float* tokens, const uint32_t* doc_len, size_t docs, size_t T,
                               size_t dim, innr_docs** out);
/* synthetic corpus on the device: token (doc,t) = normalised uniform row (row0 + doc*T + t) of stream `seed`
 * (generate_normalized, examples/maxsim_colbert.rs:212-228, on the uniform generator) */
innr_status innr_maxsim_generate(innr_ctx* ctx, size_t docs, size_t T, size_t dim, uint64_t seed, uint64_t row0,
                                 innr_docs** out);
void innr_docs_free(innr_docs* d);
size_t innr_docs_count(const innr_docs* d);
/* persistence of a document corpus: its shape, and its tokens [docs*T*dim] (+ doc_len[docs] when it has them; may be NULL) */
innr_status innr_docs_shape(const innr_docs* d, size_t* ndocs, size_t* T, size_t* dim, int* has_doc_len);
innr_status innr_docs_download(innr_docs* d, float* tokens, uint32_t* doc_len);
innr_status innr_docs_set_index_base(innr_docs* d, uint64_t base);
/* maxsim(query, doc_i) (cosine == 0) or maxsim_cosine (cosine != 0) for EVERY document: out[docs], bit-identical
 * to the portable path (dot_portable / cosine_portable order). qtok: [Tq*dim]. Empty query/document -> 0.0. */
innr_status innr_maxsim_scores(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, float* out);
/* the k best documents by that score, descending, ties -> lower document index (a stable sort of the scores, as
 * the reference example does); scores are the exact maxsim values under either engine.
 * engine: INNR_KNN_EXACT = exact scan of every document; INNR_KNN_MFMA = approximate scores on the matrix cores,
 * exact re-score of the best candidates and a margin proof (unproven -> redone exactly, stats->queries_fallback = 1;
 * needs T > 16, dim % 8 == 0, dim <= 512); INNR_KNN_AUTO picks. stats->gemm_ms = device time of the corpus scan. */
innr_status innr_maxsim_topk(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, size_t k, int engine,
                             uint64_t* out_doc, float* out_score, size_t* out_k, innr_knn_stats* stats);

/* Several queries in one call (an addition; every query's result equals innr_maxsim_topk's). On the MFMA engine the
 * queries share corpus passes four at a time. qtoks: Q queries of Tq_stride*dim floats, query i using its first tq[i]
 * tokens (tq == NULL: Tq_stride each). out_doc / out_score: [Q][*out_k]. stats->gemm_ms sums the corpus scans. */
innr_status innr_maxsim_topk_multi(innr_docs* d, int cosine, const float* qtoks, size_t Q, const uint32_t* tq,
                                   size_t Tq_stride, size_t dim, size_t k, int engine, uint64_t* out_doc, float* out_score,
                                   size_t* out_k, innr_knn_stats* stats);

/* Second stage for multi-vector corpora (an addition; the document-side twin of innr_batch_rerank): exact maxsim (cosine != 0:
 * maxsim_cosine) of query j against ITS candidates cand[j*kc .. j*kc + kc), best min(k, kc) per query. Every candidate is scored
 * exactly, once, on the exact engine's arithmetic: no approximate stage, no proof, the MFMA engine is not involved.
 * Queries as in innr_maxsim_topk_multi: Q blocks of Tq_stride*dim floats, query j using its first tq[j] tokens (tq == NULL:
 * Tq_stride each; any tq[j] <= Tq_stride, 0 included). Candidates as in innr_batch_rerank: GLOBAL document indices (index base +
 * local index), any kc >= 1, no duplicates within one query (duplicates: that query's result is unspecified, no other query is
 * affected). A candidate outside [base, base + docs) -> INNR_E_BAD_ARG, detected on the device and reported at the end of the
 * call; outputs then unspecified. *out_k = min(k, kc); out_doc[j*out_k + r], out_score[j*out_k + r], ordered by score descending
 * (total order), ties -> lower document index; scores bit-identical to innr_maxsim_scores' for the same document (an empty
 * query or document scores 0.0). The dimension check comes first (INNR_E_DIM_MISMATCH); then docs == 0, Q == 0, k == 0 or
 * kc == 0 give *out_k = 0; Q*kc beyond 32-bit slots -> INNR_E_UNSUPPORTED.
 * Out of scope: ragged candidate counts or sentinel entries, a sharded variant (innr_sharded_maxsim is unchanged), re-ranking on
 * the MFMA engine, u8 / bf16 token stores. */
innr_status innr_maxsim_rerank(innr_docs* d, int cosine, const float* qtoks, size_t Q, const uint32_t* tq, size_t Tq_stride,
                               size_t dim, const uint64_t* cand, size_t kc, size_t k, uint64_t* out_doc, float* out_score,
                               size_t* out_k);
/* the same with qtoks, cand, out_doc and out_score resident on the device (tq stays a host array); the call synchronises with
 * the host once, to read the bad-candidate flag */
innr_status innr_maxsim_rerank_dev(innr_docs* d, int cosine, const float* d_qtoks, size_t Q, const uint32_t* tq, size_t Tq_stride,
                                   size_t dim, const uint64_t* d_cand, size_t kc, size_t k, uint64_t* d_out_doc,
                                   float* d_out_score, size_t* out_k);

/* ---- L2 variants of the batch module (exact engine, one query) -------------------------------------- */
/* batch_dimension_variance (batch.rs:572-592): out[D]; sequential sums in the reference's order, cached per batch */
innr_status innr_batch_dimension_variance(innr_batch* b, float* out);
/* batch_knn_filtered (batch.rs:820-882): mask[i] != 0 <=> predicate(i); only passing vectors are scored.
 * *out_k = min(k, number passing); indices refer to the original batch positions. */
innr_status innr_batch_knn_filtered(innr_batch* b, const float* q, size_t D, size_t k, const uint8_t* mask,
                                    uint64_t* out_idx, float* out_score, size_t* out_k);
/* batch_knn_filtered (batch.rs:820-882) applied to each of Q queries, for all three metrics (the reference's function is squared
 * L2; DOT / COSINE are this library's batched addition). mask: N bytes, mask[i] != 0 <=> predicate(i), one mask for every query.
 * Writes k' = min(k, number passing) results per query to out_idx[q*k' + r], out_score[q*k' + r] (arrays sized Q*min(k,N)),
 * indices into this batch plus its index base, in innr_batch_knn's order for the metric; *out_k = k'. The dimension check comes
 * first (batch.rs:829); then N == 0, k == 0, Q == 0 or no passing vector give *out_k = 0 (batch.rs:831-847). A null mask with
 * N > 0 or a u8 code batch (that is innr_batch_knn_u8_filtered): INNR_E_BAD_ARG.
 * Engines: INNR_KNN_EXACT scans this batch with the mask applied. Every other engine, INNR_KNN_AUTO included, runs on a SELECTION:
 * the passing vectors gathered on the device, in index order, into a compact batch of their own, searched like any batch of that
 * size (innr_knn_stats.engine tells which engine ran there), the indices then mapped back; results are bit-identical either way.
 * A mask that passes every vector searches this batch itself. Memory: the batch keeps the selection of its last mask --
 * npass*D*4 bytes (D rounded up to 32), N + 4*npass bytes of mask and map, plus the filter copies the engines build on it -- so that a
 * call with the same mask (compared on the device after folding to 0/1) reuses it; a different mask replaces it, innr_batch_free
 * frees it, the option filter_keep_selection = 0 frees it at the end of every call. If it does not fit, the masked exact scan
 * serves the call. stats->total_ms covers the whole call (mask, selection build, search). */
innr_status innr_batch_knn_filtered_multi(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, size_t k,
                                          const uint8_t* mask, int engine, uint64_t* out_idx, float* out_score, size_t* out_k,
                                          innr_knn_stats* stats);
/* same, queries, mask and outputs resident on the device (innr_batch_knn_dev's conventions) */
innr_status innr_batch_knn_filtered_multi_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D, size_t k,
                                              const uint8_t* d_mask, int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k,
                                              innr_knn_stats* stats);
/* batch_knn_reordered (batch.rs:621-659): distances accumulated in decreasing-variance dimension order
 * (variance_order :599-603), then k smallest by (distance, index). */
innr_status innr_batch_knn_reordered(innr_batch* b, const float* q, size_t D, size_t k, uint64_t* out_idx,
                                     float* out_score, size_t* out_k);
/* batch_l2_squared_pruning (batch.rs:320-365): every (index, squared distance) with distance not > threshold,
 * in index order. *out_n = number of survivors; at most `cap` of them are written. */
innr_status innr_batch_l2_squared_pruning(innr_batch* b, const float* q, size_t D, float threshold, uint64_t* out_idx,
                                          float* out_dist, size_t cap, size_t* out_n);
/* Range search: batch_l2_squared_pruning (batch.rs:320-365) for Q queries at once, each with its own threshold, for all three
 * metrics (the reference's function is one query, squared L2; DOT / COSINE are this library's addition). queries: row-major [Q*D];
 * thresholds: [Q]. A vector survives for query j iff
 *   INNR_METRIC_L2SQ:          !(dist > thresholds[j])   -- the reference's rule (batch.rs:351): a NaN distance survives;
 *   INNR_METRIC_DOT / _COSINE: !(score < thresholds[j])  -- the same rule for similarities;
 * dist / score have the bits of innr_batch_scores for that query (cosine: the cached norms, both epsilon guards). Query j owns
 * [out_offsets[j], out_offsets[j+1]) of the FULL result (out_offsets: Q + 1 entries, 64-bit: Q*N can pass 2^32), its entries in
 * ascending index order as the reference pushes them, indices = index base + local index; *out_total = out_offsets[Q]. Only the
 * entries at global positions < cap are written to out_idx / out_score; cap == 0 (out_idx / out_score may then be null) is a
 * count-only call. *out_total > cap is still INNR_OK -- enlarge the buffers and call again (innr_batch_l2_squared_pruning's
 * convention). For Q = 1 and squared L2 the result equals innr_batch_l2_squared_pruning's bit for bit.
 * The dimension check comes first (INNR_E_DIM_MISMATCH); then N == 0 or Q == 0 give all-zero offsets. A u8 code batch, a null
 * out_offsets / out_total, null thresholds with Q > 0: INNR_E_BAD_ARG.
 * Engines: INNR_KNN_EXACT scans the corpus in the reference's arithmetic, up to eight queries per pass: one pass counts the
 * survivors per 256-vector chunk, a second one -- which skips every chunk without survivors -- writes them. INNR_KNN_MFMA (and the
 * _BF16 / _I8 requests) collects, in one pass of the f32 matrix-pipe filter, every vector whose approximate score is within the
 * filter's error bound of the threshold, re-scores those exactly and keeps what passes the exact predicate; a query with more
 * than 65536 collected vectors, a query norm or threshold outside the bound's range, and every query of a corpus whose largest
 * norm is outside [1e-12, 1e18] are finished by the exact scan instead (stats->queries_fallback counts them). A prefix view whose
 * length is no multiple of 32 has no matrix-pipe engine (innr_batch_knn's rule): the exact engine serves the whole call, nothing
 * counts as a fallback. Results are bit-identical either way. INNR_KNN_AUTO: the exact scan for small batches, the collect path
 * from a measured batch size on (kRangeAutoQ0 in api.hip, 64 in this build; DESIGN.md 4.5c has the table) -- a tuning constant, not part of this contract.
 * stats->engine = INNR_KNN_MFMA if a collect pass ran, else INNR_KNN_EXACT; candidates_kept = the longest
 * collected list; gemm_ms = device time of the collect passes (exact engine: of the scans), total_ms of the whole call.
 * The host-memory entry point stages min(cap, Q*N) results on the device; where that is more than 256 MiB it counts first (one
 * more search) and stages what the result needs, so a generous cap costs time, not memory; its stats describe the last search.
 * Memory: the call works in rounds of at most 4096 queries whose workspace stays within 2 GiB (per query N/64 bytes of counts;
 * on the collect path N/8 bytes of bitmap and 768 KiB of lists more).
 * Out of scope: the int8 / bf16 collect modes, a sharded variant. (u8 code batches: innr_batch_range_search_u8, whose collect
 * path runs on the int8 matrix pipe.) */
innr_status innr_batch_range_search(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, const float* thresholds,
                                    int engine, uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap,
                                    size_t* out_total, innr_knn_stats* stats);
/* same, queries, thresholds, out_offsets, out_idx and out_score resident on the device; the call synchronises with the host */
innr_status innr_batch_range_search_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D,
                                        const float* d_thresholds, int engine, uint64_t* d_out_offsets, uint64_t* d_out_idx,
                                        float* d_out_score, size_t cap, size_t* out_total, innr_knn_stats* stats);
/* batch_knn_adaptive (batch.rs:441-564) for each of Q queries (row-major [Q*D]; Q = 1 is the reference call): squared L2 with a
 * warm-up over the first min(warmup_dims, D) dimensions, a prune against the extrapolated k-th warm-up distance, then the
 * remaining dimensions for the survivors only, pruned against a threshold that is renewed after every dimension d with
 * d % 32 == 0 and never below k live vectors. The function is the reference's HEURISTIC, not an exact k-NN: its survivors depend
 * on the corpus order, and on data whose early dimensions do not carry the variance its recall against innr_batch_knn is poor.
 * The contract is the reference's answer for each query alone, bit for bit: the same indices in the same order (distance by
 * f32::total_cmp, ties to the lower index), the same score bits (every distance includes all D dimensions, accumulated as
 * innr_batch_scores(INNR_METRIC_L2SQ) does). DESIGN.md 4.5d restates the sequential loop as the phases the device runs.
 * Writes k' = min(k, N) results per query to out_idx[q*k' + r], out_score[q*k' + r]; *out_k = k'; indices = index base + local
 * index. Any k is accepted. On a prefix view D and the extrapolation factor D / warmup_dims are the view's.
 * Order of the checks (batch.rs:447-463): a null batch or out_k, a u8 code batch: INNR_E_BAD_ARG; D != the batch's:
 * INNR_E_DIM_MISMATCH; warmup_dims == 0: INNR_E_DIM_MISMATCH, "warmup_dims must be > 0" (the reference's assert!, mapped as
 * innr_batch_quantile_range maps its panic); N == 0, k == 0 or Q == 0: *out_k = 0; null queries / outputs with work to do:
 * INNR_E_BAD_ARG; D == 0: indices 0 .. k'-1 with scores 0.0.
 * stats: engine = INNR_KNN_EXACT, queries_fallback = 0, candidates_kept = the largest number of vectors alive after the
 * warm-up prune over the queries, gemm_ms = device time of the warm-up scans, total_ms = the whole call.
 * Queries run one after another; each synchronises with the host once after its warm-up prune and once per later segment that
 * still prunes (usually one or two). Memory, from the context's grow-only workspace (innr_ctx_memory reports it, innr_ctx_trim
 * returns it): of the order of 8*N bytes, for the one query in flight -- 4*N of warm-up distances, 8*N of sort keys, N/16 of counts,
 * and 17 bytes per vector alive after the warm-up prune.
 * Out of scope: sharing the warm-up pass between queries, a sharded variant, u8 code batches, other metrics (the reference's
 * function is squared L2 only), and any change to the heuristic. */
innr_status innr_batch_knn_adaptive(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, size_t warmup_dims,
                                    uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* same, queries and outputs resident on the device (innr_batch_knn_dev's conventions) */
innr_status innr_batch_knn_adaptive_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, size_t warmup_dims,
                                        uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats);

/* ---- search by stored vector (no reference counterpart beyond the accessor: the reference's corpus lives in host memory) ---- */
/* VerticalBatch::extract_vector (batch.rs:217) for n vectors at once: out[j*D + d] = vector idx[j], dimension d. Nothing but the
 * n rows moves: the corpus is not downloaded, and the row-major copy (INNR_COPY_ROWS) is read when the batch already has one
 * (and the option no_rows_copy is off) but never built for this -- reading a few rows allocates nothing of the corpus' size.
 * Indices are GLOBAL (index base + local index), like innr_batch_rerank's candidates; duplicates and any order are allowed. An
 * index outside [base, base + N): INNR_E_BAD_ARG with a message naming the range. The host entry point checks before it moves
 * anything; the _dev entry point finds such an index on the device and reports it at the end of the call -- the kernels neither
 * read nor write out of bounds for it, the output is then unspecified.
 * A copy, no arithmetic: every bit pattern arrives unchanged (a NaN's sign and payload, -0.0, denormals, +-inf). On a prefix view D
 * and the rows are the view's.
 * Order of the checks: a null batch or a u8 code batch: INNR_E_BAD_ARG; n == 0 or D == 0: INNR_OK, nothing written; null idx /
 * out with work to do: INNR_E_BAD_ARG.
 * Memory: the host entry point stages indices and rows in the context's workspace, at most 256 MiB at a time. */
innr_status innr_batch_gather_rows(innr_batch* b, const uint64_t* idx, size_t n, float* out);
/* same, d_idx and d_out resident on the device; writes exactly n*D floats; the call synchronises with the host (the index check) */
innr_status innr_batch_gather_rows_dev(innr_batch* b, const uint64_t* d_idx, size_t n, float* d_out);
/* innr_batch_knn with the queries taken from the batch itself: query j = vector idx[j] (global indices as above, duplicates and
 * any order allowed; an index outside the batch: INNR_E_BAD_ARG as above, outputs unspecified). There is no D argument: the
 * queries have the batch's dimension by construction (a prefix view's: its own). "More like this", k-NN graphs, near-duplicates.
 * exclude_self == 0: query j's result equals, bit for bit and position for position, innr_batch_knn[_dev]'s for the query
 *   gather_rows(idx[j]) with the same metric, engine and k; *out_k = min(k, N).
 * exclude_self != 0: the best k' = min(k, N - 1) of all vectors except idx[j] itself, in the metric's order: innr_batch_knn's
 *   answer for min(k + 1, N) with the entry whose index is idx[j] removed or, where that entry is absent, the last one removed.
 *   It is absent in two ways: with the dot metric a vector need not be among its own best, and among duplicates the lower indices
 *   come first. Exactly one entry is always dropped; when min(k + 1, N) == N the self entry is always present. Other vectors
 *   equal to idx[j] stay in: the index is excluded, not the value. *out_k = k' (N == 1: 0).
 * Results at out_idx[j*k' + r], out_score[j*k' + r]. Any k is accepted. With exclude_self the inner search runs with k + 1, so
 * k = 240 = INNR_MAX_K already takes the path beyond INNR_MAX_K (all N scores sorted, one query at a time).
 * Order of the checks: a null batch or out_k, a u8 code batch, an unknown metric: INNR_E_BAD_ARG; N == 0, k == 0, Q == 0 or
 * k' == 0: *out_k = 0; null idx / outputs with work to do: INNR_E_BAD_ARG.
 * The call works in rounds of at most 4096 queries: gather, search, strip. A round's workspace -- round*D*4 bytes of gathered
 * rows and, with exclude_self, round*(k + 1)*12 bytes of staged results -- stays within 256 MiB: the round shrinks to fit (by
 * k + 1 as given, also where N is smaller), never below one query. The host entry point stages the Q indices and the Q*k' results on the device besides.
 * innr_ctx_memory counts all of it, innr_ctx_trim returns it.
 * stats: engine = the last round's, queries_fallback and gemm_ms summed over the rounds, candidates_kept their maximum, total_ms
 * the whole call, gather and strip included.
 * Out of scope: u8 code batches (a code row is not an f32 query, and the reference defines no de-quantised search), document
 * corpora, a sharded variant, a fused range self-join (compose innr_batch_gather_rows_dev and
 * innr_batch_range_search_dev), excluding vectors EQUAL to the query. */
innr_status innr_batch_knn_rows(innr_batch* b, int metric, const uint64_t* idx, size_t Q, size_t k, int exclude_self, int engine,
                                uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* same, d_idx and the outputs resident on the device (innr_batch_knn_dev's conventions) */
innr_status innr_batch_knn_rows_dev(innr_batch* b, int metric, const uint64_t* d_idx, size_t Q, size_t k, int exclude_self, int engine,
                                    uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats);

/* ---- changing a resident f32 batch in place: append, overwrite and remove rows (an addition: the reference's VerticalBatch is
 * immutable) ----
 * The handle, the index base, the copy budget, alpha / offset and the matrix-pipe eligibility stay as they are;
 * innr_batch_num_vectors reports the new N. `rows` is row-major [n*D], as innr_batch_upload_rowmajor takes it; every value is
 * copied as a 32-bit word (a NaN's sign and payload, -0.0, denormals and +-inf arrive unchanged).
 * One contract for the three: after a successful call every entry point of the library answers on this batch exactly as on a
 * fresh batch uploaded with the final rows -- indices position for position, score bits, every engine. After a failed call the
 * batch is exactly as before: store, derived state, answers.
 * Derived state: a call that changes the batch drops EVERYTHING the batch derived from its store -- every INNR_COPY_* kind
 * (remembered refusals included), the kept selection, the cached norms and their by-products, the dimension variances, the int8
 * quantisation ranges and the engines' call history. Each is rebuilt by the next call that wants it, under the rules of that
 * moment: an append followed by a search pays the norms pass and the copy builds again. This is deliberately the simple rule.
 * Views: a batch must have no live prefix view when it is changed (append and keep move the store, update makes a view's
 * copies and norms stale). The C ABI cannot see live views; as with "the parent must outlive the view", the caller keeps the
 * rule. A view handle itself is refused.
 * Order of the checks, all three: a null batch, a u8 code batch or a prefix view: INNR_E_BAD_ARG; D != the batch's:
 * INNR_E_DIM_MISMATCH (an empty batch created with D = 0 takes only D = 0 rows; keep has no D); n == 0 (keep: N == 0):
 * INNR_OK, nothing touched; null rows / idx / mask with work to do: INNR_E_BAD_ARG; the size limit; the index checks.
 * Out of scope: u8 code batches (refused here: the next section's innr_batch_append_codes / _update_codes / _keep_codes change
 * one) and document corpora; reserved capacity and amortised growth (every append past the padding
 * copies the store once); incremental maintenance of norms and filter copies; sharded corpora (a rank's shard may be changed,
 * the index bases of the other shards and anything cached per communicator are the caller's business); changing a batch through
 * a view; atomicity against searches issued concurrently from another thread, beyond the context's lock. */
/* Append: the new rows get local indices N .. N+n-1, the old rows keep theirs. N + n <= the store's padded width (N rounded up
 * to 256): the rows are transposed into the zero padding in place, nothing is allocated. Otherwise a new store of
 * round_up(N + n, 256) columns is allocated and zeroed, the old block copied across on the device, the rows transposed in, and
 * the old store freed after the stream is synchronised: the call needs the old and the new store at once, a failed hipMalloc is
 * INNR_E_OOM. N + n beyond the u32 index limit of a batch: INNR_E_UNSUPPORTED. The host entry point stages the rows in the
 * context's workspace, at most 256 MiB at a time. */
innr_status innr_batch_append_rows(innr_batch* b, const float* rows, size_t n, size_t D);
/* same, d_rows resident on the device; the call synchronises with the host (the allocation) */
innr_status innr_batch_append_rows_dev(innr_batch* b, const float* d_rows, size_t n, size_t D);
/* Update: row idx[j] becomes rows[j*D ..]. Indices are GLOBAL (index base + local index, as in innr_batch_gather_rows), in any
 * order. Nothing is reallocated. Every index is checked on the device before anything is written -- against [base, base + N) and,
 * through an N-bit bitmap in the context's workspace, against the other indices of the call: an index outside the range, or one
 * that occurs twice in one call, is INNR_E_BAD_ARG with a message naming which of the two it was (duplicates are refused, not
 * "last wins": the same inputs give the same bits). The host entry point stages indices and rows in rounds of at most 256 MiB;
 * the bitmap spans all rounds, so nothing is written before every index has been checked. */
innr_status innr_batch_update_rows(innr_batch* b, const uint64_t* idx, const float* rows, size_t n, size_t D);
/* same, d_idx and d_rows resident on the device; the call synchronises with the host (the check's flag) */
innr_status innr_batch_update_rows_dev(innr_batch* b, const uint64_t* d_idx, const float* d_rows, size_t n, size_t D);
/* Keep (remove): the rows with mask[i] != 0 survive, in index order; row i's new local index is the number of kept rows below
 * it. mask: N bytes. *out_n (may be null) receives the new N. The kept rows are compacted into a new store of round_up(N', 256)
 * columns by the selection's count and gather kernels (old and new store exist at once; a failed hipMalloc is INNR_E_OOM); the
 * memory of the removed rows is given back. A mask that keeps every row changes nothing and drops nothing; a mask that keeps
 * none leaves an N = 0 batch of the same D. The host entry point stages the mask in the context's workspace. */
innr_status innr_batch_keep_rows(innr_batch* b, const uint8_t* mask, size_t* out_n);
/* same, d_mask resident on the device; the call synchronises with the host (the count, the allocation) */
innr_status innr_batch_keep_rows_dev(innr_batch* b, const uint8_t* d_mask, size_t* out_n);

/* ---- changing a resident u8 code batch in place: append, overwrite and remove rows, as codes or as f32 rows quantised on the
 * device (an addition: the reference's quantised corpus is a list of immutable QuantizedU8) ----
 * The byte twins of the f32 section above, for the batches of innr_batch_upload_u8 / _generate_u8 / _quantize_u8. The handle, the
 * index base, the copy budget and alpha / offset stay as they are; innr_batch_num_vectors reports the new N. `codes` is row-major
 * u8 [n*D], as innr_batch_upload_u8 takes it. The _quantized variants take row-major f32 [n*D] and store, for every value v,
 * quantize_u8(v) under the BATCH's alpha / offset: clamp(round((v - offset) * (255.0f / alpha))) with 255.0f / alpha computed
 * once in f32 on the host, no contraction, round half away from zero, NaN -> 0 -- the arithmetic of innr_quantize_u8,
 * innr_batch_quantize_u8 and innr_batch_generate_u8, and like them without a check on alpha. After quantising, a _quantized call
 * IS the _codes call on those codes.
 * One contract for the five: after a successful call every entry point that accepts a code batch answers on this batch exactly
 * as on a fresh code batch uploaded with the final codes -- indices position for position, score bits, every engine. After a
 * failed call the batch is exactly as before: store, derived state, answers.
 * Derived state: a successful call that changes the batch drops EVERYTHING the batch derived from its store, through the one
 * list the f32 calls use -- for a code batch the int8 copy (INNR_COPY_I8_DOT, with its `weak` mark and a remembered refusal), the
 * kept selection and the engines' call history. Each is rebuilt by the next call that wants it.
 * Views: a batch must have no live prefix view when it is changed; a view handle itself is refused (see the f32 section).
 * Order of the checks, all five: a null batch, an f32 batch or a prefix view: INNR_E_BAD_ARG (the message says which: "null",
 * "f32", "view"); D != the batch's: INNR_E_DIM_MISMATCH (keep has no D); n == 0 (keep: N == 0): INNR_OK, nothing touched, nothing
 * dropped; null codes / rows / idx / mask with work to do: INNR_E_BAD_ARG; the size limit -- N + n must stay below 2^32 - 1 - 1024,
 * the bound of every code batch: INNR_E_UNSUPPORTED, before anything is read or allocated; the index checks.
 * Memory: a code store has round_up(N, 1024) columns x round_up(D, 32) rows of bytes. The host entry points stage in the
 * context's workspace in rounds of at most 256 MiB (indices, codes and, for the _quantized variants, the f32 rows and their codes
 * together; the option mutate_round bounds the rows of a round); a _quantized_dev call quantises into that workspace, n*D bytes in
 * rounds of at most 256 MiB. An append past the padding and a keep need the old and the new store at once.
 * Out of scope: reserved capacity and amortised growth (every append past the padding copies the store once); incremental
 * maintenance of the int8 copy; re-fitting alpha / offset when appended values fall outside the range (they clamp, as quantize_u8
 * does); document corpora; sharded corpora; changing a batch through a view; atomicity against searches issued concurrently from
 * another thread, beyond the context's lock. */
/* Append: the new rows get local indices N .. N+n-1, the old rows keep theirs. N + n <= the store's padded width (N rounded up
 * to 1024): the rows are transposed into the zero padding in place, byte by byte (column N need be no multiple of 4), nothing is
 * allocated; a failure after a partial write zeroes the touched padding again. Otherwise a new store of round_up(N + n, 1024)
 * columns is allocated and zeroed, the old D x N block copied across on the device (a pitched copy), the rows transposed in, and
 * the old store freed after the stream is synchronised; a failed hipMalloc is INNR_E_OOM and leaves the batch untouched. */
innr_status innr_batch_append_codes(innr_batch* b, const uint8_t* codes, size_t n, size_t D);
/* same, d_codes resident on the device; the call synchronises with the host (the allocation) */
innr_status innr_batch_append_codes_dev(innr_batch* b, const uint8_t* d_codes, size_t n, size_t D);
/* Update: row idx[j] becomes codes[j*D ..]. Indices are GLOBAL (index base + local index), in any order. Nothing is reallocated.
 * Two passes, as innr_batch_update_rows: every index is checked on the device before anything is written -- against
 * [base, base + N) and, through an N-bit bitmap in the context's workspace that spans all staging rounds, against the other
 * indices of the call. An index outside the range, or one that occurs twice in one call, is INNR_E_BAD_ARG with a message naming
 * it (duplicates are refused, not "last wins"). The writes are single-byte stores: four neighbouring vectors share a dword of a
 * dimension row, and the three a call does not name are never read or rewritten. */
innr_status innr_batch_update_codes(innr_batch* b, const uint64_t* idx, const uint8_t* codes, size_t n, size_t D);
/* same, d_idx and d_codes resident on the device; the call synchronises with the host (the check's flag) */
innr_status innr_batch_update_codes_dev(innr_batch* b, const uint64_t* d_idx, const uint8_t* d_codes, size_t n, size_t D);
/* Keep (remove): the rows with mask[i] != 0 survive, in index order; row i's new local index is the number of kept rows below
 * it. mask: N bytes. *out_n (may be null) receives the new N. The kept rows are compacted into a new store of round_up(N', 1024)
 * columns by the selection's count and gather kernels (a failed hipMalloc is INNR_E_OOM); the memory of the removed rows is
 * given back. A mask that keeps every row changes nothing and drops nothing; a mask that keeps none leaves an N = 0 batch of the
 * same D, which append fills again. The host entry point stages the mask in the context's workspace. */
innr_status innr_batch_keep_codes(innr_batch* b, const uint8_t* mask, size_t* out_n);
/* same, d_mask resident on the device; the call synchronises with the host (the count, the allocation) */
innr_status innr_batch_keep_codes_dev(innr_batch* b, const uint8_t* d_mask, size_t* out_n);
/* innr_batch_append_codes of quantize_u8(rows) under the batch's alpha / offset, quantised on the device */
innr_status innr_batch_append_quantized(innr_batch* b, const float* rows, size_t n, size_t D);
/* same, d_rows resident on the device (fresh embeddings never visit the host) */
innr_status innr_batch_append_quantized_dev(innr_batch* b, const float* d_rows, size_t n, size_t D);
/* innr_batch_update_codes of quantize_u8(rows) under the batch's alpha / offset, quantised on the device */
innr_status innr_batch_update_quantized(innr_batch* b, const uint64_t* idx, const float* rows, size_t n, size_t D);
/* same, d_idx and d_rows resident on the device */
innr_status innr_batch_update_quantized_dev(innr_batch* b, const uint64_t* d_idx, const float* d_rows, size_t n, size_t D);

/* ---- pairwise surface kept on the host: called per PAIR by graph indexes, so a kernel
 * launch cannot pay for itself. Plain host functions in the reference's portable arithmetic order. ------------ */
float innr_dot_f32(const float* a, const float* b, size_t n);    /* dense::dot_portable dense.rs:103; DistDot = -dot, distance.rs:88 */
float innr_cosine_f32(const float* a, const float* b, size_t n); /* dense::cosine_portable dense.rs:288; DistCosine = 1 - cosine, distance.rs:76 */
float innr_l2sq_f32(const float* a, const float* b, size_t n);   /* dense::l2_distance_squared_portable dense.rs:648; DistL2 = sqrt, distance.rs:99 */
float innr_l1_f32(const float* a, const float* b, size_t n);     /* dense::l1_distance_portable dense.rs:550; DistL1, distance.rs:110 */
/* DistHamming (u8 bit-Hamming, distance.rs:116-126) and DistSlotU32 (fraction of differing u32 slots, :128-143) */
uint32_t innr_hamming_u8(const uint8_t* a, const uint8_t* b, size_t n);
float innr_slot_distance_u32(const uint32_t* a, const uint32_t* b, size_t n);
/* maxsim / maxsim_cosine of ONE (query, document) pair (maxsim.rs:96-194, portable path :142-152); tokens packed
 * row-major [n][dim]; cosine != 0 selects maxsim_cosine. Empty query or document -> 0.0. */
innr_status innr_maxsim_pair(const float* q, size_t nq, const float* d, size_t nd, size_t dim, int cosine, float* out);

/* ---- second stage of the two-stage pipeline (scalar.rs:366-368: u8 first pass, exact re-rank) --------------- */
/* exact scores (reference arithmetic order, like innr_batch_knn's) of caller-given candidates cand[Q][kc] (global
 * indices inside this batch's range, no duplicates within a query; any kc -- up to 256 candidates per query are ranked
 * in registers, beyond that every query's candidates are sorted on the device), best min(k, kc) per query in the kNN
 * functions' order (dot/cosine: score desc; L2SQ: distance asc; ties: index asc). */
innr_status innr_batch_rerank(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, const uint64_t* cand,
                              size_t kc, size_t k, uint64_t* out_idx, float* out_score, size_t* out_k);
innr_status innr_batch_rerank_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D,
                                  const uint64_t* d_cand, size_t kc, size_t k, uint64_t* d_out_idx, float* d_out_score,
                                  size_t* out_k);

/* ---- matryoshka prefix (dense.rs:436-462 matryoshka_dot / matryoshka_cosine; examples/matryoshka_search.rs) ------- */
/* A batch over the first min(prefix_dims, D) dimensions of `parent` (f32 or u8 codes): the leading rows of the
 * dimension-major corpus, shared, not copied. Every batch entry point works on it (scores, norms, kNN: its cosine uses
 * the prefix norms, as matryoshka_cosine does); the coarse stage of the two-stage search is innr_batch_knn on the view
 * with the queries' first prefix_dims values (row stride = prefix_dims), the fine stage innr_batch_rerank on the
 * parent. The parent must outlive the view; free the view with innr_batch_free. prefix_dims == 0 is INNR_E_BAD_ARG. */
innr_status innr_batch_prefix_view(innr_batch* parent, size_t prefix_dims, innr_batch** out);

/* ---- device memory: report, release, prebuild and bound what a batch derives from its corpus (an addition) ------------
 * The reference's quantised store reports memory_bytes() (scalar.rs:205-208); here a batch owns more than its store. Beside the
 * corpus it keeps DERIVED allocations, each built by the first call that wants it and kept for the batch's lifetime; one bit
 * names each kind (DESIGN.md 3 has the table: which call builds it, under which policy, its size):
 *   INNR_COPY_ROWS          the row-major copy (N * round_up(D, 4) * 4 bytes): many candidates per query re-scored exactly
 *   INNR_COPY_BF16_*        the K-packed bf16 filter copies of INNR_KNN_MFMA_BF16, one per metric
 *   INNR_COPY_BF16LO_*      the lo limbs of the dot / cosine copy: with the BF16 copy of that metric, INNR_KNN_MFMA's split filter
 *   INNR_COPY_I8_*          the K-packed int8 filter copies of INNR_KNN_MFMA_I8 (a u8 code batch has the DOT kind only)
 *   INNR_COPY_SELECTION     the kept selection of innr_batch_knn_filtered_multi / innr_batch_knn_u8_filtered: its compact store, mask and map, and every
 *                           copy the selection batch built for itself (its cached norms, 12 bytes per vector at most, are not
 *                           counted)
 * A prefix view is a batch of its own here: it shares the parent's store (corpus_bytes = 0), owns its copies and has its OWN
 * budget -- the context option's value when the view is created, not its parent's. A view's copies are not reported by, and do
 * not count against the budget of, the parent: a caller that bounds a batch with innr_batch_set_copy_budget and searches views
 * of it (the coarse stage of a matryoshka search) sets each view's budget too, or the views' copies come on top. */
#define INNR_COPY_ROWS (1u << 0)
#define INNR_COPY_BF16_DOT (1u << 1)
#define INNR_COPY_BF16_COS (1u << 2)
#define INNR_COPY_BF16_L2 (1u << 3)
#define INNR_COPY_BF16LO_DOT (1u << 4)
#define INNR_COPY_BF16LO_COS (1u << 5)
#define INNR_COPY_I8_DOT (1u << 6)
#define INNR_COPY_I8_COS (1u << 7)
#define INNR_COPY_I8_L2 (1u << 8)
#define INNR_COPY_SELECTION (1u << 9)
#define INNR_COPY_ALL 0x3FFu
/* What the batch holds on the device NOW, in bytes exactly as they were asked of hipMalloc: *corpus_bytes the store it owns (0 for
 * a prefix view), *aux_bytes its cached norms and their by-products, *derived_bytes the sum over everything INNR_COPY_ALL names,
 * *present_mask the kinds that exist. Any out pointer may be null. A null batch is INNR_E_BAD_ARG; the call touches no device
 * state (host bookkeeping, read under the context's lock).
 * Out of scope: the context's workspace (innr_ctx_memory), memory of other batches or of a view's parent, anything sharded. */
innr_status innr_batch_memory(const innr_batch* b, uint64_t* corpus_bytes, uint64_t* aux_bytes, uint64_t* derived_bytes,
                              uint32_t* present_mask);
/* the sum over the kinds in `mask` (bits outside INNR_COPY_ALL are ignored); innr_batch_copy_bytes(b, INNR_COPY_ALL) is
 * innr_batch_memory's *derived_bytes. Null batch or null `bytes`: INNR_E_BAD_ARG. */
innr_status innr_batch_copy_bytes(const innr_batch* b, uint32_t mask, uint64_t* bytes);
/* Free the kinds in `mask` (after synchronising the context's stream) and forget that any of them was ever refused for lack of
 * memory -- a refusal under the "fits with room to spare" rule is otherwise remembered for the batch's lifetime, so this is also how
 * a caller says "try again". Releasing a BF16 kind releases its BF16LO partner too (the split filter needs the pair). The next
 * call that wants a released copy builds it again under the rules of that moment; results never change. Kinds that do not exist
 * are skipped.
 * Out of scope: automatic eviction under memory pressure, re-trying a refused copy every Nth call by itself, the batch's store
 * and norms, a view's parent, sharded corpora (release on each rank's shard). */
innr_status innr_batch_release_copies(innr_batch* b, uint32_t mask);
/* Build the kinds in `mask` now instead of inside the first query that wants them (seconds at 30 GB), through the builders the
 * engines use. The "fits with room to spare" rule does not apply -- the caller asked: a failed hipMalloc is INNR_E_OOM. Skipped,
 * without an error: a kind that cannot exist for this batch (bf16 kinds and rows on a u8 code batch, int8 kinds other than DOT
 * there, an int8 kind whose corpus has nothing to quantise against, every matrix-pipe copy of a view whose length has no
 * matrix-pipe engine, of an empty batch), a kind the copy budget does not admit, and INNR_COPY_SELECTION (there is no mask to
 * select with). *built_mask (may be null) = the kinds of `mask` present at return, already existing ones included.
 * Out of scope: building in the background, choosing kinds from the call history (innr_batch_auto_engine stays a pure function
 * of the batch and Q), sharded corpora. */
innr_status innr_batch_build_copies(innr_batch* b, uint32_t mask, uint32_t* built_mask);
/* The copy budget of a batch: a derived allocation is made only if derived_bytes + its size <= budget (UINT64_MAX = unlimited,
 * the default, unless the context option copy_budget_mib -- INNR_COPY_BUDGET_MIB, -1 = unlimited -- said otherwise when the batch
 * was created; batches that exist keep theirs). What a refused allocation means is what it meant already: an explicit
 * INNR_KNN_MFMA_BF16 / _I8 request and INNR_KNN_AUTO are served by INNR_KNN_MFMA (stats->engine tells), the split filter by the
 * f32-pipe filter, the rows copy by column gathers, the selection by the masked exact scan. A budget refusal is evaluated per
 * call and never remembered: raise the budget and the next call builds. The selection's own copies count against its parent's
 * budget. Lowering the budget below the current use frees nothing -- existing copies keep being used; the caller decides what to
 * release. The squared-L2 int8 copy is admitted by its upper bound (D + 121 dimensions).
 * Out of scope: automatic eviction, budgets for document corpora or the context's workspace, moving the free-memory query
 * out of INNR_KNN_AUTO, one budget across several batches or ranks. */
innr_status innr_batch_set_copy_budget(innr_batch* b, uint64_t bytes);
innr_status innr_batch_get_copy_budget(const innr_batch* b, uint64_t* bytes);
/* the same report for a document corpus: *corpus_bytes = tokens + doc_len, *derived_bytes = the token norms the MFMA engine
 * builds on first use. Out pointers may be null; a null corpus is INNR_E_BAD_ARG. Out of scope: release, budget. */
innr_status innr_docs_memory(const innr_docs* d, uint64_t* corpus_bytes, uint64_t* derived_bytes);
/* *workspace_bytes = the device workspace of the context (grow-only buffers shared by every call on it). */
innr_status innr_ctx_memory(innr_ctx* ctx, uint64_t* workspace_bytes);
/* Give the workspace back (after synchronising the stream): every buffer a call sizes for itself is freed and grows again on
 * demand; the 4 KiB flag block, which is set up once in innr_ctx_create, stays, and so do the pinned staging area, the stream
 * and the events. Results never change; the next calls pay their hipMallocs again.
 * Out of scope: trimming to a target size, trimming by itself. */
innr_status innr_ctx_trim(innr_ctx* ctx);

/* ---- multi-GPU merge (range partition + all-gather of per-shard top-k) --------- */
/* in: G shards x Q queries x kin candidates (device pointers, layout [g][q][kin], global indices);
 * out: best kout per query by (score order of `metric`, index ascending). */
innr_status innr_merge_topk_dev(innr_ctx* ctx, int metric, const uint64_t* d_idx, const float* d_score, size_t G,
                                size_t Q, size_t kin, size_t kout, uint64_t* d_out_idx, float* d_out_score);


/* ---- the exchange step of the sharded path, behind the boundary ------------------------------------
 * The reference is one process, one thread (no counterpart in its source); north_star: "the corpus is range-partitioned
 * across the 8 GPUs of one node with a final RCCL all-gather of per-shard top-k candidates over xGMI". One process per
 * GPU; every rank holds an innr_ctx on its GPU and an innr_comm = that ctx + an RCCL communicator over all ranks. The
 * library loads librccl at run time (the copy already mapped into the process, e.g. PyTorch's, else the system one);
 * a failure of any RCCL call, or no RCCL library, is INNR_E_RCCL. All collectives run on the ctx stream. */
typedef struct innr_comm innr_comm;
#define INNR_COMM_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
/* rank 0: a fresh id (ncclGetUniqueId) that the host ships to the other ranks by its own means (env, file, socket,
 * torch.distributed store); then EVERY rank calls innr_comm_create with the same id -- collective, like ncclCommInitRank */
innr_status innr_comm_unique_id(void* id_out /* [INNR_COMM_ID_BYTES] */);
innr_status innr_comm_create(innr_ctx* ctx, const void* id, int rank, int world, innr_comm** out);
/* or borrow a communicator the host already owns (ncclComm_t as void*; its device must be the ctx's); never destroyed here */
innr_status innr_comm_attach(innr_ctx* ctx, void* nccl_comm, int rank, int world, innr_comm** out);
void innr_comm_destroy(innr_comm* comm);
int innr_comm_rank(const innr_comm* comm);
int innr_comm_world(const innr_comm* comm);

/* The exchanged unit: one BLOCK per rank = 2 + Q*k uint64:  [0] the shard's index base, [1] its vector count,
 * [2 + q*k + r] = candidate r of query q as {low 32 bits: index local to the shard (0xFFFFFFFF = no candidate),
 * high 32 bits: the f32 score bits} -- 8 bytes per entry (Q*k*8 bytes per rank).
 * innr_topk_pack_dev: a shard's kNN result (d_idx global indices [Q*kin], d_score [Q*kin], kin <= k) -> its block. */
size_t innr_topk_block_words(size_t Q, size_t k); /* = 2 + Q*k */
innr_status innr_topk_pack_dev(innr_ctx* ctx, const uint64_t* d_idx, const float* d_score, uint64_t index_base,
                               uint64_t shard_vectors, size_t Q, size_t kin, size_t k, uint64_t* d_block);
/* ONE ncclAllGather of every rank's block: d_all_blocks[world][2 + Q*k] (device), in rank order */
innr_status innr_allgather_topk_dev(innr_comm* comm, const uint64_t* d_block, size_t Q, size_t k, uint64_t* d_all_blocks);
/* merge G gathered blocks: best min(k, total vectors) per query by (score order of `metric`, GLOBAL index ascending) --
 * with contiguous ranges this is the reference's stable-sort tie rule (batch.rs:757) over the whole corpus.
 * d_out_idx / d_out_score: [Q][k'] with k' = *out_k. */
innr_status innr_merge_blocks_dev(innr_ctx* ctx, int metric, const uint64_t* d_all_blocks, size_t G, size_t Q, size_t k,
                                  uint64_t* d_out_idx, float* d_out_score, size_t* out_k);
/* The whole sharded call on every rank: local kNN on this rank's shard (f32 batch: `metric`; u8 code batch: the
 * asymmetric dot, metric ignored) + pack + all-gather + merge. Queries identical on every rank (device, [Q*D]); outputs
 * (device, sized Q*min(k, total vectors)) identical on every rank; stats describe the local search. */
innr_status innr_sharded_knn_dev(innr_comm* comm, innr_batch* shard, int metric, const float* d_queries, size_t Q, size_t D,
                                 size_t k, int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k,
                                 innr_knn_stats* stats);
/* the same with host buffers (what the Rust shim's sharded::Comm::knn binds; out arrays sized Q*k) */
innr_status innr_sharded_knn(innr_comm* comm, innr_batch* shard, int metric, const float* queries, size_t Q, size_t D, size_t k,
                             int engine, uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* maxsim over a document corpus range-partitioned across the ranks (maxsim.rs:96-137 per document; SURVEY.md 8e: "same scheme
 * for maxsim"): innr_maxsim_topk on this rank's shard (documents [base, base + count): innr_docs_set_index_base), then the same
 * exchange -- one block of 2 + k words per rank, ONE ncclAllGather, merge by (score, global document index). Query and outputs
 * as in innr_maxsim_topk (host; identical on every rank; out arrays sized k). */
innr_status innr_sharded_maxsim(innr_comm* comm, innr_docs* shard, int cosine, const float* qtok, size_t Tq, size_t dim, size_t k,
                                int engine, uint64_t* out_doc, float* out_score, size_t* out_k, innr_knn_stats* stats);
/* Failure semantics of the innr_sharded_* calls: the collective is SYMMETRIC. A rank whose local search fails (a filter copy that
 * does not fit on that GPU, a dimension mismatch, ...) still takes part in the all-gather, with a block whose header says so;
 * that rank returns its own status, every other rank INNR_E_RCCL naming the failed rank, none of them a result -- no rank waits
 * in a collective its peer never entered. After a failed RCCL call itself the communicator is unusable: innr_comm_destroy
 * then aborts it (ncclCommAbort) instead of destroying it. The shard sizes are learnt from the first exchange and cached in
 * the communicator, so a steady-state call synchronises with the host once, at its end. */

#ifdef __cplusplus
}
#endif
#endif /* INNR_HIP_H */
