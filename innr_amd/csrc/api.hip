// api.hip -- the extern "C" boundary (include/innr_hip.h) over the gfx950 kernels: contexts, batches, the kNN engines, the u8 and
// int8 paths, range search, memory. maxsim lives in maxsim.hip, batch_knn_adaptive in adaptive.hip, the multi-GPU layer in comm.hip, the full sort in sort_full.hip;
// what they share with this file is api_internal.h.
#include <ctype.h>
#include <stdarg.h>
#include <stdio.h>

#include <memory>

#include "api_internal.h"
#include "kernels_prep.h"
#include "kernels_scan.h"
#include "kernels_topk.h"
#include "kernels_gemm.h"
#include "kernels_gemm_bf16.h"
#include "kernels_ext.h"
#include "kernels_u8.h"
#include "kernels_gemm_i8.h"
#include "kernels_select.h"

namespace innr {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace innr

struct TuneName { const char* name; long innr_tuning::*field; };
static const TuneName kTuneNames[] = {
    {"gemm_waves", &innr_tuning::gemm_waves}, {"gemm_blocks_per_cu", &innr_tuning::gemm_blocks_per_cu},
    {"gemm_qt_group", &innr_tuning::gemm_qt_group}, {"gemm_seed_n", &innr_tuning::gemm_seed_n},
    {"gemm_no_seed", &innr_tuning::gemm_no_seed}, {"gemm_no_kp_retry", &innr_tuning::gemm_no_kp_retry},
    {"i8_two_limb", &innr_tuning::i8_two_limb}, {"no_auto_bf16", &innr_tuning::no_auto_bf16},
    {"no_auto_i8", &innr_tuning::no_auto_i8}, {"u8_no_i8", &innr_tuning::u8_no_i8}, {"rescore_all", &innr_tuning::rescore_all},
    {"maxsim_generic", &innr_tuning::maxsim_generic}, {"no_k_rule", &innr_tuning::no_k_rule},
    {"fail_local_search", &innr_tuning::fail_local_search}, {"no_completion", &innr_tuning::no_completion}, {"trace", &innr_tuning::trace}, {"no_rows_copy", &innr_tuning::no_rows_copy},
    {"i8_slices_per_cu", &innr_tuning::i8_slices_per_cu}, {"i8_no_small", &innr_tuning::i8_no_small},
    {"i8_no_small4", &innr_tuning::i8_no_small4}, {"i8_small_max_q", &innr_tuning::i8_small_max_q},
    {"i8_small_free", &innr_tuning::i8_small_free}, {"no_split_filter", &innr_tuning::no_split_filter},
    {"split_min_q", &innr_tuning::split_min_q}, {"no_split_screen", &innr_tuning::no_split_screen}, {"split_screen_worst_case", &innr_tuning::split_screen_worst_case}, {"split_seed_rows", &innr_tuning::split_seed_rows}, {"filter_keep_selection", &innr_tuning::filter_keep_selection},
    {"copy_budget_mib", &innr_tuning::copy_budget_mib}, {"scan_max_slots", &innr_tuning::scan_max_slots},
    {"mutate_round", &innr_tuning::mutate_round}, {"range_u8_i8_min_n", &innr_tuning::range_u8_i8_min_n},
};
static void tuning_from_env(innr_tuning* t) {
    for (const TuneName& n : kTuneNames) {
        char env[64] = "INNR_";
        size_t o = 5;
        for (const char* p = n.name; *p && o + 1 < sizeof(env); ++p) env[o++] = (char)toupper((unsigned char)*p);
        env[o] = 0;
        if (const char* e = getenv(env)) t->*(n.field) = atol(e);
    }
}

// Every workspace DevBuf of a context (innr_ctx_destroy, innr_ctx_memory, innr_ctx_trim). All but `flags` are sized by the calls
// that use them (an ensure() in front of every use) and carry nothing from one call to the next; `flags` is allocated and zeroed
// once, in innr_ctx_create, and the kernels' error words live there between the calls' own memsets: innr_ctx_trim keeps it.
static std::vector<DevBuf*> workspace_bufs(innr_ctx* c) {
    return {&c->gthr, &c->sel_tmp[0], &c->sel_tmp[1], &c->selcnt_tmp[0], &c->selcnt_tmp[1],
            &c->q_row, &c->q_kmajor, &c->q_norm, &c->lists, &c->counts, &c->sel, &c->sel_cnt,
            &c->scores, &c->tmp_norms, &c->flags, &c->out_idx, &c->out_score, &c->misc, &c->seed_idx, &c->seed_score, &c->q_one, &c->sort_keys, &c->sort_tmp, &c->q_bf16, &c->q_pad, &c->q_hat,
            &c->redo[0].q, &c->redo[0].idx, &c->redo[0].sc, &c->redo[0].map, &c->redo[0].qn,
            &c->redo[1].q, &c->redo[1].idx, &c->redo[1].sc, &c->redo[1].map, &c->redo[1].qn, &c->kmargin, &c->i8s_prog,
            &c->cmpl.q, &c->cmpl.idx, &c->cmpl.sc, &c->cmpl.map, &c->cmpl.qn, &c->flt_in, &c->flt_mask, &c->flt_scan,
            &c->rs_cnt, &c->rs_bits, &c->rs_tot, &c->rs_thr, &c->rs_off, &c->adp_scan, &c->adp_list,
            &c->rows_q, &c->rows_stage, &c->rows_io, &c->rows_flag, &c->rows_bits, &c->rows_map};
}

// kernel_of(Inst) of the recorded families whose kernels this file owns (api_internal.h: Inst, launch_kernel)
template <int KIND, int RR, int MODE, int WV> constexpr auto kernel_of(Inst<kLaunchGemmF32, KIND, RR, MODE, WV>) { return &gemm_filter_kernel<KIND, RR, MODE, WV>; }
template <int RR, int MODE> constexpr auto kernel_of(Inst<kLaunchGemmBf16, RR, MODE, 1>) { return &gemm_bf16_filter_kernel<RR, MODE, 1>; }
template <int RR, int MODE> constexpr auto kernel_of(Inst<kLaunchGemmSplit, RR, MODE, 3>) { return &gemm_bf16_filter_kernel<RR, MODE, 3>; }
// ... the same record's screened form (MODE 0: hi.hi K-loop, lo products where a wave can hit; launch_gemm_split chooses)
template <int RR> constexpr auto kernel_of(Inst<kLaunchSplitSeed, RR, 3, 3>) { return &gemm_bf16_filter_kernel<RR, 3, 3>; }
template <int RR> constexpr auto screened_kernel_of(Inst<kLaunchGemmSplit, RR, 0, 3>) { return &gemm_bf16_filter_kernel<RR, 0, 3, 1>; }
template <int RR, int MODE> constexpr auto kernel_of(Inst<kLaunchI8One, RR, MODE>) { return &gemm_i8h_filter_kernel<RR, MODE>; }
template <int RR, int MODE> constexpr auto kernel_of(Inst<kLaunchI8Two, RR, MODE>) { return &gemm_i8_filter_kernel<RR, MODE>; }
template <int NK, int CT, int MODE> constexpr auto kernel_of(Inst<kLaunchI8Small, NK, CT, MODE>) { return &gemm_i8s_filter_kernel<12, NK, CT, MODE>; }
template <int QB, int MET, int EMIT> constexpr auto kernel_of(Inst<kLaunchRangeScan, QB, MET, EMIT>) {
    return &range_scan_kernel<QB, MET == INNR_METRIC_L2SQ, MET == INNR_METRIC_COSINE, EMIT != 0>;
}
template <int QB, int RR> constexpr auto kernel_of(Inst<kLaunchScanU8Masked, QB, RR>) { return &scan_u8_filter_kernel<QB, RR, true>; }
template <int QB, int EMIT> constexpr auto kernel_of(Inst<kLaunchRangeScanU8, QB, EMIT>) { return &range_scan_u8_kernel<QB, EMIT != 0>; }

static auto metric_of(int metric) { return one_of<INNR_METRIC_COSINE, INNR_METRIC_L2SQ, INNR_METRIC_DOT>(metric); }
// RR (R in the kernels) of a list capacity of 64 RR entries: the GEMM-type filters have lists of 32 / 64 / 128 / 256 candidates
// (cand_cap: 384 / 512 / 768 / 1280 entries), the exact scans of 32 / 128 / 256 (exact_cap)
static auto rr_gemm(uint32_t cap) { return one_of<6, 8, 12, 20>(cap / 64); }

// The score space of a proof: rescore_kernel's MET, seed_thresholds_kernel's and kmargin_kernel's kind.
enum ScoreSpace : int { kSpaceDot = 0, kSpaceCos = 1, kSpaceL2 = 2, kSpaceEq = 3, kSpaceCode = 4 };
static ScoreSpace metric_space(int metric) {
    return metric == INNR_METRIC_L2SQ ? kSpaceL2 : (metric == INNR_METRIC_COSINE ? kSpaceCos : kSpaceDot);
}
// the template arguments of the exact kernels: MET of a metric's score space, RK (rounds of candidates) of lists of KP
template <class F>
static void with_space(ScoreSpace space, F&& f) {
    if (space == kSpaceCos) f(IntC<kSpaceCos>());
    else if (space == kSpaceL2) f(IntC<kSpaceL2>());
    else f(IntC<kSpaceDot>());
}
template <class F>
static void with_rk(uint32_t KP, F&& f) {
    if (KP <= 64) f(IntC<1>());
    else if (KP <= 128) f(IntC<2>());
    else f(IntC<4>());
}

namespace innr {
constexpr size_t kPinIn = 512 << 10, kPinOut = 768 << 10, kPinSmall = 256 << 10;

// host -> device; small buffers go through the pinned staging area (valid until the next ctx_sync)
hipError_t copy_in(innr_ctx* c, void* dst, const void* src, size_t bytes) {
    if (c->pin && bytes <= kPinSmall && c->pin_in_off + bytes <= kPinIn) {
        char* st = c->pin + c->pin_in_off;
        memcpy(st, src, bytes);
        c->pin_in_off += (bytes + 255) & ~(size_t)255;
        return hipMemcpyAsync(dst, st, bytes, hipMemcpyHostToDevice, c->stream);
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
}

// device -> host; small buffers land in pinned memory and reach `dst` at the next ctx_sync
hipError_t copy_out(innr_ctx* c, void* dst, const void* src, size_t bytes) {
    if (c->pin && bytes <= kPinSmall && c->pin_out_off + bytes <= kPinOut) {
        char* st = c->pin + kPinIn + c->pin_out_off;
        c->pin_out_off += (bytes + 255) & ~(size_t)255;
        c->pending.push_back({dst, st, bytes});
        return hipMemcpyAsync(st, src, bytes, hipMemcpyDeviceToHost, c->stream);
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
}

// stream synchronise + deliver the staged outputs + recycle the staging area
hipError_t ctx_sync(innr_ctx* c) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess)
        for (const auto& po : c->pending) memcpy(po.user, po.staged, po.bytes);
    c->pending.clear();
    c->pin_in_off = c->pin_out_off = 0;
    return e;
}

// which copy a call of a metric filters on: the bf16 kinds (lo: the split filter's lo limbs, dot and cosine only) and the int8 kinds
static CopyKind bf16_kind(int metric, bool lo = false) {
    if (metric == INNR_METRIC_COSINE) return lo ? kCopyBfCosLo : kCopyBfCos;
    return lo ? kCopyBfDotLo : (metric == INNR_METRIC_L2SQ ? kCopyBfL2 : kCopyBfDot);
}
static CopyKind i8_kind(int metric) {
    return metric == INNR_METRIC_COSINE ? kCopyI8Cos : (metric == INNR_METRIC_L2SQ ? kCopyI8L2 : kCopyI8Dot);
}

// The memory rule of every copy that is built unasked: it may be built when free memory is at least twice its size plus 8 GiB
static bool copy_fits(size_t free_bytes, size_t copy_bytes) { return free_bytes >= 2 * copy_bytes + ((size_t)8 << 30); }

// ---- memory accounting: every number is what was passed to hipMalloc ----
// the public bit of a copy kind (INNR_COPY_ROWS .. INNR_COPY_I8_L2 are 1 << CopyKind, in CopyKind's order)
static uint32_t copy_bit(int kind) { return 1u << kind; }
static_assert(INNR_COPY_ROWS == 1u << kCopyRows && INNR_COPY_BF16_DOT == 1u << kCopyBfDot && INNR_COPY_BF16_COS == 1u << kCopyBfCos &&
                  INNR_COPY_BF16_L2 == 1u << kCopyBfL2 && INNR_COPY_BF16LO_DOT == 1u << kCopyBfDotLo &&
                  INNR_COPY_BF16LO_COS == 1u << kCopyBfCosLo && INNR_COPY_I8_DOT == 1u << kCopyI8Dot &&
                  INNR_COPY_I8_COS == 1u << kCopyI8Cos && INNR_COPY_I8_L2 == 1u << kCopyI8L2 &&
                  INNR_COPY_SELECTION == 1u << kCopyKinds && INNR_COPY_ALL == (2u << kCopyKinds) - 1,
              "the INNR_COPY_* bits follow CopyKind");
// one of a batch's auxiliary arrays (norms and their by-products), its size recorded for innr_batch_memory
template <class T>
static hipError_t alloc_aux(innr_batch* b, T** p, size_t bytes) {
    const hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess) b->aux_bytes += bytes;
    return e;
}
static size_t corpus_copy_bytes(const innr_batch* b, uint32_t mask = INNR_COPY_ALL) {
    size_t sum = 0;
    for (int k = 0; k < kCopyKinds; ++k)
        if ((mask & copy_bit(k)) && b->copy[k].p) sum += b->copy[k].bytes;
    return sum;
}
// the selection without what the selection batch built for itself: its store, the mask and the map
static size_t selection_base_bytes(const innr_batch* b) {
    return b->fsel ? b->fsel->corpus_bytes + b->fsel_mask_bytes + b->fsel_map_bytes : 0;
}
// INNR_COPY_SELECTION: ... plus the selection batch's own copies (a selection has no selection of its own; its norms -- 12 bytes
// per vector at most -- are not counted, like the batch's own)
static size_t selection_bytes(const innr_batch* b) { return b->fsel ? selection_base_bytes(b) + corpus_copy_bytes(b->fsel) : 0; }
static size_t derived_bytes(const innr_batch* b, uint32_t mask = INNR_COPY_ALL) {
    return corpus_copy_bytes(b, mask) + ((mask & INNR_COPY_SELECTION) ? selection_bytes(b) : 0);
}
// The budget rule of every derived allocation, asked or unasked: it is made only if derived_bytes + its size <= the batch's copy
// budget. Evaluated where the allocation is decided, never remembered (CorpusCopy::refused is about free memory, not about this);
// nothing to allocate is always admitted, so copies that exist keep being used under a budget lowered below them.
// `have`: what counts as derived already -- everything, except for a selection, which takes the place of the one it replaces.
static bool budget_admits(const innr_batch* b, size_t bytes, size_t have) {
    if (b->copy_budget == UINT64_MAX || bytes == 0) return true;
    return have <= b->copy_budget && bytes <= b->copy_budget - have;
}
static bool budget_admits(const innr_batch* b, size_t bytes) { return budget_admits(b, bytes, derived_bytes(b)); }

// Device memory for copy `kind` (`what` names it in the error message); the caller packs into copy[kind].p. Two policies:
// hard (the bf16 and int8 filter copies, which a call cannot do without): a failed hipMalloc is INNR_E_OOM;
// soft (the rows copy, the lo limbs): the memory rule first, and when it or hipMalloc says no the refusal sticks, the HIP error
// is cleared and the call goes on without the copy -- INNR_OK with a null pointer.
// Either way the budget comes first (budget_admits): a soft copy it does not admit is left out for this call, without the sticky
// refusal; the hard sites resolve the budget where the engine is chosen (innr_batch_knn_dev, innr_batch_knn_u8_dev,
// innr_batch_build_copies), so for them a refusal here is an internal error.
static innr_status alloc_copy(innr_batch* b, CopyKind kind, size_t bytes, uint32_t nk, bool soft, const char* what) {
    CorpusCopy& cc = b->copy[kind];
    if (!budget_admits(b, bytes)) {
        if (soft) return INNR_OK;
        set_error("internal: the %s (%zu bytes) is beyond the batch's copy budget", what, bytes);
        return INNR_E_OOM;
    }
    size_t free_b = 0, total_b = 0;
    const bool fits = !soft || (hipMemGetInfo(&free_b, &total_b) == hipSuccess && copy_fits(free_b, bytes));
    const hipError_t e = fits ? hipMalloc((void**)&cc.p, bytes) : hipErrorOutOfMemory;
    if (e == hipSuccess) {
        cc.bytes = bytes;
        cc.nk = nk;
        return INNR_OK;
    }
    cc.p = nullptr;
    if (!soft) {
        set_error("hipMalloc(%zu bytes) for the %s failed: %s", bytes, what, hipGetErrorString(e));
        return INNR_E_OOM;
    }
    (void)hipGetLastError();
    cc.refused = true;
    return INNR_OK;
}

innr_status bind_device(innr_ctx* ctx) {
    INNR_HIP_CHECK(hipSetDevice(ctx->device));
    return INNR_OK;
}

// the copy budget a new batch starts with: the context option copy_budget_mib (< 0: unlimited)
static uint64_t budget_from_option(const innr_ctx* ctx) {
    const long mib = ctx->tune.copy_budget_mib;
    return (mib < 0 || mib >= (1L << 43)) ? UINT64_MAX : (uint64_t)mib << 20;
}

innr_status alloc_batch(innr_ctx* ctx, size_t N, size_t D, innr_batch** out) {
    if (!ctx || !out) {
        set_error("null ctx/out");
        return INNR_E_BAD_ARG;
    }
    if (N >= kMaxBatchN || D > 0x7FFFFFFFull) {
        set_error("corpus shard too large for u32 device indices (N=%zu, D=%zu)", N, D);
        return INNR_E_UNSUPPORTED;
    }
    INNR_ENTER(ctx);
    innr_batch* b = new (std::nothrow) innr_batch();
    if (!b) return INNR_E_OOM;
    b->ctx = ctx;
    b->N = N;
    b->D = D;
    b->ldN = round_up(N ? N : 1, 256);
    b->Dpad = round_up(D ? D : 1, 32);
    const size_t bytes = b->ldN * b->Dpad * sizeof(float);
    hipError_t e = hipMalloc((void**)&b->V, bytes);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for corpus failed: %s", bytes, hipGetErrorString(e));
        delete b;
        return INNR_E_OOM;
    }
    b->corpus_bytes = bytes;
    b->copy_budget = budget_from_option(ctx);
    e = hipMemsetAsync(b->V, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
        set_error("hipMemsetAsync failed: %s", hipGetErrorString(e));
        (void)hipFree(b->V);
        delete b;
        return INNR_E_HIP;
    }
    *out = b;
    return INNR_OK;
}

hipError_t transpose_rows_into(innr_ctx* c, const float* d_rows, size_t n, size_t D, float* V, size_t ldN, size_t col0) {
    if (n == 0 || D == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)((D + 31) / 32));
    transpose_rows_kernel<<<grid, 256, 0, c->stream>>>(d_rows, (uint32_t)n, (uint32_t)D, V, ldN, col0);
    return hipGetLastError();
}

static innr_status ensure_norms(innr_batch* b) {
    if (b->norms_ready) return INNR_OK;
    innr_ctx* ctx = b->ctx;
    if (!b->norms) {
        INNR_HIP_CHECK(alloc_aux(b, &b->norms, b->ldN * sizeof(float)));
        INNR_HIP_CHECK(alloc_aux(b, &b->max_norm_bits, sizeof(uint32_t)));
    }
    INNR_HIP_CHECK(hipMemsetAsync(b->max_norm_bits, 0, sizeof(uint32_t), ctx->stream));
    const unsigned blocks = (unsigned)((b->ldN / 4 + 255) / 256);
    norms_kernel<<<blocks, 256, 0, ctx->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, b->norms,
                                                   b->max_norm_bits);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t bits = 0;
    INNR_HIP_CHECK(copy_out(ctx, &bits, b->max_norm_bits, sizeof(bits)));
    INNR_HIP_CHECK(ctx_sync(ctx));
    memcpy(&b->max_norm, &bits, 4);
    b->norms_ready = true;
    return INNR_OK;
}

bool metric_ok(int m) { return m == INNR_METRIC_DOT || m == INNR_METRIC_L2SQ || m == INNR_METRIC_COSINE; }

uint32_t pick_kp(size_t k, size_t margin) {
    uint32_t kp = 32;
    while (kp < k + margin) kp <<= 1;
    return kp;
}

// Cross-producer selection: best KP per query over `nslots` lists (each <= KP entries), tree-reduced in parts of
// kSelSlots/KP lists until one part remains. Result: c->sel [Q][KP] best-first, c->sel_cnt [Q].
innr_status run_select(innr_ctx* c, const uint64_t* lists, const uint32_t* counts, uint32_t nslots,
                              uint32_t qstride, uint32_t cap, uint32_t KP, uint32_t Q) {
    INNR_TRY(c->sel.ensure((size_t)Q * KP * sizeof(uint64_t)));
    INNR_TRY(c->sel_cnt.ensure((size_t)Q * sizeof(uint32_t)));
    const uint32_t spp = kSelSlots / KP;
    int level = 0;
    while (true) {
        const uint32_t parts = (nslots + spp - 1) / spp;
        uint64_t* out = c->sel.as<uint64_t>();
        uint32_t* out_cnt = c->sel_cnt.as<uint32_t>();
        if (parts > 1) {
            INNR_TRY(c->sel_tmp[level & 1].ensure((size_t)parts * Q * KP * sizeof(uint64_t)));
            INNR_TRY(c->selcnt_tmp[level & 1].ensure((size_t)parts * Q * sizeof(uint32_t)));
            out = c->sel_tmp[level & 1].as<uint64_t>();
            out_cnt = c->selcnt_tmp[level & 1].as<uint32_t>();
        }
        select_topk_kernel<<<dim3(Q, parts ? parts : 1), kSelThreads, 0, c->stream>>>(lists, counts, nslots, qstride,
                                                                                      cap, KP, Q, out, out_cnt);
        INNR_HIP_CHECK(hipGetLastError());
        if (parts <= 1) return INNR_OK;
        lists = out;
        counts = out_cnt;
        nslots = parts;
        qstride = Q;
        cap = KP;
        ++level;
    }
}

// The one launch site of emit_results_kernel (kernels_topk.h): the first kout composites of each of Q rows of KP -> index base +
// index and score, on the context's stream
innr_status emit_results(innr_ctx* c, const uint64_t* sel, size_t KP, size_t Q, size_t kout, bool smaller_is_better, uint64_t index_base,
                         uint64_t* out_idx, float* out_score) {
    const size_t total = Q * kout;
    emit_results_kernel<<<(unsigned)((total + 255) / 256), 256, 0, c->stream>>>(sel, (uint32_t)KP, (uint32_t)Q, (uint32_t)kout,
                                                                               smaller_is_better, index_base, out_idx, out_score);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ---- exact engine ---------------------------------------------------------------------------------
// list capacity used by the exact engine for a given KP: 64*R with R in {6, 12, 20}
uint32_t exact_cap(uint32_t KP) { return KP <= 32 ? 384u : (KP <= 128 ? 768u : 1280u); }

// optional extras of the L2 variants (device pointers; both null for the plain scans)
struct ScanExt {
    const uint8_t* mask = nullptr;    // [ldN] predicate bytes (batch_knn_filtered; all three metrics: innr_batch_knn_filtered_multi)
    const uint32_t* order = nullptr;  // [D] dimension order (batch_knn_reordered)
    uint32_t nvalid = 0xFFFFFFFFu;    // query slots of the launch beyond this one are padding (zero rows): nothing is admitted for them
};

// one launch of scan_filter_kernel: `groups` groups of qb (8, 4 or 1) queries. (The exact scans are not a recorded family: one runs
// inside most recorded calls -- threshold seeding, the redo of unproven queries -- and the record's readers decode a closed set.
// They have a record of their own, innr_ctx::scan_log, with the geometry of each launch.)
static innr_status launch_scan_filter(innr_batch* b, int metric, uint32_t qb, const float* dQ, size_t ldq, const float* dQn,
                                      uint32_t nblocks, uint32_t qstride, uint32_t KP, uint32_t cap, uint32_t cps,
                                      const ScanExt& ext, uint32_t groups) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    // the extended kernel: a mask (innr_batch_knn_filtered_multi, every metric) or a dimension order (squared L2 only)
    const uint32_t* order = l2 ? ext.order : nullptr;
    dispatch([&](auto QB, auto met, auto rr, auto extended) {
        record_scan(c, kScanF32, QB, met, rr, extended != 0, cps, (size_t)nblocks * (kScanThreads / 64), groups);
        scan_filter_kernel<QB, met == INNR_METRIC_L2SQ, met == INNR_METRIC_COSINE, rr, extended != 0>
            <<<dim3(nblocks, groups), kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, dQ, ldq, cos ? b->norms : nullptr, cos ? dQn : nullptr, c->lists.as<uint64_t>(),
                c->counts.as<uint32_t>(), qstride, KP, cps, c->flags.as<uint32_t>(), ext.mask, order, ext.nvalid);
    }, one_of<8, 4, 1>(qb), metric_of(metric), rr_scan(cap), flag(ext.mask || order));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// A ragged group of an exact scan: rows [nreal, nql) of *q (row stride ldq) are zero queries, with a zero per-query value (*aux,
// nullable: the norm / the code sum), whose results are dropped; *q and *aux then point at the padded copy
static innr_status pad_queries(innr_ctx* c, size_t ldq, size_t D, uint32_t nql, uint32_t nreal, const float** q, const float** aux) {
    const size_t row_bytes = ldq * sizeof(float);
    INNR_TRY(c->q_pad.ensure(nql * row_bytes + nql * sizeof(float) + 16));
    INNR_HIP_CHECK(hipMemsetAsync(c->q_pad.p, 0, nql * row_bytes + nql * sizeof(float), c->stream));
    if (D)
        INNR_HIP_CHECK(hipMemcpy2DAsync(c->q_pad.p, row_bytes, *q, row_bytes, D * sizeof(float), nreal, hipMemcpyDeviceToDevice, c->stream));
    float* aux_pad = reinterpret_cast<float*>(c->q_pad.as<char>() + nql * row_bytes);
    if (*aux) {
        INNR_HIP_CHECK(hipMemcpyAsync(aux_pad, *aux, nreal * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        *aux = aux_pad;
    }
    *q = c->q_pad.as<float>();
    return INNR_OK;
}
// ... and its end: the best KP per query slot over the scan's lists, the first kout of the nreal real queries written out
static innr_status select_and_emit(innr_batch* b, uint32_t nslots, uint32_t nql, uint32_t cap, uint32_t KP, uint32_t nreal, size_t kout,
                                   bool l2, uint64_t* d_out_idx, float* d_out_score) {
    innr_ctx* c = b->ctx;
    INNR_TRY(run_select(c, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), nslots, nql, cap, KP, nql));
    return emit_results(c, c->sel.as<uint64_t>(), KP, nreal, kout, l2, b->index_base, d_out_idx, d_out_score);
}

// How an exact scan lays a corpus out over the chip
struct ScanGeom {
    size_t cols;          // columns that are scanned
    size_t chunk;         // ... in chunks of this many
    size_t waves_per_cu;  // wave slots: never more than this per CU, nor than there are chunks
    size_t block_waves;   // ... a whole number of blocks of this many waves
    size_t bytes;         // what one pass reads: a corpus within the Infinity Cache takes all its groups in one launch
    bool l2;              // smaller is better
};

// The rounds of an exact scan, f32 or code corpus, for queries [q0, q0+nq) (row-major on device, stride ldq; aux: the per-query value,
// nullable): results to d_out_* at row q0. launch(qb, q, aux, nblocks, nql, KP, cap, cps, groups, nreal) scans for `groups` groups
// of qb queries -- nql slots, the first nreal of them real -- into c->lists / c->counts.
template <class Launch>
static innr_status exact_scan_rounds(innr_batch* b, const ScanGeom& g, const float* dQ, size_t ldq, const float* aux, size_t q0,
                                     size_t nq, size_t kout, uint64_t* d_out_idx, float* d_out_score, Launch&& launch) {
    innr_ctx* c = b->ctx;
    const uint32_t KP = pick_kp(kout, 0);
    const uint32_t cap = exact_cap(KP);
    const size_t nchunks = g.cols / g.chunk;
    size_t nslots = cap_scan_slots(c, std::min<size_t>(nchunks, (size_t)c->num_cus * g.waves_per_cu));
    nslots = round_up(nslots, g.block_waves);
    const uint32_t cps = (uint32_t)((nchunks + nslots - 1) / nslots);
    const uint32_t nblocks = (uint32_t)(nslots / g.block_waves);
    constexpr uint32_t QBMAX = 8;
    // A corpus that stays in the Infinity Cache (<= 128 MB) is cheap to re-read and too small to fill the chip with
    // one group of 8 queries: all the 8-query groups go into ONE launch (blockIdx.y), within 256 MB of list space.
    // Large corpora keep one group per launch (each launch streams HBM once and fills the chip by itself).
    size_t max_groups = 1;
    if (g.bytes <= (size_t)128 << 20) max_groups = std::max<size_t>(1, ((size_t)256 << 20) / (nslots * QBMAX * cap * sizeof(uint64_t)));
    max_groups = std::min<size_t>(max_groups, 65535);
    size_t done = 0;
    while (done < nq) {
        const size_t rem = nq - done;
        // One corpus pass serves 8, 4 or 1 queries. A ragged tail of 5-7 (2-3) queries takes ONE 8- (4-) query pass with
        // zero rows as padding instead of several smaller passes (2 queries: 5.5 ms instead of 2 x 5.2 at 10M x 768; on a code
        // corpus the 8-query pass costs less than two of 4: one corpus stream, one widening of each code).
        const uint32_t qb = rem >= 5 ? 8 : (rem >= 2 ? 4 : 1);
        // (only 8-query passes come in several groups: with qb == 4, rem <= 4, so "qb > 1 && rem >= qb ? rem / qb" gives 1 as well)
        const uint32_t groups = (qb == 8 && rem >= 8) ? (uint32_t)std::min<size_t>(rem / 8, max_groups) : 1u;
        const uint32_t nql = qb * groups;                               // query slots of this launch
        const uint32_t nreal = (uint32_t)std::min<size_t>(nql, rem);    // ... of which real queries
        INNR_TRY(c->lists.ensure(nslots * nql * cap * sizeof(uint64_t)));
        INNR_TRY(c->counts.ensure(nslots * nql * sizeof(uint32_t)));
        const float* q = dQ + (q0 + done) * ldq;
        const float* qa = aux ? aux + q0 + done : nullptr;
        if (nreal < nql) INNR_TRY(pad_queries(c, ldq, b->D, nql, nreal, &q, &qa));
        INNR_TRY(launch(qb, q, qa, nblocks, nql, KP, cap, cps, groups, nreal));
        INNR_TRY(select_and_emit(b, (uint32_t)nslots, nql, cap, KP, nreal, kout, g.l2, d_out_idx + (q0 + done) * kout,
                                 d_out_score + (q0 + done) * kout));
        done += nreal;
    }
    return INNR_OK;
}

// Exact kNN for queries [q0, q0+nq) (row-major on device, stride ldq): results to d_out_* at row q0.
// limit_n != 0: only the first limit_n vectors of the batch take part (the GEMM engine's threshold seeding).
static innr_status knn_exact_range(innr_batch* b_full, int metric, const float* dQ, size_t ldq, const float* dQn,
                                   size_t q0, size_t nq, size_t kout, uint64_t* d_out_idx, float* d_out_score,
                                   const ScanExt& ext = ScanExt(), size_t limit_n = 0) {
    innr_batch view;  // same device buffers, shorter N (masks) -- never freed, it owns nothing
    innr_batch* b = b_full;
    if (limit_n && limit_n < b_full->N) {
        view.ctx = b_full->ctx;
        view.N = limit_n;
        view.D = b_full->D;
        view.ldN = b_full->ldN;
        view.Dpad = b_full->Dpad;
        view.V = b_full->V;
        view.norms = b_full->norms;
        view.index_base = b_full->index_base;
        b = &view;
    }
    const size_t cols = (b == &view) ? round_up(limit_n, kScanChunk) : b->ldN;
    // waves: fill the chip to the occupancy the register budget allows (HBM latency needs the waves: the single-query kernel holds
    // 72 VGPRs = 7 waves/SIMD)
    const ScanGeom g = {cols, kScanChunk, nq >= 8 ? 16u : 24u, kScanThreads / 64, cols * b->D * sizeof(float), metric == INNR_METRIC_L2SQ};
    return exact_scan_rounds(b, g, dQ, ldq, dQn, q0, nq, kout, d_out_idx, d_out_score,
                             [&](uint32_t qb, const float* q, const float* qn, uint32_t nblocks, uint32_t nql, uint32_t KP, uint32_t cap,
                                 uint32_t cps, uint32_t groups, uint32_t nreal) {
                                 ScanExt ext2 = ext;
                                 if (nreal < nql) ext2.nvalid = nreal;
                                 return launch_scan_filter(b, metric, qb, q, ldq, qn, nblocks, nql, KP, cap, cps, ext2, groups);
                             });
}

// ---- GEMM engine -------------------------------------------------------------------------------------
// The query tile of a GEMM-type engine is padded with zero queries. Left alone they cost MORE than real ones: every score
// is 0, every vector ties, every tile appends and compacts (a 16-query batch on a 256-query tile took 100 ms at C2 where 256
// real queries take 28). Their chip-wide bound starts at the largest key instead: nothing is ever admitted for them.
static innr_status close_padding_queries(innr_ctx* c, uint32_t* gthr, size_t nreal_q, size_t Qpad) {
    if (nreal_q < Qpad) INNR_HIP_CHECK(hipMemsetAsync(gthr + nreal_q, 0xFF, (Qpad - nreal_q) * sizeof(uint32_t), c->stream));
    return INNR_OK;
}

// Chip-wide threshold state of one GEMM-type launch (topk_dev.h): [Qpad][kSlotMul * KP] slots and [Qpad] bounds, zeroed for every
// launch (the bounds then seeded / closed for padding queries), followed by [Qpad] floats: the k rule's margin 2E per query
// (kmargin == null or kk == 0: +inf, the rule is off), and [Qpad] more floats that only the screened split filter reads: its screen
// margin per query (smargin).
static innr_status prep_gthr(innr_ctx* c, size_t Qpad, uint32_t KP, const uint32_t* seed, size_t nreal_q, const float* kmargin,
                             uint32_t** gslots, size_t* nslot_out, const float* smargin = nullptr) {
    const size_t nslot = Qpad * (size_t)kSlotMul * KP;
    INNR_TRY(c->gthr.ensure((nslot + 3 * Qpad) * sizeof(uint32_t)));
    INNR_HIP_CHECK(hipMemsetAsync(c->gthr.p, 0, (nslot + Qpad) * sizeof(uint32_t), c->stream));
    uint32_t* gs = c->gthr.as<uint32_t>();
    if (seed) INNR_HIP_CHECK(hipMemcpyAsync(gs + nslot, seed, Qpad * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    INNR_TRY(close_padding_queries(c, gs + nslot, nreal_q, Qpad));
    if (kmargin) INNR_HIP_CHECK(hipMemcpyAsync(gs + nslot + Qpad, kmargin, Qpad * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    else INNR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(gs + nslot + Qpad), 0x7f800000, Qpad, c->stream));
    if (smargin) INNR_HIP_CHECK(hipMemcpyAsync(gs + nslot + 2 * Qpad, smargin, Qpad * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    *gslots = gs;
    *nslot_out = nslot;
    return INNR_OK;
}
// the final bounds of the last launch's queries (what the re-score proves against)
static const uint32_t* gthr_bounds(const innr_ctx* c, size_t Qpad, uint32_t KP) { return c->gthr.as<uint32_t>() + Qpad * (size_t)kSlotMul * KP; }

// E per query by kind -> the k rule's margin 2E (+ rounding room); +inf where E is not finite and for padding queries.
// kind 0: err_scale * qnorm[j] (dot), 1: err_scale (cosine), 2: err_scale * aux[j] (squared L2 in score space, aux = C_j),
// 3: eq[j] (int8 filter of an f32 corpus), 4: err_scale * qnorm[j] + 4.8e-7 |offset * qsum[j]| + eq[j] (code corpus; eq nullable)
__global__ void kmargin_kernel(int kind, float err_scale, const float* __restrict__ qnorm, const float* __restrict__ aux,
                               const float* __restrict__ eq, float offset, const float* __restrict__ qsum, uint32_t Q, uint32_t Qpad,
                               float* __restrict__ out) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Qpad) return;
    float m = __builtin_inff();
    if (j < Q) {
        float E;
        if (kind == 0) E = err_scale * qnorm[j];
        else if (kind == 1) E = err_scale;
        else if (kind == 2) E = err_scale * aux[j];
        else if (kind == 3) E = eq[j];
        else E = err_scale * qnorm[j] + 4.8e-7f * fabsf(offset * qsum[j]) + (eq ? eq[j] : 0.0f);
        const float x = 2.0f * E * 1.0002f;
        if (x - x == 0.0f && x >= 0.0f) m = x;
    }
    out[j] = m;
}
static innr_status make_kmargin(innr_ctx* c, ScoreSpace kind, float err_scale, const float* qnorm, const float* aux, const float* eq,
                                float offset, const float* qsum, size_t Q, size_t Qpad, const float** out) {
    *out = nullptr;
    if (c->tune.no_k_rule) return INNR_OK;
    INNR_TRY(c->kmargin.ensure(Qpad * sizeof(float)));
    kmargin_kernel<<<(unsigned)((Qpad + 255) / 256), 256, 0, c->stream>>>(kind, err_scale, qnorm, aux, eq, offset, qsum, (uint32_t)Q,
                                                                          (uint32_t)Qpad, c->kmargin.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    *out = c->kmargin.as<float>();
    return INNR_OK;
}

// ---- exact re-score + proof of the selected lists (c->sel [Q][KP], c->sel_cnt [Q]) ----
// f32 corpus (rescore_kernel); qaux: C_j in the squared-L2 space, eq: per-query bounds instead of err_scale (int8 filter)
// tight: the caller's filter is the split filter or the f32 kernel, whose E is a small fraction of the gaps between the best scores
// (split filter at the C2 shape: E ~ 0.09 against a gap of ~1.0 between the 10th and the 17th best of 10M rows). A short answer
// (k <= 12) is then nearly always proven by the best 16 candidates, and every candidate less is D sector reads of the
// dimension-major store less: the progressive rounds begin with 16. The bf16 / int8 filters (E 1.5 .. 2.0 there) would only add
// a serial round and keep 32. flag word kRescoreCountWord counts the candidates re-scored (read by a test hook).
constexpr uint32_t kRescoreCountWord = 40;
static innr_status launch_rescore(innr_batch* b, ScoreSpace space, const float* dQ, size_t Q, const float* qaux, uint32_t KP,
                                  size_t kout, float err_scale, uint64_t* d_out_idx, float* d_out_score, uint32_t* fallback,
                                  const float* eq, bool early, const uint32_t* gthr, bool tight = false) {
    innr_ctx* c = b->ctx;
    const uint32_t r0 = (tight && kout <= 12) ? 16u : 32u;
    const auto launch = [&](auto met) {
        with_rk(KP, [&](auto rk) {
            rescore_kernel<decltype(met)::value, decltype(rk)::value><<<(unsigned)Q, 64, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)b->D, dQ, b->norms, c->q_norm.as<float>(), qaux, c->sel.as<uint64_t>(),
                c->sel_cnt.as<uint32_t>(), KP, (uint32_t)kout, err_scale, b->index_base, d_out_idx, d_out_score, fallback, eq, early,
                gthr, r0, c->flags.as<uint32_t>() + kRescoreCountWord);
        });
    };
    with_space(space, launch);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}
// u8 code corpus (rescore_u8_kernel); i8copy / nk: the int8 filter's copy, eq its per-query quantisation share
static innr_status launch_rescore_u8(innr_batch* b, const float* dQ, size_t Q, const float* qsum, const float* qnorm, uint32_t KP,
                                     size_t kout, float err_scale, uint64_t* d_out_idx, float* d_out_score, uint32_t* fallback,
                                     const float* eq, const uint4* i8copy, uint32_t nk, const uint32_t* gthr) {
    innr_ctx* c = b->ctx;
    with_rk(KP, [&](auto rk) {
        rescore_u8_kernel<decltype(rk)::value><<<(unsigned)Q, 64, 0, c->stream>>>(
            b->C8, b->ldN, (uint32_t)b->D, dQ, qsum, qnorm, b->alpha / 255.0f, b->offset, c->sel.as<uint64_t>(),
            c->sel_cnt.as<uint32_t>(), KP, (uint32_t)kout, err_scale, b->index_base, d_out_idx, d_out_score, fallback, eq,
            !c->tune.rescore_all, i8copy, nk, gthr);
    });
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// The proof's harvest, after the re-score: the fallback flags come back on ONE synchronise (together with whatever else the caller
// copied out before), *gemm_ms = the filter's time (ev[2] .. ev[3]). *redo: the queries whose proof failed or that the caller's
// `unprovable(q)` names, ascending; *nfallback = their count, *kept = KP.
struct NoGate {
    bool operator()(size_t) const { return false; }
};
template <class Gate = NoGate>
static innr_status harvest_proof(innr_ctx* c, const uint32_t* fallback, size_t Q, uint32_t KP, std::vector<uint32_t>* redo,
                                 uint32_t* nfallback, uint32_t* kept, float* gemm_ms, Gate unprovable = Gate()) {
    std::vector<uint32_t> fb(Q);
    INNR_HIP_CHECK(copy_out(c, fb.data(), fallback, Q * sizeof(uint32_t)));
    INNR_HIP_CHECK(ctx_sync(c));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) *gemm_ms = ms;
    redo->clear();
    for (size_t q = 0; q < Q; ++q)
        if (fb[q] || unprovable(q)) redo->push_back((uint32_t)q);
    *nfallback = (uint32_t)redo->size();
    *kept = KP;
    return INNR_OK;
}

// the candidate lists of a GEMM-type launch: [nslices][Qpad][cap] entries, [nslices][Qpad] lengths (GemmPlan or I8Plan)
template <class Plan>
static innr_status ensure_lists(innr_ctx* c, const Plan& p) {
    INNR_TRY(c->lists.ensure((size_t)p.nslices * p.Qpad * p.cap * sizeof(uint64_t)));
    return c->counts.ensure((size_t)p.nslices * p.Qpad * sizeof(uint32_t));
}

struct GemmPlan {
    size_t Qpad;
    uint32_t nqt, qtg, nslices, tps, KP, cap, nblocks, waves;
};

static GemmPlan plan_gemm(const innr_batch* b, size_t Q, size_t kout, uint32_t force_waves = 0, bool dot_kind = false) {
    GemmPlan p;
    // 512-query tiles (8 waves, one block per CU) halve the corpus re-reads (68 vs 123 GB of L2-miss traffic at C2) at
    // the same speed for the dot kind (106.9 vs 106.7 ms). The other kinds keep 4 waves, two blocks per CU: a wave
    // that stalls in its epilogue (norm loads, the append path) then holds up only its own block -- cosine 107.0 vs
    // 107.9 ms, L2 107.7 vs 108.3, u8 at C3 571 vs 582 (its 2 KiB corpus stage is only two DMA pieces, which eight
    // waves issue four times over).
    p.waves = (Q > 256 && dot_kind && !b->C8) ? 8u : 4u;
    // Small query batches: 64- and 128-query tiles (1- and 2-wave blocks, several per CU) instead of padding a 256-query
    // tile -- at 64 queries the f32 MFMA time (6.2 ms at C2) and the corpus stream (5.2 ms) are balanced.
    if (!b->C8 && Q <= 64) p.waves = 1u;
    else if (!b->C8 && Q <= 128) p.waves = 2u;
    if (const long w = b->ctx->tune.gemm_waves; w == 8 || w == 4 || ((w == 2 || w == 1) && !b->C8)) p.waves = (uint32_t)w;
    if (force_waves) p.waves = force_waves;
    const size_t bq = 64 * p.waves;
    p.Qpad = round_up(Q, bq);
    p.nqt = (uint32_t)(p.Qpad / bq);
    p.KP = pick_kp(kout, 16);
    p.cap = (uint32_t)cand_cap((int)p.KP);
    const uint32_t ntiles = (uint32_t)(b->ldN / kBC);
    // resident blocks per CU: 8 waves' worth by registers, but never more blocks than SIMDs
    uint32_t per_cu = std::min(8u / p.waves, 4u);  // 1-wave blocks: one per SIMD (measured 4 / 5 / 6 per CU: 9.96 / 13.6 / 11.8 ms at Q = 64, C2)
    if (const long v = b->ctx->tune.gemm_blocks_per_cu; v > 0) per_cu = (uint32_t)std::min<long>(v, 8);
    uint32_t target = (uint32_t)(per_cu * b->ctx->num_cus) / p.nqt;
    uint32_t ns = std::max(8u, target / 8 * 8);
    ns = std::min(ns, (uint32_t)round_up(ntiles, 8));
    p.nslices = ns;
    p.tps = (ntiles + ns - 1) / ns;
    p.nblocks = p.nqt * ns;
    // query tiles per XCD group (see gemm_filter_kernel): the smallest divisor of nqt that is >= the preferred group
    // size and leaves a group count dividing the 8 XCDs (g = nqt always qualifies)
    // Preferred 1: measured at C2 (rocprofv3 FETCH_SIZE x2): 123 GB of L2-miss reads per launch with 1 tile per XCD
    // group, 130 GB with 2, 191 GB with 4 -- blocks that share a slice drift further apart than a 4 MB L2 can
    // bridge, so co-locating query tiles buys no corpus reuse and only evicts queries. Same speed either way.
    uint32_t want = 1;
    if (const long v = b->ctx->tune.gemm_qt_group; v > 1) want = (uint32_t)v;
    p.qtg = p.nqt;
    for (uint32_t g = std::min(want, p.nqt); g <= p.nqt; ++g)
        if (p.nqt % g == 0 && 8 % (p.nqt / g) == 0) {
            p.qtg = g;
            break;
        }
    return p;
}

template <int KIND, int MODE>
static innr_status launch_gemm(innr_batch* b, const GemmPlan& p, size_t nreal_q, const float* Qt, const float* invn, const float* invq,
                               float* dump, size_t ld_dump, const uint32_t* seed = nullptr, const float* kmargin = nullptr,
                               uint32_t kk = 0) {
    innr_ctx* c = b->ctx;
    uint64_t* lists = c->lists.as<uint64_t>();
    uint32_t* counts = c->counts.as<uint32_t>();
    uint32_t* err = c->flags.as<uint32_t>();
    // chip-wide threshold state; seed: initial bounds (see seed_thresholds_kernel), valid lower bounds, the slots start empty as usual
    uint32_t* gslots = nullptr;
    size_t nslot = 0;
    if (!kmargin) kk = 0;
    INNR_TRY(prep_gthr(c, p.Qpad, MODE == 2 ? 32u : p.KP, seed, nreal_q, kmargin, &gslots, &nslot));  // (MODE 2: only the bounds are used)
    const auto launch = [&](auto rr, auto wv) {
        launch_kernel(c, Inst<kLaunchGemmF32, KIND, rr, MODE, wv>(), {p.nblocks, 64 * wv, 0, p.nqt},
                      KIND == kGemmU8 ? (const void*)b->C8 : (const void*)b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->Dpad, Qt, p.Qpad, p.nqt,
                      p.qtg, p.tps, invn, invq, b->alpha / 255.0f, lists, counts, p.KP, kk, err, gslots, gslots + nslot, dump, ld_dump);
    };
    // The 2- and 1-wave tiles exist for the product path (MODE 0) of the f32 kinds only, the 8-wave tile for the product path and
    // for the dot kind's collect pass (knn_complete); everything else, the layout-dump hook included, stays on 4 waves.
    const auto pick = [&](auto rr, auto wv) {
        constexpr bool exists = wv == 4 || (wv == 8 ? (MODE == 0 || (MODE == 2 && KIND == kGemmDot)) : (MODE == 0 && KIND != kGemmU8));
        if constexpr (exists) launch(rr, wv);
        else launch(rr, IntC<4>());
    };
    // (every instantiation has a row in tests/test_gpu_kernel_variants.py: GEMM_F32)
    if constexpr (MODE == 0) dispatch(pick, rr_gemm(p.cap), one_of<8, 2, 1, 4>(p.waves));
    else dispatch([&](auto wv) { pick(IntC<6>(), wv); }, one_of<8, 4>(p.waves));  // collect, dump: lists of 32 at most (RR 6), no narrow tiles
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

static innr_status ensure_invnorms(innr_batch* b) {
    INNR_TRY(ensure_norms(b));
    if (b->invn) return INNR_OK;
    INNR_HIP_CHECK(alloc_aux(b, &b->invn, b->ldN * sizeof(float)));
    inv_norms_kernel<<<(unsigned)((b->ldN + 255) / 256), 256, 0, b->ctx->stream>>>(b->norms, b->ldN, b->N, b->invn);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// Prepare K-major queries (+ norms, inverse norms). Leaves Qt in c->q_kmajor, norms in c->q_norm, inverses in c->misc.
static innr_status prep_queries(innr_batch* b, const GemmPlan& p, const float* dQ, size_t Q, bool cos) {
    innr_ctx* c = b->ctx;
    INNR_TRY(c->q_kmajor.ensure(b->Dpad * p.Qpad * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(p.Qpad * sizeof(float)));
    INNR_TRY(c->misc.ensure(p.Qpad * sizeof(float) + Q * sizeof(uint32_t) + 64));
    dim3 grid((unsigned)(p.Qpad / 32), (unsigned)(b->Dpad / 32));
    transpose_queries_kernel<<<grid, 256, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, c->q_kmajor.as<float>(),
                                                          p.Qpad, (uint32_t)b->Dpad);
    INNR_HIP_CHECK(hipGetLastError());
    query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, b->D,
                                                                       c->q_norm.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    if (cos) {
        inv_qnorms_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(c->q_norm.as<float>(), p.Qpad, Q,
                                                                                  c->misc.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
    }
    return INNR_OK;
}

static innr_status ensure_sqnorms(innr_batch* b) {
    INNR_TRY(ensure_norms(b));
    if (b->sqn) return INNR_OK;
    INNR_HIP_CHECK(alloc_aux(b, &b->sqn, b->ldN * sizeof(float)));
    sq_norms_kernel<<<(unsigned)((b->ldN + 255) / 256), 256, 0, b->ctx->stream>>>(b->norms, b->ldN, b->N, b->sqn);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ---- bf16 filter engine (kernels_gemm_bf16.h) ------------------------------------------------------------------
__global__ void gather_rows_kernel(const float* __restrict__ src, const uint32_t* __restrict__ map, uint32_t n, uint32_t D,
                                   float* __restrict__ dst) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (size_t)n * D) dst[t] = src[(size_t)map[t / D] * D + t % D];
}
__global__ void scatter_results_kernel(const uint64_t* __restrict__ idx, const float* __restrict__ sc, const uint32_t* __restrict__ map,
                                       uint32_t n, uint32_t k, uint64_t* __restrict__ out_idx, float* __restrict__ out_sc) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const size_t o = (size_t)map[t / k] * k + t % k;
    out_idx[o] = idx[t];
    out_sc[o] = sc[t];
}

__global__ void gather_f32_kernel(const float* __restrict__ src, const uint32_t* __restrict__ map, uint32_t n, float* __restrict__ dst) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dst[t] = src[map[t]];
}

static innr_status knn_mfma(innr_batch* b, int metric, const float* dQ, size_t Q, size_t kout, const float* dQn,
                            uint64_t* d_out_idx, float* d_out_score, uint32_t* nfallback, uint32_t* kept,
                            float* gemm_ms, bool bf16 = false, uint32_t kp_force = 0, int level = 0);
static innr_status knn_f32_i8(innr_batch* b, int metric, const float* dQ, size_t Q, size_t kout, uint64_t* d_out_idx,
                              float* d_out_score, uint32_t* nfallback, uint32_t* kept, float* gemm_ms, bool* served,
                              const float* collect_kth = nullptr, uint32_t* d_unresolved = nullptr);

// A redo set's workspace, sized for its queries' rows, norms and results; the query map `redo` uploaded (a pageable host vector)
static innr_status upload_redo(innr_ctx* c, innr_ctx::RedoBufs& rb, const std::vector<uint32_t>& redo, size_t D, size_t kout) {
    const size_t nr = redo.size();
    INNR_TRY(rb.map.ensure(nr * sizeof(uint32_t)));
    INNR_TRY(rb.q.ensure(std::max<size_t>(nr * D, 1) * sizeof(float)));
    INNR_TRY(rb.qn.ensure(nr * sizeof(float)));
    INNR_TRY(rb.idx.ensure(nr * kout * sizeof(uint64_t)));
    INNR_TRY(rb.sc.ensure(nr * kout * sizeof(float)));
    INNR_HIP_CHECK(hipMemcpyAsync(rb.map.p, redo.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    INNR_HIP_CHECK(hipStreamSynchronize(c->stream));  // redo is a pageable host vector
    return INNR_OK;
}
// ... and the way back: the set's results [nr][kout] scattered to the rows of the queries they belong to
static innr_status scatter_redo(innr_ctx* c, innr_ctx::RedoBufs& rb, size_t nr, size_t kout, uint64_t* d_out_idx, float* d_out_score) {
    scatter_results_kernel<<<(unsigned)((nr * kout + 255) / 256), 256, 0, c->stream>>>(
        rb.idx.as<uint64_t>(), rb.sc.as<float>(), rb.map.as<uint32_t>(), (uint32_t)nr, (uint32_t)kout, d_out_idx, d_out_score);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// Queries whose margin proof failed (`redo`: their indices, ascending): gathered into ONE contiguous block and redone
// together -- on the exact engine, 8 queries per corpus pass (via_gemm_kp == 0), or once more on the f32 GEMM engine
// with lists of via_gemm_kp candidates (whose own unproven queries then take the exact engine) -- and scattered back.
// One exact corpus scan PER QUERY made near-tie data cost ~5 ms per query at 10M x 768; a pass of 8 costs 6.6 ms.
// qn_all: per-query norms of the whole batch (cosine; may be null otherwise).
static innr_status redo_batch(innr_batch* b, int metric, const float* dQ, const float* qn_all,
                              const std::vector<uint32_t>& redo, size_t kout, uint64_t* d_out_idx, float* d_out_score,
                              uint32_t via_gemm_kp, int level) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size(), D = b->D;
    if (nr == 0) return INNR_OK;
    if (level < 0 || level > 1) {
        set_error("internal: redo_batch nesting %d", level);
        return INNR_E_HIP;
    }
    innr_ctx::RedoBufs& rb = c->redo[level];  // the nested GEMM pass (level + 1) reads these while filling its own set
    INNR_TRY(upload_redo(c, rb, redo, D, kout));
    const uint32_t* map = rb.map.as<uint32_t>();
    if (D) {
        gather_rows_kernel<<<(unsigned)((nr * D + 255) / 256), 256, 0, c->stream>>>(dQ, map, (uint32_t)nr, (uint32_t)D,
                                                                                rb.q.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
    }
    const float* qn = nullptr;
    if (qn_all) {
        gather_f32_kernel<<<(unsigned)((nr + 255) / 256), 256, 0, c->stream>>>(qn_all, map, (uint32_t)nr, rb.qn.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        qn = rb.qn.as<float>();
    }
    if (via_gemm_kp) {
        uint32_t nf2 = 0, kept2 = 0;
        float ms2 = 0.0f;
        INNR_TRY(knn_mfma(b, metric, rb.q.as<float>(), nr, kout, qn, rb.idx.as<uint64_t>(), rb.sc.as<float>(), &nf2, &kept2,
                          &ms2, false, via_gemm_kp, level + 1));
    } else {
        INNR_TRY(knn_exact_range(b, metric, rb.q.as<float>(), D, qn, 0, nr, kout, rb.idx.as<uint64_t>(), rb.sc.as<float>()));
    }
    return scatter_redo(c, rb, nr, kout, d_out_idx, d_out_score);
}

// ---- completion pass for queries whose margin proof failed (f32 GEMM engine) ------------------------------------------------
// After the first pass an unproven query has k candidates with EXACT scores; the k-th of them, x_k, is a lower bound of the
// corpus' true k-th best score, and every member v of the true top k has exact(v) >= x_k, hence approx(v) >= x_k - E. ONE more
// GEMM pass over the unproven queries with that FIXED threshold collects every such site into a global list per query (MODE 2 of
// gemm_filter_kernel: no list capacity to run against, no bound that moves); all collected candidates are re-scored in the
// reference's order and the best k of them ARE the answer -- proven, whatever the gaps between neighbouring scores. Near-tie
// data (the reference example's LCG rows: hundreds of vectors within 2E of every k-th score) used to send every query through
// the exact engine, 8 per corpus pass: 1024 queries = 128 passes = 0.84 s at C2; the completion pass is one GEMM pass (~0.11 s)
// plus a few hundred exact dots per query. Queries whose list overflows kCollectCap (or whose x_k / E is not finite) stay
// unresolved and take the exact engine as before.
constexpr uint32_t kCollectCap = 65536;  // candidates per query the completion pass can hold (256 KiB of indices per query)

// PDX -> row-major: Vr[i*Dr + d] = V[d*ldN + i], 32 x 32 tiles through LDS (both sides coalesced)
__global__ __launch_bounds__(256) void pdx_to_rows_kernel(const float* __restrict__ V, size_t ldN, uint32_t N, uint32_t D, float* __restrict__ Vr,
                                                           uint32_t Dr) {
    __shared__ float t[32][33];
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t i0 = (size_t)blockIdx.x * 32;
    const uint32_t d0 = blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t d = d0 + ty + 8 * r;
        t[ty + 8 * r][tx] = (d < D && i0 + tx < N) ? V[(size_t)d * ldN + i0 + tx] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t i = i0 + ty + 8 * r;
        const uint32_t d = d0 + tx;
        if (i < N && d < Dr) Vr[i * Dr + d] = t[tx][ty + 8 * r];
    }
}

// exact scores of collected candidates from the ROW-MAJOR copy. One lane per candidate (the reference's sum is a chain: d
// ascending, fl(acc + fl(q_d * v_d))), but the rows are FETCHED by the whole wave: 64 dimensions of 64 candidate rows per step
// as sixteen 16-byte loads per lane -- a quarter-wave covers one row's 256 contiguous bytes -- staged through LDS (row stride 65
// words: the per-lane walk along a row is conflict-free), the query through wave-uniform (scalar) loads. A lane reading its own
// row 16 bytes at a time touched 64 cache lines per load instruction: 65 ms for the 33 M candidates of the LCG bench row
// (1.6 TB/s); staged: see DESIGN.md.
template <int MET>
__global__ __launch_bounds__(256) void collect_scores_rows_kernel(const float* __restrict__ Vr, uint32_t Dr, uint32_t D,
                                                                   const float* __restrict__ Qm, const float* __restrict__ norms,
                                                                   const float* __restrict__ qnorm, const uint32_t* __restrict__ clist,
                                                                   const uint32_t* __restrict__ ccnt, uint32_t cap,
                                                                   uint64_t* __restrict__ keys) {
    constexpr bool COS = MET == 1, L2 = MET == 2;
    __shared__ float stage[4][64][65];
    const uint32_t q = blockIdx.y;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n = ccnt[q] < cap ? ccnt[q] : cap;
    const uint32_t base = blockIdx.x * 256 + 64 * (uint32_t)w;
    if (base >= n) return;  // (wave-uniform; no block-level synchronisation below)
    const uint32_t slot = base + (uint32_t)lane;
    const bool on = slot < n;
    const uint32_t i = clist[(size_t)q * cap + (on ? slot : base)];  // idle lanes re-read the wave's first row
    const float* qv = Qm + (size_t)q * D;
    float (*st)[65] = stage[w];
    const int sub = lane >> 4, l16 = lane & 15;
    float acc = 0.0f;
    for (uint32_t d0 = 0; d0 < D; d0 += 64) {
        float4 v[16];
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const uint32_t ir = (uint32_t)__shfl((int)i, 4 * rr + sub, 64);
            const uint32_t d = d0 + 4 * (uint32_t)l16;
            v[rr] = d < Dr ? *reinterpret_cast<const float4*>(Vr + (size_t)ir * Dr + d) : float4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            float* p = &st[4 * rr + sub][4 * l16];
            p[0] = v[rr].x; p[1] = v[rr].y; p[2] = v[rr].z; p[3] = v[rr].w;
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lim = D - d0 < 64u ? D - d0 : 64u;
        if (lim == 64u) {
#pragma unroll 16
            for (uint32_t j = 0; j < 64; ++j) {
                const float x = st[lane][j], qd = qv[d0 + j];
                if (L2) {
                    const float df = ex::sub_keepnan(qd, x);
                    acc = ex::mad2(acc, df, df);
                } else {
                    acc = ex::mad2(acc, qd, x);
                }
            }
        } else {
            for (uint32_t j = 0; j < lim; ++j) {
                const float x = st[lane][j], qd = qv[d0 + j];
                if (L2) {
                    const float df = ex::sub_keepnan(qd, x);
                    acc = ex::mad2(acc, df, df);
                } else {
                    acc = ex::mad2(acc, qd, x);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (COS) {
        const float qn = qnorm[q], vn = norms[i];
        acc = (qn < INNR_NORM_EPSILON) ? 0.0f : ((vn > INNR_NORM_EPSILON) ? ex::div(acc, ex::mul(qn, vn)) : 0.0f);
    }
    if (on) keys[(size_t)q * cap + slot] = cand_make(score_pref<L2>(acc), i);
}

__global__ void gather_kth_kernel(const float* __restrict__ scores, const uint32_t* __restrict__ map, uint32_t n, uint32_t k,
                                  float* __restrict__ out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = scores[(size_t)map[t] * k + (k - 1)];
}

// exact score of every collected candidate, in the reference's order (cf. rerank_scores_kernel): one thread per (query, slot)
template <int MET>
__global__ __launch_bounds__(256) void collect_scores_kernel(const float* __restrict__ V, size_t ldN, uint32_t D, const float* __restrict__ Qm,
                                                              const float* __restrict__ norms, const float* __restrict__ qnorm,
                                                              const uint32_t* __restrict__ clist, const uint32_t* __restrict__ ccnt,
                                                              uint32_t cap, uint64_t* __restrict__ keys) {
    constexpr bool COS = MET == 1, L2 = MET == 2;
    const uint32_t q = blockIdx.y;
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = ccnt[q] < cap ? ccnt[q] : cap;
    if (slot >= n) return;  // (the selection reads only the first n keys)
    const uint32_t i = clist[(size_t)q * cap + slot];
    const float* qv = Qm + (size_t)q * D;
    const float* col = V + i;
    float acc = 0.0f;
    if (L2) {
#pragma unroll 8
        for (uint32_t d = 0; d < D; ++d) {
            const float diff = ex::sub_keepnan(qv[d], col[(size_t)d * ldN]);
            acc = ex::mad2(acc, diff, diff);
        }
    } else {
#pragma unroll 8
        for (uint32_t d = 0; d < D; ++d) acc = ex::mad2(acc, qv[d], col[(size_t)d * ldN]);
    }
    if (COS) {
        const float qn = qnorm[q], vn = norms[i];
        acc = (qn < INNR_NORM_EPSILON) ? 0.0f : ((vn > INNR_NORM_EPSILON) ? ex::div(acc, ex::mul(qn, vn)) : 0.0f);
    }
    keys[(size_t)q * cap + slot] = cand_make(score_pref<L2>(acc), i);
}

// best kout (<= kSelSlots) of a query's n exact composites: one workgroup per query (wg_segment_topk: LDS sort, or radix select + sort)
__global__ __launch_bounds__(kSelThreads) void segment_topk_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ccnt,
                                                                    uint32_t cap, uint32_t kout, bool smaller_is_better,
                                                                    uint64_t index_base, uint64_t* __restrict__ out_idx,
                                                                    float* __restrict__ out_score, uint32_t* __restrict__ unresolved) {
    __shared__ uint64_t s[kSelSlots];
    __shared__ uint32_t hist[258];
    const uint32_t q = blockIdx.x;
    const uint32_t n = ccnt[q];
    if (n > cap || n < kout) {  // overflow (or a threshold that was not a bound: non-finite scores): the exact engine decides
        if (threadIdx.x == 0) unresolved[q] = 1u;
        return;
    }
    wg_segment_topk(keys + (size_t)q * cap, n, kout, s, hist);
    for (uint32_t r = threadIdx.x; r < kout; r += kSelThreads) {
        out_idx[(size_t)q * kout + r] = index_base + cand_idx(s[r]);
        out_score[(size_t)q * kout + r] = pref_score(cand_pref(s[r]), smaller_is_better);
    }
}

static size_t rows_copy_bytes(const innr_batch* b) { return b->N * round_up(b->D, 4) * sizeof(float); }

// the row-major copy of an f32 batch (kCopyRows), if it exists or fits with room to spare (copy_fits); soft == false
// (innr_batch_build_copies): the caller asked for it -- no memory rule, no remembered refusal, no no_rows_copy
static innr_status ensure_rowmajor(innr_batch* b, bool* have, bool soft = true) {
    CorpusCopy& rows = b->copy[kCopyRows];
    *have = rows.p != nullptr && !b->ctx->tune.no_rows_copy;
    if (rows.p || (soft && (rows.refused || b->ctx->tune.no_rows_copy)) || !b->V || b->N == 0 || b->D == 0) return INNR_OK;
    const size_t Dr = round_up(b->D, 4);
    INNR_TRY(alloc_copy(b, kCopyRows, rows_copy_bytes(b), (uint32_t)Dr, soft, "row-major copy"));
    if (!rows.p) return INNR_OK;
    dim3 grid((unsigned)((b->N + 31) / 32), (unsigned)((Dr + 31) / 32));
    pdx_to_rows_kernel<<<grid, 256, 0, b->ctx->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, reinterpret_cast<float*>(rows.p), (uint32_t)Dr);
    INNR_HIP_CHECK(hipGetLastError());
    *have = true;
    return INNR_OK;
}

// Exact composites of every collected candidate at c->sort_keys [nq][kCollectCap] (the first min(count, kCollectCap) of a query are
// written), from the row-major copy when it exists or fits (*used_rows), else by column gathers. clist / ccnt: c->lists / c->counts
// as the collect-mode kernels left them; Qm: the queries the exact scores are taken with. The range search shares this step.
static innr_status collect_rescore(innr_batch* b, int metric, const float* Qm, const float* qnorm, size_t nq, bool* used_rows) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    const size_t D = b->D;
    INNR_TRY(c->sort_keys.ensure(nq * (size_t)kCollectCap * sizeof(uint64_t)));
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    const uint32_t* clist = c->lists.as<uint32_t>();
    const uint32_t* ccnt = c->counts.as<uint32_t>();
    const dim3 sg(kCollectCap / 256, (unsigned)nq);  // (blocks beyond a query's list length return at once)
    bool rows = false;
    INNR_TRY(ensure_rowmajor(b, &rows));  // contiguous candidate rows instead of D cache lines each, when the copy exists or fits
    if (rows) {
        const CorpusCopy& rowc = b->copy[kCopyRows];
        const float* rowp = reinterpret_cast<const float*>(rowc.p);
        if (cos) collect_scores_rows_kernel<1><<<sg, 256, 0, c->stream>>>(rowp, rowc.nk, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
        else if (l2) collect_scores_rows_kernel<2><<<sg, 256, 0, c->stream>>>(rowp, rowc.nk, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
        else collect_scores_rows_kernel<0><<<sg, 256, 0, c->stream>>>(rowp, rowc.nk, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
    } else {
        if (cos) collect_scores_kernel<1><<<sg, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
        else if (l2) collect_scores_kernel<2><<<sg, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
        else collect_scores_kernel<0><<<sg, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, Qm, b->norms, qnorm, clist, ccnt, kCollectCap, keys);
    }
    INNR_HIP_CHECK(hipGetLastError());
    *used_rows = rows;
    return INNR_OK;
}
// The second half of a completion pass, whatever filter collected: those exact scores, then the best kout per query -> d_out_*
// [Q][kout]; d_unresolved[q] = 1 for overflowed lists.
static innr_status collect_finish(innr_batch* b, int metric, const float* Qm, const float* qnorm, size_t nq, size_t kout,
                                  uint64_t* d_out_idx, float* d_out_score, uint32_t* d_unresolved) {
    innr_ctx* c = b->ctx;
    const bool l2 = metric == INNR_METRIC_L2SQ;
    bool rows = false;
    INNR_TRY(collect_rescore(b, metric, Qm, qnorm, nq, &rows));
    const uint64_t* keys = c->sort_keys.as<uint64_t>();
    const uint32_t* ccnt = c->counts.as<uint32_t>();
    INNR_HIP_CHECK(hipMemsetAsync(d_unresolved, 0, nq * sizeof(uint32_t), c->stream));
    segment_topk_kernel<<<(unsigned)nq, kSelThreads, 0, c->stream>>>(keys, ccnt, kCollectCap, (uint32_t)kout, l2, b->index_base, d_out_idx,
                                                                    d_out_score, d_unresolved);
    INNR_HIP_CHECK(hipGetLastError());
    if (c->tune.trace) {
        std::vector<uint32_t> cnt(nq);
        INNR_HIP_CHECK(hipMemcpyAsync(cnt.data(), ccnt, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        INNR_HIP_CHECK(hipStreamSynchronize(c->stream));
        std::sort(cnt.begin(), cnt.end());
        fprintf(stderr, "completion pass: %zu queries, collected per query min %u / median %u / max %u (capacity %u), rows copy %d\n", nq,
                cnt.front(), cnt[nq / 2], cnt.back(), kCollectCap, (int)rows);
    }
    return INNR_OK;
}

// gather the unproven queries and their k-th exact scores into c->cmpl (map, q, qn = x_k)
static innr_status collect_gather(innr_batch* b, const float* dQ, const std::vector<uint32_t>& redo, size_t kout, const float* d_out_score) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size(), D = b->D;
    innr_ctx::RedoBufs& rb = c->cmpl;  // its own set: a nested pass (redo_batch -> knn_mfma) runs while redo[level] is live
    INNR_TRY(upload_redo(c, rb, redo, D, kout));
    const uint32_t* map = rb.map.as<uint32_t>();
    gather_rows_kernel<<<(unsigned)((nr * D + 255) / 256), 256, 0, c->stream>>>(dQ, map, (uint32_t)nr, (uint32_t)D, rb.q.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    gather_kth_kernel<<<(unsigned)((nr + 255) / 256), 256, 0, c->stream>>>(d_out_score, map, (uint32_t)nr, (uint32_t)kout, rb.qn.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}
// resolved rows back to their places; the unresolved ones (rewritten by the next engine afterwards) are listed
static innr_status collect_scatter(innr_batch* b, const std::vector<uint32_t>& redo, size_t kout, uint64_t* d_out_idx, float* d_out_score,
                                   const uint32_t* d_unres, std::vector<uint32_t>* unresolved, float* gemm_ms) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size();
    innr_ctx::RedoBufs& rb = c->cmpl;
    std::vector<uint32_t> un(nr);
    INNR_HIP_CHECK(copy_out(c, un.data(), d_unres, nr * sizeof(uint32_t)));
    INNR_HIP_CHECK(ctx_sync(c));
    float ms = 0.0f;  // the collect pass' filter time (ev[2] .. ev[3])
    if (gemm_ms && hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) *gemm_ms += ms;
    INNR_TRY(scatter_redo(c, rb, nr, kout, d_out_idx, d_out_score));
    unresolved->clear();
    for (size_t r = 0; r < nr; ++r)
        if (un[r]) unresolved->push_back(redo[r]);
    return INNR_OK;
}

// the int8 filter's completion pass (f32 corpus, dot / cosine)
static innr_status knn_complete_i8(innr_batch* b, int metric, const float* dQ, const std::vector<uint32_t>& redo, size_t kout,
                                   uint64_t* d_out_idx, float* d_out_score, std::vector<uint32_t>* unresolved, float* gemm_ms) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size();
    unresolved->clear();
    if (nr == 0) return INNR_OK;
    INNR_TRY(collect_gather(b, dQ, redo, kout, d_out_score));
    innr_ctx::RedoBufs& rb = c->cmpl;
    INNR_TRY(c->sel_cnt.ensure(nr * sizeof(uint32_t)));
    uint32_t nf = 0, kept = 0;
    bool served = false;
    INNR_TRY(knn_f32_i8(b, metric, rb.q.as<float>(), nr, kout, rb.idx.as<uint64_t>(), rb.sc.as<float>(), &nf, &kept, gemm_ms, &served,
                        rb.qn.as<float>(), c->sel_cnt.as<uint32_t>()));
    if (!served) {  // (cannot happen after a first pass of the same filter) nothing was resolved
        *unresolved = redo;
        return INNR_OK;
    }
    return collect_scatter(b, redo, kout, d_out_idx, d_out_score, c->sel_cnt.as<uint32_t>(), unresolved, gemm_ms);  // (synchronises)
}

// Squared L2 on the f32 engine, from the exact query norms (c->q_norm): the epilogue constants C_j - |q_j|^2 (in invq's place) and
// *Cj = C_j (for the proof), at c->tmp_norms
static innr_status l2_query_consts(innr_batch* b, size_t Qpad, size_t Q, float* invq, float** Cj) {
    innr_ctx* c = b->ctx;
    INNR_TRY(c->tmp_norms.ensure(Qpad * sizeof(float)));
    *Cj = c->tmp_norms.as<float>();
    l2_query_consts_kernel<<<(unsigned)((Qpad + 255) / 256), 256, 0, c->stream>>>(c->q_norm.as<float>(), Qpad, Q, b->max_norm, invq, *Cj);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ---- error bounds of the filters of an f32 corpus: err_scale, E = err_scale * |q| (dot), err_scale (cosine), err_scale * C_j (squared L2)
// dot / cosine: |approx - exact| <= (2D+8) u (1+eps) * sum|q_d v_d|: u = 2^-24, Cauchy-Schwarz for the sum.
// L2: approx = C - (|v|^2 - 2 q.v + |q|^2) assembled from the MFMA dot (<= (2D+8) u |q||v|, doubled), the squared
// cached norms and the query norm (<= (D+4) u each, relative to their own size), three epilogue roundings, and the
// reference's own direct-difference sum is within (D+2) u of the true distance: every term is <= C = (|q|+max|v|)^2,
// so |(C - approx) - exact| <= (6D+40) u C with room to spare.
static float f32_cdu(const innr_batch* b) { return 1.05f * (2.0f * (float)b->D + 8.0f) * 5.9604645e-08f; }
static float f32_filter_scale(const innr_batch* b, int metric) {
    const float cdu = f32_cdu(b);
    return metric == INNR_METRIC_L2SQ ? 1.05f * (6.0f * (float)b->D + 40.0f) * 5.9604645e-08f
                                      : (metric == INNR_METRIC_COSINE ? cdu : cdu * b->max_norm);
}
// bf16 filter: both operands rounded to 8 significant bits (|delta| <= 2^-8 each): |q'v' - qv| <= (2^-7 + 2^-16) |qv|,
// plus the f32 accumulation of the rounded products
// (cosine: both sides normalised before the rounding, |q^||v^| <= (1 + D u)^2 -- inside the 1.05)
// squared L2 on the bf16 filter, as a multiple of C = (|q| + max|v|)^2: the doubled bf16 dot is off by <= 2 (2^-7 + 2^-16) |q||v|
// <= (2^-7 + 2^-16) C / 2; the f32 accumulation of D + 6 products whose absolute values sum to <= 2 C, the limbs' residuals,
// the cached norms and c_j, and the reference's own direct-difference sum (within (D+2) u of the true distance) stay
// inside (8D + 96) u C
static float bf16_filter_scale(const innr_batch* b, int metric) {
    return metric == INNR_METRIC_L2SQ
               ? 1.05f * (0.00390625f * 1.004f + (8.0f * (float)b->D + 96.0f) * 5.9604645e-08f)
               : 1.05f * (0.0078125f * 1.004f + (2.0f * (float)b->D + 8.0f) * 5.9604645e-08f * 1.02f) *
                     (metric == INNR_METRIC_COSINE ? 1.0f : b->max_norm);
}
// split-bf16 filter, per dimension x = qh + ql + rq, y = vh + vl + rv (h = rne_bf16, l = rne_bf16 of the exact
// f32 difference; |h| <= (1 + 2^-8)|x|, |l| <= (1 + 2^-8) 2^-8 |x|, |r| <= 2^-16 |x|). The kernel sums qh vh + qh vl + ql vh; the
// dropped part xy - that = ql vl + qh rv + rq vh + ql rv + rq vl + rq rv is <= (3 (1 + 2^-7) 2^-16 + 2^-23 + 2^-32) |xy| <= 3.1 2^-16 |xy|.
// Every bf16 x bf16 product is exact in f32; their f32 accumulation on the matrix pipe -- the assumption the bf16 bound makes:
// n products accumulate within (2n + 8) u of the sum of their magnitudes -- with n = 3D products whose magnitudes sum to
// <= (1 + 2^-8)^2 (1 + 2^-7) sum|xy| <= 1.016 sum|xy|: (6D + 8) u 1.04 sum|xy|. Cauchy-Schwarz: sum|xy| <= |q| max|v|.
// Values at the bottom of the range: a limb or product below 2^-126 may be flushed to zero, at most 2^-126 per flushed
// operand times the other side (<= 2^-126 sqrt(D) (|q| + max|v|) over a row) plus 2^-126 per product or partial sum (6D of
// them). With max|v| and |q| both in [1e-12, 1e18] (the gates of choose_f32_filter and of knn_mfma's proof; cosine: both
// normalised, <= 1.0), and E >= 3 2^-16 |q| max|v|, that is below 1e-6 E -- inside the 1.05. A zero query is exact (every limb 0).
// Cosine: |q^||v^| <= (1 + D u)^2.
static float split_filter_scale(const innr_batch* b, int metric) {
    return 1.05f * (3.1f * 1.52587890625e-05f + (6.0f * (float)b->D + 8.0f) * 5.9604645e-08f * 1.04f) *
           (metric == INNR_METRIC_COSINE ? 1.0f : b->max_norm);
}

// The screened split filter's margin: its K-loop accumulates s_hh = qh.vh alone and rejects a 32 x 32 sub-tile
// without the two small products when max s_hh < thr - m. What the reject has to cover is the score the correction would have
// produced from the same accumulator, s = fl(s_hh + qh.vl + ql.vh), the small products added behind all of hi.hi:
//   * bf16 keeps 8 significant bits: |x - h| <= 2^-8 |x| for h = rne_bf16(x) (half a last place; reached just above a power of
//     two), so |l| <= (1 + 2^-8) 2^-8 |x| for l = rne_bf16(x - h) and |h| <= (1 + 2^-8) |x|. Per dimension
//     |qh vl + ql vh| <= 2 (1 + 2^-8)^2 2^-8 |q_d v_d| <= 2^-7 1.004 |q_d v_d|, and Cauchy-Schwarz over the row:
//     |qh.vl + ql.vh| <= 2^-7 1.004 |q| max|v|. (Half of that, 2^-8 1.004, holds for most data but not for all: values whose lo
//     limbs sit at half a last place with aligned signs exceed it -- tests/test_gpu_split_screen.py measures 1.07 x 2^-8.)
//   * the f32 accumulation of the 2D small products on top of s_hh: within the (6D + 8) u 1.04 |q| max|v| that split_filter_scale
//     allows for all 3D products in any order (the same assumption, the same magnitudes).
//   * flushed limbs or products at the bottom of the range: the allowance of split_filter_scale, at most
//     2^-126 (sqrt(D) (|q| + max|v|) + 6D), added per query by screen_margin_kernel.
// So s <= s_hh + m with m = 1.05 (2^-7 1.004 + (6D + 8) u 1.04) |q| max|v| (cosine: 1 for |q^||v^|, the (1 + D u)^2 inside the 1.05):
// a sub-tile below thr - m holds nothing that the full loop would have kept, and is rejected exactly as its full scores would be.
// The scores of corrected sub-tiles accumulate in another order than the full loop's; E covers any order.
//
// The first term above is the WORST CASE over all data: every lo limb at half a last place of its hi limb, signs aligned. The
// limbs the copies really hold give a bound of the same kind that is never larger: Cauchy-Schwarz on the limb vectors themselves,
//     |qh.vl_i + ql.vh_i| <= |qh| |vl_i| + |ql| |vh_i| <= |qh| Lmax + |ql| Hmax,   Hmax = max_i |vh_i|, Lmax = max_i |vl_i|
// over the rows the copies hold (limb_maxima_kernel, kept in CorpusCopy::limb_max of the hi / the lo copy) and |qh_j|, |ql_j| of the
// limbs pack_queries_bf16_kernel writes (cosine: of the normalised values on both sides) -- every norm summed in double and
// rounded up. It is as rigorous as the worst case and at most (1 + 2^-8)^2 2^-7 |q| max|v| <= the worst case's term, since
// |qh| <= (1 + 2^-8) |q|, |vl| <= (1 + 2^-8) 2^-8 |v| and the same with the roles exchanged. Lo limbs of real data are spread over
// (-1/2, 1/2) last places: root-mean-square 1 / sqrt(12) of the worst case's 1/2 each, so the sum of the two products is about
// 0.38 of the worst case on uniform data, 0.43 on normal data, and close to 1 only on data built to sit at half a last place.
// The screen's margin of a query (screen_margin_kernel) is
//     m_j = 1.0002 [ 1.05 ( |qh_j| Lmax + |ql_j| Hmax + (6D + 8) u 1.04 |q_j| max|v| ) + the flush allowance ]
// (cosine: 1 for |q_j| max|v|), or the worst-case m_j where that is smaller, the maxima are missing or not finite, or the
// tuning word split_screen_worst_case asks for it. The accumulation term and the flush allowance are the worst case's.
static float split_screen_scale(const innr_batch* b, int metric) {
    return 1.05f * (0.0078125f * 1.004f + (6.0f * (float)b->D + 8.0f) * 5.9604645e-08f * 1.04f) *
           (metric == INNR_METRIC_COSINE ? 1.0f : b->max_norm);
}
// m per query, one wave each. Worst case: scale * |q_j| (dot) or scale (cosine: |q^| = 1) + the flush allowance
// 2^-126 (flush_c + flush_v |q_j|), rounded up. From the limb norms (hmax, lmax >= 0; the host passes -1 for "worst case only"):
// the formula above in double, with |qh_j|, |ql_j| of row j of Qm ([Q][D]; qscale as pack_queries_bf16_kernel takes it) and
// accv = (6D + 8) u 1.04 max|v|, rounded up to float and one more float up; the smaller of the two counts.
// +inf (no screening: every sub-tile is corrected) where that is not a finite non-negative number. Padding queries are closed
// (close_padding_queries): their margin plays no part.
__global__ __launch_bounds__(256) void screen_margin_kernel(int cosine, float scale, float flush_v, float flush_c, float hmax, float lmax,
                                                             double accv, const float* __restrict__ qnorm, const float* __restrict__ Qm,
                                                             const float* __restrict__ qscale, uint32_t D, uint32_t Q, uint32_t Qpad,
                                                             float* __restrict__ out) {
    const uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    const uint32_t lane = threadIdx.x & 63;
    if (j >= Qpad) return;
    float m = 0.0f;
    if (j < Q) {
        const float qn = cosine ? 1.0f : qnorm[j];
        float x = (scale * (cosine ? 1.0f : qn) + 1.17549435e-38f * (flush_c + flush_v * qn)) * 1.0002f;
        if (hmax >= 0.0f && lmax >= 0.0f) {
            const float qs = qscale ? qscale[j] : 1.0f;
            double sh = 0.0, sl = 0.0;
            for (uint32_t d = lane; d < D; d += 64) {
                const float xs = Qm[(size_t)j * D + d] * qs;
                const double h = (double)__uint_as_float((uint32_t)bf16_limb(xs, 0) << 16);
                const double l = (double)__uint_as_float((uint32_t)bf16_limb(xs, 1) << 16);
                sh += h * h;
                sl += l * l;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                sh += __shfl_xor(sh, off, 64);
                sl += __shfl_xor(sl, off, 64);
            }
            const double qh = (double)f32_round_up(sqrt(sh)), ql = (double)f32_round_up(sqrt(sl));
            const double y = 1.0002 * (1.05 * (qh * (double)lmax + ql * (double)hmax + accv * (double)qn) +
                                       1.1754943508222875e-38 * ((double)flush_c + (double)flush_v * (double)qn));
            float yf = f32_round_up(y);
            if (yf - yf == 0.0f) yf = __uint_as_float(__float_as_uint(yf) + 1u);
            if (yf < x) x = yf;  // (a NaN compares false: the worst case stays)
        }
        m = (x - x == 0.0f && x >= 0.0f) ? x : __builtin_inff();
    }
    if (lane == 0) out[j] = m;
}
// c->kmargin [Qpad .. 2 Qpad): behind the k rule's margins (make_kmargin sizes the buffer for both when asked first)
// dQ: the call's queries, row-major [Q][D]; qscale: what pack_queries_split was given (cosine: 1/||q||, else null)
static innr_status make_screen_margin(innr_batch* b, int metric, const float* dQ, const float* qscale, size_t Q, size_t Qpad,
                                      const float** out) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE;
    const float sd = sqrtf((float)b->D), vmax = cos ? 1.0f : b->max_norm;
    float* m = c->kmargin.as<float>() + Qpad;
    // the limb maxima of the pair (ensure_limb_maxima); missing or not finite: the worst case alone
    float hmax = b->copy[bf16_kind(metric)].limb_max, lmax = b->copy[bf16_kind(metric, true)].limb_max;
    if (c->tune.split_screen_worst_case || !(hmax >= 0.0f && lmax >= 0.0f && hmax - hmax == 0.0f && lmax - lmax == 0.0f)) hmax = lmax = -1.0f;
    const double accv = (6.0 * (double)b->D + 8.0) * 5.9604644775390625e-08 * 1.04 * (double)vmax;
    screen_margin_kernel<<<(unsigned)((Qpad + 3) / 4), 256, 0, c->stream>>>(cos ? 1 : 0, split_screen_scale(b, metric), sd,
                                                                           sd * vmax + 6.0f * (float)b->D, hmax, lmax, accv,
                                                                           c->q_norm.as<float>(), dQ, qscale, (uint32_t)b->D, (uint32_t)Q,
                                                                           (uint32_t)Qpad, m);
    INNR_HIP_CHECK(hipGetLastError());
    c->screen_q = Q;
    c->screen_qpad = Qpad;
    *out = m;
    return INNR_OK;
}

// One collect pass of the f32 GEMM filter (MODE 2) over nr queries Qr (row-major [nr][D]) with the FIXED per-query thresholds
// x[j] - E (x: exact scores -- distances for squared L2 -- on the device): every site whose approximate score clears its query's
// threshold goes to c->lists [Qpad][kCollectCap] (indices), c->counts [Qpad] (lengths; an overfull list keeps counting). Leaves the
// exact query norms at c->q_norm, the thresholds at c->seed_score (0: x[j] - E is not finite, everything is collected) and the
// pass between ev[2] and ev[3]. The completion pass of unproven kNN queries (x = x_k) and the range search (x = the caller's
// thresholds) share it.
static innr_status collect_pass(innr_batch* b, int metric, const float* Qr, size_t nr, size_t kout, const float* x) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    GemmPlan p = plan_gemm(b, nr, kout, (!cos && !l2 && nr > 256) ? 8u : 4u, !cos && !l2);
    if (cos) INNR_TRY(ensure_invnorms(b));
    if (l2) INNR_TRY(ensure_sqnorms(b));
    INNR_TRY(prep_queries(b, p, Qr, nr, cos));  // K-major queries, exact norms (c->q_norm), cosine: 1/|q| at c->misc
    float* invq = c->misc.as<float>();
    float* Cj = nullptr;
    if (l2) INNR_TRY(l2_query_consts(b, p.Qpad, nr, invq, &Cj));
    const float err_scale = f32_filter_scale(b, metric);
    // fixed thresholds: x - E (one key lower), in the kind's score space; 0 = "no bound" where that is not finite
    INNR_TRY(c->seed_score.ensure(p.Qpad * sizeof(uint32_t)));
    uint32_t* thr = c->seed_score.as<uint32_t>();
    seed_thresholds_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(x, (uint32_t)nr, 1u, metric_space(metric), err_scale,
                                                                                    c->q_norm.as<float>(), Cj, thr, (uint32_t)p.Qpad, 0u);
    INNR_HIP_CHECK(hipGetLastError());
    // global lists: [Qpad][kCollectCap] indices, [Qpad] lengths
    INNR_TRY(c->lists.ensure(p.Qpad * (size_t)kCollectCap * sizeof(uint32_t)));
    INNR_TRY(c->counts.ensure(p.Qpad * sizeof(uint32_t)));
    INNR_HIP_CHECK(hipMemsetAsync(c->counts.p, 0, p.Qpad * sizeof(uint32_t), c->stream));
    GemmPlan pl = p;
    pl.KP = kCollectCap;  // what the kernel takes as the list capacity (launch_gemm sizes the unused slots for MODE 2 by itself)
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    if (cos) INNR_TRY((launch_gemm<kGemmCos, 2>(b, pl, nr, c->q_kmajor.as<float>(), b->invn, invq, nullptr, 0, thr)));
    else if (l2) INNR_TRY((launch_gemm<kGemmL2, 2>(b, pl, nr, c->q_kmajor.as<float>(), b->sqn, invq, nullptr, 0, thr)));
    else INNR_TRY((launch_gemm<kGemmDot, 2>(b, pl, nr, c->q_kmajor.as<float>(), nullptr, nullptr, nullptr, 0, thr)));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    return INNR_OK;
}

// redo: the unproven queries (ascending), d_out_*: the first pass' output (its k-th score per query is read, the resolved
// queries' rows are overwritten). *unresolved: those that still need the exact engine.
static innr_status knn_complete(innr_batch* b, int metric, const float* dQ, const std::vector<uint32_t>& redo, size_t kout,
                                uint64_t* d_out_idx, float* d_out_score, std::vector<uint32_t>* unresolved, float* gemm_ms) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size();
    unresolved->clear();
    if (nr == 0) return INNR_OK;
    INNR_TRY(collect_gather(b, dQ, redo, kout, d_out_score));
    innr_ctx::RedoBufs& rb = c->cmpl;
    const float* Qr = rb.q.as<float>();
    INNR_TRY(collect_pass(b, metric, Qr, nr, kout, rb.qn.as<float>()));  // x_k per unproven query
    INNR_TRY(c->sel_cnt.ensure(nr * sizeof(uint32_t)));
    INNR_TRY(collect_finish(b, metric, Qr, c->q_norm.as<float>(), nr, kout, rb.idx.as<uint64_t>(), rb.sc.as<float>(), c->sel_cnt.as<uint32_t>()));
    return collect_scatter(b, redo, kout, d_out_idx, d_out_score, c->sel_cnt.as<uint32_t>(), unresolved, gemm_ms);  // (synchronises)
}

static uint32_t bf16_nk(const innr_batch* b, CopyKind kind = kCopyBfDot) {  // K-steps of 32, even
    return (uint32_t)(round_up((b->D ? b->D : 1) + (kind == kCopyBfL2 ? kBfL2Extra : 0), 64) / 32);
}

static size_t bf16_copy_bytes(const innr_batch* b, CopyKind kind = kCopyBfDot) { return (b->ldN / 128) * (size_t)bf16_nk(b, kind) * 512 * 16; }

// kind: kCopyBfDot, kCopyBfCos (rows scaled by 1/||v||; needs b->invn) or kCopyBfL2 (needs b->sqn)
static innr_status ensure_bf16_corpus(innr_batch* b, CopyKind kind) {
    const CorpusCopy& cc = b->copy[kind];
    if (cc.p) return INNR_OK;
    const uint32_t nk = bf16_nk(b, kind);
    const size_t units = (b->ldN / 128) * (size_t)nk * 512;  // 16-byte units
    INNR_TRY(alloc_copy(b, kind, units * 16, nk, false, "bf16 corpus copy"));
    pack_corpus_bf16_kernel<<<(unsigned)((units + 255) / 256), 256, 0, b->ctx->stream>>>(
        b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, nk, units, reinterpret_cast<uint4*>(cc.p), kind == kCopyBfCos ? b->invn : nullptr,
        kind == kCopyBfL2 ? b->sqn : nullptr);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

static innr_status launch_gemm_bf16(innr_batch* b, const GemmPlan& p, size_t nreal_q, const uint32_t* seed, CopyKind kind,
                                    const float* kmargin = nullptr, uint32_t kk = 0) {
    innr_ctx* c = b->ctx;
    const CorpusCopy& cc = b->copy[kind];
    uint32_t* gslots = nullptr;
    size_t nslot = 0;
    if (!kmargin) kk = 0;
    INNR_TRY(prep_gthr(c, p.Qpad, p.KP, seed, nreal_q, kmargin, &gslots, &nslot));
    if (p.cap < 768) {  // choose_f32_filter: lists of pick_kp(4k + 64), 128 or 256 candidates
        set_error("internal: the bf16 filter has no lists of %u candidates", p.KP);
        return INNR_E_BAD_ARG;
    }
    dispatch([&](auto rr) {  // (every instantiation has a row in tests/test_gpu_kernel_variants.py: GEMM_BF16)
        launch_kernel(c, Inst<kLaunchGemmBf16, rr, 0, 1>(), {p.nblocks, 64 * kBfWaves, 0, p.nqt}, cc.p, nullptr, c->q_bf16.as<char>(),
                      (uint32_t)(b->ldN / 128), (uint32_t)b->N, cc.nk, p.Qpad, p.nqt, p.qtg, p.tps, c->lists.as<uint64_t>(),
                      c->counts.as<uint32_t>(), p.KP, kk, c->flags.as<uint32_t>(), gslots, gslots + nslot, nullptr, 0);
    }, one_of<12, 20>(p.cap / 64));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ---- split-bf16 filter of INNR_KNN_MFMA (kernels_gemm_bf16.h, LIMBS = 3) ---------------------------------
// Which filter kernel the last first pass of knn_mfma launched (innr_ctx::last_filter; innrdbg_last_filter).
enum LastFilter { kFilterNone = 0, kFilterF32 = 1, kFilterBf16 = 2, kFilterSplit = 3 };
// Smallest batch the split filter serves by default: its 512-query tile against the f32 kernel's narrow tiles, measured at C2
// (tools/split_ab.py, profiles/r04_split_ab.txt): 64 queries 13.9 ms split vs 9.2 f32 (one-wave tile), 128 queries 14.5 vs 15.7
// (two-wave tile), 256 queries 15.5 vs 28.8.
constexpr size_t kSplitMinQ = 65;
// Largest share of a call's wave tiles the screened form may correct before the batch's later calls take the full loop: between
// the measured winners and losers at C2 (profiles/r05_split_ab.txt): 18 % corrected (k = 10) 21.2 against 34.5 ms at 1024 queries,
// 31 % (k = 100, 65 queries) 12.0 against 13.9; 58 % (k = 100, 128 ... 4096 queries) 14.8 ... 151.1 against 14.6 ... 137.4, LCG data
// 98 % and 182.0 against 145.3 ms for first pass + completion. A line through the first and the last crosses near 45 %.
constexpr float kScreenMaxShare = 0.45f;

// the lo limbs of the dot / cosine kind (the cosine kind needs b->invn); soft: under the memory rule, else as a filter copy
static innr_status ensure_bf16_lo(innr_batch* b, int metric, bool soft) {
    const CopyKind hk = bf16_kind(metric), lk = bf16_kind(metric, true);
    CorpusCopy& lo = b->copy[lk];
    if (lo.p) return INNR_OK;
    const uint32_t nk = bf16_nk(b, hk);
    const size_t bytes = bf16_copy_bytes(b, hk);
    INNR_TRY(alloc_copy(b, lk, bytes, nk, soft, "bf16 lo-limb copy"));
    if (!lo.p) return INNR_OK;
    const size_t units = bytes / 16;
    pack_corpus_bf16_kernel<<<(unsigned)((units + 255) / 256), 256, 0, b->ctx->stream>>>(
        b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, nk, units, reinterpret_cast<uint4*>(lo.p), hk == kCopyBfCos ? b->invn : nullptr,
        nullptr, 1);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// The largest limb norms of a split pair that exists (CorpusCopy::limb_max of the hi and of the lo copy: the screen margin reads
// them, split_screen_scale): one pass over the f32 store with the copies' own row scaling, once per pair -- when the pair is
// built or prebuilt, or at the first split call on a hi copy another engine built. Synchronises (two words come back).
static innr_status ensure_limb_maxima(innr_batch* b, int metric) {
    CorpusCopy &hi = b->copy[bf16_kind(metric)], &lo = b->copy[bf16_kind(metric, true)];
    if (!hi.p || !lo.p || (!(hi.limb_max < 0.0f) && !(lo.limb_max < 0.0f))) return INNR_OK;
    innr_ctx* c = b->ctx;
    uint32_t* d = nullptr;
    INNR_HIP_CHECK(hipMalloc((void**)&d, 2 * sizeof(uint32_t)));
    uint32_t h[2] = {0u, 0u};
    hipError_t e = hipMemsetAsync(d, 0, sizeof(h), c->stream);
    uint32_t nrows = (uint32_t)b->N;
#if defined(INNR_MUTATE_LIMB_MAX) && INNR_MUTATE_LIMB_MAX == 2  // mutation check, never the product: all rows but the last tile's
    nrows = nrows ? (nrows - 1) / 128 * 128 : 0;
#endif
    if (e == hipSuccess) {
        limb_maxima_kernel<<<(unsigned)((b->ldN / 4 + 255) / 256), 256, 0, c->stream>>>(
            b->V, b->ldN, nrows, (uint32_t)b->D, metric == INNR_METRIC_COSINE ? b->invn : nullptr, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    INNR_HIP_CHECK(e);
#if defined(INNR_MUTATE_LIMB_MAX) && INNR_MUTATE_LIMB_MAX == 1  // ... Lmax forced to 0
    h[1] = 0u;
#endif
    memcpy(&hi.limb_max, &h[0], sizeof(float));
    memcpy(&lo.limb_max, &h[1], sizeof(float));
    return INNR_OK;
}

// The hi and lo limb copies of the dot / cosine kind. Each copy is built only when it fits (copy_fits, the rule of the other
// filter copies); *ok == false: one did not fit, the call filters on the f32 kernel instead.
static innr_status ensure_split_corpus(innr_batch* b, int metric, bool* ok) {
    *ok = false;
    const CopyKind hk = bf16_kind(metric), lk = bf16_kind(metric, true);
    CorpusCopy &hi = b->copy[hk], &lo = b->copy[lk];  // (lo.refused stands for the pair)
    if (lo.refused) return INNR_OK;
    const size_t bytes = bf16_copy_bytes(b, hk);
    // the budget has to admit what is missing of the PAIR, before either limb is built (not remembered: the next call asks again)
    if (!budget_admits(b, (hi.p ? 0 : bytes) + (lo.p ? 0 : bytes))) return INNR_OK;
    if (!hi.p) {  // (the rule like a lo limb; once it passes, a filter copy like any other: INNR_E_OOM when hipMalloc fails)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !copy_fits(free_b, bytes)) {
            lo.refused = true;
            return INNR_OK;
        }
        INNR_TRY(ensure_bf16_corpus(b, hk));
    }
    INNR_TRY(ensure_bf16_lo(b, metric, true));
    *ok = lo.p != nullptr;
    if (*ok) INNR_TRY(ensure_limb_maxima(b, metric));
    return INNR_OK;
}

// c->q_bf16: the queries' hi limbs (nk K-steps), then their lo limbs (cosine: of the normalised queries, qscale = 1/||q||)
static innr_status pack_queries_split(innr_batch* b, const GemmPlan& p, const float* dQ, size_t Q, const float* qscale) {
    innr_ctx* c = b->ctx;
    const uint32_t nk = bf16_nk(b);
    const size_t units = (size_t)nk * 4 * p.Qpad;
    INNR_TRY(c->q_bf16.ensure(2 * units * 16));
    for (int l = 0; l < 2; ++l) {
        pack_queries_bf16_kernel<<<(unsigned)((units + 255) / 256), 256, 0, c->stream>>>(
            dQ, (uint32_t)Q, (uint32_t)b->D, nk, (uint32_t)p.Qpad, reinterpret_cast<uint4*>(c->q_bf16.p) + l * units, qscale, nullptr, l);
        INNR_HIP_CHECK(hipGetLastError());
    }
    return INNR_OK;
}

template <int MODE>
static innr_status launch_gemm_split(innr_batch* b, const GemmPlan& p, size_t nreal_q, int metric, const uint32_t* seed,
                                     const float* kmargin = nullptr, uint32_t kk = 0, float* dump = nullptr, size_t ld_dump = 0,
                                     const float* smargin = nullptr) {
    innr_ctx* c = b->ctx;
    const CorpusCopy &hi = b->copy[bf16_kind(metric)], &lo = b->copy[bf16_kind(metric, true)];
    uint32_t* gslots = nullptr;
    size_t nslot = 0;
    if (!kmargin) kk = 0;
    if (hi.nk % kBfLead != 0) {  // bf16_nk: the K-loop's ring position and the correction's two K-steps per batch rely on it
        set_error("internal: the bf16 copy has an odd number of K-steps (%u)", hi.nk);
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(prep_gthr(c, p.Qpad, p.KP, seed, nreal_q, kmargin, &gslots, &nslot, smargin));
    // smargin: the screened form (hi.hi K-loop, lo products where a wave can hit) -- one record for both forms
    const bool screened = MODE == 0 && smargin != nullptr;
    const auto launch = [&](auto rr) {
        const Inst<kLaunchGemmSplit, rr, MODE, 3> inst;
        auto kernel = kernel_of(inst);
        if constexpr (MODE == 0) {
            if (screened) kernel = screened_kernel_of(inst);
        }
        launch_kernel_as(c, inst, kernel, {p.nblocks, 64 * kBfWaves, 0, p.nqt}, hi.p, lo.p, c->q_bf16.as<char>(),
                         (uint32_t)(b->ldN / 128), (uint32_t)b->N, hi.nk, p.Qpad, p.nqt, p.qtg, p.tps, c->lists.as<uint64_t>(),
                         c->counts.as<uint32_t>(), p.KP, kk, c->flags.as<uint32_t>(), gslots, gslots + nslot, dump, ld_dump);
    };
    if constexpr (MODE == 1) launch(IntC<6>());  // the dense-score dump: the list geometry plays no part
    else dispatch(launch, rr_gemm(p.cap));       // (every instantiation has a row in tests/test_gpu_kernel_variants.py: GEMM_SPLIT)
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ---- the split filter's own seeder: its first chip-wide bounds from a prefix pass on the matrix pipe ----
// The exact seeder below costs exact-engine time per prefix row (the C2 shape: 0.30 ms for 2048 rows) and its bound has to be
// exact only because the f32 scan makes it so: the k rule needs a VALID lower bound of the k-th best score, no more. The split
// kernel in MODE 3 scores a prefix P of whole tiles with the filter's own arithmetic and keeps the best score of every group of 32
// rows; the k-th largest of a query's P / 32 group maxima, less 2E, is such a bound (split_seed_kernel), and a prefix eight times
// as long costs a fifth of the scan. A longer prefix also starts the bounds higher: a one-pass top-k admits about k ln(N / n0)
// rows per query behind a seed from n0 rows, and every admission is a flagged wave tile of the screened kernel.
// Rows: split_seed_rows (0: kSplitSeedRows), clamped to a multiple of 1024 within N / 32 (seeding_on's rule: the corpus is at least
// 32 prefixes; P / 128 is then a multiple of 8, the kernel's block map) and to kSeedMaxGroups groups. 0 = the exact seeder: the
// option says so (-1), gemm_seed_n or gemm_no_seed is set, the k rule is off, lists beyond 128, or fewer than k groups (with
// exactly k the bound is the smallest group maximum: weak, and as valid as any; the default prefix has 512 groups for k <= 112).
constexpr size_t kSplitSeedRows = 16384;
static size_t split_seed_rows(const innr_batch* b, uint32_t KP, size_t kout) {
    const innr_tuning& t = b->ctx->tune;
    if (t.split_seed_rows < 0 || t.gemm_seed_n != 0 || t.gemm_no_seed || t.no_k_rule || KP > 128) return 0;
    size_t P = t.split_seed_rows >= 1024 ? (size_t)t.split_seed_rows : kSplitSeedRows;
    P = std::min(P, std::min(b->N / 32, (size_t)kSeedMaxGroups * 32)) / 1024 * 1024;
    return P / 32 >= kout ? P : 0;
}
// seeds of the call's queries at *sd [p.Qpad] (c->seed_score), the group maxima as order keys at c->seed_idx [P / 32][p.Qpad].
// The queries are packed (pack_queries_split) and their norms stand in c->q_norm.
static innr_status seed_split(innr_batch* b, const GemmPlan& p, int metric, size_t Q, size_t kout, float err_scale, size_t P,
                              uint32_t** sd) {
    innr_ctx* c = b->ctx;
    const CorpusCopy &hi = b->copy[bf16_kind(metric)], &lo = b->copy[bf16_kind(metric, true)];
    const uint32_t ntiles = (uint32_t)(P / 128), ngroups = (uint32_t)(P / 32);
    if (hi.nk % kBfLead != 0 || ntiles % 8 != 0 || P > b->N || ngroups > kSeedMaxGroups || kout > ngroups) {
        set_error("internal: the split seeder's geometry (%zu rows, %u K-steps)", P, hi.nk);
        return INNR_E_BAD_ARG;
    }
    INNR_TRY(c->seed_idx.ensure((size_t)ngroups * p.Qpad * sizeof(uint32_t)));
    INNR_TRY(c->seed_score.ensure(p.Qpad * sizeof(uint32_t)));
    // one tile per block, the kernel's own block -> (slice, query tile) map: slices = tiles, a multiple of 8
    const Inst<kLaunchSplitSeed, 6, 3, 3> inst;
    launch_kernel(c, inst, {p.nqt * ntiles, 64 * kBfWaves, 0, p.nqt}, hi.p, lo.p, c->q_bf16.as<char>(), ntiles, (uint32_t)P, hi.nk,
                  p.Qpad, p.nqt, p.qtg, 1u, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.KP, 0u, c->flags.as<uint32_t>(),
                  (uint32_t*)nullptr, (uint32_t*)nullptr, c->seed_idx.as<float>(), p.Qpad);
    INNR_HIP_CHECK(hipGetLastError());
    split_seed_kernel<<<(unsigned)p.Qpad, 64, 0, c->stream>>>(c->seed_idx.as<uint32_t>(), ngroups, (uint32_t)p.Qpad, (uint32_t)Q,
                                                               (uint32_t)kout, metric == INNR_METRIC_COSINE, err_scale,
                                                               c->q_norm.as<float>(), c->seed_score.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    *sd = c->seed_score.as<uint32_t>();
    return INNR_OK;
}

// rows of the corpus prefix whose exact top-KP seeds the chip-wide thresholds (INNR_GEMM_SEED_N overrides: tools/seed_ab.py)
// C2 shape, whole call (tools/seed_ab.py): int8 filter 13.50 / 12.80 / 12.38 / 12.12 / 12.59 ms at 512 / 1024 / 2048 / 4096 / 8192 rows
// (without seeds 17.5), bf16 filter 16.14 -> 16.00 at 4096; the f32 kernel, whose visits are cheap next to its MFMAs, 107.37 / 107.42 /
// 107.72 at 2048 / 4096 / 8192: the fast pipes take 4096 rows, the f32 pipe 2048.
// (The seeding scan costs Q x rows: at 4096 queries the C5 shape went 41.2 -> 43.3 ms with 4096 rows, so larger batches keep 2048.)
static size_t seed_prefix_rows(const innr_ctx* c, bool fast_pipe, size_t Q) {
    const long v = c->tune.gemm_seed_n;
    return v >= 256 ? (size_t)v : (size_t)((fast_pipe && Q <= 2048) ? 4096 : 2048);
}

// threshold seeding from the exact top-k of a corpus prefix (seed_thresholds_*kernel): corpora of 32 prefixes or more, lists <= 128
static bool seeding_on(const innr_batch* b, bool fast_pipe, size_t Q, uint32_t KP) {
    return b->N >= 32 * seed_prefix_rows(b->ctx, fast_pipe, Q) && KP <= 128 && !b->ctx->tune.gemm_no_seed;
}
// The prefix's exact top-kseed per query at c->seed_score [Q][kseed], best first, by exact(kseed, idx, score, rows) (the caller's
// exact engine over the first `rows` vectors); *sd: room for the [Qpad] thresholds the caller's kernel derives from them.
template <class ExactTopK>
static innr_status seed_prefix(innr_batch* b, bool fast_pipe, size_t Q, size_t Qpad, uint32_t KP, size_t kout, uint32_t* kseed,
                               uint32_t** sd, ExactTopK&& exact) {
    innr_ctx* c = b->ctx;
    // k rule (topk_dev.h): the prefix's k-th best exact score, less E, already bounds the corpus' top k; KP rule: its KP-th
    const uint32_t ks = c->tune.no_k_rule ? KP : (uint32_t)kout;
    INNR_TRY(c->seed_idx.ensure(Q * ks * sizeof(uint64_t)));
    INNR_TRY(c->seed_score.ensure(Q * ks * sizeof(float) + Qpad * sizeof(uint32_t)));
    INNR_TRY(exact(ks, c->seed_idx.as<uint64_t>(), c->seed_score.as<float>(), seed_prefix_rows(c, fast_pipe, Q)));
    *kseed = ks;
    *sd = reinterpret_cast<uint32_t*>(c->seed_score.as<float>() + Q * ks);
    return INNR_OK;
}

// knn_mfma's filter (kFilterBf16 / kFilterSplit / kFilterF32), its plan (list length included) and its bound err_scale
static innr_status choose_f32_filter(innr_batch* b, int metric, size_t Q, size_t kout, bool bf16, uint32_t kp_force, int level,
                                     int* filter, GemmPlan* plan, float* err_scale) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    // bf16 filter: every kind as the plain dot of bf16 copies (cosine: corpus and queries NORMALISED before the rounding;
    // squared L2: six more K columns carry |v|^2 and the query's constant, pack_corpus_bf16_kernel) -- no norm is loaded in
    // the kernel; candidate lists of 4k + 64 (its bound E is ~2^-7 |q||v|, so the k-th exact score must clear the KP-th
    // approximate one by a visible margin), a corpus whose scores are far from the denormal range (L2: and from overflow)
    const bool use_bf16 = bf16 && pick_kp(4 * kout + 64, 0) <= 256 && b->max_norm >= 1e-12f &&
                          (b->max_norm - b->max_norm == 0.0f) && (!l2 || b->max_norm <= 1e15f);
    // split-bf16 filter: dot and cosine from kSplitMinQ queries on, lists up to 256, a corpus whose norm keeps
    // the limbs' flush-to-zero terms far below E (or a non-finite one: every query is redone exactly below either way)
    const bool mfin = b->max_norm - b->max_norm == 0.0f;
    const size_t split_q = c->tune.split_min_q > 0 ? (size_t)c->tune.split_min_q : kSplitMinQ;
    bool use_split = !use_bf16 && !l2 && !c->tune.no_split_filter && Q >= split_q && pick_kp(kout, 16) <= 256 &&
                     (!mfin || (b->max_norm >= 1e-12f && b->max_norm <= 1e18f));
    if (use_split) {
        if (cos) INNR_TRY(ensure_invnorms(b));
        INNR_TRY(ensure_split_corpus(b, metric, &use_split));  // does not fit: the f32 kernel
    }
    *filter = use_bf16 ? kFilterBf16 : (use_split ? kFilterSplit : kFilterF32);
    if (level == 0) c->last_filter = *filter;
    GemmPlan p = plan_gemm(b, Q, kout, (use_bf16 || use_split) ? 8 : 0, !cos && !l2);
    if (kp_force && !use_bf16 && kp_force >= p.KP && kp_force <= 256) {  // second attempt of redo_batch: longer lists
        p.KP = kp_force;
        p.cap = (uint32_t)cand_cap((int)p.KP);
    }
    if (use_bf16) {
        p.KP = pick_kp(4 * kout + 64, 0);
        p.cap = (uint32_t)cand_cap((int)p.KP);
    }
    *plan = p;
    *err_scale = use_bf16 ? bf16_filter_scale(b, metric) : use_split ? split_filter_scale(b, metric) : f32_filter_scale(b, metric);
    return INNR_OK;
}

static innr_status knn_mfma(innr_batch* b, int metric, const float* dQ, size_t Q, size_t kout, const float* /*dQn*/,
                            uint64_t* d_out_idx, float* d_out_score, uint32_t* nfallback, uint32_t* kept,
                            float* gemm_ms, bool bf16, uint32_t kp_force, int level) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    INNR_TRY(ensure_norms(b));  // exact norms: cosine epilogue + max norm for the dot / L2 error bounds
    int filter;
    GemmPlan p;
    float err_scale;
    INNR_TRY(choose_f32_filter(b, metric, Q, kout, bf16, kp_force, level, &filter, &p, &err_scale));
    const bool use_bf16 = filter == kFilterBf16, use_split = filter == kFilterSplit;
    const CopyKind bfv = bf16_kind(metric);
    if (cos) INNR_TRY(ensure_invnorms(b));
    if (l2) INNR_TRY(ensure_sqnorms(b));
    INNR_TRY(prep_queries(b, p, dQ, Q, cos));  // K-major queries, exact query norms (c->q_norm), cosine: 1/||q|| at c->misc
    if (use_bf16) INNR_TRY(ensure_bf16_corpus(b, bfv));
    INNR_TRY(ensure_lists(c, p));
    float* invq = c->misc.as<float>();
    uint32_t* fallback = reinterpret_cast<uint32_t*>(c->misc.as<char>() + p.Qpad * sizeof(float));
    INNR_HIP_CHECK(hipMemsetAsync(fallback, 0, Q * sizeof(uint32_t), c->stream));
    float* Cj = nullptr;
    if (l2) INNR_TRY(l2_query_consts(b, p.Qpad, Q, invq, &Cj));
    if (use_bf16) {  // (after the L2 constants: the squared-L2 packing carries c_j = C_j - |q_j|^2 in three K columns)
        const uint32_t nk = bf16_nk(b, bfv);
        INNR_TRY(c->q_bf16.ensure((size_t)nk * 4 * p.Qpad * 16));
        pack_queries_bf16_kernel<<<(unsigned)(((size_t)nk * 4 * p.Qpad + 255) / 256), 256, 0, c->stream>>>(
            dQ, (uint32_t)Q, (uint32_t)b->D, nk, (uint32_t)p.Qpad, reinterpret_cast<uint4*>(c->q_bf16.p),
            cos ? c->misc.as<float>() : nullptr, l2 ? invq : nullptr);
        INNR_HIP_CHECK(hipGetLastError());
    }
    if (use_split) INNR_TRY(pack_queries_split(b, p, dQ, Q, cos ? c->misc.as<float>() : nullptr));

    const uint32_t* seed = nullptr;
    const size_t split_rows = use_split ? split_seed_rows(b, p.KP, kout) : 0;  // the split filter's own seeder, or 0: the exact one
    if (level == 0) c->split_seed_served = split_rows;
    if (split_rows) {
        uint32_t* sd;
        INNR_TRY(seed_split(b, p, metric, Q, kout, err_scale, split_rows, &sd));
        seed = sd;
    } else if (seeding_on(b, use_bf16, Q, p.KP)) {
        uint32_t kseed, *sd;
        INNR_TRY(seed_prefix(b, use_bf16, Q, p.Qpad, p.KP, kout, &kseed, &sd, [&](uint32_t ks, uint64_t* idx, float* sc, size_t rows) {
            return knn_exact_range(b, metric, dQ, b->D, c->q_norm.as<float>(), 0, Q, ks, idx, sc, ScanExt(), rows);
        }));
        seed_thresholds_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(
            c->seed_score.as<float>(), (uint32_t)Q, kseed, metric_space(metric), err_scale, c->q_norm.as<float>(), Cj, sd,
            (uint32_t)p.Qpad, kseed - 1);
        INNR_HIP_CHECK(hipGetLastError());
        seed = sd;
        // the exact engine used the shared list workspace: size it for the GEMM pass again
        INNR_TRY(ensure_lists(c, p));
    }

    // the k rule of topk_dev.h: 2E per query, in the score space of the kind
    const float* kmargin = nullptr;
    // the screened form of the split filter (hi.hi K-loop, lo products where a wave can hit), measured at C2 against the full loop
    // (tools/split_ab.py, profiles/r05_split_ab.txt): lists of 32 win at every size, 65 ... 4096 queries 6.8 ... 77.6 ms against
    // 13.5 ... 134.9 (18 % of the wave tiles corrected), cosine at 4096 73.1 against 135.0; lists of 128 (k = 100) at 65 / 128 / 256 /
    // 1024 / 4096 queries 12.0 / 14.8 / 17.4 / 37.9 / 151.1 against 13.9 / 14.6 / 15.8 / 35.1 / 137.4 -- long lists keep lower
    // thresholds (58 % corrected from 128 queries on, 31 % at 65) and R = 12 / 20 reload spilled registers per tile: those keep
    // the full loop beyond 128 queries, and at 128 the share rule below sends the batch's later calls there
    // Data decides as well: where the thresholds sit among near-ties (the reference example's LCG rows) nearly every sub-tile is
    // corrected and a corrected tile costs more than the full loop's (182.7 against 146.3 ms at 1024 queries). The kernel counts
    // the wave tiles it corrects (flag words kScreenCountWord); the first pass reads them with its proof flags and the batch
    // remembers the share per list class. Above kScreenMaxShare later calls take the full loop and every 64th screens again
    // (the data or the batch size may have changed). no_split_screen: 1 never screens, -1 always does.
    // Round 6 (pair correction for lists up to 64, profiles/r06_split_ab.txt): a flagged wave tile of a short list costs one or two
    // round trips instead of a sub-tile's dozen, so the screen's lead at 18 % grows (1024 queries: 15 against 34 ms); the long lists'
    // kernels have no room for the pair path and keep rule and figures. The share still counts flagged wave tiles (word 32): between
    // the 18 % of uniform data and the 98 % of LCG data, whose wave tiles overflow the pair queue and pay the sub-tile correction
    // as before, the sweep has no point that would place the constant anywhere else.
    // Round 7 (margin from the limbs' norms, publish cadence 4; profiles/r07_split_ab.txt): uniform data flags 8.4 % (k = 10) and
    // 40 % (k = 100) of its wave tiles, and lists of 128 are now faster screened at every size swept (256 queries 14.4 against
    // 15.7 ms, 4096 125.6 against 136.4). Both rules are left as they were: 40 % sits just under kScreenMaxShare, and lists of 256
    // and data between uniform and LCG have not been swept.
    const int scls = p.KP <= 64 ? 0 : 1;
    // (lists up to 64 run the pair correction, whose query offsets are 32 bits up to kPairMaxQpad = 2^20 queries: larger batches of
    //  short lists take the full loop whatever no_split_screen says; the long lists' kernels have no pair path and no such limit)
    bool screen = use_split && c->tune.no_split_screen <= 0 && (p.KP > 64 || p.Qpad <= kPairMaxQpad);
    if (screen && c->tune.no_split_screen == 0) {
        screen = p.KP <= 64 || Q <= 128;
        if (screen && level == 0 && b->screen_share[scls] > kScreenMaxShare && (++b->screen_skips[scls] % 64u) != 0) screen = false;
    }
    if (screen) INNR_TRY(c->kmargin.ensure(2 * p.Qpad * sizeof(float)));  // (before make_kmargin: growing the buffer drops its contents)
    INNR_TRY(make_kmargin(c, metric_space(metric), err_scale, c->q_norm.as<float>(), Cj, nullptr, 0.0f, nullptr, Q, p.Qpad, &kmargin));
    const float* smargin = nullptr;
    if (screen) INNR_TRY(make_screen_margin(b, metric, dQ, cos ? c->misc.as<float>() : nullptr, Q, p.Qpad, &smargin));
    const uint32_t kk = (uint32_t)kout;
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    if (use_bf16) INNR_TRY(launch_gemm_bf16(b, p, Q, seed, bfv, kmargin, kk));
    else if (use_split) INNR_TRY(launch_gemm_split<0>(b, p, Q, metric, seed, kmargin, kk, nullptr, 0, smargin));
    else if (cos) INNR_TRY((launch_gemm<kGemmCos, 0>(b, p, Q, c->q_kmajor.as<float>(), b->invn, invq, nullptr, 0, seed, kmargin, kk)));
    else if (l2) INNR_TRY((launch_gemm<kGemmL2, 0>(b, p, Q, c->q_kmajor.as<float>(), b->sqn, invq, nullptr, 0, seed, kmargin, kk)));
    // (A first pass of the same kernel over 1/16 of the corpus, only to harvest tighter bounds for the full pass, was
    //  tried: 17.6 ms for both against 16.4 for the single pass.)
    else INNR_TRY((launch_gemm<kGemmDot, 0>(b, p, Q, c->q_kmajor.as<float>(), nullptr, nullptr, nullptr, 0, seed, kmargin, kk)));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));

    INNR_TRY(run_select(c, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.nslices, (uint32_t)p.Qpad, p.cap, p.KP,
                        (uint32_t)Q));
    INNR_TRY(launch_rescore(b, metric_space(metric), dQ, Q, Cj, p.KP, kout, err_scale, d_out_idx, d_out_score, fallback, nullptr,
                            !c->tune.rescore_all, gthr_bounds(c, p.Qpad, p.KP), /*tight=*/!use_bf16));

    std::vector<float> qn_host((use_bf16 || use_split) && !cos ? Q : 0);
    if (!qn_host.empty()) INNR_HIP_CHECK(copy_out(c, qn_host.data(), c->q_norm.p, Q * sizeof(float)));  // (the harvest synchronises)
    // bf16 products / sums below the normal range may be flushed to zero: the bound E must dwarf that, else redo exactly
    // (split filter: the query-side gate of its bound, see split_filter_scale).
    // A non-finite corpus value (max_norm is then NaN or inf) voids every error bound -- for cosine too, whose bound does
    // not carry max_norm: NaN * 0 approximations can differ from the reference's 0.0 (batch.rs:722) by more than E.
    const bool mfin = b->max_norm - b->max_norm == 0.0f;
    const auto unprovable = [&](size_t q) {
        if (!mfin) return true;
        if (q >= qn_host.size()) return false;
        return use_bf16 ? !(qn_host[q] * b->max_norm >= 1e-25f) : !(qn_host[q] == 0.0f || (qn_host[q] >= 1e-12f && qn_host[q] <= 1e18f));
    };
    uint32_t screened[2] = {0u, 0u};  // corrected wave tiles / sub-tiles of this first pass (delivered by the harvest's synchronise)
    if (screen && level == 0) INNR_HIP_CHECK(copy_out(c, screened, c->flags.as<uint32_t>() + kScreenCountWord, sizeof(screened)));
    std::vector<uint32_t> redo;  // margin proof failed (near-tie at the cut, or non-finite scores)
    INNR_TRY(harvest_proof(c, fallback, Q, p.KP, &redo, nfallback, kept, gemm_ms, unprovable));
    if (screen && level == 0)  // of the wave tiles that hold a real query (padding queries are closed and never corrected)
        b->screen_share[scls] = (float)screened[0] / (float)((b->ldN / 128) * ((Q + 63) / 64));
    // f32 engine: ONE completion pass resolves what the first pass could not prove (knn_complete); a handful of queries is
    // cheaper on the exact engine (one 8-query corpus pass costs less than a GEMM pass over a 256-query tile)
    bool completed = false;
    if (!use_bf16 && redo.size() > 8 && !c->tune.no_completion && (b->max_norm - b->max_norm == 0.0f)) {
        completed = true;
        std::vector<uint32_t> still;
        INNR_TRY(knn_complete(b, metric, dQ, redo, kout, d_out_idx, d_out_score, &still, gemm_ms));
        redo.swap(still);
        if (cos || !redo.empty()) {  // (the completion pass used the query workspace: the redo below reads the norms again)
            query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, b->D, c->q_norm.as<float>());
            INNR_HIP_CHECK(hipGetLastError());
        }
    }
    if (!redo.empty()) {
        const float* qn_all = cos ? c->q_norm.as<float>() : nullptr;
        uint32_t via = 0;
        if (use_bf16 && redo.size() >= 4) {
            // The bf16 bound is ~2^15 times the f32 one: on data with small gaps at the cut many proofs fail. Those
            // queries go through the f32 GEMM engine as one batch (its own proof, and the exact engine behind it).
            via = pick_kp(kout, 16);
        } else if (!use_bf16 && !completed && !kp_force && p.KP < 256 && redo.size() >= 16 && redo.size() * 4 <= Q &&
                   !c->tune.gemm_no_kp_retry) {
            // A minority of the batch failed: isolated clusters of near-equal scores (duplicates, quantised data), which
            // lists of 256 candidates usually swallow -- one more GEMM pass over those queries instead of an exact scan
            // for each 8 of them. When most of the batch fails the data is degenerate (the reference example's LCG
            // rows: hundreds of vectors within 2E of the k-th): straight to the exact engine.
            via = 256;
        }
        if (redo.size() == 1 && !via) {
            INNR_TRY(knn_exact_range(b, metric, dQ, b->D, qn_all, redo[0], 1, kout, d_out_idx, d_out_score));
        } else {
            // at most two levels: a second GEMM attempt (kp_force set, never bf16) sends its own failures to the exact engine
            INNR_TRY(redo_batch(b, metric, dQ, qn_all, redo, kout, d_out_idx, d_out_score, level == 0 ? via : 0u, level));
        }
    }
    if (bf16 && !use_bf16) *gemm_ms = -*gemm_ms;  // told apart by the caller: the f32 engine served this call
    return INNR_OK;
}

// tools/i8h_probe.py (builds with -DINNR_I8H_PROBE=<bits>, never the product library): with bit 1 the one-limb int8 kernel never
// visits its append path -- what the K-loop and the fast reject cost alone. Such a call fills its stats and then FAILS: a timing
// run must not hand out results.
static constexpr bool i8h_probe_skips_visits() {
    return (kI8hProbe & (1 | 8 | 16 | 32 | 64 | 128)) != 0;  // (8, 16: the K-loop fed from L1 / L2 instead of its real operands)
}

innr_status check_errflag(innr_ctx* c) {
    uint32_t e = 0;
    INNR_HIP_CHECK(copy_out(c, &e, c->flags.p, sizeof(e)));
    INNR_HIP_CHECK(ctx_sync(c));
    if constexpr ((kI8hProbe & 4) != 0) {  // tools/i8h_probe.py: the one-limb int8 kernel's visit counters
        uint32_t h[24] = {0};
        INNR_HIP_CHECK(hipMemcpyAsync(h, c->flags.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        INNR_HIP_CHECK(hipStreamSynchronize(c->stream));
        unsigned long long cv, cs, ct, cq;
        memcpy(&cv, h + 12, 8); memcpy(&cs, h + 14, 8); memcpy(&ct, h + 16, 8); memcpy(&cq, h + 20, 8);
        fprintf(stderr, "i8h probe: wave epilogues that visit %u | survivors of the coarse test %u | bound re-derivations %u | cycles per "
                "visit %.0f, of them in the survivors' loops %.0f, publish + compaction %.0f | appended %u (summed over lanes) | wave epilogues "
                "with a hit %u, cycles queueing each %.0f | longest wave %.0f cycles, shortest %.0f\n", h[8], h[9], h[10],
                h[8] ? (double)cv / h[8] : 0.0, h[8] ? (double)cs / h[8] : 0.0, h[8] ? (double)ct / h[8] : 0.0, h[11], h[18],
                h[18] ? (double)cq / h[18] : 0.0, 16.0 * h[22], 16.0 * (double)(~h[23]));
        uint32_t hb[512] = {0};
        INNR_HIP_CHECK(hipMemcpyAsync(hb, c->flags.as<uint32_t>() + 128, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
        INNR_HIP_CHECK(hipStreamSynchronize(c->stream));
        fprintf(stderr, "i8h probe: Mcycles per block:");
        for (int i = 0; i < 512 && hb[i]; ++i) fprintf(stderr, "%s%.1f", i % 32 ? " " : "\n  ", 16e-6 * hb[i]);
        fprintf(stderr, "\n");
    }
    if (e) {
        set_error("internal: candidate-list invariant violated (flag=%u)", e);
        return INNR_E_HIP;
    }
    return INNR_OK;
}

// the cached selection of innr_batch_knn_filtered_multi (innr_batch::fsel), if any
static void free_selection(innr_batch* b) {
    if (b->fsel) innr_batch_free(b->fsel);
    if (b->fsel_mask) (void)hipFree(b->fsel_mask);
    if (b->fsel_map) (void)hipFree(b->fsel_map);
    b->fsel = nullptr;
    b->fsel_mask = nullptr;
    b->fsel_map = nullptr;
    b->fsel_mask_bytes = b->fsel_map_bytes = 0;
}

}  // namespace innr

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

const char* innr_last_error(void) { return g_err; }
const char* innr_version(void) { return "innr-hip 0.1.0 (gfx950)"; }

innr_status innr_ctx_create(int device, innr_ctx** out) {
    if (!out) {
        set_error("out is null");
        return INNR_E_BAD_ARG;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s): this library has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return INNR_E_HIP;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range [0,%d)", device, count);
        return INNR_E_BAD_ARG;
    }
    INNR_HIP_CHECK(hipSetDevice(device));
    innr_ctx* c = new (std::nothrow) innr_ctx();
    if (!c) return INNR_E_OOM;
    c->device = device;
    tuning_from_env(&c->tune);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipStreamCreate failed");
        delete c;
        return INNR_E_HIP;
    }
    c->own_stream = true;
    for (auto& ev : c->ev) (void)hipEventCreate(&ev);
    if (hipHostMalloc((void**)&c->pin, kPinIn + kPinOut, hipHostMallocDefault) != hipSuccess) c->pin = nullptr;  // optional
    innr_status s = c->flags.ensure(4096);
    if (s != INNR_OK) {
        innr_ctx_destroy(c);
        return s;
    }
    (void)hipMemsetAsync(c->flags.p, 0, 4096, c->stream);
    *out = c;
    return INNR_OK;
}

void innr_ctx_destroy(innr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)ctx_sync(c);
    for (DevBuf* b : workspace_bufs(c)) b->release();
    if (c->pin) (void)hipHostFree(c->pin);
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

innr_status innr_ctx_set_stream(innr_ctx* c, void* hip_stream) {
    if (!c) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = (hipStream_t)hip_stream;  // NULL = the legacy default stream (what torch uses unless told otherwise)
    c->own_stream = false;
    return INNR_OK;
}

innr_status innr_ctx_set_option(innr_ctx* c, const char* name, long value) {
    if (!c || !name) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    for (const TuneName& n : kTuneNames)
        if (!strcmp(n.name, name)) {
            c->tune.*(n.field) = value;
            return INNR_OK;
        }
    set_error("unknown option '%s'", name);
    return INNR_E_BAD_ARG;
}

innr_status innr_ctx_get_option(innr_ctx* c, const char* name, long* value) {
    if (!c || !name || !value) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    for (const TuneName& n : kTuneNames)
        if (!strcmp(n.name, name)) {
            *value = c->tune.*(n.field);
            return INNR_OK;
        }
    set_error("unknown option '%s'", name);
    return INNR_E_BAD_ARG;
}

innr_status innr_ctx_synchronize(innr_ctx* c) {
    if (!c) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// ---- VerticalBatch -----------------------------------------------------------------------------------
innr_status innr_batch_upload_colmajor(innr_ctx* ctx, const float* data, size_t N, size_t D, innr_batch** out) {
    if (!data && N * D) {
        set_error("data is null");
        return INNR_E_BAD_ARG;
    }
    if (!ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch(ctx, N, D, &b));
    if (N && D) {
        hipError_t e = hipMemcpy2DAsync(b->V, b->ldN * sizeof(float), data, N * sizeof(float), N * sizeof(float), D,
                                        hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("corpus upload failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_upload_rowmajor(innr_ctx* ctx, const float* rows, size_t N, size_t D, innr_batch** out) {
    if (!rows && N * D) {
        set_error("rows is null");
        return INNR_E_BAD_ARG;
    }
    if (!ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch(ctx, N, D, &b));
    if (N && D) {
        // stage row blocks (<= 256 MiB) and transpose them into place on the device
        const size_t max_rows = std::max<size_t>(1, (256ull << 20) / (D * sizeof(float)));
        const size_t blk = std::min(N, max_rows);
        float* stage = nullptr;
        hipError_t e = hipMalloc((void**)&stage, blk * D * sizeof(float));
        if (e != hipSuccess) {
            set_error("hipMalloc(stage) failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_OOM;
        }
        for (size_t i0 = 0; i0 < N && e == hipSuccess; i0 += blk) {
            const size_t n = std::min(blk, N - i0);
            e = copy_in(ctx, stage, rows + i0 * D, n * D * sizeof(float));
            if (e != hipSuccess) break;
            e = transpose_rows_into(ctx, stage, n, D, b->V, b->ldN, i0);
            if (e == hipSuccess) e = ctx_sync(ctx);
        }
        (void)hipFree(stage);
        if (e != hipSuccess) {
            set_error("row-major upload failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_generate(innr_ctx* ctx, size_t N, size_t D, int generator, uint64_t seed, uint64_t row0,
                                innr_batch** out) {
    if (generator != INNR_GEN_EXAMPLE_LCG && generator != INNR_GEN_UNIFORM) {
        set_error("unknown generator %d", generator);
        return INNR_E_BAD_ARG;
    }
    if (!ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch(ctx, N, D, &b));
    if (N && D) {
        if (D > 65535) {
            set_error("innr_batch_generate: D > 65535 unsupported");
            innr_batch_free(b);
            return INNR_E_UNSUPPORTED;
        }
        dim3 grid((unsigned)((b->ldN / 4 + 255) / 256), (unsigned)D);
        if (generator == INNR_GEN_UNIFORM)
            generate_pdx_kernel<1><<<grid, 256, 0, ctx->stream>>>(b->V, b->ldN, (uint32_t)N, (uint32_t)D, seed, row0);
        else
            generate_pdx_kernel<0><<<grid, 256, 0, ctx->stream>>>(b->V, b->ldN, (uint32_t)N, (uint32_t)D, seed, row0);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("generate failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

void innr_batch_free(innr_batch* b) {
    if (!b) return;
    CtxGuard _guard(b->ctx);
    if (b->ctx) {
        (void)hipSetDevice(b->ctx->device);
        (void)ctx_sync(b->ctx);
    }
    free_selection(b);
    if (b->V && !b->is_view) (void)hipFree(b->V);
    if (b->C8 && !b->is_view) (void)hipFree(b->C8);
    if (b->norms) (void)hipFree(b->norms);
    if (b->invn) (void)hipFree(b->invn);
    if (b->sqn) (void)hipFree(b->sqn);
    if (b->max_norm_bits) (void)hipFree(b->max_norm_bits);
    for (const CorpusCopy& cc : b->copy)
        if (cc.p) (void)hipFree(cc.p);
    delete b;
}

#ifdef INNR_TEST_HOOKS  // libinnr_hip_testhooks.so only (make hooks): the product library exports no innrdbg_* symbol
// Test hook: copy out the GEMM engine's last candidate selection (approximate composites) and its error-bound inputs.
innr_status innrdbg_last_selection(innr_batch* b, size_t Q, size_t KP, uint64_t* sel, uint32_t* cnt, float* qnorm,
                                   float* info /* [0]=max_norm */) {
    if (!b) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemcpy(sel, c->sel.p, Q * KP * sizeof(uint64_t), hipMemcpyDeviceToHost));
    INNR_HIP_CHECK(hipMemcpy(cnt, c->sel_cnt.p, Q * sizeof(uint32_t), hipMemcpyDeviceToHost));
    INNR_HIP_CHECK(hipMemcpy(qnorm, c->q_norm.p, Q * sizeof(float), hipMemcpyDeviceToHost));
    info[0] = b->max_norm;
    return INNR_OK;
}

// Test hook (not part of the ABI, not declared in include/innr_hip.h): dense approximate score matrix of the
// GEMM engine, out[q*N + i], to check the MFMA operand/accumulator layout against the oracle.
innr_status innrdbg_gemm_scores(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, float* out) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !queries || !out || D != b->D || Q == 0 || b->N == 0) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const bool cos = metric == INNR_METRIC_COSINE;
    const GemmPlan p = plan_gemm(b, Q, 1, /*waves=*/4);  // (k = 1: lists of 32, the RR 6 that launch_gemm pins for MODE 1)
    INNR_TRY(ensure_norms(b));
    if (cos) INNR_TRY(ensure_invnorms(b));
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_TRY(prep_queries(b, p, c->q_row.as<float>(), Q, cos));
    INNR_TRY(ensure_lists(c, p));
    INNR_TRY(c->scores.ensure(p.Qpad * b->ldN * sizeof(float)));
    if (cos) INNR_TRY((launch_gemm<kGemmCos, 1>(b, p, Q, c->q_kmajor.as<float>(), b->invn, c->misc.as<float>(),
                                            c->scores.as<float>(), b->ldN)));
    else INNR_TRY((launch_gemm<kGemmDot, 1>(b, p, Q, c->q_kmajor.as<float>(), nullptr, nullptr, c->scores.as<float>(), b->ldN)));
    INNR_HIP_CHECK(hipMemcpy2DAsync(out, b->N * sizeof(float), c->scores.p, b->ldN * sizeof(float),
                                    b->N * sizeof(float), Q, hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// Test hook: dense approximate score matrix of the split-bf16 filter (MODE 1), out[q*N + i]: dot, or cosine as the plain dot of
// the normalised limbs -- what the filter compares, to check |approx - exact| <= E. INNR_E_UNSUPPORTED when the
// limb copies do not fit.
innr_status innrdbg_split_scores(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, float* out) {
    if (b && !b->V) return INNR_E_BAD_ARG;
    if (!b || !queries || !out || D != b->D || Q == 0 || b->N == 0 || metric == INNR_METRIC_L2SQ || !metric_ok(metric))
        return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const bool cos = metric == INNR_METRIC_COSINE;
    const GemmPlan p = plan_gemm(b, Q, 1, /*waves=*/8);
    INNR_TRY(ensure_norms(b));
    if (cos) INNR_TRY(ensure_invnorms(b));
    bool ok = false;
    INNR_TRY(ensure_split_corpus(b, metric, &ok));
    if (!ok) return INNR_E_UNSUPPORTED;
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_TRY(prep_queries(b, p, c->q_row.as<float>(), Q, cos));
    INNR_TRY(pack_queries_split(b, p, c->q_row.as<float>(), Q, cos ? c->misc.as<float>() : nullptr));
    INNR_TRY(ensure_lists(c, p));
    INNR_TRY(c->scores.ensure(p.Qpad * b->ldN * sizeof(float)));
    INNR_TRY(launch_gemm_split<1>(b, p, Q, metric, nullptr, nullptr, 0, c->scores.as<float>(), b->ldN));
    INNR_HIP_CHECK(hipMemcpy2DAsync(out, b->N * sizeof(float), c->scores.p, b->ldN * sizeof(float),
                                    b->N * sizeof(float), Q, hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// Test hook: the filter kernel of the last INNR_KNN_MFMA / _BF16 first pass on this batch's context: 0 none yet, 1 the f32 kernel
// (gemm_filter_kernel), 2 the bf16 filter, 3 the split-bf16 filter (LastFilter).
int innrdbg_last_filter(const innr_batch* b) { return b && b->ctx ? b->ctx->last_filter : -1; }

// Test hook: what the screened split filter corrected in the launches since the call's entry cleared the flag words: counts[0] =
// wave tiles (128 rows x 64 queries) with at least one flagged sub-tile, counts[1] = their flagged 32 x 32 sub-tiles.
innr_status innrdbg_split_screen_counts(innr_batch* b, uint32_t* counts) {
    if (!b || !counts) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemcpy(counts, c->flags.as<uint32_t>() + kScreenCountWord, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return INNR_OK;
}
// ... and with how the flagged wave tiles were corrected: counts[2] = (row, query) pairs corrected one by one (the pair path),
// counts[3] = wave tiles with more than kPairCap flagged pairs (the MFMA correction of their flagged sub-tiles)
innr_status innrdbg_split_screen_counts4(innr_batch* b, uint32_t* counts) {
    if (!b || !counts) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemcpy(counts, c->flags.as<uint32_t>() + kScreenCountWord, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return INNR_OK;
}
// the pair path's capacity P (kPairCap) of this build
int innrdbg_split_pair_cap(void) { return kPairCap; }

// Test hook: the split filter's seeder on its own (seed_split, as knn_mfma calls it): the group maxima of the first `rows` corpus
// rows as order keys, maxima[g * Q + j] (g < rows / 32: the best split score of rows 128 (g / 4) + 4 i + g % 4, i < 32), and the
// bounds they seed for the best k, seeds[j]; info[0] = the filter's err_scale (E = err_scale |q| for dot, err_scale for cosine).
// rows: a multiple of 1024 within N. INNR_E_UNSUPPORTED when the limb copies do not fit.
innr_status innrdbg_split_seed(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, size_t k, size_t rows,
                               uint32_t* maxima, uint32_t* seeds, float* info) {
    if (b && !b->V) return INNR_E_BAD_ARG;
    if (!b || !queries || !maxima || !seeds || !info || D != b->D || Q == 0 || k == 0 || rows == 0 || rows % 1024 != 0 || rows > b->N ||
        rows / 32 > kSeedMaxGroups || k > rows / 32 || metric == INNR_METRIC_L2SQ || !metric_ok(metric))
        return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const bool cos = metric == INNR_METRIC_COSINE;
    const GemmPlan p = plan_gemm(b, Q, k, /*waves=*/8);
    INNR_TRY(ensure_norms(b));
    if (cos) INNR_TRY(ensure_invnorms(b));
    bool ok = false;
    INNR_TRY(ensure_split_corpus(b, metric, &ok));
    if (!ok) return INNR_E_UNSUPPORTED;
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_TRY(prep_queries(b, p, c->q_row.as<float>(), Q, cos));
    INNR_TRY(pack_queries_split(b, p, c->q_row.as<float>(), Q, cos ? c->misc.as<float>() : nullptr));
    info[0] = split_filter_scale(b, metric);
    uint32_t* sd = nullptr;
    INNR_TRY(seed_split(b, p, metric, Q, k, info[0], rows, &sd));
    INNR_HIP_CHECK(hipMemcpy2DAsync(maxima, Q * sizeof(uint32_t), c->seed_idx.p, p.Qpad * sizeof(uint32_t), Q * sizeof(uint32_t), rows / 32,
                                    hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(hipMemcpyAsync(seeds, sd, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}
// ... and the prefix rows it served the context's last INNR_KNN_MFMA first pass with (0: the exact seeder, or none)
size_t innrdbg_split_seed_served(const innr_batch* b) { return b && b->ctx ? b->ctx->split_seed_served : 0; }

// Test hook: candidates the progressive re-score (rescore_kernel) has re-scored exactly, summed over the queries of every launch
// since the call's entry cleared the flag words
innr_status innrdbg_rescored(innr_batch* b, uint32_t* count) {
    if (!b || !count) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemcpy(count, c->flags.as<uint32_t>() + kRescoreCountWord, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return INNR_OK;
}

// Test hook: what the screen margin was made of. maxima[0] / [1] = the largest hi / lo limb norm of the batch's split pair of
// `metric` (CorpusCopy::limb_max; -1: not computed), info[0] = max_norm; margins[0 .. n) = the margins of the context's last
// screened call (n = min(cap, its queries); *nq = its queries, 0 when no call has screened yet), qnorm[0 .. n) its query norms.
innr_status innrdbg_split_margins(innr_batch* b, int metric, float* maxima, float* info, float* margins, float* qnorm, size_t cap, size_t* nq) {
    if (!b || !maxima || !info || !nq || metric == INNR_METRIC_L2SQ || !metric_ok(metric)) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));
    maxima[0] = b->copy[bf16_kind(metric)].limb_max;
    maxima[1] = b->copy[bf16_kind(metric, true)].limb_max;
    info[0] = b->max_norm;
    const bool kept = c->kmargin.p && c->kmargin.bytes >= (c->screen_qpad + c->screen_q) * sizeof(float) && c->q_norm.p &&
                      c->q_norm.bytes >= c->screen_q * sizeof(float);  // (a trimmed workspace holds none)
    *nq = kept ? c->screen_q : 0;
    const size_t n = std::min(cap, *nq);
    if (n && margins) INNR_HIP_CHECK(hipMemcpy(margins, c->kmargin.as<float>() + c->screen_qpad, n * sizeof(float), hipMemcpyDeviceToHost));
    if (n && qnorm) INNR_HIP_CHECK(hipMemcpy(qnorm, c->q_norm.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return INNR_OK;
}

// Test hook: the pair correction's arithmetic and addressing. out[i] = qh.vl + ql.vh of corpus row pairs[2 i] and query pairs[2 i + 1]
// (i < n), from the batch's limb copies and the queries packed as knn_mfma packs them (cosine: limbs of the normalised values), by
// split_pair_delta -- the function the screened kernel corrects its flagged pairs with. INNR_E_UNSUPPORTED when the limb copies do
// not fit.
innr_status innrdbg_split_pair_scores(innr_batch* b, const float* queries, size_t Q, int metric, const uint32_t* pairs, size_t n, float* out) {
    if (b && !b->V) return INNR_E_BAD_ARG;
    if (!b || !queries || !pairs || !out || Q == 0 || n == 0 || n > (1u << 20) || b->N == 0 || metric == INNR_METRIC_L2SQ || !metric_ok(metric))
        return INNR_E_BAD_ARG;
    for (size_t i = 0; i < n; ++i)
        if (pairs[2 * i] >= b->N || pairs[2 * i + 1] >= Q) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const bool cos = metric == INNR_METRIC_COSINE;
    const size_t D = b->D;
    const GemmPlan p = plan_gemm(b, Q, 1, /*waves=*/8);
    if (p.Qpad > kPairMaxQpad) return INNR_E_BAD_ARG;
    INNR_TRY(ensure_norms(b));
    if (cos) INNR_TRY(ensure_invnorms(b));
    bool ok = false;
    INNR_TRY(ensure_split_corpus(b, metric, &ok));
    if (!ok) return INNR_E_UNSUPPORTED;
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_TRY(prep_queries(b, p, c->q_row.as<float>(), Q, cos));
    INNR_TRY(pack_queries_split(b, p, c->q_row.as<float>(), Q, cos ? c->misc.as<float>() : nullptr));
    INNR_TRY(c->scores.ensure(n * 3 * sizeof(uint32_t)));
    uint32_t* d_pairs = c->scores.as<uint32_t>();
    float* d_out = c->scores.as<float>() + 2 * n;
    INNR_HIP_CHECK(hipMemcpyAsync(d_pairs, pairs, n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const CorpusCopy &hi = b->copy[bf16_kind(metric)], &lo = b->copy[bf16_kind(metric, true)];
    split_pair_scores_kernel<<<(unsigned)((n + kPairNP - 1) / kPairNP), 64, 0, c->stream>>>(hi.p, lo.p, c->q_bf16.as<char>(), hi.nk, p.Qpad, d_pairs, (uint32_t)n, d_out);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_HIP_CHECK(hipMemcpyAsync(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// Test hook: how many selections innr_batch_knn_filtered_multi has built for this batch (its cache misses)
uint32_t innrdbg_filter_selection_builds(const innr_batch* b) { return b ? b->fsel_builds : 0u; }

// Test hook: the context's launch record (innr_ctx::launch_log), oldest first: up to `cap` entries of 16 bytes (LaunchRec) into
// `out`, the number written returned; *total = launches recorded since the last reset (beyond kLaunchLogCap the oldest are gone).
extern "C" size_t innrdbg_launch_log(innr_ctx* c, void* out, size_t cap, uint64_t* total) {
    if (!c) return 0;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    static_assert(sizeof(LaunchRec) == 16, "the hook's reader decodes 16-byte entries");
    if (total) *total = c->launch_total;
    const uint64_t have = std::min<uint64_t>(c->launch_total, kLaunchLogCap);
    const size_t n = out ? (size_t)std::min<uint64_t>(have, cap) : 0;
    for (size_t i = 0; i < n; ++i)  // the last n entries
        static_cast<LaunchRec*>(out)[i] = c->launch_log[(c->launch_total - n + i) % kLaunchLogCap];
    return n;
}
extern "C" void innrdbg_launch_log_reset(innr_ctx* c) {
    if (!c) return;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    c->launch_total = 0;
}

// Test hook: the context's record of exact-scan launches (innr_ctx::scan_log), oldest first: up to `cap` entries of 20 bytes
// (ScanRec) into `out`, the number written returned; *total = scans recorded since the last reset (beyond kScanLogCap the oldest
// are gone).
extern "C" size_t innrdbg_scan_log(innr_ctx* c, void* out, size_t cap, uint64_t* total) {
    if (!c) return 0;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    static_assert(sizeof(ScanRec) == 20, "the hook's reader decodes 20-byte entries");
    if (total) *total = c->scan_total;
    const uint64_t have = std::min<uint64_t>(c->scan_total, kScanLogCap);
    const size_t n = out ? (size_t)std::min<uint64_t>(have, cap) : 0;
    for (size_t i = 0; i < n; ++i)  // the last n entries
        static_cast<ScanRec*>(out)[i] = c->scan_log[(c->scan_total - n + i) % kScanLogCap];
    return n;
}
extern "C" void innrdbg_scan_log_reset(innr_ctx* c) {
    if (!c) return;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    c->scan_total = 0;
}

// Test hook: the context's workspace overwritten with one byte value, so that the next call meets residue no earlier call of a
// test would have left (tests/test_gpu_workspace_residue.py): every buffer of workspace_bufs() but `flags` (the documented
// exception: the kernels' error words live there between the calls' own memsets) over its full size, and the whole pinned
// staging area (nothing is pending after the synchronise). *bytes_filled = the device bytes written (innr_ctx_memory less flags).
extern "C" innr_status innrdbg_workspace_fill(innr_ctx* c, int byte, uint64_t* bytes_filled) {
    if (!c) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));
    uint64_t sum = 0;
    for (DevBuf* buf : workspace_bufs(c)) {
        if (buf == &c->flags || !buf->p || !buf->bytes) continue;
        INNR_HIP_CHECK(hipMemsetAsync(buf->p, byte, buf->bytes, c->stream));
        sum += buf->bytes;
    }
    if (c->pin) memset(c->pin, byte, kPinIn + kPinOut);
    INNR_HIP_CHECK(ctx_sync(c));
    if (bytes_filled) *bytes_filled = sum;
    return INNR_OK;
}
// ... and the size of every workspace buffer, in the order of workspace_bufs(): up to `cap` sizes into `sizes`, the number of
// buffers returned; innrdbg_workspace_names() = their names in the same order, comma-separated
extern "C" size_t innrdbg_workspace_sizes(innr_ctx* c, uint64_t* sizes, size_t cap) {
    if (!c) return 0;
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    const std::vector<DevBuf*> bufs = workspace_bufs(c);
    for (size_t i = 0; i < bufs.size() && i < cap && sizes; ++i) sizes[i] = bufs[i]->bytes;
    return bufs.size();
}
extern "C" const char* innrdbg_workspace_names(void) {
    return "gthr,sel_tmp0,sel_tmp1,selcnt_tmp0,selcnt_tmp1,q_row,q_kmajor,q_norm,lists,counts,sel,sel_cnt,scores,tmp_norms,flags,"
           "out_idx,out_score,misc,seed_idx,seed_score,q_one,sort_keys,sort_tmp,q_bf16,q_pad,q_hat,redo0.q,redo0.idx,redo0.sc,"
           "redo0.map,redo0.qn,redo1.q,redo1.idx,redo1.sc,redo1.map,redo1.qn,kmargin,i8s_prog,cmpl.q,cmpl.idx,cmpl.sc,cmpl.map,"
           "cmpl.qn,flt_in,flt_mask,flt_scan,rs_cnt,rs_bits,rs_tot,rs_thr,rs_off,adp_scan,adp_list,rows_q,rows_stage,rows_io,"
           "rows_flag,rows_bits,rows_map";
}

// Test hook: sort_full.hip's full_topk_keys on caller-given composites -- the radix select, the gather and the bitonic network with
// nothing in front of them. host_keys[0..n) -> host_sorted[0..min(k, n)), best (largest) first. Buffers as knn_full_sort lays them
// out: c->sort_keys = [n keys][full_topk_out_capacity(min(k, n)) sorted], c->sort_tmp = the selection state.
innr_status innrdbg_full_topk_keys(innr_ctx* c, const uint64_t* host_keys, size_t n, size_t k, uint64_t* host_sorted) {
    if (!c || !host_keys || !host_sorted) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    const size_t kout = std::min(k, n);
    if (kout == 0) return INNR_OK;
    size_t tmp_bytes = 0;
    INNR_HIP_CHECK(full_sort_scratch_bytes(n, &tmp_bytes));
    INNR_TRY(c->sort_keys.ensure((n + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
    INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    INNR_HIP_CHECK(hipMemcpyAsync(keys, host_keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    INNR_HIP_CHECK(full_topk_keys(keys, n, kout, keys + n, c->sort_tmp.p, c->stream));
    INNR_HIP_CHECK(hipMemcpyAsync(host_sorted, keys + n, kout * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// Test hook: segmented_topk_keys on caller-given composites, host_keys[nseg][len] -> host_sorted[nseg][min(k, len)], every segment
// best first. Buffers as innr_batch_rerank_dev lays them out: c->sort_keys = [nseg * len keys][nseg * len sorted][tmp of
// full_topk_out_capacity(min(k, len))].
innr_status innrdbg_segmented_topk_keys(innr_ctx* c, const uint64_t* host_keys, size_t nseg, size_t len, size_t k,
                                        uint64_t* host_sorted) {
    if (!c || !host_keys || !host_sorted) return INNR_E_BAD_ARG;
    INNR_ENTER(c);
    const size_t kout = std::min(k, len);
    if (kout == 0 || nseg == 0) return INNR_OK;
    size_t tmp_bytes = 0;
    INNR_HIP_CHECK(segmented_sort_scratch_bytes(nseg, len, &tmp_bytes));
    INNR_TRY(c->sort_keys.ensure((2 * nseg * len + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
    INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    INNR_HIP_CHECK(hipMemcpyAsync(keys, host_keys, nseg * len * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    INNR_HIP_CHECK(segmented_topk_keys(keys, keys + nseg * len, nseg, len, kout, keys + 2 * nseg * len, c->sort_tmp.p, c->stream));
    INNR_HIP_CHECK(hipMemcpy2DAsync(host_sorted, kout * sizeof(uint64_t), keys + nseg * len, len * sizeof(uint64_t),
                                    kout * sizeof(uint64_t), nseg, hipMemcpyDeviceToHost, c->stream));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

#endif  // INNR_TEST_HOOKS

// Second stage of the two-stage pipeline the reference describes (scalar.rs:366-368: batch_knn_u8 first pass, then an
// exact re-rank on the full-precision vectors): exact scores of caller-given candidates in the reference's arithmetic
// order, ordered like the kNN functions (score order, then index ascending), best k per query.
innr_status innr_batch_rerank_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D,
                                  const uint64_t* d_cand, size_t kc, size_t k, uint64_t* d_out_idx, float* d_out_score,
                                  size_t* out_k) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !out_k || !metric_ok(metric)) return INNR_E_BAD_ARG;
    if (D != b->D) {
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0 || kc == 0) return INNR_OK;
    if (!d_queries || !d_cand || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    const size_t kout = std::min(k, kc);
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    uint32_t* bad = c->flags.as<uint32_t>() + 65;  // set by the kernels for a candidate outside the batch
    const auto finish = [&]() -> innr_status {
        uint32_t hbad = 0;
        INNR_HIP_CHECK(copy_out(c, &hbad, bad, 4));
        INNR_HIP_CHECK(ctx_sync(c));
        if (hbad) {
            set_error("rerank: a candidate index lies outside this batch's range [%llu, %llu)",
                      (unsigned long long)b->index_base, (unsigned long long)(b->index_base + b->N));
            return INNR_E_BAD_ARG;
        }
        *out_k = kout;
        return INNR_OK;
    };
    if (kc > 256) {
        // More candidates per query than a candidate list holds: exact scores of all of them (one thread per candidate,
        // the reference's arithmetic order), then the best k of every query's kc composites, best first (radix select + sort per
        // query, sort_full.hip) -- the reference's "score, stable sort, truncate" (scalar.rs:366-368 on top of batch.rs:754-763).
        if ((Q * kc + 255) / 256 > 0x7fffffffull) {
            set_error("rerank: Q * candidates = %zu is beyond one launch", Q * kc);
            return INNR_E_UNSUPPORTED;
        }
        size_t tmp_bytes = 0;
        INNR_HIP_CHECK(segmented_sort_scratch_bytes(Q, kc, &tmp_bytes));
        INNR_TRY(c->sort_keys.ensure((2 * Q * kc + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
        INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        INNR_TRY(c->q_norm.ensure(Q * sizeof(float)));
        INNR_TRY(c->misc.ensure((Q + 1) * sizeof(uint32_t) + 64));
        INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
        if (metric == INNR_METRIC_COSINE) INNR_TRY(ensure_norms(b));
        query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(d_queries, (uint32_t)Q, (uint32_t)D, D,
                                                                           c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        uint64_t* keys = c->sort_keys.as<uint64_t>();
        const unsigned nb = (unsigned)((Q * kc + 255) / 256);
        with_space(metric_space(metric), [&](auto met) {
            rerank_scores_kernel<decltype(met)::value><<<nb, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)D, d_queries,
                                                                                  b->norms, c->q_norm.as<float>(), d_cand, (uint32_t)Q,
                                                                                  (uint32_t)kc, b->index_base, keys, bad);
        });
        INNR_HIP_CHECK(hipGetLastError());
        INNR_HIP_CHECK(segmented_topk_keys(keys, keys + Q * kc, Q, kc, kout, keys + 2 * Q * kc, c->sort_tmp.p, c->stream));
        INNR_TRY(emit_results(c, keys + Q * kc, kc, Q, kout, metric == INNR_METRIC_L2SQ, b->index_base, d_out_idx, d_out_score));
        return finish();
    }
    const uint32_t KP = pick_kp(kc, 0);  // 32..256
    INNR_TRY(c->sel.ensure(Q * KP * sizeof(uint64_t)));
    INNR_TRY(c->sel_cnt.ensure(Q * sizeof(uint32_t)));
    INNR_TRY(c->q_norm.ensure(Q * sizeof(float)));
    INNR_TRY(c->misc.ensure(Q * sizeof(uint32_t) + 64));
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    if (metric == INNR_METRIC_COSINE) INNR_TRY(ensure_norms(b));
    query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(d_queries, (uint32_t)Q, (uint32_t)D, D,
                                                                       c->q_norm.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    rerank_prepare_kernel<<<(unsigned)((Q * KP + 255) / 256), 256, 0, c->stream>>>(d_cand, (uint32_t)Q, (uint32_t)kc, KP,
                                                                                  (uint32_t)b->N, b->index_base,
                                                                                  c->sel.as<uint64_t>(),
                                                                                  c->sel_cnt.as<uint32_t>(), bad);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t* unused = c->misc.as<uint32_t>();  // the proof flags of the kNN path: no proof to make here (cnt < KP or moot)
    INNR_TRY(launch_rescore(b, metric_space(metric), d_queries, Q, c->q_norm.as<float>(), KP, kout, 0.0f, d_out_idx, d_out_score, unused,
                            nullptr, false, nullptr));
    return finish();
}

innr_status innr_batch_rerank(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, const uint64_t* cand,
                              size_t kc, size_t k, uint64_t* out_idx, float* out_score, size_t* out_k) {
    if (!b || !out_k) return INNR_E_BAD_ARG;
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0 || kc == 0) return (b->V && D != b->D) ? (set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D), INNR_E_DIM_MISMATCH) : INNR_OK;
    if (!queries || !cand || !out_idx || !out_score) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const size_t kout = std::min(k, kc);
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_TRY(c->out_idx.ensure(Q * (kout + kc) * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(Q * kout * sizeof(float)));
    uint64_t* d_cand = c->out_idx.as<uint64_t>() + Q * kout;
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, d_cand, cand, Q * kc * sizeof(uint64_t)));
    INNR_TRY(innr_batch_rerank_dev(b, metric, c->q_row.as<float>(), Q, D, d_cand, kc, k, c->out_idx.as<uint64_t>(),
                                   c->out_score.as<float>(), out_k));
    INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, Q * kout * sizeof(uint64_t)));
    INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, Q * kout * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// which engine INNR_KNN_AUTO resolves to for a Q-query call on this batch (introspection, cf. backend.rs:40-67)
// gemm_filter_kernel addresses its operands as a 64-bit scalar base + a 32-bit per-lane byte offset (up to 7 corpus
// rows / one query row): corpora or query batches beyond this take the exact engine (same results, by construction)
static bool gemm_addressable(const innr_batch* b, size_t Q) {
    return b->gemm_ok && b->ldN < ((size_t)1 << 29) && Q < ((size_t)1 << 28);
}

int innr_batch_auto_engine(const innr_batch* b, size_t Q) {
    if (!b) return INNR_KNN_EXACT;
    // from 9 queries on, the GEMM engine's 64-query tile (9-10 ms at 10M x 768) beats two passes of the exact engine (6.6 + 5.5 ms);
    // up to 8 queries one exact pass is faster (profiles/r02_midq_10Mx768.txt)
    return (Q >= 9 && b->N >= 65536 && gemm_addressable(b, Q)) ? INNR_KNN_MFMA : INNR_KNN_EXACT;
}

size_t innr_batch_num_vectors(const innr_batch* b) { return b ? b->N : 0; }
size_t innr_batch_dimension(const innr_batch* b) { return b ? b->D : 0; }

innr_status innr_batch_download_colmajor(innr_batch* b, float* out) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || (!out && b->N * b->D)) return INNR_E_BAD_ARG;
    if (b->N == 0 || b->D == 0) return INNR_OK;
    INNR_ENTER(b->ctx);
    INNR_HIP_CHECK(hipMemcpy2DAsync(out, b->N * sizeof(float), b->V, b->ldN * sizeof(float), b->N * sizeof(float),
                                    b->D, hipMemcpyDeviceToHost, b->ctx->stream));
    INNR_HIP_CHECK(ctx_sync(b->ctx));
    return INNR_OK;
}

innr_status innr_batch_set_index_base(innr_batch* b, uint64_t base) {
    if (!b) return INNR_E_BAD_ARG;
    b->index_base = base;
    return INNR_OK;
}

// ---- scans ---------------------------------------------------------------------------------------------
innr_status innr_batch_norms(innr_batch* b, float* out) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || (!out && b->N)) return INNR_E_BAD_ARG;
    if (b->N == 0) return INNR_OK;
    INNR_ENTER(b->ctx);
    INNR_TRY(ensure_norms(b));
    INNR_HIP_CHECK(copy_out(b->ctx, out, b->norms, b->N * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(b->ctx));
    return INNR_OK;
}

innr_status innr_batch_scores(innr_batch* b, int metric, const float* q, size_t D, const float* norms, float* out) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !metric_ok(metric)) {
        set_error("bad batch/metric");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // assert_eq!(query.len(), batch.dimension) batch.rs:251,285
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    if (b->N == 0) return INNR_OK;
    if (!out || (!q && D)) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const size_t ldq = round_up(D ? D : 1, 4);
    INNR_TRY(c->q_row.ensure(ldq * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(sizeof(float)));
    INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, q, D * sizeof(float)));
    const float* dn = nullptr;
    if (metric == INNR_METRIC_COSINE) {
        if (norms) {  // the reference signature passes the caller's norms (batch.rs:690)
            INNR_TRY(c->tmp_norms.ensure(b->ldN * sizeof(float)));
            INNR_HIP_CHECK(hipMemsetAsync(c->tmp_norms.p, 0, b->ldN * sizeof(float), c->stream));
            INNR_HIP_CHECK(copy_in(c, c->tmp_norms.p, norms, b->N * sizeof(float)));
            dn = c->tmp_norms.as<float>();
        } else {
            INNR_TRY(ensure_norms(b));
            dn = b->norms;
        }
        query_norms_kernel<<<1, 64, 0, c->stream>>>(c->q_row.as<float>(), 1, (uint32_t)D, ldq, c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
    }
    const size_t nchunks = b->ldN / kScanChunk;
    const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
    const float* dq = c->q_row.as<float>();
    float* ds = c->scores.as<float>();
    switch (metric) {
        case INNR_METRIC_DOT:
            scan_scores_kernel<1, false, false><<<blocks, kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)D, dq, ldq, nullptr, nullptr, ds, b->ldN);
            break;
        case INNR_METRIC_L2SQ:
            scan_scores_kernel<1, true, false><<<blocks, kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)D, dq, ldq, nullptr, nullptr, ds, b->ldN);
            break;
        default:
            scan_scores_kernel<1, false, true><<<blocks, kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)D, dq, ldq, dn, c->q_norm.as<float>(), ds, b->ldN);
            break;
    }
    INNR_HIP_CHECK(hipGetLastError());
    INNR_HIP_CHECK(copy_out(c, out, ds, b->N * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

}  // extern "C"


// k > INNR_MAX_K: more results than a candidate list holds. The reference's own algorithm, on the device: all N
// scores of one query (scan_scores_kernel: the reference-order arithmetic the exact engine uses), then the part of the full
// sort of (score, index) composites that the truncation keeps: radix select of the k-th + sort of the best k (sort_full.hip;
// batch.rs:754-763, 790-799, scalar.rs:383-392; for batch_knn's TopK, batch.rs:398-409, the same k smallest in the same order up
// to ties at equal distances). One query at a time: the path is for the rare "give me everything, ranked" call.
// metric < 0: u8 codes (aux = per-query sum(q)); cosine: aux = per-query norms.
// mask (nullable, [ldN] bytes): only the vectors with mask[i] != 0 take part (they must number kout or more; innr_batch_knn_filtered_multi).
static innr_status knn_full_sort(innr_batch* b, int metric, const float* dQ, size_t D, const float* aux, size_t Q,
                                 size_t kout, uint64_t* d_out_idx, float* d_out_score, const uint8_t* mask = nullptr) {
    innr_ctx* c = b->ctx;
    const size_t ldq = round_up(D ? D : 1, 4), N = b->N;
    size_t tmp_bytes = 0;
    INNR_HIP_CHECK(full_sort_scratch_bytes(N, &tmp_bytes));
    INNR_TRY(c->q_one.ensure(ldq * sizeof(float)));
    INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
    INNR_TRY(c->sort_keys.ensure((N + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
    INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
    INNR_HIP_CHECK(hipMemsetAsync(c->q_one.p, 0, ldq * sizeof(float), c->stream));
    if (metric == INNR_METRIC_COSINE) INNR_TRY(ensure_norms(b));
    const bool smaller = metric == INNR_METRIC_L2SQ;
    const float* dq = c->q_one.as<float>();
    float* ds = c->scores.as<float>();
    uint64_t* keys = c->sort_keys.as<uint64_t>();
    for (size_t q = 0; q < Q; ++q) {
        if (D) INNR_HIP_CHECK(hipMemcpyAsync(c->q_one.p, dQ + q * D, D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        if (metric < 0) {
            const size_t nchunks = b->ldN / kU8Chunk;
            const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
            scan_u8_scores_kernel<1><<<blocks, 256, 0, c->stream>>>(b->C8, b->ldN, (uint32_t)D, dq, ldq, aux + q,
                                                                    b->alpha / 255.0f, b->offset, ds, b->ldN);
        } else {
            const size_t nchunks = b->ldN / kScanChunk;
            const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
            if (metric == INNR_METRIC_DOT)
                scan_scores_kernel<1, false, false><<<blocks, kScanThreads, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, dq, ldq,
                                                                                           nullptr, nullptr, ds, b->ldN);
            else if (metric == INNR_METRIC_L2SQ)
                scan_scores_kernel<1, true, false><<<blocks, kScanThreads, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, dq, ldq,
                                                                                          nullptr, nullptr, ds, b->ldN);
            else
                scan_scores_kernel<1, false, true><<<blocks, kScanThreads, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, dq, ldq,
                                                                                          b->norms, aux + q, ds, b->ldN);
        }
        INNR_HIP_CHECK(hipGetLastError());
        INNR_HIP_CHECK(full_sort_scores(ds, N, smaller, keys, keys + N, c->sort_tmp.p, tmp_bytes, c->stream, mask, kout));
        INNR_TRY(emit_results(c, keys + N, 0, 1, kout, smaller, b->index_base, d_out_idx + q * kout, d_out_score + q * kout));
    }
    return INNR_OK;
}

namespace innr {
innr_status l2_prefix_scores(innr_batch* b, const float* d_query, size_t W, float* out) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kScanChunk;
    const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
    scan_scores_kernel<1, true, false><<<blocks, kScanThreads, 0, c->stream>>>(b->V, b->ldN, (uint32_t)W, d_query, W, nullptr, nullptr,
                                                                              out, b->ldN);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}
innr_status exclusive_scan_u32(innr_ctx* c, const uint32_t* counts, uint32_t n, uint32_t* offsets, uint32_t* total) {
    exclusive_scan_kernel<<<1, 1024, 0, c->stream>>>(counts, n, offsets, total);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}
}  // namespace innr

// the int8 filter in front of an f32 corpus (defined with the int8 engine further down)
static bool f32_i8_eligible(const innr_batch* b, int metric, size_t Q, size_t kout);
static size_t f32_i8_copy_bytes(const innr_batch* b, int metric);

// The end of a kNN call (ev[0] was recorded at its start): the device error flag, *out_k and the stats
static innr_status finish_knn(innr_ctx* c, int engine, size_t kout, uint32_t nfallback, uint32_t kept, float gemm_ms, size_t* out_k,
                              innr_knn_stats* stats) {
    INNR_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
    INNR_TRY(check_errflag(c));
    *out_k = kout;
    if (stats) {
        stats->engine = engine;
        stats->queries_fallback = nfallback;
        stats->candidates_kept = kept;
        stats->gemm_ms = gemm_ms;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) stats->total_ms = ms;
    }
    if (engine == INNR_KNN_MFMA_I8 && i8h_probe_skips_visits()) {
        set_error("this library is a timing build (-DINNR_I8H_PROBE): the int8 filter kernel skipped its visits, the call's results are not valid");
        return INNR_E_UNSUPPORTED;
    }
    return INNR_OK;
}

extern "C" {

// ---- kNN -----------------------------------------------------------------------------------------------
innr_status innr_batch_knn_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D, size_t k,
                               int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k,
                               innr_knn_stats* stats) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !metric_ok(metric) || !out_k) {
        set_error("bad batch/metric/out_k");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // batch.rs:386,743,778
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0) return INNR_OK;  // batch.rs:388-393, 745-750
    const size_t kout = std::min(k, b->N);              // batch.rs:395, 752
    if (!d_queries || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    // AUTO: the GEMM engine pays off once there are enough queries to fill MFMA tiles AND enough corpus per slice
    // for its threshold filter to bite (with a handful of tiles per slice nearly every score is appended)
    if (engine == INNR_KNN_AUTO) {
        engine = innr_batch_auto_engine(b, Q);
        // A low-precision FILTER (identical results) when one applies and its K-packed corpus copy exists already or fits next to
        // everything else with room to spare (copies are kept for the batch's lifetime). Measured at C2 (profiles/r03_midq_*):
        // the int8 filter (dot / cosine; N*D bytes, a quarter of the f32 corpus to stream) answers 1 .. 128 queries in 3.3 - 4.3 ms
        // where the exact engine takes 5.2 ms for ONE corpus pass and the f32 GEMM engine 9 - 17 ms: it is the choice for every
        // batch size once its copy exists, and worth building from 4 queries on; the bf16 filter (squared L2, or when the int8
        // one is ruled out; N*D*2 bytes) takes 6.0 - 6.7 ms there: from 9 queries on, where the alternative is the f32 GEMM.
        const bool big_enough = b->N >= 65536 && gemm_addressable(b, Q) && b->gemm_ok;
        if (big_enough && kout <= INNR_MAX_K && !b->ctx->tune.no_auto_bf16) {
            const CorpusCopy &i8c = b->copy[i8_kind(metric)], &bfc = b->copy[bf16_kind(metric)];
            size_t free_b = 0, total_b = 0;
            const bool have_mem = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
            // (a corpus marked weak -- its proofs failed on the int8 filter -- is looked at again every 64th call: data change)
            const bool weak = i8c.weak && (++b->i8_weak_skips % 64u) != 0;
            // (a caller that keeps sending one to three queries -- the reference's own one-query signature in a loop -- gets the copy
            //  with its fourth call: 1.6 ms per query from then on instead of 5.3)
            const bool worth = Q >= 4 || (!i8c.p && ++b->auto_small_calls >= 4);
            if (f32_i8_eligible(b, metric, Q, kout) && !b->ctx->tune.no_auto_i8 && !weak &&
                (i8c.p || (worth && have_mem && copy_fits(free_b, f32_i8_copy_bytes(b, metric)) &&
                           budget_admits(b, f32_i8_copy_bytes(b, metric)))))
                engine = INNR_KNN_MFMA_I8;
            else if (Q >= 9 && (bfc.p || (have_mem && copy_fits(free_b, bf16_copy_bytes(b, bf16_kind(metric))) &&
                                          budget_admits(b, bf16_copy_bytes(b, bf16_kind(metric))))))
                engine = INNR_KNN_MFMA_BF16;
        }
    }
    if (engine == INNR_KNN_MFMA_I8 && !f32_i8_eligible(b, metric, Q, kout))  // k > 240, a view, a u8 batch ...
        engine = INNR_KNN_MFMA;
    // an explicit low-precision request whose copy is missing and beyond the copy budget (the squared-L2 int8 copy: by its upper
    // bound): the f32 engine serves the call, as the header promises for every call these filters do not take
    if (engine == INNR_KNN_MFMA_I8 && !b->copy[i8_kind(metric)].p && !budget_admits(b, f32_i8_copy_bytes(b, metric)))
        engine = INNR_KNN_MFMA;
    if (engine == INNR_KNN_MFMA_BF16 && !b->copy[bf16_kind(metric)].p && !budget_admits(b, bf16_copy_bytes(b, bf16_kind(metric))))
        engine = INNR_KNN_MFMA;
    if ((engine == INNR_KNN_MFMA || engine == INNR_KNN_MFMA_BF16 || engine == INNR_KNN_MFMA_I8) && !gemm_addressable(b, Q)) engine = INNR_KNN_EXACT;
    if (kout > INNR_MAX_K) engine = INNR_KNN_EXACT;  // the full-sort path below: exact by construction
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    const float* dQn = nullptr;
    if (metric == INNR_METRIC_COSINE) {
        INNR_TRY(ensure_norms(b));
        INNR_TRY(c->q_norm.ensure(Q * sizeof(float)));
        query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(d_queries, (uint32_t)Q, (uint32_t)D, D,
                                                                           c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        dQn = c->q_norm.as<float>();
    }
    uint32_t nfallback = 0, kept = 0;
    float gemm_ms = 0.0f;
    if (engine == INNR_KNN_MFMA_I8) {
        bool served = false;
        INNR_TRY(knn_f32_i8(b, metric, d_queries, Q, kout, d_out_idx, d_out_score, &nfallback, &kept, &gemm_ms, &served));
        if (!served) engine = INNR_KNN_MFMA;  // a constant or non-finite corpus: nothing to quantise against
    }
    if (engine == INNR_KNN_MFMA_I8) {
    } else if (engine == INNR_KNN_MFMA || engine == INNR_KNN_MFMA_BF16) {
        INNR_TRY(knn_mfma(b, metric, d_queries, Q, kout, dQn, d_out_idx, d_out_score, &nfallback, &kept, &gemm_ms,
                          engine == INNR_KNN_MFMA_BF16));
        if (gemm_ms < 0.0f) {  // not a dot-kind call / k too large / degenerate norms: the f32 engine served it
            gemm_ms = -gemm_ms;
            engine = INNR_KNN_MFMA;
        }
    } else if (kout > INNR_MAX_K) {
        INNR_TRY(knn_full_sort(b, metric, d_queries, D, dQn, Q, kout, d_out_idx, d_out_score));
        kept = (uint32_t)b->N;
    } else {
        INNR_TRY(knn_exact_range(b, metric, d_queries, D, dQn, 0, Q, kout, d_out_idx, d_out_score));
        kept = pick_kp(kout, 0);
    }
    return finish_knn(c, engine, kout, nfallback, kept, gemm_ms, out_k, stats);
}

innr_status innr_batch_knn(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, size_t k, int engine,
                           uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !out_k) return INNR_E_BAD_ARG;
    if (D != b->D) {
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0) return INNR_OK;
    if (!queries && D) return INNR_E_BAD_ARG;
    return knn_from_host(b->ctx, queries, Q, D, std::min(k, b->N), out_idx, out_score, out_k, [&](const float* dQ, uint64_t* di, float* ds) {
        return innr_batch_knn_dev(b, metric, dQ, Q, D, k, engine, di, ds, out_k, stats);
    });
}

}  // extern "C"  (the u8 section has templates and static helpers; its entry points get C linkage from the header)

// ---- scalar-quantised corpus (scalar.rs) -----------------------------------------------------------------
innr_status innr::alloc_batch_u8(innr_ctx* ctx, size_t N, size_t D, float alpha, float offset, innr_batch** out) {
    if (!ctx || !out) return INNR_E_BAD_ARG;
    if (N >= kMaxBatchNU8 || D > 65535) {
        set_error("u8 corpus shard too large (N=%zu, D=%zu)", N, D);
        return INNR_E_UNSUPPORTED;
    }
    INNR_ENTER(ctx);
    innr_batch* b = new (std::nothrow) innr_batch();
    if (!b) return INNR_E_OOM;
    b->ctx = ctx;
    b->N = N;
    b->D = D;
    b->ldN = round_up(N ? N : 1, 1024);
    b->Dpad = round_up(D ? D : 1, 32);
    b->alpha = alpha;
    b->offset = offset;
    const size_t bytes = b->ldN * b->Dpad;
    hipError_t e = hipMalloc((void**)&b->C8, bytes);
    if (e == hipSuccess) b->corpus_bytes = bytes;
    b->copy_budget = budget_from_option(ctx);
    if (e == hipSuccess) e = hipMemsetAsync(b->C8, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
        set_error("u8 corpus allocation (%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        innr_batch_free(b);
        return INNR_E_OOM;
    }
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_upload_u8(innr_ctx* ctx, const uint8_t* codes, size_t N, size_t D, float alpha, float offset,
                                 innr_batch** out) {
    if ((!codes && N * D) || !ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch_u8(ctx, N, D, alpha, offset, &b));
    if (N && D) {
        const size_t blk = std::min(N, std::max<size_t>(1, (256ull << 20) / D));
        uint8_t* stage = nullptr;
        hipError_t e = hipMalloc((void**)&stage, blk * D);
        for (size_t i0 = 0; i0 < N && e == hipSuccess; i0 += blk) {
            const size_t n = std::min(blk, N - i0);
            e = copy_in(ctx, stage, codes + i0 * D, n * D);
            if (e != hipSuccess) break;
            dim3 grid((unsigned)((n + 31) / 32), (unsigned)((D + 31) / 32));
            transpose_rows_u8_kernel<<<grid, 256, 0, ctx->stream>>>(stage, (uint32_t)n, (uint32_t)D, b->C8, b->ldN, i0);
            e = hipGetLastError();
            if (e == hipSuccess) e = ctx_sync(ctx);
        }
        if (stage) (void)hipFree(stage);
        if (e != hipSuccess) {
            set_error("u8 upload failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_generate_u8(innr_ctx* ctx, size_t N, size_t D, uint64_t seed, uint64_t row0, float alpha,
                                   float offset, innr_batch** out) {
    if (!ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch_u8(ctx, N, D, alpha, offset, &b));
    if (N && D) {
        dim3 grid((unsigned)((b->ldN / 16 + 255) / 256), (unsigned)D);
        generate_u8_pdx_kernel<<<grid, 256, 0, ctx->stream>>>(b->C8, b->ldN, (uint32_t)N, (uint32_t)D, seed, row0, offset,
                                                              255.0f / alpha);  // scalar.rs:213 inv_alpha
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("u8 generate failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

// corpus ingest on the device: quantise a resident f32 batch into a u8 code batch (scalar.rs:212-225
// per value), and QuantizationParams::fit's global range (scalar.rs:68-87) without bringing the corpus to the host
innr_status innr_batch_quantize_u8(innr_batch* src, float alpha, float offset, innr_batch** out) {
    if (!src || !src->V || !out) {
        set_error("innr_batch_quantize_u8 needs an f32 batch");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* ctx = src->ctx;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch_u8(ctx, src->N, src->D, alpha, offset, &b));
    if (src->N && src->D) {
        dim3 grid((unsigned)((b->ldN / 16 + 255) / 256), (unsigned)src->D);
        quantize_pdx_kernel<<<grid, 256, 0, ctx->stream>>>(src->V, src->ldN, (uint32_t)src->N, (uint32_t)src->D, offset,
                                                           255.0f / alpha, b->C8, b->ldN);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("device quantize failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    b->index_base = src->index_base;
    *out = b;
    return INNR_OK;
}

// dense.rs:436-462 (matryoshka_dot / matryoshka_cosine) at batch level: the first prefix_dims dimensions of a
// dimension-major corpus ARE its first prefix_dims rows, so the coarse stage of examples/matryoshka_search.rs is a
// view, not a copy.
innr_status innr_batch_prefix_view(innr_batch* parent, size_t prefix_dims, innr_batch** out) {
    if (!parent || !out || prefix_dims == 0) {
        set_error("innr_batch_prefix_view: null batch/out or prefix_dims == 0");
        return INNR_E_BAD_ARG;
    }
    innr_batch* b = new (std::nothrow) innr_batch();
    if (!b) return INNR_E_OOM;
    b->ctx = parent->ctx;
    b->N = parent->N;
    b->ldN = parent->ldN;
    b->D = std::min(prefix_dims, parent->D);  // prefix_len.min(a.len()), dense.rs:437
    b->Dpad = round_up(b->D ? b->D : 1, 32);
    b->V = parent->V;
    b->C8 = parent->C8;
    b->alpha = parent->alpha;
    b->offset = parent->offset;
    b->index_base = parent->index_base;
    b->is_view = true;
    // a batch of its own to the accounting: it owns its copies, not the store, and its budget is its own -- from the context
    // option like any new batch's, NOT the parent's, whose budget the view's copies do not count against (the header says so)
    b->copy_budget = budget_from_option(parent->ctx);
    b->gemm_ok = parent->gemm_ok && (b->D == parent->D || b->D % 32 == 0);
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_minmax(innr_batch* b, float* out_min, float* out_max, int* out_any) {
    if (!b || !b->V || !out_min || !out_max || !out_any) {
        set_error("innr_batch_minmax needs an f32 batch");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    *out_any = 0;
    *out_min = 0.0f;
    *out_max = 0.0f;
    if (b->N == 0 || b->D == 0) return INNR_OK;
    INNR_TRY(c->misc.ensure(4096));
    INNR_HIP_CHECK(hipMemsetAsync(c->misc.p, 0, 8, c->stream));
    dim3 grid((unsigned)std::min<size_t>((b->ldN / 4 + 255) / 256, 256), (unsigned)std::min<size_t>(b->D, 32));  // <= 8192 blocks, one atomic pair each
    minmax_pdx_kernel<<<grid, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, c->misc.as<uint32_t>());
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t k[2] = {0, 0};
    INNR_HIP_CHECK(copy_out(c, k, c->misc.p, 8));
    INNR_HIP_CHECK(ctx_sync(c));
    if (k[0] && k[1]) {  // at least one non-NaN value
        *out_any = 1;
        *out_min = ord_f32(~k[0]);
        *out_max = ord_f32(k[1]);
    }
    return INNR_OK;
}

// QuantizationParams::fit_quantile's range (scalar.rs:104-139) of a resident f32 batch, without sorting it: the finite values'
// count M from a first histogram pass, the reference's two ranks from M in its own f32 arithmetic (:131-134), then a 4-pass
// radix select (one byte of the total_cmp key per pass, both ranks per pass) -- five streams of the corpus instead of a sort.
innr_status innr_batch_quantile_range(innr_batch* b, float quantile, float* out_lo, float* out_hi, int* out_any) {
    if (!b || !b->V || !out_lo || !out_hi || !out_any) {
        set_error("innr_batch_quantile_range needs an f32 batch");
        return INNR_E_BAD_ARG;
    }
    if (!(quantile > 0.0f && quantile <= 1.0f)) {  // assert!(quantile > 0.0 && quantile <= 1.0), scalar.rs:106-109
        set_error("quantile must be in (0.0, 1.0]");
        return INNR_E_DIM_MISMATCH;  // the reference panics: the host shims turn this status into their panic
    }
    if (quantile >= 1.0f) return innr_batch_minmax(b, out_lo, out_hi, out_any);  // scalar.rs:118-120: fit()
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    *out_any = 0;
    *out_lo = 0.0f;
    *out_hi = 0.0f;
    if (b->N == 0 || b->D == 0) return INNR_OK;
    INNR_TRY(c->misc.ensure(512 * sizeof(unsigned long long)));
    unsigned long long* dh = c->misc.as<unsigned long long>();
    dim3 grid((unsigned)std::min<size_t>((b->ldN / 4 + 255) / 256, 256), (unsigned)std::min<size_t>(b->D, 32));  // <= 8192 blocks, one atomic pair each
    unsigned long long hist[512];
    uint32_t pref[2] = {0u, 0u};
    unsigned long long rank[2] = {0ull, 0ull};
    for (int pass = 0; pass < 4; ++pass) {
        const uint32_t shift = 24 - 8 * pass, himask = pass ? (0xFFFFFFFFu << (shift + 8)) : 0u;
        INNR_HIP_CHECK(hipMemsetAsync(dh, 0, sizeof(hist), c->stream));
        quantile_hist_kernel<<<grid, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, shift, himask, pref[0], pref[1], dh);
        INNR_HIP_CHECK(hipGetLastError());
        INNR_HIP_CHECK(hipMemcpyAsync(hist, dh, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
        INNR_HIP_CHECK(hipStreamSynchronize(c->stream));
        if (pass == 0) {
            unsigned long long M = 0;
            for (int i = 0; i < 256; ++i) M += hist[i];
            if (M == 0) return INNR_OK;  // no finite value: alpha 1, offset 0 (scalar.rs:124-129)
            const float tail = (1.0f - quantile) / 2.0f;  // scalar.rs:131-134, f32 arithmetic
            unsigned long long lo = (unsigned long long)floorf(tail * (float)M);
            unsigned long long hi = (unsigned long long)ceilf((1.0f - tail) * (float)M);
            if (hi > M - 1) hi = M - 1;
            if (lo > M - 1) lo = M - 1;  // (the reference would index out of bounds; cannot happen for quantile in (0, 1))
            rank[0] = lo;
            rank[1] = hi;
        }
        for (int w = 0; w < 2; ++w) {  // the digit whose bucket holds the rank; the rank becomes relative to that bucket
            unsigned long long acc = 0;
            int dig = 255;
            for (int i = 0; i < 256; ++i) {
                if (rank[w] < acc + hist[256 * w + i]) {
                    dig = i;
                    break;
                }
                acc += hist[256 * w + i];
            }
            rank[w] -= acc;
            pref[w] |= (uint32_t)dig << shift;
        }
    }
    *out_lo = ord_f32(pref[0]);
    *out_hi = ord_f32(pref[1]);
    *out_any = 1;
    return INNR_OK;
}

// codes already dimension-major (what innr_batch_download_u8 wrote / a saved corpus holds): data[d*N + i]
innr_status innr_batch_upload_u8_colmajor(innr_ctx* ctx, const uint8_t* data, size_t N, size_t D, float alpha, float offset,
                                          innr_batch** out) {
    if ((!data && N * D) || !ctx) return INNR_E_BAD_ARG;
    INNR_ENTER(ctx);
    innr_batch* b = nullptr;
    INNR_TRY(alloc_batch_u8(ctx, N, D, alpha, offset, &b));
    if (N && D) {
        hipError_t e = hipMemcpy2DAsync(b->C8, b->ldN, data, N, N, D, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = ctx_sync(ctx);
        if (e != hipSuccess) {
            set_error("u8 corpus upload failed: %s", hipGetErrorString(e));
            innr_batch_free(b);
            return INNR_E_HIP;
        }
    }
    *out = b;
    return INNR_OK;
}

innr_status innr_batch_download_u8(innr_batch* b, uint8_t* out) {
    if (!b || !b->C8 || (!out && b->N * b->D)) return INNR_E_BAD_ARG;
    if (b->N == 0 || b->D == 0) return INNR_OK;
    INNR_ENTER(b->ctx);
    INNR_HIP_CHECK(hipMemcpy2DAsync(out, b->N, b->C8, b->ldN, b->N, b->D, hipMemcpyDeviceToHost, b->ctx->stream));
    INNR_HIP_CHECK(ctx_sync(b->ctx));
    return INNR_OK;
}

static innr_status u8_check(innr_batch* b, size_t D) {
    if (!b || !b->C8) {
        set_error("not a u8 batch");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // asymmetric_dot_u8_precomputed: "dimension mismatch" scalar.rs:290
        set_error("asymmetric_dot_u8_precomputed: dimension mismatch (%zu vs %zu)", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    return INNR_OK;
}

// every document's asymmetric score for one query (the map inside batch_knn_u8, scalar.rs:384-388)
innr_status innr_batch_scores_u8(innr_batch* b, const float* q, size_t D, float* out) {
    INNR_TRY(u8_check(b, D));
    if (b->N == 0) return INNR_OK;
    if (!out || (!q && D)) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    const size_t ldq = round_up(D ? D : 1, 4);
    INNR_TRY(c->q_row.ensure(ldq * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(2 * sizeof(float)));
    INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, q, D * sizeof(float)));
    float* qsum = c->q_norm.as<float>();
    query_sums_kernel<<<1, 64, 0, c->stream>>>(c->q_row.as<float>(), 1, (uint32_t)D, ldq, qsum, qsum + 1);
    const size_t nchunks = b->ldN / kU8Chunk;
    const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
    scan_u8_scores_kernel<1><<<blocks, 256, 0, c->stream>>>(b->C8, b->ldN, (uint32_t)D, c->q_row.as<float>(), ldq, qsum,
                                                            b->alpha / 255.0f, b->offset, c->scores.as<float>(), b->ldN);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_HIP_CHECK(copy_out(c, out, c->scores.p, b->N * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

static innr_status launch_scan_u8(innr_batch* b, uint32_t qb, const float* dQ, size_t ldq, const float* qsum, uint32_t nblocks,
                                  uint32_t KP, uint32_t cap, uint32_t cps, uint32_t groups, size_t limit_n, uint32_t nvalid_q,
                                  const uint8_t* mask) {
    innr_ctx* c = b->ctx;
    const uint32_t nvalid = (uint32_t)((limit_n && limit_n < b->N) ? limit_n : b->N);
    const float a255 = b->alpha / 255.0f;  // scalar.rs:299 (params.alpha / 255.0), f32
    dispatch([&](auto QB, auto rr) {
        record_scan(c, kScanU8, QB, INNR_METRIC_DOT, rr, mask != nullptr, cps, (size_t)nblocks * 4, groups);
        if (mask)  // the masked scan is a recorded family; the plain one runs inside most recorded calls and is not (cf. launch_scan_filter)
            launch_kernel(c, Inst<kLaunchScanU8Masked, QB, rr>(), {dim3(nblocks, groups), 256, 0, groups}, b->C8, b->ldN, nvalid,
                          (uint32_t)b->D, dQ, ldq, qsum, a255, b->offset, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(),
                          (uint32_t)(QB * groups), KP, cps, c->flags.as<uint32_t>(), nvalid_q, mask);
        else
            scan_u8_filter_kernel<QB, rr><<<dim3(nblocks, groups), 256, 0, c->stream>>>(
                b->C8, b->ldN, nvalid, (uint32_t)b->D, dQ, ldq, qsum, a255, b->offset, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(),
                QB * groups, KP, cps, c->flags.as<uint32_t>(), nvalid_q);
    }, one_of<8, 4, 1>(qb), rr_scan(cap));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// exact engine for queries [q0, q0+nq): qsum[] precomputed on device for all queries
// limit_n != 0: only the first limit_n documents take part (threshold seeding of the int8 engine)
// mask (nullable, [ldN] 0/1 bytes): only the vectors with mask[i] != 0 take part (innr_batch_knn_u8_filtered)
static innr_status knn_u8_exact_range(innr_batch* b, const float* dQ, size_t ldq, const float* qsum, size_t q0, size_t nq,
                                      size_t kout, uint64_t* d_out_idx, float* d_out_score, size_t limit_n = 0,
                                      const uint8_t* mask = nullptr) {
    const size_t cols = (limit_n && limit_n < b->N) ? round_up(limit_n, kU8Chunk) : b->ldN;
    const ScanGeom g = {cols, kU8Chunk, 16, 4, cols * b->D, false};
    return exact_scan_rounds(b, g, dQ, ldq, qsum, q0, nq, kout, d_out_idx, d_out_score,
                             [&](uint32_t qb, const float* q, const float* qs, uint32_t nblocks, uint32_t nql, uint32_t KP, uint32_t cap,
                                 uint32_t cps, uint32_t groups, uint32_t nreal) {
                                 return launch_scan_u8(b, qb, q, ldq, qs, nblocks, KP, cap, cps, groups, limit_n,
                                                       nreal < nql ? nreal : 0xFFFFFFFFu, mask);
                             });
}

// unproven queries of the u8 GEMM / int8 engines: gathered and redone together on the exact engine (4 per corpus pass)
static innr_status redo_batch_u8(innr_batch* b, const float* dQ, const float* qsum, const std::vector<uint32_t>& redo,
                                 size_t kout, uint64_t* d_out_idx, float* d_out_score) {
    innr_ctx* c = b->ctx;
    const size_t nr = redo.size(), D = b->D;
    if (nr == 0) return INNR_OK;
    if (nr == 1) return knn_u8_exact_range(b, dQ, D, qsum, redo[0], 1, kout, d_out_idx, d_out_score);
    innr_ctx::RedoBufs& rb = c->redo[0];
    INNR_TRY(upload_redo(c, rb, redo, D, kout));
    const uint32_t* map = rb.map.as<uint32_t>();
    if (D) {
        gather_rows_kernel<<<(unsigned)((nr * D + 255) / 256), 256, 0, c->stream>>>(dQ, map, (uint32_t)nr, (uint32_t)D,
                                                                                rb.q.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
    }
    gather_f32_kernel<<<(unsigned)((nr + 255) / 256), 256, 0, c->stream>>>(qsum, map, (uint32_t)nr, rb.qn.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    INNR_TRY(knn_u8_exact_range(b, rb.q.as<float>(), D, rb.qn.as<float>(), 0, nr, kout, rb.idx.as<uint64_t>(), rb.sc.as<float>()));
    return scatter_redo(c, rb, nr, kout, d_out_idx, d_out_score);
}

// error bound of the filters of a u8 corpus: |approx - exact| <= a255 * (2D+12) u * ||q|| * max||c||, with ||c|| <= 255 sqrt(D)
static float u8_filter_scale(const innr_batch* b) {
    const float a255 = b->alpha / 255.0f;
    return 1.05f * fabsf(a255) * (2.0f * (float)b->D + 12.0f) * 5.9604645e-08f * 255.0f * sqrtf((float)b->D);
}

// GEMM engine on a u8 corpus ("path B": codes widened to f32 in registers, f32 MFMA), same structure as knn_mfma
static innr_status knn_u8_mfma(innr_batch* b, const float* dQ, size_t Q, size_t kout, const float* qsum, const float* qnorm,
                               uint64_t* d_out_idx, float* d_out_score, uint32_t* nfallback, uint32_t* kept,
                               float* gemm_ms) {
    innr_ctx* c = b->ctx;
    const GemmPlan p = plan_gemm(b, Q, kout);
    INNR_TRY(c->q_kmajor.ensure(b->Dpad * p.Qpad * sizeof(float)));
    INNR_TRY(c->misc.ensure(p.Qpad * sizeof(float) + Q * sizeof(uint32_t) + 64));
    dim3 grid((unsigned)(p.Qpad / 32), (unsigned)(b->Dpad / 32));
    transpose_queries_kernel<<<grid, 256, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, c->q_kmajor.as<float>(), p.Qpad,
                                                          (uint32_t)b->Dpad);
    INNR_HIP_CHECK(hipGetLastError());
    float* oq = c->misc.as<float>();  // offset * sum(q) per query (0 for the padding queries)
    scale_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(qsum, b->offset, p.Qpad, Q, oq);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t* fallback = reinterpret_cast<uint32_t*>(c->misc.as<char>() + p.Qpad * sizeof(float));
    INNR_HIP_CHECK(hipMemsetAsync(fallback, 0, Q * sizeof(uint32_t), c->stream));
    INNR_TRY(ensure_lists(c, p));
    const float err_scale = u8_filter_scale(b);
    const float* kmargin = nullptr;
    INNR_TRY(make_kmargin(c, kSpaceCode, err_scale, qnorm, nullptr, nullptr, b->offset, qsum, Q, p.Qpad, &kmargin));
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    INNR_TRY((launch_gemm<kGemmU8, 0>(b, p, Q, c->q_kmajor.as<float>(), nullptr, oq, nullptr, 0, nullptr, kmargin, (uint32_t)kout)));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_TRY(run_select(c, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.nslices, (uint32_t)p.Qpad, p.cap, p.KP,
                        (uint32_t)Q));
    INNR_TRY(launch_rescore_u8(b, dQ, Q, qsum, qnorm, p.KP, kout, err_scale, d_out_idx, d_out_score, fallback, nullptr, nullptr, 0,
                               gthr_bounds(c, p.Qpad, p.KP)));
    std::vector<uint32_t> redo;
    INNR_TRY(harvest_proof(c, fallback, Q, p.KP, &redo, nfallback, kept, gemm_ms));
    return redo_batch_u8(b, dQ, qsum, redo, kout, d_out_idx, d_out_score);
}

// ---- int8 filter engine (kernels_gemm_i8.h) -------------------------------------------------------------------------
static uint32_t i8_nk(const innr_batch* b) { return (uint32_t)(round_up(b->D ? b->D : 1, 128) / 64); }  // K-steps of 64, even

// which int8 filter kernel: one limb on the matrix pipe + exact low-limb fix-up (default), or both limbs on the pipe
// (INNR_I8_TWO_LIMB=1, and for candidate lists of 256: the one-limb kernel's visit path and a 1280-entry list compaction
// do not fit the register file together -- tools/check_gemm_asm.py caught the operand ring being spilled)
static bool i8_two_limb(const innr_ctx* c, size_t kout) { return c->tune.i8_two_limb != 0 || pick_kp(kout, 16) > 128; }
static uint32_t i8_shift(bool two) { return two ? 8u : (uint32_t)kI8hS; }

static bool i8_eligible(const innr_batch* b, size_t Q) {
    return b->C8 && b->alpha > 0.0f && (b->alpha - b->alpha == 0.0f) && (b->offset - b->offset == 0.0f) && b->D >= 1 &&
           b->D <= 65535 && i8_limb_r1((uint32_t)b->D, 8) >= 1 && i8_limb_r1((uint32_t)b->D, (uint32_t)kI8hS) >= 1 &&
           b->ldN < ((size_t)1 << 31) && Q < ((size_t)1 << 24);
}

static size_t u8_i8_copy_bytes(const innr_batch* b) { return (b->ldN / 128) * (size_t)i8_nk(b) * kI8StageBytes; }

static innr_status ensure_i8_corpus(innr_batch* b) {
    const CorpusCopy& cc = b->copy[kCopyI8Dot];
    if (cc.p) return INNR_OK;
    const uint32_t nk = i8_nk(b);
    const size_t ntiles = b->ldN / 128;
    INNR_TRY(alloc_copy(b, kCopyI8Dot, u8_i8_copy_bytes(b), nk, false, "int8 corpus copy"));
    const size_t nthreads = ntiles * nk * 128;
    pack_corpus_i8_kernel<<<(unsigned)((nthreads + 255) / 256), 256, 0, b->ctx->stream>>>(b->C8, b->ldN, (uint32_t)b->N, (uint32_t)b->D, nk,
                                                                                      nthreads, reinterpret_cast<uint4*>(cc.p));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

struct I8Plan {
    size_t Qpad;
    uint32_t nqt, qtg, nslices, tps, KP, cap, nblocks, ntiles;
    const char* corpus;  // the copy the launch multiplies (built before the plan is made) ...
    uint32_t nk;         // ... and its K-steps of 64 dimensions (the squared-L2 copy has more than the others)
    bool two;  // both limbs on the matrix pipe (256-query tiles) instead of one limb + fix-up (512-query tiles)
    bool small = false;  // gemm_i8s_filter_kernel (<= 128 queries, every wave a slice of its own): nslices waves, tps QUARTER tiles each
    uint32_t small_ct = 2;  // ... its column tiles of 32 queries per wave: 2 (<= 64 queries) or 4
};
// The small-batch kernel applies to a one-limb MODE 0 launch of at most 128 queries with lists of 128 whose K-step count has an
// instantiation (even, <= 16: D <= 1024; the four-column-tile form for 65 .. 128 queries: 8 .. 16) and whose bounds are SEEDED (its
// survivors' path is built for a trickle, not for the flood of an unseeded first tile).
static bool plan_i8_small(const innr_batch* b, I8Plan* p, size_t Q, bool seeded, bool collect = false) {
    // (collect mode: fixed thresholds and global lists -- neither the list geometry nor seeding plays a part)
    if (p->two || p->nk > 16 || (p->nk & 1) || b->ctx->tune.i8_no_small) return false;
    if (!collect && (p->cap != 768 || !seeded)) return false;
    // beyond 64 queries: groups of 128 (four column tiles per wave), each a block of its own per corpus slice, the groups of a slice
    // side by side on one XCD (the slice comes from HBM once, the other groups read it from that XCD's L2)
    // (measured at C2, kernel ms, groups against the 512-query tile: 256 queries 2.63 / 3.55, 384: 3.77 / ~3.8, 512: 4.92 / 4.12, 1024:
    //  9.50 / 8.06 -- every group past the first costs another 1.15 ms = the copy at the streaming rate again: the groups of a slice
    //  drift apart and the XCD's L2 does not hold them together; profiles/r03_i8s_groups_c2.txt)
    const long maxq = b->ctx->tune.i8_small_max_q > 0 ? b->ctx->tune.i8_small_max_q : 256;
    if (Q > (size_t)kI8sBQ && (p->nk < 8 || b->ctx->tune.i8_no_small4 || Q > (size_t)std::min<long>(maxq, 1024))) return false;
    const uint32_t nquarter = 4 * p->ntiles;
    p->small = true;
    p->small_ct = Q > (size_t)kI8sBQ ? 4u : 2u;
    const uint32_t per = 32 * p->small_ct;
    p->nqt = p->qtg = (uint32_t)((Q + per - 1) / per);
    p->Qpad = (size_t)per * p->nqt;
    // blocks: nqt groups x slices; slices a multiple of 8 (XCDs), at most one block per CU
    uint32_t slices = std::max(1u, (uint32_t)b->ctx->num_cus / (8 * p->nqt)) * 8;
    slices = std::min(slices, std::max(8u, (nquarter + kI8sWaves - 1) / kI8sWaves / 8 * 8));
    p->nblocks = slices * p->nqt;
    p->nslices = slices * kI8sWaves;
    p->tps = (nquarter + p->nslices - 1) / p->nslices;
    return true;
}
static I8Plan plan_i8(const innr_batch* b, CopyKind kind, size_t Q, size_t kout, uint32_t kp_override = 0, bool one_limb = false) {
    I8Plan p;
    p.corpus = b->copy[kind].p;
    p.two = !one_limb && (i8_two_limb(b->ctx, kout) || kp_override > 128);  // (collect mode: always the one-limb kernel)
    p.nk = b->copy[kind].nk;
    const size_t bq = p.two ? (size_t)kI8BQ : (size_t)kI8hBQ;  // queries per block tile
    p.Qpad = round_up(Q, bq);
    p.nqt = (uint32_t)(p.Qpad / bq);
    p.KP = kp_override ? kp_override : pick_kp(kout, 16);
    p.cap = (uint32_t)cand_cap((int)p.KP);
    p.ntiles = (uint32_t)(b->ldN / 128);
    uint32_t target = std::max(1u, (uint32_t)b->ctx->num_cus / p.nqt);  // one 8-wave block per CU
    if (const long v = b->ctx->tune.i8_slices_per_cu; v > 1) target *= (uint32_t)std::min<long>(v, 16);
    uint32_t ns = std::max(8u, target / 8 * 8);
    ns = std::min(ns, (uint32_t)round_up(p.ntiles, 8));
    p.nslices = ns;
    p.tps = (p.ntiles + ns - 1) / ns;
    p.nblocks = p.nqt * ns;
    p.qtg = p.nqt;  // one query tile per XCD group where the tile count allows it (see plan_gemm)
    for (uint32_t g = 1; g <= p.nqt; ++g)
        if (p.nqt % g == 0 && 8 % (p.nqt / g) == 0) {
            p.qtg = g;
            break;
        }
    return p;
}

template <int MODE>
static innr_status launch_gemm_i8(innr_batch* b, const I8Plan& p, size_t nreal_q, const float* qc, float* dump, size_t ld_dump,
                                  const uint32_t* seed = nullptr, const float* kmargin = nullptr, uint32_t kk = 0) {
    innr_ctx* c = b->ctx;
    uint32_t* gslots = nullptr;
    size_t nslot = 0;
    if (!kmargin) kk = 0;
    INNR_TRY(prep_gthr(c, p.Qpad, MODE == 2 ? 32u : p.KP, seed, nreal_q, kmargin, &gslots, &nslot));  // (MODE 2: only the bounds are used)
    if (p.small) {
        if constexpr (MODE == 1) {
            set_error("internal: the small-batch int8 kernel has no mode %d", MODE);
            return INNR_E_BAD_ARG;
        } else {
            const size_t dyn = i8s_dyn_lds_bytes(p.nk, p.small_ct);
            uint32_t* prog = nullptr;
            if (p.nqt > 1 && !c->tune.i8_small_free) {
                INNR_TRY(c->i8s_prog.ensure((size_t)p.nslices * p.nqt * sizeof(uint32_t)));
                INNR_HIP_CHECK(hipMemsetAsync(c->i8s_prog.p, 0, (size_t)p.nslices * p.nqt * sizeof(uint32_t), c->stream));
                prog = c->i8s_prog.as<uint32_t>();
            }
            // (plan_i8_small: K-steps even and <= 16, lists of 128 = capacity 768 = R 12; four column tiles from 8 K-steps on. Every
            // instantiation has a row in tests/test_gpu_kernel_variants.py: I8_SMALL)
            INNR_TRY(dispatch([&](auto ct, auto nk) -> innr_status {
                if constexpr (ct == 4 && nk < 8) {
                    set_error("internal: the small-batch int8 kernel has no four-tile form of %d K-steps", (int)nk);
                    return INNR_E_BAD_ARG;
                } else {
                    constexpr auto inst = Inst<kLaunchI8Small, nk, ct, MODE>();
                    if (dyn > 48 * 1024) /* (per device and call: no process-wide state) */
                        INNR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_of(inst)),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)i8s_dyn_lds_bytes(nk, ct)));
                    launch_kernel(c, inst, {p.nblocks, 64 * kI8sWaves, dyn, p.nqt, prog != nullptr}, p.corpus, c->q_bf16.as<char>(),
                                  4 * p.ntiles, (uint32_t)b->N, p.Qpad, p.nqt, p.tps, qc, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(),
                                  p.KP, kk, c->flags.as<uint32_t>(), gslots, gslots + nslot, prog);
                    return INNR_OK;
                }
            }, one_of<4, 2>(p.small_ct), one_of<2, 4, 6, 8, 10, 12, 14, 16>(p.nk)));
        }
    } else {
        // the 512-query one-limb tile (gemm_i8h_filter_kernel) or the 256-query two-limb tile (gemm_i8_filter_kernel): one argument list
        const auto tile = [&](auto family, auto rr) {
            launch_kernel(c, Inst<family, rr, MODE>(), {p.nblocks, 64 * kI8Waves, 0, p.nqt}, p.corpus, c->q_bf16.as<char>(), p.ntiles,
                          (uint32_t)b->N, p.nk, p.Qpad, p.nqt, p.qtg, p.tps, qc, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.KP, kk,
                          c->flags.as<uint32_t>(), gslots, gslots + nslot, dump, ld_dump);
        };
        const auto limbs = one_of<kLaunchI8Two, kLaunchI8One>(p.two ? kLaunchI8Two : kLaunchI8One);
        if constexpr (MODE == 2) {  // collect (the completion pass): one-limb kernel, the list geometry plays no part
            tile(IntC<kLaunchI8One>(), IntC<6>());
        } else if constexpr (MODE == 1) {  // the dense-score dump: the list geometry plays no part
            dispatch([&](auto family) { tile(family, IntC<6>()); }, limbs);
        } else {  // (every instantiation has a row in tests/test_gpu_kernel_variants.py: I8_TILES)
            dispatch([&](auto family, auto rr) {
                if constexpr (rr == 20) tile(IntC<kLaunchI8Two>(), rr);  // lists of 256 candidates: the two-limb kernel only (plan_i8)
                else tile(family, rr);
            }, limbs, rr_gemm(p.cap));
        }
    }
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// queries -> two int8 limbs + per-query constants: Bq in c->q_bf16, qc[5][Qpad] at c->misc
// (alpha, offset: the code corpus' QuantizationParams, or the scalar quantisation of an f32 corpus' filter copy)
static innr_status prep_queries_i8(innr_batch* b, const I8Plan& p, const float* dQ, size_t Q, const float* qsum, float alpha,
                                   float offset, size_t Dq = 0 /* query dimension if not the batch's (the squared-L2 copy's D') */) {
    innr_ctx* c = b->ctx;
    if (!Dq) Dq = b->D;
    INNR_TRY(c->q_bf16.ensure((size_t)p.nk * 8 * p.Qpad * 16));
    INNR_TRY(c->misc.ensure(5 * p.Qpad * sizeof(float) + Q * sizeof(uint32_t) + 64));
    pack_queries_i8_kernel<<<(unsigned)p.Qpad, 64, 0, c->stream>>>(dQ, qsum, (uint32_t)Q, (uint32_t)Dq, p.nk, (uint32_t)p.Qpad,
                                                                   i8_limb_r1((uint32_t)Dq, i8_shift(p.two)), i8_shift(p.two), alpha / 255.0f,
                                                                   offset, reinterpret_cast<uint4*>(c->q_bf16.p), c->misc.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// int8-MFMA filter + exact re-score + proof; same contract as knn_u8_mfma
static innr_status knn_u8_i8(innr_batch* b, const float* dQ, size_t Q, size_t kout, const float* qsum, const float* qnorm,
                             uint64_t* d_out_idx, float* d_out_score, uint32_t* nfallback, uint32_t* kept, float* gemm_ms) {
    innr_ctx* c = b->ctx;
    INNR_TRY(ensure_i8_corpus(b));
    I8Plan p = plan_i8(b, kCopyI8Dot, Q, kout);
    const bool seeded = seeding_on(b, true, Q, p.KP);
    if (!plan_i8_small(b, &p, Q, seeded) && seeded && p.KP < 128 && Q <= 1024) {
        // the small-batch kernel is instantiated for lists of 128: a small k takes them too (a capacity, not a threshold -- the k
        // rule sets the bounds) rather than the 512-query tile
        I8Plan p2 = plan_i8(b, kCopyI8Dot, Q, kout, 128u);
        if (plan_i8_small(b, &p2, Q, seeded)) p = p2;
    }
    INNR_TRY(prep_queries_i8(b, p, dQ, Q, qsum, b->alpha, b->offset));
    const float* qc = c->misc.as<float>();
    uint32_t* fallback = reinterpret_cast<uint32_t*>(c->misc.as<char>() + 5 * p.Qpad * sizeof(float));
    INNR_HIP_CHECK(hipMemsetAsync(fallback, 0, Q * sizeof(uint32_t), c->stream));
    // the reference's own f32 accumulation against the true sum: (D + 2) u ||q|| max||c||, ||c|| <= 255 sqrt(D) (the bound of
    // knn_u8_mfma, whose MFMA-chain half is simply unused here); the query's quantisation share comes per query (qc[3])
    const float err_scale = u8_filter_scale(b);
    // threshold seeding: the prefix's k-th (KP-th) exact score lowered by the query's error bound is a valid chip-wide bound
    // from the first tile on
    const uint32_t* seed = nullptr;
    if (seeded) {
        uint32_t kseed, *sd;
        INNR_TRY(seed_prefix(b, true, Q, p.Qpad, p.KP, kout, &kseed, &sd, [&](uint32_t ks, uint64_t* idx, float* sc, size_t rows) {
            return knn_u8_exact_range(b, dQ, b->D, qsum, 0, Q, ks, idx, sc, rows);
        }));
        seed_thresholds_u8_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(
            c->seed_score.as<float>(), (uint32_t)Q, kseed, err_scale, qnorm, qsum, b->offset, qc + 3 * p.Qpad, sd, (uint32_t)p.Qpad,
            kseed - 1);
        INNR_HIP_CHECK(hipGetLastError());
        seed = sd;
    }
    INNR_TRY(ensure_lists(c, p));
    const float* kmargin = nullptr;
    INNR_TRY(make_kmargin(c, kSpaceCode, err_scale, qnorm, nullptr, qc + 3 * p.Qpad, b->offset, qsum, Q, p.Qpad, &kmargin));
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    INNR_TRY(launch_gemm_i8<0>(b, p, Q, qc, nullptr, 0, seed, kmargin, (uint32_t)kout));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_TRY(run_select(c, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.nslices, (uint32_t)p.Qpad, p.cap, p.KP, (uint32_t)Q));
    INNR_TRY(launch_rescore_u8(b, dQ, Q, qsum, qnorm, p.KP, kout, err_scale, d_out_idx, d_out_score, fallback, qc + 3 * p.Qpad,
                               reinterpret_cast<const uint4*>(p.corpus), p.nk, gthr_bounds(c, p.Qpad, p.KP)));
    std::vector<uint32_t> redo;
    INNR_TRY(harvest_proof(c, fallback, Q, p.KP, &redo, nfallback, kept, gemm_ms));
    return redo_batch_u8(b, dQ, qsum, redo, kout, d_out_idx, d_out_score);
}

#ifdef INNR_TEST_HOOKS
// (MODE 1 of the int8 kernels exists in this build only)
// Test hook (not part of the ABI): dense approximate score matrix of the int8 engine, out[q*N + i] = A_q V(q, i) + B_q, and
// the per-query constants qc[4][Qpad] -- to check the int8 MFMA operand layout and the limb arithmetic exactly.
extern "C" innr_status innrdbg_i8_scores(innr_batch* b, const float* queries, size_t Q, size_t D, float* out, float* qc_out,
                                         size_t* qpad_out) {
    if (!b || !b->C8 || !queries || !out || D != b->D || Q == 0 || b->N == 0 || !i8_eligible(b, Q)) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(ensure_i8_corpus(b));
    const I8Plan p = plan_i8(b, kCopyI8Dot, Q, 1);
    INNR_TRY(c->q_row.ensure(Q * D * sizeof(float)));
    INNR_TRY(c->q_norm.ensure(2 * p.Qpad * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    float* qsum = c->q_norm.as<float>();
    query_sums_kernel<<<(unsigned)((Q + 63) / 64), 64, 0, c->stream>>>(c->q_row.as<float>(), (uint32_t)Q, (uint32_t)D, D, qsum, qsum + p.Qpad);
    INNR_TRY(prep_queries_i8(b, p, c->q_row.as<float>(), Q, qsum, b->alpha, b->offset));
    INNR_TRY(ensure_lists(c, p));
    INNR_TRY(c->scores.ensure(p.Qpad * b->ldN * sizeof(float)));
    INNR_TRY(launch_gemm_i8<1>(b, p, Q, c->misc.as<float>(), c->scores.as<float>(), b->ldN));
    INNR_HIP_CHECK(hipMemcpy2DAsync(out, b->N * sizeof(float), c->scores.p, b->ldN * sizeof(float), b->N * sizeof(float), Q,
                                    hipMemcpyDeviceToHost, c->stream));
    if (qc_out) INNR_HIP_CHECK(hipMemcpyAsync(qc_out, c->misc.p, 5 * p.Qpad * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (qpad_out) *qpad_out = p.Qpad;
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}
#endif  // INNR_TEST_HOOKS

// ---- the int8 filter in front of an F32 corpus (INNR_KNN_MFMA_I8 on an f32 batch; dot and cosine) ------------------------------
// The corpus is scalar-quantised once with a single (offset, alpha) -- the reference's own quantize_u8 with the corpus' range,
// i.e. the first stage of its two-stage pipeline (scalar.rs:366-368) -- and filtered on the integer matrix pipe (twice the bf16
// rate, half the bytes of the bf16 copy); the candidates are re-scored on the f32 corpus in the reference's order and the answer
// is PROVEN against bound = query quantisation + (alpha / 510) |q|_1 + the reference's own accumulation error; unproven queries
// go through the f32 GEMM engine as one batch, like the bf16 filter's.
static bool f32_i8_eligible(const innr_batch* b, int metric, size_t Q, size_t kout) {
    const uint32_t Dx = (uint32_t)b->D + (metric == INNR_METRIC_L2SQ ? 121u : 0u);  // squared L2: up to 121 more dimensions (|v|^2)
    return b->V && kout <= INNR_MAX_K && b->D >= 1 && Dx <= 65535 &&
           i8_limb_r1(Dx, 8) >= 1 && i8_limb_r1(Dx, (uint32_t)kI8hS) >= 1 && b->ldN < ((size_t)1 << 31) &&
           Q < ((size_t)1 << 24) && b->gemm_ok;
}
static size_t f32_i8_copy_bytes(const innr_batch* b, int metric) {  // (squared L2: at most 121 more dimensions)
    const size_t nk = metric == INNR_METRIC_L2SQ ? round_up(b->D + 121, 128) / 64 : (size_t)i8_nk(b);
    return (b->ldN / 128) * nk * kI8StageBytes;
}

static innr_status ensure_f32_i8_corpus(innr_batch* b, CopyKind kind, bool* usable) {
    *usable = true;
    const bool normalised = kind == kCopyI8Cos, l2 = kind == kCopyI8L2;
    const CorpusCopy& cc = b->copy[kind];
    if (cc.p) return INNR_OK;
    // the range of what is quantised: the corpus values (dot and squared L2), resp. the normalised rows (for 768-dimensional
    // uniform data these live in +-0.06: quantising them over [-1, 1] would throw four of the eight bits away)
    innr_batch::I8Range& range = b->i8_range(kind);
    float offset = range.offset, alpha = range.alpha;
    if (!(alpha > 0.0f)) {
        innr_ctx* c = b->ctx;
        INNR_TRY(c->misc.ensure(4096));
        INNR_HIP_CHECK(hipMemsetAsync(c->misc.p, 0, 8, c->stream));
        dim3 grid((unsigned)std::min<size_t>((b->ldN / 4 + 255) / 256, 256), (unsigned)std::min<size_t>(b->D, 32));  // <= 8192 blocks, one atomic pair each
        minmax_pdx_kernel<<<grid, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, c->misc.as<uint32_t>(),
                                                       normalised ? b->invn : nullptr);
        INNR_HIP_CHECK(hipGetLastError());
        uint32_t k[2] = {0, 0};
        INNR_HIP_CHECK(copy_out(c, k, c->misc.p, 8));
        INNR_HIP_CHECK(ctx_sync(c));
        const float mn = ord_f32(~k[0]), mx = ord_f32(k[1]);
        alpha = mx - mn;
        if (!k[0] || !k[1] || !(alpha > 0.0f) || !(alpha - alpha == 0.0f)) {  // empty / constant / infinite range: nothing to quantise against
            *usable = false;
            return INNR_OK;
        }
        offset = mn;
        range = {alpha, offset};
    }
    uint32_t nk = i8_nk(b), R = 0;
    float nmax = 0.0f;
    if (l2) {
        // |v|^2 in R + 1 more dimensions: R such that the weight -(nmax / alpha) / R of each stays near the 2 q_d beside it
        nmax = b->max_norm * b->max_norm * 1.000001f;
        const float ratio = nmax / alpha;
        if (!(nmax > 0.0f) || !(ratio - ratio == 0.0f)) {
            *usable = false;
            return INNR_OK;
        }
        R = (uint32_t)std::min(120.0f, std::max(1.0f, ceilf(0.5f * ratio)));
        nk = (uint32_t)(round_up(b->D + R + 1, 128) / 64);
    }
    const size_t ntiles = b->ldN / 128;
    INNR_TRY(alloc_copy(b, kind, ntiles * nk * (size_t)kI8StageBytes, nk, false, "int8 filter copy"));
    const size_t nthreads = ntiles * nk * 128;
    pack_corpus_f32_i8_kernel<<<(unsigned)((nthreads + 255) / 256), 256, 0, b->ctx->stream>>>(
        b->V, b->ldN, (uint32_t)b->N, (uint32_t)b->D, nk, nthreads, offset, 255.0f / alpha, normalised ? b->invn : nullptr,
        reinterpret_cast<uint4*>(cc.p), l2 ? b->sqn : nullptr, R, l2 ? 1.0f / nmax : 0.0f);
    INNR_HIP_CHECK(hipGetLastError());
    if (l2) {
        b->i8l2_R = R;
        b->i8l2_nmax = nmax;
    }
    return INNR_OK;
}

// The int8 copy of a metric with what it is built from (norms, 1/norm, norm^2); *usable = false: the filter does not apply to this
// corpus (a norm outside the bound's range, constant or non-finite values)
static innr_status ensure_f32_i8_filter(innr_batch* b, int metric, bool* usable) {
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    *usable = false;
    INNR_TRY(ensure_norms(b));
    if (!(b->max_norm - b->max_norm == 0.0f) || !(b->max_norm >= 1e-12f) || (l2 && !(b->max_norm <= 1e15f))) return INNR_OK;
    if (cos) INNR_TRY(ensure_invnorms(b));
    if (l2) INNR_TRY(ensure_sqnorms(b));
    return ensure_f32_i8_corpus(b, i8_kind(metric), usable);
}

// *served = false: the engine does not apply to this corpus (constant values): the caller takes the f32 engine
// collect_kth != null: the COMPLETION pass of this filter (cf. knn_complete): dQ are the unproven queries (gathered), collect_kth[j]
// = the k-th best EXACT score query j has so far (a lower bound of the true one); the kernel runs in collect mode with the fixed
// thresholds x_k - E_j, everything collected is re-scored from the row-major copy and the best k written to d_out_* [Q][kout];
// d_unresolved[j] = 1 where the list overflowed (those queries go on to the f32 engine).
innr_status innr::knn_f32_i8(innr_batch* b, int metric, const float* dQ, size_t Q, size_t kout, uint64_t* d_out_idx,
                             float* d_out_score, uint32_t* nfallback, uint32_t* kept, float* gemm_ms, bool* served,
                             const float* collect_kth, uint32_t* d_unresolved) {
    innr_ctx* c = b->ctx;
    const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
    *served = false;
    bool usable = true;
    const CopyKind kind = i8_kind(metric);
    INNR_TRY(ensure_f32_i8_filter(b, metric, &usable));
    if (!usable) return INNR_OK;
    *served = true;
    const float alpha = b->i8_range(kind).alpha, offset = b->i8_range(kind).offset;
    // squared L2 (pack_corpus_f32_i8_kernel): a dot product over D' = D + R + 1 dimensions plus per-query constants
    const size_t Dq = l2 ? b->D + b->i8l2_R + 1 : b->D;
    // Lists of 4k + 64 let the k-th exact score clear the KP-th approximate one by a visible margin (k <= 48); beyond that the
    // lists hold k + 16 (one-limb kernel up to 128, two-limb kernel to 256), most proofs fail BY DESIGN and the completion pass
    // (one more pass of this filter in collect mode) settles them: k = 100 at C2 needs ~450 candidates per query.
    // k = 17 .. 48: direct lists would be 256 long -- the two-limb kernel (21.7 ms at C2 for k = 48, 4.7 ms for eight queries). With
    // the k rule setting the bounds, lists of 128 prove most of those answers as well (k = 32: all of a batch of eight; k = 48: 59 of
    // 64) and the collect pass settles the rest: 2.1 ms for eight queries at k = 32, 4.0 for 64 at k = 48.
    const uint32_t direct_kp = pick_kp(4 * kout + 64, 0);
    const bool direct = direct_kp <= 128;
    I8Plan p = plan_i8(b, kind, Q, kout, collect_kth ? 32u : (direct ? direct_kp : std::max(128u, pick_kp(kout, 16))), collect_kth != nullptr);
    const bool seeded = seeding_on(b, true, Q, p.KP);
    (void)plan_i8_small(b, &p, Q, seeded, collect_kth != nullptr);
    // exact query norms; cosine: 1/||q|| and the normalised copy the filter multiplies; sum and L1 norm of what it multiplies
    INNR_TRY(c->q_norm.ensure(p.Qpad * sizeof(float)));
    INNR_TRY(c->tmp_norms.ensure(6 * p.Qpad * sizeof(float)));
    float* qsum = c->tmp_norms.as<float>();
    float* ql1 = qsum + p.Qpad;
    float* invq = ql1 + p.Qpad;
    float* cq = invq + p.Qpad;  // squared L2: C_j - |q_j|^2, C_j = (|q_j| + max|v|)^2 (the score space C_j - distance of the f32 engine)
    float* Cj = cq + p.Qpad;
    float* ql1q = Cj + p.Qpad;  // ... and the L1 norm of the query itself
    query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, b->D, c->q_norm.as<float>());
    INNR_HIP_CHECK(hipGetLastError());
    const float* Qp = dQ;
    if (cos) {
        INNR_TRY(c->q_hat.ensure(std::max<size_t>(Q * b->D, 1) * sizeof(float)));
        inv_qnorms_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(c->q_norm.as<float>(), p.Qpad, Q, invq);
        INNR_HIP_CHECK(hipGetLastError());
        Qp = c->q_hat.as<float>();
    }
    const float W = l2 ? b->i8l2_nmax / alpha : 0.0f, w1 = l2 ? W / (float)b->i8l2_R : 0.0f, w2 = W / 255.0f;
    if (l2) {
        INNR_TRY(c->q_hat.ensure(std::max<size_t>(Q * Dq, 1) * sizeof(float)));
        f32i8_l2_queries_kernel<<<(unsigned)((Q * Dq + 255) / 256), 256, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, b->i8l2_R, w1, w2,
                                                                                     c->q_hat.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        f32i8_query_prep_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, nullptr, nullptr, qsum, ql1q);
        INNR_HIP_CHECK(hipGetLastError());
        l2_query_consts_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(c->q_norm.as<float>(), p.Qpad, Q, b->max_norm, cq, Cj);
        INNR_HIP_CHECK(hipGetLastError());
        Qp = c->q_hat.as<float>();
    }
    f32i8_query_prep_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(l2 ? Qp : dQ, (uint32_t)Q, (uint32_t)Dq, cos ? invq : nullptr,
                                                                            cos ? c->q_hat.as<float>() : nullptr, qsum, ql1);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_TRY(prep_queries_i8(b, p, Qp, Q, qsum, alpha, offset, Dq));
    float* qc = c->misc.as<float>();
    // the reference's own accumulation against the true dot: (D + 2) u |q||v| (half of the f32 GEMM engine's cdu)
    const float cdu = f32_cdu(b);
    // (squared L2: the corpus' quantisation touches the 2 q_d only -- the |v|^2 limbs are exact integers, their encoding error and
    //  the f32 terms are f32i8_l2_finish_kernel's)
    f32i8_finish_bound_kernel<<<(unsigned)((Q + 255) / 256), 256, 0, c->stream>>>(qc, (uint32_t)p.Qpad, (uint32_t)Q, l2 ? ql1q : ql1, c->q_norm.as<float>(),
                                                                               alpha, l2 ? 0.0f : (cos ? cdu * 1.02f : cdu * b->max_norm), cos || l2 ? 1 : 0,
                                                                               128.0f * alpha / 255.0f + offset, (float)Dq, l2 ? 2.0f : 1.0f, ql1);
    INNR_HIP_CHECK(hipGetLastError());
    if (l2) {
        // -|v|^2 = -W z1^ - w2 z2^ + K0 (+- nmax / 130050: the second limb's rounding; + the f32 roundings of z' = offset + alpha n /
        // nmax, relative to |offset| + alpha, times W); the f32 squared-L2 engine's (6D + 40) u C_j covers the cached norms, the
        // constants and the reference's own direct-difference sum
        const float K0 = W * offset + w2 * (offset + 0.5f * alpha);
        const float enc_err = b->i8l2_nmax * (1.1f / 130050.0f + 3.0e-7f * (fabsf(offset) / alpha + 1.0f));
        f32i8_l2_finish_kernel<<<(unsigned)((Q + 255) / 256), 256, 0, c->stream>>>(qc, (uint32_t)p.Qpad, (uint32_t)Q, cq, Cj, K0, enc_err,
                                                                                f32_filter_scale(b, metric));
        INNR_HIP_CHECK(hipGetLastError());
    }
    const float* eq = qc + 3 * p.Qpad;
    uint32_t* fallback = reinterpret_cast<uint32_t*>(c->misc.as<char>() + 5 * p.Qpad * sizeof(float));
    INNR_HIP_CHECK(hipMemsetAsync(fallback, 0, Q * sizeof(uint32_t), c->stream));
    if (collect_kth) {
        // ---- completion pass: fixed thresholds x_k - E_j, global lists, exact re-score of everything collected ----
        INNR_TRY(c->seed_score.ensure(p.Qpad * sizeof(uint32_t)));
        uint32_t* thr = c->seed_score.as<uint32_t>();
        seed_thresholds_eq_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(collect_kth, (uint32_t)Q, 1u, eq, thr, (uint32_t)p.Qpad, 0u,
                                                                                       l2 ? Cj : nullptr);
        INNR_HIP_CHECK(hipGetLastError());
        INNR_TRY(c->lists.ensure(p.Qpad * (size_t)kCollectCap * sizeof(uint32_t)));
        INNR_TRY(c->counts.ensure(p.Qpad * sizeof(uint32_t)));
        INNR_HIP_CHECK(hipMemsetAsync(c->counts.p, 0, p.Qpad * sizeof(uint32_t), c->stream));
        I8Plan pl = p;
        pl.KP = kCollectCap;
        INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
        INNR_TRY(launch_gemm_i8<2>(b, pl, Q, qc, nullptr, 0, thr));
        INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
        INNR_TRY(collect_finish(b, metric, dQ, c->q_norm.as<float>(), Q, kout, d_out_idx, d_out_score, d_unresolved));
        return INNR_OK;  // (the caller reads ev[2..3] once it has synchronised)
    }
    const uint32_t* seed = nullptr;
    if (seeded) {
        uint32_t kseed, *sd;
        INNR_TRY(seed_prefix(b, true, Q, p.Qpad, p.KP, kout, &kseed, &sd, [&](uint32_t ks, uint64_t* idx, float* sc, size_t rows) {
            return knn_exact_range(b, metric, dQ, b->D, c->q_norm.as<float>(), 0, Q, ks, idx, sc, ScanExt(), rows);
        }));
        seed_thresholds_eq_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(c->seed_score.as<float>(), (uint32_t)Q, kseed, eq, sd,
                                                                                       (uint32_t)p.Qpad, kseed - 1, l2 ? Cj : nullptr);
        INNR_HIP_CHECK(hipGetLastError());
        seed = sd;
    }
    INNR_TRY(ensure_lists(c, p));
    const float* kmargin = nullptr;
    INNR_TRY(make_kmargin(c, kSpaceEq, 0.0f, nullptr, nullptr, eq, 0.0f, nullptr, Q, p.Qpad, &kmargin));
    INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    INNR_TRY(launch_gemm_i8<0>(b, p, Q, qc, nullptr, 0, seed, kmargin, (uint32_t)kout));
    INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_TRY(run_select(c, c->lists.as<uint64_t>(), c->counts.as<uint32_t>(), p.nslices, (uint32_t)p.Qpad, p.cap, p.KP, (uint32_t)Q));
    INNR_TRY(launch_rescore(b, metric_space(metric), dQ, Q, l2 ? Cj : nullptr, p.KP, kout, 0.0f, d_out_idx, d_out_score, fallback, eq,
                            !c->tune.rescore_all, gthr_bounds(c, p.Qpad, p.KP)));
    std::vector<uint32_t> redo;
    INNR_TRY(harvest_proof(c, fallback, Q, p.KP, &redo, nfallback, kept, gemm_ms));
    // (lists sized for a direct proof that mostly fail: the corpus' range is blown up by outliers; AUTO takes the bf16 filter,
    //  whose error is relative, on this corpus from now on -- and looks at the int8 one again every 64th call, innr_batch_knn_dev)
    if (direct && Q >= 16) b->copy[kind].weak = redo.size() * 2 > Q;
    // ONE more pass of this filter in collect mode settles the unproven queries (k beyond the direct lists: nearly all of them)
    // (from the first unproven query on: one more pass over the int8 copy costs less than an exact pass over the f32 corpus)
    if (!redo.empty() && !c->tune.no_completion) {
        std::vector<uint32_t> still;
        INNR_TRY(knn_complete_i8(b, metric, dQ, redo, kout, d_out_idx, d_out_score, &still, gemm_ms));
        redo.swap(still);
    }
    if (!redo.empty()) {  // one batch on the f32 GEMM engine (its own proof, completion pass and the exact engine behind it)
        if (cos) {  // (the completion pass used the query workspace: the exact norms of the whole batch again)
            query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)b->D, b->D, c->q_norm.as<float>());
            INNR_HIP_CHECK(hipGetLastError());
        }
        INNR_TRY(redo_batch(b, metric, dQ, cos ? c->q_norm.as<float>() : nullptr, redo, kout, d_out_idx, d_out_score,
                            redo.size() >= 4 ? pick_kp(kout, 16) : 0u, 0));
    }
    return INNR_OK;
}

innr_status innr_batch_knn_u8_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, int engine,
                                  uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!out_k) return INNR_E_BAD_ARG;
    *out_k = 0;
    if (b && b->C8 && (b->N == 0 || k == 0)) return INNR_OK;  // scalar.rs:376-378: checked before any dimension assert
    INNR_TRY(u8_check(b, D));
    if (Q == 0) return INNR_OK;
    const size_t kout = std::min(k, b->N);  // scalar.rs:381
    if (!d_queries || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    INNR_TRY(c->q_norm.ensure(2 * round_up(Q, kBQmax) * sizeof(float)));
    float* qsum = c->q_norm.as<float>();
    float* qnorm = qsum + round_up(Q, kBQmax);
    query_sums_kernel<<<(unsigned)((Q + 63) / 64), 64, 0, c->stream>>>(d_queries, (uint32_t)Q, (uint32_t)D, D, qsum, qnorm);
    INNR_HIP_CHECK(hipGetLastError());
    if (engine == INNR_KNN_AUTO) {
        engine = innr_batch_auto_engine(b, Q);
        if (i8_eligible(b, Q) && !c->tune.u8_no_i8 && b->N >= 65536 && gemm_addressable(b, Q)) {
            // The int8 engine streams its K-packed copy (N*D more bytes of HBM, built on first use) ONCE for up to 128 queries
            // (gemm_i8s_filter_kernel: 6.0 ms = 6.4 TB/s at 50M x 768 up to 64 queries, 8.1 ms up to 128) where the exact engine takes
            // 6.4 ms for one query, 8.1 for two, 14.2 for eight (profiles/r03_u8_smallq_50Mx768.txt): from two queries on once the copy
            // exists, from four when it has to be built and fits with room to spare; larger batches as before.
            size_t free_b = 0, total_b = 0;
            const bool have_mem = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
            const size_t copy_b = u8_i8_copy_bytes(b);
            const bool have_copy = b->copy[kCopyI8Dot].p != nullptr;
            const bool worth = Q >= 4 || (Q >= 2 && !have_copy && ++b->auto_small_calls >= 4);  // (the fourth small call builds the copy)
            if (have_copy ? Q >= 2 : (worth && have_mem && copy_fits(free_b, copy_b) && budget_admits(b, copy_b))) engine = INNR_KNN_MFMA_I8;
        }
    }
    if (engine == INNR_KNN_MFMA_BF16) engine = INNR_KNN_MFMA;  // codes are exact in 8 bits: the low-precision filter is the int8 one
    if (engine == INNR_KNN_MFMA_I8 && !i8_eligible(b, Q)) engine = INNR_KNN_MFMA;  // alpha <= 0 / non-finite params / D beyond the limbs
    if (engine == INNR_KNN_MFMA_I8 && !b->copy[kCopyI8Dot].p && !budget_admits(b, u8_i8_copy_bytes(b)))  // beyond the copy budget
        engine = INNR_KNN_MFMA;
    if (engine == INNR_KNN_MFMA && !gemm_addressable(b, Q)) engine = INNR_KNN_EXACT;
    if (kout > INNR_MAX_K) engine = INNR_KNN_EXACT;
    uint32_t nfallback = 0, kept = kout > INNR_MAX_K ? (uint32_t)b->N : pick_kp(kout, 0);
    float gemm_ms = 0.0f;
    if (kout > INNR_MAX_K) {
        INNR_TRY(knn_full_sort(b, -1, d_queries, D, qsum, Q, kout, d_out_idx, d_out_score));
    } else if (engine == INNR_KNN_MFMA_I8) {
        INNR_TRY(knn_u8_i8(b, d_queries, Q, kout, qsum, qnorm, d_out_idx, d_out_score, &nfallback, &kept, &gemm_ms));
    } else if (engine == INNR_KNN_MFMA) {
        INNR_TRY(knn_u8_mfma(b, d_queries, Q, kout, qsum, qnorm, d_out_idx, d_out_score, &nfallback, &kept, &gemm_ms));
    } else {
        INNR_TRY(knn_u8_exact_range(b, d_queries, D, qsum, 0, Q, kout, d_out_idx, d_out_score));
    }
    return finish_knn(c, engine, kout, nfallback, kept, gemm_ms, out_k, stats);
}

innr_status innr_batch_knn_u8(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, int engine,
                              uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !b->C8 || !out_k) return INNR_E_BAD_ARG;
    *out_k = 0;
    if (b->N == 0 || k == 0) return INNR_OK;
    INNR_TRY(u8_check(b, D));
    if (Q == 0) return INNR_OK;
    if (!queries && D) return INNR_E_BAD_ARG;
    return knn_from_host(b->ctx, queries, Q, D, std::min(k, b->N), out_idx, out_score, out_k, [&](const float* dQ, uint64_t* di, float* ds) {
        return innr_batch_knn_u8_dev(b, dQ, Q, D, k, engine, di, ds, out_k, stats);
    });
}

extern "C" {

// ---- L2 variants (exact engine) ------------------------------------------------------------------------
innr_status innr_batch_dimension_variance(innr_batch* b, float* out) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || (!out && b->D)) return INNR_E_BAD_ARG;
    if (b->D == 0) return INNR_OK;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    if (b->dimvar.empty()) {
        INNR_TRY(c->misc.ensure(b->D * sizeof(float)));
        dimension_variance_kernel<<<(unsigned)((b->D + 63) / 64), 64, 0, c->stream>>>(b->V, b->ldN, (uint32_t)b->N,
                                                                                    (uint32_t)b->D, c->misc.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        b->dimvar.resize(b->D);
        INNR_HIP_CHECK(copy_out(c, b->dimvar.data(), c->misc.p, b->D * sizeof(float)));
        INNR_HIP_CHECK(ctx_sync(c));
    }
    memcpy(out, b->dimvar.data(), b->D * sizeof(float));
    return INNR_OK;
}

// shared driver of batch_knn_filtered / batch_knn_reordered: one query, L2, optional mask / dimension order
static innr_status knn_l2_ext(innr_batch* b, const float* q, size_t D, size_t k, const uint8_t* mask,
                              const uint32_t* order_host, uint64_t* out_idx, float* out_score, size_t* out_k) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !out_k) return INNR_E_BAD_ARG;
    if (D != b->D) {  // batch.rs:622, 829
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0) return INNR_OK;  // batch.rs:624-629, 831-836
    const size_t kout = std::min(k, b->N);
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    if (kout > INNR_MAX_K) {
        // More results than a candidate list holds: the reference's own algorithm on the device -- every distance (in the
        // caller's dimension order for batch_knn_reordered, batch.rs:640-648), a full sort of (distance, index) with the
        // vectors that do not pass the predicate keyed last (batch.rs:839-849), truncate to min(k, passing).
        const size_t N = b->N, ldq = round_up(D ? D : 1, 4);
        size_t tmp_bytes = 0, npass = N;
        INNR_HIP_CHECK(full_sort_scratch_bytes(N, &tmp_bytes));
        INNR_TRY(c->q_one.ensure(ldq * sizeof(float)));
        INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
        INNR_TRY(c->sort_keys.ensure((N + full_topk_out_capacity(kout)) * sizeof(uint64_t)));
        INNR_TRY(c->sort_tmp.ensure(std::max<size_t>(tmp_bytes, 16)));
        INNR_HIP_CHECK(hipMemsetAsync(c->q_one.p, 0, ldq * sizeof(float), c->stream));
        if (D) INNR_HIP_CHECK(copy_in(c, c->q_one.p, q, D * sizeof(float)));
        const uint8_t* dmask = nullptr;
        if (mask) {
            INNR_TRY(c->tmp_norms.ensure(b->ldN));
            INNR_HIP_CHECK(hipMemsetAsync(c->tmp_norms.p, 0, b->ldN, c->stream));
            INNR_HIP_CHECK(copy_in(c, c->tmp_norms.p, mask, N));
            dmask = c->tmp_norms.as<uint8_t>();
            npass = 0;
            for (size_t i = 0; i < N; ++i) npass += mask[i] ? 1 : 0;
        }
        const size_t nchunks = b->ldN / kScanChunk;
        const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
        if (order_host) {
            INNR_TRY(c->misc.ensure(std::max<size_t>(D, 1) * sizeof(uint32_t)));
            INNR_HIP_CHECK(copy_in(c, c->misc.p, order_host, D * sizeof(uint32_t)));
            scan_scores_kernel<1, true, false, true><<<blocks, kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)D, c->q_one.as<float>(), ldq, nullptr, nullptr, c->scores.as<float>(), b->ldN,
                c->misc.as<uint32_t>());
        } else {
            scan_scores_kernel<1, true, false><<<blocks, kScanThreads, 0, c->stream>>>(
                b->V, b->ldN, (uint32_t)D, c->q_one.as<float>(), ldq, nullptr, nullptr, c->scores.as<float>(), b->ldN);
        }
        INNR_HIP_CHECK(hipGetLastError());
        uint64_t* keys = c->sort_keys.as<uint64_t>();
        const size_t n = std::min(kout, npass);
        INNR_HIP_CHECK(full_sort_scores(c->scores.as<float>(), N, true, keys, keys + N, c->sort_tmp.p, tmp_bytes, c->stream, dmask, n));
        if (n) {
            INNR_TRY(c->out_idx.ensure(n * sizeof(uint64_t)));
            INNR_TRY(c->out_score.ensure(n * sizeof(float)));
            INNR_TRY(emit_results(c, keys + N, 0, 1, n, true, b->index_base, c->out_idx.as<uint64_t>(), c->out_score.as<float>()));
            INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, n * sizeof(uint64_t)));
            INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, n * sizeof(float)));
        }
        INNR_HIP_CHECK(ctx_sync(c));
        *out_k = n;
        return INNR_OK;
    }
    INNR_TRY(c->q_row.ensure(std::max<size_t>(D, 1) * sizeof(float)));
    INNR_TRY(c->out_idx.ensure(kout * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(kout * sizeof(float)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, q, D * sizeof(float)));
    ScanExt ext;
    if (mask) {
        INNR_TRY(c->tmp_norms.ensure(b->ldN));  // reused as the predicate byte array, zero padded
        INNR_HIP_CHECK(hipMemsetAsync(c->tmp_norms.p, 0, b->ldN, c->stream));
        INNR_HIP_CHECK(copy_in(c, c->tmp_norms.p, mask, b->N));
        ext.mask = c->tmp_norms.as<uint8_t>();
    }
    if (order_host) {
        INNR_TRY(c->misc.ensure(std::max<size_t>(D, 1) * sizeof(uint32_t)));
        INNR_HIP_CHECK(copy_in(c, c->misc.p, order_host, D * sizeof(uint32_t)));
        ext.order = c->misc.as<uint32_t>();
    }
    INNR_TRY(knn_exact_range(b, INNR_METRIC_L2SQ, c->q_row.as<float>(), D, nullptr, 0, 1, kout, c->out_idx.as<uint64_t>(),
                             c->out_score.as<float>(), ext));
    uint32_t have = 0;  // filtered: fewer than k vectors may pass (k = k.min(num_passing), batch.rs:849)
    INNR_HIP_CHECK(copy_out(c, &have, c->sel_cnt.p, sizeof(have)));
    INNR_TRY(check_errflag(c));
    const size_t n = std::min<size_t>(kout, have);
    if (n) {
        INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, n * sizeof(uint64_t)));
        INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, n * sizeof(float)));
        INNR_HIP_CHECK(ctx_sync(c));
    }
    *out_k = n;
    return INNR_OK;
}

innr_status innr_batch_knn_filtered(innr_batch* b, const float* q, size_t D, size_t k, const uint8_t* mask,
                                    uint64_t* out_idx, float* out_score, size_t* out_k) {
    if (b && b->N && !mask) {
        set_error("mask is null");
        return INNR_E_BAD_ARG;
    }
    return knn_l2_ext(b, q, D, k, mask, nullptr, out_idx, out_score, out_k);
}

innr_status innr_batch_knn_reordered(innr_batch* b, const float* q, size_t D, size_t k, uint64_t* out_idx,
                                     float* out_score, size_t* out_k) {
    if (!b) return INNR_E_BAD_ARG;
    std::vector<uint32_t> order(b->D);
    if (b->D && b->N && k && D == b->D) {
        std::vector<float> var(b->D);
        INNR_TRY(innr_batch_dimension_variance(b, var.data()));
        for (size_t d = 0; d < b->D; ++d) order[d] = (uint32_t)d;
        // variance_order (batch.rs:599-603): stable sort of the dimensions by variance, descending total_cmp
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t c2) { return f32_ord(var[a]) > f32_ord(var[c2]); });
    }
    return knn_l2_ext(b, q, D, k, nullptr, b->D ? order.data() : nullptr, out_idx, out_score, out_k);
}

// ---- batch_knn_filtered for Q queries: compact, then search (kernels_select.h) ----------------------------
// The caller's mask (device, N bytes) normalised to 0/1 into c->flt_mask, counted per chunk and scanned (c->flt_scan: [nchunks]
// counts | [nchunks] offsets | total | differs): *npass, and *same = the cached selection was built from this very mask. One
// synchronise, for the two numbers.
static innr_status filter_mask(innr_batch* b, const uint8_t* d_mask, size_t* npass, bool* same) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kSelChunk;
    INNR_TRY(c->flt_mask.ensure(b->ldN));
    INNR_TRY(c->flt_scan.ensure((2 * nchunks + 2) * sizeof(uint32_t)));
    uint32_t* cnt = c->flt_scan.as<uint32_t>();
    uint32_t* tail = cnt + 2 * nchunks;
    INNR_HIP_CHECK(hipMemsetAsync(tail, 0, 2 * sizeof(uint32_t), c->stream));
    select_mask_kernel<<<(unsigned)((nchunks + 3) / 4), 256, 0, c->stream>>>(d_mask, (uint32_t)b->N, nchunks, c->flt_mask.as<uint8_t>(),
                                                                            b->fsel ? b->fsel_mask : nullptr, cnt, tail + 1);
    INNR_HIP_CHECK(hipGetLastError());
    // (one workgroup: at most (2^32 - 257) / 256 chunks, 16384 per thread, every sum below 2^32)
    exclusive_scan_kernel<<<1, 1024, 0, c->stream>>>(cnt, (uint32_t)nchunks, cnt + nchunks, tail);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t h[2] = {0, 0};
    INNR_HIP_CHECK(copy_out(c, h, tail, sizeof(h)));
    INNR_HIP_CHECK(ctx_sync(c));
    *npass = h[0];
    *same = b->fsel != nullptr && h[1] == 0;
    return INNR_OK;
}

// A new selection of the npass vectors c->flt_mask passes (filter_mask ran): the old one freed, the columns gathered in index order,
// the map written, the mask kept. *built = false when it does not fit: the caller serves the call with the masked exact scan.
static innr_status build_selection(innr_batch* b, size_t npass, bool* built) {
    innr_ctx* c = b->ctx;
    *built = false;
    // The copy budget, for the store, the mask and the map (alloc_batch's and the two hipMallocs' sizes below) in the place of the
    // selection they replace. Not admitted: the selection of the last mask stays (the library frees nothing by itself), the
    // masked exact scan serves this call.
    // (a code batch's selection is a code batch with the parent's alpha and offset: alloc_batch_u8's size)
    const size_t store_bytes = b->C8 ? round_up(npass ? npass : 1, 1024) * round_up(b->D ? b->D : 1, 32)
                                     : round_up(npass ? npass : 1, 256) * round_up(b->D ? b->D : 1, 32) * sizeof(float);
    const size_t mask_bytes = b->ldN, map_bytes = npass * sizeof(uint32_t);
    if (!budget_admits(b, store_bytes + mask_bytes + map_bytes, corpus_copy_bytes(b))) return INNR_OK;
    free_selection(b);
    innr_batch* s = nullptr;
    const innr_status st = b->C8 ? alloc_batch_u8(c, npass, b->D, b->alpha, b->offset, &s) : alloc_batch(c, npass, b->D, &s);
    if (st == INNR_E_OOM) {
        (void)hipGetLastError();  // the failed hipMalloc must not surface at the next launch check
        return INNR_OK;
    }
    INNR_TRY(st);
    b->fsel = s;
    if (hipMalloc((void**)&b->fsel_mask, mask_bytes) != hipSuccess || hipMalloc((void**)&b->fsel_map, map_bytes) != hipSuccess) {
        (void)hipGetLastError();
        free_selection(b);
        return INNR_OK;
    }
    b->fsel_mask_bytes = mask_bytes;
    b->fsel_map_bytes = map_bytes;
    if (b->C8) {
        INNR_TRY(gather_passing_u8(b, s->C8, s->ldN, b->fsel_map));
    } else {
        INNR_TRY(gather_passing(b, s->V, s->ldN, b->fsel_map));
    }
    INNR_HIP_CHECK(hipMemcpyAsync(b->fsel_mask, c->flt_mask.p, b->ldN, hipMemcpyDeviceToDevice, c->stream));
    ++b->fsel_builds;
    *built = true;
    return INNR_OK;
}

// The masked exact scan on the batch itself (INNR_KNN_EXACT, or no room for a selection): scan_filter_kernel<..., EXT> with the
// normalised mask for every query, or beyond INNR_MAX_K all N scores of one query at a time and a full sort with the failing
// vectors keyed last (as knn_l2_ext does it). metric -1: a code batch -- scan_u8_filter_kernel<..., MASK>, or the masked full sort.
// kout <= npass.
static innr_status knn_masked_exact(innr_batch* b, int metric, const float* dQ, size_t Q, size_t D, size_t kout, size_t npass,
                                    uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats) {
    innr_ctx* c = b->ctx;
    const uint8_t* nm = c->flt_mask.as<uint8_t>();
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    const float* aux = nullptr;  // the per-query value: the norms for cosine, the sums for a code batch
    if (metric < 0) {
        INNR_TRY(c->q_norm.ensure(2 * round_up(Q, kBQmax) * sizeof(float)));
        float* qsum = c->q_norm.as<float>();
        query_sums_kernel<<<(unsigned)((Q + 63) / 64), 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)D, D, qsum, qsum + round_up(Q, kBQmax));
        INNR_HIP_CHECK(hipGetLastError());
        aux = qsum;
    } else if (metric == INNR_METRIC_COSINE) {
        INNR_TRY(ensure_norms(b));
        INNR_TRY(c->q_norm.ensure(Q * sizeof(float)));
        query_norms_kernel<<<(unsigned)Q, 64, 0, c->stream>>>(dQ, (uint32_t)Q, (uint32_t)D, D, c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        aux = c->q_norm.as<float>();
    }
    uint32_t kept;
    if (kout > INNR_MAX_K) {
        INNR_TRY(knn_full_sort(b, metric, dQ, D, aux, Q, kout, d_out_idx, d_out_score, nm));
        kept = (uint32_t)npass;
    } else {
        if (metric < 0) {
            INNR_TRY(knn_u8_exact_range(b, dQ, D, aux, 0, Q, kout, d_out_idx, d_out_score, 0, nm));
        } else {
            ScanExt ext;
            ext.mask = nm;
            INNR_TRY(knn_exact_range(b, metric, dQ, D, aux, 0, Q, kout, d_out_idx, d_out_score, ext));
        }
        kept = pick_kp(kout, 0);
    }
    return finish_knn(c, INNR_KNN_EXACT, kout, 0, kept, 0.0f, out_k, stats);
}

}  // extern "C"  (a template follows; the entry points get C linkage from the header)

// What innr_batch_knn_filtered_multi_dev and innr_batch_knn_u8_filtered_dev do once their arguments are checked: the mask, the
// selection, the search, the remap. knn(batch): the caller's engine on a batch (b itself, or its selection);
// masked(kout, npass): the masked exact scan on b.
template <class Knn, class Masked>
static innr_status knn_filtered_dev(innr_batch* b, size_t Q, size_t k, const uint8_t* d_mask, int engine, uint64_t* d_out_idx,
                                    size_t* out_k, innr_knn_stats* stats, Knn&& knn, Masked&& masked) {
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(hipEventRecord(c->ev[4], c->stream));
    size_t npass = 0;
    bool same = false;
    INNR_TRY(filter_mask(b, d_mask, &npass, &same));
    if (npass == 0) return INNR_OK;  // batch.rs:841-847
    const size_t kout = std::min(k, npass);  // batch.rs:849
    if (npass == b->N) {
        // every vector passes: the batch itself, no selection
        INNR_TRY(knn(b));
    } else {
        bool have = same;
        if (engine != INNR_KNN_EXACT && !same) INNR_TRY(build_selection(b, npass, &have));
        if (engine != INNR_KNN_EXACT && have) {
            // the selection's copies count against this batch's budget: it gets what this batch's copies and its own store leave
            const size_t used = corpus_copy_bytes(b) + selection_base_bytes(b);
            b->fsel->copy_budget = b->copy_budget == UINT64_MAX ? UINT64_MAX : (b->copy_budget > used ? b->copy_budget - used : 0);
            // the caller's engine on the selection (its own index_base is 0), then selection indices -> this batch's
            INNR_TRY(knn(b->fsel));
            const size_t n = Q * *out_k;
            if (n) {
                select_remap_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(d_out_idx, n, b->fsel_map, (uint32_t)npass,
                                                                                     b->index_base);
                INNR_HIP_CHECK(hipGetLastError());
            }
        } else {
            INNR_TRY(masked(kout, npass));
        }
    }
    INNR_HIP_CHECK(hipEventRecord(c->ev[5], c->stream));
    if (!c->tune.filter_keep_selection) free_selection(b);  // (synchronises)
    if (stats) {  // the whole call: mask, selection build, search, remap
        float ms = 0.0f;
        INNR_HIP_CHECK(hipEventSynchronize(c->ev[5]));
        if (hipEventElapsedTime(&ms, c->ev[4], c->ev[5]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}

extern "C" {

innr_status innr_batch_knn_filtered_multi_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D, size_t k,
                                              const uint8_t* d_mask, int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k,
                                              innr_knn_stats* stats) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !metric_ok(metric) || !out_k) {
        set_error("bad batch/metric/out_k");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // batch.rs:829
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0) return INNR_OK;  // batch.rs:831-836
    if (!d_mask) {
        set_error("mask is null");
        return INNR_E_BAD_ARG;
    }
    if (!d_queries || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    return knn_filtered_dev(
        b, Q, k, d_mask, engine, d_out_idx, out_k, stats,
        [&](innr_batch* on) { return innr_batch_knn_dev(on, metric, d_queries, Q, D, k, engine, d_out_idx, d_out_score, out_k, stats); },
        [&](size_t kout, size_t npass) {
            return knn_masked_exact(b, metric, d_queries, Q, D, kout, npass, d_out_idx, d_out_score, out_k, stats);
        });
}

innr_status innr_batch_knn_filtered_multi(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, size_t k,
                                          const uint8_t* mask, int engine, uint64_t* out_idx, float* out_score, size_t* out_k,
                                          innr_knn_stats* stats) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !metric_ok(metric) || !out_k) {
        set_error("bad batch/metric/out_k");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_k = 0;
    if (b->N == 0 || k == 0 || Q == 0) return INNR_OK;
    if (!mask) {
        set_error("mask is null");
        return INNR_E_BAD_ARG;
    }
    if (!queries && D) return INNR_E_BAD_ARG;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(c->flt_in.ensure(b->N));
    INNR_HIP_CHECK(hipMemcpyAsync(c->flt_in.p, mask, b->N, hipMemcpyHostToDevice, c->stream));
    return knn_from_host(c, queries, Q, D, std::min(k, b->N), out_idx, out_score, out_k, [&](const float* dQ, uint64_t* di, float* ds) {
        return innr_batch_knn_filtered_multi_dev(b, metric, dQ, Q, D, k, c->flt_in.as<uint8_t>(), engine, di, ds, out_k, stats);
    });
}

// ---- batch_knn_u8 over the vectors that pass a mask: innr_batch_knn_filtered_multi's scheme on a code batch ----
// the checks the two entry points share, in the reference's order (scalar.rs:376-378: an empty corpus or k == 0 before any dimension
// assert); *empty: nothing to search, *out_k stays 0
static innr_status knn_u8_filtered_args(innr_batch* b, size_t Q, size_t D, size_t k, const uint8_t* mask, size_t* out_k,
                                        innr_knn_stats* stats, bool* empty) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !b->C8 || !out_k) {
        set_error("this entry point needs a u8 code batch and out_k");
        return INNR_E_BAD_ARG;
    }
    *out_k = 0;
    *empty = true;
    if (b->N == 0 || k == 0) return INNR_OK;
    INNR_TRY(u8_check(b, D));
    if (Q == 0) return INNR_OK;
    if (!mask) {
        set_error("mask is null");
        return INNR_E_BAD_ARG;
    }
    *empty = false;
    return INNR_OK;
}

innr_status innr_batch_knn_u8_filtered_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, size_t k, const uint8_t* d_mask,
                                           int engine, uint64_t* d_out_idx, float* d_out_score, size_t* out_k, innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(knn_u8_filtered_args(b, Q, D, k, d_mask, out_k, stats, &empty));
    if (empty) return INNR_OK;
    if (!d_queries || !d_out_idx || !d_out_score) {
        set_error("queries / output buffers are null");
        return INNR_E_BAD_ARG;
    }
    return knn_filtered_dev(
        b, Q, k, d_mask, engine, d_out_idx, out_k, stats,
        [&](innr_batch* on) { return innr_batch_knn_u8_dev(on, d_queries, Q, D, k, engine, d_out_idx, d_out_score, out_k, stats); },
        [&](size_t kout, size_t npass) { return knn_masked_exact(b, -1, d_queries, Q, D, kout, npass, d_out_idx, d_out_score, out_k, stats); });
}

innr_status innr_batch_knn_u8_filtered(innr_batch* b, const float* queries, size_t Q, size_t D, size_t k, const uint8_t* mask, int engine,
                                       uint64_t* out_idx, float* out_score, size_t* out_k, innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(knn_u8_filtered_args(b, Q, D, k, mask, out_k, stats, &empty));
    if (empty) return INNR_OK;
    if ((!queries && D) || !out_idx || !out_score) {
        set_error("queries / output buffers are null");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_TRY(c->flt_in.ensure(b->N));
    INNR_HIP_CHECK(hipMemcpyAsync(c->flt_in.p, mask, b->N, hipMemcpyHostToDevice, c->stream));
    return knn_from_host(c, queries, Q, D, std::min(k, b->N), out_idx, out_score, out_k, [&](const float* dQ, uint64_t* di, float* ds) {
        return innr_batch_knn_u8_filtered_dev(b, dQ, Q, D, k, c->flt_in.as<uint8_t>(), engine, di, ds, out_k, stats);
    });
}

// ---- device memory: report, release, prebuild, budget (the accounting lives beside copy_fits) ------------------------------
innr_status innr_batch_memory(const innr_batch* b, uint64_t* corpus_bytes, uint64_t* aux, uint64_t* derived, uint32_t* present_mask) {
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(b->ctx);  // host bookkeeping only: no device is bound, no HIP call made
    if (corpus_bytes) *corpus_bytes = b->is_view ? 0 : b->corpus_bytes;
    if (aux) *aux = b->aux_bytes;
    if (derived) *derived = derived_bytes(b);
    if (present_mask) {
        uint32_t m = b->fsel ? INNR_COPY_SELECTION : 0u;
        for (int k = 0; k < kCopyKinds; ++k)
            if (b->copy[k].p) m |= copy_bit(k);
        *present_mask = m;
    }
    return INNR_OK;
}

innr_status innr_batch_copy_bytes(const innr_batch* b, uint32_t mask, uint64_t* bytes) {
    if (!b || !bytes) {
        set_error("batch or bytes is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(b->ctx);
    *bytes = derived_bytes(b, mask);
    return INNR_OK;
}

innr_status innr_batch_set_copy_budget(innr_batch* b, uint64_t bytes) {
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(b->ctx);
    b->copy_budget = bytes;
    return INNR_OK;
}

innr_status innr_batch_get_copy_budget(const innr_batch* b, uint64_t* bytes) {
    if (!b || !bytes) {
        set_error("batch or bytes is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(b->ctx);
    *bytes = b->copy_budget;
    return INNR_OK;
}

// the kinds of `mask` freed and their refusals forgotten (the stream is synchronised: nothing queued reads them);
// innr_batch_release_copies, and invalidate_derived for every kind
static void release_copy_kinds(innr_batch* b, uint32_t mask) {
    if (mask & INNR_COPY_BF16_DOT) mask |= INNR_COPY_BF16LO_DOT;  // the split filter needs the pair
    if (mask & INNR_COPY_BF16_COS) mask |= INNR_COPY_BF16LO_COS;
    for (int k = 0; k < kCopyKinds; ++k) {
        if (!(mask & copy_bit(k))) continue;
        CorpusCopy& cc = b->copy[k];
        if (cc.p) (void)hipFree(cc.p);
        cc.p = nullptr;
        cc.bytes = 0;
        cc.nk = 0;
        cc.limb_max = -1.0f;
        cc.refused = false;  // "try again": the next call that wants the copy asks the memory rule anew (weak is about the data: kept)
    }
    if (mask & INNR_COPY_SELECTION) free_selection(b);
}

innr_status innr_batch_release_copies(innr_batch* b, uint32_t mask) {
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));  // nothing queued may still read what is freed below
    release_copy_kinds(b, mask);
    return INNR_OK;
}

innr_status innr_batch_build_copies(innr_batch* b, uint32_t mask, uint32_t* built_mask) {
    if (built_mask) *built_mask = 0;
    if (!b) {
        set_error("batch is null");
        return INNR_E_BAD_ARG;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    mask &= INNR_COPY_ALL & ~INNR_COPY_SELECTION;  // (no mask to select with)
    const auto wants = [&](CopyKind k) { return (mask & copy_bit(k)) && !b->copy[k].p; };
    const int metrics[3] = {INNR_METRIC_DOT, INNR_METRIC_COSINE, INNR_METRIC_L2SQ};
    if (b->N && b->D && b->C8) {
        // a code batch has one derived copy: the K-packed signed codes of its int8 engine
        if (wants(kCopyI8Dot) && i8_eligible(b, 1) && budget_admits(b, u8_i8_copy_bytes(b))) INNR_TRY(ensure_i8_corpus(b));
    } else if (b->N && b->D && b->V) {
        if (wants(kCopyRows) && budget_admits(b, rows_copy_bytes(b))) {
            bool have = false;
            INNR_TRY(ensure_rowmajor(b, &have, false));
        }
        if (gemm_addressable(b, 1)) {  // (a view whose length is no multiple of 32 has no matrix-pipe engine)
            INNR_TRY(ensure_norms(b));
            const float mn = b->max_norm;
            const bool mfin = mn - mn == 0.0f;
            for (int metric : metrics) {  // the gates are choose_f32_filter's and knn_f32_i8's
                const bool cos = metric == INNR_METRIC_COSINE, l2 = metric == INNR_METRIC_L2SQ;
                const CopyKind hk = bf16_kind(metric);
                const size_t bytes = bf16_copy_bytes(b, hk);
                const bool bf_ok = mfin && mn >= 1e-12f && (!l2 || mn <= 1e15f);
                if (wants(hk) && bf_ok && budget_admits(b, bytes)) {
                    if (cos) INNR_TRY(ensure_invnorms(b));
                    if (l2) INNR_TRY(ensure_sqnorms(b));
                    INNR_TRY(ensure_bf16_corpus(b, hk));
                }
                // a lo-limb kind brings its partner: the budget has to admit what is missing of the pair
                if (!l2 && wants(bf16_kind(metric, true)) && mfin && mn >= 1e-12f && mn <= 1e18f &&
                    budget_admits(b, (b->copy[hk].p ? 0 : bytes) + bytes)) {
                    if (cos) INNR_TRY(ensure_invnorms(b));
                    INNR_TRY(ensure_bf16_corpus(b, hk));
                    INNR_TRY(ensure_bf16_lo(b, metric, false));
                    INNR_TRY(ensure_limb_maxima(b, metric));
                }
                if (wants(i8_kind(metric)) && f32_i8_eligible(b, metric, 1, 1) && budget_admits(b, f32_i8_copy_bytes(b, metric))) {
                    bool usable = false;
                    INNR_TRY(ensure_f32_i8_filter(b, metric, &usable));
                }
            }
        }
    }
    if (built_mask)
        for (int k = 0; k < kCopyKinds; ++k)
            if ((mask & copy_bit(k)) && b->copy[k].p) *built_mask |= copy_bit(k);
    return INNR_OK;
}

innr_status innr_ctx_memory(innr_ctx* c, uint64_t* workspace_bytes) {
    if (!c) {
        set_error("ctx is null");
        return INNR_E_BAD_ARG;
    }
    CtxGuard _guard(c);
    size_t sum = 0;
    for (const DevBuf* buf : workspace_bufs(c)) sum += buf->bytes;
    if (workspace_bytes) *workspace_bytes = sum;
    return INNR_OK;
}

innr_status innr_ctx_trim(innr_ctx* c) {
    if (!c) {
        set_error("ctx is null");
        return INNR_E_BAD_ARG;
    }
    INNR_ENTER(c);
    INNR_HIP_CHECK(ctx_sync(c));
    for (DevBuf* buf : workspace_bufs(c))
        if (buf != &c->flags) buf->release();  // (flags: set up once in innr_ctx_create, see workspace_bufs)
    return INNR_OK;
}

innr_status innr_batch_l2_squared_pruning(innr_batch* b, const float* q, size_t D, float threshold, uint64_t* out_idx,
                                          float* out_dist, size_t cap, size_t* out_n) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch: use the *_u8 functions)");
        return INNR_E_BAD_ARG;
    }
    if (!b || !out_n) return INNR_E_BAD_ARG;
    if (D != b->D) {  // batch.rs:325
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_n = 0;
    if (b->N == 0) return INNR_OK;
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    // full exact distances on the device (bit-identical to batch_l2_squared) ...
    const size_t ldq = round_up(D ? D : 1, 4);
    INNR_TRY(c->q_row.ensure(ldq * sizeof(float)));
    INNR_TRY(c->scores.ensure(b->ldN * sizeof(float)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, q, D * sizeof(float)));
    const size_t nchunks = b->ldN / kScanChunk;
    const unsigned blocks = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 8);
    scan_scores_kernel<1, true, false><<<blocks, kScanThreads, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, c->q_row.as<float>(),
                                                                               ldq, nullptr, nullptr, c->scores.as<float>(), b->ldN);
    INNR_HIP_CHECK(hipGetLastError());
    // ... then the survivors, in index order
    const uint32_t nb = (uint32_t)((b->N + 255) / 256);
    INNR_TRY(c->counts.ensure(((size_t)nb * 2 + 1) * sizeof(uint32_t)));
    uint32_t* cnt = c->counts.as<uint32_t>();
    uint32_t* off = cnt + nb;
    uint32_t* total = off + nb;
    prune_count_kernel<<<nb, 256, 0, c->stream>>>(c->scores.as<float>(), (uint32_t)b->N, threshold, cnt);
    exclusive_scan_kernel<<<1, 1024, 0, c->stream>>>(cnt, nb, off, total);
    INNR_HIP_CHECK(hipGetLastError());
    uint32_t n = 0;
    INNR_HIP_CHECK(copy_out(c, &n, total, sizeof(n)));
    INNR_HIP_CHECK(ctx_sync(c));
    *out_n = n;  // survivors found; the caller's buffers hold min(n, cap) of them
    const size_t m = std::min<size_t>(n, cap);
    if (m == 0) return INNR_OK;
    if (!out_idx || !out_dist) return INNR_E_BAD_ARG;
    INNR_TRY(c->out_idx.ensure(m * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(m * sizeof(float)));
    prune_scatter_kernel<<<nb, 256, 0, c->stream>>>(c->scores.as<float>(), (uint32_t)b->N, threshold, off, b->index_base,
                                                   c->out_idx.as<uint64_t>(), c->out_score.as<float>(), (uint32_t)m);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, m * sizeof(uint64_t)));
    INNR_HIP_CHECK(copy_out(c, out_dist, c->out_score.p, m * sizeof(float)));
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

innr_status innr_merge_topk_dev(innr_ctx* ctx, int metric, const uint64_t* d_idx, const float* d_score, size_t G,
                                size_t Q, size_t kin, size_t kout, uint64_t* d_out_idx, float* d_out_score) {
    if (!ctx || !metric_ok(metric) || !d_idx || !d_score || !d_out_idx || !d_out_score) return INNR_E_BAD_ARG;
    if (Q == 0 || kout == 0) return INNR_OK;
    if (kout > G * kin) {
        set_error("merge: kout=%zu > G*kin=%zu", kout, G * kin);
        return INNR_E_BAD_ARG;
    }
    INNR_ENTER(ctx);
    merge_topk_kernel<<<(unsigned)Q, 64, 0, ctx->stream>>>(d_idx, d_score, (uint32_t)G, (uint32_t)Q, (uint32_t)kin,
                                                          (uint32_t)kout, metric == INNR_METRIC_L2SQ, d_out_idx,
                                                          d_out_score);
    INNR_HIP_CHECK(hipGetLastError());
    INNR_HIP_CHECK(ctx_sync(ctx));
    return INNR_OK;
}

}  // extern "C"

// ---- what the entry points that change a batch in place (mutate.hip) take from this unit ---------------------
namespace innr {

innr_status count_mask(innr_batch* b, const uint8_t* d_mask, size_t* npass) {
    bool same = false;
    return filter_mask(b, d_mask, npass, &same);
}

// (count_mask or filter_mask ran on this batch: c->flt_mask, and the chunk offsets behind the counts in c->flt_scan)
innr_status gather_passing(innr_batch* b, float* S, size_t ldS, uint32_t* map) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kSelChunk;
    const uint32_t* off = c->flt_scan.as<uint32_t>() + nchunks;
    const size_t D = b->D;
    const uint32_t slab = (uint32_t)std::max<size_t>(kSelSlab, (D + 65534) / 65535);
    const dim3 grid((unsigned)((nchunks + 3) / 4), (unsigned)std::max<size_t>(1, (D + slab - 1) / slab));
    select_gather_kernel<<<grid, 256, 0, c->stream>>>(b->V, b->ldN, (uint32_t)D, c->flt_mask.as<uint8_t>(), off, nchunks, S, ldS, map, slab);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// ... and for a code batch (mutate_u8.hip): the same chunks, counts and offsets, select_gather_u8_kernel
innr_status gather_passing_u8(innr_batch* b, uint8_t* S, size_t ldS, uint32_t* map) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kSelChunk;
    const uint32_t* off = c->flt_scan.as<uint32_t>() + nchunks;
    const size_t D = b->D;
    const uint32_t slab = (uint32_t)std::max<size_t>(kSelSlab, (D + 65534) / 65535);
    const dim3 grid((unsigned)((nchunks + 3) / 4), (unsigned)std::max<size_t>(1, (D + slab - 1) / slab));
    select_gather_u8_kernel<<<grid, 256, 0, c->stream>>>(b->C8, b->ldN, (uint32_t)D, c->flt_mask.as<uint8_t>(), off, nchunks, S, ldS, map,
                                                         slab);
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// codes[n][D] (device, row-major) into columns col0 .. col0 + n of a code store (transpose_rows_u8_kernel, the upload's launch):
// only d < D, i < n is written, byte by byte
hipError_t transpose_codes_into(innr_ctx* c, const uint8_t* d_codes, size_t n, size_t D, uint8_t* C8, size_t ldN, size_t col0) {
    if (n == 0 || D == 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 31) / 32), (unsigned)((D + 31) / 32));
    transpose_rows_u8_kernel<<<grid, 256, 0, c->stream>>>(d_codes, (uint32_t)n, (uint32_t)D, C8, ldN, col0);
    return hipGetLastError();
}

void invalidate_derived(innr_batch* b) {
    release_copy_kinds(b, INNR_COPY_ALL);  // every copy[] kind and the kept selection
    for (CorpusCopy& cc : b->copy) cc.weak = false;  // (about the data that was: a release keeps it, new rows do not)
    if (b->norms) (void)hipFree(b->norms);
    if (b->invn) (void)hipFree(b->invn);
    if (b->sqn) (void)hipFree(b->sqn);
    if (b->max_norm_bits) (void)hipFree(b->max_norm_bits);
    b->norms = b->invn = b->sqn = nullptr;
    b->max_norm_bits = nullptr;
    b->aux_bytes = 0;
    b->norms_ready = false;
    b->max_norm = 0.0f;
    b->dimvar.clear();
    b->i8_raw = b->i8_norm = innr_batch::I8Range();
    b->i8l2_R = 0;
    b->i8l2_nmax = 0.0f;
    b->i8_weak_skips = 0;
    b->screen_share[0] = b->screen_share[1] = 0.0f;
    b->screen_skips[0] = b->screen_skips[1] = 0;
    b->auto_small_calls = 0;
}

}  // namespace innr

// =====================================================================================================================
// Range search: every vector within a per-query threshold (innr_batch_range_search)
// =====================================================================================================================
namespace innr {

// Smallest batch INNR_KNN_AUTO sends through the collect pass: the smallest measured batch from which the collect path beats the
// exact scan on both shapes by more than the spread of the repeats (tools/bench_range.py q0, squared L2, thresholds at the 100th best;
// whole call, ms, exact / collect; profiles/range_search_*.txt):
//      Q      1M x 128      10M x 768
//     16    0.42 / 0.69    14.9 / 27.0
//     32    0.73 / 0.75    28.0 / 27.2
//     64    1.25 / 0.78    53.6 / 27.2
//    128    2.40 / 0.92   104.4 / 27.7
constexpr size_t kRangeAutoQ0 = 64;
// Queries per round: their chunk counts, and on the collect path their bitmaps, lists and composites, stay within this
// (10M vectors: ~2.2 MB per query on the collect path); never more than 4096 per collect launch
constexpr size_t kRangeWorkspace = (size_t)2 << 30;
constexpr size_t kRangeMaxRound = 4096;
// Host-memory entry point: result staging up to this size is allocated for the caller's cap as it is; beyond it a count-only pass sizes it
constexpr size_t kRangeStageDirect = (size_t)256 << 20;

struct RangeScan {  // one launch of range_scan_kernel: nq queries (row-major, stride D) and where their counts / results go
    const float* Q;
    const float* qnorm;
    const float* thr;
    const uint32_t* qmap;
    uint32_t nq;
    uint32_t* cnt;
    size_t ldc;
    const uint64_t* qoff;
    uint64_t* out_idx;
    float* out_score;
    uint64_t cap;
};

// A range search on device memory, f32 or code corpus: rounds of at most kRangeMaxRound queries -- the collect path where it serves
// the call (one filter launch, exact scores of what it collected, the predicate on those bits; queries it cannot prove are redone by
// the exact scan through a query map), else the exact scan for every query: a count launch, offsets, an emit launch. The policy P
// (RangeF32, RangeU8) has what depends on the kind of corpus:
//   kChunk, kRoundExtra, kEngine   vectors per count, bytes of per-query values per round, the engine the collect path reports
//   l2                             smaller is better
//   wants_collect(Q, engine, &collect, &nfallback)   whether the collect path serves the call (and what that needs: norms, a copy)
//   carve(round)                   its per-query values in c->q_norm, for a round of that many queries
//   prepare(collect, Qp, nq, &a)   those values for a round's queries; a.qnorm where the exact scan serves them all
//   collect(Qp, thr, nq, lg, ldb, cnt, ldc, bad)     the collect step up to and including range_mark_kernel
//   scan<EMIT>(a)                  one launch of the exact scan
template <class P>
static innr_status range_search_rounds(P& p, innr_batch* b, const float* dQ, size_t Q, const float* dThr, int engine, uint64_t* d_off,
                                       uint64_t* d_idx, float* d_sc, size_t cap, size_t* out_total, innr_knn_stats* stats) {
    innr_ctx* c = b->ctx;
    const size_t D = b->D, nchunks = b->ldN / P::kChunk, ldc = nchunks + 1, ldb = b->ldN / 32;
    uint32_t nfallback = 0, kept = 0;
    float gemm_ms = 0.0f;
    bool collect = false;
    INNR_TRY(p.wants_collect(Q, engine, &collect, &nfallback));
    const size_t per_query = (ldc + 2) * sizeof(uint32_t) + P::kRoundExtra +
                             (collect ? ldb * sizeof(uint32_t) + (size_t)kCollectCap * (sizeof(uint32_t) + sizeof(uint64_t)) : 0);
    const size_t round = std::min(Q, std::max<size_t>(1, std::min(kRangeMaxRound, kRangeWorkspace / per_query)));
    INNR_TRY(c->rs_cnt.ensure(round * ldc * sizeof(uint32_t)));
    INNR_TRY(c->rs_tot.ensure(2 * round * sizeof(uint32_t)));
    INNR_TRY(p.carve(round));
    if (collect) INNR_TRY(c->rs_bits.ensure(round * ldb * sizeof(uint32_t)));
    uint32_t* cnt = c->rs_cnt.as<uint32_t>();
    uint32_t* tot = c->rs_tot.as<uint32_t>();
    uint32_t* bad = tot + round;
    INNR_HIP_CHECK(hipMemsetAsync(c->flags.p, 0, 4096, c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[0], c->stream));
    INNR_HIP_CHECK(hipMemsetAsync(d_off, 0, sizeof(uint64_t), c->stream));  // the running base, carried in the offsets themselves
    if (!collect) INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
    for (size_t q0 = 0; q0 < Q; q0 += round) {
        const size_t nq = std::min(round, Q - q0);
        const float* Qp = dQ + q0 * D;
        const float* thr = dThr + q0;
        uint64_t* off = d_off + q0;
        // the queries the exact scan serves: all of them, or after a collect pass the bad ones (gathered, with a map to their rows)
        RangeScan a = {Qp, nullptr, thr, nullptr, (uint32_t)nq, cnt, ldc, off, d_idx, d_sc, (uint64_t)cap};
        INNR_TRY(p.prepare(collect, Qp, nq, &a));
        const dim3 lg(kCollectCap / 256, (unsigned)nq);  // (blocks beyond a query's list length return at once)
        if (collect) {
            INNR_TRY(p.collect(Qp, thr, nq, lg, ldb, cnt, ldc, bad));
            // which queries the exact scan finishes, and how long the lists got (one synchronisation per round)
            std::vector<uint32_t> hb(2 * nq);
            INNR_HIP_CHECK(hipMemcpyAsync(hb.data(), bad, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            INNR_HIP_CHECK(hipMemcpyAsync(hb.data() + nq, c->counts.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            INNR_HIP_CHECK(hipStreamSynchronize(c->stream));
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) gemm_ms += ms;
            std::vector<uint32_t> redo;
            for (size_t j = 0; j < nq; ++j) {
                if (hb[j]) redo.push_back((uint32_t)j);
                kept = std::max(kept, std::min(hb[nq + j], kCollectCap));
            }
            nfallback += (uint32_t)redo.size();
            a.nq = (uint32_t)redo.size();
            if (a.nq) {  // gathered: their rows (rb.q), thresholds (rb.qn) and per-query values (rb.sc); rb.map = the rows of cnt / off
                innr_ctx::RedoBufs& rb = c->cmpl;
                INNR_TRY(upload_redo(c, rb, redo, D, 1));
                const uint32_t* map = rb.map.as<uint32_t>();
                gather_rows_kernel<<<(unsigned)(((size_t)a.nq * D + 255) / 256), 256, 0, c->stream>>>(Qp, map, a.nq, (uint32_t)D, rb.q.as<float>());
                gather_f32_kernel<<<(a.nq + 255) / 256, 256, 0, c->stream>>>(thr, map, a.nq, rb.qn.as<float>());
                // (the exact norms the collect pass left, or the sums: either way the round's first values of q_norm)
                gather_f32_kernel<<<(a.nq + 255) / 256, 256, 0, c->stream>>>(c->q_norm.as<float>(), map, a.nq, rb.sc.as<float>());
                INNR_HIP_CHECK(hipGetLastError());
                a.Q = rb.q.as<float>();
                a.thr = rb.qn.as<float>();
                a.qnorm = rb.sc.as<float>();
                a.qmap = map;
            }
        }
        if (a.nq) INNR_TRY(p.template scan<false>(a));
        range_chunk_scan_kernel<<<(unsigned)nq, 1024, 0, c->stream>>>(cnt, ldc, (uint32_t)nchunks, tot);
        range_offsets_kernel<<<1, 1024, 0, c->stream>>>(tot, (uint32_t)nq, off);
        INNR_HIP_CHECK(hipGetLastError());
        if (cap == 0) continue;  // a count-only call
        if (a.nq) INNR_TRY(p.template scan<true>(a));
        if (collect) {
            range_scatter_kernel<P::kChunk><<<lg, 256, 0, c->stream>>>(c->sort_keys.as<uint64_t>(), c->counts.as<uint32_t>(), kCollectCap, p.l2,
                                                                       c->rs_bits.as<uint32_t>(), ldb, cnt, ldc, bad, off, b->index_base, d_idx,
                                                                       d_sc, (uint64_t)cap);
            INNR_HIP_CHECK(hipGetLastError());
        }
    }
    if (!collect) INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
    INNR_HIP_CHECK(hipEventRecord(c->ev[1], c->stream));
    uint64_t total = 0;
    INNR_HIP_CHECK(copy_out(c, &total, d_off + Q, sizeof(total)));
    INNR_TRY(check_errflag(c));  // (synchronises)
    *out_total = (size_t)total;
    if (stats) {
        float ms = 0.0f;
        if (!collect && hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) gemm_ms = ms;
        stats->engine = collect ? P::kEngine : INNR_KNN_EXACT;
        stats->queries_fallback = nfallback;
        stats->candidates_kept = kept;
        stats->gemm_ms = gemm_ms;
        if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) stats->total_ms = ms;
    }
    return INNR_OK;
}

// eight, four or one query per corpus pass, never more than there are queries (the kernel's last group ends on the last query)
template <bool EMIT>
static innr_status launch_range_scan(innr_batch* b, int metric, const RangeScan& a) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kScanChunk;
    const uint32_t qb = a.nq >= 8 ? 8 : (a.nq >= 4 ? 4 : 1);
    // waves per CU as the exact kNN scan (knn_exact_range): 16 for eight queries a pass, 24 below
    const unsigned bx = (unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * (qb == 8 ? 4 : 6));
    const dim3 grid(bx, (a.nq + qb - 1) / qb);
    dispatch([&](auto QB, auto met) {
        launch_kernel(c, Inst<kLaunchRangeScan, QB, met, EMIT>(), {grid, kScanThreads, 0, grid.y}, b->V, b->ldN, (uint32_t)b->N,
                      (uint32_t)b->D, a.Q, b->D, b->norms, a.qnorm, a.thr, a.qmap, a.nq, a.cnt, a.ldc, a.qoff, b->index_base, a.out_idx,
                      a.out_score, a.cap);
    }, one_of<8, 4, 1>(qb), metric_of(metric));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

struct RangeF32 {  // range_search_rounds on an f32 batch: the f32 collect pass (it serves the bf16 / int8 requests too)
    static constexpr int kChunk = kScanChunk;
    static constexpr size_t kRoundExtra = 0;
    static constexpr int kEngine = INNR_KNN_MFMA;
    innr_batch* b;
    int metric;
    bool cos, l2;

    innr_status wants_collect(size_t Q, int engine, bool* collect, uint32_t* nfallback) {
        *collect = engine != INNR_KNN_EXACT;
        if (engine == INNR_KNN_AUTO) *collect = Q >= kRangeAutoQ0;
        if (!gemm_addressable(b, std::min(Q, kRangeMaxRound)) || b->D == 0) *collect = false;
        if (*collect || cos) INNR_TRY(ensure_norms(b));
        if (*collect && !(b->max_norm >= 1e-12f && b->max_norm <= 1e18f)) {
            // the corpus' largest norm outside the range the filter's error bound is good for (non-finite values included)
            *collect = false;
            *nfallback = (uint32_t)Q;
        }
        return INNR_OK;
    }
    innr_status carve(size_t) { return INNR_OK; }  // (the collect pass sizes q_norm itself, prepare() for the exact scan)
    innr_status prepare(bool collect, const float* Qp, size_t nq, RangeScan* a) {
        if (collect || !cos) return INNR_OK;
        innr_ctx* c = b->ctx;
        INNR_TRY(c->q_norm.ensure(nq * sizeof(float)));
        query_norms_kernel<<<(unsigned)nq, 64, 0, c->stream>>>(Qp, (uint32_t)nq, (uint32_t)b->D, b->D, c->q_norm.as<float>());
        INNR_HIP_CHECK(hipGetLastError());
        a->qnorm = c->q_norm.as<float>();
        return INNR_OK;
    }
    innr_status collect(const float* Qp, const float* thr, size_t nq, dim3 lg, size_t ldb, uint32_t* cnt, size_t ldc, uint32_t* bad) {
        innr_ctx* c = b->ctx;
        INNR_TRY(collect_pass(b, metric, Qp, nq, 1, thr));
        bool rows = false;
        INNR_TRY(collect_rescore(b, metric, Qp, c->q_norm.as<float>(), nq, &rows));
        INNR_HIP_CHECK(hipMemsetAsync(c->rs_bits.p, 0, nq * ldb * sizeof(uint32_t), c->stream));
        INNR_HIP_CHECK(hipMemsetAsync(cnt, 0, nq * ldc * sizeof(uint32_t), c->stream));
        if (l2) range_mark_kernel<true><<<lg, 256, 0, c->stream>>>(c->sort_keys.as<uint64_t>(), c->counts.as<uint32_t>(), kCollectCap, thr, c->seed_score.as<uint32_t>(), c->q_norm.as<float>(), c->rs_bits.as<uint32_t>(), ldb, cnt, ldc, bad);
        else range_mark_kernel<false><<<lg, 256, 0, c->stream>>>(c->sort_keys.as<uint64_t>(), c->counts.as<uint32_t>(), kCollectCap, thr, c->seed_score.as<uint32_t>(), c->q_norm.as<float>(), c->rs_bits.as<uint32_t>(), ldb, cnt, ldc, bad);
        INNR_HIP_CHECK(hipGetLastError());
        return INNR_OK;
    }
    template <bool EMIT>
    innr_status scan(const RangeScan& a) { return launch_range_scan<EMIT>(b, metric, a); }
};

static innr_status range_search_dev(innr_batch* b, int metric, const float* dQ, size_t Q, const float* dThr, int engine,
                                    uint64_t* d_off, uint64_t* d_idx, float* d_sc, size_t cap, size_t* out_total,
                                    innr_knn_stats* stats) {
    RangeF32 p = {b, metric, metric == INNR_METRIC_COSINE, metric == INNR_METRIC_L2SQ};
    return range_search_rounds(p, b, dQ, Q, dThr, engine, d_off, d_idx, d_sc, cap, out_total, stats);
}

// the argument checks both entry points share; *empty: nothing to search, the offsets are all zero
static innr_status range_search_args(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, const float* thresholds,
                                     uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                     innr_knn_stats* stats, bool* empty) {
    if (b && !b->V) {
        set_error("this entry point needs an f32 batch (got a u8 code batch)");
        return INNR_E_BAD_ARG;
    }
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!b || !metric_ok(metric) || !out_total) {
        set_error("bad batch/metric/out_total");
        return INNR_E_BAD_ARG;
    }
    if (D != b->D) {  // batch.rs:325
        set_error("dimension mismatch: query.len()=%zu, batch.dimension=%zu", D, b->D);
        return INNR_E_DIM_MISMATCH;
    }
    *out_total = 0;
    if (!out_offsets || Q >= 0xFFFFFFFFull) {
        set_error("out_offsets is null, or more than 2^32 - 2 queries");
        return INNR_E_BAD_ARG;
    }
    *empty = b->N == 0 || Q == 0;
    if (*empty) return INNR_OK;
    if (!thresholds || (!queries && D) || (cap && (!out_idx || !out_score))) {
        set_error("thresholds / queries / output buffers are null");
        return INNR_E_BAD_ARG;
    }
    return INNR_OK;
}

// ---- range search on a u8 code batch (innr_batch_range_search_u8) ---------------------------------------------
// Smallest batch INNR_KNN_AUTO sends through the collect pass on the int8 matrix pipe (kRangeAutoQ0's rule: the smallest measured
// batch from which the collect path beats the exact scan on both shapes by more than the spread of the repeats; tools/bench_range.py
// u8, thresholds at the 100th best, the int8 copy in place; whole call, ms, exact / collect; profiles/range_search_u8_*.txt):
//      Q      1M x 128      10M x 768       50M x 768
//      8    0.23 / 0.22     4.89 /  1.60     16.6 /  6.44     (1M x 128: 0.23 .. 0.25 against 0.20 .. 0.22 -- within the spread)
//     16    0.33 / 0.23     8.59 /  1.63     30.6 /  6.50
//     32    0.54 / 0.25    16.46 /  1.73     58.4 /  6.76
//     64    0.95 / 0.27    30.97 /  1.86    113.7 /  7.49
//    128    1.71 / 0.40    59.63 /  2.22    224.5 /  9.94
//   1024   12.83 / 1.00   459.91 / 11.64   1774.8 / 69.76
constexpr size_t kRangeU8AutoQ0 = 16;

// the exact scan's two launches per round (a.qnorm: the queries' sums); qmap: see range_scan_u8_kernel
template <bool EMIT>
static innr_status launch_range_scan_u8(innr_batch* b, const RangeScan& a) {
    innr_ctx* c = b->ctx;
    const size_t nchunks = b->ldN / kU8Chunk;
    const uint32_t qb = a.nq >= 8 ? 8 : (a.nq >= 4 ? 4 : 1);  // never more than there are queries: the last group ends on the last query
    // waves per CU as the exact u8 kNN scan (knn_u8_exact_range): 16
    const dim3 grid((unsigned)std::min<size_t>((nchunks + 3) / 4, (size_t)c->num_cus * 4), (a.nq + qb - 1) / qb);
    dispatch([&](auto QB) {
        launch_kernel(c, Inst<kLaunchRangeScanU8, QB, EMIT>(), {grid, 256, 0, grid.y}, b->C8, b->ldN, (uint32_t)b->N, (uint32_t)b->D, a.Q,
                      b->D, a.qnorm, b->alpha / 255.0f, b->offset, a.thr, a.nq, a.cnt, a.ldc, a.qoff, b->index_base, a.out_idx, a.out_score,
                      a.cap, a.qmap);
    }, one_of<8, 4, 1>(qb));
    INNR_HIP_CHECK(hipGetLastError());
    return INNR_OK;
}

// Whether the collect pass serves a call: a known engine value other than EXACT, innr_batch_knn_u8's rules for the
// int8 engine, a corpus of at least range_u8_i8_min_n vectors, and the int8 copy -- there already, or built now: on an explicit
// request whenever the copy budget admits it, under AUTO only from kRangeU8AutoQ0 queries on and with room to spare (copy_fits).
// An allocation that fails leaves the call to the exact scan.
static innr_status range_u8_wants_collect(innr_batch* b, size_t Q, int engine, bool* collect) {
    innr_ctx* c = b->ctx;
    *collect = false;
    if (engine != INNR_KNN_AUTO && engine != INNR_KNN_MFMA && engine != INNR_KNN_MFMA_BF16 && engine != INNR_KNN_MFMA_I8) return INNR_OK;
    if (!i8_eligible(b, Q) || !gemm_addressable(b, std::min(Q, kRangeMaxRound))) return INNR_OK;
    if (c->tune.range_u8_i8_min_n > 0 && b->N < (size_t)c->tune.range_u8_i8_min_n) return INNR_OK;
    if (engine == INNR_KNN_AUTO && (Q < kRangeU8AutoQ0 || c->tune.u8_no_i8)) return INNR_OK;
    if (!b->copy[kCopyI8Dot].p) {
        const size_t copy_b = u8_i8_copy_bytes(b);
        if (!budget_admits(b, copy_b)) return INNR_OK;
        if (engine == INNR_KNN_AUTO) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || !copy_fits(free_b, copy_b)) return INNR_OK;
        }
        if (ensure_i8_corpus(b) != INNR_OK) {  // no memory for the copy: the exact scan needs none
            (void)hipGetLastError();
            return INNR_OK;
        }
    }
    *collect = true;
    return INNR_OK;
}

// range_search_rounds on a code batch. The collect path: one MODE 2 pass of the int8 filter per round with the fixed thresholds
// ord(thr_j - E_j) (E_j: rescore_u8_kernel's whole bound), exact scores of everything collected from the K-packed copy, the exact
// predicate on those bits, and the finish in index order. Queries without a finite collect threshold are closed before the launch
// and, like those whose list ran past kCollectCap, finished by the exact scan through a query map.
struct RangeU8 {
    static constexpr int kChunk = kU8Chunk;
    static constexpr size_t kRoundExtra = 2 * sizeof(float);
    static constexpr int kEngine = INNR_KNN_MFMA_I8;
    static constexpr bool l2 = false;
    innr_batch* b;
    float *qsum, *qnorm;  // the round's sums and norms: q_norm, [round] each

    innr_status wants_collect(size_t Q, int engine, bool* collect, uint32_t*) { return range_u8_wants_collect(b, Q, engine, collect); }
    innr_status carve(size_t round) {
        INNR_TRY(b->ctx->q_norm.ensure(2 * round * sizeof(float)));
        qsum = b->ctx->q_norm.as<float>();
        qnorm = qsum + round;
        return INNR_OK;
    }
    innr_status prepare(bool, const float* Qp, size_t nq, RangeScan* a) {
        query_sums_kernel<<<((uint32_t)nq + 63) / 64, 64, 0, b->ctx->stream>>>(Qp, (uint32_t)nq, (uint32_t)b->D, b->D, qsum, qnorm);
        INNR_HIP_CHECK(hipGetLastError());
        a->qnorm = qsum;
        return INNR_OK;
    }
    innr_status collect(const float* Qp, const float* thr, size_t nq, dim3 lg, size_t ldb, uint32_t* cnt, size_t ldc, uint32_t* bad) {
        innr_ctx* c = b->ctx;
        I8Plan p = plan_i8(b, kCopyI8Dot, nq, 1, 32u, /*one_limb=*/true);
        (void)plan_i8_small(b, &p, nq, false, /*collect=*/true);
        INNR_TRY(prep_queries_i8(b, p, Qp, nq, qsum, b->alpha, b->offset));
        const float* qc = c->misc.as<float>();
        // fixed thresholds: thr - E (one key lower); 0 = "no bound" where that is not finite -> closed, the exact scan's
        INNR_TRY(c->seed_score.ensure(p.Qpad * sizeof(uint32_t)));
        uint32_t* seed = c->seed_score.as<uint32_t>();
        seed_thresholds_u8_kernel<<<(unsigned)((p.Qpad + 255) / 256), 256, 0, c->stream>>>(thr, (uint32_t)nq, 1u, u8_filter_scale(b), qnorm, qsum, b->offset,
                                                                                       qc + 3 * p.Qpad, seed, (uint32_t)p.Qpad, 0u);
        range_close_unbounded_kernel<<<((uint32_t)nq + 255) / 256, 256, 0, c->stream>>>(seed, (uint32_t)nq);
        INNR_HIP_CHECK(hipGetLastError());
        // global lists: [Qpad][kCollectCap] indices, [Qpad] lengths
        INNR_TRY(c->lists.ensure(p.Qpad * (size_t)kCollectCap * sizeof(uint32_t)));
        INNR_TRY(c->counts.ensure(p.Qpad * sizeof(uint32_t)));
        INNR_TRY(c->sort_keys.ensure(nq * (size_t)kCollectCap * sizeof(uint64_t)));
        INNR_HIP_CHECK(hipMemsetAsync(c->counts.p, 0, p.Qpad * sizeof(uint32_t), c->stream));
        I8Plan pl = p;
        pl.KP = kCollectCap;  // what the kernel takes as the list capacity
        INNR_HIP_CHECK(hipEventRecord(c->ev[2], c->stream));
        INNR_TRY(launch_gemm_i8<2>(b, pl, nq, qc, nullptr, 0, seed));
        INNR_HIP_CHECK(hipEventRecord(c->ev[3], c->stream));
        collect_scores_u8_kernel<<<lg, 256, 0, c->stream>>>(reinterpret_cast<const uint4*>(p.corpus), p.nk, (uint32_t)b->D, Qp, qsum,
                                                            b->alpha / 255.0f, b->offset, c->lists.as<uint32_t>(), c->counts.as<uint32_t>(),
                                                            kCollectCap, c->sort_keys.as<uint64_t>());
        INNR_HIP_CHECK(hipMemsetAsync(c->rs_bits.p, 0, nq * ldb * sizeof(uint32_t), c->stream));
        INNR_HIP_CHECK(hipMemsetAsync(cnt, 0, nq * ldc * sizeof(uint32_t), c->stream));
        range_mark_kernel<false, (int)kU8Chunk, false><<<lg, 256, 0, c->stream>>>(c->sort_keys.as<uint64_t>(), c->counts.as<uint32_t>(), kCollectCap, thr,
                                                                                  seed, nullptr, c->rs_bits.as<uint32_t>(), ldb, cnt, ldc, bad);
        INNR_HIP_CHECK(hipGetLastError());
        return INNR_OK;
    }
    template <bool EMIT>
    innr_status scan(const RangeScan& a) { return launch_range_scan_u8<EMIT>(b, a); }
};

static innr_status range_search_u8_dev(innr_batch* b, const float* dQ, size_t Q, const float* dThr, int engine, uint64_t* d_off,
                                       uint64_t* d_idx, float* d_sc, size_t cap, size_t* out_total, innr_knn_stats* stats) {
    RangeU8 p = {b, nullptr, nullptr};
    return range_search_rounds(p, b, dQ, Q, dThr, engine, d_off, d_idx, d_sc, cap, out_total, stats);
}

// the argument checks both u8 entry points share: range_search_args' order with the batch test inverted
static innr_status range_search_u8_args(innr_batch* b, const float* queries, size_t Q, size_t D, const float* thresholds,
                                        uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                        innr_knn_stats* stats, bool* empty) {
    if (stats) memset(stats, 0, sizeof(*stats));
    INNR_TRY(u8_check(b, D));  // a null or f32 batch: INNR_E_BAD_ARG; then the dimension
    if (!out_offsets || !out_total || Q >= 0xFFFFFFFFull) {
        set_error("out_offsets / out_total is null, or more than 2^32 - 2 queries");
        return INNR_E_BAD_ARG;
    }
    *out_total = 0;
    *empty = b->N == 0 || Q == 0;
    if (*empty) return INNR_OK;
    if (!thresholds || (!queries && D) || (cap && (!out_idx || !out_score))) {
        set_error("thresholds / queries / output buffers are null");
        return INNR_E_BAD_ARG;
    }
    return INNR_OK;
}

// A range search on host memory: queries, thresholds and offsets staged on the device, and room for min(cap, Q * N) results. Where
// that room is large (beyond kRangeStageDirect bytes) a count-only pass comes first and the room shrinks to what the result needs: a
// generous cap costs a second search, not memory for results that do not exist. dev(dQ, dThr, d_off, d_idx, d_sc, room) searches.
// empty (the argument checks found nothing to search): the offsets are all zero.
template <class Dev>
static innr_status range_search_from_host(innr_batch* b, bool empty, const float* queries, size_t Q, size_t D, const float* thresholds,
                                          uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                          Dev&& dev) {
    if (empty) {
        memset(out_offsets, 0, (Q + 1) * sizeof(uint64_t));
        return INNR_OK;
    }
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    size_t room = std::min(cap, Q * b->N);
    INNR_TRY(c->q_row.ensure(std::max<size_t>(Q * D, 1) * sizeof(float)));
    INNR_TRY(c->rs_thr.ensure(Q * sizeof(float)));
    INNR_TRY(c->rs_off.ensure((Q + 1) * sizeof(uint64_t)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_HIP_CHECK(copy_in(c, c->rs_thr.p, thresholds, Q * sizeof(float)));
    if (room * (sizeof(uint64_t) + sizeof(float)) > kRangeStageDirect) {
        INNR_TRY(dev(c->q_row.as<float>(), c->rs_thr.as<float>(), c->rs_off.as<uint64_t>(), nullptr, nullptr, 0));
        room = std::min(room, *out_total);
    }
    INNR_TRY(c->out_idx.ensure(std::max<size_t>(room, 1) * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(std::max<size_t>(room, 1) * sizeof(float)));
    INNR_TRY(dev(c->q_row.as<float>(), c->rs_thr.as<float>(), c->rs_off.as<uint64_t>(), c->out_idx.as<uint64_t>(), c->out_score.as<float>(), room));
    INNR_HIP_CHECK(copy_out(c, out_offsets, c->rs_off.p, (Q + 1) * sizeof(uint64_t)));
    const size_t m = std::min<size_t>(*out_total, room);
    if (m) {
        INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, m * sizeof(uint64_t)));
        INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, m * sizeof(float)));
    }
    INNR_HIP_CHECK(ctx_sync(c));
    return INNR_OK;
}

// ... and on device memory: all-zero offsets where the argument checks found nothing to search, else dev() searches
template <class Dev>
static innr_status range_search_on_device(innr_batch* b, bool empty, size_t Q, uint64_t* d_out_offsets, Dev&& dev) {
    innr_ctx* c = b->ctx;
    INNR_ENTER(c);
    if (empty) {
        INNR_HIP_CHECK(hipMemsetAsync(d_out_offsets, 0, (Q + 1) * sizeof(uint64_t), c->stream));
        INNR_HIP_CHECK(ctx_sync(c));
        return INNR_OK;
    }
    return dev();
}

}  // namespace innr

extern "C" {

innr_status innr_batch_range_search_dev(innr_batch* b, int metric, const float* d_queries, size_t Q, size_t D, const float* d_thresholds,
                                        int engine, uint64_t* d_out_offsets, uint64_t* d_out_idx, float* d_out_score, size_t cap,
                                        size_t* out_total, innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(range_search_args(b, metric, d_queries, Q, D, d_thresholds, d_out_offsets, d_out_idx, d_out_score, cap, out_total, stats, &empty));
    return range_search_on_device(b, empty, Q, d_out_offsets, [&] {
        return range_search_dev(b, metric, d_queries, Q, d_thresholds, engine, d_out_offsets, d_out_idx, d_out_score, cap, out_total, stats);
    });
}

innr_status innr_batch_range_search(innr_batch* b, int metric, const float* queries, size_t Q, size_t D, const float* thresholds, int engine,
                                    uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                    innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(range_search_args(b, metric, queries, Q, D, thresholds, out_offsets, out_idx, out_score, cap, out_total, stats, &empty));
    return range_search_from_host(b, empty, queries, Q, D, thresholds, out_offsets, out_idx, out_score, cap, out_total,
                                  [&](const float* dQ, const float* dThr, uint64_t* d_off, uint64_t* d_idx, float* d_sc, size_t room) {
                                      return range_search_dev(b, metric, dQ, Q, dThr, engine, d_off, d_idx, d_sc, room, out_total, stats);
                                  });
}

innr_status innr_batch_range_search_u8_dev(innr_batch* b, const float* d_queries, size_t Q, size_t D, const float* d_thresholds, int engine,
                                           uint64_t* d_out_offsets, uint64_t* d_out_idx, float* d_out_score, size_t cap, size_t* out_total,
                                           innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(range_search_u8_args(b, d_queries, Q, D, d_thresholds, d_out_offsets, d_out_idx, d_out_score, cap, out_total, stats, &empty));
    return range_search_on_device(b, empty, Q, d_out_offsets, [&] {
        return range_search_u8_dev(b, d_queries, Q, d_thresholds, engine, d_out_offsets, d_out_idx, d_out_score, cap, out_total, stats);
    });
}

innr_status innr_batch_range_search_u8(innr_batch* b, const float* queries, size_t Q, size_t D, const float* thresholds, int engine,
                                       uint64_t* out_offsets, uint64_t* out_idx, float* out_score, size_t cap, size_t* out_total,
                                       innr_knn_stats* stats) {
    bool empty = false;
    INNR_TRY(range_search_u8_args(b, queries, Q, D, thresholds, out_offsets, out_idx, out_score, cap, out_total, stats, &empty));
    return range_search_from_host(b, empty, queries, Q, D, thresholds, out_offsets, out_idx, out_score, cap, out_total,
                                  [&](const float* dQ, const float* dThr, uint64_t* d_off, uint64_t* d_idx, float* d_sc, size_t room) {
                                      return range_search_u8_dev(b, dQ, Q, dThr, engine, d_off, d_idx, d_sc, room, out_total, stats);
                                  });
}

}  // extern "C"
