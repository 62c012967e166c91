// api_internal.h -- what more than one translation unit of the library shares: the context and its workspace, the launch record
// and dispatch, the corpus handles, the entry guard, and the host functions that cross a unit boundary. The units: api.hip (the C
// ABI, the kNN engines, range search, memory), maxsim.hip, adaptive.hip (batch_knn_adaptive), rows.hip (search by stored vector), mutate.hip and
// mutate_u8.hip (changing an f32 / a u8 code batch in place), comm.hip (the multi-GPU layer), sort_full.hip.
// Nothing here may depend on INNR_TEST_HOOKS: every object but api.o is linked into the product library and the hook library
// alike, so the struct layouts must be the same in every object.
#pragma once

#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "common.h"

namespace innr {

// A device buffer that only grows (workspace; never reallocated inside a steady-state call).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    innr_status ensure(size_t need) {
        if (need <= bytes) return INNR_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        INNR_HIP_CHECK(hipMalloc(&p, need));
        bytes = need;
        return INNR_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

}  // namespace innr

using namespace innr;

// Tuning / experiment switches of a context. Read from the environment ONCE, in innr_ctx_create (INNR_<NAME IN CAPITALS>), and
// changed afterwards only through innr_ctx_set_option: no entry point reads the environment on the call path.
struct innr_tuning {
    long gemm_waves = 0;         // force the f32 GEMM engine's block shape (1, 2, 4, 8 waves); 0 = by batch size
    long gemm_blocks_per_cu = 0; // resident blocks per CU of the f32 GEMM engine; 0 = by block shape
    long gemm_qt_group = 1;      // query tiles per XCD group (plan_gemm)
    long gemm_seed_n = 0;        // rows of the corpus prefix that seeds the chip-wide bounds; 0 = by engine
    long gemm_no_seed = 0;       // no threshold seeding
    long gemm_no_kp_retry = 0;   // unproven minority: straight to the exact engine, no second pass with longer lists
    long i8_two_limb = 0;        // batch_knn_u8 on the int8 pipe: both limbs on the matrix pipe (the cross-check kernel)
    long no_auto_bf16 = 0;       // INNR_KNN_AUTO never picks the bf16 filter
    long no_auto_i8 = 0;         // INNR_KNN_AUTO never picks the int8 filter for an f32 corpus
    long u8_no_i8 = 0;           // INNR_KNN_AUTO never picks the int8 engine for a code corpus
    long rescore_all = 0;        // re-score every candidate (no progressive rounds)
    long maxsim_generic = 0;     // maxsim MFMA engine: the generic kernel instead of the tile-unrolled one
    long no_k_rule = 0;          // chip-wide bounds by the KP rule only (topk_dev.h): A/B of the k rule
    long fail_local_search = 0;  // TEST switch of the sharded calls: this rank's local search reports a failure
    long no_completion = 0;      // unproven queries of the f32 engine: straight to the KP retry / exact engine (no completion pass)
    long trace = 0;              // diagnostics of the redo paths on stderr (list lengths of the completion pass, ...)
    long no_rows_copy = 0;       // never build the row-major copy: the completion pass re-scores by column gathers (what a full HBM does)
    long i8_slices_per_cu = 0;   // corpus slices (= blocks) per CU and query tile of the int8 filters; 0 = by metric (plan_i8)
    long i8_no_small = 0;        // never the small-batch int8 kernel (gemm_i8s_filter_kernel): A/B against the 512-query tile
    long i8_no_small4 = 0;       // ... never its four-column-tile form (65 .. 128 queries)
    long i8_small_max_q = 0;     // ... its largest batch (groups of 128 queries beyond 128); 0 = the default
    long i8_small_free = 0;      // ... its query groups run free (no soft lockstep): A/B
    long no_split_filter = 0;    // INNR_KNN_MFMA dot / cosine: filter on the f32 kernel, never the split-bf16 one (A/B, tests)
    long split_min_q = 0;        // ... smallest batch the split-bf16 filter takes; 0 = the measured crossover (kSplitMinQ)
    long no_split_screen = 0;    // ... 1: its full three-product K-loop, never the hi.hi loop with screened corrections; -1: always the screened loop; 0: by list length, batch size and the share of wave tiles the batch's last screened call corrected (A/B, tests); lists up to 64 beyond 2^20 padded queries always take the full loop (kPairMaxQpad)
    long split_seed_rows = 0;    // ... rows of the corpus prefix whose split scores (the seeder, MODE 3 of the split kernel) seed its chip-wide bounds under the k rule; 0 = the default (kSplitSeedRows), -1 = never (the exact seeder of the other filters), >= 1024 = that many; always clamped to a multiple of 1024 within N / 32, and the exact seeder where fewer than k groups of 32 rows remain or gemm_seed_n is set
    long split_screen_worst_case = 0;  // ... the screen's margin by the worst-case formula alone (every lo limb at half a last place), never from the limbs' measured norms (A/B, tests)
    long filter_keep_selection = 1;  // innr_batch_knn_filtered_multi, innr_batch_knn_u8_filtered: keep the selection of the last mask for the next call (0: free it at the end of each call)
    long copy_budget_mib = -1;   // the copy budget (MiB) a batch gets when it is created; < 0 = unlimited (innr_batch_set_copy_budget)
    long mutate_round = 0;       // innr_batch_append_rows, innr_batch_update_rows and their u8 twins (mutate_u8.hip): at most this many rows per staging round (tests); 0 = what fits 256 MiB
    long range_u8_i8_min_n = 65536;  // innr_batch_range_search_u8: fewest vectors of a code batch whose calls the collect pass on the int8 matrix pipe serves, for every engine value (below it a tile launch plus re-score costs more than the scans; tests of small shapes set 0)
    long scan_max_slots = 0;     // exact scans (f32, u8, maxsim's document filter): at most this many wave slots, so that a wave owns several chunks on a small corpus (tests); 0 = fill the chip
};

// One templated kernel launch of the filter and scan families, as its dispatch site chose it (innr_ctx::launch_log). Written by
// plain host stores in launch_kernel, in every build; read only by the test hooks (innrdbg_launch_log), which
// tests/test_gpu_kernel_variants.py decodes: its table names every instantiation a call may reach.
enum LaunchFamily {
    kLaunchGemmF32 = 1,    // gemm_filter_kernel<KIND, RR, MODE, WV>
    kLaunchGemmBf16 = 2,   // gemm_bf16_filter_kernel<RR, 0, 1>: args RR, MODE, LIMBS
    kLaunchGemmSplit = 3,  // gemm_bf16_filter_kernel<RR, MODE, 3>: args RR, MODE, LIMBS
    kLaunchI8One = 4,      // gemm_i8h_filter_kernel<RR, MODE>
    kLaunchI8Two = 5,      // gemm_i8_filter_kernel<RR, MODE>
    kLaunchI8Small = 6,    // gemm_i8s_filter_kernel<12, NK, CT, MODE>: args NK, CT, MODE
    kLaunchMsScan = 7,     // maxsim_scan_kernel<COS, NQ, MULTI>, once per pass
    kLaunchMsTile = 8,     // maxsim_mfma_tile_kernel<COS, NB, NQ>, once per pass
    kLaunchMsGeneric = 9,  // maxsim_mfma_kernel<COS>, once per pass
    kLaunchMsRerank = 10,  // maxsim_rerank_kernel<COS, NQ, MULTI>, once per pass
    kLaunchRangeScan = 11, // range_scan_kernel<QB, L2, COS, EMIT>: args QB, metric (INNR_METRIC_*), EMIT; groups = query groups
    kLaunchScanU8Masked = 12,  // scan_u8_filter_kernel<QB, R, true> (the masked exact scan of a code batch): args QB, R; groups = query groups
    kLaunchRangeScanU8 = 13,   // range_scan_u8_kernel<QB, EMIT>: args QB, EMIT; groups = query groups
};
// ... and one family outside the closed set above, which the readers of launch_log decode (tests pin it to 1 .. 13): the split
// filter's seeder over a corpus prefix, gemm_bf16_filter_kernel<6, 3, 3>: args RR, MODE, LIMBS. It runs in front of a gemm_split
// launch wherever seed_split serves (api.hip); the calls whose records are decoded name their exact prefix (gemm_seed_n) and
// never reach it.
enum LaunchFamilySeed { kLaunchSplitSeed = 14 };
struct LaunchRec {
    uint8_t family;    // LaunchFamily
    uint8_t lockstep;  // gemm_i8s_filter_kernel: the soft-lockstep `prog` buffer was passed
    int16_t arg[4];    // the template arguments, in the order of the family's comment above (unused: 0)
    uint32_t groups;   // query groups (tiles) of the launch; the maxsim families: queries per corpus pass
};
constexpr size_t kLaunchLogCap = 64;

// One launch of an exact scan with per-wave candidate lists (topk_dev.h), with the geometry its launch site derived
// (innr_ctx::scan_log). A record of its own, beside launch_log: an exact scan runs inside most recorded calls, and launch_log's
// readers decode a closed set of families. Written by plain host stores at the three launch sites, in every build; read only by
// the test hook innrdbg_scan_log, which tests/test_gpu_scan_threshold.py decodes.
enum ScanKind { kScanF32 = 1, kScanU8 = 2, kScanDense = 3 };  // scan_filter_kernel / scan_u8_filter_kernel / dense_filter_kernel
struct ScanRec {
    uint8_t kind;    // ScanKind
    uint8_t qb;      // QB: queries per corpus pass (dense: 1)
    uint8_t metric;  // INNR_METRIC_* of the f32 scan (u8, dense: INNR_METRIC_DOT)
    uint8_t rr;      // R: list capacity / 64
    uint8_t ext;     // EXT of the f32 scan (a mask or a dimension order), MASK of the u8 scan
    uint8_t pad[3];
    uint32_t cps;     // chunks per wave slot
    uint32_t nslots;  // wave slots
    uint32_t groups;  // query groups of the launch
};
constexpr size_t kScanLogCap = 16;
struct innr_ctx {
    innr_tuning tune;
    // One call at a time per context: the workspace below (grow-by-free DevBufs, the pinned bump allocator, `pending`,
    // the flags buffer, ev[]) is shared by every entry point, so each one holds this lock for its whole duration
    // (CtxGuard). Recursive: host-pointer entry points call their _dev counterparts.
    std::recursive_mutex mu;
    int depth = 0;  // nesting of CtxGuards on the owning thread
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // [4], [5]: the span of a filtered multi-query call
    // Pinned staging for SMALL host<->device transfers (queries in, top-k out, flags): a hipMemcpyAsync on pageable
    // memory costs ~40 us per call on this stack, four of them made a single-query call 190 us; through pinned
    // memory the same copies are a few us. Inputs are staged by copy_in (bump allocation), outputs land in the
    // pinned area and are handed to the caller's buffers by ctx_sync, which every host-pointer entry point ends on.
    char* pin = nullptr;
    size_t pin_in_off = 0, pin_out_off = 0;
    struct PendingOut {
        void* user;
        const void* staged;
        size_t bytes;
    };
    std::vector<PendingOut> pending;
    // workspace (a DevBuf added here goes into workspace_bufs() below as well: destroy, innr_ctx_memory and innr_ctx_trim walk that list)
    DevBuf q_row;     // queries row-major [Q][ldq]
    DevBuf q_kmajor;  // queries K-major [Dpad][Qpad] for the GEMM engine
    DevBuf q_norm;    // [Q] exact query norms
    DevBuf lists;     // candidate lists
    DevBuf counts;    // list counts
    DevBuf sel;       // selected composites [Q][KP]
    DevBuf sel_cnt;   // [Q]
    DevBuf gthr;           // GEMM engine: global threshold slots + bounds + k-rule margins
    DevBuf kmargin;        // [Qpad] 2E per query, staged for prep_gthr
    DevBuf i8s_prog;       // gemm_i8s_filter_kernel with several query groups: [wave slices][groups] positions (soft lockstep)
    DevBuf sel_tmp[2];     // multi-level select: [parts][Q][KP]
    DevBuf selcnt_tmp[2];  // [parts][Q]
    DevBuf scores;    // [QB][ldN] materialised scores
    DevBuf tmp_norms; // caller-provided norms staged on device
    DevBuf flags;     // error flag + per-query fallback flags
    DevBuf out_idx;   // staging for host-pointer entry points
    DevBuf out_score;
    DevBuf seed_idx;   // threshold seeding: exact top-KP of a corpus prefix (indices unused, scores -> bounds)
    DevBuf seed_score;
    DevBuf misc;
    DevBuf q_bf16;     // bf16 filter engine: K-packed bf16 queries
    struct RedoBufs {
        DevBuf q, idx, sc, map, qn;
    } redo[2];  // unproven queries, gathered and redone as ONE batch; [1]: the batch's own unproven queries (redo_batch)
    RedoBufs cmpl;     // the completion pass of unproven queries (knn_complete)
    DevBuf q_hat;      // int8 filter of an f32 corpus, cosine: the normalised queries
    DevBuf q_pad;      // exact engine: a ragged tail of 2-3 / 5-7 queries padded with zero rows to a 4- / 8-query pass
    DevBuf q_one;      // full-sort path (k > INNR_MAX_K): one zero-padded query row
    DevBuf sort_keys;  // [2][N] composites: unsorted, sorted
    DevBuf sort_tmp;   // radix sort scratch
    DevBuf flt_in;     // innr_batch_knn_filtered_multi: the caller's mask bytes staged on the device (host-memory entry point)
    DevBuf flt_mask;   // ... the mask normalised to 0/1, [ldN]
    DevBuf flt_scan;   // ... passing vectors per chunk [nchunks], their exclusive scan [nchunks], the total, the mask-differs flag
    DevBuf rs_cnt;     // innr_batch_range_search[_u8]: survivors per 256-vector (codes: 1024-vector) chunk [queries][nchunks + 1], scanned in place
    DevBuf rs_bits;    // ... the collect path's survivor bitmaps [queries][ldN / 32]
    DevBuf rs_tot;     // ... [queries] totals, then [queries] flags: the exact scan finishes this query
    DevBuf rs_thr;     // ... the thresholds and [Q + 1] offsets of the host-memory entry point, staged on the device
    DevBuf rs_off;
    DevBuf adp_scan;   // innr_batch_knn_adaptive: the AdaptiveState, then per-chunk counts and their scans [4][chunks of the corpus]
    DevBuf adp_list;   // ... the live list twice (indices, distances: a compaction writes the other copy) and its death dimensions
    DevBuf rows_q;     // innr_batch_knn_rows (rows.hip): a round's gathered query rows [round][D]; shared with nothing, the inner search uses the buffers above
    DevBuf rows_stage; // ... with exclude_self: the inner search's [round][k + 1] indices, then scores
    DevBuf rows_io;    // ... and innr_batch_gather_rows, host-memory entry points: indices in, results out
    DevBuf rows_flag;  // ... the gathers' own error word (an index outside the batch): every entry point clears c->flags
    DevBuf rows_bits;  // innr_batch_update_rows (mutate.hip): one bit per vector of the batch, set by the index it was named by; zeroed per call
    DevBuf rows_map;   // innr_batch_keep_rows: old column of every kept row (the selection gather writes it; not read)
    int last_filter = 0;  // filter kernel of the last knn_mfma first pass (LastFilter; read by a test hook)
    size_t split_seed_served = 0;  // prefix rows of the split filter's seeder in the last knn_mfma first pass (0: it did not run; read by a test hook)
    size_t screen_q = 0, screen_qpad = 0;  // queries of the last screen margins written to kmargin + Qpad (0: none yet; read by a test hook)
    LaunchRec launch_log[kLaunchLogCap] = {};  // ring of the last templated launches (launch_kernel; read by a test hook)
    uint64_t launch_total = 0;                 // launches recorded so far: entry i lives at launch_log[i % kLaunchLogCap]
    ScanRec scan_log[kScanLogCap] = {};        // ring of the last exact-scan launches (record_scan; read by a test hook)
    uint64_t scan_total = 0;                   // ... recorded so far: entry i lives at scan_log[i % kScanLogCap]
};

// wave slots of an exact scan under the option scan_max_slots (a multiple of 4, at least 4); applied before cps, the block count
// and the groups per launch are derived from the slot count
static inline size_t cap_scan_slots(const innr_ctx* c, size_t nslots) {
    const long v = c->tune.scan_max_slots;
    return v > 0 ? std::min<size_t>(nslots, round_up((size_t)std::max<long>(v, 4), 4)) : nslots;
}
// (the caller holds the context's lock, as every launch site does)
static inline void record_scan(innr_ctx* c, ScanKind kind, int qb, int metric, int rr, bool ext, uint32_t cps, size_t nslots,
                               uint32_t groups) {
    c->scan_log[c->scan_total++ % kScanLogCap] =
        ScanRec{(uint8_t)kind, (uint8_t)qb, (uint8_t)metric, (uint8_t)rr, (uint8_t)ext, {0, 0, 0}, cps, (uint32_t)nslots, groups};
}

// ---- choosing a kernel instantiation from run-time values ------------------------------------------------------------
// One instantiation of a recorded family, as compile-time constants: the family and the template arguments in the order of
// LaunchFamily's comments (bool parameters as 0 / 1). kernel_of(Inst) is the kernel they name.
template <int N> using IntC = std::integral_constant<int, N>;
template <int FAMILY, int... ARGS> struct Inst {};
// (the kernel_of overloads live beside the kernels they name: api.hip, maxsim.hip)

// Record an instantiation (the caller holds the context's lock, as every dispatch site does: a few host stores) and launch it on
// the context's stream. The record is written from the constants that name the kernel, so it cannot name another one.
struct LaunchDims {
    dim3 grid, block;
    size_t lds = 0;
    uint32_t groups = 1;    // LaunchRec::groups
    bool lockstep = false;  // LaunchRec::lockstep
};
template <int FAMILY, int... ARGS, class... KernelArgs>
static void launch_kernel(innr_ctx* c, Inst<FAMILY, ARGS...> inst, const LaunchDims& d, KernelArgs... args) {
    c->launch_log[c->launch_total++ % kLaunchLogCap] = LaunchRec{(uint8_t)FAMILY, (uint8_t)d.lockstep, {ARGS...}, d.groups};
    kernel_of(inst)<<<d.grid, d.block, d.lds, c->stream>>>(args...);
}
// ... where one record stands for two forms of a kernel with the same arguments: `kernel` is the form the dispatch site chose
template <int FAMILY, int... ARGS, class Kernel, class... KernelArgs>
static void launch_kernel_as(innr_ctx* c, Inst<FAMILY, ARGS...>, Kernel kernel, const LaunchDims& d, KernelArgs... args) {
    c->launch_log[c->launch_total++ % kLaunchLogCap] = LaunchRec{(uint8_t)FAMILY, (uint8_t)d.lockstep, {ARGS...}, d.groups};
    kernel<<<d.grid, d.block, d.lds, c->stream>>>(args...);
}

// A run-time value that selects one of the constants Vs; any other value selects the LAST of them (a switch's `default:`).
// dispatch(f, one_of<..>(a), one_of<..>(b), ...) calls f(IntC<A>(), IntC<B>(), ...) with the selected constants and returns what it
// returns: f is a generic lambda, instantiated once per combination, and excludes the combinations that must not exist by
// `if constexpr` on its arguments.
template <int... Vs> struct OneOf { int v; };
template <int... Vs> static OneOf<Vs...> one_of(long v) { return {(int)v}; }
template <class F> static auto dispatch(F&& f) { return f(); }
template <class F, int V, int... Vs, class... Rest>
static auto dispatch(F&& f, OneOf<V, Vs...> o, Rest... rest) {
    const auto bound = [&](auto... cs) { return f(IntC<V>(), cs...); };
    if constexpr (sizeof...(Vs) == 0) return dispatch(bound, rest...);
    else return o.v == V ? dispatch(bound, rest...) : dispatch(f, OneOf<Vs...>{o.v}, rest...);
}
static auto flag(bool on) { return one_of<1, 0>(on); }
// RR (R in the kernels) of an exact scan's list capacity of 64 RR entries: lists of 32 / 128 / 256 candidates (exact_cap)
static auto rr_scan(uint32_t cap) { return one_of<6, 12, 20>(cap / 64); }

namespace innr {
// The derived copies of its corpus a batch can own (innr_batch::copy), and what the batch keeps of each
enum CopyKind { kCopyRows, kCopyBfDot, kCopyBfCos, kCopyBfL2, kCopyBfDotLo, kCopyBfCosLo, kCopyI8Dot, kCopyI8Cos, kCopyI8L2, kCopyKinds };
struct CorpusCopy {
    char* p = nullptr;
    size_t bytes = 0;
    uint32_t nk = 0;       // K-steps of this copy (the rows copy: Dr)
    bool refused = false;  // rows, lo limbs (for the split pair): it did not fit -- do not try again on every call
    bool weak = false;     // int8 kinds: most proofs failed on this corpus (a range blown up by outliers): AUTO stops picking the filter
    // bf16 dot / cosine kinds and their lo limbs: the largest norm of a row of this copy's limbs, rounded up (limb_maxima_kernel;
    // the split filter's screen margin); < 0: not computed for the copy that exists now. Lives and dies with the copy.
    float limb_max = -1.0f;
};
}  // namespace innr

struct innr_batch {
    innr_ctx* ctx = nullptr;
    size_t N = 0, D = 0, ldN = 0, Dpad = 0;
    float* V = nullptr;      // [Dpad][ldN]
    float* norms = nullptr;  // [ldN], lazily computed (exact batch_norms)
    float* invn = nullptr;   // [ldN], 1/norm (0 for zero-norm vectors): GEMM engine's approximate cosine
    float* sqn = nullptr;    // [ldN], norm^2: GEMM engine's approximate L2
    uint32_t* max_norm_bits = nullptr;
    size_t aux_bytes = 0;  // what norms, max_norm_bits, invn and sqn were allocated with, added up where each is allocated
    bool norms_ready = false;
    float max_norm = 0.0f;
    uint64_t index_base = 0;
    std::vector<float> dimvar;  // batch_dimension_variance, computed once (batch.rs:572)
    // scalar-quantised corpus (scalar.rs): codes C8[d*ldN + i] instead of V, with the collection's params
    uint8_t* C8 = nullptr;
    float alpha = 1.0f, offset = 0.0f;
    // innr_batch_prefix_view: V / C8 belong to another batch (never freed here). Rows D..Dpad of a view can hold the
    // parent's next dimensions instead of zero padding; the GEMM engine (which multiplies all Dpad rows) is then off.
    bool is_view = false, gemm_ok = true;
    // The derived copies of the corpus, indexed by innr::CopyKind; each is built on first use and always owned:
    //  rows: row-major rows[i*Dr + d] (Dr = D rounded up to 4, kept in nk), built on the first call that has MANY candidates per
    //    query to re-score exactly (the completion pass, k beyond the candidate lists): in the dimension-major store a candidate's D
    //    values lie in D different cache lines (64 B fetched per 4 B used); here they are contiguous. + N*Dr*4 bytes.
    //  bf16 filter engine (kernels_gemm_bf16.h): the K-packed bf16 copy (dot), the same with every row scaled by 1/||v|| (cosine,
    //    built on the first cosine call) and the squared-L2 filter's copy: six more K columns per row (|v|^2 in three limbs, three ones)
    //  split-bf16 filter of INNR_KNN_MFMA: the lo limbs x - rne_bf16(x) of the dot and the cosine copy's values, in
    //    the same layout; built on first use when they fit
    //  int8 filter engine (kernels_gemm_i8.h): of a u8 code batch the K-packed signed copy of the codes (the dot kind); of an F32
    //    batch (INNR_KNN_MFMA_I8) its values scalar-quantised with one (offset, alpha) for the whole corpus (dot), its normalised
    //    rows quantised over their own range (cosine), and the squared-L2 copy: the dot copy's quantisation plus R + 1 more
    //    dimensions that carry |v|^2 in two 8-bit limbs (pack_corpus_f32_i8_kernel); D' = D + R + 1
    innr::CorpusCopy copy[innr::kCopyKinds];
    // what the int8 copies of an F32 batch were quantised with: the raw values' range (the dot and squared-L2 copies), the
    // normalised rows' (the cosine copy), and the squared-L2 copy's extra dimensions
    struct I8Range {
        float alpha = 0.0f, offset = 0.0f;
    } i8_raw, i8_norm;
    I8Range& i8_range(innr::CopyKind k) { return k == innr::kCopyI8Cos ? i8_norm : i8_raw; }
    uint32_t i8l2_R = 0;
    float i8l2_nmax = 0.0f;
    uint32_t i8_weak_skips = 0;              // AUTO calls that skipped the int8 filter since (every 64th tries it again)
    float screen_share[2] = {0.0f, 0.0f};    // split filter: share of wave tiles the last screened first pass corrected, lists <= 64 / longer (knn_mfma)
    uint32_t screen_skips[2] = {0, 0};       // ... calls that took the full loop since (every 64th screens again)
    uint32_t auto_small_calls = 0;           // AUTO calls with fewer than four queries while no int8 copy existed: the fourth builds it
    // innr_batch_knn_filtered_multi (kernels_select.h): the selection of the last mask -- its passing vectors compacted into a batch
    // of their own (npass * Dpad * 4 bytes, plus the filter copies the engines build on it), the normalised mask it was built from
    // and the map selection index -> column of this batch. At most one; freed with the batch, when a call brings a different mask,
    // and at the end of every call under filter_keep_selection = 0.
    innr_batch* fsel = nullptr;
    uint8_t* fsel_mask = nullptr;  // [ldN] 0/1
    uint32_t* fsel_map = nullptr;  // [fsel->N]
    uint32_t fsel_builds = 0;      // selections built for this batch (read by a test hook)
    size_t fsel_mask_bytes = 0, fsel_map_bytes = 0;  // what fsel_mask / fsel_map were allocated with
    // memory accounting (innr_batch_memory): what V / C8 was allocated with (0 for a view), and the copy budget -- the most the
    // derived allocations (copy[] and the selection) may add up to; see budget_admits
    size_t corpus_bytes = 0;
    uint64_t copy_budget = UINT64_MAX;
};

struct innr_docs {
    innr_ctx* ctx = nullptr;
    size_t ndocs = 0, T = 0, dim = 0;
    float* tok = nullptr;          // [ndocs][T][dim]
    uint32_t* doc_len = nullptr;   // [ndocs] or null (every document has T tokens)
    float* tok_inv = nullptr;      // [ndocs*T] 1/|token| (0 for zero-norm tokens), built on first MFMA-engine use
    size_t tok_bytes = 0, doc_len_bytes = 0, tok_inv_bytes = 0;  // what each was allocated with (innr_docs_memory)
    float max_norm = 0.0f;         // max |token| over the corpus
    uint64_t index_base = 0;
};

namespace innr {

// api.hip: staging through the pinned area, the stream synchronisation that delivers it, the device of a context
hipError_t copy_in(innr_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t copy_out(innr_ctx* c, void* dst, const void* src, size_t bytes);
hipError_t ctx_sync(innr_ctx* c);
innr_status bind_device(innr_ctx* ctx);
// api.hip: candidate lists -> c->sel / c->sel_cnt, their geometry, the kernels' error word, results out of composites
innr_status run_select(innr_ctx* c, const uint64_t* lists, const uint32_t* counts, uint32_t nslots, uint32_t qstride, uint32_t cap,
                       uint32_t KP, uint32_t Q);
uint32_t exact_cap(uint32_t KP);
uint32_t pick_kp(size_t k, size_t margin);
bool metric_ok(int m);
innr_status check_errflag(innr_ctx* c);
innr_status emit_results(innr_ctx* c, const uint64_t* sel, size_t KP, size_t Q, size_t kout, bool smaller_is_better, uint64_t index_base,
                         uint64_t* out_idx, float* out_score);
// api.hip, for the units that need a kernel it owns: the exact engine's squared-L2 scan of one query over the first W dimension
// rows (out[0, ldN): the bits innr_batch_scores gives on a prefix view of W dimensions), and the single-workgroup exclusive scan
innr_status l2_prefix_scores(innr_batch* b, const float* d_query, size_t W, float* out);
innr_status exclusive_scan_u32(innr_ctx* c, const uint32_t* counts, uint32_t n, uint32_t* offsets, uint32_t* total);
// api.hip, for the entry points that change a batch in place (mutate.hip):
// a new f32 batch of N vectors with a zeroed store of round_up(N, 256) columns x round_up(D, 32) rows (N beyond kMaxBatchN:
// INNR_E_UNSUPPORTED; a failed hipMalloc: INNR_E_OOM) -- a mutation takes its store and frees the rest
constexpr size_t kMaxBatchN = 0xFFFFFFFFull - 256;  // a batch holds fewer vectors than this (u32 device indices)
innr_status alloc_batch(innr_ctx* ctx, size_t N, size_t D, innr_batch** out);
// rows[n][D] (device) into columns col0 .. col0 + n of a dimension-major store (transpose_rows_kernel, the upload's launch): only
// d < D, i < n is written
hipError_t transpose_rows_into(innr_ctx* c, const float* d_rows, size_t n, size_t D, float* V, size_t ldN, size_t col0);
// the selection's count (select_mask_kernel + scan: d_mask normalised into c->flt_mask, offsets in c->flt_scan, *npass; one
// synchronise) and its gather (select_gather_kernel) of the passing columns of b into S, in index order; map[npass] is written
innr_status count_mask(innr_batch* b, const uint8_t* d_mask, size_t* npass);
innr_status gather_passing(innr_batch* b, float* S, size_t ldS, uint32_t* map);
// ... and for the entry points that change a code batch in place (mutate_u8.hip) their byte twins: a new code
// batch of N vectors with a zeroed store of round_up(N, 1024) columns x round_up(D, 32) rows of bytes (N from kMaxBatchNU8 on:
// INNR_E_UNSUPPORTED; a failed hipMalloc: INNR_E_OOM), the upload's transpose at a column offset (byte stores: col0 need be no
// multiple of 4), and the selection's gather of a code batch (select_gather_u8_kernel, after count_mask)
constexpr size_t kMaxBatchNU8 = 0xFFFFFFFFull - 1024;
innr_status alloc_batch_u8(innr_ctx* ctx, size_t N, size_t D, float alpha, float offset, innr_batch** out);
hipError_t transpose_codes_into(innr_ctx* c, const uint8_t* d_codes, size_t n, size_t D, uint8_t* C8, size_t ldN, size_t col0);
innr_status gather_passing_u8(innr_batch* b, uint8_t* S, size_t ldS, uint32_t* map);
// mutate.hip: update_check_kernel over n device indices of one staging round (the caller zeroed c->rows_bits and the head of
// c->rows_flag once per call), and that head as the kernel writes it
struct UpdateFlag {
    uint32_t outside, twice;
    uint64_t outside_idx, twice_idx;
};
innr_status launch_update_check(innr_batch* b, const uint64_t* d_idx, size_t n);
// THE list of what a batch derives from its store, forgotten: every copy[] kind (as innr_batch_release_copies frees them, a
// remembered refusal included), the kept selection, the norms and their by-products, the dimension variances, the int8 ranges
// and the engines' call history. The caller has synchronised the stream. Each is rebuilt by the next call that wants it.
void invalidate_derived(innr_batch* b);
// sort_full.hip
hipError_t full_sort_scratch_bytes(size_t n, size_t* bytes);
size_t full_topk_out_capacity(size_t k);  // keys the `sorted` buffer must hold for the best k (the next power of two)
hipError_t full_topk_keys(const uint64_t* keys, size_t n, size_t k, uint64_t* sorted, void* scratch, hipStream_t stream);
hipError_t full_sort_scores(const float* scores, size_t n, bool smaller_is_better, uint64_t* keys, uint64_t* sorted,
                            void* scratch, size_t scratch_bytes, hipStream_t stream, const uint8_t* mask, size_t k);
hipError_t segmented_sort_scratch_bytes(size_t nseg, size_t len, size_t* bytes);
hipError_t segmented_topk_keys(const uint64_t* keys, uint64_t* sorted, size_t nseg, size_t len, size_t k, uint64_t* tmp, void* scratch,
                               hipStream_t stream);
// maxsim.hip
innr_status maxsim_topk_impl(innr_docs* d, int cosine, const float* qtok, size_t Tq, size_t dim, size_t k, int engine,
                             uint64_t* out_doc, float* out_score, size_t* out_k, innr_knn_stats* stats, bool to_host);

// Serialises the entry points of one context and, when the outermost entry point leaves with device->host copies still
// queued (an error return between a copy_out and its ctx_sync), cancels them: their destinations may be stack variables
// of frames that are gone, and the next successful ctx_sync must not deliver into them.
struct CtxGuard {
    innr_ctx* c;
    explicit CtxGuard(innr_ctx* ctx) : c(ctx) {
        if (c) {
            c->mu.lock();
            ++c->depth;
        }
    }
    ~CtxGuard() {
        if (!c) return;
        if (--c->depth == 0 && (!c->pending.empty() || c->pin_in_off || c->pin_out_off)) {
            (void)hipStreamSynchronize(c->stream);  // the staged copies still target the pinned area: let them land
            c->pending.clear();
            c->pin_in_off = c->pin_out_off = 0;
        }
        c->mu.unlock();
    }
    CtxGuard(const CtxGuard&) = delete;
    CtxGuard& operator=(const CtxGuard&) = delete;
};
#define INNR_ENTER(ctxp)            \
    ::innr::CtxGuard _guard(ctxp);  \
    INNR_TRY(::innr::bind_device(ctxp))

}  // namespace innr

// A kNN call on host memory: the queries staged on the device, dev(d_queries, d_out_idx, d_out_score) (a *_dev entry point, room
// for `cap` results per query), then *out_k results per query copied back
template <class Dev>
static innr_status knn_from_host(innr_ctx* c, const float* queries, size_t Q, size_t D, size_t cap, uint64_t* out_idx,
                                 float* out_score, const size_t* out_k, Dev&& dev) {
    INNR_ENTER(c);
    INNR_TRY(c->q_row.ensure(std::max<size_t>(Q * D, 1) * sizeof(float)));
    INNR_TRY(c->out_idx.ensure(Q * cap * sizeof(uint64_t)));
    INNR_TRY(c->out_score.ensure(Q * cap * sizeof(float)));
    if (D) INNR_HIP_CHECK(copy_in(c, c->q_row.p, queries, Q * D * sizeof(float)));
    INNR_TRY(dev(c->q_row.as<float>(), c->out_idx.as<uint64_t>(), c->out_score.as<float>()));
    if (*out_k) {
        INNR_HIP_CHECK(copy_out(c, out_idx, c->out_idx.p, Q * *out_k * sizeof(uint64_t)));
        INNR_HIP_CHECK(copy_out(c, out_score, c->out_score.p, Q * *out_k * sizeof(float)));
        INNR_HIP_CHECK(ctx_sync(c));
    }
    return INNR_OK;
}
