"""GPU tests of one sentence of api.hip (above workspace_bufs()): the workspace buffers of a context "carry nothing from one call to
the next". Every entry point works in the same ~60 grow-only device buffers and one pinned staging area, and the rest of the suite
runs its cases in one fixed order: each of them meets exactly one history, whatever the case before it left behind. Here a test hook
(innrdbg_workspace_fill, test-hooks library only) overwrites every workspace buffer but the 4 KiB `flags` block, and the whole pinned
area, with one byte value, and the call under test runs on top of that.

One procedure for every case (_check_residue):
  1. the call twice clean (the first run sizes the buffers and builds the batch's derived copies): both answers equal the oracle
     bit for bit, and the two runs agree in stats.engine / queries_fallback / candidates_kept, in the launch record
     (innrdbg_launch_log) and in the scan record (innrdbg_scan_log) -- a case where they do not is badly chosen;
  2. the hook reports what it filled: not zero, innr_ctx_memory less the 4096 bytes of `flags`, and every buffer the case is
     meant to reach (the audit table) has a size by now;
  3. fill 0xFF, the same call on a FRESH batch (norms, dimension variances, derived copies and the kept selection are then computed
     over poisoned workspace): the answer equals the oracle, stats and both records equal the clean run's. The records are what
     catches a proof that residue broke and the exact fallback rescued: the answer is right, queries_fallback and the launches differ;
  4. the same with 0x00, then 0x5A (as floats 0x5A5A5A5A = 1.5e16: large and finite; as a count or an index: in range of nothing).
Residue can be any byte pattern: callers' queries (NaN and +-inf included, elsewhere in the suite) land in q_row, q_kmajor, q_bf16,
q_hat, redo[].q and cmpl.q; counts and indices of one call are the next call's garbage.

The error-path tests at the end run a call that fails on a flag the device sets, then a good call of the same family and one of
another family: both equal the oracle and the clean stats. The last test names every workspace buffer no case of this file grew
(the file starts from a trimmed workspace): a new buffer cannot arrive without a case."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import test_gpu_range_search as RS
from test_gpu_exact import _SCAN_REC, SCAN_LOG_CAP, bits_equal, same_knn
from test_gpu_filtered_multi import _expected as _masked_expected
from test_gpu_kernel_variants import (_REC, D_GEMM, LOG_CAP, N_I8, _codes, _dim, _i8_oracle, _i8_queries, _i8_rows, _ms_corpus,
                                      _ms_query, _oracle_knn_u8)
from test_gpu_maxsim import _oracle_scores
from test_gpu_maxsim_rerank import PairOracle
from test_gpu_order_semantics import _all_scores as _score_bits, _from_dev, _merge_want, _rerank_ref, _shard_lists, _to_dev
from test_gpu_rows import strip
from test_gpu_u8_range_search import _all_scores as _u8_all_scores, _expected as _u8_range_expected

FILL_BYTES = (0xFF, 0x00, 0x5A)
FLAGS_BYTES = 4096  # the one buffer the hook leaves alone (and innr_ctx_trim keeps)
D = D_GEMM          # 123: five padding dimensions in Dpad = 128, a ragged last K-step of every filter
N = N_I8            # 8300: a ragged last 128-row tile, >= 32 x 256 rows: seeded once gemm_seed_n = 256
SEED256 = ("gemm_seed_n", 256)
_GROWN: set = set()  # every workspace buffer that had a size after some case of this file


# ------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


@pytest.fixture(scope="module")
def M():
    from innr_amd import maxsim
    return maxsim


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@pytest.fixture(scope="module", autouse=True)
def _own_workspace():
    """the file starts from an empty workspace (innr_ctx_trim), so that a buffer with a size was grown by a case of this file; the
    one resident corpus of the cases is freed at the end"""
    _ctx().trim()
    yield
    for obj in _RESIDENT.values():
        obj.close()
    _RESIDENT.clear()


# ------------------------------------------------------------------------------- the hooks
def _ctx():
    from innr_amd import _lib
    return _lib.default_context()


@functools.lru_cache(maxsize=1)
def _hooks():
    from conftest import hooks_lib
    L = hooks_lib()
    L.innrdbg_workspace_fill.restype = C.c_int
    L.innrdbg_workspace_fill.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]
    L.innrdbg_workspace_sizes.restype = C.c_size_t
    L.innrdbg_workspace_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.innrdbg_workspace_names.restype = C.c_char_p
    L.innrdbg_workspace_names.argtypes = []
    for name in ("innrdbg_launch_log", "innrdbg_scan_log"):
        getattr(L, name).restype = C.c_size_t
        getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        getattr(L, name + "_reset").restype = None
        getattr(L, name + "_reset").argtypes = [C.c_void_p]
    L.innrdbg_split_seed_served.restype = C.c_size_t
    L.innrdbg_split_seed_served.argtypes = [C.c_void_p]
    return L


def _fill(byte) -> int:
    """every workspace buffer but `flags`, and the pinned staging area, overwritten with `byte`; the device bytes written"""
    n = C.c_uint64(0)
    status = _hooks().innrdbg_workspace_fill(_ctx().handle, byte, C.byref(n))
    assert status == 0, f"innrdbg_workspace_fill: status {status}"
    return int(n.value)


def _sizes() -> dict:
    """name -> bytes of every buffer of workspace_bufs(), in its order"""
    names = _hooks().innrdbg_workspace_names().decode().split(",")
    buf = np.zeros(len(names) + 8, np.uint64)
    n = _hooks().innrdbg_workspace_sizes(_ctx().handle, buf.ctypes.data, buf.size)
    assert n == len(names), f"workspace_bufs() has {n} entries, innrdbg_workspace_names() names {len(names)}"
    return {name: int(b) for name, b in zip(names, buf[:n])}


class Out(NamedTuple):
    """what a run of a case hands back: the answer (arrays and numbers; the run has compared it with the oracle already), the
    stats of the call as (engine, queries_fallback, candidates_kept), and whatever else must not depend on residue"""
    answer: tuple
    stats: tuple = ()
    extra: tuple = ()


class Seen(NamedTuple):
    answer: tuple
    sig: tuple  # (stats, extra, (launches recorded, the records), (scans recorded, the records))


def _stats(st) -> tuple:
    return (int(st.engine), int(st.queries_fallback), int(st.candidates_kept))


def _observe(run, fresh) -> Seen:
    """run(fresh) between a reset and a read of both records"""
    L, h = _hooks(), _ctx().handle
    L.innrdbg_launch_log_reset(h)
    L.innrdbg_scan_log_reset(h)
    out = run(fresh)
    lbuf, ltot = np.zeros(LOG_CAP, _REC), C.c_uint64(0)
    ln = L.innrdbg_launch_log(h, lbuf.ctypes.data, LOG_CAP, C.byref(ltot))
    sbuf, stot = np.zeros(SCAN_LOG_CAP, _SCAN_REC), C.c_uint64(0)
    sn = L.innrdbg_scan_log(h, sbuf.ctypes.data, SCAN_LOG_CAP, C.byref(stot))
    launches = [(int(r["family"]), int(r["lockstep"]), tuple(int(x) for x in r["arg"]), int(r["groups"])) for r in lbuf[:ln]]
    scans = [tuple(int(r[f]) for f in _SCAN_REC.names) for r in sbuf[:sn]]
    return Seen(out.answer, (out.stats, out.extra, (int(ltot.value), launches), (int(stot.value), scans)))


def _same_answer(a, b) -> bool:
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
                return False
        elif x != y:
            return False
    return True


def _check_residue(name, run, needs=()):
    """the five steps of the module docstring; run(fresh) -> Out compares its answer with the oracle itself"""
    first = _observe(run, False)
    clean = _observe(run, False)
    assert first.sig == clean.sig, (f"{name}: two CLEAN runs disagree in stats or records -- the case is badly chosen, take inputs "
                                    f"where they agree\n  first  {first.sig}\n  second {clean.sig}")
    assert _same_answer(first.answer, clean.answer), f"{name}: two clean runs give different answers"
    sizes = _sizes()
    _GROWN.update(n for n, b in sizes.items() if b)
    unsized = [n for n in needs if not sizes[n]]
    assert not unsized, f"{name}: the case was meant to reach {unsized}, which have no size after two runs: {sizes}"
    for byte in FILL_BYTES:
        filled = _fill(byte)
        sizes = _sizes()
        assert filled > 0 and filled == _ctx().memory() - FLAGS_BYTES == sum(b for n, b in sizes.items() if n != "flags"), \
            f"{name}: the hook filled {filled} bytes, the workspace holds {_ctx().memory()} ({sizes})"
        assert all(sizes[n] for n in needs), (name, sizes)
        got = _observe(run, True)  # (the oracle comparison is inside)
        assert _same_answer(got.answer, clean.answer), f"{name}: the answer over a workspace of 0x{byte:02X} differs from the clean one"
        assert got.sig == clean.sig, (f"{name}: over a workspace of 0x{byte:02X} the call took another way than over a clean one "
                                      f"(stats, extra, launches, scans)\n  clean    {clean.sig}\n  poisoned {got.sig}")
    _GROWN.update(n for n, b in _sizes().items() if b)


# ------------------------------------------------------------------------------- resident corpora
_RESIDENT: dict = {}


@contextlib.contextmanager
def _resident(key, make, fresh):
    """the case's corpus on the device: the one resident object of `key` (one at a time), or with `fresh` a new one for this run"""
    if fresh:
        obj = make()
        try:
            yield obj
        finally:
            obj.close()
        return
    if key not in _RESIDENT:
        for o in _RESIDENT.values():
            o.close()
        _RESIDENT.clear()
        _RESIDENT[key] = make()
    yield _RESIDENT[key]


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


KNN_FN = {"dot": "batch_knn_dot_multi", "cos": "batch_knn_cosine_multi", "l2": "batch_knn_multi"}
ORACLE_KNN = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}
EXACT_BUFS = ("q_row", "out_idx", "out_score", "lists", "counts", "sel", "sel_cnt")
GEMM_BUFS = EXACT_BUFS + ("q_kmajor", "q_norm", "misc", "gthr", "kmargin")


def _assert_knn(metric, idx, sc, want, what):
    assert idx.shape[0] == len(want), what
    for j, (oi, os_) in enumerate(want):
        assert same_knn(metric, idx[j], sc[j], oi, os_), (what, j, idx[j][:8], oi[:8], sc[j][:8], os_[:8])


def _f32_run(B, innr, metric, rows_fn, key, qs, want, k, engine, extra=None):
    """one kNN call of `engine` on an f32 corpus, compared with the oracle's `want`"""
    def run(fresh):
        with _resident(key, lambda: B.VerticalBatch.from_rows(rows_fn()), fresh) as vb:
            st = innr.KnnStats()
            idx, sc = getattr(B, KNN_FN[metric])(qs, vb, k, engine=engine, stats=st)
            more = extra(vb) if extra else ()
        _assert_knn(metric, idx, sc, want, (key, metric, k, engine))
        return Out((idx, sc), _stats(st), more)
    return run


# =============================================================================== f32 k-NN
class Knn(NamedTuple):
    id: str
    metric: str
    kind: str      # _i8_rows: "uniform", or "dup" (no first-pass proof holds on it)
    nq: int
    k: int
    engine: str    # attribute of innr_amd
    options: tuple = ()
    dim: int = D
    needs: tuple = ()
    launched: tuple = ()  # (family, MODE) of api_internal.h LaunchFamily records the call must have made; MODE None: any


F32, BF16, SPLIT, I8_ONE, I8_TWO, I8_SMALL = 1, 2, 3, 4, 5, 6  # api_internal.h LaunchFamily
MODE_ARG = {F32: 2, BF16: 1, SPLIT: 1, I8_ONE: 1, I8_TWO: 1, I8_SMALL: 2}  # where MODE stands among a record's arguments
KNN_CASES = (
    [Knn(f"exact-{m}-q{q}", m, "uniform", q, 10, "KNN_EXACT", needs=EXACT_BUFS + (("q_pad",) if q == 3 else ()))
     for m in ("dot", "cos", "l2") for q in (1, 3, 9)] +
    [Knn(f"f32-filter-{m}", m, "uniform", 3, 10, "KNN_MFMA", (SEED256, ("no_split_filter", 1)),
         needs=GEMM_BUFS + ("seed_idx", "seed_score") + (("tmp_norms",) if m == "l2" else ()), launched=((F32, 0),))
     for m in ("dot", "cos", "l2")] +
    [Knn(f"split-{'full' if s == 1 else 'screened'}-{m}-k{k}", m, "uniform", 3, k, "KNN_MFMA",
         (SEED256, ("split_min_q", 1), ("no_split_screen", s)), needs=GEMM_BUFS + ("q_bf16",), launched=((SPLIT, 0),))
     for s in (1, -1) for m in ("dot", "cos") for k in (10, 100)] +
    [Knn(f"bf16-{m}", m, "uniform", 3, 10, "KNN_MFMA_BF16", (SEED256,), needs=GEMM_BUFS + ("q_bf16",), launched=((BF16, 0),))
     for m in ("dot", "cos", "l2")] +
    [Knn("i8-small-q3", "dot", "uniform", 3, 10, "KNN_MFMA_I8", (SEED256,), needs=GEMM_BUFS + ("q_bf16", "tmp_norms", "sel_tmp0", "selcnt_tmp0"),
         launched=((I8_SMALL, 0),)),
     Knn("i8-small-q130-lockstep", "dot", "uniform", 130, 10, "KNN_MFMA_I8", (SEED256,), dim=_dim(8), needs=("i8s_prog", "q_bf16"),
         launched=((I8_SMALL, 0), "lockstep")),
     Knn("i8-tile-q3", "dot", "uniform", 3, 10, "KNN_MFMA_I8", (SEED256, ("i8_no_small", 1)), needs=("q_bf16",), launched=((I8_ONE, 0),)),
     Knn("i8-cos-q3", "cos", "uniform", 3, 10, "KNN_MFMA_I8", (SEED256,), needs=("q_bf16", "q_hat"), launched=((I8_SMALL, 0),)),
     Knn("i8-l2-q3", "l2", "uniform", 3, 10, "KNN_MFMA_I8", (SEED256,), needs=("q_bf16", "q_hat"), launched=((I8_SMALL, 0),))] +
    [Knn("complete-f32-q9", "dot", "dup", 9, 100, "KNN_MFMA", (SEED256, ("no_split_filter", 1)),
         needs=("cmpl.q", "cmpl.idx", "cmpl.sc", "cmpl.map", "cmpl.qn", "sort_keys"), launched=((F32, 0), (F32, 2))),
     Knn("complete-f32-q260", "dot", "dup", 260, 100, "KNN_MFMA", (SEED256, ("no_split_filter", 1)), needs=("cmpl.q", "sort_keys"),
         launched=((F32, 0), (F32, 2))),
     Knn("complete-split-q260", "cos", "dup", 260, 100, "KNN_MFMA", (SEED256, ("no_split_screen", 1)), needs=("cmpl.q", "q_bf16"),
         launched=((SPLIT, 0), (F32, 2))),
     Knn("complete-i8-q3", "dot", "dup", 3, 100, "KNN_MFMA_I8", (SEED256,), needs=("cmpl.q", "q_bf16", "sort_keys"),
         launched=((I8_SMALL, 0), (I8_SMALL, 2)))] +
    [Knn("fullsort-k241-cos", "cos", "uniform", 2, 241, "KNN_EXACT", needs=("q_one", "scores", "sort_keys", "sort_tmp")),
     Knn("fullsort-kN-dot", "dot", "uniform", 2, N, "KNN_MFMA", needs=("q_one", "scores", "sort_keys", "sort_tmp"))]
)


@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: c.id)
def test_knn_f32(B, innr, ctx_option, case):
    for name, value in case.options:
        ctx_option(name, value)
    want = _i8_oracle(case.dim, case.kind, case.metric, case.nq, case.k)
    run = _f32_run(B, innr, case.metric, lambda: _i8_rows(case.dim, case.kind)[0], ("f32", case.dim, case.kind),
                   _i8_queries(case.dim, case.nq), want, case.k, getattr(innr, case.engine))
    if case.launched:  # the kernels the case is named after served it (test_gpu_kernel_variants.py names every instantiation)
        records = _observe(run, False).sig[2][1]
        for want_launch in case.launched:
            if want_launch == "lockstep":
                assert any(lockstep for _, lockstep, _, _ in records), f"{case.id}: no launch with the soft-lockstep buffer: {records}"
            else:
                family, mode = want_launch
                assert any(f == family and args[MODE_ARG[family]] == mode for f, _, args, _ in records), \
                    f"{case.id}: no launch of family {family} in MODE {mode}: {records}"
    _check_residue(case.id, run, case.needs)


# ---- a minority of unproven queries: the retry with lists of 256 and the redo sets of both levels
CLUSTER_AT, CLUSTER_ROWS, CLUSTER_Q, CLUSTER_NQ = 1000, 300, 20, 130


@functools.lru_cache(maxsize=1)
def _cluster_case():
    """The uniform corpus with one row, 30 long, 300 times over (rows 1000 .. 1299): for the first 20 of 130 queries (that row plus a
    little noise) the 300 copies tie at the top, far above every other row -- more exact ties than a list of 32 or of 256 holds, so
    their proofs fail on the first pass AND on a retry with lists of 256. The other 110 queries are made to score the copies below
    zero: plain uniform queries, proven by the first pass. 20 of 130 is the minority (>= 16, <= a quarter) that knn_mfma retries."""
    rows = _i8_rows(D, "uniform")[0].copy()
    u = (rows[17] / np.float32(np.sqrt(np.sum(rows[17].astype(np.float64) ** 2)))).astype(np.float32)
    rows[CLUSTER_AT:CLUSTER_AT + CLUSTER_ROWS] = (u * np.float32(30.0)).astype(np.float32)
    qs = _i8_queries(D, CLUSTER_NQ).copy()
    proj = (qs.astype(np.float64) @ u.astype(np.float64))[:, None] * u[None, :].astype(np.float64)
    qs = (qs - proj - 0.1 * u[None, :]).astype(np.float32)  # q . (30 u) = -3: the copies rank far down
    qs[:CLUSTER_Q] = (u * np.float32(30.0))[None, :] + np.float32(0.01) * _i8_queries(D, CLUSTER_Q)
    data = oracle.from_rows(rows)
    want = [oracle.batch_knn_dot(q, data, 10) for q in qs]
    for j in range(CLUSTER_NQ):  # what the data is built to do
        top_is_cluster = all(CLUSTER_AT <= int(i) < CLUSTER_AT + CLUSTER_ROWS for i in want[j][0])
        assert top_is_cluster == (j < CLUSTER_Q), j
    return _ro(rows, qs) + (want,)


@pytest.mark.parametrize("options,fallback", [((), 20), ((("no_completion", 1),), 20), ((("no_completion", 1), ("gemm_no_kp_retry", 1)), 20)],
                         ids=["completion", "kp-retry-then-exact", "exact"])
def test_knn_f32_retry_and_redo(B, innr, ctx_option, options, fallback):
    """20 of 130 queries unproven: the completion pass; with no_completion the retry with lists of 256 (redo set of level 0), whose
    own 20 unproven queries take the exact engine (redo set of level 1); with gemm_no_kp_retry on top the exact engine at once"""
    for name, value in (SEED256, ("no_split_filter", 1)) + options:
        ctx_option(name, value)
    rows, qs, want = _cluster_case()
    run = _f32_run(B, innr, "dot", lambda: rows, ("f32", "cluster"), qs, want, 10, innr.KNN_MFMA)
    seen = _observe(run, False)
    assert seen.sig[0] == (innr.KNN_MFMA, fallback, 32), seen.sig
    gemm_launches = [l for l in seen.sig[2][1] if l[0] == 1]
    needs = {0: ("cmpl.q", "cmpl.map"), 1: ("redo0.q", "redo0.idx", "redo0.sc", "redo0.map", "redo0.qn", "redo1.q", "redo1.idx", "redo1.sc",
                                             "redo1.map", "redo1.qn"), 2: ("redo0.q", "redo0.map")}[len(options)]
    assert len(gemm_launches) == (2 if len(options) < 2 else 1), seen.sig  # first pass + (collect pass | retry with lists of 256)
    _check_residue(f"retry{len(options)}", run, needs)


# ---- prefix views: 96 dimensions (whole K-steps: the matrix pipe may serve it) and 100 (rows 100 .. 127 of the view hold the
# parent's next dimensions, not padding: the exact engine)
@pytest.mark.parametrize("P,served", [(96, "KNN_MFMA"), (100, "KNN_EXACT")])
def test_knn_prefix_view(B, innr, ctx_option, P, served):
    ctx_option(*SEED256)
    ctx_option("no_split_filter", 1)
    rows = _i8_rows(D, "uniform")[0]
    qs = np.ascontiguousarray(_i8_queries(D, 3)[:, :P])
    data = oracle.from_rows(np.ascontiguousarray(rows[:, :P]))
    want = [oracle.batch_knn_cosine(q, data, 10) for q in qs]

    def run(fresh):
        with _resident(("f32", D, "uniform"), lambda: B.VerticalBatch.from_rows(rows), fresh) as vb:
            view = vb.prefix(P)
            st = innr.KnnStats()
            idx, sc = B.batch_knn_cosine_multi(qs, view, 10, engine=innr.KNN_MFMA, stats=st)
            view.close()
        _assert_knn("cos", idx, sc, want, ("prefix", P))
        assert st.engine == getattr(innr, served)
        return Out((idx, sc), _stats(st))
    _check_residue(f"prefix{P}", run, EXACT_BUFS)


# ---- the split filter's own seeder, at the shape of test_gpu_split_seed.py
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_knn_split_seeder(B, innr, ctx_option, metric):
    n, dim, nq, P = 32768 + 37, 40, 70, 1024
    ctx_option("split_seed_rows", P)
    rows, qs = _split_seed_case(n, dim, nq)
    data = oracle.from_rows(rows)
    want = [ORACLE_KNN[metric](q, data, 10) for q in qs]
    served = lambda vb: (int(_hooks().innrdbg_split_seed_served(vb._h)),)
    run = _f32_run(B, innr, metric, lambda: rows, ("f32", "split-seed"), qs, want, 10, innr.KNN_MFMA, extra=served)
    seen = _observe(run, False)
    assert seen.sig[1] == (P,), f"the split filter's seeder did not serve the call: {seen.sig}"
    assert any(l[0] == 14 for l in seen.sig[2][1]), seen.sig  # kLaunchSplitSeed
    _check_residue(f"split-seed-{metric}", run, GEMM_BUFS + ("q_bf16", "seed_idx", "seed_score"))


@functools.lru_cache(maxsize=1)
def _split_seed_case(n, dim, nq):
    import split_seed_ref as R
    return _ro(R.corpus("random", n, dim, 11), R.queries(nq, dim, 5))


# ---- more lists of 256 than one select pass merges twice over: both levels of the multi-level select
def test_knn_two_select_levels(B, innr):
    """66 000 rows are 258 chunks = 260 wave slots of the exact scan; with lists of 256 one select pass merges 16 of them: 17 parts,
    then 2, then 1 -- sel_tmp[0] and sel_tmp[1]"""
    n, dim, k = 66_000, 3, 240
    rows, qs = _wide_case(n, dim)
    data = oracle.from_rows(rows)
    want = [oracle.batch_knn_dot(q, data, k) for q in qs]
    run = _f32_run(B, innr, "dot", lambda: rows, ("f32", "wide"), qs, want, k, innr.KNN_EXACT)
    _check_residue("two-select-levels", run, ("sel_tmp0", "sel_tmp1", "selcnt_tmp0", "selcnt_tmp1"))


@functools.lru_cache(maxsize=1)
def _wide_case(n, dim):
    return _ro(oracle.generate_uniform(n, dim, 61), oracle.generate_uniform(1, dim, 62))


# =============================================================================== f32 secondary entry points
@functools.lru_cache(maxsize=1)
def _half_mask():
    return _ro((np.random.default_rng(7).random(N) < 0.5).astype(np.uint8))


def _uniform_rows():
    return _i8_rows(D, "uniform")[0]


def _uniform_data():
    return _i8_rows(D, "uniform")[1]


def _on_uniform(B, fresh):
    return _resident(("f32", D, "uniform"), lambda: B.VerticalBatch.from_rows(_uniform_rows()), fresh)


@pytest.mark.parametrize("engine,metric", [("KNN_EXACT", 1), ("KNN_MFMA", 0)], ids=["exact-l2", "mfma-dot-on-selection"])
def test_knn_filtered_multi(B, innr, ctx_option, engine, metric):
    ctx_option("no_split_filter", 1)
    qs, mask = _i8_queries(D, 3), _half_mask()
    want = _masked_expected(metric, _uniform_rows(), mask, qs, 10)

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            st = innr.KnnStats()
            idx, sc = B.batch_knn_filtered_multi(qs, vb, 10, mask, metric=metric, engine=getattr(innr, engine), stats=st)
        for j, (oi, os_) in enumerate(want):
            assert idx[j].tolist() == oi.tolist() and bits_equal(sc[j], os_), (engine, j)
        assert st.engine == getattr(innr, engine)
        return Out((idx, sc), _stats(st))
    _check_residue(f"filtered-multi-{engine}", run, ("flt_in", "flt_mask", "flt_scan"))


def test_knn_filtered_and_reordered(B):
    q, mask = _i8_queries(D, 1)[0], _half_mask()
    want_f = oracle.batch_knn_filtered(q, _uniform_data(), 10, mask)
    want_r = oracle.batch_knn_reordered(q, _uniform_data(), 10)
    want_v = oracle.batch_dimension_variance(_uniform_data())

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            f = B._l2_variant("innr_batch_knn_filtered", q, vb, 10, B._vp(mask))
            r = B.batch_knn_reordered(q, vb, 10)  # (its dimension variances are cached per batch: a fresh batch computes them)
            v = B.batch_dimension_variance(vb)
        fi, fs = np.array(f.indices, np.uint64), np.array(f.scores, np.float32)
        ri, rs = np.array(r.indices, np.uint64), np.array(r.scores, np.float32)
        assert same_knn("l2", fi, fs, *want_f) and same_knn("l2", ri, rs, *want_r) and bits_equal(v, want_v)
        return Out((fi, fs, ri, rs, v))
    _check_residue("filtered+reordered+variance", run, ("tmp_norms", "misc", "q_row"))


def test_scores_norms_and_pruning(B):
    q = _i8_queries(D, 1)[0]
    data = _uniform_data()
    norms = oracle.batch_norms(data)
    want = (oracle.batch_dot(q, data), oracle.batch_l2_squared(q, data), oracle.batch_cosine(q, data, norms))
    thr = float(np.sort(want[1])[300])
    want_p = oracle.batch_l2_squared_pruning(q, data, thr)

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            dot, l2 = B.batch_dot(q, vb), B.batch_l2_squared(q, vb)
            cos_given = B.batch_cosine(q, vb, norms)                      # the caller's norms, staged in tmp_norms
            cos_own = B._scores(B.METRIC_COSINE, q, vb)                    # the batch's own (computed once per batch)
            nrm = B.batch_norms(vb)
            pruned = B.batch_l2_squared_pruning(q, vb, thr)
        pi, ps = np.array([p[0] for p in pruned], np.uint64), np.array([p[1] for p in pruned], np.float32)
        assert bits_equal(dot, want[0]) and bits_equal(l2, want[1]) and bits_equal(cos_given, want[2]) and bits_equal(cos_own, want[2])
        assert bits_equal(nrm, norms) and pi.tolist() == want_p[0].tolist() and bits_equal(ps, want_p[1])
        return Out((dot, l2, cos_given, cos_own, nrm, pi, ps))
    _check_residue("scores+norms+pruning", run, ("scores", "tmp_norms", "q_norm", "counts"))


RANGE_CASES = [  # id, metric (INNR_METRIC_*), queries, engine, max_results (None: everything, 0: count only)
    ("exact-l2-q3", RS.L2, 3, "KNN_EXACT", None), ("exact-cos-q9", RS.COS, 9, "KNN_EXACT", None),
    ("collect-dot-q9", RS.DOT, 9, "KNN_MFMA", None), ("collect-l2-q9-cap", RS.L2, 9, "KNN_MFMA", 500),
    ("exact-dot-q3-cap", RS.DOT, 3, "KNN_EXACT", 5), ("exact-l2-q9-count-only", RS.L2, 9, "KNN_EXACT", 0),
    ("collect-cos-q3-count-only", RS.COS, 3, "KNN_MFMA", 0),
]


@functools.lru_cache(maxsize=None)
def _range_case(metric, nq):
    qs = _i8_queries(D, nq)
    scores = RS._all_scores(metric, _uniform_rows(), qs)
    thr = RS._rank_thresholds(metric, scores, (0, 1, 10, 300, 250, None))
    return _ro(qs, thr) + (RS._expected(metric, _uniform_rows(), qs, thr, scores=scores),)


@pytest.mark.parametrize("cid,metric,nq,engine,cap", RANGE_CASES, ids=[c[0] for c in RANGE_CASES])
def test_range_search(B, innr, cid, metric, nq, engine, cap):
    qs, thr, (eo, ei, es) = _range_case(metric, nq)
    total = int(eo[-1])
    assert cap is None or cap < total
    room = total if cap is None else cap

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            st = innr.KnnStats()
            off, idx, sc = B.batch_range_search(qs, vb, thr, metric=metric, engine=getattr(innr, engine), stats=st, max_results=cap)
        assert off.tolist() == eo.tolist(), cid
        assert np.array_equal(np.asarray(idx, np.uint64), ei[:room]) and bits_equal(sc, es[:room]), cid
        assert st.engine == (innr.KNN_MFMA if engine == "KNN_MFMA" else innr.KNN_EXACT)
        return Out((off, idx, sc), _stats(st))
    _check_residue(f"range-{cid}", run, ("rs_cnt", "rs_tot", "rs_thr", "rs_off") + (("rs_bits", "sort_keys") if engine == "KNN_MFMA" else ()))


def test_knn_adaptive(B, innr):
    qs = _i8_queries(D, 2)
    want = [oracle.batch_knn_adaptive(q, _uniform_data(), 10, 32) for q in qs]

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            st = innr.KnnStats()
            idx, sc = B.batch_knn_adaptive_multi(qs, vb, 10, 32, stats=st)
        for j, (oi, os_) in enumerate(want):
            assert idx[j].tolist() == oi.tolist() and bits_equal(sc[j], os_), j
        return Out((idx, sc), _stats(st))
    _check_residue("adaptive", run, ("adp_scan", "adp_list", "scores", "sort_keys", "sort_tmp"))


ROW_IDS = np.array([0, 311, 311, 2000, 42, 8299, 5, 640, 17], np.uint64)


@pytest.mark.parametrize("exclude,engine,metric", [(0, "KNN_EXACT", "l2"), (1, "KNN_MFMA", "dot")], ids=["with-self-exact", "exclude-self-mfma"])
def test_knn_rows_and_gather(B, innr, ctx_option, exclude, engine, metric):
    ctx_option(*SEED256)
    ctx_option("no_split_filter", 1)
    rows, data, k = _uniform_rows(), _uniform_data(), 10
    want = []
    for i in ROW_IDS:
        oi, os_ = ORACLE_KNN[metric](rows[int(i)], data, k + exclude)
        want.append(strip(oi, os_, int(i)) if exclude else (oi, os_))

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            st = innr.KnnStats()
            idx, sc = B.batch_knn_rows(ROW_IDS, vb, k, metric=getattr(innr, {"l2": "METRIC_L2SQ", "dot": "METRIC_DOT"}[metric]),
                                       exclude_self=bool(exclude), engine=getattr(innr, engine), stats=st)
            got = vb.rows(ROW_IDS)
        _assert_knn(metric, idx, sc, want, ("rows", exclude))
        assert bits_equal(got, rows[ROW_IDS.astype(np.int64)])
        return Out((idx, sc, got), _stats(st))
    _check_residue(f"knn_rows-exclude{exclude}", run, ("rows_q", "rows_io", "rows_flag") + (("rows_stage",) if exclude else ()))


@pytest.mark.parametrize("kc", [20, 300])  # candidate lists (<= 256), and the segmented sort beyond them
def test_rerank(B, innr, kc):
    qs = _i8_queries(D, 3)
    cand = np.stack([np.random.default_rng(kc + j).permutation(N)[:kc] for j in range(3)]).astype(np.uint64)
    wi, wb = _rerank_ref("cos", _score_bits("cos", qs, _uniform_data()), cand, 10)

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            idx, sc = B.batch_rerank(qs, vb, cand, 10, innr.METRIC_COSINE)
        assert np.array_equal(idx, wi) and np.array_equal(sc.view(np.uint32), wb), kc
        return Out((idx, sc))
    _check_residue(f"rerank-kc{kc}", run, ("q_row", "q_norm", "out_idx", "out_score") + (("sort_keys", "sort_tmp") if kc > 256 else ("sel", "sel_cnt")))


def test_quantisation_on_the_device(B, S):
    rows = _uniform_rows()
    fit, fitq = oracle.qparams_fit(rows.reshape(-1)), oracle.qparams_fit_quantile(rows.reshape(-1), 0.99)
    want_codes = oracle.quantize_u8(rows, fit)

    def run(fresh):
        with _on_uniform(B, fresh) as vb:
            p, pq = S.fit_batch(vb), S.fit_quantile_batch(vb, 0.99)
            qc = S.QuantizedCorpus.from_batch(vb, p)
            codes = qc.codes()
            qc.close()
        assert (np.float32(p.alpha), np.float32(p.offset)) == (np.float32(fit.alpha), np.float32(fit.offset)), (p.alpha, p.offset)
        assert (np.float32(pq.alpha), np.float32(pq.offset)) == (np.float32(fitq.alpha), np.float32(fitq.offset)), (pq.alpha, pq.offset)
        assert np.array_equal(codes, want_codes)
        return Out((codes, float(p.alpha), float(p.offset), float(pq.alpha), float(pq.offset)))
    _check_residue("minmax+quantile+quantize", run, ("misc",))


# =============================================================================== mutations
MUTATIONS = ["update", "append-inside-padding", "append-past-padding", "keep"]


@functools.lru_cache(maxsize=None)
def _mutation_case(kind):
    """(the change's arguments, the final rows) on the uniform corpus: ldN = 8448 leaves 148 columns of padding"""
    rows = _uniform_rows()
    rng = np.random.default_rng(len(kind))
    if kind == "update":
        ids = rng.permutation(N)[:300].astype(np.uint64)
        new = rng.uniform(-1.0, 1.0, (300, D)).astype(np.float32)
        final = rows.copy()
        final[ids.astype(np.int64)] = new
        return (ids, new), final
    if kind.startswith("append"):
        more = rng.uniform(-1.0, 1.0, (100 if kind == "append-inside-padding" else 400, D)).astype(np.float32)
        return (more,), np.vstack([rows, more])
    mask = (rng.random(N) < 0.6).astype(np.uint8)
    return (mask,), rows[mask != 0].copy()


@pytest.mark.parametrize("kind", MUTATIONS)
def test_mutations(B, innr, ctx_option, kind):
    """the download and a k-NN (matrix pipe, seeded: norms, the filter copy and the seeds are rebuilt over poisoned workspace) after
    the change, against a fresh upload of the final rows and against the oracle on them"""
    ctx_option(*SEED256)
    ctx_option("no_split_filter", 1)
    args, final = _mutation_case(kind)
    qs = _i8_queries(D, 3)
    data = oracle.from_rows(final)
    want = [oracle.batch_knn_cosine(q, data, 10) for q in qs]

    def run(_fresh):  # (a change needs a batch of its own every time)
        vb = B.VerticalBatch.from_rows(_uniform_rows())
        B.batch_norms(vb)  # something derived, for the change to drop
        if kind == "update":
            vb.update_rows(*args)
        elif kind == "keep":
            assert vb.keep(*args) == final.shape[0]
        else:
            vb.append(*args)
        store = vb.data().copy()
        st = innr.KnnStats()
        idx, sc = B.batch_knn_cosine_multi(qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
        vb.close()
        fresh_vb = B.VerticalBatch.from_rows(final)
        fidx, fsc = B.batch_knn_cosine_multi(qs, fresh_vb, 10, engine=innr.KNN_MFMA)
        fstore = fresh_vb.data().copy()
        fresh_vb.close()
        assert bits_equal(store, final.T) and bits_equal(store, fstore), kind
        assert np.array_equal(idx, fidx) and bits_equal(sc, fsc), kind
        _assert_knn("cos", idx, sc, want, kind)
        return Out((store, idx, sc), _stats(st))
    _check_residue(f"mutate-{kind}", run, {"update": ("rows_bits", "rows_io", "rows_flag"), "keep": ("rows_map", "flt_in", "flt_mask", "flt_scan")}
                   .get(kind, ("rows_io",)))


# =============================================================================== u8 codes
QP = (2.0, -1.0)  # alpha, offset


@functools.lru_cache(maxsize=1)
def _u8_case():
    codes = _codes(N, D, 12)
    qs = oracle.generate_uniform(9, D, 322)
    return _ro(codes, qs) + (_ro(_u8_all_scores(codes, oracle.QParams(*QP), qs)),)


def _on_codes(S, fresh):
    codes = _u8_case()[0]
    return _resident(("u8", D), lambda: S.QuantizedCorpus.from_codes(codes, N, D, S.QuantizationParams(*QP)), fresh)


def _rank_desc(scores, ids, k):
    """(ids, scores[ids]) by (score descending, index ascending), the first k -- finite scores"""
    ids = np.asarray(ids, np.int64)
    order = np.lexsort((ids, -scores[ids].astype(np.float64)))[:k]
    return ids[order].astype(np.uint64), scores[ids][order]


def test_scores_u8(S):
    codes, qs, scores = _u8_case()

    def run(fresh):
        with _on_codes(S, fresh) as qc:
            got = qc.scores(qs[0])
        assert bits_equal(got, scores[0])
        return Out((got,))
    _check_residue("scores_u8", run, ("q_row", "q_norm", "scores"))


KNN_U8_CASES = [  # id, engine, k, options
    ("exact", "KNN_EXACT", 10, ()), ("mfma", "KNN_MFMA", 10, (SEED256,)), ("i8-one-limb", "KNN_MFMA_I8", 10, (SEED256, ("i8_no_small", 1))),
    ("i8-small", "KNN_MFMA_I8", 10, (SEED256,)), ("i8-two-limbs-k200", "KNN_MFMA_I8", 200, (SEED256,)),
]


@pytest.mark.parametrize("cid,engine,k,options", KNN_U8_CASES, ids=[c[0] for c in KNN_U8_CASES])
def test_knn_u8(S, innr, ctx_option, cid, engine, k, options):
    for name, value in options:
        ctx_option(name, value)
    codes, qs, _ = _u8_case()
    want = [_oracle_knn_u8(q, codes, *QP, k) for q in qs]

    def run(fresh):
        with _on_codes(S, fresh) as qc:
            st = innr.KnnStats()
            idx, sc = qc.knn_multi(qs, k, engine=getattr(innr, engine), stats=st)
        _assert_knn("dot", idx, sc, want, cid)
        assert st.engine == getattr(innr, engine)
        return Out((idx, sc), _stats(st))
    _check_residue(f"knn_u8-{cid}", run, EXACT_BUFS + (("q_bf16", "gthr") if "i8" in cid else ()))


@pytest.mark.parametrize("engine", ["KNN_EXACT", "KNN_MFMA_I8"], ids=["exact", "i8-on-selection"])
def test_knn_u8_filtered(S, innr, ctx_option, engine):
    codes, qs, scores = _u8_case()
    mask = _half_mask()
    passing = np.flatnonzero(mask)
    want = [_rank_desc(scores[j], passing, 10) for j in range(len(qs))]

    def run(fresh):
        with _on_codes(S, fresh) as qc:
            st = innr.KnnStats()
            idx, sc = qc.knn_filtered_multi(qs, 10, mask, engine=getattr(innr, engine), stats=st)
        _assert_knn("dot", idx, sc, want, engine)
        assert st.engine == getattr(innr, engine)
        return Out((idx, sc), _stats(st))
    _check_residue(f"knn_u8_filtered-{engine}", run, ("flt_in", "flt_mask", "flt_scan"))


@pytest.mark.parametrize("engine", ["KNN_EXACT", "KNN_MFMA_I8"], ids=["exact", "collect"])
def test_range_search_u8(S, innr, ctx_option, engine):
    ctx_option("range_u8_i8_min_n", 0)
    codes, qs, scores = _u8_case()
    thr = np.array([np.sort(scores[j])[::-1][r] for j, r in enumerate((0, 9, 299, 250, 0, 3000, 1, 50, 700))], np.float32)
    thr[4] = np.nextafter(thr[4], np.float32(np.inf))  # no hit
    eo, ei, es = _u8_range_expected(scores, thr)

    def run(fresh):
        with _on_codes(S, fresh) as qc:
            st = innr.KnnStats()
            off, idx, sc = qc.range_search(qs, thr, engine=getattr(innr, engine), stats=st)
        assert off.tolist() == eo.tolist() and np.asarray(idx, np.uint64).tolist() == ei.tolist() and bits_equal(sc, es), engine
        assert st.engine == getattr(innr, engine)
        return Out((off, idx, sc), _stats(st))
    _check_residue(f"range_u8-{engine}", run, ("rs_cnt", "rs_tot", "rs_thr", "rs_off") + (("rs_bits", "q_bf16") if engine != "KNN_EXACT" else ()))


# =============================================================================== maxsim: 300 documents x 40 tokens, ragged doc_len
MS_DOCS, MS_T = 300, 40


@functools.lru_cache(maxsize=None)
def _ms_case(dim):
    toks, lens = _ms_corpus(MS_DOCS, MS_T, dim, False, seed=23 if dim == 48 else 21)  # (the corpora of test_gpu_kernel_variants.py)
    return _ro(toks, lens)


def _on_docs(M, dim, fresh):
    toks, lens = _ms_case(dim)
    return _resident(("docs", dim), lambda: M.DocumentCorpus.from_tokens(toks, lens), fresh)


def _ms_topk_want(q, toks, lens, cosine, k):
    s = _oracle_scores(q, toks, lens, cosine=cosine)
    order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
    return order.astype(np.uint64), s[order]


@pytest.mark.parametrize("Tq", [5, 40])  # one pass, and two (the second adds to the first's totals)
def test_maxsim_scores(M, Tq):
    toks, lens = _ms_case(64)
    q = _ms_query(Tq, 64)
    want = [_oracle_scores(q, toks, lens, cosine=c) for c in (False, True)]

    def run(fresh):
        with _on_docs(M, 64, fresh) as dc:
            got = [dc.scores(q, cosine=c) for c in (False, True)]
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
        return Out(tuple(got))
    _check_residue(f"maxsim-scores-Tq{Tq}", run, ("q_row", "q_norm", "q_kmajor", "scores"))


MS_TOPK_CASES = [  # id, dim, engine, k, query tokens, what must have a size
    ("exact", 64, "KNN_EXACT", 10, 12, ("lists", "counts", "sel", "sel_cnt")), ("mfma-tile", 64, "KNN_MFMA", 10, 40, ("misc", "q_kmajor")),
    ("mfma-generic-dim48", 48, "KNN_MFMA", 10, 12, ("misc", "q_kmajor")), ("k241", 64, "KNN_EXACT", 241, 12, ("sort_keys", "sort_tmp")),
]


@pytest.mark.parametrize("cid,dim,engine,k,Tq,needs", MS_TOPK_CASES, ids=[c[0] for c in MS_TOPK_CASES])
def test_maxsim_topk(M, innr, cid, dim, engine, k, Tq, needs):
    toks, lens = _ms_case(dim)
    q = _ms_query(Tq, dim)
    want = [_ms_topk_want(q, toks, lens, c, k) for c in (False, True)]

    def run(fresh):
        out, stats = [], []
        with _on_docs(M, dim, fresh) as dc:
            for c in (False, True):
                st = innr.KnnStats()
                out += list(dc.topk(q, k, cosine=c, engine=getattr(innr, engine), stats=st))
                stats += list(_stats(st))
        for c in (0, 1):
            assert out[2 * c].tolist() == want[c][0].tolist() and bits_equal(out[2 * c + 1], want[c][1]), (cid, c)
        assert stats[0] == stats[3] == getattr(innr, engine)
        return Out(tuple(out), tuple(stats))
    _check_residue(f"maxsim-topk-{cid}", run, ("out_idx", "out_score", "scores") + needs)


def test_maxsim_topk_multi_and_rerank(M, innr):
    toks, lens = _ms_case(64)
    queries = [_ms_query(tq, 64, seed=100 + tq) for tq in (32, 5, 17, 1)]
    want = [_ms_topk_want(q, toks, lens, True, 10) for q in queries]
    cand = np.stack([np.random.default_rng(31 + j).permutation(MS_DOCS)[:20] for j in range(4)]).astype(np.uint64)
    po = PairOracle(queries, toks, lens, False)
    want_r = [po.expect(j, cand[j], 7) for j in range(4)]

    def run(fresh):
        with _on_docs(M, 64, fresh) as dc:
            st = innr.KnnStats()
            idx, sc = dc.topk_multi(queries, 10, cosine=True, engine=innr.KNN_MFMA, stats=st)
            ridx, rsc = dc.rerank(queries, cand, 7, cosine=False)
        for j in range(4):
            assert idx[j].tolist() == want[j][0].tolist() and bits_equal(sc[j], want[j][1]), j
            assert ridx[j].tolist() == want_r[j][0].tolist() and bits_equal(rsc[j], want_r[j][1]), j
        return Out((idx, sc, ridx, rsc), _stats(st))
    _check_residue("maxsim-topk_multi+rerank", run, ("q_row", "q_kmajor", "misc", "sort_keys", "sort_tmp", "out_idx", "out_score"))


# =============================================================================== merge (one process, no collective)
def test_merge(innr):
    import torch
    from innr_amd.dist import _gpu_merge, gpu_merge_blocks, gpu_pack_block
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()
    dev, ctx = torch.device("cuda", 0), _ctx()
    k, nq, counts = 8, 3, (1000, 900, 0, 5)
    idx, bits, valid, bases = _shard_lists("dot", counts, k, nq, [0x3F800000, 0x3F800000, 0xBF800000, 0x3F000000, 0x40400000], seed=3)
    wi, wb = _merge_want("dot", idx, bits, valid, k)

    def run(_fresh):
        di, ds = _to_dev(dev, idx, bits)
        ti, tb = _from_dev(*_gpu_merge(ctx, innr.METRIC_DOT)(di, ds, k))
        blocks = []
        for g, count in enumerate(counts):
            kin = min(k, count)
            bi, bs = _to_dev(dev, idx[g, :, :kin], bits[g, :, :kin])
            blocks.append(gpu_pack_block(ctx, bi, bs, bases[g], count, k))
        mi, mb = gpu_merge_blocks(ctx, innr.METRIC_DOT, torch.stack(blocks), nq, k)
        torch.cuda.synchronize()
        mi, mb = _from_dev(mi, mb)
        assert np.array_equal(ti, wi) and np.array_equal(tb, wb) and np.array_equal(mi, wi) and np.array_equal(mb, wb)
        return Out((ti, tb, mi, mb))
    _check_residue("merge", run)  # (the merge entry points use no workspace buffer but `flags`: nothing to reach)


# =============================================================================== error paths leave nothing behind
def _good_neighbours(B, innr, ctx_option):
    """a good call of another family: the f32 filter's k-NN of three queries (seeded, proof, no fallback)"""
    ctx_option(*SEED256)
    ctx_option("no_split_filter", 1)
    want = _i8_oracle(D, "uniform", "dot", 3, 10)
    return _f32_run(B, innr, "dot", _uniform_rows, ("f32", D, "uniform"), _i8_queries(D, 3), want, 10, innr.KNN_MFMA)


def _around_a_failure(name, fail, same_family, other_family):
    """the two good calls clean, the failing call, the two good calls again: same answers (the runs compare with the oracle), same
    stats and records"""
    from innr_amd._lib import InnrError
    before = [_observe(run, False) for run in (same_family, other_family)]
    with pytest.raises(InnrError):
        fail()
    after = [_observe(run, False) for run in (same_family, other_family)]
    for b, a, which in zip(before, after, ("the same family", "another family")):
        assert _same_answer(a.answer, b.answer), f"{name}: a good call of {which} answers differently after the failed call"
        assert a.sig == b.sig, f"{name}: a good call of {which} after the failed call\n  before {b.sig}\n  after  {a.sig}"


def test_failed_rerank_leaves_nothing(B, innr, ctx_option):
    qs = _i8_queries(D, 3)
    cand = np.stack([np.random.default_rng(j).permutation(N)[:20] for j in range(3)]).astype(np.uint64)
    wi, wb = _rerank_ref("dot", _score_bits("dot", qs, _uniform_data()), cand, 10)
    bad = cand.copy()
    bad[1, 7] = N  # the first index outside the batch

    def good(fresh):
        with _on_uniform(B, fresh) as vb:
            idx, sc = B.batch_rerank(qs, vb, cand, 10, innr.METRIC_DOT)
        assert np.array_equal(idx, wi) and np.array_equal(sc.view(np.uint32), wb)
        return Out((idx, sc))

    def fail():
        with _on_uniform(B, False) as vb:
            B.batch_rerank(qs, vb, bad, 10, innr.METRIC_DOT)
    _around_a_failure("rerank", fail, good, _good_neighbours(B, innr, ctx_option))


def test_failed_maxsim_rerank_leaves_nothing(B, M, innr, ctx_option):
    toks, lens = _ms_case(64)
    queries = [_ms_query(tq, 64, seed=100 + tq) for tq in (32, 5, 17)]
    cand = np.stack([np.random.default_rng(41 + j).permutation(MS_DOCS)[:20] for j in range(3)]).astype(np.uint64)
    po = PairOracle(queries, toks, lens, True)
    want = [po.expect(j, cand[j], 7) for j in range(3)]
    bad = cand.copy()
    bad[2, 0] = MS_DOCS
    dc = M.DocumentCorpus.from_tokens(toks, lens)

    def good(_fresh):
        idx, sc = dc.rerank(queries, cand, 7, cosine=True)
        for j in range(3):
            assert idx[j].tolist() == want[j][0].tolist() and bits_equal(sc[j], want[j][1]), j
        return Out((idx, sc))
    try:
        _around_a_failure("maxsim rerank", lambda: dc.rerank(queries, bad, 7, cosine=True), good, _good_neighbours(B, innr, ctx_option))
    finally:
        dc.close()


def test_failed_gather_leaves_nothing(B, innr, ctx_option):
    """the device entry point: the host one checks its indices before anything moves"""
    import torch
    torch.zeros(1, device="cuda:0")
    rows = _uniform_rows()
    ids = torch.from_numpy(ROW_IDS.astype(np.int64)).to("cuda:0")
    bad = ids.clone()
    bad[4] = N

    def good(fresh):
        with _on_uniform(B, fresh) as vb:
            got = vb.rows(ids).cpu().numpy()
        assert bits_equal(got, rows[ROW_IDS.astype(np.int64)])
        return Out((got,))

    def fail():
        with _on_uniform(B, False) as vb:
            vb.rows(bad)
    _around_a_failure("gather_rows_dev", fail, good, _good_neighbours(B, innr, ctx_option))


def test_failed_update_leaves_nothing(B, innr, ctx_option):
    (ids, new), final = _mutation_case("update")
    twice = ids.copy()
    twice[5] = twice[250]
    vb = B.VerticalBatch.from_rows(_uniform_rows())
    data = oracle.from_rows(final)
    qs = _i8_queries(D, 3)
    want = [oracle.batch_knn_dot(q, data, 10) for q in qs]

    def good(_fresh):
        """the good update (the same rows again: idempotent), and the batch answers like the oracle on the final rows"""
        vb.update_rows(ids, new)
        st = innr.KnnStats()
        idx, sc = B.batch_knn_dot_multi(qs, vb, 10, engine=innr.KNN_EXACT, stats=st)
        _assert_knn("dot", idx, sc, want, "after update")
        return Out((vb.data().copy(), idx, sc), _stats(st))
    try:
        _around_a_failure("update_rows", lambda: vb.update_rows(twice, new), good, _good_neighbours(B, innr, ctx_option))
        assert bits_equal(vb.data(), final.T)  # the refused call wrote nothing
    finally:
        vb.close()


# =============================================================================== every buffer has a case
def test_every_workspace_buffer_was_grown_by_a_case():
    """runs last. The file began with a trimmed workspace; a buffer of workspace_bufs() that is still empty now has no case here.
    (Buffers that only the sharded collectives grow would be exempt: there are none -- comm.hip keeps its own.)"""
    sizes = _sizes()
    _GROWN.update(n for n, b in sizes.items() if b)
    empty = [n for n in sizes if n not in _GROWN]
    print(f"{len(sizes) - len(empty)} of {len(sizes)} workspace buffers grown by this file; never grown: {empty}")
    assert not empty, f"workspace buffers without a case in this file: {empty}"
