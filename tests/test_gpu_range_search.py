"""GPU tests of innr_batch_range_search (batch_l2_squared_pruning, batch.rs:320-365, for Q queries with a threshold each, every
metric): the exact engine (range_scan_kernel: count per chunk, scan, emit) and the collect path (one MODE 2 pass of the f32 GEMM
filter, exact re-score, bitmap finish; overflowing or gated queries finished by the exact scan). Bar: the oracle as it is --
orc_batch_l2_squared_pruning per query for squared L2, batch_dot / batch_cosine over batch_norms and ~(s < thr) for the other two
-- with identical offsets and indices and bit-identical scores.

Unless a test says otherwise, query j's threshold is its own r-th best oracle score (the boundary vector scores exactly the
threshold and must be included), r cycling through: beyond the best (no hit), 1, 10, 300, about 3 % of N, worse than the worst
(every vector)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal

EXACT, MFMA, BF16, I8, AUTO = 1, 2, 3, 4, 0  # INNR_KNN_*
DOT, L2, COS = 0, 1, 2                       # INNR_METRIC_*
METRICS = (L2, DOT, COS)
F = np.float32


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


# ------------------------------------------------------------------------------------------------ the oracle side
def _scores(metric, q, data, norms):
    if metric == L2:
        return oracle.batch_l2_squared(q, data)
    return oracle.batch_dot(q, data) if metric == DOT else oracle.batch_cosine(q, data, norms)


def _all_scores(metric, rows, qs):
    data = oracle.from_rows(rows)
    norms = oracle.batch_norms(data) if metric == COS else None
    return [_scores(metric, q, data, norms) for q in qs]


def _expected(metric, rows, qs, thr, base=0, scores=None):
    """(offsets uint64 [Q+1], indices uint64, scores f32) of the whole batch, query after query"""
    data = oracle.from_rows(rows)
    scores = scores if scores is not None else _all_scores(metric, rows, qs)
    off, idx, sc = [0], [], []
    for q, t, s in zip(qs, thr, scores):
        if metric == L2:
            oi, os_ = oracle.batch_l2_squared_pruning(q, data, float(t))
        else:
            keep = ~(s < F(t))
            oi, os_ = np.nonzero(keep)[0].astype(np.uint64), s[keep]
        idx.append(oi.astype(np.uint64) + np.uint64(base))
        sc.append(os_)
        off.append(off[-1] + len(oi))
    return np.array(off, np.uint64), np.concatenate(idx), np.concatenate(sc).astype(np.float32)


def _rank_thresholds(metric, scores, ranks):
    """query j's threshold: its ranks[j % len]-th best score; 0 = one step beyond the best, None = one step past the worst"""
    thr = np.empty(len(scores), np.float32)
    for j, s in enumerate(scores):
        o = np.sort(s) if metric == L2 else np.sort(s)[::-1]
        toward_better = F(-np.inf) if metric == L2 else F(np.inf)
        r = ranks[j % len(ranks)]
        if r == 0:
            thr[j] = np.nextafter(o[0], toward_better)
        elif r is None:
            thr[j] = np.nextafter(o[-1], -toward_better)
        else:
            thr[j] = o[min(r, len(o)) - 1]
    return thr


def _ranks(n):
    return (0, 1, 10, 300, max(1, (3 * n) // 100), None)


@functools.lru_cache(maxsize=None)
def _case(n, dim, nq, metric):
    rows = oracle.generate_uniform(n, dim, 31)
    qs = oracle.generate_uniform(nq, dim, 32)
    scores = _all_scores(metric, rows, qs)
    thr = _rank_thresholds(metric, scores, _ranks(n))
    exp = _expected(metric, rows, qs, thr, scores=scores)
    for a in (rows, qs, thr) + exp:
        a.setflags(write=False)
    return rows, qs, thr, exp


def _run(B, vb, qs, thr, metric, engine, **kw):
    from innr_amd import KnnStats
    st = KnnStats()
    off, idx, sc = B.batch_range_search(qs, vb, thr, metric=metric, engine=engine, stats=st, **kw)
    return off, idx, sc, st


def _assert_same(got, exp, what):
    off, idx, sc = got[:3]
    eo, ei, es = exp
    assert off.tolist() == eo.tolist(), f"{what}: offsets {off[:8].tolist()} != {eo[:8].tolist()}"
    assert np.array_equal(np.asarray(idx, np.uint64), ei), f"{what}: indices differ"
    assert bits_equal(sc, es), f"{what}: scores differ"


# ------------------------------------------------------------------------------------------------ 1. parity matrix
SHAPES = [(1, 5, 3), (255, 32, 9), (3000, 33, 7), (20001, 128, 130), (60000, 96, 1)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,dim,nq", SHAPES, ids=lambda v: str(v))
def test_parity_matrix(B, n, dim, nq, metric):
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for engine in (EXACT, MFMA, AUTO):
            got = _run(B, vb, qs, thr, metric, engine)
            _assert_same(got, exp, f"metric={metric} engine={engine} shape={(n, dim, nq)}")
            if engine == EXACT:
                assert got[3].engine == EXACT and got[3].queries_fallback == 0
            if engine == MFMA:
                assert got[3].engine == MFMA, "an MFMA request on a plain batch runs a collect pass"
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 2. the one-query function
def test_q1_l2_equals_pruning(B):
    n, dim = 3000, 33
    rows = oracle.generate_uniform(n, dim, 41).copy()
    rows[7, 20] = np.nan  # a NaN that arrives after the partial sum has passed a small threshold: the full distance decides
    qs = oracle.generate_uniform(4, dim, 42)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for q in qs:
            d = oracle.batch_l2_squared(q, oracle.from_rows(rows))
            for t in (np.sort(d)[0], np.sort(d)[99], np.sort(d)[-2], F(0.0), F(np.nan)):
                pairs = B.batch_l2_squared_pruning(q, vb, float(t))
                assert 7 in [p[0] for p in pairs]
                for engine in (EXACT, MFMA, AUTO):
                    off, idx, sc, _ = _run(B, vb, q, [t], L2, engine)
                    assert off.tolist() == [0, len(pairs)]
                    assert idx.tolist() == [p[0] for p in pairs]
                    assert bits_equal(sc, np.array([p[1] for p in pairs], np.float32))
    finally:
        vb.close()


def test_kat_pruning_through_range_search(B):
    """the reference's own pruning tests (tests/kat_cases.py: kat_pruning), driven through the new entry point with Q = 1"""
    from backends import HipBackend
    from kat_cases import kat_pruning

    for engine in (EXACT, MFMA, AUTO):
        class Be(HipBackend):
            def batch_l2_squared_pruning(self, q, b, t):
                off, idx, sc = B.batch_range_search(np.asarray(q, np.float32), b, t, metric=L2, engine=engine)
                assert off.tolist() == [0, len(idx)]
                return np.asarray(idx, np.uint64), np.asarray(sc, np.float32)
        kat_pruning(Be())


# ------------------------------------------------------------------------------------------------ 3. near ties
@pytest.mark.parametrize("metric", METRICS)
def test_near_ties_lcg(B, metric):
    """the reference example's LCG rows (examples/batch_demo.rs:167: a one-parameter family): many vectors sit within the filter's
    error bound of every threshold, so the exact re-score decides who is in"""
    n, dim, nq = 20_000, 64, 70
    rows = oracle.generate_corpus(n, dim, 0)
    qs = oracle.generate_corpus(nq, dim, 1_000_003)
    scores = _all_scores(metric, rows, qs)
    thr = _rank_thresholds(metric, scores, (10,))
    exp = _expected(metric, rows, qs, thr, scores=scores)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        got = _run(B, vb, qs, thr, metric, MFMA)
        _assert_same(got, exp, f"LCG rows metric={metric}")
        assert got[3].engine == MFMA
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 4. list overflow
@pytest.mark.parametrize("metric", METRICS)
def test_list_overflow_takes_the_exact_path(B, metric):
    n, dim, nq = 70_000, 32, 5
    rows = oracle.generate_uniform(n, dim, 51)
    qs = oracle.generate_uniform(nq, dim, 52)
    scores = _all_scores(metric, rows, qs)
    # queries 1 and 3 pass everything: 70 000 > the 65 536 entries of a collected list; the others are selective
    thr = _rank_thresholds(metric, scores, (10, None, 300, None, 1))
    exp = _expected(metric, rows, qs, thr, scores=scores)
    assert (np.diff(exp[0].astype(np.int64)) == n).sum() == 2
    vb = B.VerticalBatch.from_rows(rows)
    try:
        got = _run(B, vb, qs, thr, metric, MFMA)
        _assert_same(got, exp, f"overflow metric={metric}")
        assert got[3].engine == MFMA and got[3].queries_fallback == 2
        assert got[3].candidates_kept == 65536
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 5. capacity
@pytest.mark.parametrize("engine", (EXACT, MFMA))
def test_capacity(B, engine):
    n, dim, nq, metric = 3000, 33, 7, DOT
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    total = int(exp[0][-1])
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for cap in (1, 17, total // 2, total - 1):
            off, idx, sc, _ = _run(B, vb, qs, thr, metric, engine, max_results=cap)
            assert off.tolist() == exp[0].tolist(), f"cap={cap}: the offsets are the full ones"
            assert len(idx) == cap and np.array_equal(np.asarray(idx, np.uint64), exp[1][:cap]) and bits_equal(sc, exp[2][:cap])
        off, idx, sc, _ = _run(B, vb, qs, thr, metric, engine, max_results=0)  # count only
        assert off.tolist() == exp[0].tolist() and len(idx) == 0 and len(sc) == 0
        _assert_same(_run(B, vb, qs, thr, metric, engine, max_results=total), exp, "cap = total")
        # the raw count-only call: null result buffers
        from innr_amd import _lib
        offs = np.zeros(nq + 1, np.uint64)
        tot = C.c_size_t(0)
        _lib.check(_lib.load().innr_batch_range_search(vb._h, metric, qs.ctypes.data, nq, dim, thr.ctypes.data, engine,
                                                       offs.ctypes.data, None, None, 0, C.byref(tot), None))
        assert tot.value == total and offs.tolist() == exp[0].tolist()
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 6. special values
def _special_rows(n, dim, neg_nan=True):
    """The NaNs sit in dimension 0 and no row / query pair has equal infinities in one later dimension: the reference (and the
    oracle) drops a vector as soon as a PARTIAL sum passes the threshold, which is the full-distance rule !(dist > thr) unless a
    partial sum passes it before a NaN arrives -- the one place where the two would differ (test_q1_l2_equals_pruning covers a
    late NaN against the one-query function, which has always used the full distance)."""
    rows = oracle.generate_uniform(n, dim, 61).copy()
    rows[3, 0] = np.nan
    rows[10, 0] = np.inf
    rows[11, 1] = -np.inf
    rows[12, :] = 0.0            # zero-norm rows
    rows[300, :] = 0.0
    if neg_nan:
        rows[13, 0] = -np.nan
    return rows


def _special_queries(dim, nan=True):
    """Query 1's NaN sits in a dimension where no row has one, and meets a NaN threshold (nothing is ever dropped on a partial
    sum). A +NaN query is never paired with a -NaN row: once the accumulator holds the row's NaN and the product brings the query's,
    the sum has two NaN operands, and which one an ISA hands on is its own business (x86: the first operand; the exact engine's
    arithmetic, unchanged here, may hand on the other) -- with equal bits that does not show, with opposite signs it does, in every
    exact entry point, innr_batch_scores included. Hence the three row / query sets of test_special_values."""
    qs = oracle.generate_uniform(8, dim, 62).copy()
    if nan:
        qs[1, 3] = np.nan
    qs[2, 0] = np.inf
    qs[3, 5] = -np.inf
    qs[4, :] = 0.0               # the zero query
    return qs


SPECIAL_THR = (F(0.25), F(np.nan), F(np.inf), F(-np.inf), F(0.0), F(-0.0), F(1.5), F(-np.nan))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("rows_kind", ("special", "nan_both", "plain"))
def test_special_values(B, metric, rows_kind):
    """NaN / +-inf in rows and queries, NaN and +-inf thresholds, zero-norm rows and a zero query: a non-finite corpus sends every
    query of an MFMA request to the exact scan; on a finite one only the queries with non-finite norms or thresholds go there.
    special: rows with +NaN, -NaN, +-inf and zero rows, queries with +-inf and zero; nan_both: the same rows without the -NaN one,
    the queries with a NaN one as well; plain: finite rows, all the special queries."""
    n, dim = 600, 16
    rows = oracle.generate_uniform(n, dim, 61) if rows_kind == "plain" else _special_rows(n, dim, neg_nan=rows_kind == "special")
    qs = _special_queries(dim, nan=rows_kind != "special")
    thr = np.array(SPECIAL_THR, np.float32)
    exp = _expected(metric, rows, qs, thr)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for engine in (EXACT, MFMA):
            got = _run(B, vb, qs, thr, metric, engine)
            _assert_same(got, exp, f"special values rows={rows_kind} metric={metric} engine={engine}")
            if engine == MFMA and rows_kind != "plain":
                assert got[3].engine == EXACT and got[3].queries_fallback == len(qs)
            if engine == MFMA and rows_kind == "plain":
                assert got[3].engine == MFMA and 3 <= got[3].queries_fallback < len(qs)
    finally:
        vb.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("row_scale,q_scale", [(1e-15, 1.0), (1e20, 1.0), (1.0, 1e-15), (1.0, 1e20), (1e-6, 1e-6)])
def test_norm_gates(B, metric, row_scale, q_scale):
    """norms below 1e-12 or above 1e18 (corpus: every query; query: that query) are outside the filter's bound: exact scan"""
    n, dim, nq = 3000, 24, 6
    rows = (oracle.generate_uniform(n, dim, 71) * F(row_scale)).astype(np.float32)
    qs = oracle.generate_uniform(nq, dim, 72).copy()
    qs[::2] *= F(q_scale)  # every other query scaled
    scores = _all_scores(metric, rows, qs)
    thr = _rank_thresholds(metric, scores, (10, 300, 1))
    exp = _expected(metric, rows, qs, thr, scores=scores)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for engine in (EXACT, MFMA):
            got = _run(B, vb, qs, thr, metric, engine)
            _assert_same(got, exp, f"norm gates rows*{row_scale} queries*{q_scale} metric={metric} engine={engine}")
        st = got[3]
        if row_scale != 1.0 and row_scale != 1e-6:
            assert st.engine == EXACT and st.queries_fallback == nq
        elif q_scale not in (1.0, 1e-6):
            assert st.engine == MFMA and st.queries_fallback >= 3
        else:
            assert st.engine == MFMA
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 7. base, views, device entry
def test_index_base(B):
    n, dim, nq, metric = 3000, 33, 7, L2
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    base = (1 << 33) + 12345
    vb = B.VerticalBatch.from_rows(rows)
    try:
        vb.set_index_base(base)
        for engine in (EXACT, MFMA):
            got = _run(B, vb, qs, thr, metric, engine)
            _assert_same(got, (exp[0], exp[1] + np.uint64(base), exp[2]), f"index base engine={engine}")
    finally:
        vb.close()


@pytest.mark.parametrize("metric", METRICS)
def test_prefix_views(B, metric):
    n, dim, nq = 5000, 96, 11
    rows = oracle.generate_uniform(n, dim, 81)
    qs = oracle.generate_uniform(nq, dim, 82)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for P, want_engine in ((64, MFMA), (33, EXACT)):
            prow, pq = np.ascontiguousarray(rows[:, :P]), np.ascontiguousarray(qs[:, :P])
            scores = _all_scores(metric, prow, pq)
            thr = _rank_thresholds(metric, scores, _ranks(n))
            exp = _expected(metric, prow, pq, thr, scores=scores)
            view = vb.prefix(P)
            try:
                got = _run(B, view, pq, thr, metric, MFMA)
                _assert_same(got, exp, f"prefix {P} metric={metric}")
                assert got[3].engine == want_engine, f"prefix {P}: a collect launch only if P % 32 == 0"
                _assert_same(_run(B, view, pq, thr, metric, EXACT), exp, f"prefix {P} metric={metric} exact")
            finally:
                view.close()
    finally:
        vb.close()


@pytest.mark.parametrize("engine", (EXACT, MFMA))
def test_device_entry_equals_host_entry(B, engine):
    import torch
    n, dim, nq, metric = 20001, 128, 130, COS
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        dev = torch.device("cuda", vb._ctx.device)
        tq = torch.from_numpy(np.array(qs)).to(dev)
        tt = torch.from_numpy(np.array(thr)).to(dev)
        off, idx, sc = B.batch_range_search(tq, vb, tt, metric=metric, engine=engine)
        assert off.is_cuda and idx.is_cuda and sc.is_cuda
        got = (off.cpu().numpy().astype(np.uint64), idx.cpu().numpy().astype(np.uint64), sc.cpu().numpy())
        _assert_same(got, exp, f"device entry engine={engine}")
        # a capacity below the total, on the device
        off2, idx2, sc2 = B.batch_range_search(tq, vb, tt, metric=metric, engine=engine, max_results=100)
        assert off2.cpu().numpy().tolist() == exp[0].tolist() and idx2.numel() == 100
        assert np.array_equal(idx2.cpu().numpy().astype(np.uint64), exp[1][:100]) and bits_equal(sc2.cpu().numpy(), exp[2][:100])
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 8. which kernel ran
_REC = np.dtype({"names": ["family", "lockstep", "arg", "groups"], "formats": ["u1", "u1", ("<i2", (4,)), "<u4"],
                 "offsets": [0, 1, 2, 12], "itemsize": 16})  # api_internal.h LaunchRec
GEMM_F32, RANGE_SCAN = 1, 11                                 # api_internal.h LaunchFamily


def _logged(call):
    """the launch records (raw: family, args, groups) of one call"""
    from conftest import hooks_lib
    from innr_amd import _lib
    L = hooks_lib()
    L.innrdbg_launch_log.restype = C.c_size_t
    L.innrdbg_launch_log.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.innrdbg_launch_log_reset.restype = None
    L.innrdbg_launch_log_reset.argtypes = [C.c_void_p]
    h = _lib.default_context().handle
    L.innrdbg_launch_log_reset(h)
    res = call()
    buf = np.zeros(64, _REC)
    total = C.c_uint64(0)
    n = L.innrdbg_launch_log(h, buf.ctypes.data, 64, C.byref(total))
    assert total.value == n
    return res, [(int(r["family"]), [int(a) for a in r["arg"]], int(r["groups"])) for r in buf[:n]]


@pytest.mark.parametrize("metric", METRICS)
def test_which_kernel_ran(B, metric):
    n, dim, nq = 20001, 128, 130
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        total = int(exp[0][-1])
        got, log = _logged(lambda: _run(B, vb, qs, thr, metric, MFMA, max_results=total))
        _assert_same(got, exp, "MFMA")
        kind = {DOT: 0, COS: 1, L2: 3}[metric]  # kernels_gemm.h: kGemmDot / kGemmCos / kGemmL2
        assert [(f, a[0], a[2]) for f, a, _ in log if f == GEMM_F32] == [(GEMM_F32, kind, 2)], log  # one MODE 2 launch
        assert not [r for r in log if r[0] == RANGE_SCAN], log
        got, log = _logged(lambda: _run(B, vb, qs, thr, metric, EXACT, max_results=total))
        _assert_same(got, exp, "EXACT")
        groups = (nq + 7) // 8
        assert log == [(RANGE_SCAN, [8, metric, 0, 0], groups), (RANGE_SCAN, [8, metric, 1, 0], groups)], log
        # AUTO with one query: the exact scan, one query per pass
        t1 = thr[2:3]
        e1 = _expected(metric, rows, qs[2:3], t1)
        got, log = _logged(lambda: _run(B, vb, qs[2:3], t1, metric, AUTO, max_results=int(e1[0][-1])))
        _assert_same(got, e1, "AUTO Q=1")
        assert log == [(RANGE_SCAN, [1, metric, 0, 0], 1), (RANGE_SCAN, [1, metric, 1, 0], 1)], log
        assert got[3].engine == EXACT
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 9. engine agreement at size
@pytest.mark.parametrize("metric", METRICS)
def test_engines_agree_at_size(B, metric):
    """1M x 128 generated on the device, 256 queries, thresholds = each query's 50th best score from the kNN call"""
    from innr_amd import GEN_UNIFORM
    n, dim, nq, k = 1_000_000, 128, 256, 50
    qs = oracle.generate_uniform(nq, dim, 92)
    vb = B.VerticalBatch.generate(n, dim, seed=91, generator=GEN_UNIFORM)
    try:
        kidx, ksc = B.knn_multi(metric, qs, vb, k)
        thr = np.ascontiguousarray(ksc[:, k - 1])
        a = _run(B, vb, qs, thr, metric, EXACT)
        m = _run(B, vb, qs, thr, metric, MFMA)
        assert m[3].engine == MFMA and m[3].queries_fallback == 0
        assert a[0].tolist() == m[0].tolist() and np.array_equal(a[1], m[1]) and bits_equal(a[2], m[2])
        off = a[0].astype(np.int64)
        assert (np.diff(off) >= k).all()
        for j in range(nq):
            mine = a[1][off[j]:off[j + 1]]
            assert (np.diff(mine.astype(np.int64)) > 0).all(), "ascending index order"
            assert np.isin(kidx[j], mine).all(), f"q={j}: the kNN call's indices are within the threshold"
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ several rounds
@pytest.mark.parametrize("engine", (EXACT, MFMA))
def test_more_queries_than_one_round(B, engine):
    """more than 4096 queries: the batch is worked off in rounds -- the running 64-bit base carried in the offsets, each round's
    queries, thresholds and offsets against round-local counts, flags and lists"""
    n, dim, nq, metric = 1000, 8, 4100, DOT
    rows, qs, thr, exp = _case(n, dim, nq, metric)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        got = _run(B, vb, qs, thr, metric, engine)
        _assert_same(got, exp, f"{nq} queries engine={engine}")
        assert got[3].engine == engine and got[3].queries_fallback == 0
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_checks(B):
    from innr_amd import InnrPanic
    from innr_amd import scalar as S
    rows = oracle.generate_uniform(100, 8, 1)
    qs = oracle.generate_uniform(3, 8, 2)
    vb = B.VerticalBatch.from_rows(rows)
    empty = B.VerticalBatch.from_rows([])
    try:
        with pytest.raises(InnrPanic):  # the dimension check comes first
            B.batch_range_search(qs[:, :7], vb, [0.0, 0.0, 0.0])
        with pytest.raises(InnrPanic):  # one threshold per query
            B.batch_range_search(qs, vb, [0.0, 0.0])
        off, idx, sc = B.batch_range_search(qs, vb, 1e9, metric=L2)  # a scalar threshold is broadcast
        assert off.tolist() == [0, 100, 200, 300] and idx.tolist() == list(range(100)) * 3
        off, idx, sc = B.batch_range_search(np.empty((0, 8), np.float32), vb, np.empty(0, np.float32))
        assert off.tolist() == [0] and len(idx) == 0
        off, idx, sc = B.batch_range_search(np.empty((2, 0), np.float32), empty, [1.0, 2.0])
        assert off.tolist() == [0, 0, 0] and len(idx) == 0
        p = S.QuantizationParams.from_range(-1.0, 1.0)
        qc = S.QuantizedCorpus.from_codes(oracle.quantize_u8(rows, oracle.QParams(p.alpha, p.offset)), 100, 8, p)
        from innr_amd import _lib
        offs, tot, thr = np.zeros(4, np.uint64), C.c_size_t(0), np.zeros(3, np.float32)
        st = _lib.load().innr_batch_range_search(qc._h, L2, qs.ctypes.data, 3, 8, thr.ctypes.data, AUTO, offs.ctypes.data, None, None, 0,
                                                 C.byref(tot), None)
        assert st == _lib.E_BAD_ARG  # a u8 code batch
        st = _lib.load().innr_batch_range_search(vb._h, L2, qs.ctypes.data, 3, 8, None, AUTO, offs.ctypes.data, None, None, 0,
                                                 C.byref(tot), None)
        assert st == _lib.E_BAD_ARG  # null thresholds with Q > 0
    finally:
        vb.close()
        empty.close()
