"""GPU tests of innr_batch_knn_filtered_multi (batch_knn_filtered, batch.rs:820-882, for Q queries and every metric and engine):
the exact engine scans the batch with the mask applied; the other engines search a SELECTION (the passing vectors compacted on
the device, kernels_select.h) and map the indices back. Bar: the oracle's answer per query -- orc_batch_knn_filtered for squared L2,
batch_knn_dot / batch_knn_cosine on the passing rows (indices mapped back) for the other two -- with identical indices and
bit-identical scores; the selection cache observed through the test hook innrdbg_filter_selection_builds."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal

EXACT, MFMA, BF16, I8, AUTO = 1, 2, 3, 4, 0  # INNR_KNN_*
DOT, L2, COS = 0, 1, 2                       # INNR_METRIC_*
ENGINES = (EXACT, MFMA, BF16, I8, AUTO)
METRICS = (L2, DOT, COS)


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


def _builds(vb) -> int:
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_filter_selection_builds
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p]
    return int(fn(vb._h))


def _masks(n, k, seed=7):
    rng = np.random.default_rng(seed)
    few = np.zeros(n, np.uint8)
    few[rng.choice(n, size=max(k - 3, 1), replace=False)] = 1
    return {
        "rand50": (rng.random(n) < 0.5).astype(np.uint8),
        "rand3": (rng.random(n) < 0.03).astype(np.uint8),
        "range": ((np.arange(n) >= n // 10) & (np.arange(n) < n // 10 + n // 3)).astype(np.uint8),
        "every7": (np.arange(n) % 7 == 0).astype(np.uint8),
        "all": np.ones(n, np.uint8),
        "none": np.zeros(n, np.uint8),
        "fewer_than_k": few,
    }


def _expected(metric, rows, mask, qs, k, base=0):
    """the reference's batch_knn_filtered per query (squared L2), or the batched dot / cosine kNN over the passing rows"""
    out = []
    if metric == L2:
        data = oracle.from_rows(rows)
        for q in qs:
            oi, os_ = oracle.batch_knn_filtered(q, data, k, mask)
            out.append((oi.astype(np.uint64) + np.uint64(base), os_))
        return out
    sel = np.nonzero(mask)[0]
    sub = oracle.from_rows(rows[sel]) if sel.size else np.empty((0, 0), np.float32)
    fn = oracle.batch_knn_dot if metric == DOT else oracle.batch_knn_cosine
    for q in qs:
        if sel.size == 0:
            out.append((np.empty(0, np.uint64), np.empty(0, np.float32)))
            continue
        oi, os_ = fn(q, sub, k)
        out.append((sel[oi.astype(np.int64)].astype(np.uint64) + np.uint64(base), os_))
    return out


def _assert_same(idx, sc, exp, what):
    assert idx.shape[0] == len(exp), what
    for j, (oi, os_) in enumerate(exp):
        assert idx[j].tolist() == oi.tolist(), f"{what} q={j}: indices {idx[j][:8].tolist()} != {oi[:8].tolist()}"
        assert bits_equal(sc[j], os_), f"{what} q={j}: scores differ"


def _run(B, vb, qs, k, mask, metric, engine):
    from innr_amd import KnnStats
    st = KnnStats()
    idx, sc = B.batch_knn_filtered_multi(qs, vb, k, mask, metric=metric, engine=engine, stats=st)
    return idx, sc, st


# ------------------------------------------------------------------------------------------------ 1. parity matrix
SIZES = [(3000, 33, 7), (20001, 128, 130), (60000, 96, 1)]


@pytest.mark.parametrize("mask_name", list(_masks(10, 10)))
@pytest.mark.parametrize("n,dim,nq", SIZES, ids=lambda v: str(v))
def test_parity_matrix(B, n, dim, nq, mask_name):
    k = 10
    rows = oracle.generate_uniform(n, dim, 11)
    qs = oracle.generate_uniform(nq, dim, 12)
    mask = _masks(n, k)[mask_name]
    npass = int(mask.sum())
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for metric in METRICS:
            exp = _expected(metric, rows, mask, qs, k)
            for engine in ENGINES:
                idx, sc, st = _run(B, vb, qs, k, mask, metric, engine)
                what = f"metric={metric} engine={engine} mask={mask_name}"
                assert idx.shape == (nq, min(k, npass)), what
                _assert_same(idx, sc, exp, what)
                if engine in (MFMA, BF16, I8) and npass >= 1000:
                    assert st.engine != EXACT, f"{what}: the selection was not searched by a matrix-pipe engine"
                if engine == EXACT and npass:
                    assert st.engine == EXACT, what
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 2. the one-query entry point
def test_agrees_with_one_query_function(B):
    n, dim, k = 3000, 33, 12
    rows = oracle.generate_uniform(n, dim, 21)
    qs = oracle.generate_uniform(9, dim, 22)
    mask = _masks(n, k)["rand50"]
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for engine in (EXACT, MFMA, AUTO):
            idx, sc, _ = _run(B, vb, qs, k, mask, L2, engine)
            for j, q in enumerate(qs):
                r = B.batch_knn_filtered(q, vb, k, lambda i: bool(mask[i]))
                assert idx[j].tolist() == r.indices, f"engine={engine} q={j}"
                assert bits_equal(sc[j], np.float32(r.scores)), f"engine={engine} q={j}"
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 3. large k
@pytest.mark.parametrize("metric", METRICS)
def test_large_k(B, metric):
    n, dim = 12000, 40
    rows = oracle.generate_uniform(n, dim, 31)
    qs = oracle.generate_uniform(3, dim, 32)
    rng = np.random.default_rng(3)
    wide = (rng.random(n) < 0.4).astype(np.uint8)   # npass ~ 4800 > k = 300
    narrow = np.zeros(n, np.uint8)
    narrow[rng.choice(n, 500, replace=False)] = 1    # npass = 500 < k = 1000: k' = 500 > INNR_MAX_K
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for mask, k in ((wide, 300), (narrow, 1000), (narrow, 300)):
            exp = _expected(metric, rows, mask, qs, k)
            for engine in ENGINES:
                idx, sc, _ = _run(B, vb, qs, k, mask, metric, engine)
                assert idx.shape == (3, min(k, int(mask.sum())))
                _assert_same(idx, sc, exp, f"engine={engine} k={k} npass={int(mask.sum())}")
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 4. special values
@pytest.mark.parametrize("metric", (L2, DOT))  # cosine of an inf row divides inf / inf (tests/test_gpu_exact.py pins that sign)
def test_special_values_order_like_total_cmp(B, metric):
    n, dim = 5000, 16
    rows = oracle.generate_uniform(n, dim, 41)
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    neg_nan = np.uint32(0xFFC00000).view(np.float32)
    for i, (d, v) in {30: (3, np.nan), 32: (0, np.inf), 33: (0, -np.inf), 35: (5, neg_nan),  # passing (i % 3 != 1)
                      31: (2, np.nan), 34: (1, np.inf), 37: (4, -np.inf)}.items():          # masked out
        rows[i, d] = v
    rows[38] = -0.0
    rows[39] = 0.0
    rows[40] = -0.0  # masked out
    qs = oracle.generate_uniform(5, dim, 42)
    qs[0] = 0.0
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for k in (8, 300):
            exp = _expected(metric, rows, mask, qs, k)
            for engine in ENGINES:
                idx, sc, _ = _run(B, vb, qs, k, mask, metric, engine)
                _assert_same(idx, sc, exp, f"metric={metric} engine={engine} k={k}")
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 5. the selection cache
def test_selection_cache(B, ctx_option):
    n, dim, k = 70000, 64, 10
    rows = oracle.generate_uniform(n, dim, 51)
    qs = oracle.generate_uniform(16, dim, 52)
    rng = np.random.default_rng(5)
    mask = (rng.random(n) < 0.2).astype(np.uint8)
    scaled = mask * rng.integers(1, 256, n).astype(np.uint8)  # the same predicate, other non-zero bytes
    other = mask.copy()
    other[np.nonzero(mask)[0][7]] = 0
    exp = _expected(DOT, rows, mask, qs, k)
    exp_other = _expected(DOT, rows, other, qs, k)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        assert _builds(vb) == 0
        for m in (mask, mask, scaled, mask.astype(bool)):
            idx, sc, st = _run(B, vb, qs, k, m, DOT, MFMA)
            _assert_same(idx, sc, exp, "cache hit")
            assert st.engine != EXACT
        assert _builds(vb) == 1, "the same mask built a second selection"
        idx, sc, _ = _run(B, vb, qs, k, other, DOT, MFMA)
        _assert_same(idx, sc, exp_other, "other mask")
        assert _builds(vb) == 2
        # the exact engine and the all-pass mask never build one
        _run(B, vb, qs, k, mask, DOT, EXACT)
        _run(B, vb, qs, k, np.ones(n, np.uint8), DOT, MFMA)
        assert _builds(vb) == 2
        ctx_option("filter_keep_selection", 0)  # (the selection of `other` is still cached: `mask` builds anew, every time)
        for _ in range(2):
            idx, sc, _ = _run(B, vb, qs, k, mask, DOT, MFMA)
            _assert_same(idx, sc, exp, "filter_keep_selection = 0")
        assert _builds(vb) == 4, "filter_keep_selection = 0 must rebuild on every call"
    finally:
        vb.close()


def test_option_filter_keep_selection_default():
    from innr_amd import _lib
    assert _lib.default_context().get_option("filter_keep_selection") == 1


# ------------------------------------------------------------------------------------------------ 6. index base, prefix view
def test_index_base(B):
    n, dim, k = 20001, 64, 10
    rows = oracle.generate_uniform(n, dim, 61)
    qs = oracle.generate_uniform(20, dim, 62)
    mask = _masks(n, k)["every7"]
    base = 5_000_000_000
    vb = B.VerticalBatch.from_rows(rows)
    try:
        vb.set_index_base(base)
        for metric in METRICS:
            exp = _expected(metric, rows, mask, qs, k, base=base)
            for engine in (EXACT, MFMA, AUTO):
                idx, sc, _ = _run(B, vb, qs, k, mask, metric, engine)
                _assert_same(idx, sc, exp, f"metric={metric} engine={engine}")
    finally:
        vb.close()


def test_prefix_view_parent(B):
    n, dim, p, k = 20000, 96, 40, 10  # p % 32 != 0: the view itself has no GEMM engine, its selection does
    rows = oracle.generate_uniform(n, dim, 71)
    qs = oracle.generate_uniform(70, p, 72)
    mask = _masks(n, k)["rand50"]
    vb = B.VerticalBatch.from_rows(rows)
    view = vb.prefix(p)
    try:
        sub = np.ascontiguousarray(rows[:, :p])
        for metric in METRICS:
            exp = _expected(metric, sub, mask, qs, k)
            for engine in (EXACT, MFMA, BF16, I8):
                idx, sc, st = _run(B, view, qs, k, mask, metric, engine)
                _assert_same(idx, sc, exp, f"metric={metric} engine={engine}")
                if engine != EXACT:
                    assert st.engine != EXACT, "the selection of a prefix view must take a GEMM engine"
    finally:
        view.close()
        vb.close()


# ------------------------------------------------------------------------------------------------ 7. device entry point
def test_dev_variant_matches_host(B):
    import torch
    n, dim, k = 30000, 64, 10
    rows = oracle.generate_uniform(n, dim, 81)
    qs = oracle.generate_uniform(33, dim, 82)
    mask = _masks(n, k)["rand3"]
    vb = B.VerticalBatch.from_rows(rows)
    try:
        dq = torch.from_numpy(qs).cuda()
        for metric in METRICS:
            for engine in (EXACT, MFMA, AUTO):
                hi, hs, _ = _run(B, vb, qs, k, mask, metric, engine)
                for dm in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(bool)).cuda()):
                    di, ds, _ = _run(B, vb, dq, k, dm, metric, engine)
                    torch.cuda.synchronize()
                    assert di.is_cuda and di.shape == (33, min(k, int(mask.sum())))
                    assert np.array_equal(di.cpu().numpy().view(np.uint64), hi), f"metric={metric} engine={engine}"
                    assert bits_equal(ds.cpu().numpy(), hs), f"metric={metric} engine={engine}"
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 8. errors
def test_errors(B):
    from innr_amd import _lib, scalar as S
    from innr_amd._lib import InnrPanic
    n, dim = 1000, 16
    rows = oracle.generate_uniform(n, dim, 91)
    qs = oracle.generate_uniform(2, dim, 92)
    mask = np.ones(n, np.uint8)
    vb = B.VerticalBatch.from_rows(rows)
    L = _lib.load()
    idx = np.empty(2 * 10, np.uint64)
    sc = np.empty(2 * 10, np.float32)
    out_k = C.c_size_t(7)
    try:
        with pytest.raises(InnrPanic):  # dimension mismatch (batch.rs:829)
            B.batch_knn_filtered_multi(qs[:, :15], vb, 10, mask)
        with pytest.raises(InnrPanic):  # short mask
            B.batch_knn_filtered_multi(qs, vb, 10, mask[:-1])
        assert L.innr_batch_knn_filtered_multi(vb._h, L2, qs.ctypes.data, 2, dim - 1, 10, mask.ctypes.data, AUTO, idx.ctypes.data,
                                               sc.ctypes.data, C.byref(out_k), None) == _lib.E_DIM_MISMATCH
        # the dimension check comes before the mask check
        assert L.innr_batch_knn_filtered_multi(vb._h, L2, qs.ctypes.data, 2, dim - 1, 10, None, AUTO, idx.ctypes.data,
                                               sc.ctypes.data, C.byref(out_k), None) == _lib.E_DIM_MISMATCH
        assert L.innr_batch_knn_filtered_multi(vb._h, L2, qs.ctypes.data, 2, dim, 10, None, AUTO, idx.ctypes.data,
                                               sc.ctypes.data, C.byref(out_k), None) == _lib.E_BAD_ARG
        assert L.innr_batch_knn_filtered_multi_dev(vb._h, L2, qs.ctypes.data, 2, dim, 10, None, AUTO, idx.ctypes.data,
                                                   sc.ctypes.data, C.byref(out_k), None) == _lib.E_BAD_ARG
        out_k.value = 7  # k == 0: *out_k = 0 (batch.rs:831)
        assert L.innr_batch_knn_filtered_multi(vb._h, L2, qs.ctypes.data, 2, dim, 0, mask.ctypes.data, AUTO, idx.ctypes.data,
                                               sc.ctypes.data, C.byref(out_k), None) == _lib.OK and out_k.value == 0
        p = S.QuantizationParams.from_range(-1.0, 1.0)
        codes = oracle.quantize_u8(rows, oracle.QParams(p.alpha, p.offset))
        qc = S.QuantizedCorpus.from_codes(codes, n, dim, p)
        try:
            assert L.innr_batch_knn_filtered_multi(qc._h, L2, qs.ctypes.data, 2, dim, 10, mask.ctypes.data, AUTO, idx.ctypes.data,
                                                   sc.ctypes.data, C.byref(out_k), None) == _lib.E_BAD_ARG
        finally:
            qc.close()
    finally:
        vb.close()


def test_empty_batch(B):
    vb = B.VerticalBatch.from_flat(np.empty(0, np.float32), 0, 8)
    try:
        idx, sc = B.batch_knn_filtered_multi(np.ones((3, 8), np.float32), vb, 5, np.empty(0, np.uint8))
        assert idx.shape == (3, 0) and sc.shape == (3, 0)
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ 9. one mid-size case
def test_mid_size_auto_on_selection(B):
    from innr_amd import KnnStats
    n, dim, nq, k = 1_000_000, 768, 1024, 10  # 10 %: a selection of ~100k vectors, where AUTO takes a matrix-pipe engine
    vb = B.VerticalBatch.generate(n, dim, seed=3)
    qs = oracle.generate_uniform(nq, dim, 93)
    mask = (np.random.default_rng(9).random(n) < 0.1).astype(np.uint8)
    try:
        b0 = _builds(vb)
        st = KnnStats()
        idx, sc = B.batch_knn_filtered_multi(qs, vb, k, mask, metric=DOT, engine=AUTO, stats=st)
        assert _builds(vb) == b0 + 1 and st.engine != EXACT, "AUTO did not run on the selection"
        sub = np.r_[0:32, nq - 32:nq]
        for metric in (DOT, L2):
            if metric != DOT:
                idx, sc = B.batch_knn_filtered_multi(qs, vb, k, mask, metric=metric, engine=AUTO)
            ei, es = B.batch_knn_filtered_multi(qs[sub], vb, k, mask, metric=metric, engine=EXACT)
            assert np.array_equal(idx[sub], ei), f"metric={metric}"
            assert bits_equal(sc[sub], es), f"metric={metric}"
        assert _builds(vb) == b0 + 1
    finally:
        vb.close()
