"""batch_knn_adaptive on the device (innr_batch_knn_adaptive / _dev) against the oracle's orc_batch_knn_adaptive: the same indices
in the same order with the same score bits, for every query of every case -- the reference's stable sort makes ties deterministic,
so nothing is compared as a set. tests/adaptive_ref.py (pinned against the oracle by tests/test_adaptive_abi.py) gives the alive
count after the warm-up prune that stats.candidates_kept reports."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import order_ref as R
from adaptive_ref import adaptive_ref


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def run(B, vb, qs, k, w, stats=None):
    idx, sc = B.batch_knn_adaptive_multi(np.atleast_2d(np.asarray(qs, np.float32)), vb, k, w, stats=stats)
    return idx, sc


def check(B, innr, rows, qs, k, w, vb=None, kept=True):
    """every query of qs through the ABI in one call == the oracle on that query alone; candidates_kept == the mirror's count"""
    rows = np.ascontiguousarray(rows, np.float32)
    qs = np.atleast_2d(np.asarray(qs, np.float32))
    data = oracle.from_rows(rows)
    own = vb is None
    if own:
        vb = B.VerticalBatch.from_rows(rows)
    try:
        st = innr.KnnStats()
        idx, sc = run(B, vb, qs, k, w, st)
        assert idx.shape == sc.shape == (len(qs), min(k, len(rows)))
        alive = 0
        for j, q in enumerate(qs):
            oi, os_ = oracle.batch_knn_adaptive(q, data, k, w)
            assert idx[j].tolist() == oi.tolist(), (j, k, w, idx[j][:8], oi[:8])
            assert np.array_equal(R.bits(sc[j]), R.bits(os_)), (j, k, w)
            if kept:
                alive = max(alive, adaptive_ref(q, data, k, w)[2])
        assert st.engine == innr.KNN_EXACT and st.queries_fallback == 0
        assert st.total_ms > 0.0 and st.gemm_ms > 0.0 and st.gemm_ms <= st.total_ms
        if kept:
            assert st.candidates_kept == alive
        return idx, sc
    finally:
        if own:
            vb.close()


# ---- the reference's own known answers (batch.rs:1512-1570, tests/batch_tests.rs:268-290) through the ABI -------------------------
def test_reference_known_answers(B):
    assert B.batch_knn_adaptive([], B.VerticalBatch.from_rows([]), 5, 2).indices == []
    assert B.batch_knn_adaptive([1, 2], B.VerticalBatch.from_rows([[1, 2]]), 0, 1).indices == []
    vb = B.VerticalBatch.from_rows([[0, 0, 0, 0], [100, 100, 100, 100], [0.1, 0.1, 0.1, 0.1]])
    assert B.batch_knn_adaptive([0, 0, 0, 0], vb, 1, 2).indices[0] == 0
    vb = B.VerticalBatch.from_rows([[0.0, 1.0]])
    assert B.batch_knn_adaptive([0, 0], vb, 1, 1) == B.batch_knn([0, 0], vb, 1)
    vb = B.VerticalBatch.from_flat([], 3, 0)  # three zero-dimensional vectors
    r = B.batch_knn_adaptive([], vb, 2, 1)
    assert r.indices == [0, 1] and r.scores == [0.0, 0.0]
    rows = [[float(i), math.sin(i * 0.1), math.cos(i * 0.1)] for i in range(100)]
    vb = B.VerticalBatch.from_rows(rows)
    basic = B.batch_knn([50, 0, 1], vb, 10).indices
    adapt = B.batch_knn_adaptive([50, 0, 1], vb, 10, 1)
    assert set(basic) <= set(adapt.indices)
    oi, os_ = oracle.batch_knn_adaptive([50, 0, 1], oracle.from_rows(rows), 10, 1)
    assert adapt.indices == oi.tolist() and np.array_equal(R.bits(adapt.scores), R.bits(os_))


# ---- uniform data: the guard alive_count > k binds in the middle of a chunk, the answer depends on index order --------------------
@pytest.mark.parametrize("n,dim,k,w,order_dependent", [(3000, 96, 10, 16, True), (3000, 96, 10, 40, True), (2000, 40, 5, 33, False),
                                                       (5000, 70, 100, 8, True)])
def test_uniform_ordered_cut(B, innr, n, dim, k, w, order_dependent):
    rows = oracle.generate_uniform(n, dim, 11)
    q = oracle.generate_uniform(1, dim, 12)
    idx, sc = check(B, innr, rows, q, k, w)
    if order_dependent:  # a call that silently ran the exact kNN would pass the oracle comparison only if the two agreed
        ei, _ = oracle.batch_knn(q[0], oracle.from_rows(rows), k)
        assert sorted(idx[0].tolist()) != sorted(ei.tolist())


# ---- more than one workgroup, one scan block and one radix pass; k above the candidate-list sizes ---------------------------------
@pytest.fixture(scope="module")
def big(B):
    rows = oracle.generate_uniform(70001, 130, 21)
    vb = B.VerticalBatch.from_rows(rows)
    yield rows, vb
    vb.close()


@pytest.mark.parametrize("k", [1, 300])
def test_beyond_one_workgroup(B, innr, big, k):
    rows, vb = big
    check(B, innr, rows, oracle.generate_uniform(1, 130, 22), k, 20, vb=vb)


# ---- segment boundaries: an update right after the first phase-2 dimension, none at all, W >= D ---------------------------------
@pytest.fixture(scope="module")
def seg(B):
    rows = oracle.generate_uniform(1200, 97, 31)
    vb = B.VerticalBatch.from_rows(rows)
    yield rows, vb
    vb.close()


@pytest.mark.parametrize("w", [1, 31, 32, 33, 64, 65, 96, 97, 200])
def test_segment_boundaries(B, innr, seg, w):
    rows, vb = seg
    q = oracle.generate_uniform(1, 97, 32)
    idx, sc = check(B, innr, rows, q, 7, w, vb=vb)
    if w >= 97:  # clamped: no second phase, every distance is complete at the prune. The exact answer wherever no tie straddles the cut
        ei, es = oracle.batch_knn(q[0], oracle.from_rows(rows), 8)
        if R.bits(es)[6] != R.bits(es)[7]:
            assert sorted(idx[0].tolist()) == sorted(ei[:7].tolist()) and np.array_equal(R.bits(sc[0]), R.bits(es[:7]))


# ---- k >= N, k = N - 1, N = 1 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(257, 257), (257, 1000), (257, 256), (1, 1), (1, 3)])
def test_k_at_the_corpus_size(B, innr, n, k):
    check(B, innr, oracle.generate_uniform(n, 50, 41), oracle.generate_uniform(1, 50, 42), k, 9)


# ---- exact ties -------------------------------------------------------------------------------------------------------------------
def test_ties_on_a_half_grid(B, innr):
    rows = (np.round(oracle.generate_uniform(4000, 48, 51) * 4) / 2).astype(np.float32)
    q = (np.round(oracle.generate_uniform(2, 48, 52) * 4) / 2).astype(np.float32)
    check(B, innr, rows, q, 64, 8)


def test_ties_of_duplicated_rows(B, innr):
    """every row twice: ties straddle the ordered cut (equal death dimensions, resolved by list position) and the final cut"""
    half = oracle.generate_uniform(1500, 48, 53)
    for rows in (np.repeat(half, 2, axis=0), np.concatenate([half, half])):  # neighbours, and 1500 apart
        for k in (9, 64):  # odd: the final cut splits a pair
            check(B, innr, rows, oracle.generate_uniform(1, 48, 54), k, 8)


# ---- special values ---------------------------------------------------------------------------------------------------------------
def _special_rows():
    rows = oracle.generate_uniform(1500, 70, 61).copy()
    u = rows.view(np.uint32)
    # (row, dimension): in the warm-up (W = 12) and after it; one special value per row
    for r, d, pat in ((3, 2, R.PNAN), (40, 5, R.NNAN), (77, 1, R.PINF), (130, 7, R.NINF), (200, 20, R.PNAN), (333, 33, R.NNAN),
                      (510, 40, R.PINF), (511, 64, R.NINF), (900, 69, R.PNAN), (1499, 32, R.NNAN), (1000, 4, R.PINF), (1001, 50, R.PINF)):
        u[r, d] = np.uint32(pat)
    return rows


@pytest.mark.parametrize("qkind", ["plain", "inf_in_warmup", "inf_later"])
@pytest.mark.parametrize("k", [5, 40])
def test_special_values(B, innr, qkind, k):
    rows = _special_rows()
    q = oracle.generate_uniform(1, 70, 62).copy()
    if qkind == "inf_in_warmup":
        q[0, 4] = np.inf   # row 1000: inf - inf, a generated NaN; every other row: +inf from the warm-up on
    elif qkind == "inf_later":
        q[0, 50] = np.inf  # row 1001: inf - inf at dimension 50
    check(B, innr, rows, q, k, 12)


@pytest.mark.parametrize("pat", [R.NNAN, R.PNAN])
def test_nan_threshold_prunes_nothing(B, innr, pat):
    """the k-th warm-up distance is NaN: the threshold is NaN, no comparison against it holds, and all N vectors stay alive until a
    later update brings a number"""
    n, dim, w = 1500, 70, 12
    rows = oracle.generate_uniform(n, dim, 63).copy()
    q = oracle.generate_uniform(1, dim, 64)
    if pat == R.NNAN:  # -NaN sorts first: five of them, k = 3
        rows.view(np.uint32)[[10, 500, 900, 1200, 1400], 3] = np.uint32(pat)
        k = 3
    else:              # +NaN sorts last: ten of them, k = N - 4
        rows.view(np.uint32)[np.arange(10) * 149, 3] = np.uint32(pat)
        k = n - 4
    data = oracle.from_rows(rows)
    warm = oracle.batch_l2_squared(q[0, :w], np.ascontiguousarray(data[:w]))
    kth = R.f32(R.bits(warm)[np.argsort(R.total_key(R.bits(warm)), kind="stable")[k - 1:k]])[0]
    assert np.isnan(kth)
    st = innr.KnnStats()
    vb = B.VerticalBatch.from_rows(rows)
    run(B, vb, q, k, w, st)
    assert st.candidates_kept == n
    check(B, innr, rows, q, k, w, vb=vb)
    vb.close()


# ---- decaying variance: where the heuristic works -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_decaying_variance(B, innr, seed):
    n, dim, k, w = 20000, 128, 10, 32
    rng = np.random.default_rng(seed)
    s = (np.float32(0.9) ** np.arange(dim, dtype=np.float32)).astype(np.float32)
    rows = rng.standard_normal((n, dim)).astype(np.float32) * s
    q = (rng.standard_normal((1, dim)).astype(np.float32) * s).astype(np.float32)
    idx, _ = check(B, innr, rows, q, k, w)
    ei, _ = oracle.batch_knn(q[0], oracle.from_rows(rows), k)
    print(f"decaying variance seed {seed}: recall against batch_knn {len(set(idx[0].tolist()) & set(ei.tolist())) / k:.2f}")


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plumb(B):
    rows = oracle.generate_uniform(3000, 96, 71)
    vb = B.VerticalBatch.from_rows(rows)
    yield rows, vb, oracle.generate_uniform(5, 96, 72)
    vb.close()


def test_five_queries_equal_five_calls(B, innr, plumb):
    rows, vb, qs = plumb
    idx, sc = check(B, innr, rows, qs, 10, 16, vb=vb)
    for j in range(5):
        r = B.batch_knn_adaptive(qs[j], vb, 10, 16)
        assert r.indices == idx[j].tolist() and np.array_equal(R.bits(r.scores), R.bits(sc[j]))


def test_device_entry_point_equals_host(B, innr, plumb):
    import torch
    rows, vb, qs = plumb
    st = innr.KnnStats()
    didx, dsc = B.batch_knn_adaptive_multi(torch.from_numpy(qs).cuda(), vb, 10, 16, stats=st)
    idx, sc = run(B, vb, qs, 10, 16)
    assert didx.is_cuda and np.array_equal(didx.cpu().numpy().astype(np.uint64), idx)
    assert np.array_equal(R.bits(dsc.cpu().numpy()), R.bits(sc))
    assert st.candidates_kept == max(adaptive_ref(q, oracle.from_rows(rows), 10, 16)[2] for q in qs)


def test_index_base(B, innr, plumb):
    rows, _, qs = plumb
    vb = B.VerticalBatch.from_rows(rows)
    vb.set_index_base(1 << 33)
    idx, sc = run(B, vb, qs[:2], 10, 16)
    vb.close()
    for j in range(2):
        oi, os_ = oracle.batch_knn_adaptive(qs[j], oracle.from_rows(rows), 10, 16)
        assert (idx[j] - np.uint64(1 << 33)).tolist() == oi.tolist() and np.array_equal(R.bits(sc[j]), R.bits(os_))


def test_prefix_view(B, innr, plumb):
    rows, vb, qs = plumb
    view = vb.prefix(64)
    check(B, innr, rows[:, :64], qs[:2, :64], 10, 16, vb=view)  # D, and the extrapolation factor, are the view's: 64 / 16
    check(B, innr, rows[:, :64], qs[:1, :64], 10, 100, vb=view)  # the warm-up is clamped to the view's 64 dimensions
    view.close()


def test_repeat_after_trim(B, innr, plumb):
    from innr_amd import _lib
    rows, vb, qs = plumb
    a = run(B, vb, qs, 10, 16)
    ctx = _lib.default_context()
    assert ctx.memory() > 0
    ctx.trim()
    b = run(B, vb, qs, 10, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(R.bits(a[1]), R.bits(b[1]))
    assert ctx.memory() >= 12 * 3000  # the call's workspace is the context's: warm-up distances and sort keys at least


def test_statuses(B, innr, plumb):
    from innr_amd import _lib
    from innr_amd import scalar as S
    rows, vb, qs = plumb
    lib = _lib.load()
    idx, sc = np.zeros(16, np.uint64), np.zeros(16, np.float32)
    out_k = C.c_size_t(7)

    def call(h, q, nq, d, k, w):
        q = np.ascontiguousarray(q, np.float32)
        return lib.innr_batch_knn_adaptive(h, C.c_void_p(q.ctypes.data), nq, d, k, w, C.c_void_p(idx.ctypes.data), C.c_void_p(sc.ctypes.data),
                                           C.byref(out_k), None)

    assert call(vb._h, qs[0], 1, 95, 10, 16) == _lib.E_DIM_MISMATCH
    assert call(vb._h, qs[0], 1, 96, 10, 0) == _lib.E_DIM_MISMATCH and "warmup_dims must be > 0" in _lib.last_error()
    empty = B.VerticalBatch.from_flat([], 0, 96)
    assert call(empty._h, qs[0], 1, 96, 10, 0) == _lib.E_DIM_MISMATCH and "warmup_dims must be > 0" in _lib.last_error()
    assert call(empty._h, qs[0], 1, 96, 10, 4) == _lib.OK and out_k.value == 0
    assert call(empty._h, qs[0], 1, 95, 10, 4) == _lib.E_DIM_MISMATCH  # the dimension check comes first
    assert call(None, qs[0], 1, 96, 10, 4) == _lib.E_BAD_ARG
    assert lib.innr_batch_knn_adaptive(vb._h, None, 1, 96, 10, 4, C.c_void_p(idx.ctypes.data), C.c_void_p(sc.ctypes.data), C.byref(out_k),
                                       None) == _lib.E_BAD_ARG
    assert lib.innr_batch_knn_adaptive(vb._h, C.c_void_p(qs.ctypes.data), 1, 96, 10, 4, None, None, C.byref(out_k), None) == _lib.E_BAD_ARG
    assert call(vb._h, qs[0], 0, 96, 10, 4) == _lib.OK and out_k.value == 0
    p = S.QuantizationParams.from_range(-1.0, 1.0)
    qc = S.QuantizedCorpus.from_codes(oracle.quantize_u8(rows[:64], oracle.QParams(p.alpha, p.offset)), 64, 96, p)
    assert call(qc._h, qs[0], 1, 96, 10, 4) == _lib.E_BAD_ARG
    assert lib.innr_batch_knn_adaptive_dev(qc._h, None, 1, 96, 10, 4, None, None, C.byref(out_k), None) == _lib.E_BAD_ARG
    with pytest.raises(_lib.InnrPanic):
        B.batch_knn_adaptive(qs[0][:95], vb, 10, 16)
    with pytest.raises(_lib.InnrPanic, match="warmup_dims must be > 0"):
        B.batch_knn_adaptive(qs[0], vb, 10, 0)
