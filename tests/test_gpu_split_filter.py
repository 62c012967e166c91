"""GPU tests of the split-bf16 filter (kernels_gemm_bf16.h, LIMBS = 3): INNR_KNN_MFMA's dot / cosine filter
as hi.hi + hi.lo + lo.hi on the bf16 matrix pipe. Answers must be the oracle's, and bit for bit those of the f32 filter kernel
(context option no_split_filter = 1); the dense approximate scores must stay within the bound E the proof uses; the f32 kernel
keeps serving squared L2, small batches and the option."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import _check_knn, _corpus, _queries, bits_equal

F32_KERNEL, SPLIT_KERNEL = 1, 3  # innrdbg_last_filter (api.hip LastFilter)
SPLIT_MIN_Q = 65                 # api.hip kSplitMinQ


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _last_filter(vb):
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_last_filter
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p]
    return fn(vb._h)


def _split_scores(vb, metric, queries):
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_scores
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    q = np.ascontiguousarray(queries, np.float32)
    out = np.empty((q.shape[0], vb.num_vectors()), np.float32)
    _lib.check(fn(vb._h, metric, q.ctypes.data, q.shape[0], q.shape[1], out.ctypes.data))
    return out


def _knn(B, innr, metric, vb, qs, k):
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi, "l2": B.batch_knn_multi}[metric]
    return fn(qs, vb, k, engine=innr.KNN_MFMA)


def _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, qs, k, force=True):
    """the split filter serves the call (asserted through the hook), answers == oracle, and == the f32 kernel's bit for bit"""
    data = oracle.from_rows(rows)
    if force:
        ctx_option("split_min_q", 1)
    vb = _check_knn(B, innr, metric, rows, data, qs, k, innr.KNN_MFMA)
    assert _last_filter(vb) == SPLIT_KERNEL
    i1, s1 = _knn(B, innr, metric, vb, qs, k)
    assert _last_filter(vb) == SPLIT_KERNEL
    ctx_option("no_split_filter", 1)
    i0, s0 = _knn(B, innr, metric, vb, qs, k)
    assert _last_filter(vb) == F32_KERNEL
    ctx_option("no_split_filter", 0)
    assert np.array_equal(i0, i1) and bits_equal(s0, s1)
    return vb


# ------------------------------------------------------------------------------- answers
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("k", [1, 10, 16, 48, 100, 240])
def test_split_every_k(B, innr, ctx_option, metric, k):
    rows, _ = _corpus(20_000, 64, 3, uniform=True)
    _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, _queries(40, 64, 17, uniform=True), k)


@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("n,dim", [(3001, 1), (2049, 7), (5000, 33), (4000, 768), (3333, 1000)])
def test_split_dims_and_ragged_n(B, innr, ctx_option, metric, n, dim):
    rows, _ = _corpus(n, dim, 5, uniform=True)
    _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, _queries(33, dim, 23, uniform=True), 10)


@pytest.mark.parametrize("nq", [SPLIT_MIN_Q - 1, SPLIT_MIN_Q, 128, 512, 513, 1024])
def test_split_batch_sizes_and_crossover(B, innr, ctx_option, nq):
    # default options: the split filter from kSplitMinQ queries on, the f32 kernel's one-wave tile below
    rows, data = _corpus(30_000, 96, 7, uniform=True)
    qs = _queries(nq, 96, 29, uniform=True)
    for metric in ("dot", "cos"):
        if nq < SPLIT_MIN_Q:
            vb = _check_knn(B, innr, metric, rows, data, qs, 10, innr.KNN_MFMA)
            assert _last_filter(vb) == F32_KERNEL
        else:
            _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, qs, 10, force=False)


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_split_lcg_data(B, innr, ctx_option, metric):
    # the reference example's generator: near-ties at the cut, proofs fail for many queries, completion pass behind the split filter
    rows, _ = _corpus(20_000, 128, 0)
    _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, _queries(300, 128), 10, force=False)


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_split_tiny_elements_mixed_with_normal_ones(B, innr, ctx_option, metric):
    rows, _ = _corpus(8000, 48, 9, uniform=True)
    rng = np.random.default_rng(4)
    mask = rng.random(rows.shape) < 0.3
    rows = np.where(mask, rows * np.float32(1e-30), rows).astype(np.float32)  # lo limbs near 4e-33, products near 1e-30
    rows[:50] *= np.float32(1e-30)  # ... and whole rows of them
    qs = _queries(40, 48, 31, uniform=True)
    qs[:5] = np.where(rng.random((5, 48)) < 0.5, qs[:5] * np.float32(1e-30), qs[:5]).astype(np.float32)
    _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, qs, 10)


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_split_nonfinite_rows(B, innr, ctx_option, metric):
    rows, _ = _corpus(4000, 32, 1, uniform=True)
    rows[17, 3] = np.nan
    rows[300, 0] = np.inf
    rows[301, 5] = -np.inf
    _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, _queries(12, 32, 5, uniform=True), 5)


# ------------------------------------------------------------------------------- the bound
def _bound_check(vb, innr, rows, qs, metric):
    D = rows.shape[1]
    u = 2.0 ** -24
    rel = 1.05 * (3.1 * 2.0 ** -16 + (6 * D + 8) * u * 1.04)  # api.hip split_filter_scale, before |q| max|v|
    got = _split_scores(vb, innr.METRIC_DOT if metric == "dot" else innr.METRIC_COSINE, qs).astype(np.float64)
    if metric == "cos":
        # the filter's operands: rows and queries scaled by their f32 inverse norms (inv_norms_kernel / inv_qnorms_kernel)
        vn = oracle.batch_norms(oracle.from_rows(rows)).astype(np.float32)
        qn = np.sqrt((qs.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        v = (rows * (np.float32(1) / vn)[:, None]).astype(np.float32).astype(np.float64)
        q = (qs * (np.float32(1) / qn)[:, None]).astype(np.float32).astype(np.float64)
    else:
        v, q = rows.astype(np.float64), qs.astype(np.float64)
    exact = q @ v.T
    mag = np.abs(q) @ np.abs(v).T  # sum |q_d v_d|: the bound before Cauchy-Schwarz
    err = np.abs(got - exact)
    assert np.all(err <= rel * mag + 1e-37), (err / np.maximum(mag, 1e-300)).max() / rel
    # and the form the proof uses: E = split_scale |q| max|v| (cosine: split_scale)
    E = rel * (1.0 if metric == "cos" else np.sqrt((q ** 2).sum(1))[:, None] * np.sqrt((v ** 2).sum(1)).max())
    assert np.all(err <= E)
    return err.max(), np.max(E)


@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("dim", [7, 64, 768])
def test_split_bound_random(B, innr, metric, dim):
    rows, _ = _corpus(3000, dim, 11, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    _bound_check(vb, innr, rows, _queries(70, dim, 13, uniform=True), metric)


def _off_ties(rng, shape):
    # values just off bf16 rounding ties: a bf16 value plus half its last place, nudged by a few f32 places either way
    h = (rng.uniform(-2, 2, size=shape).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    half = (np.abs(h).view(np.uint32) & np.uint32(0x7F800000)).view(np.float32) * np.float32(2.0 ** -8)
    nudge = rng.integers(-3, 4, size=shape).astype(np.float32) * half * np.float32(2.0 ** -15)
    return (h + np.sign(h) * half + nudge).astype(np.float32)


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_split_bound_stressed_limbs(B, innr, metric):
    rng = np.random.default_rng(21)
    dim = 200
    rows = _off_ties(rng, (2000, dim))
    qs = _off_ties(rng, (40, dim))
    # wide exponent spread within a row: 2^-40 .. 2^40
    rows[1000:] *= np.exp2(rng.integers(-40, 41, size=(1000, dim))).astype(np.float32)
    qs[20:] *= np.exp2(rng.integers(-40, 41, size=(20, dim))).astype(np.float32)
    rows = rows.astype(np.float32)
    qs = qs.astype(np.float32)
    vb = B.VerticalBatch.from_rows(rows)
    _bound_check(vb, innr, rows, qs, metric)


# ------------------------------------------------------------------------------- the f32 kernel keeps its coverage
@pytest.mark.parametrize("waves", ["1", "2", "4", "8"])
def test_f32_kernel_block_shapes_every_metric(B, innr, ctx_option, waves):
    # test_gpu_mfma.py's block-shape matrix, with the split filter off: dot and cosine at 600 queries would take it otherwise
    rows, data = _corpus(70_000, 64, 31, uniform=True)
    ctx_option("no_split_filter", 1)
    ctx_option("gemm_waves", int(waves))
    vb = None
    for metric in ("dot", "cos", "l2"):
        vb = _check_knn(B, innr, metric, vb if vb is not None else rows, data, _queries(600, 64, 777, uniform=True), 10,
                        innr.KNN_MFMA)
        assert _last_filter(vb) == F32_KERNEL


def test_squared_l2_stays_on_the_f32_kernel(B, innr):
    rows, data = _corpus(30_000, 64, 8, uniform=True)
    vb = _check_knn(B, innr, "l2", rows, data, _queries(600, 64, 3, uniform=True), 10, innr.KNN_MFMA)
    assert _last_filter(vb) == F32_KERNEL


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_completion_pass_behind_the_split_filter(B, innr, ctx_option, metric):
    # every vector 40 times: the first pass (split filter) cannot prove the cut, the f32 collect pass (MODE 2) settles it
    base, _ = _corpus(1500, 96, 5, uniform=True)
    rows = np.repeat(base, 40, axis=0)
    rows[::7] *= np.float32(1.0 + 2.0 ** -20)
    qs = _queries(300, 96, 9, uniform=True)
    vb = _split_vs_oracle_and_f32(B, innr, ctx_option, metric, rows, qs, 10, force=False)
    st = innr.KnnStats()
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi}[metric]
    fn(qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    assert st.engine == innr.KNN_MFMA and st.queries_fallback > 8 and _last_filter(vb) == SPLIT_KERNEL
