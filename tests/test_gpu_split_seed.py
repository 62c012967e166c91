"""The split filter's own seeder (kernels_gemm_bf16.h: gemm_bf16_filter_kernel<6, 3, 3> and split_seed_kernel; api.hip seed_split;
DESIGN.md 4.4e): a prefix of the corpus scored on the matrix pipe, the best split score of every group of 32 rows kept, and the
k-th largest of a query's group maxima, less 2E, as its first chip-wide bound. The maxima and the seeds through a test hook
against numpy; the calls it seeds against the oracle, bit for bit; and a bound one rank too high must show as a wrong answer or a
failed proof. Context option split_seed_rows = 1024 seeds a corpus of 32 768 + 37 rows (ragged last tile)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import split_seed_ref as R
from test_gpu_exact import same_knn
from test_gpu_split_filter import SPLIT_KERNEL, _last_filter, _split_scores

N, P = 32768 + 37, 1024
SHAPES = [(40, 70), (200, 600)]  # (D, Q): one padded query tile, two query tiles
U = 2.0 ** -24


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _seed_hook(vb, metric, qs, k, rows):
    """(group maxima as floats [rows / 32][Q], seeds as order keys [Q], err_scale)"""
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_seed
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    q = np.ascontiguousarray(qs, np.float32)
    maxima = np.zeros((rows // 32, q.shape[0]), np.uint32)
    seeds = np.zeros(q.shape[0], np.uint32)
    info = np.zeros(1, np.float32)
    _lib.check(fn(vb._h, metric, q.ctypes.data, q.shape[0], q.shape[1], k, rows, maxima.ctypes.data, seeds.ctypes.data, info.ctypes.data))
    return R.key_to_f32(maxima), seeds, float(info[0])


def _served(vb):
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_seed_served
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p]
    return fn(vb._h)


_CACHE = {}


def _case(B, layout, dim, nq):
    """(rows, queries, batch) of a layout and shape, built once"""
    key = (layout, dim, nq)
    if key not in _CACHE:
        rows = R.corpus(layout, N, dim, 11)
        _CACHE[key] = (rows, R.queries(nq, dim, 5), B.VerticalBatch.from_rows(rows))
    return _CACHE[key]


def _operands(metric, rows, qs):
    """float64 operands of the filter's plain dot (cosine: rows and queries scaled by their f32 inverse norms)"""
    if metric == "cos":
        vn = oracle.batch_norms(oracle.from_rows(rows)).astype(np.float32)
        qn = np.sqrt((qs.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        return ((qs * (np.float32(1) / qn)[:, None]).astype(np.float32).astype(np.float64),
                (rows * (np.float32(1) / vn)[:, None]).astype(np.float32).astype(np.float64))
    return qs.astype(np.float64), rows.astype(np.float64)


# ------------------------------------------------------------------------------- the maxima and the seeds
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("dim,nq", SHAPES)
def test_maxima_and_seeds_against_numpy(B, innr, metric, layout, dim, nq):
    rows, qs, vb = _case(B, layout, dim, nq)
    m = innr.METRIC_DOT if metric == "dot" else innr.METRIC_COSINE
    dense = _split_scores(vb, m, qs)[:, :P].astype(np.float64)  # the filter's own scores (MODE 1), row by row
    want = R.group_maxima(dense)                                 # [Q][P / 32]
    q64, v64 = _operands(metric, rows, qs)
    mag = np.abs(q64) @ np.abs(v64[:P]).T
    gtol = (6 * dim + 8) * U * 1.04 * R.group_maxima(mag)        # per group: the accumulation term of the filter's bound
    tol = gtol.max(axis=1)                                       # per query (the k-th largest moves by at most the largest change)
    exact_all = q64 @ v64.T
    qn = np.sqrt((qs.astype(np.float64) ** 2).sum(1))
    for k in (1, 10, 32):
        got, seeds, err_scale = _seed_hook(vb, m, qs, k, P)
        assert got.shape == (P // 32, nq)
        d = np.abs(got.T.astype(np.float64) - want)
        print(f"{metric} {layout} D={dim} Q={nq} k={k}: max |maximum - numpy| / tol = {(d / gtol).max():.3g}")
        assert np.all(d <= gtol)
        E = err_scale * (1.0 if metric == "cos" else qn) * 1.0001
        t = R.kth_largest(want, k)
        assert np.all(seeds != 0)
        s = R.key_to_f32(seeds + np.uint32(1)).astype(np.float64)  # the seed is one key below key(t - 2E)
        ds = np.abs(s - (t - 2 * E))
        slack = tol + 4 * np.spacing(np.abs(t).astype(np.float32)).astype(np.float64) + 1e-6 * E
        print(f"   max |seed - (t - 2E)| / slack = {(ds / slack).max():.3g}")
        assert np.all(ds <= slack)
        kth = R.kth_largest(exact_all, k)                          # float64, of the whole corpus
        assert np.all(s <= kth - E), (s - (kth - E)).max()


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_seed_is_zero_for_a_nonfinite_query_norm(B, innr, metric):
    rows, qs, vb = _case(B, "random", 40, 70)
    qs = qs.copy()
    qs[3, 5] = np.inf
    qs[9, 0] = np.nan
    qs[11] = np.float32(3e38)  # finite values, a norm that overflows
    m = innr.METRIC_DOT if metric == "dot" else innr.METRIC_COSINE
    _, seeds, _ = _seed_hook(vb, m, qs, 10, P)
    assert seeds[3] == 0 and seeds[9] == 0 and seeds[11] == 0
    ok = np.ones(70, bool)
    ok[[3, 9, 11]] = False
    assert np.all(seeds[ok] != 0)


# ------------------------------------------------------------------------------- end to end
def _knn_vs_oracle(B, innr, metric, vb, rows, qs, ks, data=None, stats=None):
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi}[metric]
    ofn = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine}[metric]
    data = oracle.from_rows(rows) if data is None else data
    kmax = max(ks)
    want = [ofn(q, data, kmax) for q in qs]  # (a total order -- score, then index: the best k are a prefix of the best kmax)
    for k in ks:
        idx, sc = fn(qs, vb, k, engine=innr.KNN_MFMA, stats=stats)
        for j in range(len(qs)):
            oi, os_ = want[j]
            assert same_knn(metric, idx[j], sc[j], oi[:k], os_[:k]), (metric, k, j, idx[j], oi[:k])
        yield k


@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("dim,nq", SHAPES)
def test_seeded_calls_against_the_oracle(B, innr, ctx_option, metric, layout, dim, nq):
    rows, qs, vb = _case(B, layout, dim, nq)
    ctx_option("split_seed_rows", P)
    for k in _knn_vs_oracle(B, innr, metric, vb, rows, qs, (1, 10, 32)):
        assert _last_filter(vb) == SPLIT_KERNEL
        assert _served(vb) == P, k  # the new seeder served the call, with 1024 rows


def test_long_answers_and_the_off_switch_take_the_exact_seeder(B, innr, ctx_option):
    rows, qs, vb = _case(B, "random", 40, 70)
    ctx_option("split_seed_rows", P)
    for _ in _knn_vs_oracle(B, innr, "dot", vb, rows, qs, (100,)):  # 32 groups cannot certify 100 rows
        assert _last_filter(vb) == SPLIT_KERNEL and _served(vb) == 0
    for _ in _knn_vs_oracle(B, innr, "dot", vb, rows, qs, (10,)):
        assert _served(vb) == P
    ctx_option("gemm_seed_n", 256)  # a call that names its exact prefix keeps it
    for _ in _knn_vs_oracle(B, innr, "dot", vb, rows, qs, (10,)):
        assert _last_filter(vb) == SPLIT_KERNEL and _served(vb) == 0
    ctx_option("gemm_seed_n", 0)
    ctx_option("split_seed_rows", -1)
    for _ in _knn_vs_oracle(B, innr, "dot", vb, rows, qs, (10,)):
        assert _last_filter(vb) == SPLIT_KERNEL and _served(vb) == 0
    ctx_option("split_seed_rows", 0)  # the default prefix, clamped to the corpus: 1024 rows here as well
    for _ in _knn_vs_oracle(B, innr, "dot", vb, rows, qs, (10,)):
        assert _served(vb) == P


# ------------------------------------------------------------------------------- a seed one rank too high must show
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_seed_from_one_rank_too_high_would_show(B, innr, ctx_option, metric):
    """The prefix holds exactly k - 1 strong rows, each in a group of its own; the true k-th best is one medium row behind the
    prefix, far above every ordinary row. The k-th largest group maximum is an ordinary row's score: a valid bound. The (k - 1)-th
    is a strong row's: seeded from it, the filter rejects the medium row, and the answer is wrong or its proof fails."""
    dim, nq, k, medium_at = 200, 70, 10, 20_001
    rows = oracle.generate_uniform(N, dim, 23)
    strong_at = [R.group_rows(t // 4, t % 4, 4)[3] for t in range(k - 1)]  # groups 0 .. k - 2 of the prefix, one row each
    assert max(strong_at) < P and medium_at >= P and len({(r // 128, r % 4) for r in strong_at}) == k - 1
    rows[strong_at] = R.strong_rows(k - 1, dim, 29)
    rows[medium_at] = (1.0 + 0.8 * (-1.0) ** np.arange(dim)).astype(np.float32)  # (cosine: 6 % below the strong rows at the least)
    qs = R.queries(nq, dim, 31)
    # what the data is built to do, on the CPU: the medium row is every query's k-th best, clear of both neighbours
    q64, v64 = _operands(metric, rows, qs)
    exact = q64 @ v64.T
    order = np.argsort(-exact, axis=1)[:, :k + 1]
    assert np.all(order[:, k - 1] == medium_at)
    assert all(set(order[j, :k - 1]) == set(strong_at) for j in range(nq))
    s = np.take_along_axis(exact, order, axis=1)
    assert np.all(s[:, k - 2] - s[:, k - 1] > 0.05 * np.abs(s[:, k - 1])) and np.all(s[:, k - 1] - s[:, k] > 0.05 * np.abs(s[:, k - 1]))
    gm = R.group_maxima(exact[:, :P])  # ... and lies between the k-th and the (k - 1)-th largest group maximum of the prefix
    assert np.all(R.kth_largest(gm, k) < 0.9 * s[:, k - 1]) and np.all(R.kth_largest(gm, k - 1) > 1.05 * s[:, k - 1])
    vb = B.VerticalBatch.from_rows(rows)
    ctx_option("split_seed_rows", P)
    st = innr.KnnStats()
    for _ in _knn_vs_oracle(B, innr, metric, vb, rows, qs, (k,), stats=st):
        assert _last_filter(vb) == SPLIT_KERNEL and _served(vb) == P
        assert st.queries_fallback == 0
