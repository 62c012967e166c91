"""The first round of the progressive re-score (kernels_gemm.h rescore_kernel; api.hip launch_rescore): behind a tight filter --
the split filter, the f32 kernel -- and for answers up to k = 12 the wave re-scores the best 16 candidates first and stops there
when the proof closes; otherwise, and behind the bf16 filter, the first round is the best 32 as before. A test hook counts the
candidates re-scored; the answers are the oracle's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import split_seed_ref as R
from test_gpu_exact import same_knn
from test_gpu_split_filter import F32_KERNEL, SPLIT_KERNEL, _last_filter

N, DIM, NQ = 20_000, 200, 70
BF16_KERNEL = 2  # innrdbg_last_filter (api.hip LastFilter)


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _rescored(vb):
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_rescored
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(1, np.uint32)
    _lib.check(fn(vb._h, out.ctypes.data))
    return int(out[0])


@pytest.fixture(scope="module")
def separated(B):
    """uniform rows and 32 strong rows, a hundredth apart from each other and far above the rest, for every query: the best 32
    candidates of every query are the strong rows, the 10th best clears the 17th by 7 % of its score"""
    rows = oracle.generate_uniform(N, DIM, 41)
    at = [97 + 613 * i for i in range(32)]
    rows[at] = R.strong_rows(32, DIM, 43)
    return rows, oracle.from_rows(rows), R.queries(NQ, DIM, 47), B.VerticalBatch.from_rows(rows)


def _call(B, innr, vb, data, qs, k, engine, stats=None):
    idx, sc = B.batch_knn_dot_multi(qs, vb, k, engine=engine, stats=stats)
    for j, q in enumerate(qs):
        oi, os_ = oracle.batch_knn_dot(q, data, k)
        assert same_knn("dot", idx[j], sc[j], oi, os_), (j, idx[j], oi)
    return _rescored(vb)


@pytest.mark.parametrize("f32_kernel", [False, True])
def test_best_16_prove_a_short_answer(B, innr, ctx_option, separated, f32_kernel):
    rows, data, qs, vb = separated
    if f32_kernel:
        ctx_option("no_split_filter", 1)
    st = innr.KnnStats()
    assert _call(B, innr, vb, data, qs, 10, innr.KNN_MFMA, st) == 16 * NQ
    assert _last_filter(vb) == (F32_KERNEL if f32_kernel else SPLIT_KERNEL) and st.queries_fallback == 0


@pytest.mark.parametrize("k,first", [(12, 16), (13, 32)])
def test_first_round_by_answer_length(B, innr, separated, k, first):
    rows, data, qs, vb = separated
    assert _call(B, innr, vb, data, qs, k, innr.KNN_MFMA) == first * NQ  # lists of 32 either way
    assert _last_filter(vb) == SPLIT_KERNEL


def test_bf16_filter_keeps_its_first_round_of_32(B, innr, separated):
    rows, data, qs, vb = separated
    assert _call(B, innr, vb, data, qs, 10, innr.KNN_MFMA_BF16) == 32 * NQ
    assert _last_filter(vb) == BF16_KERNEL


@pytest.mark.parametrize("f32_kernel", [False, True])
def test_ties_at_the_cut_take_the_second_round(B, innr, ctx_option, separated, f32_kernel):
    """20 copies of a row that is the best of query 0 alone: its 10th best exact score equals the approximate score of its 17th
    candidate, the proof cannot close at 16 and closes at 32; the copies come out by index. Every other query stops at 16."""
    rows, data, qs, _ = separated
    rows = rows.copy()
    x = (5.0 * (qs[0] - np.float32(0.5))).astype(np.float32)
    at = [311 + 977 * i for i in range(20)]
    rows[at] = x
    s = rows.astype(np.float64) @ qs.astype(np.float64).T  # [N][Q]
    assert np.all(np.argsort(-s[:, 0], kind="stable")[:20] == np.array(at))       # query 0: the copies lead
    assert np.all(s[at[0], 1:] < 0.7 * np.sort(s[:, 1:], axis=0)[-32])             # ... and far below everybody else's best 32
    if f32_kernel:
        ctx_option("no_split_filter", 1)
    vb = B.VerticalBatch.from_rows(rows)
    st = innr.KnnStats()
    n = _call(B, innr, vb, oracle.from_rows(rows), qs, 10, innr.KNN_MFMA, st)
    assert n == 16 * (NQ - 1) + 32 and st.queries_fallback == 0
    idx, _ = B.batch_knn_dot_multi(qs[:1], vb, 10, engine=innr.KNN_EXACT)
    assert idx[0].tolist() == at[:10]
