"""GPU tests of the proofs of the int8 filter of an f32 corpus (INNR_KNN_MFMA_I8, api.hip knn_f32_i8) and of the bf16 filter
(INNR_KNN_MFMA_BF16) on coherently rounded corpora (coherent_ref.py): every dimension of the k true rows rounds towards a LOWER
approximate score, every dimension of the decoys towards a higher one, and the decoys' exact scores sit just below the true
rows'. Approximately every decoy beats every true row by almost twice the leading term of the filter's bound E_j; a filter keeps
the true rows only because of E_j, wherever it subtracts it: the running k-rule margin, the seeded thresholds, the proof of the
re-score, the completion pass's fixed thresholds x_k - E_j. A bound that is short -- by ~15 % (int8), or by one forgotten operand
(bf16) -- loses them and reports a wrong answer as proven (test_coherent_rounding_ref.py checks that the data has this power).
The bar is the suite's: scores bit-identical to the oracle's, index lists identical, for every query of the batch.

Placements (coherent_ref.py): crowded -- 600 decoys, more than any list holds: the first pass cannot contain the true rows, the
proof has to fail and the completion pass (or, with no_completion, the f32 engine) has to collect them; sparse -- 2k decoys inside
the first 1024 rows, the true rows in the last tile: no list fills, only the k-rule margin (and, with no_k_rule, the proof) stands
between a short bound and a false proof; seeded -- gemm_seed_n = 1024, all decoys inside the seeding prefix, the true rows behind
it: the seed is the prefix's k-th exact score less E_j.

Sparse and seeded calls also assert queries_fallback == 0. There a list of 128 holds every band row and the filler rows score far
below all of them, so the proof compares x_k - E_j (x_k: the k-th exact score, a true row's) with a threshold that is at most the
k-th best approximate score (a decoy's, its exact score below x_k) less 2 E_j, or the seed (a decoy's exact score less E_j): it
holds whenever E_j covers the decoy's own rounding error -- for every bound that is one. An unproven query there means that E_j is
smaller than an error the filter really made: with the bf16 bound halved every such query is unproven (and redone exactly, which
the index lists alone would not show)."""
from __future__ import annotations

import functools

import pytest

pytestmark = pytest.mark.gpu

import oracle
import coherent_ref as R
from test_gpu_exact import B, innr, same_knn  # noqa: F401  (fixtures)
from test_gpu_kernel_variants import logged  # the context's launch record: which kernel instantiation served a call

ORACLE_KNN = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}


@functools.lru_cache(maxsize=None)
def _oracle(args):
    """the oracle's answers, once per corpus, shared by the cases that run it"""
    case = R.make(*args)
    data = oracle.from_rows(case.rows)
    out = [ORACLE_KNN[case.metric](q, data, case.k) for q in case.qs]
    for oi, _ in out:
        assert sorted(int(i) for i in oi) == case.true_idx.tolist()  # (the CPU test's first condition)
    return out


_VB: dict = {}


def _batch(B, args):
    if args not in _VB:
        _VB.clear()  # one resident corpus at a time
        _VB[args] = B.VerticalBatch.from_rows(R.make(*args).rows)
    return _VB[args]


def _run(B, innr, args, engine=None, expect_engine=None):
    """one call on the corpus `args` (coherent_ref.make), every query compared with the oracle exactly; (stats, launches)"""
    case = R.make(*args)
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi, "l2": B.batch_knn_multi}[case.metric]
    if engine is None:
        engine = innr.KNN_MFMA_I8 if case.engine == "i8" else innr.KNN_MFMA_BF16
    vb = _batch(B, args)
    st = innr.KnnStats()
    (idx, sc), log = logged(lambda: fn(case.qs, vb, case.k, engine=engine, stats=st))
    assert st.engine == (engine if expect_engine is None else expect_engine)
    for j, (oi, os_) in enumerate(_oracle(args)):
        assert same_knn(case.metric, idx[j], sc[j], oi, os_), (R.case_id(args), j, idx[j], oi, sc[j], os_)
    print(f"{R.case_id(args)}: {st.queries_fallback} of {len(case.qs)} queries unproven after the first pass; launches "
          f"{sorted({e.inst for e in log})}")
    return st, log


def _first_pass(log, families=("i8_small", "i8_one", "i8_two")):
    """the MODE 0 launches of the int8 kernels"""
    return [e for e in log if e.family in families and e.args[-1] == 0]


def _collected(log):
    """a collect-mode (MODE 2) launch of the int8 filter ran: the completion pass"""
    return any(e.family in ("i8_small", "i8_one") and e.args[-1] == 2 for e in log)


def _i8(metric, dim, placement, nq=40, k=10, n=R.N_ROWS):
    args = ("i8", metric, dim, placement, nq, k, n)
    assert args in R.CORPORA  # the CPU test has checked the conditions on this corpus
    return args


def _bf16(metric, dim, placement):
    args = ("bf16", metric, dim, placement, 40, 10, R.N_ROWS)
    assert args in R.CORPORA
    return args


I8_SHAPES = [("dot", 64), ("dot", 100), ("dot", 768), ("cos", 64), ("l2", 64)]  # (100: an odd K-step tail)


# ------------------------------------------------------------------------------- int8, crowded
@pytest.mark.parametrize("metric,dim", I8_SHAPES)
def test_i8_crowded_completion_pass_collects_the_true_rows(B, innr, ctx_option, metric, dim):
    """32768 rows are fewer than 32 default prefixes: unseeded, the 512-query tile. No list of 128 can hold the true rows behind
    600 decoys: every proof fails, the collect pass (thresholds x_k - E_j) finds them. Then with no_completion: the f32 engine."""
    args = _i8(metric, dim, "crowded")
    st, log = _run(B, innr, args)
    assert st.queries_fallback > 0 and _collected(log), log
    assert [e.inst for e in _first_pass(log)] == [("i8_one", 12, 0)], log
    ctx_option("no_completion", 1)
    st, log = _run(B, innr, args)
    assert st.queries_fallback > 0 and not _collected(log), log
    assert any(e.family == "gemm_f32" for e in log), log


@pytest.mark.parametrize("nq", [1, 40])
def test_i8_crowded_small_batch_kernel(B, innr, ctx_option, nq):
    """seeded from the first 1024 rows (a share of the decoys among them): the small-batch kernel and its collect twin"""
    ctx_option("gemm_seed_n", R.PREFIX)
    st, log = _run(B, innr, _i8("dot", 64, "crowded", nq))
    assert st.queries_fallback > 0, log
    assert [e.inst for e in _first_pass(log)] == [("i8_small", 2, 2, 0)], log
    assert any(e.inst == ("i8_small", 2, 2, 2) for e in log), log


@pytest.mark.parametrize("option,inst", [("i8_no_small", ("i8_one", 12, 0)), ("i8_two_limb", ("i8_two", 12, 0))])
def test_i8_crowded_tile_kernels(B, innr, ctx_option, option, inst):
    ctx_option("gemm_seed_n", R.PREFIX)
    ctx_option(option, 1)
    st, log = _run(B, innr, _i8("dot", 64, "crowded"))
    assert st.queries_fallback > 0 and _collected(log), log
    assert [e.inst for e in _first_pass(log)] == [inst], log
    if option == "i8_no_small":
        assert not any(e.family == "i8_small" for e in log), log


def test_i8_crowded_512_query_tile(B, innr):
    st, log = _run(B, innr, _i8("dot", 64, "crowded", nq=300))
    assert st.queries_fallback > 0 and _collected(log), log
    assert [e.inst for e in _first_pass(log)] == [("i8_one", 12, 0)], log


def test_i8_crowded_k_100(B, innr):
    """lists of k + 16 rounded to 128: the collect pass settles nearly everything by design -- here behind 600 decoys"""
    st, log = _run(B, innr, _i8("dot", 64, "crowded", k=100))
    assert st.queries_fallback > 0 and _collected(log), log
    assert [e.inst for e in _first_pass(log)] == [("i8_one", 12, 0)], log


def test_i8_crowded_auto(B, innr):
    """INNR_KNN_AUTO takes the int8 filter for dot (65536 rows: the size from which it takes a filter at all)"""
    st, log = _run(B, innr, _i8("dot", 64, "crowded", n=2 * R.N_ROWS), engine=innr.KNN_AUTO, expect_engine=innr.KNN_MFMA_I8)
    assert st.queries_fallback > 0 and _collected(log), log


# ------------------------------------------------------------------------------- int8, sparse
@pytest.mark.parametrize("option", [None, "gemm_no_seed", "no_k_rule", "i8_two_limb"])
@pytest.mark.parametrize("metric,dim", I8_SHAPES)
def test_i8_sparse_k_rule_margin(B, innr, ctx_option, metric, dim, option):
    """2k decoys in the first tiles, the true rows in the last: the list never fills, the running bound is the k-th best
    approximate score seen (a decoy's) less the margin 2 E_j -- short, and the last tile's rows are rejected unseen"""
    if option:
        ctx_option(option, 1)
    st, log = _run(B, innr, _i8(metric, dim, "sparse"))
    assert st.queries_fallback == 0, st.queries_fallback
    assert [e.family for e in _first_pass(log)] == ["i8_two" if option == "i8_two_limb" else "i8_one"], log


# ------------------------------------------------------------------------------- int8, seeded
@pytest.mark.parametrize("metric,dim", I8_SHAPES)
def test_i8_seeded_thresholds(B, innr, ctx_option, metric, dim):
    """the bounds start at the prefix's k-th best EXACT score (a decoy's) less E_j; the small-batch kernel serves (the squared-L2
    copy has D + R + 1 dimensions: its own K-step count)"""
    ctx_option("gemm_seed_n", R.PREFIX)
    st, log = _run(B, innr, _i8(metric, dim, "seeded"))
    assert st.queries_fallback == 0, st.queries_fallback
    first = _first_pass(log)
    assert len(first) == 1 and first[0].family == "i8_small" and first[0].args[1:] == (2, 0), log
    if metric != "l2":
        assert first[0].args[0] == -(-dim // 128) * 2, log


def test_i8_seeded_one_query(B, innr, ctx_option):
    ctx_option("gemm_seed_n", R.PREFIX)
    st, log = _run(B, innr, _i8("dot", 64, "seeded", nq=1))
    assert st.queries_fallback == 0, st.queries_fallback
    assert [e.inst for e in _first_pass(log)] == [("i8_small", 2, 2, 0)], log


@pytest.mark.parametrize("option,inst", [("i8_no_small", ("i8_one", 12, 0)), ("i8_two_limb", ("i8_two", 12, 0))])
def test_i8_seeded_tile_kernels(B, innr, ctx_option, option, inst):
    ctx_option("gemm_seed_n", R.PREFIX)
    ctx_option(option, 1)
    st, log = _run(B, innr, _i8("dot", 64, "seeded"))
    assert st.queries_fallback == 0, st.queries_fallback
    assert [e.inst for e in _first_pass(log)] == [inst], log
    assert not any(e.family == "i8_small" and e.args[-1] == 0 for e in log), log


# ------------------------------------------------------------------------------- bf16
BF16_SHAPES = [("dot", 768), ("dot", 128), ("cos", 128)]


def _bf16_served(log):
    assert any(e.inst == ("gemm_bf16", 12, 0, 1) for e in log), log  # k = 10: lists of 4k + 64 -> 128
    assert not any(e.family == "gemm_split" for e in log), log


@pytest.mark.parametrize("metric,dim", BF16_SHAPES)
def test_bf16_crowded(B, innr, metric, dim):
    """600 decoys ahead of the true rows in lists of 128: no proof may hold; the f32 engine redoes the batch"""
    st, log = _run(B, innr, _bf16(metric, dim, "crowded"))
    _bf16_served(log)
    assert st.queries_fallback > 0, log


@pytest.mark.parametrize("option", [None, "gemm_no_seed", "no_k_rule", "gemm_seed_n"])
@pytest.mark.parametrize("metric,dim", BF16_SHAPES)
def test_bf16_sparse(B, innr, ctx_option, metric, dim, option):
    """the k-rule margin 2 E_j (default, gemm_no_seed), the proof alone (no_k_rule) and the seeded thresholds (gemm_seed_n = 1024:
    the decoys are the prefix's best rows) on the bf16 kernel"""
    if option:
        ctx_option(option, R.PREFIX if option == "gemm_seed_n" else 1)
    st, log = _run(B, innr, _bf16(metric, dim, "sparse"))
    assert st.queries_fallback == 0, st.queries_fallback
    _bf16_served(log)
