"""The screened split-bf16 filter (kernels_gemm_bf16.h, gemm_bf16_filter_kernel<R, 0, 3, 1>): the K-loop multiplies
hi.hi alone, and a wave adds qh.vl + ql.vh only to the 32 x 32 sub-tiles whose best hi.hi score comes within the screen margin of
their queries' thresholds. Answers must be the oracle's, bit for bit those of the full three-product loop (context option
no_split_screen = 1) and of the f32 kernel (no_split_filter = 1); both the skip path and the correction must run; and the margin
must hold where hi.hi is furthest from the split score. The formula of the margin is checked on the CPU (no gpu mark)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_gpu_exact import _check_knn, _corpus, _queries, bits_equal
from test_gpu_split_filter import F32_KERNEL, SPLIT_KERNEL, _knn, _last_filter, _off_ties

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _screen_counts(vb):
    """(corrected wave tiles, corrected 32 x 32 sub-tiles) of the last call's screened launches"""
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_screen_counts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(2, np.uint32)
    _lib.check(fn(vb._h, out.ctypes.data))
    return int(out[0]), int(out[1])


def _three_ways(B, innr, ctx_option, metric, rows, qs, k, force=False):
    """screened == oracle; == the full split loop and == the f32 kernel, indices and scores bit for bit; the split filter serves"""
    data = oracle.from_rows(rows)
    if force:
        ctx_option("split_min_q", 1)
    vb = _check_knn(B, innr, metric, rows, data, qs, k, innr.KNN_MFMA)  # (a new batch: the default dispatch screens its first call)
    assert _last_filter(vb) == SPLIT_KERNEL
    assert _screen_counts(vb)[0] > 0  # the screened form ran, and corrected something
    ctx_option("no_split_screen", -1)  # always screen: these small corpora correct most wave tiles, later calls would not
    i1, s1 = _knn(B, innr, metric, vb, qs, k)
    assert _last_filter(vb) == SPLIT_KERNEL and _screen_counts(vb)[0] > 0
    ctx_option("no_split_screen", 1)
    i2, s2 = _knn(B, innr, metric, vb, qs, k)
    assert _last_filter(vb) == SPLIT_KERNEL
    assert _screen_counts(vb) == (0, 0)  # the full loop corrects nothing
    ctx_option("no_split_screen", -1)
    ctx_option("no_split_filter", 1)
    i0, s0 = _knn(B, innr, metric, vb, qs, k)
    assert _last_filter(vb) == F32_KERNEL
    ctx_option("no_split_filter", 0)
    assert np.array_equal(i1, i2) and bits_equal(s1, s2)
    assert np.array_equal(i1, i0) and bits_equal(s1, s0)
    return vb


# ------------------------------------------------------------------------------- same answers
@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("k", [1, 10, 100, 240])  # lists of 32 / 32 / 128 / 256: R = 6, 6, 12, 20 (k = 48: R = 8, below)
def test_screen_every_list_length(B, innr, ctx_option, metric, k):
    rows, _ = _corpus(20_000, 64, 3, uniform=True)
    _three_ways(B, innr, ctx_option, metric, rows, _queries(65, 64, 17, uniform=True), k)


@gpu
def test_screen_lists_of_64(B, innr, ctx_option):
    rows, _ = _corpus(20_000, 64, 3, uniform=True)
    _three_ways(B, innr, ctx_option, "dot", rows, _queries(65, 64, 17, uniform=True), 48)  # R = 8


@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("n,dim", [(3001, 1), (2049, 7), (5000, 33), (4000, 768), (3333, 1000)])
def test_screen_ragged_tiles_and_k_steps(B, innr, ctx_option, metric, n, dim):
    rows, _ = _corpus(n, dim, 5, uniform=True)
    _three_ways(B, innr, ctx_option, metric, rows, _queries(33, dim, 23, uniform=True), 10, force=True)


@gpu
@pytest.mark.parametrize("nq", [65, 512, 513, 1024])
def test_screen_query_tiles_and_padding(B, innr, ctx_option, nq):
    rows, _ = _corpus(30_000, 96, 7, uniform=True)
    qs = _queries(nq, 96, 29, uniform=True)
    for metric in ("dot", "cos"):
        _three_ways(B, innr, ctx_option, metric, rows, qs, 10)


# ------------------------------------------------------------------------------- both paths run
@gpu
@pytest.mark.parametrize("seeded", [True, False])
def test_screen_skips_and_corrects(B, innr, ctx_option, seeded):
    n, nq = 20_000, 130
    rows, data = _corpus(n, 64, 3, uniform=True)
    qs = _queries(nq, 64, 17, uniform=True)
    if seeded:
        ctx_option("gemm_seed_n", 256)  # 20 000 >= 32 x 256: the bounds start at the prefix's k-th best
    else:
        ctx_option("gemm_no_seed", 1)
    vb = _check_knn(B, innr, "dot", rows, data, qs, 10, innr.KNN_MFMA)
    assert _last_filter(vb) == SPLIT_KERNEL
    tiles, subs = _screen_counts(vb)
    ntiles = ((n + 255) // 256 * 256) // 128  # corpus tiles of the batch's padded row count (the padding rows score 0)
    real = ntiles * ((nq + 63) // 64)    # wave tiles that hold a real query
    every = ntiles * 8                   # ... and those of padding queries only (one 512-query tile): closed, never corrected
    # (at this size a slice is one tile and the best 32 of 20 000 are 1.6e-3 of all pairs: nearly every 1024-pair sub-tile of a
    #  real query can reach its bound, so the waves that are skipped here are the padding ones; the next test skips real ones)
    assert 0 < tiles <= real < every, (tiles, real)
    assert tiles <= subs <= 8 * tiles
    if not seeded:
        # without seeds a tile that starts before any bound is published has none: its wave tiles with a real query are corrected
        # whole -- at least those of the first block to run
        assert subs >= 8 * ((nq + 63) // 64)


@gpu
def test_screen_skips_tiles_of_real_queries(B, innr, ctx_option):
    # rows past the first 2048 scaled by 0.05: their scores (< 0.5) stay far below the seeded bounds (the 10th best of a full-scale
    # 256-row prefix, ~4.6) less the margin (~0.2), so only the 16 full-scale tiles can be corrected
    n, nq = 20_000, 130
    rows, _ = _corpus(n, 64, 3, uniform=True)
    rows[2048:] *= np.float32(0.05)
    data = oracle.from_rows(rows)
    ctx_option("gemm_seed_n", 256)
    vb = _check_knn(B, innr, "dot", rows, data, _queries(nq, 64, 17, uniform=True), 10, innr.KNN_MFMA)
    assert _last_filter(vb) == SPLIT_KERNEL
    tiles, _ = _screen_counts(vb)
    assert 0 < tiles <= (2048 // 128) * ((nq + 63) // 64)
    # ... a tenth of the wave tiles: the batch goes on screening
    _knn(B, innr, "dot", vb, _queries(nq, 64, 17, uniform=True), 10)
    assert _screen_counts(vb)[0] > 0


@gpu
def test_batch_that_corrects_most_tiles_takes_the_full_loop_next(B, innr, ctx_option):
    # 20 000 uniform rows: nearly every wave tile of a real query is corrected (above), far beyond the share at which the full loop
    # is faster (kScreenMaxShare, api.hip). The batch remembers: its next calls run the full loop -- same record, same answers
    rows, data = _corpus(20_000, 64, 3, uniform=True)
    qs = _queries(130, 64, 17, uniform=True)
    vb = _check_knn(B, innr, "dot", rows, data, qs, 10, innr.KNN_MFMA)
    assert _last_filter(vb) == SPLIT_KERNEL and _screen_counts(vb)[0] > 0
    i1, s1 = _knn(B, innr, "dot", vb, qs, 10)
    for _ in range(3):
        i2, s2 = _knn(B, innr, "dot", vb, qs, 10)
        assert _last_filter(vb) == SPLIT_KERNEL and _screen_counts(vb) == (0, 0)
        assert np.array_equal(i1, i2) and bits_equal(s1, s2)
    ctx_option("no_split_screen", -1)
    i3, s3 = _knn(B, innr, "dot", vb, qs, 10)
    assert _screen_counts(vb)[0] > 0 and np.array_equal(i1, i3) and bits_equal(s1, s3)


# ------------------------------------------------------------------------------- near ties
@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_screen_lcg_near_ties(B, innr, ctx_option, metric):
    rows, _ = _corpus(20_000, 128, 0)
    qs = _queries(300, 128)
    vb = _three_ways(B, innr, ctx_option, metric, rows, qs, 10)
    st = innr.KnnStats()
    {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi}[metric](qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    assert st.engine == innr.KNN_MFMA and st.queries_fallback > 0 and _last_filter(vb) == SPLIT_KERNEL


@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_screen_repeated_rows(B, innr, ctx_option, metric):
    base, _ = _corpus(1500, 96, 5, uniform=True)
    rows = np.repeat(base, 40, axis=0)
    rows[::7] *= np.float32(1.0 + 2.0 ** -20)
    qs = _queries(300, 96, 9, uniform=True)
    vb = _three_ways(B, innr, ctx_option, metric, rows, qs, 10)
    st = innr.KnnStats()
    {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi}[metric](qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    assert st.engine == innr.KNN_MFMA and st.queries_fallback > 0 and _last_filter(vb) == SPLIT_KERNEL


# ------------------------------------------------------------------------------- soundness of the margin
def _coherent_limbs(seed, n, nq, dim):
    """Rows and queries whose lo limbs sit at (just under) half a last place of their hi limbs, with the sign of the hi limb, and
    one sign per dimension for every row and query: every qh_d vl_d and ql_d vh_d is positive, so the dropped products add up
    coherently -- hi.hi is as far below the split score as the margin allows for. Then copies of query 0's best row, scaled by
    1 - j 2^-10: many candidates within the margin of the cut."""
    rng = np.random.default_rng(seed)

    def shape(x):
        h = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)           # the bf16 value below |x|
        half = (np.abs(h).view(np.uint32) & np.uint32(0x7F800000)).view(np.float32) * np.float32(2.0 ** -8)
        return (np.abs(h) + half * np.float32(1 - 2.0 ** -10)).astype(np.float32)  # rounds DOWN to h: lo = +half (1 - 2^-10)

    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    rows = shape(_off_ties(rng, (n, dim))) * sign
    qs = shape(_off_ties(rng, (nq, dim))) * sign
    best = rows[np.argmax(rows.astype(np.float64) @ qs[0].astype(np.float64))]
    block = np.stack([best * np.float32(1.0 - j * 2.0 ** -10) for j in range(1, 65)]).astype(np.float32)
    return np.concatenate([rows, block]).astype(np.float32), qs.astype(np.float32)


@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_screen_margin_with_coherent_lo_limbs(B, innr, ctx_option, metric):
    # (mutation check, DESIGN.md 4.4e: this case passes on variant libraries with the margin set to 0 or halved; the late-candidate
    #  case below is the one that tells them apart)
    rows, qs = _coherent_limbs(21, 4000, 70, 200)
    vb = _three_ways(B, innr, ctx_option, metric, rows, qs, 10)
    tiles, _ = _screen_counts(vb)  # (the last call was the f32 kernel's: its entry cleared the counts)
    assert tiles == 0
    _knn(B, innr, metric, vb, qs, 10)
    assert _screen_counts(vb)[0] > 0


# ------------------------------------------------------------------------------- the formula, on the CPU
def _rne_bf16(x):
    """round-to-nearest-even f32 -> bf16 on the bit patterns (finite inputs), returned as f32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _limbs(x):
    h = _rne_bf16(x)
    return h, _rne_bf16((x - h).astype(np.float32))  # x - h is exact in f32


def _host_margin_scale(dim):
    """api.hip split_screen_scale, before |q| max|v|: 1.05 (2^-7 1.004 + (6D + 8) u 1.04)"""
    return 1.05 * (2.0 ** -7 * 1.004 + (6 * dim + 8) * 2.0 ** -24 * 1.04)


def _cross_ratio(rows, qs):
    """max over all pairs of |qh.vl + ql.vh| / (|q| max|v|), in float64 on the emulated limbs; the host's margin covers every pair"""
    vh, vl = _limbs(rows)
    qh, ql = _limbs(qs)
    cross = qh.astype(np.float64) @ vl.astype(np.float64).T + ql.astype(np.float64) @ vh.astype(np.float64).T
    qn = np.sqrt((qs.astype(np.float64) ** 2).sum(1))[:, None]
    vmax = np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    assert np.all(_host_margin_scale(rows.shape[1]) * qn * vmax >= np.abs(cross))
    return (np.abs(cross) / (qn * vmax)).max()


def _uniform(dim):
    rng = np.random.default_rng(dim)
    return rng.uniform(-1, 1, size=(3000, dim)).astype(np.float32), rng.uniform(-1, 1, size=(70, dim)).astype(np.float32)


@pytest.mark.parametrize("dim", [7, 64, 768])
def test_cross_term_bound_uniform(dim):
    # both the bound the margin is built on (2^-7 1.004: bf16 keeps 8 significant bits) and the tighter 2^-8 1.004 hold here
    assert _cross_ratio(*_uniform(dim)) <= 2.0 ** -8 * 1.004


def test_cross_term_bound_coherent_lo_limbs():
    worst = _cross_ratio(*_coherent_limbs(21, 4000, 70, 200))
    assert worst <= 2.0 ** -7 * 1.004
    assert worst > 0.5 * 2.0 ** -7  # the data does what it is for: the dropped products use more than half of the bound


def test_half_the_margin_is_not_a_bound():
    """Why the margin's first term is 2^-7 1.004 and not 2^-8 1.004, the value first proposed from |x - rne_bf16(x)| <= 2^-9 |x|: bf16
    keeps 8 significant bits, so the rounding error reaches 2^-8 |x| just above a power of two, and no statement about the code can
    make |qh.vl + ql.vh| <= 2^-8 1.004 |q| max|v| true. On the coherent data (mantissas uniform in [1, 2)) the products reach
    1.0695 x 2^-8, 0.35 % of the 70 x 4064 pairs above 1.004 x 2^-8; with mantissas in [1, 1.0625) (the late candidate's data) they
    reach 1.79 x 2^-8, more than a margin built on 2^-8 would cover. _cross_ratio checks the host's margin against every pair."""
    assert _cross_ratio(*_coherent_limbs(21, 4000, 70, 200)) > 2.0 ** -8 * 1.004
    rows, qs, _ = _late_candidate()
    worst = _cross_ratio(rows, qs)
    assert 0.5 * _host_margin_scale(200) < worst <= 2.0 ** -7 * 1.004


# ------------------------------------------------------------------------------- a candidate only the margin keeps
def _late_candidate(seed=33, n=9000, nq=70, dim=200, at=5000):
    """One row L whose hi.hi score stays below the SEEDED threshold of every query while its split score clears query 0's: all
    values have mantissas just above a power of two (lo limb = almost half a last place = almost 2^-8 |x|) and one sign per
    dimension, so hi.hi is ~1.8 2^-8 below the score for every pair. Rows 0..9 -- inside the 256-row prefix that seeds the
    thresholds -- are L (1 - j 2^-14), j = 11..20: every query's seeded bound is within 0.12 % of its score for L, from below. L
    itself sits at row `at`, and the other 127 rows of its tile are scaled by 2^-6, so nothing else flags its sub-tiles. Rows
    1000 + 256 i are L (1 - j 2^-14), j = 1..10: found whatever the margin (plain f32 values, hi.hi is nearly their whole score),
    they fill the top 10 well above the seeded bound, so that the proof closes with or without L -- a filter that drops L
    returns a wrong answer instead of sending the query to the exact engine."""
    rng = np.random.default_rng(seed)

    def make(k):
        x = (np.exp2(rng.integers(-1, 1, size=(k, dim))) * (1 + rng.random((k, dim)) / 16)).astype(np.float32)
        h = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        half = (h.view(np.uint32) & np.uint32(0x7F800000)).view(np.float32) * np.float32(2.0 ** -8)
        return (h + half * np.float32(1 - 2.0 ** -10)).astype(np.float32)

    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0).astype(np.float32)
    rows, qs = make(n) * sign, make(nq) * sign
    best = int(np.argmax(rows.astype(np.float64) @ qs[0].astype(np.float64)))
    L = rows[best].copy()
    rows[best] = rows[at]
    t0 = at // 128 * 128
    rows[t0:t0 + 128] *= np.float32(2.0 ** -6)
    rows[at] = L
    for j in range(1, 11):
        rows[j - 1] = (L * np.float32(1.0 - (10 + j) * 2.0 ** -14)).astype(np.float32)
        rows[1000 + 256 * (j - 1)] = (L * np.float32(1.0 - j * 2.0 ** -14)).astype(np.float32)
    return rows, qs, at


def _late_candidate_figures():
    """for query 0, in units of |q| max|v|: (seeded bound - hi.hi score of L, split score of L - seeded bound)"""
    rows, qs, at = _late_candidate()
    q = qs[0].astype(np.float64)
    vh, vl = _limbs(rows[at])
    qh, ql = _limbs(qs[0])
    hh = float(qh.astype(np.float64) @ vh.astype(np.float64))
    split = hh + float(qh.astype(np.float64) @ vl.astype(np.float64) + ql.astype(np.float64) @ vh.astype(np.float64))
    unit = np.sqrt((q ** 2).sum()) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    tenth = np.sort(rows[:256].astype(np.float64) @ q)[-10]
    E = 1.05 * (3.1 * 2.0 ** -16 + (6 * 200 + 8) * 2.0 ** -24 * 1.04) * unit  # split_filter_scale
    return (tenth - E - hh) / unit, (split - tenth) / unit


def test_late_candidate_needs_more_than_half_the_margin():
    # the data has the power it is built for: the seeded bound lies above L's hi.hi score by more than HALF the host's margin (so a
    # halved or zero margin rejects L unseen), by less than the margin, and below L's split score
    gap, above = _late_candidate_figures()
    assert 0.5 * _host_margin_scale(200) < gap < _host_margin_scale(200) / 1.0002 and above > 0


@gpu
def test_screen_keeps_a_candidate_only_the_margin_covers(B, innr, ctx_option):
    # (mutation check, DESIGN.md 4.4e: on variant libraries with the margin set to 0 or halved the filter drops L, the proofs fail
    #  and the exact engine redoes 70 / 69 of the 70 queries -- the answers stay right, queries_fallback is what shows it)
    rows, qs, at = _late_candidate()
    ctx_option("gemm_seed_n", 256)  # 9000 >= 32 x 256: bounds seeded from the first 256 rows
    vb = _three_ways(B, innr, ctx_option, "dot", rows, qs, 10)
    st = innr.KnnStats()
    idx, _ = B.batch_knn_dot_multi(qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    assert at in [int(i) for i in idx[0]]
    assert _last_filter(vb) == SPLIT_KERNEL and st.queries_fallback == 0  # the filter itself kept L: nothing was redone
