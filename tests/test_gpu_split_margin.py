"""The split-bf16 filter's screen margin from the limbs' real norms, on the device (api.hip screen_margin_kernel / ensure_limb_maxima,
kernels_gemm_bf16.h limb_maxima_kernel): the maxima and the margins match the numpy emulation of
tests/test_split_margin_bound.py; a candidate that only the margin's own terms keep is kept; a band of rows that only the
worst-case margin flags is flagged by it alone; and the answers are the oracle's with fewer corrections than the worst case
(context option split_screen_worst_case = 1). What the data is built to do is asserted on the CPU first."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from test_gpu_exact import _corpus, _queries, same_knn
from test_gpu_split_filter import SPLIT_KERNEL, _knn, _last_filter
from test_gpu_split_screen import _late_candidate, _limbs, _rne_bf16, _screen_counts
from test_split_margin_bound import U, limb_norms, margins

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _device_margins(vb, innr, metric, cap):
    """((Hmax, Lmax), max_norm, margins, query norms) of the batch's split pair and of the context's last screened call"""
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_margins
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    maxima, info = np.zeros(2, np.float32), np.zeros(1, np.float32)
    m, qn, nq = np.zeros(cap, np.float32), np.zeros(cap, np.float32), C.c_size_t(0)
    _lib.check(fn(vb._h, innr.METRIC_DOT if metric == "dot" else innr.METRIC_COSINE, maxima.ctypes.data, info.ctypes.data,
                  m.ctypes.data, qn.ctypes.data, cap, C.byref(nq)))
    assert nq.value == cap
    return maxima, float(info[0]), m, qn


def _split_E(dim, unit):
    return 1.05 * (3.1 * 2.0 ** -16 + (6 * dim + 8) * U * 1.04) * unit  # api.hip split_filter_scale


def _worst_case_f32(dim, qn, vmax, cos):
    """the worst-case margin exactly as the host and the kernel compute it, in f32 (split_screen_scale, screen_margin_kernel)"""
    f = np.float32
    scale = f(f(1.05) * f(f(f(0.0078125) * f(1.004)) + f(f(f(f(f(6.0) * f(dim)) + f(8.0)) * f(5.9604645e-08)) * f(1.04)))) * f(vmax)
    sd = f(np.sqrt(f(dim)))
    flush_c = f(f(sd * f(vmax)) + f(f(6.0) * f(dim)))
    qn = np.ones_like(qn, dtype=np.float32) if cos else qn.astype(np.float32)
    return ((scale * qn + f(1.17549435e-38) * (flush_c + sd * qn)) * f(1.0002)).astype(np.float32)


def _oracle_answers(metric, data, qs, k):
    ofn = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine}[metric]
    return [ofn(q, data, k) for q in qs]


def _assert_oracle(metric, got, want):
    idx, sc = got
    for j, (oi, os_) in enumerate(want):
        assert same_knn(metric, idx[j], sc[j], oi, os_), (metric, j, idx[j], oi)


# ------------------------------------------------------------------------------- 1. the maxima and the margins match numpy
@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("n", [1000, 4133])       # ragged last tile, padding rows up to a multiple of 256
@pytest.mark.parametrize("dim", [7, 200, 768])    # a ragged K-step, several lanes' strides in the query kernel
def test_maxima_and_margins_match_numpy(B, innr, ctx_option, metric, n, dim):
    rows, _ = _corpus(n, dim, 5, uniform=True)
    qs = _queries(33, dim, 23, uniform=True)
    rows[n // 2] = 0.0
    qs[2] = 0.0
    ctx_option("split_min_q", 1)
    ctx_option("no_split_screen", -1)
    vb = B.VerticalBatch.from_rows(rows)
    _knn(B, innr, metric, vb, qs, 10)
    assert _last_filter(vb) == SPLIT_KERNEL
    maxima, max_norm, got, qn = _device_margins(vb, innr, metric, len(qs))
    cos = metric == "cos"
    if not cos:  # the f32 norms the device took for the accumulation term are the float64 ones up to their own rounding
        assert np.allclose(qn, np.sqrt((qs.astype(np.float64) ** 2).sum(1)), rtol=1e-4, atol=0)
        assert abs(max_norm - np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()) <= 1e-4 * max_norm
    _, _, new, (hmax, lmax) = margins(metric, rows, qs, qn=qn.astype(np.float64), vmax=max_norm)
    print(f"{metric} n {n} dim {dim}: Hmax {maxima[0]:.9g} (numpy {hmax:.9g}), Lmax {maxima[1]:.9g} (numpy {lmax:.9g})")
    for dev, ref in ((float(maxima[0]), hmax), (float(maxima[1]), lmax)):
        assert ref <= dev <= ref * (1 + 1e-3)
    # the smaller of the limb-norm form (float64) and the worst case (the kernel's own f32 value)
    want = np.minimum(new, _worst_case_f32(dim, qn, 1.0 if cos else max_norm, cos).astype(np.float64))
    worst = np.max(got.astype(np.float64) / want)
    print(f"  margins / numpy: {np.min(got.astype(np.float64) / want):.9f} .. {worst:.9f}; margin / worst case {np.max(want / _worst_case_f32(dim, qn, 1.0 if cos else max_norm, cos)):.3f}")
    assert np.all(got.astype(np.float64) >= want) and np.all(got.astype(np.float64) <= want * (1 + 1e-3))
    # the tuning word gives the worst case back, bit for bit
    ctx_option("split_screen_worst_case", 1)
    _knn(B, innr, metric, vb, qs, 10)
    _, _, forced, _ = _device_margins(vb, innr, metric, len(qs))
    assert np.array_equal(forced.view(np.uint32), _worst_case_f32(dim, qn, 1.0 if cos else max_norm, cos).view(np.uint32))


# ------------------------------------------------------------------------------- 2. a candidate only the margin's own terms keep
_L_N, _L_AT, _L_DIM = 9000, 8990, 200  # L in the last tile (rows 8960 .. 8999: ragged)


@functools.lru_cache(maxsize=None)
def _late_exact_rows():
    """The late candidate of tests/test_gpu_split_screen.py with every row but L rounded to bf16 (lo limb 0): Lmax is L's own lo-limb
    norm. The ten prefix decoys (rows 0 .. 9) and the nine rows above L (1000 + 256 i) are L's hi limb with its first n values one
    bf16 place larger in magnitude (each adds about 0.004 of the margin to the score: one sign per dimension). The decoys' exact
    scores for query 0 lie between 0.60 and 0.74 of the margin above L's hi.hi score plus E, so the seeded bound is inside (1/2, 1)
    of the margin above it; the nine (n = 112, 123 .. 200) score above L's split score."""
    rows, qs, at = _late_candidate(n=_L_N, dim=_L_DIM, at=_L_AT)
    L = rows[at].copy()
    rows = _rne_bf16(rows)
    rows[at] = L
    q = qs[0].astype(np.float64)
    vh, _ = _limbs(L)

    def bumped(n):
        b = vh.copy().view(np.uint32)
        b[:n] += np.uint32(0x10000)
        return b.view(np.float32)

    for i in range(9):
        rows[1000 + 256 * i] = bumped(112 + 11 * i)
    rows[1000 + 256 * 9] = rows[1000 + 256 * 9 + 1]  # (the tenth of the original construction: an ordinary row again)
    # the margin does not depend on the decoys (their norms are below the nine's): place them by it
    for j in range(10):
        rows[j] = rows[100 + j]
    m0 = margins("dot", rows, qs)[0][0]
    qh, _ = _limbs(qs[0])
    hh = float(qh.astype(np.float64) @ vh.astype(np.float64))
    unit = np.sqrt((q ** 2).sum()) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    E = _split_E(_L_DIM, unit)
    lo, hi = hh + E + 0.60 * m0, hh + E + 0.74 * m0
    inside = [n for n in range(_L_DIM + 1) if lo < float(bumped(n).astype(np.float64) @ q) < hi]
    assert len(inside) >= 10
    for j in range(10):
        rows[j] = bumped(inside[j * (len(inside) - 1) // 9])
    return rows, qs, at


def _late_exact_figures():
    rows, qs, at = _late_exact_rows()
    q = qs[0].astype(np.float64)
    m0 = margins("dot", rows, qs)[0][0]
    others = np.delete(rows, at, axis=0)
    nvh, nvl = limb_norms(others)
    without = margins("dot", rows, qs, maxima=(float(limb_norms(rows)[0].max()), float(nvl.max())))[0][0]
    vh, vl = (x.astype(np.float64) for x in _limbs(rows[at]))
    qh, ql = (x.astype(np.float64) for x in _limbs(qs[0]))
    hh = float(qh @ vh)
    split = hh + float(qh @ vl + ql @ vh)
    unit = np.sqrt((q ** 2).sum()) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    E = _split_E(_L_DIM, unit)
    tenth = np.sort(rows[:256].astype(np.float64) @ q)[-10]
    return dict(gap=tenth - E - hh, above=split - tenth, m=m0, without=without, lmax_others=float(nvl.max()), E=E)


def test_late_candidate_needs_the_maxima():
    f = _late_exact_figures()
    print({k: float(v) for k, v in f.items()})
    assert f["lmax_others"] == 0.0                 # Lmax is attained on L alone
    assert 0.5 * f["m"] < f["gap"] < f["m"]        # the seeded bound: above L's hi.hi score by (1/2, 1) of the margin
    assert f["above"] > 2 * f["E"]                 # L's split score clears the bound, and the ten decoys below it by the proof's 2E
    assert f["without"] < f["gap"]                 # the margin from the other rows' Lmax (0) would reject L unseen
    # every query's proof closes (nothing goes to the exact engine): its 10th best lies well above what a list of 32 leaves out
    rows, qs, _ = _late_exact_rows()
    s = np.sort(qs.astype(np.float64) @ rows.astype(np.float64).T, axis=1)
    unit = np.sqrt((qs.astype(np.float64) ** 2).sum(1)) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    assert np.all(s[:, -10] - s[:, -33] > 2.5 * _split_E(_L_DIM, unit))


@gpu
def test_screen_keeps_a_candidate_only_the_limb_maxima_cover(B, innr, ctx_option):
    # (mutation checks, DESIGN.md 4.4e: on variant libraries with Lmax forced to 0, or with the maxima taken over all rows but the
    #  last tile's, the filter drops L and the exact engine redoes queries: queries_fallback is what shows it)
    rows, qs, at = _late_exact_rows()
    data = oracle.from_rows(rows)
    ctx_option("gemm_seed_n", 256)
    ctx_option("no_split_screen", -1)
    vb = B.VerticalBatch.from_rows(rows)
    st = innr.KnnStats()
    idx, sc = B.batch_knn_dot_multi(qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    _assert_oracle("dot", (idx, sc), _oracle_answers("dot", data, qs, 10))
    assert at in [int(i) for i in idx[0]]
    assert _last_filter(vb) == SPLIT_KERNEL and _screen_counts(vb)[0] > 0  # the screened kernel ran
    assert st.queries_fallback == 0                                        # ... and kept L itself: nothing was redone


# ------------------------------------------------------------------------------- 3. a band only the worst-case margin flags
_B_N, _B_DIM, _B_NQ = 9000, 64, 130
_B_AT = [300, 2999, 3000, 5555, 8990]  # tiles 2, 23 (twice), 43 and the last, ragged one: four wave tiles of query 0's wave


@functools.lru_cache(maxsize=None)
def _band_rows():
    rows, _ = _corpus(_B_N, _B_DIM, 3, uniform=True)
    qs = _queries(_B_NQ, _B_DIM, 19, uniform=True)  # (seed 17: the copies enter query 64's top 10)
    rows[256:] *= np.float32(2.0 ** -7)  # full scale only in the prefix that seeds the bounds: the seeds hold the final top 10
    q = qs[0].astype(np.float64)
    best = rows[int(np.argmax(rows[:256].astype(np.float64) @ q))].copy()
    m, old, _, _ = margins("dot", rows, qs)
    unit = np.sqrt((q ** 2).sum()) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    E = _split_E(_B_DIM, unit)
    s10 = np.sort(rows[:256].astype(np.float64) @ q)[-10]
    lo, hi = s10 + E - old[0], s10 - E - m[0]
    assert lo < hi
    qh = _limbs(qs[0])[0].astype(np.float64)
    top = float(qh @ _limbs(best)[0].astype(np.float64))
    for i, at in enumerate(_B_AT):
        target = lo + (hi - lo) * (i + 1) / (len(_B_AT) + 1)
        rows[at] = (best * np.float32(target / top)).astype(np.float32)
    return rows, qs, (lo, hi)


def _band_figures():
    rows, qs, (lo, hi) = _band_rows()
    q64, v64 = qs.astype(np.float64), rows.astype(np.float64)
    m, old, _, _ = margins("dot", rows, qs)
    unit = np.sqrt((q64 ** 2).sum(1)) * np.sqrt((v64 ** 2).sum(1)).max()
    E = _split_E(_B_DIM, unit)
    s10 = np.sort(q64 @ v64[:256].T, axis=1)[:, -10]
    hh = _limbs(qs)[0].astype(np.float64) @ _limbs(rows)[0].astype(np.float64).T
    return hh, s10, E, m, old, (lo, hi)


def test_band_lies_between_the_two_margins():
    rows, qs, _ = _band_rows()
    hh, s10, E, m, old, (lo, hi) = _band_figures()
    print(f"interval ({lo:.4f}, {hi:.4f}) of width {(hi - lo):.4f}; copies' hi.hi scores {hh[0, _B_AT]}")
    assert lo < hi
    assert np.all(hh[0, _B_AT] > lo) and np.all(hh[0, _B_AT] < hi)
    # the seeds hold the final top 10 of every query: nothing beyond the prefix comes near them
    full = np.sort(qs.astype(np.float64) @ rows.astype(np.float64).T, axis=1)[:, -10]
    assert np.array_equal(full, s10)
    # with the margin from the limbs NO pair beyond the prefix tiles reaches any query's seeded bound less the margin ...
    assert not np.any(hh[:, 256:] >= (s10 - E - m)[:, None])
    # ... and the worst case flags every copy for query 0
    assert np.all(hh[0, _B_AT] >= s10[0] + E[0] - old[0])


@gpu
def test_band_is_flagged_by_the_worst_case_margin_alone(B, innr, ctx_option):
    rows, qs, _ = _band_rows()
    want = _oracle_answers("dot", oracle.from_rows(rows), qs, 10)
    ctx_option("gemm_seed_n", 256)
    ctx_option("no_split_screen", -1)
    vb = B.VerticalBatch.from_rows(rows)
    _assert_oracle("dot", _knn(B, innr, "dot", vb, qs, 10), want)
    assert _last_filter(vb) == SPLIT_KERNEL
    new_tiles = _screen_counts(vb)[0]
    ctx_option("split_screen_worst_case", 1)
    _assert_oracle("dot", _knn(B, innr, "dot", vb, qs, 10), want)
    old_tiles = _screen_counts(vb)[0]
    prefix = 2 * ((_B_NQ + 63) // 64)  # wave tiles of the prefix's two corpus tiles that hold a real query
    copies = len({at // 128 for at in _B_AT})
    print("flagged wave tiles: margin from the limbs", new_tiles, " worst case", old_tiles)
    assert 0 < new_tiles <= prefix            # nothing beyond the prefix tiles
    assert old_tiles >= new_tiles + copies    # the bounds are the seeds from the start: the worst case flags a superset, and the copies


# ------------------------------------------------------------------------------- 4. the oracle's answers, fewer corrections
def _repeated():
    base, _ = _corpus(1500, 96, 5, uniform=True)
    rows = np.repeat(base, 40, axis=0)
    rows[::7] *= np.float32(1.0 + 2.0 ** -20)
    return rows, _queries(300, 96, 9, uniform=True)


_ORACLE_DATA = {
    "uniform": lambda: (_corpus(20_000, 64, 3, uniform=True)[0], _queries(130, 64, 17, uniform=True)),
    "lcg": lambda: (_corpus(20_000, 128, 0)[0], _queries(300, 128)),
    "repeated": _repeated,
}


@gpu
@pytest.mark.parametrize("k", [10, 100])  # lists of 32 and of 128: R = 6 (the pair path) and R = 12
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("name", sorted(_ORACLE_DATA))
def test_margin_from_the_limbs_against_the_oracle(B, innr, ctx_option, name, metric, k):
    rows, qs = _ORACLE_DATA[name]()
    want = _oracle_answers(metric, oracle.from_rows(rows), qs, k)
    ctx_option("no_split_screen", -1)
    vb = B.VerticalBatch.from_rows(rows)
    _assert_oracle(metric, _knn(B, innr, metric, vb, qs, k), want)
    assert _last_filter(vb) == SPLIT_KERNEL
    new_tiles = _screen_counts(vb)[0]
    ctx_option("split_screen_worst_case", 1)
    _assert_oracle(metric, _knn(B, innr, metric, vb, qs, k), want)
    old_tiles = _screen_counts(vb)[0]
    print(f"{name} {metric} k {k}: flagged wave tiles {new_tiles} (margin from the limbs) / {old_tiles} (worst case)")
    assert 0 < new_tiles <= old_tiles
