"""The pair correction of the screened split-bf16 filter (kernels_gemm_bf16.h, split_pair_delta and the screen branch of
gemm_bf16_filter_kernel<R, 0, 3, 1>): a wave tile that flags at most P (row, query) pairs adds qh.vl + ql.vh to
exactly those pairs, each by the whole wave from global memory; a wave tile that flags more keeps the MFMA correction of its
flagged 32 x 32 sub-tiles. The arithmetic and the addressing are checked pair by pair against numpy (hook
innrdbg_split_pair_scores), both paths against the oracle, the full loop and the f32 kernel, and a candidate that only the
correction admits is moved through the accumulator positions. What the data is built to do is checked on the CPU (no gpu mark)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
from test_gpu_exact import _check_knn, _corpus, _queries, bits_equal
from test_gpu_split_filter import F32_KERNEL, SPLIT_KERNEL, _knn, _last_filter
from test_gpu_split_screen import _host_margin_scale, _late_candidate, _limbs, _three_ways

gpu = pytest.mark.gpu

PAIR_CAP = 16  # kernels_gemm_bf16.h kPairCap (P)


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


def _counts4(vb):
    """(wave tiles that flagged something, flagged sub-tiles, pairs corrected on the pair path, wave tiles on the MFMA fallback)"""
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_screen_counts4
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(4, np.uint32)
    _lib.check(fn(vb._h, out.ctypes.data))
    return tuple(int(x) for x in out)


def _pair_cap():
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_pair_cap
    fn.restype = C.c_int
    fn.argtypes = []
    return fn()


def _pair_scores(vb, metric, qs, pairs):
    from innr_amd import _lib
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_split_pair_scores
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    q = np.ascontiguousarray(qs, np.float32)
    p = np.ascontiguousarray(pairs, np.uint32)
    out = np.empty(p.shape[0], np.float32)
    _lib.check(fn(vb._h, q.ctypes.data, q.shape[0], metric, p.ctypes.data, p.shape[0], out.ctypes.data))
    return out


def _seq_norms(x):
    """f32 norms in the reference's order: s = fl(s + fl(x_d x_d)) over d ascending, then the square root"""
    s = np.zeros(x.shape[0], np.float32)
    for d in range(x.shape[1]):
        s = (s + x[:, d] * x[:, d]).astype(np.float32)
    return np.sqrt(s).astype(np.float32)


def _operands(metric, rows, qs):
    """what the pack kernels split into limbs: the values themselves, or (cosine) the values times their f32 inverse norms"""
    rows, qs = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(qs, np.float32)
    if metric == "dot":
        return rows, qs
    return ((rows * (np.float32(1) / _seq_norms(rows))[:, None]).astype(np.float32),
            (qs * (np.float32(1) / _seq_norms(qs))[:, None]).astype(np.float32))


# ------------------------------------------------------------------------------- arithmetic and addressing
# rows: every r % 4, both halves of a tile (bit 4 of r / 4), the last row of a tile, a second tile, the ragged third one
_ROWS = [0, 1, 2, 3, 17, 18, 62, 64, 67, 113, 127, 128, 131, 255, 256, 297, 298, 299]
# queries: ct 0 and 1 (even / odd), the first and the last wave of a 512-query tile, a second query tile (Q = 513: Qpad 1024);
# Q = 65: one query beyond the first wave, Qpad 512
_QUERIES = {65: [0, 1, 2, 31, 62, 63, 64], 513: [0, 1, 63, 64, 447, 448, 449, 510, 511, 512]}


@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
@pytest.mark.parametrize("dim", [7, 33, 520, 768, 1000, 1100])  # ragged K-steps; a second unit per lane from 520; a third trip at 1100
def test_pair_delta_against_numpy(B, innr, metric, dim):
    rows, _ = _corpus(300, dim, 11, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    for nq, qsel in _QUERIES.items():
        qs = _queries(nq, dim, 41, uniform=True)
        pairs = np.array([(r, q) for r in _ROWS for q in qsel], np.uint32)
        got = _pair_scores(vb, innr.METRIC_DOT if metric == "dot" else innr.METRIC_COSINE, qs, pairs).astype(np.float64)
        v, q = _operands(metric, rows, qs)
        vh, vl = (x.astype(np.float64) for x in _limbs(v[pairs[:, 0]]))
        qh, ql = (x.astype(np.float64) for x in _limbs(q[pairs[:, 1]]))
        want = (qh * vl + ql * vh).sum(1)
        mag = (np.abs(qh * vl) + np.abs(ql * vh)).sum(1)
        # exact products, 2D of them summed in f32 in some order: 2D u sum|products| (not tuned)
        tol = 2 * dim * 2.0 ** -24 * mag
        worst = np.max(np.abs(got - want) / np.maximum(tol, 1e-300))
        print(f"dim {dim} {metric} Q {nq}: worst |got - want| / tol = {worst:.3g}")
        assert np.all(mag > 0) and np.all(np.abs(got - want) <= tol), (dim, metric, nq, worst)


# ------------------------------------------------------------------------------- both correction paths
def _two_path_corpus():
    """20 000 x 64 uniform rows: the first 256 at full scale (the prefix that seeds the bounds), the others scaled by 0.05, one
    row in every 128 put back to full scale"""
    rows, _ = _corpus(20_000, 64, 3, uniform=True)
    full = rows.copy()
    rows[256:] *= np.float32(0.05)
    rows[256 + 77::128] = full[256 + 77::128]
    return rows, _queries(130, 64, 17, uniform=True)


def _flags_per_wave_tile(metric, rows, qs, k=10, seed_rows=256):
    """flagged pairs per (corpus tile, 64-query wave) under the SEEDED bounds: hi.hi >= (k-th best exact score of the prefix - E) - m.
    Bounds only rise during a call, so a wave tile never flags more than this."""
    dim = rows.shape[1]
    v, q = _operands(metric, rows, qs)
    v64, q64 = v.astype(np.float64), q.astype(np.float64)
    unit = np.ones(len(qs)) if metric == "cos" else np.sqrt((q64 ** 2).sum(1)) * np.sqrt((v64 ** 2).sum(1)).max()
    E = 1.05 * (3.1 * 2.0 ** -16 + (6 * dim + 8) * 2.0 ** -24 * 1.04) * unit  # split_filter_scale
    m = _host_margin_scale(dim) * 1.0002 * unit                                # split_screen_scale, screen_margin_kernel
    kth = np.sort(q64 @ v64[:seed_rows].T, axis=1)[:, -k]
    hh = _limbs(q)[0].astype(np.float64) @ _limbs(v)[0].astype(np.float64).T
    flagged = hh >= (kth - E - m)[:, None]
    nt, nw = (len(rows) + 127) // 128, (len(qs) + 63) // 64
    out = np.zeros((nt, nw), np.int64)
    for w in range(nw):
        per_row = flagged[64 * w:64 * w + 64].sum(0)
        out[:, w] = np.add.reduceat(per_row, np.arange(0, len(rows), 128))
    return out


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_two_path_corpus_flags_few_and_many(metric):
    # figures (seeded bounds), of 157 x 3 wave tiles. dot: the prefix's four wave tiles of 64 real queries flag 365 .. 387 pairs
    # each, its 2-query ones 8 and 15; 305 wave tiles flag between 1 and 16 pairs (a sprinkled row against some of 64 queries),
    # none outside the prefix more than 8. cosine does not see the scale: every 64-query wave tile flags 340 .. 416 pairs until the
    # bounds rise, the 2-query ones 7 .. 18 (125 of them at most 16). Bounds rise during the call: the real counts are lower.
    n = _flags_per_wave_tile(metric, *_two_path_corpus())
    few = int(((n >= 1) & (n <= PAIR_CAP)).sum())
    print(metric, "wave tiles with 1..P flagged pairs:", few, " with more:", int((n > PAIR_CAP).sum()), " prefix:", n[:2].tolist(),
          " most outside the prefix:", int(n[2:].max()))
    assert few >= 50                          # the pair path has work
    assert np.all(n[:2, :2] > 4 * PAIR_CAP)   # the prefix tiles of the full waves flag densely: the fallback
    if metric == "dot":
        assert n[2:].max() <= PAIR_CAP        # ... and nothing outside the prefix can take it


@gpu
@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_both_paths_give_the_reference_answers(B, innr, ctx_option, metric):
    assert _pair_cap() == PAIR_CAP
    rows, qs = _two_path_corpus()
    data = oracle.from_rows(rows)
    ctx_option("gemm_seed_n", 256)  # 20 000 >= 32 x 256: the bounds start at the prefix's k-th best
    vb = _check_knn(B, innr, metric, rows, data, qs, 10, innr.KNN_MFMA)  # == the oracle
    assert _last_filter(vb) == SPLIT_KERNEL
    tiles, subs, pairs, fallbacks = _counts4(vb)
    print(metric, "wave tiles", tiles, "sub-tiles", subs, "pairs", pairs, "fallbacks", fallbacks)
    assert pairs > 0 and fallbacks > 0
    assert fallbacks <= tiles
    assert pairs <= PAIR_CAP * (tiles - fallbacks)
    ctx_option("no_split_screen", -1)
    i1, s1 = _knn(B, innr, metric, vb, qs, 10)
    assert _last_filter(vb) == SPLIT_KERNEL and _counts4(vb)[2] > 0 and _counts4(vb)[3] > 0
    ctx_option("no_split_screen", 1)
    i2, s2 = _knn(B, innr, metric, vb, qs, 10)
    assert _last_filter(vb) == SPLIT_KERNEL and _counts4(vb) == (0, 0, 0, 0)  # the full loop
    ctx_option("no_split_screen", -1)
    ctx_option("no_split_filter", 1)
    i0, s0 = _knn(B, innr, metric, vb, qs, 10)
    assert _last_filter(vb) == F32_KERNEL
    assert np.array_equal(i1, i2) and bits_equal(s1, s2)
    assert np.array_equal(i1, i0) and bits_equal(s1, s0)


# ------------------------------------------------------------------------------- a candidate only the pair correction admits
# (row of L, index of L's query): rt = row % 4, r / 4 % 32 = (g & 3) + 4 half + 8 (g >> 2); ct = query & 1. The batch has SIX queries
# (split_min_q = 1), so a wave tile holds at most 6 x 128 pairs and L's tile -- its other 127 rows scaled by 2^-6 -- flags at most six
# (one sign per dimension: L scores high for every query). Only the prefix tile, with ten near-copies of L against six queries,
# can flag more than P: every other flagged wave tile, L's among them, must take the pair path, which the counters then show.
_LATE_DIM = 768  # two units per lane: dimensions 512 .. 767 are a third of the correction
_LATE_NQ = 6
_LATE_AT = [(5000, 0), (5017, 1), (5026, 5), (5119, 3)]  # (rt, half, g, ct) = (0, 0, 2, 0), (1, 1, 2, 1), (2, 0, 4, 1), (3, 1, 15, 1)


def _late_case(at, qpos):
    rows, qs, at = _late_candidate(nq=_LATE_NQ, dim=_LATE_DIM, at=at)
    qs = qs.copy()
    qs[[0, qpos]] = qs[[qpos, 0]]
    return rows, qs, at


@pytest.mark.parametrize("at,qpos", _LATE_AT)
def test_late_pair_needs_the_whole_correction(at, qpos):
    # figures at (5000, 0), in units of 2^-8 |q| max|v|: bound - hi.hi 1.38 (host margin 2.19), the correction 1.75, its dimensions
    # below 512 alone 1.18
    rows, qs, at = _late_case(at, qpos)
    q = qs[qpos].astype(np.float64)
    vh, vl = (x.astype(np.float64) for x in _limbs(rows[at]))
    qh, ql = (x.astype(np.float64) for x in _limbs(qs[qpos]))
    unit = np.sqrt((q ** 2).sum()) * np.sqrt((rows.astype(np.float64) ** 2).sum(1)).max()
    E = 1.05 * (3.1 * 2.0 ** -16 + (6 * _LATE_DIM + 8) * 2.0 ** -24 * 1.04) * unit
    bound = np.sort(rows[:256].astype(np.float64) @ q)[-10] - E
    hh, delta = float(qh @ vh), qh * vl + ql * vh
    hm = _host_margin_scale(_LATE_DIM)
    n = _flags_per_wave_tile("dot", rows, qs)
    print(f"bound - hh {(bound - hh) / unit * 256:.3f}, delta {delta.sum() / unit * 256:.3f}, first unit only "
          f"{delta[:512].sum() / unit * 256:.3f}, margin {hm * 256:.3f} (x 2^-8 |q| max|v|); flags: L's tile {n[at // 128, 0]}, "
          f"prefix tile {n[0, 0]}, most elsewhere {n[1:, 0].max()}")
    assert 0.5 * hm < (bound - hh) / unit < hm / 1.0002  # flagged by the margin, not by half of it
    assert hh + delta.sum() > bound                      # admitted with the whole correction ...
    assert hh + delta[:512].sum() < bound                # ... not with its first unit per lane alone, and not without it
    assert n.shape[1] == 1 and 1 <= n[at // 128, 0] <= _LATE_NQ  # L's wave tile: by pairs
    assert n[1:, 0].max() <= PAIR_CAP < n[0, 0]                  # the prefix tile alone can overflow the queue


@gpu
@pytest.mark.parametrize("at,qpos", _LATE_AT)
def test_pair_path_keeps_a_candidate_only_the_correction_admits(B, innr, ctx_option, at, qpos):
    # (mutation check, DESIGN.md 4.4e: with the pair path's delta forced to 0 the filter drops L and all four cases fail)
    assert _pair_cap() == PAIR_CAP
    rows, qs, at = _late_case(at, qpos)
    ctx_option("gemm_seed_n", 256)
    vb = _three_ways(B, innr, ctx_option, "dot", rows, qs, 10, force=True)
    st = innr.KnnStats()
    idx, _ = B.batch_knn_dot_multi(qs, vb, 10, engine=innr.KNN_MFMA, stats=st)
    assert at in [int(i) for i in idx[qpos]]
    assert _last_filter(vb) == SPLIT_KERNEL and st.queries_fallback == 0  # the filter itself kept L: nothing was redone
    tiles, subs, pairs, fallbacks = _counts4(vb)
    print("wave tiles", tiles, "sub-tiles", subs, "pairs", pairs, "fallbacks", fallbacks)
    # the prefix wave tile is the only one that can have flagged more than P pairs (the CPU test above: seeded bounds, and bounds
    # only rise): at most that one took the fallback, so L's wave tile -- flagged, or L would be missing above -- went by pairs
    assert fallbacks <= 1 and tiles - fallbacks >= 1
    assert 1 <= pairs <= PAIR_CAP * (tiles - fallbacks)
