"""The screen margin of the split-bf16 filter from the limbs' real norms (api.hip split_screen_scale / screen_margin_kernel,
kernels_gemm_bf16.h limb_maxima_kernel), emulated in numpy with the round-to-nearest-even limbs the pack kernels
write:

    m_j = 1.0002 [ 1.05 ( |qh_j| Lmax + |ql_j| Hmax + (6D + 8) u 1.04 |q_j| max|v| ) + the flush allowance ],

or the worst-case margin 1.0002 [ 1.05 (2^-7 1.004 + (6D + 8) u 1.04) |q_j| max|v| + the flush allowance ] where that is smaller.
Every pair's |qh.vl + ql.vh| must stay below it; it is never above the worst case, well below it on ordinary data and close to it
on data built to sit at half a last place. CPU only; tests/test_gpu_split_margin.py compares the device's values with these."""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_split_pairs import _seq_norms
from test_gpu_split_screen import _coherent_limbs, _host_margin_scale, _late_candidate, _limbs

U = 2.0 ** -24
NORM_EPSILON = np.float32(1e-9)  # common.h INNR_NORM_EPSILON


def operands(metric, rows, qs):
    """what the pack kernels split into limbs: the values, or (cosine) the values times their f32 inverse norms -- 0 for a row whose
    norm is not above the epsilon and for a query whose norm is below it (inv_norms_kernel, kernels_gemm.h)"""
    rows, qs = np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(qs, np.float32)
    if metric == "dot":
        return rows, qs
    vn, qn = _seq_norms(rows), _seq_norms(qs)
    with np.errstate(divide="ignore"):
        vi = np.where(vn > NORM_EPSILON, np.float32(1) / vn, np.float32(0)).astype(np.float32)
        qi = np.where(qn >= NORM_EPSILON, np.float32(1) / qn, np.float32(0)).astype(np.float32)
    return (rows * vi[:, None]).astype(np.float32), (qs * qi[:, None]).astype(np.float32)


def limb_norms(x):
    """(|xh_i|, |xl_i|) per row, float64"""
    h, l = _limbs(x)
    return np.sqrt((h.astype(np.float64) ** 2).sum(1)), np.sqrt((l.astype(np.float64) ** 2).sum(1))


def flush_allowance(dim, qn, vmax):
    """2^-126 (flush_c + flush_v |q|) with the host's f32 constants (make_screen_margin)"""
    sd = np.float32(np.sqrt(np.float32(dim)))
    flush_c = np.float32(sd * np.float32(vmax) + np.float32(6.0) * np.float32(dim))
    return 2.0 ** -126 * (np.float64(flush_c) + np.float64(sd) * qn)


def worst_case_margin(dim, qn, vmax):
    return 1.0002 * (_host_margin_scale(dim) * qn * vmax + flush_allowance(dim, qn, vmax))


def limb_margin(dim, nqh, nql, hmax, lmax, qn, vmax):
    return 1.0002 * (1.05 * (nqh * lmax + nql * hmax + (6 * dim + 8) * U * 1.04 * qn * vmax) + flush_allowance(dim, qn, vmax))


def margins(metric, rows, qs, qn=None, vmax=None, maxima=None):
    """(the margin per query, its worst-case form, its limb-norm form, (Hmax, Lmax)), float64. qn / vmax: the norms the device
    used (its f32 values), else the float64 ones; cosine: both 1. maxima: (Hmax, Lmax) to use instead of the rows' own."""
    dim = rows.shape[1]
    v, q = operands(metric, rows, qs)
    if metric == "cos":
        qn, vmax = np.ones(len(qs)), 1.0
    else:
        qn = np.sqrt((q.astype(np.float64) ** 2).sum(1)) if qn is None else np.asarray(qn, np.float64)
        vmax = float(np.sqrt((v.astype(np.float64) ** 2).sum(1)).max()) if vmax is None else float(vmax)
    nvh, nvl = limb_norms(v)
    nqh, nql = limb_norms(q)
    hmax, lmax = (float(nvh.max()), float(nvl.max())) if maxima is None else maxima
    old = worst_case_margin(dim, qn, vmax)
    new = limb_margin(dim, nqh, nql, hmax, lmax, qn, vmax)
    return np.minimum(new, old), old, new, (hmax, lmax)


def cross(metric, rows, qs):
    """|qh.vl + ql.vh| of every (query, row) pair, float64"""
    v, q = operands(metric, rows, qs)
    vh, vl = (x.astype(np.float64) for x in _limbs(v))
    qh, ql = (x.astype(np.float64) for x in _limbs(q))
    return np.abs(qh @ vl.T + ql @ vh.T)


def _uniform(dim, n=3000, nq=70):
    rng = np.random.default_rng(dim)
    return rng.uniform(-1, 1, size=(n, dim)).astype(np.float32), rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)


def _one_full_scale_row(dim=200):
    rows, qs = _uniform(dim)
    rows *= np.float32(2.0 ** -6)
    rows[1234] *= np.float32(2.0 ** 6)
    return rows, qs


def _with_zeros(dim=64):
    rows, qs = _uniform(dim)
    rows[[0, 77, 2999]] = 0.0
    qs[3] = 0.0
    return rows, qs


def _late():
    rows, qs, _ = _late_candidate()
    return rows, qs


DATA = {
    "uniform7": lambda: _uniform(7), "uniform64": lambda: _uniform(64), "uniform768": lambda: _uniform(768),
    "coherent": lambda: _coherent_limbs(21, 4000, 70, 200), "late": _late, "one_full_scale_row": _one_full_scale_row,
    "zeros": _with_zeros,
}


@pytest.mark.parametrize("metric", ["dot", "cos"])  # cos: the normalised form, limbs of v / |v| and q / |q|
@pytest.mark.parametrize("name", sorted(DATA))
def test_margin_covers_every_pair_and_never_exceeds_the_worst_case(name, metric):
    rows, qs = DATA[name]()
    m, old, new, _ = margins(metric, rows, qs)
    c = cross(metric, rows, qs)
    print(f"{name} {metric}: new / old = {np.nanmax(new / np.maximum(old, 1e-300)):.3f}, max |cross| / new = {(c / np.maximum(new, 1e-300)[:, None]).max():.3f}")
    assert np.all(np.isfinite(m)) and np.all(m >= 0)
    assert np.all(c <= new[:, None])  # the limb-norm form is a bound by itself ...
    assert np.all(c <= m[:, None])    # ... and so is the smaller of the two
    assert np.all(m <= old)


def test_zero_query_and_zero_rows():
    rows, qs = _with_zeros()
    for metric in ("dot", "cos"):
        m, old, new, _ = margins(metric, rows, qs)
        c = cross(metric, rows, qs)
        assert np.all(c[3] == 0) and np.all(c[:, [0, 77, 2999]] == 0)
        assert 0 < m[3] < 1e-30 if metric == "dot" else 0 < m[3] < m[0]  # (cosine keeps the accumulation term: |q^| counts as 1)


def test_margin_is_less_than_half_the_worst_case_on_uniform_768():
    m, old, _, _ = margins("dot", *_uniform(768))
    assert np.all(m < 0.5 * old)


def test_margin_stays_above_nine_tenths_of_the_worst_case_on_the_late_candidate():
    m, old, _, _ = margins("dot", *_late())
    assert np.all(m > 0.9 * old)


def test_one_full_scale_row_sets_the_maxima():
    rows, qs = _one_full_scale_row()
    nvh, nvl = limb_norms(rows)
    assert int(np.argmax(nvh)) == 1234 and int(np.argmax(nvl)) == 1234
    assert np.sort(nvl)[-2] < 2.0 ** -5 * nvl.max()
