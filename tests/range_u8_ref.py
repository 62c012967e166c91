"""NumPy model of the int8 filter behind innr_batch_range_search_u8's collect path, for the tests of its bound:
what pack_queries_i8_kernel, the one-limb kernels and seed_thresholds_u8_kernel compute for one query, step by step in f32.

    t      = clip(rint(q / s), +-T),  s = max|q| / T,  T = (R1 << 6) + 31 with i8_limb_r1's R1     (the 14-bit query value)
    V      = sum_d (c_d - 128) t_d                                                                (exact, int64)
    approx = fma(A, V, B),  A = alpha/255 s,  B = (128 alpha/255 + offset) sum(q)
    E      = err_scale |q| + 4.8e-7 |offset sum(q)| + qc3                                         (rescore_u8_kernel's bound)
    a site is collected when approx >= thr - E (the kernel's fixed threshold: thr - 1.0001 E - 1e-30, one key lower)"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import oracle

F = np.float32
S = 6  # kI8hS: the shift of the one-limb kernels


def limb_r1(dim: int, s: int = S) -> int:
    """kernels_gemm_i8.h i8_limb_r1"""
    tmax = ((1 << 31) - 1) // (max(dim, 1) * 128)
    lo_max = (1 << (s - 1)) - 1
    if tmax < lo_max + (1 << s):
        return 0
    return min((tmax - lo_max) >> s, 127)


def limb_t(dim: int) -> int:
    return (limb_r1(dim) << S) + (1 << (S - 1)) - 1


def all_scores(codes, p, qs) -> np.ndarray:
    """scores[j][i]: the reference's score of code row i for query j (its full ranking scattered back by index)"""
    n = codes.shape[0]
    out = np.empty((len(qs), n), F)
    for j, q in enumerate(qs):
        oi, os_ = oracle.batch_knn_u8(q, codes, p, n)
        out[j, oi.astype(np.int64)] = os_
    return out


class Filtered(NamedTuple):
    approx: np.ndarray  # [N] f32: the filter's score of every code row
    E: float            # the query's whole bound (f32; inf: no collect threshold exists)
    t: np.ndarray       # [D] int64: the quantised query
    s: float            # its scale
    resid: np.ndarray   # [D] f64: q / s - t


def filter_query(q, codes, alpha: float, offset: float) -> Filtered:
    q = np.ascontiguousarray(q, F)
    dim = q.size
    T = F(limb_t(dim))
    a255 = F(alpha) / F(255.0)
    off = F(offset)
    mx = F(np.abs(q).max())
    s = F(mx / T)
    inv_s = F(1.0) / s
    t = np.clip(np.rint(q * inv_s), -T, T).astype(np.int64)
    V = (codes.astype(np.int64) - 128) @ t
    assert np.abs(V).max() < 2 ** 31
    qs = F(oracle.query_sum(q))
    qn = F(np.sqrt(np.cumsum((q * q).astype(F), dtype=F)[-1]))  # the chain of query_sums_kernel (the bound has room for its last place)
    A = F(a255 * s)
    B = F(F(F(128.0) * a255) + off) * qs
    B = F(B)
    # fma(A, (float)V, B): the product of two f32 is exact in f64; one f64 rounding of the sum before the f32 one (double rounding
    # moves a result by at most one f32 last place in 2^-29 of the cases: far inside what the bound leaves)
    approx = (np.float64(A) * V.astype(F).astype(np.float64) + np.float64(B)).astype(F)
    vmax = F(128.0) * F(dim) * T
    qc3 = F(1.02) * (abs(a255) * s * F(64.0) * F(dim) + F(2.4e-7) * (abs(A) * vmax + abs(B)) +
                     F(2.4e-7) * (abs(F(128.0) * a255 * qs) + abs(off * qs)))
    err_scale = F(1.05) * abs(a255) * (F(2.0) * F(dim) + F(12.0)) * F(5.9604645e-08) * F(255.0) * F(np.sqrt(F(dim)))
    E = F(err_scale * qn) + F(4.8e-7) * abs(F(off * qs)) + F(qc3)
    return Filtered(approx, float(F(E)), t, float(s), q.astype(np.float64) / np.float64(s) - t)


def collect_threshold(thr, E) -> np.float32:
    """seed_thresholds_u8_kernel's t (the kernel admits from one key below it on)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return F(F(F(thr) - F(F(E) * F(1.0001))) - F(1e-30))


def collected(f: Filtered, thr) -> np.ndarray:
    """the sites the collect pass takes for this threshold (all False: no finite collect threshold -- the exact scan's query)"""
    t = collect_threshold(thr, f.E)
    if not np.isfinite(t):
        return np.zeros(f.approx.shape, bool)
    return f.approx >= t
