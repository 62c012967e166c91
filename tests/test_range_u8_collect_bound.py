"""The bound behind the collect path of innr_batch_range_search_u8, checked on the CPU against the oracle with the NumPy model of
the int8 filter (tests/range_u8_ref.py): for every (query, code row) pair |approx - oracle score| <= E, and therefore no vector
that survives a threshold -- !(score < thr) on the oracle's bits -- lies outside what the collect pass takes, {approx >= thr - E}.
Thresholds sit on exact scores and one last place either side of them, where a survivor is decided by a single bit.

Inputs that push on the bound from different sides: uniform data; a corpus of constant rows (every row's error has one sign: the
quantisation errors of the query add up instead of cancelling); queries whose residuals q / s - t all share one sign (the same
from the query's side); and an off-centre range (offset >> alpha: the scores are dominated by offset * sum(q), whose rounding the
4.8e-7 term of the bound has to cover)."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from range_u8_ref import all_scores, collect_threshold, collected, filter_query, limb_t

N = 600
DIMS = (37, 500)  # two K-steps with a ragged last one; eight


def _uniform(dim):
    rows = oracle.generate_uniform(N, dim, 11)
    p = oracle.qparams_fit(rows)
    return oracle.quantize_u8(rows, p), p, oracle.generate_uniform(6, dim, 12)


def _constant_rows(dim):
    codes = np.repeat((np.arange(N) * 37 % 256).astype(np.uint8)[:, None], dim, axis=1)  # row i: the code 37 i mod 256, D times
    return codes, oracle.QParams(2.0, -1.0), oracle.generate_uniform(6, dim, 13)


def _one_sided(dim):
    """q_d = s (t_d + r): every residual is r (+0.4, -0.4, ... per query); q_0 = s T fixes the scale at s = 2^-12"""
    codes, p, _ = _uniform(dim)
    T = limb_t(dim)
    rng = np.random.default_rng(14)
    s = 2.0 ** -12
    qs = []
    for r in (0.4, -0.4, 0.45, -0.45, 0.25, -0.25):
        t = rng.integers(-T + 2, T - 1, size=dim).astype(np.float64)
        q = s * (t + r)
        q[0] = s * T
        qs.append(q)
    return codes, p, np.asarray(qs, np.float32)


def _off_centre(dim):
    rows = oracle.generate_uniform(N, dim, 15) * np.float32(0.005) + np.float32(50.0)
    p = oracle.QParams(0.01, 49.995)
    return oracle.quantize_u8(rows, p), p, oracle.generate_uniform(6, dim, 16)


CASES = {"uniform": _uniform, "constant_rows": _constant_rows, "one_sided": _one_sided, "off_centre": _off_centre}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", sorted(CASES))
def test_bound_and_survivors(kind, dim):
    codes, p, qs = CASES[kind](dim)
    scores = all_scores(codes, p, qs)
    assert np.isfinite(scores).all()
    for j, q in enumerate(qs):
        f = filter_query(q, codes, p.alpha, p.offset)
        assert np.isfinite(f.E) and f.E > 0.0
        if kind == "one_sided":
            r = f.resid[1:]
            assert (np.sign(r) == np.sign(r[0])).all() and np.abs(r).min() > 0.2, "the residuals share one sign"
        err = np.abs(f.approx.astype(np.float64) - scores[j].astype(np.float64))
        print(f"{kind} D={dim} q{j}: max |approx - score| = {err.max():.3e}, E = {f.E:.3e} ({err.max() / f.E:.3f} of it)")
        assert (err <= f.E).all(), (kind, dim, j, float(err.max()), f.E)
        # thresholds at exact scores (the best, the 10th best, the median, the worst) and one last place either side
        srt = np.sort(scores[j])
        for x in (srt[-1], srt[-10], srt[N // 2], srt[0]):
            for thr in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
                keep = np.flatnonzero(~(scores[j] < thr))
                took = collected(f, thr)
                assert np.isfinite(collect_threshold(thr, f.E))
                assert took[keep].all(), (kind, dim, j, float(thr), keep[~took[keep]][:5])


def test_no_collect_threshold():
    """a NaN or infinite threshold, and a query whose bound is not finite, have no finite collect threshold: the exact scan's"""
    codes, p, qs = _uniform(37)
    f = filter_query(qs[0], codes, p.alpha, p.offset)
    for thr in (np.nan, np.inf, -np.inf):
        assert not np.isfinite(collect_threshold(thr, f.E)) and not collected(f, thr).any()
    assert not np.isfinite(collect_threshold(0.25, np.inf))
