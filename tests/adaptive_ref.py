"""NumPy statement of batch_knn_adaptive (src/batch.rs:441-564) as the phases the device runs -- no tests here.

The reference is one sequential loop over (dimension, vector); its only coupling between vectors is the guard `alive_count > k`.
This mirror restates it as: warm-up distances, the k-th order statistic, a flag-and-cut in index order, then per segment of
dimensions with a constant threshold "accumulate, find each vector's death dimension, apply the deaths in (dimension, index) order
until k are left". tests/test_adaptive_abi.py checks it against the oracle bit for bit; the GPU tests use its third return value,
the alive count after the warm-up prune, for stats.candidates_kept."""
from __future__ import annotations

import numpy as np

import order_ref as R


def _kth(dist: np.ndarray, k: int) -> np.float32:
    """the value at rank k-1 under f32::total_cmp"""
    b = R.bits(dist)
    i = np.argsort(R.total_key(b), kind="stable")[k - 1]
    return R.f32(b[i:i + 1])[0]


def adaptive_ref(q, data, k: int, warmup_dims: int):
    """data: dimension-major (D, N) float32. Returns (indices uint64 [k'], scores float32 [k'], alive after the warm-up prune)."""
    data = np.ascontiguousarray(data, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1)
    D, N = data.shape
    assert q.size == D and warmup_dims > 0
    if N == 0 or k == 0:
        return np.empty(0, np.uint64), np.empty(0, np.float32), 0
    k = min(k, N)
    if D == 0:
        return np.arange(k, dtype=np.uint64), np.zeros(k, np.float32), N
    W = min(warmup_dims, D)
    scale = np.float32(D) / np.float32(W)
    with np.errstate(all="ignore"):
        dist = np.zeros(N, np.float32)
        for d in range(W):
            diff = q[d] - data[d]
            dist = dist + diff * diff
        thr = _kth(dist, k) * scale
        flagged = np.flatnonzero(dist * scale > thr * np.float32(1.5))
        alive = np.ones(N, bool)
        alive[flagged[:min(flagged.size, N - k)]] = False
        L = np.flatnonzero(alive)
        dist = dist[L]
        after_warmup = L.size
        s0 = W
        while s0 < D:
            s1 = min((s0 + 31) // 32 * 32, D - 1)
            death = np.full(L.size, -1, np.int64)
            for d in range(s0, s1 + 1):
                diff = q[d] - data[d, L]
                dist = dist + diff * diff
                if L.size > k:
                    death[(death < 0) & (dist > thr)] = d
            if L.size > k:
                dying = np.flatnonzero(death >= 0)
                dying = dying[np.lexsort((dying, death[dying]))]  # by (death dimension, list position = index order)
                keep = np.ones(L.size, bool)
                keep[dying[:min(dying.size, L.size - k)]] = False
                L, dist = L[keep], dist[keep]
            if s1 % 32 == 0:
                thr = _kth(dist, k)
            s0 = s1 + 1
    o = R.order_of(R.bits(dist), L, True)[:k]
    return L[o].astype(np.uint64), dist[o], after_warmup
