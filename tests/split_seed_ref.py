"""numpy mirror of the split filter's seeder (kernels_gemm_bf16.h MODE 3, split_seed_kernel) and the corpora its
tests share. A group is the 32 rows 128 tile + 4 i + rt (i < 32) of one tile and row tile; group g = 4 tile + rt."""
from __future__ import annotations

import numpy as np

import oracle


def group_maxima(scores):
    """scores [Q][P] of a prefix of whole tiles (P a multiple of 128) -> [Q][P / 32], group g = 4 tile + rt"""
    q, p = scores.shape
    assert p % 128 == 0
    return scores.reshape(q, p // 128, 32, 4).max(axis=2).reshape(q, p // 32)


def kth_largest(a, k):
    """the k-th largest along the last axis"""
    return np.sort(a, axis=-1)[..., -k]


def key_to_f32(keys):
    """order keys (common.h f32_ord) -> floats"""
    o = np.asarray(keys, np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o)
    return bits.astype(np.uint32).view(np.float32)


def group_rows(tile, rt, count):
    """the first `count` rows of group (tile, rt)"""
    return [128 * tile + 4 * i + rt for i in range(count)]


def queries(nq, dim, seed):
    """uniform queries shifted to [-0.5, 1.5): every one has a clearly positive dot with the rows of strong_rows()"""
    return (oracle.generate_uniform(nq, dim, seed) + np.float32(0.5)).astype(np.float32)


def strong_rows(count, dim, seed, scale=2.0):
    """`count` distinct rows near scale * (1, ..., 1): far better than any uniform row for every query of queries(), by dot and by
    cosine, and no two of them tie"""
    rng = np.random.default_rng(seed)
    r = np.ones((count, dim), np.float32) * np.float32(scale)
    r += rng.uniform(-0.05, 0.05, size=(count, dim)).astype(np.float32)
    r *= (1.0 + 0.01 * np.arange(count, dtype=np.float32))[:, None]
    return r.astype(np.float32)


LAYOUTS = ("random", "one_group", "copies")


def corpus(layout, n, dim, seed):
    """uniform rows; one_group: the 32 best rows all in group (tile 3, rt 1) of the prefix; copies: the best row 40 times, 25
    copies spread over the first 1024 rows (several per group) and 15 behind them"""
    rows = oracle.generate_uniform(n, dim, seed)
    if layout == "one_group":
        rows[group_rows(3, 1, 32)] = strong_rows(32, dim, seed + 1)
    elif layout == "copies":
        at = [7 + 41 * i for i in range(25)] + [1024 + 1999 * i for i in range(15)]
        assert at[-1] < n
        rows[at] = strong_rows(1, dim, seed + 1)[0]
    else:
        assert layout == "random"
    return rows
