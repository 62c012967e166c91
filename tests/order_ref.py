"""NumPy statement of the order every kNN-shaped result of the library follows -- no tests here, the modules that need it import it.

The reference sorts (index, score) pairs with a STABLE sort on f32::total_cmp (batch.rs:757: descending for dot / cosine,
ascending for squared L2) starting from index order, so equal keys stay in index order: the result is the list sorted by
(total-order key in the metric's direction, index ascending). tests/test_order_ref.py checks these few lines against the oracle."""
from __future__ import annotations

import numpy as np

PNAN, NNAN = 0x7FC00000, 0xFFC00000          # the quiet NaNs: +NaN sorts above +inf, -NaN below -inf in total_cmp
PINF, NINF = 0x7F800000, 0xFF800000
PZERO, NZERO = 0x00000000, 0x80000000


def bits(a) -> np.ndarray:
    """float32 values as their uint32 bit patterns"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(b) -> np.ndarray:
    """uint32 bit patterns as float32 values (no conversion: NaN payloads and signs survive)"""
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def total_key(score_bits) -> np.ndarray:
    """core::f32::total_cmp's key: bits ^ (((bits as i32) >> 31) as u32 >> 1), compared as i32 (returned as int64)"""
    b = np.ascontiguousarray(score_bits, dtype=np.uint32).view(np.int32)
    flip = ((b >> 31).view(np.uint32) >> np.uint32(1)).view(np.int32)
    return (b ^ flip).astype(np.int64)


def order_of(score_bits, index, smaller_is_better: bool) -> np.ndarray:
    """positions of the pairs in result order: best key first, equal keys by ascending index"""
    key = total_key(score_bits)
    if not smaller_is_better:
        key = -key
    return np.lexsort((np.asarray(index).astype(np.uint64), key))


def topk_ref(score_bits, index, smaller_is_better: bool, k: int):
    """(indices uint64, score bits uint32) of the best min(k, len) pairs"""
    score_bits = np.ascontiguousarray(score_bits, dtype=np.uint32)
    index = np.asarray(index).astype(np.uint64)
    o = order_of(score_bits, index, smaller_is_better)[:k]
    return index[o], score_bits[o]


def merge_ref(all_idx, all_bits, valid, smaller_is_better: bool, kout: int):
    """Shard merge of one query: all_idx / all_bits / valid are [G, k] (global index, score bits, slot holds a candidate);
    the valid pairs in result order, cut to kout."""
    v = np.asarray(valid, dtype=bool).reshape(-1)
    return topk_ref(np.asarray(all_bits, np.uint32).reshape(-1)[v], np.asarray(all_idx).reshape(-1)[v], smaller_is_better, kout)
