"""CPU: the NumPy order reference of tests/order_ref.py IS the reference's order. The GPU tests of the re-rank and of the shard
merge (tests/test_gpu_order_semantics.py) compare the device with order_ref on inputs no corpus produces; here order_ref itself is
compared with the oracle's sort-based kNN on a corpus full of ties, cut into three index ranges like a sharded call."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import order_ref as R
from test_gpu_exact import same_knn

METRICS = ("dot", "cos", "l2")
KNN = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}


def _tie_corpus(metric):
    """61 x 6: every row is one of nine patterns, so nearly every score occurs in all three ranges; two patterns are zero rows
    (+0.0 / mixed-sign zeros: cosine 0.0 through the norm guard), and for dot / l2 one is an infinite and one a +NaN row."""
    pat = oracle.generate_uniform(9, 6, 31).copy()
    pat[2, :] = 0.0
    pat[5, :] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    pat[7] = -pat[1]
    if metric != "cos":  # (an infinite row's cosine is a generated NaN: pinned by test_generated_nan_sign_and_rank_are_pinned)
        pat[4, 1] = np.inf
        pat[6, 0] = np.nan
    rng = np.random.default_rng(17)
    rows = pat[rng.integers(0, 9, size=61)]
    return np.ascontiguousarray(rows, np.float32)


def test_total_key_is_the_oracles():
    specials = np.array([R.PNAN, R.NNAN, R.PINF, R.NINF, R.PZERO, R.NZERO, 0x3F800000, 0xBF800000, 0x00000001, 0x80000001,
                         0x7FFFFFFF, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    rnd = np.random.default_rng(3).integers(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32)
    # (oracle.total_key takes its argument through a C double, which quiets a signalling NaN: give it quiet ones only)
    snan = ((rnd & 0x7F800000) == 0x7F800000) & ((rnd & 0x007FFFFF) != 0) & ((rnd & 0x00400000) == 0)
    rnd[snan] |= np.uint32(0x00400000)
    for b in np.concatenate([specials, rnd]):
        assert int(R.total_key([b])[0]) == oracle.total_key(R.f32([b])[0]), hex(int(b))
    # the order itself, spelt out once: -NaN < -inf < -1 < -0.0 < +0.0 < 1 < +inf < +NaN
    line = np.array([R.NNAN, R.NINF, 0xBF800000, R.NZERO, R.PZERO, 0x3F800000, R.PINF, R.PNAN], np.uint32)
    assert np.all(np.diff(R.total_key(line)) > 0)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 8, 25, 61, 100])
def test_merge_reference_carries_the_reference_tie_rule(metric, k):
    rows = _tie_corpus(metric)
    n = len(rows)
    qs = oracle.generate_uniform(3, 6, 32).copy()
    qs[2] = rows[0]  # squared L2: exact zeros against every copy of that pattern
    l2 = metric == "l2"
    ranges = [(0, 20), (20, 7), (27, 34)]  # one range shorter than k = 8, all of them shorter than k = 61
    whole = oracle.from_rows(rows)
    ties = 0
    for q in qs:
        all_idx = np.full((3, k), np.iinfo(np.uint64).max, np.uint64)
        all_bits = np.full((3, k), R.PINF if not l2 else R.NINF, np.uint32)  # what an empty slot holds must not matter
        valid = np.zeros((3, k), bool)
        for g, (start, count) in enumerate(ranges):
            shard = oracle.from_rows(rows[start:start + count])
            # (squared L2: a shard's local list in the sort-based order as well, see below)
            li, ls = oracle.batch_knn_filtered(q, shard, k, np.ones(count, np.uint8)) if l2 else KNN[metric](q, shard, k)
            assert len(li) == min(k, count)
            all_idx[g, :len(li)] = li + np.uint64(start)
            all_bits[g, :len(li)] = R.bits(ls)
            valid[g, :len(li)] = True
        gi, gb = R.merge_ref(all_idx, all_bits, valid, l2, min(k, n))
        oi, os_ = KNN[metric](q, whole, k)
        if l2:
            # batch_knn keeps its k best in a TopK, where the place of an EQUAL distance -- and with it which members of the group
            # of the k-th distance stay -- is core's binary search's business (test_gpu_exact.same_knn): against it the distances
            # are compared position by position, every group better than the k-th as a set, the k-th's as "rows of that
            # distance". Position by position the comparison is with the reference's sort-based squared-L2 kNN,
            # batch_knn_filtered under a predicate that passes everything (stable ascending sort from index order,
            # batch.rs:866-873): the order the library gives every L2 result.
            assert np.array_equal(gb, R.bits(os_)), (metric, k)
            inner = gb != gb[-1]
            assert same_knn("l2", gi[inner], R.f32(gb[inner]), oi[inner], os_[inner]), (metric, k)
            dist = R.bits(oracle.batch_l2_squared(q, whole))
            assert np.all(dist[gi[~inner].astype(np.int64)] == gb[-1]) and len(set(gi.tolist())) == len(gi)
            oi, os_ = oracle.batch_knn_filtered(q, whole, k, np.ones(n, np.uint8))
        assert gi.tolist() == oi.tolist() and np.array_equal(gb, R.bits(os_)), (metric, k)
        ties += int(np.sum(gb[1:] == gb[:-1]))
        # ... and topk_ref on the whole score list is the oracle's kNN
        full = {"dot": lambda: oracle.batch_dot(q, whole), "cos": lambda: oracle.batch_cosine(q, whole, oracle.batch_norms(whole)),
                "l2": lambda: oracle.batch_l2_squared(q, whole)}[metric]()
        ti, tb = R.topk_ref(R.bits(full), np.arange(n), l2, k)
        assert ti.tolist() == oi.tolist() and np.array_equal(tb, R.bits(os_))
    assert k == 1 or ties > 0  # the corpus does what it is for
