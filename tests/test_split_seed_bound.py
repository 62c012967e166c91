"""The certificate of the split filter's seeder, on the CPU: the groups of 32 rows are disjoint, so the k-th
largest of a prefix's group maxima is reached by at least k distinct rows and never exceeds the k-th best score -- of the prefix,
and so of any corpus that holds it. Checked where the maxima hide the most: every one of the k best rows in one group, and the
best row many times over."""
from __future__ import annotations

import numpy as np
import pytest

import split_seed_ref as R

P, N = 1024, 1024 + 700


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("dim", [40, 200])
@pytest.mark.parametrize("k", [1, 10, 32])
def test_kth_group_maximum_never_exceeds_the_kth_best(layout, dim, k):
    rows = R.corpus(layout, 32768 + 37, dim, 11)[:N].astype(np.float64)
    if layout == "copies":  # (the corpus' later copies lie beyond this slice: put some behind the prefix here too)
        rows[P + 5] = rows[7]
    qs = R.queries(70, dim, 5).astype(np.float64)
    for scores in (qs @ rows.T, (qs / np.linalg.norm(qs, axis=1)[:, None]) @ (rows / np.linalg.norm(rows, axis=1)[:, None]).T):
        gm = R.group_maxima(scores[:, :P])
        assert gm.shape == (70, P // 32)
        t = R.kth_largest(gm, k)
        assert np.all(t <= R.kth_largest(scores[:, :P], k))
        assert np.all(t <= R.kth_largest(scores, k))
        # the certificate itself: at least k rows of the prefix reach t
        assert np.all((scores[:, :P] >= t[:, None]).sum(axis=1) >= k)
        if layout == "one_group" and k > 1:
            # the k best rows share one group: the bound comes from an ordinary row, strictly below the k-th best
            assert np.all(t < R.kth_largest(scores, k))
        if layout == "random":
            assert np.all(R.kth_largest(gm, 1) == scores[:, :P].max(axis=1))


def test_groups_partition_the_prefix():
    ids = np.arange(P, dtype=np.float64)[None, :]
    gm = R.group_maxima(ids)
    # group g = 4 tile + rt holds rows 128 tile + 4 i + rt: its largest row number is 128 tile + 124 + rt
    g = np.arange(P // 32)
    assert np.array_equal(gm[0], 128 * (g // 4) + 124 + g % 4)
    rows = sorted(r for t in range(P // 128) for rt in range(4) for r in R.group_rows(t, rt, 32))
    assert rows == list(range(P))


def test_key_to_f32_inverts_the_order_key():
    x = np.array([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1e-40], np.float32)
    b = x.view(np.uint32)
    keys = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)  # common.h f32_ord
    assert np.array_equal(R.key_to_f32(keys).view(np.uint32), b)
    strict = np.array([0, 2, 3, 4, 5, 6])  # (without -0.0, which equals 0.0 as a float and sorts below it as a key)
    assert np.all(np.diff(keys[strict][np.argsort(x[strict])].astype(np.int64)) > 0)
