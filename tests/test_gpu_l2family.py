"""GPU parity tests, part 3: the L2 variants of src/batch.rs on the device -- batch_knn_filtered (:820-882),
batch_knn_reordered (:621-659) with batch_dimension_variance (:572-592), batch_l2_squared_pruning (:320-365)."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import kat_cases as K
from backends import HipBackend
from test_gpu_exact import _corpus, _queries, bits_equal, same_knn


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.mark.parametrize("kat", K.L2_FAMILY_KATS, ids=lambda f: f.__name__)
def test_reference_kat_l2_family(kat):
    kat(HipBackend())


@pytest.mark.parametrize("n,dim", [(1, 3), (2, 1), (300, 17), (5000, 64), (20_001, 128)])
def test_dimension_variance_bit_exact(B, n, dim):
    rows, data = _corpus(n, dim, 4, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    assert bits_equal(B.batch_dimension_variance(vb), oracle.batch_dimension_variance(data))


@pytest.mark.parametrize("n,dim,k", [(50, 16, 5), (200, 64, 10), (3000, 33, 40), (10_000, 128, 10)])
def test_reordered_equals_oracle(B, n, dim, k):
    rows, data = _corpus(n, dim, 21, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    for q in _queries(3, dim, 5, uniform=True):
        r = B.batch_knn_reordered(q, vb, k)
        oi, os_ = oracle.batch_knn_reordered(q, data, k)
        assert r.indices == oi.tolist() and bits_equal(np.float32(r.scores), os_)
        # the reference's claim (batch.rs:607): same neighbours as the plain exact kNN on well-separated data
        assert set(r.indices) == set(B.batch_knn(q, vb, k).indices)


@pytest.mark.parametrize("n,dim,k,mod", [(100, 2, 5, 2), (5000, 32, 10, 7), (5000, 32, 100, 3), (4099, 16, 240, 17)])
def test_filtered_equals_oracle(B, n, dim, k, mod):
    rows, data = _corpus(n, dim, 8, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    pred = lambda i: i % mod == 0  # noqa: E731
    mask = np.array([1 if pred(i) else 0 for i in range(n)], dtype=np.uint8)
    for q in _queries(3, dim, 6, uniform=True):
        r = B.batch_knn_filtered(q, vb, k, pred)
        oi, os_ = oracle.batch_knn_filtered(q, data, k, mask)
        assert r.indices == oi.tolist() and bits_equal(np.float32(r.scores), os_)
    # fewer passing than k -> min(k, passing) results (batch.rs:849)
    r = B.batch_knn_filtered(rows[0], vb, 50, lambda i: i < 3)
    assert sorted(r.indices) == [0, 1, 2] and r.indices[0] == 0


@pytest.mark.parametrize("n,dim", [(10, 2), (1000, 16), (70_000, 24)])
def test_pruning_equals_oracle(B, n, dim):
    rows, data = _corpus(n, dim, 9, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    q = _queries(1, dim, 3, uniform=True)[0]
    d = oracle.batch_l2_squared(q, data)
    for thr in (0.0, float(np.percentile(d, 1)), float(np.median(d)), 1e9):
        got = B.batch_l2_squared_pruning(q, vb, thr)
        oi, od = oracle.batch_l2_squared_pruning(q, data, thr)
        assert [g[0] for g in got] == oi.tolist()
        assert bits_equal(np.float32([g[1] for g in got]), od)


# =====================================================================================================================
# Ties, NaN signs and the paths the comparisons above never reach. Everything below is bit-exact against the oracle.
# =====================================================================================================================
import ctypes as C  # noqa: E402

import order_ref as R  # noqa: E402

SENT_I, SENT_F = np.uint64(0xDEADBEEFDEADBEEF), np.uint32(0xDEADBEEF)


def _setbits(a, where, pattern):
    """store a bit pattern (a NaN of a given sign / payload) into a float32 array without any conversion"""
    a.view(np.uint32)[where] = np.uint32(pattern)


# ------------------------------------------------------------------------------------------------ A. dimension_variance
@pytest.mark.parametrize("dim", [1, 65, 130])    # one lane per dimension, 64 lanes per workgroup: a partial last workgroup
@pytest.mark.parametrize("n", [2, 3, 5, 7, 1023])  # float4 body + 0..3 tail elements; n < 4: tail only
def test_dimension_variance_tails(B, n, dim):
    rows, data = _corpus(n, dim, 40 + n, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        assert bits_equal(B.batch_dimension_variance(vb), oracle.batch_dimension_variance(data))
    finally:
        vb.close()


def _special_columns(n=41, dim=12):
    """One special per column; at most one NaN per column and never two signs in one (test_gpu_range_search._special_queries: a
    sum with two NaN operands of different sign is ISA-defined even in the reference)."""
    rows = oracle.generate_uniform(n, dim, 77).copy()
    _setbits(rows, (5 % n, 0), R.PNAN)   # a single +NaN: sum, mean and every x - mean are +NaN in the reference
    _setbits(rows, (17 % n, 1), R.NNAN)  # a single -NaN
    rows[3 % n, 2] = np.inf              # mean = +inf, inf - inf in that row: a GENERATED NaN (0xFFC00000, include/innr_hip.h)
    rows[9 % n, 3] = -np.inf
    rows[:, 4] = np.float32(0.37)       # constant
    rows[:, 5] = np.float32(-0.0)       # the sums fold from -0.0 and stay there
    rows[:, 6] = np.float32(3e38)       # the sum overflows: mean = inf, variance = inf, no NaN
    rows[:, 8] = rows[:, 7]             # two bit-identical columns
    return rows


@pytest.mark.parametrize("n", [41, 3])  # 3: the kernel's scalar tail loops alone (their own subtraction)
def test_dimension_variance_special_columns(B, n):
    """While the kernel subtracted the mean with a plain a - b (gfx950: a + (-b), which flips the sign of a NaN mean), the device
    returned 0xFFC00000 for the +NaN column and 0x7FC00000 for the -NaN one; the infinite columns matched (0xFFC00000)."""
    rows = _special_columns(n)
    data = oracle.from_rows(rows)
    want = oracle.batch_dimension_variance(data)
    # what the reference's arithmetic gives on the host ISAs: a propagated NaN keeps its sign, a generated one is 0xFFC00000
    assert R.bits(want)[[0, 1, 2, 3]].tolist() == [R.PNAN, R.NNAN, R.NNAN, R.NNAN]
    assert R.bits(want)[5] == R.PZERO and R.bits(want)[6] == R.PINF and R.bits(want)[7] == R.bits(want)[8]
    vb = B.VerticalBatch.from_rows(rows)
    try:
        got = B.batch_dimension_variance(vb)
        print("variance bits: +NaN column %#010x, -NaN column %#010x, +inf column %#010x, -inf column %#010x"
              % tuple(int(x) for x in R.bits(got)[[0, 1, 2, 3]]))
        assert bits_equal(got, want), [hex(int(x)) for x in R.bits(got)]
        assert bits_equal(B.batch_dimension_variance(vb), want)  # the cached copy
        # a prefix view has its own cache: the parent's 12 variances are cached by now, the view answers for its own dimensions
        for p in (1, 2, 9):
            view = vb.prefix(p)
            assert bits_equal(B.batch_dimension_variance(view), oracle.batch_dimension_variance(data[:p])), p
            view.close()
    finally:
        vb.close()


def test_dimension_variance_prefix_view_before_parent(B):
    rows, data = _corpus(257, 9, 5, uniform=True)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        view = vb.prefix(4)
        assert bits_equal(B.batch_dimension_variance(view), oracle.batch_dimension_variance(data[:4]))
        assert bits_equal(B.batch_dimension_variance(vb), oracle.batch_dimension_variance(data))
        assert bits_equal(B.batch_dimension_variance(view), oracle.batch_dimension_variance(data[:4]))
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ B. knn_reordered
def _reordered_emulation(q, data, order, k):
    """batch_knn_reordered (batch.rs:640-657) in NumPy f32, one dimension at a time in `order`: (indices, distance bits) of the k
    nearest, and the distance bits of all rows. Separate multiply and add: two roundings, like the reference."""
    dist = np.zeros(data.shape[1], np.float32)
    for d in order:
        diff = np.float32(q[d]) - data[d]
        dist = dist + diff * diff
    idx, b = R.topk_ref(R.bits(dist), np.arange(dist.size), True, k)
    return idx, b, R.bits(dist)


def _variance_order(data):
    """variance_order (batch.rs:599-603): stable sort of the dimensions by variance, descending total_cmp"""
    var = oracle.batch_dimension_variance(data)
    return R.order_of(R.bits(var), np.arange(var.size), False).tolist()


def _check_reordered(B, vb, q, data, k, base=0):
    r = B.batch_knn_reordered(q, vb, k)
    oi, os_ = oracle.batch_knn_reordered(q, data, k)
    assert r.indices == (oi + np.uint64(base)).tolist(), (r.indices, oi)
    assert bits_equal(np.float32(r.scores), os_)
    return oi, os_


@pytest.mark.parametrize("k", [10, 300])  # 300 = N > INNR_MAX_K: every distance in the caller's order, then the full sort
def test_reordered_nan_dimension_comes_first(B, k):
    """A dimension holding one +NaN has variance +NaN, which a descending total_cmp sort puts FIRST. A device variance of -NaN
    would put it last, and every finite row would accumulate its distance in another order."""
    n, dim, nan_dim = 300, 17, 6
    rows = oracle.generate_uniform(n, dim, 1234).copy()
    _setbits(rows, (123, nan_dim), R.PNAN)
    data = oracle.from_rows(rows)
    q = oracle.generate_uniform(1, dim, 4321)[0]
    order = _variance_order(data)
    assert order[0] == nan_dim
    moved = order[1:] + [nan_dim]  # the order a sign-flipped NaN variance gives
    oi, os_ = oracle.batch_knn_reordered(q, data, k)
    ei, eb, _ = _reordered_emulation(q, data, order, k)
    assert ei.tolist() == oi.tolist() and np.array_equal(eb, R.bits(os_))  # the emulation is the oracle
    mi, mb, _ = _reordered_emulation(q, data, moved, k)
    # this is what lets the comparison below fail: the other place for the NaN dimension changes top-k score bits
    changed = int(np.sum(mb != eb))
    print(f"k={k}: moving the NaN dimension to the end changes {changed} of {k} top-k score bit patterns")
    assert changed >= 1
    vb = B.VerticalBatch.from_rows(rows)
    try:
        got = B.batch_dimension_variance(vb)
        print("device variance of the +NaN dimension: %#010x" % int(R.bits(got)[nan_dim]))
        _check_reordered(B, vb, q, data, k)
    finally:
        vb.close()


@pytest.mark.parametrize("k", [10, 300])
def test_reordered_variance_ties_keep_dimension_order(B, k):
    """Two bit-identical columns d1 < d2 have equal variance: the stable sort keeps d1 before d2. The query differs in the two
    dimensions, so the other order sums other numbers."""
    n, dim, d1, d2 = 300, 17, 4, 11
    rows = oracle.generate_uniform(n, dim, 2345).copy()
    rows[:, d2] = rows[:, d1]
    data = oracle.from_rows(rows)
    q = oracle.generate_uniform(1, dim, 5432)[0].copy()
    q[d1], q[d2] = np.float32(0.75), np.float32(-0.4)
    order = _variance_order(data)
    p1, p2 = order.index(d1), order.index(d2)
    assert p2 == p1 + 1
    swapped = list(order)
    swapped[p1], swapped[p2] = d2, d1
    oi, os_ = oracle.batch_knn_reordered(q, data, k)
    ei, eb, _ = _reordered_emulation(q, data, order, k)
    assert ei.tolist() == oi.tolist() and np.array_equal(eb, R.bits(os_))
    mi, mb, _ = _reordered_emulation(q, data, swapped, k)
    changed = int(np.sum(mb != eb))
    print(f"k={k}: d2 before d1 changes {changed} of {k} top-k score bit patterns")
    assert changed >= 1
    vb = B.VerticalBatch.from_rows(rows)
    try:
        _check_reordered(B, vb, q, data, k)
    finally:
        vb.close()


@pytest.mark.parametrize("n,k", [(1, 1), (1, 3), (5, 5), (7, 7), (7, 3), (7, 100), (300, 10), (300, 300), (300, 1000)])
def test_reordered_exact_distance_ties(B, n, k):
    """Duplicate rows have equal distances: the lower index comes first (stable ascending sort from index order, batch.rs:651).
    k = N < 8, N = 1 and k > N included; once more with an index base and on a prefix view."""
    dim = 6
    pat = oracle.generate_uniform(3, dim, 99)
    rows = np.ascontiguousarray(pat[np.arange(n) % 3 if n < 8 else np.random.default_rng(7).integers(0, 3, size=n)])
    data = oracle.from_rows(rows)
    q = oracle.generate_uniform(1, dim, 98)[0]
    vb = B.VerticalBatch.from_rows(rows)
    try:
        oi, os_ = _check_reordered(B, vb, q, data, k)
        assert len(oi) == min(k, n)
        b = R.bits(os_)
        assert all(oi[t] < oi[t + 1] for t in range(len(oi) - 1) if b[t] == b[t + 1])
        assert n < 3 or k < 2 or np.any(b[1:] == b[:-1])  # there ARE ties in the result
        base = (1 << 40) + 77
        vb.set_index_base(base)
        _check_reordered(B, vb, q, data, k, base=base)
        vb.set_index_base(0)
        view = vb.prefix(4)
        _check_reordered(B, view, q[:4], data[:4], k)
        view.close()
    finally:
        vb.close()


# ------------------------------------------------------------------------------------------------ C. knn_filtered, the C ABI
def _filtered_abi(vb, q, k, mask):
    """innr_batch_knn_filtered with the caller's own mask bytes (the Python wrapper only ever makes 0 / 1)"""
    from innr_amd import _lib
    n = vb.num_vectors()
    kk = max(min(int(k), n), 1)
    idx = np.full(kk, SENT_I, np.uint64)
    sc = np.zeros(kk, np.float32)
    out_k = C.c_size_t(12345)
    q = np.ascontiguousarray(q, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    assert mask.size == n
    _lib.check(_lib.load().innr_batch_knn_filtered(vb._h, q.ctypes.data, q.size, int(k), mask.ctypes.data, idx.ctypes.data,
                                                   sc.ctypes.data, C.byref(out_k)))
    r = int(out_k.value)
    return idx[:r], sc[:r]


MASK_BYTES = np.array([0, 1, 2, 0x80, 0xFF], np.uint8)


def _masks(n, rng):
    nz = MASK_BYTES[1:]
    only_last = np.zeros(n, np.uint8); only_last[n - 1] = 0x80
    only_first = np.zeros(n, np.uint8); only_first[0] = 2
    return {"mixed": MASK_BYTES[rng.integers(0, 5, size=n)], "only_last": only_last, "only_first": only_first,
            "none": np.zeros(n, np.uint8), "all": nz[rng.integers(0, 4, size=n)]}


def _filtered_rows(n, dim, mask, rng):
    """Rows that do not pass hold NaN / +-inf (they must not matter); the passing ones hold duplicates and one +NaN in dimension 0"""
    rows = oracle.generate_uniform(n, dim, 500 + n).copy()
    out = np.flatnonzero(mask == 0)
    poison = np.array([np.nan, np.inf, -np.inf], np.float32)
    for t, i in enumerate(out):
        rows[i, t % dim] = poison[t % 3]
        if t % 4 == 0:
            _setbits(rows, (i, 0), R.NNAN)
    ok = np.flatnonzero(mask != 0)
    if ok.size >= 4:
        dup = rng.choice(ok, size=max(ok.size // 2, 2), replace=False)
        rows[dup[1:]] = rows[dup[0]]                         # one large group of equal distances
        _setbits(rows, (int(ok[ok.size // 2]), 0), R.PNAN)   # (may land in the group: then that copy's distance is +NaN)
    return rows


@pytest.mark.parametrize("n", [5, 6, 7, 1021, 4099])  # N % 4 = 1, 2, 3, 1, 3: the last mask word is read byte by byte
def test_filtered_mask_bytes_through_the_abi(B, n):
    """The contract is mask[i] != 0. k <= 240 takes the candidate lists, k > 240 (N > 240) the full sort with non-passing vectors
    keyed last; fewer passing than k gives min(k, passing)."""
    dim = 6
    rng = np.random.default_rng(n)
    q = oracle.generate_uniform(1, dim, 600 + n)[0]
    for name, mask in _masks(n, rng).items():
        rows = _filtered_rows(n, dim, mask, rng)
        data = oracle.from_rows(rows)
        passing = int(np.count_nonzero(mask))
        vb = B.VerticalBatch.from_rows(rows)
        try:
            for k in (1, 3, 240, 241, n, n + 3):
                gi, gs = _filtered_abi(vb, q, k, mask)
                oi, os_ = oracle.batch_knn_filtered(q, data, k, (mask != 0).astype(np.uint8))
                assert len(gi) == min(k, passing), (name, k)
                assert gi.tolist() == oi.tolist() and bits_equal(gs, os_), (name, k, gi[:8], oi[:8])
            if name == "mixed":
                base = (1 << 36) + 5
                vb.set_index_base(base)
                gi, gs = _filtered_abi(vb, q, 7, mask)
                oi, os_ = oracle.batch_knn_filtered(q, data, 7, (mask != 0).astype(np.uint8))
                assert gi.tolist() == (oi + np.uint64(base)).tolist() and bits_equal(gs, os_)
        finally:
            vb.close()


# ------------------------------------------------------------------------------------------------ D. l2_squared_pruning, the C ABI
def _pruning_abi(vb, q, thr, cap, room=None, null=False):
    """innr_batch_l2_squared_pruning -> (*out_n, index buffer, distance-bits buffer); the buffers hold `room` (default cap + 16)
    sentinel-filled entries of which the call may write the first min(*out_n, cap)."""
    from innr_amd import _lib
    room = cap + 16 if room is None else room
    idx = np.full(room, SENT_I, np.uint64)
    ds = np.full(room, SENT_F, np.uint32)
    out_n = C.c_size_t(54321)
    q = np.ascontiguousarray(q, np.float32)
    _lib.check(_lib.load().innr_batch_l2_squared_pruning(vb._h, q.ctypes.data, q.size, C.c_float(thr), None if null else idx.ctypes.data,
                                                         None if null else ds.ctypes.data, int(cap), C.byref(out_n)))
    return int(out_n.value), idx, ds


class _Prune:
    """300 001 x 4: 1172 chunks of 256, so the single-workgroup scan of the chunk counts gives each thread two (per = 2)"""
    n, dim = 300_001, 4

    def __init__(self, B):
        rows = oracle.generate_uniform(self.n, self.dim, 9).copy()
        # NaNs in dimension 0 ONLY: the device keeps a vector on its FULL distance, the reference drops it on a partial sum before
        # a late NaN arrives (a documented difference, test_gpu_range_search._special_rows); +-inf rows: their distance is +inf
        _setbits(rows, (7, 0), R.PNAN)
        _setbits(rows, (200_000, 0), R.NNAN)
        rows[9, 1] = np.inf
        rows[300_000, 2] = -np.inf
        self.q = rows[5].copy()           # the query equals rows 5 and 262_200: distance +0.0
        rows[262_200] = rows[5]
        self.rows = rows
        self.data = oracle.from_rows(rows)
        self.vb = B.VerticalBatch.from_rows(rows)
        d = oracle.batch_l2_squared(self.q, self.data)
        fin = d[np.isfinite(d)]
        self.p1, self.median, self.above = float(np.percentile(fin, 1)), float(np.median(fin)), float(fin.max()) * 2.0
        self._oracle = {}

    def want(self, thr):
        key = int(R.bits([thr])[0])
        if key not in self._oracle:
            oi, od = oracle.batch_l2_squared_pruning(self.q, self.data, thr)
            self._oracle[key] = (oi, R.bits(od))
        return self._oracle[key]


@pytest.fixture(scope="module")
def prune(B):
    p = _Prune(B)
    yield p
    p.vb.close()


def _assert_pruned(got, want, cap, what):
    n, idx, ds = got
    oi, ob = want
    m = min(len(oi), cap)
    assert n == len(oi), (what, n, len(oi))                      # *out_n is the full count, whatever cap is
    assert np.array_equal(idx[:m], oi[:m]) and np.array_equal(ds[:m], ob[:m]), what
    assert np.all(idx[m:] == SENT_I) and np.all(ds[m:] == SENT_F), what  # nothing is written past min(total, cap)


@pytest.mark.parametrize("which", ["p1", "median", "above"])
def test_pruning_scan_with_two_counts_per_thread(prune, which):
    thr = getattr(prune, which)
    want = prune.want(thr)
    assert len(want[0]) > 1500 and (which != "above" or len(want[0]) == prune.n - 2)
    _assert_pruned(_pruning_abi(prune.vb, prune.q, thr, prune.n), want, prune.n, which)


def test_pruning_cap_below_the_survivor_count(prune):
    want = prune.want(prune.median)
    total = len(want[0])
    for cap in (total - 1, 1):
        _assert_pruned(_pruning_abi(prune.vb, prune.q, prune.median, cap), want, cap, f"cap={cap}")
    # the count-only call: cap = 0 and null buffers
    n, _, _ = _pruning_abi(prune.vb, prune.q, prune.median, 0, null=True)
    assert n == total
    _assert_pruned(_pruning_abi(prune.vb, prune.q, prune.median, 0), want, 0, "cap=0")


@pytest.mark.parametrize("thr_bits,expect", [(R.PNAN, "all"), (R.NNAN, "all"), (R.PINF, "all"), (R.NINF, "nan"), (R.NZERO, "zero+nan"),
                                             (R.PZERO, "zero+nan")])
def test_pruning_special_thresholds(prune, thr_bits, expect):
    """`dist > threshold` drops: false for a NaN threshold or a NaN distance; inf > inf is false; 0 > -0.0 is false"""
    thr = float(R.f32([thr_bits])[0])
    want = prune.want(thr)
    expected = {"all": list(range(prune.n)), "nan": [7, 200_000], "zero+nan": [5, 7, 200_000, 262_200]}[expect]
    assert want[0].tolist() == expected
    _assert_pruned(_pruning_abi(prune.vb, prune.q, thr, prune.n), want, prune.n, hex(thr_bits))


def test_pruning_index_base_prefix_view_and_range_search(B, prune):
    import innr_amd
    want = prune.want(prune.p1)
    base = (1 << 35) + 3
    prune.vb.set_index_base(base)
    try:
        _assert_pruned(_pruning_abi(prune.vb, prune.q, prune.p1, prune.n), (want[0] + np.uint64(base), want[1]), prune.n, "base")
    finally:
        prune.vb.set_index_base(0)
    view = prune.vb.prefix(3)
    thr3 = prune.p1 * 0.5
    oi, od = oracle.batch_l2_squared_pruning(prune.q[:3], prune.data[:3], thr3)
    assert len(oi) > 100
    _assert_pruned(_pruning_abi(view, prune.q[:3], thr3, prune.n), (oi, R.bits(od)), prune.n, "prefix view")
    view.close()
    # include/innr_hip.h: for Q = 1 and squared L2 innr_batch_range_search's result equals this function's bit for bit
    for thr in (prune.p1, prune.median, float("nan"), -0.0, float("-inf")):
        n, idx, ds = _pruning_abi(prune.vb, prune.q, thr, prune.n)
        off, ri, rs = B.batch_range_search(prune.q, prune.vb, thr, metric=innr_amd.METRIC_L2SQ)
        assert off.tolist() == [0, n] and np.array_equal(ri, idx[:n]) and np.array_equal(R.bits(rs), ds[:n]), thr
