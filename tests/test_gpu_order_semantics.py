"""GPU: the ORDER of the re-rank (innr_batch_rerank[_dev]) and of the shard-merge kernels (innr_merge_topk_dev, innr_topk_pack_dev,
innr_merge_blocks_dev) on the inputs uniform random data never produces: equal scores, -0.0 / +0.0, +-inf, NaNs of both signs,
empty slots in the middle of a list, candidates whose preference key is 0, and the sizes at which a kernel changes its path.
Every comparison is bit-exact against tests/order_ref.py (validated against the oracle on the CPU by tests/test_order_ref.py):
sorted by (total-order key in the metric's direction, index ascending)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import order_ref as R

METRICS = ("dot", "cos", "l2")


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module", autouse=True)
def _torch_device_up():
    """torch's import and its first touch of the device happen here, not inside whichever test needs a device tensor first"""
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()


def _met(innr, metric):
    return {"dot": innr.METRIC_DOT, "cos": innr.METRIC_COSINE, "l2": innr.METRIC_L2SQ}[metric]


# =====================================================================================================================
# E. batch_rerank, host and _dev
# =====================================================================================================================
def _all_scores(metric, qs, data):
    """the oracle's exact score of every (query, row): [Q, N] bit patterns"""
    norms = oracle.batch_norms(data) if metric == "cos" else None
    fn = {"dot": lambda q: oracle.batch_dot(q, data), "cos": lambda q: oracle.batch_cosine(q, data, norms),
          "l2": lambda q: oracle.batch_l2_squared(q, data)}[metric]
    return np.stack([R.bits(fn(q)) for q in qs])


def _rerank_ref(metric, score_bits, cand, k):
    """per query: the candidates' (score, index) pairs in result order, cut to k"""
    out = [R.topk_ref(score_bits[j][cand[j].astype(np.int64)], cand[j], metric == "l2", k) for j in range(len(cand))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _rerank_dev(vb, qs, cand, k, met):
    """innr_batch_rerank_dev: queries, candidates and results in device memory"""
    import torch
    from innr_amd import _lib
    dev = torch.device("cuda", 0)
    vb._ctx.bind_torch_stream()
    q = torch.from_numpy(np.ascontiguousarray(qs, np.float32)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(cand, np.uint64).view(np.int64)).to(dev)
    nq, kc = cand.shape
    kk = max(min(int(k), kc), 1)
    idx = torch.empty((nq * kk,), dtype=torch.int64, device=dev)
    sc = torch.empty((nq * kk,), dtype=torch.float32, device=dev)
    out_k = C.c_size_t(0)
    _lib.check(_lib.load().innr_batch_rerank_dev(vb._h, met, C.c_void_p(q.data_ptr()), nq, q.shape[1], C.c_void_p(c.data_ptr()), kc,
                                                 int(k), C.c_void_p(idx.data_ptr()), C.c_void_p(sc.data_ptr()), C.byref(out_k)))
    torch.cuda.synchronize()
    r = int(out_k.value)
    return (idx[:nq * r].cpu().numpy().view(np.uint64).reshape(nq, r), sc[:nq * r].cpu().numpy().reshape(nq, r))


def _check_rerank(B, innr, vb, metric, qs, score_bits, cand, k, base=0, what=""):
    """host and device entry point against the reference; `cand` holds LOCAL indices, the calls get base + cand"""
    met = _met(innr, metric)
    wi, wb = _rerank_ref(metric, score_bits, cand, k)
    gcand = cand.astype(np.uint64) + np.uint64(base)
    for name, (gi, gs) in (("host", B.batch_rerank(qs, vb, gcand, k, met)), ("dev", _rerank_dev(vb, qs, gcand, k, met))):
        assert gi.shape == wi.shape, (what, name, gi.shape, wi.shape)
        assert np.array_equal(gi, wi + np.uint64(base)), (what, name, metric)
        assert np.array_equal(R.bits(gs), wb), (what, name, metric)
    return wi, wb


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kc", [8, 256, 257, 300])  # <= 256: candidate lists; beyond: one thread per candidate, segment sort
def test_rerank_ties_come_out_in_index_order(B, innr, metric, kc):
    """Candidates that are copies of one corpus row score the same bits: index order decides, whatever order they were given in"""
    n, dim, nq = 400, 8, 3
    pat = oracle.generate_uniform(5, dim, 41)
    rng = np.random.default_rng(kc)
    rows = np.ascontiguousarray(pat[rng.integers(0, 5, size=n)])
    data = oracle.from_rows(rows)
    qs = oracle.generate_uniform(nq, dim, 42)
    sb = _all_scores(metric, qs, data)
    shuffled = np.stack([rng.choice(n, size=kc, replace=False) for _ in range(nq)]).astype(np.uint64)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for k in (kc, 5):
            wi, wb = _check_rerank(B, innr, vb, metric, qs, sb, shuffled, k, what=f"shuffled k={k}")
            _check_rerank(B, innr, vb, metric, qs, sb, np.sort(shuffled, axis=1), k, what=f"sorted k={k}")  # the same reference
            assert np.array_equal(_rerank_ref(metric, sb, np.sort(shuffled, axis=1), k)[0], wi)
        # five distinct scores among kc >= 8 candidates: the result is runs of equal bits with ascending indices inside
        wi, wb = _rerank_ref(metric, sb, shuffled, kc)
        assert all(len(set(wb[j].tolist())) <= 5 for j in range(nq))
        assert all(wi[j][t] < wi[j][t + 1] for j in range(nq) for t in range(kc - 1) if wb[j][t] == wb[j][t + 1])
    finally:
        vb.close()


@pytest.mark.parametrize("metric", ["dot", "l2"])  # (an infinite row's cosine is a generated NaN, pinned by the exact engine's tests)
@pytest.mark.parametrize("n", [40, 300])           # every row is a candidate: kc = 40 (lists) and kc = 300 (segment sort)
def test_rerank_special_scores(B, innr, metric, n):
    """Rows that score +NaN, +inf, -inf (dot) and +0.0: +NaN is the best dot score and the worst distance, +-inf sit at the ends
    of the finite range, equal zeros tie by index. (-0.0 cannot come out of these scores: the accumulators start at +0.0, and
    +0.0 + -0.0 = +0.0; the merge tests below order -0.0 against +0.0.) One NaN per row, none in the queries: a sum with two
    NaN operands is the ISA's business (test_gpu_range_search._special_queries)."""
    dim, nq = 6, 3
    rows = oracle.generate_uniform(n, dim, 43).copy()
    rows.view(np.uint32)[2, 0] = R.PNAN
    rows.view(np.uint32)[n - 3, 4] = R.PNAN
    rows[5, 1] = np.inf
    rows[n - 2, 1] = np.inf
    rows[7, 2] = -np.inf
    rows[11, :] = 0.0
    rows[n - 1, :] = 0.0
    rows[13, :] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    qs = oracle.generate_uniform(nq, dim, 44).copy()
    qs[1, 1] = -qs[0, 1]                      # opposite signs in the +-inf dimension: both infinities occur among the dot scores
    qs[2] = 0.0 if metric == "l2" else qs[2]  # squared L2: the zero rows are at distance +0.0 from the zero query
    data = oracle.from_rows(rows)
    sb = _all_scores(metric, qs, data)
    seen = set(np.unique(sb).tolist())
    assert {R.PNAN, R.PINF, R.PZERO} <= seen and (metric == "l2" or R.NINF in seen) and R.NZERO not in seen
    cand = np.tile(np.arange(n, dtype=np.uint64)[::-1], (nq, 1))  # given in DESCENDING index order
    vb = B.VerticalBatch.from_rows(rows)
    try:
        for k in (n, 7):
            _check_rerank(B, innr, vb, metric, qs, sb, cand, k, what=f"k={k}")
    finally:
        vb.close()


@pytest.mark.parametrize("metric", METRICS)
def test_rerank_more_results_than_the_lds_sort_window(B, innr, metric):
    """k = kc = 4500 > kSelSlots (4096): the per-query radix select + global bitonic sort"""
    n, dim, nq, kc = 5000, 8, 2, 4500
    rows = oracle.generate_uniform(n, dim, 45)
    data = oracle.from_rows(rows)
    qs = oracle.generate_uniform(nq, dim, 46)
    sb = _all_scores(metric, qs, data)
    rng = np.random.default_rng(47)
    cand = np.stack([rng.choice(n, size=kc, replace=False) for _ in range(nq)]).astype(np.uint64)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        _check_rerank(B, innr, vb, metric, qs, sb, cand, kc)
    finally:
        vb.close()


@pytest.mark.parametrize("kc", [40, 300])
def test_rerank_index_base_near_2_40(B, innr, kc):
    n, dim, nq = 400, 8, 2
    pat = oracle.generate_uniform(7, dim, 48)
    rng = np.random.default_rng(49)
    rows = np.ascontiguousarray(pat[rng.integers(0, 7, size=n)])
    data = oracle.from_rows(rows)
    qs = oracle.generate_uniform(nq, dim, 50)
    cand = np.stack([rng.choice(n, size=kc, replace=False) for _ in range(nq)]).astype(np.uint64)
    vb = B.VerticalBatch.from_rows(rows)
    try:
        vb.set_index_base((1 << 40) - 17)  # the results straddle 2^40
        for metric in METRICS:
            _check_rerank(B, innr, vb, metric, qs, _all_scores(metric, qs, data), cand, kc, base=(1 << 40) - 17)
    finally:
        vb.close()


# =====================================================================================================================
# F. merge and pack, on one GPU with synthetic lists
# =====================================================================================================================
NO_CAND = 0xFFFFFFFF            # the exchange block's "no candidate" entry (score bits 0, local index all ones)
INVALID = np.uint64(2**64 - 1)  # innr_merge_topk_dev's empty slot


@pytest.fixture(scope="module")
def gpu(innr):
    import torch
    ctx = innr.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx, torch.device("cuda", 0)
    ctx.close()


def _pref0_bits(metric):
    """the VALID candidate whose preference key is 0, like an empty slot's: the lowest total-order key for dot / cosine (-NaN with
    every payload bit set), the highest for squared L2 (+NaN with every payload bit set)"""
    return 0x7FFFFFFF if metric == "l2" else 0xFFFFFFFF


def _shard_lists(metric, counts, k, nq, pool, seed, pref0_at=None, stride=1000):
    """G shards of `counts` vectors at bases 0, stride, ...: per shard and query min(k, count) valid candidates with score bits drawn
    from `pool` (so scores repeat within and across shards) and distinct local indices, each list in result order like a real
    local search's; the slots beyond stay empty. pref0_at = (g, slot): that candidate gets the preference-key-0 score.
    Returns idx [G, Q, k] uint64 (INVALID in empty slots), bits [G, Q, k] uint32, valid [G, Q, k], bases."""
    rng = np.random.default_rng(seed)
    G = len(counts)
    idx = np.full((G, nq, k), INVALID, np.uint64)
    # an empty slot's score must not matter: give it the bits that would WIN if it were read
    bits = np.full((G, nq, k), R.NINF if metric == "l2" else R.PNAN, np.uint32)
    valid = np.zeros((G, nq, k), bool)
    bases = [g * stride for g in range(G)]
    for g, count in enumerate(counts):
        kin = min(k, count)
        for j in range(nq):
            if kin == 0:
                continue
            b = np.asarray(pool, np.uint32)[rng.integers(0, len(pool), size=kin)]
            if pref0_at is not None and pref0_at[0] == g:
                b[pref0_at[1]] = _pref0_bits(metric)
            loc = rng.choice(count, size=kin, replace=False).astype(np.uint64) + np.uint64(bases[g])
            li, lb = R.topk_ref(b, loc, metric == "l2", kin)
            idx[g, j, :kin], bits[g, j, :kin], valid[g, j, :kin] = li, lb, True
    return idx, bits, valid, bases


def _merge_want(metric, idx, bits, valid, kout):
    nq = idx.shape[1]
    out = [R.merge_ref(idx[:, j], bits[:, j], valid[:, j], metric == "l2", kout) for j in range(nq)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _to_dev(dev, idx, bits):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(idx).view(np.int64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(bits).view(np.float32)).to(dev))


def _from_dev(i, s):
    return i.cpu().numpy().view(np.uint64), s.cpu().numpy().view(np.uint32)


def _run_merge_topk(innr, gpu, metric, idx, bits, kout):
    from innr_amd.dist import _gpu_merge
    import torch
    ctx, dev = gpu
    di, ds = _to_dev(dev, idx, bits)
    oi, os_ = _gpu_merge(ctx, _met(innr, metric))(di, ds, kout)
    torch.cuda.synchronize()
    return _from_dev(oi, os_)


def _run_merge_blocks(innr, gpu, metric, idx, bits, valid, bases, counts, k):
    """pack every shard's list (its min(k, count) leading entries) with innr_topk_pack_dev, stack, innr_merge_blocks_dev"""
    from innr_amd.dist import gpu_merge_blocks, gpu_pack_block
    import torch
    ctx, dev = gpu
    nq = idx.shape[1]
    blocks = []
    for g, count in enumerate(counts):
        kin = min(k, count)
        assert valid[g, :, :kin].all() and not valid[g, :, kin:].any()  # header consistency: exactly min(k, count) valid entries
        di, ds = _to_dev(dev, idx[g, :, :kin], bits[g, :, :kin])
        blocks.append(gpu_pack_block(ctx, di, ds, bases[g], count, k))
    oi, os_ = gpu_merge_blocks(ctx, _met(innr, metric), torch.stack(blocks), nq, k)
    torch.cuda.synchronize()
    return _from_dev(oi, os_)


SPECIAL_POOL = [0x3F800000, 0x3F800000, 0x3F800000, R.NZERO, R.PZERO, R.PINF, R.NINF, R.PNAN, R.NNAN, 0xBF800000, 0x00000001, 0x80000001]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("counts,pref0_at", [((1000, 900, 0, 5), (3, 2)),   # an empty shard, one shorter than k; kout = k = 8
                                             ((3, 0, 2, 1), (2, 1))],       # six vectors in all: kout = 6, EVERY valid one is output
                         ids=["k_of_many", "all_of_six"])
def test_merge_special_scores_and_ties(innr, gpu, metric, counts, pref0_at):
    """Equal scores across shards (the global index decides), -0.0 below +0.0, +-inf, +-NaN, and a valid candidate with preference
    key 0 -- in the six-vector case it is part of the result and must come before the empty slots, which share its key."""
    k, nq = 8, 3
    idx, bits, valid, bases = _shard_lists(metric, counts, k, nq, SPECIAL_POOL, seed=len(metric) + sum(counts), pref0_at=pref0_at)
    kout = min(k, sum(counts))
    wi, wb = _merge_want(metric, idx, bits, valid, kout)
    if sum(counts) <= k:
        assert all(_pref0_bits(metric) == wb[j][-1] for j in range(nq))  # ... as the last of the six
    assert any(wb[j][t] == wb[j][t + 1] and (wi[j][t] // 1000) != (wi[j][t + 1] // 1000) for j in range(nq) for t in range(kout - 1)) \
        or sum(counts) <= k  # a tie ACROSS shards is in the result
    ti, tb = _run_merge_topk(innr, gpu, metric, idx, bits, kout)
    assert np.array_equal(ti, wi) and np.array_equal(tb, wb), (metric, ti, wi)
    bi, bb = _run_merge_blocks(innr, gpu, metric, idx, bits, valid, bases, counts, k)
    assert bi.shape == (nq, kout) and np.array_equal(bi, wi) and np.array_equal(bb, wb), (metric, bi, wi)


@pytest.mark.parametrize("metric", METRICS)
def test_merge_topk_empty_slot_between_valid_ones(innr, gpu, metric):
    """innr_merge_topk_dev takes any list: UINT64_MAX marks an empty slot wherever it stands, and its score is not read"""
    k, nq, counts = 8, 3, (1000, 900, 700, 5)
    idx, bits, valid, _ = _shard_lists(metric, counts, k, nq, SPECIAL_POOL, seed=5)
    for g, slot in ((0, 3), (1, 0), (2, 6), (3, 1)):
        idx[g, :, slot], valid[g, :, slot] = INVALID, False
        bits[g, :, slot] = R.NINF if metric == "l2" else R.PNAN
    wi, wb = _merge_want(metric, idx, bits, valid, k)
    ti, tb = _run_merge_topk(innr, gpu, metric, idx, bits, k)
    assert np.array_equal(ti, wi) and np.array_equal(tb, wb), (metric, ti, wi)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1024, 1025])  # G * k = 3072: the last size staged in LDS; 3073: candidates re-read from global memory
def test_merge_blocks_lds_staging_switch(innr, gpu, metric, k):
    """Each shard repeats the same eight scores, so nearly every comparison is decided by the global index"""
    nq, counts = 3, (5000, 4000, 3000)
    pool = [0x3F800000, 0xBF800000, R.PZERO, R.NZERO, 0x3F000000, R.PINF, R.NINF, R.PNAN]
    idx, bits, valid, bases = _shard_lists(metric, counts, k, nq, pool, seed=k, stride=10_000)
    wi, wb = _merge_want(metric, idx, bits, valid, k)
    bi, bb = _run_merge_blocks(innr, gpu, metric, idx, bits, valid, bases, counts, k)
    assert bi.shape == (nq, k) and np.array_equal(bi, wi) and np.array_equal(bb, wb), metric
    ti, tb = _run_merge_topk(innr, gpu, metric, idx, bits, k)  # equal inputs: the two kernels agree bit for bit
    assert np.array_equal(ti, bi) and np.array_equal(tb, bb), metric


def test_pack_block_words(gpu):
    """innr_topk_pack_dev: header = {base, count}; an entry is score bits << 32 | local index -- the bits as they are, NaN payload
    included; an index below the base, a local index >= 2^32 - 1 and the slots kin..k are the "no candidate" entry."""
    from innr_amd.dist import gpu_pack_block
    import torch
    ctx, dev = gpu
    base, count, k, kin, nq = (1 << 40) + 1000, 77_000, 7, 5, 3
    loc = np.array([[0, 76_999, 5, 17, 3],
                    [1, 2, 3, 4, 6],
                    [9, 8, 7, 6, 5]], np.int64)
    idx = (loc + base).astype(np.uint64)
    idx[1, 1] = np.uint64(base - 1)                 # below the base
    idx[1, 3] = np.uint64(base + 0xFFFFFFFF)        # local index 2^32 - 1: the "no candidate" pattern itself
    idx[2, 0] = np.uint64(base + (1 << 32) + 9)     # ... and beyond
    idx[2, 4] = np.uint64(base + 0xFFFFFFFE)        # the largest local index an entry can hold
    idx[0, 2] = INVALID                             # an empty slot of the local result
    bits = np.array([[R.PNAN | 0x12345, 0xFFFFFFFF, R.PINF, R.NZERO, 0x7FFFFFFF],
                     [R.NNAN | 0x00001, R.PINF, R.NINF, R.PNAN, 0x3F800000],
                     [R.PNAN, R.PZERO, 0x00000001, 0x80000001, 0xFF800001]], np.uint32)
    di, ds = _to_dev(dev, idx, bits)
    block = gpu_pack_block(ctx, di, ds, base, count, k)
    torch.cuda.synchronize()
    w = block.cpu().numpy().view(np.uint64)
    assert w.shape == (2 + nq * k,) and int(w[0]) == base and int(w[1]) == count
    e = w[2:].reshape(nq, k)
    want = np.full((nq, k), NO_CAND, np.uint64)
    want[:, :kin] = (bits.astype(np.uint64) << np.uint64(32)) | (idx - np.uint64(base))
    for j, r in ((1, 1), (1, 3), (2, 0), (0, 2)):
        want[j, r] = NO_CAND
    assert np.array_equal(e, want), (e, want)
    # kin = 0 (a shard without vectors): a header and k empty entries per query
    empty = gpu_pack_block(ctx, di[:, :0].contiguous(), ds[:, :0].contiguous(), 5, 0, k)
    torch.cuda.synchronize()
    w = empty.cpu().numpy().view(np.uint64)
    assert w[:2].tolist() == [5, 0] and np.all(w[2:] == NO_CAND)
