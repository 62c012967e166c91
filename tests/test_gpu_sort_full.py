"""GPU tests of the full sort and selection (innr_amd/csrc/sort_full.hip, select_dev.h) past two LDS sort windows.

kSelSlots = 4096 keys fit one window. At npad = 8192 the only stage above the window is the last one, which is descending
everywhere; from npad = 16384 on the global network has ascending halves, from 32768 on global steps at j >= 2 * kSelSlots, and
from n > 2^20 the select kernels' grid-stride loops read more than one key per thread.

1. key level, through the hooks innrdbg_full_topk_keys / innrdbg_segmented_topk_keys of the test-hooks library: caller-given
   64-bit keys against np.sort(keys)[::-1][:k], compared for equality -- exact when keys repeat too, because the output is sorted
   (phase 0 + phase 1 of the gather must deliver exactly the top-k multiset);
2. one case per call site at k past 8192, against the CPU oracle's scores ranked by tests/order_ref.topk_ref, bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import order_ref as R
from adaptive_ref import adaptive_ref
from test_gpu_exact import bits_equal
from test_gpu_maxsim_rerank import PairOracle, _check as _check_maxsim_rerank
from test_gpu_order_semantics import _all_scores, _check_rerank

WINDOW = 4096          # kSelSlots
GRID_KEYS = 1 << 20    # 4096 blocks of 256 threads: beyond, a thread of the select kernels reads a second key
U64 = np.uint64


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


@pytest.fixture(scope="module")
def M():
    from innr_amd import maxsim
    return maxsim


@pytest.fixture(scope="module")
def torch_device_up():
    """torch's import and its first touch of the device happen here, not inside the first case that hands over device tensors"""
    import torch
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()


# =====================================================================================================================
# 1. key level
# =====================================================================================================================
def _call_hook(name, argtypes, *args):
    """a hook of the test-hooks library on the default context. The product library is loaded FIRST: its loader maps the one HIP
    runtime both libraries have to share (innr_amd/_lib.py); the hook library on its own would bring a second one, in which the
    context's stream and buffers mean nothing."""
    from conftest import hooks_lib
    from innr_amd import _lib
    ctx = _lib.default_context().handle
    L = hooks_lib()
    fn = getattr(L, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + argtypes
    status = fn(ctx, *args)
    if status != _lib.OK:  # the message is the hook library's own (a thread-local of its copy of the sources)
        L.innr_last_error.restype = C.c_char_p
        raise _lib.InnrError(status, L.innr_last_error().decode("utf-8", "replace"))


def full_topk(keys, k):
    """full_topk_keys on the device: the best min(k, n) of keys[0..n), largest first"""
    keys = np.ascontiguousarray(keys, U64)
    out = np.full(min(k, keys.size), 0xDEADDEADDEADDEAD, U64)
    _call_hook("innrdbg_full_topk_keys", [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p], keys.ctypes.data, keys.size, k,
               out.ctypes.data)
    return out


def segmented_topk(keys, k):
    """segmented_topk_keys on the device: keys [nseg, len] -> the best min(k, len) of every segment, largest first"""
    keys = np.ascontiguousarray(keys, U64)
    nseg, ln = keys.shape
    out = np.full((nseg, min(k, ln)), 0xDEADDEADDEADDEAD, U64)
    _call_hook("innrdbg_segmented_topk_keys", [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p], keys.ctypes.data,
               nseg, ln, k, out.ctypes.data)
    return out


def _ref(keys, k):
    return np.sort(np.asarray(keys, U64))[::-1][:k]


def _rand(rng, n, lo=1, hi=None):
    """n random keys in [lo, hi) (hi: 2^64), none of them 0 ("not a candidate")"""
    if hi is None:
        return rng.integers(lo, 0xFFFFFFFFFFFFFFFF, size=n, dtype=U64, endpoint=True)
    return rng.integers(lo, hi, size=n, dtype=U64)


def _kth(keys, k):
    return int(np.sort(keys)[::-1][min(k, keys.size) - 1])


def make_keys(pattern, n, k, seed):
    """the key patterns of this file; every one has at least min(k, n) non-zero keys (the callers' contract)"""
    rng = np.random.default_rng(seed)
    k = min(k, n)
    if pattern == "random":       # (a) distinct random 64-bit keys
        keys = _rand(rng, n)
        assert np.unique(keys).size == n
    elif pattern == "sorted_desc":  # (b)
        keys = np.sort(_rand(rng, n))[::-1].copy()
    elif pattern == "sorted_asc":
        keys = np.sort(_rand(rng, n))
    elif pattern == "one_score":  # (c) composites of one score: equal top 32 bits, ~index below
        keys = (U64(0x3F800000) << U64(32)) | (~np.arange(n, dtype=np.uint32)).astype(U64)
    elif pattern == "low_byte":   # (d) only the lowest byte differs, plus a few far larger keys: the last radix pass decides
        keys = U64(0x3F80000012345600) | rng.integers(0, 256, size=n, dtype=U64)
        nbig = min(5, n // 2)
        keys[rng.choice(n, size=nbig, replace=False)] = _rand(rng, nbig, lo=0xF000000000000000)
        assert k <= nbig or _kth(keys, k) >> 8 == 0x3F800000123456
    elif pattern == "kth_top_byte_00":  # (e) fewer than k keys above bin 0 of the first pass
        keys = _rand(rng, n, hi=1 << 56)
        nhi = (k - 1) // 2
        keys[rng.choice(n, size=nhi, replace=False)] = _rand(rng, nhi, lo=1 << 56)
        assert _kth(keys, k) >> 56 == 0x00
    elif pattern == "kth_top_byte_ff":  # (f) k or more keys in bin 255 of the first pass
        keys = _rand(rng, n, hi=0xFF << 56)
        nff = k + (n - k) // 2
        keys[rng.choice(n, size=nff, replace=False)] = U64(0xFF << 56) | _rand(rng, nff, hi=1 << 56)
        assert _kth(keys, k) >> 56 == 0xFF
    elif pattern in ("zeros_exactly_k_real", "zeros_interleaved"):  # (g) masked vectors between the real keys
        keys = _rand(rng, n)
        nzero = n - k if pattern == "zeros_exactly_k_real" else (n - k) // 2
        keys[rng.choice(n, size=nzero, replace=False)] = 0
        assert np.count_nonzero(keys) >= k
    elif pattern == "repeats":    # (h) repeated keys; a run of equal keys straddles rank k
        v = np.sort(_rand(rng, n))[::-1].copy()
        v[1::3] = v[0::3][:v[1::3].size]          # pairs of equal keys all along
        lo, hi = max(k - 4, 0), min(k + 3, n)
        v[lo:hi] = v[lo]                          # ranks k-3 .. k+3 hold one key
        assert v[k - 1] == v[lo] and (k == n or v[k] == v[lo]) and np.all(v[:-1] >= v[1:])
        keys = rng.permutation(v)
    else:
        raise AssertionError(pattern)
    return np.ascontiguousarray(keys, U64)


PATTERNS = ["random", "sorted_desc", "sorted_asc", "one_score", "low_byte", "kth_top_byte_00", "kth_top_byte_ff",
            "zeros_exactly_k_real", "zeros_interleaved", "repeats"]

# npad: 4097 -> 8192 (one global stage, descending everywhere); 8193 -> 16384 (the first ascending merge windows -- which at
# k = 8193 hold one key and padding: a merge kernel that sorts them the wrong way round still ends sorted, measured by mutation;
# 12345 and 16384 fill them); 16385 -> 32768 (the first global step at j = 2 * kSelSlots); 40000, 65536 -> 65536; 70000 (below)
# -> 2^17; 131073 -> 2^18 (six global stages)
KS = [1, 2, 4095, 4096, 4097, 8192, 8193, 12345, 16384, 16385, 40000, 65536, 131073]
BIG_N = GRID_KEYS + 4097  # the grid-stride loops of select_hist_kernel / select_gather_kernel take a second trip


@pytest.mark.parametrize("k", KS)
def test_full_topk_sizes(k):
    for n in (k, k + 1, 2 * k + 3):
        keys = make_keys("random", n, k, seed=k * 7 + n)
        got = full_topk(keys, k)
        assert np.array_equal(got, _ref(keys, k)), (k, n)


@pytest.mark.parametrize("k", [300, 5000, 70000])
def test_full_topk_beyond_one_key_per_thread(k):
    keys = make_keys("random", BIG_N, k, seed=k)
    assert np.array_equal(full_topk(keys, k), _ref(keys, k))


def test_full_topk_k_beyond_n_clamps():
    keys = make_keys("random", 9001, 9001, seed=3)
    assert np.array_equal(full_topk(keys, 10**9), _ref(keys, 9001))


PATTERN_SIZES = [(4097, 8197), (8193, 8193), (8193, 16389), (12345, 12346), (16385, 16386), (16385, 32773), (5000, BIG_N)]  # (k, n)


@pytest.mark.parametrize("k,n", PATTERN_SIZES)
@pytest.mark.parametrize("pattern", PATTERNS[1:])
def test_full_topk_patterns(pattern, k, n):
    keys = make_keys(pattern, n, k, seed=n + len(pattern))
    got = full_topk(keys, k)
    assert np.array_equal(got, _ref(keys, k)), (pattern, k, n)


# (9000, 100), (9000, 4096), (70000, 10): the workgroup radix select of wg_segment_topk; (4097, *): its smallest segment;
# (9000, 4097), (9000, 9000): the branch beyond the window, one full_topk_keys per segment (segment bases 9000, 18000: no
# multiple of the window)
SEGMENT_SIZES = [(4097, 1), (4097, 4096), (9000, 100), (9000, 4096), (9000, 4097), (9000, 9000), (70000, 10)]  # (len, k)
SEGMENT_PATTERNS = ["random", "one_score", "low_byte"]


def _check_segments(keys, k):
    got = segmented_topk(keys, k)
    for s in range(keys.shape[0]):
        assert np.array_equal(got[s], _ref(keys[s], k)), (s, keys.shape, k)


@pytest.mark.parametrize("ln,k", SEGMENT_SIZES)
@pytest.mark.parametrize("pattern", SEGMENT_PATTERNS)
def test_segmented_topk_one_segment(pattern, ln, k):
    _check_segments(make_keys(pattern, ln, k, seed=ln + k).reshape(1, ln), k)


@pytest.mark.parametrize("ln,k", SEGMENT_SIZES)
@pytest.mark.parametrize("first", [0, 1, 2])
def test_segmented_topk_three_segments(first, ln, k):
    """every segment its own pattern: a wrong segment base cannot go unnoticed"""
    pats = [SEGMENT_PATTERNS[(first + s) % 3] for s in range(3)]
    keys = np.stack([make_keys(p, ln, k, seed=ln + k + 11 * s) for s, p in enumerate(pats)])
    _check_segments(keys, k)


# =====================================================================================================================
# 2. the callers, end to end
# =====================================================================================================================
N, D, NQ = 20011, 6, 2
VARIANTS = ["uniform", "patterns300"]
METRICS = ["dot", "cos", "l2"]
K_PAST = [8193, 16385, N, N + 5]


def _met(innr, metric):
    return {"dot": innr.METRIC_DOT, "cos": innr.METRIC_COSINE, "l2": innr.METRIC_L2SQ}[metric]


def _rows(variant, n, dim, seed):
    """uniform rows; or rows drawn from 300 patterns: long runs of equal scores cross the window boundaries, index order decides"""
    if variant == "uniform":
        return oracle.generate_uniform(n, dim, seed)
    pat = oracle.generate_uniform(300, dim, seed + 1)
    return np.ascontiguousarray(pat[np.random.default_rng(seed).integers(0, 300, size=n)])


class Corpus:
    """the shared N x D corpus of one variant on the device, with the oracle's score of every (metric, query, row), made once"""

    def __init__(self, B, variant):
        self.rows = _rows(variant, N, D, 61)
        self.data = oracle.from_rows(self.rows)
        self.qs = oracle.generate_uniform(NQ, D, 62)
        self.vb = B.VerticalBatch.from_rows(self.rows)
        self.sb = {m: _all_scores(m, self.qs, self.data) for m in METRICS}
        for a in self.sb.values():
            a.setflags(write=False)
        rng = np.random.default_rng(63)
        self.mask = np.zeros(N, np.uint8)
        self.mask[rng.choice(N, size=17000, replace=False)] = 1
        self.sel = np.flatnonzero(self.mask)
        self._u8 = None

    def u8(self, S):
        """codes of the same rows on the device, and the oracle's asymmetric score of every (query, row)"""
        if self._u8 is None:
            p = oracle.qparams_fit(self.rows)
            codes = oracle.quantize_u8(self.rows, p)
            qc = S.QuantizedCorpus.from_codes(codes, N, D, S.QuantizationParams(p.alpha, p.offset))
            sb = np.empty((NQ, N), np.uint32)
            for j, q in enumerate(self.qs):
                oi, os_ = oracle.batch_knn_u8(q, codes, p, N)  # every row, scored
                sb[j, oi.astype(np.int64)] = R.bits(os_)
            self._u8 = (qc, sb)
        return self._u8

    def close(self):
        self.vb.close()
        if self._u8 is not None:
            self._u8[0].close()


@pytest.fixture(scope="module")
def corpora(B):
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = Corpus(B, variant)
        return made[variant]

    yield get
    for c in made.values():
        c.close()


def _same(idx, sc, want_idx, want_bits, what):
    idx = np.asarray(idx)
    assert idx.shape == want_idx.shape, (what, idx.shape, want_idx.shape)
    assert np.array_equal(idx.astype(U64), want_idx), what
    assert np.array_equal(R.bits(sc), want_bits), what


def _knn_dev(vb, met, qs, k, engine):
    """innr_batch_knn_dev: queries and results in device memory"""
    import torch
    from innr_amd.dist import _gpu_local_search
    q = torch.from_numpy(np.ascontiguousarray(qs, np.float32)).to(torch.device("cuda", 0))
    idx, sc = _gpu_local_search(vb, met, engine)(q, k)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(U64), sc.cpu().numpy()


# ---- (a) innr_batch_knn, host and _dev ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K_PAST)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_knn_past_two_windows(B, innr, corpora, torch_device_up, variant, metric, k):
    c = corpora(variant)
    met = _met(innr, metric)
    hi, hs = B.knn_multi(met, c.qs, c.vb, k, innr.KNN_AUTO)
    di, ds = _knn_dev(c.vb, met, c.qs, k, innr.KNN_AUTO)
    for j in range(NQ):
        wi, wb = R.topk_ref(c.sb[metric][j], np.arange(N), metric == "l2", k)
        assert wi.size == min(k, N)
        _same(hi[j], hs[j], wi, wb, ("host", variant, metric, k, j))
        _same(di[j], ds[j], wi, wb, ("dev", variant, metric, k, j))


@pytest.mark.parametrize("metric", METRICS)
def test_knn_past_two_windows_index_base_near_2_40(B, innr, corpora, torch_device_up, metric):
    c = corpora("patterns300")
    base, k = (1 << 40) - 9, 16385
    c.vb.set_index_base(base)
    try:
        hi, hs = B.knn_multi(_met(innr, metric), c.qs, c.vb, k, innr.KNN_AUTO)
        di, ds = _knn_dev(c.vb, _met(innr, metric), c.qs, k, innr.KNN_AUTO)
    finally:
        c.vb.set_index_base(0)
    for j in range(NQ):
        wi, wb = R.topk_ref(c.sb[metric][j], np.arange(N), metric == "l2", k)
        assert int(wi.max()) + base > 1 << 40 > int(wi.min()) + base
        _same(hi[j], hs[j], wi + U64(base), wb, ("host", metric, j))
        _same(di[j], ds[j], wi + U64(base), wb, ("dev", metric, j))


# ---- (b) QuantizedCorpus.knn_multi --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_knn_u8_past_two_windows(S, corpora, variant):
    c = corpora(variant)
    qc, sb = c.u8(S)
    idx, sc = qc.knn_multi(c.qs, 16385)
    for j in range(NQ):
        wi, wb = R.topk_ref(sb[j], np.arange(N), False, 16385)
        _same(idx[j], sc[j], wi, wb, (variant, j))


# ---- (c) the masked sort: innr_batch_knn_filtered_multi, innr_batch_knn_u8_filtered ----------------------------------------------
@pytest.mark.parametrize("k", [16385, 10**6])  # k' = 16385; k' = the 17000 that pass
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_filtered_multi_past_two_windows(B, innr, corpora, variant, metric, k):
    c = corpora(variant)
    idx, sc = B.batch_knn_filtered_multi(c.qs, c.vb, k, c.mask, metric=_met(innr, metric))
    assert idx.shape == (NQ, min(k, 17000))
    for j in range(NQ):
        wi, wb = R.topk_ref(c.sb[metric][j][c.sel], c.sel, metric == "l2", k)
        _same(idx[j], sc[j], wi, wb, (variant, metric, k, j))


@pytest.mark.parametrize("k", [16385, 10**6])
@pytest.mark.parametrize("variant", VARIANTS)
def test_u8_filtered_past_two_windows(S, corpora, variant, k):
    c = corpora(variant)
    qc, sb = c.u8(S)
    idx, sc = qc.knn_filtered_multi(c.qs, k, c.mask)
    assert idx.shape == (NQ, min(k, 17000))
    for j in range(NQ):
        wi, wb = R.topk_ref(sb[j][c.sel], c.sel, False, k)
        _same(idx[j], sc[j], wi, wb, (variant, k, j))


# ---- (d) the one-query entry points: innr_batch_knn_filtered, innr_batch_knn_reordered ------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_query_filtered_and_reordered_past_two_windows(B, corpora, variant):
    c = corpora(variant)
    k = 16385
    for j, q in enumerate(c.qs):
        r = B.batch_knn_filtered(q, c.vb, k, lambda i: bool(c.mask[i]))
        wi, wb = R.topk_ref(c.sb["l2"][j][c.sel], c.sel, True, k)
        _same(r.indices, np.float32(r.scores), wi, wb, ("filtered", variant, j))
        # reordered: the distances are summed in decreasing-variance dimension order -- the oracle's own scores of every row
        oi, os_ = oracle.batch_knn_reordered(q, c.data, N)
        sb = np.empty(N, np.uint32)
        sb[oi.astype(np.int64)] = R.bits(os_)
        r = B.batch_knn_reordered(q, c.vb, k)
        wi, wb = R.topk_ref(sb, np.arange(N), True, k)
        _same(r.indices, np.float32(r.scores), wi, wb, ("reordered", variant, j))


# ---- (e) innr_batch_rerank, host and _dev --------------------------------------------------------------------------------
RN, RQ, RKC = 12000, 3, 9000


@pytest.fixture(scope="module")
def rerank_corpora(B):
    made = {}

    def get(variant):
        if variant not in made:
            rows = _rows(variant, RN, D, 71)
            data = oracle.from_rows(rows)
            qs = oracle.generate_uniform(RQ, D, 72)
            rng = np.random.default_rng(73)
            cand = np.stack([rng.choice(RN, size=RKC, replace=False) for _ in range(RQ)]).astype(U64)
            made[variant] = (B.VerticalBatch.from_rows(rows), qs, {m: _all_scores(m, qs, data) for m in METRICS}, cand)
        return made[variant]

    yield get
    for vb, *_ in made.values():
        vb.close()


# k = 100, 4096: the workgroup radix select over kc = 9000 keys; 4097, 9000: three segments through full_topk_keys
@pytest.mark.parametrize("k", [100, 4096, 4097, 9000])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_rerank_more_candidates_than_the_window(B, innr, rerank_corpora, torch_device_up, variant, metric, k):
    vb, qs, sb, cand = rerank_corpora(variant)
    _check_rerank(B, innr, vb, metric, qs, sb[metric], cand, k, what=f"{variant} k={k}")


# ---- (f), (g) innr_maxsim_topk, innr_maxsim_rerank -------------------------------------------------------------------------
NDOCS, T, TDIM, TQ = 20011, 2, 8, 3


class Docs:
    def __init__(self, M, variant):
        self.toks = _rows(variant, NDOCS, T * TDIM, 81).reshape(NDOCS, T, TDIM)
        self.queries = list(oracle.generate_uniform(2 * TQ, TDIM, 82).reshape(2, TQ, TDIM))
        self.dc = M.DocumentCorpus.from_tokens(self.toks)
        self.po = {cos: PairOracle(self.queries, self.toks, None, cos) for cos in (False, True)}  # each pair scored once
        rng = np.random.default_rng(83)
        self.cand = np.stack([rng.permutation(NDOCS)[:9000] for _ in range(2)]).astype(U64)


@pytest.fixture(scope="module")
def docs(M):
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = Docs(M, variant)
        return made[variant]

    yield get
    for d in made.values():
        d.dc.close()


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_maxsim_topk_ranks_every_document(docs, variant, cosine):
    d = docs(variant)
    idx, sc = d.dc.topk(d.queries[0], NDOCS, cosine=cosine)
    ei, es = d.po[cosine].expect(0, np.arange(NDOCS, dtype=U64), NDOCS)
    assert idx.tolist() == ei.tolist() and bits_equal(sc, es), (variant, cosine)


@pytest.mark.parametrize("kc,k", [(9000, 10), (9000, 9000), (5000, 5000)])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_maxsim_rerank_more_candidates_than_the_window(docs, variant, cosine, kc, k):
    d = docs(variant)
    cand = np.ascontiguousarray(d.cand[:, :kc])
    _check_maxsim_rerank(d.dc, d.po[cosine], d.queries, cand, k, cosine, what=f"{variant} kc={kc} k={k} cos={cosine}")


# ---- (h) innr_batch_knn on more keys than the select kernels have threads -------------------------------------------------------
@pytest.fixture(scope="module")
def wide(B):
    rows = oracle.generate_uniform(BIG_N, 2, 91)
    q = oracle.generate_uniform(1, 2, 92)
    sb = R.bits(oracle.batch_dot(q[0], oracle.from_rows(rows)))
    want = R.topk_ref(sb, np.arange(BIG_N), False, 5000)
    vb = B.VerticalBatch.from_flat(rows.reshape(-1), BIG_N, 2)
    yield vb, q, want
    vb.close()


@pytest.mark.parametrize("k", [300, 5000])
def test_knn_dot_beyond_one_key_per_thread(B, wide, k):
    vb, q, (wi, wb) = wide
    idx, sc = B.batch_knn_dot_multi(q, vb, k)
    _same(idx[0], sc[0], wi[:k], wb[:k], k)


# ---- (i) innr_batch_knn_adaptive ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_adaptive_past_two_windows(B, corpora, variant):
    c = corpora(variant)
    k, w = 8193, 2
    idx, sc = B.batch_knn_adaptive_multi(c.qs, c.vb, k, w)
    assert idx.shape == (NQ, k)
    for j, q in enumerate(c.qs):
        wi, ws, _ = adaptive_ref(q, c.data, k, w)
        _same(idx[j], sc[j], wi, R.bits(ws), (variant, j))
