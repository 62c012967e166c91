"""GPU parity tests: DocumentCorpus.rerank / innr_maxsim_rerank[_dev] -- many queries, each scored exactly against ITS OWN
candidate documents. The oracle is oracle.maxsim per (query, candidate) pair, ordered by (score descending under total_cmp,
index ascending); every comparison is exact (bits_equal on scores, list equality on indices)."""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    from innr_amd import maxsim
    return maxsim


def _tokens(ndocs, T, dim, seed):
    rows = oracle.generate_uniform(ndocs * T, dim, seed)
    n = np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    return (rows / np.maximum(n, 1e-12)).astype(np.float32).reshape(ndocs, T, dim)


def _ord(x):
    """f32 -> u32 keys whose unsigned order is total_cmp's"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _rank(docs, scores, k):
    """(docs, scores) ordered by (score descending under total_cmp, index ascending), first k"""
    docs = np.asarray(docs, np.uint64)
    scores = np.asarray(scores, np.float32)
    order = np.lexsort((docs, -_ord(scores).astype(np.int64)))[:k]
    return docs[order], scores[order]


class PairOracle:
    """oracle.maxsim per (query, document) pair, each distinct pair scored once"""

    def __init__(self, queries, toks, lens=None, cosine=False):
        self.q, self.toks, self.lens, self.cos, self.memo = queries, toks, lens, cosine, {}

    def score(self, j, doc):
        key = (j, int(doc))
        if key not in self.memo:
            d = self.toks[doc] if self.lens is None else self.toks[doc][:self.lens[doc]]
            self.memo[key] = np.float32(oracle.maxsim(self.q[j], d, cosine=self.cos)) if len(d) and len(self.q[j]) else np.float32(0.0)
        return self.memo[key]

    def expect(self, j, cand_row, k, base=0):
        sc = np.array([self.score(j, int(c) - base) for c in cand_row], np.float32)
        return _rank(cand_row, sc, k)


def _check(dc, po, queries, cand, k, cosine, base=0, what=""):
    idx, sc = dc.rerank(queries, cand, k, cosine=cosine)
    kout = min(k, cand.shape[1])
    assert idx.shape == (len(queries), kout) and sc.shape == (len(queries), kout), what
    for j in range(len(queries)):
        ei, es = po.expect(j, cand[j], k, base)
        assert idx[j].tolist() == ei.tolist(), (what, j)
        print(f"{what} q={j}: max |score - oracle| = {np.max(np.abs(sc[j].astype(np.float64) - es.astype(np.float64)), initial=0.0)}")
        assert bits_equal(sc[j], es), (what, j)
    return idx, sc


def _cands(rng, Q, ndocs, kc):
    return np.stack([rng.permutation(ndocs)[:kc] for _ in range(Q)]).astype(np.uint64)


# a LIST of cases (not a cross product) that between them cover T in {1, 3, 16, 17, 64, 100}, dim in {8, 33, 96, 128},
# Tq in {1, 5, 32, 40, 70}, Q in {1, 7, 130}, kc in {1, 10, 256, 257, 1000}, k in {1, 10, kc, kc + 5}; the largest costs
# pairs*Tq*T*dim = 9e7 multiply-adds of the oracle, the file about 1e9
CASES = [  # ndocs, T, dim, Tq, Q, kc, k
    (5, 1, 8, 1, 1, 1, 1),
    (40, 3, 33, 5, 7, 10, 10),
    (300, 16, 96, 32, 7, 256, 256),
    (300, 17, 128, 40, 1, 257, 262),
    (1100, 64, 8, 70, 1, 1000, 10),
    (60, 100, 96, 5, 130, 10, 1),
    (64, 64, 128, 32, 7, 10, 15),
    (1200, 3, 8, 1, 130, 1000, 10),
]


@pytest.mark.parametrize("ndocs,T,dim,Tq,Q,kc,k", CASES)
def test_rerank_parity(M, ndocs, T, dim, Tq, Q, kc, k):
    rng = np.random.default_rng(ndocs * 31 + kc)
    toks = _tokens(ndocs, T, dim, 3)
    queries = list(_tokens(Q, Tq, dim, 99))
    cand = _cands(rng, Q, ndocs, kc)
    dc = M.DocumentCorpus.from_tokens(toks)
    for cosine in (False, True):
        _check(dc, PairOracle(queries, toks, None, cosine), queries, cand, k, cosine, what=f"plain cos={cosine}")
    # unnormalised tokens and queries, one zero-norm token (the cosine guards, dense.rs:341-345), per-document lengths with 0 and T
    toks2 = (toks * np.float32(3.5)).astype(np.float32)
    toks2[0, 0, :] = 0.0
    lens = np.array([(i * 7) % (T + 1) for i in range(ndocs)], dtype=np.uint32)
    lens[0] = T
    lens[ndocs - 1] = 0 if ndocs > 1 else T
    if ndocs > 2:
        lens[1] = T
    q2 = [(q * np.float32(0.25)).astype(np.float32) for q in queries]
    dc2 = M.DocumentCorpus.from_tokens(toks2, lens)
    cand2 = cand.copy()
    if kc >= 3 and ndocs > 2:  # documents 0 (zero-norm token), 1 (full length) and the empty last one are candidates of query 0
        rest = [c for c in cand[0].tolist() if c not in (0, 1, ndocs - 1)][:kc - 3]
        cand2[0] = np.array([0, 1, ndocs - 1] + rest, np.uint64)
    for cosine in (False, True):
        _check(dc2, PairOracle(q2, toks2, lens, cosine), q2, cand2, k, cosine, what=f"unnormalised+doc_len cos={cosine}")


def test_rerank_per_query_token_counts(M):
    ndocs, T, dim, kc, k = 50, 16, 32, 20, 7
    tq = [0, 1, 31, 32, 33, 70]
    toks = _tokens(ndocs, T, dim, 5)
    allq = _tokens(len(tq), 70, dim, 8)
    queries = [allq[j, :tq[j]] for j in range(len(tq))]
    cand = _cands(np.random.default_rng(1), len(tq), ndocs, kc)
    dc = M.DocumentCorpus.from_tokens(toks)
    for cosine in (False, True):
        idx, sc = _check(dc, PairOracle(queries, toks, None, cosine), queries, cand, k, cosine, what=f"tq cos={cosine}")
        for j in range(len(tq)):
            i1, s1 = dc.rerank([queries[j]], cand[j:j + 1], k, cosine=cosine)
            assert i1[0].tolist() == idx[j].tolist() and bits_equal(s1[0], sc[j]), (cosine, j)
        # the empty query: every score 0.0, candidates in index order
        assert idx[0].tolist() == sorted(cand[0].tolist())[:k] and np.all(sc[0].view(np.uint32) == 0)
    # the same through the C ABI with garbage in the unused token rows of the common stride
    from innr_amd._lib import check, load
    packed = np.full((len(tq), 70, dim), np.nan, np.float32)
    for j in range(len(tq)):
        packed[j, :tq[j]] = queries[j]
    tqa = np.array(tq, np.uint32)
    oi = np.empty((len(tq), k), np.uint64)
    os_ = np.empty((len(tq), k), np.float32)
    out_k = C.c_size_t(0)
    check(load().innr_maxsim_rerank(dc._h, 0, C.c_void_p(packed.ctypes.data), len(tq), C.c_void_p(tqa.ctypes.data), 70, dim,
                                    C.c_void_p(cand.ctypes.data), kc, k, C.c_void_p(oi.ctypes.data), C.c_void_p(os_.ctypes.data),
                                    C.byref(out_k)))
    i0, s0 = dc.rerank(queries, cand, k)
    assert out_k.value == k and oi.tolist() == i0.tolist() and bits_equal(os_, s0)


def test_rerank_agrees_with_scores_and_topk(M):
    import innr_amd
    ndocs, T, dim, Tq, Q = 500, 24, 64, 8, 4
    toks = _tokens(ndocs, T, dim, 12)
    toks[7] = toks[3]            # an exact tie: the lower index first
    toks[11, 2, 5] = np.nan      # a NaN token in the corpus
    queries = list(_tokens(Q, Tq, dim, 4))
    dc = M.DocumentCorpus.from_tokens(toks)
    rng = np.random.default_rng(2)
    others = np.array([c for c in range(ndocs) if c not in (7, 3, 11)], np.uint64)
    cand = np.stack([np.concatenate([np.array([7, 3, 11], np.uint64), rng.permutation(others)[:47]]) for _ in range(Q)])
    every = np.tile(np.arange(ndocs, dtype=np.uint64), (Q, 1))
    for cosine in (False, True):
        po = PairOracle(queries, toks, None, cosine)
        idx, sc = _check(dc, po, queries, cand, 50, cosine, what=f"vs scores cos={cosine}")
        for j in range(Q):
            full = dc.scores(queries[j], cosine=cosine)
            ei, es = _rank(cand[j], full[cand[j].astype(np.int64)], 50)
            assert idx[j].tolist() == ei.tolist() and bits_equal(sc[j], es), (cosine, j)
            assert idx[j].tolist().index(3) + 1 == idx[j].tolist().index(7), "tie: lower index first"
        for k in (10, ndocs):
            ia, sa = dc.rerank(queries, every, k, cosine=cosine)
            for j in range(Q):
                ti, ts = dc.topk(queries[j], k, cosine=cosine, engine=innr_amd.KNN_EXACT)
                assert ia[j].tolist() == ti.tolist() and bits_equal(sa[j], ts), (cosine, k, j)


def test_rerank_independent_lists(M):
    ndocs, T, dim, Tq, kc, k = 120, 16, 32, 5, 30, 12
    toks = _tokens(ndocs, T, dim, 6)
    queries = list(_tokens(4, Tq, dim, 7))
    dc = M.DocumentCorpus.from_tokens(toks)
    a = np.arange(0, 30, dtype=np.uint64)
    cand = np.stack([a, a + 15, a + 60, a + 90])  # 0/1 overlap, 2 and 3 disjoint from the others
    for cosine in (False, True):
        po = PairOracle(queries, toks, None, cosine)
        idx, sc = _check(dc, po, queries, cand, k, cosine, what=f"lists cos={cosine}")
        rng = np.random.default_rng(3)
        for variant in (cand[:, ::-1].copy(), np.stack([rng.permutation(r) for r in cand])):
            i2, s2 = dc.rerank(queries, variant, k, cosine=cosine)
            assert i2.tolist() == idx.tolist() and bits_equal(s2, sc)
        # a query's result does not depend on what the other queries bring
        i1, s1 = dc.rerank(queries[1:2], cand[1:2], k, cosine=cosine)
        assert i1[0].tolist() == idx[1].tolist() and bits_equal(s1[0], sc[1])


def test_rerank_index_base(M):
    base = 5_000_000_000
    ndocs, T, dim, Tq, kc, k = 80, 8, 16, 4, 25, 9
    toks = _tokens(ndocs, T, dim, 9)
    queries = list(_tokens(3, Tq, dim, 10))
    dc = M.DocumentCorpus.from_tokens(toks)
    dc.set_index_base(base)
    cand = _cands(np.random.default_rng(4), 3, ndocs, kc) + np.uint64(base)
    idx, sc = _check(dc, PairOracle(queries, toks), queries, cand, k, False, base=base, what="index base")
    assert idx.min() >= base


def test_rerank_device_entry_point(M):
    import torch
    ndocs, T, dim, Tq, Q, kc, k = 400, 32, 64, 40, 9, 300, 20
    toks = _tokens(ndocs, T, dim, 13)
    q = _tokens(Q, Tq, dim, 14)
    cand = _cands(np.random.default_rng(5), Q, ndocs, kc)
    dc = M.DocumentCorpus.from_tokens(toks)
    for cosine in (False, True):
        hi, hs = dc.rerank(q, cand, k, cosine=cosine)
        po = PairOracle(list(q), toks, None, cosine)
        for j in (0, Q - 1):
            ei, es = po.expect(j, cand[j], k)
            assert hi[j].tolist() == ei.tolist() and bits_equal(hs[j], es)
        di, ds = dc.rerank(torch.from_numpy(q).cuda(), torch.from_numpy(cand.astype(np.int64)).cuda(), k, cosine=cosine)
        assert di.is_cuda and ds.is_cuda and di.dtype == torch.int64 and ds.dtype == torch.float32
        assert di.cpu().numpy().tolist() == hi.astype(np.int64).tolist() and bits_equal(ds.cpu().numpy(), hs)


def _raw(dc, q, Q, stride, dim, cand, kc, k, tq=None, null_cand=False):
    from innr_amd._lib import load
    q = np.ascontiguousarray(q, np.float32)
    cand = np.ascontiguousarray(cand, np.uint64)
    n = max(Q * max(min(k, kc), 1), 1)
    oi, os_ = np.zeros(n, np.uint64), np.zeros(n, np.float32)
    out_k = C.c_size_t(12345)
    st = load().innr_maxsim_rerank(dc._h, 0, C.c_void_p(q.ctypes.data) if q.size else None, Q,
                                   C.c_void_p(tq.ctypes.data) if tq is not None else None, stride, dim,
                                   None if null_cand or not cand.size else C.c_void_p(cand.ctypes.data), kc, k,
                                   C.c_void_p(oi.ctypes.data), C.c_void_p(os_.ctypes.data), C.byref(out_k))
    return st, int(out_k.value), oi, os_


def test_rerank_errors(M):
    from innr_amd import InnrPanic
    from innr_amd import _lib
    ndocs, T, dim, Tq, kc = 30, 8, 16, 4, 5
    base = 1000
    toks = _tokens(ndocs, T, dim, 15)
    q = _tokens(2, Tq, dim, 16)
    dc = M.DocumentCorpus.from_tokens(toks)
    dc.set_index_base(base)
    good = (_cands(np.random.default_rng(6), 2, ndocs, kc) + np.uint64(base)).astype(np.uint64)
    # the dimension check comes before everything else: bad candidates, k == 0, a null candidate pointer
    bad_dim = np.ones((2, Tq, dim + 1), np.float32)
    for kw in (dict(kc=kc, k=3), dict(kc=kc, k=0), dict(kc=0, k=3), dict(kc=kc, k=3, null_cand=True)):
        st, ok, _, _ = _raw(dc, bad_dim, 2, Tq, dim + 1, good - np.uint64(base), **kw)
        assert st == _lib.E_DIM_MISMATCH and "dimension mismatch" in _lib.last_error(), kw
    with pytest.raises(InnrPanic):
        dc.rerank(bad_dim, good, 3)
    # a candidate below the base / at base + ndocs: E_BAD_ARG naming the range; the next valid call succeeds
    for wrong in (base - 1, base + ndocs):
        c2 = good.copy()
        c2[1, 2] = wrong
        st, ok, _, _ = _raw(dc, q, 2, Tq, dim, c2, kc, 3)
        assert st == _lib.E_BAD_ARG and f"[{base}, {base + ndocs})" in _lib.last_error(), (wrong, _lib.last_error())
        with pytest.raises(_lib.InnrError):
            dc.rerank(q, c2, 3)
        _check(dc, PairOracle(list(q), toks), list(q), good, 3, False, base=base, what="after a bad candidate")
    # nothing to do: out_k == 0 and INNR_OK
    for kw in (dict(Q=2, kc=kc, k=0), dict(Q=2, kc=0, k=3), dict(Q=0, kc=kc, k=3)):
        st, ok, _, _ = _raw(dc, q, kw["Q"], Tq, dim, good, kw["kc"], kw["k"])
        assert st == _lib.OK and ok == 0, kw
    empty = M.DocumentCorpus.from_tokens(np.empty((0, T, dim), np.float32))
    st, ok, _, _ = _raw(empty, q, 2, Tq, dim, good, kc, 3)
    assert st == _lib.OK and ok == 0
    # more slots than the kernels' 32-bit indices reach: refused before anything is read or allocated
    st, ok, _, _ = _raw(dc, q, 70_000, Tq, dim, good, 70_000, 1)
    assert st == _lib.E_UNSUPPORTED and "beyond one launch" in _lib.last_error() and ok == 0
    # a null candidate pointer with work to do
    st, ok, _, _ = _raw(dc, q, 2, Tq, dim, good, kc, 3, null_cand=True)
    assert st == _lib.E_BAD_ARG


def test_rerank_mid_size_against_full_scan(M):
    ndocs, T, dim, Q, Tq, kc, k = 200_000, 64, 128, 256, 32, 100, 10
    dc = M.DocumentCorpus.generate(ndocs, T, dim, seed=0)
    q = _tokens(Q, Tq, dim, 77)
    rng = np.random.default_rng(8)
    cand = np.stack([rng.choice(ndocs, size=kc, replace=False) for _ in range(Q)]).astype(np.uint64)
    for cosine in (False, True):
        idx, sc = dc.rerank(q, cand, k, cosine=cosine)
        assert idx.shape == (Q, k)
        for j in rng.choice(Q, size=8, replace=False):
            full = dc.scores(q[j], cosine=cosine)
            ei, es = _rank(cand[j], full[cand[j].astype(np.int64)], k)
            assert idx[j].tolist() == ei.tolist() and bits_equal(sc[j], es), (cosine, int(j))


def test_maxsim_rerank_example_runs(capsys):
    spec = importlib.util.spec_from_file_location("maxsim_rerank", os.path.join(ROOT, "examples", "maxsim_rerank.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    recall = m.main(n_docs=400, n_doc_tokens=16, n_query_tokens=8, dim=32, n_queries=6, kc=400, k=10)
    assert recall == 1.0 and "recall@10 = 1.000" in capsys.readouterr().out
