"""GPU tests of the maxsim engines where a wave walks SEVERAL documents and ONE (token slot, query token) pair decides the answer.

The launch geometry caps the MFMA engine's grid at 8 blocks of 4 waves per CU and the exact scan's and the re-rank's at 2: a wave takes
a second document only past 32 CUs (8 CUs x 64/Tp) documents. The corpora here are just past two such strides, built by
tests/maxsim_plant_ref.py: a quiet background, and P planted documents per query that each owe their place in the top-k to one query
token in one token slot -- in document 0, in every stride, in the ragged last one, behind empty / 1 / 32 / 33 / T-token predecessors
on the same wave, in front of an empty successor, in the last valid slot of a short document. A tile kernel that requests the wrong
next tile, takes the next document's length from the current one, masks a valid row or drops a query token loses a planted document,
and the hosts rank far below the candidate cut without their plant, so the exact re-score cannot bring it back. (Each of those four
was tried as a one-line change of the kernels, which touches no address: every case of the kernel concerned fails.)

Everything goes through DocumentCorpus.scores / topk / topk_multi / rerank; the launch record says which instantiation served."""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
import maxsim_plant_ref as R
from test_gpu_exact import bits_equal
from test_gpu_kernel_variants import logged
from test_gpu_maxsim import _oracle_scores
from test_gpu_maxsim_rerank import PairOracle, _check as _check_rerank

P = K = 40


@pytest.fixture(scope="module")
def M():
    from innr_amd import maxsim
    return maxsim


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@functools.lru_cache(maxsize=1)
def _cus():
    import torch
    from innr_amd import _lib
    return torch.cuda.get_device_properties(_lib.default_context().device).multi_processor_count


def _mfma_geometry(dim):
    """(waves of the MFMA engine's grid = documents per stride, a corpus size past it with every index class)"""
    nwaves = 32 * _cus()
    return nwaves, (2 * nwaves + 5 if dim < 128 else nwaves + nwaves // 2 + 5)


def _pass_insts(family, cosine, tq, *args):
    return [(family, int(cosine)) + args] * ((tq + 31) // 32)


def _check_planted(innr, dc, queries, tokens, lens, pl, cosine, engine, want_launches, multi):
    st = innr.KnnStats()
    if multi:
        (idx, sc), log = logged(lambda: dc.topk_multi(queries, K, cosine=cosine, engine=engine, stats=st))
    else:
        (idx, sc), log = logged(lambda: dc.topk(queries[0], K, cosine=cosine, engine=engine, stats=st))
        idx, sc = idx[None], sc[None]
    print(f"cos={cosine}: min gap {[round(g, 3) for g in pl.min_gap]}, worst unplanted rank {pl.worst_rank}, without the query token {pl.blind_rank}; "
          f"{[e.inst for e in log if e.family in ('ms_tile', 'ms_generic')]} on {len(tokens)} documents, {32 * _cus()} waves; "
          f"engine {st.engine} fallback {st.queries_fallback}")
    for qi, q in enumerate(queries):
        docs, want = R.expected_topk(q, tokens, lens, pl.docs[qi], cosine)
        assert idx[qi].tolist() == docs.tolist(), (cosine, qi, sorted(set(docs.tolist()) - set(idx[qi].tolist())))
        assert bits_equal(sc[qi], want), (cosine, qi)
    # the gap is hundreds of times the engine's error bound: a fallback to the exact engine is a finding, not an outcome
    assert st.engine == innr.KNN_MFMA and st.queries_fallback == 0, (cosine, st.engine, st.queries_fallback)
    got = [e.inst for e in log if e.family in ("ms_tile", "ms_generic")]
    assert got == want_launches, (cosine, log)
    if want_launches[0][0] == "ms_tile":
        assert all(e.groups == len(queries) for e in log if e.family == "ms_tile"), log


MFMA_CASES = [  # T, dim, tqs, generic option, seed (maxsim_plant_ref.build asserts its conditions: the seed is one for which they hold)
    (40, 32, [12], 0, 1), (33, 64, [32], 0, 1), (40, 96, [32], 0, 1), (40, 128, [32], 0, 1),  # one query, tile kernel, NB = 1..4
    (40, 128, [40], 0, 1), (40, 128, [64], 0, 1),                                             # two passes on NQ = 1
    (40, 128, [16, 5, 12, 1], 0, 1), (40, 64, [16, 9], 0, 1), (33, 32, [8, 3, 4, 1], 0, 1),   # groups of 4 / 2 queries; NB = 1 with NQ = 4
    (40, 48, [24], 0, 1), (70, 256, [70], 0, 1),                                              # generic kernel; three passes
    (40, 128, [32], 1, 1),                                                                    # generic kernel by option
]


@pytest.mark.parametrize("T,dim,tqs,generic,seed", MFMA_CASES)
def test_mfma_engine_planted_winners(M, innr, ctx_option, T, dim, tqs, generic, seed):
    if generic:
        ctx_option("maxsim_generic", 1)
    nwaves, ndocs = _mfma_geometry(dim)
    assert ndocs > nwaves + 4  # more than one document per wave, a ragged last stride
    tiled = dim % 32 == 0 and dim <= 128 and not generic
    for cosine in (False, True):
        queries, tokens, lens, pl = R.build(ndocs, T, dim, tqs, P, nwaves, cosine, seed)
        dc = M.DocumentCorpus.from_tokens(tokens, lens)
        try:
            want = _pass_insts("ms_tile", cosine, max(tqs), dim // 32, len(tqs)) if tiled else _pass_insts("ms_generic", cosine, max(tqs))
            _check_planted(innr, dc, queries, tokens, lens, pl, cosine, innr.KNN_MFMA, want, multi=len(tqs) > 1)
        finally:
            dc.close()


def test_auto_engine_planted_winners(M, innr):
    """KNN_AUTO on a corpus of 4096 documents or more resolves to the MFMA engine: the same answer, the same kernel"""
    T, dim, tqs, seed = 40, 64, [12], 1
    nwaves, ndocs = _mfma_geometry(dim)
    assert ndocs >= 4096
    for cosine in (False, True):
        queries, tokens, lens, pl = R.build(ndocs, T, dim, tqs, P, nwaves, cosine, seed)
        dc = M.DocumentCorpus.from_tokens(tokens, lens)
        try:
            _check_planted(innr, dc, queries, tokens, lens, pl, cosine, innr.KNN_AUTO, _pass_insts("ms_tile", cosine, 12, 2, 1), multi=False)
        finally:
            dc.close()


@pytest.mark.parametrize("T,dim,Tq,seed", [(16, 32, 12, 1), (40, 32, 12, 1), (33, 64, 32, 1), (129, 32, 5, 1)])
def test_exact_scan_every_document_past_one_stride(M, T, dim, Tq, seed):
    """maxsim_scan_kernel: 2 blocks per CU, 64/Tp documents per wave -- three strides and a ragged fourth, every score against the oracle"""
    Tp = 1
    while Tp < T and Tp < 64:
        Tp <<= 1
    stride = 8 * _cus() * (64 // Tp)  # documents per stride of the scan's grid
    ndocs = 3 * stride + 5
    for cosine in (False, True):
        queries, tokens, lens, pl = R.build(ndocs, T, dim, [Tq], P, stride, cosine, seed)
        dc = M.DocumentCorpus.from_tokens(tokens, lens)
        try:
            got, log = logged(lambda: dc.scores(queries[0], cosine=cosine))
            want = _oracle_scores(queries[0], tokens, lens, cosine=cosine)
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (cosine, bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist(), lens[bad[:10]].tolist())
            nq = 8 if Tq <= 8 else (16 if Tq <= 16 else 32)
            assert [e.inst for e in log if e.family == "ms_scan"] == [("ms_scan", int(cosine), nq, int(T > 64))], log
            # ... and the planted documents are the best P of them, in the oracle's stable order
            docs, sc = R.expected_topk(queries[0], tokens, lens, pl.docs[0], cosine)
            assert np.argsort(-want.astype(np.float64), kind="stable")[:P].tolist() == docs.tolist()
        finally:
            dc.close()


def test_rerank_past_one_stride(M):
    """maxsim_rerank_kernel: Q kc = 3500 units of one candidate each on a grid of 8 waves per CU; every query's planted documents among
    its candidates, query lengths from 0 to 14 tokens, both metrics"""
    ndocs, T, dim, tqs, kc, seed = 3000, 40, 64, [12, 5, 14, 1], 700, 1
    assert (len(tqs) + 1) * kc > 8 * _cus()
    for cosine in (False, True):
        queries, tokens, lens, pl = R.build(ndocs, T, dim, tqs, P, 512, cosine, seed)
        queries = queries + [np.empty((0, dim), np.float32)]  # the empty query: every candidate scores 0.0, ordered by index
        rng = np.random.default_rng(seed)
        cand = []
        for qi in range(len(queries)):
            mine = pl.docs[qi] if qi < len(tqs) else np.empty(0, np.int64)
            rest = np.setdiff1d(np.arange(ndocs), mine)
            row = np.concatenate([mine, rng.permutation(rest)[:kc - len(mine)]])
            cand.append(rng.permutation(row))
        cand = np.stack(cand).astype(np.uint64)
        assert all(len(set(r.tolist())) == kc for r in cand)
        dc = M.DocumentCorpus.from_tokens(tokens, lens)
        try:
            po = PairOracle(queries, tokens, lens, cosine)
            (idx, sc), log = logged(lambda: _check_rerank(dc, po, queries, cand, kc, cosine, what=f"strides cos={cosine}"))
            assert [e.inst for e in log if e.family == "ms_rerank"] == [("ms_rerank", int(cosine), 16, 0)], log
            for qi in range(len(tqs)):  # the planted documents lead their query's list
                assert sorted(idx[qi, :P].tolist()) == sorted(pl.docs[qi].tolist()), qi
        finally:
            dc.close()


@pytest.mark.parametrize("cosine", [False, True])
def test_ladder_of_near_ties(M, innr, cosine):
    """100 copies of one document whose scores differ by roundings, more of them than the engine keeps candidates: the approximate order
    decides who is re-scored. Whatever the proof makes of it, the answer is the oracle's stable order -- proven on the MFMA engine, or
    redone on the exact one, and the statistics say which."""
    q, tokens, lens, rungs = R.ladder(cosine=cosine, seed=5)
    want = _oracle_scores(q, tokens, lens, cosine=cosine)
    order = np.argsort(-want.astype(np.float64), kind="stable")
    assert set(order[:len(rungs)].tolist()) == set(rungs.tolist())
    dc = M.DocumentCorpus.from_tokens(tokens, lens)
    try:
        for k in (1, 10):
            st = innr.KnnStats()
            idx, sc = dc.topk(q, k, cosine=cosine, engine=innr.KNN_MFMA, stats=st)
            print(f"ladder cos={cosine} k={k}: engine {st.engine}, fallback {st.queries_fallback}")
            assert idx.tolist() == order[:k].tolist() and bits_equal(sc, want[order[:k]]), (k, idx.tolist(), order[:k].tolist())
            assert st.queries_fallback in (0, 1) and (st.engine == innr.KNN_EXACT) == (st.queries_fallback == 1), (k, st.engine, st.queries_fallback)
    finally:
        dc.close()
