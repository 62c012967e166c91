#!/usr/bin/env python3
"""Two-stage late-interaction retrieval, the way multi-vector rerankers are deployed: a cheap dense first stage over ONE
pooled vector per document picks kc candidates per query (batch_knn_dot_multi on a VerticalBatch), then maxsim scores only
those candidates -- every query against its own list, all queries in one device call (DocumentCorpus.rerank). Recall is
measured against maxsim over the whole corpus (DocumentCorpus.topk_multi).

    python examples/maxsim_rerank.py [n_docs] [kc]          (needs a GPU)
"""
from __future__ import annotations

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from innr_amd import batch as B
from innr_amd import maxsim as M


def _unit(x):
    return (x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-12)).astype(np.float32)


def main(n_docs: int = 20000, n_doc_tokens: int = 32, n_query_tokens: int = 16, dim: int = 64, n_queries: int = 64, kc: int = 200,
         k: int = 10) -> float:
    print("Two-stage MaxSim: pooled dense first stage, exact late-interaction re-rank\n")
    rng = np.random.default_rng(11)
    # documents: tokens scattered around a per-document topic; queries: noisy copies of some tokens of a target document
    topics = _unit(rng.normal(size=(n_docs, 1, dim)))
    toks = _unit(topics + 0.8 * rng.normal(size=(n_docs, n_doc_tokens, dim)).astype(np.float32) / np.sqrt(dim) * 4.0)
    targets = rng.integers(0, n_docs, size=n_queries)
    pick = rng.integers(0, n_doc_tokens, size=(n_queries, n_query_tokens))
    queries = _unit(toks[targets[:, None], pick] + 0.3 * rng.normal(size=(n_queries, n_query_tokens, dim)).astype(np.float32))

    corpus = M.DocumentCorpus.from_tokens(toks)
    pooled = _unit(toks.mean(axis=1))
    vb = B.VerticalBatch.from_flat(pooled.reshape(-1), n_docs, dim)
    kc = min(kc, n_docs)

    t0 = time.perf_counter()
    cand, _ = B.batch_knn_dot_multi(_unit(queries.mean(axis=1)), vb, kc)   # stage 1: kc candidates per query
    t1 = time.perf_counter()
    idx, sc = corpus.rerank(queries, cand, k)                              # stage 2: exact maxsim of those, one call
    t2 = time.perf_counter()
    full_idx, full_sc = corpus.topk_multi(list(queries), k)               # what stage 2 replaces: maxsim over every document
    t3 = time.perf_counter()

    kk = idx.shape[1]
    hits = sum(len(set(idx[j].tolist()) & set(full_idx[j].tolist())) for j in range(n_queries))
    recall = hits / float(n_queries * kk)
    print(f"   {n_docs} documents x {n_doc_tokens} tokens x {dim} dims, {n_queries} queries x {n_query_tokens} tokens")
    print(f"   stage 1 (pooled dot, top-{kc}):      {(t1 - t0) * 1e3:8.2f} ms")
    print(f"   stage 2 (maxsim re-rank, top-{kk}):   {(t2 - t1) * 1e3:8.2f} ms   ({n_queries * kc} pairs)")
    print(f"   maxsim over the whole corpus:        {(t3 - t2) * 1e3:8.2f} ms   ({n_queries * n_docs} pairs)")
    print(f"   recall@{kk} = {recall:.3f} against the whole-corpus ranking")
    # a re-ranked score IS the maxsim of that pair: wherever both rankings name a document, the scores are the same bits
    for j in range(n_queries):
        full = dict(zip(full_idx[j].tolist(), full_sc[j].view(np.uint32).tolist()))
        assert all(full.get(d, b) == b for d, b in zip(idx[j].tolist(), sc[j].view(np.uint32).tolist()))
    print("   re-ranked scores are the exact maxsim values")
    print()
    return recall


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000, kc=int(sys.argv[2]) if len(sys.argv) > 2 else 200)
