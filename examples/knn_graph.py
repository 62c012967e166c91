#!/usr/bin/env python3
"""Search by stored vector on the MI355X library: the k-NN graph of a resident corpus (the input of HNSW construction, UMAP or
graph clustering) and near-duplicate detection, both without a second copy of the corpus outside the library.

  1. batch_knn_graph: every vector's k nearest OTHER vectors. The queries are the corpus' own rows, gathered on the device;
     each vector's own index is taken out of its list (only the index: an identical vector stays in, at distance 0).
  2. near-duplicates: rows(ids) on the device hands the vectors to batch_range_search as they are -- every vector within a small
     squared distance of each probe, the probe itself included.
  3. append: the resident corpus grows in place (VerticalBatch.append), and the graph of the grown corpus includes the new vectors.

    python examples/knn_graph.py [corpus_size]          (needs a GPU)
"""
from __future__ import annotations

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from innr_amd import METRIC_L2SQ
from innr_amd import batch as B


def main(corpus_size: int = 20_000, dim: int = 64, k: int = 8, planted: int = 12, probes: int = 256) -> None:
    import torch
    print("k-NN graph and near-duplicates of a resident corpus")
    print("====================================================\n")
    rng = np.random.default_rng(0xC0FFEE)
    rows = rng.uniform(-1, 1, (corpus_size, dim)).astype(np.float32)
    # plant near-duplicates: vector dst[j] = vector src[j] plus a little noise
    pick = rng.choice(corpus_size, 2 * planted, replace=False)
    src, dst = pick[:planted], pick[planted:]
    rows[dst] = rows[src] + rng.uniform(-1e-3, 1e-3, (planted, dim)).astype(np.float32)
    vb = B.VerticalBatch.from_flat(rows.reshape(-1), corpus_size, dim)
    del rows  # from here on the library's copy is the only one

    # ---- 1. the graph
    B.batch_knn_graph(vb, k, first=0, count=min(corpus_size, 256))  # warm-up
    t0 = time.perf_counter()
    gi, gs = B.batch_knn_graph(vb, k)
    t1 = time.perf_counter()
    print(f"graph: {corpus_size} vectors x {dim}d, k = {k}: {1e3 * (t1 - t0):.1f} ms")
    assert gi.shape == (corpus_size, k) and not (gi == np.arange(corpus_size, dtype=np.uint64)[:, None]).any()
    assert (np.diff(gs, axis=1) >= 0).all()  # nearest first
    found = sum(int(gi[s, 0]) == int(d) and int(gi[d, 0]) == int(s) for s, d in zip(src, dst))
    print(f"  planted pairs that are each other's nearest neighbour: {found} / {planted}")
    assert found == planted
    mutual = np.mean([v in gi[int(gi[v, 0])] for v in range(0, corpus_size, max(1, corpus_size // 500))])
    print(f"  vectors that are among their nearest neighbour's own {k} nearest: {100 * mutual:.0f}%\n")

    # ---- 2. near-duplicates of a sample, probes taken from the corpus on the device
    ids = np.unique(np.concatenate([src, rng.integers(0, corpus_size, probes)]))
    d_ids = torch.from_numpy(ids.astype(np.int64)).cuda()
    d_probes = vb.rows(d_ids)  # (n, dim) float32 on the device, bit for bit the stored vectors
    off, idx, sc = B.batch_range_search(d_probes, vb, 0.01, metric=METRIC_L2SQ)
    off, idx = off.cpu().numpy(), idx.cpu().numpy()
    pairs = set()
    for j, i in enumerate(ids):
        hits = idx[off[j]:off[j + 1]]
        assert int(i) in hits  # a vector is within any threshold of itself
        pairs.update((min(int(i), int(h)), max(int(i), int(h))) for h in hits if int(h) != int(i))
    want = set((min(int(s), int(d)), max(int(s), int(d))) for s, d in zip(src, dst))
    print(f"near-duplicates: {len(ids)} probes, squared distance <= 0.01: {len(pairs)} pairs")
    assert pairs == want, (sorted(pairs), sorted(want))
    assert np.array_equal(vb.rows(ids[:4]), d_probes[:4].cpu().numpy())  # host and device gathers agree
    print("every planted near-duplicate found, nothing else; no copy of the corpus outside the library")

    # ---- 3. the corpus grows in place: a few new vectors, each a near-duplicate of a stored one, and their rows of the graph
    extra = min(4, corpus_size)
    twins = np.arange(extra) * (corpus_size // extra)
    vb.append(vb.rows(twins) + np.float32(1e-3))  # only these rows cross the bus; the handle and the old indices stay
    assert vb.num_vectors() == corpus_size + extra
    gi2, _ = B.batch_knn_graph(vb, k, first=corpus_size, count=extra)  # the graph rows of the new vectors ...
    assert gi2[:, 0].tolist() == twins.tolist()
    back, _ = B.batch_knn_rows(twins, vb, k)                           # ... and the grown corpus' rows of their twins
    assert all(corpus_size + j in back[j] for j in range(extra))
    print(f"appended {extra} vectors in place: the graph of the grown corpus ({vb.num_vectors()} vectors) includes them")
    vb.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20_000)
