#!/usr/bin/env python3
"""A/B of INNR_KNN_MFMA's two dot / cosine filters at the C2 corpus (10M x 768): the split-bf16 filter (kernels_gemm_bf16.h,
LIMBS = 3) against the f32 kernel (context option no_split_filter = 1), alternating in one process.

Per row: the default dispatch, the f32 kernel, and the split filter forced at every batch size (split_min_q = 1: what sets the
crossover kSplitMinQ in api.hip) -- best of REPS calls each, in ms per call -- and whether all three return the same answers
(indices and score bits).

    python tools/split_ab.py [REPS]        (profiles/r04_split_ab.txt)
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from innr_amd import GEN_EXAMPLE_LCG, GEN_UNIFORM, KNN_MFMA, METRIC_COSINE, METRIC_DOT, KnnStats  # noqa: E402
from innr_amd import _lib  # noqa: E402
from innr_amd import batch as B  # noqa: E402
from innr_amd.dist import _gpu_local_search  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N, D = 10_000_000, 768
ctx = _lib.default_context()
dev = torch.device("cuda:0")
SETTINGS = (("default", {}), ("f32", {"no_split_filter": 1}), ("split", {"split_min_q": 1}))


def queries(nq, gen):
    qb = (B.VerticalBatch.generate(nq, D, seed=N, generator=GEN_EXAMPLE_LCG) if gen == GEN_EXAMPLE_LCG
          else B.VerticalBatch.generate(nq, D, seed=0xBE7C))
    q = np.ascontiguousarray(np.asarray(qb.data(), dtype=np.float32).reshape(D, nq).T)
    qb.close()
    return torch.from_numpy(q).to(dev)


def run(search, q, k, opts):
    for name in ("no_split_filter", "split_min_q"):
        ctx.set_option(name, opts.get(name, 0))
    st = KnnStats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, sc = search(q, k, st)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, st, idx, sc


def row(label, search, q, k):
    best = {n: None for n, _ in SETTINGS}
    out = {}
    for n, o in SETTINGS:  # warm-up: builds the limb copies / the row-major copy once
        run(search, q, k, o)
    for _ in range(REPS):
        for n, o in SETTINGS:
            ms, st, idx, sc = run(search, q, k, o)
            if best[n] is None or ms < best[n][0]:
                best[n] = (ms, st.gemm_ms, st.queries_fallback)
            out[n] = (idx, sc)
    same = all(torch.equal(out["f32"][0], out[n][0]) and torch.equal(out["f32"][1].view(torch.int32), out[n][1].view(torch.int32))
               for n in ("default", "split"))
    cells = "  ".join(f"{n} {best[n][0]:8.2f} ms (filter {best[n][1]:7.2f}, redone {best[n][2]:4d})" for n, _ in SETTINGS)
    print(f"{label:<34} {cells}  same answers: {same}", flush=True)


print(f"C2 corpus {N} x {D}; best of {REPS} calls per setting, settings alternating; "
      f"{torch.cuda.get_device_name(0)}", flush=True)
vb = B.VerticalBatch.generate(N, D, seed=0, generator=GEN_UNIFORM)
for metric, label in ((METRIC_DOT, "dot"), (METRIC_COSINE, "cos")):
    search = _gpu_local_search(vb, metric, KNN_MFMA)
    sizes = (1, 8, 64, 128, 256, 384, 512, 1024, 4096) if metric == METRIC_DOT else (4096,)
    for nq in sizes:
        q = queries(nq, GEN_UNIFORM)
        for k in ((10, 100) if metric == METRIC_DOT else (10,)):
            row(f"uniform {label} Q={nq} k={k}", search, q, k)
vb.close()
lvb = B.VerticalBatch.generate(N, D, seed=0, generator=GEN_EXAMPLE_LCG)
search = _gpu_local_search(lvb, METRIC_DOT, KNN_MFMA)
row("lcg dot Q=1024 k=10", search, queries(1024, GEN_EXAMPLE_LCG), 10)
lvb.close()
for name in ("no_split_filter", "split_min_q"):
    ctx.set_option(name, 0)
