"""Filtered multi-query kNN at the C2 corpus (10M x 768 f32 uniform, 1024 queries, k = 10) under INNR_KNN_AUTO:
innr_batch_knn_filtered_multi (compact the passing vectors into a selection, then search it) against the alternatives.

    python tools/bench_filtered.py [N] [D] [Q] [MASKS] > profiles/filtered_c2.txt

(MASKS: comma-separated labels, e.g. "random 10%", to run only those cases; METRICS likewise in the environment variable of
that name, "l2sq" or "dot".)

Per metric (squared L2, dot) and mask (random at 100 / 50 / 10 / 1 / 0.1 %, a contiguous 10 % range, every 7th vector):
  first   total_ms of a call that builds its selection (option filter_keep_selection = 0, so every call builds: the selection and
          the filter copy the engine builds on it) and searches it
  repeat  total_ms of a call that finds the selection cached (best of 3)
  build   the selection build alone: a 1-query k = 1 INNR_KNN_MFMA call that builds minus the same call on the cached selection
          (best of 3 each); GB/s = the parent's 4*N*D bytes / build (every lane with a passing vector reads its cache lines)
  direct  the same 1024-query AUTO search on a batch of npass rows made directly (innr_batch_generate: same size, same
          distribution), best of 3 after a warm-up call
  one-q   8 queries through the one-query innr_batch_knn_filtered (squared L2, exact scan), wall time, extrapolated to Q
All ms are device time from innr_knn_stats (HIP events on the context's stream) except one-q (host wall clock of the calls)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from innr_amd import KNN_AUTO, KNN_MFMA, METRIC_DOT, METRIC_L2SQ, KnnStats, _lib
from innr_amd import batch as B

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
nq = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
only = set(sys.argv[4].split(",")) if len(sys.argv) > 4 else None
only_metrics = set(os.environ["METRICS"].split(",")) if os.environ.get("METRICS") else None
k = 10
ctx = _lib.default_context()
L = _lib.load()
vb = B.VerticalBatch.generate(n, dim, 0)
rng = np.random.default_rng(0)
queries = rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)
names = {1: "exact", 2: "gemm", 3: "bf16", 4: "int8"}


def masks():
    r = np.random.default_rng(1)
    for p in (1.0, 0.5, 0.1, 0.01, 0.001):
        yield f"random {p * 100:g}%", (r.random(n) < p).astype(np.uint8)
    m = np.zeros(n, np.uint8)
    m[n // 2:n // 2 + n // 10] = 1
    yield "range 10%", m
    yield "every 7th", (np.arange(n) % 7 == 0).astype(np.uint8)


def call(qs, mask, metric, engine, kk=k):
    st = KnnStats()
    B.batch_knn_filtered_multi(qs, vb, kk, mask, metric=metric, engine=engine, stats=st)
    return st


def best(f, reps=3):
    return min((f() for _ in range(reps)), key=lambda s: s.total_ms)


def one_query_ms(mask, reps=8):
    idx = np.empty(k, np.uint64)
    sc = np.empty(k, np.float32)
    out_k = C.c_size_t(0)
    t = []
    for j in range(reps):
        q = np.ascontiguousarray(queries[j])
        t0 = time.perf_counter()
        _lib.check(L.innr_batch_knn_filtered(vb._h, q.ctypes.data, dim, k, mask.ctypes.data, idx.ctypes.data, sc.ctypes.data,
                                             C.byref(out_k)))
        t.append(time.perf_counter() - t0)
    return 1e3 * sum(t) / len(t)


print(f"# innr_batch_knn_filtered_multi, {n} x {dim} f32 uniform, {nq} queries, k = {k}, INNR_KNN_AUTO, one MI355X")
print(f"# {'metric':>6} {'mask':>12} {'npass':>9} {'first ms':>9} {'repeat':>8} {'engine':>6} {'build ms':>9} {'GB/s':>7} "
      f"{'direct ms':>9} {'rep/dir':>7} {'one-q ms':>9} {'x{nq}'.rjust(9)} {'speedup':>8}")
for metric, mname in ((METRIC_L2SQ, "l2sq"), (METRIC_DOT, "dot")):
    if only_metrics and mname not in only_metrics:
        continue
    for label, mask in masks():
        if only and label not in only:
            continue
        npass = int(mask.sum())
        with ctx.option("filter_keep_selection", 0):
            first = call(queries, mask, metric, KNN_AUTO)
        call(queries, mask, metric, KNN_AUTO)  # builds the cached selection
        rep = best(lambda: call(queries, mask, metric, KNN_AUTO))
        build_ms = float("nan")
        if npass < n:
            with ctx.option("filter_keep_selection", 0):
                call(queries[:1], mask, metric, KNN_MFMA, 1)  # frees the cached selection: each call below builds one
                b1 = best(lambda: call(queries[:1], mask, metric, KNN_MFMA, 1))
            call(queries[:1], mask, metric, KNN_MFMA, 1)
            b2 = best(lambda: call(queries[:1], mask, metric, KNN_MFMA, 1))
            build_ms = b1.total_ms - b2.total_ms
        gbs = 4.0 * n * dim / (build_ms * 1e-3) / 1e9 if build_ms == build_ms and build_ms > 0 else float("nan")
        direct = B.VerticalBatch.generate(npass, dim, 7)
        try:
            fn = B.batch_knn_multi if metric == METRIC_L2SQ else B.batch_knn_dot_multi
            fn(queries, direct, k, engine=KNN_AUTO)

            def run_direct():
                st = KnnStats()
                fn(queries, direct, k, engine=KNN_AUTO, stats=st)
                return st
            dst = best(run_direct)
        finally:
            direct.close()
        oq = one_query_ms(mask) if metric == METRIC_L2SQ else float("nan")
        print(f"  {mname:>6} {label:>12} {npass:>9} {first.total_ms:>9.2f} {rep.total_ms:>8.2f} {names.get(rep.engine, '?'):>6} "
              f"{build_ms:>9.2f} {gbs:>7.0f} {dst.total_ms:>9.2f} {rep.total_ms / dst.total_ms:>7.2f} {oq:>9.2f} "
              f"{oq * nq:>9.0f} {oq * nq / rep.total_ms:>8.0f}", flush=True)
