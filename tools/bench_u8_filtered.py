"""Filtered k-NN and range search over a u8 code corpus at the C3 shape (50M x 768 generated codes, 1024 queries, k = 100):
innr_batch_knn_u8_filtered and innr_batch_range_search_u8 against what the library offers without them.

    python tools/bench_u8_filtered.py [N] [D] [Q] > profiles/u8_filtered_c3.txt

 (a) gather   the selection build alone at 1 / 10 / 50 % random selectivity: a 1-query k = 1 INNR_KNN_MFMA call that builds its
              selection (option filter_keep_selection = 0) minus the same call on the cached selection (best of 3 each);
              GB/s = the parent's N*D bytes / that time. Beside it the time of one plain stream of the same bytes in the same run:
              the 1-query count-only range scan (device time of range_scan_u8_kernel<1, count>, which reads every code through
              the loop scan_u8_scores_kernel<1> uses and writes 4 bytes per 1024 vectors), and the ratio.
 (b) repeat   a repeated INNR_KNN_AUTO call at 10 % (the selection cached, best of 3) against innr_batch_knn_u8 under the same
              engine request on a corpus of npass generated codes (same size, same distribution), best of 3 after a warm-up.
 (c) first    the first AUTO call at 10 %: mask, selection build, the selection's int8 copy, search.
 (d) range    1, 8 and 64 queries, thresholds at each query's 99.9th score percentile (taken on a 1M-row sample of the same
              stream): wall time of a whole host call against one innr_batch_scores_u8 call per query plus a NumPy filter (at most
              8 queries timed, extrapolated), and the count-only device time against the exact u8 k-NN scan of the same batch.
The library that INNR_HIP_LIB_PATH names is measured (A/B builds); PARTS=a,b,... in the environment runs only those parts.
All ms are device time from innr_knn_stats (HIP events on the context's stream) unless marked wall."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from innr_amd import KNN_AUTO, KNN_EXACT, KNN_MFMA, KnnStats, _lib
from innr_amd import scalar as S

n = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
nq = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
parts = set(os.environ["PARTS"].split(",")) if os.environ.get("PARTS") else {"a", "b", "c", "d"}
k = 100
ctx = _lib.default_context()
params = S.QuantizationParams.from_range(-1.0, 1.0)
qc = S.QuantizedCorpus.generate(n, dim, params, seed=0)
rng = np.random.default_rng(0)
queries = rng.uniform(-1, 1, size=(nq, dim)).astype(np.float32)
names = {1: "exact", 2: "gemm", 3: "bf16", 4: "int8"}


def filtered(qs, mask, engine, kk=k):
    st = KnnStats()
    qc.knn_filtered_multi(qs, kk, mask, engine=engine, stats=st)
    return st


def best(f, reps=3):
    return min((f() for _ in range(reps)), key=lambda s: s.total_ms)


def count_only(qs, thr):
    st = KnnStats()
    qc.range_search(qs, thr, stats=st, cap=0)
    return st


print(f"# u8 code corpus {n} x {dim} (generated), {nq} queries, k = {k}, one MI355X; library: {_lib.LIB_PATH}")
r = np.random.default_rng(1)
masks = {p: (r.random(n) < p).astype(np.uint8) for p in (0.01, 0.1, 0.5)}

if "a" in parts:
    stream = min((count_only(queries[:1], np.float32([np.inf])) for _ in range(3)), key=lambda s: s.gemm_ms).gemm_ms
    qc.scores(queries[0])  # (under rocprofv3 --kernel-trace the trace then holds scan_u8_scores_kernel<1> over the same corpus)
    print(f"# (a) gather: stream of the same {n * dim / 1e9:.1f} GB (1-query count-only range scan): {stream:.2f} ms = "
          f"{n * dim / stream / 1e6:.0f} GB/s")
    print(f"# {'mask':>10} {'npass':>9} {'gather ms':>9} {'GB/s':>7} {'/ stream':>8}")
    for p, mask in masks.items():
        with ctx.option("filter_keep_selection", 0):
            filtered(queries[:1], mask, KNN_MFMA, 1)  # frees any cached selection: each call below builds one
            b1 = best(lambda: filtered(queries[:1], mask, KNN_MFMA, 1))
        filtered(queries[:1], mask, KNN_MFMA, 1)
        b2 = best(lambda: filtered(queries[:1], mask, KNN_MFMA, 1))
        ms = b1.total_ms - b2.total_ms
        print(f"  {f'random {p * 100:g}%':>10} {int(mask.sum()):>9} {ms:>9.2f} {n * dim / ms / 1e6:>7.0f} {ms / stream:>8.2f}", flush=True)
    qc.release_copies(_lib.COPY_SELECTION)

if "b" in parts or "c" in parts:
    mask = masks[0.1]
    npass = int(mask.sum())
    with ctx.option("filter_keep_selection", 0):
        first = filtered(queries, mask, KNN_AUTO)
    filtered(queries, mask, KNN_AUTO)  # builds the cached selection and its copy
    rep = best(lambda: filtered(queries, mask, KNN_AUTO))
    direct = S.QuantizedCorpus.generate(npass, dim, params, seed=7)
    try:
        direct.knn_multi(queries, k, engine=KNN_AUTO)

        def run_direct():
            st = KnnStats()
            direct.knn_multi(queries, k, engine=KNN_AUTO, stats=st)
            return st
        dst = best(run_direct)
    finally:
        direct.close()
    print(f"# (b) random 10% ({npass} passing), AUTO: repeat {rep.total_ms:.2f} ms ({names.get(rep.engine, '?')}, fallback "
          f"{rep.queries_fallback}), direct {dst.total_ms:.2f} ms ({names.get(dst.engine, '?')}, fallback {dst.queries_fallback}), "
          f"repeat / direct = {rep.total_ms / dst.total_ms:.3f}")
    print(f"# (c) first call (mask, selection, int8 copy, search): {first.total_ms:.2f} ms ({names.get(first.engine, '?')})", flush=True)
    qc.release_copies(_lib.COPY_SELECTION)

if "d" in parts:
    sample = S.QuantizedCorpus.generate(min(n, 1_000_000), dim, params, seed=0)
    try:
        thr = np.float32([np.quantile(sample.scores(q), 0.999) for q in queries[:64]])
    finally:
        sample.close()
    print(f"# (d) range search, thresholds at the 99.9th percentile of each query's scores")
    print(f"# {'Q':>4} {'total':>9} {'call wall':>10} {'scores+filter wall':>19} {'speedup':>8} {'count ms':>9} {'exact kNN ms':>13} {'count/kNN':>10}")
    for q_ in (1, 8, 64):
        qs, t = queries[:q_], thr[:q_]
        qc.range_search(qs, t)  # warm-up: workspace
        t0 = time.perf_counter()
        off, idx, sc = qc.range_search(qs, t)
        wall = 1e3 * (time.perf_counter() - t0)
        m = min(q_, 8)
        t0 = time.perf_counter()
        for j in range(m):
            s = qc.scores(qs[j])
            keep = np.flatnonzero(~(s < t[j]))
            _ = s[keep]
        base = 1e3 * (time.perf_counter() - t0) / m * q_
        cnt = best(lambda: count_only(qs, t))
        st = KnnStats()
        qc.knn_multi(qs, k, engine=KNN_EXACT, stats=st)
        qc.knn_multi(qs, k, engine=KNN_EXACT, stats=st)
        print(f"  {q_:>4} {int(off[-1]):>9} {wall:>10.2f} {base:>19.1f} {base / wall:>8.1f} {cnt.total_ms:>9.2f} {st.total_ms:>13.2f} "
              f"{cnt.total_ms / st.total_ms:>10.2f}", flush=True)
qc.close()
