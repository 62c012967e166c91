"""Range search (innr_batch_range_search) against the only way to do it before: one innr_batch_l2_squared_pruning call per query.

    python tools/bench_range.py compare [N] [D] [Q,Q,...]  > profiles/range_search_<shape>.txt     (a)
    python tools/bench_range.py q0      [N] [D] [Q,Q,...]  >> profiles/range_search_<shape>.txt    (b)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_range.py shares [N] [D] [Q]        (c)
    python tools/bench_range.py u8      [N] [D] [Q,Q,...]  > profiles/range_search_u8_<shape>.txt  (d)

Squared L2, uniform corpus generated on the device, thresholds = each query's 100th best distance (innr_batch_knn), so every query
has 100 results (ties aside). One process, the variants ALTERNATE within each repeat (loop, exact, collect, loop, ...), one warm-up
round first; every variant is timed with device events on the stream the library runs on (torch events around the calls: the
span on the device's timeline, host round trips between the calls included -- what the caller waits for), the new engines also
report innr_knn_stats.total_ms (events inside the call). Printed: the median of the repeats and their spread (min .. max).
  compare: loop of Q pruning calls | INNR_KNN_EXACT | INNR_KNN_MFMA, Q in {1, 8, 64, 1024}
  q0     : INNR_KNN_EXACT | INNR_KNN_MFMA at Q in {4, 8, 16, 32, 64, 128, 256}: the crossover behind kRangeAutoQ0 (api.hip)
  u8     : innr_batch_range_search_u8 on a code corpus (uniform rows quantised over [-1, 1], thresholds = each query's 100th best
           score): INNR_KNN_EXACT | INNR_KNN_MFMA_I8 with the int8 copy in place, at Q in {8, 16, 32, 64, 128, 1024}: the crossover
           behind kRangeU8AutoQ0 (api.hip)
  shares : the MFMA call five times and nothing else, for a kernel trace of its own (the collect pass, the re-score, the finish
           kernels and the fills that zero the bitmaps and counts are told apart by kernel name in the trace's statistics)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import KNN_EXACT, KNN_MFMA, KNN_MFMA_I8, METRIC_L2SQ, KnnStats, _lib
from innr_amd import batch as B
from innr_amd import scalar as S

mode = sys.argv[1] if len(sys.argv) > 1 else "compare"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
dim = int(sys.argv[3]) if len(sys.argv) > 3 else 768
default_q = {"compare": "1,8,64,1024", "q0": "4,8,16,32,64,128,256", "shares": "1024", "u8": "8,16,32,64,128,1024"}[mode]
qlist = [int(x) for x in (sys.argv[4] if len(sys.argv) > 4 else default_q).split(",")]
reps = int(os.environ.get("REPS", "5"))

ctx = _lib.default_context()
ctx.bind_torch_stream()  # the library's kernels on torch's current stream: torch events bracket them
u8 = mode == "u8"
if u8:
    qc = S.QuantizedCorpus.generate(n, dim, S.QuantizationParams.from_range(-1.0, 1.0), 0)
    qc.build_copies(_lib.COPY_I8_DOT)  # the copy in place: its build is not part of any timed call
else:
    vb = B.VerticalBatch.generate(n, dim, 0)
allq = np.random.default_rng(0xA11CE).uniform(-1, 1, size=(max(qlist), dim)).astype(np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def loop(qs, thr):
    return sum(len(B.batch_l2_squared_pruning(q, vb, float(t))) for q, t in zip(qs, thr))


def engine(eng):
    def run(qs, thr):
        st = KnnStats()
        off, _, _ = B.batch_range_search(qs, vb, thr, metric=METRIC_L2SQ, engine=eng, stats=st, max_results=len(qs) * 128)
        return int(off[-1]), st
    return run


def engine_u8(eng):
    def run(qs, thr):
        st = KnnStats()
        off, _, _ = qc.range_search(qs, thr, engine=eng, stats=st, cap=len(qs) * 128)
        assert st.engine == eng, f"asked for engine {eng}, served by {st.engine}"
        return int(off[-1]), st
    return run


def thresholds(qs):
    """each query's 100th best: distances of the f32 corpus, scores of the code corpus"""
    if u8:
        return np.ascontiguousarray(qc.knn_multi(qs, 100)[1][:, 99])
    return np.ascontiguousarray(B.knn_multi(METRIC_L2SQ, qs, vb, 100)[1][:, 99])


def fmt(ts):
    return f"{statistics.median(ts):>9.2f} ({min(ts):.2f} .. {max(ts):.2f})"


variants = [("exact", engine_u8(KNN_EXACT)), ("mfma", engine_u8(KNN_MFMA_I8))] if u8 else [("exact", engine(KNN_EXACT)), ("mfma", engine(KNN_MFMA))]
if mode == "compare":
    variants.insert(0, ("loop", loop))
print(f"# range search, {'asymmetric score, ' + str(n) + ' x ' + str(dim) + ' u8 codes' if u8 else 'squared L2, ' + str(n) + ' x ' + str(dim) + ' f32'} "
      f"uniform, thresholds at each query's 100th best, one MI355X; ms = median (min .. max) of {reps} alternating repeats after one "
      f"warm-up round" + ("; mfma = INNR_KNN_MFMA_I8, the int8 copy in place" if u8 else ""))
if mode == "shares":
    qs = allq[:qlist[0]]
    thr = np.ascontiguousarray(B.knn_multi(METRIC_L2SQ, qs, vb, 100)[1][:, 99])
    for _ in range(5):
        ms, (total, st) = timed(lambda: engine(KNN_MFMA)(qs, thr))
        print(f"  mfma Q={len(qs)}: {ms:.2f} ms (stats: total {st.total_ms:.2f}, collect pass {st.gemm_ms:.2f}, longest list "
              f"{st.candidates_kept}, fallback {st.queries_fallback}), {total} results", flush=True)
    sys.exit(0)
print("# " + f"{'Q':>5} " + " ".join(f"{name + ' ms':>30}" for name, _ in variants) + "   stats.total_ms exact / mfma (collect pass, fallback)")
for nq in qlist:
    qs = allq[:nq]
    thr = thresholds(qs)
    times = {name: [] for name, _ in variants}
    stats = {}
    totals = set()
    for it in range(reps + 1):
        for name, fn in variants:
            ms, out = timed(lambda: fn(qs, thr))
            total, st = out if isinstance(out, tuple) else (out, None)
            totals.add(total)
            if it:
                times[name].append(ms)
                if st is not None:
                    stats.setdefault(name, []).append(st)
    assert len(totals) == 1, f"the variants disagree on the number of results: {totals}"
    ex = statistics.median(s.total_ms for s in stats["exact"])
    mf = statistics.median(s.total_ms for s in stats["mfma"])
    m0 = stats["mfma"][0]
    print(f"  {nq:>5} " + " ".join(f"{fmt(times[name]):>30}" for name, _ in variants) +
          f"   {ex:.2f} / {mf:.2f} ({statistics.median(s.gemm_ms for s in stats['mfma']):.2f}, {m0.queries_fallback}); "
          f"{totals.pop()} results", flush=True)
