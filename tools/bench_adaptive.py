"""batch_knn_adaptive on the device (innr_batch_knn_adaptive) against the exact engine's innr_batch_knn for the same queries.

    python tools/bench_adaptive.py [N] [D] [k]  > profiles/adaptive_<shape>.txt

Squared L2, uniform corpus generated on the device (the largest N that fits if N x D does not). One process, the two calls
ALTERNATE within each repeat, one warm-up round first; each is timed with device events on the stream the library runs on (torch
events around the call: the span on the device's timeline, host round trips inside the call included -- what the caller waits
for). Printed: the median of the repeats and their spread (min .. max), stats.candidates_kept (the most vectors alive after a
query's warm-up prune), the warm-up scans' share (stats.gemm_ms) and how many of the exact answer's indices the heuristic kept.
Rows: one query and 8 queries, warm-up in {32, 64, 128, 256}. The comparison is the exact row of the same run, never an
earlier number. Then a decaying-variance corpus of test size (20000 x 128, rows and queries scaled by 0.9^d), where the heuristic
is meant to work: recall against batch_knn."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import KNN_EXACT, METRIC_L2SQ, KnnStats, _lib
from innr_amd import batch as B

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
reps = int(os.environ.get("REPS", "5"))

ctx = _lib.default_context()
ctx.bind_torch_stream()  # the library's kernels on torch's current stream: torch events bracket them
free_b, _ = torch.cuda.mem_get_info()
n = min(n, int(free_b * 0.8) // (4 * ((dim + 31) // 32 * 32) + 16) // 1024 * 1024)  # the corpus, and the call's 12 bytes per vector


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def fmt(ts):
    return f"{statistics.median(ts):>8.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def table(vb, allq, warmups, label):
    print(f"# {label}; k = {k}; ms = median (min .. max) of {reps} alternating repeats after one warm-up round")
    print(f"# {'Q':>3} {'warm-up':>7} {'adaptive ms':>26} {'exact batch_knn ms':>26} {'kept':>9} {'warm-up scans ms':>16} {'recall':>7}")
    for nq in (1, 8):
        qs = allq[:nq]
        for w in warmups:
            ta, te = [], []
            for it in range(reps + 1):
                st = KnnStats()
                ms_a, (ai, _) = timed(lambda: B.batch_knn_adaptive_multi(qs, vb, k, w, stats=st))
                ms_e, (ei, _) = timed(lambda: B.knn_multi(METRIC_L2SQ, qs, vb, k, engine=KNN_EXACT))
                if it:
                    ta.append(ms_a)
                    te.append(ms_e)
            recall = np.mean([len(set(ai[j].tolist()) & set(ei[j].tolist())) / ei.shape[1] for j in range(nq)])
            print(f"  {nq:>3} {w:>7} {fmt(ta):>26} {fmt(te):>26} {st.candidates_kept:>9} {st.gemm_ms:>16.2f} {recall:>7.2f}", flush=True)


vb = B.VerticalBatch.generate(n, dim, 0)
rng = np.random.default_rng(0xADA)
table(vb, rng.uniform(-1, 1, size=(8, dim)).astype(np.float32), [w for w in (32, 64, 128, 256) if w <= dim],
      f"batch_knn_adaptive, squared L2, {n} x {dim} f32 uniform generated on the device, one MI355X")
vb.close()

tn, tdim = 20000, 128
s = (np.float32(0.9) ** np.arange(tdim, dtype=np.float32)).astype(np.float32)
rows = rng.standard_normal((tn, tdim)).astype(np.float32) * s
vb = B.VerticalBatch.from_rows(rows)
table(vb, (rng.standard_normal((8, tdim)).astype(np.float32) * s).astype(np.float32), [32, 64],
      f"decaying variance (rows and queries scaled by 0.9^d, normal), {tn} x {tdim}")
vb.close()
