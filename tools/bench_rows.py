"""Search by stored vector (innr_batch_gather_rows_dev, innr_batch_knn_rows_dev) at the headline shape.

    python tools/bench_rows.py [N] [D] [section ...]  > profiles/rows_<shape>.txt        sections: gather knn extract (default: all)

Uniform corpus generated on the device (the largest N that fits if N x D and its row-major copy do not). One process; the library
runs on torch's current stream and every figure is the span between two torch events around the call on that stream -- the device's
timeline, the call's own host round trip (the index flag) included: what a caller waits for. One warm-up round, then REPS repeats
in which the variants of a section ALTERNATE; printed: median (min .. max).
  gather   4096 consecutive and 4096 random ids, from the dimension-major store and from the row-major copy, beside a device-to-
           device copy of the same n*D*4 bytes; bytes WRITTEN per second.
  knn      innr_batch_knn_rows_dev (1024 consecutive ids, k = 10, exclude_self, AUTO) against innr_batch_knn_dev on the same 1024
           vectors already row-major on the device at k = 11 -- the same search, without gather and strip -- and the gather alone.
           The results are compared. (The strip kernel has no entry point of its own: its time is the kernel trace's, a separate
           run of this section under rocprofv3 --kernel-trace --stats.)
  extract  VerticalBatch.extract_vector on the fresh batch: host wall time of the call."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import COPY_ROWS, KNN_AUTO, METRIC_L2SQ, KnnStats, _lib
from innr_amd import batch as B

args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 10_000_000
dim = int(args[1]) if len(args) > 1 else 768
sections = args[2:] or ["extract", "gather", "knn"]
reps = int(os.environ.get("REPS", "9"))

ctx = _lib.default_context()
ctx.bind_torch_stream()
lib = _lib.load()
free_b, _ = torch.cuda.mem_get_info()
n = min(n, int(free_b * 0.8) // (8 * ((dim + 31) // 32 * 32) + 64) // 1024 * 1024)  # the store and the row-major copy


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def fmt(ts):
    return f"{statistics.median(ts):>9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def ptr(t):
    return C.c_void_p(t.data_ptr())


vb = B.VerticalBatch.generate(n, dim, 0)
print(f"# {n} x {dim} f32 uniform generated on the device, one MI355X; ms = median (min .. max) of {reps} alternating repeats after "
      f"one warm-up round")

if "extract" in sections:
    ts = []
    for i in (0, n // 2, n - 1, 12345, n // 3):
        t0 = time.perf_counter()
        v = vb.extract_vector(i)
        ts.append(1e3 * (time.perf_counter() - t0))
    assert vb._host is None and v.shape == (dim,)
    print(f"# extract_vector on the fresh batch (host wall time, ms; the first call sizes the workspace): "
          f"{', '.join(f'{t:.3f}' for t in ts)}   -- {dim * 4} bytes each, the corpus stays on the device")

if "gather" in sections:
    m = 4096
    out = torch.empty((m, dim), dtype=torch.float32, device="cuda")
    src = torch.rand((m, dim), dtype=torch.float32, device="cuda")
    lists = {"consecutive": torch.arange(n // 2, n // 2 + m, dtype=torch.int64, device="cuda"),
             "random": torch.from_numpy(np.random.default_rng(1).integers(0, n, m)).cuda()}
    nbytes = m * dim * 4
    print(f"# gather: {m} ids -> {nbytes} bytes written")
    print(f"# {'ids':>12} {'source':>10} {'gather ms':>30} {'GB/s written':>13} {'d2d copy of the same bytes ms':>32}")
    for source in ("store", "rows copy"):
        if source == "rows copy":
            assert vb.build_copies(COPY_ROWS) & COPY_ROWS
        for name, ids in lists.items():
            tg, tc = [], []
            for it in range(reps + 1):
                ms_g, st = timed(lambda: lib.innr_batch_gather_rows_dev(vb._h, ptr(ids), m, ptr(out)))
                assert st == 0
                ms_c, _ = timed(lambda: out.copy_(src))
                if it:
                    tg.append(ms_g)
                    tc.append(ms_c)
            print(f"  {name:>12} {source:>10} {fmt(tg):>30} {nbytes / statistics.median(tg) / 1e6:>13.1f} {fmt(tc):>32}", flush=True)
    vb.release_copies(COPY_ROWS)

if "knn" in sections:
    q, k = 1024, 10
    ids = torch.arange(n // 2, n // 2 + q, dtype=torch.int64, device="cuda")
    rows = vb.rows(ids)  # the same vectors, row-major on the device
    oi_r = torch.empty((q * k,), dtype=torch.int64, device="cuda")
    os_r = torch.empty((q * k,), dtype=torch.float32, device="cuda")
    oi_k = torch.empty((q * (k + 1),), dtype=torch.int64, device="cuda")
    os_k = torch.empty((q * (k + 1),), dtype=torch.float32, device="cuda")
    gout = torch.empty((q, dim), dtype=torch.float32, device="cuda")
    st_r, st_k, out_k = KnnStats(), KnnStats(), C.c_size_t(0)

    def knn_rows():
        return lib.innr_batch_knn_rows_dev(vb._h, METRIC_L2SQ, ptr(ids), q, k, 1, KNN_AUTO, ptr(oi_r), ptr(os_r), C.byref(out_k),
                                           C.byref(st_r))

    def knn_dev():
        return lib.innr_batch_knn_dev(vb._h, METRIC_L2SQ, ptr(rows), q, dim, k + 1, KNN_AUTO, ptr(oi_k), ptr(os_k), C.byref(out_k),
                                      C.byref(st_k))

    def gather():
        return lib.innr_batch_gather_rows_dev(vb._h, ptr(ids), q, ptr(gout))

    tr, tk, tg = [], [], []
    for it in range(reps + 1):
        for fn, ts in ((knn_rows, tr), (knn_dev, tk), (gather, tg)):
            ms, st = timed(fn)
            assert st == 0
            if it:
                ts.append(ms)
    # the same answers: k + 1 results with the query's own index removed
    full_i, full_s = oi_k.cpu().numpy().reshape(q, k + 1), os_k.cpu().numpy().reshape(q, k + 1)
    got_i, got_s = oi_r.cpu().numpy().reshape(q, k), os_r.cpu().numpy().reshape(q, k)
    me = ids.cpu().numpy()
    for j in range(q):
        keep = full_i[j] != me[j]
        assert keep.sum() == k and (full_i[j][keep] == got_i[j]).all() and (full_s[j][keep].view(np.uint32) == got_s[j].view(np.uint32)).all()
    print(f"# knn: {q} consecutive ids, squared L2, AUTO (engine {st_r.engine} / {st_k.engine}); results equal")
    print(f"  innr_batch_knn_rows_dev  k = {k}, exclude_self      {fmt(tr)}   (stats.total_ms {st_r.total_ms:.3f}, gemm_ms {st_r.gemm_ms:.3f})")
    print(f"  innr_batch_knn_dev       k = {k + 1}, rows resident     {fmt(tk)}   (stats.total_ms {st_k.total_ms:.3f}, gemm_ms {st_k.gemm_ms:.3f})")
    print(f"  innr_batch_gather_rows_dev alone                 {fmt(tg)}")
    print(f"  difference of the medians                        {statistics.median(tr) - statistics.median(tk):>9.3f}")
vb.close()
