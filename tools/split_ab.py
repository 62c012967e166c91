#!/usr/bin/env python3
"""A/B of INNR_KNN_MFMA's two dot / cosine filters at the C2 corpus (10M x 768): the split-bf16 filter (kernels_gemm_bf16.h,
LIMBS = 3) against the f32 kernel (context option no_split_filter = 1), alternating in one process.

Per row: the default dispatch, the f32 kernel, the split filter forced at every batch size (split_min_q = 1: what sets the
crossover kSplitMinQ in api.hip), the split filter forced in its screened form (no_split_screen = -1) and with its full
three-product K-loop (no_split_screen = 1: the A/B of the hi.hi screen) -- best of REPS calls each, in ms per
call --, whether all return the same answers (indices and score bits), and the share of wave tiles the screened form corrected
(test hook innrdbg_split_screen_counts). `default` and `split` follow the batch's remembered share (knn_mfma).

    python tools/split_ab.py [REPS] [quick]        (profiles/r04_split_ab.txt, r05_split_ab.txt)
quick: 65 / 128 / 1024 queries and the LCG row only.
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
QUICK = len(sys.argv) > 2 and sys.argv[2] == "quick"
SETTINGS = (("default", {}), ("f32", {"no_split_filter": 1}), ("split", {"split_min_q": 1}),
            ("screen", {"split_min_q": 1, "no_split_screen": -1}), ("no_split_screen", {"split_min_q": 1, "no_split_screen": 1}))
OPTIONS = ("no_split_filter", "split_min_q", "no_split_screen")


def queries(nq, gen):
    qb = (B.VerticalBatch.generate(nq, D, seed=N, generator=GEN_EXAMPLE_LCG) if gen == GEN_EXAMPLE_LCG
          else B.VerticalBatch.generate(nq, D, seed=0xBE7C))
    q = np.ascontiguousarray(np.asarray(qb.data(), dtype=np.float32).reshape(D, nq).T)
    qb.close()
    return torch.from_numpy(q).to(dev)


SHARE = [None]
_hooks = None


def corrected_share(nq):
    """wave tiles the last call's screened launch corrected, of those that hold a real query (hook innrdbg_split_screen_counts)"""
    global _hooks
    import ctypes as C
    if _hooks is None:
        _hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libinnr_hip_testhooks.so"))
        _hooks.innrdbg_split_screen_counts.restype = C.c_int
        _hooks.innrdbg_split_screen_counts.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(2, np.uint32)
    if CUR[0] is None or _hooks.innrdbg_split_screen_counts(CUR[0]._h, out.ctypes.data) != 0:
        return None
    return float(out[0]) / (((N + 255) // 256 * 256) // 128 * ((nq + 63) // 64))


CUR = [None]


def run(search, q, k, opts):
    for name in OPTIONS:
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
            if n == "screen":
                SHARE[0] = corrected_share(q.shape[0])
            if best[n] is None or ms < best[n][0]:
                best[n] = (ms, st.gemm_ms, st.queries_fallback)
            out[n] = (idx, sc)
    same = all(torch.equal(out["f32"][0], out[n][0]) and torch.equal(out["f32"][1].view(torch.int32), out[n][1].view(torch.int32))
               for n in ("default", "split", "screen", "no_split_screen"))
    share = ""
    if SHARE[0] is not None:
        share = f"  corrected {100.0 * SHARE[0]:5.1f} % of wave tiles"
    cells = "  ".join(f"{n} {best[n][0]:8.2f} ms (filter {best[n][1]:7.2f}, redone {best[n][2]:4d})" for n, _ in SETTINGS)
    print(f"{label:<34} {cells}  same answers: {same}{share}", flush=True)


print(f"C2 corpus {N} x {D}; best of {REPS} calls per setting, settings alternating; "
      f"{torch.cuda.get_device_name(0)}", flush=True)
vb = B.VerticalBatch.generate(N, D, seed=0, generator=GEN_UNIFORM)
CUR[0] = vb
for metric, label in ((METRIC_DOT, "dot"), (METRIC_COSINE, "cos")):
    search = _gpu_local_search(vb, metric, KNN_MFMA)
    sizes = (1, 8, 64, 65, 128, 256, 384, 512, 1024, 4096) if metric == METRIC_DOT else (4096,)
    if QUICK:
        sizes = (65, 128, 1024) if metric == METRIC_DOT else ()
    for nq in sizes:
        q = queries(nq, GEN_UNIFORM)
        for k in ((10, 100) if metric == METRIC_DOT else (10,)):
            row(f"uniform {label} Q={nq} k={k}", search, q, k)
vb.close()
lvb = B.VerticalBatch.generate(N, D, seed=0, generator=GEN_EXAMPLE_LCG)
CUR[0] = lvb
search = _gpu_local_search(lvb, METRIC_DOT, KNN_MFMA)
row("lcg dot Q=1024 k=10", search, queries(1024, GEN_EXAMPLE_LCG), 10)
lvb.close()
for name in OPTIONS:
    ctx.set_option(name, 0)
