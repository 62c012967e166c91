#!/usr/bin/env python3
"""Flagged wave tiles / sub-tiles of the screened split filter, the pairs its pair path corrected and the wave tiles
that took the MFMA fallback, in three calls at the C2 shape (10M x 768, 1024 queries, k = 10), read through the test hook
innrdbg_split_screen_counts4 of libinnr_hip_testhooks.so -- first with the screen margin by the worst-case formula alone (context
option split_screen_worst_case = 1), then with the margin from the limbs' measured norms (the default).

    python tools/screen_counts.py        (profiles/r05_screen_counts.txt: the first two words; r06_, r07_screen_counts.txt)
"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from innr_amd import GEN_UNIFORM, KNN_MFMA, METRIC_DOT, KnnStats, _lib
from innr_amd import batch as B
from innr_amd.dist import _gpu_local_search
N, D, Q = 10_000_000, 768, 1024
hooks = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libinnr_hip_testhooks.so"))
fn = hooks.innrdbg_split_screen_counts4; fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_void_p]
vb = B.VerticalBatch.generate(N, D, seed=0, generator=GEN_UNIFORM)
qb = B.VerticalBatch.generate(Q, D, seed=0xBE7C)
q = torch.from_numpy(np.ascontiguousarray(np.asarray(qb.data(), dtype=np.float32).reshape(D, Q).T)).to("cuda:0")
search = _gpu_local_search(vb, METRIC_DOT, KNN_MFMA)
for worst in (1, 0):
    _lib.default_context().set_option("split_screen_worst_case", worst)
    print("margin:", "worst-case formula" if worst else "from the limb norms", flush=True)
    for rep in range(3):
        st = KnnStats(); search(q, 10, st); torch.cuda.synchronize()
        out = np.zeros(4, np.uint32); assert fn(vb._h, out.ctypes.data) == 0
        ntiles = ((N + 255) // 256 * 256) // 128; wt = ntiles * (Q // 64)
        print(f"call {rep}: filter {st.gemm_ms:.2f} ms, redone {st.queries_fallback}; corrected wave tiles {out[0]} of {wt} = {100.0*out[0]/wt:.3f} %; "
              f"sub-tiles {out[1]} of {8*wt} = {100.0*out[1]/(8*wt):.4f} %; pairs corrected one by one {out[2]}, "
              f"{out[2]/max(1, int(out[0])-int(out[3])):.2f} per wave tile on the pair path; wave tiles on the MFMA fallback {out[3]} = "
              f"{100.0*out[3]/max(1, int(out[0])):.2f} % of the flagged", flush=True)
