"""Threshold seeding A/B at the C2 shape: python tools/seed_ab.py 0 1024 2048 4096 8192   (0 = no seeding; INNR_GEMM_SEED_N)
The split filter's own seeder (context option split_seed_rows; -1 = the exact seeder), alternating in one process, three calls each:
    python tools/seed_ab.py split -1 2048 8192 16384 32768"""
import os, subprocess, sys
code = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
from innr_amd import KNN_MFMA_I8, KNN_MFMA_BF16, KnnStats
from innr_amd import batch as B
vb = B.VerticalBatch.generate(10_000_000, 768, 0)
q = np.random.default_rng(0xBE7C).uniform(-1, 1, size=(1024, 768)).astype(np.float32)
for name, eng in (("int8", KNN_MFMA_I8), ("bf16", KNN_MFMA_BF16)):
    best = None
    for it in range(5):
        st = KnnStats()
        B.batch_knn_dot_multi(q, vb, 10, engine=eng, stats=st)
        if it and (best is None or st.total_ms < best.total_ms):
            best = st
    print(f"seed prefix {os.environ.get('INNR_GEMM_SEED_N', 'none' if os.environ.get('INNR_GEMM_NO_SEED') else '2048')} {name}: kernel {best.gemm_ms:.3f} ms, call {best.total_ms:.3f} ms, redone {best.queries_fallback}", flush=True)
'''
# the f32 engine on device-resident queries (bench.py's path), the flagged share through the hook tools/screen_counts.py reads
split_code = r'''
import ctypes as C, os, sys
sys.path.insert(0, os.getcwd())
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
values = [int(v) for v in sys.argv[1:]]
wt = ((N + 255) // 256 * 256) // 128 * (Q // 64)
for v in values[:1] * 2:  # warm-up: the limb copies, the workspace
    search(q, 10, KnnStats())
for rep in range(3):
    for v in values:
        _lib.default_context().set_option("split_seed_rows", v)
        search(q, 10, KnnStats()); torch.cuda.synchronize()  # (the first call of a value may grow the seeder's buffers)
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        st = KnnStats(); t0.record(); search(q, 10, st); t1.record(); torch.cuda.synchronize()
        out = np.zeros(4, np.uint32); assert fn(vb._h, out.ctypes.data) == 0
        print(f"split_seed_rows {v:6d} round {rep}: call {t0.elapsed_time(t1):.3f} ms, filter kernel {st.gemm_ms:.3f} ms, redone {st.queries_fallback}, "
              f"flagged wave tiles {out[0]} of {wt} = {100.0 * out[0] / wt:.3f} %", flush=True)
'''
if sys.argv[1:2] == ["split"]:
    raise SystemExit(subprocess.run([sys.executable, "-c", split_code] + (sys.argv[2:] or ["-1", "2048", "8192", "16384", "32768"])).returncode)
for n in sys.argv[1:] or ["2048"]:
    env = dict(os.environ)
    if n == "0":
        env["INNR_GEMM_NO_SEED"] = "1"
    else:
        env["INNR_GEMM_SEED_N"] = n
    subprocess.run([sys.executable, "-c", code], env=env, check=False)
