"""Maxsim re-rank (innr_maxsim_rerank_dev) at C4's corpus: 1M docs x 64 tokens x 128 dims generated, 32-token queries, random
candidates, (Q, kc) in {(1, 100), (1, 1000), (64, 1000), (1024, 100), (1024, 1000)}, dot and cosine. Per configuration: the whole
call (HIP events on the call's stream around DocumentCorpus.rerank with device tensors, median of `reps` calls after warm-up) and
the scan kernels alone (the library's own events around its launches, read from its `trace` diagnostic on stderr, median
likewise); effective rate = 4*Q*kc*T*dim bytes / kernel time. Two yardsticks from the same run: the exact full scan
(innr_maxsim_scores' engine, KnnStats.gemm_ms of an exact top-k) and a full-corpus innr_maxsim_topk call under INNR_KNN_AUTO,
which is what a caller without the re-rank pays per query. Prints one JSON line per measurement and a summary line.

    python tools/bench_maxsim_rerank.py [ndocs] [reps]
"""
import json
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import KNN_AUTO, KNN_EXACT, KnnStats
from innr_amd import maxsim as M

ndocs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
T, dim, Tq = 64, 128, 32
CONFIGS = [(1, 100), (1, 1000), (64, 1000), (1024, 100), (1024, 1000)]


class StderrCapture:
    """the library writes its `trace` diagnostics with fprintf(stderr): catch file descriptor 2"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def unit(x):
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(axis=-1, keepdims=True))).astype(np.float32)


dc = M.DocumentCorpus.generate(ndocs, T, dim, seed=0)
ctx = dc._ctx
rng = np.random.default_rng(123)
q1 = unit(rng.uniform(-1.0, 1.0, size=(Tq, dim)).astype(np.float32))
summary = {"workload": f"maxsim re-rank, {ndocs} docs x {T} tokens x {dim} dims f32, {Tq}-token queries", "reps": reps}

# yardstick 1: the exact full scan's rate; yardstick 2: one full-corpus top-100 call under AUTO
for name, cos in (("dot", False), ("cosine", True)):
    scan, auto = [], []
    for it in range(2 + reps):
        st = KnnStats()
        dc.topk(q1, 100, cosine=cos, stats=st, engine=KNN_EXACT)
        sa = KnnStats()
        dc.topk(q1, 100, cosine=cos, stats=sa, engine=KNN_AUTO)
        if it >= 2:
            scan.append(st.gemm_ms)
            auto.append(sa.total_ms)
    scan_ms, auto_ms = statistics.median(scan), statistics.median(auto)
    summary[f"{name}_full_scan"] = {"scan_ms": scan_ms, "TBps": 4.0 * ndocs * T * dim / (scan_ms * 1e-3) / 1e12}
    summary[f"{name}_topk100_auto"] = {"total_ms": auto_ms, "engine": sa.engine}
    print(json.dumps({"yardstick": name, "full_scan_ms": scan, "topk100_auto_ms": auto}), flush=True)

for Q, kc in CONFIGS:
    q = torch.from_numpy(unit(rng.uniform(-1.0, 1.0, size=(Q, Tq, dim)).astype(np.float32))).cuda()
    cand = torch.from_numpy(np.stack([rng.choice(ndocs, size=kc, replace=False) for _ in range(Q)]).astype(np.int64)).cuda()
    for name, cos in (("dot", False), ("cosine", True)):
        for _ in range(3):
            dc.rerank(q, cand, 10, cosine=cos)
        torch.cuda.synchronize()
        call_ms, kern_ms = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with ctx.option("trace", 1), StderrCapture() as cap:
                e0.record()
                idx, sc = dc.rerank(q, cand, 10, cosine=cos)
                e1.record()
                torch.cuda.synchronize()
            call_ms.append(e0.elapsed_time(e1))
            m = re.search(r"maxsim_rerank .*scan kernels ([0-9.]+) ms", cap.text)
            kern_ms.append(float(m.group(1)))
        # parity of one query against the full scan (bitwise)
        full = dc.scores(q[0].cpu().numpy(), cosine=cos)
        c0 = cand[0].cpu().numpy()
        order = np.lexsort((c0, -full[c0].astype(np.float64)))[:10]
        assert idx[0].cpu().numpy().tolist() == c0[order].tolist()
        assert np.array_equal(sc[0].cpu().numpy().view(np.uint32), full[c0][order].view(np.uint32))
        cm, km = statistics.median(call_ms), statistics.median(kern_ms)
        nbytes = 4.0 * Q * kc * T * dim
        row = {"Q": Q, "kc": kc, "metric": name, "call_ms": cm, "kernel_ms": km, "kernel_TBps": nbytes / (km * 1e-3) / 1e12,
               "pairs_per_s": Q * kc / (cm * 1e-3), "call_ms_all": call_ms, "kernel_ms_all": kern_ms}
        print(json.dumps(row), flush=True)
        summary[f"{name}_Q{Q}_kc{kc}"] = {k2: row[k2] for k2 in ("call_ms", "kernel_ms", "kernel_TBps")}

for name in ("dot", "cosine"):
    big, mid = summary[f"{name}_Q1024_kc1000"], summary[f"{name}_Q1024_kc100"]
    scan, auto = summary[f"{name}_full_scan"], summary[f"{name}_topk100_auto"]
    budget = 1024 * auto["total_ms"] * 10 * (100 / ndocs)
    summary[f"{name}_yardsticks"] = {
        "rate_vs_full_scan": big["kernel_TBps"] / scan["TBps"], "half_of_scan_rate_reached": big["kernel_TBps"] >= 0.5 * scan["TBps"],
        "Q1024_kc100_call_ms": mid["call_ms"], "budget_ms_1024_full_calls_x10_x_kc_over_ndocs": budget,
        "under_budget": mid["call_ms"] < budget}
print(json.dumps(summary))
