#!/usr/bin/env python3
"""bench.py -- BASELINE.json's headline metric on MI355X.

Workload (configs[1]): batch_knn_dot, f32, 10M x 768 corpus per GPU, 1024-query batch, k = 10.
A "step" = one pass of the hot path over one query batch: innr_batch_knn_dev (query transpose, f32-MFMA GEMM
with fused top-k filter, cross-slice select, exact re-score + margin proof [, exact-engine redo of unproven
queries]) with the corpus and the queries already resident in HBM; for N > 1 GPUs (one process per GPU, corpus
range-partitioned, weak scaling: 10M vectors PER GPU) the step also includes the RCCL all-gather of the
per-shard top-k and the merge. value = vectors scanned per second = Q * N_total / step time.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  N > 1: one process per GPU -- launched by `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`, or, from a
  bare shell, by bench.py itself (it starts that launcher as a child before touching a GPU and relays rank 0's line).

Prints ONE JSON line on rank 0 with the `roofline` object described in DESIGN.md (dominant kernel: the GEMM, timed live with
HIP events on the stream it is launched on, inside the timed steps). A plain run does only what that line needs: set-up,
warm-up, the timed steps, the --dump-outputs arrays and the line. --full adds the measurements that take runs of their own
(N = 1 only): the side rows (the same call on the bf16 and int8 filter engines with a bit-equality check against the f32
engine, and on the reference example's LCG data) and `cpu_baseline` (the CPU oracle = "port" of innr's portable path, single
thread like the reference, on a bounded sample); --no-side-rows and --no-cpu-baseline drop either from a --full run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 256 flop/clk x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2516.0  # dense bf16: v_mfma_f32_32x32x16_bf16, 256 CU x 4096 flop/clk x 2.4 GHz (--engine bf16 only)


def cpu_baseline(dim: int, k: int, budget_s: float = 20.0):
    """Oracle (port of batch_knn_dot: src/batch.rs:742-764 = scan :284-297 + full stable sort :756-758) on the
    host, ONE thread (the reference has no threading), on a 1M-vector sub-sample of the same uniform stream."""
    import numpy as np
    import oracle

    n = 1_000_000
    rows = oracle.generate_uniform(n, dim, 0)
    data = oracle.from_rows(rows)
    del rows
    queries = oracle.generate_uniform(128, dim, 0xBE7C)
    knn = oracle.native_knn_dot()  # the -march=native build made at the start of this run (None: no compiler on this host)
    flags = "-O3 -march=native -ffp-contract=off (built on this host)" if knn else "-O3 -march=x86-64-v3 -ffp-contract=off (the portable build)"
    knn = knn or oracle.batch_knn_dot
    i0, s0 = knn(queries[0], data[:, :1000].copy(), k)  # warm the library; the native build must agree with the checker's
    i1, s1 = oracle.batch_knn_dot(queries[0], data[:, :1000].copy(), k)
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    done, t0 = 0, time.perf_counter()
    while done < len(queries):
        knn(queries[done], data, k)
        done += 1
        if time.perf_counter() - t0 >= budget_s:
            break
    dt = time.perf_counter() - t0
    out = {
        "value": done * n / dt,
        "unit": "vectors/s",
        "cores": 1,
        "kind": "port",
        "qps_at_10M": (done / dt) * (n / 10_000_000),
        "sample": f"oracle batch_knn_dot (scan + full stable sort), {done} queries x {n} x {dim} f32 uniform(-1,1), k={k}, "
                  f"{dt:.1f} s on 1 host thread; the scan is O(N) so vectors/s carries to 10M; gcc {flags}",
    }
    # the only parallelism a reference user could add without changing innr: one query per host core
    try:
        from concurrent.futures import ThreadPoolExecutor
        cores = min(len(os.sched_getaffinity(0)), 16)  # a 1-GPU box's CPU share is 16 cores whatever the affinity mask says
        if cores > 1:
            def one(j):
                knn(queries[j % len(queries)], data, k)  # ctypes releases the GIL
            t1 = time.perf_counter()
            jobs = 0
            with ThreadPoolExecutor(cores) as ex:
                while time.perf_counter() - t1 < 8.0:
                    list(ex.map(one, range(jobs, jobs + cores)))
                    jobs += cores
            dt2 = time.perf_counter() - t1
            out["all_host_cores"] = {"value": jobs * n / dt2, "unit": "vectors/s", "cores": cores,
                                     "sample": f"{jobs} queries, one per thread, {dt2:.1f} s"}
    except Exception as exc:  # the single-thread figure is the baseline; this row is extra
        out["all_host_cores"] = {"error": repr(exc)}
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir: str, idx, sc) -> None:
    """--dump-outputs: what the timed path returned in its last step, as DIR/indices.npy (float64: every index < 2^53 is exact)
    and DIR/scores.npy (float32), one row per query. Above DUMP_LIMIT_BYTES a fixed, seeded, sorted sample of query rows is
    written instead, with its row numbers in DIR/query_rows.npy."""
    import numpy as np
    idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).astype(np.float64)
    sc = np.asarray(sc.cpu() if hasattr(sc, "cpu") else sc).astype(np.float32)
    os.makedirs(out_dir, exist_ok=True)
    row_bytes = idx.shape[1] * 8 + sc.shape[1] * 4 + 8
    if idx.shape[0] * row_bytes > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(idx.shape[0], DUMP_LIMIT_BYTES // row_bytes, replace=False))
        idx, sc = idx[rows], sc[rows]
        np.save(os.path.join(out_dir, "query_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "indices.npy"), idx)
    np.save(os.path.join(out_dir, "scores.npy"), sc)


def pmc_traffic(args):
    """HBM-side bytes per GEMM launch from the committed rocprofv3 PMC passes of THIS command (profiles/, collected
    in separate --pmc runs: a counter pass cannot share a run with the timed region). FETCH_SIZE/WRITE_SIZE are in
    KB; on gfx950 FETCH_SIZE tallies 128-B requests at 64 B for wide streaming reads -> x2 (MI355X_MICROARCH.md,
    section HBM; calibrated here on norms_kernel: 1.50e7 KB reported for a 30.72 GB read)."""
    default = (args.n_per_gpu, args.dim, args.queries, args.k, args.metric) == (10_000_000, 768, 1024, 10, "dot")
    vals = {}
    rnd = next((r for r in ("r03", "r02", "r01") if os.path.exists(os.path.join(ROOT, "profiles", f"{r}_bench_n1_pmc_FETCH_SIZE.csv"))), "r01")
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
        path = os.path.join(ROOT, "profiles", f"{rnd}_bench_n1_pmc_{name}.csv")
        if not default or not os.path.exists(path):
            return {"traffic": None}
        for line in open(path):
            if "gemm_filter_kernel" in line and f",{name}," in line:
                vals[name] = float(line.rsplit(",", 1)[1])
    if len(vals) != 2:
        return {"traffic": None}
    rd, wr = vals["FETCH_SIZE"] * 1024.0 * 2.0, vals["WRITE_SIZE"] * 1024.0
    return {"traffic": rd + wr, "traffic_unit": "bytes per launch",
            "traffic_source": f"profiles/{rnd}" + "_bench_n1_pmc_{FETCH,WRITE}_SIZE.csv (FETCH_SIZE x2 gfx950 correction; "
                              "L2-miss side, Infinity-Cache hits included)",
            "algorithmic_bytes_per_launch": 4.0 * args.n_per_gpu * args.dim}


def rehearse_cpu(args) -> int:
    """--rehearse-cpu: the N-rank choreography of main() with a torch stand-in for the per-shard search (no HIP, no number)."""
    import torch
    import torch.distributed as dist
    from innr_amd.dist import ShardedKnn, shard_range
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    n_total = args.n_per_gpu * world
    start, count = shard_range(n_total, world, rank)
    g = torch.Generator().manual_seed(1234)
    corpus = torch.rand((n_total, args.dim), generator=g) * 2 - 1  # every rank draws the whole stream, keeps its range
    shard = corpus[start:start + count]
    queries = torch.rand((args.queries, args.dim), generator=torch.Generator().manual_seed(99)) * 2 - 1

    def local_search(q, k, stats=None):
        sc, idx = torch.topk(q @ shard.T, min(k, count), dim=1)
        return idx.to(torch.int64) + start, sc

    def merge(all_idx, all_sc, kout):  # [G, Q, kin] -> best kout by (score desc, global index asc)
        gq = all_idx.permute(1, 0, 2).reshape(all_idx.shape[1], -1)
        sq = all_sc.permute(1, 0, 2).reshape(all_sc.shape[1], -1).clone()
        sq[gq < 0] = float("-inf")  # a shard with fewer than k vectors pads its block (INVALID_INDEX)
        order = torch.argsort(gq, dim=1, stable=True)
        gq, sq = torch.gather(gq, 1, order), torch.gather(sq, 1, order)
        o2 = torch.argsort(sq, dim=1, descending=True, stable=True)[:, :kout]
        return torch.gather(gq, 1, o2), torch.gather(sq, 1, o2)

    sk = ShardedKnn(n_total, rank=rank, world=world, local_search=local_search, merge=merge) if world > 1 else None
    step = (lambda: sk.search(queries, args.k)) if sk is not None else (lambda: local_search(queries, args.k))
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        idx, sc = step()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    want_sc, want_idx = torch.topk(queries @ corpus.T, min(args.k, n_total), dim=1)
    same = bool(torch.equal(idx, want_idx.to(torch.int64)))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, idx, sc)
    if rank == 0:
        print(json.dumps({"metric": "vectors scanned/sec (batch_knn_dot f32 d=768 k=10)", "value": None, "unit": "vectors/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "synthetic", "rehearsal": "cpu: torch stand-in engine, gloo; plumbing only, nothing measured",
                          "sharded_result_equals_whole_corpus": same,
                          "config": {"workload": f"rehearsal {args.n_per_gpu}x{args.dim} per rank, {args.queries} queries, k={args.k}"}}),
              flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if same else 3


def self_launch(n: int) -> int:
    import socket
    import subprocess
    with socket.socket() as so:  # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this driver
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for out in proc.stdout:  # rank 0 prints ONE JSON line; anything else the ranks print goes to stderr
        if out.lstrip().startswith("{") and '"metric"' in out:
            line = out.strip()
        else:
            sys.stderr.write(out)
    rc = proc.wait()
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks exited without printing a result line\n")
        rc = 1
    if line is not None and rc == 0:
        print(line, flush=True)
    return rc


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-per-gpu", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", choices=["dot", "cosine"], default="dot")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the side rows and the CPU baseline (N = 1 "
                         "only); off by default, so a plain run does only set-up, warm-up, the timed steps and its outputs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-side-rows", action="store_true", help="with --full: skip the bf16 / int8 filter-engine and LCG-data side rows")
    ap.add_argument("--data", choices=["uniform", "lcg"], default="uniform",
                    help="uniform: i.i.d. uniform(-1,1), the distribution of the reference's criterion benches (default, the "
                         "judged row); lcg: the reference EXAMPLE's generator (examples/batch_demo.rs:233-242: corpus row i = "
                         "generate_embedding(dim, i), query j = generate_embedding(dim, N + j)), a one-parameter family with "
                         "tens of thousands of vectors within the f32 error bound of every k-th score -- the adversarial row: every "
                         "margin proof of the first pass fails and every query goes through the completion pass")
    ap.add_argument("--rehearse-cpu", action="store_true",
                    help="plumbing rehearsal WITHOUT a GPU (tests/test_bench_launch.py): launcher, rendezvous (gloo), the ranks' range "
                         "partition, ONE all-gather of the exchange blocks, merge, barrier / MAX timing and the JSON relay run as in "
                         "the real thing; the per-shard search is a torch.matmul stand-in on a small corpus, nothing is measured "
                         "(value = null) and no HIP code runs. Never a measurement path.")
    ap.add_argument("--engine", choices=["f32", "bf16", "i8"], default="f32",
                    help="f32: the MFMA GEMM filter on the f32 pipe (default, the judged configuration); bf16: the same "
                         "pipeline with the filter on the bf16 pipe (INNR_KNN_MFMA_BF16) -- identical results, reported "
                         "as a side measurement with its own roofline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the indices and scores the last timed step returned to DIR/*.npy "
                         "(rank 0; float64 indices, float32 scores, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` from a bare shell: start the N ranks ourselves -- one fresh process per GPU under
        # torch.distributed.run, BEFORE this process imports torch or touches a GPU -- relay rank 0's one JSON line and exit
        # with the launcher's code (non-zero if any rank failed).
        raise SystemExit(self_launch(args.gpus))

    import numpy as np

    if args.rehearse_cpu:
        raise SystemExit(rehearse_cpu(args))

    if args.full and not args.no_cpu_baseline and int(os.environ.get("RANK", "0")) == 0:
        import oracle
        oracle.lib()  # load (or, on a stale build, re-make) the CPU checker BEFORE this process touches the GPU: no exec after HIP init
        oracle.build_native()  # the same source compiled -march=native on THIS host, for the cpu_baseline leg

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("INNR_BENCH_ALL_ON_DEVICE0") == "1":  # rehearsal of the N > 1 path on a one-GPU box
        local_rank = 0
    if args.gpus != world and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("INNR_BENCH_BACKEND", "nccl")  # "gloo": rehearsal only (ranks sharing one GPU)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from innr_amd import KNN_MFMA, KNN_MFMA_BF16, KNN_MFMA_I8, METRIC_COSINE, METRIC_DOT, Context, KnnStats
    from innr_amd import batch as B
    from innr_amd.dist import Comm, ShardedKnn

    metric = METRIC_DOT if args.metric == "dot" else METRIC_COSINE
    engine = {"bf16": KNN_MFMA_BF16, "i8": KNN_MFMA_I8}.get(args.engine, KNN_MFMA)
    ctx = Context(local_rank)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)  # one stream for the kernels and the collective
    n_total = args.n_per_gpu * world
    # N > 1: the exchange step runs inside the library (innr_sharded_knn_dev: local search + pack + ONE ncclAllGather of
    # 8-byte entries + merge) on an RCCL communicator it owns; torch.distributed only carries the communicator id.
    # (A one-GPU rehearsal with gloo has no RCCL: the same blocks then travel through torch.distributed.all_gather.)
    comm, exchange = None, "none (1 GPU)"
    if world > 1 and dist.get_backend() == "nccl":
        err = ""
        try:
            comm = Comm.from_torch_group(ctx)
        except Exception as exc:  # no librccl / init failure on this rank
            err = repr(exc)
        ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)  # all ranks take the same path
        if int(ok.item()) == 1:
            exchange = "innr_sharded_knn_dev: ncclAllGather of 8-byte candidates on the library's own RCCL communicator"
        else:
            if comm is not None:
                comm.close()
            comm = None
            exchange = f"torch.distributed.all_gather of the same blocks (library communicator unavailable: {err or 'another rank failed'})"
    elif world > 1:
        exchange = "torch.distributed.all_gather of the same blocks through the host (gloo rehearsal)"
    sk = ShardedKnn(n_total, rank=rank, world=world, comm=comm) if world > 1 else None
    row0 = rank * args.n_per_gpu
    from innr_amd import GEN_EXAMPLE_LCG, GEN_UNIFORM
    gen = GEN_EXAMPLE_LCG if args.data == "lcg" else GEN_UNIFORM
    vb = B.VerticalBatch.generate(args.n_per_gpu, args.dim, seed=0, generator=gen, row0=row0, ctx=ctx)  # resident in HBM
    if sk is not None:
        sk.attach_gpu_batch(vb, metric, engine)
    # queries: rows of the same uniform stream under another seed, generated by the library on the device
    qb = (B.VerticalBatch.generate(args.queries, args.dim, seed=n_total, generator=gen, ctx=ctx) if args.data == "lcg"
          else B.VerticalBatch.generate(args.queries, args.dim, seed=0xBE7C, ctx=ctx))
    q_host = np.ascontiguousarray(np.asarray(qb.data(), dtype=np.float32).reshape(args.dim, args.queries).T)
    qb.close()
    q_dev = torch.from_numpy(q_host).to(dev)  # resident in HBM before the timed region

    from innr_amd.dist import _gpu_local_search
    local = _gpu_local_search(vb, metric, engine)
    gemm_ms, fallbacks, kept = [], [], 0

    def step():
        nonlocal kept
        st = KnnStats()
        out = sk.search(q_dev, args.k, st) if sk is not None else local(q_dev, args.k, st)
        gemm_ms.append(st.gemm_ms)
        fallbacks.append(st.queries_fallback)
        kept = st.candidates_kept
        return out

    for _ in range(args.warmup):
        step()
    gemm_ms.clear(); fallbacks.clear()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        idx, sc = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, idx, sc)

    if rank == 0:
        ms_per_step = dt / args.steps * 1e3
        value = args.queries * n_total / (dt / args.steps)
        g_ms = float(np.mean(gemm_ms))
        flop = 2.0 * args.queries * args.n_per_gpu * args.dim  # algorithmic flop of ONE launch (one GPU's shard)
        achieved = flop / (g_ms * 1e-3) / 1e12
        out = {
            "metric": "vectors scanned/sec (batch_knn_dot f32 d=768 k=10)" if args.metric == "dot"
                      else "vectors scanned/sec (batch_knn_cosine f32)",
            "value": value,
            "unit": "vectors/s",
            "qps": args.queries / (dt / args.steps),
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": ("synthetic: i.i.d. uniform(-1,1) f32 generated on device (distribution of the reference's "
                     "criterion benches, benches/batch.rs:11-21)") if args.data == "uniform" else
                    ("synthetic: the reference example's LCG generator (examples/batch_demo.rs:233-242), generated on "
                     "device: near-tie data, every query goes through the completion pass"),
            "config": {
                "workload": f"batch_knn_{args.metric} f32, {args.n_per_gpu}x{args.dim} corpus per GPU "
                            f"({n_total} total), {args.queries}-query batch, k={args.k}",
                "engine": {"f32": "f32 MFMA GEMM + fused top-k filter + exact re-score",
                           "bf16": "bf16 MFMA GEMM filter (K-packed bf16 corpus copy) + fused top-k filter + exact f32 re-score "
                                   "and proof: identical results",
                           "i8": "int8 MFMA GEMM filter (scalar-quantised K-packed corpus copy, 14-bit queries) + fused top-k filter + "
                                 "exact f32 re-score and proof: identical results"}[args.engine],
                "candidates_per_query": int(kept),
                "queries_redone_exactly_per_step": float(np.mean(fallbacks)),
                "parallelism": f"range-partitioned corpus x{world}, all-gather of per-shard top-k" if world > 1 else "1 GPU",
                "exchange": exchange,
            },
            "roofline": {
                "bound": "mfma",
                "kernel": {"f32": "gemm_filter_kernel (v_mfma_f32_32x32x2_f32)", "bf16": "gemm_bf16_filter_kernel (v_mfma_f32_32x32x16_bf16)",
                           "i8": "gemm_i8h_filter_kernel (v_mfma_i32_32x32x32_i8)"}[args.engine],
                "achieved": achieved,
                "peak": {"f32": PEAK_F32_MFMA_TFLOPS, "bf16": PEAK_BF16_MFMA_TFLOPS, "i8": 2 * PEAK_BF16_MFMA_TFLOPS}[args.engine],
                "unit": "TFLOP/s" if args.engine != "i8" else "TOP/s",
                "frac": achieved / {"f32": PEAK_F32_MFMA_TFLOPS, "bf16": PEAK_BF16_MFMA_TFLOPS, "i8": 2 * PEAK_BF16_MFMA_TFLOPS}[args.engine],
                "kernel_ms": g_ms,
                "algorithmic_flop_per_launch": flop,
                **(pmc_traffic(args) if args.engine == "f32" else {"traffic": None}),
            },
        }
        if args.full and world == 1 and args.engine == "f32" and args.data == "uniform" and not args.no_side_rows:
            # side rows (not `value`): the same call with the FILTER stage on a low-precision matrix pipe -- the bf16 copy
            # (INNR_KNN_MFMA_BF16, what INNR_KNN_AUTO picks for such a batch) and the scalar-quantised int8 copy
            # (INNR_KNN_MFMA_I8) -- each with a check that it returns the f32 engine's answer bit for bit
            f_idx, f_sc = idx.clone(), sc.clone()
            for key, eng, kname, peak in (("bf16_filter_engine", KNN_MFMA_BF16, "gemm_bf16_filter_kernel (v_mfma_f32_32x32x16_bf16)", PEAK_BF16_MFMA_TFLOPS),
                                          ("int8_filter_engine", KNN_MFMA_I8, "gemm_i8h_filter_kernel (v_mfma_i32_32x32x32_i8)", 2 * PEAK_BF16_MFMA_TFLOPS)):
                bl = _gpu_local_search(vb, metric, eng)
                st2 = KnnStats()
                bl(q_dev, args.k, st2)  # builds the K-packed corpus copy
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    st2 = KnnStats()
                    b_idx, b_sc = bl(q_dev, args.k, st2)
                torch.cuda.synchronize()
                dt2 = (time.perf_counter() - t1) / args.steps
                out[key] = {
                    "ms_per_step": dt2 * 1e3, "value": args.queries * n_total / dt2, "unit": "vectors/s", "kernel_ms": st2.gemm_ms,
                    "kernel": kname, "engine_ran": int(st2.engine),
                    "kernel_frac_of_pipe_peak": flop / (st2.gemm_ms * 1e-3) / 1e12 / peak if st2.gemm_ms > 0 else None,
                    "queries_redone": int(st2.queries_fallback), "candidates_per_query": int(st2.candidates_kept),
                    "identical_to_f32_engine": bool(torch.equal(f_idx, b_idx) and torch.equal(f_sc.view(torch.int32), b_sc.view(torch.int32))),
                }
        if args.full and world == 1 and args.engine == "f32" and args.data == "uniform" and not args.no_side_rows:
            # side row (not `value`): the same call on the reference EXAMPLE's generator (examples/batch_demo.rs:233-242, what
            # SURVEY 8d names) -- near-tie data on which every margin proof of the first pass fails (tens of thousands of vectors
            # within the f32 error bound of every k-th score); the step is then the GEMM pass + ONE completion pass (collect mode,
            # fixed thresholds) + the exact re-score of everything collected from the row-major copy
            vb.close()
            lvb = B.VerticalBatch.generate(args.n_per_gpu, args.dim, seed=0, generator=GEN_EXAMPLE_LCG, ctx=ctx)
            lqb = B.VerticalBatch.generate(args.queries, args.dim, seed=n_total, generator=GEN_EXAMPLE_LCG, ctx=ctx)
            lq = torch.from_numpy(np.ascontiguousarray(np.asarray(lqb.data(), dtype=np.float32).reshape(args.dim, args.queries).T)).to(dev)
            lqb.close()
            ll = _gpu_local_search(lvb, metric, KNN_MFMA)
            st3 = KnnStats()
            ll(lq, args.k, st3)  # builds the row-major copy the completion pass re-scores from
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            nl = 2
            for _ in range(nl):
                st3 = KnnStats()
                ll(lq, args.k, st3)
            torch.cuda.synchronize()
            dt3 = (time.perf_counter() - t2) / nl
            out["lcg_side_row"] = {"ms_per_step": dt3 * 1e3, "value": args.queries * n_total / dt3, "unit": "vectors/s", "steps": nl,
                                   "gemm_passes_ms": st3.gemm_ms, "queries_unproven_after_first_pass": int(st3.queries_fallback),
                                   "data": "reference example LCG generator (examples/batch_demo.rs:233-242), generated on device"}
            lvb.close()
        if args.data == "lcg":
            # every proof of the first pass fails on this data: the step is the GEMM pass + ONE completion pass (the same kernel in
            # collect mode, fixed thresholds) + the exact re-score of everything collected; kernel_ms above sums the two GEMM passes
            out["completion_pass"] = {"queries_unproven_after_first_pass": float(np.mean(fallbacks)), "gemm_passes_ms": g_ms,
                                      "rest_of_step_ms": max(ms_per_step - g_ms, 0.0),
                                      "note": "rest = seeding, select, re-score of the first pass; gather, exact re-score of the collected "
                                              "candidates from the row-major copy, radix select + sort of the second"}
            out["roofline"]["achieved"] = 2.0 * flop / (g_ms * 1e-3) / 1e12
            out["roofline"]["frac"] = out["roofline"]["achieved"] / PEAK_F32_MFMA_TFLOPS
            out["roofline"]["algorithmic_flop_per_launch"] = flop
            out["roofline"]["launches_per_step"] = 2
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.dim, args.k)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
