"""One communicator serving a large shard and then a small one (innr_sharded_knn_dev): the shard total cached from the first
exchange is larger than the truth on the second call. The result buffers hold Q * min(k, true total) entries, as the header
documents, and nothing may be written past them. The buffers here are the front of larger tensors filled with a sentinel: an
overrun shows as a changed sentinel instead of a stray write into somebody else's memory."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle


def test_cached_total_of_a_larger_shard_does_not_overrun_the_result():
    import torch
    import innr_amd
    from innr_amd import batch as B
    from innr_amd._lib import check, load
    from innr_amd.dist import Comm, ShardedKnn

    ctx = innr_amd.Context(0)
    dev = torch.device("cuda", 0)
    comm = Comm(ctx, 0, 1, Comm.unique_id())
    n, small_n, dim, nq, k = 3_000, 5, 40, 37, 9
    queries = oracle.generate_uniform(nq, dim, 99)
    q_dev = torch.from_numpy(queries).to(dev)
    big = B.VerticalBatch.generate(n, dim, seed=7, row0=0, ctx=ctx)
    sk = ShardedKnn(n, rank=0, world=1, comm=comm)
    sk.attach_gpu_batch(big, innr_amd.METRIC_DOT)
    idx, _ = sk.search(q_dev, k)  # the communicator learns total = 3000
    assert idx.shape == (nq, k)

    small = B.VerticalBatch.generate(small_n, dim, seed=7, row0=0, ctx=ctx)
    want_i, want_s = B.knn_multi(innr_amd.METRIC_DOT, queries, small, k, engine=innr_amd.KNN_EXACT)
    assert want_i.shape == (nq, small_n)
    room, sentinel = nq * k, -7
    out_i = torch.full((room,), sentinel, dtype=torch.int64, device=dev)
    out_s = torch.full((room,), float(sentinel), dtype=torch.float32, device=dev)
    out_k = C.c_size_t(0)
    ctx.bind_torch_stream()
    check(load().innr_sharded_knn_dev(comm._h, small._h, innr_amd.METRIC_DOT, C.c_void_p(q_dev.data_ptr()), nq, dim, k,
                                      innr_amd.KNN_EXACT, C.c_void_p(out_i.data_ptr()), C.c_void_p(out_s.data_ptr()),
                                      C.byref(out_k), None))
    torch.cuda.synchronize()
    assert out_k.value == small_n
    used = nq * small_n  # what a caller allocates: Q * min(k, total vectors)
    got_i, got_s = out_i.cpu().numpy(), out_s.cpu().numpy()
    assert np.array_equal(got_i[:used].reshape(nq, small_n), want_i.astype(np.int64))
    assert np.array_equal(got_s[:used].view(np.uint32), np.ascontiguousarray(want_s).reshape(-1).view(np.uint32))
    assert np.all(got_i[used:] == sentinel) and np.all(got_s[used:] == float(sentinel)), "written past Q * min(k, total) entries"
    # and back to the large shard: the total is learnt again
    idx2, _ = sk.search(q_dev, k)
    assert torch.equal(idx2, idx)
    for o in (small, big):
        o.close()
