"""Changing a resident batch in place (innr_batch_append_rows_dev, innr_batch_update_rows_dev) at 10M x 128.

    python tools/bench_mutate.py [N] [D]  > profiles/mutate_<shape>.txt

Uniform corpus generated on the device. One process; the library runs on torch's current stream. Every entry point timed here
synchronises with the host (the allocation, the check's flag), so a figure is host wall time around the call, the stream drained
before it starts: what a caller waits for. One warm-up, then REPS repeats; printed: median (min .. max) and the bytes the case moves.
  append  in place: the padding of a store is less than 256 columns by construction (no reserved capacity), so the in-place case
          appends 25 rows at a time into the 255 free columns of a batch of N - N % 256 + 1 vectors -- the call's fixed cost;
          reallocating: 10 000 rows, every repeat (the store grows by 10 000 each time and is copied once per call).
  update  10 000 scattered (random, distinct) and 10 000 consecutive indices."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import _lib
from innr_amd import batch as B

args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 10_000_000
dim = int(args[1]) if len(args) > 1 else 128
reps = int(os.environ.get("REPS", "9"))
m = 10_000

ctx = _lib.default_context()
ctx.bind_torch_stream()
lib = _lib.load()
dpad = (dim + 31) // 32 * 32


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = fn()
    torch.cuda.synchronize()
    assert st == 0, _lib.last_error()
    return 1e3 * (time.perf_counter() - t0)


def fmt(ts):
    return f"{statistics.median(ts):>9.3f} ({min(ts):.3f} .. {max(ts):.3f})"


def ptr(t):
    return C.c_void_p(t.data_ptr())


print(f"# {n} x {dim} f32 uniform generated on the device, one MI355X; host wall time, ms = median (min .. max) of {reps} repeats "
      f"after one warm-up")
new = torch.rand((m, dim), dtype=torch.float32, device="cuda")

# ---- append, in place
n_in = n - n % 256 + 1
vb = B.VerticalBatch.generate(n_in, dim, 0)
ts = []
for it in range(reps + 1):
    ms = timed(lambda: lib.innr_batch_append_rows_dev(vb._h, ptr(new), 25, dim))
    if it:
        ts.append(ms)
print(f"  append   25 rows in place (N = {n_in})            {fmt(ts)}   {25 * dim * 4} bytes read, as many written")
vb.close()

# ---- append, reallocating
vb = B.VerticalBatch.generate(n, dim, 0)
ts, moved = [], 0
for it in range(reps + 1):
    n_now = int(lib.innr_batch_num_vectors(vb._h))
    ld_new = (n_now + m + 255) // 256 * 256
    moved = ld_new * dpad * 4 + 2 * n_now * dim * 4 + 2 * m * dim * 4  # zeroing, the old block read and written, the rows read and written
    ms = timed(lambda: lib.innr_batch_append_rows_dev(vb._h, ptr(new), m, dim))
    if it:
        ts.append(ms)
print(f"  append   {m} rows reallocating (N = {n} ..)   {fmt(ts)}   {moved / 1e9:.2f} GB moved, "
      f"{moved / statistics.median(ts) / 1e9:.2f} TB/s")
vb._changed()
n_now = vb.num_vectors()

# ---- update
lists = {"scattered": torch.from_numpy(np.random.default_rng(1).choice(n_now, m, replace=False).astype(np.int64)).cuda(),
         "consecutive": torch.arange(n_now // 2, n_now // 2 + m, dtype=torch.int64, device="cuda")}
for name, ids in lists.items():
    ts = []
    for it in range(reps + 1):
        ms = timed(lambda: lib.innr_batch_update_rows_dev(vb._h, ptr(ids), ptr(new), m, dim))
        if it:
            ts.append(ms)
    print(f"  update   {m} {name:>11} rows                  {fmt(ts)}   {m * dim * 4} bytes read, as many written "
          f"({'one 4-byte word per cache line' if name == 'scattered' else 'whole lines of a dimension row'})", flush=True)
assert np.array_equal(vb.rows(lists["scattered"][:8]).cpu().numpy().view(np.uint32), new[:8].cpu().numpy().view(np.uint32))
vb.close()
