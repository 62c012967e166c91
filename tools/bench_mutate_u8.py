"""Changing a resident u8 code batch in place (innr_batch_append_codes_dev, innr_batch_update_codes_dev,
innr_batch_append_quantized_dev) at 10M x 128, against the only alternative there was before: a fresh
innr_batch_upload_u8 of the final corpus from host memory (and, for f32 rows, innr_quantize_u8 on the host in front of it).

    python tools/bench_mutate_u8.py [N] [D]  > profiles/mutate_u8_<shape>.txt

Random codes made on the host (the yardstick needs them there). One process; the library runs on torch's current stream. Every
entry point timed here synchronises with the host, so a figure is host wall time around the call, the stream drained before it
starts: what a caller waits for. One warm-up, then REPS repeats of (the new call, the yardstick) in turn; printed: median
(min .. max) of each and the bytes the case moves. The yardstick's figure leaves out freeing the old handle.
  append  in place: the padding of a code store is less than 1024 columns by construction (no reserved capacity), so the in-place
          case appends 25 rows at a time into the 1023 free columns of a batch of N - N % 1024 + 1 vectors -- the call's fixed
          cost; reallocating: 10 000 rows, every repeat (the store grows by 10 000 each time and is copied once per call).
  update  10 000 scattered (random, distinct) and 10 000 consecutive indices.
  quantised append: the same two appends fed f32 rows on the device."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from innr_amd import _lib
from innr_amd import scalar as S

args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 10_000_000
dim = int(args[1]) if len(args) > 1 else 128
reps = int(os.environ.get("REPS", "9"))
m = 10_000
alpha, offset = 2.0, -1.0

ctx = _lib.default_context()
ctx.bind_torch_stream()
lib = _lib.load()
dpad = (dim + 31) // 32 * 32
params = S.QuantizationParams(alpha, offset)


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


def hptr(a):
    return C.c_void_p(a.ctypes.data)


def fresh_upload(n_rows, rows_f32=None):
    """the yardstick: the final corpus of n_rows codes from host memory into a new batch (freed outside the timing); with
    rows_f32, their quantisation on the host into the tail of the host codes first"""
    h = C.c_void_p()

    def call():
        if rows_f32 is not None:
            k = rows_f32.shape[0]
            lib.innr_quantize_u8(hptr(rows_f32), rows_f32.size, C.c_float(alpha), C.c_float(offset), hptr(host[n_rows - k:n_rows]))
        return lib.innr_batch_upload_u8(ctx.handle, hptr(host), n_rows, dim, C.c_float(alpha), C.c_float(offset), C.byref(h))

    ms = timed(call)
    lib.innr_batch_free(h)
    return ms


def alternate(new_call, yardstick):
    a, b = [], []
    for it in range(reps + 1):
        x, y = timed(new_call), yardstick()
        if it:
            a.append(x)
            b.append(y)
    return a, b


print(f"# {n} x {dim} u8 codes, one MI355X, ONE run; host wall time, ms = median (min .. max) of {reps} repeats after one warm-up;"
      f" 'fresh' = innr_batch_upload_u8 of the final corpus from pageable host memory, measured in turn with the new call")
# room for every append of this run
host = np.random.default_rng(0).integers(0, 256, (n + 4 * (reps + 1) * m + 1024, dim), dtype=np.uint8)
new = torch.randint(0, 256, (m, dim), dtype=torch.uint8, device="cuda")
new_f32 = torch.rand((m, dim), dtype=torch.float32, device="cuda") * 2.0 - 1.0
new_f32_host = new_f32.cpu().numpy()

# ---- append, in place: codes, then f32 rows
n_in = n - n % 1024 + 1
for what, fn, rows, hrows in (("append   ", lib.innr_batch_append_codes_dev, new, None),
                              ("append q.", lib.innr_batch_append_quantized_dev, new_f32, new_f32_host[:25])):
    qc = S.QuantizedCorpus.from_codes(host[:n_in], n_in, dim, params)
    ld0 = qc.memory().corpus_bytes
    ts, ys = alternate(lambda: fn(qc._h, ptr(rows), 25, dim),
                       lambda: fresh_upload(int(lib.innr_batch_num_vectors(qc._h)), hrows))
    assert qc.memory().corpus_bytes == ld0  # every repeat stayed in place
    src = 25 * dim * (4 if hrows is not None else 1)
    print(f"  {what} 25 rows in place (N = {n_in})          {fmt(ts)}   {src} bytes read, {25 * dim} written"
          f"   | fresh {fmt(ys)}   {n_in * dim / 1e9:.2f} GB over the host link", flush=True)
    qc.close()

# ---- append, reallocating: codes, then f32 rows
for what, fn, rows, hrows in (("append   ", lib.innr_batch_append_codes_dev, new, None),
                              ("append q.", lib.innr_batch_append_quantized_dev, new_f32, new_f32_host)):
    qc = S.QuantizedCorpus.from_codes(host[:n], n, dim, params)
    n_last = n + reps * m
    moved = ((n_last + m + 1023) // 1024 * 1024) * dpad + 2 * n_last * dim + 2 * m * dim  # zeroing, the old block read and written, the rows
    ts, ys = alternate(lambda: fn(qc._h, ptr(rows), m, dim),
                       lambda: fresh_upload(int(lib.innr_batch_num_vectors(qc._h)), hrows))
    print(f"  {what} {m} rows reallocating (N = {n} ..) {fmt(ts)}   {moved / 1e9:.2f} GB moved on the device, "
          f"{moved / statistics.median(ts) / 1e9:.2f} TB/s   | fresh {fmt(ys)}   {n_last * dim / 1e9:.2f} GB over the host link", flush=True)
    if hrows is None:
        qc._changed()
        keep = qc
    else:
        qc.close()
qc = keep
n_now = len(qc)

# ---- update
lists = {"scattered": torch.from_numpy(np.random.default_rng(1).choice(n_now, m, replace=False).astype(np.int64)).cuda(),
         "consecutive": torch.arange(n_now // 2, n_now // 2 + m, dtype=torch.int64, device="cuda")}
for name, ids in lists.items():
    ts, ys = alternate(lambda: lib.innr_batch_update_codes_dev(qc._h, ptr(ids), ptr(new), m, dim), lambda: fresh_upload(n_now))
    print(f"  update    {m} {name:>11} codes                {fmt(ts)}   {m * dim} bytes read, as many written "
          f"({'one byte per cache line' if name == 'scattered' else 'runs of a dimension row, byte stores'})"
          f"   | fresh {fmt(ys)}   {n_now * dim / 1e9:.2f} GB over the host link", flush=True)
idx, _ = qc.knn_multi(np.where(new_f32_host[:4] > 0, 1.0, -1.0).astype(np.float32), 1)  # (the calls still answer)
assert idx.shape == (4, 1)
qc.close()
