"""CPU-only checks of the boundary of the entry points that change a batch in place (append, update, keep): the six are declared
with the documented parameter names, exported, bound in Python and in the Rust shim; a null handle is refused before any device
call; mutate.o owns its two kernels alone; the Python and Rust mirrors have the documented shape."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")
PARAMS = {
    "innr_batch_append_rows": ["b", "rows", "n", "D"],
    "innr_batch_append_rows_dev": ["b", "d_rows", "n", "D"],
    "innr_batch_update_rows": ["b", "idx", "rows", "n", "D"],
    "innr_batch_update_rows_dev": ["b", "d_idx", "d_rows", "n", "D"],
    "innr_batch_keep_rows": ["b", "mask", "out_n"],
    "innr_batch_keep_rows_dev": ["b", "d_mask", "out_n"],
}
E_BAD_ARG = -2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_the_six_entry_points():
    raw = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for s, want in PARAMS.items():
        m = re.search(r"innr_status\s+%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, f"{s} not declared in include/innr_hip.h"
        names = [re.sub(r".*?(\w+)$", r"\1", a.strip()) for a in m.group(1).split(",")]
        assert names == want, (s, names)
    # the header comment in the house style: contract, order of the checks, memory, out of scope
    sec = raw[raw.index("changing a resident f32 batch in place"):raw.index("innr_batch_keep_rows_dev(")]
    for word in ("Order of the checks", "Out of scope", "INNR_E_DIM_MISMATCH", "INNR_E_UNSUPPORTED", "INNR_E_OOM", "prefix view",
                 "reserved capacity", "sharded", "256 MiB"):
        assert word in sec, word


def test_library_exports_and_binding_table_has_them(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    for s, want in PARAMS.items():
        assert hasattr(lib, s), f"{s} not exported"
        assert s in built.SIGNATURES, f"{s} not in SIGNATURES"
        assert len(built.SIGNATURES[s][1]) == len(want), s


def test_rust_ffi_binds_them():
    rs = open(SHIM).read()
    ffi = rs[rs.index("mod ffi"):]
    ffi = ffi[:ffi.index("\n}\n")]
    for s, want in PARAMS.items():
        m = re.search(r"pub fn %s\s*\(([^;]*)\)\s*->\s*c_int;" % s, ffi)
        assert m, f"{s} not bound in mod ffi"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(want), s
    impl = rs[rs.index("pub mod batch"):]
    # `&mut self`: a PrefixBatch borrows the batch, so the borrow checker keeps "no live view while the batch changes"
    assert re.search(r"pub fn append\(&mut self, rows: &\[f32\]\)", impl)
    assert re.search(r"pub fn update_rows\(&mut self, indices: &\[u64\], rows: &\[f32\]\)", impl)
    assert re.search(r"pub fn keep\(&mut self, mask: &\[u8\]\) -> usize", impl)
    for s in ("innr_batch_append_rows(", "innr_batch_update_rows(", "innr_batch_keep_rows("):
        assert "ffi::" + s in impl, s


def test_null_handle_is_bad_arg_without_a_gpu(built):
    lib = built.load()
    buf = (ctypes.c_float * 4)()
    idx = (ctypes.c_uint64 * 1)()
    mask = (ctypes.c_uint8 * 1)()
    n = ctypes.c_size_t(7)
    for fn in (lib.innr_batch_append_rows, lib.innr_batch_append_rows_dev):
        assert fn(None, buf, 1, 4) == E_BAD_ARG and "null" in built.last_error()
    for fn in (lib.innr_batch_update_rows, lib.innr_batch_update_rows_dev):
        assert fn(None, idx, buf, 1, 4) == E_BAD_ARG and "null" in built.last_error()
    for fn in (lib.innr_batch_keep_rows, lib.innr_batch_keep_rows_dev):
        assert fn(None, mask, ctypes.byref(n)) == E_BAD_ARG and "null" in built.last_error()
        assert fn(None, mask, None) == E_BAD_ARG
    assert n.value == 7  # a refused call writes nothing


def test_python_mirror_signatures():
    from innr_amd import batch as B
    vb = B.VerticalBatch
    assert list(inspect.signature(vb.append).parameters) == ["self", "rows"]
    assert list(inspect.signature(vb.update_rows).parameters) == ["self", "indices", "rows"]
    assert list(inspect.signature(vb.keep).parameters) == ["self", "mask"]
    assert list(inspect.signature(vb.remove).parameters) == ["self", "indices"]
    for fn in (vb.append, vb.update_rows, vb.keep):
        src = inspect.getsource(fn)
        assert "self._before_change(" in src and "self._changed()" in src and "bind_torch_stream()" in src, fn.__name__
    assert "self._host = None" in inspect.getsource(vb._changed)
    assert "_views" in inspect.getsource(vb._before_change)


def test_mutate_object_owns_its_kernels_alone(built):
    """tests/test_abi.py's one-owner rule, for the new object: the scatter and the validation kernel, nothing else, shared with
    no other object"""
    libdir = os.path.dirname(built.LIB_PATH)
    objs = {o: os.path.join(libdir, o) for o in ("mutate.o", "rows.o", "adaptive.o", "api.o", "maxsim.o", "comm.o", "sort_full.o")}
    if not all(os.path.exists(p) for p in objs.values()):
        pytest.skip("build-box check (the object files are not shipped to the GPU box)")
    stubs = {}
    for o, p in objs.items():
        out = subprocess.run(["nm", "--defined-only", p], capture_output=True, text=True, check=True).stdout
        stubs[o] = set(l.split()[-1] for l in out.splitlines() if "__device_stub__" in l)
    assert len(stubs["mutate.o"]) == 2, stubs["mutate.o"]
    assert all(("scatter_rows_pdx" in s) or ("update_check" in s) for s in stubs["mutate.o"]), stubs["mutate.o"]
    for o in objs:
        if o != "mutate.o":
            assert not (stubs["mutate.o"] & stubs[o]), (o, stubs["mutate.o"] & stubs[o])
