"""CPU-only checks of the boundary of the entry points that change a u8 code batch in place (append, update, keep, and the variants
fed f32 rows): the ten are declared with the documented parameter names, exported, bound in Python and in the Rust
shim; a null handle is refused before any device call; mutate_u8.o owns its two kernels alone and mutate.o still owns exactly its
two; the Python and Rust mirrors have the documented shape."""
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
    "innr_batch_append_codes": ["b", "codes", "n", "D"],
    "innr_batch_append_codes_dev": ["b", "d_codes", "n", "D"],
    "innr_batch_update_codes": ["b", "idx", "codes", "n", "D"],
    "innr_batch_update_codes_dev": ["b", "d_idx", "d_codes", "n", "D"],
    "innr_batch_keep_codes": ["b", "mask", "out_n"],
    "innr_batch_keep_codes_dev": ["b", "d_mask", "out_n"],
    "innr_batch_append_quantized": ["b", "rows", "n", "D"],
    "innr_batch_append_quantized_dev": ["b", "d_rows", "n", "D"],
    "innr_batch_update_quantized": ["b", "idx", "rows", "n", "D"],
    "innr_batch_update_quantized_dev": ["b", "d_idx", "d_rows", "n", "D"],
}
E_BAD_ARG = -2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_the_ten_entry_points():
    raw = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for s, want in PARAMS.items():
        m = re.search(r"innr_status\s+%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, f"{s} not declared in include/innr_hip.h"
        names = [re.sub(r".*?(\w+)$", r"\1", a.strip()) for a in m.group(1).split(",")]
        assert names == want, (s, names)
    # after the f32 section, with a header comment in the house style: contract, order of the checks, memory, out of scope
    assert raw.index("innr_batch_keep_rows_dev(") < raw.index("changing a resident u8 code batch in place")
    sec = raw[raw.index("changing a resident u8 code batch in place"):raw.index("innr_batch_update_quantized_dev(")]
    for word in ("Order of the checks", "Out of scope", "Memory", "INNR_E_DIM_MISMATCH", "INNR_E_UNSUPPORTED", "INNR_E_OOM",
                 "prefix view", "reserved capacity", "int8 copy", "re-fitting", "document corpora", "sharded", "through a view",
                 "atomicity", "256 MiB", "mutate_round", "single-byte", "half away from zero", "DESIGN.md 4.5h"):
        assert word in sec, word
    # the f32 section's "Out of scope" points here
    f32 = raw[raw.index("changing a resident f32 batch in place"):raw.index("innr_batch_keep_rows_dev(")]
    assert "innr_batch_append_codes" in f32


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
    impl = rs[rs.index("pub mod scalar"):]
    impl = impl[:impl.index("pub mod maxsim")]
    # `&mut self`, for the reason tests/test_mutate_abi.py gives for the f32 batch: nothing that borrows the corpus is alive
    assert re.search(r"pub fn append_codes\(&mut self, codes: &\[u8\]\)", impl)
    assert re.search(r"pub fn append\(&mut self, rows: &\[f32\]\)", impl)
    assert re.search(r"pub fn update_codes\(&mut self, indices: &\[u64\], codes: &\[u8\]\)", impl)
    assert re.search(r"pub fn update_rows\(&mut self, indices: &\[u64\], rows: &\[f32\]\)", impl)
    assert re.search(r"pub fn keep\(&mut self, mask: &\[u8\]\) -> usize", impl)
    for s in ("innr_batch_append_codes(", "innr_batch_append_quantized(", "innr_batch_update_codes(", "innr_batch_update_quantized(",
              "innr_batch_keep_codes("):
        assert "ffi::" + s in impl, s


def test_null_handle_is_bad_arg_without_a_gpu(built):
    lib = built.load()
    rows = (ctypes.c_float * 4)()
    codes = (ctypes.c_uint8 * 4)()
    idx = (ctypes.c_uint64 * 1)()
    mask = (ctypes.c_uint8 * 1)()
    n = ctypes.c_size_t(7)
    for fn, buf in ((lib.innr_batch_append_codes, codes), (lib.innr_batch_append_codes_dev, codes),
                    (lib.innr_batch_append_quantized, rows), (lib.innr_batch_append_quantized_dev, rows)):
        assert fn(None, buf, 1, 4) == E_BAD_ARG and "null" in built.last_error()
    for fn, buf in ((lib.innr_batch_update_codes, codes), (lib.innr_batch_update_codes_dev, codes),
                    (lib.innr_batch_update_quantized, rows), (lib.innr_batch_update_quantized_dev, rows)):
        assert fn(None, idx, buf, 1, 4) == E_BAD_ARG and "null" in built.last_error()
    for fn in (lib.innr_batch_keep_codes, lib.innr_batch_keep_codes_dev):
        assert fn(None, mask, ctypes.byref(n)) == E_BAD_ARG and "null" in built.last_error()
        assert fn(None, mask, None) == E_BAD_ARG
    assert n.value == 7  # a refused call writes nothing


def test_python_mirror_signatures():
    from innr_amd import scalar as S
    qc = S.QuantizedCorpus
    assert list(inspect.signature(qc.append_codes).parameters) == ["self", "codes"]
    assert list(inspect.signature(qc.append).parameters) == ["self", "rows"]
    assert list(inspect.signature(qc.update_codes).parameters) == ["self", "indices", "codes"]
    assert list(inspect.signature(qc.update_rows).parameters) == ["self", "indices", "rows"]
    assert list(inspect.signature(qc.keep).parameters) == ["self", "mask"]
    assert list(inspect.signature(qc.remove).parameters) == ["self", "indices"]
    for fn in (qc._append, qc._update, qc.keep):  # what the five public methods run through
        src = inspect.getsource(fn)
        assert "self._before_change(" in src and "self._changed()" in src and "bind_torch_stream()" in src, fn.__name__
    assert "innr_batch_num_vectors" in inspect.getsource(qc._changed)
    assert "_views" in inspect.getsource(qc._before_change)
    assert "self._base = int(base)" in inspect.getsource(qc.set_index_base)  # remove() works on global indices


def test_mutate_objects_own_their_kernels_alone(built):
    """tests/test_abi.py's one-owner rule, for the new object: the byte scatter and the row quantiser, nothing else, shared with no
    other object -- the kernels it borrows (the u8 transpose, the selection's count and gather, the index validation) stay with
    api.o and mutate.o, which still owns exactly its two"""
    libdir = os.path.dirname(built.LIB_PATH)
    objs = {o: os.path.join(libdir, o)
            for o in ("mutate_u8.o", "mutate.o", "rows.o", "adaptive.o", "api.o", "maxsim.o", "comm.o", "sort_full.o")}
    if not all(os.path.exists(p) for p in objs.values()):
        pytest.skip("build-box check (the object files are not shipped to the GPU box)")
    stubs = {}
    for o, p in objs.items():
        out = subprocess.run(["nm", "--defined-only", p], capture_output=True, text=True, check=True).stdout
        stubs[o] = set(l.split()[-1] for l in out.splitlines() if "__device_stub__" in l)
    mine = stubs["mutate_u8.o"]
    assert len(mine) == 2, mine
    assert any("scatter_rows_u8_pdx_kernel" in s for s in mine) and any("quantize_rows_u8_kernel" in s for s in mine), mine
    for o in objs:
        if o != "mutate_u8.o":
            assert not (mine & stubs[o]), (o, mine & stubs[o])
    assert len(stubs["mutate.o"]) == 2, stubs["mutate.o"]
    assert all(("scatter_rows_pdx" in s) or ("update_check" in s) for s in stubs["mutate.o"]), stubs["mutate.o"]
