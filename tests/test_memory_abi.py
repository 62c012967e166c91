"""ABI of the memory entry points (innr_batch_memory, _copy_bytes, _release_copies, _build_copies, _set / _get_copy_budget,
innr_docs_memory, innr_ctx_memory, innr_ctx_trim): declared in the header, exported by the built product library, bound by
innr_amd/_lib.py and by the Rust shim (the `mod ffi` block and a safe wrapper each); the INNR_COPY_* bits agree between the
header, Python and Rust; a null handle is INNR_E_BAD_ARG before anything touches a device. CPU only."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")

SYMBOLS = ["innr_batch_memory", "innr_batch_copy_bytes", "innr_batch_release_copies", "innr_batch_build_copies",
           "innr_batch_set_copy_budget", "innr_batch_get_copy_budget", "innr_docs_memory", "innr_ctx_memory", "innr_ctx_trim"]
KINDS = ["ROWS", "BF16_DOT", "BF16_COS", "BF16_L2", "BF16LO_DOT", "BF16LO_COS", "I8_DOT", "I8_COS", "I8_L2", "SELECTION"]


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _header_masks():
    """name -> value of every `#define INNR_COPY_<NAME> <1u << n | hex | decimal>` of the header"""
    out = {}
    for name, expr in re.findall(r"^#define\s+INNR_COPY_(\w+)\s+(.+?)\s*$", _header_code(), flags=re.M):
        expr = expr.strip("()")
        m = re.fullmatch(r"1u\s*<<\s*(\d+)", expr)
        out[name] = 1 << int(m.group(1)) if m else int(expr.rstrip("uU"), 0)
    return out


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_the_symbols():
    hdr = _header_code()
    for s in SYMBOLS:
        assert re.search(r"innr_status\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/innr_hip.h"
    # the report takes const handles: it changes nothing
    assert re.search(r"innr_batch_memory\s*\(\s*const innr_batch\*", hdr) and re.search(r"innr_docs_memory\s*\(\s*const innr_docs\*", hdr)


def test_mask_bits_are_distinct_and_all_covers_them():
    masks = _header_masks()
    assert sorted(masks) == sorted(KINDS + ["ALL"]), sorted(masks)
    bits = [masks[k] for k in KINDS]
    assert all(b and b & (b - 1) == 0 for b in bits), "one bit per kind"
    assert len(set(bits)) == len(bits)
    union = 0
    for b in bits:
        union |= b
    assert masks["ALL"] == union


def test_python_constants_equal_the_header():
    import innr_amd
    from innr_amd import _lib
    for name, value in _header_masks().items():
        assert getattr(_lib, "COPY_" + name) == value, name
        assert getattr(innr_amd, "COPY_" + name) == value, name
    assert _lib.COPY_BUDGET_UNLIMITED == 2 ** 64 - 1


def test_rust_constants_equal_the_header():
    src = open(SHIM).read()
    for name, value in _header_masks().items():
        m = re.search(r"pub const INNR_COPY_" + name + r": u32 = ([^;]+);", src)
        assert m, f"INNR_COPY_{name} missing from the Rust shim"
        expr = m.group(1).strip()
        mm = re.fullmatch(r"1\s*<<\s*(\d+)", expr)
        assert (1 << int(mm.group(1)) if mm else int(expr, 0)) == value, name


def test_library_exports_and_binding_table(built):
    lib = C.CDLL(built.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), f"{s} not exported by {built.LIB_PATH}"
        res, args = built.SIGNATURES[s]
        assert res is C.c_int and args[0] is C.c_void_p, s
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    assert list(built.SIGNATURES["innr_batch_memory"][1]) == [C.c_void_p, u64p, u64p, u64p, u32p]
    assert list(built.SIGNATURES["innr_batch_set_copy_budget"][1]) == [C.c_void_p, C.c_uint64]
    assert list(built.SIGNATURES["innr_batch_build_copies"][1]) == [C.c_void_p, C.c_uint32, u32p]


def test_null_handles_are_bad_arg_without_a_gpu(built):
    """every entry point checks its handle before it binds a device: the answer is the same with and without a GPU"""
    L = built.load()
    v64, v32 = C.c_uint64(7), C.c_uint32(7)
    calls = [
        L.innr_batch_memory(None, C.byref(v64), C.byref(v64), C.byref(v64), C.byref(v32)),
        L.innr_batch_memory(None, None, None, None, None),
        L.innr_batch_copy_bytes(None, built.COPY_ALL, C.byref(v64)),
        L.innr_batch_release_copies(None, built.COPY_ALL),
        L.innr_batch_build_copies(None, built.COPY_ALL, C.byref(v32)),
        L.innr_batch_build_copies(None, built.COPY_ALL, None),
        L.innr_batch_set_copy_budget(None, 0),
        L.innr_batch_get_copy_budget(None, C.byref(v64)),
        L.innr_docs_memory(None, C.byref(v64), C.byref(v64)),
        L.innr_ctx_memory(None, C.byref(v64)),
        L.innr_ctx_trim(None),
    ]
    assert calls == [built.E_BAD_ARG] * len(calls), calls
    assert "null" in built.last_error()


def test_python_surface():
    from innr_amd import _lib, batch, maxsim, scalar
    for cls in (batch.VerticalBatch, scalar.QuantizedCorpus):
        for name in ("memory", "copy_bytes", "release_copies", "build_copies"):
            assert callable(getattr(cls, name)), (cls, name)
        assert isinstance(cls.copy_budget, property) and cls.copy_budget.fset is not None
    assert callable(maxsim.DocumentCorpus.memory) and callable(_lib.Context.memory) and callable(_lib.Context.trim)
    assert _lib.BatchMemory._fields == ("corpus_bytes", "aux_bytes", "derived_bytes", "present_mask")
    assert _lib.DocsMemory._fields == ("corpus_bytes", "derived_bytes")


def test_rust_shim_binds_and_wraps_every_symbol():
    src = open(SHIM).read()
    ffi = src[src.index("mod ffi"):]
    ffi, rest = ffi[:ffi.index("\n}\n") + 3], ffi[ffi.index("\n}\n") + 3:]
    for s in SYMBOLS:
        assert re.search(r"pub fn " + s + r"\(", ffi), f"{s} missing from mod ffi (regenerate with tools/gen_rust_ffi.py --write)"
        assert "ffi::" + s + "(" in rest, f"no safe wrapper calls ffi::{s}"
    for mod, end in (("pub mod batch", "pub mod scalar"), ("pub mod scalar", "pub mod maxsim")):
        body = src[src.index(mod):src.index(end)]
        for fn in ("memory", "copy_bytes", "release_copies", "build_copies", "set_copy_budget", "copy_budget"):
            assert re.search(r"pub fn " + fn + r"\(&self", body), (mod, fn)
    body = src[src.index("pub mod maxsim"):src.index("pub mod distance")]
    assert re.search(r"pub fn memory\(&self", body)
