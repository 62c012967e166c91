"""ABI of the maxsim re-rank (innr_maxsim_rerank / innr_maxsim_rerank_dev): declared in the header with the documented parameter
lists, exported by the built product library, bound by innr_amd/_lib.py and by the Rust shim's `mod ffi`, and reachable as
DocumentCorpus.rerank. CPU only."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")

# (C type, name) per parameter, as the header documents them
HOST = [("innr_docs*", "d"), ("int", "cosine"), ("const float*", "qtoks"), ("size_t", "Q"), ("const uint32_t*", "tq"),
        ("size_t", "Tq_stride"), ("size_t", "dim"), ("const uint64_t*", "cand"), ("size_t", "kc"), ("size_t", "k"),
        ("uint64_t*", "out_doc"), ("float*", "out_score"), ("size_t*", "out_k")]
DEV = [(t, {"qtoks": "d_qtoks", "cand": "d_cand", "out_doc": "d_out_doc", "out_score": "d_out_score"}.get(n, n)) for t, n in HOST]
RUST = ["*mut InnrDocs", "c_int", "*const f32", "usize", "*const u32", "usize", "usize", "*const u64", "usize", "usize", "*mut u64",
        "*mut f32", "*mut usize"]


def _prototype(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"innr_status\s+" + name + r"\s*\(([^;{]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/innr_hip.h"
    params = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        mm = re.match(r"(.*?)(\w+)$", a)
        params.append((mm.group(1).replace(" *", "*").strip(), mm.group(2)))
    return params


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


@pytest.mark.parametrize("name,want", [("innr_maxsim_rerank", HOST), ("innr_maxsim_rerank_dev", DEV)])
def test_header_declares_the_documented_parameter_lists(name, want):
    assert _prototype(name) == want


def test_product_library_exports_both(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    for s in ("innr_maxsim_rerank", "innr_maxsim_rerank_dev"):
        assert hasattr(lib, s), f"{s} not exported by {built.LIB_PATH}"


def test_binding_table_binds_both(built):
    C = ctypes
    want = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
            C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    for s in ("innr_maxsim_rerank", "innr_maxsim_rerank_dev"):
        res, args = built.SIGNATURES[s]
        assert res is C.c_int and list(args) == want, s


@pytest.mark.parametrize("name", ["innr_maxsim_rerank", "innr_maxsim_rerank_dev"])
def test_rust_ffi_binds_both(name):
    src = open(SHIM).read()
    m = re.search(r"pub fn " + name + r"\(([^)]*)\)\s*->\s*c_int;", src)
    assert m, f"{name} missing from mod ffi (regenerate with tools/gen_rust_ffi.py --write)"
    assert [a.split(":", 1)[1].strip() for a in m.group(1).split(",")] == RUST


def test_rust_shim_has_rerank_beside_topk():
    src = open(SHIM).read()
    mod = src[src.index("pub mod maxsim"):src.index("pub mod distance")]
    assert re.search(r"pub fn rerank\(&self", mod) and "ffi::innr_maxsim_rerank(" in mod


def test_document_corpus_has_rerank():
    from innr_amd import maxsim
    import inspect
    sig = inspect.signature(maxsim.DocumentCorpus.rerank)
    assert list(sig.parameters) == ["self", "queries", "candidates", "k", "cosine"] and sig.parameters["cosine"].default is False
