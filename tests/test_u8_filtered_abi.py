"""CPU-only checks of the filtered k-NN and range search over u8 code batches at every layer above the kernels: the four entry
points are declared in include/innr_hip.h with the contract's parameter order, exported by the library, bound in the Python
table with matching kinds, wrapped by QuantizedCorpus methods with the documented signatures, and wrapped in the Rust shim."""
from __future__ import annotations

import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
RUST_SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")

KNN = ["b", "queries", "Q", "D", "k", "mask", "engine", "out_idx", "out_score", "out_k", "stats"]
RANGE = ["b", "queries", "Q", "D", "thresholds", "engine", "out_offsets", "out_idx", "out_score", "cap", "out_total", "stats"]
PARAMS = {
    "innr_batch_knn_u8_filtered": KNN,
    "innr_batch_knn_u8_filtered_dev": ["b", "d_queries", "Q", "D", "k", "d_mask", "engine", "d_out_idx", "d_out_score", "out_k", "stats"],
    "innr_batch_range_search_u8": RANGE,
    "innr_batch_range_search_u8_dev": ["b", "d_queries", "Q", "D", "d_thresholds", "engine", "d_out_offsets", "d_out_idx", "d_out_score",
                                       "cap", "out_total", "stats"],
}
KNN_TYPES = ["innr_batch*", "const float*", "size_t", "size_t", "size_t", "const uint8_t*", "int", "uint64_t*", "float*", "size_t*",
             "innr_knn_stats*"]
RANGE_TYPES = ["innr_batch*", "const float*", "size_t", "size_t", "const float*", "int", "uint64_t*", "uint64_t*", "float*", "size_t",
               "size_t*", "innr_knn_stats*"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def _prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"innr_status\s+(innr_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", hdr):
        params = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            mm = re.match(r"(.*?)\s*(\w+)$", a)
            params.append((mm.group(1).replace(" *", "*"), mm.group(2)))
        out[m.group(1)] = params
    return out


def test_header_declares_the_four_entry_points_in_the_contract_order():
    protos = _prototypes()
    for name, names in PARAMS.items():
        assert name in protos, f"{name} is not declared in include/innr_hip.h"
        assert [n for _, n in protos[name]] == names, name
        assert [t for t, _ in protos[name]] == (KNN_TYPES if "knn" in name else RANGE_TYPES), name


def test_library_exports_and_binds_them(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    for name in PARAMS:
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = built.SIGNATURES[name]
        assert res is ctypes.c_int
        want = KNN_TYPES if "knn" in name else RANGE_TYPES
        assert len(args) == len(want), name
        for a, t in zip(args, want):
            if t == "size_t":
                assert a is sz, (name, t)
            elif t == "int":
                assert a is ci, (name, t)
            else:  # every pointer kind
                assert a is vp or issubclass(a, ctypes._Pointer), (name, t)


def test_python_methods_have_the_documented_signatures():
    from innr_amd import scalar as S
    from innr_amd._lib import KNN_AUTO
    sig = inspect.signature(S.QuantizedCorpus.knn_filtered_multi)
    assert list(sig.parameters) == ["self", "queries", "k", "mask", "engine", "stats"]
    assert sig.parameters["engine"].default == KNN_AUTO and sig.parameters["stats"].default is None
    sig = inspect.signature(S.QuantizedCorpus.range_search)
    assert list(sig.parameters) == ["self", "queries", "thresholds", "engine", "stats", "cap"]
    assert sig.parameters["engine"].default == KNN_AUTO and sig.parameters["stats"].default is None
    assert sig.parameters["cap"].default is None


def test_rust_shim_binds_and_wraps_them():
    rs = open(RUST_SHIM).read()
    ffi = rs[rs.index("mod ffi"):]
    ffi = ffi[:ffi.index("\n}\n")]
    for name in PARAMS:
        assert re.search(r"pub fn %s\s*\(" % name, ffi), f"{name} is not bound in mod ffi"
    scalar = rs[rs.index("pub mod scalar"):]
    scalar = scalar[:scalar.index("pub mod maxsim")]
    impl = scalar[scalar.index("impl QuantizedCorpus"):]
    assert re.search(r"pub fn knn_filtered_multi\s*\(&self", impl) and "ffi::innr_batch_knn_u8_filtered(" in impl
    assert re.search(r"pub fn range_search\s*\(&self", impl) and "ffi::innr_batch_range_search_u8(" in impl


def test_launch_families_are_12_and_13():
    src = open(os.path.join(ROOT, "innr_amd", "csrc", "api_internal.h")).read()
    enum = src[src.index("enum LaunchFamily"):]
    enum = enum[:enum.index("};")]
    vals = {int(v): n for n, v in re.findall(r"(kLaunch\w+)\s*=\s*(\d+)", enum)}
    assert vals[12] == "kLaunchScanU8Masked" and vals[13] == "kLaunchRangeScanU8" and sorted(vals) == list(range(1, 14))
