"""CPU-only checks of the boundary of search by stored vector: the four entry points are declared with the documented parameter
names, bound and exported; the Python and Rust mirrors have the documented shape; extract_vector no longer downloads the corpus;
rows.o shares no kernel with the other objects."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")
PARAMS = {
    "innr_batch_gather_rows": ["b", "idx", "n", "out"],
    "innr_batch_gather_rows_dev": ["b", "d_idx", "n", "d_out"],
    "innr_batch_knn_rows": ["b", "metric", "idx", "Q", "k", "exclude_self", "engine", "out_idx", "out_score", "out_k", "stats"],
    "innr_batch_knn_rows_dev": ["b", "metric", "d_idx", "Q", "k", "exclude_self", "engine", "d_out_idx", "d_out_score", "out_k",
                                "stats"],
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_the_four_entry_points():
    raw = open(HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for s, want in PARAMS.items():
        m = re.search(r"innr_status\s+%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, f"{s} not declared in include/innr_hip.h"
        names = [re.sub(r".*?(\w+)$", r"\1", a.strip()) for a in m.group(1).split(",")]
        assert names == want, (s, names)
    assert "batch.rs:217" in raw and "exclude_self" in raw


def test_binding_table_and_library_have_them(built):
    import ctypes
    lib = ctypes.CDLL(built.LIB_PATH)
    for s, want in PARAMS.items():
        assert s in built.SIGNATURES and hasattr(lib, s), s
        assert len(built.SIGNATURES[s][1]) == len(want), s


def test_python_mirror_signatures():
    from innr_amd import METRIC_L2SQ, KNN_AUTO
    from innr_amd import batch as B
    assert list(inspect.signature(B.VerticalBatch.rows).parameters) == ["self", "indices"]
    sig = inspect.signature(B.batch_knn_rows)
    assert list(sig.parameters) == ["indices", "batch", "k", "metric", "exclude_self", "engine", "stats"]
    assert sig.parameters["metric"].default == METRIC_L2SQ and sig.parameters["exclude_self"].default is True
    assert sig.parameters["engine"].default == KNN_AUTO and sig.parameters["stats"].default is None
    sig = inspect.signature(B.batch_knn_graph)
    assert list(sig.parameters) == ["batch", "k", "metric", "engine", "first", "count"]
    assert sig.parameters["first"].default == 0 and sig.parameters["count"].default is None


def test_extract_vector_does_not_download_the_corpus():
    from innr_amd import batch as B
    for fn in (B.VerticalBatch.extract_vector, B.VerticalBatch.get):
        src = inspect.getsource(fn)
        assert "self.data()" not in src, fn.__name__  # only the cached host copy, and only when it exists
        assert "self._host is not None" in src
    assert "self.rows(" in inspect.getsource(B.VerticalBatch.extract_vector)
    assert "data()" in inspect.getsource(B.VerticalBatch.dimension_slice)  # stays as it is: a whole dimension row


def test_rust_shim_goes_through_the_gather():
    rs = open(SHIM).read()
    impl = rs[rs.index("pub mod batch"):]
    assert "ffi::innr_batch_gather_rows(" in impl and "ffi::innr_batch_knn_rows(" in impl
    ev = impl[impl.index("pub fn extract_vector"):]
    ev = ev[:ev.index("\n        }\n")]
    assert "gather_rows" in ev and "self.data()" not in ev and "self.get(" not in ev
    assert re.search(r"pub fn knn_rows\(&self, metric: i32, indices: &\[u64\], k: usize, exclude_self: bool\) -> Vec<BatchKnnResult>", impl)


def test_rows_object_owns_its_kernels_alone(built):
    """tests/test_abi.py's one-owner rule, for the object it does not list"""
    libdir = os.path.dirname(built.LIB_PATH)
    objs = {o: os.path.join(libdir, o) for o in ("rows.o", "adaptive.o", "api.o", "maxsim.o", "comm.o", "sort_full.o")}
    if not all(os.path.exists(p) for p in objs.values()):
        pytest.skip("build-box check (the object files are not shipped to the GPU box)")
    stubs = {}
    for o, p in objs.items():
        out = subprocess.run(["nm", "--defined-only", p], capture_output=True, text=True, check=True).stdout
        stubs[o] = set(l.split()[-1] for l in out.splitlines() if "__device_stub__" in l)
    assert len(stubs["rows.o"]) == 3, stubs["rows.o"]
    assert all(("gather_rows" in s) or ("strip_self" in s) for s in stubs["rows.o"]), stubs["rows.o"]
    for o in objs:
        if o != "rows.o":
            assert not (stubs["rows.o"] & stubs[o]), (o, stubs["rows.o"] & stubs[o])
