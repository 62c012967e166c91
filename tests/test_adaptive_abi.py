"""CPU-only checks of batch_knn_adaptive's boundary: both entry points are declared, bound and mirrored with the reference's
parameter order; adaptive.o shares no kernel with the other objects; and the NumPy restatement the GPU tests lean on
(tests/adaptive_ref.py) equals the oracle bit for bit."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import order_ref as R
from adaptive_ref import adaptive_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")
SYMBOLS = ("innr_batch_knn_adaptive", "innr_batch_knn_adaptive_dev")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_both_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s in SYMBOLS:
        m = re.search(r"innr_status\s+%s\s*\(([^;]*)\)\s*;" % s, hdr)
        assert m, f"{s} not declared in include/innr_hip.h"
        names = [re.sub(r".*?(\w+)$", r"\1", a.strip()) for a in m.group(1).split(",")]
        assert [n.replace("d_", "") for n in names] == ["b", "queries", "Q", "D", "k", "warmup_dims", "out_idx", "out_score", "out_k",
                                                        "stats"], names
    assert "batch.rs:441-564" in open(HEADER).read()


def test_binding_table_and_library_have_them(built):
    import ctypes
    lib = ctypes.CDLL(built.LIB_PATH)
    for s in SYMBOLS:
        assert s in built.SIGNATURES and hasattr(lib, s), s
        assert len(built.SIGNATURES[s][1]) == 10


def test_python_mirror_has_the_reference_signature():
    from innr_amd import batch as B
    assert list(inspect.signature(B.batch_knn_adaptive).parameters) == ["query", "batch", "k", "warmup_dims"]  # batch.rs:441-446
    assert list(inspect.signature(B.batch_knn_adaptive_multi).parameters) == ["queries", "batch", "k", "warmup_dims", "stats"]


def test_rust_shim_has_the_wrapper():
    rs = open(os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")).read()
    assert re.search(r"pub fn batch_knn_adaptive\(query: &\[f32\], batch: &VerticalBatch, k: usize, warmup_dims: usize\) -> BatchKnnResult", rs)
    assert 'assert!(warmup_dims > 0, "warmup_dims must be > 0")' in rs


def test_adaptive_object_owns_its_kernels_alone(built):
    """tests/test_abi.py's one-owner rule, for the object it does not list: no kernel launch stub of adaptive.o is defined in
    another object of the library."""
    libdir = os.path.dirname(built.LIB_PATH)
    objs = {o: os.path.join(libdir, o) for o in ("adaptive.o", "api.o", "maxsim.o", "comm.o", "sort_full.o")}
    if not all(os.path.exists(p) for p in objs.values()):
        pytest.skip("build-box check (the object files are not shipped to the GPU box)")
    stubs = {}
    for o, p in objs.items():
        out = subprocess.run(["nm", "--defined-only", p], capture_output=True, text=True, check=True).stdout
        stubs[o] = set(l.split()[-1] for l in out.splitlines() if "__device_stub__" in l)
    assert len(stubs["adaptive.o"]) >= 8 and all("adaptive" in s for s in stubs["adaptive.o"]), stubs["adaptive.o"]
    for o in objs:
        if o != "adaptive.o":
            assert not (stubs["adaptive.o"] & stubs[o]), (o, stubs["adaptive.o"] & stubs[o])


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------
KINDS = ("uniform", "halves", "decay", "special")


def make_case(seed: int):
    """(q, data (D, N), k, warmup_dims) -- N 1-900, D 1-140, k 1-60, warm-up 1 .. D+4, four data kinds in turn"""
    rng = np.random.default_rng(1000 + seed)
    kind = KINDS[seed % 4]
    n, dim = int(rng.integers(1, 901)), int(rng.integers(1, 141))
    k, w = int(rng.integers(1, 61)), int(rng.integers(1, dim + 5))
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    q = rng.uniform(-1, 1, dim).astype(np.float32)
    if kind == "halves":  # many exact ties
        rows, q = (np.round(rows * 4) / 2).astype(np.float32), (np.round(q * 4) / 2).astype(np.float32)
    elif kind == "decay":
        s = (np.float32(0.9) ** np.arange(dim, dtype=np.float32)).astype(np.float32)
        rows = rng.standard_normal((n, dim)).astype(np.float32) * s
        q = rng.standard_normal(dim).astype(np.float32) * s
    elif kind == "special":  # one special value per row at most: a propagated NaN keeps its sign, a generated one is -NaN
        for r in rng.choice(n, size=min(n, 1 + n // 10), replace=False):
            d = int(rng.integers(0, dim))
            pat = (R.PNAN, R.NNAN, R.PINF, R.NINF)[int(rng.integers(0, 4))]
            rows.view(np.uint32)[r, d] = np.uint32(pat)
        if seed % 8 == 3:
            q[int(rng.integers(0, dim))] = np.inf  # inf - inf where a row holds +inf there
    return q, np.ascontiguousarray(rows.T), k, w


@pytest.mark.parametrize("seed", range(48))
def test_mirror_equals_oracle(seed):
    q, data, k, w = make_case(seed)
    oi, os_ = oracle.batch_knn_adaptive(q, data, k, w)
    mi, ms, alive = adaptive_ref(q, data, k, w)
    assert mi.tolist() == oi.tolist(), (KINDS[seed % 4], data.shape, k, w)
    assert np.array_equal(R.bits(ms), R.bits(os_))
    assert min(k, data.shape[1]) <= alive <= data.shape[1]


def test_mirror_degenerate_cases():
    i, s, a = adaptive_ref([], np.empty((0, 3), np.float32), 2, 1)
    assert i.tolist() == [0, 1] and s.tolist() == [0.0, 0.0] and a == 3
    assert adaptive_ref([1, 2], np.empty((2, 0), np.float32), 5, 2)[0].size == 0
    assert adaptive_ref([1, 2], oracle.from_rows([[1, 2]]), 0, 1)[0].size == 0
