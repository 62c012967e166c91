"""CPU-only checks of the drop-in boundary: the C-ABI library builds, loads, and exports exactly the
symbols include/innr_hip.h declares; the Python binding table matches the header; without a GPU the
product path fails loudly instead of computing on the CPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "innr_hip.h")


def _declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(innr_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from innr_amd import _lib
    return _lib


def test_header_declares_symbols():
    syms = _declared_symbols()
    assert "innr_batch_knn" in syms and "innr_ctx_create" in syms and len(syms) >= 15


def test_library_exports_every_declared_symbol(built):
    lib = ctypes.CDLL(built.LIB_PATH)
    for s in _declared_symbols():
        assert hasattr(lib, s), f"{s} declared in include/innr_hip.h but not exported"


def test_binding_table_matches_header(built):
    assert sorted(built.SIGNATURES) == _declared_symbols()


def test_no_extra_public_symbols(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True).stdout
    # every defined C symbol that carries the library's prefix in ANY spelling (innr_, innrdbg_, ...): exactly the header's set.
    # The innrdbg_* layout hooks live in libinnr_hip_testhooks.so only (make hooks).
    exported = sorted(set(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("innr")))
    assert exported == _declared_symbols()
    assert not [l for l in out.splitlines() if "innrdbg" in l], "debug hooks leaked into the product library"


def test_code_object_is_gfx950(built):
    # every device code object in the fat binary is a gfx950 one (bundle ids "…amdhsa--<arch>"); rocPRIM's host-side
    # tuning tables carry other architectures' NAMES as strings, which is why the check is on the bundle ids
    import re
    data = open(built.LIB_PATH, "rb").read()
    archs = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", data))
    assert archs == {b"gfx950"} and b"nvptx" not in data and b"sm_" not in data


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_fails_loudly_without_gpu(built):
    from innr_amd import InnrError
    from innr_amd import batch as B
    with pytest.raises(InnrError):
        B.VerticalBatch.from_rows([[1.0, 2.0]])
    assert "no CPU fallback" in built.last_error() or "HIP" in built.last_error() or "device" in built.last_error()


def test_gemm_asm_guard(built):
    """The GEMM kernels wait for their inline-asm loads with hand-counted s_waitcnt; whether the register allocator kept
    the operand registers untouched in between, and whether every asm load takes its base from an in-statement
    s_mov_b64, is checked on the ISA of every instantiation (tools/check_gemm_asm.py) -- here, on the CPU box, before any
    GPU time is spent. `make asm` regenerates the ISA only when a kernel source changed."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("build-box check (the ISA listing is not shipped to the GPU box)")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "innr_amd", "csrc"), "asm"])
    r = subprocess.run(["python3", os.path.join(ROOT, "tools", "check_gemm_asm.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.count(" ok") >= 40, r.stdout


def test_every_kernel_has_one_owning_object(built):
    """Every __global__ kernel is compiled into exactly one object of the product library. hipcc emits a host launch stub per
    kernel (`__device_stub__` in its mangled name; a template instantiation's is a weak symbol, so the linker would merge a second
    copy without a word while the device code doubles): no stub may be defined in two objects. Translation units share only
    api_internal.h and the headers of templates and __forceinline__ device functions (innr_amd/csrc/Makefile)."""
    libdir = os.path.dirname(built.LIB_PATH)
    objects = [os.path.join(libdir, o) for o in ("api.o", "maxsim.o", "comm.o", "sort_full.o")]
    if not all(os.path.exists(o) for o in objects):
        pytest.skip("build-box check (the object files are not shipped to the GPU box)")
    owners = {}
    for o in objects:
        out = subprocess.run(["nm", "--defined-only", o], capture_output=True, text=True, check=True).stdout
        stubs = set(l.split()[-1] for l in out.splitlines() if "__device_stub__" in l)
        assert stubs, f"no kernel launch stub found in {os.path.basename(o)}"
        for s in stubs:
            owners.setdefault(s, []).append(os.path.basename(o))
    shared = {s: o for s, o in owners.items() if len(o) > 1}
    assert not shared, f"kernels compiled into more than one object: {shared}"


RUST_SHIM = os.path.join(ROOT, "rust", "innr-hip", "src", "lib.rs")


def _c_params(decl: str):
    """parameter C types of one prototype, normalised: pointers -> 'ptr', everything else its base type"""
    args = decl[decl.index("(") + 1:decl.rindex(")")].strip()
    if args in ("", "void"):
        return []
    out = []
    for a in args.split(","):
        a = a.strip()
        if "*" in a:
            out.append("ptr")
        else:
            out.append(re.sub(r"\s+\w+$", "", a).strip())  # drop the parameter name
    return out


def _rust_params(decl: str):
    args = decl[decl.index("(") + 1:decl.rindex(")")].strip()
    if not args:
        return []
    out = []
    for a in args.split(","):
        a = a.strip()
        if not a:
            continue
        ty = a.split(":", 1)[1].strip()
        out.append("ptr" if ty.startswith("*") else ty)
    return out


C_TO_RUST = {"int": "c_int", "size_t": "usize", "uint64_t": "u64", "uint32_t": "u32", "float": "f32", "innr_status": "c_int", "long": "c_long"}


def test_rust_shim_binds_the_whole_header():
    """rust/innr-hip `mod ffi` against include/innr_hip.h, as text (this image has no rustc): every declared entry point is
    bound, nothing else is, and each binding has the header's parameter count with pointer / scalar kinds and scalar
    types matching."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(2): m.group(0) for m in re.finditer(r"([\w\s\*]+?)\b(innr_[a-z0-9_]+)\s*\([^;{]*\)\s*;", hdr)}
    rs = open(RUST_SHIM).read()
    ffi = rs[rs.index("mod ffi"):]
    ffi = ffi[:ffi.index("\n}\n") + 3]
    ffi = re.sub(r"//.*", "", ffi)
    bound = {m.group(1): m.group(0) for m in re.finditer(r"pub fn (innr_[a-z0-9_]+)\s*\([^;]*\)[^;]*;", ffi)}
    assert sorted(bound) == sorted(protos), (sorted(set(protos) - set(bound)), sorted(set(bound) - set(protos)))
    for name, decl in protos.items():
        want = [t if t == "ptr" else C_TO_RUST.get(t, t) for t in _c_params(decl)]
        got = _rust_params(bound[name])
        assert got == want, (name, got, want)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "innr_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "innr_oracle" not in txt, f
