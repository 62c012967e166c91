"""GPU tests of innr_batch_knn_u8_filtered (batch_knn_u8, scalar.rs:370-393, over the vectors that pass a mask, for Q queries and
every engine): the exact engine scans the codes with the mask applied (launch family 12); the other engines search a SELECTION
(the passing codes compacted on the device, select_gather_u8_kernel) and map the indices back. Bar: per query
oracle.batch_knn_u8(q, codes[sel], p, k) with sel = flatnonzero(mask), indices mapped back through sel -- the gather keeps index
order, so the reference's tie rule carries over -- with identical index lists and bit-identical scores (a descending stable sort
leaves no freedom: no tolerance). The selection cache is observed through the hook innrdbg_filter_selection_builds."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal

AUTO, EXACT, MFMA, I8 = 0, 1, 2, 4  # INNR_KNN_*
ENGINES = (EXACT, MFMA, I8, AUTO)
MAX_K = 240                         # INNR_MAX_K
SCAN_U8_MASKED = 12                 # api_internal.h LaunchFamily
N, D = 2500, 37                     # three 1024-chunks (the last part full), ten 256-chunks (the last at 196); D % 8, 16, 32 != 0
QS = (1, 3, 8, 13)                  # one query, the padded 4-query pass, one 8-pass, 8 + 5 ragged
KS = (1, 10, 50, 300)               # 300 > INNR_MAX_K: the masked full sort

_REC = np.dtype({"names": ["family", "lockstep", "arg", "groups"], "formats": ["u1", "u1", ("<i2", (4,)), "<u4"],
                 "offsets": [0, 1, 2, 12], "itemsize": 16})  # api_internal.h LaunchRec


def _logged(call):
    """the launch records (family, args, groups) of one call"""
    from conftest import hooks_lib
    from innr_amd import _lib
    L = hooks_lib()
    L.innrdbg_launch_log.restype = C.c_size_t
    L.innrdbg_launch_log.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.innrdbg_launch_log_reset.restype = None
    L.innrdbg_launch_log_reset.argtypes = [C.c_void_p]
    h = _lib.default_context().handle
    L.innrdbg_launch_log_reset(h)
    res = call()
    buf = np.zeros(64, _REC)
    total = C.c_uint64(0)
    n = L.innrdbg_launch_log(h, buf.ctypes.data, 64, C.byref(total))
    return res, [(int(r["family"]), [int(a) for a in r["arg"]], int(r["groups"])) for r in buf[:n]]


def _builds(qc) -> int:
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_filter_selection_builds
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p]
    return int(fn(qc._h))


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


def _make(n, dim, nq, seed):
    """codes = quantize_u8 of uniform rows with the fitted params; query 0's best row copied to three later positions (ties)"""
    rows = oracle.generate_uniform(n, dim, seed)
    p = oracle.qparams_fit(rows)
    codes = oracle.quantize_u8(rows, p)
    qs = oracle.generate_uniform(nq, dim, seed + 1)
    best = int(oracle.batch_knn_u8(qs[0], codes, p, 1)[0][0])
    later = sorted({(best + 257) % n, (best + 1031) % n, (best + 2 * 1031 + 5) % n})
    for i in later:
        codes[i] = codes[best]
    ties = sorted([best] + later)
    return codes, p, qs, ties


@pytest.fixture(scope="module")
def small():
    return _make(N, D, max(QS), 101)


def _masks(n, ties, seed=7):
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    few = np.zeros(n, np.uint8)
    few[rng.choice(n, size=7, replace=False)] = 1  # fewer than k = 10, 50, 300
    chunky = (rng.random(n) < 0.5).astype(np.uint8)
    chunky[512:768] = 0   # a whole 256-chunk empty ...
    chunky[768:1024] = 1  # ... next to a whole chunk full
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    bytes_ = (rng.random(n) < 0.5).astype(np.uint8) * np.where(idx % 2 == 0, 2, 255).astype(np.uint8)  # passing bytes 2 and 255
    no_first_tie = np.ones(n, np.uint8)
    no_first_tie[ties[0]] = 0  # the lowest-index copy of the tied rows fails
    return {
        "rand50": (rng.random(n) < 0.5).astype(np.uint8),
        "rand3": (rng.random(n) < 0.03).astype(np.uint8),
        "range": ((idx >= n // 10) & (idx < n // 10 + n // 3)).astype(np.uint8),
        "every7": (idx % 7 == 0).astype(np.uint8),
        "all": np.ones(n, np.uint8),
        "none": np.zeros(n, np.uint8),
        "fewer_than_k": few,
        "chunky": chunky,
        "only_last": last,
        "bytes_2_255": bytes_,
        "no_first_tie": no_first_tie,
    }


MASK_NAMES = list(_masks(16, [0]))


def _expected(codes, p, mask, qs, k, base=0):
    sel = np.flatnonzero(mask)
    out = []
    for q in qs:
        if sel.size == 0:
            out.append((np.empty(0, np.uint64), np.empty(0, np.float32)))
            continue
        oi, os_ = oracle.batch_knn_u8(q, codes[sel], p, k)
        out.append((sel[oi.astype(np.int64)].astype(np.uint64) + np.uint64(base), os_))
    return out


def _assert_same(idx, sc, exp, what):
    assert idx.shape[0] == len(exp), what
    for j, (oi, os_) in enumerate(exp):
        assert idx[j].tolist() == oi.tolist(), f"{what} q={j}: indices {idx[j][:8].tolist()} != {oi[:8].tolist()}"
        assert bits_equal(sc[j], os_), f"{what} q={j}: scores differ"


def _corpus(S, codes, p):
    return S.QuantizedCorpus.from_codes(codes, codes.shape[0], codes.shape[1], S.QuantizationParams(p.alpha, p.offset))


def _run(qc, qs, k, mask, engine):
    from innr_amd import KnnStats
    st = KnnStats()
    idx, sc = qc.knn_filtered_multi(qs, k, mask, engine=engine, stats=st)
    return idx, sc, st


def _plain_engine(sub, qs, k, engine):
    """what innr_batch_knn_u8 reports for this engine on a corpus made of the passing codes"""
    from innr_amd import KnnStats
    st = KnnStats()
    sub.knn_multi(qs, k, engine=engine, stats=st)
    return st.engine


def _check_matrix(S, codes, p, qs_all, mask, name, nqs, ks):
    n = codes.shape[0]
    sel = np.flatnonzero(mask)
    npass = sel.size
    qc = _corpus(S, codes, p)
    sub = _corpus(S, codes[sel], p) if npass else None
    try:
        for k in ks:
            exp_all = _expected(codes, p, mask, qs_all, k)
            for nq in nqs:
                qs, exp = qs_all[:nq], exp_all[:nq]
                for engine in ENGINES:
                    what = f"mask={name} Q={nq} k={k} engine={engine}"
                    before = _builds(qc)
                    (idx, sc, st), log = _logged(lambda: _run(qc, qs, k, mask, engine))
                    assert idx.shape == (nq, min(k, npass)), what
                    _assert_same(idx, sc, exp, what)
                    if npass and engine in (MFMA, I8):
                        assert st.engine == _plain_engine(sub, qs, k, engine), f"{what}: not the engine a batch of the passing codes gets"
                    if npass and engine == EXACT:
                        assert st.engine == EXACT, what
                        assert _builds(qc) == before, f"{what}: the exact engine built a selection"
                        masked = [r for r in log if r[0] == SCAN_U8_MASKED]
                        if 0 < npass < n and min(k, npass) <= MAX_K:
                            assert masked and all(a[0] in (8, 4, 1) and a[1] in (6, 12, 20) for _, a, _ in masked), (what, log)
                        else:  # every vector passes: the plain scan; beyond INNR_MAX_K: the masked full sort
                            assert not masked, (what, log)
    finally:
        qc.close()
        if sub is not None:
            sub.close()


# ------------------------------------------------------------------------------------------------ 1. parity matrix
@pytest.mark.parametrize("mask_name", MASK_NAMES)
def test_parity_matrix(S, small, mask_name):
    codes, p, qs, ties = small
    _check_matrix(S, codes, p, qs, _masks(N, ties)[mask_name], mask_name, QS, KS)


@pytest.mark.parametrize("mask_name", ["rand50", "rand3"])
def test_parity_larger_selection(S, mask_name):
    """20001 x 128, 130 queries: a selection large enough for the small-batch and tile forms of the int8 filter"""
    n, dim, nq = 20001, 128, 130
    codes, p, qs, ties = _make(n, dim, nq, 201)
    _check_matrix(S, codes, p, qs, _masks(n, ties)[mask_name], mask_name, (nq,), (10,))


# ------------------------------------------------------------------------------------------------ 2. ties across the cut
@pytest.mark.parametrize("k", (2, 3))
def test_ties_across_the_cut(S, small, k):
    codes, p, qs, ties = small
    assert len(ties) == 4 and all(np.array_equal(codes[t], codes[ties[0]]) for t in ties)
    masks = _masks(N, ties)
    qc = _corpus(S, codes, p)
    try:
        for name, want in (("all", ties[:k]), ("no_first_tie", ties[1:1 + k])):
            exp = _expected(codes, p, masks[name], qs[:1], k)
            assert exp[0][0].tolist() == want  # the four copies tie for the best score: the lowest passing indices win
            for engine in ENGINES:
                idx, sc, _ = _run(qc, qs[:1], k, masks[name], engine)
                _assert_same(idx, sc, exp, f"mask={name} engine={engine}")
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 3. the selection cache
def test_selection_cache_and_memory(S, small, ctx_option):
    from innr_amd._lib import COPY_I8_DOT, COPY_SELECTION
    codes, p, qs, ties = small
    k = 10
    masks = _masks(N, ties)
    mask, other = masks["rand50"], masks["chunky"]
    scaled = masks["rand50"] * np.uint8(255)  # the same predicate, other non-zero bytes
    exp, exp_other = _expected(codes, p, mask, qs, k), _expected(codes, p, other, qs, k)
    sel = np.flatnonzero(mask)
    npass = sel.size
    qc = _corpus(S, codes, p)
    sub = _corpus(S, codes[sel], p)
    try:
        assert _builds(qc) == 0 and qc.memory().present_mask & COPY_SELECTION == 0
        for m in (mask, mask, scaled, mask.astype(bool)):
            idx, sc, st = _run(qc, qs, k, m, I8)
            _assert_same(idx, sc, exp, "cache hit")
        assert _builds(qc) == 1, "the same mask built a second selection"
        # the size: codes, mask and map, plus the int8 copy the selection built for itself (what a batch of the passing codes builds)
        sub.knn_multi(qs, k, engine=I8)
        base = -(-npass // 1024) * 1024 * (-(-D // 32) * 32) + (-(-N // 1024) * 1024) + 4 * npass
        assert qc.memory().present_mask & COPY_SELECTION
        assert qc.copy_bytes(COPY_SELECTION) == base + sub.copy_bytes(COPY_I8_DOT)
        assert qc.memory().derived_bytes == qc.copy_bytes(COPY_SELECTION) + qc.copy_bytes(COPY_I8_DOT)
        idx, sc, _ = _run(qc, qs, k, other, I8)
        _assert_same(idx, sc, exp_other, "other mask")
        assert _builds(qc) == 2
        # the exact engine and the all-pass mask never build one
        _run(qc, qs, k, mask, EXACT)
        _run(qc, qs, k, masks["all"], MFMA)
        assert _builds(qc) == 2
        qc.release_copies(COPY_SELECTION)
        assert qc.copy_bytes(COPY_SELECTION) == 0 and qc.memory().present_mask & COPY_SELECTION == 0
        idx, sc, _ = _run(qc, qs, k, other, MFMA)
        _assert_same(idx, sc, exp_other, "after release")
        assert _builds(qc) == 3, "a released selection must be rebuilt"
        # copy budget 0: no selection is admitted, the masked exact scan serves the call
        qc.release_copies(COPY_SELECTION)
        qc.copy_budget = 0
        for engine in (MFMA, I8, AUTO):
            idx, sc, st = _run(qc, qs, k, mask, engine)
            _assert_same(idx, sc, exp, f"budget 0 engine={engine}")
            assert st.engine == EXACT and qc.copy_bytes(COPY_SELECTION) == 0
        assert _builds(qc) == 3
        qc.copy_budget = None
        ctx_option("filter_keep_selection", 0)
        for _ in range(2):
            idx, sc, _ = _run(qc, qs, k, mask, MFMA)
            _assert_same(idx, sc, exp, "filter_keep_selection = 0")
            assert qc.copy_bytes(COPY_SELECTION) == 0, "nothing may be kept after the call"
        assert _builds(qc) == 5, "filter_keep_selection = 0 must rebuild on every call"
    finally:
        qc.close()
        sub.close()


# ------------------------------------------------------------------------------------------------ 4. index base, prefix view, device
def test_index_base(S, small):
    codes, p, qs, ties = small
    base, k = 10 ** 9, 10
    mask = _masks(N, ties)["every7"]
    exp = _expected(codes, p, mask, qs, k, base=base)
    qc = _corpus(S, codes, p)
    try:
        qc.set_index_base(base)
        for engine in ENGINES:
            idx, sc, _ = _run(qc, qs, k, mask, engine)
            _assert_same(idx, sc, exp, f"engine={engine}")
    finally:
        qc.close()


def test_prefix_view(S, small):
    codes, p, qs, ties = small
    P, k = 20, 10
    mask = _masks(N, ties)["rand50"]
    sub = np.ascontiguousarray(codes[:, :P])
    qp = np.ascontiguousarray(qs[:, :P])
    exp = _expected(sub, p, mask, qp, k)
    qc = _corpus(S, codes, p)
    view = qc.prefix(P)
    try:
        for engine in ENGINES:
            idx, sc, _ = _run(view, qp, k, mask, engine)
            _assert_same(idx, sc, exp, f"engine={engine}")
    finally:
        view.close()
        qc.close()


def test_dev_variant_matches_host(S, small):
    import torch
    codes, p, qs, ties = small
    k = 10
    mask = _masks(N, ties)["rand3"]
    qc = _corpus(S, codes, p)
    try:
        dq = torch.from_numpy(qs).cuda()
        for engine in ENGINES:
            hi, hs, _ = _run(qc, qs, k, mask, engine)
            for dm in (torch.from_numpy(mask).cuda(), torch.from_numpy(mask.astype(bool)).cuda()):
                di, ds, _ = _run(qc, dq, k, dm, engine)
                torch.cuda.synchronize()
                assert di.is_cuda and di.shape == (len(qs), min(k, int(mask.sum())))
                assert np.array_equal(di.cpu().numpy().view(np.uint64), hi), f"engine={engine}"
                assert bits_equal(ds.cpu().numpy(), hs), f"engine={engine}"
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 5. the checks, in their order
def test_checks_in_order(S, small):
    from innr_amd import _lib
    from innr_amd import batch as B
    codes, p, qs, ties = small
    L = _lib.load()
    q2 = np.ascontiguousarray(qs[:2])
    mask = np.ones(N, np.uint8)
    none = np.zeros(N, np.uint8)
    idx = np.empty(2 * 10, np.uint64)
    sc = np.empty(2 * 10, np.float32)
    out_k = C.c_size_t(7)
    qc = _corpus(S, codes, p)
    empty = S.QuantizedCorpus.from_codes(np.empty(0, np.uint8), 0, D, S.QuantizationParams(p.alpha, p.offset))
    vb = B.VerticalBatch.from_rows(oracle.generate_uniform(100, D, 5))

    def call(fn, h, q=q2.ctypes.data, Q=2, d=D, k=10, m=mask.ctypes.data, oi=idx.ctypes.data, os_=sc.ctypes.data, ok=C.byref(out_k)):
        out_k.value = 7
        return fn(h, q, Q, d, k, m, AUTO, oi, os_, ok, None)

    try:
        for fn in (L.innr_batch_knn_u8_filtered, L.innr_batch_knn_u8_filtered_dev):
            # 1. a null batch, an f32 batch, a null out_k -- before anything else
            assert call(fn, None, d=D - 1) == _lib.E_BAD_ARG
            assert call(fn, vb._h, d=D - 1) == _lib.E_BAD_ARG
            assert call(fn, qc._h, d=D - 1, ok=None) == _lib.E_BAD_ARG
            # 2. N == 0 or k == 0: *out_k = 0, before the dimension check
            assert call(fn, qc._h, d=D - 1, k=0) == _lib.OK and out_k.value == 0
            assert call(fn, empty._h, d=D - 1, m=None) == _lib.OK and out_k.value == 0
            # 3. the dimension, before Q == 0 and the mask
            assert call(fn, qc._h, d=D - 1, Q=0, m=None) == _lib.E_DIM_MISMATCH
            # 4. Q == 0, before the mask
            assert call(fn, qc._h, Q=0, m=None, q=None) == _lib.OK and out_k.value == 0
            # 5. a null mask
            assert call(fn, qc._h, m=None) == _lib.E_BAD_ARG
            # 6. null queries / outputs with work to do
            assert call(fn, qc._h, q=None) == _lib.E_BAD_ARG
            assert call(fn, qc._h, oi=None) == _lib.E_BAD_ARG
            assert call(fn, qc._h, os_=None) == _lib.E_BAD_ARG
        # 7. no passing vector: *out_k = 0 (host entry point: the arrays above are host memory)
        assert call(L.innr_batch_knn_u8_filtered, qc._h, m=none.ctypes.data) == _lib.OK and out_k.value == 0
        assert call(L.innr_batch_knn_u8_filtered, qc._h) == _lib.OK and out_k.value == 10
    finally:
        vb.close()
        empty.close()
        qc.close()
