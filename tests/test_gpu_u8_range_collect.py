"""GPU tests of the collect path of innr_batch_range_search_u8: one MODE 2 pass of the int8 filter over the
K-packed copy of a code batch with fixed thresholds thr_j - E_j, exact scores of everything collected, the exact predicate on those
bits, the finish in index order; queries without a finite collect threshold or with an overfull list go to the exact scan.

The bar is test_gpu_u8_range_search.py's: offsets, indices and score bits equal to the oracle's full ranking filtered with
~(score < thr), no tolerance -- its _case, _thresholds and _expected are imported. Beyond the results every case asserts through
the launch record which MODE 2 instantiation served the call, and through innr_knn_stats that exactly the queries without a finite
collect threshold (a -inf, +inf or NaN threshold, a NaN query) or with an overfull list were finished by the exact scan: an
implementation that always falls back cannot pass. Small shapes set the context option range_u8_i8_min_n to 0."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from range_u8_ref import filter_query
from test_gpu_exact import bits_equal
from test_gpu_kernel_variants import _REC, FAMILIES, LOG_CAP, _hook
from test_gpu_u8_range_search import _assert_same, _case, _corpus, _expected, _run, _thresholds

AUTO, EXACT, MFMA, BF16, I8 = 0, 1, 2, 3, 4  # INNR_KNN_*
_FAMILIES = dict(FAMILIES)
_FAMILIES.update({12: "scan_u8_masked", 13: "range_scan_u8"})  # api_internal.h LaunchFamily
_NARGS = {"i8_one": 2, "i8_two": 2, "i8_small": 3, "range_scan_u8": 2}
COLLECT_CAP = 65536  # api.hip kCollectCap


def _logged(call):
    """(the call's result, its launches as (family, template arguments) in order)"""
    from innr_amd import _lib
    h = _lib.default_context().handle
    _hook().innrdbg_launch_log_reset(h)
    res = call()
    buf = np.zeros(LOG_CAP, _REC)
    total = C.c_uint64(0)
    n = _hook().innrdbg_launch_log(h, buf.ctypes.data, LOG_CAP, C.byref(total))
    assert total.value == n
    out = []
    for r in buf[:n]:
        fam = _FAMILIES[int(r["family"])]
        out.append((fam,) + tuple(int(x) for x in r["arg"][:_NARGS[fam]]))
    return res, out


def _collect_launches(log):
    return [e for e in log if e[0] in ("i8_one", "i8_two", "i8_small")]


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


@functools.lru_cache(maxsize=None)
def _shape(n, dim, nq, seed):
    """_case once per shape, read-only: codes, params, queries, scores [nq][n], the cycling thresholds"""
    out = _case(n, dim, nq, seed)
    for a in (out[0], out[2], out[3], out[4]):
        a.setflags(write=False)
    return out


def _no_bound(thr):
    return int((~np.isfinite(thr)).sum())  # -inf, +inf, NaN: no finite collect threshold


def _served_max(exp_off, thr):
    cnt = np.diff(exp_off.astype(np.int64))
    served = np.isfinite(thr)
    return int(cnt[served].max()) if served.any() else 0


# ------------------------------------------------------------------------------------------------ 1. small shapes
SMALL = [  # n, dim, nq, i8_no_small, the MODE 2 instantiation
    (2500, 37, 1, 0, ("i8_small", 2, 2, 2)),
    (2500, 37, 5, 0, ("i8_small", 2, 2, 2)),
    (2500, 37, 13, 0, ("i8_small", 2, 2, 2)),
    (2500, 37, 300, 0, ("i8_one", 6, 2)),      # the 512-query tile
    (2500, 37, 13, 1, ("i8_one", 6, 2)),       # ... at a small batch
    (8300, 500, 1, 0, ("i8_small", 8, 2, 2)),
    (8300, 500, 5, 0, ("i8_small", 8, 2, 2)),
    (8300, 500, 13, 0, ("i8_small", 8, 2, 2)),
    (8300, 500, 70, 0, ("i8_small", 8, 4, 2)),  # four column tiles
]
_MAXQ = {(2500, 37): 300, (8300, 500): 70}


@pytest.mark.parametrize("n,dim,nq,no_small,inst", SMALL)
def test_small_shapes(S, ctx_option, n, dim, nq, no_small, inst):
    ctx_option("range_u8_i8_min_n", 0)
    if no_small:
        ctx_option("i8_no_small", 1)
    codes, p, qs, scores, thr = _shape(n, dim, _MAXQ[(n, dim)], 501 + dim)
    qc = _corpus(S, codes, p)
    try:
        # batches below eight queries take the queries in windows of nq: every threshold kind is exercised at every batch size
        for rot in (range(0, 8, nq) if nq < 8 else (0,)):
            sel = list(range(rot, rot + nq))
            q, t, sc = qs[sel].copy(), thr[sel].copy(), scores[sel].copy()
            nan_q = 0
            if nq >= 13:  # a NaN query with a finite (median) threshold: every score is NaN and survives; bits = scores()'s
                q[11, 5] = np.nan
                sc[11] = qc.scores(q[11])
                assert np.isnan(sc[11]).all() and np.isfinite(t[11])
                nan_q = 1
            exp = _expected(sc, t)
            got, log = _logged(lambda: _run(qc, q, t, I8, cap=max(int(exp[0][-1]), 1)))
            _assert_same(got, exp, f"N={n} D={dim} Q={nq} rot={rot}")
            st = got[3]
            assert st.engine == I8
            assert _collect_launches(log) == [inst], log
            assert st.queries_fallback == _no_bound(t) + nan_q, (st.queries_fallback, t)
            kept_floor = _served_max(exp[0], np.where(np.arange(nq) == 11, np.nan, t) if nan_q else t)
            assert kept_floor <= st.candidates_kept <= COLLECT_CAP, (st.candidates_kept, kept_floor)
            # the exact scan ran for the fallback queries only: a count and an emit launch, or none
            scans = [e for e in log if e[0] == "range_scan_u8"]
            assert len(scans) == (2 if st.queries_fallback else 0), log
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 2. overflow, default floor
N_BIG, D_BIG = 70_000, 37


@functools.lru_cache(maxsize=None)
def _big():
    return _shape(N_BIG, D_BIG, 13, 601)


def test_overflow(S):
    codes, p, qs, scores, _ = _big()
    q, sc = qs[:3], scores[:3]
    thr = np.array([np.nextafter(sc[0].min(), np.float32(-np.inf)),  # below every score: N > 65536 collected -> the exact scan
                    np.sort(sc[1])[N_BIG // 2],                      # the median: about half the corpus collected, served
                    np.sort(sc[2])[-50]], np.float32)                # the 50th best
    # the median query stays within the list: whatever is collected has approx >= thr - E, hence score >= thr - 2 E
    E = filter_query(q[1], codes[:256], p.alpha, p.offset).E
    within = int((sc[1] >= thr[1] - 2.0001 * E).sum())
    assert N_BIG // 2 <= within < COLLECT_CAP, within
    exp = _expected(sc, thr)
    assert np.diff(exp[0].astype(np.int64)).tolist()[0] == N_BIG
    qc = _corpus(S, codes, p)
    try:
        got, log = _logged(lambda: _run(qc, q, thr, I8, cap=int(exp[0][-1])))
        _assert_same(got, exp, "overflow")
        st = got[3]
        assert st.engine == I8 and st.queries_fallback == 1, (st.engine, st.queries_fallback)
        assert st.candidates_kept == COLLECT_CAP
        assert _collect_launches(log) == [("i8_small", 2, 2, 2)], log
        assert [e for e in log if e[0] == "range_scan_u8"] == [("range_scan_u8", 1, 0), ("range_scan_u8", 1, 1)], log
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 3. mixed rounds: call shapes
@pytest.fixture(scope="module")
def small():
    return _shape(2500, 37, 300, 501 + 37)


def test_count_only_and_cut(S, ctx_option, small):
    """13 queries, served and fallback queries mixed in the one round (thresholds: -inf, +inf, NaN, the median, equality on a vector's
    exact score, all but one, survivors in the last chunk only, a 1024-chunk left empty between two populated ones, ...)"""
    import torch
    from innr_amd import KnnStats, _lib
    ctx_option("range_u8_i8_min_n", 0)
    codes, p, qs, scores, thr = small
    nq, dim = 13, codes.shape[1]
    q, t = np.ascontiguousarray(qs[:nq]), np.ascontiguousarray(thr[:nq])
    exp = _expected(scores[:nq], t)
    total = int(exp[0][-1])
    L = _lib.load()
    qc = _corpus(S, codes, p)
    try:
        # cap = 0 with null outputs: counts only
        off = np.zeros(nq + 1, np.uint64)
        tot = C.c_size_t(0)
        st = KnnStats()
        rc, log = _logged(lambda: L.innr_batch_range_search_u8(qc._h, q.ctypes.data, nq, dim, t.ctypes.data, I8, off.ctypes.data, None, None, 0,
                                                              C.byref(tot), C.byref(st)))
        assert rc == _lib.OK and tot.value == total and off.tolist() == exp[0].tolist()
        assert st.engine == I8 and st.queries_fallback == _no_bound(t)
        assert _collect_launches(log) == [("i8_small", 2, 2, 2)] and [e for e in log if e[0] == "range_scan_u8"] == [("range_scan_u8", 4, 0)], log
        # a cap that cuts inside query 0 (all N survive: the exact scan's), inside a served query and inside a 1024-chunk
        cut_served = int(exp[0][3]) + 1100  # query 3 (the median, ~1250 survivors): past its first 1024-chunk, before its end
        assert exp[0][3] < cut_served < exp[0][4]
        for cap in (1500, cut_served, total - 1):
            idx = np.full(total + 8, 0xDEADBEEFDEADBEEF, np.uint64)
            sc = np.full(total + 8, -123.0, np.float32)
            off[:] = 0
            rc = L.innr_batch_range_search_u8(qc._h, q.ctypes.data, nq, dim, t.ctypes.data, I8, off.ctypes.data, idx.ctypes.data,
                                              sc.ctypes.data, cap, C.byref(tot), C.byref(st))
            assert rc == _lib.OK and tot.value == total and off.tolist() == exp[0].tolist(), cap
            assert st.engine == I8
            assert idx[:cap].tolist() == exp[1][:cap].tolist() and bits_equal(sc[:cap], exp[2][:cap]), cap
            assert (idx[cap:] == 0xDEADBEEFDEADBEEF).all() and (sc[cap:] == -123.0).all(), f"cap={cap}: written past cap"
        # ... and the device entry point, which writes the caller's buffers itself
        qc._ctx.bind_torch_stream()
        dq, dt = torch.from_numpy(q.copy()).cuda(), torch.from_numpy(t.copy()).cuda()
        for cap in (1500, cut_served):
            doff = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            didx = torch.full((total + 8,), -7, dtype=torch.int64, device="cuda")
            dsc = torch.full((total + 8,), -123.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rc = L.innr_batch_range_search_u8_dev(qc._h, dq.data_ptr(), nq, dim, dt.data_ptr(), I8, doff.data_ptr(), didx.data_ptr(),
                                                  dsc.data_ptr(), cap, C.byref(tot), C.byref(st))
            torch.cuda.synchronize()
            assert rc == _lib.OK and tot.value == total and st.engine == I8
            assert doff.cpu().numpy().view(np.uint64).tolist() == exp[0].tolist()
            hi, hs = didx.cpu().numpy(), dsc.cpu().numpy()
            assert hi[:cap].view(np.uint64).tolist() == exp[1][:cap].tolist() and bits_equal(hs[:cap], exp[2][:cap]), cap
            assert (hi[cap:] == -7).all() and (hs[cap:] == -123.0).all(), f"cap={cap}: written past cap (device)"
    finally:
        qc.close()


def test_threshold_kinds_are_what_they_say(small):
    codes, p, qs, scores, thr = small
    n = codes.shape[0]
    e = _expected(scores[:8], thr[:8])
    cnt = np.diff(e[0].astype(np.int64))
    assert cnt[0] == n and cnt[1] == 0 and cnt[2] == n and cnt[5] == 1
    i4 = e[1][int(e[0][4]):int(e[0][5])]
    assert (977 * 5) % n in i4.tolist(), "equality on a vector's exact score"
    i7 = e[1][int(e[0][7]):int(e[0][8])]
    assert ((i7 >= 1024) & (i7 < 2048)).sum() == 0 and (i7 < 1024).any() and (i7 >= 2048).any(), "an empty chunk between two populated ones"


def test_index_base_and_prefix_views(S, ctx_option, small):
    """an index base; a prefix view of 32 dimensions, served by the collect pass on a copy of its own; and one of 20 dimensions,
    which the matrix-pipe engines do not address (innr_batch_knn_u8's rule for views: whole groups of 32 dimensions) -- exact scan"""
    ctx_option("range_u8_i8_min_n", 0)
    codes, p, qs, scores, thr = small
    nq, base = 13, 10 ** 9
    qc = _corpus(S, codes, p)
    qc.set_index_base(base)
    views = {P: qc.prefix(P) for P in (32, 20)}  # (a view takes the index base its parent has when it is made)
    try:
        got, log = _logged(lambda: _run(qc, qs[:nq], thr[:nq], I8))
        _assert_same(got, _expected(scores[:nq], thr[:nq], base=base), "index base")
        assert got[3].engine == I8 and got[3].queries_fallback == _no_bound(thr[:nq])
        for P, view in views.items():
            sub = np.ascontiguousarray(codes[:, :P])
            qp = np.ascontiguousarray(qs[:nq, :P])
            ps = np.empty((nq, codes.shape[0]), np.float32)
            for j in range(nq):
                oi, os_ = oracle.batch_knn_u8(qp[j], sub, p, codes.shape[0])
                ps[j, oi.astype(np.int64)] = os_
            pt = _thresholds(ps)
            got, log = _logged(lambda: _run(view, qp, pt, I8))
            _assert_same(got, _expected(ps, pt, base=base), f"prefix view P={P}")
            if P % 32 == 0:
                assert got[3].engine == I8 and got[3].queries_fallback == _no_bound(pt)
                assert _collect_launches(log) == [("i8_small", 2, 2, 2)], log
            else:
                assert got[3].engine == EXACT and got[3].queries_fallback == 0 and not _collect_launches(log), log
    finally:
        for view in views.values():
            view.close()
        qc.close()


# ------------------------------------------------------------------------------------------------ 4. policy
def test_floor_keeps_small_corpora_on_the_exact_scan(S, small):
    from innr_amd import _lib
    codes, p, qs, scores, thr = small
    exp = _expected(scores[:13], thr[:13])
    qc = _corpus(S, codes, p)
    try:
        for engine in (AUTO, EXACT, MFMA, BF16, I8, 17, -3):
            got, log = _logged(lambda: _run(qc, qs[:13], thr[:13], engine))
            _assert_same(got, exp, f"engine={engine}")
            assert got[3].engine == EXACT and got[3].queries_fallback == 0 and got[3].candidates_kept == 0, engine
            assert not _collect_launches(log), log
        assert not qc.memory().present_mask & _lib.COPY_I8_DOT
    finally:
        qc.close()


def test_policy_at_the_floor(S, ctx_option):
    from innr_amd import _lib
    codes, p, qs, scores, _ = _big()
    thr = np.array([np.sort(scores[j])[-20 - j] for j in range(13)], np.float32)
    exp = _expected(scores, thr)
    qc = _corpus(S, codes, p)
    try:
        # AUTO at one query: the exact scan, no copy built
        got = _run(qc, qs[:1], thr[:1], AUTO)
        _assert_same(got, _expected(scores[:1], thr[:1]), "AUTO Q=1")
        assert got[3].engine == EXACT and not qc.memory().present_mask & _lib.COPY_I8_DOT
        # a copy budget of 0: an explicit request stays on the exact scan, same results, no copy
        qc.copy_budget = 0
        got, log = _logged(lambda: _run(qc, qs, thr, I8))
        _assert_same(got, exp, "budget 0")
        assert got[3].engine == EXACT and got[3].queries_fallback == 0 and not _collect_launches(log)
        assert not qc.memory().present_mask & _lib.COPY_I8_DOT
        # unknown engine values: the exact scan, as before
        qc.copy_budget = None
        got = _run(qc, qs, thr, 17)
        _assert_same(got, exp, "engine 17")
        assert got[3].engine == EXACT and not qc.memory().present_mask & _lib.COPY_I8_DOT
        # an explicit request builds the copy; it is reported and released like the one kNN builds
        for engine in (I8, MFMA, BF16):
            got, log = _logged(lambda: _run(qc, qs, thr, engine))
            _assert_same(got, exp, f"engine={engine}")
            assert got[3].engine == I8 and got[3].queries_fallback == 0, engine
            assert _collect_launches(log) == [("i8_small", 2, 2, 2)], log
            assert qc.memory().present_mask & _lib.COPY_I8_DOT
        assert got[3].candidates_kept >= 32
        # EXACT stays EXACT with the copy in place, and so does AUTO below its batch size
        for engine, nq in ((EXACT, 13), (AUTO, 1)):
            got = _run(qc, qs[:nq], thr[:nq], engine)
            _assert_same(got, _expected(scores[:nq], thr[:nq]), f"engine={engine} with the copy")
            assert got[3].engine == EXACT
        qc.release_copies(_lib.COPY_I8_DOT)
        assert not qc.memory().present_mask & _lib.COPY_I8_DOT
    finally:
        qc.close()


def test_auto_by_batch_size(S, ctx_option, small):
    """INNR_KNN_AUTO: the exact scan below kRangeU8AutoQ0 = 16 queries (api.hip), the collect path from there on; u8_no_i8 keeps
    AUTO on the scan"""
    from innr_amd import _lib
    ctx_option("range_u8_i8_min_n", 0)
    codes, p, qs, scores, thr = small
    qc = _corpus(S, codes, p)
    try:
        for nq, engine in ((15, EXACT), (16, I8)):
            exp = _expected(scores[:nq], thr[:nq])
            got, log = _logged(lambda: _run(qc, qs[:nq], thr[:nq], AUTO, cap=int(exp[0][-1])))
            _assert_same(got, exp, f"AUTO Q={nq}")
            assert got[3].engine == engine, (nq, got[3].engine)
            assert bool(_collect_launches(log)) == (engine == I8), log
            assert bool(qc.memory().present_mask & _lib.COPY_I8_DOT) == (engine == I8)
        ctx_option("u8_no_i8", 1)
        got = _run(qc, qs[:16], thr[:16], AUTO)
        _assert_same(got, _expected(scores[:16], thr[:16]), "AUTO, u8_no_i8")
        assert got[3].engine == EXACT
    finally:
        qc.close()


def test_negative_alpha_takes_the_exact_scan(S, ctx_option):
    ctx_option("range_u8_i8_min_n", 0)
    codes, _, qs, _, _ = _shape(2500, 37, 300, 501 + 37)
    p = oracle.QParams(-2.0, 1.0)
    q = qs[:5]
    scores = np.empty((5, codes.shape[0]), np.float32)
    for j in range(5):
        oi, os_ = oracle.batch_knn_u8(q[j], codes, p, codes.shape[0])
        scores[j, oi.astype(np.int64)] = os_
    thr = np.array([np.sort(scores[j])[-30] for j in range(5)], np.float32)
    qc = _corpus(S, codes, p)
    try:
        got, log = _logged(lambda: _run(qc, q, thr, I8))
        _assert_same(got, _expected(scores, thr), "alpha < 0")
        assert got[3].engine == EXACT and not _collect_launches(log)
    finally:
        qc.close()


def test_option_round_trip(ctx_option):
    """the floor is a context option like the others: 65536 unless set"""
    from innr_amd import _lib
    ctx = _lib.default_context()
    assert ctx.get_option("range_u8_i8_min_n") == 65536
    ctx_option("range_u8_i8_min_n", 0)
    assert ctx.get_option("range_u8_i8_min_n") == 0
