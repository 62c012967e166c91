"""GPU tests of innr_batch_range_search_u8: every vector of a u8 code batch whose asymmetric score reaches a per-query threshold,
in index order (innr_batch_range_search's contract with the one metric of a code batch). Bar: per query all N scores from
oracle.batch_knn_u8(q, codes, p, N) scattered back by index, survivors flatnonzero(~(score < thr)) -- offsets, indices and score
bits equal, no tolerance. The exact scan (launch family 13: a count launch, then an emit launch) serves every engine value."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal

AUTO, EXACT, MFMA, BF16, I8 = 0, 1, 2, 3, 4  # INNR_KNN_*
RANGE_SCAN_U8 = 13                           # api_internal.h LaunchFamily
N, D = 2500, 37                              # three 1024-chunks, the last part full; D % 8, 16, 32 != 0
QS = (1, 3, 4, 8, 13)                        # one query a pass; 1 + 1 + 1; one 4-pass; one 8-pass; 8 + a ragged group moved back

_REC = np.dtype({"names": ["family", "lockstep", "arg", "groups"], "formats": ["u1", "u1", ("<i2", (4,)), "<u4"],
                 "offsets": [0, 1, 2, 12], "itemsize": 16})  # api_internal.h LaunchRec


def _logged(call):
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
    assert total.value == n
    return res, [(int(r["family"]), [int(a) for a in r["arg"]], int(r["groups"])) for r in buf[:n]]


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


def _all_scores(codes, p, qs):
    """scores[j][i]: the reference's score of code row i for query j (the full ranking scattered back by index)"""
    n = codes.shape[0]
    out = np.empty((len(qs), n), np.float32)
    for j, q in enumerate(qs):
        oi, os_ = oracle.batch_knn_u8(q, codes, p, n)
        out[j, oi.astype(np.int64)] = os_
    return out


def _thresholds(scores):
    """one kind per query, cycling: -inf, +inf, NaN, the median, a vector's exact score, above all but one, survivors only in the
    last part-full 1024-chunk, a whole 1024-chunk empty between two populated ones"""
    nq, n = scores.shape
    thr = np.empty(nq, np.float32)
    for j in range(nq):
        s = scores[j]
        kind = j % 8
        if kind == 0:
            thr[j] = -np.inf
        elif kind == 1:
            thr[j] = np.inf
        elif kind == 2:
            thr[j] = np.nan
        elif kind == 3:
            thr[j] = np.sort(s)[n // 2]
        elif kind == 4:
            thr[j] = s[(977 * (j + 1)) % n]   # that vector survives on equality
        elif kind == 5:
            thr[j] = np.sort(s)[-1]           # above all scores but the best
        elif kind == 6:
            last0 = (n - 1) // 1024 * 1024 or n - 256                   # (a corpus of one chunk: its last 256 vectors)
            thr[j] = np.nextafter(s[:last0].max(), np.float32(np.inf))  # nothing below the last chunk survives
        else:
            mid = s[1024:2048].max() if n > 2048 else s[n // 3:2 * n // 3].max()
            thr[j] = np.nextafter(mid, np.float32(np.inf))              # the middle chunk stays empty
    return thr


def _expected(scores, thr, base=0):
    off = [0]
    idx, sc = [], []
    for j in range(scores.shape[0]):
        with np.errstate(invalid="ignore"):
            keep = np.flatnonzero(~(scores[j] < thr[j]))
        idx.append(keep.astype(np.uint64) + np.uint64(base))
        sc.append(scores[j][keep])
        off.append(off[-1] + keep.size)
    return np.array(off, np.uint64), np.concatenate(idx), np.concatenate(sc)


def _case(n, dim, nq, seed):
    rows = oracle.generate_uniform(n, dim, seed)
    p = oracle.qparams_fit(rows)
    codes = oracle.quantize_u8(rows, p)
    qs = oracle.generate_uniform(nq, dim, seed + 1)
    # the code row that maximises a query's score (255 where q > 0, else 0; alpha > 0) planted where thresholds 6 and 7 of the first
    # eight queries need a survivor: in the last chunk for query 6, in the first and the last chunk for query 7
    codes[n - 200] = np.where(qs[6] > 0, 255, 0)
    codes[100] = codes[n - 100] = np.where(qs[7] > 0, 255, 0)
    scores = _all_scores(codes, p, qs)
    return codes, p, qs, scores, _thresholds(scores)


@pytest.fixture(scope="module")
def small():
    return _case(N, D, max(QS), 301)


def _corpus(S, codes, p):
    return S.QuantizedCorpus.from_codes(codes, codes.shape[0], codes.shape[1], S.QuantizationParams(p.alpha, p.offset))


def _run(qc, qs, thr, engine=AUTO, cap=None):
    from innr_amd import KnnStats
    st = KnnStats()
    off, idx, sc = qc.range_search(qs, thr, engine=engine, stats=st, cap=cap)
    return off, idx, sc, st


def _assert_same(got, exp, what):
    off, idx, sc = got[:3]
    assert np.asarray(off).astype(np.uint64).tolist() == exp[0].tolist(), f"{what}: offsets"
    assert np.asarray(idx).astype(np.uint64).tolist() == exp[1].tolist(), f"{what}: indices"
    assert bits_equal(np.asarray(sc), exp[2]), f"{what}: scores"


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("nq", QS)
def test_parity(S, small, nq):
    codes, p, qs, scores, thr = small
    # every threshold kind is exercised at every batch size: batches below eight queries take the queries in windows of nq
    qc = _corpus(S, codes, p)
    try:
        for rot in (range(0, 8, nq) if nq < 8 else (0,)):
            sel = list(range(rot, rot + nq))
            exp = _expected(scores[sel], thr[sel])
            for engine in (AUTO, EXACT, MFMA, BF16, I8):
                got = _run(qc, qs[sel], thr[sel], engine)
                _assert_same(got, exp, f"Q={nq} rot={rot} engine={engine}")
                st = got[3]
                assert st.engine == EXACT and st.queries_fallback == 0 and st.candidates_kept == 0, f"engine={engine}"
        # the thresholds really are what their names say
        e = _expected(scores[:8], thr[:8])
        cnt = np.diff(e[0].astype(np.int64))
        assert cnt[0] == N and cnt[1] == 0 and cnt[2] == N and cnt[5] == 1
        i6 = e[1][int(e[0][6]):int(e[0][7])]
        assert i6.size and i6.min() >= 2048
        i7 = e[1][int(e[0][7]):int(e[0][8])]
        assert ((i7 >= 1024) & (i7 < 2048)).sum() == 0 and (i7 < 1024).any() and (i7 >= 2048).any()
        i4 = e[1][int(e[0][4]):int(e[0][5])]
        assert (977 * 5) % N in i4.tolist()
    finally:
        qc.close()


def test_parity_larger(S):
    n, dim, nq = 20001, 128, 130
    codes, p, qs, scores, thr = _case(n, dim, nq, 401)
    thr[thr == -np.inf] = np.sort(scores[0])[-50]  # (keep the total small: 130 x 20001 entries add nothing)
    thr[np.isnan(thr)] = np.sort(scores[2])[-70]
    exp = _expected(scores, thr)
    qc = _corpus(S, codes, p)
    try:
        got, log = _logged(lambda: _run(qc, qs, thr, EXACT, cap=int(exp[0][-1])))
        _assert_same(got, exp, "130 queries")
        groups = (nq + 7) // 8
        assert log == [(RANGE_SCAN_U8, [8, 0, 0, 0], groups), (RANGE_SCAN_U8, [8, 1, 0, 0], groups)], log
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 2. cap
def test_count_only_and_cut(S, small):
    from innr_amd import _lib
    codes, p, qs, scores, thr = small
    exp = _expected(scores, thr)
    total = int(exp[0][-1])
    L = _lib.load()
    qc = _corpus(S, codes, p)
    try:
        # cap = 0 with null outputs: counts only, one launch per round
        off = np.zeros(len(qs) + 1, np.uint64)
        tot = C.c_size_t(0)
        rc, log = _logged(lambda: L.innr_batch_range_search_u8(qc._h, qs.ctypes.data, len(qs), D, thr.ctypes.data, AUTO, off.ctypes.data,
                                                              None, None, 0, C.byref(tot), None))
        assert rc == _lib.OK and tot.value == total and off.tolist() == exp[0].tolist()
        assert log == [(RANGE_SCAN_U8, [8, 0, 0, 0], 2)], log
        # a cap that cuts inside query 0 (all N survive) and inside a 1024-chunk: the prefix is written, the rest untouched
        for cap in (1500, N + 3, total - 1):
            idx = np.full(total + 8, 0xDEADBEEFDEADBEEF, np.uint64)
            sc = np.full(total + 8, -123.0, np.float32)
            off[:] = 0
            rc = L.innr_batch_range_search_u8(qc._h, qs.ctypes.data, len(qs), D, thr.ctypes.data, EXACT, off.ctypes.data,
                                              idx.ctypes.data, sc.ctypes.data, cap, C.byref(tot), None)
            assert rc == _lib.OK and tot.value == total and off.tolist() == exp[0].tolist(), cap
            assert idx[:cap].tolist() == exp[1][:cap].tolist() and bits_equal(sc[:cap], exp[2][:cap]), cap
            assert (idx[cap:] == 0xDEADBEEFDEADBEEF).all() and (sc[cap:] == -123.0).all(), f"cap={cap}: written past cap"
    finally:
        qc.close()


def test_dev_cap_guard(S, small):
    """the device entry point writes nothing at or past cap (the host one stages: this is the kernel's own bound)"""
    import torch
    from innr_amd import _lib
    codes, p, qs, scores, thr = small
    exp = _expected(scores, thr)
    total = int(exp[0][-1])
    L = _lib.load()
    qc = _corpus(S, codes, p)
    try:
        qc._ctx.bind_torch_stream()
        dq, dt = torch.from_numpy(qs).cuda(), torch.from_numpy(thr).cuda()
        cap = 1500
        off = torch.zeros(len(qs) + 1, dtype=torch.int64, device="cuda")
        idx = torch.full((total + 8,), -7, dtype=torch.int64, device="cuda")
        sc = torch.full((total + 8,), -123.0, dtype=torch.float32, device="cuda")
        tot = C.c_size_t(0)
        torch.cuda.synchronize()
        rc = L.innr_batch_range_search_u8_dev(qc._h, dq.data_ptr(), len(qs), D, dt.data_ptr(), AUTO, off.data_ptr(), idx.data_ptr(),
                                              sc.data_ptr(), cap, C.byref(tot), None)
        torch.cuda.synchronize()
        assert rc == _lib.OK and tot.value == total
        assert off.cpu().numpy().view(np.uint64).tolist() == exp[0].tolist()
        hi, hs = idx.cpu().numpy(), sc.cpu().numpy()
        assert hi[:cap].view(np.uint64).tolist() == exp[1][:cap].tolist() and bits_equal(hs[:cap], exp[2][:cap])
        assert (hi[cap:] == -7).all() and (hs[cap:] == -123.0).all(), "written past cap"
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 3. NaN, Q = 1, scores()
def test_nan_query_and_scores_bits(S, small):
    codes, p, qs, scores, thr = small
    qc = _corpus(S, codes, p)
    try:
        q = qs[:3].copy()
        q[1, 5] = np.nan
        t = np.array([np.sort(scores[0])[-20], 0.25, np.sort(scores[2])[-30]], np.float32)
        off, idx, sc, _ = _run(qc, q, t)
        ref = qc.scores(q[1])
        assert np.isnan(ref).all()
        assert int(off[2] - off[1]) == N, "a NaN score survives every threshold"
        assert idx[int(off[1]):int(off[2])].tolist() == list(range(N))
        assert bits_equal(sc[int(off[1]):int(off[2])], ref), "the scores of a NaN query are innr_batch_scores_u8's bits"
        # Q = 1 against a filter of scores() done in NumPy
        for j in (0, 2):
            s = qc.scores(q[j])
            assert bits_equal(s, scores[j])
            keep = np.flatnonzero(~(s < t[j]))
            o1, i1, s1, _ = _run(qc, q[j], t[j:j + 1])
            assert o1.tolist() == [0, keep.size] and i1.tolist() == keep.tolist() and bits_equal(s1, s[keep]), j
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 4. index base, prefix view, device
def test_index_base_prefix_view_and_dev(S, small):
    import torch
    codes, p, qs, scores, thr = small
    base, P = 10 ** 9, 20
    qc = _corpus(S, codes, p)
    qc.set_index_base(base)
    view = qc.prefix(P)  # (a view takes the index base its parent has when it is made)
    try:
        exp = _expected(scores, thr, base=base)
        got = _run(qc, qs, thr)
        _assert_same(got, exp, "index base")
        dgot = _run(qc, torch.from_numpy(qs).cuda(), torch.from_numpy(thr).cuda())
        torch.cuda.synchronize()
        assert dgot[0].is_cuda and dgot[1].is_cuda and dgot[2].is_cuda
        _assert_same([t.cpu().numpy() for t in dgot[:3]], exp, "device entry point")
        sub = np.ascontiguousarray(codes[:, :P])
        qp = np.ascontiguousarray(qs[:, :P])
        ps = _all_scores(sub, p, qp)
        pt = _thresholds(ps)
        _assert_same(_run(view, qp, pt), _expected(ps, pt, base=base), "prefix view")  # (a view inherits the index base)
    finally:
        view.close()
        qc.close()


# ------------------------------------------------------------------------------------------------ 5. which kernel ran
def test_launch_records(S, small):
    codes, p, qs, scores, thr = small
    qc = _corpus(S, codes, p)
    try:
        for nq, qb, groups in ((1, 1, 1), (3, 1, 3), (4, 4, 1), (8, 8, 1), (13, 8, 2)):
            exp = _expected(scores[:nq], thr[:nq])
            got, log = _logged(lambda: _run(qc, qs[:nq], thr[:nq], AUTO, cap=int(exp[0][-1])))
            _assert_same(got, exp, f"Q={nq}")
            assert log == [(RANGE_SCAN_U8, [qb, 0, 0, 0], groups), (RANGE_SCAN_U8, [qb, 1, 0, 0], groups)], (nq, log)
            got, log = _logged(lambda: _run(qc, qs[:nq], thr[:nq], AUTO, cap=0))
            assert log == [(RANGE_SCAN_U8, [qb, 0, 0, 0], groups)], (nq, log)
            assert got[0].tolist() == exp[0].tolist() and got[1].size == 0
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 6. several rounds
@pytest.fixture(scope="module")
def many():
    """4100 queries on 1000 codes of 8 dimensions, built once and read-only: the case and its CPU expectation"""
    case = _case(1000, 8, 4100, 601)
    exp = _expected(case[3], case[4])
    for a in (case[0], case[2], case[3], case[4]) + exp:
        a.setflags(write=False)
    return case, exp


@pytest.mark.parametrize("engine", (EXACT, I8))
def test_more_queries_than_one_round(S, many, ctx_option, engine):
    """more than 4096 queries: the batch is worked off in rounds -- the running 64-bit base carried in the offsets, each round's
    queries, thresholds and offsets against round-local counts, sums, norms, seeds, flags and lists (the collect path, which a
    corpus this small takes only with range_u8_i8_min_n = 0, finishes the queries without a finite collect bound by the exact scan)"""
    from test_gpu_u8_range_collect import _no_bound
    (codes, p, qs, scores, thr), exp = many
    if engine == I8:
        ctx_option("range_u8_i8_min_n", 0)
    qc = _corpus(S, codes, p)
    try:
        got = _run(qc, qs, thr, engine)
        _assert_same(got, exp, f"{len(qs)} queries engine={engine}")
        st = got[3]
        assert st.engine == engine
        if engine == I8:
            assert st.queries_fallback == _no_bound(thr), (st.queries_fallback, _no_bound(thr))
    finally:
        qc.close()


# ------------------------------------------------------------------------------------------------ 7. the checks, in their order
def test_checks_in_order(S, small):
    from innr_amd import _lib
    from innr_amd import batch as B
    codes, p, qs, scores, thr = small
    L = _lib.load()
    q2, t2 = np.ascontiguousarray(qs[:2]), np.ascontiguousarray(thr[3:5])
    off = np.full(3, 99, np.uint64)
    idx = np.empty(2 * N, np.uint64)
    sc = np.empty(2 * N, np.float32)
    tot = C.c_size_t(7)
    qc = _corpus(S, codes, p)
    empty = S.QuantizedCorpus.from_codes(np.empty(0, np.uint8), 0, D, S.QuantizationParams(p.alpha, p.offset))
    vb = B.VerticalBatch.from_rows(oracle.generate_uniform(100, D, 5))

    def call(fn, h, q=q2.ctypes.data, Q=2, d=D, t=t2.ctypes.data, o=off.ctypes.data, oi=idx.ctypes.data, os_=sc.ctypes.data, cap=2 * N,
             ot=C.byref(tot)):
        tot.value = 7
        off[:] = 99
        return fn(h, q, Q, d, t, AUTO, o, oi, os_, cap, ot, None)

    try:
        for fn in (L.innr_batch_range_search_u8, L.innr_batch_range_search_u8_dev):
            # 1. an f32 (or null) batch, before the dimension
            assert call(fn, vb._h, d=D - 1) == _lib.E_BAD_ARG
            assert call(fn, None, d=D - 1) == _lib.E_BAD_ARG
            # 2. the dimension, before the null checks
            assert call(fn, qc._h, d=D - 1, o=None, ot=None) == _lib.E_DIM_MISMATCH
            # 3. a null out_offsets or out_total, before the empty cases
            assert call(fn, qc._h, o=None, Q=0) == _lib.E_BAD_ARG
            assert call(fn, qc._h, ot=None, Q=0) == _lib.E_BAD_ARG
            # 5. null thresholds, queries or outputs with work to do
            assert call(fn, qc._h, t=None) == _lib.E_BAD_ARG
            assert call(fn, qc._h, q=None) == _lib.E_BAD_ARG
            assert call(fn, qc._h, oi=None) == _lib.E_BAD_ARG
            assert call(fn, qc._h, os_=None) == _lib.E_BAD_ARG
        # 4. N == 0 or Q == 0: all-zero offsets, whatever else is null (host entry point: `off` is host memory)
        fn = L.innr_batch_range_search_u8
        assert call(fn, empty._h, t=None, q=None, oi=None, os_=None) == _lib.OK and off.tolist() == [0, 0, 0] and tot.value == 0
        assert call(fn, qc._h, Q=0, t=None, q=None) == _lib.OK and off[0] == 0 and tot.value == 0
        assert call(fn, qc._h) == _lib.OK and tot.value == int(off[2])
    finally:
        vb.close()
        empty.close()
        qc.close()
