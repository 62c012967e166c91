"""GPU tests of search by stored vector (innr_amd/csrc/rows.hip): innr_batch_gather_rows[_dev] returns vectors of
the corpus bit for bit, from the dimension-major store and from the row-major copy; innr_batch_knn_rows[_dev] is innr_batch_knn
with those vectors as queries, optionally without each query's own index. Expected results are plain NumPy indexing of the
uploaded rows and the CPU oracle called with those rows."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal, same_knn

BASE = 10 ** 9
NNAN, PNAN = 0xFFC12345, 0x7FC54321      # quiet NaNs with payloads, both signs
SNAN = 0x7F812345                        # a signalling pattern: a copy must not quiet it
SPECIALS = (NNAN, PNAN, SNAN, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000)  # ..., -0.0, denormals, +-inf


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@pytest.fixture(scope="module")
def lib():
    from innr_amd import _lib
    return _lib.load()


def _rows(n, dim, seed):
    rows = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    bits = rows.view(np.uint32)
    for j, pat in enumerate(SPECIALS):  # one special value per planted row, spread over rows and dimensions
        bits[(j * 37) % n, (j * 11) % dim] = np.uint32(pat)
    return rows


def _index_lists(n, seed):
    rng = np.random.default_rng(seed)
    return {"ascending": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "random": rng.integers(0, n, 500),
            "one": np.array([n - 1]), "empty": np.array([], dtype=np.int64)}


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


# =============================================================================== gather
GATHER_SHAPES = [(1, 1), (257, 33), (1000, 128), (4099, 100)]


@pytest.mark.parametrize("n,dim", GATHER_SHAPES)
@pytest.mark.parametrize("with_copy", [False, True], ids=["store", "rows_copy"])
def test_gather_is_a_bitwise_copy(B, innr, n, dim, with_copy):
    rows = _rows(n, dim, 7 + n)
    vb = B.VerticalBatch.from_rows(rows)
    if with_copy:
        assert vb.build_copies(innr.COPY_ROWS) & innr.COPY_ROWS
    else:
        vb.release_copies(innr.COPY_ALL)
    before = vb.memory()
    assert bool(before.present_mask & innr.COPY_ROWS) == with_copy
    for name, ids in _index_lists(n, n).items():
        got = vb.rows(ids)
        assert got.shape == (len(ids), dim) and got.dtype == np.float32, name
        assert bits_equal(got, rows[ids]), (name, n, dim, with_copy)
    assert vb.memory() == before  # a gather builds nothing: without the copy it reads the store, and the copy stays absent
    vb.close()


def test_gather_paths_agree_and_ignore_the_copy_when_told(B, innr, ctx_option):
    n, dim = 1000, 128
    rows = _rows(n, dim, 3)
    ids = np.random.default_rng(4).integers(0, n, 777)
    vb = B.VerticalBatch.from_rows(rows)
    from_store = vb.rows(ids)
    vb.build_copies(innr.COPY_ROWS)
    from_copy = vb.rows(ids)
    ctx_option("no_rows_copy", 1)  # the copy exists but is not to be used: the store path again
    from_store_again = vb.rows(ids)
    assert bits_equal(from_store, rows[ids]) and bits_equal(from_copy, from_store) and bits_equal(from_store_again, from_store)
    vb.close()


@pytest.mark.parametrize("with_copy", [False, True], ids=["store", "rows_copy"])
def test_gather_index_base(B, innr, with_copy):
    n, dim = 257, 33
    rows = _rows(n, dim, 11)
    vb = B.VerticalBatch.from_rows(rows)
    vb.set_index_base(BASE)
    if with_copy:
        vb.build_copies(innr.COPY_ROWS)
    ids = np.random.default_rng(12).integers(0, n, 300)
    assert bits_equal(vb.rows(ids + BASE), rows[ids])
    assert bits_equal(vb.extract_vector(256), rows[256]) and vb._host is None  # extract_vector's index stays local
    vb.close()


@pytest.mark.parametrize("P", [20, 32])
@pytest.mark.parametrize("with_copy", [False, True], ids=["store", "rows_copy"])
def test_gather_prefix_view(B, innr, P, with_copy):
    """rows P .. round_up(P, 32) of a view's store hold the parent's next dimensions: P = 20 catches a mask by the padded count"""
    n, dim = 1000, 37
    rows = _rows(n, dim, 13)
    vb = B.VerticalBatch.from_rows(rows)
    view = vb.prefix(P)
    if with_copy:
        assert view.build_copies(innr.COPY_ROWS) & innr.COPY_ROWS
    for name, ids in _index_lists(n, 14).items():
        got = view.rows(ids)
        assert got.shape == (len(ids), P) and bits_equal(got, rows[ids][:, :P]), (name, P, with_copy)
    view.close()
    vb.close()


@pytest.mark.parametrize("n,dim,with_copy,skew", [(257, 33, False, 0), (1000, 128, False, 0), (1000, 128, True, 0),
                                                  (1000, 128, True, 1), (4099, 100, True, 0), (257, 33, True, 0)])
def test_gather_device_entry(B, innr, lib, n, dim, with_copy, skew):
    """skew = 1: an output that is not 16-byte aligned, so the copy path's scalar form serves a D % 4 == 0 batch"""
    import torch
    rows = _rows(n, dim, 21 + n)
    vb = B.VerticalBatch.from_rows(rows)
    if with_copy:
        vb.build_copies(innr.COPY_ROWS)
    ids = np.random.default_rng(22).integers(0, n, 601)
    d_ids = torch.from_numpy(ids).to("cuda", torch.int64)
    got = vb.rows(d_ids)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (601, dim)
    assert bits_equal(got.cpu().numpy(), rows[ids])
    # the raw entry point writes exactly n*D floats
    sentinel = -12345.0
    out = torch.full((skew + 601 * dim + 64,), sentinel, dtype=torch.float32, device="cuda")
    vb._ctx.bind_torch_stream()
    st = lib.innr_batch_gather_rows_dev(vb._h, C.c_void_p(d_ids.data_ptr()), 601, C.c_void_p(out.data_ptr() + 4 * skew))
    assert st == 0
    host = out.cpu().numpy()
    assert bits_equal(host[skew:skew + 601 * dim].reshape(601, dim), rows[ids])
    assert (host[:skew] == sentinel).all() and (host[skew + 601 * dim:] == sentinel).all()
    assert vb.rows(torch.empty((0,), dtype=torch.int64, device="cuda")).shape == (0, dim)
    vb.close()


def test_extract_vector_and_get_do_not_download(B):
    n, dim = 300, 19
    rows = _rows(n, dim, 31)
    vb = B.VerticalBatch.from_rows(rows)
    for i in (0, 37, 299):
        assert bits_equal(vb.extract_vector(i), rows[i])
    assert vb.get(12, 37) == float(rows[37, 12]) and vb.get(0, 299) == float(rows[299, 0])
    assert vb._host is None
    with pytest.raises(IndexError):
        vb.extract_vector(n)
    data = vb.data()  # the cached host copy serves from now on, with the same values
    assert vb._host is data and bits_equal(vb.extract_vector(37), rows[37]) and vb.get(12, 37) == float(rows[37, 12])
    vb.close()


def _u8_corpus(n, dim):
    from innr_amd import scalar as S
    p = S.QuantizationParams.from_range(-1.0, 1.0)
    codes = np.random.default_rng(5).integers(0, 256, (n, dim)).astype(np.uint8)
    return S.QuantizedCorpus.from_codes(codes, n, dim, p)


def test_gather_errors_and_flag_reset(B, innr, lib):
    import torch
    from innr_amd._lib import E_BAD_ARG, InnrError
    from innr_amd import _lib
    n, dim = 257, 33
    rows = _rows(n, dim, 41)
    vb = B.VerticalBatch.from_rows(rows)
    vb.set_index_base(BASE)
    good = np.arange(BASE, BASE + 40, dtype=np.uint64)
    d_good = torch.from_numpy(good.astype(np.int64)).cuda()
    vb._ctx.bind_torch_stream()
    out = np.empty((40, dim), np.float32)
    d_out = torch.empty((40 * dim,), dtype=torch.float32, device="cuda")
    for bad in (BASE + n, BASE - 1):
        ids = good.copy()
        ids[17] = bad
        with pytest.raises(InnrError) as e:
            vb.rows(ids)
        assert e.value.status == E_BAD_ARG and str(BASE) in str(e.value) and str(BASE + n) in str(e.value)
        assert bits_equal(vb.rows(good), rows[:40])  # a valid call right after a failed one
        with pytest.raises(InnrError) as e:
            vb.rows(torch.from_numpy(ids.astype(np.int64)).cuda())
        assert e.value.status == E_BAD_ARG and str(BASE) in str(e.value) and str(BASE + n) in str(e.value)
        assert bits_equal(vb.rows(d_good).cpu().numpy(), rows[:40])  # the device flag was reset
    # the documented order of the checks, on both entry points
    qc = _u8_corpus(64, 16)
    for fn, ids_p, out_p in ((lib.innr_batch_gather_rows, _vp(good), _vp(out)),
                             (lib.innr_batch_gather_rows_dev, C.c_void_p(d_good.data_ptr()), C.c_void_p(d_out.data_ptr()))):
        assert fn(None, ids_p, 40, out_p) == E_BAD_ARG
        assert fn(qc._h, ids_p, 40, out_p) == E_BAD_ARG and "u8" in _lib.last_error()
        assert fn(qc._h, None, 0, None) == E_BAD_ARG  # the batch kind comes before the empty list
        assert fn(vb._h, None, 0, None) == 0
        assert fn(vb._h, None, 40, out_p) == E_BAD_ARG
        assert fn(vb._h, ids_p, 40, None) == E_BAD_ARG
        assert fn(vb._h, ids_p, 40, out_p) == 0
    assert bits_equal(out, rows[:40]) and bits_equal(d_out.cpu().numpy().reshape(40, dim), rows[:40])
    qc.close()
    vb.close()


# =============================================================================== k-NN of rows
N0, D0 = 2500, 37
TWINS = (5, 900, 1700)   # identical rows
ZEROS = (100, 2000)      # all-zero rows
METRICS = {"dot": "METRIC_DOT", "l2": "METRIC_L2SQ", "cos": "METRIC_COSINE"}
ORACLE = {"dot": oracle.batch_knn_dot, "l2": oracle.batch_knn, "cos": oracle.batch_knn_cosine}
ENGINES = ["KNN_AUTO", "KNN_EXACT", "KNN_MFMA", "KNN_MFMA_BF16", "KNN_MFMA_I8"]


def _base_rows():
    rows = np.random.default_rng(100).uniform(-1.0, 1.0, (N0, D0)).astype(np.float32)
    rows[TWINS[1]] = rows[TWINS[0]]
    rows[TWINS[2]] = rows[TWINS[0]]
    for z in ZEROS:
        rows[z] = 0.0
    return rows


class Corpus:
    """rows, their oracle layout, a resident batch; expected results are computed once per (metric, id, k, exclude)"""

    def __init__(self, B, rows, base=0):
        self.rows, self.data, self.base = rows, oracle.from_rows(rows), base
        self.vb = B.VerticalBatch.from_rows(rows)
        if base:
            self.vb.set_index_base(base)
        self.expected = functools.lru_cache(maxsize=None)(self._expected)

    def _expected(self, metric, i, k, exclude):
        n = self.rows.shape[0]
        if not exclude:
            oi, os_ = ORACLE[metric](self.rows[i], self.data, k)
            return np.asarray(oi, np.uint64) + np.uint64(self.base), np.asarray(os_, np.float32)
        oi, os_ = ORACLE[metric](self.rows[i], self.data, min(k + 1, n))
        return strip(np.asarray(oi, np.uint64) + np.uint64(self.base), np.asarray(os_, np.float32), i + self.base)


def strip(idx, sc, me):
    """one entry goes: the one whose index is `me`, else the last"""
    pos = np.flatnonzero(np.asarray(idx, np.uint64) == np.uint64(me))
    p = int(pos[0]) if pos.size else len(idx) - 1
    return np.delete(idx, p), np.delete(sc, p)


@pytest.fixture(scope="module")
def corpus(B):
    c = Corpus(B, _base_rows())
    yield c
    c.vb.close()


def _check_rows(B, innr, c, metric, ids, k, exclude, engine, stats=None):
    idx, sc = B.batch_knn_rows(np.asarray(ids) + c.base, c.vb, k, metric=getattr(innr, METRICS[metric]), exclude_self=exclude,
                               engine=engine, stats=stats)
    n = c.rows.shape[0]
    assert idx.shape == sc.shape == (len(ids), min(k, n - 1 if exclude else n)), (idx.shape, k, exclude)
    for j, i in enumerate(ids):
        oi, os_ = c.expected(metric, int(i), k, bool(exclude))
        assert same_knn(metric, idx[j], sc[j], oi, os_), (metric, k, exclude, engine, int(i), idx[j], oi, sc[j], os_)
        if exclude:
            assert int(i) + c.base not in [int(x) for x in idx[j]]
    return idx, sc


ID_LISTS = [[1234], [7, 2499, 7], [0, 311, 311, 2000, 42, 1999, 5, 0, 640, 17, 2498, 900, 1313]]  # Q = 1, 3, 13, duplicates among them


@pytest.mark.parametrize("metric", list(METRICS))
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("exclude", [0, 1])
def test_knn_rows_base_case(B, innr, corpus, metric, engine, exclude):
    """k = 10 and 50 only for the lists that query a twin or a zero row under squared L2: with k + 1 < 3 the oracle's top-(k + 1)
    cuts through a group of equal distances, whose members core's binary_search picks (test_knn_rows_duplicates covers k = 1
    there against the library's own order)"""
    for ids in ID_LISTS:
        for k in (1, 10, 50):
            if metric == "l2" and k == 1 and set(ids) & set(TWINS + ZEROS):
                continue
            _check_rows(B, innr, corpus, metric, ids, k, exclude, getattr(innr, engine))


def test_knn_rows_served_by_the_matrix_pipe(B, innr):
    n, dim, nq, k = 20001, 128, 130, 10
    rows = oracle.generate_uniform(n, dim, 77)
    c = Corpus(B, rows)
    ids = np.random.default_rng(78).integers(0, n, nq)
    for metric in ("dot", "l2"):
        st = innr.KnnStats()
        _check_rows(B, innr, c, metric, ids, k, 1, innr.KNN_MFMA, stats=st)
        assert st.engine == innr.KNN_MFMA and 0.0 < st.gemm_ms <= st.total_ms
    c.vb.close()


def test_knn_rows_self_absent_branch(B, innr):
    """Dot metric: eight rows scaled by 100 head every list (all values non-negative, so every dot product with them is large and
    positive), so with k + 1 <= 8 an ordinary vector is not among its own best and the LAST entry is the one that goes"""
    rows = np.abs(_base_rows())
    big = [3, 400, 801, 1202, 1603, 2004, 2405, 2499]
    rows[big] *= np.float32(100.0)
    c = Corpus(B, rows)
    ids = [10, 3, 1500, 2405, 11]
    k = 5
    absent = 0
    for i in ids:
        oi, os_ = oracle.batch_knn_dot(rows[i], c.data, k + 1)
        if i not in [int(x) for x in oi]:
            absent += 1
            ti, ts = oracle.batch_knn_dot(rows[i], c.data, k)
            ei, es = c.expected("dot", i, k, True)
            assert [int(x) for x in ei] == [int(x) for x in ti] and bits_equal(es, ts)  # the expectation IS the oracle's top-k
    assert absent >= 1
    for engine in ENGINES:
        idx, sc = B.batch_knn_rows(ids, c.vb, k, metric=innr.METRIC_DOT, exclude_self=True, engine=getattr(innr, engine))
        for j, i in enumerate(ids):
            oi, os_ = c.expected("dot", i, k, True)
            assert same_knn("dot", idx[j], sc[j], oi, os_), (engine, i, idx[j], oi)
    c.vb.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_knn_rows_duplicates(B, innr, corpus, engine):
    """Identical rows and all-zero rows, each queried: only the INDEX is excluded, equal vectors stay in, lower indices first"""
    eng = getattr(innr, engine)
    ids = list(TWINS) + list(ZEROS)
    for metric in ("dot", "cos"):
        for k in (1, 2, 10):
            _check_rows(B, innr, corpus, metric, ids, k, 1, eng)
    _check_rows(B, innr, corpus, "l2", ids, 10, 1, eng)
    # squared L2 against the library's own order among equal distances (ties to the lower index), not the oracle's
    for k in (1, 2, 10):
        idx, sc = B.batch_knn_rows(ids, corpus.vb, k, metric=innr.METRIC_L2SQ, exclude_self=True, engine=eng)
        fi, fs = B.knn_multi(innr.METRIC_L2SQ, corpus.rows[ids], corpus.vb, k + 1, engine=eng)
        for j, i in enumerate(ids):
            wi, ws = strip(fi[j], fs[j], i)
            assert [int(x) for x in idx[j]] == [int(x) for x in wi] and bits_equal(sc[j], ws), (engine, k, i, idx[j], wi)
    # the twins see each other at distance 0; with k = 1 the highest twin, whose own index is cut off, keeps the lowest
    idx, sc = B.batch_knn_rows(list(TWINS), corpus.vb, 1, metric=innr.METRIC_L2SQ, exclude_self=True, engine=eng)
    assert [int(r[0]) for r in idx] == [900, 5, 5] and (sc == 0.0).all()


def test_knn_rows_k_limits(B, innr, lib):
    n, dim = 260, 12
    rows = np.random.default_rng(200).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    c = Corpus(B, rows)
    ids = [0, 131, 259, 131]
    for metric in ("l2", "dot"):
        for k in (n, n + 5):  # k' = N - 1: everything but the query itself
            idx, _ = _check_rows(B, innr, c, metric, ids, k, 1, innr.KNN_AUTO)
            assert idx.shape[1] == n - 1
            idx, _ = _check_rows(B, innr, c, metric, ids, k, 0, innr.KNN_AUTO)
            assert idx.shape[1] == n
        for k in (239, 240, 250):  # exclude_self: 240 + 1 is past INNR_MAX_K already
            _check_rows(B, innr, c, metric, ids, k, 1, innr.KNN_AUTO)
            _check_rows(B, innr, c, metric, ids, k, 0, innr.KNN_AUTO)
    c.vb.close()
    # k = 300 of a larger corpus
    c = Corpus(B, np.random.default_rng(201).uniform(-1.0, 1.0, (700, 9)).astype(np.float32))
    _check_rows(B, innr, c, "l2", [5, 699], 300, 1, innr.KNN_AUTO)
    _check_rows(B, innr, c, "cos", [5, 699], 240, 1, innr.KNN_EXACT)
    for k, q in ((0, [1, 2]), (3, [])):
        idx, sc = B.batch_knn_rows(q, c.vb, k)
        assert idx.shape == sc.shape == (len(q), 0)
    c.vb.close()
    one = B.VerticalBatch.from_rows(rows[:1])
    idx, sc = B.batch_knn_rows([0, 0], one, 4, exclude_self=True)
    assert idx.shape == (2, 0)
    idx, sc = B.batch_knn_rows([0, 0], one, 4, exclude_self=False)
    assert idx.tolist() == [[0], [0]] and (sc == 0.0).all()
    one.close()


def test_knn_rows_more_than_one_round(B, innr):
    n, dim, k = 1000, 8, 5
    rows = np.random.default_rng(300).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    c = Corpus(B, rows)
    ids = np.random.default_rng(301).integers(0, n, 4100)  # 4096 + 4
    st, st_a, st_b = innr.KnnStats(), innr.KnnStats(), innr.KnnStats()
    idx, sc = B.batch_knn_rows(ids, c.vb, k, engine=innr.KNN_MFMA, stats=st)
    ia, sa = B.batch_knn_rows(ids[:4096], c.vb, k, engine=innr.KNN_MFMA, stats=st_a)
    ib, sb = B.batch_knn_rows(ids[4096:], c.vb, k, engine=innr.KNN_MFMA, stats=st_b)
    assert np.array_equal(idx, np.concatenate([ia, ib])) and bits_equal(sc, np.concatenate([sa, sb]))
    assert st.engine == st_b.engine and st.queries_fallback == st_a.queries_fallback + st_b.queries_fallback
    assert st.candidates_kept == max(st_a.candidates_kept, st_b.candidates_kept)
    assert st.gemm_ms > 0.0 and st_a.gemm_ms > 0.0 and st_b.gemm_ms > 0.0  # both rounds' filters are in the sum ...
    assert st.gemm_ms <= st.total_ms                                         # ... and the sum lies inside the whole call
    for j in range(0, 4100, 41):  # and every 41st against the oracle (the last round included)
        oi, os_ = c.expected("l2", int(ids[j]), k, True)
        assert same_knn("l2", idx[j], sc[j], oi, os_), j
    oi, os_ = c.expected("l2", int(ids[4099]), k, True)
    assert same_knn("l2", idx[4099], sc[4099], oi, os_)
    c.vb.close()


def test_knn_rows_round_shrinks_to_the_workspace_bound(B, innr):
    """k = 2^20 with exclude_self: a query's share is D*4 + (k + 1)*12 = 12 582 956 bytes, so 256 MiB hold a round of 21 queries,
    not 4096 (the bound goes by k + 1 as given, though N = 300 caps the lists): 50 ids run in three rounds"""
    n, dim, k = 300, 8, 1 << 20
    assert (256 << 20) // (dim * 4 + (k + 1) * 12) == 21
    rows = np.random.default_rng(310).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    c = Corpus(B, rows)
    ids = np.random.default_rng(311).integers(0, n, 50)
    from innr_amd import _lib
    ctx = _lib.default_context()
    ctx.trim()
    idx, _ = _check_rows(B, innr, c, "l2", ids, k, 1, innr.KNN_AUTO)
    assert idx.shape == (50, n - 1)
    assert ctx.memory() < (64 << 20)  # far inside the bound: the staged lists hold min(k + 1, N) entries
    _check_rows(B, innr, c, "dot", ids[:25], k, 1, innr.KNN_AUTO)
    c.vb.close()


def test_knn_rows_index_base_and_prefix_view(B, innr):
    rows = _base_rows()
    c = Corpus(B, rows, base=BASE)
    ids = [0, 2499, 5, 1700, 77]
    for metric in METRICS:
        idx, _ = _check_rows(B, innr, c, metric, ids, 10, 1, innr.KNN_AUTO)
        assert int(idx.min()) >= BASE and int(idx.max()) < BASE + N0
        _check_rows(B, innr, c, metric, ids, 10, 0, innr.KNN_EXACT)
    # a view of the first 20 dimensions: the queries are the view's rows
    view = c.vb.prefix(20)
    vdata = oracle.from_rows(np.ascontiguousarray(rows[:, :20]))
    for metric, exclude in (("l2", 1), ("dot", 0), ("cos", 1)):
        idx, sc = B.batch_knn_rows(np.asarray(ids) + BASE, view, 7, metric=getattr(innr, METRICS[metric]), exclude_self=bool(exclude))
        for j, i in enumerate(ids):
            q = np.ascontiguousarray(rows[i, :20])
            oi, os_ = ORACLE[metric](q, vdata, 8 if exclude else 7)
            oi = np.asarray(oi, np.uint64) + np.uint64(BASE)
            if exclude:
                oi, os_ = strip(oi, np.asarray(os_, np.float32), i + BASE)
            assert same_knn(metric, idx[j], sc[j], oi, os_), (metric, exclude, i)
    view.close()
    c.vb.close()


def test_knn_rows_device_entry(B, innr, lib, corpus):
    import torch
    ids = np.array([1234, 5, 5, 2000, 2499, 900, 64], dtype=np.int64)
    d_ids = torch.from_numpy(ids).cuda()
    for metric in METRICS:
        m = getattr(innr, METRICS[metric])
        for exclude, k in ((True, 10), (False, 10), (True, 250)):
            hi, hs = B.batch_knn_rows(ids, corpus.vb, k, metric=m, exclude_self=exclude)
            di, ds = B.batch_knn_rows(d_ids, corpus.vb, k, metric=m, exclude_self=exclude)
            assert di.is_cuda and di.dtype == torch.int64 and ds.dtype == torch.float32
            assert np.array_equal(di.cpu().numpy().astype(np.uint64), hi) and bits_equal(ds.cpu().numpy(), hs)
    # the raw entry point writes exactly Q*k' entries
    q, k = len(ids), 10
    oi = torch.full((q * k + 64,), -7, dtype=torch.int64, device="cuda")
    os_ = torch.full((q * k + 64,), -7.0, dtype=torch.float32, device="cuda")
    out_k = C.c_size_t(99)
    corpus.vb._ctx.bind_torch_stream()
    st = lib.innr_batch_knn_rows_dev(corpus.vb._h, innr.METRIC_L2SQ, C.c_void_p(d_ids.data_ptr()), q, k, 1, innr.KNN_AUTO,
                                     C.c_void_p(oi.data_ptr()), C.c_void_p(os_.data_ptr()), C.byref(out_k), None)
    assert st == 0 and out_k.value == k
    hi, hs = B.batch_knn_rows(ids, corpus.vb, k)
    assert np.array_equal(oi.cpu().numpy()[:q * k].reshape(q, k).astype(np.uint64), hi)
    assert bits_equal(os_.cpu().numpy()[:q * k].reshape(q, k), hs)
    assert (oi.cpu().numpy()[q * k:] == -7).all() and (os_.cpu().numpy()[q * k:] == -7.0).all()


def test_knn_graph(B, innr, corpus):
    k = 5
    gi, gs = B.batch_knn_graph(corpus.vb, k)
    assert gi.shape == gs.shape == (N0, k) and gi.dtype == np.uint64 and gs.dtype == np.float32
    assert not (gi == np.arange(N0, dtype=np.uint64)[:, None]).any()  # no row contains its own index
    for i0 in range(0, N0, 500):  # every row equals the per-id call
        ids = np.arange(i0, i0 + 500)
        idx, sc = B.batch_knn_rows(ids, corpus.vb, k)
        assert np.array_equal(gi[i0:i0 + 500], idx) and bits_equal(gs[i0:i0 + 500], sc)
    for i in (0, 5, 900, 1700, 100, 2000, 2499, 1234):  # and a few against the oracle
        oi, os_ = corpus.expected("l2", i, 10, True)  # (k + 1 = 11 holds every group of equal distances whole)
        assert bits_equal(gs[i], os_[:k])
    pi, ps = B.batch_knn_graph(corpus.vb, k, metric=innr.METRIC_DOT, engine=innr.KNN_EXACT, first=2400, count=60)
    idx, sc = B.batch_knn_rows(np.arange(2400, 2460), corpus.vb, k, metric=innr.METRIC_DOT, engine=innr.KNN_EXACT)
    assert np.array_equal(pi, idx) and bits_equal(ps, sc)
    with pytest.raises(IndexError):
        B.batch_knn_graph(corpus.vb, k, first=2400, count=101)


def test_knn_rows_errors(B, innr, lib, corpus):
    import torch
    from innr_amd._lib import E_BAD_ARG, InnrError
    from innr_amd import _lib
    vb = corpus.vb
    for bad in (N0, 2 ** 40):
        with pytest.raises(InnrError) as e:
            B.batch_knn_rows([3, bad, 4], vb, 5)
        assert e.value.status == E_BAD_ARG and f"[0, {N0})" in str(e.value)
        with pytest.raises(InnrError) as e:
            B.batch_knn_rows(torch.tensor([3, bad, 4], dtype=torch.int64, device="cuda"), vb, 5)
        assert e.value.status == E_BAD_ARG and f"[0, {N0})" in str(e.value)
        _check_rows(B, innr, corpus, "l2", [3, 4], 5, 1, innr.KNN_AUTO)  # a valid call right after
    ids = np.array([3, 4], dtype=np.uint64)
    oi, os_ = np.empty(10, np.uint64), np.empty(10, np.float32)
    d_ids = torch.from_numpy(ids.astype(np.int64)).cuda()
    d_oi, d_os = torch.empty(10, dtype=torch.int64, device="cuda"), torch.empty(10, dtype=torch.float32, device="cuda")
    qc = _u8_corpus(64, 16)
    out_k = C.c_size_t(99)
    vb._ctx.bind_torch_stream()
    for fn, ip, op, sp in ((lib.innr_batch_knn_rows, _vp(ids), _vp(oi), _vp(os_)),
                           (lib.innr_batch_knn_rows_dev, C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_oi.data_ptr()),
                            C.c_void_p(d_os.data_ptr()))):
        L2, AUTO = innr.METRIC_L2SQ, innr.KNN_AUTO
        assert fn(None, L2, ip, 2, 5, 1, AUTO, op, sp, C.byref(out_k), None) == E_BAD_ARG
        assert fn(vb._h, L2, ip, 2, 5, 1, AUTO, op, sp, None, None) == E_BAD_ARG
        assert fn(qc._h, L2, ip, 2, 5, 1, AUTO, op, sp, C.byref(out_k), None) == E_BAD_ARG and "u8" in _lib.last_error()
        assert fn(vb._h, 7, ip, 2, 5, 1, AUTO, op, sp, C.byref(out_k), None) == E_BAD_ARG
        assert fn(vb._h, 7, None, 0, 5, 1, AUTO, None, None, C.byref(out_k), None) == E_BAD_ARG  # the metric comes before Q == 0
        for q, k in ((0, 5), (2, 0)):
            out_k.value = 99
            assert fn(vb._h, L2, None, q, k, 1, AUTO, None, None, C.byref(out_k), None) == 0 and out_k.value == 0
        assert fn(vb._h, L2, None, 2, 5, 1, AUTO, op, sp, C.byref(out_k), None) == E_BAD_ARG
        assert fn(vb._h, L2, ip, 2, 5, 1, AUTO, None, sp, C.byref(out_k), None) == E_BAD_ARG
        assert fn(vb._h, L2, ip, 2, 5, 1, AUTO, op, None, C.byref(out_k), None) == E_BAD_ARG
        assert fn(vb._h, L2, ip, 2, 5, 1, AUTO, op, sp, C.byref(out_k), None) == 0 and out_k.value == 5
    assert np.array_equal(oi.reshape(2, 5), d_oi.cpu().numpy().reshape(2, 5).astype(np.uint64))
    qc.close()


def test_workspace_is_counted_and_trimmed(B, innr, corpus):
    from innr_amd import _lib
    ctx = _lib.default_context()
    ctx.trim()
    floor = ctx.memory()
    B.batch_knn_rows(np.arange(64), corpus.vb, 10)
    corpus.vb.rows(np.arange(64))
    assert ctx.memory() >= floor + 64 * D0 * 4 + 64 * 11 * 12  # the gathered rows and the staged lists at least
    ctx.trim()
    assert ctx.memory() == floor
    _check_rows(B, innr, corpus, "l2", [1, 2, 3], 10, 1, innr.KNN_AUTO)  # and everything comes back on demand
