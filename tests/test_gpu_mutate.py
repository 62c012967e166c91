"""GPU tests of the entry points that change a resident f32 batch in place (innr_amd/csrc/mutate.hip):
innr_batch_append_rows / _update_rows / _keep_rows and their _dev twins. The contract under test is one sentence: after a change
the batch answers, on every entry point and engine, exactly as a fresh batch uploaded with the final rows -- indices position for
position, score bits -- and after a refused call it is exactly as before. Expected stores are plain NumPy edits of the uploaded
rows; expected answers are a fresh upload's and, for the exact engine, the CPU oracle's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal, same_knn

BASE = 10 ** 9
E_DIM_MISMATCH, E_BAD_ARG = -1, -2
# -NaN and +NaN with payloads, a signalling pattern, -0.0, denormals of both signs, +-inf
SPECIALS = (0xFFC12345, 0x7FC54321, 0x7F812345, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000)
METRICS = {"dot": 0, "l2": 1, "cosine": 2}
ORACLE_KNN = {"dot": oracle.batch_knn_dot, "l2": oracle.batch_knn, "cosine": oracle.batch_knn_cosine}


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


@pytest.fixture(scope="module")
def last_error():
    from innr_amd import _lib
    return _lib.last_error


def _uniform(n, dim, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def _round_up(x, m):
    return (x + m - 1) // m * m


def _store(vb):
    """the store as it is on the device now (never the cached host copy)"""
    vb._host = None
    return vb.data().copy()


def assert_like_fresh(B, vb, rows, what, base=0):
    """store, rows read back, norms and memory report of `vb` against a fresh upload of `rows`"""
    n, dim = rows.shape
    assert vb.num_vectors() == n and vb.dimension() == dim, what
    fresh = B.VerticalBatch.from_rows(rows) if n else B.VerticalBatch.from_flat(np.empty(0, np.float32), 0, dim)
    assert bits_equal(_store(vb), rows.T), what
    assert bits_equal(_store(vb), fresh.data()), what
    if n and dim:
        assert bits_equal(vb.rows(np.arange(n) + base), rows), what
    m, fm = vb.memory(), fresh.memory()
    assert m.corpus_bytes == fm.corpus_bytes == _round_up(max(n, 1), 256) * _round_up(max(dim, 1), 32) * 4, what
    if n:
        assert bits_equal(B.batch_norms(vb), B.batch_norms(fresh)), what
    fresh.close()


def assert_nothing_derived(vb, what):
    m = vb.memory()
    assert m.derived_bytes == 0 and m.aux_bytes == 0 and m.present_mask == 0, (what, m)


# =============================================================================== 1. layout
def test_append_in_place_then_reallocating(B, innr):
    """N = 1000, D = 40 (Dpad = 64 > D): 10 rows fit the padding of ldN = 1024, 300 more move the store to ldN = 1536"""
    rows = _uniform(1000, 40, 1)
    vb = B.VerticalBatch.from_rows(rows)
    B.batch_norms(vb)
    vb.build_copies(innr.COPY_ALL)
    before = vb.memory()
    assert before.present_mask and before.aux_bytes and before.corpus_bytes == 1024 * 64 * 4
    more = _uniform(10, 40, 2)
    vb.append(more)
    assert_nothing_derived(vb, "append 10")
    assert vb.memory().corpus_bytes == before.corpus_bytes  # in place: the store did not move or grow
    rows = np.vstack([rows, more])
    assert_like_fresh(B, vb, rows, "append 10")
    vb.build_copies(innr.COPY_ALL)
    more = _uniform(300, 40, 3)
    vb.append(more)
    assert_nothing_derived(vb, "append 300")
    assert vb.memory().corpus_bytes == 1536 * 64 * 4
    rows = np.vstack([rows, more])
    assert_like_fresh(B, vb, rows, "append 300")
    vb.close()


def test_append_at_a_256_boundary_and_to_an_empty_batch(B):
    rows = _uniform(1024, 40, 4)
    vb = B.VerticalBatch.from_rows(rows)
    one = _uniform(1, 40, 5)
    vb.append(one)
    assert_nothing_derived(vb, "append at 1024")
    assert_like_fresh(B, vb, np.vstack([rows, one]), "append at 1024")
    vb.close()
    empty = B.VerticalBatch.from_flat(np.empty(0, np.float32), 0, 64)
    assert empty.num_vectors() == 0 and empty.dimension() == 64
    few = _uniform(7, 64, 6)
    empty.append(few)  # inside the padding of an empty batch's 256 columns
    assert_like_fresh(B, empty, few, "append to empty")
    many = _uniform(300, 64, 7)
    empty.append(many)
    assert_like_fresh(B, empty, np.vstack([few, many]), "append to empty, reallocating")
    empty.append(np.empty((0, 64), np.float32))  # n == 0: nothing touched
    assert empty.num_vectors() == 307
    empty.close()


def test_append_in_staging_rounds(B, ctx_option):
    """the host entry point in rounds of 64 rows, in place and reallocating: the column offset of every round"""
    ctx_option("mutate_round", 64)
    rows = _uniform(1000, 40, 8)
    vb = B.VerticalBatch.from_rows(rows)
    a, b = _uniform(20, 40, 9), _uniform(333, 40, 10)
    vb.append(a)
    vb.append(b)
    assert_like_fresh(B, vb, np.vstack([rows, a, b]), "rounds of 64")
    vb.close()


# =============================================================================== 2. bit patterns
def test_bit_patterns_arrive_unchanged(B):
    n, dim = 1000, 40
    rows = _uniform(n, dim, 11)
    vb = B.VerticalBatch.from_rows(rows)
    special = _uniform(3, dim, 12)
    bits = special.view(np.uint32)
    for j, pat in enumerate(SPECIALS):
        bits[j % 3, (j * 7) % dim] = np.uint32(pat)
    vb.append(special)
    assert bits_equal(vb.rows(np.arange(n, n + 3)), special)
    ids = np.array([999, 0, 513])
    vb.update_rows(ids, special[::-1])
    assert bits_equal(vb.rows(ids), special[::-1])
    rows[ids] = special[::-1]
    assert bits_equal(_store(vb), np.vstack([rows, special]).T)
    vb.close()


# =============================================================================== 3. stale copies
def _check_every_engine(B, innr, vb, rows, queries, name, what, k=10):
    """every engine's answer on `vb` against a fresh batch of `rows`; the exact engine's also against the oracle"""
    fresh = B.VerticalBatch.from_rows(rows)
    data = oracle.from_rows(rows)
    results = {}
    for engine in (innr.KNN_EXACT, innr.KNN_MFMA, innr.KNN_MFMA_BF16, innr.KNN_MFMA_I8):
        idx, sc = B.knn_multi(METRICS[name], queries, vb, k, engine=engine)
        fidx, fsc = B.knn_multi(METRICS[name], queries, fresh, k, engine=engine)
        assert np.array_equal(idx, fidx) and bits_equal(sc, fsc), (what, name, engine)
        results[engine] = idx
    idx, sc = B.knn_multi(METRICS[name], queries, vb, k, engine=innr.KNN_EXACT)
    for j in range(len(queries)):
        oi, os_ = ORACLE_KNN[name](queries[j], data, k)
        assert same_knn(name, idx[j], sc[j], oi, os_), (what, name, j)
    fresh.close()
    return results[innr.KNN_EXACT]


@pytest.mark.parametrize("name", list(METRICS))
def test_no_engine_answers_from_a_stale_copy(B, innr, name):
    """Copies, norms and quantisation ranges are built, then rows change so that new rows become top hits and old top hits go:
    an engine that still read a copy, a norm or a range of the old rows would miss them. The planted row of query j is 2 q_j for
    dot and cosine; under squared L2 that row lies |q_j|^2 away, which is about what the nearest of 3000 uniform rows reaches, so
    there the planted row is q_j itself (distance 0): the best vector of the query under its metric either way."""
    n, dim, nq = 3000, 64, 130
    scale = np.float32(1.0 if name == "l2" else 2.0)
    rows = _uniform(n, dim, 20)
    queries = _uniform(nq, dim, 21)
    vb = B.VerticalBatch.from_rows(rows)
    assert vb.build_copies(innr.COPY_ALL)
    _check_every_engine(B, innr, vb, rows, queries, name, "as uploaded")
    assert vb.memory().present_mask
    # update: row u_j becomes the planted row of query j
    upd = np.array([5, 700, 2999, 1024, 31, 32, 2047, 1500, 256, 1])
    rows[upd] = scale * queries[:10]
    vb.update_rows(upd, scale * queries[:10])
    assert_nothing_derived(vb, "update")
    top = _check_every_engine(B, innr, vb, rows, queries, name, "updated")
    assert top[:10, 0].tolist() == upd.tolist()
    # append: the same for queries 10 .. 29, past the padding (3000 + 100 > 3072)
    vb.build_copies(innr.COPY_ALL)
    more = np.vstack([scale * queries[10:30], _uniform(80, dim, 22)])
    rows = np.vstack([rows, more])
    vb.append(more)
    assert_nothing_derived(vb, "append")
    top = _check_every_engine(B, innr, vb, rows, queries, name, "appended")
    assert top[10:30, 0].tolist() == list(range(n, n + 20))
    # keep: the top hits of queries 0 .. 4 and 10 .. 14 go, and every 7th row
    vb.build_copies(innr.COPY_ALL)
    mask = np.ones(len(rows), np.uint8)
    mask[::7] = 0
    mask[upd[:5]] = 0
    mask[n:n + 5] = 0
    assert vb.keep(mask) == int(mask.sum())
    assert_nothing_derived(vb, "keep")
    rows = rows[mask != 0]
    top = _check_every_engine(B, innr, vb, rows, queries, name, "kept")
    new_index = np.cumsum(mask) - 1
    assert top[5:10, 0].tolist() == [int(new_index[u]) for u in upd[5:]]  # the surviving planted rows, at their new indices
    vb.close()


# =============================================================================== 4. the other entry points after a change
def test_other_entry_points_after_a_change(B, innr):
    n, dim = 2000, 40
    rows = _uniform(n, dim, 30)
    queries = _uniform(9, dim, 31)
    vb = B.VerticalBatch.from_rows(rows)
    # state of the old rows: a kept selection for the old N, the dimension variances, norms
    old_mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    B.batch_knn_filtered_multi(queries, vb, 5, old_mask, engine=innr.KNN_MFMA)
    assert vb.memory().present_mask & innr.COPY_SELECTION
    B.batch_dimension_variance(vb)
    B.batch_knn_reordered(queries[0], vb, 5)
    # change: rows that reorder the variances (dimension 39 becomes the widest), fewer rows than before
    more = _uniform(400, dim, 32)
    more[:, 39] *= 50.0
    vb.append(more)
    upd = np.array([0, 1999, 2399, 777])
    new = _uniform(4, dim, 33)
    vb.update_rows(upd, new)
    rows = np.vstack([rows, more])
    rows[upd] = new
    keep = np.ones(len(rows), np.uint8)
    keep[100:1100:2] = 0
    vb.keep(keep)
    rows = rows[keep != 0]
    fresh = B.VerticalBatch.from_rows(rows)
    nn = len(rows)
    assert vb.num_vectors() == nn
    for name, metric in METRICS.items():
        d0 = ORACLE_KNN[name](queries[0], oracle.from_rows(rows), 30)[1][-1]
        thr = np.full(len(queries), d0, np.float32)
        for a, b in zip(B.batch_range_search(queries, vb, thr, metric=metric), B.batch_range_search(queries, fresh, thr, metric=metric)):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), ("range", name)
        mask = (np.arange(nn) % 5 != 1).astype(np.uint8)
        for engine in (innr.KNN_EXACT, innr.KNN_MFMA):
            gi, gs = B.batch_knn_filtered_multi(queries, vb, 7, mask, metric=metric, engine=engine)
            fi, fs = B.batch_knn_filtered_multi(queries, fresh, 7, mask, metric=metric, engine=engine)
            assert np.array_equal(gi, fi) and bits_equal(gs, fs), ("filtered", name, engine)
        ids = np.array([0, nn - 1, 1234, 99])
        gi, gs = B.batch_knn_rows(ids, vb, 6, metric=metric, exclude_self=True)
        fi, fs = B.batch_knn_rows(ids, fresh, 6, metric=metric, exclude_self=True)
        assert np.array_equal(gi, fi) and bits_equal(gs, fs), ("knn_rows", name)
    var, fvar = B.batch_dimension_variance(vb), B.batch_dimension_variance(fresh)
    assert bits_equal(var, fvar) and bits_equal(var, oracle.batch_dimension_variance(oracle.from_rows(rows)))
    assert int(np.argmax(var)) == 39
    for j in range(3):
        g, f = B.batch_knn_reordered(queries[j], vb, 8), B.batch_knn_reordered(queries[j], fresh, 8)
        assert g.indices == f.indices and bits_equal(g.scores, f.scores), "reordered"
        g, f = B.batch_knn_adaptive(queries[j], vb, 8, 16), B.batch_knn_adaptive(queries[j], fresh, 8, 16)
        assert g.indices == f.indices and bits_equal(g.scores, f.scores), "adaptive"
    fresh.close()
    vb.close()


# =============================================================================== 5. update: validation
def test_update_accepts_any_order_every_row_and_an_index_base(B):
    n, dim = 1000, 40
    rows = _uniform(n, dim, 40)
    vb = B.VerticalBatch.from_rows(rows)
    vb.set_index_base(BASE)
    perm = np.random.default_rng(41).permutation(n)
    new = _uniform(n, dim, 42)
    vb.update_rows(perm + BASE, new)  # n = N, shuffled: every row is written
    rows[perm] = new
    assert_like_fresh(B, vb, rows, "every row", base=BASE)
    few = np.array([999, 0, 500])
    vb.update_rows(few + BASE, rows[few] * 3.0)
    rows[few] *= 3.0
    assert_like_fresh(B, vb, rows, "three rows", base=BASE)
    idx, _ = B.knn_multi(METRICS["l2"], rows[few], vb, 1)
    assert idx[:, 0].tolist() == (few + BASE).tolist()  # the base is still the batch's
    vb.close()


@pytest.mark.parametrize("case", ["below_base", "beyond_end", "dup_two_tiles", "dup_two_rounds", "dup_adjacent"])
def test_update_refuses_bad_indices_and_writes_nothing(B, innr, last_error, ctx_option, case):
    from innr_amd import InnrError
    n, dim = 1000, 40
    vb = B.VerticalBatch.from_rows(_uniform(n, dim, 43))
    vb.set_index_base(BASE)
    vb.build_copies(innr.COPY_BF16_DOT)
    before, mem = _store(vb), vb.memory()
    ids = np.random.default_rng(44).permutation(n)[:200].astype(np.int64) + BASE
    kind = "more than once"
    if case == "below_base":
        ids[150], kind = BASE - 1, "outside"
    elif case == "beyond_end":
        ids[199], kind = BASE + n, "outside"
    elif case == "dup_two_tiles":
        ids[70] = ids[5]    # positions in different tiles of 32 indices
    elif case == "dup_two_rounds":
        ctx_option("mutate_round", 64)
        ids[150] = ids[3]   # positions in different staging rounds of 64 rows
    else:
        ids[8] = ids[7]
    with pytest.raises(InnrError) as e:
        vb.update_rows(ids, _uniform(200, dim, 45))
    assert e.value.status == E_BAD_ARG and kind in str(e.value) and "update_rows" in str(e.value), str(e.value)
    if kind == "outside":
        assert str(int(ids[150] if case == "below_base" else ids[199])) in str(e.value)
    assert bits_equal(_store(vb), before) and vb.memory() == mem  # the store and the derived state as before
    vb.close()


def test_update_device_entry_refuses_bad_indices(B, last_error):
    import torch
    from innr_amd import InnrError
    n, dim = 1000, 40
    vb = B.VerticalBatch.from_rows(_uniform(n, dim, 46))
    before = _store(vb)
    new = torch.from_numpy(_uniform(100, dim, 47)).cuda()
    for bad, kind in ((n, "outside"), (17, "more than once")):
        ids = np.arange(100, dtype=np.int64) * 3
        ids[40] = bad if kind == "outside" else ids[bad]
        with pytest.raises(InnrError) as e:
            vb.update_rows(torch.from_numpy(ids).cuda(), new)
        assert e.value.status == E_BAD_ARG and kind in str(e.value)
        assert bits_equal(_store(vb), before)
    vb.close()


# =============================================================================== 6. keep
def test_keep_compacts_in_index_order(B, innr):
    n, dim = 3500, 64
    rows = _uniform(n, dim, 50)
    vb = B.VerticalBatch.from_rows(rows)
    vb.build_copies(innr.COPY_ALL)
    B.batch_norms(vb)
    mem = vb.memory()
    assert vb.keep(np.ones(n, np.uint8)) == n  # every row stays: nothing changes, nothing is dropped
    assert vb.memory() == mem and vb.num_vectors() == n
    mask = np.ones(n, bool)
    mask[::3] = False          # every 3rd row
    mask[1000:1300] = False    # a run across chunk boundaries
    mask[0] = mask[n - 1] = False
    assert vb.keep(mask) == int(mask.sum())
    assert_nothing_derived(vb, "keep")
    kept = rows[mask]
    assert_like_fresh(B, vb, kept, "keep")
    # rank among the kept: a row that stayed is found at the number of kept rows below it
    new_index = np.cumsum(mask) - 1
    probe = np.array([1, 998, 1301, n - 3])
    assert mask[probe].all()
    idx, sc = B.knn_multi(METRICS["l2"], rows[probe], vb, 1, engine=innr.KNN_EXACT)
    assert idx[:, 0].tolist() == new_index[probe].tolist() and not sc.any()
    # remove(): the same through a list of indices
    gone = np.array([0, 5, 5, len(kept) - 1])
    assert vb.remove(gone) == len(kept) - 3
    assert_like_fresh(B, vb, np.delete(kept, [0, 5, len(kept) - 1], axis=0), "remove")
    vb.close()


def test_keep_none_leaves_an_empty_batch(B, innr):
    n, dim = 1000, 40
    vb = B.VerticalBatch.from_rows(_uniform(n, dim, 51))
    assert vb.keep(np.zeros(n, np.uint8)) == 0
    assert vb.num_vectors() == 0 and vb.dimension() == dim
    assert vb.memory().corpus_bytes == 256 * 64 * 4
    idx, sc = B.knn_multi(METRICS["dot"], _uniform(3, dim, 52), vb, 5)
    assert idx.shape == (3, 0) and sc.shape == (3, 0)  # *out_k == 0
    assert vb.keep(np.zeros(0, np.uint8)) == 0  # N == 0: nothing to do
    back = _uniform(5, dim, 53)
    vb.append(back)
    assert_like_fresh(B, vb, back, "append after keep-none")
    vb.close()


def test_keep_out_n_may_be_null(B, lib):
    n, dim = 1000, 40
    rows = _uniform(n, dim, 54)
    vb = B.VerticalBatch.from_rows(rows)
    mask = (np.arange(n) % 2).astype(np.uint8)
    assert lib.innr_batch_keep_rows(vb._h, _vp(mask), None) == 0
    assert lib.innr_batch_num_vectors(vb._h) == 500
    vb._changed()
    assert_like_fresh(B, vb, rows[1::2], "keep, out_n null")
    vb.close()


# =============================================================================== 7. device variants
def test_device_variants_give_the_host_path_bits(B):
    import torch
    n, dim = 1000, 40
    rows = _uniform(n, dim, 60)
    more = _uniform(333, dim, 61)
    more.view(np.uint32)[3, 3] = np.uint32(SPECIALS[0])
    ids = np.random.default_rng(62).permutation(n + 333)[:150]
    new = _uniform(150, dim, 63)
    new.view(np.uint32)[7, 39] = np.uint32(SPECIALS[2])
    mask = np.random.default_rng(64).uniform(size=n + 333) < 0.6
    host, dev = B.VerticalBatch.from_rows(rows), B.VerticalBatch.from_rows(rows)
    host.append(more[:10])
    host.append(more[10:])
    dev.append(torch.from_numpy(more[:10]).cuda())   # in place
    dev.append(torch.from_numpy(more[10:]).cuda())   # reallocating
    assert bits_equal(_store(dev), _store(host)) and dev.num_vectors() == n + 333
    host.update_rows(ids, new)
    dev.update_rows(torch.from_numpy(ids).cuda(), torch.from_numpy(new).cuda())
    assert bits_equal(_store(dev), _store(host))
    assert host.keep(mask) == dev.keep(torch.from_numpy(mask).cuda()) == int(mask.sum())
    assert bits_equal(_store(dev), _store(host))
    final = np.vstack([rows, more])
    final[ids] = new
    assert_like_fresh(B, dev, final[mask], "device variants")
    host.close()
    dev.close()


# =============================================================================== 8. refusals
def test_code_batches_views_and_wrong_dimensions_are_refused(B, lib, last_error):
    from innr_amd import InnrError, InnrPanic
    from innr_amd import scalar as S
    n, dim = 1000, 40
    rows = _uniform(n, dim, 70)
    buf, idx, mask, out_n = _uniform(2, dim, 71), np.array([0, 1], np.uint64), np.ones(n, np.uint8), C.c_size_t(0)
    p = S.QuantizationParams.from_range(-1.0, 1.0)
    qc = S.QuantizedCorpus.from_codes(oracle.quantize_u8(rows, oracle.QParams(p.alpha, p.offset)), n, dim, p)
    vb = B.VerticalBatch.from_rows(rows)
    view = vb.prefix(32)
    for h, word in ((qc._h, "u8"), (view._h, "view")):
        assert lib.innr_batch_append_rows(h, _vp(buf), 2, dim) == E_BAD_ARG and word in last_error()
        assert lib.innr_batch_update_rows(h, _vp(idx), _vp(buf), 2, dim) == E_BAD_ARG and word in last_error()
        assert lib.innr_batch_keep_rows(h, _vp(mask), C.byref(out_n)) == E_BAD_ARG and word in last_error()
    with pytest.raises(InnrError):
        view.append(buf[:, :32])
    # the parent of an open view: the Python class raises before the call (the store would move under the view)
    before = _store(vb)
    for call in (lambda: vb.append(buf), lambda: vb.update_rows(idx, buf), lambda: vb.keep(mask[::-1] * 0), lambda: vb.remove([3])):
        with pytest.raises(InnrError) as e:
            call()
        assert "open prefix view" in str(e.value)
    assert vb.num_vectors() == n and bits_equal(_store(vb), before)
    view.close()
    vb.append(buf)  # with the view closed the same call goes through
    assert vb.num_vectors() == n + 2
    # a wrong D
    assert lib.innr_batch_append_rows(vb._h, _vp(buf), 2, dim - 1) == E_DIM_MISMATCH
    assert lib.innr_batch_update_rows(vb._h, _vp(idx), _vp(buf), 2, dim + 1) == E_DIM_MISMATCH
    assert lib.innr_batch_append_rows(vb._h, None, 0, dim + 1) == E_DIM_MISMATCH  # before "n == 0: nothing to do"
    with pytest.raises(InnrPanic):
        vb.append(_uniform(3, dim, 72).reshape(-1)[:-1])
    empty0 = B.VerticalBatch.from_rows([])  # created with D = 0: rows of any other dimension are a mismatch
    assert lib.innr_batch_append_rows(empty0._h, _vp(buf), 2, dim) == E_DIM_MISMATCH
    # null pointers with work to do
    assert lib.innr_batch_append_rows(vb._h, None, 2, dim) == E_BAD_ARG
    assert lib.innr_batch_update_rows(vb._h, None, _vp(buf), 2, dim) == E_BAD_ARG
    assert lib.innr_batch_keep_rows(vb._h, None, None) == E_BAD_ARG
    assert vb.num_vectors() == n + 2
    for b in (empty0, vb, qc):
        b.close()
