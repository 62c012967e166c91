"""GPU tests of the entry points that change a resident u8 code batch in place (innr_amd/csrc/mutate_u8.hip):
innr_batch_append_codes / _update_codes / _keep_codes, the variants fed f32 rows (innr_batch_append_quantized / _update_quantized)
and their _dev twins, through scalar.QuantizedCorpus. The contract under test is one sentence: after a change the corpus answers, on
every entry point and engine, exactly as a fresh corpus uploaded with the final codes -- indices position for position, score bits
-- and after a refused call it is exactly as before. Expected stores are plain NumPy edits of the uploaded codes; expected answers
are a fresh QuantizedCorpus.from_codes' and the CPU oracle's (quantize_u8, asymmetric_dot_u8). Equality of bytes throughout: no
tolerance is involved."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle

BASE = 10 ** 9
OK, E_DIM_MISMATCH, E_BAD_ARG, E_UNSUPPORTED = 0, -1, -2, -6
ALPHA, OFFSET = 2.0, -1.0


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


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


def _codes(n, dim, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, dim), dtype=np.uint8)


def _uniform(n, dim, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def _round_up(x, m):
    return (x + m - 1) // m * m


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _params(S, alpha=ALPHA, offset=OFFSET):
    return S.QuantizationParams(alpha, offset)


def _corpus(S, codes, base=0, p=None):
    n, dim = codes.shape
    qc = S.QuantizedCorpus.from_codes(codes, n, dim, p or _params(S))
    if base:
        qc.set_index_base(base)
    return qc


def _store_bytes(n, dim):
    return _round_up(max(n, 1), 1024) * _round_up(max(dim, 1), 32)


def assert_like_fresh(S, qc, codes, what, base=0, p=None):
    """the codes read back and the memory report of `qc` against a fresh upload of `codes`: nothing derived is left"""
    n, dim = codes.shape
    assert len(qc) == n and qc.dimension() == dim, what
    fresh = _corpus(S, codes, base, p)
    got = qc.codes()
    assert np.array_equal(got, codes), what
    assert np.array_equal(got, fresh.codes()), what
    m, fm = qc.memory(), fresh.memory()
    assert m == fm and m.corpus_bytes == _store_bytes(n, dim), (what, m, fm)
    assert m.derived_bytes == 0 and m.present_mask == 0, (what, m)
    fresh.close()


def _derive(innr, qc, nq=4):
    """the int8 copy and a kept selection: what a change must drop and a refused call must leave"""
    n, dim = len(qc), qc.dimension()
    assert qc.build_copies(innr.COPY_I8_DOT) & innr.COPY_I8_DOT
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    qc.knn_filtered_multi(_uniform(nq, dim, 900), 5, mask, engine=innr.KNN_MFMA_I8)
    m = qc.memory()
    assert m.present_mask & innr.COPY_I8_DOT and m.present_mask & innr.COPY_SELECTION and m.derived_bytes, m
    return m


# =============================================================================== 1. append, layout
def test_append_in_place_then_reallocating(S, innr):
    """N = 1000, D = 40 (Dpad = 64 > D): 10 rows fit the padding of ldN = 1024, 300 more move the store to ldN = 2048"""
    codes = _codes(1000, 40, 1)
    qc = _corpus(S, codes)
    before = _derive(innr, qc)
    assert before.corpus_bytes == 1024 * 64
    more = _codes(10, 40, 2)
    qc.append_codes(more)
    assert qc.memory().corpus_bytes == 1024 * 64  # in place: the store did not move or grow
    codes = np.vstack([codes, more])
    assert_like_fresh(S, qc, codes, "append 10")
    _derive(innr, qc)
    more = _codes(300, 40, 3)
    qc.append_codes(more)
    assert qc.memory().corpus_bytes == 2048 * 64
    codes = np.vstack([codes, more])
    assert_like_fresh(S, qc, codes, "append 300")
    qc.close()


@pytest.mark.parametrize("n0,dim", [(1001, 40), (1003, 40), (1001, 33), (1003, 1), (1019, 33)])
def test_append_at_byte_columns_not_aligned_to_four(S, n0, dim):
    """the column the rows go to is a byte column: N = 1001 and 1003 are no multiples of 4, and the rows' neighbours in the same
    dword of a dimension row keep their codes; 5 rows in place (from 1019: up to the last padding column), then 37 more across the 1024 boundary (n no multiple of 32)"""
    codes = _codes(n0, dim, 4)
    qc = _corpus(S, codes)
    a, b = _codes(5, dim, 5), _codes(37, dim, 6)
    qc.append_codes(a)
    assert qc.memory().corpus_bytes == _store_bytes(n0, dim)
    assert_like_fresh(S, qc, np.vstack([codes, a]), "5 rows in place")
    qc.append_codes(b)
    assert_like_fresh(S, qc, np.vstack([codes, a, b]), "37 rows, reallocating")
    qc.close()


def test_append_in_staging_rounds(S, ctx_option):
    """the host entry point in rounds of 7 rows, in place and reallocating: the column offset of every round"""
    ctx_option("mutate_round", 7)
    codes = _codes(1000, 33, 7)
    qc = _corpus(S, codes)
    a, b = _codes(20, 33, 8), _codes(100, 33, 9)
    qc.append_codes(a)
    qc.append_codes(b)
    assert_like_fresh(S, qc, np.vstack([codes, a, b]), "rounds of 7")
    qc.close()


# =============================================================================== 2. answers as a fresh corpus
def _best_codes(q):
    """the code row with the largest asymmetric score for q (alpha > 0): 255 where q > 0, else 0"""
    return np.where(q > 0, 255, 0).astype(np.uint8)


def _search_everything(S, innr, qc, queries, mask, thr, what):
    """every entry point that takes a code batch, as one dict of arrays (and the engines the stats named)"""
    I8, EXACT, MFMA, AUTO = innr.KNN_MFMA_I8, innr.KNN_EXACT, innr.KNN_MFMA, innr.KNN_AUTO
    out = {"scores": qc.scores(queries[0])}
    for k in (10, 300):  # 300: beyond INNR_MAX_K, the full sort
        for engine in (EXACT, MFMA, I8):
            st = innr.KnnStats()
            out["knn", k, engine] = qc.knn_multi(queries, k, engine=engine, stats=st)
            if k == 10:
                assert st.engine == engine, (what, k, engine, st.engine)  # the int8 engine really ran on this batch
    for engine in (EXACT, AUTO, I8):  # (the int8 engine searches a kept selection: the stale one, were it still there)
        out["filtered", engine] = qc.knn_filtered_multi(queries, 10, mask, engine=engine)
    out["range", EXACT] = qc.range_search(queries, thr, engine=EXACT)
    st = innr.KnnStats()
    out["range", I8] = qc.range_search(queries, thr, engine=I8, stats=st)
    assert st.engine == I8, (what, st.engine)  # (range_u8_i8_min_n = 0: the collect pass on the int8 copy served the call)
    view = qc.prefix(32)
    out["prefix"] = view.knn_multi(queries[:, :32], 10, engine=EXACT)
    view.close()
    return out


def _flatten(v):
    return list(v) if isinstance(v, tuple) else [v]


def test_every_entry_point_answers_as_a_fresh_corpus(S, innr, ctx_option):
    """An append + update + keep sequence with a non-zero index base. The searches also run BEFORE the change, so that the int8 copy
    and a selection of the old codes exist: the changes plant new best documents (the code row with the largest score of a query)
    and remove old ones, so an engine that still read a stale copy or selection would have something wrong to return."""
    ctx_option("range_u8_i8_min_n", 0)
    n, dim, nq = 3000, 64, 12
    p, op = _params(S), oracle.QParams(ALPHA, OFFSET)
    codes = _codes(n, dim, 20)
    queries = _uniform(nq, dim, 21)
    qc = _corpus(S, codes, BASE)
    thr = np.sort(np.stack([_corpus_scores(codes, q, op) for q in queries]), axis=1)[:, -30].astype(np.float32)
    old_mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    before = _search_everything(S, innr, qc, queries, old_mask, thr, "before")
    m = qc.memory()
    assert m.present_mask & innr.COPY_I8_DOT and m.present_mask & innr.COPY_SELECTION
    # update: document u_j becomes the best possible document of query j
    upd = np.array([5, 700, 2999, 1024, 31, 1500])
    planted = np.stack([_best_codes(queries[j]) for j in range(6)])
    qc.update_codes(upd + BASE, planted)
    codes[upd] = planted
    # append: the same for queries 6 .. 9, past the padding (3000 + 200 > 3072)
    more = np.vstack([np.stack([_best_codes(queries[j]) for j in range(6, 10)]), _codes(196, dim, 22)])
    qc.append_codes(more)
    codes = np.vstack([codes, more])
    # keep: the planted documents of queries 0 .. 2 and 6 .. 7 go, and every 7th document
    keep = np.ones(len(codes), np.uint8)
    keep[1::7] = 0
    keep[upd[:3]] = 0
    keep[n:n + 2] = 0
    assert qc.keep(keep) == int(keep.sum())
    codes = codes[keep != 0]
    assert_like_fresh(S, qc, codes, "after the sequence", BASE)
    fresh = _corpus(S, codes, BASE)
    nn = len(codes)
    mask = (np.arange(nn) % 5 != 1).astype(np.uint8)
    thr = np.sort(np.stack([_corpus_scores(codes, q, op) for q in queries]), axis=1)[:, -30].astype(np.float32)
    got = _search_everything(S, innr, qc, queries, mask, thr, "changed")
    want = _search_everything(S, innr, fresh, queries, mask, thr, "fresh")
    assert got.keys() == want.keys()
    for key in want:
        for a, b in zip(_flatten(got[key]), _flatten(want[key])):
            assert bits_equal(np.asarray(a), np.asarray(b)), key
    # the comparison is not vacuous: the answers moved with the codes, and the exact scores are the oracle's
    new_index = np.cumsum(keep) - 1
    top = got["knn", 10, innr.KNN_MFMA_I8][0][:, 0]
    assert top[3:6].tolist() == [BASE + int(new_index[u]) for u in upd[3:]]
    assert top[8:10].tolist() == [BASE + int(new_index[n + 2]), BASE + int(new_index[n + 3])]
    assert not bits_equal(before["knn", 10, innr.KNN_MFMA_I8][0], got["knn", 10, innr.KNN_MFMA_I8][0])
    assert bits_equal(got["scores"], _corpus_scores(codes, queries[0], op))
    fresh.close()
    qc.close()


def _corpus_scores(codes, q, op):
    return np.array([oracle.asymmetric_dot_u8(q, c, op) for c in codes], np.float32)


# =============================================================================== 3. update
def test_update_every_row_in_any_order(S):
    """N = 1000, D = 33: one call names every index in a random order, so the four bytes of every dword of a dimension row are
    written by four different threads of different blocks -- the case a dword read-modify-write loses"""
    n, dim = 1000, 33
    codes = _codes(n, dim, 30)
    qc = _corpus(S, codes, BASE)
    perm = np.random.default_rng(31).permutation(n)
    new = _codes(n, dim, 32)
    qc.update_codes(perm + BASE, new)
    codes[perm] = new
    assert_like_fresh(S, qc, codes, "every row", BASE)
    qc.close()


def test_update_one_byte_of_every_dword(S):
    """only the indices = 1 (mod 4): the three other bytes of every dword belong to documents the call does not name"""
    n, dim = 1000, 33
    codes = _codes(n, dim, 33)
    qc = _corpus(S, codes)
    ids = np.arange(1, n, 4)
    new = _codes(len(ids), dim, 34)
    qc.update_codes(ids, new)
    want = codes.copy()
    want[ids] = new
    others = np.setdiff1d(np.arange(n), ids)
    got = qc.codes()
    assert np.array_equal(got[others], codes[others]) and np.array_equal(got[ids], new)
    assert_like_fresh(S, qc, want, "indices 1 mod 4")
    qc.close()


def test_update_in_staging_rounds(S, ctx_option):
    ctx_option("mutate_round", 7)
    n, dim = 1000, 33
    codes = _codes(n, dim, 35)
    qc = _corpus(S, codes, BASE)
    perm = np.random.default_rng(36).permutation(n)[:500]
    new = _codes(500, dim, 37)
    qc.update_codes(perm + BASE, new)
    codes[perm] = new
    assert_like_fresh(S, qc, codes, "rounds of 7", BASE)
    qc.close()


@pytest.mark.parametrize("entry", ["codes", "rows"])
@pytest.mark.parametrize("case", ["below_base", "beyond_end", "dup_later_round", "dup_adjacent"])
def test_update_refuses_bad_indices_and_writes_nothing(S, innr, ctx_option, case, entry):
    from innr_amd import InnrError
    n, dim = 1000, 33
    qc = _corpus(S, _codes(n, dim, 40), BASE)
    mem = _derive(innr, qc)
    before = qc.codes()
    ids = np.random.default_rng(41).permutation(n)[:200].astype(np.int64) + BASE
    kind, named = "more than once", None
    if case == "below_base":
        ids[150], kind = BASE - 1, "outside"
        named = ids[150]
    elif case == "beyond_end":
        ids[199], kind = BASE + n, "outside"
        named = ids[199]
    elif case == "dup_later_round":
        ctx_option("mutate_round", 64)
        ids[150] = named = ids[3]  # positions in different staging rounds of 64 rows
    else:
        ids[8] = named = ids[7]
    with pytest.raises(InnrError) as e:
        if entry == "codes":
            qc.update_codes(ids, _codes(200, dim, 42))
        else:
            qc.update_rows(ids, _uniform(200, dim, 42))
    assert e.value.status == E_BAD_ARG and kind in str(e.value) and str(int(named)) in str(e.value), str(e.value)
    assert np.array_equal(qc.codes(), before) and qc.memory() == mem  # the store and the derived state as before
    qc.close()


# =============================================================================== 4. keep
def _run_mask(n):
    """runs that straddle boundaries of the gather's 256-document chunks and leave ragged survivor counts in them"""
    m = np.zeros(n, np.uint8)
    for lo, hi in ((250, 263), (509, 770), (1021, 1030), (2815, 2999)):
        m[lo:hi] = 1
    return m


KEEP_MASKS = {
    "half": lambda n: (np.random.default_rng(50).uniform(size=n) < 0.5).astype(np.uint8),
    "one": lambda n: (np.arange(n) == 1777).astype(np.uint8),
    "runs": _run_mask,
}


@pytest.mark.parametrize("name", list(KEEP_MASKS))
def test_keep_compacts_in_index_order(S, innr, lib, name):
    """N = 3000, D = 40: three blocks of 1024 columns, twelve chunks of 256 documents"""
    n, dim = 3000, 40
    codes = _codes(n, dim, 51)
    mask = KEEP_MASKS[name](n)
    if name == "runs":
        counts = np.add.reduceat(mask.astype(np.int64), np.arange(0, n, 256))
        assert (counts % 4 != 0).sum() >= 6, counts  # the gather's ragged dword ends
    qc = _corpus(S, codes, BASE)
    _derive(innr, qc)
    out_n = C.c_size_t(0)
    assert lib.innr_batch_keep_codes(qc._h, _vp(mask), C.byref(out_n)) == OK
    assert out_n.value == int(mask.sum()) == lib.innr_batch_num_vectors(qc._h)
    qc._changed()
    assert_like_fresh(S, qc, codes[mask != 0], name, BASE)
    qc.close()


def test_keep_all_changes_nothing_and_keep_none_leaves_an_empty_corpus(S, innr, lib):
    n, dim = 3000, 40
    codes = _codes(n, dim, 52)
    qc = _corpus(S, codes, BASE)
    mem = _derive(innr, qc)
    assert qc.keep(np.ones(n, np.uint8)) == n  # every row stays: nothing changes, nothing is dropped
    assert qc.memory() == mem and len(qc) == n and np.array_equal(qc.codes(), codes)
    assert qc.keep(np.zeros(n, bool)) == 0
    assert len(qc) == 0 and qc.dimension() == dim
    m = qc.memory()
    assert m.corpus_bytes == 1024 * 64 and m.derived_bytes == 0 and m.present_mask == 0
    idx, sc = qc.knn_multi(_uniform(3, dim, 53), 5)
    assert idx.shape == (3, 0) and sc.shape == (3, 0)  # *out_k == 0
    assert qc.keep(np.zeros(0, np.uint8)) == 0  # N == 0: nothing to do
    back = _codes(5, dim, 54)
    qc.append_codes(back)
    assert_like_fresh(S, qc, back, "append after keep-none", BASE)
    idx, _ = qc.knn_multi(_uniform(3, dim, 53), 5, engine=innr.KNN_EXACT)
    assert idx.min() >= BASE  # the index base is still the corpus'
    qc.close()


def test_keep_out_n_may_be_null_and_remove_takes_global_indices(S, lib):
    n, dim = 3000, 40
    codes = _codes(n, dim, 55)
    qc = _corpus(S, codes, BASE)
    mask = (np.arange(n) % 2).astype(np.uint8)
    assert lib.innr_batch_keep_codes(qc._h, _vp(mask), None) == OK
    assert lib.innr_batch_num_vectors(qc._h) == 1500
    qc._changed()
    kept = codes[1::2]
    assert_like_fresh(S, qc, kept, "keep, out_n null", BASE)
    gone = np.array([0, 5, 5, 1499])
    assert qc.remove(gone + BASE) == 1497  # duplicates allowed
    assert_like_fresh(S, qc, np.delete(kept, [0, 5, 1499], axis=0), "remove", BASE)
    for bad in (BASE - 1, BASE + 1497, 3):
        with pytest.raises(IndexError):
            qc.remove([BASE, bad])
    assert len(qc) == 1497
    qc.close()


# =============================================================================== 5. quantised ingest
def _hard_rows(n, dim, seed, alpha, offset):
    """rows around and beyond the quantisation range, with every value class the rounding treats on its own"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(offset - 0.2 * alpha, offset + 1.2 * alpha, (n, dim)).astype(np.float32)
    flat = rows.reshape(-1)
    step = np.float32(alpha) / np.float32(255.0)
    halves = [np.float32(offset) + (np.float32(k) + np.float32(0.5)) * step for k in (0, 1, 2, 126, 127, 128, 253, 254, 255)]
    special = [np.float32(np.nan), -np.float32(np.nan), np.float32(np.inf), -np.float32(np.inf), np.float32(-0.0), np.float32(0.0),
               np.float32(1e-40), np.float32(-1e-40), np.float32(offset) - np.float32(10.0 * alpha),
               np.float32(offset) + np.float32(11.0 * alpha), np.float32(3.0e38), np.float32(-3.0e38),
               np.float32(offset), np.float32(offset) + np.float32(alpha)] + halves
    pos = rng.permutation(flat.size)[:4 * len(special)]
    for t, where in enumerate(pos):
        flat[where] = special[t % len(special)]
    flat[0], flat[-1] = special[0], halves[0]  # also at the two ends of the flat range
    return rows


@pytest.mark.parametrize("alpha,offset", [(2.0, -1.0), (255.0, 0.0), (255.0, -3.0)])
@pytest.mark.parametrize("round_", [0, 7])
def test_quantised_ingest_stores_the_oracles_codes(S, ctx_option, alpha, offset, round_):
    """(255, 0) and (255, -3): 255 / alpha = 1, so k + 0.5 - offset IS the code boundary and the rounding rule decides. D = 33: the
    flat range of n * D values has an unaligned tail; rounds of 7 rows: the staged path, a round's f32 rows beside their codes"""
    from innr_amd import batch as B
    if round_:
        ctx_option("mutate_round", round_)
    p, op = _params(S, alpha, offset), oracle.QParams(alpha, offset)
    n, dim = 1000, 33
    codes = _codes(n, dim, 60)
    qc = _corpus(S, codes, BASE, p)
    rows = _hard_rows(37, dim, 61, alpha, offset)
    if alpha == 255.0:
        rows[5, :20] = np.arange(20, dtype=np.float32) + np.float32(0.5) + np.float32(offset)  # exactly k + 0.5 in code units
        rows[6, :20] = -(np.arange(20, dtype=np.float32) + np.float32(0.5)) + np.float32(offset)
    want = oracle.quantize_u8(rows, op)
    assert want.min() == 0 and want.max() == 255
    vb = B.VerticalBatch.from_rows(rows)
    by_batch = S.QuantizedCorpus.from_batch(vb, p)
    assert np.array_equal(by_batch.codes(), want)  # the two device quantisers and the oracle agree
    by_batch.close()
    vb.close()
    qc.append(rows)
    assert_like_fresh(S, qc, np.vstack([codes, want]), "append(rows)", BASE, p)
    ids = np.random.default_rng(62).permutation(n + 37)[:29]
    new = _hard_rows(29, dim, 63, alpha, offset)
    qc.update_rows(ids + BASE, new)
    final = np.vstack([codes, want])
    final[ids] = oracle.quantize_u8(new, op)
    assert_like_fresh(S, qc, final, "update_rows(ids, rows)", BASE, p)
    qc.close()


# =============================================================================== 6. device variants
def test_device_variants_give_the_host_path_bytes(S):
    import torch
    n, dim = 1000, 33
    p, op = _params(S), oracle.QParams(ALPHA, OFFSET)
    codes = _codes(n, dim, 70)
    more = _codes(333, dim, 71)
    rows = _hard_rows(41, dim, 72, ALPHA, OFFSET)
    total = n + 333 + 41
    ids = np.random.default_rng(73).permutation(total)[:150].astype(np.int64)
    new = _codes(150, dim, 74)
    ids2 = np.random.default_rng(75).permutation(total)[:29].astype(np.int64)
    new_rows = _hard_rows(29, dim, 76, ALPHA, OFFSET)
    mask = np.random.default_rng(77).uniform(size=total) < 0.6
    host, dev = _corpus(S, codes, BASE), _corpus(S, codes, BASE)
    host.append_codes(more[:10])
    host.append_codes(more[10:])
    dev.append_codes(torch.from_numpy(more[:10]).cuda())   # in place
    dev.append_codes(torch.from_numpy(more[10:]).cuda())   # reallocating
    assert np.array_equal(dev.codes(), host.codes()) and len(dev) == n + 333
    host.append(rows)
    # float32 rows at a device address that is 4 bytes past a 16-byte boundary: the quantiser's scalar head
    big = torch.zeros(41 * dim + 8, dtype=torch.float32, device="cuda")
    big[1:1 + 41 * dim] = torch.from_numpy(rows.reshape(-1)).cuda()
    dev.append(big[1:1 + 41 * dim].reshape(41, dim))
    assert np.array_equal(dev.codes(), host.codes()) and len(dev) == total
    host.update_codes(ids + BASE, new)
    dev.update_codes(torch.from_numpy(ids + BASE).cuda(), torch.from_numpy(new).cuda())
    assert np.array_equal(dev.codes(), host.codes())
    host.update_rows(ids2 + BASE, new_rows)
    dev.update_rows(torch.from_numpy(ids2 + BASE).cuda(), torch.from_numpy(new_rows).cuda())
    assert np.array_equal(dev.codes(), host.codes())
    assert host.keep(mask) == dev.keep(torch.from_numpy(mask).cuda()) == int(mask.sum())  # a bool mask on the device
    assert np.array_equal(dev.codes(), host.codes())
    final = np.vstack([codes, more, oracle.quantize_u8(rows, op)])
    final[ids] = new
    final[ids2] = oracle.quantize_u8(new_rows, op)
    final = final[mask]
    assert_like_fresh(S, dev, final, "device variants", BASE)
    m8 = (np.arange(len(final)) % 3 != 0).astype(np.uint8)
    assert dev.keep(torch.from_numpy(m8).cuda()) == int(m8.sum())  # a uint8 mask on the device
    assert_like_fresh(S, dev, final[m8 != 0], "device keep, uint8 mask", BASE)
    host.close()
    dev.close()


def test_device_update_refuses_bad_indices(S, innr):
    import torch
    from innr_amd import InnrError
    n, dim = 1000, 33
    qc = _corpus(S, _codes(n, dim, 78))
    mem = _derive(innr, qc)
    before = qc.codes()
    new = torch.from_numpy(_codes(100, dim, 79)).cuda()
    for bad, kind in ((n, "outside"), (17, "more than once")):
        ids = np.arange(100, dtype=np.int64) * 3
        ids[40] = bad if kind == "outside" else ids[bad]
        with pytest.raises(InnrError) as e:
            qc.update_codes(torch.from_numpy(ids).cuda(), new)
        assert e.value.status == E_BAD_ARG and kind in str(e.value) and str(int(ids[40])) in str(e.value)
        assert np.array_equal(qc.codes(), before) and qc.memory() == mem
    qc.close()


# =============================================================================== 7. refusals and no-ops
def test_f32_batches_views_wrong_dimensions_and_sizes_are_refused(S, innr, lib, last_error):
    from innr_amd import InnrError, InnrPanic
    from innr_amd import batch as B
    n, dim = 1000, 40
    codes = _codes(n, dim, 80)
    cbuf, fbuf = _codes(2, dim, 81), _uniform(2, dim, 82)
    idx, mask, out_n = np.array([0, 1], np.uint64), np.ones(n, np.uint8), C.c_size_t(7)
    qc = _corpus(S, codes)
    vb = B.VerticalBatch.from_rows(_uniform(n, dim, 83))
    view = qc.prefix(32)

    def all_five(h, D, nrows=2):
        return [lib.innr_batch_append_codes(h, _vp(cbuf), nrows, D), lib.innr_batch_append_quantized(h, _vp(fbuf), nrows, D),
                lib.innr_batch_update_codes(h, _vp(idx), _vp(cbuf), nrows, D),
                lib.innr_batch_update_quantized(h, _vp(idx), _vp(fbuf), nrows, D)]

    for h, word, D in ((vb._h, "f32", dim), (view._h, "view", 32)):
        for fn, args in ((lib.innr_batch_append_codes, (_vp(cbuf), 2, D)), (lib.innr_batch_append_quantized, (_vp(fbuf), 2, D)),
                         (lib.innr_batch_update_codes, (_vp(idx), _vp(cbuf), 2, D)),
                         (lib.innr_batch_update_quantized, (_vp(idx), _vp(fbuf), 2, D)),
                         (lib.innr_batch_keep_codes, (_vp(mask), C.byref(out_n)))):
            assert fn(h, *args) == E_BAD_ARG and word in last_error(), (word, last_error())
    assert out_n.value == 7
    with pytest.raises(InnrError):
        view.append_codes(cbuf[:, :32])
    # the parent of an open view: the Python class raises before the call (the store would move under the view)
    mem = _derive(innr, qc)
    for call in (lambda: qc.append_codes(cbuf), lambda: qc.append(fbuf), lambda: qc.update_codes(idx, cbuf),
                 lambda: qc.update_rows(idx, fbuf), lambda: qc.keep(mask * 0), lambda: qc.remove([3])):
        with pytest.raises(InnrError) as e:
            call()
        assert "open prefix view" in str(e.value)
    assert len(qc) == n and np.array_equal(qc.codes(), codes) and qc.memory() == mem
    view.close()
    # a wrong D, even with n = 0 (before "n == 0: nothing to do")
    assert all_five(qc._h, dim - 1) == [E_DIM_MISMATCH] * 4
    assert all_five(qc._h, dim + 1, 0) == [E_DIM_MISMATCH] * 4
    with pytest.raises(InnrPanic):
        qc.append_codes(_codes(3, dim, 84).reshape(-1)[:-1])
    # n = 0 with the right D: nothing touched, nothing dropped
    assert all_five(qc._h, dim, 0) == [OK] * 4
    assert lib.innr_batch_append_codes(qc._h, None, 0, dim) == OK
    assert qc.memory() == mem and lib.innr_batch_num_vectors(qc._h) == n
    # null pointers with work to do
    assert lib.innr_batch_append_codes(qc._h, None, 2, dim) == E_BAD_ARG
    assert lib.innr_batch_append_quantized(qc._h, None, 2, dim) == E_BAD_ARG
    assert lib.innr_batch_update_codes(qc._h, None, _vp(cbuf), 2, dim) == E_BAD_ARG
    assert lib.innr_batch_update_quantized(qc._h, _vp(idx), None, 2, dim) == E_BAD_ARG
    assert lib.innr_batch_keep_codes(qc._h, None, None) == E_BAD_ARG
    # the size limit comes before every read: n = 2^32 rows "in" a buffer of two
    assert all_five(qc._h, dim, 2 ** 32) == [E_UNSUPPORTED] * 4
    assert len(qc) == n and np.array_equal(qc.codes(), codes) and qc.memory() == mem
    # with the view closed the same calls go through
    qc.append_codes(cbuf)
    qc.update_rows(idx, fbuf)
    assert len(qc) == n + 2
    for b in (vb, qc):
        b.close()
