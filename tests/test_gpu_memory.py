"""GPU tests of the memory entry points (include/innr_hip.h, "device memory"): innr_batch_memory / _copy_bytes report what a
batch derived from its corpus, _release_copies gives it back, _build_copies builds it ahead of the first query, the copy budget
bounds it, and innr_docs_memory / innr_ctx_memory / innr_ctx_trim do the same for a document corpus and the context's workspace.

Bar: every answer equals the INNR_KNN_EXACT engine's answer for the same call, indices and score bits; every byte count is
compared with what the header documents for that allocation (a lower bound, or the exact size where it gives one). No assertion
reads the device's free memory, and none depends on INNR_KNN_AUTO or on the "fits with room to spare" rule: engines are requested
explicitly, and the one copy that rule can add to an explicit call -- the row-major copy of a completion pass -- is switched off
with the context option no_rows_copy wherever a test counts bits (the rows copy and the lo limbs are reached through
innr_batch_build_copies instead).

Shapes: f32 10 000 x 128 uniform rows (40 tiles of 256: several blocks, the last one part full), 16 queries, k = 10; u8 codes
4 000 x 64."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_kernel_variants import logged

N, D, NQ, K = 10_000, 128, 16, 10
NU, DU = 4_000, 64
UNLIMITED = 2 ** 64 - 1


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


def _batch(B, innr, n=N, d=D):
    return B.VerticalBatch.generate(n, d, seed=3, generator=innr.GEN_UNIFORM)


def _codes(S):
    return S.QuantizedCorpus.generate(NU, DU, S.QuantizationParams.from_range(-1.0, 1.0), seed=5)


@pytest.fixture(scope="module")
def queries():
    return oracle.generate_uniform(NQ, D, 99)


@pytest.fixture(scope="module")
def exact(B, innr, queries):
    """metric -> (indices, scores) of the exact engine, computed once; read-only"""
    vb = _batch(B, innr)
    out = {m: B.knn_multi(m, queries, vb, K, engine=innr.KNN_EXACT) for m in METRICS(innr)}
    vb.close()
    for idx, sc in out.values():
        idx.setflags(write=False)
        sc.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def exact_u8(S, innr, queries):
    qc = _codes(S)
    idx, sc = qc.knn_multi(queries[:, :DU], K, engine=innr.KNN_EXACT)
    qc.close()
    return idx, sc


def METRICS(innr):
    return (innr.METRIC_DOT, innr.METRIC_COSINE, innr.METRIC_L2SQ)


def _i8_bit(innr, m):
    return {innr.METRIC_DOT: innr.COPY_I8_DOT, innr.METRIC_COSINE: innr.COPY_I8_COS, innr.METRIC_L2SQ: innr.COPY_I8_L2}[m]


def _bf_bit(innr, m):
    return {innr.METRIC_DOT: innr.COPY_BF16_DOT, innr.METRIC_COSINE: innr.COPY_BF16_COS, innr.METRIC_L2SQ: innr.COPY_BF16_L2}[m]


def _same(got, want) -> bool:
    """indices identical, scores bit-identical"""
    return (np.array_equal(np.asarray(got[0], np.uint64), np.asarray(want[0], np.uint64)) and
            np.array_equal(np.ascontiguousarray(got[1], np.float32).view(np.uint32),
                           np.ascontiguousarray(want[1], np.float32).view(np.uint32)))


def _knn(B, innr, vb, m, q, engine):
    st = innr.KnnStats()
    res = B.knn_multi(m, q, vb, K, engine=engine, stats=st)
    return res, st.engine


def _bits(innr):
    return [innr.COPY_ROWS, innr.COPY_BF16_DOT, innr.COPY_BF16_COS, innr.COPY_BF16_L2, innr.COPY_BF16LO_DOT, innr.COPY_BF16LO_COS,
            innr.COPY_I8_DOT, innr.COPY_I8_COS, innr.COPY_I8_L2, innr.COPY_SELECTION]


def _sum_of_bits(innr, vb) -> int:
    return sum(vb.copy_bytes(b) for b in _bits(innr))


def _builds(vb) -> int:
    from conftest import hooks_lib
    fn = hooks_lib().innrdbg_filter_selection_builds
    fn.restype = C.c_uint32
    fn.argtypes = [C.c_void_p]
    return int(fn(vb._h))


# ------------------------------------------------------------------------------- 1. report: a fresh batch
def test_fresh_batch_has_no_derived_memory(B, S, innr):
    vb, qc = _batch(B, innr), _codes(S)
    for obj, store in ((vb, N * D * 4), (qc, NU * DU)):
        m = obj.memory()
        assert m.derived_bytes == 0 and m.present_mask == 0, m
        assert m.corpus_bytes >= store, m
        assert obj.copy_bytes(innr.COPY_ALL) == m.derived_bytes
        assert obj.copy_budget == UNLIMITED
    vb.close()
    qc.close()


# ------------------------------------------------------------------------------- 2. every explicit engine builds its copy
def test_each_explicit_engine_builds_exactly_its_copy(B, innr, queries, exact, ctx_option):
    ctx_option("no_rows_copy", 1)
    vb = _batch(B, innr)
    present = 0
    for m in METRICS(innr):
        for engine, bit, floor in ((innr.KNN_MFMA_I8, _i8_bit(innr, m), N * D), (innr.KNN_MFMA_BF16, _bf_bit(innr, m), N * D * 2)):
            res, ran = _knn(B, innr, vb, m, queries, engine)
            assert ran == engine, (m, engine, ran)
            assert _same(res, exact[m]), (m, engine)
            present |= bit
            mem = vb.memory()
            assert mem.present_mask == present, (m, engine, bin(mem.present_mask), bin(present))
            assert vb.copy_bytes(bit) >= floor, (m, engine, vb.copy_bytes(bit))
            assert mem.derived_bytes == _sum_of_bits(innr, vb) == vb.copy_bytes(innr.COPY_ALL)
    vb.close()


# ------------------------------------------------------------------------------- 3. prebuild
def test_build_copies_all(B, S, innr):
    vb = _batch(B, innr)
    nine = innr.COPY_ALL & ~innr.COPY_SELECTION
    assert vb.build_copies(innr.COPY_ALL) == nine
    mem = vb.memory()
    assert mem.present_mask == nine
    assert vb.copy_bytes(innr.COPY_ROWS) == N * ((D + 3) // 4 * 4) * 4  # the header's documented size
    for bit in (innr.COPY_BF16_DOT, innr.COPY_BF16_COS, innr.COPY_BF16_L2, innr.COPY_BF16LO_DOT, innr.COPY_BF16LO_COS):
        assert vb.copy_bytes(bit) >= N * D * 2, bit
    assert vb.copy_bytes(innr.COPY_BF16LO_DOT) == vb.copy_bytes(innr.COPY_BF16_DOT)  # same layout, the header says
    for bit in (innr.COPY_I8_DOT, innr.COPY_I8_COS, innr.COPY_I8_L2):
        assert vb.copy_bytes(bit) >= N * D, bit
    assert mem.derived_bytes == _sum_of_bits(innr, vb)
    # DESIGN.md section 3's size column at this shape (ldN = N rounded up to 256)
    ld, up = -(-N // 256) * 256, lambda x, m: -(-x // m) * m
    assert vb.copy_bytes(innr.COPY_BF16_DOT) == vb.copy_bytes(innr.COPY_BF16_COS) == vb.copy_bytes(innr.COPY_BF16LO_COS) == ld * up(D, 64) * 2
    assert vb.copy_bytes(innr.COPY_BF16_L2) == ld * up(D + 6, 64) * 2
    assert vb.copy_bytes(innr.COPY_I8_DOT) == vb.copy_bytes(innr.COPY_I8_COS) == ld * up(D, 128)
    assert ld * up(D + 2, 128) <= vb.copy_bytes(innr.COPY_I8_L2) <= ld * up(D + 121, 128)
    before = [vb.copy_bytes(b) for b in _bits(innr)]
    assert vb.build_copies(innr.COPY_ALL) == nine  # kinds that exist count as present; nothing is built twice
    assert [vb.copy_bytes(b) for b in _bits(innr)] == before and vb.memory() == mem
    assert vb.build_copies(innr.COPY_I8_COS | innr.COPY_SELECTION) == innr.COPY_I8_COS  # only the named kinds are reported
    vb.close()

    qc = _codes(S)
    assert qc.build_copies(innr.COPY_ALL) == innr.COPY_I8_DOT
    assert qc.memory().present_mask == innr.COPY_I8_DOT and qc.copy_bytes(innr.COPY_I8_DOT) >= NU * DU
    qc.close()


def test_prebuilt_copies_serve_the_engines(B, innr, queries, exact):
    """what build_copies built is what the engines use: no byte is added by the calls, the answers are the exact engine's"""
    vb = _batch(B, innr)
    nine = vb.build_copies(innr.COPY_ALL)
    mem = vb.memory()
    for m in METRICS(innr):
        for engine in (innr.KNN_MFMA_I8, innr.KNN_MFMA_BF16, innr.KNN_MFMA):
            res, ran = _knn(B, innr, vb, m, queries, engine)
            assert ran == engine and _same(res, exact[m]), (m, engine, ran)
    after = vb.memory()
    assert after.derived_bytes == mem.derived_bytes and after.present_mask == nine
    vb.close()


# ------------------------------------------------------------------------------- 4. release
def test_release(B, innr, queries, exact, ctx_option):
    ctx_option("no_rows_copy", 1)
    vb = _batch(B, innr)
    nine = vb.build_copies(innr.COPY_ALL)
    s = vb.copy_bytes(innr.COPY_I8_DOT)
    vb.release_copies(innr.COPY_I8_DOT)
    assert vb.memory().present_mask == nine & ~innr.COPY_I8_DOT and vb.copy_bytes(innr.COPY_I8_DOT) == 0
    res, ran = _knn(B, innr, vb, innr.METRIC_DOT, queries, innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA_I8 and _same(res, exact[innr.METRIC_DOT])
    assert vb.memory().present_mask == nine and vb.copy_bytes(innr.COPY_I8_DOT) == s  # back, same size
    vb.release_copies(innr.COPY_BF16_DOT)  # the lo limbs are of no use without their partner
    assert vb.memory().present_mask == nine & ~(innr.COPY_BF16_DOT | innr.COPY_BF16LO_DOT)
    vb.release_copies(innr.COPY_BF16LO_COS)  # ... but the hi limbs are: the bf16 filter's copy stays
    assert vb.memory().present_mask == nine & ~(innr.COPY_BF16_DOT | innr.COPY_BF16LO_DOT | innr.COPY_BF16LO_COS)
    vb.release_copies()
    mem = vb.memory()
    assert mem.derived_bytes == 0 and mem.present_mask == 0 and mem.corpus_bytes >= N * D * 4
    vb.release_copies()  # nothing left: a no-op
    res, ran = _knn(B, innr, vb, innr.METRIC_COSINE, queries, innr.KNN_MFMA_BF16)  # rebuilt on demand
    assert ran == innr.KNN_MFMA_BF16 and _same(res, exact[innr.METRIC_COSINE])
    vb.release_copies()
    vb.close()  # innr_batch_free after a release: every pointer freed once


# ------------------------------------------------------------------------------- 5. budget 0
def test_budget_zero(B, S, innr, queries, exact, exact_u8, ctx_option):
    ctx_option("split_min_q", 1)  # the split-bf16 filter would take these 16 queries: the budget must refuse its limbs
    vb = _batch(B, innr)
    vb.copy_budget = 0
    assert vb.copy_budget == 0
    for m in METRICS(innr):
        for engine in (innr.KNN_MFMA_I8, innr.KNN_MFMA_BF16, innr.KNN_MFMA):
            (res, ran), log = logged(lambda: _knn(B, innr, vb, m, queries, engine))
            assert ran == innr.KNN_MFMA, (m, engine, ran)
            assert _same(res, exact[m]), (m, engine)
            fams = {e.family for e in log}
            assert "gemm_f32" in fams and not fams & {"gemm_split", "gemm_bf16", "i8_one", "i8_two", "i8_small"}, (m, engine, log)
    assert vb.build_copies(innr.COPY_ALL) == 0
    mem = vb.memory()
    assert mem.derived_bytes == 0 and mem.present_mask == 0
    vb.close()

    qc = _codes(S)
    qc.copy_budget = 0
    st = innr.KnnStats()
    res = qc.knn_multi(queries[:, :DU], K, engine=innr.KNN_MFMA_I8, stats=st)
    assert st.engine == innr.KNN_MFMA and _same(res, exact_u8)
    assert qc.build_copies(innr.COPY_ALL) == 0 and qc.memory().derived_bytes == 0
    qc.copy_budget = None  # unlimited again: the same request now runs on the integer pipe
    res = qc.knn_multi(queries[:, :DU], K, engine=innr.KNN_MFMA_I8, stats=st)
    assert st.engine == innr.KNN_MFMA_I8 and _same(res, exact_u8) and qc.memory().present_mask == innr.COPY_I8_DOT
    qc.close()


# ------------------------------------------------------------------------------- 6. a budget of one copy; refusals are not remembered
def test_budget_of_one_copy_is_not_sticky(B, innr, queries, exact):
    dot = innr.METRIC_DOT
    probe = _batch(B, innr)
    assert probe.build_copies(innr.COPY_I8_DOT) == innr.COPY_I8_DOT
    s = probe.copy_bytes(innr.COPY_I8_DOT)
    probe.close()
    vb = _batch(B, innr)
    vb.copy_budget = s
    res, ran = _knn(B, innr, vb, dot, queries, innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA_I8 and _same(res, exact[dot])
    assert vb.memory().derived_bytes == s
    res, ran = _knn(B, innr, vb, dot, queries, innr.KNN_MFMA_BF16)
    assert ran == innr.KNN_MFMA and _same(res, exact[dot])
    assert vb.memory().derived_bytes <= s and vb.memory().present_mask == innr.COPY_I8_DOT
    assert vb.build_copies(innr.COPY_ALL) == innr.COPY_I8_DOT and vb.memory().derived_bytes <= s
    vb.copy_budget = None
    res, ran = _knn(B, innr, vb, dot, queries, innr.KNN_MFMA_BF16)
    assert ran == innr.KNN_MFMA_BF16 and _same(res, exact[dot])
    assert vb.memory().present_mask & innr.COPY_BF16_DOT
    vb.close()


# ------------------------------------------------------------------------------- 7. lowering the budget frees nothing
def test_lowering_the_budget_frees_nothing(B, innr, queries, exact, ctx_option):
    ctx_option("no_rows_copy", 1)
    dot = innr.METRIC_DOT
    vb = _batch(B, innr)
    assert vb.build_copies(innr.COPY_I8_DOT | innr.COPY_BF16_DOT | innr.COPY_BF16LO_DOT) == \
        innr.COPY_I8_DOT | innr.COPY_BF16_DOT | innr.COPY_BF16LO_DOT
    mem = vb.memory()
    vb.copy_budget = 0
    assert vb.memory() == mem
    for engine in (innr.KNN_MFMA_I8, innr.KNN_MFMA_BF16):  # the copies that exist keep being used
        res, ran = _knn(B, innr, vb, dot, queries, engine)
        assert ran == engine and _same(res, exact[dot]), engine
    res, ran = _knn(B, innr, vb, innr.METRIC_COSINE, queries, innr.KNN_MFMA_I8)  # ... and no new one appears
    assert ran == innr.KNN_MFMA and _same(res, exact[innr.METRIC_COSINE])
    after = vb.memory()  # (the cosine call cached 1/norm: aux_bytes may grow, it is not a copy)
    assert (after.derived_bytes, after.present_mask, after.corpus_bytes) == (mem.derived_bytes, mem.present_mask, mem.corpus_bytes)
    vb.close()


# ------------------------------------------------------------------------------- 8. the context option
def test_context_option_sets_the_budget_of_new_batches(B, S, innr, ctx_option):
    from innr_amd import _lib
    assert _lib.default_context().get_option("copy_budget_mib") == -1
    old = _batch(B, innr, 512, 32)
    ctx_option("copy_budget_mib", 0)
    new, view, codes = _batch(B, innr, 512, 32), old.prefix(16), S.QuantizedCorpus.generate(512, 32, S.QuantizationParams(2.0, -1.0))
    assert new.copy_budget == 0 and view.copy_budget == 0 and codes.copy_budget == 0
    assert old.copy_budget == UNLIMITED
    ctx_option("copy_budget_mib", 3)
    three = _batch(B, innr, 512, 32)
    assert three.copy_budget == 3 << 20 and new.copy_budget == 0
    for o in (view, old, new, codes, three):
        o.close()


# ------------------------------------------------------------------------------- 9. the kept selection
def test_selection_is_reported_released_and_budgeted(B, innr, queries, exact):
    dot = innr.METRIC_DOT
    mask = (np.arange(N) % 2 == 0).astype(np.uint8)
    npass = int(mask.sum())
    vb = _batch(B, innr)

    def call(engine):
        st = innr.KnnStats()
        return B.batch_knn_filtered_multi(queries, vb, K, mask, metric=dot, engine=engine, stats=st), st.engine

    want, ran = call(innr.KNN_EXACT)
    assert ran == innr.KNN_EXACT and vb.memory().derived_bytes == 0 and _builds(vb) == 0
    res, ran = call(innr.KNN_MFMA)
    assert ran == innr.KNN_MFMA and _same(res, want)
    mem = vb.memory()
    assert mem.present_mask == innr.COPY_SELECTION and _builds(vb) == 1
    assert vb.copy_bytes(innr.COPY_SELECTION) >= npass * D * 4 + N + 4 * npass  # store, mask, map (the header's sizes)
    assert mem.derived_bytes == vb.copy_bytes(innr.COPY_SELECTION)
    vb.release_copies(innr.COPY_SELECTION)
    assert vb.memory().derived_bytes == 0 and vb.memory().present_mask == 0
    res, ran = call(innr.KNN_MFMA)
    assert ran == innr.KNN_MFMA and _same(res, want) and _builds(vb) == 2
    # the selection's own copies are the parent's to account for and to bound
    sel = vb.copy_bytes(innr.COPY_SELECTION)
    vb.copy_budget = sel  # room for the selection that exists, none for a filter copy on it
    res, ran = call(innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA and _same(res, want) and vb.copy_bytes(innr.COPY_SELECTION) == sel and _builds(vb) == 2
    vb.copy_budget = None
    res, ran = call(innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA_I8 and _same(res, want) and _builds(vb) == 2
    assert vb.copy_bytes(innr.COPY_SELECTION) >= sel + npass * D and vb.memory().present_mask == innr.COPY_SELECTION
    # budget 0: no room for a selection, the masked exact scan serves the call
    vb.release_copies(innr.COPY_SELECTION)
    vb.copy_budget = 0
    res, ran = call(innr.KNN_MFMA)
    assert ran == innr.KNN_EXACT and _same(res, want) and _builds(vb) == 2
    assert vb.memory().derived_bytes == 0
    vb.close()


# ------------------------------------------------------------------------------- 10. a prefix view owns its copies, not the store
def test_prefix_view(B, innr, queries):
    dot = innr.METRIC_DOT
    vb = _batch(B, innr)
    assert vb.build_copies(innr.COPY_I8_DOT) == innr.COPY_I8_DOT
    parent = vb.memory()
    view = vb.prefix(64)
    assert view.memory().corpus_bytes == 0 and view.memory().derived_bytes == 0
    q = np.ascontiguousarray(queries[:, :64])
    want, _ = _knn(B, innr, view, dot, q, innr.KNN_EXACT)
    res, ran = _knn(B, innr, view, dot, q, innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA_I8 and _same(res, want)
    assert view.memory().present_mask & innr.COPY_I8_DOT and view.copy_bytes(innr.COPY_I8_DOT) >= N * 64
    assert vb.memory().derived_bytes == parent.derived_bytes and vb.memory().present_mask == parent.present_mask
    assert vb.memory().corpus_bytes == parent.corpus_bytes
    vb.release_copies()
    assert vb.memory().derived_bytes == 0
    assert view.memory().present_mask & innr.COPY_I8_DOT and view.copy_bytes(innr.COPY_I8_DOT) >= N * 64
    res, ran = _knn(B, innr, view, dot, q, innr.KNN_MFMA_I8)
    assert ran == innr.KNN_MFMA_I8 and _same(res, want)
    # a view whose length has no matrix-pipe engine gets the rows copy and nothing else
    odd = vb.prefix(50)
    assert odd.build_copies(innr.COPY_ALL) == innr.COPY_ROWS and odd.copy_bytes(innr.COPY_ROWS) == N * 52 * 4
    odd.close()
    view.close()
    vb.close()


# ------------------------------------------------------------------------------- 11. the context's workspace
STATE_BYTES = 4096  # the flag block innr_ctx_create sets up: the one buffer innr_ctx_trim keeps


def test_context_workspace_trim(B, innr, queries):
    from innr_amd import _lib
    ctx = _lib.default_context()
    vb = _batch(B, innr)
    thr = np.full(NQ, 70.0, np.float32)  # (squared distances of these rows centre on 2 D / 3 = 85, sigma 9: a few per cent pass)

    def both():
        knn = B.knn_multi(innr.METRIC_DOT, queries, vb, K, engine=innr.KNN_MFMA)
        rng = B.batch_range_search(queries, vb, thr, metric=innr.METRIC_L2SQ, engine=innr.KNN_EXACT)
        return knn, rng

    knn0, (off0, idx0, sc0) = both()
    assert off0[-1] > 0  # the threshold keeps something: the range search has answers to compare
    assert ctx.memory() > STATE_BYTES
    ctx.trim()
    assert ctx.memory() <= STATE_BYTES
    ctx.trim()  # nothing left to free
    knn1, (off1, idx1, sc1) = both()
    assert _same(knn1, knn0) and np.array_equal(off1, off0) and _same((idx1, sc1), (idx0, sc0))
    assert ctx.memory() > STATE_BYTES
    vb.close()


# ------------------------------------------------------------------------------- 12. document corpora
def test_document_corpus_memory(innr):
    from innr_amd import maxsim as M
    # 300 documents of up to 24 tokens x 48 dimensions: the MFMA engine, which builds the token norms, needs more than 16 tokens
    # per document (innr_maxsim_topk), so the 300 x 16 x 48 floor below is met by the smallest corpus of that kind that has one
    docs, T, dim = 300, 24, 48
    rng = np.random.default_rng(11)
    tok = rng.uniform(-1.0, 1.0, (docs, T, dim)).astype(np.float32)
    doc_len = rng.integers(1, T + 1, docs).astype(np.uint32)
    dc = M.DocumentCorpus.from_tokens(tok, doc_len)
    mem = dc.memory()
    assert mem.corpus_bytes == docs * T * dim * 4 + docs * 4 and mem.derived_bytes == 0
    q = rng.uniform(-1.0, 1.0, (8, dim)).astype(np.float32)
    want = dc.topk(q, 5, engine=innr.KNN_EXACT)
    assert dc.memory().derived_bytes == 0
    got = dc.topk(q, 5, engine=innr.KNN_MFMA)
    assert [int(i) for i in got[0]] == [int(i) for i in want[0]]
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32))
    mem = dc.memory()
    assert mem.derived_bytes >= docs * T * 4 >= 300 * 16 * 4 and mem.corpus_bytes == docs * T * dim * 4 + docs * 4 >= 300 * 16 * 48 * 4
    dc.close()
