"""GPU tests of the kernel INSTANTIATIONS behind the f32 / bf16 / split-bf16 GEMM filters, the int8 filter and the maxsim entry
points: one case per instantiation a public call (or, for the dense-score dump mode, a hook of the test-hooks library) can reach.
Every case (1) compares the call's answer with the CPU oracle bit for bit and (2) asserts, through the context's
launch record (api_internal.h: innr_ctx::launch_log, written at every templated dispatch, read by the hook innrdbg_launch_log of the
test-hooks library), that the instantiation it is named after really served the call -- a dispatch that silently declines (an
unseeded corpus, a K-step count without an instantiation, ...) fails the case instead of passing on another kernel's answer.

The table (GEMM_F32, GEMM_BF16, GEMM_SPLIT, I8_SMALL, I8_TILES, MS_SCAN, MS_TILE, MS_GENERIC, MS_RERANK) names every instantiation of
those families; the last test of the file checks that nothing outside it was launched by any case here, so a new instantiation
cannot appear without a row. The range scan is recorded as well (and decoded) but has no table."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import _corpus, _queries, bits_equal, same_knn
from test_gpu_maxsim import _oracle_scores, _tokens
from test_gpu_mfma import _dense_scores
from test_gpu_split_filter import _split_scores
from test_gpu_maxsim_rerank import PairOracle, _check as _check_rerank, _rank


def _codes(n, dim, seed, alpha=2.0, offset=-1.0):
    """uniform rows quantised to u8 codes, (n, dim)  (test_gpu_u8.py imports this module: no import from there)"""
    return oracle.quantize_u8(oracle.generate_uniform(n, dim, seed), oracle.QParams(alpha, offset))


def _oracle_knn_u8(q, codes, alpha, offset, k):
    return oracle.batch_knn_u8(q, codes, oracle.QParams(alpha, offset), k)


# ------------------------------------------------------------------------------- the launch record
FAMILIES = {1: "gemm_f32", 2: "gemm_bf16", 3: "gemm_split", 4: "i8_one", 5: "i8_two", 6: "i8_small", 7: "ms_scan", 8: "ms_tile",
            9: "ms_generic", 10: "ms_rerank", 11: "range_scan"}  # api_internal.h LaunchFamily
_REC = np.dtype({"names": ["family", "lockstep", "arg", "groups"], "formats": ["u1", "u1", ("<i2", (4,)), "<u4"],
                 "offsets": [0, 1, 2, 12], "itemsize": 16})  # api_internal.h LaunchRec (the C layout: groups aligned to 4 bytes)
LOG_CAP = 64  # api_internal.h kLaunchLogCap


class Launch(NamedTuple):
    family: str     # FAMILIES
    args: tuple     # the template arguments in the order api_internal.h's LaunchFamily comments give, without trailing unused ones
    groups: int     # query groups of the launch (maxsim: queries per corpus pass)
    lockstep: bool  # gemm_i8s_filter_kernel: the soft-lockstep buffer was passed

    @property
    def inst(self):
        return (self.family,) + self.args


_NARGS = {"gemm_f32": 4, "gemm_bf16": 3, "gemm_split": 3, "i8_one": 2, "i8_two": 2, "i8_small": 3, "ms_scan": 3, "ms_tile": 3,
          "ms_generic": 1, "ms_rerank": 3, "range_scan": 3}


def _hook():
    from conftest import hooks_lib
    L = hooks_lib()
    L.innrdbg_launch_log.restype = C.c_size_t
    L.innrdbg_launch_log.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.innrdbg_launch_log_reset.restype = None
    L.innrdbg_launch_log_reset.argtypes = [C.c_void_p]
    return L


def launch_log():
    """the default context's launches since the last reset, oldest first"""
    from innr_amd import _lib
    buf = np.zeros(LOG_CAP, _REC)
    total = C.c_uint64(0)
    n = _hook().innrdbg_launch_log(_lib.default_context().handle, buf.ctypes.data, LOG_CAP, C.byref(total))
    assert total.value == n, f"{total.value} launches since the reset: more than the record's {LOG_CAP} entries"
    out = []
    for r in buf[:n]:
        fam = FAMILIES[int(r["family"])]
        out.append(Launch(fam, tuple(int(x) for x in r["arg"][:_NARGS[fam]]), int(r["groups"]), bool(r["lockstep"])))
    return out


def logged(call):
    """reset the launch record, run `call`, return (its result, the launches it made)"""
    from innr_amd import _lib
    _hook().innrdbg_launch_log_reset(_lib.default_context().handle)
    res = call()
    return res, launch_log()


# ------------------------------------------------------------------------------- the table
DOT, COS, U8, L2 = 0, 1, 2, 3  # kernels_gemm.h kGemmDot / kGemmCos / kGemmU8 / kGemmL2
RR_OF_K = {10: 6, 40: 8, 100: 12, 200: 20}  # lists of pick_kp(k, 16) = 32 / 64 / 128 / 256 candidates: capacity 64 RR
GEMM_F32 = [("gemm_f32", kind, rr, 0, wv) for kind in (DOT, COS, L2) for rr in (6, 8, 12, 20) for wv in (1, 2, 4, 8)] + \
           [("gemm_f32", U8, rr, 0, wv) for rr in (6, 8, 12, 20) for wv in (4, 8)] + \
           [("gemm_f32", kind, 6, 2, 4) for kind in (DOT, COS, L2)] + [("gemm_f32", DOT, 6, 2, 8)] + \
           [("gemm_f32", kind, 6, 1, 4) for kind in (DOT, COS)]                                # gemm_filter_kernel<KIND, RR, MODE, WV>
GEMM_BF16 = [("gemm_bf16", rr, 0, 1) for rr in (12, 20)]                                     # gemm_bf16_filter_kernel<RR, 0, 1>
GEMM_SPLIT = [("gemm_split", rr, 0, 3) for rr in (6, 8, 12, 20)] + [("gemm_split", 6, 1, 3)]  # gemm_bf16_filter_kernel<RR, MODE, 3>
I8_SMALL = [("i8_small", nk, ct, mode) for mode in (0, 2) for nk, ct in
            [(nk, 2) for nk in range(2, 17, 2)] + [(nk, 4) for nk in range(8, 17, 2)]]          # gemm_i8s_filter_kernel<12, NK, CT, MODE>
I8_TILES = [("i8_one", rr, 0) for rr in (6, 8, 12)] + [("i8_one", 6, 2)] + \
           [("i8_two", rr, 0) for rr in (6, 8, 12, 20)]                                       # gemm_i8h_ / gemm_i8_filter_kernel<RR, MODE>
MS_SCAN = [("ms_scan", c, nq, m) for c in (0, 1) for nq in (8, 16, 32) for m in (0, 1)]       # maxsim_scan_kernel<COS, NQ, MULTI>
MS_TILE = [("ms_tile", c, nb, nq) for c in (0, 1) for nb in (1, 2, 3, 4) for nq in (1, 2, 4)]  # maxsim_mfma_tile_kernel<COS, NB, NQ>
MS_GENERIC = [("ms_generic", c) for c in (0, 1)]                                              # maxsim_mfma_kernel<COS>
MS_RERANK = [("ms_rerank", c, nq, m) for c in (0, 1) for nq in (8, 16, 32) for m in (0, 1)]   # maxsim_rerank_kernel<COS, NQ, MULTI>
TABLE = set(GEMM_F32 + GEMM_BF16 + GEMM_SPLIT + I8_SMALL + I8_TILES + MS_SCAN + MS_TILE + MS_GENERIC + MS_RERANK)
TABLE_FAMILIES = {t[0] for t in TABLE}
_SEEN: set = set()      # every instantiation a case of this file launched
_ASSERTED: set = set()  # ... and the ones a case asserted by name


def _run(call):
    res, log = logged(call)
    _SEEN.update(e.inst for e in log)
    return res, log


def _expect(log, inst, groups=None, lockstep=None):
    """the named instantiation is in the record (with this group count / lockstep flag, when given)"""
    assert inst in TABLE, inst
    hits = [e for e in log if e.inst == inst and (groups is None or e.groups == groups) and (lockstep is None or e.lockstep == lockstep)]
    assert hits, f"{inst} (groups {groups}, lockstep {lockstep}) not launched; the call launched {log}"
    _ASSERTED.add(inst)
    return hits[0]


@pytest.fixture(scope="module")
def B():
    from innr_amd import batch
    return batch


@pytest.fixture(scope="module")
def S():
    from innr_amd import scalar
    return scalar


@pytest.fixture(scope="module")
def M():
    from innr_amd import maxsim
    return maxsim


@pytest.fixture(scope="module")
def innr():
    import innr_amd
    return innr_amd


# ------------------------------------------------------------------------------- int8 family
N_I8 = 8300          # the last 128-row tile partly full; >= 32 x 256 rows: seeded once gemm_seed_n = 256
SMALL_SHAPES = [(nk, 2) for nk in range(2, 17, 2)] + [(nk, 4) for nk in range(8, 17, 2)]  # the 13 (NK, CT) pairs
Q_OF_CT = {2: 3, 4: 65}


def _dim(nk):
    return 64 * nk - 5  # a ragged last K-step pair; round_up(D, 128) / 64 == nk for every even nk


@functools.lru_cache(maxsize=2)
def _i8_rows(dim, kind):
    """uniform: 8300 uniform rows with unequal norms. dup: 52 such rows, each ~160 times (interleaved; every 7th copy a few ulps
    longer): more exact (near-)ties at the top than the lists of 128 hold, so NO query's answer can be proven by the first pass
    and every one of them goes through the completion pass (collect mode), whatever the data."""
    if kind == "uniform":
        rows, _ = _corpus(N_I8, dim, 5, uniform=True)
        rows = (rows * (1.0 + 0.5 * np.sin(np.arange(N_I8, dtype=np.float32)))[:, None]).astype(np.float32)
    else:
        base, _ = _corpus(52, dim, 6, uniform=True)
        base = (base * (1.0 + 0.5 * np.sin(np.arange(52, dtype=np.float32)))[:, None]).astype(np.float32)
        rows = np.tile(base, (160, 1))[:N_I8].copy()
        rows[::7] *= np.float32(1.0 + 2.0 ** -20)
    rows.setflags(write=False)
    data = oracle.from_rows(rows)
    data.setflags(write=False)
    return rows, data


@functools.lru_cache(maxsize=None)
def _i8_oracle(dim, kind, metric, nq, k):
    """the oracle's answer, computed once per (corpus, metric, batch, k) and shared by the cases that need it"""
    _, data = _i8_rows(dim, kind)
    ofn = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}[metric]
    return [ofn(q, data, k) for q in _i8_queries(dim, nq)]


def _i8_queries(dim, nq):
    return _queries(nq, dim, 99, uniform=True)


_VB: dict = {}


def _i8_batch(B, dim, kind):
    if (dim, kind) not in _VB:
        _VB.clear()  # one resident corpus at a time
        _VB[(dim, kind)] = B.VerticalBatch.from_rows(_i8_rows(dim, kind)[0])
    return _VB[(dim, kind)]


def _knn_vs_oracle(B, innr, metric, dim, kind, nq, k, stats=None, engine=None):
    """one call of `engine` (INNR_KNN_MFMA_I8 unless given) on the f32 corpus, compared with the oracle exactly; returns
    (idx, scores), launches"""
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi, "l2": B.batch_knn_multi}[metric]
    engine = innr.KNN_MFMA_I8 if engine is None else engine
    vb, qs = _i8_batch(B, dim, kind), _i8_queries(dim, nq)
    st = stats if stats is not None else innr.KnnStats()
    (idx, sc), log = _run(lambda: fn(qs, vb, k, engine=engine, stats=st))
    assert st.engine == engine
    for j, (oi, os_) in enumerate(_i8_oracle(dim, kind, metric, nq, k)):
        assert same_knn(metric, idx[j], sc[j], oi, os_), (metric, j, idx[j], oi, sc[j], os_)
    return (idx, sc), log


@pytest.mark.parametrize("nk,ct", SMALL_SHAPES)
def test_i8_small_filter_dot(B, innr, ctx_option, nk, ct):
    """gemm_i8s_filter_kernel<12, NK, CT, 0>: dot on an f32 corpus, k = 10 (lists of 128, every answer proven by the first pass)"""
    ctx_option("gemm_seed_n", 256)
    _, log = _knn_vs_oracle(B, innr, "dot", _dim(nk), "uniform", Q_OF_CT[ct], 10)
    _expect(log, ("i8_small", nk, ct, 0), groups=1, lockstep=False)
    assert not any(e.family in ("i8_one", "i8_two") for e in log), log


@pytest.mark.parametrize("nk,ct", SMALL_SHAPES)
def test_i8_small_collect_dot(B, innr, ctx_option, nk, ct):
    """the collect twin <12, NK, CT, 2>: k = 100, lists of k + 16 rounded to 128 on a corpus with more near-ties at the top than
    a list holds: no first-pass proof can hold, every query goes through the completion pass (the same batch size, so the
    same CT) in collect mode"""
    ctx_option("gemm_seed_n", 256)
    st = innr.KnnStats()
    _, log = _knn_vs_oracle(B, innr, "dot", _dim(nk), "dup", Q_OF_CT[ct], 100, stats=st)
    print(f"NK {nk} CT {ct}: {st.queries_fallback} of {Q_OF_CT[ct]} queries unproven after the first pass; launches {log}")
    _expect(log, ("i8_small", nk, ct, 0), groups=1, lockstep=False)
    _expect(log, ("i8_small", nk, ct, 2), groups=1, lockstep=False)


@pytest.mark.parametrize("metric", ["cos", "l2"])
def test_i8_small_cosine_and_squared_l2(B, innr, ctx_option, metric):
    ctx_option("gemm_seed_n", 256)
    nk = 6
    _, log = _knn_vs_oracle(B, innr, metric, _dim(nk), "uniform", 3, 10)
    small = [e for e in log if e.family == "i8_small"]
    assert len(small) == 1 and small[0].inst in TABLE, log
    got_nk, got_ct, got_mode = small[0].args
    # squared L2 filters on a copy of D + R + 1 dimensions (R from the corpus' norms): the record says which K-step count that made
    assert (got_ct, got_mode) == (2, 0) and (got_nk == nk if metric == "cos" else nk <= got_nk <= nk + 2), log
    _expect(log, small[0].inst, groups=1, lockstep=False)


@pytest.mark.parametrize("nk,ct", [(2, 2), (8, 2), (16, 2), (8, 4), (16, 4)])
def test_i8_small_code_corpus(S, innr, ctx_option, nk, ct):
    """the same kernel under a u8 code corpus (innr_batch_knn_u8): k = 10 takes lists of 128 for its sake"""
    ctx_option("gemm_seed_n", 256)
    dim, nq = _dim(nk), Q_OF_CT[ct]
    codes = _codes(N_I8, dim, 11)
    qc = S.QuantizedCorpus.from_codes(codes, N_I8, dim, S.QuantizationParams(2.0, -1.0))
    qs = oracle.generate_uniform(nq, dim, 321)
    st = innr.KnnStats()
    (idx, sc), log = _run(lambda: qc.knn_multi(qs, 10, engine=innr.KNN_MFMA_I8, stats=st))
    assert st.engine == innr.KNN_MFMA_I8
    for j in range(nq):
        oi, os_ = _oracle_knn_u8(qs[j], codes, 2.0, -1.0, 10)
        assert same_knn("dot", idx[j], sc[j], oi, os_), (j, idx[j], oi)
    _expect(log, ("i8_small", nk, ct, 0), groups=1, lockstep=False)
    qc.close()


def test_i8_small_two_groups_lockstep(B, innr, ctx_option):
    """130 queries: two groups of 128 side by side, kept together by the soft-lockstep buffer -- or not (i8_small_free): same bits"""
    ctx_option("gemm_seed_n", 256)
    nk = 8
    (i1, s1), log = _knn_vs_oracle(B, innr, "dot", _dim(nk), "uniform", 130, 10)
    _expect(log, ("i8_small", nk, 4, 0), groups=2, lockstep=True)
    ctx_option("i8_small_free", 1)
    (i2, s2), log = _knn_vs_oracle(B, innr, "dot", _dim(nk), "uniform", 130, 10)
    _expect(log, ("i8_small", nk, 4, 0), groups=2, lockstep=False)
    assert not any(e.lockstep for e in log), log
    assert np.array_equal(i1, i2) and bits_equal(s1, s2)


@pytest.mark.parametrize("family,option", [("i8_one", "i8_no_small"), ("i8_two", "i8_two_limb")])
@pytest.mark.parametrize("k,rr", [(10, 6), (40, 8), (100, 12), (200, 20)])
def test_i8_tiles_code_corpus(S, innr, ctx_option, family, option, k, rr):
    """the 512-query tile gemm_i8h_filter_kernel<RR, 0> (one limb) and the 256-query tile gemm_i8_filter_kernel<RR, 0> (two limbs):
    lists of 32 / 64 / 128 are RR 6 / 8 / 12; lists of 256 exist on the two-limb kernel only, whatever the option"""
    ctx_option("gemm_seed_n", 256)
    ctx_option(option, 1)
    if rr == 20:
        family = "i8_two"
    dim, nq = 123, 9
    codes = _codes(N_I8, dim, 12)
    qc = S.QuantizedCorpus.from_codes(codes, N_I8, dim, S.QuantizationParams(2.0, -1.0))
    qs = oracle.generate_uniform(nq, dim, 322)
    (idx, sc), log = _run(lambda: qc.knn_multi(qs, k, engine=innr.KNN_MFMA_I8))
    for j in range(nq):
        oi, os_ = _oracle_knn_u8(qs[j], codes, 2.0, -1.0, k)
        assert same_knn("dot", idx[j], sc[j], oi, os_), (j, idx[j], oi)
    _expect(log, (family, rr, 0), groups=1)
    assert not any(e.family == "i8_small" for e in log), log
    qc.close()


def test_i8_one_limb_tile_f32_corpus_and_its_collect_pass(B, innr, ctx_option):
    """the f32 corpus on the 512-query tile (i8_no_small): <12, 0> with lists of 128, and the completion pass on <6, 2>"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("i8_no_small", 1)
    _, log = _knn_vs_oracle(B, innr, "dot", _dim(2), "uniform", 3, 10)
    _expect(log, ("i8_one", 12, 0), groups=1)
    _, log = _knn_vs_oracle(B, innr, "dot", _dim(2), "dup", 3, 100)
    _expect(log, ("i8_one", 12, 0), groups=1)
    _expect(log, ("i8_one", 6, 2), groups=1)
    assert not any(e.family == "i8_small" for e in log), log


# ------------------------------------------------------------------------------- f32 / bf16 / split-bf16 GEMM families
D_GEMM = 123  # ragged: no multiple of the kernels' K-steps; with N_I8 rows the last 128-row corpus tile is partly full
KIND_OF = {"dot": DOT, "cos": COS, "l2": L2}


@pytest.mark.parametrize("wv", [1, 2, 4, 8])
@pytest.mark.parametrize("k", sorted(RR_OF_K))
@pytest.mark.parametrize("metric", ["dot", "cos", "l2"])
def test_gemm_f32_filter(B, innr, ctx_option, metric, k, wv):
    """gemm_filter_kernel<KIND, RR, 0, WV>: 3 queries on a tile of 64 WV (gemm_waves; the rest of the tile is padding), lists of
    32 / 64 / 128 / 256 candidates; no_split_filter keeps dot and cosine on this kernel"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("no_split_filter", 1)
    ctx_option("gemm_waves", wv)
    _, log = _knn_vs_oracle(B, innr, metric, D_GEMM, "uniform", 3, k, engine=innr.KNN_MFMA)
    _expect(log, ("gemm_f32", KIND_OF[metric], RR_OF_K[k], 0, wv), groups=1)
    assert not any(e.family in ("gemm_bf16", "gemm_split") for e in log), log


def test_gemm_f32_three_query_tiles(B, innr, ctx_option):
    """130 queries on one-wave tiles of 64: three query tiles, the last one mostly padding"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("no_split_filter", 1)
    ctx_option("gemm_waves", 1)
    _, log = _knn_vs_oracle(B, innr, "dot", D_GEMM, "uniform", 130, 10, engine=innr.KNN_MFMA)
    _expect(log, ("gemm_f32", DOT, 6, 0, 1), groups=3)


@pytest.mark.parametrize("metric,nq,wv", [("dot", 9, 4), ("cos", 9, 4), ("l2", 9, 4), ("dot", 260, 8)])
def test_gemm_f32_collect(B, innr, ctx_option, metric, nq, wv):
    """the collect twin <KIND, 6, 2, WV> of the completion pass: k = 100 on the corpus with more near-ties at the top than a list
    of 128 holds, so no query is proven by the first pass. 9 queries: up to 8 unproven ones take the exact engine instead (knn_mfma);
    the 8-wave tile serves the dot kind from 257 unproven queries on"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("no_split_filter", 1)
    st = innr.KnnStats()
    _, log = _knn_vs_oracle(B, innr, metric, D_GEMM, "dup", nq, 100, stats=st, engine=innr.KNN_MFMA)
    print(f"{metric}: {st.queries_fallback} of {nq} queries unproven after the first pass; launches {log}")
    _expect(log, ("gemm_f32", KIND_OF[metric], 12, 0, wv if nq > 256 else 1), groups=1)
    _expect(log, ("gemm_f32", KIND_OF[metric], 6, 2, wv), groups=1)


@functools.lru_cache(maxsize=None)
def _u8_case(k):
    """the code corpus, the queries and the oracle's answers of the u8-kind cases (shared by the tile widths)"""
    codes = _codes(N_I8, D_GEMM, 13)
    qs = oracle.generate_uniform(3, D_GEMM, 323)
    return codes, qs, [_oracle_knn_u8(q, codes, 2.0, -1.0, k) for q in qs]


@pytest.mark.parametrize("wv", [4, 8])
@pytest.mark.parametrize("k", sorted(RR_OF_K))
def test_gemm_f32_filter_code_corpus(S, innr, ctx_option, k, wv):
    """the u8 kind <kGemmU8, RR, 0, WV> (innr_batch_knn_u8 on INNR_KNN_MFMA): 4- and 8-wave tiles only"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("gemm_waves", wv)
    codes, qs, expect = _u8_case(k)
    qc = S.QuantizedCorpus.from_codes(codes, N_I8, D_GEMM, S.QuantizationParams(2.0, -1.0))
    st = innr.KnnStats()
    (idx, sc), log = _run(lambda: qc.knn_multi(qs, k, engine=innr.KNN_MFMA, stats=st))
    assert st.engine == innr.KNN_MFMA
    for j, (oi, os_) in enumerate(expect):
        assert same_knn("dot", idx[j], sc[j], oi, os_), (j, idx[j], oi)
    _expect(log, ("gemm_f32", U8, RR_OF_K[k], 0, wv), groups=1)
    qc.close()


def _small_integers(n, nq, dim):
    """rows and queries of small integers: every product and partial sum is exact in f32 (and every value in bf16), so a dense
    score must EQUAL the integer product; asymmetric, so a transposed operand or accumulator map shows"""
    rows = ((np.arange(n)[:, None] * 7 + np.arange(dim)[None, :] * 3) % 11 - 5).astype(np.float32)
    qs = ((np.arange(nq)[:, None] * 5 + np.arange(dim)[None, :]) % 7 - 3).astype(np.float32)
    return rows, qs, (qs.astype(np.int64) @ rows.astype(np.int64).T).astype(np.float32)


@pytest.mark.parametrize("metric", ["dot", "cos"])
def test_gemm_f32_dump(B, innr, metric):
    """the dense-score mode <KIND, 6, 1, 4> behind the layout hook innrdbg_gemm_scores (lists of 32, four waves, whatever the call)"""
    rows, qs, exact = _small_integers(300, 3, D_GEMM)
    vb = B.VerticalBatch.from_rows(rows)
    if metric == "dot":
        got, log = _run(lambda: _dense_scores(vb, innr.METRIC_DOT, qs))
        assert np.array_equal(got, exact)
    else:  # the approximate cosine: the bound of test_gpu_mfma.py's dense check
        got, log = _run(lambda: _dense_scores(vb, innr.METRIC_COSINE, qs))
        data = oracle.from_rows(rows)
        norms = oracle.batch_norms(data)
        for j in range(len(qs)):
            assert np.all(np.abs(got[j] - oracle.batch_cosine(qs[j], data, norms)) <= 2e-4), j
    _expect(log, ("gemm_f32", KIND_OF[metric], 6, 1, 4), groups=1)


@pytest.mark.parametrize("k,rr", [(10, 12), (40, 20)])
def test_gemm_bf16_filter(B, innr, ctx_option, k, rr):
    """gemm_bf16_filter_kernel<RR, 0, 1> (INNR_KNN_MFMA_BF16): lists of pick_kp(4k + 64), never below 128, so RR is 12 or 20;
    every metric has a packed copy of its own"""
    ctx_option("gemm_seed_n", 256)
    for metric in ("dot", "cos", "l2"):
        _, log = _knn_vs_oracle(B, innr, metric, D_GEMM, "uniform", 3, k, engine=innr.KNN_MFMA_BF16)
        _expect(log, ("gemm_bf16", rr, 0, 1), groups=1)


@pytest.mark.parametrize("k", sorted(RR_OF_K))
def test_gemm_split_filter(B, innr, ctx_option, k):
    """gemm_bf16_filter_kernel<RR, 0, 3>: INNR_KNN_MFMA's dot / cosine filter, taken at 3 queries with split_min_q = 1"""
    ctx_option("gemm_seed_n", 256)
    ctx_option("split_min_q", 1)
    for metric in ("dot", "cos"):
        _, log = _knn_vs_oracle(B, innr, metric, D_GEMM, "uniform", 3, k, engine=innr.KNN_MFMA)
        _expect(log, ("gemm_split", RR_OF_K[k], 0, 3), groups=1)
        assert not any(e.family == "gemm_f32" and e.args[2] == 0 for e in log), log  # no first pass on the f32 kernel


def test_gemm_split_dump(B, innr):
    """the dense-score mode <6, 1, 3> behind innrdbg_split_scores: small integers have no lo limb, the sum is exact"""
    rows, qs, exact = _small_integers(300, 3, D_GEMM)
    vb = B.VerticalBatch.from_rows(rows)
    got, log = _run(lambda: _split_scores(vb, innr.METRIC_DOT, qs))
    assert np.array_equal(got, exact)
    _expect(log, ("gemm_split", 6, 1, 3), groups=1)


# ------------------------------------------------------------------------------- maxsim family
def _ms_corpus(ndocs, T, dim, full, seed=3):
    """unnormalised tokens with one zero-norm token; doc_len (unless `full`) with a T, a 0 and a 1 in it"""
    toks = (_tokens(ndocs, T, dim, seed) * np.float32(3.5)).astype(np.float32)
    toks[0, 0, :] = 0.0
    if full:
        return toks, None
    lens = np.array([(i * 7 + 3) % (T + 1) for i in range(ndocs)], dtype=np.uint32)
    lens[0], lens[1], lens[2] = T, 0, 1
    return toks, lens


def _ms_query(Tq, dim, seed=99):
    return (_tokens(1, Tq, dim, seed)[0] * np.float32(0.25)).astype(np.float32)


def _nq_of(tokens):  # the NQ instantiation of a pass of `tokens` query tokens (maxsim_scan_exact, ms_pass_nq)
    return 8 if tokens <= 8 else (16 if tokens <= 16 else 32)


def _pass_nqs(Tq):
    return [_nq_of(min(32, Tq - p0)) for p0 in range(0, Tq, 32)]


SCAN_CASES = [  # ndocs, T, dim, Tq, full
    (37, 33, 64, 5, False), (37, 16, 64, 12, False), (37, 33, 96, 32, False), (37, 16, 64, 32, False),      # Tp = 64 / 16, one group
    (9, 65, 64, 5, False), (10, 129, 64, 12, False), (10, 129, 33, 12, False),                               # MULTI: 1-token group, tail dims
    (9, 128, 128, 32, True), (9, 128, 128, 64, True), (9, 256, 128, 32, False), (9, 256, 128, 64, False),     # the reference's bench shapes
    (9, 512, 128, 32, False), (9, 512, 128, 64, False),
    (10, 65, 64, 70, False),                                                                                # passes of 32, 32 and 6 tokens
]


@pytest.mark.parametrize("ndocs,T,dim,Tq,full", SCAN_CASES)
def test_maxsim_scan_variants(M, ndocs, T, dim, Tq, full):
    toks, lens = _ms_corpus(ndocs, T, dim, full)
    q = _ms_query(Tq, dim)
    dc = M.DocumentCorpus.from_tokens(toks, lens)
    for cosine in (False, True):
        got, log = _run(lambda: dc.scores(q, cosine=cosine))
        assert bits_equal(got, _oracle_scores(q, toks, lens, cosine=cosine)), (cosine, got)
        scans = [e.inst for e in log if e.family == "ms_scan"]
        assert scans == [("ms_scan", int(cosine), nq, int(T > 64)) for nq in _pass_nqs(Tq)], log  # one launch per pass, in order
        for inst in scans:
            _expect(log, inst)
    dc.close()


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("nq", [1, 2, 4])
def test_maxsim_tile_variants(M, innr, nb, nq):
    """maxsim_mfma_tile_kernel<COS, NB, NQ>: dim = 32 NB; topk is NQ = 1, topk_multi of 2 / 4 queries of <= 32 tokens NQ = 2 / 4"""
    ndocs, T, dim, k = 300, 40, 32 * nb, 10
    toks, lens = _ms_corpus(ndocs, T, dim, False, seed=21)
    queries = [_ms_query(tq, dim, seed=100 + tq) for tq in (32, 5, 17, 1)[:nq]]
    dc = M.DocumentCorpus.from_tokens(toks, lens)
    for cosine in (False, True):
        st = innr.KnnStats()
        if nq == 1:
            (idx, sc), log = _run(lambda: dc.topk(queries[0], k, cosine=cosine, engine=innr.KNN_MFMA, stats=st))
            idx, sc = idx[None], sc[None]
        else:
            (idx, sc), log = _run(lambda: dc.topk_multi(queries, k, cosine=cosine, engine=innr.KNN_MFMA, stats=st))
        assert st.engine == innr.KNN_MFMA
        for i, q in enumerate(queries):
            s = _oracle_scores(q, toks, lens, cosine=cosine)
            order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
            assert idx[i].tolist() == order.tolist() and bits_equal(sc[i], s[order]), (cosine, i)
        _expect(log, ("ms_tile", int(cosine), nb, nq), groups=nq)
        assert not any(e.family == "ms_generic" for e in log), log
    dc.close()


def test_maxsim_tile_two_passes(M, innr):
    """a 40-token query on the tile kernel: two passes, the second adds to the first's totals (partial_in)"""
    ndocs, T, dim, k = 300, 40, 64, 10
    toks, lens = _ms_corpus(ndocs, T, dim, False, seed=22)
    q = _ms_query(40, dim)
    dc = M.DocumentCorpus.from_tokens(toks, lens)
    for cosine in (False, True):
        st = innr.KnnStats()
        (idx, sc), log = _run(lambda: dc.topk(q, k, cosine=cosine, engine=innr.KNN_MFMA, stats=st))
        s = _oracle_scores(q, toks, lens, cosine=cosine)
        order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        assert idx.tolist() == order.tolist() and bits_equal(sc, s[order]) and st.engine == innr.KNN_MFMA, cosine
        assert [e.inst for e in log if e.family == "ms_tile"] == [("ms_tile", int(cosine), 2, 1)] * 2, log
        _expect(log, ("ms_tile", int(cosine), 2, 1), groups=1)
    dc.close()


@pytest.mark.parametrize("dim,generic_option", [(48, 0), (128, 1)])
def test_maxsim_generic_kernel(M, innr, ctx_option, dim, generic_option):
    """maxsim_mfma_kernel<COS>: a dimension the tile kernel has no instantiation for, and dim 128 with maxsim_generic = 1"""
    if generic_option:
        ctx_option("maxsim_generic", 1)
    ndocs, T, k = 300, 40, 10
    toks, lens = _ms_corpus(ndocs, T, dim, False, seed=23)
    q = _ms_query(12, dim)
    dc = M.DocumentCorpus.from_tokens(toks, lens)
    for cosine in (False, True):
        st = innr.KnnStats()
        (idx, sc), log = _run(lambda: dc.topk(q, k, cosine=cosine, engine=innr.KNN_MFMA, stats=st))
        s = _oracle_scores(q, toks, lens, cosine=cosine)
        order = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        assert idx.tolist() == order.tolist() and bits_equal(sc, s[order]) and st.engine == innr.KNN_MFMA, cosine
        _expect(log, ("ms_generic", int(cosine)))
        assert not any(e.family == "ms_tile" for e in log), log
    dc.close()


RERANK_CASES = [  # ndocs, T, dim, tq (per query), full
    (37, 33, 64, [5, 5, 5], False), (37, 16, 64, [12, 12, 12], False), (37, 33, 96, [32, 32, 32], False),
    (10, 65, 64, [5, 5, 5], False), (10, 129, 33, [12, 12, 12], False), (9, 128, 128, [32, 32, 32], True),
    (10, 129, 64, [70, 33, 0], False),  # three passes (32, 32, 6 tokens), a query that ends after the second, the empty query
    (9, 256, 128, [64, 64, 64], False), (9, 512, 128, [32, 32, 32], False),
]


@pytest.mark.parametrize("ndocs,T,dim,tq,full", RERANK_CASES)
def test_maxsim_rerank_variants(M, ndocs, T, dim, tq, full):
    kc = k = 7
    toks, lens = _ms_corpus(ndocs, T, dim, full)
    allq = (_tokens(len(tq), max(tq), dim, 8) * np.float32(0.25)).astype(np.float32)
    queries = [allq[j, :tq[j]] for j in range(len(tq))]
    rng = np.random.default_rng(ndocs * 31 + T)
    cand = np.stack([rng.permutation(ndocs)[:kc] for _ in range(len(tq))]).astype(np.uint64)
    cand[0] = np.array([0, 1, 2] + [c for c in cand[0].tolist() if c not in (0, 1, 2)][:kc - 3], np.uint64)  # the full, empty, 1-token documents
    dc = M.DocumentCorpus.from_tokens(toks, lens)
    for cosine in (False, True):
        po = PairOracle(queries, toks, lens, cosine)
        (idx, sc), log = _run(lambda: _check_rerank(dc, po, queries, cand, k, cosine, what=f"T={T} cos={cosine}"))
        passes = [e.inst for e in log if e.family == "ms_rerank"]
        assert passes == [("ms_rerank", int(cosine), nq, int(T > 64)) for nq in _pass_nqs(max(tq))], log
        for inst in passes:
            _expect(log, inst, groups=len(tq))
        if T > 64:  # the wave pass is a hand copy of the scan kernel's body: the two must agree bit for bit
            for j in range(len(tq)):
                full_sc = dc.scores(queries[j], cosine=cosine)
                ei, es = _rank(cand[j], full_sc[cand[j].astype(np.int64)], k)
                assert idx[j].tolist() == ei.tolist() and bits_equal(sc[j], es), (cosine, j)
    dc.close()


# ------------------------------------------------------------------------------- the table is complete
def test_every_launch_of_this_file_has_a_row():
    """runs last: whatever the cases above launched in the tabled families is named by the table. (With the whole file run, every
    row has also been asserted by some case: rows a public call cannot reach would show here.)"""
    stray = {i for i in _SEEN if i[0] in TABLE_FAMILIES} - TABLE
    assert not stray, f"instantiations without a row in the table: {sorted(stray)}"
    print(f"{len(_ASSERTED)} of {len(TABLE)} instantiations asserted; not asserted in this run: {sorted(TABLE - _ASSERTED)}")
