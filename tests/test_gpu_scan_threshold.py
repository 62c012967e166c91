"""GPU tests of the exact scans where a wave's RUNNING THRESHOLD filters (topk_dev.h): scan_filter_kernel (kernels_scan.h),
scan_u8_filter_kernel (kernels_u8.h) and dense_filter_kernel (kernels_maxsim.h). A wave owns `cps` consecutive chunks; it admits
what is not worse than its list's threshold and compacts the list (wave_compact) when it runs short of room, which sets the
threshold. At the default geometry a wave owns ONE chunk until the chip is full (1.5M f32 vectors, 4M codes, 0.5M documents), so the
threshold is computed and never applied. The option scan_max_slots = 4 cuts a small corpus into four wave slots instead: a
20 000-vector corpus then runs at cps = 20, and the CPU oracle still costs milliseconds.

Every case (1) compares the public call's answer with the CPU oracle bit for bit and (2) asserts from the record of exact-scan
launches (api_internal.h: innr_ctx::scan_log, read by the hook innrdbg_scan_log of the test-hooks library) that the instantiation
it is named after served the call, at a cps of at least what the case needs: >= 2 everywhere, >= 6 where an in-loop compaction
of a list of 256 (R = 20: it fills after four chunks) is the point. A case that ran at cps = 1 fails.

Patterns (each on every R and QB at least once, but for rank_k): ascending and descending scores (D = 2, and D = 1), the best
candidates late in a wave's range and in the ragged last chunk, rank_k -- the k-th best alone behind the threshold of the k - 1
better ones; k = KP, the one case where a threshold one rank too high changes the answer, so by construction R = 6 and R = 12
only: k = 240 leaves sixteen ranks of slack in a list of 256 --, a tie plateau across rank k, +-inf and +-NaN scores, clipped and empty slots, masks with
empty chunks, ragged query groups; three f32 cases and one u8 case run at the default geometry on a corpus just past the chip.

The table names every instantiation of the three kernels; the last test checks that each one was asserted by some case."""
from __future__ import annotations

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle
from test_gpu_exact import bits_equal, same_knn, scanned
from test_gpu_filtered_multi import _expected as _expected_masked
from test_gpu_maxsim import _oracle_scores

DOT, L2, COS = 0, 1, 2  # INNR_METRIC_*
CODE = {"dot": DOT, "l2": L2, "cos": COS}
R_OF_K = {32: 6, 128: 12, 240: 20}  # lists of pick_kp(k) = 32 / 128 / 256 candidates: capacity 64 R (exact_cap); k = KP for the first two
QBS, KS, METRICS = (1, 4, 8), (32, 128, 240), ("dot", "l2", "cos")
DIAG = [(1, 32), (4, 128), (8, 240)]  # every QB and every R once
QB_OF_NQ = {1: 1, 3: 4, 4: 4, 6: 8, 8: 8}  # knn_exact_range: 2-3 queries share a padded 4-query pass, 5-7 a padded 8-query pass

F32_PLAIN = [("f32", qb, m, rr, 0) for qb in QBS for m in (DOT, L2, COS) for rr in (6, 12, 20)]  # scan_filter_kernel<QB, L2, COS, R, false>
F32_EXT = [("f32", qb, m, rr, 1) for qb in QBS for m in (DOT, L2, COS) for rr in (6, 12, 20)]    # ... <QB, L2, COS, R, true>
U8 = [("u8", qb, rr, mk) for qb in QBS for rr in (6, 12, 20) for mk in (0, 1)]                   # scan_u8_filter_kernel<QB, R, MASK>
DENSE = [("dense", rr) for rr in (6, 12, 20)]                                                    # dense_filter_kernel<R>
TABLE = set(F32_PLAIN + F32_EXT + U8 + DENSE)
_SEEN: set = set()      # every instantiation a case of this file launched
_ASSERTED: set = set()  # ... and the ones a case asserted by name

N_F32 = 20_400   # 80 chunks of 256, the last one with 176 vectors: four slots of 20 chunks
CPS_F32 = 20
N_U8 = 20_999    # 21 chunks of 1024 codes, the last one with 519: slots of 6, 6, 6 and 3 chunks
N_DOCS = 5_500   # 22 chunks of 256 documents, the last one with 124: slots of 6, 6, 6 and 4 chunks
QP = (2.0, -1.0)  # alpha, offset of the code corpora


def _run(call):
    res, log = scanned(call)
    _SEEN.update(e.inst for e in log)
    return res, log


def _expect(log, inst, min_cps, groups=None, nslots=4):
    """the named instantiation is in the scan record, every launch of the call ran at cps >= min_cps on `nslots` wave slots"""
    assert inst in TABLE, inst
    assert min_cps >= 2
    hits = [e for e in log if e.inst == inst and (groups is None or e.groups == groups)]
    assert hits, f"{inst} (groups {groups}) not launched; the call's exact scans: {log}"
    low = [e for e in log if e.cps < min_cps or (nslots is not None and e.nslots != nslots)]
    assert not low, f"{inst}: a wave must own >= {min_cps} chunks on {nslots} slots for this case to mean anything, the call ran {low}"
    _ASSERTED.add(inst)
    return hits[0]


def _min_cps(k):
    return 6 if R_OF_K[k] == 20 else 2


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


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


@pytest.fixture
def four_slots(ctx_option):
    ctx_option("scan_max_slots", 4)


_VB: dict = {}


def _batch(B, key, rows):
    """one resident f32 corpus at a time, shared by consecutive cases"""
    if key not in _VB:
        for vb in _VB.values():
            vb.close()
        _VB.clear()
        _VB[key] = B.VerticalBatch.from_rows(rows)
    return _VB[key]


OFN = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}


def _knn(B, innr, metric, key, rows, data, qs, k, cut_tie=None):
    """the plain exact call of `metric` for the queries `qs`, compared with the oracle per query; returns (oracle answers, scans)"""
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi, "l2": B.batch_knn_multi}[metric]
    vb = _batch(B, key, rows)
    (idx, sc), log = _run(lambda: fn(qs, vb, k, engine=innr.KNN_EXACT))
    assert idx.shape == (len(qs), min(k, len(rows)))
    exp = [OFN[metric](q, data, k) for q in qs]
    for j, (oi, os_) in enumerate(exp):
        if metric == "l2" and cut_tie is not None:
            # Squared L2 with a tie ACROSS rank k: which of the tied vectors the reference keeps is a property of core's binary
            # search inside TopK::insert, so at the cut only the distances are comparable with the oracle
            # (test_gpu_mfma.py::test_knn_mfma_near_ties_around_the_cut): identical score lists, identical indices above the
            # last distance. The tied ones are held to the library's own documented rule instead (include/innr_hip.h: distance
            # ascending, ties -> lower index): exactly the first members of the plateau `cut_tie`, in index order.
            assert bits_equal(sc[j], os_), (k, j, sc[j][:8], os_[:8])
            inner = os_ != os_[-1]
            assert sorted(idx[j][inner].tolist()) == sorted(oi[inner].tolist()), (k, j)
            ntied = int((~inner).sum())
            assert idx[j][~inner].tolist() == list(range(cut_tie[0], cut_tie[0] + ntied)) and ntied < cut_tie[1] - cut_tie[0], (k, j, idx[j][~inner][:8])
            continue
        assert same_knn(metric, idx[j], sc[j], oi, os_), (metric, k, j, idx[j][:8], oi[:8], sc[j][:8], os_[:8])
    return exp, log


def _knn_masked(B, innr, metric, key, rows, qs, k, mask):
    """innr_batch_knn_filtered_multi on the exact engine: the masked scan (EXT); the reference's batch_knn_filtered is a stable
    sort for every metric, so the index lists are compared position by position"""
    vb = _batch(B, key, rows)
    st = innr.KnnStats()
    (idx, sc), log = _run(lambda: B.batch_knn_filtered_multi(qs, vb, k, mask, metric=CODE[metric], engine=innr.KNN_EXACT, stats=st))
    assert st.engine == innr.KNN_EXACT
    exp = _expected_masked(CODE[metric], rows, mask, qs, k)
    assert idx.shape == (len(qs), min(k, int(mask.sum())))
    for j, (oi, os_) in enumerate(exp):
        assert idx[j].tolist() == oi.tolist(), (metric, k, j, idx[j][:8], oi[:8])
        assert bits_equal(sc[j], os_), (metric, k, j, sc[j][:8], os_[:8])
    return exp, log


# ------------------------------------------------------------------------------- f32 corpora and their queries
@functools.lru_cache(maxsize=None)
def _monotone(n=N_F32):
    """rows (x_i, 1) with x rising with the index. Under a query of the ASCENDING kind every score beats everything before it: each
    vector is admitted, lists fill and compact at every step. Under one of the DESCENDING kind the first compaction's threshold
    must reject everything later without losing rank KP."""
    rows = np.ones((n, 2), np.float32)
    rows[:, 0] = np.arange(n, dtype=np.float32) * np.float32(0.0002)
    return _ro(rows, oracle.from_rows(rows))


def _monotone_queries(metric, nq, n=N_F32, kinds="ad"):
    """query j is ascending ('a') or descending ('d') by kinds[j % len(kinds)]; all distinct"""
    xmax = float(n) * 0.0002
    qs = np.zeros((nq, 2), np.float32)
    for j in range(nq):
        up = kinds[j % len(kinds)] == "a"
        if metric == "dot":    # x * a + b
            qs[j] = [(1.0 + 0.25 * j) * (1 if up else -1), 0.5 - 0.1 * j]
        elif metric == "l2":   # (c - x)^2 + 0: c beyond the last x, or below the first
            qs[j] = [xmax + 1.0 + j if up else -1.0 - j, 1.0]
        else:                  # (a x + b) / (|q| sqrt(x^2 + 1)): rises with x while x < a / b = 10 (1 + j) / j > xmax
            qs[j] = [(1.0 + j) * (1 if up else -1), 0.1 * j * (1 if up else -1)]
    return qs


U_DIR = np.float32([0.6, -0.5, 0.62])
PLANT = (19 * 256 + 10, 79 * 256 + 5)  # chunk 19: the last of wave 0's range; chunk 79: the ragged last chunk of the corpus
PLANT_LEN = 120


@functools.lru_cache(maxsize=None)
def _late(n=N_F32):
    """uniform rows in the half space away from U_DIR, and 240 rows near U_DIR -- the best under every metric for queries near
    U_DIR -- planted where a wave sees them last: in the last chunk of wave 0's range and in the ragged last chunk"""
    rows = oracle.generate_uniform(n, 3, 101).copy()
    rows[(rows @ U_DIR) > 0] *= np.float32(-1.0)
    noise = oracle.generate_uniform(2 * PLANT_LEN, 3, 102)
    planted = []
    for h, start in enumerate(PLANT):
        for m in range(PLANT_LEN):
            rows[start + m] = U_DIR * np.float32(1.0 + 0.002 * m) + np.float32(0.2) * noise[h * PLANT_LEN + m]
            planted.append(start + m)
    assert max(planted) < n
    return _ro(rows, oracle.from_rows(rows)) + (frozenset(planted),)


def _late_queries(nq):
    noise = oracle.generate_uniform(nq, 3, 103)
    return np.stack([U_DIR * np.float32(1.0 + 0.03 * j) + np.float32(0.05) * noise[j] for j in range(nq)]).astype(np.float32)


PLATEAU = (17 * 256 + 100, 23 * 256 + 50)  # chunks 17..22: three chunks of wave 0's range and three of wave 1's
PLATEAU_X = np.float32(2.0)


@functools.lru_cache(maxsize=None)
def _plateau(k, n=N_F32):
    """rows (x_i, 1): k // 2 rows with distinct x > 2 (scattered, some of them late), a plateau of 1486 rows with x = 2 exactly that
    straddles rank k, spans several chunks of wave 0 and crosses into wave 1's range, everything else below 1. Equal x, equal score
    under every metric: the k - k // 2 plateau members with the lowest indices complete the answer."""
    rows = np.ones((n, 2), np.float32)
    rows[:, 0] = (0.1 + 0.8 * ((np.arange(n) * 0.6180339887) % 1.0)).astype(np.float32)
    rows[PLATEAU[0]:PLATEAU[1], 0] = PLATEAU_X
    better = [60 * 256 + 9, 79 * 256 + 170, 16 * 256 + 255, 23 * 256 + 60]
    better += [i for i in ((m * 2731 + 77) % n for m in range(k)) if not PLATEAU[0] <= i < PLATEAU[1]][:k // 2 - 4]
    assert len(set(better)) == len(better) == k // 2
    for m, i in enumerate(better):
        rows[i, 0] = np.float32(3.0 + 0.01 * m)
    return _ro(rows, oracle.from_rows(rows))


def _neg_nan():
    return np.uint32(0xFFC00000).view(np.float32)


@functools.lru_cache(maxsize=None)
def _special_dot(kp, n=N_F32):
    """dot: KP + 8 rows scoring +inf early in wave 0's range, so the first compaction's threshold IS +inf; +NaN rows later in the same
    range (total_cmp ranks +NaN above +inf: they must still be admitted, and come first). The same in wave 2's range with fewer
    than KP infinities; a few -inf and -NaN rows, which rank last."""
    rows = oracle.generate_uniform(n, 2, 111).copy()
    rows[10:10 + kp + 8, 0] = np.inf
    rows[40 * 256 + 3:40 * 256 + 3 + kp // 2, 0] = np.inf
    nans = [15 * 256 + 77, 19 * 256 + 250, 59 * 256 + 1]
    for i in nans:
        rows[i, 0] = np.nan
    for i in (5, 18 * 256 + 9, 79 * 256 + 100):
        rows[i, 0] = -np.inf
    for i in (7, 17 * 256 + 30, 70 * 256):
        rows[i, 0] = _neg_nan()
    return _ro(rows, oracle.from_rows(rows)) + (tuple(nans),)


@functools.lru_cache(maxsize=None)
def _special_l2(kp, n=N_F32):
    """squared L2, where smaller is better and total_cmp ranks -NaN below everything: KP + 8 copies of (0.5, 0.5) early in wave 0's
    range -- distances from 0 to 1e-7 -- then -NaN rows later in the same range: they must still be admitted, and come first.
    +NaN and +-inf rows rank last."""
    rows = oracle.generate_uniform(n, 2, 112).copy()
    rows[10:10 + kp + 8, 0] = 0.5
    rows[10:10 + kp + 8, 1] = (0.5 + 1e-6 * np.arange(kp + 8)).astype(np.float32)  # (distinct distances: no tie at the cut)
    nnans = [15 * 256 + 77, 19 * 256 + 250, 59 * 256 + 1]
    for i in nnans:
        rows[i, 0] = _neg_nan()
    for i, v in ((5, np.inf), (18 * 256 + 9, -np.inf), (79 * 256 + 100, np.inf), (7, np.nan), (17 * 256 + 30, np.nan)):
        rows[i, 0] = v
    return _ro(rows, oracle.from_rows(rows)) + (tuple(nnans),)


def _chunk_mask(n, chunk, seed):
    """by chunk of `chunk` vectors: every third one empty, every third one with ONE passing vector, the others half full"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, np.uint8)
    for c in range((n + chunk - 1) // chunk):
        lo, hi = c * chunk, min((c + 1) * chunk, n)
        if c % 3 == 1:
            mask[lo + (c * 37) % (hi - lo)] = 1
        elif c % 3 == 2:
            mask[lo:hi] = rng.random(hi - lo) < 0.5
    return mask


# ------------------------------------------------------------------------------- scan_filter_kernel, EXT = 0
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb", QBS)
def test_f32_ascending_and_descending(B, innr, four_slots, qb, metric, k):
    """all 27 plain instantiations: scores that rise with the index (every vector admitted, a compaction every step) and scores that
    fall with it (the first threshold rejects the rest), both kinds in every group of 4 or 8 queries"""
    rows, data = _monotone()
    inst = ("f32", qb, CODE[metric], R_OF_K[k], 0)
    for kinds in (("a", "d") if qb == 1 else ("ad",)):
        _, log = _knn(B, innr, metric, "monotone", rows, data, _monotone_queries(metric, qb, kinds=kinds), k)
        e = _expect(log, inst, min_cps=_min_cps(k), groups=1)
        assert e.cps == CPS_F32 and len(log) == 1, log


@functools.lru_cache(maxsize=None)
def _monotone_1d(n=N_F32):
    """_monotone's first column alone: D = 1, where the dimension loop of scan_accumulate is a single step of its tail"""
    rows = np.ascontiguousarray(_monotone(n)[0][:, :1])
    return _ro(rows, oracle.from_rows(rows))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k", DIAG)
def test_f32_single_dimension(B, innr, four_slots, qb, k, metric):
    """D = 1: ascending and descending scores under dot and squared L2; under cosine every score is +1, -1 or (the zero row) 0, one
    tie plateau over the whole corpus, so the first k indices (ascending kind: from row 1 on) are the answer"""
    rows, data = _monotone_1d()
    qs = np.ascontiguousarray(_monotone_queries(metric, max(qb, 2))[:, :1])
    for sel in ((slice(0, 1), slice(1, 2)) if qb == 1 else (slice(0, qb),)):
        exp, log = _knn(B, innr, metric, "monotone_1d", rows, data, qs[sel], k)
        if metric == "cos":  # the test's own construction
            assert all(oi.tolist() == list(range(1, k + 1)) if q[0] > 0 else int(oi[0]) == 0 for q, (oi, _) in zip(qs[sel], exp))
        _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=_min_cps(k), groups=1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k", DIAG)
def test_f32_late_best_candidates(B, innr, four_slots, qb, k, metric):
    """the k best arrive in the last chunk of a wave's range and in the ragged last chunk of the corpus, behind a threshold that
    twenty chunks of ordinary rows have raised"""
    rows, data, planted = _late()
    exp, log = _knn(B, innr, metric, "late", rows, data, _late_queries(qb), k)
    for oi, _ in exp:
        assert set(int(i) for i in oi) <= planted, "the test's own construction: the best k are the planted rows"
        assert any(int(i) >= PLANT[1] for i in oi) and any(int(i) < PLANT[1] for i in oi)
    _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=_min_cps(k), groups=1)


RANK_K_X = 19 * 256 + 250  # in the last chunk of wave 0's range
RANK_K_DECOY = 200


@functools.lru_cache(maxsize=None)
def _rank_k_late(kp, n=N_F32):
    """rows (x_i, 1), the whole top KP inside wave 0's range: KP - 1 rows with x >= 3 and a decoy with x = 2 in chunk 0, so the first
    compaction (after chunk 0 for lists of 32, after chunk 2 for lists of 128) holds exactly these KP and its threshold is the
    decoy's score; then, seventeen chunks later, ONE row with x = 2.5. With k = KP it is the k-th best and replaces the decoy -- a
    threshold one rank too high (the worst of the KP - 1) would reject it. Everything else has x < 1."""
    assert kp - 1 + 5 <= RANK_K_DECOY < 256
    rows = np.ones((n, 2), np.float32)
    rows[:, 0] = (0.1 + 0.8 * ((np.arange(n) * 0.6180339887) % 1.0)).astype(np.float32)
    rows[5:5 + kp - 1, 0] = (3.0 + 0.01 * np.arange(kp - 1)).astype(np.float32)
    rows[RANK_K_DECOY, 0] = 2.0
    rows[RANK_K_X, 0] = 2.5
    return _ro(rows, oracle.from_rows(rows))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k", [(1, 32), (4, 128), (8, 32), (1, 128), (4, 32), (8, 128)])
def test_f32_rank_k_arrives_after_the_threshold(B, innr, four_slots, qb, k, metric):
    """k = KP: the k-th best of the corpus arrives alone, late in the range of the wave that already holds the k - 1 better ones and
    a threshold -- no slack for a threshold that is one rank off"""
    rows, data = _rank_k_late(k)
    exp, log = _knn(B, innr, metric, ("rank_k", k), rows, data, _monotone_queries(metric, qb, kinds="a"), k)
    for oi, _ in exp:  # the test's own construction
        assert int(oi[-1]) == RANK_K_X and RANK_K_DECOY not in oi.tolist() and sorted(oi[:-1].tolist()) == list(range(5, 5 + k - 1))
    _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=2, groups=1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k", DIAG)
def test_f32_tie_plateau_straddles_rank_k(B, innr, four_slots, qb, k, metric):
    """exactly equal scores across rank k, over several chunks of one wave and the boundary between two: ties go to the lower index
    (dot, cosine: position by position against the oracle; squared L2: see _knn)"""
    rows, data = _plateau(k)
    exp, log = _knn(B, innr, metric, ("plateau", k), rows, data, _monotone_queries(metric, qb, kinds="a"), k, cut_tie=PLATEAU)
    oi, os_ = exp[0]
    tied = [int(i) for i, s in zip(oi, os_) if s == os_[-1]]
    assert len(tied) == k - k // 2 and all(PLATEAU[0] <= i < PLATEAU[1] for i in tied), "the test's own construction"
    if metric != "l2":
        assert sorted(tied) == list(range(PLATEAU[0], PLATEAU[0] + len(tied)))
    _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=_min_cps(k), groups=1)


@pytest.mark.parametrize("metric", ["dot", "l2"])
@pytest.mark.parametrize("qb,k", DIAG)
def test_f32_special_scores_pass_a_saturated_threshold(B, innr, four_slots, qb, k, metric):
    """the best score there is (+NaN under dot, -NaN under squared L2) arrives after the wave's threshold has reached the best
    ordinary one (+inf / distance 0): it is admitted and ranks first"""
    kp = {32: 32, 128: 128, 240: 256}[k]
    if metric == "dot":
        rows, data, first = _special_dot(kp)
        qs = np.float32([[1.0 + 0.25 * j, 0.5 - 0.05 * j] for j in range(qb)])
    else:
        rows, data, first = _special_l2(kp)
        qs = np.float32([[0.5 + 0.001 * j, 0.5] for j in range(qb)])
    exp, log = _knn(B, innr, metric, ("special", metric, kp), rows, data, qs, k)
    for oi, os_ in exp:  # the test's own construction, on the oracle's answer
        assert sorted(int(i) for i in oi[:3]) == sorted(first) and np.isnan(os_[:3]).all() and not np.isnan(os_[3:]).any()
        assert bool(np.signbit(os_[0])) == (metric == "l2")
    _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=_min_cps(k), groups=1)


@pytest.mark.parametrize("max_slots,n", [(4, 8 * 256 + 77), (12, 24 * 256 + 77)])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k", [(1, 32), (4, 128), (8, 240), (8, 32), (1, 240)])
def test_f32_clipped_and_empty_slots(B, innr, ctx_option, qb, k, metric, max_slots, n):
    """nchunks = 2 nslots + 1: cps = 3, so the slot after the full ones is clipped to one ragged chunk and the rest own nothing (four
    slots: 3 + 3 + 3 + 0 chunks; twelve: eight full ones, one chunk, three empty): the ch1 > nchunks clip, the zero counts it
    leaves and what the select makes of them. (At cps = 3 a list of 256 cannot compact inside the loop: the R = 20 rows are here
    for the clip, at cps >= 2 like the others. The four-slot corpus has 2 125 vectors because nine chunks have no more.)"""
    ctx_option("scan_max_slots", max_slots)
    rows, data = _monotone(n)
    _, log = _knn(B, innr, metric, ("monotone", n), rows, data, _monotone_queries(metric, qb, n=n), k)
    e = _expect(log, ("f32", qb, CODE[metric], R_OF_K[k], 0), min_cps=2, groups=1, nslots=max_slots)
    assert e.cps == 3 and 2 * e.nslots + 1 == (n + 255) // 256, log


@pytest.mark.parametrize("nq", [3, 6, 19])
@pytest.mark.parametrize("metric,k", [("dot", 32), ("l2", 128), ("cos", 240), ("l2", 32)])
def test_f32_ragged_query_groups(B, innr, four_slots, nq, metric, k):
    """3 queries: a padded 4-group; 6: a padded 8-group; 19: two 8-groups in one launch, then a padded 4-group in a launch of its own.
    The zero rows that pad a group contribute nothing; every real query matches the oracle."""
    for key, (rows, data), qs in (("monotone", _monotone(), _monotone_queries(metric, nq)), ("late", _late()[:2], _late_queries(nq))):
        _, log = _knn(B, innr, metric, key, rows, data, qs, k)
        rr, m = R_OF_K[k], CODE[metric]
        if nq == 19:
            assert [(e.inst, e.groups) for e in log] == [(("f32", 8, m, rr, 0), 2), (("f32", 4, m, rr, 0), 1)], log
            _expect(log, ("f32", 8, m, rr, 0), min_cps=_min_cps(k), groups=2)
            _expect(log, ("f32", 4, m, rr, 0), min_cps=_min_cps(k), groups=1)
        else:
            assert len(log) == 1, log
            _expect(log, ("f32", QB_OF_NQ[nq], m, rr, 0), min_cps=_min_cps(k), groups=1)


# ------------------------------------------------------------------------------- scan_filter_kernel, EXT = 1
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb", QBS)
def test_f32_masked(B, innr, four_slots, qb, metric, k):
    """all 27 extended instantiations through innr_batch_knn_filtered_multi on the exact engine. The mask has whole chunks empty,
    chunks with one passing vector and half-full ones; the corpus is the one with the best rows late, then the ascending one."""
    mask = _chunk_mask(N_F32, 256, 5)
    inst = ("f32", qb, CODE[metric], R_OF_K[k], 1)
    rows, _, _ = _late()
    _, log = _knn_masked(B, innr, metric, "late", rows, _late_queries(qb), k, mask)
    _expect(log, inst, min_cps=_min_cps(k), groups=1)
    rows, _ = _monotone()
    _, log = _knn_masked(B, innr, metric, "monotone", rows, _monotone_queries(metric, qb), k, mask)
    _expect(log, inst, min_cps=_min_cps(k), groups=1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("qb,k,npass", [(1, 32, 20), (4, 128, 100), (8, 240, 200), (8, 240, 1)])  # (one more passes: see below)
def test_f32_masked_fewer_passing_than_k(B, innr, four_slots, qb, k, npass, metric):
    """fewer vectors pass than k: every one of them is returned, in order. `npass` random vectors and one row of the ragged last
    chunk pass (row 0 never does), so k becomes 21, 101, 201 or 2: the first three keep the list length of k = 32, 128 and 240,
    two passing vectors take the shortest lists"""
    rows, _, _ = _late()
    mask = np.zeros(N_F32, np.uint8)
    mask[np.random.default_rng(npass).choice(N_F32, size=npass, replace=False)] = 1
    mask[PLANT[1] + 3] = 1
    mask[0] = 0
    npass = int(mask.sum())
    exp, log = _knn_masked(B, innr, metric, "late", rows, _late_queries(qb), k, mask)
    assert all(len(oi) == npass for oi, _ in exp)
    rr = 6 if npass <= 32 else R_OF_K[k]
    _expect(log, ("f32", qb, CODE[metric], rr, 1), min_cps=6 if rr == 20 else 2, groups=1)


@pytest.mark.parametrize("k", KS)
def test_f32_single_query_l2_forms(B, innr, four_slots, k):
    """innr_batch_knn_filtered (a mask) and innr_batch_knn_reordered (a dimension order): the reference's single-query squared-L2
    forms, both on scan_filter_kernel<1, L2, R, EXT>"""
    inst = ("f32", 1, L2, R_OF_K[k], 1)
    mask = _chunk_mask(N_F32, 256, 6)
    for key, (rows, data), q in (("late", _late()[:2], _late_queries(1)[0]), ("monotone", _monotone(), _monotone_queries("l2", 1)[0])):
        vb = _batch(B, key, rows)
        r, log = _run(lambda: B.batch_knn_filtered(q, vb, k, lambda i: bool(mask[i])))
        oi, os_ = oracle.batch_knn_filtered(q, data, k, mask)
        assert r.indices == oi.tolist() and bits_equal(np.float32(r.scores), os_), (key, r.indices[:8], oi[:8])
        _expect(log, inst, min_cps=_min_cps(k), groups=1)
        r, log = _run(lambda: B.batch_knn_reordered(q, vb, k))
        oi, os_ = oracle.batch_knn_reordered(q, data, k)
        assert r.indices == oi.tolist() and bits_equal(np.float32(r.scores), os_), (key, r.indices[:8], oi[:8])
        _expect(log, inst, min_cps=_min_cps(k), groups=1)
    few = np.zeros(N_F32, np.uint8)  # fewer passing than k: all of them, in order
    few[[3, 19 * 256 + 200, PLANT[1] + 1, N_F32 - 1]] = 1
    r, log = _run(lambda: B.batch_knn_filtered(q, vb, k, lambda i: bool(few[i])))
    oi, os_ = oracle.batch_knn_filtered(q, data, k, few)
    assert len(oi) == 4 and r.indices == oi.tolist() and bits_equal(np.float32(r.scores), os_)
    _expect(log, inst, min_cps=_min_cps(k), groups=1)


# ------------------------------------------------------------------------------- scan_u8_filter_kernel
@functools.lru_cache(maxsize=None)
def _codes(kind, n=N_U8):
    """rising: one dimension, codes that rise with the index -- 256 plateaus of 82 equal scores each, ascending under a positive
    query and descending under a negative one. late: three dimensions of random codes below 200 and 240 rows of (255 - m % 50, 255,
    255), the best under an all-positive query, in the last chunk of wave 0's range and in the ragged last chunk of the corpus."""
    if kind == "rising":
        codes = ((np.arange(n, dtype=np.int64) * 256) // n).astype(np.uint8).reshape(n, 1)
    else:
        codes = np.random.default_rng(7).integers(0, 200, size=(n, 3), dtype=np.uint8)
        last = (n - 1) // 1024
        cps = ((last + 1) + 3) // 4
        for start in ((cps - 1) * 1024 + 600, last * 1024 + 11):
            for m in range(PLANT_LEN):
                codes[start + m] = (255 - m % 50, 255, 255)
        assert last * 1024 + 11 + PLANT_LEN <= n
    return _ro(codes)


def _code_queries(kind, nq):
    if kind == "rising":
        return np.float32([[(1.0 + 0.25 * j) * (1 if j % 2 == 0 else -1)] for j in range(nq)])
    return np.float32([[1.0 + 0.1 * j, 0.5 + 0.05 * j, 0.75] for j in range(nq)])


_QC: dict = {}


def _code_corpus(S, key, codes):
    if key not in _QC:
        for qc in _QC.values():
            qc.close()
        _QC.clear()
        _QC[key] = S.QuantizedCorpus.from_codes(codes, codes.shape[0], codes.shape[1], S.QuantizationParams(*QP))
    return _QC[key]


def _knn_u8(S, innr, key, codes, qs, k, mask=None):
    """knn_multi / knn_filtered_multi of a code corpus on the exact engine against batch_knn_u8 (a stable sort: position by position)"""
    qc = _code_corpus(S, key, codes)
    st = innr.KnnStats()
    if mask is None:
        (idx, sc), log = _run(lambda: qc.knn_multi(qs, k, engine=innr.KNN_EXACT, stats=st))
        sel = np.arange(len(codes))
    else:
        (idx, sc), log = _run(lambda: qc.knn_filtered_multi(qs, k, mask, engine=innr.KNN_EXACT, stats=st))
        sel = np.flatnonzero(mask)
    assert st.engine == innr.KNN_EXACT and idx.shape == (len(qs), min(k, len(sel)))
    sub = np.ascontiguousarray(codes[sel])
    for j, q in enumerate(qs):
        oi, os_ = oracle.batch_knn_u8(q, sub, oracle.QParams(*QP), k)
        oi = sel[oi.astype(np.int64)]
        assert idx[j].tolist() == oi.tolist(), (key, k, j, idx[j][:8], oi[:8])
        assert bits_equal(sc[j], os_), (key, k, j, sc[j][:8], os_[:8])
    return log


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("qb", QBS)
def test_u8_plain(S, innr, four_slots, qb, k):
    """the 9 plain instantiations: the multi-chunk loop of the code scan (a wave owns 6 chunks of 1024 codes, the last slot 3)"""
    for kind in ("rising", "late"):
        log = _knn_u8(S, innr, kind, _codes(kind), _code_queries(kind, qb), k)
        e = _expect(log, ("u8", qb, R_OF_K[k], 0), min_cps=_min_cps(k), groups=1)
        assert e.cps == 6 and len(log) == 1, log


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("qb", QBS)
def test_u8_masked(S, innr, four_slots, qb, k):
    """the 9 masked instantiations: whole chunks of 1024 empty (skipped before their codes are read), chunks with one passing code"""
    mask = _chunk_mask(N_U8, 1024, 8)
    for kind in ("rising", "late"):
        log = _knn_u8(S, innr, kind, _codes(kind), _code_queries(kind, qb), k, mask)
        _expect(log, ("u8", qb, R_OF_K[k], 1), min_cps=_min_cps(k), groups=1)


@pytest.mark.parametrize("qb,k", DIAG)
def test_u8_masked_fewer_passing_than_k(S, innr, four_slots, qb, k):
    npass = {32: 20, 128: 100, 240: 200}[k]
    mask = np.zeros(N_U8, np.uint8)
    mask[np.random.default_rng(k).choice(N_U8, size=npass, replace=False)] = 1
    log = _knn_u8(S, innr, "late", _codes("late"), _code_queries("late", qb), k, mask)
    _expect(log, ("u8", qb, R_OF_K[k], 1), min_cps=_min_cps(k), groups=1)


@functools.lru_cache(maxsize=None)
def _codes_rank_k(kp, n=N_U8):
    """_rank_k_late for one-dimensional codes: KP - 1 codes of 210 and more and a decoy of 150 in the first quarter-step of chunk 0
    (a lane owns 16 consecutive codes and admits them four at a time, compacting in between: lists of 32 compact after the first
    quarter-step, lists of 128 after the third), ONE code of 180 in the last chunk of wave 0's range, everything else <= 100"""
    codes = np.random.default_rng(9).integers(0, 101, size=(n, 1), dtype=np.uint8)
    q0 = [i for i in range(1024) if i % 16 < 4]
    for m, i in enumerate(q0[:kp - 1]):
        codes[i, 0] = 210 + m % 40
    decoy, x = q0[kp + 2], 5 * 1024 + 1000
    codes[decoy, 0] = 150
    codes[x, 0] = 180
    return _ro(codes), decoy, x


@pytest.mark.parametrize("qb,k", [(1, 32), (4, 128), (8, 32), (1, 128), (4, 32), (8, 128)])
def test_u8_rank_k_arrives_after_the_threshold(S, innr, four_slots, qb, k):
    codes, decoy, x = _codes_rank_k(k)
    qs = np.float32([[1.0 + 0.25 * j] for j in range(qb)])
    oi, _ = oracle.batch_knn_u8(qs[0], codes, oracle.QParams(*QP), k)
    assert int(oi[-1]) == x and decoy not in oi.tolist(), "the test's own construction"
    log = _knn_u8(S, innr, ("rank_k", k), codes, qs, k)
    _expect(log, ("u8", qb, R_OF_K[k], 0), min_cps=2, groups=1)


@pytest.mark.parametrize("qb,k", [(1, 32), (4, 128), (8, 240), (8, 32), (1, 240)])
def test_u8_clipped_and_empty_slots(S, innr, four_slots, qb, k):
    """nchunks = 2 nslots + 1 = 9 chunks of 1024 codes: cps = 3, the ch1 > nchunks clip leaves the last slot empty"""
    n = 8 * 1024 + 77
    log = _knn_u8(S, innr, ("rising", n), _codes("rising", n), _code_queries("rising", qb), k)
    e = _expect(log, ("u8", qb, R_OF_K[k], 0), min_cps=2, groups=1)
    assert e.cps == 3, log


@pytest.mark.parametrize("nq", [3, 6, 19])
def test_u8_ragged_query_groups(S, innr, four_slots, nq):
    """3: a padded 4-group; 6: a padded 8-group; 19: two 8-groups in one launch and a padded 4-group in the next"""
    for kind, k in (("rising", 32), ("late", 128)):
        log = _knn_u8(S, innr, kind, _codes(kind), _code_queries(kind, nq), k)
        rr = R_OF_K[k]
        if nq == 19:
            assert [(e.inst, e.groups) for e in log] == [(("u8", 8, rr, 0), 2), (("u8", 4, rr, 0), 1)], log
            _expect(log, ("u8", 8, rr, 0), min_cps=2, groups=2)
            _expect(log, ("u8", 4, rr, 0), min_cps=2, groups=1)
        else:
            _expect(log, ("u8", QB_OF_NQ[nq], rr, 0), min_cps=2, groups=1)


# ------------------------------------------------------------------------------- dense_filter_kernel
def _doc_x(pattern, k, n=N_DOCS):
    i = np.arange(n)
    if pattern == "ascending":
        return (i * 0.0005).astype(np.float32)
    if pattern == "descending":
        return ((n - 1 - i) * 0.0005).astype(np.float32)
    x = (0.1 + 0.8 * ((i * 0.6180339887) % 1.0)).astype(np.float32)
    if pattern == "late":  # the 240 best in the last chunk of wave 0's range (chunk 5) and in the ragged last chunk (21)
        for start in (5 * 256 + 100, 21 * 256 + 2):
            x[start:start + PLANT_LEN] = (3.0 + 0.01 * np.arange(PLANT_LEN)).astype(np.float32)
        return x
    if pattern == "rank_k":  # _rank_k_late's construction: chunk 5 is the last of wave 0's range
        x[5:5 + k - 1] = (3.0 + 0.01 * np.arange(k - 1)).astype(np.float32)
        x[RANK_K_DECOY] = 2.0
        x[5 * 256 + 250] = 2.5
        return x
    x[4 * 256 + 100:8 * 256 + 50] = 2.0  # plateau: chunks 4..7, two of wave 0's range and two of wave 1's, across rank k
    better = [(m * 911 + 7) % n for m in range(k // 2)]
    better = [b for b in better if not 4 * 256 + 100 <= b < 8 * 256 + 50]
    x[better] = (3.0 + 0.01 * np.arange(len(better))).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _docs(pattern, k, T, dim, cosine):
    """documents whose first token is (x_i, 1, 0, ...) and whose second (T = 2) is (x_i - 1, 1, 0, ...); the query's tokens have
    positive first coordinates, so a document's score rises with x_i. Returns tokens, query, the oracle's scores."""
    x = _doc_x(pattern, k)
    toks = np.zeros((N_DOCS, T, dim), np.float32)
    toks[:, :, 1] = 1.0
    toks[:, 0, 0] = x
    if T == 2:
        toks[:, 1, 0] = x - np.float32(1.0)
    q = np.zeros((2, dim), np.float32)
    q[0, :2] = [1.0, 0.0 if cosine else 0.5]
    q[1, :2] = [0.5, 0.0 if cosine else 0.25]
    return _ro(toks, q, _oracle_scores(q, toks, None, cosine=cosine))


@pytest.mark.parametrize("cosine", [False, True], ids=["maxsim", "cosine"])
@pytest.mark.parametrize("k", KS)
def test_dense_document_filter(M, innr, four_slots, k, cosine):
    """dense_filter_kernel<R> behind DocumentCorpus.topk on the exact engine, against a stable sort of the oracle's scores: 5500
    documents in four slots of 6, 6, 6 and 4 chunks; ascending and descending scores, the best documents late, a tie plateau across
    rank k and (k = KP) the k-th best alone behind the threshold of the k - 1 better ones"""
    T, dim = (2, 8) if k == 128 else (1, 4)
    for pattern in ("ascending", "descending", "late", "plateau") + (("rank_k",) if k != 240 else ()):
        toks, q, sc = _docs(pattern, k if pattern in ("plateau", "rank_k") else 0, T, dim, cosine)
        order = np.argsort(-sc.astype(np.float64), kind="stable")[:k]
        if pattern == "rank_k":
            assert order[-1] == 5 * 256 + 250 and RANK_K_DECOY not in order.tolist(), "the test's own construction"
        if pattern == "plateau":
            assert sc[order[-1]] == sc[order[-2]] == sc[4 * 256 + 100] and sc[order[0]] > sc[order[-1]], "the test's own construction"
        dc = M.DocumentCorpus.from_tokens(toks)
        st = innr.KnnStats()
        (idx, s), log = _run(lambda: dc.topk(q, k, cosine=cosine, engine=innr.KNN_EXACT, stats=st))
        dc.close()
        assert st.engine == innr.KNN_EXACT
        assert idx.tolist() == order.tolist() and bits_equal(s, sc[order]), (pattern, idx[:8], order[:8])
        e = _expect(log, ("dense", R_OF_K[k]), min_cps=_min_cps(k), groups=1)
        assert e.cps == 6 and [x.kind for x in log] == ["dense"], log


# ------------------------------------------------------------------------------- the default geometry, no option set
@functools.lru_cache(maxsize=1)
def _past_the_chip():
    """a two-dimensional corpus of (2 * 24 CUs + 1) * 256 + 17 uniform vectors: with the production slot count (24 waves per CU, 16
    from eight queries on) every wave owns three (four) chunks"""
    import torch
    from innr_amd import _lib
    cus = torch.cuda.get_device_properties(_lib.default_context().device).multi_processor_count
    n = (2 * 24 * cus + 1) * 256 + 17
    rows = oracle.generate_uniform(n, 2, 77)
    return cus, n, _ro(oracle.from_rows(rows))


@pytest.mark.parametrize("metric", METRICS)
def test_f32_default_geometry_past_the_chip(B, innr, metric):
    """no option: N just past two chunks per production wave slot. One query with lists of 32 and of 128 (QB = 1, R = 6 and 12), and for
    squared L2 eight queries as well; the scan record must show cps >= 2 on the production slot count."""
    from innr_amd import _lib
    assert _lib.default_context().get_option("scan_max_slots") == 0
    cus, n, data = _past_the_chip()
    if "big" not in _VB:
        for vb in _VB.values():
            vb.close()
        _VB.clear()
        _VB["big"] = B.VerticalBatch.generate(n, 2, 77)  # the device generator: the bits of oracle.generate_uniform (test_gpu_exact.py)
    vb = _VB["big"]
    fn = {"dot": B.batch_knn_dot_multi, "cos": B.batch_knn_cosine_multi, "l2": B.batch_knn_multi}[metric]
    q = oracle.generate_uniform(9, 2, 78)
    oi, os_ = OFN[metric](q[0], data, 128)
    for k in (32, 128):
        (idx, sc), log = _run(lambda: fn(q[:1], vb, k, engine=innr.KNN_EXACT))
        if metric == "l2" and k == 32:
            oi32, os32 = OFN[metric](q[0], data, 32)
        else:
            oi32, os32 = oi[:k], os_[:k]  # a stable sort's first k
        assert same_knn(metric, idx[0], sc[0], oi32, os32), (metric, k, idx[0][:8], oi32[:8])
        e = _expect(log, ("f32", 1, CODE[metric], R_OF_K[k], 0), min_cps=2, groups=1, nslots=None)
        assert e.nslots == 24 * cus and len(log) == 1, (log, cus)
    if metric == "l2":
        (idx, sc), log = _run(lambda: fn(q[1:], vb, 32, engine=innr.KNN_EXACT))
        for j in range(8):
            oj, osj = OFN[metric](q[1 + j], data, 32)
            assert same_knn(metric, idx[j], sc[j], oj, osj), (j, idx[j][:8], oj[:8])
        e = _expect(log, ("f32", 8, L2, 6, 0), min_cps=2, groups=1, nslots=None)
        assert e.nslots == 16 * cus and len(log) == 1, (log, cus)


def test_u8_default_geometry_past_the_chip(S, innr):
    """no option: one-dimensional codes just past two chunks of 1024 per production wave slot (16 waves per CU), one query. 256
    distinct scores: every rank is inside a tie, the lower index wins. (The oracle's stable sort of 8.4M scores takes 2.9 s.)"""
    import torch
    from innr_amd import _lib
    assert _lib.default_context().get_option("scan_max_slots") == 0
    cus = torch.cuda.get_device_properties(_lib.default_context().device).multi_processor_count
    n = 16 * cus * 1024 * 2 + 1024 + 5
    codes = np.random.default_rng(1).integers(0, 256, size=(n, 1), dtype=np.uint8)
    log = _knn_u8(S, innr, "big", codes, np.float32([[1.0]]), 32)
    e = _expect(log, ("u8", 1, 6, 0), min_cps=2, groups=1, nslots=None)
    assert e.nslots == 16 * cus and len(log) == 1, (log, cus)


# ------------------------------------------------------------------------------- the table is complete
def test_every_instantiation_was_asserted(request):
    """runs last: nothing outside the table was launched by a case of this file, and -- when the whole file ran -- every
    instantiation of the three kernels was asserted by name, at cps >= 2, by some case"""
    for vb in list(_VB.values()) + list(_QC.values()):
        vb.close()
    _VB.clear()
    _QC.clear()
    stray = _SEEN - TABLE
    assert not stray, f"instantiations without a row in the table: {sorted(stray)}"
    missing = sorted(TABLE - _ASSERTED)
    print(f"{len(_ASSERTED)} of {len(TABLE)} instantiations asserted; not asserted in this run: {missing}")
    # "the whole file ran" = every case of this module was selected (counted from the parametrize marks) and this test was reached:
    # a run narrowed by -k, a node id, --deselect or --lf selects fewer, and skips the completeness check
    import sys
    mod = sys.modules[__name__]
    want = 0
    for name, fn in vars(mod).items():
        if name.startswith("test_") and callable(fn):
            cases = 1
            for mark in getattr(fn, "pytestmark", []):
                if mark.name == "parametrize":
                    cases *= len(mark.args[1])
            want += cases
    selected = sum(1 for item in request.session.items if getattr(item, "module", None) is mod)
    if selected == want:
        assert not missing, f"instantiations no case asserted: {missing}"
