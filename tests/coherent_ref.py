"""Coherently rounded corpora for the int8 filter of an f32 corpus (INNR_KNN_MFMA_I8, api.hip knn_f32_i8) and the bf16 filter
(INNR_KNN_MFMA_BF16), and float64 emulations of both filters' approximate scores. numpy and the oracle only: nothing here comes
from innr_amd.

Both filters keep a row when its approximate score can still reach the top k once the bound E_j is allowed for. On ordinary data
the per-dimension rounding errors have random signs and add up like sqrt(D); here every dimension rounds the same way:
  * k TRUE rows sit just inside a rounding boundary on the side that makes the approximate score LOWER than the exact one,
  * DECOYS sit on the other side (approximate score HIGHER than the exact one), their exact scores just below the true rows',
  * int8: two PIN rows fix the range the library derives from the corpus (alpha = 2, offset = -1: step 2 / 255),
among filler rows that score far lower. Exactly the top k is the true rows; approximately every decoy beats every true row by
almost twice the bound's leading term ((alpha / 510) |q|_1 resp. 2^-7 |q| max|v|), so a filter whose bound is short loses them.

Placements of the same rows (n rows, prefix = the first 1024):
  crowded  600 decoys and the true rows anywhere: more decoys than any candidate list holds
  sparse   2k decoys inside the prefix, the true rows in the last 128-row tile: no list fills
  seeded   4k decoys inside the prefix, the true rows anywhere behind it"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import oracle

STEP = 2.0 / 255.0          # of the int8 copies: alpha = 2 (the pins), 255 steps
PREFIX = 1024
N_ROWS = 32768
PLACEMENTS = ("crowded", "sparse", "seeded")
# bf16 keeps 8 significant bits: DN rounds down to 1, UP rounds up to 1 + 2^-7, both by almost half a last place
DN = 1.0 + 2.0 ** -8 * (1.0 - 2.0 ** -6)
UP = 1.0 + 2.0 ** -8 * (1.0 + 2.0 ** -6)


class Case(NamedTuple):
    engine: str          # "i8" | "bf16"
    metric: str          # "dot" | "cos" | "l2"
    k: int
    rows: np.ndarray     # [n][dim] f32
    qs: np.ndarray       # [nq][dim] f32
    true_idx: np.ndarray
    decoy_idx: np.ndarray


# ------------------------------------------------------------------------------- placement
def _place(placement, n, k, rng, reserved=()):
    """row numbers of (true rows, decoys)"""
    assert placement in PLACEMENTS and n % 128 == 0 and n >= 4 * PREFIX
    free = np.setdiff1d(np.arange(n), np.asarray(reserved, np.int64))
    if placement == "crowded":
        at = rng.permutation(free)[:k + 600]
        return np.sort(at[:k]), np.sort(at[k:])
    ndec = 2 * k if placement == "sparse" else 4 * k
    dec = np.sort(rng.permutation(free[free < PREFIX])[:ndec])
    behind = free[free >= n - 128] if placement == "sparse" else free[free >= PREFIX]
    return np.sort(rng.permutation(behind)[:k]), dec


def _distinct(base, count, ndims, amount):
    """`count` copies of `base`, copy r lowered by (r // ndims + 1) * amount in dimension r % ndims: no two alike"""
    out = np.tile(base, (count, 1))
    r = np.arange(count)
    out[r, r % ndims] -= (r // ndims + 1) * amount
    return out


# ------------------------------------------------------------------------------- int8
PIN_ROWS = (2000, 2001)  # behind the prefix, outside the last tile


def _i8_unit_rows(vals, count, dim):
    """cosine: `vals` (dim - 1 values) on a unit vector whose last dimension absorbs what unit norm still needs"""
    v = _distinct(vals, count, dim - 1, STEP * 2.0 ** -12)
    rest = 1.0 - (v * v).sum(1)
    assert np.all(rest > 0.01)
    return np.concatenate([v, np.sqrt(rest)[:, None]], axis=1)


@functools.lru_cache(maxsize=2)
def int8_case(metric, dim, placement, nq, k=10, n=N_ROWS, seed=7):
    """dot / l2: band values -1 + (code -+ 0.49) STEP with codes 190 .. 230 (l2: 220, so that q_d > v_d everywhere); positive
    queries uniform in [0.8, 1): the rounding error of every dimension has the same sign for every query of the batch.
    cos: the same on unit vectors (codes 138 .. 146 over dim - 1 dimensions, the last one free), every row times a scale of its own;
    the pins are +-e_0, so the normalised rows span [-1, 1]."""
    rng = np.random.default_rng(seed + 1000 * dim + {"dot": 0, "cos": 1, "l2": 2}[metric])
    cos = metric == "cos"
    nd = dim - 1 if cos else dim
    lo, hi = (138, 146) if cos else (190, 220 if metric == "l2" else 230)
    b = rng.integers(lo, hi + 1, size=nd).astype(np.float64)
    s = np.zeros(nd)
    s[rng.permutation(nd)[:int(round((0.95 if cos else 0.92) * nd))]] = 1.0
    true_at, decoy_at = _place(placement, n, k, rng, PIN_ROWS)
    assert (max(len(decoy_at), k) // nd + 1) * 2.0 ** -12 < 0.008  # the decoys stay inside their cells (0.01 of a step of room)
    dec_vals = -1.0 + (b - 0.49) * STEP        # rounds UP to b
    tru_vals = -1.0 + (b - s + 0.49) * STEP    # rounds DOWN to b - s
    rows = rng.uniform(-1.0, 0.3, size=(n, dim))
    if cos:
        scale = lambda m, ph: (1.0 + 0.37 * np.sin(ph + np.arange(m)))[:, None]  # noqa: E731  (no power of two: cosine != dot order)
        rows[decoy_at] = _i8_unit_rows(dec_vals, len(decoy_at), dim) * scale(len(decoy_at), 0.3)
        rows[true_at] = _i8_unit_rows(tru_vals, k, dim) * scale(k, 1.1)
        rows[PIN_ROWS[0]] = 0.0
        rows[PIN_ROWS[1]] = 0.0
        rows[PIN_ROWS[0], 0] = 1.0
        rows[PIN_ROWS[1], 0] = -1.0
    else:
        rows[decoy_at] = _distinct(dec_vals, len(decoy_at), dim, STEP * 2.0 ** -12)
        rows[true_at] = _distinct(tru_vals, k, dim, STEP * 2.0 ** -12)
        rows[PIN_ROWS[0]] = -1.0
        rows[PIN_ROWS[1]] = -1.0
        rows[PIN_ROWS[1], dim // 2] = 1.0
    qs = rng.uniform(0.8, 1.0, size=(nq, dim)).astype(np.float32)
    rows = rows.astype(np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return Case("i8", metric, k, rows, qs, true_at, decoy_at)


# ------------------------------------------------------------------------------- bf16
def _up_type(e, i):
    """2^e (1 + i 2^-7 + 2^-8 (1 + 2^-6)): rounds up by almost half a last place for every i in 0 .. 127"""
    return 2.0 ** e * (1.0 + i * 2.0 ** -7 + 2.0 ** -8 * (1.0 + 2.0 ** -6))


def _dn_type(e, i):
    return 2.0 ** e * (1.0 + i * 2.0 ** -7 + 2.0 ** -8 * (1.0 - 2.0 ** -6))


def _tuned_i(e, short, qd):
    """the largest i for which replacing 2^e UP by _up_type(e - 1, i) under the query value qd lowers the score by `short` or more,
    with room for the levels below it"""
    for i in range(127, 8, -1):
        if qd * (2.0 ** e * UP - _up_type(e - 1, i)) >= short:
            return i
    raise AssertionError("one dimension cannot make up the difference")


@functools.lru_cache(maxsize=2)
def bf16_case(metric, dim, placement, nq, k=10, n=N_ROWS, seed=11):
    """dot: the query is DN on the first half of the dimensions and UP on the second; true rows are DN on the first half (both
    operands round down), decoys UP-type on the second (both round up). True row r has r values one bf16 step up (_dn_type(0, 1)):
    distinct scores. Decoy j has one value replaced by _up_type(-1, i), i = i0 - j // (dim / 2), in dimension j % (dim / 2) of its
    half, i0 the largest i that leaves its exact score short of the true rows' by 10 accumulation allowances (_tuned_i): a small,
    tuned amount -- steps of 2^-8, not of whole dimensions. Query j of the batch is the base query times 2^(j - nq / 2).
    cos (dim 128): the same on unit vectors. The adversarial values are 2^-3 DN resp. 2^-3 UP (rows, 62 dimensions of their half)
    and 2^-3 / 2^-4 times DN resp. UP (query; 2^-7 in the one dimension where the true rows differ from each other, so that their
    scores are distinct and still close); the one dimension that absorbs what unit norm still needs lies, for the rows, where the
    query is zero and, for the query, where every band row is zero, so it moves no score. Every row times a scale of its own."""
    rng = np.random.default_rng(seed + dim)
    h = dim // 2
    true_at, decoy_at = _place(placement, n, k, rng)
    rows = rng.uniform(-0.5, 0.5, size=(n, dim))
    assert k <= 16 and len(decoy_at) // h < 100
    if metric == "dot":
        q = np.concatenate([np.full(h, DN), np.full(dim - h, UP)])
        tru = np.zeros((k, dim))
        tru[:, :h] = DN
        for r in range(k):
            tru[r, :r] = _dn_type(0, 1)
        dec = np.zeros((len(decoy_at), dim))
        dec[:, h:] = UP
        j = np.arange(len(decoy_at))
        i0 = _tuned_i(0, (UP * UP - DN * DN) * h + 10.0 * (dim + 2) * 2.0 ** -24 * DN * DN * h, UP)
        dec[j, h + j % (dim - h)] = _up_type(-1, i0 - j // (dim - h))
        qs = np.stack([q * 2.0 ** (i - nq // 2) for i in range(nq)])
    else:
        assert metric == "cos" and dim == 128
        na = h - 2                          # adversarial dimensions of a half: 0 .. 61 and 64 .. 125
        q = np.zeros(dim)
        big = rng.permutation(na)[:21]      # 21 at 2^-3 and 41 at 2^-4 in each half: the squares sum to 0.984
        w = np.full(na, 2.0 ** -4)
        w[big] = 2.0 ** -3
        mark = int(np.setdiff1d(np.arange(na), big)[0])
        w[mark] = 2.0 ** -7                 # ... and one nearly silent: where the true rows differ from each other
        q[:na] = w * DN
        q[h:h + na] = w * UP
        q[na] = np.sqrt(1.0 - (q * q).sum())            # the query's free dimension (62): zero in every band row
        tru = np.zeros((k, dim))
        tru[:, :na] = 2.0 ** -3 * DN
        tru[:, mark] = _dn_type(-3, np.arange(k))           # distinct scores, 2^-10 2^-7 apart
        tru[:, h - 1] = np.sqrt(1.0 - (tru * tru).sum(1))  # the true rows' free dimension (63): zero in the query
        dec = np.zeros((len(decoy_at), dim))
        dec[:, h:h + na] = 2.0 ** -3 * UP
        j = np.arange(len(decoy_at))
        qv = 2.0 ** -3 * float(w.sum())      # sum of q_d v_d over a half, before DN^2 resp. UP^2
        i0 = _tuned_i(-3, (UP * UP - DN * DN) * qv + 10.0 * (dim + 2) * 2.0 ** -24 * DN * DN * qv, 2.0 ** -3 * UP)
        dec[j, h + big[j % 21]] = _up_type(-4, i0 - (j // 21) % 4)  # (rows alike up to their scale tie exactly: harmless among decoys)
        dec[:, dim - 1] = np.sqrt(1.0 - (dec * dec).sum(1))  # the decoys' free dimension (127): zero in the query
        tru *= (1.0 + 0.37 * np.sin(1.1 + np.arange(k)))[:, None]
        dec *= (1.0 + 0.37 * np.sin(0.3 + j))[:, None]
        rows *= 0.5
        qs = np.stack([q * 2.0 ** (i - nq // 2) for i in range(nq)])
    rows[true_at] = tru
    rows[decoy_at] = dec
    rows, qs = rows.astype(np.float32), qs.astype(np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return Case("bf16", metric, k, rows, qs, true_at, decoy_at)


def make(engine, metric, dim, placement, nq, k=10, n=N_ROWS):
    return (int8_case if engine == "i8" else bf16_case)(metric, dim, placement, nq, k, n)


# ------------------------------------------------------------------------------- float64 emulations
def rne_bf16(x):
    """round-to-nearest-even f32 -> bf16 on the bit patterns (finite inputs), returned as f32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _unit32(x):
    """rows of x over their norms, rounded to f32 as the device holds them (it normalises in f32: ~1e-7 relative either way)"""
    x = x.astype(np.float64)
    return (x / np.sqrt((x * x).sum(1))[:, None]).astype(np.float32)


class Scores(NamedTuple):
    exact: np.ndarray    # [nq][n] float64, in the metric's score space (larger is better; l2: 2 q.v - |v|^2)
    approx: np.ndarray   # [nq][n] float64: the filter's approximate score in the same space
    lead: np.ndarray     # [nq]: the bound's leading term
    allow: np.ndarray    # [nq]: the reference's own accumulation allowance (D + 2) 2^-24 sum|q_d v_d| at the band rows, same space


def scores(case):
    rows, qs = case.rows.astype(np.float64), case.qs.astype(np.float64)
    dim = rows.shape[1]
    band = np.concatenate([case.true_idx, case.decoy_idx])
    u = (dim + 2) * 2.0 ** -24
    qn, vn = np.sqrt((qs * qs).sum(1)), np.sqrt((rows * rows).sum(1))
    absdot = (np.abs(qs) @ np.abs(rows[band]).T)
    if case.metric == "cos":
        qe, ve = _unit32(case.qs), _unit32(case.rows)  # what both filters round: the normalised values
        exact = (qs @ rows.T) / (qn[:, None] * vn[None, :])
        allow = u * (absdot / (qn[:, None] * vn[band][None, :])).max(1)
    else:
        qe, ve = case.qs, case.rows
        exact = qs @ rows.T
        allow = u * absdot.max(1)
        if case.metric == "l2":
            exact = 2.0 * exact - (vn * vn)[None, :]
            d2 = (qn * qn)[:, None] - exact[:, band]   # the reference sums (q_d - v_d)^2 directly
            allow = u * d2.max(1)
    if case.engine == "i8":
        mn, mx = np.float32(ve.min()), np.float32(ve.max())
        alpha, offset = np.float32(mx - mn), mn
        codes = oracle.quantize_u8(ve, oracle.QParams(float(alpha), float(offset)))
        deq = float(offset) + float(alpha) * codes.astype(np.float64) / 255.0
        approx = qe.astype(np.float64) @ deq.T
        lead = float(alpha) / 510.0 * np.abs(qe.astype(np.float64)).sum(1)
        if case.metric == "l2":  # the quantised values meet 2 q; |v|^2 travels beside them (two 8-bit limbs, exact to nmax / 130050)
            approx = 2.0 * approx - (vn * vn)[None, :]
            lead = 2.0 * lead
    else:
        approx = rne_bf16(qe).astype(np.float64) @ rne_bf16(ve).astype(np.float64).T
        lead = 2.0 ** -7 * (np.ones(len(qs)) if case.metric == "cos" else qn * vn.max())
    return Scores(exact, approx, lead, allow)


class Figures(NamedTuple):
    gap: float        # min over queries of (worst true row's exact score - best decoy's) / the accumulation allowance
    gap_lead: float   # ... the same gap over the leading term
    use: float        # min over queries and band rows of |approx - exact| / leading term
    dlead: float      # min over queries of (worst decoy's approx - best true row's approx) / (2 leading terms)
    kept_full: bool   # the model filter (keep if approx >= k-th best approx - 2 E) with E = the leading term keeps every true row ...
    lost_short: bool  # ... and with E = `short` times it drops every true row, for every query


def figures(case, sc, short):
    t, d = case.true_idx, case.decoy_idx
    band = np.concatenate([t, d])
    gap = sc.exact[:, t].min(1) - sc.exact[:, d].max(1)
    use = (np.abs(sc.approx[:, band] - sc.exact[:, band]) / sc.lead[:, None]).min()
    dlead = (sc.approx[:, d].min(1) - sc.approx[:, t].max(1)) / (2.0 * sc.lead)
    kth = np.sort(sc.approx, axis=1)[:, -case.k]
    kept = lambda f: sc.approx[:, t] >= (kth - 2.0 * f * sc.lead)[:, None]  # noqa: E731
    return Figures(float((gap / sc.allow).min()), float((gap / sc.lead).min()), float(use), float(dlead.min()),
                   bool(kept(1.0).all()), bool(not kept(short).any()))


# ------------------------------------------------------------------------------- the corpora the GPU tests run
def _corpora():
    out = []
    for placement in PLACEMENTS:
        out += [("i8", "dot", dim, placement, 40, 10, N_ROWS) for dim in (64, 100, 768)]
        out += [("i8", metric, 64, placement, 40, 10, N_ROWS) for metric in ("cos", "l2")]
    out += [("i8", "dot", 64, placement, 1, 10, N_ROWS) for placement in ("crowded", "seeded")]
    out += [("i8", "dot", 64, "crowded", 300, 10, N_ROWS), ("i8", "dot", 64, "crowded", 40, 100, N_ROWS),
            ("i8", "dot", 64, "crowded", 40, 10, 2 * N_ROWS)]  # (INNR_KNN_AUTO takes a filter from 65536 rows on)
    for placement in ("crowded", "sparse"):
        out += [("bf16", "dot", 768, placement, 40, 10, N_ROWS), ("bf16", "dot", 128, placement, 40, 10, N_ROWS),
                ("bf16", "cos", 128, placement, 40, 10, N_ROWS)]
    return out


CORPORA = _corpora()
# condition 2 of the data: share of the leading term the band rows use, and the decoys' approximate lead over the true rows as a
# share of twice it; condition 3: the factor on the leading term at which the model filter must lose every true row
NEEDS = {"i8": dict(use=0.90, dlead=0.85, short=0.8), "bf16": dict(use=0.60, dlead=0.58, short=0.5)}


def case_id(args):
    return "-".join(str(a) for a in args)
