"""Corpora for the maxsim tests in which ONE (document token slot, query token) pair decides whether a document belongs in the
answer (numpy + the CPU oracle only; no GPU code is imported here).

On i.i.d. tokens a structural miss of the approximate stage -- a query token dropped, a token row left out of the max, the last
valid token of a short document masked -- lowers every document by about the same amount: the candidate set barely moves, the exact
re-score repairs the scores and the answer is right all the same. Here the background is QUIET: every background token has the
component it had inside the span of the call's query tokens shrunk to 3 %, so an unplanted document scores around 0.1, and each
PLANTED document carries exactly one query token j in exactly one slot t, which alone is worth 1.0. A kernel that does not see
(t, j) loses that document from the top-k, and the hosts are drawn from documents that are far from the candidate cut without
their plant, so the exact re-score cannot bring it back.

build() places the hosts where a strided document loop can go wrong: document 0, the first stride [1, nwaves), the second
[nwaves, 2 nwaves), the ragged last stride, the last document; behind predecessors (h - nwaves) of length 0, 1, 32, 33 and T and in
front of a successor (h + nwaves) of length 0; in hosts of length 1 and 33 and with the plant in the last valid slot of a short
document. It asserts, in float64, that every planted document beats every other one by at least GAP and that no host would reach the
top 2 KP without its plant -- neither with the planted token gone nor with the token there and its query token not counted
(KP = the candidate count of the engine under test for k = P). The query tokens of a call are orthonormal, so that the second
holds: the planted pair is all a planted token contributes."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import oracle

GAP = 0.2
SLOTS = (0, 3, 4, 7, 8, 28, 31, 32, 35)  # and T - 1; clamped to the host's last valid slot
SHRINK = 0.97


def pick_kp(k, margin):
    """api.hip pick_kp: candidates kept for k results"""
    kp = 32
    while kp < k + margin:
        kp <<= 1
    return kp


def _dedupe(seq):
    out = []
    for x in seq:
        if x not in out:
            out.append(x)
    return out


def slot_cycle(T):
    return _dedupe([min(s, T - 1) for s in SLOTS + (T - 1,)])


def qtok_cycle(tq):
    want = [0, 1, 15, 16, tq - 2, tq - 1] + ([31, 32, 33] if tq > 32 else [])
    return _dedupe([j for j in want if 0 <= j < tq])


def _query_tokens(rng, tqs, dim):
    """random unit vectors, the call's tokens orthogonal to one another (a random orthonormal frame, split into the queries). With merely
    independent tokens a planted q_j also scores q_i . q_j ~ dim^-1/2 against each of the OTHER query tokens, in sum several times an
    unplanted document's whole score: a kernel that drops query token j would still keep the document among its candidates on that
    cross-talk, a one-token host (score: the signed sum of q_i . q_j) could fall below the background, and the planted documents of
    one query of a group would stand high in the lists of the others."""
    frame, _ = np.linalg.qr(rng.standard_normal((dim, sum(tqs))))
    rows = frame.T.astype(np.float32)
    cuts = np.cumsum([0] + list(tqs))
    return [np.ascontiguousarray(rows[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def _pair_scores(t64, q64, cosine):
    """[..., T, dim] x [m, dim] -> [..., T, m] token-pair scores in float64 (cosine: 0 for a zero-norm token, dense.rs:341-345)"""
    s = t64 @ q64.T
    if cosine:
        tn = np.sqrt((t64 * t64).sum(axis=-1))
        qn = np.sqrt((q64 * q64).sum(axis=-1))
        den = tn[..., None] * qn
        s = np.where(den > 0.0, s / np.where(den > 0.0, den, 1.0), 0.0)
    return s


def scores64(query, tokens, doc_len, cosine, docs=None):
    """float64 maxsim of one query against the documents `docs` (default: all) of tokens[ndocs, T, dim]"""
    q64 = np.asarray(query, np.float64)
    docs = np.arange(len(tokens)) if docs is None else np.asarray(docs, np.int64)
    out = np.zeros(len(docs))
    T, dim = tokens.shape[1:]
    step = max(1, (1 << 22) // max(T * max(dim, len(q64)), 1))
    for c0 in range(0, len(docs), step):
        d = docs[c0:c0 + step]
        s = _pair_scores(tokens[d].astype(np.float64), q64, cosine)
        live = np.arange(T)[None, :] < np.asarray(doc_len)[d][:, None]
        s = np.where(live[:, :, None], s, -np.inf).max(axis=1)
        out[c0:c0 + step] = np.where(live.any(axis=1), s.sum(axis=1), 0.0)
    return out


class _Background:
    """quiet tokens, random lengths, and for every document its float64 score at its own length and at the lengths build() may force"""

    def __init__(self, ndocs, T, dim, queries, cosine, seed, rng):
        self.ndocs, self.T, self.dim, self.cosine = ndocs, T, dim, cosine
        self.bounds = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
        qall = np.concatenate(queries).astype(np.float64)
        assert len(qall) <= dim // 2, "the query tokens of one call must leave half the space to the background"
        basis, _ = np.linalg.qr(qall.T)  # [dim, m] orthonormal basis of the span of every query token of the call
        self.lens = rng.integers(0, T + 1, ndocs).astype(np.uint32)
        self.lens[rng.random(ndocs) < 0.3] = T
        mrng = np.random.default_rng([seed, 1])  # a stream of its own: the dot and the cosine corpus of one seed share hosts and lengths
        self.mags = np.exp(mrng.uniform(np.log(0.25), np.log(4.0), (ndocs, T))).astype(np.float32) if cosine else None
        self.tokens = oracle.generate_uniform(ndocs * T, dim, seed).reshape(ndocs, T, dim)
        self.opts = sorted({1, min(32, T), min(33, T), T})
        nq = len(queries)
        self.tab = {L: np.zeros((nq, ndocs)) for L in self.opts}  # score at the forced length L
        self.cur = np.zeros((nq, ndocs))                          # score at the current length
        step = max(1, (1 << 22) // (T * dim))
        for c0 in range(0, ndocs, step):
            r = self.tokens[c0:c0 + step].astype(np.float64)
            r /= np.sqrt((r * r).sum(axis=-1, keepdims=True))
            r -= SHRINK * ((r @ basis) @ basis.T)
            r /= np.sqrt((r * r).sum(axis=-1, keepdims=True))
            t32 = r.astype(np.float32)
            if cosine:
                t32 *= self.mags[c0:c0 + step, :, None]
            self.tokens[c0:c0 + step] = t32
            cm = np.maximum.accumulate(_pair_scores(t32.astype(np.float64), qall, cosine), axis=1)  # prefix max over token slots
            ln = self.lens[c0:c0 + step].astype(np.int64)
            own = np.take_along_axis(cm, np.maximum(ln - 1, 0)[:, None, None], axis=1)[:, 0, :]
            for qi in range(nq):
                a, b = self.bounds[qi], self.bounds[qi + 1]
                for L in self.opts:
                    self.tab[L][qi, c0:c0 + step] = cm[:, L - 1, a:b].sum(axis=1)
                self.cur[qi, c0:c0 + step] = np.where(ln > 0, own[:, a:b].sum(axis=1), 0.0)

    def force_len(self, d, L):
        L = min(L, self.T)
        self.lens[d] = L
        self.cur[:, d] = self.tab[L][:, d] if L else 0.0

    def swap(self, d, e):
        if d == e:
            return
        for a in [self.tokens, self.lens, self.mags] + list(self.tab.values()):
            if a is None:
                continue
            if a.shape[0] == self.ndocs:
                a[[d, e]] = a[[e, d]]
            else:
                a[:, [d, e]] = a[:, [e, d]]
        self.cur[:, [d, e]] = self.cur[:, [e, d]]

    def plant(self, d, slot, token, scale=1.0):
        t = np.asarray(token, np.float64) * scale
        if self.cosine:
            t = t * np.float64(self.mags[d, slot])
        self.tokens[d, slot] = t.astype(np.float32)


@dataclass
class Planted:
    KP: int
    docs: list = field(default_factory=list)        # per query: planted documents, in planting order
    slots: list = field(default_factory=list)       # per query: the slot each carries its plant in
    qtoks: list = field(default_factory=list)       # per query: the query token planted there
    lens: list = field(default_factory=list)        # per query: the hosts' lengths
    classes: dict = field(default_factory=dict)     # index class -> [(query, host)]
    pred_len: dict = field(default_factory=dict)    # length of the predecessor h - nwaves -> [(query, host)]
    succ_len: dict = field(default_factory=dict)    # length of the successor h + nwaves -> [(query, host)]
    min_gap: list = field(default_factory=list)     # per query: min planted score - max other score (float64); asserted >= GAP
    worst_rank: list = field(default_factory=list)  # per query: best rank of a host WITHOUT its plant; asserted >= 2 KP
    blind_rank: list = field(default_factory=list)  # per query: best rank of a host scored WITHOUT the planted query token; >= 2 KP
    slots_required: list = field(default_factory=list)
    qtoks_required: list = field(default_factory=list)


def index_classes(ndocs, nwaves):
    """name -> [lo, hi) of the document index classes of a loop that strides by nwaves"""
    last0 = ((ndocs - 1) // nwaves) * nwaves
    return {"first": (0, 1), "stride0": (1, min(nwaves, ndocs)), "stride1": (nwaves, min(2 * nwaves, ndocs)),
            "last_stride": (last0, ndocs), "last": (ndocs - 1, ndocs)}


def build(ndocs, T, dim, tqs, P, nwaves, cosine, seed):
    """-> queries (list of [tq, dim] f32), tokens [ndocs, T, dim] f32, doc_len [ndocs] u32, Planted. Deterministic in its arguments."""
    rng = np.random.default_rng(seed)
    nq = len(tqs)
    KP = pick_kp(P, 16)
    assert ndocs > nwaves and ndocs >= 4 * KP + 4 * nq * P and sum(tqs) <= dim // 2
    queries = _query_tokens(rng, tqs, dim)
    bg = _Background(ndocs, T, dim, queries, cosine, seed, rng)
    thr = [np.sort(bg.cur[qi])[::-1][4 * KP - 1] for qi in range(nq)]  # below it: ranks below 4 KP among all documents
    used = np.zeros(ndocs, bool)
    classes = index_classes(ndocs, nwaves)
    pl = Planted(KP=KP, slots_required=slot_cycle(T), qtoks_required=[qtok_cycle(tq) for tq in tqs])
    SL = pl.slots_required

    def eligible(qi, lo, hi, min_len, max_len=None, at=None):
        d = np.arange(lo, hi)
        sc = bg.cur[qi, lo:hi] if at is None else bg.tab[at][qi, lo:hi]
        ok = ~used[lo:hi] & (sc < thr[qi])
        if at is None:
            ok &= (bg.lens[lo:hi] >= min_len) & (bg.lens[lo:hi] <= (T if max_len is None else max_len))
        return d[ok]

    def draw(qi, lo, hi, min_len, **kw):
        c = eligible(qi, lo, hi, min_len, **kw)
        assert len(c), ("no quiet host left", qi, lo, hi, min_len, kw)
        return int(c[rng.integers(len(c))])

    def neighbour_free(c, off):
        return np.array([h for h in c if 0 <= h + off < ndocs and not used[h + off]], np.int64)

    # the hosts with a condition of their own, dealt to the queries in turn; each is (kind, slot index n it takes)
    specials = ["first", "last", "last_stride", "pred0", "pred1", "pred32", "pred33", "predT", "succ0", "len1", "len33", "lenm1"]
    want_n = {"len1": SL.index(0), "len33": SL.index(min(32, T - 1)), "lenm1": SL.index(T - 1)}
    plan = [dict() for _ in range(nq)]  # n -> kind
    for s, kind in enumerate(specials):
        qi = s % nq
        n = want_n.get(kind)
        if n is None or n in plan[qi]:
            n = next(i for i in range(1, P) if i not in plan[qi] and i not in want_n.values())
        plan[qi][n] = kind
    for qi in range(nq):
        docs, slots, qtoks = [], [], []
        QT = pl.qtoks_required[qi]
        regular = 0
        for n in range(P):
            slot, j = SL[n % len(SL)], QT[(n + n // len(SL)) % len(QT)]
            kind = plan[qi].get(n)
            if kind in ("first", "last", "last_stride"):  # a fixed place: it takes the content of a quiet full-length document
                lo, hi = classes[kind]
                if kind == "last_stride" and hi - lo > 1:
                    hi -= 1
                spot = [d for d in range(lo, hi) if not used[d]]
                assert spot, kind
                h = spot[0]
                used[h] = True  # (not its own donor unless it qualifies)
                c = eligible(qi, 1, ndocs, T)
                used[h] = False
                e = h if (bg.lens[h] == T and bg.cur[qi, h] < thr[qi]) else int(c[rng.integers(len(c))])
                bg.swap(h, e)
            elif kind in ("pred0", "pred1", "pred32", "pred33", "predT"):
                L = {"pred0": 0, "pred1": 1, "pred32": 32, "pred33": 33, "predT": T}[kind]
                c = neighbour_free(eligible(qi, *classes["stride1"], T), -nwaves)
                assert len(c), kind
                h = int(c[rng.integers(len(c))])
                bg.force_len(h - nwaves, L)
                used[h - nwaves] = True
            elif kind == "succ0":
                c = neighbour_free(eligible(qi, 0, ndocs - nwaves, T), nwaves)
                assert len(c), kind
                h = int(c[rng.integers(len(c))])
                bg.force_len(h + nwaves, 0)
                used[h + nwaves] = True
            elif kind == "len1":
                h = draw(qi, 0, ndocs, 0, at=1)
                bg.force_len(h, 1)
            elif kind == "len33":  # plant in slot 32, the first of a second 32-token tile
                h = draw(qi, 0, ndocs, 0, at=min(33, T))
                bg.force_len(h, 33)
                slot = 32
            elif kind == "lenm1":  # a short document with its plant in its last valid slot
                h = draw(qi, 0, ndocs, 2, max_len=T - 1)
                slot = T - 1
            else:
                lo, hi = (classes["stride0"], classes["stride1"], (0, ndocs))[min(regular, 2)]
                regular += 1
                c = eligible(qi, lo, hi, slot + 1)
                if not len(c):
                    c = eligible(qi, 0, ndocs, slot + 1)
                if not len(c):
                    c = eligible(qi, 0, ndocs, 1)
                assert len(c), "no quiet host left"
                h = int(c[rng.integers(len(c))])
            used[h] = True
            docs.append(h)
            slots.append(min(slot, int(bg.lens[h]) - 1))
            qtoks.append(j)
        pl.docs.append(np.array(docs, np.int64))
        pl.slots.append(slots)
        pl.qtoks.append(qtoks)
    # the unplanted scores of the corpus as it now stands, then the plants
    unplanted = bg.cur.copy()
    for qi in range(nq):
        for h, slot, j in zip(pl.docs[qi], pl.slots[qi], pl.qtoks[qi]):
            bg.plant(h, slot, queries[qi][j])
    tokens, lens = bg.tokens, bg.lens
    final = unplanted.copy()
    hosts = np.concatenate(pl.docs)
    for qi in range(nq):
        final[qi, hosts] = scores64(queries[qi], tokens, lens, cosine, hosts)
    for qi in range(nq):
        mine = np.zeros(ndocs, bool)
        mine[pl.docs[qi]] = True
        pl.min_gap.append(float(final[qi, mine].min() - final[qi, ~mine].max()))
        ranks = [int((final[qi] > unplanted[qi, h]).sum() - (final[qi, h] > unplanted[qi, h])) for h in pl.docs[qi]]
        pl.worst_rank.append(min(ranks))
        blind = []  # the host as a kernel scores it that sees the token but not query token j: every other query token's term
        for h, j in zip(pl.docs[qi], pl.qtoks[qi]):
            b = scores64(np.delete(queries[qi], j, axis=0), tokens, lens, cosine, [h])[0] if tqs[qi] > 1 else 0.0
            blind.append(int((final[qi] > b).sum() - (final[qi, h] > b)))
        pl.blind_rank.append(min(blind))
        pl.lens.append([int(lens[h]) for h in pl.docs[qi]])
        for name, (lo, hi) in classes.items():
            pl.classes.setdefault(name, []).extend((qi, int(h)) for h in pl.docs[qi] if lo <= h < hi)
        for h in pl.docs[qi]:
            if h >= nwaves:
                pl.pred_len.setdefault(int(lens[h - nwaves]), []).append((qi, int(h)))
            if h + nwaves < ndocs:
                pl.succ_len.setdefault(int(lens[h + nwaves]), []).append((qi, int(h)))
    check(pl)
    return queries, tokens, lens, pl


def check(pl):
    """the conditions every test on a planted corpus rests on: the planted documents lead; a plant not seen -- the token slot, or the
    query token alone -- leaves its host outside the candidates"""
    assert min(pl.min_gap) >= GAP, f"a planted document leads the rest by only {min(pl.min_gap)}"
    assert min(pl.worst_rank) >= 2 * pl.KP, f"a host ranks {min(pl.worst_rank)} without its plant: the re-score of {pl.KP} could rescue it"
    assert min(pl.blind_rank) >= 2 * pl.KP, f"a host ranks {min(pl.blind_rank)} on the other query tokens alone"


def expected_topk(query, tokens, doc_len, planted, cosine):
    """the planted documents of this query (their indices) ordered by oracle score descending, ties to the lower index; -> (docs, scores f32).
    That they ARE the top-k is the float64 gap build() asserted: the oracle runs on them alone."""
    docs = np.sort(np.asarray(planted, np.int64))
    sc = np.array([oracle.maxsim(query, tokens[d, :doc_len[d]], cosine=cosine) for d in docs], np.float32)
    order = np.argsort(-sc.astype(np.float64), kind="stable")
    return docs[order], sc[order]


def ladder(ndocs=600, T=40, dim=64, tq=12, L=100, cosine=False, seed=0):
    """-> query [tq, dim], tokens, doc_len, rungs (L document indices). The rungs are L copies of one document; rung i (in shuffled
    order) carries query token 0 in slot 0, scaled by 1 + i 2^-23 (dot) or turned to unit(q0 + i 2^-11 v), v orthogonal to q0 (cosine):
    neighbouring rungs' exact scores differ by amounts around or below the error bound of the matrix pipe's sum -- under dot many are
    equal --, and there are more rungs than the engine keeps candidates."""
    rng = np.random.default_rng(seed)
    query = _query_tokens(rng, [tq], dim)[0]
    bg = _Background(ndocs, T, dim, [query], cosine, seed, rng)
    rungs = np.sort(rng.choice(ndocs, L, replace=False))
    q0 = query[0].astype(np.float64)
    v = rng.standard_normal(dim)
    v -= (v @ q0) / (q0 @ q0) * q0
    v /= np.sqrt(v @ v)
    order = rng.permutation(L)  # the rung's height is not its index order
    bg.lens[rungs[0]] = max(int(bg.lens[rungs[0]]), 1)
    for i, d in zip(order, rungs):
        bg.tokens[d], bg.lens[d] = bg.tokens[rungs[0]], bg.lens[rungs[0]]  # one document L times over: only the rung's token differs
        if cosine:
            bg.mags[d] = bg.mags[rungs[0]]
        if cosine:
            t = q0 + float(i) * 2.0 ** -11 * v
            bg.plant(d, 0, t / np.sqrt(t @ t))
        else:
            bg.plant(d, 0, q0, 1.0 + float(i) * 2.0 ** -23)
    return query, bg.tokens, bg.lens, rungs
