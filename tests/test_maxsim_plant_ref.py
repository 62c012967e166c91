"""The planted maxsim corpora (tests/maxsim_plant_ref.py) are what they claim to be: the float64 conditions hold, every slot, query
token, index class and neighbour length the GPU tests rely on occurs, and a plant that a kernel does not see costs its document the
top-k -- so tests/test_gpu_maxsim_strides.py can fail. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import maxsim_plant_ref as R

NWAVES = 64
SHAPES = [  # ndocs, T, dim, tqs, P, seed: one query over two tiles of tokens; four queries of one call, a one-token query among them
    (700, 40, 64, [12], 24, 1),
    (1100, 33, 32, [8, 3, 4, 1], 24, 1),
]


@pytest.fixture(scope="module", params=[(s, c) for s in SHAPES for c in (False, True)], ids=lambda p: f"{p[0][1]}x{p[0][2]}-{'cos' if p[1] else 'dot'}")
def corpus(request):
    (ndocs, T, dim, tqs, P, seed), cosine = request.param
    queries, tokens, lens, pl = R.build(ndocs, T, dim, tqs, P, NWAVES, cosine, seed)
    tokens.setflags(write=False)
    return (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl


def test_same_arguments_same_corpus(corpus):
    (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl = corpus
    q2, t2, l2, p2 = R.build(ndocs, T, dim, tqs, P, NWAVES, cosine, seed)
    assert all(np.array_equal(a, b) for a, b in zip(queries, q2)) and np.array_equal(tokens.view(np.uint32), t2.view(np.uint32))
    assert np.array_equal(lens, l2) and all(np.array_equal(a, b) for a, b in zip(pl.docs, p2.docs))


def test_the_conditions_recomputed(corpus):
    """not the builder's own bookkeeping: every document scored again in float64 from the corpus as returned"""
    (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl = corpus
    assert pl.KP == R.pick_kp(P, 16) == 64
    hosts = np.concatenate(pl.docs)
    assert len(set(hosts.tolist())) == len(tqs) * P and np.all(lens[hosts] >= 1)
    bare = tokens.copy()
    for qi in range(len(tqs)):
        for h, slot in zip(pl.docs[qi], pl.slots[qi]):
            bare[h, slot] = 0.0
    for qi, q in enumerate(queries):
        sc = R.scores64(q, tokens, lens, cosine)
        mine = np.zeros(ndocs, bool)
        mine[pl.docs[qi]] = True
        gap = sc[mine].min() - sc[~mine].max()
        assert gap >= R.GAP and abs(gap - pl.min_gap[qi]) < 1e-9, (qi, gap, pl.min_gap[qi])
        # a plant a kernel does not see (here: zeroed): the document falls out of the top 2 KP, the re-score of KP cannot bring it back
        without = R.scores64(q, bare, lens, cosine, pl.docs[qi])
        for h, w in zip(pl.docs[qi], without):
            rank = int((np.delete(sc, h) > w).sum())
            assert rank >= 2 * pl.KP, (qi, h, rank)
        assert pl.worst_rank[qi] >= 2 * pl.KP
        # the token seen but not the planted query token (a pass that drops token j): the other query tokens do not keep it in either
        for h, j in zip(pl.docs[qi], pl.qtoks[qi]):
            rest = np.delete(q, j, axis=0)
            w = R.scores64(rest, tokens, lens, cosine, [h])[0] if len(rest) else 0.0
            rank = int((np.delete(sc, h) > w).sum())
            assert rank >= 2 * pl.KP, (qi, h, j, rank)
        assert pl.blind_rank[qi] >= 2 * pl.KP
        gram = q.astype(np.float64) @ q.astype(np.float64).T
        assert np.abs(gram - np.eye(len(q))).max() < 1e-6  # unit query tokens, no cross-talk between them


def test_plants_are_where_the_record_says(corpus):
    (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl = corpus
    for qi, q in enumerate(queries):
        for h, slot, j, ln in zip(pl.docs[qi], pl.slots[qi], pl.qtoks[qi], pl.lens[qi]):
            assert ln == lens[h] and 0 <= slot < ln
            t = tokens[h, slot].astype(np.float64)
            cos = float(t @ q[j].astype(np.float64)) / np.sqrt(float(t @ t) * float(q[j].astype(np.float64) @ q[j].astype(np.float64)))
            assert cos > 1.0 - 1e-6, (qi, h, slot, j, cos)
            if not cosine:
                assert np.array_equal(tokens[h, slot], q[j])


def test_coverage(corpus):
    (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl = corpus
    assert pl.slots_required == R.slot_cycle(T) and {0, 3, 4, 7, 8, 28, 31, 32, T - 1} <= set(pl.slots_required)
    assert set(pl.slots_required) <= {s for sl in pl.slots for s in sl}
    for qi, tq in enumerate(tqs):
        want = {j for j in (0, 1, 15, 16, tq - 2, tq - 1) if 0 <= j < tq}
        assert want == set(pl.qtoks_required[qi]) <= set(pl.qtoks[qi]), (qi, pl.qtoks[qi])
    for name, (lo, hi) in R.index_classes(ndocs, NWAVES).items():
        assert pl.classes.get(name), name
        assert all(lo <= h < hi for _, h in pl.classes[name])
    assert [h for _, h in pl.classes["first"]] == [0] and [h for _, h in pl.classes["last"]] == [ndocs - 1]
    assert {0, 1, 32, min(33, T), T} <= set(pl.pred_len) and 0 in pl.succ_len
    for L, hosts in pl.pred_len.items():
        assert all(lens[h - NWAVES] == L for _, h in hosts)
    assert all(lens[h + NWAVES] == 0 for _, h in pl.succ_len[0])
    host_lens = [ln for ls in pl.lens for ln in ls]
    assert 1 in host_lens and min(33, T) in host_lens
    assert any(slot == ln - 1 < T - 1 for sl, ls in zip(pl.slots, pl.lens) for slot, ln in zip(sl, ls))
    frac_full = float((lens == T).mean())
    assert 0.2 < frac_full < 0.45 and lens.min() == 0 and lens.max() == T


def test_query_token_cycle_of_a_long_query():
    assert R.qtok_cycle(70) == [0, 1, 15, 16, 68, 69, 31, 32, 33] and R.qtok_cycle(1) == [0] and R.qtok_cycle(5) == [0, 1, 3, 4]
    assert R.slot_cycle(40) == [0, 3, 4, 7, 8, 28, 31, 32, 35, 39] and R.slot_cycle(33) == [0, 3, 4, 7, 8, 28, 31, 32]


def test_expected_topk_orders_ties_by_index(corpus):
    (ndocs, T, dim, tqs, P, seed), cosine, queries, tokens, lens, pl = corpus
    for qi, q in enumerate(queries):
        docs, sc = R.expected_topk(q, tokens, lens, pl.docs[qi], cosine)
        assert sorted(docs.tolist()) == sorted(pl.docs[qi].tolist()) and sc.dtype == np.float32
        keys = list(zip((-sc.astype(np.float64)).tolist(), docs.tolist()))
        assert keys == sorted(keys)
        if tqs[qi] == 1 and not cosine:  # one query token, planted everywhere: exact ties, on purpose
            assert len(set(sc.tolist())) == 1 and docs.tolist() == sorted(docs.tolist())


@pytest.mark.parametrize("cosine", [False, True])
def test_ladder(cosine):
    L = 100
    q, tokens, lens, rungs = R.ladder(cosine=cosine, seed=5)
    assert tokens.shape == (600, 40, 64) and q.shape == (12, 64) and len(set(rungs.tolist())) == L and np.all(lens[rungs] >= 1)
    sc = R.scores64(q, tokens, lens, cosine)
    on = np.zeros(600, bool)
    on[rungs] = True
    assert sc[on].min() - sc[~on].max() >= R.GAP          # the rungs are the top L ...
    spread = sc[on].max() - sc[on].min()
    # ... one copy of a document apart from the rung's token: 99 roundings of the planted pair end to end (dot); a turn of at most
    # 99 * 2^-11 rad, felt to first order by the other eleven query tokens only (cosine)
    assert 0.0 < spread < (0.1 if cosine else 1e-4), spread
    steps = np.diff(np.sort(sc[on]))
    assert np.median(steps) < (2e-3 if cosine else 1e-6), np.median(steps)
    assert L > R.pick_kp(10, 16)                          # more rungs than candidates: the approximate order decides who is re-scored
