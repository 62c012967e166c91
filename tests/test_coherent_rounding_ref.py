"""The coherently rounded corpora of coherent_ref.py have the power they are built for (numpy and the oracle only; the GPU tests
that run them are test_gpu_coherent_rounding.py). For every corpus of the GPU tests and every query:
  1. the oracle's top k is exactly the true rows, and the smallest exact gap between true rows and decoys is at least 8 x the
     reference's own accumulation allowance (D + 2) 2^-24 sum|q_d v_d|;
  2. the band rows use at least 0.90 (int8) / 0.60 (bf16) of the bound's leading term -- (alpha / 510) |q|_1 (squared L2: twice
     that), 2^-7 |q| max|v| (cosine: 2^-7) -- and the decoys lead the true rows approximately by at least 0.85 / 0.58 of twice it, in
     float64 emulations of the filters' scores (int8: quantize_u8 with the corpus' own range, dequantised values . q; bf16: RNE-rounded
     operands): a bound short by ~15 % (int8), or by the factor 2 of one forgotten operand (bf16), loses the true rows;
  3. a model filter (keep a row if approx >= k-th best approx - 2 E) keeps every true row with E = the leading term and drops every
     one of them with E = 0.8 x (int8) / 0.5 x (bf16) of it."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import coherent_ref as R

ORACLE_KNN = {"dot": oracle.batch_knn_dot, "cos": oracle.batch_knn_cosine, "l2": oracle.batch_knn}


@pytest.mark.parametrize("args", R.CORPORA, ids=R.case_id)
def test_coherent_corpus_conditions(args):
    case = R.make(*args)
    need = R.NEEDS[case.engine]
    data = oracle.from_rows(case.rows)
    for j, q in enumerate(case.qs):
        oi, _ = ORACLE_KNN[case.metric](q, data, case.k)
        assert sorted(int(i) for i in oi) == case.true_idx.tolist(), j
    f = R.figures(case, R.scores(case), need["short"])
    print(f"{R.case_id(args)}: exact gap {f.gap:.1f} x the accumulation allowance ({f.gap_lead:.4f} of the leading term); band rows use "
          f"{f.use:.4f} of the leading term; decoys lead by {f.dlead:.4f} of twice it; model filter keeps all true rows at 1.0 x: "
          f"{f.kept_full}, loses all at {need['short']} x: {f.lost_short}")
    assert f.gap >= 8.0
    assert f.use >= need["use"] and f.dlead >= need["dlead"]
    assert f.kept_full and f.lost_short


def test_bf16_boundary_values_round_as_built():
    dn, up = np.float32(R.DN), np.float32(R.UP)
    assert float(dn) == R.DN and float(up) == R.UP  # both are f32 values
    assert R.rne_bf16(dn) == np.float32(1.0) and R.rne_bf16(up) == np.float32(1.0 + 2.0 ** -7)
    for e in (0, -1, -4):
        for i in (0, 1, 69, 127):
            x, y = np.float32(R._up_type(e, i)), np.float32(R._dn_type(e, i))
            assert R.rne_bf16(x) > x and R.rne_bf16(y) < y
            assert R.rne_bf16(x) - x > np.float32(0.98 * 2.0 ** (e - 8)) and y - R.rne_bf16(y) > np.float32(0.98 * 2.0 ** (e - 8))
