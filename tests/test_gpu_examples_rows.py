"""examples/knn_graph.py (the k-NN graph of a resident corpus, near-duplicates through rows() + batch_range_search) runs end to end."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_graph_example_runs(capsys):
    spec = importlib.util.spec_from_file_location("knn_graph", os.path.join(ROOT, "examples", "knn_graph.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(corpus_size=3000, dim=32, k=5, planted=6, probes=64)
    out = capsys.readouterr().out
    assert "planted pairs that are each other's nearest neighbour: 6 / 6" in out
    assert "every planted near-duplicate found, nothing else" in out
