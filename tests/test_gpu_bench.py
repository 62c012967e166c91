"""bench.py on the GPU at a small size, in this process: a plain run prints the headline line and nothing that --full adds, and
--full adds the side rows (bf16 / int8 filter engines, each bit-equal to the f32 engine, and the LCG-data row) without changing
what the timed steps return. The CPU baseline is left out here (--no-cpu-baseline): it builds the oracle in a child process,
which must not start from a process that has initialised the GPU."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = ["--n-per-gpu", "20000", "--dim", "128", "--queries", "64", "--k", "10", "--steps", "2", "--warmup", "1"]
FULL_ONLY = ("bf16_filter_engine", "int8_filter_engine", "lcg_side_row", "cpu_baseline")


def _bench(monkeypatch, capsys, *extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *SHAPE, *extra])
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.lstrip().startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _dumped(d):
    return {n: np.load(d / f"{n}.npy") for n in ("indices", "scores")}


def test_bench_plain_and_full(monkeypatch, capsys, tmp_path):
    plain = _bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "plain"))
    assert plain["unit"] == "vectors/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert plain["value"] == pytest.approx(64 * 20000 / (plain["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [key for key in FULL_ONLY if key in plain]

    full = _bench(monkeypatch, capsys, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert "cpu_baseline" not in full
    for key in ("bf16_filter_engine", "int8_filter_engine"):
        assert full[key]["identical_to_f32_engine"] is True, full[key]
    assert full["lcg_side_row"]["steps"] == 2 and full["lcg_side_row"]["ms_per_step"] > 0

    a, b = _dumped(tmp_path / "plain"), _dumped(tmp_path / "full")
    assert a["indices"].shape == (64, 10)
    assert np.array_equal(a["indices"], b["indices"]) and np.array_equal(a["scores"].view(np.uint32), b["scores"].view(np.uint32))
