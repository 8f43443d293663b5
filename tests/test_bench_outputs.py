"""bench.py's plain run and --dump-outputs: the budgeted, seeded dump of the tallies (no GPU), and on the GPU
a plain run of the C3 model at 20,000 packets per wavelength, twice in this process: the line holds the
headline fields and the steps asked for, leaves out what --full adds, and the two dumps agree element for
element (the same packets on the same Philox streams; only the order of the f64 atomic adds differs, 1e-9 as
in the same-stream parity tests)."""
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402

LIMIT = 64 * 1000 * 1000


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def test_dump_keeps_small_arrays_whole_and_samples_large_ones(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8000)
    big = np.arange(5000, dtype=np.float64)
    small = np.arange(7, dtype=np.float64) * 0.5
    bench.dump_outputs(str(tmp_path), {"big": big, "small": small})
    assert np.array_equal(np.load(tmp_path / "small.npy"), small)
    got = np.load(tmp_path / "big.npy")
    assert got.dtype == np.float64 and 0 < got.size < big.size
    # the sample is a fixed function of the array's size: sorted, without repeats, the same on every call
    idx = bench.dump_sample(big.size, got.size)
    assert np.array_equal(got, big[idx]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, bench.dump_sample(big.size, got.size))
    assert _dir_bytes(str(tmp_path)) <= 8000


def test_dump_budget_is_below_64_mb_with_every_array_oversized(tmp_path):
    assert bench.DUMP_BUDGET_BYTES < LIMIT
    n = bench.DUMP_BUDGET_BYTES // 8  # each of the three alone would fill the budget
    arrays = {k: np.zeros(n) for k in ("a", "b", "c")}
    bench.dump_outputs(str(tmp_path), arrays)
    assert _dir_bytes(str(tmp_path)) <= bench.DUMP_BUDGET_BYTES
    assert all(np.load(tmp_path / (k + ".npy")).size > n // 4 for k in arrays)


def _plain_run(monkeypatch, capsys, outdir):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                                      "--packets-per-lambda", "20000", "--dump-outputs", outdir])
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: pytest.fail("a plain run ran the CPU baseline"))
    bench.main()
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path, monkeypatch, capsys):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain_run(monkeypatch, capsys, a)
    _plain_run(monkeypatch, capsys, b)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and "cpu_baseline" not in line
    # two timed steps of 25 wavelengths x 20,000 packages
    assert line["config"]["packages_per_step"] == 25 * 20000
    assert line["value"] == pytest.approx(2 * 25 * 20000 / (2 * line["ms_per_step"] / 1e3), rel=1e-9)
    assert sorted(os.listdir(a)) == ["instruments.npy", "labs.npy"]
    assert _dir_bytes(a) <= LIMIT
    for name in os.listdir(a):
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        assert x.dtype == np.float64 and x.shape == y.shape and np.isfinite(x).all()
        assert x.sum() > 0
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=0)
