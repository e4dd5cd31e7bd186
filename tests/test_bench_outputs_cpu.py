"""bench.py's --dump-outputs writer and --full switch (CPU): what a plain run writes after its timed steps, in which dtype and layout, and
that a point set beyond the 64 MB budget is thinned to the same seeded sample every time."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _summary_and_trace(n_iter):
    from sfm_toy_library_amd.structs import SfmbaIteration, SfmbaSummary
    s = SfmbaSummary()
    s.iterations, s.successful_steps, s.residual_evals, s.jacobian_evals = n_iter, n_iter, n_iter + 1, n_iter + 1
    s.initial_cost, s.final_cost, s.seconds = 10.0, 1.5, 0.25
    trace = []
    for i in range(n_iter + 1):
        it = SfmbaIteration()
        it.iteration, it.cost, it.trust_region_radius = i, 10.0 / (i + 1), 1e4 * 10 ** i
        trace.append(it.as_dict())
    return s.as_dict(), trace


def test_dump_outputs_writes_float64_arrays(tmp_path):
    b = _bench_module()
    rng = np.random.default_rng(3)
    cam6, pt3 = rng.normal(size=(7, 6)), rng.normal(size=(50, 3))
    summ, trace = _summary_and_trace(3)
    b.dump_outputs(str(tmp_path / "out"), cam6, pt3, 512.0, summ, trace)
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == ["cameras.npy", "focal.npy", "points.npy", "summary.npy", "trace.npy"]
    a = {n[:-4]: np.load(tmp_path / "out" / n) for n in names}
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["cameras"], cam6) and np.array_equal(a["points"], pt3) and a["focal"].tolist() == [512.0]
    s = dict(zip(b.SUMMARY_FIELDS, a["summary"].tolist()))
    assert s["iterations"] == 3 and s["final_cost"] == 1.5 and s["initial_cost"] == 10.0
    assert "seconds" not in b.SUMMARY_FIELDS                    # wall time differs from run to run: not an output
    assert a["trace"].shape == (4, 10) and a["trace"][:, 0].tolist() == [0, 1, 2, 3] and a["trace"][2, 4] == 10.0 / 3
    # a path without a trace (the sharded solve) writes none
    b.dump_outputs(str(tmp_path / "sh"), cam6, pt3, 512.0, summ)
    assert not os.path.exists(tmp_path / "sh" / "trace.npy") and os.path.exists(tmp_path / "sh" / "summary.npy")


def test_dump_outputs_thins_points_beyond_the_budget_to_a_fixed_sample(tmp_path, monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 3 << 20)
    pt3 = np.arange(3 * 200000, dtype=np.float64).reshape(-1, 3)
    summ, trace = _summary_and_trace(1)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), np.zeros((2, 6)), pt3, 1.0, summ, trace)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 3 << 20
    rows, pts = np.load(tmp_path / "a" / "point_rows.npy"), np.load(tmp_path / "a" / "points.npy")
    assert 0 < len(rows) < len(pt3) and np.all(np.diff(rows) > 0) and np.array_equal(pts, pt3[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "point_rows.npy"))


def test_full_is_off_by_default(monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "somewhere"
