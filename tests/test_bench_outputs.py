"""bench.py's plain run and its outputs: a run without --full does set-up, warm-up, the timed steps and nothing else, `--steps`
sets the number of timed steps, and --dump-outputs writes what those steps computed (residual history, a fixed sample of x)
as float32 / float64 .npy files of at most 64 MB, the same from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_options_default_to_the_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse(["--gpus", "2", "--dump-outputs", "out"])


class _FakeSolver:
    """stands in for pkg.Solver: counts iterations, x and the history are functions of them; the extras of --full fail"""

    def __init__(self, n, dtype):
        self.n, self.dtype, self.calls, self.done = n, np.dtype(dtype), [], 0

    def set_rhs(self, b, x0, on_device=False):
        self.done = 0

    def iterate(self, k):
        self.calls.append(k)
        self.done += k

    def x(self):
        return (np.arange(self.n) * (self.done + 1.5)).astype(self.dtype)

    def history(self):
        return (1.0 / (1.0 + np.arange(self.done + 1, dtype=np.float64))).astype(self.dtype).reshape(-1, 1)

    def iterate_timed(self, k):
        raise AssertionError("a plain run must not run the instrumented pass")

    def spmv(self, *a, **k):
        raise AssertionError("a plain run must not time the SpMV on its own")

    def close(self):
        pass


def _fake_env(n, dtype):
    solvers = []

    def make_solver(ctx, n_, nnz, data, indptr, indices, nrhs, flags=0, dtype=None):
        solvers.append(_FakeSolver(n_, dtype))
        return solvers[-1]

    cols = types.SimpleNamespace(numel=lambda: 7 * n)
    pkg = types.SimpleNamespace(
        _lib=types.SimpleNamespace(MATRIX_ON_DEVICE=1, NO_GRAPH=2, UNFUSED=4),
        generators=types.SimpleNamespace(laplace3d=lambda ctx, nx, ny, nz, dtype=None: (None, cols, None),
                                         torch_dtype=lambda dt: dt),
        Solver=make_solver)
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=lambda: None),
                                  full=lambda shape, v, dtype=None, device=None: np.full(shape, v, dtype=dtype))
    ctx = types.SimpleNamespace(synchronize=lambda: None)
    return pkg, torch, ctx, solvers


@pytest.mark.parametrize("dtype", ["f64", "c64"])
def test_plain_run_times_exactly_the_requested_steps(tmp_path, dtype):
    nx, ny, nz = 16, 12, 10
    n = nx * ny * nz
    pkg, torch, ctx, solvers = _fake_env(n, bench.NP_DTYPE[dtype])
    args = bench.parse(["--steps", "13", "--warmup", "3", "--dtype", dtype, "--dump-outputs", str(tmp_path)])
    res = bench.bench_single(args, pkg, ctx, torch, "cpu", nx, ny, nz, bench.NP_DTYPE[dtype])
    assert solvers[0].calls == [3, 13]                       # warm-up, then the timed steps; nothing after them
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res
    assert res["steps"] == 13 and res["dtype"] == dtype and res["higher_is_better"] is True
    assert res["ms_per_step"] > 0 and abs(res["value"] * res["ms_per_step"] - 1e3) < 1e-6 * res["value"]
    assert res["residual_check"]["iterations"] == 16
    assert not {"roofline", "values_as_passed", "small_system", "cpu_baseline"} & set(res)
    # what the caller of the timed path receives: x after 16 iterations (all of it, n < the sample size) and the history
    h = np.load(tmp_path / "history.npy")
    x = np.load(tmp_path / "x_sample.npy")
    idx = np.load(tmp_path / "x_sample_index.npy")
    want_x = solvers[0].x()
    want_h = solvers[0].history()
    if np.dtype(bench.NP_DTYPE[dtype]).kind == "c":
        assert h.dtype == x.dtype == np.float32 and x.shape == (n, 2) and h.shape == (17, 1, 2)
        want_x = np.stack([want_x.real, want_x.imag], -1)
        want_h = np.stack([want_h.real, want_h.imag], -1)
    else:
        assert h.dtype == x.dtype == np.float64 and x.shape == (n,) and h.shape == (17, 1)
    assert np.array_equal(idx, np.arange(n, dtype=np.float64))
    assert np.array_equal(x, want_x) and np.array_equal(h, want_h)


def test_dump_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    n = 3 * bench.DUMP_X_SAMPLE + 17
    x = np.random.default_rng(1).standard_normal(n)
    hist = np.arange(1001, dtype=np.float64).reshape(-1, 1)
    names = bench.dump_outputs(str(tmp_path / "a"), x, hist)
    bench.dump_outputs(str(tmp_path / "b"), x, hist)
    assert names == ["history", "x_sample", "x_sample_index"]
    got = {d: {f: np.load(tmp_path / d / (f + ".npy")) for f in names} for d in ("a", "b")}
    for f in names:
        assert np.array_equal(got["a"][f], got["b"][f])          # same entries every run
        assert got["a"][f].dtype in (np.float32, np.float64)
    idx = got["a"]["x_sample_index"]
    assert idx.size == bench.DUMP_X_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(got["a"]["x_sample"], x[idx.astype(np.int64)])
    assert np.array_equal(got["a"]["history"], hist)
    assert sum(os.path.getsize(tmp_path / "a" / (f + ".npy")) for f in names) <= 64 << 20
    # a history longer than the budget leaves room for keeps its LAST rows
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 8 * bench.DUMP_X_SAMPLE + 8 * 100)
    bench.dump_outputs(str(tmp_path / "c"), x, hist)
    assert np.array_equal(np.load(tmp_path / "c" / "history.npy"), hist[-100:])


def _bench(out_dir, *extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "5",
                        "--grid", "40x36x32", "--dump-outputs", str(out_dir)] + list(extra),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    return json.loads(lines[0]), {f: np.load(os.path.join(out_dir, f + ".npy")) for f in ("history", "x_sample", "x_sample_index")}


@pytest.mark.gpu
def test_bench_dumps_the_solution_of_its_timed_steps(tmp_path):
    """two plain runs on a small grid: the line holds the headline fields only, the outputs are the same bits both times
    and are the CG iterates of the system (against the CPU oracle)"""
    import cg_numpy
    import cg_oracle
    line, out = _bench(tmp_path / "a")
    _, again = _bench(tmp_path / "b")
    assert line["steps"] == 30 and line["ms_per_step"] > 0 and line["unit"] == "CG iterations/s"
    assert not {"roofline", "values_as_passed", "small_system", "cpu_baseline"} & set(line)
    for f in out:
        assert np.array_equal(out[f], again[f]), f
    ip, ix, da = cg_numpy.laplace3d(40, 36, 32)
    n = 40 * 36 * 32
    xo, ho = cg_oracle.cg(ip, ix, da, np.full(n, 5.0), n_iterations=35, mode=cg_oracle.MODE_FAST)
    assert out["history"].shape == (36, 1) and out["x_sample"].shape == (n,)
    assert np.max(np.abs(out["history"] - ho) / np.abs(ho)) < 1e-10
    assert np.linalg.norm(out["x_sample"] - xo[out["x_sample_index"].astype(np.int64)]) / np.linalg.norm(xo) < 1e-9
