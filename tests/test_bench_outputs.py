"""bench.py --dump-outputs and --full.  CPU: the dumped sample is fixed and within bounds, the files are float64 and within
64 MB, the option is refused where it has no meaning.  GPU: a plain run writes what the optimizer holds after its last
timed step (bit for bit what the binding gets with the same inputs and steps) and leaves out what --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_sample_index_is_fixed_sorted_and_in_bounds():
    assert np.array_equal(bench.dump_sample_index(1000), np.arange(1000))
    n = 10_000_000
    a, b = bench.dump_sample_index(n), bench.dump_sample_index(n)
    assert np.array_equal(a, b)
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) > 0)
    assert 0.9 * bench.DUMP_SAMPLE < a.size <= bench.DUMP_SAMPLE


class _Field:
    def __init__(self, v):
        self.v = v

    def to_host(self):
        return self.v.copy()


class _FakeOpt:
    def __init__(self, n):
        self.n = n
        for i, name in enumerate(bench.DUMP_FIELDS):
            setattr(self, name, _Field(np.arange(n, dtype=np.float64) + i * 0.5))
        self.current_objective_value, self.delta_objective_value, self.last_step_length, self.iteration_count = 1.5, -0.25, 0.5, 45


@pytest.mark.parametrize("n", [4099, 3_000_000])
def test_dump_outputs_writes_float64_within_64_mb(tmp_path, n):
    names = bench.dump_outputs(_FakeOpt(n), str(tmp_path / "out"))
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(x + ".npy" for x in names)
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 << 20
    idx = np.load(tmp_path / "out" / "sample_index.npy")
    for f in files:
        assert np.load(tmp_path / "out" / f).dtype == np.float64
    for i, name in enumerate(bench.DUMP_FIELDS):
        assert np.array_equal(np.load(tmp_path / "out" / (name + ".npy")), idx + i * 0.5)
    assert np.load(tmp_path / "out" / "iteration_count.npy").tolist() == [45.0]


def test_dump_outputs_is_refused_outside_the_lbfgs_line(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "adgd", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


def _bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    from dzo_loader import dzo
    n, m, steps, warm = 2_000_000, 20, 6, 2
    out = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warm), "--dim", str(n), "--dump-outputs", str(tmp_path)], 600)
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["value"] > 0
    for key in ("cpu_baseline", "sustained", "secondary"):
        assert key not in out
    assert out["roofline"] is None or "two_pass" not in out["roofline"]
    idx = np.load(tmp_path / "sample_index.npy").astype(np.int64)
    assert np.array_equal(idx, bench.dump_sample_index(n))
    dzo.init(0)
    opt = dzo.LBFGSOptimizer(None, dzo.Problem(dzo.ROSENBROCK_CHAIN, n), None,
                             dzo.DeviceArray.from_host(bench.rosenbrock_chain_x0(n, seed=5)), 1.0, m)
    for _ in range(m + warm + steps):
        opt.step()
    assert np.load(tmp_path / "iteration_count.npy").tolist() == [float(opt.iteration_count)] == [float(m + warm + steps)]
    assert np.load(tmp_path / "current_objective_value.npy")[0] == opt.current_objective_value == out["config"]["f_end"]
    for name in bench.DUMP_FIELDS:
        assert np.array_equal(np.load(tmp_path / (name + ".npy")), getattr(opt, name).to_host()[idx]), name
    opt.close()


@pytest.mark.gpu
def test_full_run_keeps_the_legs_a_plain_run_leaves_out():
    # (a size whose run does not end stuck within these steps: `sustained` continues only an optimizer that is not stuck)
    out = _bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--dim", "400000", "--full"], 600)
    assert out["steps"] == 5 and out["ms_per_step"] > 0
    assert out["cpu_baseline"]["value"] > 0
    assert "sustained" in out or out["config"]["any_stuck"]
    assert out["roofline"]["two_pass"]["steps"] >= 20
