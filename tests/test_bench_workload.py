"""What `bench.py --gpus N` runs (no GPU needed): N = 1 is BASELINE configs[2]; N >= 2 is the north star's workload
(strong scaling on 4800x1600 at Re 200) whenever a rank's share fits its HBM, otherwise weak scaling."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_workloads_per_gpu_count():
    B = _bench()
    assert B.choose_workload(1) == ("weak", 1200, 400, 100.0)
    assert B.choose_workload(2) == ("weak", 2400, 400, 100.0)          # 327 GB per rank: the strong case does not fit
    assert B.choose_workload(4) == ("strong", 4800, 1600, 200.0)       # 164 GB per rank
    assert B.choose_workload(8) == ("strong", 4800, 1600, 200.0)       # 82 GB per rank
    # a rank's share of the strong-scaling case: below 0.8 x 288 GB and below 2^31 non-zeros in block (0,0)
    for n in (4, 8):
        assert B.BYTES_PER_DOF * B.N_DOFS_NORTH_STAR / n <= 0.8 * B.HBM_BYTES
        assert 428_350_320 * 16 / n < 2 ** 31


def test_explicit_arguments_win():
    B = _bench()
    assert B.choose_workload(8, "weak") == ("weak", 9600, 400, 100.0)
    assert B.choose_workload(2, "strong") == ("strong", 4800, 1600, 200.0)
    assert B.choose_workload(4, "auto", "600,200", 50.0) == ("weak", 2400, 200, 50.0)
    assert B.choose_workload(4, "strong", "600,200") == ("strong", 600, 200, 100.0)


class _FakeSolver:
    """What dump_outputs reads of a LinearSolver after the timed steps."""
    def __init__(self, n_u, n_p):
        import numpy as np
        self.xu, self.xp = np.linspace(0.0, 1.0, n_u), -np.linspace(0.0, 1.0, n_p)

    def download_solution(self):
        return self.xu.copy(), self.xp.copy()

    def history(self):
        return [1.0, 0.5, 0.25]


def test_dump_outputs_small_and_sampled(tmp_path):
    import numpy as np
    B = _bench()
    B.dump_outputs(_FakeSolver(30, 7), 0.25, str(tmp_path / "small"), 0, 1)
    d = tmp_path / "small"
    assert sorted(p.name for p in d.iterdir()) == ["final_residual.npy", "residual_history.npy", "solution_p.npy",
                                                   "solution_u.npy"]
    assert np.array_equal(np.load(d / "solution_u.npy"), np.linspace(0.0, 1.0, 30))
    assert np.load(d / "final_residual.npy").tolist() == [0.25]
    # above the budget: a fixed sample, the same from run to run, within 64 MB in all
    n_u, n_p = B.DUMP_VALUES, B.DUMP_VALUES // 3
    runs = []
    for k in range(2):
        out = tmp_path / f"big{k}"
        B.dump_outputs(_FakeSolver(n_u, n_p), 1.0, str(out), 0, 1)
        arrs = {p.name: np.load(p) for p in out.iterdir()}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 2 ** 20
        assert arrs["solution_u.npy"].size + arrs["solution_p.npy"].size <= B.DUMP_VALUES
        assert np.all(np.diff(arrs["solution_u.npy"]) > 0)      # sorted distinct indices of an increasing vector
        runs.append(arrs)
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])
