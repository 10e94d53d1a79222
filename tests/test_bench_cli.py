"""bench.py's launcher logic (no GPU): `--gpus N` without a torch.distributed.run environment must start N ranks itself
BEFORE anything touches a GPU, relay the child's exit code, and refuse a world size that contradicts `--gpus`."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_gpus_n_spawns_torch_distributed_run(monkeypatch):
    import bench
    for k in ("RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return R()
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setitem(sys.modules, "torch", None)          # importing torch in the launcher process would be a bug
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert e.value.code == 7                                   # the child's exit code is relayed
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_must_match_gpus(monkeypatch):
    import bench
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "2"); monkeypatch.setenv("MASTER_PORT", "29999")
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "8"])
    assert e.value.code == 2


def test_default_workload_per_world_size():
    import bench
    a = bench.parse_args([])
    assert a.gpus == 1 and a.steps == 20 and a.warmup == 5 and a.batch == 4096 and a.mode is None
    # mode None -> independent seeds (configs[2]) at N = 1, shared theta + all-reduce (configs[3]) at N > 1: see bench.main
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'args.mode or ("shared" if world > 1 else "independent")' in src


def test_config_selects_the_baseline_workload():
    """`--config` picks BASELINE configs[1] / configs[4] with their own batch, grid and arithmetic; explicit flags still win."""
    import bench
    a = bench.parse_args(["--config", "robotarm"])
    assert (a.batch, a.n_grid, a.dtype) == (1024, 50, "f32") and bench.WORKLOADS["robotarm"]["method"] == "Vanilla"
    r = bench.parse_args(["--config", "rocket"])
    assert (r.batch, r.n_grid, r.dtype) == (1024, 100, "f32") and bench.WORKLOADS["rocket"]["aux_dtype"] == "f64"
    assert bench.parse_args(["--config", "rocket", "--batch", "64", "--n-grid", "15"]).batch == 64
    q = bench.parse_args([])
    assert (q.config, q.batch, q.n_grid, q.dtype, q.no_f64_leg) == ("quadrotor", 4096, 50, "f32", False)
    with pytest.raises(SystemExit):
        bench.parse_args(["--config", "pendulum"])


def test_full_and_dump_outputs_are_opt_in():
    """A plain run times the headline only; `--full` adds the roofline, fp64, CPU-baseline and oracle-parity legs."""
    import bench
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    b = bench.parse_args(["--full", "--dump-outputs", "out", "--steps", "7"])
    assert b.full is True and b.dump_outputs == "out" and b.steps == 7


def test_dump_outputs_keeps_precision_and_samples_the_same_rows_over_the_limit(tmp_path):
    import numpy as np
    import torch
    import bench
    B = 1000
    idx = np.arange(B, dtype=np.float64)
    arrays = dict(loss=idx.astype(np.float32), grad=torch.tensor(np.tile(idx[:, None], (1, 7))),
                  state_grid=np.tile(idx[:, None, None], (1, 51, 13)).astype(np.float32), iters=np.arange(B, dtype=np.int32))
    shapes = bench.dump_outputs(str(tmp_path / "all"), arrays)
    assert shapes == {"loss": [B], "grad": [B, 7], "state_grid": [B, 51, 13], "iters": [B]}
    got = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in shapes}
    assert got["loss"].dtype == np.float32 and got["grad"].dtype == np.float64 and got["iters"].dtype == np.float64
    assert np.array_equal(got["state_grid"][:, 3, 5], idx) and np.array_equal(got["grad"][:, 0], idx)
    # over the limit: one seeded sample of rows for every array, within the limit, the same from call to call
    limit = 200_000
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    s1 = {k: np.load(str(tmp_path / "s1" / (k + ".npy"))) for k in shapes}
    s2 = {k: np.load(str(tmp_path / "s2" / (k + ".npy"))) for k in shapes}
    assert sum(a.nbytes for a in s1.values()) <= limit and 0 < len(s1["loss"]) < B
    rows = s1["loss"].astype(np.float64)
    assert np.all(np.diff(rows) > 0)
    assert np.array_equal(s1["grad"][:, 6], rows) and np.array_equal(s1["state_grid"][:, 50, 12], rows) and np.array_equal(s1["iters"], rows)
    assert all(np.array_equal(s1[k], s2[k]) for k in shapes)


def test_a_window_longer_than_the_examples_run_starts_the_run_again():
    """Warmup + steps beyond the example's outer-iteration count (WORKLOADS `outer_iters`) restart the learner from its initial
    parameters with a fresh optimizer state and cold-started solves, i.e. as a new learner on the same seeds."""
    import types
    import numpy as np
    import torch
    import bench
    assert [bench.WORKLOADS[c]["outer_iters"] for c in ("quadrotor", "robotarm", "rocket")] == [50, 100, 1000]

    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

        def elapsed_time(self, other):
            return 1.0

    class Learner:
        def __init__(self):
            self.theta = torch.tensor([[0.5, -1.0]])
            self.m, self.v, self.vhat = (torch.zeros(1, 2) for _ in range(3))
            self.iter_idx, self.event_hook, self._sol, self.seen = 0, None, None, []

        def step(self):
            self.seen.append((self.iter_idx, float(self.theta[0, 0]), float(self.m[0, 0]), self._sol is None))
            for name in ("oc_solve", "aux_riccati", "aux_forward", "update", "end"):
                if self.event_hook:
                    self.event_hook(name)
            self.theta += 1.0
            self.m += 2.0
            self.iter_idx += 1
            self._sol = {}
            return torch.tensor([float(self.iter_idx)]), self.theta.clone()

    fake_torch = types.SimpleNamespace(cuda=types.SimpleNamespace(Event=Event))
    L = Learner()
    last = {}
    bench.timed_steps(L, 7, 5, lambda: None, fake_torch, last, run=(4, L.theta.clone()))
    assert [s[0] for s in L.seen] == [0, 1, 2, 3] * 3
    assert all(th == 0.5 + it and m == 2.0 * it and (sol_none == (it == 0)) for it, th, m, sol_none in L.seen)
    assert float(last["loss"][0]) == 4.0 and np.allclose(last["grad"].numpy(), [[4.5, 3.0]])
    L = Learner()
    bench.timed_steps(L, 7, 5, lambda: None, fake_torch)
    assert [s[0] for s in L.seen] == list(range(12))
