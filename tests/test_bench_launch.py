"""bench.py --gpus N: the N-rank launch the driver's scaling run relies on.

``python bench.py --gpus 2`` with no launcher around it must start two ranks
itself (one child torch.distributed.run, before any GPU call), and the JSON
line must report the world size it actually ran at.  Exercised on CPU with
gloo through ``--dist-selftest`` (same launch, barrier and max-over-ranks
path as the GPU run)."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dist-selftest", "--steps", "3",
                          "--warmup", "1", *extra], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_spawns_two_ranks():
    line = _run("--gpus", "2")
    assert line["n_gpus"] == 2 and line["steps"] == 3


def test_bench_single_rank_default():
    line = _run()
    assert line["n_gpus"] == 1


def test_dump_outputs_writes_float_npy_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs: one <name>.npy per array, float64 kept and everything
    else as float32; an array over its share of the budget is written as the
    same sorted sample of its elements in every run."""
    import numpy as np
    import torch

    import bench

    arrays = {"a": torch.arange(12, dtype=torch.int64).view(3, 4), "b": torch.linspace(0, 1, 5, dtype=torch.float64),
              "c": torch.arange(1000, dtype=torch.float32), "d": torch.tensor([0, 1], dtype=torch.uint8)}
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 400)  # 400 bytes per array: only "c" is over
    for run in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    out = {n: np.load(tmp_path / "r1" / f"{n}.npy") for n in arrays}
    assert sorted(p.name for p in (tmp_path / "r1").iterdir()) == ["a.npy", "b.npy", "c.npy", "d.npy"]
    assert out["a"].dtype == np.float32 and out["a"].shape == (3, 4) and out["a"][2, 3] == 11
    assert out["b"].dtype == np.float64 and np.array_equal(out["b"], arrays["b"].numpy())
    assert out["d"].dtype == np.float32
    c = out["c"]
    assert c.dtype == np.float32 and c.shape == (100,) and np.all(np.diff(c) > 0) and set(c) <= set(range(1000))
    assert np.array_equal(c, np.load(tmp_path / "r2" / "c.npy"))
    assert sum(a.nbytes for a in out.values()) <= 4 * 400


def test_plain_run_leaves_the_side_measurements_to_full(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    import bench

    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "x"


def test_bench_reads_the_roofline_pmc_summary():
    """bench.py's roofline.traffic comes from the newest profiles/rN_pmc_traffic.json
    (not another kernel's rN_*_pmc_traffic.json)."""
    import bench

    pmc = bench.load_pmc_traffic()
    assert pmc is not None and "gae_bytes" in pmc and "loss_bytes" in pmc, pmc
