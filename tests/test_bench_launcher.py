"""bench.py's N-rank launcher (CPU, gloo): `python bench.py --gpus N` without WORLD_SIZE starts
torch.distributed.run itself (the driver's scaling command form), and a WORLD_SIZE that
disagrees with --gpus fails loudly.  The dry run swaps the GPU decomposition for a stub, so
this covers the launch, the rank-0 JSON line and the gather over gloo -- not numbers."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    env["OMP_NUM_THREADS"] = "1"
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=240, env=env, cwd=ROOT)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def test_gpus2_launches_two_ranks():
    p = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1", "--batch", "3"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    d = lines[0]
    assert d["n_gpus"] == 2 and d["dry_run"] is True and d["gathered_matrices"] == 6
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["parallelism"] == "dp2 (matrix-sharded)"


def test_gpus1_runs_in_process():
    p = _run(["--gpus", "1", "--dry-run", "--steps", "1", "--warmup", "0"])
    assert p.returncode == 0, p.stderr[-3000:]
    (d,) = _json_lines(p.stdout)
    assert d["n_gpus"] == 1 and d["gathered_matrices"] == 4


def test_world_size_mismatch_fails_loudly():
    p = _run(["--gpus", "2", "--dry-run"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE=1 but --gpus 2" in p.stderr


def _npys(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_dump_outputs_dry_run_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy files,
    the same values from run to run."""
    import numpy as np
    dumps = []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        p = _run(["--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "1", "--batch", "3", "--dump-outputs", d])
        assert p.returncode == 0, p.stderr[-3000:]
        (line,) = _json_lines(p.stdout)
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        dumps.append(_npys(d))
    a, b = dumps
    assert set(a) == {"codes", "L", "R", "Q_scale", "global_scale", "errors_Q", "errors_LR"}
    assert a["codes"].shape == (3, 32 * 64 // 4) and a["L"].shape == (3, 32, 4) and a["R"].shape == (3, 4, 64)
    assert a["errors_Q"].shape == (3, 1) and a["Q_scale"].shape == (3,)
    assert a["codes"].max() > 1  # the stub's packed bytes, not zeros
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), (k, a[k].dtype)
        assert np.array_equal(a[k], b[k]), k


def test_dump_outputs_samples_large_tensors_at_fixed_positions(tmp_path, monkeypatch):
    """A tensor over its share of the budget is written as the entries at seeded flat positions
    (the same in every call, a function of its size alone); ragged lengths are concatenated."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 8 * 3 * 100)  # 2 names, 3 matrices: 100 entries each
    g = torch.Generator().manual_seed(1)
    big = [torch.randn(40, 50, generator=g) for _ in range(3)]
    rag = [torch.randn(7, generator=g, dtype=torch.float64), torch.randn(500, generator=g, dtype=torch.float64),
           torch.randn(7, generator=g, dtype=torch.float64)]
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), {"big": big, "rag": rag}, {"s": [1.0, 2.0, 3.0]})
    a, b = _npys(str(tmp_path / "a")), _npys(str(tmp_path / "b"))
    assert a["big"].shape == (3, 100) and a["big"].dtype == np.float32
    assert a["rag"].shape == (7 + 100 + 7,) and a["rag"].dtype == np.float64
    assert a["s"].tolist() == [1.0, 2.0, 3.0]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # every matrix of one size is sampled at the same positions, and they are entries of the tensor
    pos = [int(np.flatnonzero(big[0].reshape(-1).numpy() == v)[0]) for v in a["big"][0]]
    assert pos == sorted(pos) and len(set(pos)) == len(pos) == 100
    for i in (1, 2):
        assert np.array_equal(a["big"][i], big[i].reshape(-1).numpy()[pos])
    assert np.array_equal(a["rag"][:7], rag[0].numpy()) and np.array_equal(a["rag"][-7:], rag[2].numpy())
