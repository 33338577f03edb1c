"""`python bench.py --gpus N` must produce an N-rank line or fail: the self-launch, on CPU.

No GPU work: `--launch-check` makes every rank join the process group, all_reduce 2**rank and rank 0 print what it saw."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _run(argv, env_extra=None, drop=("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + argv, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)


def _json(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus_2_without_a_launcher_starts_two_ranks():
    p = _run(["--gpus", "2", "--backend", "gloo", "--launch-check"])
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    d = _json(p.stdout)
    assert d == {"launch_check": True, "n_gpus": 2, "ranks_seen": 2, "backend": "gloo"}


def test_gpus_3_without_a_launcher_starts_three_ranks():
    d = _json(_run(["--gpus", "3", "--backend", "gloo", "--launch-check"]).stdout)
    assert d["n_gpus"] == 3 and d["ranks_seen"] == 3


def test_rccl_with_fewer_devices_than_ranks_is_an_error_not_a_smaller_run():
    import torch

    have = torch.cuda.device_count()
    p = _run(["--gpus", str(have + 1 if have else 2), "--launch-check"])            # backend nccl (the default)
    assert p.returncode == 2 and "visible GPUs" in p.stderr and not p.stdout.strip()


def test_a_launcher_with_another_world_size_is_an_error():
    p = _run(["--gpus", "4", "--backend", "gloo", "--launch-check"], env_extra={"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert p.returncode == 2 and "WORLD_SIZE=1" in p.stderr


def test_single_gpu_workloads_refuse_n_ranks():
    p = _run(["--gpus", "2", "--backend", "gloo", "--workload", "warp"])
    assert p.returncode == 2 and "single-GPU" in p.stderr


def test_dump_outputs_refuses_workloads_without_a_dump():
    p = _run(["--workload", "cli", "--dump-outputs", "unused"])
    assert p.returncode == 2 and "--dump-outputs" in p.stderr and not p.stdout.strip()


def test_dump_outputs_writes_float32_or_float64_within_the_limit(tmp_path):
    """bench.dump_outputs / frame_outputs in a child process (importing bench.py sets process-wide defaults)."""
    code = f"""
import numpy as np, types, bench
r = types.SimpleNamespace(xyxy=np.ones((3, 4), np.float32), conf=np.ones(3, np.float32), cls=np.array([0, 2, 1], np.int32),
                          ids=np.array([5, 6, 7], np.int64), xywh_stab=None, H=None, gmc=np.eye(2, 3))
out = bench.frame_outputs([r])
bench.dump_outputs({str(tmp_path / "d")!r}, dict(out, big=np.zeros(10, np.float64)))
try:
    bench.dump_outputs({str(tmp_path / "e")!r}, {{"x": np.zeros((bench.DUMP_LIMIT_BYTES // 4) + 1, np.int32)}})
except ValueError:
    print("refused")
"""
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and p.stdout.strip() == "refused", p.stdout + p.stderr
    import numpy as np

    got = {f.stem: np.load(f) for f in (tmp_path / "d").glob("*.npy")}
    assert set(got) == {"frame0_xyxy", "frame0_conf", "frame0_cls", "frame0_ids", "frame0_xywh_stab", "frame0_H", "frame0_gmc", "big"}
    assert got["frame0_cls"].dtype == np.float32 and got["frame0_cls"].tolist() == [0, 2, 1] and got["frame0_ids"].tolist() == [5, 6, 7]
    assert got["frame0_H"].dtype == np.float64 and np.isnan(got["frame0_H"]).all() and got["frame0_xywh_stab"].shape == (0, 4)
    assert got["frame0_gmc"].dtype == np.float64 and got["big"].dtype == np.float64
    assert not (tmp_path / "e").exists()


def test_gpus_1_launches_nothing():
    d = _json(_run(["--gpus", "1", "--launch-check"]).stdout)
    assert d["n_gpus"] == 1 and d["ranks_seen"] == 1
