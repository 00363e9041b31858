"""bench.py's multi-GPU launcher on CPU (--dry-run: gloo, stand-in workload).

`python bench.py --gpus N` outside torch.distributed.run starts N rank
processes itself; these tests run that path with N = 2 and check the JSON
line's n_gpus, that every rank took part in the reductions, that a failing
rank ends the job with its exit code instead of a hang, and that --gpus must
agree with a WORLD_SIZE set by torch.distributed.run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="1", **kw)
    return env


def _run(args, **env):
    return subprocess.run([sys.executable, BENCH, *args], env=_env(**env), capture_output=True, text=True,
                          timeout=180, cwd="/tmp")


def test_dry_run_two_ranks_prints_one_line_with_n_gpus():
    p = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["ranks_seen"] == 2
    assert d["steps"] == 2 and d["scaling"] == "weak"
    # whole-job rate: both ranks' steps over the slowest rank's time
    assert abs(d["value"] - 2 * d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3)) < 1e-3 * d["value"] + 1e-3


def test_dry_run_single_rank():
    p = _run(["--dry-run", "--steps", "1", "--warmup", "0"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs DIR: one float .npy per output after the timed steps,
    the same values from run to run (seeded inputs); a plain run and --full
    both accept it."""
    import numpy as np
    got = []
    for sub, extra in (("a", []), ("b", ["--full"])):
        p = _run(["--dry-run", "--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / sub), *extra])
        assert p.returncode == 0, p.stderr[-2000:]
        assert json.loads(p.stdout.strip().splitlines()[-1])["steps"] == 2
        assert sorted(os.listdir(tmp_path / sub)) == ["dry_step.npy"]
        got.append(np.load(tmp_path / sub / "dry_step.npy"))
    assert got[0].dtype == np.float64 and got[0].shape == (1,) and np.isfinite(got[0]).all()
    np.testing.assert_array_equal(got[0], got[1])


def test_dump_outputs_samples_a_large_array(tmp_path, monkeypatch):
    """An output over the size cap is written as a fixed sample: the same
    sorted choice of elements on every call, within the cap."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    big = np.arange(10_000, dtype=np.float64)
    small = np.arange(7, dtype=np.int32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), 0, {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.nbytes <= 2048 and a.size == 256 and np.all(np.diff(a) > 0)
    np.testing.assert_array_equal(a, b)
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    bench.dump_outputs(str(tmp_path / "a"), 3, {"small": small})
    assert os.path.exists(tmp_path / "a" / "small.rank3.npy")


def test_failing_rank_stops_the_job():
    p = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1"], FCS_BENCH_DRY_FAIL_RANK="1")
    assert p.returncode == 3
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_gpus_must_match_world_size():
    p = _run(["--gpus", "2", "--dry-run"], WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert p.returncode != 0 and "WORLD_SIZE=1" in p.stderr
