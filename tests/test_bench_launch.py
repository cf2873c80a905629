"""bench.py's multi-GPU entry (CPU): `--gpus N` without a launcher starts N ranks itself and
refuses, rather than silently measuring fewer GPUs, when it cannot honour N.  One GPU test: what a
plain run, `--full` and `--dump-outputs` each do."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_more_gpus_than_visible_is_refused():
    r = _run(["--gpus", "2", "--steps", "1"], {"CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""})
    assert r.returncode != 0
    assert "not measuring" in r.stderr
    assert '"n_gpus"' not in r.stdout


def test_launcher_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_zero_steps_is_refused():
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0
    assert "--steps" in r.stderr and '"ms_per_step"' not in r.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_frame(tmp_path, monkeypatch, capsys):
    """A plain run times the headline frames only; --full adds the FP32 and C-ABI records beside the
    same line; --dump-outputs writes the last timed frame, identical from run to run and equal to
    the frame the line's `check` digests."""
    import hashlib
    import json
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench

    def run(name, extra):
        out = tmp_path / name
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--warmup-s", "0",
                                          "--dump-outputs", str(out)] + extra)
        capsys.readouterr()
        bench.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert sorted(os.listdir(out)) == ["frame.npy"]
        return line, np.load(out / "frame.npy")

    a, fa = run("a", [])
    b, fb = run("b", [])
    c, fc = run("c", ["--full", "--no-cpu-baseline"])
    for line in (a, b, c):
        assert line["steps"] == 2 and line["dtype"] == "f64" and line["unit"] == "Msamples/s"
        assert line["higher_is_better"] is True and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["metric"].startswith("Msamples/s") and line["roofline"]["kernel_ms"] > 0
        assert line["cpu_baseline"] is None
    for line in (a, b):
        assert "f32_fast_path" not in line and "abi_device_list" not in line
    assert c["f32_fast_path"]["dtype"] == "f32" and c["f32_fast_path"]["value"] > 0
    assert c["abi_device_list"]["sha16_equals_line"] is True
    assert fa.dtype == np.float64 and fa.shape == (600, 600, 3) and np.isfinite(fa).all()
    assert hashlib.sha256(fa.tobytes()).hexdigest()[:16] == a["check"]["sha16"]
    assert np.array_equal(fa, fb) and np.array_equal(fa, fc)


def test_wait_exited_sees_exits_and_zombies():
    """bench.py times the C-ABI device list only once the other ranks have exited: wait_exited
    returns when the processes are gone or zombies (exited, GPU contexts released, not yet reaped)."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    p = subprocess.Popen([sys.executable, "-c", "import time; time.sleep(0.3)"])
    t0 = time.perf_counter()
    waited = bench.wait_exited([p.pid], timeout_s=20.0)
    assert 0.1 < waited < 10.0 and time.perf_counter() - t0 < 10.0
    # not reaped yet: a zombie counts as exited
    assert bench.wait_exited([p.pid], timeout_s=5.0) < 1.0
    p.wait()
    assert bench.wait_exited([p.pid, 2 ** 22 + 12345], timeout_s=5.0) < 1.0  # gone / never existed
    q = subprocess.Popen([sys.executable, "-c", "import time; time.sleep(30)"])
    try:
        assert bench.wait_exited([q.pid], timeout_s=0.5) >= 0.5  # gives up at the timeout
    finally:
        q.kill()
        q.wait()
