"""bench.py's plain run and --dump-outputs: the lean result line, and the files hold what the timed step returned
(CPU: the writer and its 64 MB cap; GPU: a plain run against the same op called through the Python wrappers)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_every_array(tmp_path):
    bench = _bench_module()
    arrays = {"dist": np.arange(12, dtype=np.float32).reshape(4, 3), "idx": np.arange(4, dtype=np.float64)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["dist.npy", "idx.npy"]
    for k, a in arrays.items():
        back = np.load(tmp_path / "out" / (k + ".npy"))
        assert back.dtype == a.dtype and np.array_equal(back, a)


def test_dump_outputs_samples_batch_elements_beyond_the_cap(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    rng = np.random.RandomState(3)
    arrays = {"a": rng.rand(64, 10).astype(np.float32), "b": rng.rand(64, 5, 3).astype(np.float64)}
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), dict(arrays))
    sel = np.load(tmp_path / "one" / "batch_index.npy")
    assert np.array_equal(sel, np.load(tmp_path / "two" / "batch_index.npy"))  # a fixed sample
    assert 1 <= sel.size < 64 and np.all(np.diff(sel) > 0)
    total = 0
    for k, a in arrays.items():
        back = np.load(tmp_path / "one" / (k + ".npy"))
        assert np.array_equal(back, a[sel.astype(np.int64)])
        total += back.nbytes
    assert total + sel.nbytes <= 4096


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_step(tmp_path):
    """A plain run: the headline fields, none of --full's, and the dumped last step equal to nn_distance +
    nn_distance_grad on the same seeded inputs."""
    import torch

    from rfnet_amd._raw import nn_distance, nn_distance_grad
    B, N, M = 4, 700, 3000
    out_dir = tmp_path / "outputs"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RF_FORCE_PG")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--batch", str(B), "--n", str(N), "--m", str(M), "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout[:500]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["unit"] == "pairs/s" and d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert "roofline" not in d and "cpu_baseline" not in d and "c5" not in d
    rng = np.random.RandomState(100)
    a = torch.from_numpy(rng.randn(B, N, 3).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.randn(B, M, 3).astype(np.float32)).cuda()
    d1, i1, d2, i2 = nn_distance(a, c)
    g1, g2 = nn_distance_grad(a, c, torch.ones_like(d1), i1, torch.ones_like(d2), i2)
    got = {k: np.load(out_dir / (k + ".npy")) for k in ("dist1", "idx1", "dist2", "idx2", "grad_xyz1", "grad_xyz2")}
    assert got["dist1"].dtype == np.float32 and got["idx1"].dtype == np.float64
    assert np.array_equal(got["dist1"], d1.cpu().numpy()) and np.array_equal(got["dist2"], d2.cpu().numpy())
    assert np.array_equal(got["idx1"], i1.cpu().numpy()) and np.array_equal(got["idx2"], i2.cpu().numpy())
    assert np.allclose(got["grad_xyz1"], g1.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(got["grad_xyz2"], g2.cpu().numpy(), rtol=1e-5, atol=1e-6)
