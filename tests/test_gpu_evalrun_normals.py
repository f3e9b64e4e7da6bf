"""GPU: the evaluation driver's normal consistency (evalrun.evaluate(normal_consistency=True)) on the synthetic data set of
tests/test_gpu_evalrun.py, three models: normals.csv next to results.csv and metrics.csv, whose bytes do not change; its rows
what glue.normal_consistency returns per model; off by default, with the outputs of today."""
import os

import numpy as np
import pytest
import torch

from test_gpu_evalrun import _make_dataset

pytestmark = pytest.mark.gpu


def test_normals_csv_and_untouched_tables(tmp_path):
    from rfnet_amd import evalio, evalrun, glue
    from rfnet_amd.rfnet import RFNet
    ids = _make_dataset(str(tmp_path), np.random.RandomState(4), cats=("02691156",), per_cat=3)
    torch.manual_seed(0)
    net = RFNet().cuda().eval()
    k = 12
    run = lambda sub, **kw: evalrun.evaluate(net, str(tmp_path / "test.list"), str(tmp_path), str(tmp_path / sub), graph=False,
                                             rng=np.random.RandomState(1), warm_models=1, extra_metrics=True, **kw)
    plain = run("plain")
    assert not os.path.exists(tmp_path / "plain" / "normals.csv") and "average_nc" not in plain
    res = run("normals", normal_consistency=True, normal_k=k)
    assert set(res) == set(plain) | {"average_nc"}
    for name in ("results.csv", "metrics.csv"):
        assert (tmp_path / "normals" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    rows = evalio.read_normals_csv(str(tmp_path / "normals" / "normals.csv"))
    assert (tmp_path / "normals" / "normals.csv").read_text().splitlines()[0] == "id,nc,nc12,nc21"
    assert [r[0] for r in rows] == ids and len(rows) == 3
    rng = np.random.RandomState(1)  # the driver's resampling, replayed
    for mid, nc, nc12, nc21 in rows:
        partial = evalio.resample_pcd(evalio.read_pcd(str(tmp_path / "partial" / (mid + ".pcd"))), 3000, rng=rng)
        x = torch.from_numpy(np.ascontiguousarray(partial, np.float32))[None].cuda()
        gt = torch.from_numpy(evalio.read_pcd(str(tmp_path / "complete" / (mid + ".pcd"))).astype(np.float32))[None].cuda()
        with torch.no_grad():
            want = glue.normal_consistency(net(x)[3], gt, k=k)
        assert (nc, nc12, nc21) == (float(want["nc"][0]), float(want["nc12"][0]), float(want["nc21"][0])), mid
        assert 0 < nc <= 1 and 0 < nc12 <= 1 and 0 < nc21 <= 1
    assert abs(res["average_nc"] - np.mean([r[1] for r in rows])) < 1e-12
