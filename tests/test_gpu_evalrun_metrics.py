"""GPU: the evaluation driver's extra metrics (evalrun.evaluate(extra_metrics=True)) on the synthetic data set of
tests/test_gpu_evalrun.py, smaller: metrics.csv next to an unchanged results.csv, its rows what glue.chamfer_metrics
returns per model, the summary's three new averages; off by default, with the outputs of today."""
import os

import numpy as np
import pytest
import torch

from test_gpu_evalrun import _make_dataset

pytestmark = pytest.mark.gpu


def test_extra_metrics_csv_and_summary(tmp_path):
    from rfnet_amd import evalio, evalrun, glue
    from rfnet_amd.rfnet import RFNet
    ids = _make_dataset(str(tmp_path), np.random.RandomState(3), per_cat=2)
    torch.manual_seed(0)
    net = RFNet().cuda().eval()
    tau, alpha = 0.05, 200.0
    run = lambda sub, **kw: evalrun.evaluate(net, str(tmp_path / "test.list"), str(tmp_path), str(tmp_path / sub), graph=False,
                                             rng=np.random.RandomState(1), warm_models=1, **kw)
    plain = run("plain")
    assert not os.path.exists(tmp_path / "plain" / "metrics.csv")
    assert set(plain) == {"models", "average_time_s", "average_cd", "average_emd", "per_category", "graph", "mode"}
    res = run("extra", extra_metrics=True, tau=tau, alpha=alpha)
    assert set(res) == set(plain) | {"average_fscore", "average_hausdorff", "average_dcd"}
    base = evalio.read_results_csv(str(tmp_path / "plain" / "results.csv"))
    rows = evalio.read_results_csv(str(tmp_path / "extra" / "results.csv"))  # the reference's format, still
    extra = evalio.read_metrics_csv(str(tmp_path / "extra" / "metrics.csv"))
    assert [r[0] for r in rows] == ids and [r[0] for r in extra] == ids
    rng = np.random.RandomState(1)  # the driver's resampling, replayed
    for (mid, cd0, fd0), (_, cd, fd), (_, mcd, mfd, fscore, hd, dcd) in zip(base, rows, extra):
        assert mcd == cd and mfd == fd and fd == fd0
        assert abs(cd - cd0) <= 1e-5 * abs(cd0)  # the same number from the metrics epilogue and from chamfer_big
        partial = evalio.resample_pcd(evalio.read_pcd(str(tmp_path / "partial" / (mid + ".pcd"))), 3000, rng=rng)
        x = torch.from_numpy(np.ascontiguousarray(partial, np.float32))[None].cuda()
        gt = torch.from_numpy(evalio.read_pcd(str(tmp_path / "complete" / (mid + ".pcd"))).astype(np.float32))[None].cuda()
        with torch.no_grad():
            met = glue.chamfer_metrics(net(x)[3], gt, tau=tau, alpha=alpha)
        for got, key in ((mcd, "cd_l1"), (fscore, "fscore"), (hd, "hausdorff"), (dcd, "dcd")):
            assert got == float(met[key][0]), (mid, key)
        assert 0 <= fscore <= 1 and hd > 0 and 0 < dcd < 1
    for col, key in ((3, "average_fscore"), (4, "average_hausdorff"), (5, "average_dcd")):
        assert abs(res[key] - np.mean([r[col] for r in extra])) < 1e-12
    assert abs(res["average_cd"] - np.mean([r[1] for r in rows])) < 1e-12
