"""GPU: the evaluation driver's minimal matching distance (evalrun.evaluate(mmd_refs=...)) on the synthetic data set of
tests/test_gpu_evalrun.py, smaller: mmd.csv next to an unchanged results.csv, its rows what glue.minimal_matching
returns on the recomputed completions, the summary's average_mmd; off by default, with the outputs of today."""
import os

import numpy as np
import pytest
import torch

from test_gpu_evalrun import _make_dataset

pytestmark = pytest.mark.gpu


def test_mmd_csv_and_summary(tmp_path):
    from rfnet_amd import evalio, evalrun, glue
    from rfnet_amd.rfnet import RFNet
    ids = _make_dataset(str(tmp_path), np.random.RandomState(3), per_cat=2)
    torch.manual_seed(0)
    net = RFNet().cuda().eval()
    refs = (np.random.RandomState(5).random_sample((5, 700, 3)) - 0.5).astype(np.float32)
    run = lambda sub, **kw: evalrun.evaluate(net, str(tmp_path / "test.list"), str(tmp_path), str(tmp_path / sub), graph=False,
                                             rng=np.random.RandomState(1), warm_models=1, **kw)
    plain = run("plain")
    assert sorted(os.listdir(tmp_path / "plain")) == ["results.csv"]
    assert set(plain) == {"models", "average_time_s", "average_cd", "average_emd", "per_category", "graph", "mode"}
    res = run("mmd", mmd_refs=refs)
    assert set(res) == set(plain) | {"average_mmd"}
    assert sorted(os.listdir(tmp_path / "mmd")) == ["mmd.csv", "results.csv"]
    assert open(tmp_path / "mmd" / "results.csv").read() == open(tmp_path / "plain" / "results.csv").read()
    rows = evalio.read_mmd_csv(str(tmp_path / "mmd" / "mmd.csv"))
    assert [r[0] for r in rows] == ids  # one row per model
    rng = np.random.RandomState(1)  # the driver's resampling, replayed
    done = []
    for mid in ids:
        partial = evalio.resample_pcd(evalio.read_pcd(str(tmp_path / "partial" / (mid + ".pcd"))), 3000, rng=rng)
        x = torch.from_numpy(np.ascontiguousarray(partial, np.float32))[None].cuda()
        with torch.no_grad():
            done.append(net(x)[3][0].clone())
    val, at = glue.minimal_matching(torch.stack(done), torch.from_numpy(refs).cuda())
    assert [r[1] for r in rows] == val.cpu().tolist() and [r[2] for r in rows] == at.cpu().tolist()
    assert all(0 <= r[2] < 5 and r[1] > 0 for r in rows)
    assert abs(res["average_mmd"] - np.mean([r[1] for r in rows])) < 1e-12
