"""The evaluation driver of the reference (`test(args)`, recon_test.py:19-100) on the MI355X stack:
per model of a list -- read the partial / complete PCD, resample the partial scan to 3000 points
(`resample_pcd`), time the completion forward at batch 1, Chamfer distance of the completion to the
ground truth (`chamfer_big`) and fidelity of the input to the completion (`fidelity_loss`, the CSV's
`emd` column, recon_test.py:27-28,65), results.csv with the `id,cd,emd` header, per-category means,
average time skipping the first 10 models (recon_test.py:63,92).  Plots (matplotlib) are out of scope.

Batch-1 inference is launch-bound, not compute-bound: the generator is ~400 small kernels and the
host cannot enqueue them as fast as the GPU retires them.  `GraphedForward` therefore captures the
whole forward -- library GEMMs and this repository's HIP ops alike -- into ONE HIP graph at the fixed
input shape and replays it per model: one launch instead of ~400 (MI355X-first: "HIP streams and
graphs instead of a tracing compiler").  Replay runs the very same kernels: outputs are
bit-identical to the eager forward.
"""
import os
import sys
import time

import numpy as np
import torch

from . import evalio, glue


class GraphedForward:
    """net(x) for one fixed input shape as a captured HIP graph.  `__call__` copies the input into
    the graph's static buffer, replays, and returns the outputs (the graph's own static tensors:
    valid until the next call).

    The forward holds torch reductions, which replay stale on ROCm 7 unless the HIP runtime was started
    with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 (`rfnet_amd.enable_graph_safe_runtime()`): the runtime is asked
    (`_host.graph_replay_ok`) and, beyond that, ONE replay on a second input is compared with the eager
    forward before the graph is trusted.  Either check failing leaves `self.graph = None` and every call
    eager, with a note on stderr (`self.mode` says which)."""

    def __init__(self, net, example, warmup=3, check=True):
        from ._host import graph_replay_ok
        self.net = net
        self.graph = None
        self.static_in = example.detach().clone()
        if not graph_replay_ok(example.device):
            self.mode = ("eager (torch reductions do not replay from a HIP graph in this process: the HIP runtime "
                         "was started without DEBUG_CLR_GRAPH_PACKET_CAPTURE=0)")
            sys.stderr.write(f"rfnet_amd.evalrun: forward not captured -- {self.mode}\n")
            return
        cur = torch.cuda.current_stream(example.device)
        side = torch.cuda.Stream(device=example.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):  # lazy initialisations (library handles, the device check) happen here
                net(self.static_in)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = net(self.static_in)
        self.mode = "hip graph"
        if check:
            # a replay on a SECOND input against the eager forward (what a capture froze shows here)
            probe = torch.roll(example.detach(), 1, dims=-2) * 0.97
            with torch.no_grad():
                want = [t.clone() for t in net(probe)]
            got = self(probe)
            same = all(bool(torch.allclose(a, b, rtol=1e-5, atol=1e-6)) for a, b in zip(got, want))
            self.static_in.copy_(example)
            if not same:
                self.graph = None
                self.mode = "eager (a replay on a second input differed from the eager forward)"
                sys.stderr.write(f"rfnet_amd.evalrun: captured forward discarded -- {self.mode}\n")

    def __call__(self, x):
        if self.graph is None:
            with torch.no_grad():
                return self.net(x)
        self.static_in.copy_(x)
        self.graph.replay()
        return self.static_out


def evaluate(net, list_path, data_dir, results_dir, num_input_points=3000, save_pcd=False, graph=True, rng=None,
             warm_models=10, extra_metrics=False, tau=0.01, alpha=1000.0, mmd_refs=None, normal_consistency=False,
             normal_k=16):
    """recon_test.py's test(): returns the summary dict it prints (average time / CD / "EMD" and the
    per-category means) and writes <results_dir>/results.csv.

    `extra_metrics`: the per-model Chamfer comes from glue.chamfer_metrics(completion, gt) (the completion is the
    prediction) and its F-score at `tau`, Hausdorff distance and density-aware Chamfer distance (`alpha`) go to
    <results_dir>/metrics.csv (id, cd, fd, fscore, hausdorff, dcd) and, averaged, into the summary as
    average_fscore / average_hausdorff / average_dcd.  Off (the default): outputs exactly as before.

    `mmd_refs`: an (r, m, 3) array or tensor of reference clouds (a shelf of shapes, for scans without a ground
    truth).  The completions stay on the device, glue.minimal_matching (CD-L2 of the Chamfer matrix, one sort per
    cloud) runs after the loop, <results_dir>/mmd.csv gets id, mmd, ref_index and the summary `average_mmd`.  None
    (the default): outputs exactly as before.

    `normal_consistency`: glue.normal_consistency(completion, gt, k=normal_k) per model -- both clouds' normals estimated
    by PCA of their `normal_k` nearest neighbours -- into <results_dir>/normals.csv (id, nc, nc12, nc21) and, averaged, into
    the summary as average_nc.  Off (the default): outputs exactly as before; on, every other file keeps its bytes."""
    dev = next(net.parameters()).device
    with open(list_path) as f:
        model_list = f.read().splitlines()
    os.makedirs(results_dir, exist_ok=True)
    fwd = None
    rows, extra_rows, normal_rows, total_time = [], [], [], 0.0
    kept = []  # the completions, on the device (mmd_refs only)
    rng = rng if rng is not None else np.random.RandomState(0)
    for i, model_id in enumerate(model_list):
        partial = evalio.read_pcd(os.path.join(data_dir, "partial", "%s.pcd" % model_id))
        complete = evalio.read_pcd(os.path.join(data_dir, "complete", "%s.pcd" % model_id))
        partial = evalio.resample_pcd(partial, num_input_points, rng=rng)
        x = torch.from_numpy(np.ascontiguousarray(partial, np.float32))[None].to(dev)
        gt = torch.from_numpy(np.ascontiguousarray(complete, np.float32))[None].to(dev)
        if graph and fwd is None:
            fwd = GraphedForward(net, x)
        torch.cuda.synchronize(dev)
        start = time.time()
        with torch.no_grad():
            completion = (fwd(x) if fwd is not None else net(x))[3]
        torch.cuda.synchronize(dev)  # sess.run returns the completion to the host: the time includes the GPU work
        mytime = time.time() - start
        if i >= warm_models:
            total_time += mytime
        with torch.no_grad():
            if extra_metrics:
                met = glue.chamfer_metrics(completion, gt, tau=tau, alpha=alpha)
                cd = float(met["cd_l1"].mean())
            else:
                cd = float(glue.chamfer_big(completion, gt)[0])
            fd = float(glue.fidelity_loss(x, completion))
            if normal_consistency:
                nc = glue.normal_consistency(completion, gt, k=normal_k)
                normal_rows.append((model_id, float(nc["nc"][0]), float(nc["nc12"][0]), float(nc["nc21"][0])))
        rows.append((model_id, cd, fd))
        if mmd_refs is not None:
            kept.append(completion[0].clone())  # (a replayed graph hands out the same buffer every time)
        if extra_metrics:
            extra_rows.append((model_id, cd, fd, float(met["fscore"][0]), float(met["hausdorff"][0]), float(met["dcd"][0])))
        if save_pcd:
            synset_id, name = model_id.split("/")
            os.makedirs(os.path.join(results_dir, "pcds", synset_id), exist_ok=True)
            evalio.save_pcd(os.path.join(results_dir, "pcds", synset_id, "%s.pcd" % name), completion[0].cpu().numpy())
    evalio.write_results_csv(os.path.join(results_dir, "results.csv"), rows)
    timed = max(len(model_list) - warm_models, 1)
    extra = {}
    if extra_metrics:
        evalio.write_metrics_csv(os.path.join(results_dir, "metrics.csv"), extra_rows)
        for col, key in ((3, "average_fscore"), (4, "average_hausdorff"), (5, "average_dcd")):
            extra[key] = float(np.mean([r[col] for r in extra_rows])) if extra_rows else 0.0
    if normal_consistency:
        evalio.write_normals_csv(os.path.join(results_dir, "normals.csv"), normal_rows)
        extra["average_nc"] = float(np.mean([r[1] for r in normal_rows])) if normal_rows else 0.0
    if mmd_refs is not None:
        refs = torch.as_tensor(mmd_refs, dtype=torch.float32).to(dev)
        mmd_rows = []
        if kept:
            with torch.no_grad():
                val, at = glue.minimal_matching(torch.stack(kept), refs)
            mmd_rows = list(zip(model_list, val.cpu().tolist(), at.cpu().tolist()))
        evalio.write_mmd_csv(os.path.join(results_dir, "mmd.csv"), mmd_rows)
        extra["average_mmd"] = float(np.mean([r[1] for r in mmd_rows])) if mmd_rows else 0.0
    return {
        "models": len(model_list),
        "average_time_s": total_time / timed,
        "average_cd": float(np.mean([r[1] for r in rows])) if rows else 0.0,
        "average_emd": float(np.mean([r[2] for r in rows])) if rows else 0.0,
        "per_category": evalio.per_category_means(rows),
        "graph": fwd is not None and fwd.graph is not None,
        "mode": fwd.mode if fwd is not None else "eager (graph not requested)",
        **extra,
    }


def main(argv=None):
    """`python -m rfnet_amd.evalrun` with recon_test.py's flags (recon_test.py:103-112).  `--checkpoint`
    takes a torch state_dict of rfnet_amd.rfnet.RFNet (the reference's TensorFlow checkpoint blob is
    not part of the reference repository: SURVEY.md T10); without it the weights are random-init."""
    import argparse

    from .rfnet import RFNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--list_path", default="../../dense_data/test.list")
    ap.add_argument("--data_dir", default="../../dense_data/test")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--results_dir", default="results/recon")
    ap.add_argument("--num_gt_points", type=int, default=16384)  # kept for the reference's CLI; gt size comes from the files
    ap.add_argument("--save_pcd", action="store_true")
    ap.add_argument("--no_graph", action="store_true", help="eager forward instead of the captured HIP graph")
    ap.add_argument("--extra_metrics", action="store_true",
                    help="F-score, Hausdorff and density-aware Chamfer distance per model into metrics.csv")
    ap.add_argument("--tau", type=float, default=0.01, help="F-score distance threshold")
    ap.add_argument("--alpha", type=float, default=1000.0, help="DCD's exponent scale")
    ap.add_argument("--mmd_list", default=None,
                    help="a list of model ids whose complete/<id>.pcd files are the reference shelf: minimal matching "
                         "distance of every completion to it into mmd.csv (the clouds must have one size)")
    ap.add_argument("--normal_consistency", action="store_true",
                    help="normal consistency of every completion with its ground truth into normals.csv")
    ap.add_argument("--normal_k", type=int, default=16, help="neighbours of the normal estimation")
    a = ap.parse_args(argv)
    from . import enable_graph_safe_runtime
    enable_graph_safe_runtime()  # before the HIP runtime starts
    net = RFNet().cuda().eval()
    if a.checkpoint:
        net.load_state_dict(torch.load(a.checkpoint, map_location="cuda"))
    refs = None
    if a.mmd_list:
        with open(a.mmd_list) as f:
            refs = np.stack([evalio.read_pcd(os.path.join(a.data_dir, "complete", "%s.pcd" % ref_id)).astype(np.float32)
                             for ref_id in f.read().splitlines() if ref_id])
    res = evaluate(net, a.list_path, a.data_dir, a.results_dir, save_pcd=a.save_pcd, graph=not a.no_graph,
                   extra_metrics=a.extra_metrics, tau=a.tau, alpha=a.alpha, mmd_refs=refs,
                   normal_consistency=a.normal_consistency, normal_k=a.normal_k)
    print("Average time: %f" % res["average_time_s"])
    print("Average Chamfer distance: %f" % res["average_cd"])
    print("Average Earth mover distance: %f" % res["average_emd"])
    if a.extra_metrics:
        print("Average F-score@%g: %f" % (a.tau, res["average_fscore"]))
        print("Average Hausdorff distance: %f" % res["average_hausdorff"])
        print("Average density-aware Chamfer distance: %f" % res["average_dcd"])
    if a.normal_consistency:
        print("Average normal consistency (k = %d): %f" % (a.normal_k, res["average_nc"]))
    if refs is not None:
        print("Average minimal matching distance: %f" % res["average_mmd"])
    print("Chamfer distance per category")
    for k, v in res["per_category"].items():
        print(k, "%f" % v[0])
    print("Earth mover distance per category")
    for k, v in res["per_category"].items():
        print(k, "%f" % v[1])


if __name__ == "__main__":
    main()
