"""Surface normals by local PCA and normal consistency against the best routes without the ops, on one GPU (ms per call, device
events):
  estimate_normals   glue.estimate_normals: knn_point of the cloud against itself, then rf_local_pca
  local_pca          rf_local_pca alone, on an idx computed before the clock starts
  torch eigh         the same idx, then group_point, the centred einsum to (b, n, 3, 3) and torch.linalg.eigh (fp32)
  torch closed form  the same covariances, the smallest eigenvalue from the trigonometric closed form and its vector as the
                     largest cross product of two rows of C - l0 I (fp32)
  knn_point          the neighbour search both routes share
The baseline of estimate_normals is knn_point plus the faster torch route.  Same device, same process, routes alternated round by
round (a round is `reps` back-to-back calls between two events, the calls rotating over two sets of inputs; the figure is the
median over the rounds with the spread next to it), then the library's own per-kernel device times (rf_profile_*).  A torch route
whose single call takes longer than SLOW_MS is timed by that one call and stays out of the rounds.  Before anything is timed the
agreement of the routes is reported: the fraction of points whose normals agree to |cos| >= 0.999.
Then normal_consistency: rf_nn_normal_consistency against its torch expression (gather by idx, dot, abs, mean) on nn_distance's
indices.
python tools/ab_normals.py [rounds] [output file]      (writes profiles/normals_ab.txt)"""
import math
import os
import sys

import numpy as np
import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
from rfnet_amd import _raw, glue  # noqa: E402
from rfnet_amd._lib import profile_collect, profile_enable  # noqa: E402
from rfnet_amd.tf_ops.grouping.tf_grouping import group_point  # noqa: E402

# (b, n, k)
SHAPES = [(32, 2048, 16), (1, 16384, 16), (32, 2048, 64)]
LAST_SHAPE = (32, 16384, 16)  # the largest batched eigen-solve of the torch route: timed last, so that the rest is on file
NC_SHAPES = [(32, 2048, 2048), (32, 16384, 16384)]
SLOW_MS = 1000.0
OUT = os.path.join(ROOT, "profiles", "normals_ab.txt")


def say(s=""):
    """to the terminal and, line by line, to the profile: a run that ends early leaves what it measured"""
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        fn(k & 1)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernels(fn, reps=4):
    profile_enable(True)
    for k in range(reps):
        fn(k & 1)
    torch.cuda.synchronize()
    prof = profile_collect()
    profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}


def ab(routes, rounds):
    """routes {name: fn(set)} -> {name: (median, min, max, reps)}, alternated round by round; a route slower than SLOW_MS per
    call is timed once, after its warm-up call, and reported with reps = 1"""
    fast, res = {}, {}
    for name, fn in routes.items():
        fn(0)  # warm-up: code objects, workspaces, the allocator, the libraries' choices
        torch.cuda.synchronize()
        once = window(fn, 1)
        if once > SLOW_MS:
            res[name] = (once, once, once, 1)
        else:
            fast[name] = fn
    reps = {k: max(2, min(50, int(math.ceil(200.0 / rounds / max(window(fn, 2), 1e-3))))) for k, fn in fast.items()}
    times = {k: [] for k in fast}
    for _ in range(rounds):
        for k, fn in fast.items():
            times[k].append(window(fn, reps[k]))
    res.update({k: (float(np.median(v)), min(v), max(v), reps[k]) for k, v in times.items()})
    return res


def covariances(xyz, idx):
    nbr = group_point(xyz, idx)  # (b, n, k, 3)
    d = nbr - nbr.mean(2, keepdim=True)
    return torch.einsum("bnki,bnkj->bnij", d, d) / idx.shape[2]


def torch_eigh(xyz, idx):
    w, v = torch.linalg.eigh(covariances(xyz, idx))
    return v[..., 0], w


def torch_closed(xyz, idx):
    """The smallest eigenvalue of a symmetric 3 x 3 matrix in closed form (the trigonometric solution of the characteristic cubic)
    and its eigenvector as the largest of the three cross products of rows of C - l0 I."""
    C = covariances(xyz, idx)
    eye = torch.eye(3, device=C.device, dtype=C.dtype)
    q = (C[..., 0, 0] + C[..., 1, 1] + C[..., 2, 2]) / 3
    Bm = C - q[..., None, None] * eye
    p = torch.sqrt((Bm * Bm).sum((-1, -2)) / 6).clamp_min(1e-30)
    Bn = Bm / p[..., None, None]
    det = (Bn[..., 0, 0] * (Bn[..., 1, 1] * Bn[..., 2, 2] - Bn[..., 1, 2] * Bn[..., 2, 1])
           - Bn[..., 0, 1] * (Bn[..., 1, 0] * Bn[..., 2, 2] - Bn[..., 1, 2] * Bn[..., 2, 0])
           + Bn[..., 0, 2] * (Bn[..., 1, 0] * Bn[..., 2, 1] - Bn[..., 1, 1] * Bn[..., 2, 0]))
    phi = torch.acos((det / 2).clamp(-1, 1)) / 3
    l0 = q + 2 * p * torch.cos(phi + 2 * math.pi / 3)  # the smallest of the three
    A = C - l0[..., None, None] * eye
    r0, r1, r2 = A[..., 0, :], A[..., 1, :], A[..., 2, :]
    cr = torch.stack([torch.linalg.cross(r0, r1), torch.linalg.cross(r0, r2), torch.linalg.cross(r1, r2)], -2)
    best = (cr * cr).sum(-1).argmax(-1)
    n = torch.gather(cr, -2, best[..., None, None].expand(*best.shape, 1, 3)).squeeze(-2)
    return n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30), l0


def fmt(res, name):
    med, lo, hi, reps = res[name]
    return f"  {name:24s} median {med:.4f}  min {lo:.4f}  max {hi:.4f}   ({reps} calls per round)" if reps > 1 else \
        f"  {name:24s} ONE call {med:.1f}   (slower than {SLOW_MS:.0f} ms: not in the rounds)"


def one_shape(b, n, k, rounds):
    say(f"\n## b = {b}, n = {n}, k = {k}")
    g = torch.Generator(device="cuda").manual_seed(n + k)
    # a noisy sphere: a surface, as the clouds this op is for
    x = []
    for _ in range(2):
        p = torch.randn(b, n, 3, device="cuda", generator=g)
        x.append((p / p.norm(dim=-1, keepdim=True) * (1 + 0.005 * torch.randn(b, n, 1, device="cuda", generator=g))).contiguous())
    idx = [_raw.knn_point(k, t, t)[1] for t in x]
    ours = glue.local_pca(x[0], idx[0])["normals"]
    for name, fn in (("torch eigh", torch_eigh), ("torch closed form", torch_closed)):
        cos = (ours * fn(x[0], idx[0])[0]).sum(-1).abs()
        say(f"  agreement with {name}: {float((cos >= 0.999).float().mean()):.5f} of the normals within |cos| >= 0.999, smallest {float(cos.min()):.4f}")
    del ours, cos
    torch.cuda.empty_cache()
    routes = {"estimate_normals": lambda s: glue.estimate_normals(x[s], k), "knn_point": lambda s: _raw.knn_point(k, x[s], x[s]),
              "local_pca": lambda s: glue.local_pca(x[s], idx[s]), "torch eigh": lambda s: torch_eigh(x[s], idx[s]),
              "torch closed form": lambda s: torch_closed(x[s], idx[s])}
    res = ab(routes, rounds)
    for name in routes:
        say(fmt(res, name))
    best = min(("torch eigh", "torch closed form"), key=lambda r: res[r][0])
    say(f"  local_pca / {best} (medians): {res['local_pca'][0] / res[best][0]:.4f}")
    say(f"  estimate_normals / (knn_point + {best}): {res['estimate_normals'][0] / (res['knn_point'][0] + res[best][0]):.4f}")
    kern = kernels(routes["estimate_normals"])
    say(f"  kernels of estimate_normals (ms per call) {kern}")
    ms = kern.get("local_pca")
    if ms:
        say(f"  local_pca kernel: {b * n} queries in {ms:.4f} ms = {ms * 1e6 / (b * n):.2f} ns per query over the chip")


def nc_torch(n1, n2, i1, i2):
    def half(a, c, ix):
        d = (a * torch.gather(c, 1, ix.long()[..., None].expand(-1, -1, 3))).sum(-1)
        return d.abs().mean(1), d.mean(1)
    a12, s12 = half(n1, n2, i1)
    a21, s21 = half(n2, n1, i2)
    return torch.stack([a12, a21, s12, s21], 1)


def one_nc_shape(b, n, m, rounds):
    say(f"\n## normal consistency, b = {b}, n = {n}, m = {m}")
    g = torch.Generator(device="cuda").manual_seed(n + m)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, 3, device="cuda", generator=g), dim=-1)  # noqa: E731
    x1, x2 = torch.rand(b, n, 3, device="cuda", generator=g), torch.rand(b, m, 3, device="cuda", generator=g)
    _, i1, _, i2 = _raw.nn_distance(x1, x2)
    n1, n2 = [unit(b, n) for _ in range(2)], [unit(b, m) for _ in range(2)]
    err = float((_raw.nn_normal_consistency(n1[0], n2[0], i1, i2) - nc_torch(n1[0], n2[0], i1, i2)).abs().max())
    say(f"  agreement: largest difference of the two routes {err:.2e}")
    routes = {"nn_normal_consistency": lambda s: _raw.nn_normal_consistency(n1[s], n2[s], i1, i2),
              "torch gather + dot + mean": lambda s: nc_torch(n1[s], n2[s], i1, i2)}
    res = ab(routes, rounds)
    for name in routes:
        say(fmt(res, name))
    say(f"  ratio ours / torch (medians): {res['nn_normal_consistency'][0] / res['torch gather + dot + mean'][0]:.4f}")
    say(f"  kernels ours (ms per call) {kernels(routes['nn_normal_consistency'])}")


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# normals A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call")
    say("# routes: ours = knn_point + rf_local_pca ; torch = the same idx, group_point, centred einsum, then linalg.eigh or the closed form")
    for shape in SHAPES:
        one_shape(*shape, rounds)
        torch.cuda.empty_cache()
    for shape in NC_SHAPES:
        one_nc_shape(*shape, rounds)
        torch.cuda.empty_cache()
    one_shape(*LAST_SHAPE, rounds)


if __name__ == "__main__":
    main()
