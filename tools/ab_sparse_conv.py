"""Submanifold sparse convolution against the best routes without the op, on one GPU (ms per call, device events):
  ours    rf_sparse_conv_map (one workgroup per sample: keys, the LDS sort, a binary search per slot), rf_sparse_conv for the
          forward and the gradient to the features, rf_sparse_conv_grad_weight (glue.sparse_conv)
  torch   the map: int64 keys with the batch index folded in, one sort, torch.searchsorted per slot;
          the convolution, two routes, the faster is reported:  im2col -- feat_pad[nbr] as a (rows, K c) matrix and ONE mm --
          and the per-offset loop -- index_select, mm, index_add_ per slot over that slot's live pairs (the pair lists are built
          outside the timed region: they belong to the map); autograd for the backward of both
Clouds are synthetic surfaces (points on a sphere), the cell chosen so that there are about half as many cells as points; the
features live on the cells (grid_pool's rows).  Same device, same process, routes alternated round by round (the method of
tools/ab_grid_pool.py: a round is `reps` back-to-back calls between two events, the median over the rounds with the spread next
to it), then the library's own per-kernel device times.  Before anything is timed the routes are compared.  Per shape also: the
share of live slots, the fraction of (32-row tile, slot) blocks no row of which has the slot -- what the kernel skips -- and the
achieved fraction of the 157.3 TF fp32 matrix peak counted on live slots.
python tools/ab_sparse_conv.py [rounds] [output file]      (writes profiles/sparse_conv_ab.txt)"""
import os
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_grid_pool as AB  # noqa: E402  (window, ab, kernels, fmt: the method, once)
from rfnet_amd import _raw, glue  # noqa: E402

# (b, points, cin, cout, kernel_size)
SHAPES = [(32, 16384, 64, 64, 3), (32, 16384, 32, 32, 3), (32, 16384, 128, 128, 3), (32, 16384, 32, 32, 5), (1, 16384, 64, 64, 3),
          (32, 2048, 64, 64, 3), (1, 2048, 64, 64, 3)]
PEAK = 157.3e12
OUT = os.path.join(ROOT, "profiles", "sparse_conv_ab.txt")


def say(s=""):
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def sphere(b, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.randn(b, n, 3, device="cuda", generator=g)
    return 0.5 * v / v.norm(dim=-1, keepdim=True)


def cell_for_half(xyz):
    """the cell edge that gives about half as many cells as points (bisection on the op itself; set-up, not timed)"""
    lo, hi, want = 1e-4, 1.0, xyz.shape[0] * xyz.shape[1] / 2
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        if _raw.grid_cluster(xyz, mid)["nclusters"].sum().item() > want:
            lo = mid
        else:
            hi = mid
    return hi


# ---- the routes without the op ---------------------------------------------------------------------------------------------------
def torch_map(coords, ncl, ks):
    b, n, _ = coords.shape
    r = ks // 2
    c = coords.long() + 32768
    live = torch.arange(n, device=coords.device)[None] < ncl[:, None]
    key = (torch.arange(b, device=coords.device)[:, None] << 48) | (c[..., 0] << 32) | (c[..., 1] << 16) | c[..., 2]
    key = torch.where(live, key, torch.full_like(key, 1 << 62)).reshape(-1)
    skey, order = torch.sort(key)
    d = torch.arange(-r, r + 1, device=coords.device)
    off = ((d[:, None, None] << 32) + (d[None, :, None] << 16) + d[None, None, :]).reshape(-1)
    want = key[:, None] + off[None]
    pos = torch.searchsorted(skey, want).clamp(max=b * n - 1)
    hit = (skey[pos] == want) & live.reshape(-1, 1)
    return torch.where(hit, order[pos] % n, -1).reshape(b, n, -1).int()


class TorchRoutes:
    """what belongs to the map, built once: the live rows, their neighbours as global rows (the zero row for absent ones), and
    per slot the (output row, input row) pairs"""

    def __init__(self, nbr, ncl):
        b, n, K = nbr.shape
        live = (torch.arange(n, device=nbr.device)[None] < ncl[:, None]).reshape(-1)
        self.rows = live.nonzero().squeeze(1)
        rank = torch.cumsum(live.long(), 0) - 1  # global row -> compact row
        g = nbr.long() + (torch.arange(b, device=nbr.device) * n)[:, None, None]
        self.R = int(self.rows.numel())
        self.idx = torch.where(nbr >= 0, rank[g.clamp(min=0)], self.R).reshape(b * n, K)[self.rows]  # (R, K), R = absent
        self.pairs = []
        for t in range(K):
            o = (self.idx[:, t] < self.R).nonzero().squeeze(1)
            self.pairs.append((o, self.idx[o, t]))

    def compact(self, feat):
        return feat.reshape(-1, feat.shape[-1])[self.rows]

    def im2col(self, f, w):  # f (R, cin)
        K, cin, cout = w.shape
        pad = torch.cat([f, f.new_zeros(1, cin)])
        return pad[self.idx].reshape(self.R, K * cin) @ w.reshape(K * cin, cout)

    def loop(self, f, w):
        out = f.new_zeros(self.R, w.shape[2])
        for t, (o, i) in enumerate(self.pairs):
            if o.numel():
                out = out.index_add(0, o, f.index_select(0, i) @ w[t])
        return out


def fwdbwd(fn, f, w, g):
    f, w = f.detach().requires_grad_(), w.detach().requires_grad_()
    fn(f, w).backward(g)
    return f.grad, w.grad


def pair(res, ours, torches, what):
    say(AB.fmt(res, ours))
    for t in torches:
        say(AB.fmt(res, t))
    best = min(torches, key=lambda t: res[t][0])
    ratio = res[ours][0] / res[best][0]
    say(f"  ours / best torch route ({best.strip()}) {what}: {ratio:.3f}  {'LOSES' if ratio > 1 else 'wins'}")
    return res[ours][0]


def one_shape(b, n, cin, cout, ks, rounds):
    K = ks ** 3
    xyz = sphere(b, n, n + b)
    cell = cell_for_half(xyz)
    info = _raw.grid_cluster(xyz, cell, "z")
    coords, ncl = info["coords"], info["nclusters"]
    M = int(ncl.sum().item())
    say(f"\n## b = {b}, {n} points on a sphere, cell = {cell:.4f}: {M} cells ({M / b:.0f} per sample), {cin} -> {cout} channels, K = {K}")
    nbr = _raw.sparse_conv_map(coords, ncl, ks)
    assert torch.equal(nbr, torch_map(coords, ncl, ks)), "the two maps differ"
    live = nbr >= 0
    slots = int(live.sum().item())
    pad = (-n) % 32
    tiles = torch.nn.functional.pad(live, (0, 0, 0, pad)).reshape(b, -1, 32, K).any(2)  # (b, tiles, K)
    ntiles = int(((torch.arange(tiles.shape[1], device="cuda") * 32)[None] < ncl[:, None]).sum().item())
    say(f"  live slots {slots} of {M * K} ({slots / (M * K):.3f}); (tile, slot) blocks with no live row, skipped by the kernel: "
        f"{1 - int(tiles.sum().item()) / (ntiles * K):.3f} of {ntiles * K}")
    res = AB.ab({"ours  map": lambda s: _raw.sparse_conv_map(coords, ncl, ks), "torch map (sort + searchsorted)": lambda s: torch_map(coords, ncl, ks)},
                rounds)
    pair(res, "ours  map", ["torch map (sort + searchsorted)"], "map")

    g = torch.Generator(device="cuda").manual_seed(1)
    feat = [torch.randn(b, n, cin, device="cuda", generator=g) for _ in range(2)]
    gout = [torch.randn(b, n, cout, device="cuda", generator=g) for _ in range(2)]
    w = torch.randn(K, cin, cout, device="cuda", generator=g) / (K * cin) ** 0.5
    T = TorchRoutes(nbr, ncl)
    fc, gc = [T.compact(f) for f in feat], [T.compact(x) for x in gout]
    ours = lambda f, ww: glue.sparse_conv(f, ww, nbr, ncl)  # noqa: E731
    o, a, lp = T.compact(ours(feat[0], w)), T.im2col(fc[0], w), T.loop(fc[0], w)
    scale = float(a.abs().max())
    say(f"  agreement: ours - im2col {float((o - a).abs().max()) / scale:.1e}, loop - im2col {float((lp - a).abs().max()) / scale:.1e} "
        f"(of the largest output)")
    go, ga = fwdbwd(ours, feat[0], w, gout[0]), fwdbwd(T.im2col, fc[0], w, gc[0])
    say(f"  gradients: feat {float((T.compact(go[0]) - ga[0]).abs().max() / ga[0].abs().max()):.1e}, "
        f"weight {float((go[1] - ga[1]).abs().max() / ga[1].abs().max()):.1e}")
    del o, a, lp, go, ga
    routes = {"ours  forward": lambda s: ours(feat[s], w), "torch forward im2col": lambda s: T.im2col(fc[s], w),
              "torch forward loop": lambda s: T.loop(fc[s], w),
              "ours  fwd+bwd": lambda s: fwdbwd(ours, feat[s], w, gout[s]), "torch fwd+bwd im2col": lambda s: fwdbwd(T.im2col, fc[s], w, gc[s]),
              "torch fwd+bwd loop": lambda s: fwdbwd(T.loop, fc[s], w, gc[s])}
    res = AB.ab(routes, rounds)
    ms = pair(res, "ours  forward", ["torch forward im2col", "torch forward loop"], "forward")
    pair(res, "ours  fwd+bwd", ["torch fwd+bwd im2col", "torch fwd+bwd loop"], "fwd+bwd")
    k = AB.kernels(routes["ours  fwd+bwd"])
    say(f"  kernels ours, fwd+bwd (ms per call; sparse_conv is the forward and the gradient to the features together) {k}")
    flops = 2.0 * slots * cin * cout
    say(f"  forward: {flops / (ms * 1e-3) / 1e12:.2f} TF on live slots = {flops / (ms * 1e-3) / PEAK:.3f} of the fp32 matrix peak (call time); "
        f"weight gradient kernel: {flops / (k.get('sparse_conv_wgrad', float('nan')) * 1e-3) / PEAK:.3f}")


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    AB.OUT = OUT
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# submanifold sparse convolution A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call, medians with min and max")
    say("# ours = rf_sparse_conv_map, rf_sparse_conv (forward, gradient to the features), rf_sparse_conv_grad_weight ; torch = sorted "
        "int64 keys + searchsorted for the map, im2col (one mm) and the per-offset loop (index_select, mm, index_add) with autograd")
    for shape in SHAPES:
        one_shape(*shape, rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
