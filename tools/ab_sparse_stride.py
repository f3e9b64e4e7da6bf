"""Strided sparse convolution (kernel 2, stride 2) and its transpose against the routes without the op, on one GPU (ms per call,
device events):
  ours    rf_sparse_stride_map (one workgroup per sample: coarse keys, the LDS sort, a scan of the heads), rf_sparse_conv_strided
          in its four modes and rf_sparse_conv_strided_grad_weight (glue.sparse_conv_down / sparse_conv_up)
  torch   the map: coords >> 1, int64 keys with the batch index folded in, torch.unique(return_inverse) (a host synchronisation);
          the convolution, two routes on the compacted rows, the faster is reported: im2col -- down: feat_pad[child] as a
          (rows, 8 c) matrix and ONE mm; up: ONE mm onto all eight slots, (rows, 8 c'), of which each fine row takes
          [parent][slot] -- and the per-slot loop -- index_select, mm, index_add per slot over that slot's pairs (the pair lists
          are built outside the timed region: they belong to the map); autograd for the backward of both
  gather  the fan-out modes through the GATHER kernel: the same library entry in the mode "down" on a (b, n, 8) expansion of up
          (row i has its parent in slot t and seven absent slots), so a tile of 32 fine rows runs every slot some row has.  The
          same bits; it is the simpler alternative the fan-out kernel has to beat.
Clouds are those of tools/ab_sparse_conv.py: points on a sphere, the cell chosen so that there are about half as many cells as
points.  Same device, same process, routes alternated round by round (the method of tools/ab_grid_pool.py: the median over the
rounds with min and max); every table has one route TWICE under two names, whose difference is the same-against-same spread
the other differences are to be read against.  Before anything is timed the routes are compared.
python tools/ab_sparse_stride.py [rounds] [output file]      (writes profiles/sparse_stride_ab.txt)"""
import os
import sys

import torch

ROOT = __file__.rsplit("/", 2)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ab_grid_pool as AB  # noqa: E402  (window, ab, kernels, fmt: the method, once)
import ab_sparse_conv as SC  # noqa: E402  (sphere, cell_for_half, fwdbwd: the clouds, once)
from rfnet_amd import _raw, glue  # noqa: E402

# (b, points, channels of the fine level, channels of the coarse level)
SHAPES = [(32, 16384, 32, 64), (32, 16384, 64, 128), (32, 2048, 32, 64), (32, 2048, 64, 128), (1, 16384, 32, 64), (1, 16384, 64, 128)]
OUT = os.path.join(ROOT, "profiles", "sparse_stride_ab.txt")


def say(s=""):
    print(s, flush=True)
    with open(OUT, "a") as f:
        f.write(s + "\n")


def torch_map(coords, ncl):
    b, n, _ = coords.shape
    c = (coords.long() >> 1) + 16384
    live = torch.arange(n, device=coords.device)[None] < ncl[:, None]
    key = (torch.arange(b, device=coords.device)[:, None] << 48) | (c[..., 0] << 32) | (c[..., 1] << 16) | c[..., 2]
    cells, inverse = torch.unique(key[live], return_inverse=True)  # (sizes known on the host: the call synchronised)
    return cells, inverse


class TorchRoutes:
    """what belongs to the map, built once, on compacted rows: per coarse row its eight children (the zero row for absent ones),
    per fine row its entry 8 parent + slot (the zero row for none), per slot the (coarse row, fine row) pairs"""

    def __init__(self, level, ncl, n):
        child, up, nclc = level["child"], level["up"], level["nclusters"]
        b, nc, _ = child.shape
        dev = child.device
        live_f = (torch.arange(n, device=dev)[None] < ncl[:, None]).reshape(-1)
        live_c = (torch.arange(nc, device=dev)[None] < nclc[:, None]).reshape(-1)
        self.rows_f, self.rows_c = live_f.nonzero().squeeze(1), live_c.nonzero().squeeze(1)
        self.Rf, self.Rc = int(self.rows_f.numel()), int(self.rows_c.numel())
        rank_f, rank_c = torch.cumsum(live_f.long(), 0) - 1, torch.cumsum(live_c.long(), 0) - 1
        g = child.long() + (torch.arange(b, device=dev) * n)[:, None, None]
        self.child = torch.where(child >= 0, rank_f[g.clamp(min=0)], self.Rf).reshape(b * nc, 8)[self.rows_c]  # (Rc, 8)
        j = (up.long() >> 3) + (torch.arange(b, device=dev) * nc)[:, None]
        self.up = torch.where(up >= 0, rank_c[j.clamp(min=0)] * 8 + (up.long() & 7), self.Rc * 8).reshape(-1)[self.rows_f]  # (Rf,)
        self.pairs = []
        for t in range(8):
            o = (self.child[:, t] < self.Rf).nonzero().squeeze(1)
            self.pairs.append((o, self.child[o, t]))

    def fine(self, x):
        return x.reshape(-1, x.shape[-1])[self.rows_f]

    def coarse(self, x):
        return x.reshape(-1, x.shape[-1])[self.rows_c]

    def down_im2col(self, f, w):  # f (Rf, cin) -> (Rc, cout)
        _, cin, cout = w.shape
        pad = torch.cat([f, f.new_zeros(1, cin)])
        return pad[self.child].reshape(self.Rc, 8 * cin) @ w.reshape(8 * cin, cout)

    def down_loop(self, f, w):
        out = f.new_zeros(self.Rc, w.shape[2])
        for t, (j, i) in enumerate(self.pairs):
            if j.numel():
                out = out.index_add(0, j, f.index_select(0, i) @ w[t])
        return out

    def up_im2col(self, f, w):  # f (Rc, cin) -> (Rf, cout)
        _, cin, cout = w.shape
        all8 = (f @ w.permute(1, 0, 2).reshape(cin, 8 * cout)).reshape(self.Rc * 8, cout)
        return torch.cat([all8, all8.new_zeros(1, cout)])[self.up]

    def up_loop(self, f, w):
        out = f.new_zeros(self.Rf, w.shape[2])
        for t, (j, i) in enumerate(self.pairs):
            if j.numel():
                out = out.index_add(0, i, f.index_select(0, j) @ w[t])
        return out


def pair(res, ours, others, what):
    say(AB.fmt(res, ours))
    say(AB.fmt(res, ours + " (again)"))
    for t in others:
        say(AB.fmt(res, t))
    spread = abs(res[ours][0] - res[ours + " (again)"][0]) / res[ours][0]
    best = min(others, key=lambda t: res[t][0])
    ratio = res[ours][0] / res[best][0]
    say(f"  ours / best other route ({best.strip()}) {what}: {ratio:.3f}  {'LOSES' if ratio > 1 else 'wins'}   "
        f"(same against same: {spread:.3f})")


def one_shape(b, n, cf, cc, rounds):
    xyz = SC.sphere(b, n, n + b)
    cell = SC.cell_for_half(xyz)
    info = _raw.grid_cluster(xyz, cell, "z")
    coords, ncl = info["coords"], info["nclusters"]
    level = glue.sparse_stride_map(coords, ncl)
    child, up, nclc = level["child"], level["up"], level["nclusters"]
    Mf, Mc = int(ncl.sum().item()), int(nclc.sum().item())
    say(f"\n## b = {b}, {n} points on a sphere, cell = {cell:.4f}: {Mf} fine cells ({Mf / b:.0f} per sample), {Mc} coarse cells "
        f"({Mf / Mc:.2f} children each), {cf} channels fine, {cc} coarse")
    cells, inverse = torch_map(coords, ncl)
    live_f = torch.arange(n, device="cuda")[None] < ncl[:, None]
    base = torch.cumsum(nclc.long(), 0) - nclc.long()  # the first global coarse rank of each sample
    same = cells.numel() == Mc and torch.equal(inverse, ((up[live_f].long() >> 3) + base[:, None].expand(b, n)[live_f]))
    say(f"  agreement: torch.unique finds {cells.numel()} coarse cells; parents {'equal' if same else 'NOT equal'}")
    assert same
    res = AB.ab({"ours  map": lambda s: glue.sparse_stride_map(coords, ncl), "ours  map (again)": lambda s: glue.sparse_stride_map(coords, ncl),
                 "torch map (unique)": lambda s: torch_map(coords, ncl)}, rounds)
    pair(res, "ours  map", ["torch map (unique)"], "map")

    g = torch.Generator(device="cuda").manual_seed(1)
    ff = [torch.randn(b, n, cf, device="cuda", generator=g) for _ in range(2)]   # fine features / gradients
    fc = [torch.randn(b, n, cc, device="cuda", generator=g) for _ in range(2)]   # coarse (n_coarse = n rows)
    wd = torch.randn(8, cf, cc, device="cuda", generator=g) / (8 * cf) ** 0.5
    wu = torch.randn(8, cc, cf, device="cuda", generator=g) / (8 * cc) ** 0.5
    T = TorchRoutes(level, ncl, n)
    cff, cfc = [T.fine(x) for x in ff], [T.coarse(x) for x in fc]
    # the expansion of up for the gather kernel: E[i][t] = parent where up[i] = 8 parent + t
    slot = torch.arange(8, device="cuda", dtype=torch.int32)
    E = torch.where((up[..., None] >= 0) & ((up[..., None] & 7) == slot), up[..., None] >> 3, -1).contiguous()
    down = lambda f, w: glue.sparse_conv_down(f, w, level, ncl)  # noqa: E731
    upc = lambda f, w: glue.sparse_conv_up(f, w, level, ncl)  # noqa: E731
    up_gather = lambda f, w: _raw.sparse_conv_strided(f, w, E, up, nclc, ncl, "down")  # noqa: E731  (rows out: fine; source: coarse)
    dgi = lambda gr, w: _raw.sparse_conv_strided(gr, w, child, up, ncl, nclc, "down_grad_input")  # noqa: E731
    dgi_gather = lambda gr, w: _raw.sparse_conv_strided(gr, w.transpose(1, 2).contiguous(), E, up, nclc, ncl, "down")  # noqa: E731
    o, a, lp = T.coarse(down(ff[0], wd)), T.down_im2col(cff[0], wd), T.down_loop(cff[0], wd)
    say(f"  agreement down: ours - im2col {float((o - a).abs().max() / a.abs().max()):.1e}, loop - im2col {float((lp - a).abs().max() / a.abs().max()):.1e}")
    o, a, lp = T.fine(upc(fc[0], wu)), T.up_im2col(cfc[0], wu), T.up_loop(cfc[0], wu)
    say(f"  agreement up: ours - im2col {float((o - a).abs().max() / a.abs().max()):.1e}, loop - im2col {float((lp - a).abs().max() / a.abs().max()):.1e}; "
        f"fan-out and gather kernel bit for bit: up {torch.equal(upc(fc[0], wu), up_gather(fc[0], wu))}, "
        f"down_grad_input {torch.equal(dgi(fc[0], wd), dgi_gather(fc[0], wd))}")
    go, ga = SC.fwdbwd(down, ff[0], wd, fc[0]), SC.fwdbwd(T.down_im2col, cff[0], wd, cfc[0])
    say(f"  gradients down: feat {float((T.fine(go[0]) - ga[0]).abs().max() / ga[0].abs().max()):.1e}, "
        f"weight {float((go[1] - ga[1]).abs().max() / ga[1].abs().max()):.1e}")
    go, ga = SC.fwdbwd(upc, fc[0], wu, ff[0]), SC.fwdbwd(T.up_im2col, cfc[0], wu, cff[0])
    say(f"  gradients up: feat {float((T.coarse(go[0]) - ga[0]).abs().max() / ga[0].abs().max()):.1e}, "
        f"weight {float((go[1] - ga[1]).abs().max() / ga[1].abs().max()):.1e}")
    del o, a, lp, go, ga
    routes = {"ours  down": lambda s: down(ff[s], wd), "ours  down (again)": lambda s: down(ff[s], wd),
              "torch down im2col": lambda s: T.down_im2col(cff[s], wd), "torch down loop": lambda s: T.down_loop(cff[s], wd),
              "ours  up": lambda s: upc(fc[s], wu), "ours  up (again)": lambda s: upc(fc[s], wu),
              "gather up": lambda s: up_gather(fc[s], wu),
              "torch up im2col": lambda s: T.up_im2col(cfc[s], wu), "torch up loop": lambda s: T.up_loop(cfc[s], wu),
              "ours  down_grad_input": lambda s: dgi(fc[s], wd), "ours  down_grad_input (again)": lambda s: dgi(fc[s], wd),
              "gather down_grad_input": lambda s: dgi_gather(fc[s], wd)}
    res = AB.ab(routes, rounds)
    pair(res, "ours  down", ["torch down im2col", "torch down loop"], f"down {cf} -> {cc}")
    pair(res, "ours  up", ["torch up im2col", "torch up loop"], f"up {cc} -> {cf}")
    pair(res, "ours  up", ["gather up"], "up, fan-out against gather kernel")
    pair(res, "ours  down_grad_input", ["gather down_grad_input"], "down_grad_input, fan-out against gather kernel")
    routes = {"ours  down fwd+bwd": lambda s: SC.fwdbwd(down, ff[s], wd, fc[s]), "ours  down fwd+bwd (again)": lambda s: SC.fwdbwd(down, ff[s], wd, fc[s]),
              "torch down fwd+bwd im2col": lambda s: SC.fwdbwd(T.down_im2col, cff[s], wd, cfc[s]),
              "torch down fwd+bwd loop": lambda s: SC.fwdbwd(T.down_loop, cff[s], wd, cfc[s]),
              "ours  up fwd+bwd": lambda s: SC.fwdbwd(upc, fc[s], wu, ff[s]), "ours  up fwd+bwd (again)": lambda s: SC.fwdbwd(upc, fc[s], wu, ff[s]),
              "torch up fwd+bwd im2col": lambda s: SC.fwdbwd(T.up_im2col, cfc[s], wu, cff[s]),
              "torch up fwd+bwd loop": lambda s: SC.fwdbwd(T.up_loop, cfc[s], wu, cff[s])}
    res = AB.ab(routes, rounds)
    pair(res, "ours  down fwd+bwd", ["torch down fwd+bwd im2col", "torch down fwd+bwd loop"], "down fwd+bwd")
    pair(res, "ours  up fwd+bwd", ["torch up fwd+bwd im2col", "torch up fwd+bwd loop"], "up fwd+bwd")
    say(f"  kernels ours, down fwd+bwd (ms per call) {AB.kernels(routes['ours  down fwd+bwd'])}")
    say(f"  kernels ours, up fwd+bwd (ms per call) {AB.kernels(routes['ours  up fwd+bwd'])}")


def main():
    global OUT
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    AB.OUT = OUT
    torch.cuda.init()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    say(f"# strided sparse convolution A/B on {torch.cuda.get_device_name(0)}: alternating rounds, ms per call, medians with min and max")
    say("# ours = rf_sparse_stride_map, rf_sparse_conv_strided, rf_sparse_conv_strided_grad_weight ; torch = int64 keys + torch.unique "
        "for the map, im2col (one mm) and the per-slot loop (index_select, mm, index_add) with autograd ; gather = the fan-out modes "
        "through the gather kernel on an expansion of up ; '(again)' = the same route a second time: the same-against-same spread")
    for shape in SHAPES:
        one_shape(*shape, rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
