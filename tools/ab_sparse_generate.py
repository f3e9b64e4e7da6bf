"""The decoder entries of the sparse voxel grid against the routes without them, on one GPU (ms per call, device events):
  generate  rf_sparse_generate_map against torch's repeat_interleave + the eight offsets (child and up as aranges under the
            count: the torch route does NOT look for duplicate or out-of-range parents, the kernel does)
  prune     rf_sparse_prune_map + rf_sparse_take_rows at c = 64 (glue.sparse_prune) against cumsum + scatter (no host
            synchronisation, what composes with device counts) and against the boolean mask (coords[keep], feat[keep]: a host
            synchronisation, and compacted over the batch instead of per sample)
  lookup    rf_sparse_lookup at shift 0 and 3 against int64 keys with the batch index folded in + torch.sort of the table +
            torch.searchsorted
  step      one decoder step, forward + backward: generate -> convolution 64 -> 32 -> prune with the features.  ours: the three
            entries and rf_sparse_conv_strided "up" with its two gradients; torch: ONE mm onto all eight slots, the
            repeat_interleave map, cumsum + scatter, autograd
The parents are cells of a sphere's surface (tools/ab_sparse_conv.py's clouds), P per sample, every one of them live; half of the
8 P children, picked at random, are "occupied".  Routes are alternated round by round (the method of tools/ab_grid_pool.py: the
median over the rounds with min and max); every table has ours TWICE, whose difference is the same-against-same spread the other
differences are to be read against.  Before anything is timed the routes are compared.  Every shape is timed in a fresh process
of its own under its own time limit; a shape that fails or runs out of time ends the run.
python tools/ab_sparse_generate.py [rounds] [output file]      (writes profiles/sparse_generate_ab.txt)"""
import os
import subprocess
import sys

ROOT = __file__.rsplit("/", 2)[0]
SHAPES = [(32, 1024), (32, 2048), (1, 1024), (1, 2048)]  # (b, parents per sample)
CIN, COUT, C_MOVE = 64, 32, 64
LIMIT = 240  # seconds per shape
OUT = os.path.join(ROOT, "profiles", "sparse_generate_ab.txt")


def one_shape(b, P, rounds):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ab_grid_pool as AB
    import ab_sparse_conv as SC
    from rfnet_amd import _raw, glue
    AB.OUT = OUT
    say = AB.say

    def pair(res, ours, others, what):
        say(AB.fmt(res, ours))
        say(AB.fmt(res, ours + " (again)"))
        for t in others:
            say(AB.fmt(res, t))
        spread = abs(res[ours][0] - res[ours + " (again)"][0]) / res[ours][0]
        for t in others:
            ratio = res[ours][0] / res[t][0]
            say(f"  ours / {t.strip()} {what}: {ratio:.3f}  {'LOSES' if ratio > 1 else 'wins'}   (same against same: {spread:.3f})")

    torch.cuda.init()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(b + P)
    xyz = SC.sphere(b, 4 * P, b + P)
    info = _raw.grid_cluster(xyz, SC.cell_for_half(xyz), "z")
    assert int(info["nclusters"].min()) >= P
    coords = info["coords"][:, :P].contiguous()  # P distinct cells per sample
    cnt = torch.full((b,), P, dtype=torch.int32, device=dev)
    nf = 8 * P
    gen = glue.sparse_generate_map(coords, cnt)
    say(f"\n## b = {b}, {P} parents per sample on a sphere's surface -> {nf} created cells per sample")

    # ---- generate ----
    off = torch.tensor([[(t >> 2) & 1, (t >> 1) & 1, t & 1] for t in range(8)], dtype=torch.int32, device=dev)

    def torch_generate(c, n_):
        live = (torch.arange(P, device=dev)[None] < n_[:, None])
        fine = (2 * c).repeat_interleave(8, dim=1) + off.repeat(P, 1)[None]
        livef = live.repeat_interleave(8, dim=1)
        ar = torch.arange(nf, device=dev, dtype=torch.int32)[None].expand(b, nf)
        return (torch.where(livef[..., None], fine, 0), 8 * n_, torch.where(live[..., None], ar.reshape(b, P, 8), -1),
                torch.where(livef, ar, -1))
    tg = torch_generate(coords, cnt)
    same = all(torch.equal(x, y) for x, y in zip(tg, (gen["coords"], gen["nclusters"], gen["child"], gen["up"])))
    say(f"  agreement generate: coords, count, child and up {'equal' if same else 'NOT equal'}")
    assert same
    res = AB.ab({"ours  generate": lambda s: glue.sparse_generate_map(coords, cnt),
                 "ours  generate (again)": lambda s: glue.sparse_generate_map(coords, cnt),
                 "torch generate (repeat_interleave)": lambda s: torch_generate(coords, cnt)}, rounds)
    pair(res, "ours  generate", ["torch generate (repeat_interleave)"], "generate map")

    # ---- prune + feature move ----
    fc, fn = gen["coords"], gen["nclusters"]
    keeps = [torch.rand(b, nf, device=dev, generator=g) < 0.5 for _ in range(2)]
    feats = [torch.randn(b, nf, C_MOVE, device=dev, generator=g) for _ in range(2)]
    rows = torch.arange(nf, device=dev)[None].expand(b, nf)

    def torch_prune_scatter(c, keep, n_, feat):
        sel = keep & (rows < n_[:, None])
        rank = torch.cumsum(sel, 1) - 1
        to = torch.where(sel, rank, nf)  # the rows that are dropped go to a spare row
        src = torch.full((b, nf + 1), -1, dtype=torch.int32, device=dev).scatter_(1, to, rows.to(torch.int32))[:, :nf]
        co = torch.zeros(b, nf + 1, 3, dtype=torch.int32, device=dev).scatter_(1, to[..., None].expand(-1, -1, 3), c)[:, :nf]
        fo = feat.new_zeros(b, nf + 1, feat.shape[-1]).scatter(1, to[..., None].expand(-1, -1, feat.shape[-1]), feat)[:, :nf]
        return co, sel.sum(1).to(torch.int32), src, torch.where(sel, rank, -1).to(torch.int32), fo

    def torch_prune_mask(c, keep, n_, feat):
        sel = keep & (rows < n_[:, None])
        return c[sel], sel.sum(1), feat[sel]  # (sizes known on the host: the call synchronised)
    o, t = glue.sparse_prune(fc, keeps[0], feats[0], fn), torch_prune_scatter(fc, keeps[0], fn, feats[0])
    same = all(torch.equal(x, y) for x, y in zip((o["coords"], o["nclusters"], o["src"], o["dst"], o["feat"]), t))
    m = torch_prune_mask(fc, keeps[0], fn, feats[0])
    live_out = rows < o["nclusters"][:, None]
    same_m = torch.equal(o["coords"][live_out], m[0]) and torch.equal(o["feat"][live_out], m[2])
    say(f"  agreement prune: cumsum + scatter {'equal' if same else 'NOT equal'}, boolean mask {'equal' if same_m else 'NOT equal'}; "
        f"{int(o['nclusters'].sum())} of {b * nf} cells kept")
    assert same and same_m
    res = AB.ab({"ours  prune + move": lambda s: glue.sparse_prune(fc, keeps[s], feats[s], fn),
                 "ours  prune + move (again)": lambda s: glue.sparse_prune(fc, keeps[s], feats[s], fn),
                 "torch cumsum + scatter": lambda s: torch_prune_scatter(fc, keeps[s], fn, feats[s]),
                 "torch boolean mask (host sync)": lambda s: torch_prune_mask(fc, keeps[s], fn, feats[s])}, rounds)
    pair(res, "ours  prune + move", ["torch cumsum + scatter", "torch boolean mask (host sync)"], f"prune + move, c = {C_MOVE}")
    say(f"  kernels ours (ms per call) {AB.kernels(lambda s: glue.sparse_prune(fc, keeps[s], feats[s], fn))}")

    # ---- lookup ----
    truth = glue.sparse_prune(fc, keeps[0], None, fn)  # the occupied children: the table at shift 0
    t0, n0 = truth["coords"], truth["nclusters"]
    t3 = (t0 << 3) + torch.randint(0, 8, t0.shape, device=dev, generator=g, dtype=torch.int32)  # cells three levels below

    def key(c, n_):
        k = c.long() + 32768
        k = (torch.arange(b, device=dev)[:, None] << 48) | (k[..., 0] << 32) | (k[..., 1] << 16) | k[..., 2]
        return torch.where(torch.arange(c.shape[1], device=dev)[None] < n_[:, None], k, (1 << 62))

    def torch_lookup(q, qn, table, tn, shift):
        tk, order = torch.sort(key(table >> shift, tn).reshape(-1), stable=True)
        qk = key(q, qn).reshape(-1)
        at = torch.searchsorted(tk, qk).clamp(max=tk.numel() - 1)
        hit = (tk[at] == qk) & (qk < (1 << 62))
        return torch.where(hit, order[at] % table.shape[1], -1).to(torch.int32).reshape(q.shape[:2])
    for shift, table in ((0, t0), (3, t3)):
        o, t = glue.sparse_lookup(fc, table, fn, n0, shift), torch_lookup(fc, fn, table, n0, shift)
        same = torch.equal(o, t) and torch.equal(o >= 0, keeps[0] & (rows < fn[:, None]))
        say(f"  agreement lookup shift {shift}: {'equal' if same else 'NOT equal'}; {int((o >= 0).sum())} of {b * nf} cells found")
        assert same
        res = AB.ab({f"ours  lookup shift {shift}": lambda s: glue.sparse_lookup(fc, table, fn, n0, shift),
                     f"ours  lookup shift {shift} (again)": lambda s: glue.sparse_lookup(fc, table, fn, n0, shift),
                     "torch int64 sort + searchsorted": lambda s: torch_lookup(fc, fn, table, n0, shift)}, rounds)
        pair(res, f"ours  lookup shift {shift}", ["torch int64 sort + searchsorted"], f"lookup, shift {shift}")

    # ---- one decoder step, forward + backward ----
    xs = [torch.randn(b, P, CIN, device=dev, generator=g) for _ in range(2)]
    w = torch.randn(8, CIN, COUT, device=dev, generator=g) / CIN ** 0.5
    gs = [torch.randn(b, nf, COUT, device=dev, generator=g) for _ in range(2)]

    def ours_step(x, wt, keep):
        gn = glue.sparse_generate_map(coords, cnt)
        f = glue.sparse_conv_generate(x, wt, gn, cnt)
        return glue.sparse_prune(gn["coords"], keep, f, gn["nclusters"])["feat"]

    def torch_step(x, wt, keep):
        fine, n_, _, _ = torch_generate(coords, cnt)
        f = (x @ wt.permute(1, 0, 2).reshape(CIN, 8 * COUT)).reshape(b, nf, COUT)
        return torch_prune_scatter(fine, keep, n_, f)[4]

    def fwdbwd(step, s):
        x, wt = xs[s].detach().requires_grad_(), w.detach().requires_grad_()
        step(x, wt, keeps[s]).backward(gs[s])
        return x.grad, wt.grad
    go, gt = fwdbwd(ours_step, 0), fwdbwd(torch_step, 0)
    fo, ft = ours_step(xs[0], w, keeps[0]), torch_step(xs[0], w, keeps[0])
    say(f"  agreement step: forward {float((fo - ft).abs().max() / ft.abs().max()):.1e}, grad feat "
        f"{float((go[0] - gt[0]).abs().max() / gt[0].abs().max()):.1e}, grad weight {float((go[1] - gt[1]).abs().max() / gt[1].abs().max()):.1e}")
    res = AB.ab({"ours  step fwd+bwd": lambda s: fwdbwd(ours_step, s), "ours  step fwd+bwd (again)": lambda s: fwdbwd(ours_step, s),
                 "torch step fwd+bwd": lambda s: fwdbwd(torch_step, s)}, rounds)
    pair(res, "ours  step fwd+bwd", ["torch step fwd+bwd"], f"decoder step {CIN} -> {COUT}, fwd+bwd")
    say(f"  kernels ours, step fwd+bwd (ms per call) {AB.kernels(lambda s: fwdbwd(ours_step, s))}")


def main():
    global OUT
    if len(sys.argv) > 1 and sys.argv[1] == "--shape":  # a child: one shape, appended to the file the parent opened
        OUT = sys.argv[5]
        one_shape(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if len(sys.argv) > 2:
        OUT = os.path.abspath(sys.argv[2])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("# decoder entries of the sparse voxel grid, A/B on one MI355X: alternating rounds, ms per call, medians with min and "
                "max\n# ours = rf_sparse_generate_map, rf_sparse_prune_map + rf_sparse_take_rows, rf_sparse_lookup, "
                "rf_sparse_conv_strided (up) on the generated maps ; torch = repeat_interleave + offsets, cumsum + scatter or the "
                "boolean mask, int64 keys + sort + searchsorted, one mm onto the eight slots with autograd ; '(again)' = the same "
                "route a second time: the same-against-same spread\n")
    for b, P in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(b), str(P), str(rounds), OUT], timeout=LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit(f"b = {b}, {P} parents: no result within {LIMIT} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"b = {b}, {P} parents: ended with status {r.returncode}; nothing further is started")


if __name__ == "__main__":
    main()
