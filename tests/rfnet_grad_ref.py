"""TEST INFRASTRUCTURE ONLY -- torch restatement of RFNetOracle.forward and RFNetOracle.training_loss
(oracle/rfnet_oracle.py), statement by statement, so that autograd differentiates the whole training step: the
reference of tests/test_gpu_rfnet_grad.py, checked on the CPU by tests/test_rfnet_grad_ref_host.py.  Imports nothing
from rfnet_amd.

Generic in dtype: float64 is the reference; float32 only measures what fp32 arithmetic does to these gradients (the
noise floor of the GPU test).  Runs on the CPU.  Variables come in as the oracle takes them, {tf variable name:
array} (net.tf_state_dict()), and every name is ONE leaf tensor: a kernel shared between the applications of `cell` /
`decode_cell` is one leaf used several times, whose uses autograd sums; the biases are fresh per application.

Discrete and non-differentiated quantities are INPUTS (`choices`), held constant as the reference's TF graph holds
them:
  fps32 (B, 32), merge1 (B, 64), merge2 (B, 1024), merge3 (B, 16384)     indices into the sample's own raw cloud
  gt_fps64 (B, 64), gt_fps1024 (B, 1024)                                 FPS of gt
  cd3, cd4: (idx1, idx2) of nn_distance(gt, points3 / points_final)
  recd3: (idx1, idx2) of nn_distance(points3 slices, gt slices), (8 B, 2048) each, slice i of sample s at s * 8 + i
  zg1: idx2 of nn_distance(gt1, gt2) (B, 1024);  zg2: idx2 of nn_distance(gt2, gt) (B, 16384)
  match1 (B, 64, 64), match2 (B, 1024, 1024): approx_match(gt1 / gt2, points1_pre / points2_pre); approx_match has
      no gradient in the reference, match_cost has.
With the indices given a Chamfer term is a gather plus a squared norm: no N x M matrix is formed.

A ragged batch is a LIST of per-sample clouds (n_i, 3): the forward runs per sample at B = 1 on the sample's own
slice, the outputs are stacked and the loss block runs on the stack.  There is no masking logic here.

`mutate` selects one deliberate error (MUTATIONS), for the host test that shows each class of error is visible above
the GPU test's bar.

Kinks.  The loss is piecewise smooth, and at a ReLU unit whose pre-activation is zero the gradient jumps.  Where the
float64 pre-activation of a unit lies within fp32 rounding of zero, two correct fp32 forwards land on different sides
and return the two one-sided gradients, which differ by a finite amount however small the rounding: in a layer of R
rows the unit is one of R terms of a column sum (a unit of refine_layer1/feat_refine1, 64 rows, at +1.4e-8 moves that
layer's weight gradient by 3.7 % of its maximum: profiles/rfnet_grad_ref.txt).  No bar is widened for that.  `probe`
records the pre-activations of the layers of at most KINK_ROWS rows, `kink_units` names the units an fp32 forward may
put on either side, `flip` runs the reference with such units on the other side, and `one_sided_reference` returns the
one-sided float64 gradient nearest to a given result: a result that misses the bar against the reference is compared,
under the same bar, with that gradient -- exact for the same loss at the same point -- and with nothing else."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MUTATIONS = ("shared_first_only",  # a shared kernel's gradient counted for its first application only
             "recd3_weight",       # the 0.2 on recd3 applied to the value, not to the gradient
             "hinge_open",         # zero_groupnear's relu passes gradient when it is clamped
             "sqrt_swap")          # the two Chamfer directions' 0.5 / sqrt(d) factors exchanged
TERMS = ("cd1", "cd2", "cd3", "cd4", "recd3", "moveloss", "loss_d1", "loss_d2", "loss_dec", "loss")
OUTPUTS = ("points1", "points2", "points3", "points_final", "points1_pre", "points2_pre", "refinemove3",
           "decode_move64", "decode_move1024")
FACTOR = 8.0  # the GPU test's bar: FACTOR x the float32 run's own error against the float64 run
KINK_ROWS = 128  # layers of at most this many rows are probed for units on a kink: the 32- and 64-point stages, the
#                 one-row code words and states, a raw cloud of up to 128 points


def is_dead(name):
    """The variables full_process leaves without a path to the loss (tf names): the feat_refine branch of
    refine_layer_final (6) and the second decode_cell's state biases (2 + 32); test_forward_backward_on_hip_ops."""
    return "refine_layer_final/feat_refine" in name or (name.startswith("decode_cell_1/state") and "state_trans" not in name)


def tf_name(param_name):
    """RFNet.named_parameters() name -> tf variable name."""
    kind, _, key = param_name.partition(".")
    if not key:
        return param_name
    return key.replace("__", "/") + ("/weights" if kind == "weights" else "/Variable")


def _value_with_gradient_of(value, carrier):
    """`value`'s number with `carrier`'s derivative."""
    return carrier + (value - carrier).detach()


def _act(x, act):
    if act == "relu":
        return torch.relu(x)
    if act == "tanh":
        return torch.tanh(x)
    if act == "leaky_relu":  # tf.nn.leaky_relu default alpha = 0.2
        return torch.where(x > 0, x, 0.2 * x)
    return x


def _take(x, idx):
    """np.take_along_axis(x, idx[..., None], 1) for x (B, N, C), idx (B, M)."""
    idx = torch.as_tensor(np.asarray(idx, np.int64))
    return torch.gather(x, 1, idx.unsqueeze(-1).expand(-1, -1, x.shape[-1]))


def _rep(x, n):
    return x.expand(-1, n, -1)


class _Graph:
    def __init__(self, leaves, mutate, flip=None, probe=None):
        self.p = leaves
        self.mutate = mutate
        self.flip, self.probe, self.sample = flip or {}, probe, 0

    def conv(self, scope, name, x, act="relu", call=0):
        base = f"{scope}/{name}" if scope else name
        sc = scope if call == 0 else f"{scope}_{call}"
        bname = f"{sc}/{name}" if sc else name
        w = self.p[base + "/weights"][0, 0]
        if self.mutate == "shared_first_only" and call > 0:
            w = w.detach()
        b = self.p[bname + "/Variable"]
        assert x.shape[-1] == w.shape[0], (base, tuple(x.shape), tuple(w.shape))
        pre = x @ w + b
        if act in ("relu", "leaky_relu") and x.shape[1] <= KINK_ROWS:
            key = (scope, name, call, self.sample)
            if self.probe is not None:
                self.probe[key] = pre.detach().double().numpy()
            if key in self.flip:  # the other one-sided derivative of these units (their value is ~0 on both sides)
                on = (pre > 0).reshape(-1)
                idx = torch.as_tensor(np.asarray(self.flip[key], np.int64))
                on[idx] = ~on[idx]
                return torch.where(on.reshape(pre.shape), pre, (0.2 if act == "leaky_relu" else 0.0) * pre)
        return _act(pre, act)

    def global_mlp(self, scope, xyz, mlp):
        t = xyz
        for i, _ in enumerate(mlp):
            t = self.conv(scope, f"ini_layer{i}", t)
        return t.max(dim=1, keepdim=True).values

    def encode_cell(self, input_tensor, state_tensor, call, mlp=(256, 384), mlpout=(256, 256)):
        n = input_tensor.shape[1]
        new_state = torch.cat([input_tensor, _rep(state_tensor, n)], -1)
        for i, _ in enumerate(mlp):
            new_state = self.conv("cell", f"state{i}", new_state, call=call)
        new_state = self.conv("cell", "state_end", new_state, call=call).max(dim=1, keepdim=True).values
        codeout = new_state
        for i, _ in enumerate(mlpout):
            codeout = self.conv("cell", f"codemlp{i}", codeout, call=call)
        return codeout, new_state

    def recover_cell(self, scope, input_tensor, con_tensor, mlp2=(256, 256)):
        n = con_tensor.shape[1]
        t = torch.cat([_rep(input_tensor, n), con_tensor], -1)
        i = 0
        for i, _ in enumerate(mlp2):
            t = self.conv(scope, f"recover2{i}", t)
        t = t.max(dim=1, keepdim=True).values
        return self.conv(scope, f"recover2out{i}", t, act=None)

    def merge_layer(self, rawpts, newpts, decfactor, idx2):
        grouped = _take(rawpts, idx2)
        diff = grouped - newpts
        dismat = (diff * diff).sum(-1, keepdim=True)
        ratio = torch.exp(-dismat / (1e-8 + decfactor ** 2))
        return newpts + ratio * diff

    def init_move_layer(self, startpts, codeword, mlp=(256, 256, 256), mlp1=(256, 128), mlp2=(256, 128, 64)):
        n = startpts.shape[1]
        tensor1 = torch.cat([startpts, _rep(codeword.reshape(-1, 1, codeword.shape[-1]), n)], -1)
        t = tensor1
        for i, _ in enumerate(mlp):
            t = self.conv("", f"ini_layer{i}", t)
        t = torch.cat([tensor1, _rep(t.max(dim=1, keepdim=True).values, n)], -1)
        outfeats = t
        for i, _ in enumerate(mlp1):
            outfeats = self.conv("", f"ini_featout{i}", outfeats)
        outfeats = self.conv("", "inimove_featout", outfeats)
        for i, _ in enumerate(mlp2):
            t = self.conv("", f"ini_ptsout{i}", t)
        outpts = startpts + self.conv("", "inimove_ptsout", t, act="tanh")
        return outpts, outfeats

    def feat_trans(self, feat, mlp=(256, 256)):
        for i, _ in enumerate(mlp):
            feat = self.conv("", f"partfeat{i}", feat)
        return feat

    def init_decode_layer(self, input_tensor, ptnum=32, mlp=(256, 256), mlp2=(256, 256)):
        sc = "init_cell"
        new_state = self.conv(sc, "input_trans", input_tensor)
        for i, _ in enumerate(mlp):
            new_state = self.conv(sc, f"basic_state{i}", new_state)
        po = self.conv(sc, "points_out", new_state, act=None)
        transmat = po[..., -12:-3].reshape(-1, 3, 3)
        movemat = po[..., -3:].reshape(-1, 1, 3)
        pts = torch.tanh(po[..., :-12]).reshape(-1, ptnum, 3)
        pts = pts @ transmat + movemat
        so = self.conv(sc, "state_out", new_state).reshape(-1, ptnum, 16)
        so = torch.cat([so, _rep(new_state, ptnum)], -1)
        for i, _ in enumerate(mlp2):
            so = self.conv(sc, f"state{i}", so)
        return pts, self.conv(sc, "state_outo", so)

    def refine_layer(self, scope, ptcoor, feat, feat2, mlp=(128, 64, 64), mlp2=(128, 128), mlpself=(128, 128)):
        n = ptcoor.shape[1]
        t = torch.cat([ptcoor, _rep(feat, n)], -1)
        for i, _ in enumerate(mlpself):
            t = self.conv(scope, f"ini_layer{i}", t)
        t = torch.cat([ptcoor, _rep(t.max(dim=1, keepdim=True).values, n)], -1)
        for i, _ in enumerate(mlp):
            t = self.conv(scope, f"refine_layers{i}", t)
        newvec = self.conv(scope, "refine_layer_final", t, act="tanh")
        newcoor = newvec + ptcoor
        t = torch.cat([newcoor, feat2, _rep(feat, feat2.shape[1])], -1)
        for i, _ in enumerate(mlp2):
            t = self.conv(scope, f"feat_refine{i}", t)
        newfeat = self.conv(scope, "feat_refine_final", t, act="tanh")
        return newcoor, newfeat + feat2, newvec

    def decode_cell(self, input_tensor, center, state_tensor, call, up_ratio=16, mlp=(256, 256), mlp1=(128, 64),
                    mlp2=(128, 128), mlp_mask=(128, 128), mlp_expand=(128,)):
        sc = "decode_cell"
        n = state_tensor.shape[1]
        mask = torch.cat([center, _rep(input_tensor, n)], -1)
        for i, _ in enumerate(mlp_mask):
            mask = self.conv(sc, f"mlp_mask{i}", mask, call=call)
        mask = self.conv(sc, "mask_tensor", mask, call=call)
        input_info = self.conv(sc, "input_trans", mask * input_tensor, call=call)
        state_info = self.conv(sc, "state_trans", state_tensor, call=call)
        new_state = torch.cat([input_info, state_info], -1)
        for i, _ in enumerate(mlp):
            new_state = self.conv(sc, f"basic_state{i}", new_state, call=call)
        po = new_state
        for i, _ in enumerate(mlp1):
            po = self.conv(sc, f"points{i}", po, call=call)
        po = self.conv(sc, "points_out", po, act="tanh", call=call)
        points_move = po.reshape(-1, n, up_ratio, 3)
        points_out = (center[:, :, None, :] + points_move).reshape(-1, n * up_ratio, 3)
        new_state = torch.cat([new_state, _rep(input_tensor, n)], -1)
        for i, _ in enumerate(mlp2):
            new_state = self.conv(sc, f"state{i}", new_state, call=call)
        newnew = new_state
        parts = []
        for i in range(up_ratio):
            for j, _ in enumerate(mlp_expand):
                newnew = self.conv(sc, f"state_expand{i}_{j}", newnew, call=call)
            newnew = self.conv(sc, f"state_expand{i}", newnew, act="leaky_relu", call=call)
            parts.append(newnew)
        state_move = torch.stack(parts, 2)
        new_state = (state_tensor[:, :, None, :] + state_move).reshape(-1, n * up_ratio, state_tensor.shape[-1])
        return points_out, new_state, points_move

    def forward(self, pc, ch):
        """pc (1, n, 3); ch: this sample's fps32 / merge1..3, each (1, k)."""
        state0 = self.global_mlp("init_mlp", pc, (64, 128, 256))
        code1, state = self.encode_cell(pc, state0, 0)
        code1 = self.recover_cell("recover1", code1, pc)
        start = _take(pc, ch["fps32"])
        points1, dstate = self.init_move_layer(start, code1)
        partfeat = self.global_mlp("part_mlp", torch.cat([pc, points1], 1), (64, 128, 256))
        points0, dstate0 = self.init_decode_layer(self.feat_trans(torch.cat([partfeat, code1], -1)))
        points1, dstate = torch.cat([points0, points1], 1), torch.cat([dstate0, dstate], 1)
        points1_pre = points1
        points1 = self.merge_layer(pc, points1, self.p["decline_factor0"][0], ch["merge1"])
        points1, dstate, _ = self.refine_layer("refine_layer1", points1, code1, dstate)

        pin = torch.cat([pc, points1], 1)
        code2, state = self.encode_cell(pin, state, 1)
        code2 = code1 + self.recover_cell("recover2", code2, pin)
        points2, dstate, move64 = self.decode_cell(code2, points1, dstate, 0)
        points2_pre = points2
        points2 = self.merge_layer(pc, points2, self.p["decline_factor1"][0], ch["merge2"])
        points2, dstate, _ = self.refine_layer("refine_layer2", points2, code2, dstate)

        pin = torch.cat([pc, points2], 1)
        code3, state = self.encode_cell(pin, state, 2)
        code3 = code2 + self.recover_cell("recover3", code3, pin)
        points3, dstate, move1024 = self.decode_cell(code3, points2, dstate, 1)
        final = self.merge_layer(pc, points3, self.p["decline_factor"][0], ch["merge3"])
        final, _, refinemove3 = self.refine_layer("refine_layer_final", final, code3, dstate)
        return {"points1": points1, "points2": points2, "points3": points3, "points_final": final,
                "points1_pre": points1_pre, "points2_pre": points2_pre, "refinemove3": refinemove3,
                "decode_move64": move64, "decode_move1024": move1024}

    # ---- the loss block ------------------------------------------------------------------------------------------------
    def chamfer_big(self, pcd1, pcd2, idx):
        """(mean sqrt(d1) + mean sqrt(d2)) / 2, d1[j] = |pcd1[j] - pcd2[idx1[j]]|^2, d2[k] = |pcd2[k] - pcd1[idx2[k]]|^2."""
        d1 = ((pcd1 - _take(pcd2, idx[0])) ** 2).sum(-1)
        d2 = ((pcd2 - _take(pcd1, idx[1])) ** 2).sum(-1)
        value = (torch.sqrt(d1).mean() + torch.sqrt(d2).mean()) / 2
        if self.mutate == "sqrt_swap":
            assert d1.shape == d2.shape
            f1, f2 = (0.5 / torch.sqrt(d2)).detach(), (0.5 / torch.sqrt(d1)).detach()
            return _value_with_gradient_of(value, ((d1 * f1).mean() + (d2 * f2).mean()) / 2)
        return value

    def earth_mover(self, pcd1, pcd2, match):
        """mean_b(sum_kl match[l, k] |pcd2[l] - pcd1[k]| / n): orc.match_cost's distance (tf_approxmatch.cu:183-228), whose
        gradient kernel holds the squared distance at 1e-20 or above."""
        m = torch.as_tensor(np.asarray(match), dtype=pcd1.dtype)                       # (B, m, n)
        d2 = ((pcd2[:, :, None, :] - pcd1[:, None, :, :]) ** 2).sum(-1)                # (B, m, n)
        cost = (torch.sqrt(d2.clamp_min(1e-20)) * m).sum((1, 2))
        return (cost / float(pcd1.shape[1])).mean()

    def re_chamfer(self, gt, pred, idx, part=8):
        b, interval = gt.shape[0], int(gt.shape[1] / 8)
        g = gt[:, :part * interval].reshape(b * part, interval, 3)
        p = pred[:, :part * interval].reshape(b * part, interval, 3)
        # the mean over the slices of chamfer_big's batch means = the mean over all b * part equal-sized slices
        return self.chamfer_big(p, g, idx)

    def zero_groupnear(self, ptcens, rawpts, outmat, idx2):
        dist = ((rawpts - _take(ptcens, idx2)) ** 2).sum(-1)
        outval = (outmat * outmat).sum(-1).mean(-1).mean(-1).mean()
        x = outval - 0.4 * dist.mean()
        if self.mutate == "hinge_open":
            return _value_with_gradient_of(torch.relu(x), x)
        return torch.relu(x)

    def training_loss(self, out, gt, ch, alpha1):
        g = gt
        gt1, gt2 = _take(g, ch["gt_fps64"]), _take(g, ch["gt_fps1024"])
        t = {}
        t["cd1"] = self.earth_mover(gt1, out["points1_pre"], ch["match1"])
        t["cd2"] = self.earth_mover(gt2, out["points2_pre"], ch["match2"])
        t["cd3"] = self.chamfer_big(g, out["points3"], ch["cd3"])
        t["cd4"] = self.chamfer_big(g, out["points_final"], ch["cd4"])
        t["recd3"] = self.re_chamfer(g, out["points3"], ch["recd3"], 8)
        t["moveloss"] = (out["refinemove3"] ** 2).sum(-1).mean()
        t["loss_d1"] = 0.05 * self.zero_groupnear(gt1, gt2, out["decode_move64"], ch["zg1"])
        t["loss_d2"] = 0.05 * self.zero_groupnear(gt2, g, out["decode_move1024"], ch["zg2"])
        t["loss_dec"] = sum(self.p[k][0] ** 2 for k in ("decline_factor0", "decline_factor1", "decline_factor"))
        recd3 = 0.2 * t["recd3"]
        if self.mutate == "recd3_weight":
            recd3 = _value_with_gradient_of(recd3, t["recd3"])
        t["loss"] = (0.2 * (t["cd1"] + t["cd2"]) + t["cd3"] + t["cd4"] + recd3
                     + 0.1 * t["moveloss"] + t["loss_d1"] + t["loss_d2"] + alpha1 * t["loss_dec"])
        return t


def run(variables, clouds, gt, choices, dtype=torch.float64, mutate=None, alpha1=0.01, term="loss", grad=True,
        flip=None, probe=None):
    """variables {tf name: array}; clouds: list of (n_i, 3) arrays (or a (B, n, 3) array); gt (B, 16384, 3); choices as
    the module docstring lists them.  -> {"terms": {name: float}, "out": {name: (B, ., .) float64 array},
    "grads": {tf name: float64 array, or None where `term` does not depend on the variable}, "input_grads": [per sample
    (n_i, 3) float64 array, or None]}: the derivatives of `term` (default: the whole loss).
    probe: a dict that receives {(scope, layer, call, sample): pre-activations} of the ReLU layers of at most KINK_ROWS rows;
    flip: {such a key: flat indices of units whose ReLU mask is inverted} (see Kinks above)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    leaves = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype).requires_grad_(grad) for k, v in variables.items()}
    pcs = [torch.as_tensor(np.asarray(c, np.float64)).to(dtype).reshape(1, -1, 3).requires_grad_(grad) for c in clouds]
    graph = _Graph(leaves, mutate, flip, probe)
    with torch.set_grad_enabled(grad):
        per = []
        for i, pc in enumerate(pcs):
            graph.sample = i
            per.append(graph.forward(pc, {k: np.asarray(choices[k])[i:i + 1] for k in ("fps32", "merge1", "merge2", "merge3")}))
        out = {k: torch.cat([o[k] for o in per], 0) for k in OUTPUTS}
        terms = graph.training_loss(out, torch.as_tensor(np.asarray(gt, np.float64)).to(dtype), choices, alpha1)
    res = {"terms": {k: float(v.detach()) for k, v in terms.items()},
           "out": {k: v.detach().double().numpy() for k, v in out.items()}, "grads": None, "input_grads": None}
    if grad:
        names = list(leaves)
        got = torch.autograd.grad(terms[term], [leaves[k] for k in names] + pcs, allow_unused=True)
        as_np = lambda t: None if t is None else t.double().numpy()
        res["grads"] = {k: as_np(t) for k, t in zip(names, got[:len(names)])}
        res["input_grads"] = [None if t is None else as_np(t)[0] for t in got[len(names):]]
    return res


# ---- the frozen choices, taken with the C operator oracle from fp32 tensors --------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def loss_choices(orc, out, gt):
    """The loss block's choices as RFNetOracle.training_loss takes them: the C oracle's operators on fp32 tensors.
    out: {"points1_pre", "points2_pre", "points3", "points_final"} (B, ., 3); gt (B, 16384, 3)."""
    g = _f32(gt)
    b, interval = g.shape[0], g.shape[1] // 8
    ch = {"gt_fps64": orc.farthest_point_sample(64, g), "gt_fps1024": orc.farthest_point_sample(1024, g)}
    gt1 = np.take_along_axis(g, ch["gt_fps64"][..., None].astype(np.int64), 1)
    gt2 = np.take_along_axis(g, ch["gt_fps1024"][..., None].astype(np.int64), 1)
    p3 = _f32(out["points3"])
    pairs = {"cd3": (g, p3), "cd4": (g, _f32(out["points_final"])),
             "recd3": (p3[:, :8 * interval].reshape(b * 8, interval, 3), g[:, :8 * interval].reshape(b * 8, interval, 3)),
             "zg1": (gt1, gt2), "zg2": (gt2, g)}
    # the sweeps are serial C, independent per batch element and free of shared state: one thread each
    jobs = [(key, i) for key, (a, _) in pairs.items() for i in range(a.shape[0])]
    with ThreadPoolExecutor(max_workers=8) as pool:
        got = list(pool.map(lambda j: orc.nn_distance(np.ascontiguousarray(pairs[j[0]][0][j[1]:j[1] + 1]),
                                                      np.ascontiguousarray(pairs[j[0]][1][j[1]:j[1] + 1])), jobs))
    for key in pairs:
        rows = [r for (k, _), r in zip(jobs, got) if k == key]
        i1, i2 = np.concatenate([r[1] for r in rows]), np.concatenate([r[3] for r in rows])
        ch[key] = i2 if key in ("zg1", "zg2") else (i1, i2)
    ch["match1"] = orc.approx_match(gt1, _f32(out["points1_pre"]))
    ch["match2"] = orc.approx_match(gt2, _f32(out["points2_pre"]))
    return ch


def forward_choices(orc, clouds, out):
    """fps32 and merge1..3 as RFNetOracle.forward takes them from its own tensors (`out`: its result, or any run's
    points1_pre / points2_pre / points3): FPS of the raw cloud, idx2 of nn_distance(raw, generated), per sample."""
    ch = {"fps32": [], "merge1": [], "merge2": [], "merge3": []}
    for i, c in enumerate(clouds):
        pc = _f32(c).reshape(1, -1, 3)
        ch["fps32"].append(orc.farthest_point_sample(32, pc)[0])
        for key, name in (("merge1", "points1_pre"), ("merge2", "points2_pre"), ("merge3", "points3")):
            ch[key].append(orc.nn_distance(pc, _f32(out[name][i:i + 1]))[3][0])
    return {k: np.stack(v) for k, v in ch.items()}


# ---- comparison ------------------------------------------------------------------------------------------------------------
def flat_gradient(res):
    """{name: array} of every gradient that exists, the input clouds' as "input"."""
    g = {k: v for k, v in res["grads"].items() if v is not None}
    g["input"] = np.concatenate([v.reshape(-1) for v in res["input_grads"]])
    return g


def errors(got, ref):
    """got, ref: {name: array} over the same names -> ({name: max |got - ref| / max |ref|}, relative L2 error of the
    concatenated gradient)."""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    err, num, den = {}, 0.0, 0.0
    for k, r in ref.items():
        r = np.asarray(r, np.float64).reshape(-1)
        d = np.asarray(got[k], np.float64).reshape(-1) - r
        err[k] = float(np.abs(d).max() / np.abs(r).max())
        num, den = num + float(d @ d), den + float(r @ r)
    return err, float(np.sqrt(num / den))


def bars(err32, rel32):
    """The bar of the GPU test from the float32 run's own errors against the float64 run: per name FACTOR x
    max(err32[name], median of err32) (the median floors scalars and tiny tensors whose err32 happens to be near zero);
    for the relative L2 error FACTOR x the float32 run's."""
    med = float(np.median(list(err32.values())))
    return {k: FACTOR * max(v, med) for k, v in err32.items()}, FACTOR * rel32


# ---- units on a kink (module docstring, "Kinks") --------------------------------------------------------------------------
def kink_units(probe64, probe32):
    """[(layer key, flat index)] of the probed units whose float64 pre-activation lies within FACTOR x the layer's largest
    |float32 - float64| pre-activation difference of zero: an fp32 forward may put them on either side.  A generous set
    costs no tightness: the units only name the one-sided gradients a result may be compared with."""
    units = []
    for key in sorted(probe64, key=str):
        a = probe64[key].reshape(-1)
        reach = FACTOR * float(np.abs(a - probe32[key].reshape(-1)).max())
        units += [(key, int(i)) for i in np.flatnonzero(np.abs(a) <= reach)]
    return units


def _vector(g):
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in sorted(g)])


def _flip_of(units):
    flip = {}
    for key, i in units:
        flip.setdefault(key, []).append(i)
    return flip


def kink_jumps(variables, clouds, gt, choices, r64, units):
    """[(unit, g(unit flipped) - g as one vector)] in the float64 reference, for the units whose flip moves the gradient at
    all (a unit of a pooled chain that is not the arg-max row of its channel moves nothing; the ~1e-8 by which a flipped
    unit's value changes moves everything by as little)."""
    base = _vector(flat_gradient(r64))
    jumps = []
    for unit in units:
        d = _vector(flat_gradient(run(variables, clouds, gt, choices, flip=_flip_of([unit])))) - base
        if np.sqrt(d @ d) > 1e-6 * np.sqrt(base @ base):
            jumps.append((unit, d))
    return jumps


def choose_flips(jumps, got, r64):
    """The units whose jump vectors, added to the reference gradient, come nearest to `got` in the least-squares sense:
    coefficients of got - g over the jump vectors, rounded to 0 or 1.  Only a proposal: the caller re-runs the reference
    with these units flipped and compares against that gradient, which is exact."""
    if not jumps:
        return []
    d = np.stack([v for _, v in jumps], 1)
    coef = np.linalg.lstsq(d.T @ d, d.T @ (_vector(got) - _vector(flat_gradient(r64))), rcond=None)[0]
    return [unit for (unit, _), c in zip(jumps, coef) if c > 0.5]


def one_sided_reference(variables, clouds, gt, choices, r64, units, got):
    """(the units flipped, the float64 reference run with them flipped): the one-sided gradient of the same loss at the same
    point that lies nearest to `got` among those the units on a kink allow; (none, r64) when no flip brings it nearer."""
    chosen = choose_flips(kink_jumps(variables, clouds, gt, choices, r64, units), got, r64)
    return chosen, (run(variables, clouds, gt, choices, flip=_flip_of(chosen)) if chosen else r64)


def table(err32, bar, err, limit=None):
    """Lines `name err32 bar error error/bar error/err32`, worst error / bar first."""
    rows = sorted(err, key=lambda k: -err[k] / bar[k])[:limit]
    out = [f"{'variable':58s} {'err32':>10s} {'bar':>10s} {'error':>10s} {'err/bar':>8s} {'err/err32':>9s}"]
    for k in rows:
        out.append(f"{k:58s} {err32[k]:10.3e} {bar[k]:10.3e} {err[k]:10.3e} {err[k] / bar[k]:8.3f} "
                   f"{err[k] / max(err32[k], 1e-300):9.2f}")
    return out
