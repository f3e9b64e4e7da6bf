"""RFNet generator graph (`full_process`, vv_recon.py:194-244 and the cells it calls, :84-160,
246-364) on PyTorch-ROCm -- the second "next" row.

Every layer of the reference is a 1x1 convolution over points, i.e. a dense layer on the channel
axis, so tensors are kept as (batch, points, channels) and the GEMMs go to the library
(rocBLAS/hipBLASLt through torch) -- "plain library GEMMs".  The point-cloud operators inside the
graph (FPS + gather in `sampling`, Chamfer + group_point in `merge_layer`) are the HIP ops of this
repository.

What is pinned: the PARAMETER INVENTORY.  `tests/golden/rfnet_variables.json` is the list of
variable names and shapes read out of the reference's checkpoint index
(bestrecord/model-229999.index, with tools/read_tf_index.py -- data only); `RFNet.tf_variables()`
must reproduce it entry for entry, which checks every layer's existence, name, fan-in and fan-out,
and the reference's sharing quirk: `encode_cell` ('cell') is applied three times and `decode_cell`
twice with SHARED kernels (tf.get_variable under reuse=True) but FRESH biases per application
(tf.Variable: `cell/...`, `cell_1/...`, `cell_2/...`, `decode_cell_1/...`).  The checkpoint's weight
blob is absent and TensorFlow cannot run here, so numerical parity of the forward pass with the
reference is NOT established; initialisation follows the reference (Xavier-uniform
kernels, zero biases).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _raw, glue

_MLP3 = [("ini_layer0", 3, 64), ("ini_layer1", 64, 128), ("ini_layer2", 128, 256)]
_RECOVER = [("recover20", 259, 256), ("recover21", 256, 256), ("recover2out1", 256, 256)]
_REFINE = [("ini_layer0", 259, 128), ("ini_layer1", 128, 128), ("refine_layers0", 131, 128),
           ("refine_layers1", 128, 64), ("refine_layers2", 64, 64), ("refine_layer_final", 64, 3),
           ("feat_refine0", 387, 128), ("feat_refine1", 128, 128), ("feat_refine_final", 128, 128)]
_DECODE = ([("mlp_mask0", 259, 128), ("mlp_mask1", 128, 128), ("mask_tensor", 128, 256),
            ("input_trans", 256, 256), ("state_trans", 128, 128), ("basic_state0", 384, 256),
            ("basic_state1", 256, 256), ("points0", 256, 128), ("points1", 128, 64),
            ("points_out", 64, 48), ("state0", 512, 128), ("state1", 128, 128)]
           + [x for i in range(16) for x in ((f"state_expand{i}_0", 128, 128), (f"state_expand{i}", 128, 128))])

# (variable scope, layers (name, fan_in, fan_out), number of applications)
LAYERS = [
    ("init_mlp", _MLP3, 1),
    ("cell", [("state0", 259, 256), ("state1", 256, 384), ("state_end", 384, 256),
              ("codemlp0", 256, 256), ("codemlp1", 256, 256)], 3),
    ("recover1", _RECOVER, 1), ("recover2", _RECOVER, 1), ("recover3", _RECOVER, 1),
    ("", [("ini_layer0", 259, 256), ("ini_layer1", 256, 256), ("ini_layer2", 256, 256),
          ("ini_featout0", 515, 256), ("ini_featout1", 256, 128), ("inimove_featout", 128, 128),
          ("ini_ptsout0", 515, 256), ("ini_ptsout1", 256, 128), ("ini_ptsout2", 128, 64),
          ("inimove_ptsout", 64, 3), ("partfeat0", 512, 256), ("partfeat1", 256, 256)], 1),
    ("part_mlp", _MLP3, 1),
    ("init_cell", [("input_trans", 256, 256), ("basic_state0", 256, 256), ("basic_state1", 256, 256),
                   ("points_out", 256, 108), ("state_out", 256, 512), ("state0", 272, 256),
                   ("state1", 256, 256), ("state_outo", 256, 128)], 1),
    ("refine_layer1", _REFINE, 1), ("refine_layer2", _REFINE, 1), ("refine_layer_final", _REFINE, 1),
    ("decode_cell", _DECODE, 2),
]


def _key(name):
    return name.replace("/", "__")


def _splits(rows):
    """How many batches to cut the row axis of a weight-gradient GEMM into (see _wgrad)."""
    s = 1
    while s < 128 and rows // (2 * s) >= 2048:
        s *= 2
    return s


def _wgrad(x2d, g2d):
    """x2d^T @ g2d for x2d (R, cin), g2d (R, cout): the weight gradient of a per-point dense layer.
    R = batch * points (up to 620 288 here) and the output is tiny, so the library's plain GEMM runs on
    a handful of workgroups, one per output tile, each looping over all R rows (1.3 ms for 128 x 256 at
    R = 524 288).  Cut into S row blocks as ONE strided-batched GEMM plus a sum over the S partial
    products it fills the chip: 0.27 ms (tools/experiments/wgrad_splitk.py; 143 TFLOP/s at 256 x 256)."""
    rows = x2d.shape[0]
    s = _splits(rows) if x2d.is_cuda else 1
    if s == 1:
        return x2d.t() @ g2d
    q = rows // s
    main = s * q
    out = torch.bmm(x2d[:main].view(s, q, -1).transpose(1, 2), g2d[:main].view(s, q, -1)).sum(0)
    if main < rows:
        out = out + x2d[main:].t() @ g2d[main:]
    return out


def _tail_grad(grad, y, act):
    """(g, bias gradient) of a layer tail act(. + b) from the upstream gradient and the layer's OUTPUT y,
    both (rows, c): g = grad * act'(y), bias gradient = column sums of g.  One pass through
    rf_act_grad_colsum (the rows cut into pseudo-samples so that the strip partials fold in parallel)
    instead of an activation-backward kernel plus a sum reduction that reads g again."""
    grad = grad.contiguous()
    rows, c = grad.shape
    if grad.is_cuda and _raw.act_grad_colsum_supported(c) and rows >= 1024:
        nb = 1
        while nb < 64 and rows % (2 * nb) == 0 and rows // (2 * nb) >= 256:
            nb *= 2
        g, sums = _raw.act_grad_colsum(grad.view(nb, rows // nb, c), None if act is None else y.view(nb, rows // nb, c), act)
        return g.view(rows, c), sums.sum(0)
    if act == "relu":
        g = torch.ops.aten.threshold_backward(grad, y, 0.0)
    elif act == "tanh":
        g = grad * (1.0 - y * y)
    elif act == "leaky_relu":
        g = torch.where(y > 0, grad, grad * 0.2)
    else:
        g = grad
    return g, g.sum(0)


class _MaxPool(torch.autograd.Function):
    """max over the points axis with rf_maxpool_points_idx; the backward routes each channel's gradient
    to its arg-max point (zero fill + one scatter).  `lengths`: per-sample row counts of a ragged batch
    (rf_maxpool_points_idx_lengths); every arg-max lies below its sample's count, so the same scatter leaves
    the padded rows at zero."""

    @staticmethod
    def forward(ctx, t, lengths=None):
        out, idx = _raw.maxpool_points_idx(t, lengths)
        ctx.save_for_backward(idx)
        ctx.n = t.shape[1]
        return out

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        b, _, c = grad.shape
        gin = grad.new_zeros(b, ctx.n, c)
        gin.scatter_(1, idx.long().unsqueeze(1), grad.contiguous())
        return gin, None


class _PooledChain(torch.autograd.Function):
    """maxpool_points(fn(*tensors)) for a per-point MLP chain `fn` whose output feeds ONLY the pooling
    (global_mlp, encode_cell, recover_cell, the first half of refine_layer: vv_recon.py:84-131,273-286).
    The pooled gradient reaches at most C rows per sample -- row idx[b, c] for channel c -- out of up to
    19 384, and every layer of the chain acts row by row, so the WHOLE chain's backward lives on those
    rows: it is recomputed on the (B, C, .) gather of the per-point inputs and differentiated there
    (the diagonal of the recomputed (B, C, C) block is the pooled output).  Same derivative as the dense
    backward -- which multiplies (B, N, C) matrices that are zero outside those rows: at C5 size 75 % of
    the step's backward GEMM flops plus the activation-gradient and zero-fill passes over them -- and the
    (B, N, C) activations of the chain are not kept for the backward at all.
    `lengths`: per-sample row counts of a ragged batch; the arg-max rows then lie below each sample's count
    and the backward, which lives on those rows, is unchanged."""

    @staticmethod
    def forward(ctx, fn, nparams, lengths, *args):
        # args = the chain's parameters (the module's own Parameter objects: `fn` reads them from the
        # module; they are inputs here so that autograd accumulates their gradients), then its tensors
        tensors = args[nparams:]
        with torch.no_grad():
            t = fn(*tensors)
            out, idx = _raw.maxpool_points_idx(t, lengths)
        ctx.fn, ctx.params, ctx.n = fn, args[:nparams], t.shape[1]
        # the backward RE-RUNS fn, which reads the module's CURRENT weights: their versions are recorded
        # so that an in-place update between forward and backward (two forwards, an optimizer step, then
        # the first one's backward) raises instead of silently differentiating other weights
        ctx.versions = tuple(p._version for p in ctx.params)
        ctx.save_for_backward(idx, *tensors)
        return out

    @staticmethod
    def backward(ctx, grad):
        idx, *tensors = ctx.saved_tensors
        if tuple(p._version for p in ctx.params) != ctx.versions:
            raise RuntimeError("_PooledChain: a parameter of the chain was modified in place between this forward "
                               "and its backward (the backward recomputes the chain from the current weights)")
        ix = idx.long()  # (B, C): the arg-max row of every channel
        np_ = len(ctx.params)
        need_p, need_t = ctx.needs_input_grad[3:3 + np_], ctx.needs_input_grad[3 + np_:]
        with torch.enable_grad():
            leaves, rows = [], []
            for t, nd in zip(tensors, need_t):
                d = t.detach().requires_grad_(nd)
                leaves.append(d)
                per_point = d.dim() == 3 and d.shape[1] == ctx.n and ctx.n > 1
                rows.append(torch.gather(d, 1, ix.unsqueeze(-1).expand(-1, -1, d.shape[-1])) if per_point else d)
            block = ctx.fn(*rows)                               # (B, C, C)
            pooled = torch.diagonal(block, dim1=1, dim2=2)      # (B, C) = the pooled output
            wanted = [p for p, nd in zip(ctx.params, need_p) if nd] + [d for d, nd in zip(leaves, need_t) if nd]
            got = iter(torch.autograd.grad(pooled, wanted, grad.reshape(pooled.shape), allow_unused=True))
        gp = tuple(next(got) if nd else None for nd in need_p)
        gt = tuple(next(got) if nd else None for nd in need_t)
        return (None, None, None) + gp + gt


class _MatW(torch.autograd.Function):
    """x @ w for per-point features x (..., cin) and a layer kernel w (cin, cout); torch's own matmul
    with the weight gradient computed by _wgrad."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return x @ w

    @staticmethod
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        grad = grad.contiguous()
        gx = grad @ w.t() if ctx.needs_input_grad[0] else None
        gw = _wgrad(x.reshape(-1, x.shape[-1]), grad.reshape(-1, grad.shape[-1])) if ctx.needs_input_grad[1] else None
        return gx, gw


def matw(x, w):
    if x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad):
        return _MatW.apply(x, w)
    return x @ w


class _LinearRelu(torch.autograd.Function):
    """relu(x @ W + b) as ONE library GEMM with a bias + ReLU epilogue (hipBLASLt through
    torch._addmm_activation): the activation costs no extra pass over the (points, channels) output.
    torch ships no derivative for that op, hence this Function (mask from the saved output)."""

    @staticmethod
    def forward(ctx, x2d, w, b):
        y = torch._addmm_activation(b, x2d, w)
        ctx.save_for_backward(x2d, w, y)
        return y

    @staticmethod
    def backward(ctx, grad):
        x2d, w, y = ctx.saved_tensors
        g, gb = _tail_grad(grad, y, "relu")
        return g @ w.t(), _wgrad(x2d, g), gb


class _LinearAct(torch.autograd.Function):
    """act(x @ W + b) for the layers that do not end in a ReLU (none / tanh / leaky_relu 0.2): library
    GEMM with the bias folded in (addmm) + the activation; backward as _LinearRelu's."""

    @staticmethod
    def forward(ctx, x2d, w, b, act):
        y = torch.addmm(b, x2d, w)
        if act == "tanh":
            y.tanh_()
        elif act == "leaky_relu":
            F.leaky_relu(y, 0.2, inplace=True)
        ctx.act = act
        ctx.save_for_backward(x2d, w, y)
        return y

    @staticmethod
    def backward(ctx, grad):
        x2d, w, y = ctx.saved_tensors
        g, gb = _tail_grad(grad, y, ctx.act)
        return g @ w.t(), _wgrad(x2d, g), gb, None


class _PointAffine(torch.autograd.Function):
    """act(y + p @ w + r) through rf_point_affine (one pass); backward with tensor ops."""

    @staticmethod
    def forward(ctx, y, p, w, r, act):
        out = _raw.point_affine(y, p, w, r, act)
        ctx.act = act
        ctx.has = (y is not None, p is not None)
        ctx.rshape = r.shape
        ctx.save_for_backward(out, p if p is not None else out.new_empty(0), w if w is not None else out.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, grad):
        out, p, w = ctx.saved_tensors
        g, sums = _raw.act_grad_colsum(grad, None if ctx.act is None else out, ctx.act)  # (b,n,c), (b,c)
        gy = g if ctx.has[0] else None
        gp = gw = None
        if ctx.has[1]:
            gp = g @ w.t()
            gw = _wgrad(p.reshape(-1, p.shape[-1]), g.reshape(-1, g.shape[-1]))
        gr = sums if len(ctx.rshape) > 1 else sums.sum(0)
        return gy, gp, gw, gr.reshape(ctx.rshape), None


def maxpool_points(t, lengths=None):
    """max over the points axis, keepdim (tf.reduce_max(axis=1), e.g. vv_recon.py:90,107,129).  Without
    autograd: rf_maxpool_points (values only); with autograd: rf_maxpool_points_idx and an index-scatter
    backward (one pass, as torch's `max`, instead of amax's compare / count / divide / multiply; every
    pooled tensor of the graph comes out of a ReLU, so how ties share the gradient is immaterial: tied
    entries are zeros, whose ReLU passes no gradient).  torch's own max reduction takes 0.14 ms per call
    at 32 x 16384 x 256 against 0.03 ms here.  `lengths`: per-sample row counts of a ragged batch -- sample i
    pools t[i, :lengths[i]]; only the library's kernels do that (a tensor they cannot take is an error)."""
    own = t.is_cuda and t.dtype == torch.float32 and t.shape[-1] % 4 == 0 and t.shape[-1] <= 1024 and t.shape[1] > 0
    if lengths is not None:
        if not own:
            raise ValueError("maxpool_points: lengths need a float32 GPU tensor with a multiple of 4 (<= 1024) channels")
        if torch.is_grad_enabled() and t.requires_grad:
            return _MaxPool.apply(t, lengths)
        return _raw.maxpool_points(t, lengths)
    if torch.is_grad_enabled() and t.requires_grad:
        return _MaxPool.apply(t) if own else t.max(1, keepdim=True).values
    if own:
        # this repository's own two-launch kernel: faster than amax, and independent of the ROCm graph replay
        # fault that makes torch reductions go stale inside a captured HIP graph
        return _raw.maxpool_points(t)
    return t.amax(1, keepdim=True)


def linear_relu(x, w, b):
    """relu(x @ w + b) on the last axis; w is (cin, cout) -- the reference's kernel layout."""
    if not x.is_cuda:
        return F.relu(F.linear(x, w.t(), b))
    x2d = x.reshape(-1, x.shape[-1])
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad):
        y = _LinearRelu.apply(x2d, w, b)
    else:
        y = torch._addmm_activation(b, x2d, w)
    return y.reshape(*x.shape[:-1], w.shape[1])


class RFNet(nn.Module):
    """points (B, 3000, 3) -> (points1 (B,64,3), points2 (B,1024,3), points3 (B,16384,3),
    points_final (B,16384,3)), as `full_process`."""

    def __init__(self):
        super().__init__()
        self.weights = nn.ParameterDict()
        self.biases = nn.ParameterDict()
        self._tf_names = {}
        for scope, layers, ncall in LAYERS:
            for name, cin, cout in layers:
                base = f"{scope}/{name}" if scope else name
                w = nn.Parameter(torch.empty(cin, cout))
                nn.init.xavier_uniform_(w)  # tf.contrib.layers.xavier_initializer on [1,1,cin,cout]
                self.weights[_key(base)] = w
                self._tf_names[f"{base}/weights"] = [1, 1, cin, cout]
                for c in range(ncall):
                    # tf.Variable under a re-entered scope lands in a uniquified NAME scope
                    sc = scope if c == 0 else f"{scope}_{c}"
                    bname = f"{sc}/{name}" if sc else name
                    self.biases[_key(bname)] = nn.Parameter(torch.zeros(cout))
                    self._tf_names[f"{bname}/Variable"] = [cout]
        for dn in ("decline_factor0", "decline_factor1", "decline_factor"):
            p = nn.Parameter(torch.empty(1))
            nn.init.uniform_(p, -math.sqrt(3.0), math.sqrt(3.0))  # xavier on shape [1]
            setattr(self, dn, p)
            self._tf_names[dn] = [1]

    def tf_variables(self):
        """{TensorFlow variable name: shape} of this module (checked against the checkpoint index)."""
        return dict(self._tf_names)

    # -- one 1x1 convolution = dense layer on the channel axis -------------------------------
    def d(self, scope, name, x, act="relu", call=0):
        base = f"{scope}/{name}" if scope else name
        sc = scope if call == 0 else f"{scope}_{call}"
        bname = f"{sc}/{name}" if sc else name
        if act == "relu":
            return linear_relu(x, self.weights[_key(base)], self.biases[_key(bname)])
        w, bias = self.weights[_key(base)], self.biases[_key(bname)]
        if x.is_cuda and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or bias.requires_grad):
            return _LinearAct.apply(x.reshape(-1, x.shape[-1]), w, bias, act).reshape(*x.shape[:-1], w.shape[1])
        y = F.linear(x, w.t(), bias)
        if act == "tanh":
            return torch.tanh(y)
        if act == "leaky_relu":
            return F.leaky_relu(y, 0.2)
        return y

    def dcat(self, scope, name, parts, act="relu", call=0):
        """The same dense layer applied to the CONCATENATION of `parts` along the channel axis --
        without building it.  The reference tiles a global code word over all points and concatenates
        it to per-point features before most layers (tf.tile + tf.concat, e.g. vv_recon.py:101,127,
        144,148,280,288,299,317,343): cat([p, tile(g)]) @ W  ==  p @ W[:cp] + (g @ W[cp:]) broadcast.
        A (B,1,C) part costs one row per sample instead of one per point, the (B,N,sum C) tensor is
        never written, and the per-point GEMM shrinks to the channels that really vary per point
        (259 -> 3 for most first layers).  Same weights, same layout: row blocks of the [cin, cout]
        kernel, in concatenation order."""
        base = f"{scope}/{name}" if scope else name
        sc = scope if call == 0 else f"{scope}_{call}"
        bname = f"{sc}/{name}" if sc else name
        w = self.weights[_key(base)]
        bias = self.biases[_key(bname)]
        npts = max(p.shape[1] for p in parts)
        fused = parts[0].is_cuda and w.shape[1] % 4 == 0 and w.shape[1] <= 1024 and act in ("relu", "tanh", None)
        y = r = narrow = wn = None
        row = 0
        for p in parts:
            c = p.shape[-1]
            wp = w[row:row + c]
            row += c
            if p.shape[1] == 1 and npts > 1:          # a tiled (global) part: one row per sample
                t = p @ wp
                r = t if r is None else r + t
            elif fused and c <= 16 and narrow is None:  # the coordinates: applied inside the fused tail
                narrow, wn = p, wp
            elif y is None:                             # wide per-point parts: library GEMMs, accumulated
                y = matw(p, wp)
            elif torch.is_grad_enabled() and (p.requires_grad or wp.requires_grad):
                y = y + matw(p, wp)
            else:
                y = torch.baddbmm(y, p, wp.unsqueeze(0).expand(p.shape[0], -1, -1)) if p.dim() == 3 else y + p @ wp
        assert row == w.shape[0], (base, row, tuple(w.shape))
        r = bias if r is None else r + bias
        if fused and (y is not None or narrow is not None) and npts > 1:
            return _PointAffine.apply(y, narrow, wn, r, act)
        # small or CPU case: plain tensor ops
        acc = r
        for t in (y, None if narrow is None else narrow @ wn):
            if t is not None:
                acc = acc + t
        if act == "relu":
            return F.relu(acc)
        if act == "tanh":
            return torch.tanh(acc)
        return acc

    # chains that feed only a max-pool: dense forward, row-sparse backward (_PooledChain)
    sparse_pool_backward = True

    def pooled(self, fn, layers, *tensors, lengths=None):
        """maxpool_points(fn(*tensors)); `layers` = [(scope, name, call)] the chain applies; `lengths`: per-sample
        row counts of the per-point tensors in a ragged batch (the pooling skips the rows behind them).
        The row-sparse backward (_PooledChain) sends each channel's pooled gradient to ONE arg-max row, as
        torch's `max` does; every chain routed here ENDS IN A ReLU (ties are zeros, whose derivative is
        zero on every tied row, so the choice of row cannot matter) -- a chain ending otherwise must use
        the dense path (`sparse_pool_backward = False`)."""
        ps = []
        for scope, name, call in layers:
            base = f"{scope}/{name}" if scope else name
            sc = scope if call == 0 else f"{scope}_{call}"
            ps += [self.weights[_key(base)], self.biases[_key(f"{sc}/{name}" if sc else name)]]
        npts = max(t.shape[1] for t in tensors)
        cout = ps[-1].shape[0]
        if (self.sparse_pool_backward and torch.is_grad_enabled() and tensors[0].is_cuda and npts > 2 * cout
                and cout % 4 == 0 and cout <= 1024 and any(t.requires_grad for t in list(tensors) + ps)):
            return _PooledChain.apply(fn, len(ps), lengths, *ps, *tensors)
        return maxpool_points(fn(*tensors), lengths)

    def mlp(self, scope, prefix, n, x, call=0, first=0):
        for i in range(first, n):
            x = self.d(scope, f"{prefix}{i}", x, call=call)
        return x

    # -- cells ---------------------------------------------------------------------------------
    def global_mlp(self, scope, xyz, lengths=None):  # vv_recon.py:84-91
        return self.pooled(lambda x: self.mlp(scope, "ini_layer", 3, x),
                           [(scope, f"ini_layer{i}", 0) for i in range(3)], xyz, lengths=lengths)

    def encode_cell(self, x, state, call, lengths=None):  # :93-112
        def chain(x_, st):
            s = self.dcat("cell", "state0", [x_, st], call=call)
            s = self.mlp("cell", "state", 2, s, call, first=1)
            return self.d("cell", "state_end", s, call=call)
        new_state = self.pooled(chain, [("cell", n, call) for n in ("state0", "state1", "state_end")], x, state,
                                lengths=lengths)
        return self.mlp("cell", "codemlp", 2, new_state, call), new_state

    def recover_cell(self, scope, code, con, lengths=None):  # :124-131
        t = self.pooled(lambda cd, cn: self.mlp(scope, "recover2", 2, self.dcat(scope, "recover20", [cd, cn]), first=1),
                        [(scope, "recover20", 0), (scope, "recover21", 0)], code, con, lengths=lengths)
        return self.d(scope, "recover2out1", t, act=None)

    def init_move_layer(self, startpts, codeword):  # :140-159
        t = self.dcat("", "ini_layer0", [startpts, codeword])
        t = self.mlp("", "ini_layer", 3, t, first=1)
        mx = maxpool_points(t)
        feats = self.dcat("", "ini_featout0", [startpts, codeword, mx])
        feats = self.d("", "inimove_featout", self.mlp("", "ini_featout", 2, feats, first=1))
        pts = self.dcat("", "ini_ptsout0", [startpts, codeword, mx])
        pts = self.d("", "inimove_ptsout", self.mlp("", "ini_ptsout", 3, pts, first=1), act="tanh")
        return startpts + pts, feats

    def init_decode_layer(self, x, ptnum=32):  # :246-272 with state_tensor=None
        ns = self.d("init_cell", "input_trans", x)
        ns = self.mlp("init_cell", "basic_state", 2, ns)
        po = self.d("init_cell", "points_out", ns, act=None)  # (B,1,3*ptnum+12)
        transmat = po[..., -12:-3].reshape(-1, 3, 3)
        movemat = po[..., -3:].reshape(-1, 1, 3)
        pts = torch.tanh(po[..., :-12]).reshape(-1, ptnum, 3) @ transmat + movemat
        so = self.d("init_cell", "state_out", ns).reshape(-1, ptnum, 16)
        so = self.dcat("init_cell", "state0", [so, ns])
        so = self.mlp("init_cell", "state", 2, so, first=1)
        return pts, self.d("init_cell", "state_outo", so)

    def refine_layer(self, scope, ptcoor, feat, feat2, collect=None, need_feat=True):  # :273-308
        """need_feat=False: only the refined coordinates are wanted -- `full_process` drops the features
        the LAST refine layer returns (vv_recon.py:238), and a TensorFlow session never executes a branch
        no fetch depends on, so the reference does not run `feat_refine*` there either."""
        n = ptcoor.shape[1]
        mx = self.pooled(lambda pc, ft: self.mlp(scope, "ini_layer", 2, self.dcat(scope, "ini_layer0", [pc, ft]), first=1),
                         [(scope, "ini_layer0", 0), (scope, "ini_layer1", 0)], ptcoor, feat)
        t = self.dcat(scope, "refine_layers0", [ptcoor, mx])
        t = self.mlp(scope, "refine_layers", 3, t, first=1)
        newvec = self.d(scope, "refine_layer_final", t, act="tanh")
        if collect is not None:
            collect[f"{scope}{n}"] = newvec  # tf.add_to_collection(scope+str(ptnum), newvec), :298
        newcoor = ptcoor + newvec
        if not need_feat:
            return newcoor, None
        t = self.dcat(scope, "feat_refine0", [newcoor, feat2, feat])
        t = self.mlp(scope, "feat_refine", 2, t, first=1)
        return newcoor, self.d(scope, "feat_refine_final", t, act="tanh") + feat2

    def decode_cell(self, code, center, state, call, up_ratio=16, collect=None, need_state=True):  # :310-364
        """need_state=False: the expanded state is not wanted (the second application's state only feeds
        the features of the last refine layer, which `full_process` drops: its 34 layers are never
        executed by the reference's session, nor here)."""
        n = state.shape[1]
        sc = "decode_cell"
        mask = self.dcat(sc, "mlp_mask0", [center, code], call=call)
        mask = self.d(sc, "mask_tensor", self.mlp(sc, "mlp_mask", 2, mask, call, first=1), call=call)
        info = self.d(sc, "input_trans", mask * code, call=call)
        ns = self.dcat(sc, "basic_state0", [info, self.d(sc, "state_trans", state, call=call)], call=call)
        ns = self.mlp(sc, "basic_state", 2, ns, call, first=1)
        move = self.d(sc, "points_out", self.mlp(sc, "points", 2, ns, call), act="tanh", call=call)
        if collect is not None:
            collect[f"decode_cell{n}"] = move.reshape(-1, n, up_ratio, 3)  # collection scope+str(ptnum), :338
        pts = (center.unsqueeze(2) + move.reshape(-1, n, up_ratio, 3)).reshape(-1, n * up_ratio, 3)
        if not need_state:
            return pts, None
        ns = self.dcat(sc, "state0", [ns, code], call=call)
        ns = self.mlp(sc, "state", 2, ns, call, first=1)
        parts, cur = [], ns
        for i in range(up_ratio):  # a CHAIN: expansion i feeds expansion i+1
            cur = self.d(sc, f"state_expand{i}_0", cur, call=call)
            cur = self.d(sc, f"state_expand{i}", cur, act="leaky_relu", call=call)
            parts.append(cur)
        move_state = torch.stack(parts, 2)  # (B, n, up_ratio, 128)
        return pts, (state.unsqueeze(2) + move_state).reshape(-1, n * up_ratio, state.shape[-1])

    # -- the graph -------------------------------------------------------------------------------
    def forward(self, pointcloud, collect=None, lengths=None):
        """`collect` (optional dict) receives what the reference keeps in graph collections for the
        loss block ('points1', 'points2', 'refine_layer_final16384', 'decode_cell64',
        'decode_cell1024': vv_recon.py:210,222,298,338) and the indices taken by the
        index-producing operators ('fps32', 'merge1', 'merge2', 'merge3').

        `lengths`: per-sample point counts of a ragged batch -- sample i is pointcloud[i, :lengths[i]], the rows behind
        may hold anything (NaN included); list, tuple, numpy array, CPU or CUDA tensor.  The counts reach the three
        places where the raw cloud enters the graph: the poolings over the points axis, the three merge layers and the
        FPS of the 32 start points; every output is what the sample's own slice gives up to the batch size of the GEMMs.
        The graph draws 32 FPS samples, so 32 <= lengths[i] <= N: host-given counts outside that raise; counts on the
        device are not read on the host (no synchronisation, the call can be captured into a graph) -- the kernels hold
        them inside [1, N], and keeping them at 32 or above is the caller's responsibility.  The per-point GEMMs still
        run over the padded rows (of a private copy whose padding is zeroed): that work is not removed here."""
        if lengths is not None:
            return self._forward_lengths(pointcloud, collect, lengths)
        x = pointcloud
        c = collect
        # `pointcloud` is the raw side of all three merge layers: put it in curve order once
        raw_sorted = glue.sort_if_large(pointcloud)
        state0 = self.global_mlp("init_mlp", x)
        code1, state = self.encode_cell(x, state0, 0)
        code1 = self.recover_cell("recover1", code1, x)
        fidx, start = glue.sampling(32, pointcloud, use_type="f")
        points1, dstate = self.init_move_layer(start, code1)
        partfeat = self.global_mlp("part_mlp", torch.cat([pointcloud, points1], 1))
        ft = self.mlp("", "partfeat", 2, torch.cat([partfeat, code1], -1))
        points0, dstate0 = self.init_decode_layer(ft)
        points1, dstate = torch.cat([points0, points1], 1), torch.cat([dstate0, dstate], 1)
        pre1 = points1
        points1, m1 = glue.merge_layer(pointcloud, points1.contiguous(), self.decline_factor0, knum=1,
                                       sorted_raw=raw_sorted, return_idx=True)
        points1, dstate = self.refine_layer("refine_layer1", points1, code1, dstate, c)

        pin = torch.cat([pointcloud, points1], 1)
        code2, state = self.encode_cell(pin, state, 1)
        code2 = code1 + self.recover_cell("recover2", code2, pin)
        points2, dstate = self.decode_cell(code2, points1, dstate, 0, collect=c)
        pre2 = points2
        points2, m2 = glue.merge_layer(pointcloud, points2.contiguous(), self.decline_factor1, knum=1,
                                       sorted_raw=raw_sorted, return_idx=True)
        points2, dstate = self.refine_layer("refine_layer2", points2, code2, dstate, c)

        pin = torch.cat([pointcloud, points2], 1)
        code3, state = self.encode_cell(pin, state, 2)
        code3 = code2 + self.recover_cell("recover3", code3, pin)
        # the state of the last decoder and the features of the last refine layer reach no output and no
        # loss term (their parameters get no gradient in the reference either): not computed
        points3, _ = self.decode_cell(code3, points2, dstate, 1, collect=c, need_state=False)
        final, m3 = glue.merge_layer(pointcloud, points3.contiguous(), self.decline_factor, knum=1,
                                     sorted_raw=raw_sorted, return_idx=True)
        final, _ = self.refine_layer("refine_layer_final", final, code3, None, c, need_feat=False)
        if c is not None:
            c.update({"points1": pre1, "points2": pre2, "fps32": fidx, "merge1": m1, "merge2": m2, "merge3": m3})
        return points1, points2, points3, final

    def _forward_lengths(self, pointcloud, collect, lengths):
        """forward() over a ragged batch.  The graph of forward(), with three differences: the raw cloud is a private
        copy whose padded rows are zeros (one masked pass, driven by the device counts: what the per-point layers and
        their weight gradients then see on a padded row is finite, and its upstream gradient is zero); the poolings
        over raw + generated points see cat([generated, raw]) with counts n_generated + lengths, formed on the device
        (a max does not depend on the order, and each sample keeps ONE contiguous valid range); no sorted handle of the
        raw cloud is built (the ragged merge layer sorts inside when it takes the culled sweep)."""
        b, n = pointcloud.shape[0], pointcloud.shape[1]
        ln = _raw._check_lengths(lengths, b, n, "lengths")
        if not ln.is_cuda and b > 0 and int(ln.min()) < 32:
            raise ValueError("RFNet.forward: lengths must lie in [32, N] (the graph draws 32 FPS samples per cloud)")
        # (held inside [1, N] on the device, as the kernels hold them: the sums n_generated + lengths below rely on it)
        ln = _raw._lengths_up(ln, pointcloud.device, n).clamp(1, n)
        valid = torch.arange(n, device=pointcloud.device, dtype=torch.int32).view(1, n, 1) < ln.view(b, 1, 1)
        x = torch.where(valid, pointcloud, pointcloud.new_zeros(()))
        c = collect
        state0 = self.global_mlp("init_mlp", x, ln)
        code1, state = self.encode_cell(x, state0, 0, ln)
        code1 = self.recover_cell("recover1", code1, x, ln)
        fidx, start = glue.sampling(32, x, use_type="f", lengths=ln)
        points1, dstate = self.init_move_layer(start, code1)
        partfeat = self.global_mlp("part_mlp", torch.cat([points1, x], 1), ln + points1.shape[1])
        ft = self.mlp("", "partfeat", 2, torch.cat([partfeat, code1], -1))
        points0, dstate0 = self.init_decode_layer(ft)
        points1, dstate = torch.cat([points0, points1], 1), torch.cat([dstate0, dstate], 1)
        pre1 = points1
        points1, m1 = glue.merge_layer(x, points1.contiguous(), self.decline_factor0, knum=1, return_idx=True, lengths=ln)
        points1, dstate = self.refine_layer("refine_layer1", points1, code1, dstate, c)

        pin, lp = torch.cat([points1, x], 1), ln + points1.shape[1]
        code2, state = self.encode_cell(pin, state, 1, lp)
        code2 = code1 + self.recover_cell("recover2", code2, pin, lp)
        points2, dstate = self.decode_cell(code2, points1, dstate, 0, collect=c)
        pre2 = points2
        points2, m2 = glue.merge_layer(x, points2.contiguous(), self.decline_factor1, knum=1, return_idx=True, lengths=ln)
        points2, dstate = self.refine_layer("refine_layer2", points2, code2, dstate, c)

        pin, lp = torch.cat([points2, x], 1), ln + points2.shape[1]
        code3, state = self.encode_cell(pin, state, 2, lp)
        code3 = code2 + self.recover_cell("recover3", code3, pin, lp)
        points3, _ = self.decode_cell(code3, points2, dstate, 1, collect=c, need_state=False)
        final, m3 = glue.merge_layer(x, points3.contiguous(), self.decline_factor, knum=1, return_idx=True, lengths=ln)
        final, _ = self.refine_layer("refine_layer_final", final, code3, None, c, need_feat=False)
        if c is not None:
            c.update({"points1": pre1, "points2": pre2, "fps32": fidx, "merge1": m1, "merge2": m2, "merge3": m3})
        return points1, points2, points3, final

    def tf_state_dict(self):
        """{TensorFlow variable name: numpy array in the reference's layout} (kernels [1,1,cin,cout])."""
        out = {}
        for name in self._tf_names:
            if name.endswith("/weights"):
                out[name] = self.weights[_key(name[:-len("/weights")])].detach().cpu().numpy()[None, None]
            elif name.endswith("/Variable"):
                out[name] = self.biases[_key(name[:-len("/Variable")])].detach().cpu().numpy()
            else:
                out[name] = getattr(self, name).detach().cpu().numpy()
        return out


_SIDE_STREAMS = {}


def _side_stream(device):
    """One side stream per device, reused (scratch buffers are cached per (device, stream))."""
    key = torch.device(device).index
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


class GroundTruth:
    """Everything the loss block derives from `gt` alone (vv_recon.py:474-475 and the Chamfers' gt side):
    the FPS subsets gt1 (64) / gt2 (1024) and the curve-ordered handles of gt and gt2.  None of it
    depends on the network.  FPS is a serial chain on one CU per cloud (1.1 ms at 16384 -> 1024 points
    while 7/8 of the chip idles), so with `overlap` it can be enqueued on a SIDE STREAM underneath the
    network's forward (`join()` makes the current stream wait for it).  With eager launches that is a coin
    toss on the MI355X (C5 step 8.45 .. 10.0 ms against 8.9 in line: the latency-bound chain slows down
    when GEMM waves share its CUs, and the host's enqueue order decides who gets there first), so the
    default is in line; INSIDE a captured HIP graph the fork is a branch of the graph and pays reliably
    (8.49 -> 8.05 ms per C5 step, tools/experiments/c5_graph_overlap.py).  The 64-point
    subset is the first 64 picks of the 1024-point run (greedy FPS from the same start is a prefix
    chain: one run instead of the reference's two, same indices)."""

    def __init__(self, gt, n1=64, n2=1024, overlap=False):
        self.gt = gt
        self._side = None
        if overlap and gt.is_cuda:
            cur = torch.cuda.current_stream(gt.device)
            capturing = torch.cuda.is_current_stream_capturing()
            self._side = _side_stream(gt.device)
            self._side.wait_stream(cur)  # (inside a capture: a fork of the graph)
            with torch.cuda.stream(self._side):
                self._compute(n1, n2)
            if not capturing:
                # allocated on the side stream, consumed on the current one (a capturing graph owns its
                # pool, and record_stream is not permitted there)
                held = [self.gt1, self.gt2, self.idx1, self.idx2]
                held += [h.buf for h in (self.h_gt, self.h_gt2) if h is not None]
                for t in held:
                    t.record_stream(cur)
        else:
            self._compute(n1, n2)

    def _compute(self, n1, n2):
        big = max(n1, n2)
        idx, pts = glue.sampling(big, self.gt, use_type="f")
        self.idx1, self.idx2 = idx[:, :n1].contiguous(), idx[:, :n2].contiguous()
        self.gt1, self.gt2 = pts[:, :n1].contiguous(), pts[:, :n2].contiguous()
        self.h_gt = glue.sort_if_large(self.gt)
        self.h_gt2 = glue.sort_if_large(self.gt2)

    def join(self):
        if self._side is not None:
            torch.cuda.current_stream(self.gt.device).wait_stream(self._side)
            self._side = None
        return self


def training_loss(net, outputs, collect, gt, alpha1=0.01, terms=None, prepared=None):
    """The loss block of the reference's train() (vv_recon.py:474-500) on the fused ops:
    loss = 0.2 (cd1 + cd2) + cd3 + cd4 + 0.2 recd3 + 0.1 moveloss + loss_d1 + loss_d2 + alpha1 loss_dec,
    cd1/cd2 = earth_mover(FPS(gt), pre-merge points1/points2), cd3/cd4 = chamfer_big(gt, out3/out4),
    recd3 = re_chamfer(gt, out3), loss_d* = 0.05 zero_groupnear(...), loss_dec = sum decfactor^2
    (alpha1 = 0.01 up to step 50000, :482-483).  `gt` is Chamfered five times: sorted once.
    `prepared`: a GroundTruth started before the forward (its FPS then overlapped the network)."""
    out1, out2, out3, out4 = outputs
    g = (prepared if prepared is not None else GroundTruth(gt, out1.shape[1], out2.shape[1], overlap=False)).join()
    hgt, hgt2, gt1, gt2 = g.h_gt, g.h_gt2, g.gt1, g.gt2
    t = {}
    t["cd1"] = glue.earth_mover(gt1, collect["points1"])
    t["cd2"] = glue.earth_mover(gt2, collect["points2"])
    t["cd3"] = glue.chamfer_big(gt, out3, sorted1=hgt)[0]
    t["cd4"] = glue.chamfer_big(gt, out4, sorted1=hgt)[0]  # = chamfer_loss, :484
    t["recd3"] = glue.re_chamfer(gt, out3, part=8)
    t["moveloss"] = (collect[f"refine_layer_final{out4.shape[1]}"] ** 2).sum(-1).mean()
    t["loss_d1"] = 0.05 * glue.zero_groupnear(gt1, gt2, collect[f"decode_cell{out1.shape[1]}"])
    t["loss_d2"] = 0.05 * glue.zero_groupnear(gt2, gt, collect[f"decode_cell{out2.shape[1]}"], hgt2, hgt)
    t["loss_dec"] = net.decline_factor0[0] ** 2 + net.decline_factor1[0] ** 2 + net.decline_factor[0] ** 2
    t["loss"] = (0.2 * (t["cd1"] + t["cd2"]) + t["cd3"] + t["cd4"] + 0.2 * t["recd3"] + 0.1 * t["moveloss"]
                 + t["loss_d1"] + t["loss_d2"] + alpha1 * t["loss_dec"])
    if terms is not None:
        terms.update(t)
        terms.update({"gt_fps64": g.idx1, "gt_fps1024": g.idx2})
    return t["loss"]
