"""GPU: the memory contract of include/rfops.h, entry point by entry point, straight through the C ABI.

Every call gets its buffers from one guarded allocation (tests/arena.py): exact byte lengths, chosen residues, guard
bytes between them, outputs and scratch poisoned.  Four runs per case -- variant `aligned` (every buffer at residue 0
mod 256) or `natural` (tensors at 4 mod 16, workspaces and sorted handles at 16, count arrays and device radii at 4:
what the header allows) times poison 0xFF (NaN / -1) or 0x5A (about 1.5e16 / large positive) -- and each run asserts
  (a) status 0,  (b) no byte changed outside the buffers the call may write,  (c) every output equals the oracle at
  the bar of the op's own GPU test file (regions the header leaves unwritten still hold their poison),
  (d) the outputs agree with the earlier runs of the same case: bit for bit where (c) is bit-exact or the project
      claims a fixed summation order, within (c)'s tolerance elsewhere.
CASES is the table tests/test_memory_contract_host.py checks against _lib.SIGNATURES."""
import ctypes as C

import numpy as np
import pytest
import torch

from arena import Arena
from conftest import assert_rel
from test_gpu_emd_lengths import check_padding_zero, hostile
from test_gpu_fuzz import _match_close
from test_gpu_knn import np_grads, ref_knn, same_val

pytestmark = pytest.mark.gpu

F32, I32, U8 = np.float32, np.int32, np.uint8
LEVELS7 = [-256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0]  # a non-reference schedule (test_gpu_emd_lengths.py)
RF_EINVAL = -1

CASES = {}     # case id -> (entry points it calls, function)
# Check (d) lives in these module-level tables: a run is compared with the FIRST run of its case that got as far as its outputs
# in this session, so it needs the case's runs in one session (the default: all four, back to back).  A run selected alone
# with -k, or one whose earlier siblings failed, has nothing to be compared with and passes (d) vacuously.  A case's entries
# are dropped after its fourth run, so the inputs and outputs of 90-odd cases do not stay alive to the end of the session.
_REFS = {}     # case id -> inputs and oracle results, computed once and shared by the four runs
_RUNS = {}     # case id -> outputs of the first run: {name: (array, None | (rel, abs))}
_SEEN = {}     # case id -> runs started
RUNS_PER_CASE = 4


def case(*entries):
    def reg(fn):
        CASES[fn.__name__] = (entries, fn)
        return fn
    return reg


class Ctx:
    def __init__(self, cid, variant, poison, orc):
        from rfnet_amd._lib import lib
        self.cid, self.variant, self.poison, self.orc, self.lib = cid, variant, poison, orc, lib
        nat = variant == "natural"
        self.T = 4 if nat else 0      # tensors
        self.T16 = 16 if nat else 0   # tensors of the entries the header lists as needing 16 bytes
        self.W = 16 if nat else 0     # workspaces, sorted handles
        self.L = 4 if nat else 0      # count arrays, device radii
        self.kept = {}

    def res(self, k):
        """residue k in the natural variant (zero-fill heads: 4, 8, 12), 0 in the aligned one"""
        return k if self.variant == "natural" else 0

    def ref(self, fn):
        if self.cid not in _REFS:
            _REFS[self.cid] = fn()
        return _REFS[self.cid]

    def arena(self):
        return Arena("cuda", self.poison)

    def ws(self, A, nbytes, name="ws"):
        """-> (pointer, size): scratch of exactly `nbytes` (NULL when the size query says 0)"""
        nbytes = int(nbytes)
        if nbytes == 0:
            return None, 0
        A.add(name, (nbytes,), U8, "scratch", self.W)
        return name, nbytes

    def call(self, A, name, *args):
        args = [A.ptr(a) if isinstance(a, str) else a for a in args]
        st = getattr(self.lib, name)(*args)
        torch.cuda.synchronize()
        assert st == 0, f"{name} returned {st}"
        A.check(f"{name} [{self.cid}, {self.variant}, poison {self.poison:#x}]")

    # ---- (c) and (d) ----
    def exact(self, name, got, exp):
        got, exp = np.asarray(got), np.asarray(exp)
        if got.dtype == F32:
            assert same_val(got, np.asarray(exp, F32)) or np.array_equal(got, exp), f"{self.cid}: {name} differs from the oracle"
        else:
            assert np.array_equal(got, exp), f"{self.cid}: {name} differs from the oracle"
        self.kept[name] = (got, None)

    def close(self, name, got, exp, rel, abs_=0.0, fixed_order=False):
        assert_rel(got, exp, rel, abs_, what=f"{self.cid}: {name}")
        self.kept[name] = (np.asarray(got), None if fixed_order else (rel, abs_))

    def keep(self, name, got, tol=None):
        self.kept[name] = (np.asarray(got), tol)

    def poisoned(self, A, name):
        assert A.still_poison(name), f"{self.cid}: '{name}' is documented as not written but lost its poison"

    def across_runs(self):
        first = _RUNS.setdefault(self.cid, self.kept)
        if first is self.kept:
            return
        for name, (got, tol) in self.kept.items():
            ref = first[name][0]
            if tol is None:
                assert got.tobytes() == ref.tobytes(), \
                    f"{self.cid}: {name} is not bit-equal across variant / poison ({self.variant}, {self.poison:#x})"
            elif tol == "match":
                _match_close(got, ref, f"{self.cid}: {name} across runs")
            else:
                assert_rel(got, ref, tol[0], tol[1], what=f"{self.cid}: {name} across runs")


def _randn(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(F32)


def _unit(seed, *shape):
    return (np.random.RandomState(seed).random_sample(shape) - 0.5).astype(F32)


def _amax(x):
    return float(np.abs(x).max())


# =============================================================================== Chamfer ======
B, N, M = 3, 301, 203


def _nn_ref(x, seed=1, b=B, n=N, m=M):
    a, c = _randn(seed, b, n, 3), _randn(seed + 1, b, m, 3)
    return dict(a=a, c=c, e=x.orc.nn_distance(a, c))


def _nn_io(x, A, r, b=B, n=N, m=M):
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("d1", (b, n), F32, "out", x.T)
    A.add("i1", (b, n), I32, "out", x.T)
    A.add("d2", (b, m), F32, "out", x.T)
    A.add("i2", (b, m), I32, "out", x.T)


def _nn_check(x, A, e, dirs=(1, 2)):
    for d in (1, 2):
        if d in dirs:
            x.exact(f"d{d}", A.get(f"d{d}"), e[2 * d - 2])
            x.exact(f"i{d}", A.get(f"i{d}"), e[2 * d - 1])
        else:
            x.poisoned(A, f"d{d}")
            x.poisoned(A, f"i{d}")


@case("rf_nn_distance")
def nn_distance(x):
    r = x.ref(lambda: _nn_ref(x))
    A = x.arena()
    _nn_io(x, A, r)
    ws, wsz = x.ws(A, x.lib.rf_nn_distance_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_nn_distance", B, N, M, "a", "c", "d1", "i1", "d2", "i2", ws, wsz, None)
    _nn_check(x, A, r["e"])


def _nn_mode(x, mode):
    r = x.ref(lambda: _nn_ref(x))
    A = x.arena()
    _nn_io(x, A, r)
    ws, wsz = x.ws(A, x.lib.rf_nn_distance_mode_workspace_bytes(B, N, M, mode))
    A.build()
    x.call(A, "rf_nn_distance_mode", B, N, M, "a", "c", "d1", "i1", "d2", "i2", ws, wsz, None, mode, None)
    _nn_check(x, A, r["e"])


@case("rf_nn_distance_mode")
def nn_distance_mode_dense(x):
    _nn_mode(x, 1)


@case("rf_nn_distance_mode")
def nn_distance_mode_culled(x):
    _nn_mode(x, 2)


def _nn_dir(x, w1, w2):
    """all four outputs passed: those of the direction that is not wanted keep their poison"""
    r = x.ref(lambda: _nn_ref(x))
    A = x.arena()
    _nn_io(x, A, r)
    ws, wsz = x.ws(A, x.lib.rf_nn_distance_dir_workspace_bytes(B, N, M, w1, w2))
    A.build()
    x.call(A, "rf_nn_distance_dir", B, N, M, "a", "c", "d1", "i1", "d2", "i2", ws, wsz, None, w1, w2)
    _nn_check(x, A, r["e"], [d for d, w in ((1, w1), (2, w2)) if w])


@case("rf_nn_distance_dir")
def nn_distance_dir_1(x):
    _nn_dir(x, 1, 0)


@case("rf_nn_distance_dir")
def nn_distance_dir_2(x):
    _nn_dir(x, 0, 1)


def _sorted_handles(x, A, names):
    """rf_nn_sort of the clouds in `names` ({cloud: (handle, b, n)}): the handle is an output of the sort and, frozen,
    an input of everything after it"""
    for cloud, (h, b, n) in names.items():
        x.call(A, "rf_nn_sort", b, n, cloud, h, A.nbytes(h), None)
    for h, _, _ in names.values():
        A.freeze(h)


@case("rf_nn_sort", "rf_nn_distance_sorted")
def nn_sort_then_sorted_sweep(x):
    r = x.ref(lambda: _nn_ref(x))
    A = x.arena()
    _nn_io(x, A, r)
    A.add("h1", (x.lib.rf_nn_sort_bytes(B, N),), U8, "out", x.W)
    A.add("h2", (x.lib.rf_nn_sort_bytes(B, M),), U8, "out", x.W)
    A.build()
    _sorted_handles(x, A, {"a": ("h1", B, N), "c": ("h2", B, M)})
    x.call(A, "rf_nn_distance_sorted", B, N, M, "h1", "h2", "d1", "i1", "d2", "i2", None)
    _nn_check(x, A, r["e"])


def _nn_grad_ref(x, seed=3, b=B, n=N, m=M):
    r = _nn_ref(x, seed, b, n, m)
    rng = np.random.RandomState(seed + 2)
    r["gd1"], r["gd2"] = rng.rand(b, n).astype(F32), rng.rand(b, m).astype(F32)
    r["g"] = x.orc.nn_distance_grad(r["a"], r["c"], r["gd1"], r["e"][1], r["gd2"], r["e"][3])
    return r


@case("rf_nn_distance_grad")
def nn_distance_grad(x):
    """grad_xyz1 / grad_xyz2 (3 * 301 * 3 and 3 * 203 * 3 words, not multiples of 4) at residues 4 and 8: zero-fill heads
    of 3 and 2 words (runtime.hip zero_async)"""
    r = x.ref(lambda: _nn_grad_ref(x))
    A = x.arena()
    for k in ("a", "c", "gd1", "gd2"):
        A.add(k, r[k], F32, "in", x.T)
    A.add("i1", r["e"][1], I32, "in", x.T)
    A.add("i2", r["e"][3], I32, "in", x.T)
    A.add("g1", (B, N, 3), F32, "out", x.res(4))
    A.add("g2", (B, M, 3), F32, "out", x.res(8))
    A.build()
    x.call(A, "rf_nn_distance_grad", B, N, M, "a", "c", "gd1", "i1", "gd2", "i2", "g1", "g2", None)
    for k, o in (("g1", r["g"][0]), ("g2", r["g"][1])):  # test_gpu_chamfer.py's bar
        x.close(k, A.get(k), o, 1e-5, 1e-5 * _amax(o))


def _chamfer_step(x, b, n, m, culled):
    r = x.ref(lambda: _nn_grad_ref(x, 5, b, n, m))
    A = x.arena()
    for k in ("a", "c", "gd1", "gd2"):
        A.add(k, r[k], F32, "in", x.T)
    for k, shape, dt in (("d1", (b, n), F32), ("i1", (b, n), I32), ("d2", (b, m), F32), ("i2", (b, m), I32)):
        A.add(k, shape, dt, "out", x.T)
    A.add("g1", (b, n, 3), F32, "out", x.res(12))
    A.add("g2", (b, m, 3), F32, "out", x.res(4))
    need = x.lib.rf_chamfer_step_workspace_bytes(b, n, m)
    # the culled step keeps the winners in its workspace: larger than the forward's alone (rfops.h)
    assert (need > x.lib.rf_nn_distance_workspace_bytes(b, n, m)) == culled, "not the route under test"
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_chamfer_step", b, n, m, "a", "c", "gd1", "gd2", "d1", "i1", "d2", "i2", "g1", "g2", ws, wsz, None)
    _nn_check(x, A, r["e"])
    for k, o in (("g1", r["g"][0]), ("g2", r["g"][1])):  # test_gpu_chamfer_ext.py's bar
        x.close(k, A.get(k), o, 1e-5, 1e-5 * _amax(o))


@case("rf_chamfer_step")
def chamfer_step_dense(x):
    _chamfer_step(x, B, N, M, False)


@case("rf_chamfer_step")
def chamfer_step_culled(x):
    _chamfer_step(x, 2, 2053, 4093, True)  # culled from 2^24 pairs on (clouds of at most 4096 points)


def _counts(seed, b, n, lo=1):
    """one full count, one short, the rest random"""
    l = np.random.RandomState(seed).randint(max(lo, n // 3), n + 1, b)
    l[0] = n
    if b > 1:
        l[-1] = max(lo, n // 5)
    return l.astype(I32)


def _nn_lengths_ref(x, seed=7):
    r = _nn_grad_ref(x, seed)
    a, c = r["a"], r["c"]
    l1, l2 = _counts(seed, B, N), _counts(seed + 1, B, M)
    for i in range(B):  # hostile padding: it must never reach a result
        a[i, l1[i]:] = np.nan
        c[i, l2[i]:] = 1e30
    d1, d2 = np.zeros((B, N), F32), np.zeros((B, M), F32)
    i1, i2 = np.full((B, N), -1, I32), np.full((B, M), -1, I32)
    g1, g2 = np.zeros((B, N, 3), F32), np.zeros((B, M, 3), F32)
    for i in range(B):
        n_, m_ = l1[i], l2[i]
        e = x.orc.nn_distance(a[i:i + 1, :n_], c[i:i + 1, :m_])
        d1[i, :n_], i1[i, :n_], d2[i, :m_], i2[i, :m_] = e[0][0], e[1][0], e[2][0], e[3][0]
        g = x.orc.nn_distance_grad(a[i:i + 1, :n_], c[i:i + 1, :m_], r["gd1"][i:i + 1, :n_], e[1], r["gd2"][i:i + 1, :m_], e[3])
        g1[i, :n_], g2[i, :m_] = g[0][0], g[1][0]
    r.update(l1=l1, l2=l2, e=(d1, i1, d2, i2), g=(g1, g2))
    return r


def _nn_lengths(x, mode):
    r = x.ref(lambda: _nn_lengths_ref(x))
    A = x.arena()
    _nn_io(x, A, r)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    ws, wsz = x.ws(A, x.lib.rf_nn_distance_lengths_workspace_bytes(B, N, M, mode))
    A.build()
    x.call(A, "rf_nn_distance_lengths", B, N, M, "a", "c", "l1", "l2", "d1", "i1", "d2", "i2", ws, wsz, None, mode)
    _nn_check(x, A, r["e"])  # padded slots: dist 0, idx -1


@case("rf_nn_distance_lengths")
def nn_distance_lengths_dense(x):
    _nn_lengths(x, 1)


@case("rf_nn_distance_lengths")
def nn_distance_lengths_culled(x):
    _nn_lengths(x, 2)


@case("rf_nn_distance_grad_lengths")
def nn_distance_grad_lengths(x):
    r = x.ref(lambda: _nn_lengths_ref(x))
    rng = np.random.RandomState(0)
    A = x.arena()
    for k in ("a", "c", "gd1", "gd2"):
        A.add(k, r[k], F32, "in", x.T)
    # whatever idx holds beyond a count (here: out of range) reaches nothing
    A.add("i1", np.where(r["e"][1] < 0, rng.randint(-9, 1 << 20, (B, N)), r["e"][1]), I32, "in", x.T)
    A.add("i2", np.where(r["e"][3] < 0, rng.randint(-9, 1 << 20, (B, M)), r["e"][3]), I32, "in", x.T)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    A.add("g1", (B, N, 3), F32, "out", x.res(8))
    A.add("g2", (B, M, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_nn_distance_grad_lengths", B, N, M, "a", "c", "l1", "l2", "gd1", "i1", "gd2", "i2", "g1", "g2", None)
    for k, o, l in (("g1", r["g"][0], r["l1"]), ("g2", r["g"][1], r["l2"])):  # test_gpu_nn_lengths.py's _tol
        got = A.get(k)
        check_padding_zero(got, l, 1, k)
        x.close(k, got, o, 1e-4, 1e-5 * _amax(o))


def _loss64(d, lens=None):
    d = np.sqrt(d.astype(np.float64))
    if lens is None:
        return d.mean(1)
    return np.array([d[i, :k].mean() for i, k in enumerate(lens)])


def _loss_grad_ref(x, r, l1=None, l2=None):
    """chamfer_loss's backward (test_gpu_chamfer_ext.py): NnDistanceGrad with gd = gl / count * 0.5 / sqrt(d)"""
    e = r["e"]
    gl = (np.random.RandomState(9).rand(B, 2) + 0.5).astype(F32)
    n1 = np.full(B, N) if l1 is None else l1
    n2 = np.full(B, M) if l2 is None else l2
    g1, g2 = np.zeros((B, N, 3), F32), np.zeros((B, M, 3), F32)
    for i in range(B):
        n_, m_ = n1[i], n2[i]
        gd1 = (gl[i, 0] / n_ * 0.5 / np.sqrt(e[0][i:i + 1, :n_].astype(np.float64))).astype(F32)
        gd2 = (gl[i, 1] / m_ * 0.5 / np.sqrt(e[2][i:i + 1, :m_].astype(np.float64))).astype(F32)
        g = x.orc.nn_distance_grad(r["a"][i:i + 1, :n_], r["c"][i:i + 1, :m_], gd1, e[1][i:i + 1, :n_], gd2, e[3][i:i + 1, :m_])
        g1[i, :n_], g2[i, :m_] = g[0][0], g[1][0]
    return gl, g1, g2


def _chamfer_loss(x, handles):
    r = x.ref(lambda: _nn_ref(x, 11))
    A = x.arena()
    _nn_io(x, A, r)
    A.add("loss", (B, 2), F32, "out", x.T)
    if handles:
        A.add("h1", (x.lib.rf_nn_sort_bytes(B, N),), U8, "out", x.W)
        A.add("h2", (x.lib.rf_nn_sort_bytes(B, M),), U8, "out", x.W)
    h1, h2 = ("h1", "h2") if handles else (None, None)
    ws, wsz = x.ws(A, x.lib.rf_chamfer_loss_workspace_bytes(B, N, M, 1, 1, int(handles), int(handles)))
    A.build()
    if handles:
        _sorted_handles(x, A, {"a": ("h1", B, N), "c": ("h2", B, M)})
    x.call(A, "rf_chamfer_loss", B, N, M, "a", "c", h1, h2, "loss", "d1", "i1", "d2", "i2", ws, wsz, None)
    _nn_check(x, A, r["e"])
    exp = np.stack([_loss64(r["e"][0]), _loss64(r["e"][2])], 1)
    x.close("loss", A.get("loss"), exp, 2e-6, 1e-9)  # test_gpu_chamfer_ext.py's bar


@case("rf_chamfer_loss")
def chamfer_loss(x):
    _chamfer_loss(x, False)


@case("rf_chamfer_loss", "rf_nn_sort")
def chamfer_loss_sorted_handles(x):
    _chamfer_loss(x, True)


@case("rf_chamfer_loss")
def chamfer_loss_one_direction(x):
    """direction 2 skipped by NULL pointers: loss[:, 1] = 0"""
    r = x.ref(lambda: _nn_ref(x, 11))
    A = x.arena()
    _nn_io(x, A, r)
    A.add("loss", (B, 2), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_chamfer_loss_workspace_bytes(B, N, M, 1, 0, 0, 0))
    A.build()
    x.call(A, "rf_chamfer_loss", B, N, M, "a", "c", None, None, "loss", "d1", "i1", None, None, ws, wsz, None)
    _nn_check(x, A, r["e"], [1])
    x.close("loss", A.get("loss"), np.stack([_loss64(r["e"][0]), np.zeros(B)], 1), 2e-6, 1e-9)


@case("rf_chamfer_loss_grad")
def chamfer_loss_grad(x):
    def mk():
        r = _nn_ref(x, 11)
        r["gl"], r["g1"], r["g2"] = _loss_grad_ref(x, r)
        return r
    r = x.ref(mk)
    A = x.arena()
    for k, v, dt in (("a", r["a"], F32), ("c", r["c"], F32), ("d1", r["e"][0], F32), ("i1", r["e"][1], I32),
                     ("d2", r["e"][2], F32), ("i2", r["e"][3], I32), ("gl", r["gl"], F32)):
        A.add(k, v, dt, "in", x.T)
    A.add("g1", (B, N, 3), F32, "out", x.res(12))
    A.add("g2", (B, M, 3), F32, "out", x.res(8))
    A.build()
    x.call(A, "rf_chamfer_loss_grad", B, N, M, "a", "c", "d1", "i1", "d2", "i2", "gl", "g1", "g2", None)
    for k in ("g1", "g2"):  # test_gpu_chamfer_ext.py's bar
        x.close(k, A.get(k), r[k], 1e-4, 1e-5 * _amax(r[k]))


@case("rf_chamfer_loss_lengths")
def chamfer_loss_lengths(x):
    r = x.ref(lambda: _nn_lengths_ref(x, 13))
    A = x.arena()
    _nn_io(x, A, r)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    A.add("loss", (B, 2), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_chamfer_loss_lengths_workspace_bytes(B, N, M, 1, 1))
    A.build()
    x.call(A, "rf_chamfer_loss_lengths", B, N, M, "a", "c", "l1", "l2", "loss", "d1", "i1", "d2", "i2", ws, wsz, None)
    _nn_check(x, A, r["e"])
    exp = np.stack([_loss64(r["e"][0], r["l1"]), _loss64(r["e"][2], r["l2"])], 1)
    # the float64 reference of test_gpu_chamfer_ext.py and its bar (test_gpu_nn_lengths.py compares two GPU results)
    x.close("loss", A.get("loss"), exp, 2e-6, 1e-9)


@case("rf_chamfer_loss_grad_lengths")
def chamfer_loss_grad_lengths(x):
    def mk():
        r = _nn_lengths_ref(x, 13)
        r["gl"], r["g1"], r["g2"] = _loss_grad_ref(x, r, r["l1"], r["l2"])
        return r
    r = x.ref(mk)
    A = x.arena()
    for k, v, dt in (("a", r["a"], F32), ("c", r["c"], F32), ("d1", r["e"][0], F32), ("i1", r["e"][1], I32),
                     ("d2", r["e"][2], F32), ("i2", r["e"][3], I32), ("gl", r["gl"], F32)):
        A.add(k, v, dt, "in", x.T)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    A.add("g1", (B, N, 3), F32, "out", x.res(4))
    A.add("g2", (B, M, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_chamfer_loss_grad_lengths", B, N, M, "a", "c", "l1", "l2", "d1", "i1", "d2", "i2", "gl", "g1", "g2", None)
    for k, l in (("g1", r["l1"]), ("g2", r["l2"])):  # test_gpu_nn_lengths.py's _tol
        got = A.get(k)
        check_padding_zero(got, l, 1, k)
        x.close(k, got, r[k], 1e-4, 1e-5 * _amax(r[k]))


def _merge_ref(x):
    """float64 of the reference's formula (vv_recon.py:132-139) over the oracle's idx2, and its gradients by autograd"""
    rng = np.random.RandomState(17)
    raw, new = (rng.rand(B, N, 3) - 0.5).astype(F32), (rng.rand(B, M, 3) - 0.5).astype(F32)
    dec = np.array([0.07], F32)
    i2 = x.orc.nn_distance(raw, new)[3]
    go = rng.randn(B, M, 3).astype(F32)
    traw = torch.from_numpy(raw).double().requires_grad_(True)
    tnew = torch.from_numpy(new).double().requires_grad_(True)
    tdec = torch.from_numpy(dec).double().expand(B).clone().requires_grad_(True)  # one copy per sample: grad_dec is per sample
    g = torch.gather(traw, 1, torch.from_numpy(i2).long()[..., None].expand(B, M, 3))
    diff = g - tnew
    ratio = torch.exp(-(diff * diff).sum(-1, keepdim=True) / (1e-8 + tdec.view(B, 1, 1) ** 2))
    out = tnew + ratio * diff
    (out * torch.from_numpy(go).double()).sum().backward()
    return dict(raw=raw, new=new, dec=dec, i2=i2, go=go, out=out.detach().numpy(), gnew=tnew.grad.numpy(),
                graw=traw.grad.numpy(), gdec=tdec.grad.numpy())


@case("rf_merge_layer")
def merge_layer(x):
    r = x.ref(lambda: _merge_ref(x))
    A = x.arena()
    A.add("raw", r["raw"], F32, "in", x.T)
    A.add("new", r["new"], F32, "in", x.T)
    A.add("dec", r["dec"], F32, "in", x.L)
    A.add("out", (B, M, 3), F32, "out", x.T)
    A.add("i2", (B, M), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_merge_layer_workspace_bytes(B, N, M, 0))
    A.build()
    x.call(A, "rf_merge_layer", B, N, M, "raw", "new", None, "dec", "out", "i2", ws, wsz, None)
    x.exact("i2", A.get("i2"), r["i2"])
    x.close("out", A.get("out"), r["out"], 1e-5, 1e-6)  # test_gpu_chamfer_ext.py's bar


@case("rf_merge_layer_grad")
def merge_layer_grad(x):
    r = x.ref(lambda: _merge_ref(x))
    A = x.arena()
    for k, dt in (("raw", F32), ("new", F32), ("i2", I32), ("go", F32)):
        A.add(k, r[k], dt, "in", x.T)
    A.add("dec", r["dec"], F32, "in", x.L)
    A.add("gnew", (B, M, 3), F32, "out", x.res(4))
    A.add("gdec", (B,), F32, "out", x.res(8))
    A.add("graw", (B, N, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_merge_layer_grad", B, N, M, "raw", "new", "dec", "i2", "go", "gnew", "gdec", "graw", None)
    x.close("gnew", A.get("gnew"), r["gnew"], 1e-4, 1e-5 * _amax(r["gnew"]))  # test_gpu_chamfer_ext.py's bars
    x.close("graw", A.get("graw"), r["graw"], 1e-4, 1e-5 * _amax(r["graw"]))
    # (that file bounds the SUM of the per-sample terms by rel 1e-3 + abs 1e-4 * |sum| + 1e-6; the same bar per sample)
    x.close("gdec", A.get("gdec"), r["gdec"], 1e-3, 1e-4 * _amax(r["gdec"]) + 1e-6)


# =============================================================================== EMD ==========
def _am64(a, c, levels):
    """the annealing schedule of approx_match (oracle/rfops_oracle.c orc_approxmatch_levels) in float64"""
    a, c = a.astype(np.float64), c.astype(np.float64)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    out = np.zeros((b, m, n))
    for i in range(b):
        d2 = ((c[i][:, None, :] - a[i][None, :, :]) ** 2).sum(-1)
        rl, rr = np.full(n, max(1.0, float(m // n))), np.full(m, max(1.0, float(n // m)))
        for lv in levels:
            e = np.exp(lv * d2)
            ratio_l = rl / (1e-9 + (e * rr[:, None]).sum(0))
            s = (e * ratio_l[None, :]).sum(1) * rr
            ratio_r = rr * np.minimum(rr / (s + 1e-9), 1.0)
            rr = np.maximum(0.0, rr - s)
            p = e * ratio_l[None, :] * ratio_r[:, None]
            out[i] += p
            rl = np.maximum(0.0, rl - p.sum(0))
    return out


def _marginals_well_posed(x, a, c, om, levels=None):
    """`match` is compared on inputs whose two clouds carry the same total mass (n == m, or one count a multiple of the other).
    Where they do not -- 301 against 203 points: multipliers 1 and 1, a third of the mass never shipped -- which column keeps how
    much hangs on the clamps of the schedule, and the fp32 ORACLE's own column sums are 3e-5 .. 1e-3 away from a float64
    evaluation of the same schedule (ten seeds at 3 x 301 x 203), outside _match_close's marginal bar of 1e-5 + 1e-5 |sum| before
    any kernel is involved; with equal masses they are within 6e-6.  This asserts that property of the INPUT, from the
    reference alone, so that the bar is only asked where the reference itself can be held to it."""
    levels = [float(v) for v in x.orc.default_levels()] if levels is None else levels
    ex = _am64(a, c, levels)
    assert_rel(om.astype(np.float64).sum(1), ex.sum(1), 1e-5, 1e-5, what="oracle's own column sums vs float64")
    assert_rel(om.astype(np.float64).sum(2), ex.sum(2), 1e-5, 1e-5, what="oracle's own row sums vs float64")


def _emd_ref(x, n=N, m=M, levels=None, match_is_checked=False):
    a, c = _unit(21, B, n, 3), _unit(22, B, m, 3)
    om = x.orc.approx_match(a, c) if levels is None else x.orc.approx_match(a, c, levels=levels)
    if match_is_checked:
        _marginals_well_posed(x, a, c, om, levels)
    g = x.orc.match_cost_grad(a, c, om)
    return dict(a=a, c=c, om=om, cost=x.orc.match_cost(a, c, om), g1=g[0], g2=g[1])


NR, MR = 406, 203  # a rectangular match (b, 203, 406) with equal masses: 406 points of mass 1 against 203 of mass 2


def _approxmatch(x, entry, levels=None, mode=None, n=N, m=N):
    """n, m: equal total masses (_marginals_well_posed) -- square, or one count twice the other"""
    r = x.ref(lambda: _emd_ref(x, n, m, levels, True))
    nlv = 0 if levels is None else len(levels)
    lv = None if levels is None else (C.c_float * nlv)(*levels)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("match", (B, m, n), F32, "out", x.T)
    if mode is None:
        need = x.lib.rf_approxmatch_workspace_bytes(B, n, m, nlv)
    else:
        need = x.lib.rf_approxmatch_mode_workspace_bytes(B, n, m, nlv, mode)
    ws, wsz = x.ws(A, need)
    A.build()
    if entry == "rf_approxmatch":
        x.call(A, entry, B, n, m, "a", "c", "match", ws, wsz, None)
    elif entry == "rf_approxmatch_levels":
        x.call(A, entry, B, n, m, "a", "c", "match", lv, nlv, ws, wsz, None)
    else:
        x.call(A, entry, B, n, m, "a", "c", "match", lv, nlv, ws, wsz, None, mode)
    got = A.get("match")
    _match_close(got, r["om"], f"{x.cid}: match")
    x.keep("match", got, "match")


@case("rf_approxmatch")
def approxmatch(x):
    _approxmatch(x, "rf_approxmatch")


@case("rf_approxmatch")
def approxmatch_rectangular(x):
    _approxmatch(x, "rf_approxmatch", n=NR, m=MR)


@case("rf_approxmatch_levels")
def approxmatch_levels(x):
    _approxmatch(x, "rf_approxmatch_levels", LEVELS7)


@case("rf_approxmatch_levels")
def approxmatch_levels_rectangular(x):
    _approxmatch(x, "rf_approxmatch_levels", LEVELS7, n=NR, m=MR)


@case("rf_approxmatch_mode")
def approxmatch_mode_swept(x):
    _approxmatch(x, "rf_approxmatch_mode", None, 1)


@case("rf_approxmatch_mode")
def approxmatch_mode_swept_rectangular(x):
    _approxmatch(x, "rf_approxmatch_mode", None, 1, n=NR, m=MR)


@case("rf_matchcost")
def matchcost(x):
    r = x.ref(lambda: _emd_ref(x))
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("match", r["om"], F32, "in", x.T)
    A.add("cost", (B,), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_matchcost_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_matchcost", B, N, M, "a", "c", "match", "cost", ws, wsz, None)
    x.close("cost", A.get("cost"), r["cost"], 1e-5)


def _mcg_rows_form(n, m):
    """approxmatch.hip mcg_launch's rule for the row form (with 16-byte aligned xyz1 and match)"""
    return n % 4 == 0 and 4 * n >= 3 * -(-n // 1024) * 1024 and m >= 16


def _matchcost_grad(x, n, m, rows):
    """test_gpu_fuzz.py test_fuzz_match_cost_grad_both_forms: its inputs and its bar"""
    def mk():
        rng = np.random.RandomState(23 + n)
        a, c = rng.randn(B, n, 3).astype(F32) * F32(0.3), rng.randn(B, m, 3).astype(F32) * F32(0.3)
        c[:, 1] = a[:, 0]  # a coincident pair
        mt = (rng.random_sample((B, m, n)) ** 6).astype(F32) / F32(n)
        return dict(a=a, c=c, mt=mt, g=x.orc.match_cost_grad(a, c, mt))
    r = x.ref(mk)
    assert _mcg_rows_form(n, m) == rows, "not the route under test"
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)   # natural: xyz1 and match 4-byte aligned, the row form's shape on the tile form
    A.add("c", r["c"], F32, "in", x.T)
    A.add("match", r["mt"], F32, "in", x.T)
    A.add("g1", (B, n, 3), F32, "out", x.res(12))
    A.add("g2", (B, m, 3), F32, "out", x.res(8))
    A.build()
    x.call(A, "rf_matchcost_grad", B, n, m, "a", "c", "match", "g1", "g2", None)
    x.close("g1", A.get("g1"), r["g"][0], 1e-4, 2e-6 * max(1, m // 256))
    x.close("g2", A.get("g2"), r["g"][1], 1e-4, 2e-6 * max(1, n // 256))


@case("rf_matchcost_grad")
def matchcost_grad_tile_form(x):
    _matchcost_grad(x, N, M, False)


@case("rf_matchcost_grad")
def matchcost_grad_row_form(x):
    _matchcost_grad(x, 772, M, True)


def _earth_mover(x, entry, grads, mode=None, shape=None):
    """with gradients at equal masses (they are built on the GPU's own match entries: _marginals_well_posed), the cost alone
    at 301 x 203"""
    n, m = shape or ((N, N) if grads else (N, M))
    r = x.ref(lambda: _emd_ref(x, n, m, None, grads))
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("cost", (B,), F32, "out", x.T)
    if grads:
        A.add("g1", (B, n, 3), F32, "out", x.res(8))
        A.add("g2", (B, m, 3), F32, "out", x.res(4))
    g1, g2 = ("g1", "g2") if grads else (None, None)
    need = x.lib.rf_earth_mover_workspace_bytes(B, n, m) if mode is None else x.lib.rf_earth_mover_mode_workspace_bytes(B, n, m, mode)
    ws, wsz = x.ws(A, need)
    A.build()
    if mode is None:
        x.call(A, entry, B, n, m, "a", "c", "cost", g1, g2, ws, wsz, None)
    else:
        x.call(A, entry, B, n, m, "a", "c", "cost", g1, g2, ws, wsz, None, mode)
    x.close("cost", A.get("cost"), r["cost"], 1e-5)
    if grads:
        # test_gpu_fuzz.py test_fuzz_emd_chain_and_fused, the bar for random inputs: the oracle's match_cost / match_cost_grad ON
        # THE GPU's OWN match, which isolates the fused kernel from the ill-conditioning of single match entries (a clamp flip
        # moves up to 2e-3 of a unit mass between neighbours, _match_close; the gradient rows inherit exactly that)
        M2 = x.arena()
        M2.add("a", r["a"], F32, "in", x.T)
        M2.add("c", r["c"], F32, "in", x.T)
        M2.add("match", (B, m, n), F32, "out", x.T)
        mode_ = 0 if mode is None else mode
        ws2, wsz2 = x.ws(M2, x.lib.rf_approxmatch_mode_workspace_bytes(B, n, m, 0, mode_))
        M2.build()
        x.call(M2, "rf_approxmatch_mode", B, n, m, "a", "c", "match", None, 0, ws2, wsz2, None, mode_)
        gm = M2.get("match")
        assert_rel(A.get("cost"), x.orc.match_cost(r["a"], r["c"], gm), 1e-5, what="fused cost vs oracle on the GPU's match")
        o1, o2 = x.orc.match_cost_grad(r["a"], r["c"], gm)
        assert_rel(A.get("g1"), o1, 1e-4, 1e-5 * max(1, m // n), what=f"{x.cid}: g1")
        assert_rel(A.get("g2"), o2, 1e-4, 1e-5 * max(1, n // m), what=f"{x.cid}: g2")
        # across the four runs: test_gpu_emd.py test_earth_mover_fused_vs_oracle's bar
        x.keep("g1", A.get("g1"), (1e-4, 1e-4 * max(1, m // n)))
        x.keep("g2", A.get("g2"), (1e-4, 1e-4 * max(1, n // m)))


@case("rf_earth_mover", "rf_approxmatch_mode")
def earth_mover_with_gradients(x):
    _earth_mover(x, "rf_earth_mover", True)


@case("rf_earth_mover", "rf_approxmatch_mode")
def earth_mover_with_gradients_rectangular(x):
    _earth_mover(x, "rf_earth_mover", True, None, (NR, MR))


@case("rf_earth_mover")
def earth_mover_cost_only(x):
    _earth_mover(x, "rf_earth_mover", False)


@case("rf_earth_mover_mode", "rf_approxmatch_mode")
def earth_mover_mode_swept(x):
    _earth_mover(x, "rf_earth_mover_mode", True, 1)


NE, ME = NR, MR  # the ragged EMD cases: padded to 406 x 203, every sample's counts with equal total masses (_marginals_well_posed)


def _emd_lengths_ref(x):
    a, c = _unit(31, B, NE, 3), _unit(32, B, ME, 3)
    l1, l2 = np.array([NE, 150, 240], I32), np.array([ME, 150, 120], I32)  # full, equal, one twice the other
    a, c = hostile(a, l1, 1e30), hostile(c, l2, np.nan)
    om = np.zeros((B, ME, NE), F32)
    cost = np.zeros(B, F32)
    g1, g2 = np.zeros((B, NE, 3), F32), np.zeros((B, ME, 3), F32)
    for i in range(B):
        sa, sc = a[i:i + 1, :l1[i]], c[i:i + 1, :l2[i]]
        o = x.orc.approx_match(sa, sc)
        _marginals_well_posed(x, sa, sc, o)
        om[i, :l2[i], :l1[i]] = o[0]
        cost[i] = x.orc.match_cost(sa, sc, o)[0]
        g = x.orc.match_cost_grad(sa, sc, o)
        g1[i, :l1[i]], g2[i, :l2[i]] = g[0][0], g[1][0]
    return dict(a=a, c=c, l1=l1, l2=l2, om=om, cost=cost, g1=g1, g2=g2)


def _emd_lengths_in(x, A, r):
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)


@case("rf_approxmatch_lengths")
def approxmatch_lengths(x):
    r = x.ref(lambda: _emd_lengths_ref(x))
    A = x.arena()
    _emd_lengths_in(x, A, r)
    A.add("match", (B, ME, NE), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_approxmatch_lengths_workspace_bytes(B, NE, ME, 0))
    A.build()
    x.call(A, "rf_approxmatch_lengths", B, NE, ME, "a", "c", "l1", "l2", "match", None, 0, ws, wsz, None)
    got = A.get("match")
    check_padding_zero(got, r["l2"], 1, "match rows")
    check_padding_zero(got, r["l1"], 2, "match columns")
    for i in range(B):
        k1, k2 = r["l1"][i], r["l2"][i]
        _match_close(got[i:i + 1, :k2, :k1], r["om"][i:i + 1, :k2, :k1], f"{x.cid}: match, sample {i}")
    x.keep("match", got, "match")


@case("rf_matchcost_lengths")
def matchcost_lengths(x):
    r = x.ref(lambda: _emd_lengths_ref(x))
    A = x.arena()
    _emd_lengths_in(x, A, r)
    mt = r["om"].copy()
    for i in range(B):  # the padded entries of the caller's match reach nothing
        mt[i, r["l2"][i]:] = np.nan
        mt[i, :, r["l1"][i]:] = 1e30
    A.add("match", mt, F32, "in", x.T)
    A.add("cost", (B,), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_matchcost_lengths_workspace_bytes(B, NE, ME))
    A.build()
    x.call(A, "rf_matchcost_lengths", B, NE, ME, "a", "c", "l1", "l2", "match", "cost", ws, wsz, None)
    x.close("cost", A.get("cost"), r["cost"], 1e-5)


@case("rf_matchcost_grad_lengths")
def matchcost_grad_lengths(x):
    r = x.ref(lambda: _emd_lengths_ref(x))
    A = x.arena()
    _emd_lengths_in(x, A, r)
    A.add("match", r["om"], F32, "in", x.T)
    A.add("g1", (B, NE, 3), F32, "out", x.res(4))
    A.add("g2", (B, ME, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_matchcost_grad_lengths", B, NE, ME, "a", "c", "l1", "l2", "match", "g1", "g2", None)
    for k, l in (("g1", r["l1"]), ("g2", r["l2"])):  # test_gpu_emd_lengths.py's bar
        got = A.get(k)
        check_padding_zero(got, l, 1, k)
        x.close(k, got, r[k], 1e-4, 1e-5)


@case("rf_earth_mover_lengths")
def earth_mover_lengths(x):
    r = x.ref(lambda: _emd_lengths_ref(x))
    A = x.arena()
    _emd_lengths_in(x, A, r)
    A.add("cost", (B,), F32, "out", x.T)
    A.add("g1", (B, NE, 3), F32, "out", x.res(12))
    A.add("g2", (B, ME, 3), F32, "out", x.res(8))
    ws, wsz = x.ws(A, x.lib.rf_earth_mover_lengths_workspace_bytes(B, NE, ME))
    A.build()
    x.call(A, "rf_earth_mover_lengths", B, NE, ME, "a", "c", "l1", "l2", "cost", "g1", "g2", ws, wsz, None)
    x.close("cost", A.get("cost"), r["cost"], 1e-5)
    g1, g2 = A.get("g1"), A.get("g2")
    check_padding_zero(g1, r["l1"], 1, "g1")
    check_padding_zero(g2, r["l2"], 1, "g2")
    for i in range(B):  # test_gpu_emd_lengths.py: 1e-4 times the row's mass, per sample
        k1, k2 = int(r["l1"][i]), int(r["l2"][i])
        assert_rel(g1[i], r["g1"][i], 1e-4, 1e-4 * max(1, k2 // k1), what=f"fused grad1, sample {i}")
        assert_rel(g2[i], r["g2"][i], 1e-4, 1e-4 * max(1, k1 // k2), what=f"fused grad2, sample {i}")
    mass = max(max(1, int(k2) // int(k1), int(k1) // int(k2)) for k1, k2 in zip(r["l1"], r["l2"]))
    x.keep("g1", g1, (1e-4, 1e-4 * mass))
    x.keep("g2", g2, (1e-4, 1e-4 * mass))


# =============================================================================== sampling =====
def _fps_ref(x, b, n, m, seed=41):
    p = np.random.RandomState(seed).rand(b, n, 3).astype(F32)
    return dict(p=p, idx=x.orc.farthest_point_sample(m, p))


def _fps_plain(x, b, n, m, temp):
    r = x.ref(lambda: _fps_ref(x, b, n, m))
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("out", (b, m), I32, "out", x.T)
    nt = x.lib.rf_farthestpointsampling_temp_floats(b, n)
    assert (nt > 0) == temp, "not the route under test"
    if nt:
        A.add("temp", (nt,), F32, "scratch", x.T)
    A.build()
    x.call(A, "rf_farthestpointsampling", b, n, m, "p", "temp" if nt else None, "out", None)
    x.exact("out", A.get("out"), r["idx"])


@case("rf_farthestpointsampling")
def fps_registers(x):
    _fps_plain(x, B, N, 67, False)


@case("rf_farthestpointsampling")
def fps_with_temp(x):
    _fps_plain(x, 2, 16411, 33, True)


def _fps_ws(x, b, n, m, sorted_route):
    r = x.ref(lambda: _fps_ref(x, b, n, m))
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("out", (b, m), I32, "out", x.T)
    need = x.lib.rf_farthestpointsampling_workspace_bytes(b, n, m)
    assert (need > 0) == sorted_route, "not the route under test"
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_farthestpointsampling_ws", b, n, m, "p", ws, wsz, "out", None)
    x.exact("out", A.get("out"), r["idx"])


@case("rf_farthestpointsampling_ws")
def fps_ws_sorted_cloud(x):
    _fps_ws(x, 2, 6007, 301, True)


@case("rf_farthestpointsampling_ws")
def fps_ws_no_workspace(x):
    _fps_ws(x, 2, 6007, 101, False)


@case("rf_farthestpointsampling_sorted")
def fps_sorted(x):
    """form 0 (the one defined form), with new_xyz"""
    b, n, m = 2, 1031, 67
    r = x.ref(lambda: _fps_ref(x, b, n, m))
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("out", (b, m), I32, "out", x.T)
    A.add("nx", (b, m, 3), F32, "out", x.T)
    need = x.lib.rf_farthestpointsampling_sorted_workspace_bytes(b, n)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_farthestpointsampling_sorted", b, n, m, 0, "p", ws, wsz, "out", "nx", None)
    x.exact("out", A.get("out"), r["idx"])
    x.exact("nx", A.get("nx"), x.orc.gather_point(r["p"], r["idx"]))


def _fps_lengths(x, b, n, m, sorted_route):
    def mk():
        p = np.random.RandomState(43).rand(b, n, 3).astype(F32)
        ln, lo = _counts(44, b, n), _counts(45, b, m)
        idx, nx = np.zeros((b, m), I32), np.zeros((b, m, 3), F32)
        for i in range(b):
            p[i, ln[i]:] = np.nan
            s = x.orc.farthest_point_sample(int(lo[i]), p[i:i + 1, :ln[i]])
            idx[i, :lo[i]] = s[0]
            nx[i, :lo[i]] = p[i, s[0]]
        return dict(p=p, ln=ln, lo=lo, idx=idx, nx=nx)
    r = x.ref(mk)
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("ln", r["ln"], I32, "in", x.L)
    A.add("lo", r["lo"], I32, "in", x.L)
    A.add("out", (b, m), I32, "out", x.T)
    A.add("nx", (b, m, 3), F32, "out", x.T)
    need = x.lib.rf_farthestpointsampling_lengths_workspace_bytes(b, n, m)
    assert (need > 0) == sorted_route, "not the route under test"
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_farthestpointsampling_lengths", b, n, m, "p", "ln", "lo", ws, wsz, "out", "nx", None)
    x.exact("out", A.get("out"), r["idx"])  # zeros behind len_out
    x.exact("nx", A.get("nx"), r["nx"])


@case("rf_farthestpointsampling_lengths")
def fps_lengths(x):
    _fps_lengths(x, B, N, 67, False)


@case("rf_farthestpointsampling_lengths")
def fps_lengths_sorted_cloud(x):
    _fps_lengths(x, 2, 6007, 301, True)


@case("rf_gatherpoint")
def gatherpoint(x):
    def mk():
        rng = np.random.RandomState(47)
        p, idx = rng.rand(B, N, 3).astype(F32), rng.randint(0, N, (B, 67)).astype(I32)
        return dict(p=p, idx=idx, out=x.orc.gather_point(p, idx))
    r = x.ref(mk)
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("out", (B, 67, 3), F32, "out", x.T)
    A.build()
    x.call(A, "rf_gatherpoint", B, N, 67, "p", "idx", "out", None)
    x.exact("out", A.get("out"), r["out"])


@case("rf_scatteraddpoint")
def scatteraddpoint(x):
    def mk():
        rng = np.random.RandomState(48)
        p, idx = rng.rand(B, N, 3).astype(F32), rng.randint(0, N, (B, 67)).astype(I32)
        og = rng.randn(B, 67, 3).astype(F32)
        return dict(idx=idx, og=og, g=x.orc.gather_point_grad(p, idx, og))
    r = x.ref(mk)
    A = x.arena()
    A.add("og", r["og"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("g", (B, N, 3), F32, "out", x.res(4))
    A.build()
    x.call(A, "rf_scatteraddpoint", B, N, 67, "og", "idx", "g", None)
    x.close("g", A.get("g"), r["g"], 1e-5, 1e-6)  # test_gpu_sampling_grouping.py's bar


@case("rf_probsample")
def probsample(x):
    def mk():
        rng = np.random.RandomState(49)
        p, u = rng.rand(B, 41).astype(F32), rng.rand(B, 101).astype(F32)
        p[:, 3] = 0.0
        out, cs = x.orc.prob_sample(p, u)
        return dict(p=p, u=u, out=out, cs=np.ascontiguousarray(cs, F32))
    r = x.ref(mk)
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    A.add("u", r["u"], F32, "in", x.T)
    A.add("temp", (B, 41), F32, "out", x.T)  # receives the cumulative sums
    A.add("out", (B, 101), I32, "out", x.T)
    A.build()
    x.call(A, "rf_probsample", B, 41, 101, "p", "u", "temp", "out", None)
    x.exact("out", A.get("out"), r["out"])
    x.exact("temp", A.get("temp"), r["cs"])


# =============================================================================== grouping =====
MQ, NS, RAD = 67, 13, 0.2


def _qb_ref(x, n=N):
    rng = np.random.RandomState(51)
    p = rng.rand(B, n, 3).astype(F32)
    q = rng.rand(B, MQ, 3).astype(F32)
    q[:, 0] = 9.0  # an empty ball: its idx row is not written
    idx, cnt = x.orc.query_ball_point(F32(RAD), NS, p, q) if n else (np.zeros((B, MQ, NS), I32), np.zeros((B, MQ), I32))
    return dict(p=p, q=q, idx=idx, cnt=cnt, rad=np.array([RAD], F32))


def _qb_check(x, A, r):
    cnt, idx = A.get("cnt"), A.get("idx")
    x.exact("cnt", cnt, r["cnt"])
    has = r["cnt"] > 0
    assert np.array_equal(idx[has], r["idx"][has]), f"{x.cid}: idx differs from the oracle"
    raw = A.get("idx").view(np.uint8).reshape(B, MQ, NS * 4)
    assert (raw[~has] == x.poison).all(), f"{x.cid}: rows of empty balls are documented as left untouched"
    assert (~has).any()
    x.keep("idx", np.where(has[..., None], idx, 0))


def _qb_io(x, A, r):
    A.add("p", r["p"], F32, "in", x.T)
    A.add("q", r["q"], F32, "in", x.T)
    A.add("idx", (B, MQ, NS), I32, "out", x.T)
    A.add("cnt", (B, MQ), I32, "out", x.T)


@case("rf_queryballpoint")
def queryballpoint(x):
    r = x.ref(lambda: _qb_ref(x))
    A = x.arena()
    _qb_io(x, A, r)
    A.build()
    x.call(A, "rf_queryballpoint", B, N, MQ, C.c_float(RAD), NS, "p", "q", "idx", "cnt", None)
    _qb_check(x, A, r)


@case("rf_queryballpoint")
def queryballpoint_empty_dataset(x):
    """n = 0: pts_cnt = 0, idx left as it was"""
    r = x.ref(lambda: _qb_ref(x, 0))
    A = x.arena()
    _qb_io(x, A, r)
    A.build()
    x.call(A, "rf_queryballpoint", B, 0, MQ, C.c_float(RAD), NS, "p", "q", "idx", "cnt", None)
    x.exact("cnt", A.get("cnt"), r["cnt"])
    x.poisoned(A, "idx")


@case("rf_queryballpoint_dev")
def queryballpoint_dev(x):
    r = x.ref(lambda: _qb_ref(x))
    A = x.arena()
    _qb_io(x, A, r)
    A.add("rad", r["rad"], F32, "in", x.L)
    A.build()
    x.call(A, "rf_queryballpoint_dev", B, N, MQ, "rad", NS, "p", "q", "idx", "cnt", None)
    _qb_check(x, A, r)


def _qb_boxes(x, dev_radius):
    r = x.ref(lambda: _qb_ref(x))
    A = x.arena()
    _qb_io(x, A, r)
    if dev_radius:
        A.add("rad", r["rad"], F32, "in", x.L)
    need = x.lib.rf_queryballpoint_boxes_workspace_bytes(B, N)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_queryballpoint_boxes", B, N, MQ, C.c_float(0.0 if dev_radius else RAD), "rad" if dev_radius else None, NS,
           "p", "q", None, "idx", "cnt", ws, wsz, None)
    _qb_check(x, A, r)


@case("rf_queryballpoint_boxes")
def queryballpoint_boxes(x):
    _qb_boxes(x, False)


@case("rf_queryballpoint_boxes")
def queryballpoint_boxes_device_radius(x):
    _qb_boxes(x, True)


@case("rf_queryballpoint_boxes", "rf_nn_sort")
def queryballpoint_boxes_sorted_handle(x):
    r = x.ref(lambda: _qb_ref(x))
    A = x.arena()
    _qb_io(x, A, r)
    A.add("h", (x.lib.rf_nn_sort_bytes(B, N),), U8, "out", x.W)
    ws, wsz = x.ws(A, x.lib.rf_queryballpoint_boxes_workspace_bytes(B, N))
    A.build()
    _sorted_handles(x, A, {"p": ("h", B, N)})
    x.call(A, "rf_queryballpoint_boxes", B, N, MQ, C.c_float(RAD), None, NS, "p", "q", "h", "idx", "cnt", ws, wsz, None)
    _qb_check(x, A, r)


def _qb_lengths(x, form):
    def mk():
        r = _qb_ref(x)
        l1, l2 = _counts(52, B, N), _counts(53, B, MQ)
        idx, cnt = np.zeros((B, MQ, NS), I32), np.zeros((B, MQ), I32)
        for i in range(B):
            r["p"][i, l1[i]:] = np.nan
            r["q"][i, l2[i]:] = r["p"][i, 0]
            oi, oc = x.orc.query_ball_point(F32(RAD), NS, r["p"][i:i + 1, :l1[i]], r["q"][i:i + 1, :l2[i]])
            idx[i, :l2[i]], cnt[i, :l2[i]] = np.where(oc[0][:, None] > 0, oi[0], 0), oc[0]
        r.update(l1=l1, l2=l2, idx=idx, cnt=cnt)
        return r
    r = x.ref(mk)
    A = x.arena()
    _qb_io(x, A, r)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    A.add("rad", r["rad"], F32, "in", x.L)
    need = x.lib.rf_queryballpoint_lengths_workspace_bytes(B, N, MQ, NS, form)
    assert (need > 0) == (form == 2)
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_queryballpoint_lengths", B, N, MQ, C.c_float(0.0), "rad", NS, "p", "q", "l1", "l2", "idx", "cnt", ws, wsz,
           None, form)
    x.exact("idx", A.get("idx"), r["idx"])  # every row written: empty balls and padded queries are zeros
    x.exact("cnt", A.get("cnt"), r["cnt"])


@case("rf_queryballpoint_lengths")
def queryballpoint_lengths_scan(x):
    _qb_lengths(x, 1)


@case("rf_queryballpoint_lengths")
def queryballpoint_lengths_boxes(x):
    _qb_lengths(x, 2)


def _sag_ref(x, ragged):
    p = np.random.RandomState(55).rand(B, N, 3).astype(F32)
    ln = _counts(56, B, N, 64) if ragged else np.full(B, N, I32)
    lo = _counts(57, B, MQ) if ragged else np.full(B, MQ, I32)
    fi, nx = np.zeros((B, MQ), I32), np.zeros((B, MQ, 3), F32)
    idx, cnt, gx = np.zeros((B, MQ, NS), I32), np.zeros((B, MQ), I32), np.zeros((B, MQ, NS, 3), F32)
    for i in range(B):
        p[i, ln[i]:] = np.nan
        s = p[i:i + 1, :ln[i]]
        f = x.orc.farthest_point_sample(int(lo[i]), s)
        q = x.orc.gather_point(s, f)
        oi, oc = x.orc.query_ball_point(F32(RAD), NS, s, q)
        fi[i, :lo[i]], nx[i, :lo[i]], idx[i, :lo[i]], cnt[i, :lo[i]] = f[0], q[0], oi[0], oc[0]
        gx[i, :lo[i]] = x.orc.group_point(s, oi)[0]
    return dict(p=p, ln=ln, lo=lo, fi=fi, nx=nx, idx=idx, cnt=cnt, gx=gx)


def _sag(x, ragged):
    r = x.ref(lambda: _sag_ref(x, ragged))
    A = x.arena()
    A.add("p", r["p"], F32, "in", x.T)
    if ragged:
        A.add("ln", r["ln"], I32, "in", x.L)
        A.add("lo", r["lo"], I32, "in", x.L)
    for k, shape, dt in (("fi", (B, MQ), I32), ("nx", (B, MQ, 3), F32), ("idx", (B, MQ, NS), I32), ("cnt", (B, MQ), I32),
                         ("gx", (B, MQ, NS, 3), F32)):
        A.add(k, shape, dt, "out", x.T)
    if ragged:
        need = x.lib.rf_sample_and_group_lengths_workspace_bytes(B, N)
    else:
        need = x.lib.rf_sample_and_group_workspace_bytes(B, N)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    if ragged:
        x.call(A, "rf_sample_and_group_lengths", B, N, MQ, C.c_float(RAD), None, NS, "p", "ln", "lo", "fi", "nx", "idx", "cnt",
               "gx", ws, wsz, None, None)
    else:
        x.call(A, "rf_sample_and_group", B, N, MQ, C.c_float(RAD), None, NS, "p", "fi", "nx", "idx", "cnt", "gx", ws, wsz, None,
               None)
    for k in ("fi", "nx", "idx", "cnt", "gx"):
        x.exact(k, A.get(k), r[k])


@case("rf_sample_and_group")
def sample_and_group(x):
    _sag(x, False)


@case("rf_sample_and_group_lengths")
def sample_and_group_lengths(x):
    _sag(x, True)


def _group_ref(x, b, n, m, ns, c, seed=61):
    rng = np.random.RandomState(seed + c)
    pts = rng.randn(b, n, c).astype(F32)
    idx = np.sort(rng.randint(0, n, (b, m, ns)), -1).astype(I32)
    idx[:, :min(m, 5)] = 7 % n  # a popular row
    go = rng.randn(b, m, ns, c).astype(F32)
    return dict(pts=pts, idx=idx, go=go)


def _grouppoint(x, c):
    b, n, m, ns = B, N, 37, 5

    def mk():
        r = _group_ref(x, b, n, m, ns, c)
        r["out"] = x.orc.group_point(r["pts"], r["idx"])
        return r
    r = x.ref(mk)
    A = x.arena()
    A.add("pts", r["pts"], F32, "in", x.T)  # natural, c = 64: grouping.hip's 4-wide form is not taken
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("out", (b, m, ns, c), F32, "out", x.T)
    A.build()
    x.call(A, "rf_grouppoint", b, n, c, m, ns, "pts", "idx", "out", None)
    x.exact("out", A.get("out"), r["out"])


@case("rf_grouppoint")
def grouppoint_c64(x):
    _grouppoint(x, 64)


@case("rf_grouppoint")
def grouppoint_c61(x):
    _grouppoint(x, 61)


def _grouppoint_grad(x, entry, b, n, m, ns, c, sorted_slots):
    def mk():
        r = _group_ref(x, b, n, m, ns, c)
        r["g"] = x.orc.group_point_grad(np.zeros((b, n, c), F32), r["idx"], r["go"])
        return r
    r = x.ref(mk)
    A = x.arena()
    A.add("go", r["go"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("g", (b, n, c), F32, "out", x.res(12))
    ws, wsz = None, 0
    if entry == "rf_grouppoint_grad_ws":
        need = x.lib.rf_grouppoint_grad_workspace_bytes(b, n, c, m, ns)
        assert (need > 0) == sorted_slots, "not the route under test"
        ws, wsz = x.ws(A, need)
    A.build()
    if entry == "rf_grouppoint_grad_ws":
        x.call(A, entry, b, n, c, m, ns, "go", "idx", "g", ws, wsz, None)
    else:
        x.call(A, entry, b, n, c, m, ns, "go", "idx", "g", None)
    if sorted_slots:  # test_gpu_scatter_rows.py's bar; sums in double, every row written once: the same bits in every run
        x.close("g", A.get("g"), r["g"], 1e-5, 1e-6 * max(1.0, _amax(r["g"])), fixed_order=True)
    else:             # test_gpu_sampling_grouping.py's bar
        x.close("g", A.get("g"), r["g"], 1e-5, 1e-6)


@case("rf_grouppoint_grad")
def grouppoint_grad_c64(x):
    _grouppoint_grad(x, "rf_grouppoint_grad", B, N, 37, 5, 64, False)


@case("rf_grouppoint_grad")
def grouppoint_grad_c61(x):
    _grouppoint_grad(x, "rf_grouppoint_grad", B, N, 37, 5, 61, False)


@case("rf_grouppoint_grad_ws")
def grouppoint_grad_ws_atomics(x):
    _grouppoint_grad(x, "rf_grouppoint_grad_ws", B, N, 37, 5, 64, False)


@case("rf_grouppoint_grad_ws")
def grouppoint_grad_ws_sorted_slots_c64(x):
    _grouppoint_grad(x, "rf_grouppoint_grad_ws", 3, 4099, 683, 32, 64, True)  # >= 2^22 gradient elements


@case("rf_grouppoint_grad_ws")
def grouppoint_grad_ws_sorted_slots_c61(x):
    _grouppoint_grad(x, "rf_grouppoint_grad_ws", 3, 4099, 719, 32, 61, True)


@case("rf_grouppoint_grad_ws")
def grouppoint_grad_ws_sorted_slots_c3(x):
    _grouppoint_grad(x, "rf_grouppoint_grad_ws", 8, 4099, 2049, 32, 3, True)  # >= 2^19 slots


@case("rf_selectionsort")
def selectionsort(x):
    b, n, m, k = 2, 33, 5, 7

    def mk():
        d = np.random.RandomState(63).rand(b, m, n).astype(F32)
        oi, ov = x.orc.select_top_k(k, d)
        return dict(d=d, oi=oi, ov=ov)
    r = x.ref(mk)
    A = x.arena()
    A.add("d", r["d"], F32, "in", x.T)
    A.add("oi", (b, m, n), I32, "out", x.T)
    A.add("ov", (b, m, n), F32, "out", x.T)
    A.build()
    x.call(A, "rf_selectionsort", b, n, m, k, "d", "oi", "ov", None)
    x.exact("oi", A.get("oi"), r["oi"])
    x.exact("ov", A.get("ov"), r["ov"])


# =============================================================================== neighbours ===
K = 7


def _knn_ref(x):
    a, q = np.random.RandomState(71).rand(B, N, 3).astype(F32), np.random.RandomState(72).rand(B, M, 3).astype(F32)
    val, idx = ref_knn(K, a, q)
    return dict(a=a, q=q, val=val, idx=idx.astype(I32))


def _knn_io(x, A, r):
    A.add("a", r["a"], F32, "in", x.T)
    A.add("q", r["q"], F32, "in", x.T)
    A.add("val", (B, M, K), F32, "out", x.T)
    A.add("idx", (B, M, K), I32, "out", x.T)


@case("rf_knn")
def knn(x):
    r = x.ref(lambda: _knn_ref(x))
    A = x.arena()
    _knn_io(x, A, r)
    A.build()
    x.call(A, "rf_knn", B, N, M, K, "a", "q", "val", "idx", None)
    x.exact("val", A.get("val"), r["val"])
    x.exact("idx", A.get("idx"), r["idx"])


@case("rf_knn_boxes")
def knn_boxes(x):
    r = x.ref(lambda: _knn_ref(x))
    A = x.arena()
    _knn_io(x, A, r)
    need = x.lib.rf_knn_boxes_workspace_bytes(B, N, M)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_knn_boxes", B, N, M, K, "a", "q", None, None, "val", "idx", ws, wsz, None)
    x.exact("val", A.get("val"), r["val"])
    x.exact("idx", A.get("idx"), r["idx"])


@case("rf_knn_boxes", "rf_nn_sort")
def knn_boxes_sorted_handles(x):
    r = x.ref(lambda: _knn_ref(x))
    A = x.arena()
    _knn_io(x, A, r)
    A.add("h1", (x.lib.rf_nn_sort_bytes(B, N),), U8, "out", x.W)
    A.add("h2", (x.lib.rf_nn_sort_bytes(B, M),), U8, "out", x.W)
    ws, wsz = x.ws(A, x.lib.rf_knn_boxes_workspace_bytes(B, N, M))
    A.build()
    _sorted_handles(x, A, {"a": ("h1", B, N), "q": ("h2", B, M)})
    x.call(A, "rf_knn_boxes", B, N, M, K, "a", "q", "h1", "h2", "val", "idx", ws, wsz, None)
    x.exact("val", A.get("val"), r["val"])
    x.exact("idx", A.get("idx"), r["idx"])


@case("rf_knn_grad")
def knn_grad(x):
    def mk():
        r = _knn_ref(x)
        r["gv"] = np.random.RandomState(73).randn(B, M, K).astype(F32)
        r["g1"], r["g2"] = np_grads(r["a"], r["q"], r["idx"].astype(np.int64), r["gv"])
        return r
    r = x.ref(mk)
    A = x.arena()
    for k, dt in (("a", F32), ("q", F32), ("idx", I32), ("gv", F32)):
        A.add(k, r[k], dt, "in", x.T)
    A.add("g1", (B, N, 3), F32, "out", x.res(4))
    A.add("g2", (B, M, 3), F32, "out", x.res(8))
    need = x.lib.rf_knn_grad_workspace_bytes(B, N, M, K)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_knn_grad", B, N, M, K, "a", "q", "idx", "gv", "g1", "g2", ws, wsz, None)
    # test_gpu_knn.py's bar; every row written once from sums in double: the same bits in every run
    x.close("g1", A.get("g1"), r["g1"], 1e-5, 1e-6, fixed_order=True)
    x.close("g2", A.get("g2"), r["g2"], 1e-5, 1e-6, fixed_order=True)


def _knn_lengths_ref(x):
    r = _knn_ref(x)
    l1, l2 = _counts(74, B, N), _counts(75, B, M)
    l1[-1] = K - 2  # fewer candidates than k: their neighbours in the first slots, zeros behind
    val, idx = np.zeros((B, M, K), F32), np.zeros((B, M, K), I32)
    gv = np.random.RandomState(76).randn(B, M, K).astype(F32)
    g1, g2 = np.zeros((B, N, 3), F32), np.zeros((B, M, 3), F32)
    for i in range(B):
        r["a"][i, l1[i]:] = np.nan
        r["q"][i, l2[i]:] = 1e30
        k = min(K, int(l1[i]))
        sa, sq = r["a"][i:i + 1, :l1[i]], r["q"][i:i + 1, :l2[i]]
        v, ix = ref_knn(k, sa, sq)
        val[i, :l2[i], :k], idx[i, :l2[i], :k] = v[0], ix[0]
        e1, e2 = np_grads(sa, sq, ix, gv[i:i + 1, :l2[i], :k])
        g1[i, :l1[i]], g2[i, :l2[i]] = e1[0], e2[0]
    r.update(l1=l1, l2=l2, val=val, idx=idx, gv=gv, g1=g1, g2=g2)
    return r


def _knn_lengths(x, form):
    r = x.ref(lambda: _knn_lengths_ref(x))
    A = x.arena()
    _knn_io(x, A, r)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    need = x.lib.rf_knn_lengths_workspace_bytes(B, N, M, K, form)
    assert (need > 0) == (form == 2)
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_knn_lengths", B, N, M, K, "a", "q", "l1", "l2", "val", "idx", ws, wsz, None, form)
    x.exact("val", A.get("val"), r["val"])
    x.exact("idx", A.get("idx"), r["idx"])


@case("rf_knn_lengths")
def knn_lengths_scan(x):
    _knn_lengths(x, 1)


@case("rf_knn_lengths")
def knn_lengths_boxes(x):
    _knn_lengths(x, 2)


@case("rf_knn_grad_lengths")
def knn_grad_lengths(x):
    r = x.ref(lambda: _knn_lengths_ref(x))
    rng = np.random.RandomState(77)
    idx = r["idx"].copy()
    for i in range(B):  # slots of padded queries and slots t >= len1 hold anything
        idx[i, r["l2"][i]:] = rng.randint(-5, N + 5, idx[i, r["l2"][i]:].shape)
        idx[i, :, min(K, int(r["l1"][i])):] = rng.randint(-5, N + 5, idx[i, :, min(K, int(r["l1"][i])):].shape)
    A = x.arena()
    for k, v, dt in (("a", r["a"], F32), ("q", r["q"], F32), ("idx", idx, I32), ("gv", r["gv"], F32)):
        A.add(k, v, dt, "in", x.T)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    A.add("g1", (B, N, 3), F32, "out", x.res(12))
    A.add("g2", (B, M, 3), F32, "out", x.res(4))
    need = x.lib.rf_knn_grad_lengths_workspace_bytes(B, N, M, K)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_knn_grad_lengths", B, N, M, K, "a", "q", "l1", "l2", "idx", "gv", "g1", "g2", ws, wsz, None)
    for k, l in (("g1", r["l1"]), ("g2", r["l2"])):
        got = A.get(k)
        check_padding_zero(got, l, 1, k)
        x.close(k, got, r[k], 1e-5, 1e-6, fixed_order=True)


def _tnn_ref(x):
    a, c = np.random.RandomState(81).rand(B, N, 3).astype(F32), np.random.RandomState(82).rand(B, M, 3).astype(F32)
    d, i = x.orc.three_nn(a, c)
    return dict(a=a, c=c, d=d, i=i)


def _tnn_io(x, A, r):
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("d", (B, N, 3), F32, "out", x.T)
    A.add("i", (B, N, 3), I32, "out", x.T)


@case("rf_threenn")
def threenn(x):
    r = x.ref(lambda: _tnn_ref(x))
    A = x.arena()
    _tnn_io(x, A, r)
    A.build()
    x.call(A, "rf_threenn", B, N, M, "a", "c", "d", "i", None)
    x.exact("d", A.get("d"), r["d"])
    x.exact("i", A.get("i"), r["i"])


@case("rf_threenn_boxes")
def threenn_boxes(x):
    r = x.ref(lambda: _tnn_ref(x))
    A = x.arena()
    _tnn_io(x, A, r)
    need = x.lib.rf_threenn_boxes_workspace_bytes(B, N, M)
    assert need > 0
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_threenn_boxes", B, N, M, "a", "c", None, None, "d", "i", ws, wsz, None)
    x.exact("d", A.get("d"), r["d"])
    x.exact("i", A.get("i"), r["i"])


def _tnn_lengths(x, form):
    def mk():
        r = _tnn_ref(x)
        l1, l2 = _counts(83, B, N), _counts(84, B, M, 3)
        d, ix = np.zeros((B, N, 3), F32), np.zeros((B, N, 3), I32)
        for i in range(B):
            r["a"][i, l1[i]:] = np.nan
            r["c"][i, l2[i]:] = r["c"][i, 0]
            od, oi = x.orc.three_nn(r["a"][i:i + 1, :l1[i]], r["c"][i:i + 1, :l2[i]])
            d[i, :l1[i]], ix[i, :l1[i]] = od[0], oi[0]
        r.update(l1=l1, l2=l2, d=d, i=ix)
        return r
    r = x.ref(mk)
    A = x.arena()
    _tnn_io(x, A, r)
    A.add("l1", r["l1"], I32, "in", x.L)
    A.add("l2", r["l2"], I32, "in", x.L)
    need = x.lib.rf_threenn_lengths_workspace_bytes(B, N, M, form)
    assert (need > 0) == (form == 2)
    ws, wsz = x.ws(A, need)
    A.build()
    x.call(A, "rf_threenn_lengths", B, N, M, "a", "c", "l1", "l2", "d", "i", ws, wsz, None, form)
    x.exact("d", A.get("d"), r["d"])
    x.exact("i", A.get("i"), r["i"])


@case("rf_threenn_lengths")
def threenn_lengths_scan(x):
    _tnn_lengths(x, 1)


@case("rf_threenn_lengths")
def threenn_lengths_boxes(x):
    _tnn_lengths(x, 2)


def _interp_ref(x, b, n, m, c, seed=85):
    rng = np.random.RandomState(seed + c)
    pts = rng.randn(b, m, c).astype(F32)
    idx = rng.randint(0, m, (b, n, 3)).astype(I32)
    idx[:, ::7, 1] = idx[:, ::7, 0]
    w = rng.rand(b, n, 3).astype(F32)
    go = rng.randn(b, n, c).astype(F32)
    return dict(pts=pts, idx=idx, w=w, go=go)


def _threeinterpolate(x, c):
    def mk():
        r = _interp_ref(x, B, N, M, c)
        r["out"] = x.orc.three_interpolate(r["pts"], r["idx"], r["w"])
        return r
    r = x.ref(mk)
    A = x.arena()
    A.add("pts", r["pts"], F32, "in", x.T)  # natural, c = 64: interpolate.hip's 4-wide form is not taken
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("w", r["w"], F32, "in", x.T)
    A.add("out", (B, N, c), F32, "out", x.T)
    A.build()
    x.call(A, "rf_threeinterpolate", B, M, c, N, "pts", "idx", "w", "out", None)
    x.exact("out", A.get("out"), r["out"])


@case("rf_threeinterpolate")
def threeinterpolate_c64(x):
    _threeinterpolate(x, 64)


@case("rf_threeinterpolate")
def threeinterpolate_c61(x):
    _threeinterpolate(x, 61)


def _threeinterpolate_grad(x, entry, b, n, c, m, route):
    """route: 'tile' (the known points fit the LDS tile), 'sorted' (sorted slots), 'atomics'"""
    def mk():
        r = _interp_ref(x, b, n, m, c)
        r["g"] = x.orc.three_interpolate_grad(np.zeros((b, m, c), F32), r["idx"], r["w"], r["go"])
        return r
    r = x.ref(mk)
    A = x.arena()
    A.add("go", r["go"], F32, "in", x.T)
    A.add("idx", r["idx"], I32, "in", x.T)
    A.add("w", r["w"], F32, "in", x.T)
    A.add("g", (b, m, c), F32, "out", x.res(8))
    need = x.lib.rf_threeinterpolate_grad_workspace_bytes(b, n, c, m)
    assert (need > 0) == (route == "sorted"), "not the route under test"
    fits_tile = (c % 8 == 0 and m * 8 <= 16384) or (c <= 64 and m * c <= 16384)  # interpolate.hip tig_tile_cs
    assert fits_tile == (route == "tile"), "not the route under test"
    ws, wsz = None, 0
    if entry == "rf_threeinterpolate_grad_ws":
        ws, wsz = x.ws(A, need)
    A.build()
    if entry == "rf_threeinterpolate_grad_ws":
        x.call(A, entry, b, n, c, m, "go", "idx", "w", "g", ws, wsz, None)
    else:
        x.call(A, entry, b, n, c, m, "go", "idx", "w", "g", None)
    if route == "sorted":  # test_gpu_scatter_rows.py's bar
        x.close("g", A.get("g"), r["g"], 1e-5, 1e-6 * max(1.0, _amax(r["g"])), fixed_order=True)
    else:                  # test_gpu_sampling_grouping.py's bar
        x.close("g", A.get("g"), r["g"], 1e-5, 1e-5)


@case("rf_threeinterpolate_grad")
def threeinterpolate_grad_tile_c64(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad", B, N, 64, M, "tile")


@case("rf_threeinterpolate_grad")
def threeinterpolate_grad_tile_c61(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad", B, N, 61, M, "tile")


@case("rf_threeinterpolate_grad")
def threeinterpolate_grad_atomics(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad", 2, N, 64, 2051, "atomics")


@case("rf_threeinterpolate_grad_ws")
def threeinterpolate_grad_ws_tile_c64(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad_ws", B, N, 64, M, "tile")


@case("rf_threeinterpolate_grad_ws")
def threeinterpolate_grad_ws_sorted_slots_c64(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad_ws", 2, 10923, 64, 2051, "sorted")


@case("rf_threeinterpolate_grad_ws")
def threeinterpolate_grad_ws_sorted_slots_c61(x):
    _threeinterpolate_grad(x, "rf_threeinterpolate_grad_ws", 2, 11503, 61, 2051, "sorted")


# =============================================================================== other ========
@case("rf_auctionmatch")
def auctionmatch(x):
    n = 101

    def mk():
        rng = np.random.RandomState(91)
        a = rng.randn(B, n, 3).astype(F32)
        c = np.roll(a + 0.01 * rng.randn(B, n, 3).astype(F32), 5, axis=1)
        ml, mr = x.orc.auction_match(a, c)
        return dict(a=a, c=c, ml=ml, mr=mr)
    r = x.ref(mk)
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("ml", (B, n), I32, "out", x.T)
    A.add("mr", (B, n), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_auctionmatch_workspace_bytes(B, n))
    A.build()
    x.call(A, "rf_auctionmatch", B, n, "a", "c", "ml", "mr", ws, wsz, None)
    x.exact("ml", A.get("ml"), r["ml"])
    x.exact("mr", A.get("mr"), r["mr"])


@case("rf_probe_exp2")
def probe_exp2(x):
    v = np.array([0.0, -1.0, -10.0, -126.0, 3.0, -160.0, -200.0], F32)
    A = x.arena()
    A.add("x", v, F32, "in", x.T)
    A.add("y", (7,), F32, "out", x.T)
    A.build()
    x.call(A, "rf_probe_exp2", "x", "y", 7, None)
    got = A.get("y")
    assert np.allclose(got[:5], np.exp2(v[:5].astype(np.float64)), rtol=1e-6) and (got[5:] == 0).all()  # test_gpu_emd.py
    x.keep("y", got)


CF = 68  # channels of the layer-tail helpers: a multiple of 4 that is no power of two (17 quads, 15 points per pass)


def _feat(seed):
    xv = np.random.RandomState(seed).randn(B, N, CF).astype(F32)
    xv[:, 3] = xv[:, 1]  # ties: the lower point index wins
    return xv


@case("rf_maxpool_points")
def maxpool_points(x):
    r = x.ref(lambda: dict(x=_feat(93)))
    A = x.arena()
    A.add("x", r["x"], F32, "in", x.T16)
    A.add("out", (B, CF), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_maxpool_points_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_maxpool_points", B, N, CF, "x", "out", ws, wsz, None)
    x.exact("out", A.get("out"), r["x"].max(1))


@case("rf_maxpool_points_idx")
def maxpool_points_idx(x):
    r = x.ref(lambda: dict(x=_feat(93)))
    A = x.arena()
    A.add("x", r["x"], F32, "in", x.T16)
    A.add("out", (B, CF), F32, "out", x.T)
    A.add("idx", (B, CF), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_maxpool_points_idx_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_maxpool_points_idx", B, N, CF, "x", "out", "idx", ws, wsz, None)
    x.exact("out", A.get("out"), r["x"].max(1))
    x.exact("idx", A.get("idx"), r["x"].argmax(1).astype(I32))  # numpy's argmax: the first position of the maximum


def _colsum_ref():
    grad, out = _feat(95), _feat(96)
    out[0, 0, 0] = 0.0  # relu: zero is NOT positive
    g = np.where(out > 0, grad, F32(0))
    return dict(grad=grad, out=out, g=g, sums=g.astype(np.float64).sum(1))


def _colsum_check(x, A, r, gname):
    x.exact("g", A.get(gname), r["g"])
    # test_rfnet_model.py's bar; a fixed summation order: the same bits in every run
    x.close("sums", A.get("sums"), r["sums"], 1e-5, 1e-5 * _amax(r["sums"]) + 1e-6, fixed_order=True)


@case("rf_act_grad_colsum")
def act_grad_colsum(x):
    r = x.ref(_colsum_ref)
    A = x.arena()
    A.add("grad", r["grad"], F32, "in", x.T16)
    A.add("out", r["out"], F32, "in", x.T16)
    A.add("g", (B, N, CF), F32, "out", x.T16)
    A.add("sums", (B, CF), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_act_grad_colsum_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_act_grad_colsum", B, N, CF, "grad", "out", 1, "g", "sums", ws, wsz, None)
    _colsum_check(x, A, r, "g")


@case("rf_act_grad_colsum")
def act_grad_colsum_in_place(x):
    r = x.ref(_colsum_ref)
    A = x.arena()
    A.add("grad", r["grad"], F32, "inout", x.T16)
    A.add("out", r["out"], F32, "in", x.T16)
    A.add("sums", (B, CF), F32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_act_grad_colsum_workspace_bytes(B, N, CF))
    A.build()
    x.call(A, "rf_act_grad_colsum", B, N, CF, "grad", "out", 1, "grad", "sums", ws, wsz, None)
    _colsum_check(x, A, r, "grad")


@case("rf_act_grad_colsum")
def act_grad_colsum_no_points(x):
    """n = 0: sums zero-filled by the call, nothing else touched"""
    A = x.arena()
    A.add("sums", (B, CF), F32, "out", x.T)
    A.build()
    x.call(A, "rf_act_grad_colsum", B, 0, CF, None, None, 1, None, "sums", None, 0, None)
    x.exact("sums", A.get("sums"), np.zeros((B, CF), F32))


@case("rf_point_affine")
def point_affine(x):
    kp = 3

    def mk():
        rng = np.random.RandomState(97)
        y, p = rng.randn(B, N, CF).astype(F32), rng.randn(B, N, kp).astype(F32)
        w, r_ = rng.randn(kp, CF).astype(F32), rng.randn(B, CF).astype(F32)
        ref = y.astype(np.float64) + p.astype(np.float64) @ w.astype(np.float64) + r_.astype(np.float64)[:, None]
        return dict(y=y, p=p, w=w, r=r_, out=np.maximum(ref, 0))
    r = x.ref(mk)
    A = x.arena()
    A.add("y", r["y"], F32, "in", x.T16)
    A.add("p", r["p"], F32, "in", x.T)
    A.add("w", r["w"], F32, "in", x.T16)
    A.add("r", r["r"], F32, "in", x.T16)
    A.add("out", (B, N, CF), F32, "out", x.T16)
    A.build()
    x.call(A, "rf_point_affine", B, N, CF, "y", "p", kp, "w", "r", 1, 1, "out", None)
    x.close("out", A.get("out"), r["out"], 1e-5, 1e-5)  # test_rfnet_model.py's bar


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", list(CASES))
def test_memory_contract(orc, cid, variant, poison):
    x = Ctx(cid, variant, poison, orc)
    _SEEN[cid] = _SEEN.get(cid, 0) + 1
    try:
        CASES[cid][1](x)
        assert x.kept, "a case must check at least one output"
        x.across_runs()
    finally:
        if _SEEN[cid] == RUNS_PER_CASE:
            _REFS.pop(cid, None)
            _RUNS.pop(cid, None)


def test_layer_tail_entries_refuse_less_aligned_tensors():
    """The four pointmlp.hip entries read and write their (.., c) tensors as float4: a tensor that is valid but only
    4- or 8-byte aligned is RF_EINVAL before anything is launched (status only: the arena shows that nothing was written)."""
    from rfnet_amd._lib import lib
    for off in (4, 8):
        A = Arena("cuda", 0xFF)
        xv = _feat(99)
        A.add("x", xv, F32, "in", off)
        A.add("x16", xv, F32, "in", 0)
        A.add("w", xv[0, :3].copy(), F32, "in", off)
        A.add("w16", xv[0, :3].copy(), F32, "in", 0)
        A.add("r", xv[:, 0].copy(), F32, "in", off)
        A.add("r16", xv[:, 0].copy(), F32, "in", 0)
        A.add("p", xv[:, :, :3].copy(), F32, "in", 0)
        A.add("big", (B, N, CF), F32, "out", off)
        A.add("big16", (B, N, CF), F32, "out", 0)
        A.add("small", (B, CF), F32, "out", 0)
        A.add("idx", (B, CF), I32, "out", 0)
        need = lib.rf_maxpool_points_idx_workspace_bytes(B, N, CF)
        A.add("ws", (need,), U8, "scratch", 0)
        A.add("wsoff", (need,), U8, "scratch", off)
        A.build()
        P = A.ptr
        assert lib.rf_maxpool_points(B, N, CF, P("x"), P("small"), P("ws"), need, None) == RF_EINVAL
        assert lib.rf_maxpool_points(B, N, CF, P("x16"), P("small"), P("wsoff"), need, None) == RF_EINVAL
        assert lib.rf_maxpool_points_idx(B, N, CF, P("x"), P("small"), P("idx"), P("ws"), need, None) == RF_EINVAL
        assert lib.rf_maxpool_points_idx(B, N, CF, P("x16"), P("small"), P("idx"), P("wsoff"), need, None) == RF_EINVAL
        for grad, out, g in (("x", "x16", "big16"), ("x16", "x", "big16"), ("x16", "x16", "big")):
            assert lib.rf_act_grad_colsum(B, N, CF, P(grad), P(out), 1, P(g), P("small"), P("ws"), need, None) == RF_EINVAL
        assert lib.rf_act_grad_colsum(B, N, CF, P("x16"), P("x16"), 1, P("big16"), P("small"), P("wsoff"), need, None) == RF_EINVAL
        for y, w, r_, out in (("x", "w16", "r16", "big16"), ("x16", "w", "r16", "big16"), ("x16", "w16", "r", "big16"),
                              ("x16", "w16", "r16", "big")):
            assert lib.rf_point_affine(B, N, CF, P(y), P("p"), 3, P(w), P(r_), 1, 1, P(out), None) == RF_EINVAL
        for b in A.bufs.values():
            b.role = "in"  # nothing at all may have been written
        A.check("refused calls")
