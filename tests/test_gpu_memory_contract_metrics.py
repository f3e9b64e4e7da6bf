"""GPU: the memory contract of include/rfops.h for the Chamfer metrics entries: rf_nn_metrics,
rf_chamfer_metrics and rf_chamfer_metrics_grad straight through the C ABI, on guarded, poisoned buffers at the residues
the header allows (tensors and count arrays 4 bytes, the workspace 16), with ragged counts that include 1 and the full size.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this module
is imported, exactly as tests/test_gpu_memory_contract_model.py does (see its docstring for what that means for a run of
tests/test_memory_contract_host.py on its own); `test_memory_contract_metrics` here runs them."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_chamfer_metrics_host import NCOL, grad_weights_ref, metrics_ref
from test_gpu_memory_contract import B, F32, I32, M, N, case

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


LEN1 = np.array([N, 1, 129], I32)
LEN2 = np.array([77, M, 1], I32)
TAU2, ALPHA = F32(0.1) * F32(0.1), 40.0


def _ref(x):
    """Sample by sample on the unpadded slices; padding: NaN behind len1, copies of the sample's own valid xyz1 points
    behind len2 (distance 0: read, they would win every search and be counted)."""
    rng = np.random.RandomState(41)
    a, c = (rng.rand(B, N, 3) - 0.5).astype(F32), (rng.rand(B, M, 3) - 0.5).astype(F32)
    gm = rng.randn(B, NCOL).astype(F32)
    r = dict(d1=np.zeros((B, N), F32), i1=np.full((B, N), -1, I32), d2=np.zeros((B, M), F32), i2=np.full((B, M), -1, I32),
             c1=np.zeros((B, N), I32), c2=np.zeros((B, M), I32), met=np.zeros((B, NCOL)),
             g1=np.zeros((B, N, 3), F32), g2=np.zeros((B, M, 3), F32))
    for i, (n_, m_) in enumerate(zip(LEN1, LEN2)):
        c[i, m_:] = a[i, np.arange(M - m_) % n_]
        a[i, n_:] = np.nan
        ai, ci = a[i:i + 1, :n_].copy(), c[i:i + 1, :m_].copy()
        e = x.orc.nn_distance(ai, ci)
        r["d1"][i, :n_], r["i1"][i, :n_], r["d2"][i, :m_], r["i2"][i, :m_] = e[0][0], e[1][0], e[2][0], e[3][0]
        r["met"][i], r["c1"][i, :n_], r["c2"][i, :m_] = metrics_ref(e[0][0], e[1][0], e[2][0], e[3][0], TAU2, ALPHA)
        gd1 = grad_weights_ref(e[0][0], e[1][0], r["c2"][i], gm[i], 1, ALPHA).astype(F32)
        gd2 = grad_weights_ref(e[2][0], e[3][0], r["c1"][i], gm[i], 2, ALPHA).astype(F32)
        g = x.orc.nn_distance_grad(ai, ci, gd1[None], e[1], gd2[None], e[3])
        r["g1"][i, :n_], r["g2"][i, :m_] = g[0][0], g[1][0]
    gm_nan = gm.copy()
    gm_nan[:, 4:9] = np.nan  # columns without a gradient: never read
    r.update(a=a, c=c, gm=gm_nan)
    return r


def _check_metrics(x, A, r):
    met = A.get("met")
    x.exact("met[4:8]", met[:, 4:8], r["met"][:, 4:8].astype(F32))
    x.close("met[8]", met[:, 8], r["met"][:, 8], 1e-6, fixed_order=True)
    x.close("met[0:4]", met[:, 0:4], r["met"][:, 0:4], 1e-5, fixed_order=True)
    x.close("met[9:11]", met[:, 9:11], r["met"][:, 9:11], 1e-5, 1e-6, fixed_order=True)
    x.exact("c1", A.get("c1"), r["c1"])
    x.exact("c2", A.get("c2"), r["c2"])


@own("rf_nn_metrics")
def nn_metrics_lengths(x):
    r = x.ref(lambda: _ref(x))
    A = x.arena()
    for k, dt in (("d1", F32), ("i1", I32), ("d2", F32), ("i2", I32)):
        v = r[k].copy()
        for i, ln in enumerate(LEN1 if k[1] == "1" else LEN2):  # padded slots are not read: poison of their own
            v[i, ln:] = np.nan if dt is F32 else (1 << 30)
        A.add(k, v, dt, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("met", (B, NCOL), F32, "out", x.T)
    A.add("c1", (B, N), I32, "out", x.T)
    A.add("c2", (B, M), I32, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_nn_metrics_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_nn_metrics", B, N, M, "d1", "i1", "d2", "i2", "l1", "l2", float(TAU2), ALPHA, "met", "c1", "c2", ws, wsz, None)
    _check_metrics(x, A, r)


@own("rf_chamfer_metrics")
def chamfer_metrics_lengths(x):
    r = x.ref(lambda: _ref(x))
    A = x.arena()
    A.add("a", r["a"], F32, "in", x.T)
    A.add("c", r["c"], F32, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("met", (B, NCOL), F32, "out", x.T)
    for k, shape, dt in (("d1", (B, N), F32), ("i1", (B, N), I32), ("d2", (B, M), F32), ("i2", (B, M), I32),
                         ("c1", (B, N), I32), ("c2", (B, M), I32)):
        A.add(k, shape, dt, "out", x.T)
    ws, wsz = x.ws(A, x.lib.rf_chamfer_metrics_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_chamfer_metrics", B, N, M, "a", "c", "l1", "l2", float(TAU2), ALPHA, "met", "d1", "i1", "d2", "i2", "c1", "c2",
           ws, wsz, None)
    T._nn_check(x, A, (r["d1"], r["i1"], r["d2"], r["i2"]))  # padded slots: dist 0, idx -1
    _check_metrics(x, A, r)


@own("rf_chamfer_metrics_grad")
def chamfer_metrics_grad_lengths(x):
    r = x.ref(lambda: _ref(x))
    A = x.arena()
    for k, dt in (("a", F32), ("c", F32), ("d1", F32), ("i1", I32), ("d2", F32), ("i2", I32), ("c1", I32), ("c2", I32), ("gm", F32)):
        A.add(k, r[k], dt, "in", x.T)
    A.add("l1", LEN1, I32, "in", x.L)
    A.add("l2", LEN2, I32, "in", x.L)
    A.add("g1", (B, N, 3), F32, "out", x.res(4))
    A.add("g2", (B, M, 3), F32, "out", x.res(12))
    ws, wsz = x.ws(A, x.lib.rf_chamfer_metrics_grad_workspace_bytes(B, N, M))
    A.build()
    x.call(A, "rf_chamfer_metrics_grad", B, N, M, "a", "c", "l1", "l2", "d1", "i1", "d2", "i2", "c1", "c2", ALPHA, "gm", "g1", "g2",
           ws, wsz, None)
    g1, g2 = A.get("g1"), A.get("g2")
    for i, (n_, m_) in enumerate(zip(LEN1, LEN2)):  # exactly +0 behind the counts
        assert not g1[i, n_:].any() and not np.signbit(g1[i, n_:]).any() and not g2[i, m_:].any() and not np.signbit(g2[i, m_:]).any(), i
    x.close("g1", g1, r["g1"], 1e-4, 1e-5)  # rfops.h's bar for fused gradients
    x.close("g2", g2, r["g2"], 1e-4, 1e-5)


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_metrics(orc, cid, variant, poison):
    x = T.Ctx(cid, variant, poison, orc)
    T._SEEN[cid] = T._SEEN.get(cid, 0) + 1
    try:
        T.CASES[cid][1](x)
        assert x.kept, "a case must check at least one output"
        x.across_runs()
    finally:
        if T._SEEN[cid] == T.RUNS_PER_CASE:
            T._REFS.pop(cid, None)
            T._RUNS.pop(cid, None)
