"""GPU: the memory contract of include/rfops.h for rf_expansion_penalty, rf_expansion_penalty_grad and rf_mds (DESIGN.md
5.3n), straight through the C ABI: dist / father / length exactly (b, n), mean / info exactly (b, P), the gradient exactly
(b, n, 3), MDS' out exactly (b, m), info (b) and the emitted coordinates (b, m, 3) or NULL; no workspace; inputs, outputs,
the scale and the count array at the residues the header allows (4 bytes); a non-finite patch between healthy ones, counts
with 1 and n among them over NaN padding and more samples asked for than a cloud has; after the call every byte outside
the outputs is unchanged and every output slot is written.

The cases use the machinery of tests/test_gpu_memory_contract.py and register themselves in its CASES table when this
module is imported, exactly as tests/test_gpu_memory_contract_emd_assign.py does; `test_memory_contract_msn` runs them."""
import numpy as np
import pytest

import test_gpu_memory_contract as T
from test_gpu_memory_contract import F32, I32, case
from test_gpu_msn_ops import bits, xp_batch, xp_expect, xp_grad_close, xp_grad_ref, xp_trees
from test_msn_ops_host import MDS_BADSIGMA, MDS_OK, XP_NONFINITE, mds_ref

pytestmark = pytest.mark.gpu

_OWN = []  # the case ids this module registers, in order


def own(*entries):
    def reg(fn):
        assert fn.__name__ not in T.CASES, fn.__name__
        _OWN.append(fn.__name__)
        return case(*entries)(fn)
    return reg


B, S, P = 3, 67, 3  # 67 points: the one-wave form with its last lanes empty
N = S * P
ALPHA = 1.0


def _xp_ref():
    xyz = xp_batch("uniform", S, B, P, 90)
    xyz[1] = xp_batch("lattice", S, 1, P, 91)[0]
    xyz[2, S + 5, 1] = np.nan  # one patch is reported, its neighbours are not touched
    trees = xp_trees(xyz, S)
    e = xp_expect(trees, S, ALPHA)
    g = np.random.RandomState(92).randn(B, N).astype(F32)
    return dict(xyz=xyz, trees=trees, g=g, grad=xp_grad_ref(np.nan_to_num(xyz), S, trees, ALPHA, g), **e)


@own("rf_expansion_penalty")
def expansion_penalty_with_a_non_finite_patch(x):
    r = x.ref(_xp_ref)
    A = x.arena()
    A.add("xyz", r["xyz"], F32, "in", x.T)
    A.add("dist", (B, N), F32, "out", x.res(4))
    A.add("father", (B, N), I32, "out", x.res(8))
    A.add("length", (B, N), F32, "out", x.res(12))
    A.add("mean", (B, P), F32, "out", x.T)
    A.add("info", (B, P), I32, "out", x.res(4))
    A.build()
    x.call(A, "rf_expansion_penalty", B, N, S, ALPHA, "xyz", "dist", "father", "length", "mean", "info", None)
    assert A.get("dist").nbytes == B * N * 4 and A.get("mean").nbytes == B * P * 4 and A.get("info").nbytes == B * P * 4
    for k in ("dist", "father", "length", "mean", "info"):
        got = A.get(k)
        assert got.shape == r[k].shape and bits(got).tobytes() == bits(r[k]).tobytes(), f"{x.cid}: {k} differs from the reference"
        x.keep(k, got)
    assert A.get("info")[2, 1] == XP_NONFINITE and A.get("info").sum() == XP_NONFINITE


@own("rf_expansion_penalty_grad")
def expansion_penalty_grad_with_a_non_finite_patch(x):
    r = x.ref(_xp_ref)
    A = x.arena()
    A.add("xyz", r["xyz"], F32, "in", x.T)
    A.add("father", r["father"], I32, "in", x.res(8))
    A.add("dist", r["dist"], F32, "in", x.T)
    A.add("g", r["g"], F32, "in", x.res(12))
    A.add("grad", (B, N, 3), F32, "out", x.res(4))
    A.build()
    x.call(A, "rf_expansion_penalty_grad", B, N, S, "xyz", "father", "dist", "g", "grad", None)
    got = A.get("grad")
    assert got.shape == (B, N, 3) and got.nbytes == B * N * 12
    xp_grad_close(got, r["grad"], x.cid)  # test_gpu_msn_ops.py's bar; exactly +0 where nothing contributes
    assert not bits(got[2, S:2 * S]).any()  # the reported patch has no penalised edge
    x.keep("grad", got)


MB, MN, MM = 5, 131, 90
MLEN = np.array([MN, 1, 77, 100, 131], I32)
MSIGMA = np.array([0.1, 0.1, 0.05, 0.0, 0.3], F32)


def _mds_ref():
    xyz = np.random.RandomState(93).rand(MB, MN, 3).astype(F32)
    for i in range(MB):
        xyz[i, MLEN[i]:] = np.nan
    ragged = [mds_ref(xyz[i], MM, MSIGMA[i], MLEN[i]) for i in range(MB)]
    pack = lambda rs: (np.stack([q[0] for q in rs]), np.array([q[1] for q in rs], I32), np.stack([q[2] for q in rs]))  # noqa: E731
    return dict(xyz=xyz, ragged=pack(ragged))


@own("rf_mds")
def mds_ragged_with_coordinates(x):
    r = x.ref(_mds_ref)
    A = x.arena()
    A.add("xyz", r["xyz"], F32, "in", x.T)
    A.add("sigma", MSIGMA, F32, "in", x.L)
    A.add("len", MLEN, I32, "in", x.L)
    A.add("out", (MB, MM), I32, "out", x.res(8))
    A.add("info", (MB,), I32, "out", x.res(4))
    A.add("nx", (MB, MM, 3), F32, "out", x.res(12))
    A.build()
    x.call(A, "rf_mds", MB, MN, MM, "xyz", "sigma", "len", "out", "info", "nx", None)
    out, info, nx = r["ragged"]
    assert A.get("out").nbytes == MB * MM * 4 and A.get("info").nbytes == MB * 4 and A.get("nx").nbytes == MB * MM * 12
    x.exact("out", A.get("out"), out)
    x.exact("info", A.get("info"), info)
    assert bits(A.get("nx")).tobytes() == bits(nx).tobytes()  # +0 behind min(m, count) included
    x.keep("nx", A.get("nx"))
    assert info.tolist() == [MDS_OK, MDS_OK, MDS_OK, MDS_BADSIGMA, MDS_OK] and not out[1].any() and not out[2, 77:].any()


@own("rf_mds")
def mds_indices_only(x):
    """No counts and no coordinates: both pointers NULL.  The padding of the ragged case is data here; the samples with a
    full count give the same indices as there."""
    r = x.ref(_mds_ref)
    A = x.arena()
    xyz = np.nan_to_num(r["xyz"], nan=0.25)
    A.add("xyz", xyz, F32, "in", x.T)
    A.add("sigma", MSIGMA, F32, "in", x.L)
    A.add("out", (MB, MM), I32, "out", x.res(12))
    A.add("info", (MB,), I32, "out", x.T)
    A.build()
    x.call(A, "rf_mds", MB, MN, MM, "xyz", "sigma", None, "out", "info", None, None)
    exp = np.stack([mds_ref(xyz[i], MM, MSIGMA[i])[0] for i in range(MB)])
    x.exact("out", A.get("out"), exp)
    x.keep("info", A.get("info"))
    assert np.array_equal(A.get("out")[[0, 4]], r["ragged"][0][[0, 4]])


# =============================================================================== the runs =====
@pytest.mark.parametrize("poison", [0xFF, 0x5A], ids=["ff", "5a"])
@pytest.mark.parametrize("variant", ["aligned", "natural"])
@pytest.mark.parametrize("cid", _OWN)
def test_memory_contract_msn(orc, cid, variant, poison):
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
