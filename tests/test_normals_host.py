"""CPU: surface normals by local PCA and normal consistency (include/rfops.h, "surface normals") at the boundary -- declared,
exported, bound; every argument rule answered before a device is touched; the wrappers' checks -- and pca_ref / nc_ref, the
numpy restatements of the contract that the GPU tests hold the kernels to (pca_ref bit for bit).  The restatements are checked
here: the Jacobi sweeps against numpy.linalg.eigh on planes, exact-grid planes, lines, duplicates, balls and clouds scaled by
1e18 and 1e-30, and cases by hand.

pca_ref is vectorised over the queries: elementwise numpy operations on float64 arrays are the IEEE operations the header
spells, one rounding each, so thousands of rows cost well under a second."""
import ctypes
import math

import numpy as np
import pytest
import torch

F32, F64, I32 = np.float32, np.float64, np.int32
FAMILIES = ("plane", "grid", "line", "duplicates", "ball", "x1e18", "x1e-30")
KS = (1, 2, 3, 8, 16, 64)
QNAN_BITS = 0x7FC00000
PAIRS = ((0, 1), (0, 2), (1, 2))
SWEEPS = 6


# ---- the references ------------------------------------------------------------------------------------------------------
def _key(i, j):
    return (i, j) if i <= j else (j, i)


def _rotate(A, V, p, q):
    """One Jacobi rotation (step 3 of the contract) on A {(i, j): (R,)} and V (R, 3, 3), in place, rows with A_pq == 0 skipped."""
    r = 3 - p - q
    app, aqq, apq = A[(p, p)], A[(q, q)], A[(p, q)]
    arp, arq = A[_key(r, p)], A[_key(r, q)]
    act = apq != 0.0
    theta = (aqq - app) / (2.0 * apq)
    t = np.copysign(1.0, theta) / (np.fabs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[(p, p)] = np.where(act, app - h, app)
    A[(q, q)] = np.where(act, aqq + h, aqq)
    A[(p, q)] = np.where(act, 0.0, apq)
    A[_key(r, p)] = np.where(act, c * arp - s * arq, arp)
    A[_key(r, q)] = np.where(act, s * arp + c * arq, arq)
    for i in range(3):
        vp, vq = V[:, i, p].copy(), V[:, i, q].copy()
        V[:, i, p] = np.where(act, c * vp - s * vq, vp)
        V[:, i, q] = np.where(act, s * vp + c * vq, vq)


def pca_core(P, live, viewpoint=None, sweeps=SWEEPS):
    """Steps 1-5 for R neighbourhoods: P (R, k, 3) float32 the slots' points, live (R, k) bool the slots that are used,
    viewpoint (R, 3) float32 or None -> dict of float64 arrays: mu (R, 3), C (R, 3, 3), bad (R,) the non-finite
    neighbourhoods, A (the dict after the sweeps), V (R, 3, 3), w (R, 3) ascending, vec (R, 3, 3) the vectors as rows."""
    P = np.asarray(P, F32)
    R, k = live.shape
    with np.errstate(all="ignore"):
        X = P.astype(F64)
        cnt = live.sum(1).astype(F64)
        s = np.zeros((R, 3), F64)
        for t in range(k):
            s = np.where(live[:, t, None], s + X[:, t], s)
        mu = s / cnt[:, None]
        acc = {key: np.zeros(R, F64) for key in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
        for t in range(k):
            d = X[:, t] - mu
            for (a, b) in acc:
                acc[(a, b)] = np.where(live[:, t], acc[(a, b)] + d[:, a] * d[:, b], acc[(a, b)])
        A = {key: v / cnt for key, v in acc.items()}
        C = np.empty((R, 3, 3), F64)
        for (a, b), v in A.items():
            C[:, a, b] = C[:, b, a] = v
        bad = ~np.isfinite(C).all((1, 2)) | (cnt == 0)
        V = np.zeros((R, 3, 3), F64)
        V[:, [0, 1, 2], [0, 1, 2]] = 1.0
        for _ in range(sweeps):
            for p, q in PAIRS:
                _rotate(A, V, p, q)
        diag = np.stack([A[(0, 0)], A[(1, 1)], A[(2, 2)]], 1)
        order = np.argsort(diag, axis=1, kind="stable")  # ascending by (value, w)
        w = np.take_along_axis(diag, order, 1)
        vec = np.take_along_axis(V.transpose(0, 2, 1), order[:, :, None], 1)  # row i: column order[i] of V
        lead = np.take_along_axis(vec, np.abs(vec).argmax(2)[:, :, None], 2)  # (argmax: the first of equal magnitudes)
        vec = np.where(lead < 0.0, -vec, vec)
        if viewpoint is not None:
            v = np.asarray(viewpoint, F32).astype(F64)
            n = vec[:, 0]
            side = ((v[:, 0] - mu[:, 0]) * n[:, 0] + (v[:, 1] - mu[:, 1]) * n[:, 1]) + (v[:, 2] - mu[:, 2]) * n[:, 2]
            vec[:, 0] = np.where((side < 0.0)[:, None], -n, n)
    return dict(mu=mu, C=C, bad=bad, A=A, V=V, w=w, vec=vec)


def _counts(lens, b, n):
    return np.full(b, n, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 1, n)


def pca_ref(xyz, idx, len1=None, len2=None, viewpoint=None):
    """rf_local_pca -> (normals (b, m, 3), eigenvalues (b, m, 3), axes (b, m, 3, 3)), float32."""
    xyz, idx = np.asarray(xyz, F32), np.asarray(idx, I32)
    b, n, _ = xyz.shape
    _, m, k = idx.shape
    L1, L2 = _counts(len1, b, n), _counts(len2, b, m)
    ix = idx.astype(np.int64)
    live = (np.arange(k)[None, None, :] < np.minimum(k, L1)[:, None, None]) & (ix >= 0) & (ix < L1[:, None, None])
    P = xyz[np.arange(b)[:, None, None], np.where(live, ix, 0)]
    vp = None if viewpoint is None else np.repeat(np.asarray(viewpoint, F32).reshape(b, 1, 3), m, 1).reshape(b * m, 3)
    r = pca_core(P.reshape(b * m, k, 3), live.reshape(b * m, k), vp)
    with np.errstate(all="ignore"):
        eig, axes = r["w"].astype(F32), r["vec"].astype(F32)
    eig[r["bad"]] = np.array([QNAN_BITS], np.uint32).view(F32)[0]
    axes[r["bad"]] = 0
    eig, axes = eig.reshape(b, m, 3), axes.reshape(b, m, 3, 3)
    pad = np.arange(m)[None, :] >= L2[:, None]
    eig[pad] = 0
    axes[pad] = 0
    return np.ascontiguousarray(axes[:, :, 0]), eig, axes


def nc_ref(nrm1, nrm2, idx1, idx2, len1=None, len2=None):
    """rf_nn_normal_consistency in float64 -> (ref (b, 4), mean |term| (b, 2), L (b, 2)): every product of widened values
    rounded once, the sums exact (math.fsum), one division."""
    nrm1, nrm2 = np.asarray(nrm1, F32).astype(F64), np.asarray(nrm2, F32).astype(F64)
    b, n, m = nrm1.shape[0], nrm1.shape[1], nrm2.shape[1]
    L1, L2 = _counts(len1, b, n), _counts(len2, b, m)
    ref, mean_abs, Ls = np.zeros((b, 4)), np.zeros((b, 2)), np.stack([L1, L2], 1)
    for i in range(b):
        for d, (own, oth, ix, L, Lo) in enumerate(((nrm1[i], nrm2[i], idx1[i], L1[i], L2[i]), (nrm2[i], nrm1[i], idx2[i], L2[i], L1[i]))):
            j = np.asarray(ix[:L], np.int64)
            ok = (j >= 0) & (j < Lo)
            a, c = own[:L], oth[np.where(ok, j, 0)]
            dot = (a[:, 0] * c[:, 0] + a[:, 1] * c[:, 1]) + a[:, 2] * c[:, 2]
            ok &= (a != 0).any(1) & (c != 0).any(1)
            dot = np.where(ok, dot, 0.0)
            ref[i, d] = math.fsum(np.abs(dot)) / float(L)
            ref[i, 2 + d] = math.fsum(dot) / float(L)
            mean_abs[i, d] = ref[i, d]
    return ref, mean_abs, Ls


def nc_bound(ref, mean_abs, Ls):
    """2^-23 |ref| + L 2^-52 mean|term| per entry of ref (b, 4): one fp32 rounding plus at most L double additions."""
    extra = Ls.astype(F64) * 2.0 ** -52 * mean_abs
    return 2.0 ** -23 * np.abs(ref) + np.concatenate([extra, extra], 1)


def family_cloud(name, n, seed):
    """The input families of the tests -> (n, 3) float32."""
    rng = np.random.RandomState(seed)
    f = lambda x: np.ascontiguousarray(x, F32)  # noqa: E731
    if name == "plane":  # a tilted plane
        q, _ = np.linalg.qr(rng.randn(3, 3))
        return f(rng.rand(n, 1) * q[0] + rng.rand(n, 1) * q[1] + rng.randn(3))
    if name == "grid":  # dyadic coordinates on the plane y = 0.25, some of them -0
        g = np.stack([rng.randint(0, 16, n) / 16.0, np.full(n, 0.25), rng.randint(-8, 8, n) / 8.0], 1)
        g[(g[:, 0] == 0) & (np.arange(n) % 2 == 1), 0] = -0.0
        return f(g)
    if name == "line":
        return f(rng.rand(n, 1) * rng.randn(3) + rng.randn(3))
    if name == "duplicates":  # 8 copies of every point
        return f(rng.rand((n + 7) // 8, 3)[np.arange(n) // 8])
    if name == "ball":
        return f(rng.randn(n, 3))
    if name == "x1e18":
        return f(rng.rand(n, 3) * 1e18)
    if name == "x1e-30":  # a thin sheet, tiny
        return f(rng.rand(n, 3) * [1.0, 1.0, 1e-3] * 1e-30)
    raise KeyError(name)


def brute_knn(xyz, k):
    """(n, 3) -> (n, k) int32: every point's k nearest by (distance in float64, index), itself included."""
    x = np.asarray(xyz, F32).astype(F64)
    with np.errstate(all="ignore"):
        d = ((x[:, None] - x[None]) ** 2).sum(-1)
    return np.argsort(d, 1, kind="stable")[:, :k].astype(I32)


# ---- the restatement is checked --------------------------------------------------------------------------------------------
N_HOST = 70


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("family", FAMILIES)
def test_the_sweeps_against_eigh(family, k):
    xyz = family_cloud(family, N_HOST, 7 + k)
    idx = brute_knn(xyz, k)
    r = pca_core(xyz[idx], np.ones(idx.shape, bool))
    assert not r["bad"].any()
    C, V, w = r["C"], r["V"], r["w"]
    for key in ((0, 1), (0, 2), (1, 2)):
        assert not r["A"][key].any(), f"off-diagonal {key} is not exactly 0 after the sixth sweep"
    scale = np.abs(C).max((1, 2))
    ref_w, ref_v = np.linalg.eigh(C)
    err_w = float((np.abs(w - ref_w).max(1) / np.where(scale > 0, scale, 1.0)).max())
    err_v = float(np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max())
    print(f"{family} k={k}: eigenvalues {err_w:.2e} of max|C|, |VtV - I| {err_v:.2e}")
    assert err_w <= 1e-13 and err_v <= 1e-14
    assert (np.diff(w, axis=1) >= 0).all()
    if family == "plane" and k >= 8:
        miss = float((1.0 - np.abs((r["vec"][:, 0] * ref_v[:, :, 0]).sum(1))).max())
        print(f"plane k={k}: 1 - |n . n_eigh| = {miss:.2e}")
        assert miss <= 1e-13


def test_fewer_sweeps_do_not_suffice():
    """Why six: after three sweeps off-diagonal mass is still there on some neighbourhood."""
    xyz = family_cloud("ball", N_HOST, 3)
    idx = brute_knn(xyz, 16)
    r3 = pca_core(xyz[idx], np.ones(idx.shape, bool), sweeps=3)
    assert any(r3["A"][key].any() for key in ((0, 1), (0, 2), (1, 2)))


def test_cases_by_hand():
    # an exact-grid plane: dyadic coordinates, y = 0.25
    pts = np.array([[0, 0.25, 0], [1, 0.25, 0], [0, 0.25, 1], [0.5, 0.25, 0.75], [-0.0, 0.25, -0.5], [0.25, 0.25, 2]], F32)
    idx = np.arange(6, dtype=I32)[None, None]
    nrm, eig, axes = pca_ref(pts[None], idx)
    assert nrm[0, 0].tolist() == [0, 1, 0] and eig[0, 0, 0].view(np.uint32) == 0  # exactly +0
    assert eig[0, 0, 1] > 0 and np.array_equal(axes[0, 0, 0], nrm[0, 0])
    assert all(float(a[np.abs(a).argmax()]) > 0 for a in axes[0, 0])  # the canonical sign
    nrm2, eig2, axes2 = pca_ref(pts[None], idx, viewpoint=np.array([[0.3, -1.0, 0.2]], F32))
    assert nrm2[0, 0].tolist() == [0, -1, 0] and np.array_equal(axes2[0, 0, 0], nrm2[0, 0])
    assert np.array_equal(eig2, eig) and np.array_equal(axes2[0, 0, 1:], axes[0, 0, 1:])  # the normal only
    nrm3, _, _ = pca_ref(pts[None], idx, viewpoint=np.array([[0.3, 7.0, 0.2]], F32))
    assert nrm3[0, 0].tolist() == [0, 1, 0]
    # one NaN: the NaN eigenvalues and the zero normal
    bad = pts.copy()
    bad[3, 2] = np.nan
    nrm, eig, axes = pca_ref(bad[None], idx)
    assert (eig.view(np.uint32) == QNAN_BITS).all() and not nrm.view(np.uint32).any() and not axes.view(np.uint32).any()
    # skipped slots: indices outside [0, len1) do not count; none left is a non-finite neighbourhood; rows behind len2 are zeros
    idx = np.array([[[0, 1, 2, 3, 4, 5], [0, -1, 1, 9, 2, 6], [7, -3, 6, 6, 6, 6], [0, 1, 2, 3, 4, 5]]], I32)
    nrm, eig, axes = pca_ref(pts[None], idx, len1=[6], len2=[3])
    want = pca_ref(pts[None], np.array([[[0, 1, 2]]], I32))
    assert np.array_equal(eig[0, 1], want[1][0, 0]) and np.array_equal(nrm[0, 1], want[0][0, 0])
    assert (eig[0, 2].view(np.uint32) == QNAN_BITS).all() and not nrm[0, 2].any()
    assert not eig[0, 3].view(np.uint32).any() and not axes[0, 3].view(np.uint32).any()
    # len1 < k: the first len1 slots are live
    nrm, eig, _ = pca_ref(pts[None], np.array([[[0, 1, 2, 3, 4, 5]]], I32), len1=[3])
    assert np.array_equal(eig[0, 0], want[1][0, 0])
    # one point: a zero covariance, the frame is the identity
    nrm, eig, axes = pca_ref(pts[None], np.array([[[4]]], I32))
    assert not eig.any() and np.array_equal(axes[0, 0], np.eye(3, dtype=F32))


def test_nc_ref_by_hand():
    n1 = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, -1]]], F32)
    n2 = np.array([[[-1, 0, 0], [0, 1, 0], [0.6, 0.8, 0]]], F32)
    idx1, idx2 = np.array([[0, 2, 1, 7]], I32), np.array([[0, 1, 2]], I32)
    ref, mean_abs, Ls = nc_ref(n1, n2, idx1, idx2)
    # 1 -> -1; (0,1,0).(0.6,0.8,0) = 0.8f; a zero normal; an index outside
    assert ref[0, 0] == (1.0 + float(F32(0.8))) / 4 and ref[0, 2] == (-1.0 + float(F32(0.8))) / 4
    assert ref[0, 1] == 2.0 / 3 and ref[0, 3] == 0.0  # -1, +1 and the zero normal n1[2]
    assert Ls.tolist() == [[4, 3]] and mean_abs[0, 0] == ref[0, 0]
    ref, _, Ls = nc_ref(n1, n2, idx1, idx2, len1=[2], len2=[1])
    assert Ls.tolist() == [[2, 1]] and ref[0, 0] == 0.5 and ref[0, 1] == 1.0  # slot 1 names row 2, behind len2: +0


def test_normals_csv_round_trip(tmp_path):
    from rfnet_amd import evalio
    rows = [("02691156/m00", float(F32(0.7)), 0.5, float(F32(0.9))), ("03001627/m01", 1.0, 1.0, 1.0)]
    path = str(tmp_path / "sub" / "normals.csv")
    evalio.write_normals_csv(path, rows)
    assert open(path).read().splitlines()[0] == "id,nc,nc12,nc21"
    assert evalio.read_normals_csv(path) == rows  # repr of a float: nothing is lost


# ---- the ABI -------------------------------------------------------------------------------------------------------------
ENTRIES = ("rf_local_pca", "rf_nn_normal_consistency")


def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib, _raw, glue
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ENTRIES:
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    header = open(_lib._PKG + "/../include/rfops.h").read()
    assert f"#define RF_PCA_MAX_K {_raw.PCA_MAX_K}\n" in header and _raw.PCA_MAX_K == 64
    for fn in ("local_pca", "nn_normal_consistency"):
        assert callable(getattr(_raw, fn))
    for fn in ("local_pca", "estimate_normals", "normal_consistency"):
        assert callable(getattr(glue, fn))


PTR = 0x10000  # never dereferenced: every call below must return at its argument checks


def _pca(b=2, n=100, m=50, k=16, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 9  # xyz, idx, len1, len2, viewpoint, normals, eigenvalues, axes, (stream)
    t[8] = None
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_local_pca(b, n, m, k, *t)


def _nc(b=2, n=100, m=50, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [PTR] * 8  # nrm1, nrm2, idx1, idx2, len1, len2, out, (stream)
    t[7] = None
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_nn_normal_consistency(b, n, m, *t)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL = 0, -1
    # an optional tensor left out passes the rules and the call goes on to the device: it is made only where there is none --
    # with a device it would launch a kernel on the made-up pointers
    launches = torch.cuda.is_available()
    assert _pca(b=0) == OK and _pca(b=0, n=0, m=0, k=0) == OK
    for bad in (dict(b=-1), dict(b=65536), dict(n=0), dict(n=-3), dict(n=65537), dict(m=0), dict(m=65537), dict(k=0), dict(k=-1),
                dict(k=65)):
        assert _pca(**bad) == EINVAL, bad
    for t in range(8):
        optional = t in (2, 3, 4, 7)  # len1, len2, viewpoint, axes
        assert (optional and launches) or (_pca(null=t) == EINVAL) == (not optional), f"rf_local_pca: NULL tensor {t}"
        assert _pca(at=(t, PTR + 2)) == EINVAL, f"rf_local_pca: tensor {t} not 4-byte aligned"
    assert _nc(b=0) == OK and _nc(b=0, n=0, m=0) == OK
    for bad in (dict(b=-1), dict(b=65536), dict(n=0), dict(n=-3), dict(m=0), dict(m=-1)):
        assert _nc(**bad) == EINVAL, bad
    for t in range(7):
        optional = t in (4, 5)
        assert (optional and launches) or (_nc(null=t) == EINVAL) == (not optional), f"rf_nn_normal_consistency: NULL tensor {t}"
        assert _nc(at=(t, PTR + 2)) == EINVAL, f"rf_nn_normal_consistency: tensor {t} not 4-byte aligned"
    if not torch.cuda.is_available():  # a call that passes the rules gets as far as the device check
        assert _pca() == -3 and _pca(null=7) == -3 and _nc() == -3


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    xyz, idx = np.zeros((2, 8, 3), F32), np.zeros((2, 5, 4), I32)
    with pytest.raises(ValueError, match="xyz"):
        _raw.local_pca(np.zeros((2, 8, 2), F32), idx)
    with pytest.raises(ValueError, match="idx"):
        _raw.local_pca(xyz, np.zeros((3, 5, 4), I32))
    with pytest.raises(ValueError, match="k <= 64"):
        _raw.local_pca(xyz, np.zeros((2, 5, 65), I32))
    with pytest.raises(ValueError, match="viewpoint"):
        _raw.local_pca(xyz, idx, viewpoint=np.zeros((3, 3), F32))
    with pytest.raises(ValueError, match="lengths1"):
        _raw.local_pca(xyz, idx, lengths1=[8, 9])
    with pytest.raises(ValueError, match="viewpoint"):
        glue.local_pca(torch.zeros(2, 8, 3), torch.zeros(2, 5, 4, dtype=torch.int32), viewpoint=[0.0, 1.0])
    nrm = np.zeros((2, 8, 3), F32)
    with pytest.raises(ValueError, match="normals"):
        _raw.nn_normal_consistency(nrm, np.zeros((3, 8, 3), F32), np.zeros((2, 8), I32), np.zeros((2, 8), I32))
    with pytest.raises(ValueError, match="idx1"):
        _raw.nn_normal_consistency(nrm, nrm, np.zeros((2, 7), I32), np.zeros((2, 8), I32))
    with pytest.raises(ValueError, match="lengths2"):
        _raw.nn_normal_consistency(nrm, nrm, np.zeros((2, 8), I32), np.zeros((2, 8), I32), lengths2=[0, 8])
