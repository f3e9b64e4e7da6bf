"""CPU: the Chamfer matrix entry (include/rfops.h, "the Chamfer matrix of two collections of clouds") at the boundary --
declared, exported, bound; the workspace size; every argument rule answered before a device is touched -- the float64
restatement of its six columns that the GPU tests hold the kernels to (cross_ref), and glue.set_metrics against a
brute-force float64 restatement and cases with known answers."""
import ctypes

import numpy as np
import pytest
import torch

NCOL = 6


# ---- the reference: the six columns of one pair in float64, from the fp32 distances of its valid slices --------------
def cross_ref(d1, d2):
    """d1 (L1,), d2 (L2,): nn_distance's fp32 outputs for one pair, both directions -> (6,) float64."""
    out = np.zeros(NCOL)
    for d, dist in enumerate((np.asarray(d1, np.float32), np.asarray(d2, np.float32))):
        x = dist.astype(np.float64)
        out[0 + d] = np.sqrt(x).mean()
        out[2 + d] = x.mean()
        out[4 + d] = x.max()
    return out


def test_cross_ref_by_hand():
    got = cross_ref([0.25, 0.0, 1.0], [4.0])
    assert got.tolist() == [0.5, 2.0, 1.25 / 3, 4.0, 1.0, 4.0]


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    from test_boundary import _header_symbols
    from rfnet_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    for name in ("rf_chamfer_cross", "rf_chamfer_cross_workspace_bytes"):
        assert name in syms, f"include/rfops.h does not declare {name}"
        assert hasattr(raw, name), f"librfops.so lacks {name}"
        assert name in _lib.SIGNATURES, f"ctypes binding lacks {name}"
    assert "#define RF_CX_NCOL 6" in open(_lib._PKG + "/../include/rfops.h").read()


def test_workspace_size():
    from rfnet_amd._lib import lib
    fn = lib.rf_chamfer_cross_workspace_bytes
    for shape in ((0, 3, 10, 10), (3, 0, 10, 10), (2, 2, 0, 10), (2, 2, 10, 0), (-1, 2, 10, 10), (2, -2, 10, 10),
                  (2, 2, -5, 10), (2, 2, 10, -5)):
        assert fn(*shape) == 0, shape
    for s, r, n, m in ((1, 1, 1, 1), (3, 5, 130, 257), (1, 2, 65536, 512), (32, 32, 2048, 2048), (8, 64, 16384, 16384)):
        assert fn(s, r, n, m) > 0, (s, r, n, m)
        assert fn(s, r, n, m) >= lib.rf_nn_sort_bytes(s, n) + lib.rf_nn_sort_bytes(r, m), (s, r, n, m)
    # nothing of the size of the expanded pairs: 64 * 64 * 2048 floats are 32 MiB
    assert fn(64, 64, 2048, 2048) < 64 * 64 * 2048 * 4
    # per pair it grows with a record per 64 points and direction, not with the points
    grow = fn(64, 64, 2048, 2048) - fn(64, 32, 2048, 2048)
    assert grow < 64 * 32 * 2048 * 4 // 2


P, WS, BIG = 0x10000, 0x200000, 1 << 40  # never dereferenced: every call below must return at its argument checks


def _call(s=2, r=3, n=300, m=200, ws=WS, wsz=BIG, l1=P, l2=P, null=None, at=None):
    from rfnet_amd._lib import lib
    t = [P] * 3  # xyz1, xyz2, out
    if null is not None:
        t[null] = None
    if at is not None:
        t[at[0]] = at[1]
    return lib.rf_chamfer_cross(s, r, n, m, t[0], t[1], l1, l2, t[2], ws, wsz, None)


def test_argument_rules_are_answered_without_a_device():
    OK, EINVAL, EWORKSPACE = 0, -1, -2
    from rfnet_amd._lib import lib
    assert _call(s=0) == OK and _call(r=0) == OK
    assert _call(s=0, r=0, n=0, m=0, ws=None, wsz=0) == OK
    for bad in (dict(s=-1), dict(r=-1), dict(n=-3), dict(m=-3), dict(s=0, n=-1), dict(r=0, s=-2), dict(n=0), dict(m=0),
                dict(n=65537), dict(m=65537), dict(s=65536), dict(r=65536)):
        assert _call(**bad) == EINVAL, bad
    for k in range(3):
        assert _call(null=k) == EINVAL, f"NULL tensor {k}"
        assert _call(at=(k, P + 2)) == EINVAL, f"tensor {k} not 4-byte aligned"
    assert _call(l1=P + 2) == EINVAL and _call(l2=P + 1) == EINVAL  # count arrays: 4 bytes
    assert _call(ws=None) == EINVAL
    assert _call(ws=WS + 4) == EINVAL and _call(ws=WS + 8) == EINVAL  # workspace: 16 bytes
    need = lib.rf_chamfer_cross_workspace_bytes(2, 3, 300, 200)
    assert _call(wsz=need - 1) == EWORKSPACE and _call(wsz=0) == EWORKSPACE
    # NULL counts mean "all", and the largest sizes are sizes: neither is the error here
    assert _call(wsz=0, l1=None, l2=None) == EWORKSPACE
    assert _call(s=65535, r=65535, n=65536, m=65536, wsz=0) == EWORKSPACE


def test_wrappers_check_before_any_launch():
    from rfnet_amd import _raw, glue
    a, c = np.zeros((2, 4, 3), np.float32), np.zeros((3, 5, 3), np.float32)
    with pytest.raises(ValueError, match="xyz1"):
        _raw.chamfer_cross(np.zeros((2, 4), np.float32), c)
    with pytest.raises(ValueError, match="xyz2"):
        _raw.chamfer_cross(a, np.zeros((3, 5, 2), np.float32))
    with pytest.raises(ValueError, match="lengths1"):
        _raw.chamfer_cross(a, c, lengths1=[4, 5])
    with pytest.raises(ValueError, match="lengths2"):
        _raw.chamfer_cross(a, c, lengths2=[5, 5])  # (r,) counts, not (s,)
    with pytest.raises(ValueError, match="lengths1 only"):
        _raw.chamfer_cross(a, None, lengths2=[4, 4])
    with pytest.raises(ValueError, match="metric"):
        glue.minimal_matching(torch.zeros(2, 4, 3), torch.zeros(3, 5, 3), metric="emd")
    with pytest.raises(ValueError, match="chunk"):
        glue.minimal_matching(torch.zeros(2, 4, 3), torch.zeros(3, 5, 3), chunk=0)


def test_mmd_csv_round_trip(tmp_path):
    from rfnet_amd import evalio
    rows = [("02691156/a", float(np.float32(0.1)), 3), ("03001627/b", 1.5e-7, 0)]
    path = str(tmp_path / "out" / "mmd.csv")
    evalio.write_mmd_csv(path, rows)
    assert open(path).readline().strip() == "id,mmd,ref_index"
    assert evalio.read_mmd_csv(path) == rows


# ---- glue.set_metrics --------------------------------------------------------------------------------------------------
def set_metrics_ref(d_gr, d_gg=None, d_rr=None):
    """The definitions, one loop per sentence, in float64; every argmin the first of the smallest."""
    d_gr = np.asarray(d_gr, np.float64)
    g, r = d_gr.shape
    out = {"mmd": float(np.mean([min(d_gr[i, j] for i in range(g)) for j in range(r)]))}
    chosen = set()
    for i in range(g):
        best = 0
        for j in range(1, r):
            if d_gr[i, j] < d_gr[i, best]:
                best = j
        chosen.add(best)
    out["cov"] = len(chosen) / r
    if d_gg is not None:
        full = np.block([[np.asarray(d_gg, np.float64), d_gr], [d_gr.T, np.asarray(d_rr, np.float64)]])
        right = 0
        for a in range(g + r):
            best = None
            for b in range(g + r):
                if b != a and (best is None or full[a, b] < full[a, best]):
                    best = b
            right += (best < g) == (a < g)
        out["one_nna"] = right / (g + r)
    return out


def _sym(rng, k, levels):
    x = rng.randint(1, levels, (k, k)).astype(np.float32)
    return np.triu(x, 1) + np.triu(x, 1).T


@pytest.mark.parametrize("g, r, levels", [(7, 5, 4), (4, 9, 3), (6, 6, 1000), (1, 3, 5), (3, 1, 5)])
def test_set_metrics_against_the_restatement(g, r, levels):
    """Few levels: many ties.  g != r.  Column 0 is made the largest of every row: no row chooses it, cov < 1."""
    from rfnet_amd import glue
    rng = np.random.RandomState(g * 100 + r)
    d_gr = rng.randint(1, levels + 1, (g, r)).astype(np.float32) / 8
    if r > 1:
        d_gr[:, 0] = (levels + 1) / 8
    d_gg, d_rr = _sym(rng, g, levels + 1) / 8, _sym(rng, r, levels + 1) / 8
    exp = set_metrics_ref(d_gr, d_gg, d_rr)
    got = glue.set_metrics(torch.from_numpy(d_gr), torch.from_numpy(d_gg), torch.from_numpy(d_rr))
    assert set(got) == {"mmd", "cov", "one_nna"} and all(v.dim() == 0 for v in got.values())
    for k in exp:
        assert float(got[k]) == pytest.approx(exp[k], rel=1e-6), k
    if r > 1:
        assert float(got["cov"]) < 1
    only = glue.set_metrics(torch.from_numpy(d_gr))
    assert set(only) == {"mmd", "cov"} and float(only["cov"]) == pytest.approx(exp["cov"], rel=1e-6)
    with pytest.raises(ValueError):
        glue.set_metrics(torch.from_numpy(d_gr), torch.from_numpy(d_gg))


def test_set_metrics_known_answers():
    from rfnet_amd import glue
    # two well-separated clusters: everyone's nearest other item is of its own kind
    near, far = 0.01, 5.0
    d_gg = torch.full((3, 3), near)
    d_rr = torch.full((4, 4), near)
    d_gr = torch.full((3, 4), far)
    assert float(glue.set_metrics(d_gr, d_gg, d_rr)["one_nna"]) == 1.0
    # identical sets: distances of a set to itself with a zero diagonal and distinct off-diagonal entries
    pts = torch.tensor([0.0, 1.0, 3.0, 7.0])
    d = (pts[:, None] - pts[None, :]).abs()
    got = glue.set_metrics(d, d, d)
    assert float(got["mmd"]) == 0.0 and float(got["cov"]) == 1.0
    # ties go to the lowest index: both rows choose column 0 of an all-equal matrix
    assert float(glue.set_metrics(torch.ones(2, 4))["cov"]) == 0.25
