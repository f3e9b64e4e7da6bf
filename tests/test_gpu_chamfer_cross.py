"""GPU: rf_chamfer_cross (rfnet_amd/csrc/chamfer_cross.hip), the Chamfer matrix of two collections of clouds, against
the float64 restatement of its six columns (tests/test_chamfer_cross_host.py: cross_ref) applied to the oracle's
nn_distance outputs on the unpadded slices of every pair.

Bars (the issue's, include/rfops.h's): columns 4, 5 bit-exact; columns 0-3 rel 1e-5; a direction whose cloud has a single
valid point returns sqrtf(d), d, d exactly.

Shapes: each is the smallest that reaches its path -- collection sizes that are no multiple of anything and padding
lanes in the last superblock ("sizes"), clouds of 1 / 63 / 64 / 65 points ("tiny"), 66 candidate superblocks in two
distant clusters with an outlier ("cull": a second round of 64 boxes, boxes really skipped, a max whose nearest box is
not the seed), duplicates and exact copies ("dups"), ragged counts over hostile padding ("ragged") and the large-cloud
sort with a 65536-term sum ("large")."""
import numpy as np
import pytest
import torch

from conftest import assert_rel
from test_chamfer_cross_host import NCOL, cross_ref

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32


def _unit(rng, *shape):
    return (rng.random_sample(shape) - 0.5).astype(F32)


def _inputs(name):
    """-> (xyz1 (s, n, 3), xyz2 (r, m, 3), len1 | None, len2 | None)"""
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "sizes":
        return _unit(rng, 3, 130, 3), _unit(rng, 5, 257, 3), None, None
    if name.startswith("tiny"):
        n, m = (int(v) for v in name.split("_")[1:])
        return _unit(rng, 2, n, 3), _unit(rng, 2, m, 3), None, None
    if name == "cull":
        a, c = _unit(rng, 2, 130, 3), _unit(rng, 3, 4161, 3)
        a[:, 65:] += F32(40.0)   # two distant clusters in every cloud
        c[:, 2000:] += F32(40.0)
        a[:, 7] = (F32(-9.0), F32(13.0), F32(21.0))   # one outlier per cloud, far from every box of its partners
        c[:, 3000] = (F32(17.0), F32(-25.0), F32(8.0))
        return a, c, None, None
    if name == "dups":
        a, c = _unit(rng, 2, 200, 3), _unit(rng, 3, 150, 3)
        a[:, 100:140] = a[:, 0:40]          # duplicated points inside a cloud
        c[0] = a[0, :150]                   # an exact copy of most of a cloud
        c[1, :70] = a[1, rng.randint(0, 200, 70)]  # copies of some of its points
        c[2, 100:] = c[2, :50]
        return a, c, None, None
    if name == "ragged":
        a, c = _unit(rng, 4, 130, 3), _unit(rng, 4, 200, 3)
        l1, l2 = np.array([130, 1, 64, 65], I32), np.array([1, 200, 65, 64], I32)
        a[1, 1:], a[2, 64:] = np.nan, np.inf
        a[3, 65:] = a[3, np.arange(130 - 65) % 65]  # copies of valid points: read, they would be counted in the means
        c[0, 1:] = a[0, np.arange(199) % 130]       # copies of the OTHER side's points: read, they would win with 0
        c[2, 65:], c[3, 64:] = np.nan, -np.inf
        return a, c, l1, l2
    assert name == "large"
    return _unit(rng, 1, 65536, 3), _unit(rng, 2, 512, 3), None, None


_CASES = {}


def case(name, orc):
    """Inputs and reference of a shape, computed once and shared (never modified)."""
    if name in _CASES:
        return _CASES[name]
    a, c, l1, l2 = _inputs(name)
    s, n, r, m = a.shape[0], a.shape[1], c.shape[0], c.shape[1]
    L1 = np.full(s, n, I32) if l1 is None else l1
    L2 = np.full(r, m, I32) if l2 is None else l2
    exp = np.zeros((s, r, NCOL))
    one = np.zeros((s, r, 2, 3), F32)  # per direction: sqrtf(d), d, d of a single-point cloud
    for i in range(s):
        for j in range(r):
            e = orc.nn_distance(a[i:i + 1, :L1[i]].copy(), c[j:j + 1, :L2[j]].copy())
            exp[i, j] = cross_ref(e[0][0], e[2][0])
            for d, dist in enumerate((e[0][0], e[2][0])):
                one[i, j, d] = (np.sqrt(F32(dist[0])), dist[0], dist[0])
    _CASES[name] = dict(a=a, c=c, l1=l1, l2=l2, L1=L1, L2=L2, exp=exp, one=one, s=s, r=r, n=n, m=m)
    return _CASES[name]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(r, device_counts=False):
    from rfnet_amd import _raw
    l1 = None if r["l1"] is None else (_dev(r["l1"]) if device_counts else r["l1"].tolist())
    l2 = None if r["l2"] is None else (_dev(r["l2"]) if device_counts else r["l2"].tolist())
    out = _raw.chamfer_cross(_dev(r["a"]), _dev(r["c"]), lengths1=l1, lengths2=l2)
    torch.cuda.synchronize()
    assert out.shape == (r["s"], r["r"], NCOL) and out.dtype == torch.float32 and not out.requires_grad
    return out.cpu().numpy()


def check(got, r, what):
    exp = r["exp"]
    print(f"{what}: max rel err by column",
          " ".join("%.2e" % (np.abs(got[..., k] - exp[..., k]) / np.maximum(np.abs(exp[..., k]), 1e-300)).max() for k in range(NCOL)))
    assert np.array_equal(got[..., 4:6], exp[..., 4:6].astype(F32)), f"{what}: columns 4, 5 are not bit-exact"
    assert_rel(got[..., 0:4], exp[..., 0:4], 1e-5, what=f"{what}: columns 0-3")
    assert not np.signbit(got).any(), f"{what}: a negative zero"
    for i in range(r["s"]):
        for j in range(r["r"]):
            for d, L in enumerate((r["L1"][i], r["L2"][j])):
                if L == 1:
                    assert got[i, j, d::2].tobytes() == r["one"][i, j, d].tobytes(), f"{what}: single point, pair {i, j} direction {d + 1}"


TINY = ["tiny_%d_%d" % (n, m) for n in (1, 63, 64, 65) for m in (1, 63, 64, 65)]


@pytest.mark.parametrize("name", ["sizes", "cull", "dups", "ragged", "large"] + TINY)
def test_matrix_against_the_oracle(orc, name):
    r = case(name, orc)
    if name == "cull":
        assert -(-r["m"] // 64) == 66  # 66 candidate superblocks: two rounds of 64 boxes
    got = run(r)
    check(got, r, name)
    again = run(r, device_counts=True)  # counts as a device tensor; and a second call: identical bits
    assert got.tobytes() == again.tobytes(), f"{name}: two calls differ"


def test_ragged_equals_the_call_on_the_sliced_clouds(orc):
    """Rows behind a count never reach a result: every pair of the ragged call is, bit for bit, the call on the two
    clouds cut to their counts."""
    from rfnet_amd import _raw
    r = case("ragged", orc)
    got = run(r, device_counts=True)
    for i in range(r["s"]):
        for j in range(r["r"]):
            cut = _raw.chamfer_cross(_dev(r["a"][i:i + 1, :r["L1"][i]]), _dev(r["c"][j:j + 1, :r["L2"][j]]))
            assert cut.cpu().numpy()[0, 0].tobytes() == got[i, j].tobytes(), (i, j)


def test_batch_invariance():
    from rfnet_amd import _raw
    rng = np.random.RandomState(77)
    a, c = _dev(_unit(rng, 4, 300, 3)), _dev(_unit(rng, 5, 700, 3))
    full = _raw.chamfer_cross(a, c)
    part = _raw.chamfer_cross(a[1:3], c[2:4])
    assert torch.equal(full[1:3, 2:4], part) and full[1:3, 2:4].cpu().numpy().tobytes() == part.cpu().numpy().tobytes()
    assert _raw.chamfer_cross(a, c).cpu().numpy().tobytes() == full.cpu().numpy().tobytes()


@pytest.mark.parametrize("ragged", [False, True])
def test_self_call(ragged):
    from rfnet_amd import _raw
    rng = np.random.RandomState(78)
    a = _unit(rng, 5, 333, 3)
    a[2, 40:80] = a[2, 0:40]  # duplicates: equal sort keys, whose order the sort leaves open
    lens = [333, 1, 200, 65, 64] if ragged else None
    A = _dev(a)
    me = _raw.chamfer_cross(A, lengths1=lens).cpu().numpy()
    two = _raw.chamfer_cross(A, A.clone(), lengths1=lens, lengths2=lens).cpu().numpy()
    assert me.tobytes() == two.tobytes(), "the self call is not the general call bit for bit"
    diag = me[np.arange(5), np.arange(5)]
    assert not diag.any() and not np.signbit(diag).any(), "the diagonal is not +0"
    assert np.array_equal(me[..., 4], me[..., 5].T) and np.array_equal(me[..., 0], me[..., 1].T) \
        and np.array_equal(me[..., 2], me[..., 3].T)


def test_chamfer_matrix_against_chamfer_metrics():
    from rfnet_amd import glue
    rng = np.random.RandomState(79)
    a, c = _dev(_unit(rng, 3, 301, 3)), _dev(_unit(rng, 3, 257, 3))
    got = glue.chamfer_matrix(a, c)
    assert set(got) == {"cd_l1", "cd_l2", "hausdorff", "raw"} and got["raw"].shape == (3, 3, NCOL)
    pairs = glue.chamfer_metrics(a[:, None].expand(3, 3, 301, 3).reshape(9, 301, 3),
                                 c[None].expand(3, 3, 257, 3).reshape(9, 257, 3))
    for k in ("cd_l1", "cd_l2"):
        assert got[k].shape == (3, 3)
        assert_rel(got[k].cpu().numpy().reshape(9), pairs[k].cpu().numpy(), 1e-5, what=k)
    assert torch.equal(got["hausdorff"].reshape(9), pairs["hausdorff"]), "hausdorff is not exact"
    assert torch.equal(got["raw"][..., 4:6].reshape(9, 2), pairs["raw"][:, 4:6])


def test_minimal_matching():
    from rfnet_amd import glue
    rng = np.random.RandomState(80)
    pred, refs = _unit(rng, 4, 150, 3), _unit(rng, 5, 130, 3)
    refs[1] = refs[3] = pred[2, :130]  # a planted exact tie: references 1 and 3 are one cloud, and prediction 2 is nearest to it
    P, R = _dev(pred), _dev(refs)
    for metric in ("cd_l2", "cd_l1", "hausdorff"):
        mat = glue.chamfer_matrix(P, R)[metric].cpu().numpy()
        val, at = glue.minimal_matching(P, R, metric=metric)
        assert at.dtype == torch.int64 and val.shape == (4,) and at.shape == (4,)
        exp_at = np.array([int(np.flatnonzero(row == row.min())[0]) for row in mat])
        assert np.array_equal(at.cpu().numpy(), exp_at) and exp_at[2] == 1, (metric, at, exp_at)
        assert val.cpu().numpy().tobytes() == mat[np.arange(4), exp_at].tobytes()
        for chunk in (1, 2, 3):
            v2, a2 = glue.minimal_matching(P, R, metric=metric, chunk=chunk)
            assert v2.cpu().numpy().tobytes() == val.cpu().numpy().tobytes() and torch.equal(a2, at), (metric, chunk)
    # ragged references, chunked: the counts follow their clouds
    l2 = [130, 100, 1, 100, 64]
    val, at = glue.minimal_matching(P, R, lengths2=l2)
    v2, a2 = glue.minimal_matching(P, R, lengths2=torch.tensor(l2, dtype=torch.int32).cuda(), chunk=2)
    assert v2.cpu().numpy().tobytes() == val.cpu().numpy().tobytes() and torch.equal(a2, at)


def test_graph_capture_with_device_counts(orc):
    """No host synchronisation anywhere: the call is captured with device counts and, replayed once, returns what the
    eager call returns."""
    from rfnet_amd import _host, _raw
    if not _host.graph_replay_ok():
        pytest.skip("this process started the HIP runtime without DEBUG_CLR_GRAPH_PACKET_CAPTURE=0: captured graphs "
                    "do not replay correctly")
    r = case("ragged", orc)
    a, c, l1, l2 = _dev(r["a"]), _dev(r["c"]), _dev(r["l1"]), _dev(r["l2"])
    eager = _raw.chamfer_cross(a, c, lengths1=l1, lengths2=l2).cpu().numpy()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        _raw.chamfer_cross(a, c, lengths1=l1, lengths2=l2)
    cur.wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _raw.chamfer_cross(a, c, lengths1=l1, lengths2=l2)
    graph.replay()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    check(got, r, "replay")
    assert got.tobytes() == eager.tobytes()
