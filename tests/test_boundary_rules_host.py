"""CPU: the pointer rules of the C-ABI entries whose own host tests do not pin them pointer by pointer (include/rfops.h: tensors
non-NULL and, in the newer entries, 4-byte aligned; workspaces and sorted-set handles non-NULL and 16-byte aligned; the size check
after them): the entries without a host test of their rules, and the _lengths entries, whose tests misalign the counts only.
Each entry checks exactly what it is pinned to check here -- the older ones test for NULL only.

EVERY call below is one the library rejects at its argument checks, with RF_EINVAL or RF_EWORKSPACE: the addresses are
made up and never dereferenced, and this file also runs where a device is present."""
import pytest

P, WS, BIG = 0x10000, 0x200000, 1 << 40
EINVAL, EWORKSPACE = -1, -2


class Entry:
    """One entry: its arguments in order, pointers by NAME (every other value is passed as it is).  A call takes every pointer
    as P, the workspace `ws` as WS and its size `wsz` as 0, unless overridden."""

    def __init__(self, fn, args, null=(), odd=(), at16=(), ws16=True, need=None, small=EWORKSPACE):
        self.fn, self.args, self.null, self.odd, self.at16, self.ws16, self.need, self.small = fn, args, null, odd, at16, ws16, need, small

    def call(self, lib, **over):
        vals = []
        for a in self.args:
            if isinstance(a, str):
                a = over[a] if a in over else {"ws": WS, "wsz": 0}.get(a, P)
            vals.append(a)
        return getattr(lib, self.fn)(*vals)


# (b, n, m) = (32, 2048, 16384) is a shape of the culled sweep, whose workspace is never empty
B, N, M = 32, 2048, 16384
ENTRIES = [
    Entry("rf_maxpool_points", [2, 100, 8, "x", "out", "ws", "wsz", None], null=["x", "out", "ws"], odd=["out"], at16=["x"],
          need=("rf_maxpool_points_workspace_bytes", 2, 100, 8)),
    Entry("rf_maxpool_points_idx", [2, 100, 8, "x", "out", "idx", "ws", "wsz", None], null=["x", "out", "idx", "ws"],
          odd=["out", "idx"], at16=["x"], need=("rf_maxpool_points_idx_workspace_bytes", 2, 100, 8)),
    Entry("rf_act_grad_colsum", [2, 100, 8, "grad", "out", 1, "g", "sums", "ws", "wsz", None], null=["grad", "out", "sums", "ws"],
          odd=["sums"], at16=["grad", "out", "g"], need=("rf_act_grad_colsum_workspace_bytes", 2, 100, 8)),
    Entry("rf_point_affine", [2, 100, 128, "y", "p", 3, "w", "r", 0, 1, "out", None], null=["p", "w", "r", "out"], odd=["p"],
          at16=["y", "w", "r", "out"], ws16=False, small=None),
    Entry("rf_sample_and_group", [2, 128, 16, 0.1, None, 8, "xyz", "fps_idx", "new_xyz", "idx", "pts_cnt", "grouped", "ws", "wsz",
                                  None, None],
          null=["xyz", "fps_idx", "new_xyz", "idx", "pts_cnt", "grouped", "ws"], need=("rf_sample_and_group_workspace_bytes", 2, 128)),
    Entry("rf_threenn_boxes", [2, 500, 300, "xyz1", "xyz2", None, None, "dist", "idx", "ws", "wsz", None],
          null=["xyz1", "xyz2", "dist", "idx", "ws"], need=("rf_threenn_boxes_workspace_bytes", 2, 500, 300)),
    Entry("rf_threenn_boxes", [2, 500, 300, "xyz1", "xyz2", "sorted1", "sorted2", "dist", "idx", "ws", "wsz", None],
          at16=["sorted1", "sorted2"]),
    Entry("rf_queryballpoint_boxes", [2, 128, 16, 0.1, None, 8, "xyz1", "xyz2", None, "idx", "pts_cnt", "ws", "wsz", None],
          null=["xyz1", "xyz2", "idx", "pts_cnt", "ws"], need=("rf_queryballpoint_boxes_workspace_bytes", 2, 128)),
    Entry("rf_queryballpoint_boxes", [2, 128, 16, 0.1, None, 8, "xyz1", "xyz2", "sorted1", "idx", "pts_cnt", "ws", "wsz", None],
          at16=["sorted1"]),
    Entry("rf_nn_sort", [2, 500, "xyz", "ws", "wsz", None], null=["xyz", "ws"], need=("rf_nn_sort_bytes", 2, 500)),
    Entry("rf_nn_distance_sorted", [2, 500, 300, "sorted1", "sorted2", "d1", "i1", "d2", "i2", None], null=["sorted1", "sorted2"],
          at16=["sorted1", "sorted2"], ws16=False, small=None),
    Entry("rf_nn_distance_mode", [B, N, M, "xyz1", "xyz2", "d1", "i1", "d2", "i2", "ws", "wsz", None, 0, None],
          null=["xyz1", "xyz2", "d1", "i1", "d2", "i2", "ws"], need=("rf_nn_distance_workspace_bytes", B, N, M)),
    Entry("rf_chamfer_step", [B, N, M, "xyz1", "xyz2", "gd1", "gd2", "d1", "i1", "d2", "i2", "gx1", "gx2", "ws", "wsz", None],
          null=["xyz1", "xyz2", "gd1", "gd2", "d1", "i1", "d2", "i2", "gx1", "gx2", "ws"],
          need=("rf_nn_distance_workspace_bytes", B, N, M)),
    Entry("rf_merge_layer", [2, 300, 200, "raw", "new", None, "dec", "refined", "idx2", "ws", "wsz", None],
          null=["raw", "new", "dec", "refined", "idx2", "ws"], ws16=False),
    Entry("rf_merge_layer_grad", [2, 300, 200, "raw", "new", "dec", "idx2", "grad_refined", "grad_new", "grad_dec", "grad_raw", None],
          null=["grad_dec"], ws16=False, small=None),
    Entry("rf_approxmatch", [2, 300, 200, "xyz1", "xyz2", "match", "ws", "wsz", None], null=["xyz1", "xyz2", "match", "ws"],
          need=("rf_approxmatch_workspace_bytes", 2, 300, 200, 0)),
    Entry("rf_matchcost", [2, 300, 200, "xyz1", "xyz2", "match", "cost", "ws", "wsz", None],
          null=["xyz1", "xyz2", "match", "cost", "ws"], ws16=False, need=("rf_matchcost_workspace_bytes", 2, 300, 200)),
    Entry("rf_earth_mover", [2, 300, 200, "xyz1", "xyz2", "cost", None, None, "ws", "wsz", None], null=["xyz1", "xyz2", "cost", "ws"],
          need=("rf_earth_mover_workspace_bytes", 2, 300, 200)),
    Entry("rf_auctionmatch", [2, 256, "xyz1", "xyz2", "matchl", "matchr", None, 0, None], null=["xyz1", "xyz2", "matchl", "matchr"],
          ws16=False, small=None),
    Entry("rf_selectionsort", [2, 8, 4, 2, "dist", "outi", "out", None], null=["dist", "outi", "out"], ws16=False, small=None),
    Entry("rf_gatherpoint", [2, 100, 10, "inp", "idx", "out", None], null=["inp", "idx", "out"], ws16=False, small=None),
    Entry("rf_probsample", [2, 100, 10, "inp_p", "inp_r", "temp", "out", None], null=["inp_p", "inp_r", "temp", "out"], ws16=False,
          small=None),
    Entry("rf_grouppoint", [2, 100, 8, 10, 4, "points", "idx", "out", None], null=["points", "idx", "out"], ws16=False, small=None),
    Entry("rf_threeinterpolate", [2, 50, 8, 100, "points", "idx", "weight", "out", None], null=["points", "idx", "weight", "out"],
          ws16=False, small=None),
    Entry("rf_knn", [2, 100, 50, 4, "xyz1", "xyz2", "val", "idx", None], null=["xyz1", "xyz2", "val", "idx"], ws16=False, small=None),
    # The _lengths entries: their own host tests pin sizes, NULL, the counts and the workspace; here EVERY pointer that the
    # entry holds to the 4-byte rule is misaligned in turn, the optional ones too.  (small=None where a workspace of 0 bytes
    # is a valid call: the scanning form needs none.)
    Entry("rf_nn_distance_lengths", [B, N, M, "xyz1", "xyz2", "len1", "len2", "d1", "i1", "d2", "i2", "ws", "wsz", None, 0],
          null=["xyz1", "xyz2", "d1", "i1", "d2", "i2", "ws"], odd=["xyz1", "xyz2", "len1", "len2", "d1", "i1", "d2", "i2"],
          need=("rf_nn_distance_lengths_workspace_bytes", B, N, M, 0)),
    Entry("rf_sample_and_group_lengths", [2, 128, 16, 0.1, "radius_dev", 8, "xyz", "len", "len_out", "fps_idx", "new_xyz", "idx",
                                          "pts_cnt", "grouped", "ws", "wsz", None, None],
          null=["xyz", "fps_idx", "new_xyz", "idx", "pts_cnt", "grouped", "ws"],
          odd=["radius_dev", "xyz", "len", "len_out", "fps_idx", "new_xyz", "idx", "pts_cnt", "grouped"],
          need=("rf_sample_and_group_lengths_workspace_bytes", 2, 128)),
    Entry("rf_threenn_lengths", [2, 500, 300, "xyz1", "xyz2", "len1", "len2", "dist", "idx", "ws", "wsz", None, 0],
          null=["xyz1", "xyz2", "dist", "idx"], odd=["xyz1", "xyz2", "len1", "len2", "dist", "idx"], small=None),
    Entry("rf_knn_lengths", [2, 100, 50, 4, "xyz1", "xyz2", "len1", "len2", "val", "idx", "ws", "wsz", None, 0],
          null=["xyz1", "xyz2", "val", "idx"], odd=["xyz1", "xyz2", "len1", "len2", "val", "idx"], small=None),
    Entry("rf_queryballpoint_lengths", [2, 128, 16, 0.1, "radius_dev", 8, "xyz1", "xyz2", "len1", "len2", "idx", "pts_cnt", "ws",
                                        "wsz", None, 0],
          null=["xyz1", "xyz2", "idx", "pts_cnt"], odd=["radius_dev", "xyz1", "xyz2", "len1", "len2", "idx", "pts_cnt"], small=None),
    Entry("rf_farthestpointsampling_lengths", [2, 20000, 64, "inp", "len", "len_out", "ws", "wsz", "out", "new_xyz", None],
          null=["inp", "out", "ws"], odd=["inp", "len", "len_out", "out", "new_xyz"],
          need=("rf_farthestpointsampling_lengths_workspace_bytes", 2, 20000, 64)),
    Entry("rf_maxpool_points_lengths", [2, 100, 8, "x", "len", "out", "ws", "wsz", None], null=["x", "out", "ws"],
          odd=["len", "out"], at16=["x"], need=("rf_maxpool_points_lengths_workspace_bytes", 2, 100, 8)),
    Entry("rf_maxpool_points_idx_lengths", [2, 100, 8, "x", "len", "out", "idx", "ws", "wsz", None], null=["x", "out", "idx", "ws"],
          odd=["len", "out", "idx"], at16=["x"], need=("rf_maxpool_points_idx_lengths_workspace_bytes", 2, 100, 8)),
    # these hold only their count arrays to the 4-byte rule (the tensors: NULL alone)
    Entry("rf_knn_grad_lengths", [2, 100, 50, 4, "xyz1", "xyz2", "len1", "len2", "idx", "grad_val", "gx1", "gx2", "ws", "wsz", None],
          null=["xyz1", "xyz2", "idx", "grad_val", "gx1", "gx2", "ws"], odd=["len1", "len2"],
          need=("rf_knn_grad_lengths_workspace_bytes", 2, 100, 50, 4)),
    Entry("rf_approxmatch_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "match", None, 0, "ws", "wsz", None],
          null=["xyz1", "xyz2", "match", "ws"], odd=["len1", "len2"], need=("rf_approxmatch_lengths_workspace_bytes", 2, 300, 200, 0)),
    Entry("rf_matchcost_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "match", "cost", "ws", "wsz", None],
          null=["xyz1", "xyz2", "match", "cost", "ws"], odd=["len1", "len2"], need=("rf_matchcost_lengths_workspace_bytes", 2, 300, 200)),
    Entry("rf_matchcost_grad_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "match", "grad1", "grad2", None],
          null=["xyz1", "xyz2", "match", "grad1", "grad2"], odd=["len1", "len2"], ws16=False, small=None),
    Entry("rf_earth_mover_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "cost", None, None, "ws", "wsz", None],
          null=["xyz1", "xyz2", "cost", "ws"], odd=["len1", "len2"], need=("rf_earth_mover_lengths_workspace_bytes", 2, 300, 200)),
    Entry("rf_nn_distance_grad_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "gd1", "i1", "gd2", "i2", "gx1", "gx2", None],
          null=["xyz1", "xyz2", "gd1", "i1", "gd2", "i2", "gx1", "gx2"], odd=["len1", "len2"], ws16=False, small=None),
    Entry("rf_chamfer_loss_lengths", [B, N, M, "xyz1", "xyz2", "len1", "len2", "loss", "d1", "i1", "d2", "i2", "ws", "wsz", None],
          null=["xyz1", "xyz2", "loss", "ws"], odd=["len1", "len2"], need=("rf_chamfer_loss_lengths_workspace_bytes", B, N, M, 1, 1)),
    Entry("rf_chamfer_loss_grad_lengths", [2, 300, 200, "xyz1", "xyz2", "len1", "len2", "d1", "i1", "d2", "i2", "grad_loss", "gx1",
                                           "gx2", None],
          null=["grad_loss"], odd=["len1", "len2"], ws16=False, small=None),
    Entry("rf_merge_layer_lengths", [2, 300, 200, "raw", "new", "len_raw", "len_new", "dec", "refined", "idx2", "ws", "wsz", None],
          null=["raw", "new", "dec", "refined", "idx2", "ws"], odd=["len_raw", "len_new"],
          need=("rf_merge_layer_lengths_workspace_bytes", 2, 300, 200)),
    Entry("rf_merge_layer_grad_lengths", [2, 300, 200, "raw", "new", "len_raw", "len_new", "dec", "idx2", "grad_refined", "grad_new",
                                          "grad_dec", "grad_raw", None],
          null=["raw", "new", "dec", "idx2", "grad_refined", "grad_new", "grad_dec"], odd=["len_raw", "len_new"], ws16=False,
          small=None),
]


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.fn + ("" if e.null else "_handles"))
def test_argument_rules_are_answered_without_a_device(e):
    from rfnet_amd._lib import lib
    has_ws = "ws" in e.args
    big = dict(wsz=BIG) if has_ws else {}
    for name in e.null:
        assert e.call(lib, **{name: None}, **big) == EINVAL, f"{e.fn}: NULL {name}"
    for name in e.odd:
        assert e.call(lib, **{name: P + 2}, **big) == EINVAL, f"{e.fn}: {name} not 4-byte aligned"
    for name in e.at16:
        assert e.call(lib, **{name: P + 4}, **big) == EINVAL and e.call(lib, **{name: P + 8}, **big) == EINVAL, \
            f"{e.fn}: {name} not 16-byte aligned"
    if has_ws and e.ws16:
        assert e.call(lib, ws=WS + 4, wsz=BIG) == EINVAL and e.call(lib, ws=WS + 8, wsz=BIG) == EINVAL, f"{e.fn}: workspace"
    if has_ws and e.small is not None and e.null:
        if e.need:  # (first: a query that answered 0 would make the calls below valid ones)
            need = getattr(lib, e.need[0])(*e.need[1:])
            assert need > 0, e.need
            assert e.call(lib, wsz=need - 1) == e.small, f"{e.fn}: one byte short"
        assert e.call(lib) == e.small, f"{e.fn}: a workspace of 0 bytes"


def test_a_check_order_that_callers_can_see():
    """rf_chamfer_loss sizes before it looks at alignment: a misaligned workspace that is also too small is RF_EWORKSPACE, a
    NULL one where bytes are needed too; large enough and misaligned is RF_EINVAL, as is a misaligned sorted-set handle."""
    from rfnet_amd._lib import lib
    call = lambda ws, wsz, s1=None, x=P: lib.rf_chamfer_loss(B, N, M, x, P, s1, None, P, P, P, P, P, ws, wsz, None)
    assert lib.rf_chamfer_loss_workspace_bytes(B, N, M, 1, 1, 0, 0) > 0
    assert call(WS + 4, 0) == EWORKSPACE and call(None, BIG) == EWORKSPACE and call(WS, 0) == EWORKSPACE
    assert call(WS + 4, BIG) == EINVAL and call(WS + 8, BIG) == EINVAL
    assert call(WS, BIG, s1=WS + 8) == EINVAL
    assert call(WS, BIG, x=None) == EINVAL
    assert lib.rf_chamfer_loss(B, N, M, P, P, None, None, None, P, P, P, P, WS, BIG, None) == EINVAL   # loss
    assert lib.rf_chamfer_loss(B, N, M, P, P, None, None, P, None, P, P, None, WS, BIG, None) == EINVAL  # no whole direction
