"""Host side of the NMS edge tests (no GPU): the C restatement of the rotated IoU reproduces the compiled reference's values on the degenerate
pairs of tests/golden/iou_edges.npz bit for bit, and the keep lists that test_gpu_nms_edges.py expects of the kernels -- written down from the
construction of each pattern in nms_edge_cases.py -- are what the oracle's greedy sweep returns on the crafted boxes."""
import numpy as np
import pytest

import nms_edge_cases as nec
from parity_util import nms_layout


def test_restatement_reproduces_the_compiled_reference_on_degenerate_pairs(golden):
    from oracle import ops as oops

    g = golden("iou_edges.npz")
    a, b, ref = g["a"], g["b"], g["iou"]
    names = [str(s) for s in g["family_names"]]
    assert 600 <= len(a) <= 1000 and a.shape == b.shape == (len(ref), 7) and np.all(np.isfinite(ref))
    counts = np.bincount(g["family"], minlength=len(names))
    assert names == ["identical", "axis0", "contain", "quarter", "nearpar", "extents", "range_edge", "threshold"] and counts.min() >= 36, counts
    # pair by pair, as recorded, and as the diagonal of the full matrix (the form the GPU test launches)
    pair = np.array([oops.boxes_iou_bev(a[i:i + 1], b[i:i + 1])[0, 0] for i in range(len(a))], np.float32)
    assert np.array_equal(pair.view(np.uint32), ref.view(np.uint32)), np.nonzero(pair != ref)[0][:10]
    full = np.diagonal(oops.boxes_iou_bev(a, b)).astype(np.float32)
    assert np.array_equal(full.view(np.uint32), ref.view(np.uint32))
    # what the families are there for
    fam = {n: g["family"] == i for i, n in enumerate(names)}
    assert np.all(np.abs(ref[fam["identical"]] - 1.0) <= 1e-5)
    assert np.all(a[fam["axis0"], 6] == 0) and np.all(b[fam["axis0"], 6] == 0) and np.all(a[fam["threshold"], 6] == 0)
    t = ref[fam["threshold"]]
    assert (t < 0.2).sum() >= 20 and (t > 0.2).sum() >= 20 and np.abs(t - 0.2).min() < 1e-3  # both sides of the NMS threshold, in steps of 1e-3
    assert ref[fam["extents"]].max() > 100.0  # the reference's IoU is not bounded by 1 on vanishing extents


@pytest.mark.parametrize("n", nec.SIZES)
@pytest.mark.parametrize("name", nec.PATTERNS)
def test_expected_keep_lists_are_the_oracles(name, n):
    """Two independent derivations of every expected answer: the list written down from the construction and the oracle's greedy sweep on the
    boxes -- in the layout fd_rotated_nms gets them and in the layout the decode hands to its NMS (extents swapped, yaw -pi/2: no longer an
    exact angle).  Every pair's IoU is at least 0.05 away from the threshold, so neither list hangs on rounding."""
    from oracle import ops as oops

    pos, want = nec.pattern(name, n)
    assert len(pos) == n and want == sorted(set(want)) and want[0] == 0
    b = nec.boxes(pos)
    for layout in (b, nms_layout(b)):
        iou = oops.boxes_iou_bev(layout, layout)
        assert nec.iou_clear_of_threshold(iou), (name, n)
        assert oops.nms(layout, nec.IOU_THR).tolist() == want, (name, n)
        assert nec.greedy(iou > nec.IOU_THR) == want
    # the circular predicate (squared centre distance <= radius, circle_nms_jit.py) on the same scenes gives the same lists
    xy = b[:, :2]
    assert nec.radius_clear_of_distances(xy)
    d = (xy[:, None, 0] - xy[None, :, 0]) ** 2 + (xy[:, None, 1] - xy[None, :, 1]) ** 2  # float32, as the kernel evaluates it
    assert nec.greedy(d <= np.float32(nec.RADIUS)) == want


def test_patterns_reach_the_block_boundaries_they_are_named_for():
    assert nec.pattern("chain", 129)[1][31:33] == [62, 64] and 128 in nec.pattern("chain", 129)[1]   # 63 -> 64 and 127 -> 128 crossings
    starts = nec.pattern("clusters", 1000)[1]
    assert {0, 1, 3, 62, 63, 64}.issubset(starts) and np.diff(starts + [1000]).tolist()[5:10] == [63, 64, 65, 1, 2]
    pos, keep = nec.pattern("late", 1000)
    same0 = np.nonzero((pos == pos[0]).all(1))[0]
    assert same0[1] >= 960 and len(same0) > 20 and keep[:2] == [0, 1] and keep[2] >= 960  # row 0 suppresses rows of column block 15 only
    # with post_max 83 the sweep stops in the middle of block 1 ("free") and of block 2 ("chain")
    assert nec.pattern("free", 1000)[1][82] == 82 and nec.pattern("chain", 1000)[1][82] == 164
