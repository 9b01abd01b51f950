"""-m gpu: the point-in-box kernels -- fd_points_in_boxes_count / _extract (csrc/fd_points_in_boxes.hip) and fd_gt_min_points_filter
(csrc/fd_augment_map.hip) -- bit for bit against tests/points_in_boxes_ref.py and against the reference's recorded decisions
(tests/golden/points_in_boxes.npz); replay; the ``min_points_in_gt`` filter in ``aug(batch)`` and in the two static steps; the
ground-truth database writer.  The kernel and the restatement take every decision with the same fp32 operations, so the random cases
need no margin: points on faces, NaN and Inf included."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import points_in_boxes_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TILE = 64  # FD_POINTS_IN_BOXES_TILE
WG = 256   # points per workgroup
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False), class_names=["car"])


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _case(n, m, ndim, cols=12, seed=0, special=True):
    """m boxes within +-50 m (the first two overlap) and n points: most in some box's own frame within 0.75 dims (inside and just
    outside), the rest anywhere; with ``special`` a few exact-boundary points (a box centre moved by exactly half a dimension along an
    axis-aligned box), NaN and Inf coordinates"""
    r = np.random.default_rng(1000 * n + 10 * m + ndim + seed)
    boxes = np.zeros((m, cols), np.float32)
    if m:
        boxes[:, 0:2], boxes[:, 2] = r.uniform(-50, 50, (m, 2)), r.uniform(-3, 1, m)
        boxes[:, 3:6] = r.uniform([0.5, 0.6, 0.8], [3.0, 9.0, 3.5], (m, 3))
        boxes[:, 6:] = r.normal(0, 2, (m, cols - 6))
        boxes[:, -1] = r.uniform(-np.pi, np.pi, m)
        boxes[0, -1] = 0.0  # axis-aligned: its faces are hit exactly below
        boxes[0, 0:6] = (4.0, -8.0, 0.5, 2.0, 4.0, 1.0)
    if m > 1:
        boxes[1] = boxes[0]
        boxes[1, 0:2] += np.float32(0.5)
        boxes[1, -1] = 0.3
    pts = np.zeros((n, ndim), np.float32)
    pts[:, 0:2], pts[:, 2] = r.uniform(-55, 55, (n, 2)), r.uniform(-5, 3, n)
    if m and n:
        j = r.integers(0, m, n)
        near = r.random(n) < 0.8
        u = r.uniform(-0.75, 0.75, (n, 3)) * boxes[j, 3:6]
        a = boxes[j, -1].astype(np.float64)
        local = np.stack([u[:, 0] * np.cos(a) + u[:, 1] * np.sin(a) + boxes[j, 0], -u[:, 0] * np.sin(a) + u[:, 1] * np.cos(a) + boxes[j, 1],
                          u[:, 2] + boxes[j, 2]], axis=1)
        pts[near, :3] = local[near]
    pts[:, 3] = r.uniform(0, 255, n)
    if ndim == 5:
        pts[:, 4] = r.integers(0, 10, n) * 0.05
    if special and m and n >= 8:
        c = boxes[0, :3]
        pts[0, :3] = c                                     # the centre: inside
        pts[1, :3] = c + np.float32([1.0, 0.0, 0.0])       # on the +x face: outside
        pts[2, :3] = c + np.float32([0.0, -2.0, 0.0])      # on the -y face
        pts[3, :3] = c + np.float32([1.0, 2.0, 0.5])       # a corner
        pts[4, :3] = (np.nan, c[1], c[2])                  # NaN: inside every box
        pts[5, :3] = (np.inf, c[1], c[2])
        pts[6, :3] = (c[0], c[1], -np.inf)
        pts[7, :3] = (1e30, 1e30, 1e30)                    # the GT sampler's sentinel row
    return pts, boxes


def _run(hip, pts, boxes, ncols=None, n_boxes=None, cap_rows=None, guard=3):
    """count + extract on the device: (counts, rows [the rows that must be written], offsets, status); rows behind the buffer's
    ``cap_rows`` are canaries that must stay"""
    p, b = torch.from_numpy(pts).to(DEV), torch.from_numpy(boxes).to(DEV)
    nb = torch.tensor([n_boxes], dtype=torch.int32, device=DEV) if n_boxes is not None else None
    counts, ws = hip.points_in_boxes_count(p, b, n_boxes=nb)
    total = int(counts.sum())
    cap = total if cap_rows is None else cap_rows
    ncols = pts.shape[1] if ncols is None else ncols
    buf = torch.full((cap + guard, ncols), -777.0, dtype=torch.float32, device=DEV)
    rows, offsets, status = hip.points_in_boxes_extract(p, b, ws, buf[:cap], n_boxes=nb)
    torch.cuda.synchronize()
    assert bool((buf[cap:] == -777.0).all()), "rows behind cap_rows were written"
    return counts.cpu().numpy(), buf[:min(cap, total)].cpu().numpy(), offsets.cpu().numpy(), int(status[0])


def _check(hip, pts, boxes, ncols=None, n_boxes=None):
    counts, rows, offsets, status = _run(hip, pts, boxes, ncols=ncols, n_boxes=n_boxes)
    want_rows, want_off, _ = R.extract(pts, boxes, ncols=ncols, n_boxes=n_boxes)
    assert np.array_equal(counts, R.counts(pts, boxes, n_boxes)), "counts"
    assert np.array_equal(offsets, want_off) and status == 0
    assert rows.shape == want_rows.shape and np.array_equal(_bits(rows), _bits(want_rows)), "rows"
    return counts


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3 * WG + 1])
def test_count_and_extract_bit_for_bit(hip, n):
    inside = 0
    for k, m in enumerate([0, 1, 2, TILE - 1, TILE, TILE + 1]):
        ndim = 4 + (k + n) % 2
        pts, boxes = _case(n, m, ndim)
        inside += int(_check(hip, pts, boxes).sum())
        _check(hip, pts, boxes, ncols=3 if ndim == 4 else 4)  # ncols_out < ndim
    assert inside > 0 or n == 0


def test_against_the_reference_golden(hip, golden):
    g = golden("points_in_boxes.npz")
    for name in [str(v) for v in g["names"]]:
        pts, boxes, mask = g[name + "/points"], g[name + "/boxes"], g[name + "/mask"]
        counts, rows, offsets, _ = _run(hip, pts, boxes)
        assert np.array_equal(counts, g[name + "/counts"]) and np.array_equal(offsets[1:], np.cumsum(mask.sum(axis=0)))
        for j in range(boxes.shape[0]):  # the database writer's rows: points[mask] - centre
            want = pts[mask[:, j]].copy()
            want[:, :3] -= boxes[j, :3]
            assert np.array_equal(_bits(rows[offsets[j]:offsets[j + 1]]), _bits(want)), (name, j)


def test_one_box_holding_every_point_and_overlapping_boxes(hip):
    """the scan crosses the workgroups: every workgroup contributes 256 rows to the same box; identical boxes give identical rows"""
    n = 4 * WG + 37
    r = np.random.default_rng(5)
    pts = np.zeros((n, 5), np.float32)
    pts[:, :3] = r.uniform(-1, 1, (n, 3))
    pts[:, 3] = np.arange(n)
    boxes = np.zeros((3, 7), np.float32)
    boxes[:, 3:6] = 10.0
    boxes[1, 0] = 100.0  # an empty box between two full ones
    counts = _check(hip, pts, boxes)
    assert counts.tolist() == [n, 0, n]
    _, rows, offsets, _ = _run(hip, pts, boxes)
    assert offsets.tolist() == [0, n, n, 2 * n] and np.array_equal(rows[:n, 3], np.arange(n, dtype=np.float32)), "cloud order"
    assert np.array_equal(_bits(rows[:n]), _bits(rows[n:]))


def test_special_values(hip):
    pts, boxes = _case(300, 5, 5)
    m = R.mask(pts, boxes)
    assert m[0, 0] and not m[1, 0] and not m[2, 0] and not m[3, 0], "centre inside; face, edge and corner points outside"
    assert m[4].all(), "a NaN coordinate is inside every box"
    assert not m[5].any() and not m[6].any() and not m[7].any(), "Inf and the sentinel row are in no box"
    _check(hip, pts, boxes)
    flat = boxes.copy()
    flat[2, 3:6] = 0.0  # a zero-size box holds no finite point
    assert R.counts(pts[np.isfinite(pts).all(axis=1)], flat)[2] == 0
    _check(hip, pts, flat)
    swapped = boxes.copy()  # the answer follows the LAST column
    swapped[:, 10], swapped[:, 11] = boxes[:, 11] + 0.7, boxes[:, 11]
    assert np.array_equal(_check(hip, pts, swapped), _check(hip, pts, boxes))
    swapped[:, 11] = boxes[:, 11] + 0.7
    assert not np.array_equal(R.mask(pts, swapped), m)


def test_device_count_below_n_boxes_max_with_poisoned_rows(hip):
    pts, boxes = _case(600, TILE + 9, 4)
    full = R.counts(pts, boxes)
    for nb in (0, 1, TILE - 1, TILE, TILE + 3, TILE + 9, TILE + 50, -4):
        poisoned = boxes.copy()
        poisoned[max(min(nb, len(boxes)), 0):] = np.nan  # a NaN box would hold every point
        counts = _check(hip, pts, poisoned, n_boxes=nb)
        k = max(min(nb, len(boxes)), 0)
        assert np.array_equal(counts[:k], full[:k]) and not counts[k:].any()


def test_cap_rows_one_short(hip):
    pts, boxes = _case(700, 9, 5)
    want, off, _ = R.extract(pts, boxes)
    total = len(want)
    assert total > 20
    counts, rows, offsets, status = _run(hip, pts, boxes, cap_rows=total - 1)
    assert status == R.NO_ROOM and np.array_equal(offsets, off) and np.array_equal(_bits(rows), _bits(want[:total - 1]))
    counts, rows, offsets, status = _run(hip, pts, boxes, cap_rows=total + 2)
    assert status == 0 and np.array_equal(_bits(rows), _bits(want))
    assert _run(hip, pts, boxes, cap_rows=0)[3] == R.NO_ROOM


def test_front_end_refusals(hip):
    E = hip.FutureDetHipError
    p, b = torch.zeros((10, 5), device=DEV), torch.zeros((3, 12), device=DEV)
    with pytest.raises(E, match=r"\[n, 4\] or \[n, 5\]"):
        hip.points_in_boxes_count(torch.zeros((10, 3), device=DEV), b)
    with pytest.raises(E, match=">= 7"):
        hip.points_in_boxes_count(p, torch.zeros((3, 6), device=DEV))
    with pytest.raises(E, match="contiguous"):
        hip.points_in_boxes_count(p, torch.zeros((12, 3), device=DEV).t())
    with pytest.raises(E, match="ONE int32"):
        hip.points_in_boxes_count(p, b, n_boxes=torch.zeros((2,), dtype=torch.int32, device=DEV))
    with pytest.raises(E, match="out must be int32"):
        hip.points_in_boxes_count(p, b, out=torch.zeros((4,), dtype=torch.int32, device=DEV))
    with pytest.raises(E, match="workspace holds"):
        hip.points_in_boxes_count(p, b, workspace=torch.zeros((8,), dtype=torch.uint8, device=DEV))
    counts, ws = hip.points_in_boxes_count(p, b)
    with pytest.raises(E, match="rows must be"):
        hip.points_in_boxes_extract(p, b, ws, torch.zeros((4, 6), device=DEV))
    with pytest.raises(E, match="offsets must be"):
        hip.points_in_boxes_extract(p, b, ws, torch.zeros((4, 5), device=DEV), offsets=torch.zeros((3,), dtype=torch.int64, device=DEV))
    with pytest.raises(E, match="point_counts must be int32"):
        hip.gt_min_points_filter(torch.zeros((1, 1, 3, 12), device=DEV), torch.zeros((1, 1), dtype=torch.int32, device=DEV),
                                 torch.zeros((1, 1, 3), dtype=torch.int32, device=DEV), torch.zeros((1, 4), dtype=torch.int32, device=DEV), 1)


# ---------------------------------------------------------------------------------------------------------------------- replay
def test_two_runs_give_the_same_bits(hip):
    pts, boxes = _case(5 * WG + 3, TILE + 5, 5)
    a, b = _run(hip, pts, boxes), _run(hip, pts, boxes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


def test_graph_capture_and_replay_with_changed_inputs(hip):
    n, m = 2 * WG + 11, TILE + 2
    p = torch.zeros((n, 5), device=DEV)
    b = torch.zeros((m, 12), device=DEV)
    nb = torch.zeros((1,), dtype=torch.int32, device=DEV)
    counts = torch.zeros((m,), dtype=torch.int32, device=DEV)
    ws = hip.points_in_boxes_workspace(n, m, DEV)
    rows = torch.zeros((4 * n, 4), device=DEV)
    offsets, status = torch.zeros((m + 1,), dtype=torch.int64, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)

    def launch():
        hip.points_in_boxes_count(p, b, n_boxes=nb, out=counts, workspace=ws)
        hip.points_in_boxes_extract(p, b, ws, rows, n_boxes=nb, offsets=offsets, status=status)

    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            launch()
    for seed, k in ((1, m), (2, TILE - 3)):
        pts, boxes = _case(n, m, 5, seed=seed)
        p.copy_(torch.from_numpy(pts)), b.copy_(torch.from_numpy(boxes)), nb.fill_(k), rows.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        want, off, _ = R.extract(pts, boxes, ncols=4, n_boxes=k)
        assert len(want) <= 4 * n and int(status[0]) == 0
        assert np.array_equal(counts.cpu().numpy(), R.counts(pts, boxes, k)) and np.array_equal(offsets.cpu().numpy(), off)
        assert np.array_equal(_bits(rows[:len(want)]), _bits(want)) and bool((rows[len(want):] == -1.0).all())


# ---------------------------------------------------------------------------------------------------------------------- the filter
def _filter_case(B, T, n_max, seed):
    r = np.random.default_rng(seed)
    boxes = r.normal(0, 10, (B, T, n_max, 12)).astype(np.float32)
    counts = np.zeros((B, T), np.int32)
    counts[:] = r.integers(n_max // 2, n_max + 1, (B, 1))
    classes = r.integers(1, 11, (B, T, n_max)).astype(np.int32)
    traj = r.integers(0, 3, (B, T, n_max)).astype(np.int32)
    pc = r.integers(0, 9, (B, n_max)).astype(np.int32)
    return boxes, counts, classes, traj, pc


def _check_filter(hip, case, min_points, inplace, with_traj=True):
    boxes, counts, classes, traj, pc = case
    t = [torch.from_numpy(a.copy()).to(DEV) for a in (boxes, counts, classes, traj)]
    out = hip.gt_min_points_filter(t[0], t[1], t[2], torch.from_numpy(pc).to(DEV), min_points, trajectory=t[3] if with_traj else None,
                                   out="inplace" if inplace else None)
    torch.cuda.synchronize()
    want = R.min_points_filter(boxes, counts, classes, traj if with_traj else None, pc, min_points)
    assert np.array_equal(_bits(out[0]), _bits(want[0])) and np.array_equal(out[1].cpu().numpy(), want[1])
    assert np.array_equal(out[2].cpu().numpy(), want[2]) and np.array_equal(out[4].cpu().numpy(), want[4])
    if with_traj:
        assert np.array_equal(out[3].cpu().numpy(), want[3])
    else:
        assert out[3] is None
    assert (out[0] is t[0]) == inplace
    return want


@pytest.mark.parametrize("T", [1, 3])
def test_min_points_filter_exact(hip, T):
    for n_max in (1, 63, 65, 300):
        case = _filter_case(2, T, n_max, 10 * T + n_max)
        for inplace in (False, True):
            want = _check_filter(hip, case, 4, inplace)
        pc, c0 = case[4], case[1][:, 0]
        for b in range(2):  # count == min is kept, min - 1 is dropped; behind the count: zero padding
            assert want[1][b, 0] == int((pc[b, :c0[b]] >= 4).sum())
            assert not want[0][b, :, want[1][b, 0]:].any() and not want[2][b, :, want[1][b, 0]:].any()
        _check_filter(hip, case, 4, False, with_traj=False)
    case = _filter_case(2, T, 40, 99)
    case[4][0, :5] = (3, 4, 5, 4, 3)
    case[1][0] = 5
    assert _check_filter(hip, case, 4, True)[1][0, 0] == 3
    assert _check_filter(hip, case, 0, False)[1][0, 0] == 5 and _check_filter(hip, case, 100, False)[1][0, 0] == 0
    if T > 1:  # the count-mismatch status
        case[1][1, 1] = case[1][1, 0] - 2
        case[1][0, T - 1] = 41
        assert _check_filter(hip, case, 4, True)[4].tolist() == [1, 1]


def test_range_filter_results_keep_their_bits(hip):
    """fd_gt_range_filter shares its compaction with the new filter: on a mask both can express -- every corner inside or every corner
    far outside -- the two give the same bytes, and the range filter still gives the restatement's (its own tests pin the rest)"""
    import range_filter_ref as rf

    r = np.random.default_rng(3)
    boxes, counts, classes, traj, _ = _filter_case(2, 3, 70, 7)
    boxes[..., 3:6] = r.uniform(1, 3, boxes[..., 3:6].shape)
    boxes[..., 0:2] = np.where(r.random((2, 1, 70, 1)) < 0.5, r.uniform(-30, 30, (2, 3, 70, 2)), r.uniform(200, 300, (2, 3, 70, 2)))
    rng = (-54.0, -54.0, 54.0, 54.0)
    keep = np.stack([rf.mask(boxes[b, 0], rng) for b in range(2)])
    t = [torch.from_numpy(a).to(DEV) for a in (boxes, counts, classes, traj)]
    a = hip.gt_range_filter(t[0], t[1], t[2], rng, trajectory=t[3])
    b = hip.gt_min_points_filter(t[0], t[1], t[2], torch.from_numpy(keep.astype(np.int32)).to(DEV), 1, trajectory=t[3])
    want = rf.apply(boxes, counts, classes, traj, rng)
    for x, y, w in zip(a, b, want):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(w))
    assert 0 < int(a[1].sum()) < int(t[1].sum())


# ---------------------------------------------------------------------------------------------------------------------- eager path and steps
@pytest.fixture
def deterministic_convs():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def world(hip):
    from futuredet_amd.targets import TargetAssigner
    from test_gpu_train_static import MAX_VOXELS, _World

    w = _World()
    w.vg = dict(w.vg, range=[-28.8, -28.8, -5.0, 28.8, 28.8, 3.0], max_voxel_num=[MAX_VOXELS, MAX_VOXELS])
    w.ta = TargetAssigner(w.cfg.train_cfg.assigner, np.array([768, 768, 40]), w.vg["range"], w.vg["voxel_size"])
    return w


@pytest.fixture(scope="module")
def pillars(hip):
    from futuredet_amd.targets import TargetAssigner
    from test_gpu_pillars_static import _Pillars

    w = _Pillars()
    rng = list(w.vg["range"])
    rng[0], rng[1], rng[3], rng[4] = -25.6, -25.6, 25.6, 25.6
    w.vg = dict(w.vg, range=rng)
    w.grid = np.array([256, 256, 1])
    w.ta = TargetAssigner(w.cfg.train_cfg.assigner, w.grid, w.vg["range"], w.vg["voxel_size"])
    return w


MIN_POINTS = 4


def _with_points_in_boxes(batch):
    """the batch with i % 8 points put at (and around) the centre of object i of every cloud's timestep-0 boxes: counts on both sides of
    MIN_POINTS whatever the scene holds"""
    out = dict(batch)
    clouds = []
    for b, c in enumerate(batch["clouds"]):
        boxes = batch["gt_boxes"][b, 0].cpu().numpy()
        r = np.random.default_rng(b)
        extra = []
        for i in range(int(batch["gt_counts"][b, 0])):
            p = np.zeros((i % 8, c.shape[1]), np.float32)
            p[:, :3] = boxes[i, :3] + r.uniform(-0.2, 0.2, (i % 8, 3)).astype(np.float32)
            p[:, 3] = 7.0
            extra.append(p)
        clouds.append(torch.cat([c, torch.from_numpy(np.concatenate(extra)).to(DEV)]).contiguous())
    out["clouds"] = clouds
    return out


def _augment(point_filter=True, sampler=None, **kw):
    from futuredet_amd.augment import GlobalAugment

    cfg = dict(CFG, min_points_in_gt=MIN_POINTS, **kw)
    if sampler is not None:
        cfg["db_sampler"] = dict(enable=True, sample_groups=[dict(car=40)], global_random_rotation_range_per_object=[0, 0])
    return GlobalAugment(cfg, seed=3, point_filter=point_filter, sampler=sampler)


def _restated_filter(batch):
    traj = batch.get("gt_trajectory")
    boxes = batch["gt_boxes"].cpu().numpy()
    pc = np.stack([R.counts(c.cpu().numpy(), boxes[b, 0], int(batch["gt_counts"][b, 0])) for b, c in enumerate(batch["clouds"])])
    return R.min_points_filter(boxes, batch["gt_counts"].cpu().numpy(), batch["gt_classes"].cpu().numpy(),
                               traj.cpu().numpy() if traj is not None else None, pc, MIN_POINTS), pc


def test_aug_batch_filters_first(world):
    from futuredet_amd.augment import GlobalAugment, filter_gt_by_min_points, points_count_rbbox

    batch = _with_points_in_boxes(world.batch([5, 6], [4000, 2500]))
    (wb, wc, wk, wt, ws), pc = _restated_filter(batch)
    assert 3 <= wc[0, 0] <= 21 and (wc[:, 0] == (pc[:, :24] >= MIN_POINTS).sum(axis=1)).all()
    got = filter_gt_by_min_points(batch, MIN_POINTS)
    assert np.array_equal(_bits(got["gt_boxes"]), _bits(wb)) and np.array_equal(got["gt_counts"].cpu().numpy(), wc)
    assert np.array_equal(got["gt_classes"].cpu().numpy(), wk) and np.array_equal(got["gt_point_counts"].cpu().numpy(), pc)
    assert got["gt_boxes"] is not batch["gt_boxes"] and not bool(got["gt_min_points_status"].any())
    assert np.array_equal(points_count_rbbox(batch["clouds"][0], batch["gt_boxes"][0, 0]).cpu().numpy(), pc[0])
    # aug(batch): the filter on the raw batch, then the transforms of the filtered one
    aug, off = _augment(), _augment(point_filter=True, no_augmentation=True)
    assert aug.min_points == MIN_POINTS and off.min_points == 0
    params = aug.draw(2)
    out = aug(batch, params)
    want = GlobalAugment(CFG, seed=0)(got, params)
    for k in ("gt_boxes", "gt_counts", "gt_classes"):
        assert torch.equal(out[k], want[k]), k
    for a, b in zip(out["clouds"], want["clouds"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(off(batch)["gt_counts"], batch["gt_counts"]) and _augment(mode="val").min_points == 0


def test_a_sampled_entry_with_few_points_survives(world):
    """sampling comes after the filter: database entries of 8..29 points join a ground truth filtered at 40 points per object"""
    from futuredet_amd.augment import GlobalAugment
    from test_gpu_augment import _pad_gt
    from test_gpu_gt_sample import _candidates, _sampler

    sampler = _sampler(point_cap=300)
    cfg = dict(CFG, min_points_in_gt=40, db_sampler=dict(enable=True, sample_groups=[dict(car=40)], global_random_rotation_range_per_object=[0, 0]))
    aug = GlobalAugment(cfg, seed=3, sampler=sampler, point_filter=True)
    batch = _pad_gt(_with_points_in_boxes(world.batch([5], [4000])), 32)
    batch = dict(batch, aug_params=aug.draw(1), gt_sample_candidates=_candidates(1, sampler.K, 9))
    out = aug(batch)
    kept, acc = int(out["gt_point_counts"][0, :24].ge(40).sum()), int(out["gt_sample_accepted"].sum())
    assert kept < 24 and acc > 0 and int(out["gt_counts"][0, 0]) == kept + acc
    assert int(sampler.database.host["rows"].max()) < 40
    # and the step loads the same: filter, selection, transforms
    step = world.step(1, augment=aug)
    step._load(batch, 0)
    torch.cuda.synchronize()
    assert torch.equal(step.gt_counts, out["gt_counts"]) and torch.equal(step.gt_sample["accepted"], out["gt_sample_accepted"])
    c = int(out["gt_counts"][0, 0])
    assert torch.equal(step.gt_boxes[:, :, :c].view(torch.int32), out["gt_boxes"][:, :, :c].view(torch.int32))
    assert torch.equal(step.gt_classes[:, :, :c], out["gt_classes"][:, :, :c])
    n = out["clouds"][0].shape[0]
    assert torch.equal(step.points[0, :n].view(torch.int32), out["clouds"][0].view(torch.int32))


def _step_equivalence(w, batch):
    """a static step with the filter, without a host synchronisation, against aug(batch) followed by the plain step"""
    from test_gpu_augment import _run, _same
    from test_gpu_train_static import _flat

    B = len(batch["clouds"])
    aug = _augment()
    params = aug.draw(B)
    fed = dict(batch, aug_params=params)
    w.fresh()
    step = w.step(B, augment=aug)
    assert step.point_filter is not None and step.point_filter["min_points"] == MIN_POINTS
    step.warm_up([fed])
    step(fed, check=False)  # first call: capacities, scratch and permutations uploaded
    torch.cuda.synchronize()
    w.fresh()
    step.iteration = 0
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(fed, check=False)
        with pytest.raises(RuntimeError):
            out["loss"][0].item()  # the mode is enforced
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert not step.overflowed()
    l1, s1 = _flat(out), w.state()
    (wb, wc, wk, wt, ws), pc = _restated_filter(batch)
    assert np.array_equal(step.gt_counts.cpu().numpy(), wc) and 3 <= wc[0, 0] <= 21
    assert np.array_equal(step.point_filter["counts"][:, :pc.shape[1]].cpu().numpy(), pc) and not bool(step.point_filter["status"].any())
    pre = aug(batch, params)
    assert np.array_equal(pre["gt_counts"].cpu().numpy(), wc)
    l2, s2, _ = _run(w, pre)
    _same(l1, l2, "min_points_in_gt: loss terms")
    _same(s1, s2, "min_points_in_gt: state")
    l3, _, _ = _run(w, dict(batch, aug_params=params), augment=_inactive())
    assert not all(torch.equal(l1[k], l3[k]) for k in l1), "the filtered batch is another batch"


def _inactive():
    from futuredet_amd.augment import GlobalAugment

    return GlobalAugment(CFG, seed=3, point_filter=True)  # the keyword without min_points_in_gt: nothing to do


def test_step_equivalence_voxelnet(world, deterministic_convs):
    _step_equivalence(world, _with_points_in_boxes(world.batch([5], [4000])))


def test_step_equivalence_pillars(pillars, deterministic_convs):
    _step_equivalence(pillars, _with_points_in_boxes(pillars.batch([2], [6000])))


@pytest.mark.parametrize("which", ["world", "pillars"])
def test_a_step_with_an_inactive_filter_loads_what_it_loaded_before(request, hip, which):
    from futuredet_amd.augment import GlobalAugment

    w = request.getfixturevalue(which)
    batch = _with_points_in_boxes(w.batch([2], [3000]))
    a, b = w.step(1, augment=_inactive()), w.step(1, augment=GlobalAugment(CFG, seed=3))
    c = w.step(1, augment=_augment(no_augmentation=True))  # min_points_in_gt set, but the reference filters in its augmenting branch only
    assert a.point_filter is None and b.point_filter is None and c.point_filter is None
    params = GlobalAugment(CFG, seed=3).draw(1)
    for s in (a, b):
        s._load(dict(batch, aug_params=params), 0)
    torch.cuda.synchronize()
    for k in ("points", "counts", "gt_boxes", "gt_counts", "gt_classes"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.gt_counts, batch["gt_counts"])


# ---------------------------------------------------------------------------------------------------------------------- the database
def _samples():
    out = []
    names = ["car", "pedestrian", "truck"]
    for k, (n, m, ndim) in enumerate([(900, 6, 5), (400, 0, 5), (700, 4, 5)]):
        pts, boxes0 = _case(n, m, ndim, special=False, seed=50 + k)
        r = np.random.default_rng(k)
        boxes = np.stack([boxes0, boxes0 + r.normal(0, 0.3, boxes0.shape).astype(np.float32)])  # T = 2
        out.append(dict(points=pts, boxes=boxes, names=[names[i % 3] for i in range(m)], trajectory=[("static", "linear", "nonlinear")[(i + k) % 3] for i in range(m)],
                        image_idx=100 + k))
    return out


def test_create_gt_database_and_round_trip(hip, tmp_path):
    from futuredet_amd.augment import GTDatabase, create_gt_database

    samples = _samples()
    db_path, info_path = tmp_path / "gt_database_10sweeps", tmp_path / "dbinfos.pkl"
    infos = create_gt_database([dict(s, points=torch.from_numpy(s["points"]).to(DEV)) for s in samples], db_path, info_path)
    files, want = R.database_files(samples, "gt_database_10sweeps")
    with open(info_path, "rb") as f:
        stored = pickle.load(f)
    assert list(stored) == list(want) == list(infos) and sum(len(v) for v in want.values()) == 10
    on_disk = sorted(os.path.relpath(os.path.join(d, f), tmp_path) for d, _, fs in os.walk(db_path) for f in fs)
    assert on_disk == sorted(files)
    some_points = 0
    for name in want:
        assert len(stored[name]) == len(want[name])
        for got, w in zip(stored[name], want[name]):
            assert set(got) == {"name", "trajectory", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty", "group_id"}
            for k in ("name", "trajectory", "path", "image_idx", "gt_idx", "num_points_in_gt", "group_id"):
                assert got[k] == w[k], (name, k)
            assert [int(d) for d in got["difficulty"]] == w["difficulty"] and len(got["box3d_lidar"]) == 2
            assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got["box3d_lidar"], w["box3d_lidar"]))
            raw = open(os.path.join(tmp_path, got["path"]), "rb").read()
            assert raw == files[w["path"]].tobytes() and len(raw) == 20 * got["num_points_in_gt"]
            some_points += got["num_points_in_gt"]
    assert some_points > 50
    # the round trip, and what num_points_in_gt feeds
    classes = ["car", "truck", "pedestrian"]
    a = GTDatabase.from_dbinfos(str(info_path), str(tmp_path), classes, 5, device=DEV)
    b = GTDatabase.from_samples(samples, classes, device=DEV)
    for k in ("boxes", "steps", "classes", "trajectory", "offsets", "points"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert len(a) == 10
    least = sorted(i["num_points_in_gt"] for i in stored["car"])[1]
    c = GTDatabase.from_dbinfos(str(info_path), str(tmp_path), ["car"], 5, db_prep_steps=[dict(filter_by_min_num_points=dict(car=least + 1))], device=DEV)
    assert len(c) == sum(i["num_points_in_gt"] > least for i in stored["car"]) < len(stored["car"])
    used = create_gt_database(samples[:1], tmp_path / "only_cars", tmp_path / "cars.pkl", used_classes=["car"], num_point_features=4, device=DEV)
    assert list(used) == ["car"] and os.path.getsize(os.path.join(tmp_path, used["car"][0]["path"])) == 16 * used["car"][0]["num_points_in_gt"]
