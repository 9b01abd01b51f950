"""The host side of the point-in-box kernels (csrc/fd_points_in_boxes.hip, fd_gt_min_points_filter in csrc/fd_augment_map.hip,
futuredet_amd/augment.py, the ``point_filter`` keyword of GlobalAugment): the numpy restatement (tests/points_in_boxes_ref.py) against the
reference's recorded decisions (tests/golden/points_in_boxes.npz) and against closed forms, exported symbols and ctypes prototypes,
every argument check (no device needed: they come before any device work), the workspace function, and when the filter is accepted and
active.  CPU only."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import points_in_boxes_ref as R  # noqa: E402
from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402

NAMES = {"fd_points_in_boxes_workspace_bytes", "fd_points_in_boxes_count", "fd_points_in_boxes_extract", "fd_gt_min_points_filter"}
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False), class_names=["car"])


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _define(name):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    return re.search(r"#define %s (\S+)" % name, hdr).group(1)


# ---- the restatement against the reference
def test_restatement_gives_the_reference_decisions_exactly(golden):
    g = golden("points_in_boxes.npz")
    names = [str(n) for n in g["names"]]
    assert names == ["c12_p5", "c12_p4", "c7_p5", "c7_p4"] and float(g["margin"]) == 1e-3
    for name in names:
        pts, boxes, mask, counts = (g["%s/%s" % (name, k)] for k in ("points", "boxes", "mask", "counts"))
        assert pts.dtype == np.float32 and boxes.dtype == np.float32 and mask.dtype == np.bool_
        assert pts.shape == (1200, int(name[-1])) and boxes.shape == (8, int(name[1:].split("_")[0])) and mask.shape == (1200, 8)
        assert mask.any(axis=0).all() and (mask.sum(axis=1) >= 2).any()
        assert np.array_equal(R.mask(pts, boxes), mask), name
        assert np.array_equal(R.counts(pts, boxes), counts), name
        rows, offsets, status = R.extract(pts, boxes)
        assert status == 0 and np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)]))
        for j in range(8):  # what create_gt_database writes for object j
            want = pts[mask[:, j]].copy()
            want[:, :3] -= boxes[j, :3]
            assert np.array_equal(rows[offsets[j]:offsets[j + 1]].view(np.int32), want.view(np.int32))
    boxes = g["c12_p5/boxes"].copy()  # the angle is column 11: reading column 10 changes decisions
    boxes[:, 11] = boxes[:, 10]
    assert (R.mask(g["c12_p5/points"], boxes) != g["c12_p5/mask"]).sum() > 40


# ---- closed forms
def _unit_box(cols=12):
    b = np.zeros((1, cols), np.float32)
    b[0, 3:6] = 1.0
    return b


def test_unit_box_faces_edges_and_corners_are_outside():
    b = _unit_box()
    h = 0.5
    inside = [(0, 0, 0), (0.49, -0.49, 0.49), (-0.25, 0.25, 0)]
    faces = [(h, 0, 0), (-h, 0, 0), (0, h, 0), (0, -h, 0), (0, 0, h), (0, 0, -h), (h, 0.2, -0.3)]
    edges = [(h, h, 0), (-h, 0, h), (0, -h, -h)]
    corners = [(sx * h, sy * h, sz * h) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    outside = [(0.51, 0, 0), (0, 0, -0.75), (3, 3, 3)]
    pts = np.array(inside + faces + edges + corners + outside, np.float32)
    pts = np.concatenate([pts, np.zeros((len(pts), 2), np.float32)], axis=1)
    m = R.mask(pts, b)[:, 0]
    assert m.tolist() == [True] * len(inside) + [False] * (len(pts) - len(inside))
    n, d = R.planes(b)
    assert sorted(map(tuple, n[0].tolist())) == sorted([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]) and (d == -0.5).all()
    for cols in (7, 9):  # any row width: the angle is the last column
        assert np.array_equal(R.mask(pts, _unit_box(cols))[:, 0], m)
    assert R.counts(pts, b).tolist() == [len(inside)] and R.counts(pts, b).dtype == np.int32


def test_nan_is_inside_and_a_zero_size_box_holds_nothing():
    b = _unit_box()
    pts = np.zeros((4, 4), np.float32)
    pts[0, 0], pts[1, 1], pts[2, 2] = np.nan, np.nan, np.nan
    pts[3, :3] = (np.inf, 0, 0)
    assert R.mask(pts, b)[:, 0].tolist() == [True, True, True, False]
    far = b.copy()
    far[0, 0] = 1e6
    assert R.mask(pts, far)[:, 0].tolist() == [True, True, True, False], "as in the reference: a NaN is never >= 0"
    zero = _unit_box()
    zero[0, 3:6] = 0.0
    r = np.random.default_rng(0)
    cloud = np.concatenate([r.normal(0, 1e-3, (500, 4)), np.zeros((1, 4))]).astype(np.float32)  # the centre itself too
    assert not R.mask(cloud, zero).any()


def test_the_answer_follows_column_11():
    b = _unit_box()
    b[0, 3:6] = (1.0, 8.0, 1.0)  # long in y
    b[0, 10], b[0, 11] = np.pi / 2, 0.0
    pts = np.array([[0, 3, 0, 0], [3, 0, 0, 0]], np.float32)
    assert R.mask(pts, b)[:, 0].tolist() == [True, False]
    b[0, 10], b[0, 11] = 0.0, np.pi / 2
    assert R.mask(pts, b)[:, 0].tolist() == [False, True]
    quarter = R.corners(b)[0]  # rotation_3d_in_axis: x' = x c + y s, y' = -x s + y c: corner 0 (-w/2, -l/2) turns to about (-4, 0.5)
    assert np.allclose(quarter[0], (-4.0, 0.5, -0.5), atol=1e-6)


def test_sentinel_rows_are_in_no_finite_box():
    assert float(_define("FD_GT_SAMPLE_SENTINEL").rstrip("f")) == hip_ops.GT_SAMPLE_SENTINEL == 1e30
    r = np.random.default_rng(1)
    boxes = np.zeros((200, 12), np.float32)
    boxes[:, 0:3] = r.uniform(-80, 80, (200, 3))
    boxes[:, 3:6] = r.uniform(0.1, 30, (200, 3))
    boxes[:, 11] = r.uniform(-4, 4, 200)
    sentinel = np.array([[1e30, 1e30, 1e30, 0, 0]], np.float32)
    assert not R.mask(sentinel, boxes).any()


def test_restatement_of_the_extraction_the_filter_and_the_files():
    pts = np.zeros((6, 5), np.float32)
    pts[:, 0] = (0.1, 5.0, 0.2, 5.1, -0.1, 9.0)
    pts[:, 3] = np.arange(6)
    boxes = np.zeros((3, 12), np.float32)
    boxes[:, 3:6] = 1.0
    boxes[1, 0], boxes[2, 0] = 5.0, 0.25
    rows, offsets, status = R.extract(pts, boxes, ncols=4)
    assert offsets.tolist() == [0, 3, 5, 8] and status == 0 and rows.shape == (8, 4)
    assert rows[:, 3].tolist() == [0, 2, 4, 1, 3, 0, 2, 4], "box after box, cloud order; a point in two boxes appears under both"
    assert np.array_equal(rows[5:, 0], pts[[0, 2, 4], 0] - np.float32(0.25))
    assert R.extract(pts, boxes, n_boxes=1)[1].tolist() == [0, 3, 3, 3]
    short = R.extract(pts, boxes, cap_rows=7)
    assert short[2] == R.NO_ROOM and np.array_equal(short[0], rows_all(pts, boxes)[:7])
    # the filter: count == min is kept, min - 1 dropped, the same mask at every timestep, zero padding
    gt = np.arange(2 * 2 * 4 * 12, dtype=np.float32).reshape(2, 2, 4, 12) + 1
    counts = np.array([[4, 4], [3, 2]], np.int32)
    classes = np.arange(16, dtype=np.int32).reshape(2, 2, 4) + 1
    pc = np.array([[5, 4, 6, 0], [9, 0, 9, 9]], np.int32)
    ob, oc, ok, ot, st = R.min_points_filter(gt, counts, classes, None, pc, 5)
    assert oc.tolist() == [[2, 2], [2, 1]] and st.tolist() == [0, 1] and ot is None
    assert np.array_equal(ob[0, 1, :2], gt[0, 1, [0, 2]]) and not ob[0, :, 2:].any() and ok[0, 0].tolist() == [1, 3, 0, 0]
    assert np.array_equal(ob[1, 1, :1], gt[1, 1, [0]]) and ok[1, 1].tolist() == [13, 0, 0, 0]
    # the files
    sample = dict(points=pts, boxes=np.stack([boxes, boxes]), names=["car", "truck", "car"], trajectory=["static", "linear", "static"], image_idx=7)
    files, infos = R.database_files([sample, dict(sample, boxes=np.zeros((2, 0, 12), np.float32), names=[], trajectory=[])], "db")
    assert sorted(files) == [os.path.join("db", "car", "7_car_0.bin"), os.path.join("db", "car", "7_car_2.bin"), os.path.join("db", "truck", "7_truck_1.bin")]
    assert [i["num_points_in_gt"] for i in infos["car"]] == [3, 3] and infos["truck"][0]["group_id"] == 1 and infos["car"][1]["gt_idx"] == 2
    assert infos["truck"][0]["name"] == ["truck", "truck"] and files[os.path.join("db", "truck", "7_truck_1.bin")].shape == (2, 5)


def rows_all(pts, boxes):
    return R.extract(pts, boxes)[0]


# ---- the C surface
def test_symbols_header_build_flags_and_prototypes(L):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, bare)
        assert m, name
        assert name in lib.SIGNATURES and name in exported, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
    assert lib.SIGNATURES["fd_points_in_boxes_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.SIGNATURES["fd_gt_min_points_filter"][1][5] is ctypes.c_int  # min_points by value
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    assert "fd_points_in_boxes.hip" in build.SOURCES and build.EXTRA["fd_points_in_boxes.hip"] == build.EXTRA["fd_gt_sample.hip"]
    assert "-ffp-contract=off" in build.EXTRA["fd_points_in_boxes.hip"] and "-fno-slp-vectorize" in build.EXTRA["fd_points_in_boxes.hip"]
    assert int(_define("FD_POINTS_IN_BOXES_TILE")) == 64 and int(_define("FD_POINTS_IN_BOXES_NO_ROOM")) == hip_ops.POINTS_IN_BOXES_NO_ROOM == R.NO_ROOM
    assert int(_define("FD_RANGE_FILTER_MAX_N")) == hip_ops.POINTS_IN_BOXES_MAX_N
    src = open(os.path.join(REPO, "futuredet_amd", "csrc", "fd_points_in_boxes.hip")).read()
    assert "atomic" not in src.split("namespace {", 1)[1].lower() and "hipMalloc" not in src, "no atomics, no allocation"


def test_workspace_bytes(L):
    f = L.fd_points_in_boxes_workspace_bytes
    assert f(0, 0) == 0 and f(1000, 0) == 0
    assert f(0, 10) == 40, "the totals alone"
    assert f(1, 10) == f(256, 10) == 80 and f(257, 10) == 120
    assert f(300000, 400) == (1172 + 1) * 400 * 4
    max_rows, max_n = 1 << 28, int(_define("FD_RANGE_FILTER_MAX_N"))
    assert f(max_rows, max_n) == ((1 << 20) + 1) * max_n * 4
    assert f(-1, 10) == 0 and f(max_rows + 1, 10) == 0 and f(10, -1) == 0 and f(10, max_n + 1) == 0


def test_count_and_extract_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = [ctypes.c_void_p(0x1000000 * (i + 1)) for i in range(8)]
    odd2, odd4 = ctypes.c_void_p(0x1000002), ctypes.c_void_p(0x1000004)
    max_n, max_cols = int(_define("FD_RANGE_FILTER_MAX_N")), int(_define("FD_POINTS_IN_BOXES_MAX_COLS"))
    need = L.fd_points_in_boxes_workspace_bytes(1000, 20)

    def count(**kw):
        a = dict(points=p[0], n=1000, ndim=5, boxes=p[1], m=20, cols=12, nb=p[2], counts=p[3], ws=p[4], ws_bytes=need)
        a.update(kw)
        return L.fd_points_in_boxes_count(a["points"], a["n"], a["ndim"], a["boxes"], a["m"], a["cols"], a["nb"], a["counts"], a["ws"], a["ws_bytes"], None)

    def extract(**kw):
        a = dict(points=p[0], n=1000, ndim=5, boxes=p[1], m=20, cols=12, nb=p[2], ws=p[4], ws_bytes=need, rows=p[5], cap=500, ncols=5, offsets=p[6],
                 status=p[7])
        a.update(kw)
        return L.fd_points_in_boxes_extract(a["points"], a["n"], a["ndim"], a["boxes"], a["m"], a["cols"], a["nb"], a["ws"], a["ws_bytes"], a["rows"],
                                            a["cap"], a["ncols"], a["offsets"], a["status"], None)

    def bad(call, text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())

    for call in (count, extract):
        for ndim in (3, 6):
            bad(call, "ndim", ndim=ndim)
        bad(call, "n (", n=-1)
        bad(call, "n (", n=(1 << 28) + 1)
        bad(call, "n_boxes_max", m=-1)
        bad(call, "n_boxes_max", m=max_n + 1)
        bad(call, "box_cols", cols=6)
        bad(call, "box_cols", cols=max_cols + 1)
        bad(call, "points must be", points=None)
        bad(call, "points must be", points=odd2)
        bad(call, "boxes must be", boxes=None)
        bad(call, "boxes must be", boxes=odd2)
        bad(call, "device box count", nb=odd2)
        bad(call, "workspace holds", ws_bytes=need - 1)
        bad(call, "workspace holds", ws=None)
        bad(call, "workspace holds", ws=odd2)
    bad(count, "counts must be", counts=None)
    bad(count, "counts must be", counts=odd2)
    bad(count, "overlap", counts=ctypes.c_void_p(0x5000000 + 8))        # inside the workspace
    bad(count, "overlap", counts=ctypes.c_void_p(0x2000000 + 12 * 4))   # inside the boxes
    bad(count, "overlap", ws=ctypes.c_void_p(0x1000000 + 40))           # the workspace inside the points
    bad(extract, "ncols_out", ncols=0)
    bad(extract, "ncols_out", ncols=6)
    bad(extract, "ncols_out", ncols=5, ndim=4)
    bad(extract, "cap_rows", cap=-1)
    bad(extract, "cap_rows", cap=(1 << 28) + 1)
    bad(extract, "rows must be", rows=None)
    bad(extract, "rows must be", rows=odd2)
    bad(extract, "offsets", offsets=None)
    bad(extract, "offsets", offsets=odd4)
    bad(extract, "offsets", status=None)
    bad(extract, "offsets", status=odd2)
    bad(extract, "overlap", rows=ctypes.c_void_p(0x1000000 + 16))      # rows inside the points
    bad(extract, "overlap", offsets=ctypes.c_void_p(0x6000000 + 8))    # offsets inside rows
    bad(extract, "overlap", status=ctypes.c_void_p(0x7000000 + 16))    # status inside offsets
    bad(extract, "overlap", rows=ctypes.c_void_p(0x5000000))           # rows are the workspace
    # the empty cases are valid up to the launch (which needs a device): null arrays of no elements pass the checks
    assert count(n=0, points=None, m=0, boxes=None, counts=None, ws=None, ws_bytes=0) == 0


def test_min_points_filter_invalid_arguments_are_einval_without_a_device(L):
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(10)]
    odd4, odd2 = ctypes.c_void_p(0x100004), ctypes.c_void_p(0x100002)
    max_n = int(_define("FD_RANGE_FILTER_MAX_N"))

    def call(**kw):
        a = dict(boxes=p[0], counts=p[1], classes=p[2], traj=p[3], pc=p[9], min_points=5, boxes_out=p[4], counts_out=p[5], classes_out=p[6],
                 traj_out=p[7], status=p[8], B=2, T=3, n=5)
        a.update(kw)
        return L.fd_gt_min_points_filter(a["boxes"], a["counts"], a["classes"], a["traj"], a["pc"], a["min_points"], a["boxes_out"], a["counts_out"],
                                         a["classes_out"], a["traj_out"], a["status"], a["B"], a["T"], a["n"], None)

    def bad(text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())
        assert "fd_gt_min_points_filter" in L.fd_last_error().decode()

    bad("must be >= 1", B=0)
    bad("must be >= 1", T=0)
    bad("n_max", n=0)
    bad("n_max", n=max_n + 1)
    bad("rows, at most", B=1 << 14, T=1 << 14, n=2)
    for k in ("boxes", "counts", "classes", "boxes_out", "counts_out", "classes_out", "status"):
        bad("null", **{k: None})
    bad("needs trajectory_out", traj_out=None)
    bad("16-byte aligned", boxes=odd4)
    bad("16-byte aligned", boxes_out=odd4)
    for k in ("counts", "classes", "traj", "counts_out", "classes_out", "traj_out", "status"):
        bad("4-byte aligned", **{k: odd2})
    bad("not overlap", boxes_out=ctypes.c_void_p(0x100000 + 48))
    bad("not overlap", counts_out=ctypes.c_void_p(0x200000 + 4))
    bad("point_counts must be non-null", pc=None)
    bad("point_counts must be non-null", pc=odd2)
    bad("point_counts must not overlap", pc=p[4])                              # the boxes' output
    bad("point_counts must not overlap", pc=ctypes.c_void_p(0x700000 + 8))     # inside classes_out
    bad("point_counts must not overlap", pc=p[8])                              # the status


def test_front_end_argument_checks():
    E = hip_ops.FutureDetHipError
    with pytest.raises(E, match="HIP device"):
        hip_ops.points_in_boxes_count(torch.zeros(4, 5), torch.zeros(2, 12))
    with pytest.raises(E, match="HIP device"):
        hip_ops.points_in_boxes_extract(torch.zeros(4, 5), torch.zeros(2, 12), torch.zeros(64, dtype=torch.uint8), torch.zeros(4, 5))
    with pytest.raises(E, match="HIP device"):
        hip_ops.gt_min_points_filter(torch.zeros(1, 1, 2, 12), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1, 2), dtype=torch.int32),
                                     torch.zeros((1, 2), dtype=torch.int32), 5)


# ---- augment.py and the steps
def test_point_filter_acceptance_and_inactivity():
    from futuredet_amd.augment import GlobalAugment

    params = inspect.signature(GlobalAugment.__init__).parameters
    assert params["point_filter"].default is False and list(params)[-1] == "point_filter"
    with pytest.raises(NotImplementedError, match="min_points_in_gt"):
        GlobalAugment(dict(CFG, min_points_in_gt=5))
    with pytest.raises(NotImplementedError, match="npoints"):
        GlobalAugment(dict(CFG, min_points_in_gt=5, npoints=20000), point_filter=True)  # npoints stays refused
    assert "never uses" in GlobalAugment.__doc__
    aug = GlobalAugment(dict(CFG, min_points_in_gt=5), seed=0, point_filter=True)
    assert aug.point_filter and aug.min_points == 5
    # as in the reference, only in train mode without no_augmentation; -1 / 0 / absent mean no filter
    for cfg in (dict(CFG, min_points_in_gt=5, no_augmentation=True), dict(CFG, min_points_in_gt=5, mode="val"), dict(CFG, min_points_in_gt=-1),
                dict(CFG, min_points_in_gt=0), CFG):
        assert GlobalAugment(cfg, seed=0, point_filter=True).min_points == 0, cfg
    assert GlobalAugment(CFG, seed=0).min_points == 0 and GlobalAugment(CFG, seed=0).point_filter is False
    # the draws do not depend on the keyword
    assert np.array_equal(aug.draw(3), GlobalAugment(CFG, seed=0).draw(3))


@pytest.mark.parametrize("cls", ["StaticTrainStep", "StaticPillarsTrainStep"])
def test_steps_load_through_the_filter_only_when_it_is_active(cls):
    src = inspect.getsource(solver._StaticTrainBase._load_gt)
    assert src.index("gt_min_points_filter") < src.index("gt_sample_select") < src.index("augment_boxes"), "filter, selection, transforms"
    assert "point_filter" in inspect.getsource(solver._StaticTrainBase._init_common) and "point_filter" in getattr(solver, cls).__doc__ + solver.StaticTrainStep.__doc__


def test_exports():
    from futuredet_amd import augment

    for name in ("points_count_rbbox", "points_in_boxes", "filter_gt_by_min_points", "create_gt_database"):
        assert name in augment.__all__ and callable(getattr(augment, name))
    assert callable(augment.GTDatabase.from_samples)
    assert list(inspect.signature(augment.create_gt_database).parameters)[:6] == ["samples", "db_path", "dbinfo_path", "used_classes",
                                                                                  "num_point_features", "relative_path"]
