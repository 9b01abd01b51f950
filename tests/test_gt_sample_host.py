"""The host side of GT-database sampling (csrc/fd_gt_sample.hip, augment.GTDatabase / GTSampler, ``GlobalAugment(sampler=...)`` and the
static steps): exported symbols and mirrors, argument checks (they come before any device work), the numpy restatement
(tests/gt_sample_ref.py) against what the reference's own sampler returned (tests/golden/gt_sample.npz: decisions exactly, rows and
points bit for bit) and against closed-form containment cases, the BatchSampler restatement against the reference's recorded index
sequences, the database reader with both prep filters, and the refusals.  CPU only."""
import ctypes
import inspect
import os
import pickle
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

import gt_sample_ref as R  # noqa: E402
from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402
from futuredet_amd.augment import GlobalAugment, GTDatabase, GTSampler, _BatchSampler, check_db_sampler_cfg  # noqa: E402

NAMES = {"fd_gt_sample_select", "fd_gt_sample_points"}
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False), class_names=["car"])
DB_ON = dict(type="GT-AUG", enable=True, db_info_path="dbinfos_train.pkl", sample_groups=[dict(car=2)],
             db_prep_steps=[dict(filter_by_min_num_points=dict(car=5)), dict(filter_by_difficulty=[-1])],
             global_random_rotation_range_per_object=[0, 0], rate=1.0)
CASES = ["chain_a", "chain_b", "groups", "angle_cols", "short_forecast", "trajectory", "full", "rate"]


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "gt_sample.npz"))


def _define(name):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    return re.search(r"#define %s (\S+)" % name, hdr).group(1)


def golden_case(golden, name, spare_rows=None):
    """(boxes [T, n_max, 12], counts [T], classes, trajectory [T, n_max], db, cand, groups, rate, point_cap) of a recorded case"""
    k = lambda s: golden["%s/%s" % (name, s)]
    gtb = k("gt_boxes")
    T, n0 = gtb.shape[:2]
    cand = k("cand")
    n_max = n0 + (len(cand) if spare_rows is None else spare_rows)
    boxes, cls, tr = np.zeros((T, n_max, 12), np.float32), np.zeros((T, n_max), np.int32), np.zeros((T, n_max), np.int32)
    boxes[:, :n0], cls[:, :n0], tr[:, :n0] = gtb, k("gt_classes"), k("gt_trajectory")
    db = dict(boxes=k("db_boxes"), steps=k("db_steps"), classes=k("db_classes"), trajectory=k("db_trajectory"), offsets=k("db_offsets"),
              points=k("db_points"))
    cap = int(sum(db["offsets"][e + 1] - db["offsets"][e] for e in cand if e >= 0))
    return boxes, np.full((T,), n0, np.int32), cls, tr, db, cand, [tuple(int(v) for v in g) for g in k("groups")], float(k("rate")), cap


# ---- the C surface
def test_symbols_header_build_flags_and_mirrors(L, tmp_path):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, bare)
        assert m, name
        assert name in lib.SIGNATURES and name in exported, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    assert "fd_gt_sample.hip" in build.SOURCES and build.EXTRA["fd_gt_sample.hip"] == build.EXTRA["fd_augment.hip"]
    assert "-ffp-contract=off" in build.EXTRA["fd_gt_sample.hip"] and "-fno-slp-vectorize" in build.EXTRA["fd_gt_sample.hip"]
    assert int(_define("FD_GT_SAMPLE_MAX_K")) == hip_ops.GT_SAMPLE_MAX_K == 64
    assert int(_define("FD_GT_SAMPLE_MAX_GROUPS")) == hip_ops.GT_SAMPLE_MAX_GROUPS == 16
    assert float(_define("FD_GT_SAMPLE_SENTINEL").rstrip("f")) == hip_ops.GT_SAMPLE_SENTINEL and np.float32(hip_ops.GT_SAMPLE_SENTINEL) == R.SENTINEL
    bits = [int(_define("FD_GT_SAMPLE_" + n)) for n in ("NO_ROW", "NO_POINTS", "COUNTS_DIFFER", "BAD_INDEX")]
    assert bits == [hip_ops.GT_SAMPLE_NO_ROW, hip_ops.GT_SAMPLE_NO_POINTS, hip_ops.GT_SAMPLE_COUNTS_DIFFER, hip_ops.GT_SAMPLE_BAD_INDEX]
    assert bits == [R.NO_ROW, R.NO_POINTS, R.COUNTS_DIFFER, R.BAD_INDEX] == [1, 2, 4, 8]
    src = tmp_path / "rec.c"
    fields = [n for n, _ in lib.GtSampleGroup._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "futuredet_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu", sizeof(fd_gt_sample_group), sizeof(fd_gt_sample_plan), offsetof(fd_gt_sample_plan, src_row), '
                   'offsetof(fd_gt_sample_plan, rows), offsetof(fd_gt_sample_plan, dst_row));\n'
                   + "".join('printf(" %%zu", offsetof(fd_gt_sample_group, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "rec")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got[0] == ctypes.sizeof(lib.GtSampleGroup) == 20 and got[1:5] == [4 * hip_ops.GT_SAMPLE_PLAN_WORDS, 0, 8, 12]
    assert got[5:] == [getattr(lib.GtSampleGroup, f).offset for f in fields] and fields == ["class_id", "trajectory", "max_num", "first", "n"]


def _groups(*rows):
    return hip_ops.gt_sample_groups(rows)


def test_select_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = [ctypes.c_void_p(0x1000000 * (i + 1)) for i in range(18)]
    odd4, odd2, odd8 = ctypes.c_void_p(0x1000004), ctypes.c_void_p(0x1000002), ctypes.c_void_p(0x1000008)
    names = ["boxes", "counts", "classes", "traj", "db_boxes", "db_steps", "db_class", "db_traj", "db_off", "cand", "boxes_out", "counts_out",
             "classes_out", "traj_out", "accepted", "plan", "n_points", "status"]
    max_n, max_t = int(_define("FD_RANGE_FILTER_MAX_N")), int(_define("FD_GT_SAMPLE_MAX_T"))
    assert max_t >= 7

    def call(**kw):
        a = dict(zip(names, p), groups=_groups((1, -1, 2, 0, 2), (2, 1, 3, 2, 3)), G=None, rate=1.0, cap=100, B=2, T=3, n=9, K=6, M=10, Tdb=3, P=50)
        a.update(kw)
        G = len(a["groups"]) if a["G"] is None else a["G"]
        return L.fd_gt_sample_select(a["boxes"], a["counts"], a["classes"], a["traj"], a["db_boxes"], a["db_steps"], a["db_class"], a["db_traj"],
                                     a["db_off"], a["M"], a["Tdb"], a["P"], a["cand"], a["groups"], G, a["rate"], a["cap"], a["boxes_out"],
                                     a["counts_out"], a["classes_out"], a["traj_out"], a["accepted"], a["plan"], a["n_points"], a["status"],
                                     a["B"], a["T"], a["n"], a["K"], None)

    def bad(text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())

    bad("B (0)", B=0)
    bad("T (0)", T=0)
    bad("T (%d)" % (max_t + 1), T=max_t + 1)
    bad("n_max", n=0)
    bad("n_max", n=max_n + 1)
    bad("rows, at most", B=1 << 20, T=64, n=max_n)
    bad("K (0)", K=0)
    bad("K (65)", K=65)
    bad("G (0)", G=0)
    bad("G (17)", G=17)
    bad("G (2)", groups=None, G=2)
    bad("M (0)", M=0)
    bad("Tdb (0)", Tdb=0)
    bad("P (-1)", P=-1)
    bad("point_cap", cap=-1)
    bad("point_cap", cap=(1 << 28) + 1)
    bad("rate", rate=-0.5)
    bad("rate", rate=float("nan"))
    bad("without overlap", groups=_groups((1, -1, 2, 0, 3), (2, -1, 3, 2, 3)))   # overlapping
    bad("without overlap", groups=_groups((1, -1, 2, 3, 3), (2, -1, 3, 0, 3)))   # out of slot order
    bad("without overlap", groups=_groups((1, -1, 2, 0, 2), (2, -1, 3, 2, 5)))   # past K
    bad("without overlap", groups=_groups((1, -1, 2, 0, -1)))
    bad("trajectory is null", traj=None, traj_out=None)
    assert call(traj=None, traj_out=None, groups=_groups((1, 0, 2, 0, 2)), K=2) == -1
    for k in names:
        if k not in ("traj", "traj_out"):
            bad("null pointer", **{k: None})
    bad("needs trajectory_out", traj_out=None)
    for k in ("boxes", "boxes_out", "db_boxes"):
        bad("16-byte aligned", **{k: odd4})
    bad("16-byte aligned", plan=odd8)
    bad("8-byte aligned", db_off=odd4)
    for k in ("counts", "classes", "traj", "counts_out", "classes_out", "traj_out", "db_steps", "db_class", "db_traj", "cand", "accepted",
              "n_points", "status"):
        bad("4-byte aligned", **{k: odd2})
    bad("not overlap", boxes_out=ctypes.c_void_p(0x1000000 + 48))
    bad("not overlap", counts_out=ctypes.c_void_p(0x2000000 + 4))
    bad("not overlap", classes_out=ctypes.c_void_p(0x3000000 + 4))
    bad("not overlap", traj_out=ctypes.c_void_p(0x4000000 + 4))
    bad("in place) or none", boxes_out=p[0])
    bad("in place) or none", boxes_out=p[0], counts_out=p[1], classes_out=p[2])


def test_points_invalid_arguments_are_einval_without_a_device(L):
    p = [ctypes.c_void_p(0x1000000 * (i + 1)) for i in range(6)]
    odd2, odd4 = ctypes.c_void_p(0x1000002), ctypes.c_void_p(0x1000004)
    names = ["db_points", "db_boxes", "cand", "accepted", "plan", "dst"]

    def call(**kw):
        a = dict(zip(names, p), P=1000, ndim=5, M=10, Tdb=3, K=6, cap=100)
        a.update(kw)
        return L.fd_gt_sample_points(a["db_points"], a["P"], a["ndim"], a["db_boxes"], a["M"], a["Tdb"], a["cand"], a["accepted"], a["plan"],
                                     a["K"], a["dst"], a["cap"], None)

    def bad(text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())

    for ndim in (3, 6, 0):
        bad("ndim", ndim=ndim)
    bad("K (0)", K=0)
    bad("K (65)", K=65)
    bad("M (0)", M=0)
    bad("Tdb (0)", Tdb=0)
    bad("P (-1)", P=-1)
    bad("point_cap", cap=-1)
    bad("point_cap", cap=(1 << 28) + 1)
    assert call(cap=0, dst=None) == 0  # a no-op
    for k in names:
        bad("null pointer", **{k: None})
    for k in ("db_points", "db_boxes", "cand", "accepted", "dst"):
        bad("misaligned", **{k: odd2})
    bad("misaligned", plan=odd4)
    bad("must not overlap", dst=ctypes.c_void_p(0x1000000 + 1000 * 5 * 4 - 4))
    bad("must not overlap", db_points=ctypes.c_void_p(0x6000000 + 100 * 5 * 4 - 4))


def test_front_end_argument_checks():
    E = hip_ops.FutureDetHipError
    db = GTDatabase.from_arrays(np.zeros((2, 1, 12), np.float32), [1, 1], [1, 1], [0, 0], np.zeros((3, 5), np.float32), [0, 1, 3], "cpu")
    with pytest.raises(E, match="HIP device"):
        hip_ops.gt_sample_select(torch.zeros(1, 1, 4, 12), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1, 4), dtype=torch.int32), db,
                                 torch.zeros((1, 2), dtype=torch.int32), [(1, -1, 2, 0, 2)], 1.0, 3)
    with pytest.raises(E, match="HIP device"):
        hip_ops.gt_sample_points(db, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 4), dtype=torch.int32),
                                 torch.zeros(3, 5), 3)
    with pytest.raises(E, match="group records"):
        hip_ops.gt_sample_groups([])
    with pytest.raises(E, match="group records"):
        hip_ops.gt_sample_groups([(1, -1, 2, 0)])
    with pytest.raises(E, match="group records"):
        hip_ops.gt_sample_groups([(1, -1, 2, 0, 1)] * 17)


# ---- the restatement against the reference
def test_golden_covers_what_the_issue_asks(golden):
    assert list(golden["names"]) == CASES and float(golden["grow"]) == 2e-3
    for name in CASES:
        acc, cand = golden["%s/accepted" % name], golden["%s/cand" % name]
        assert acc.sum() >= 1 and acc.sum() == len(golden["%s/ref_gt_boxes" % name]) and len(acc) == len(cand), name
    assert golden["short_forecast/ref_forecast_steps"].min() < golden["short_forecast/gt_boxes"].shape[0]
    g = golden["trajectory/groups"]
    assert str(golden["trajectory/sampler_type"]) != "standard" and [tuple(r[:3]) for r in g] == [(1, 0, 2), (1, 1, 4), (1, 2, 6)]
    assert float(golden["rate/rate"]) == 0.5 and float(golden["chain_a/rate"]) == 1.0
    b = golden["angle_cols/db_boxes"][golden["angle_cols/cand"][:2], 0]
    assert np.allclose(np.abs(b[:, 10] - b[:, 11]), np.pi / 2, atol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden, name):
    """decisions exactly; the appended rows (columns 0..5 of timestep 0's box, 6..11 of the recorded forecast, timestep 0's where an
    entry is short), classes, trajectories and the pasted points bit for bit"""
    boxes, counts, cls, tr, db, cand, groups, rate, cap = golden_case(golden, name)
    o = R.select_one(boxes, counts, cls, tr, db, cand, groups, rate, cap)
    k = lambda s: golden["%s/%s" % (name, s)]
    assert np.array_equal(o["accepted"], k("accepted")) and o["status"] == 0
    n0, na = int(counts[0]), int(k("accepted").sum())
    assert np.array_equal(o["counts"], counts + na)
    rb, fc, fs = k("ref_gt_boxes"), k("ref_forecast"), k("ref_forecast_steps")
    for t in range(boxes.shape[0]):
        exp = rb.copy()
        for j in range(na):  # preprocess.py:169-174
            exp[j, 6:] = fc[j, t] if t < fs[j] else fc[j, 0]
        assert np.array_equal(o["boxes"][t, n0:n0 + na].view(np.uint32), exp.view(np.uint32)), t
        assert np.array_equal(o["boxes"][t, :n0], boxes[t, :n0]) and not o["boxes"][t, n0 + na:].any()
        assert np.array_equal(o["classes"][t, n0:n0 + na], k("ref_classes")) and np.array_equal(o["trajectory"][t, n0:n0 + na], k("ref_trajectory"))
    pts, rp = R.paste(db, cand, o["accepted"], o["plan"], cap), k("ref_points")
    assert o["n_points"] == len(rp) and np.array_equal(pts[:len(rp)].view(np.uint32), rp.view(np.uint32))
    tail = pts[len(rp):]
    assert np.all(tail[:, :3] == np.float32(1e30)) and not tail[:, 3:].any()


def _quad(x, y, w, l, a=0.0):
    b = np.zeros((12,), np.float32)
    b[[0, 1, 3, 4, 10, 11]] = (x, y, w, l, a, a)
    return R.corners(b, 11)


def test_containment_and_touching_edges_in_closed_form():
    big, small = _quad(0.0, 0.0, 8.0, 8.0), _quad(0.5, -0.5, 1.0, 2.0)
    assert R.collide(big, small) and R.collide(small, big)            # no edges cross: the containment branch decides, either way round
    assert R.collide(_quad(0.0, 0.0, 8.0, 8.0, 0.3), _quad(0.5, -0.5, 1.0, 2.0, -1.1))
    left, right = _quad(0.0, 0.0, 2.0, 4.0), _quad(2.0, 0.0, 2.0, 4.0)  # sharing the edge x = 1
    assert not R.collide(left, right) and not R.collide(right, left)    # the stand-up overlap is 0, not > 0
    assert not R.collide(left, _quad(0.0, 4.0, 2.0, 4.0)) and not R.collide(left, _quad(2.0, 4.0, 2.0, 4.0))  # an edge, a corner
    assert R.collide(left, _quad(1.5, 0.5, 2.0, 4.0)) and not R.collide(left, _quad(2.5, 0.5, 2.0, 4.0))
    assert R.collide(_quad(0.0, 0.0, 3.0, 4.0), _quad(0.0, 0.0, 2.0, 2.0)) and R.collide(_quad(0.0, 0.0, 2.0, 2.0), _quad(0.0, 0.0, 3.0, 4.0))


def test_walk_order_limits_and_status_bits():
    """one group of four far-apart entries: rows and points run out exactly where the definition says"""
    M = 4
    dbb = np.zeros((M, 2, 12), np.float32)
    for e in range(M):
        dbb[e, :, :6] = (20.0 * e, 50.0, 0.0, 2.0, 4.0, 1.5)
        dbb[e, 1, 6:] = e + 1
    sizes = [5, 9, 3, 2]
    db = dict(boxes=dbb, steps=np.array([2, 1, 2, 2], np.int32), classes=np.full(M, 1, np.int32), trajectory=np.arange(M, dtype=np.int32) % 3,
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), points=np.arange(19 * 4, dtype=np.float32).reshape(19, 4))
    boxes, cls = np.zeros((2, 6, 12), np.float32), np.zeros((2, 6), np.int32)
    boxes[:, 0, :6] = (0, 0, 0, 2, 4, 1.5)
    cls[:, 0] = 1
    counts = np.array([1, 1], np.int32)
    cand, groups = np.array([0, 1, 2, 3], np.int32), [(1, -1, 5, 0, 4)]
    o = R.select_one(boxes, counts, cls, None, db, cand, groups, 1.0, 100)
    assert list(o["accepted"]) == [1, 1, 1, 1] and o["status"] == 0 and o["n_points"] == 19 and list(o["counts"]) == [5, 5]
    assert np.array_equal(o["boxes"][1, 1:5, 6], [1, 0, 3, 4])  # entry 1 has one timestep: timestep 0's columns
    assert [tuple(r) for r in o["plan"]] == [(0, 5, 0), (5, 9, 5), (14, 3, 14), (17, 2, 17)]
    o = R.select_one(boxes, counts, cls, None, db, cand, groups, 1.0, 13)  # entry 1 overflows by one point, the smaller ones fit
    assert list(o["accepted"]) == [1, 0, 1, 1] and o["status"] == R.NO_POINTS and o["n_points"] == 10
    o = R.select_one(boxes[:, :4], counts, cls[:, :4], None, db, cand, groups, 1.0, 100)  # three free rows
    assert list(o["accepted"]) == [1, 1, 1, 0] and o["status"] == R.NO_ROW
    o = R.select_one(boxes, np.array([1, 2], np.int32), cls, None, db, cand, groups, 1.0, 100)
    assert o["status"] == R.COUNTS_DIFFER and list(o["counts"]) == [5, 6] and list(o["accepted"]) == [1, 1, 1, 1]
    o = R.select_one(boxes, counts, cls, None, db, np.array([-1, 7, 2, -5], np.int32), groups, 1.0, 100)
    assert list(o["accepted"]) == [0, 0, 1, 0] and o["status"] == R.BAD_INDEX
    o = R.select_one(boxes, counts, cls, None, db, cand, [(1, -1, 3, 0, 4)], 1.0, 100)  # 3 - 1 = 2 of the four slots take part
    assert list(o["accepted"]) == [1, 1, 0, 0]
    for rate, want in ((0.5, 2), (0.25, 1), (0.125, 0), (0.375, 2)):  # 4 x rate = 2, 1, 0.5 -> 0, 1.5 -> 2: half to even
        o = R.select_one(boxes, counts, cls, None, db, cand, groups, rate, 100)
        assert int(o["accepted"].sum()) == want, rate


# ---- the host classes
class _Replay(object):
    """a Generator stand-in whose shuffles replay recorded permutations"""

    def __init__(self, perms):
        self.perms = [np.asarray(p) for p in perms]

    def shuffle(self, a):
        a[:] = self.perms.pop(0)


def test_batch_sampler_follows_the_reference_across_epoch_boundaries(golden):
    k = lambda s: golden["batch_sampler/" + s]
    bs = _BatchSampler(int(k("n")), _Replay(k("perms")))
    got = [bs.sample(int(n)) for n in k("nums")]
    assert [len(g) for g in got] == list(k("lens")) and np.array_equal(np.concatenate(got), k("seq"))
    assert list(k("lens")) != list(k("nums"))  # the record holds short draws: the last slice of an epoch
    assert not bs._rng.perms                     # every recorded reshuffle happened


def _synthetic_dbinfos(root):
    r = np.random.default_rng(3)
    infos, uid = {}, 0
    for name, sizes in (("car", [3, 5, 8, 12]), ("pedestrian", [1, 7]), ("bus", [9])):
        lst = []
        for j, n in enumerate(sizes):
            steps = 1 + (uid % 3)
            pts = r.normal(size=(n, 5)).astype(np.float32)
            rel = os.path.join("gt_db", "%d.bin" % uid)
            os.makedirs(os.path.join(root, "gt_db"), exist_ok=True)
            pts.tofile(os.path.join(root, rel))
            box = [r.normal(size=12).astype(np.float32) for _ in range(steps)]
            lst.append(dict(name=[name] * steps, trajectory=[("static", "linear", "nonlinear")[uid % 3]] * steps, path=rel, image_idx=0, gt_idx=j,
                            box3d_lidar=box, num_points_in_gt=n, difficulty=[np.int32(0)] * steps if uid != 1 else -1, group_id=uid, _pts=pts))
            uid += 1
        infos[name] = lst
    return infos


def test_database_from_dbinfos_with_both_prep_filters(tmp_path):
    root = str(tmp_path)
    infos = _synthetic_dbinfos(root)
    stripped = {k: [{kk: vv for kk, vv in i.items() if kk != "_pts"} for i in v] for k, v in infos.items()}
    pkl = os.path.join(root, "dbinfos.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(stripped, f)
    names = ["car", "pedestrian"]
    db = GTDatabase.from_dbinfos(pkl, root, names, 5, device="cpu")
    assert len(db) == 6 and db.boxes.shape == (6, 3, 12) and db.points.shape == (36, 5)  # the bus is no class of the model
    assert db.classes.tolist() == [1, 1, 1, 1, 2, 2] and db.trajectory.tolist() == [0, 1, 2, 0, 1, 2] and db.steps.tolist() == [1, 2, 3, 1, 2, 3]
    assert db.offsets.tolist() == [0, 3, 8, 16, 28, 29, 36] and db.offsets.dtype == torch.int64
    flat = infos["car"] + infos["pedestrian"]
    for e, i in enumerate(flat):
        assert np.array_equal(db.points[db.offsets[e]:db.offsets[e + 1]].numpy(), i["_pts"])
        assert np.array_equal(db.boxes[e, :len(i["box3d_lidar"])].numpy(), np.stack(i["box3d_lidar"])) and not db.boxes[e, len(i["box3d_lidar"]):].any()
    # filter_by_min_num_points drops per class; the shipped filter_by_difficulty=[-1] meets list-valued difficulties and removes nothing
    # -- only the one entry whose difficulty is the scalar -1 goes, as `info["difficulty"] not in [-1]` says
    steps = [dict(filter_by_min_num_points=dict(car=5, pedestrian=0, truck=9)), dict(filter_by_difficulty=[-1])]
    db2 = GTDatabase.from_dbinfos(stripped, root, names, 5, db_prep_steps=steps, device="cpu")
    assert db2.offsets.tolist() == [0, 8, 20, 21, 28] and db2.classes.tolist() == [1, 1, 2, 2]  # cars of 3 (too few) and 5 (scalar -1) are gone
    db3 = GTDatabase.from_dbinfos(stripped, root, names, 5, db_prep_steps=[dict(filter_by_min_num_points=dict(car=5))], device="cpu")
    assert db3.offsets.tolist() == [0, 5, 13, 25, 26, 33]
    with pytest.raises(ValueError, match="unknown database prep"):
        GTDatabase.from_dbinfos(stripped, root, names, 5, db_prep_steps=[dict(filter_by_size=1)], device="cpu")
    with pytest.raises(ValueError, match="no entry"):
        GTDatabase.from_dbinfos(stripped, root, ["truck"], 5, device="cpu")
    with pytest.raises(ValueError):
        GTDatabase.from_arrays(np.zeros((2, 1, 12)), [1, 1], [1, 1], [0, 0], np.zeros((3, 5)), [0, 1, 2], "cpu")  # offsets end short


def _db(classes, traj, sizes, names=("car", "pedestrian")):
    M = len(classes)
    return GTDatabase.from_arrays(np.zeros((M, 2, 12), np.float32), np.full(M, 2), classes, traj, np.zeros((int(np.sum(sizes)), 5), np.float32),
                                  np.concatenate([[0], np.cumsum(sizes)]), "cpu", class_names=list(names))


def test_sampler_slots_pools_and_point_cap():
    db = _db([1, 1, 1, 2, 2, 1], [0, 1, 2, 0, 0, 0], [4, 9, 2, 6, 1, 3])
    s = GTSampler(db, [dict(car=3), dict(pedestrian=2)], rate=1.0, seed=1)
    assert s.records == [(1, -1, 3, 0, 3), (2, -1, 2, 3, 2)] and s.K == 5 and s.point_cap == 3 * 9 + 2 * 6
    d = np.concatenate([s.draw(2) for _ in range(6)])
    assert d.shape == (12, 5) and d.dtype == np.int32
    assert set(d[:, :3].ravel()) <= {-1, 0, 1, 2, 5} and set(d[:, 3:].ravel()) <= {-1, 3, 4}
    assert (d == -1).any()  # short draws at the end of an epoch (pools of four and two entries, three and two per draw)
    again = np.concatenate([GTSampler(db, [dict(car=3), dict(pedestrian=2)], seed=1).draw(12)])
    assert np.array_equal(d, again)  # its own Generator: the seed decides
    s = GTSampler(db, [dict(car=7), dict(pedestrian=3)], rate=0.5, seed=0)
    assert [r[3:] for r in s.records] == [(0, 4), (4, 2)]  # round(3.5) = 4, round(1.5) = 2: half to even
    t = GTSampler(db, [dict(static_car=2), dict(linear_car=4), dict(nonlinear_car=6)], sampler_type="trajectory", seed=0, point_cap=50)
    assert t.records == [(1, 0, 2, 0, 2), (1, 1, 4, 2, 4), (1, 2, 6, 6, 6)] and t.K == 12 and t.point_cap == 50
    d = t.draw(3)
    assert set(d[:, :2].ravel()) <= {-1, 0, 5} and set(d[:, 2:6].ravel()) <= {-1, 1} and set(d[:, 6:].ravel()) <= {-1, 2}
    with pytest.raises(NotImplementedError, match="group sampling"):
        GTSampler(db, [dict(car=2, pedestrian=2)])
    with pytest.raises(ValueError, match="outside class_names"):
        GTSampler(db, [dict(truck=2)])
    with pytest.raises(ValueError, match="slots"):
        GTSampler(db, [dict(car=40), dict(pedestrian=30)])
    with pytest.raises(KeyError):
        GTSampler(db, [dict(parked_car=2)], sampler_type="trajectory")
    for text in ("always draws", "mutates a database entry"):  # the two intended differences are written down
        assert text in GTSampler.__doc__


def test_global_augment_refusals_with_and_without_a_sampler():
    sampler = GTSampler(_db([1, 1], [0, 0], [4, 4]), [dict(car=2)], seed=0)
    on = dict(CFG, db_sampler=DB_ON)
    with pytest.raises(NotImplementedError, match="db_sampler"):
        GlobalAugment(on)
    with pytest.raises(NotImplementedError, match="db_sampler"):
        GlobalAugment(dict(CFG, db_sampler=dict(type="GT-AUG")), sampler=None)
    assert inspect.signature(GlobalAugment.__init__).parameters["sampler"].default is None
    aug = GlobalAugment(on, seed=0, sampler=sampler)
    assert aug.sampler is sampler and aug.sampling
    assert GlobalAugment(CFG, sampler=sampler).sampling and GlobalAugment(CFG).sampler is None and not GlobalAugment(CFG).sampling
    assert not GlobalAugment(dict(on, no_augmentation=True), sampler=sampler).sampling  # the reference samples in its augmenting branch only
    for rot in ([-0.1, 0.1], 0.3, [0, 0.01]):
        with pytest.raises(NotImplementedError, match="per-object rotation"):
            GlobalAugment(dict(CFG, db_sampler=dict(DB_ON, global_random_rotation_range_per_object=rot)), sampler=sampler)
    for rot in ([0, 0], [], [0.2, 0.2004], None):
        GlobalAugment(dict(CFG, db_sampler=dict(DB_ON, global_random_rotation_range_per_object=rot)), sampler=sampler)
    with pytest.raises(NotImplementedError, match="group sampling"):
        GlobalAugment(dict(CFG, db_sampler=dict(DB_ON, sample_groups=[dict(car=2, truck=1)])), sampler=sampler)
    check_db_sampler_cfg(DB_ON)
    for key in ("min_points_in_gt", "npoints"):  # still out of scope, sampler or not
        with pytest.raises(NotImplementedError, match=key):
            GlobalAugment(dict(on, **{key: 5}), sampler=sampler)


@pytest.mark.parametrize("cls", ["StaticTrainStep", "StaticPillarsTrainStep"])
def test_step_refuses_a_cloud_that_cannot_grow_before_anything_changes(cls):
    class _Scheduler(object):
        stepped = 0

        def step(self, it):
            self.stepped += 1

    sampler = GTSampler(_db([1, 1], [0, 0], [4, 6]), [dict(car=2)], seed=0)
    assert sampler.point_cap == 12
    step = object.__new__(getattr(solver, cls))
    step.B, step.capacity, step.ndim, step.bev, step.scheduler = 2, 100, 5, None, _Scheduler()
    step.augment, step.gt_sample = GlobalAugment(CFG, seed=0, sampler=sampler), dict()
    batch = dict(clouds=[torch.zeros((88, 5)), torch.zeros((89, 5))])
    with pytest.raises(ValueError, match=r"89 rows \+ point_cap = 12"):
        step._load(batch, 0)
    assert step.scheduler.stepped == 0 and np.array_equal(step.augment.rng.random(3), np.random.default_rng(0).random(3))  # nothing drawn either
