"""Generates tests/golden/gt_sample.npz: ground-truth database sampling by the reference's own DataBaseSamplerV2.sample_all
(det3d/core/sampler/sample_ops.py:101-253), IMPORTED with the import shims of make_golden.py, on a synthetic database written to a
temporary directory (db_infos as det3d/datasets/utils/create_gt_database.py:146-157 builds them, one .bin per entry).  Every case uses
a fresh sampler and deep-copied infos, so no entry is used twice.  Run:  python tests/golden/make_golden_gt_sample.py

Under the shims numba.jit is the identity, so box_collision_test runs as plain Python, whose containment branch is dead code
(``np.bool_ is False``).  Cases are therefore drawn by REJECTION BEFORE RECORDING, and nothing is excluded afterwards:
  robust          a float64 separating-axis test gives the same answer for every pair the sampler can consult (a candidate, angle =
                  column 11, against a ground-truth box, angle = column 10, against a candidate of its own group, column 11, and against
                  one of an earlier group, column 10) with both boxes grown by 2 mm and with both shrunk by 2 mm;
  no containment  in no such pair do all four corners of one box lie inside the other grown by 2 mm.
The generator asserts what each case is for:
  chain_a         candidate 0 collides only with candidate 1 and candidate 1 with a ground-truth box: both rejected
  chain_b         candidate 0 collides only with an otherwise free candidate 1: 0 rejected, 1 accepted
  groups          a group-2 candidate overlaps a REJECTED group-1 candidate and a not yet drawn group-3 candidate and is accepted;
                  another overlaps an ACCEPTED group-1 box and is rejected; the group-3 candidate then meets the accepted group-2 box
  angle_cols      columns 10 and 11 differ by 90 degrees and every decision flips with the column read
  short_forecast  entries with fewer timesteps than T
  trajectory      a non-standard sampler_type with the typed groups static_car=2, linear_car=4, nonlinear_car=6
  full            a class at its max_num and one above it: nothing of them is drawn
  rate            0.5 with odd differences: round half to even decides
and that every case has an accepted and a rejected candidate.  Also recorded: the index sequences of the reference's BatchSampler across
an epoch boundary, with the permutations its shuffles produced.

The fixture holds, per case: the ground truth (boxes [T, n0, 12], class and trajectory ids), the database as arrays (boxes
[M, Tdb, 12], steps, classes, trajectory, offsets, points), the groups, the rate, the drawn slots ``cand`` (a group's slots hold its
draw in order; the slots the reference did not draw are filled with other entries, which must stay unused), and what sample_all
returned: the accepted slots, gt_boxes, gt_forecast (padded to Tdb), points, names and trajectories as ids."""
import copy
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

GROW = 2e-3
CLASS_NAMES = ["car", "pedestrian", "truck"]
TRAJ = ("static", "linear", "nonlinear")
NDIM = 5
TDB = 3
T = 3


class _Log(object):
    def info(self, *a, **k):
        pass


# ---------------------------------------------------------------------------------------------------------------- float64 geometry
def quad64(box, col, grow=0.0):
    w, l, a = float(box[3]) + 2 * grow, float(box[4]) + 2 * grow, float(box[col])
    s, c = np.sin(a), np.cos(a)
    return np.array([(w * nx * c + l * ny * s + float(box[0]), -(w * nx) * s + l * ny * c + float(box[1]))
                     for nx, ny in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))])


def sat(p, q):
    """float64 separating-axis test of two convex quadrilaterals: True = they overlap"""
    for poly in (p, q):
        for k in range(4):
            e = poly[(k + 1) % 4] - poly[k]
            axis = np.array([-e[1], e[0]])
            a, b = p @ axis, q @ axis
            if a.max() <= b.min() or b.max() <= a.min():
                return False
    return True


def inside_all(p, q):
    """all corners of q inside the convex quadrilateral p (either orientation)"""
    signs = []
    for k in range(4):
        e = p[(k + 1) % 4] - p[k]
        signs.append([e[0] * (c[1] - p[k][1]) - e[1] * (c[0] - p[k][0]) for c in q])
    s = np.array(signs)
    return bool(np.all(s < 0) or np.all(s > 0))


def pair(bp, cp, bq, cq):
    """(overlap, robust, contained) of box bp read with column cp against bq read with cq"""
    big, small = sat(quad64(bp, cp, GROW), quad64(bq, cq, GROW)), sat(quad64(bp, cp, -GROW), quad64(bq, cq, -GROW))
    contained = inside_all(quad64(bp, cp, GROW), quad64(bq, cq)) or inside_all(quad64(bq, cq, GROW), quad64(bp, cp))
    return sat(quad64(bp, cp), quad64(bq, cq)), big == small, contained


# ---------------------------------------------------------------------------------------------------------------- building blocks
def box(x, y, w=2.0, l=4.5, a10=0.0, a11=None, z=-1.0, h=1.6, vel=(0.0, 0.0, 0.0, 0.0)):
    b = np.zeros((12,), np.float32)
    b[:6] = (x, y, z, w, l, h)
    b[6:10] = vel
    b[10] = a10
    b[11] = a10 if a11 is None else a11
    return b


def entry(r, name, traj, b, steps=TDB):
    """one database entry in draw order: its box at every timestep (moving on), its points object-centred"""
    rows = []
    for t in range(steps):
        nb = b.copy()
        nb[0:2] += np.float32(0.7 * t) * r.normal(0.0, 1.0, 2).astype(np.float32)
        nb[6:10] = r.normal(0.0, 2.0, 4)
        nb[10:12] += np.float32(0.1 * t)
        rows.append(nb if t else b.copy())
    n = int(r.integers(5, 40))
    pts = np.zeros((n, NDIM), np.float32)
    pts[:, 0:3] = r.uniform(-0.5, 0.5, (n, 3)) * b[3:6]
    pts[:, 3] = r.uniform(0, 255, n)
    pts[:, 4] = r.integers(0, 10, n) * 0.05
    return dict(name=name, traj=traj, rows=rows, points=pts)


def jitter(r, b, pos=0.03, ang=0.02):
    b = b.copy()
    b[0:2] += r.uniform(-pos, pos, 2).astype(np.float32)
    b[10:12] += np.float32(r.uniform(-ang, ang))
    return b


def far(r, k):
    """a free spot: far from everything a case places near the origin and from the other free spots"""
    return 40.0 + 12.0 * k + r.uniform(-1, 1), -40.0 + r.uniform(-1, 1)


# ---------------------------------------------------------------------------------------------------------------- one case through the reference
def run_case(sample_ops, root, case, seed):
    """case: gt (list of (name, traj, box rows [T])), pools {class: [entries in DRAW order]}, groups [(key, max_num)], rate, sampler_type.
    Returns the arrays of the fixture, or None when the case is not robust."""
    gt, pools, groups, rate, stype = case["gt"], case["pools"], case["groups"], case["rate"], case["sampler_type"]
    # the pools in the list order that makes the sampler's shuffle produce the intended draw order
    np.random.seed(seed)
    db_infos, uid_of, flat = {}, {}, []
    for name, entries in pools.items():
        idx = np.arange(len(entries))
        np.random.shuffle(idx)  # BatchSampler.__init__
        infos = [None] * len(entries)
        for draw_pos, e in enumerate(entries):
            infos[idx[draw_pos]] = e
        db_infos[name] = infos
    for name, infos in db_infos.items():
        for e in infos:
            e["uid"] = len(flat)
            flat.append(e)
    ref_infos = {}
    for name, infos in db_infos.items():
        lst = []
        for e in infos:
            rel = os.path.join("db", "%d.bin" % e["uid"])
            os.makedirs(os.path.join(root, "db"), exist_ok=True)
            e["points"].tofile(os.path.join(root, rel))
            lst.append({"name": [e["name"]] * len(e["rows"]), "trajectory": [e["traj"]] * len(e["rows"]), "path": rel, "image_idx": 0,
                        "gt_idx": e["uid"], "box3d_lidar": [r.copy() for r in e["rows"]], "num_points_in_gt": len(e["points"]),
                        "difficulty": [np.int32(0)] * len(e["rows"]), "group_id": e["uid"], "uid": e["uid"]})
        ref_infos[name] = lst
    np.random.seed(seed)
    sampler = sample_ops.DataBaseSamplerV2(copy.deepcopy(ref_infos), [dict([g]) for g in groups], None, rate, [0, 0], logger=_Log())
    drawn = []  # per sample_class_v2 call: the entries it kept, in order
    orig = sampler.sample_class_v2

    def recording(name, num, gt_boxes, sampler_type):
        want = name.split("_")[0] if sampler_type != "standard" else None
        pool = sampler._sampler_dict.get(name.split("_")[-1] if want else name)
        got = []
        if pool is not None:
            inner = pool.sample

            def sample(n):
                out = inner(n)
                got.extend(o["uid"] for o in out if want is None or o["trajectory"][0] == want)
                return out
            pool.sample = sample
        try:
            return orig(name, num, gt_boxes, sampler_type)
        finally:
            if pool is not None:
                del pool.sample
            drawn.append((name, [int(u) for u in got]))
    sampler.sample_class_v2 = recording
    gt0 = np.stack([g[2][0] for g in gt]) if gt else np.zeros((0, 12), np.float32)
    names = np.array([g[0] for g in gt])
    trajs = np.array([g[1] for g in gt])
    ret = sampler.sample_all(root, gt0.copy(), names, trajs, NDIM, False, gt_group_ids=None, calib=None, road_planes=None, sampler_type=stype)

    # the slots
    K_g = [max(0, int(np.round(rate * m))) for _, m in groups]
    first = np.concatenate([[0], np.cumsum(K_g)]).astype(int)
    cand = np.full((int(first[-1]),), -1, np.int32)
    by_group = dict(drawn)
    assert len(by_group) == len(drawn)
    fill = np.random.default_rng(seed)
    records = []
    for g, (key, max_num) in enumerate(groups):
        cls = key.split("_")[-1]
        tr = TRAJ.index(key.split("_")[0]) if stype != "standard" else -1
        records.append((CLASS_NAMES.index(cls) + 1, tr, max_num, first[g], K_g[g]))
        got = by_group.get(key, [])
        assert len(got) <= K_g[g]
        cand[first[g]:first[g] + len(got)] = got
        others = [e["uid"] for e in db_infos.get(cls, []) if e["uid"] not in got]
        for i in range(first[g] + len(got), first[g] + K_g[g]):  # never looked at
            cand[i] = others[int(fill.integers(0, len(others)))] if others and fill.random() < 0.7 else -1

    # robustness of every pair the sampler can consult
    group_of = np.concatenate([np.full(k, g) for g, k in enumerate(K_g)]) if len(cand) else np.zeros((0,), int)
    used = [i for g in range(len(groups)) for i in range(first[g], first[g] + len(by_group.get(groups[g][0], [])))]
    overlaps = {}
    for i in used:
        bi = flat[cand[i]]["rows"][0]
        pairs = [(("gt", j), gt0[j], 10) for j in range(len(gt0))]
        pairs += [(("slot", j), flat[cand[j]]["rows"][0], 11 if group_of[j] == group_of[i] else 10) for j in used
                  if j != i and group_of[j] <= group_of[i]]
        for key, bq, cq in pairs:
            hit, robust, contained = pair(bi, 11, bq, cq)
            if not robust or contained:
                return None
            overlaps[(i,) + key] = hit

    # what the reference returned
    M = len(flat)
    acc = np.zeros((len(cand),), np.int32)
    out = dict(cand=cand, groups=np.array(records, np.int32), rate=np.float64(rate))
    if ret is not None:
        ref_pts = ret["points"]
        sizes, slots = [], []
        at = 0
        # the accepted entries, identified by their points (every entry's points are unique) in the order of the result
        for b in ret["gt_boxes"]:
            match = [i for i in used if not acc[i] and np.array_equal(flat[cand[i]]["rows"][0][:6], b[:6])]
            assert len(match) >= 1
            i = match[0]
            n = len(flat[cand[i]]["points"])
            assert np.array_equal(ref_pts[at:at + n, 3:], flat[cand[i]]["points"][:, 3:])
            at += n
            acc[i] = 1
            slots.append(i)
        assert at == len(ref_pts) and slots == sorted(slots)
        fc = np.zeros((len(slots), TDB, 6), np.float32)
        fsteps = np.zeros((len(slots),), np.int32)
        for k, f in enumerate(ret["gt_forecast"]):
            fsteps[k] = len(f)
            fc[k, :len(f)] = np.stack(f)
        out.update(ref_gt_boxes=np.asarray(ret["gt_boxes"], np.float32).copy(), ref_forecast=fc, ref_forecast_steps=fsteps,
                   ref_points=np.asarray(ref_pts, np.float32), ref_classes=np.array([CLASS_NAMES.index(n) + 1 for n in ret["gt_names"]], np.int32),
                   ref_trajectory=np.array([TRAJ.index(t) for t in ret["gt_trajectory"]], np.int32))
    else:
        out.update(ref_gt_boxes=np.zeros((0, 12), np.float32), ref_forecast=np.zeros((0, TDB, 6), np.float32),
                   ref_forecast_steps=np.zeros((0,), np.int32), ref_points=np.zeros((0, NDIM), np.float32),
                   ref_classes=np.zeros((0,), np.int32), ref_trajectory=np.zeros((0,), np.int32))
    out["accepted"] = acc
    # ground truth and database as arrays
    n0 = len(gt)
    gtb = np.zeros((T, n0, 12), np.float32)
    for j, g in enumerate(gt):
        gtb[:, j] = np.stack(g[2])
    out["gt_boxes"] = gtb
    out["gt_classes"] = np.array([CLASS_NAMES.index(g[0]) + 1 for g in gt], np.int32)
    out["gt_trajectory"] = np.array([TRAJ.index(g[1]) for g in gt], np.int32)
    dbb = np.zeros((M, TDB, 12), np.float32)
    for e in flat:
        dbb[e["uid"], :len(e["rows"])] = np.stack(e["rows"])
    out["db_boxes"] = dbb
    out["db_steps"] = np.array([len(e["rows"]) for e in flat], np.int32)
    out["db_classes"] = np.array([CLASS_NAMES.index(e["name"]) + 1 for e in flat], np.int32)
    out["db_trajectory"] = np.array([TRAJ.index(e["traj"]) for e in flat], np.int32)
    out["db_offsets"] = np.concatenate([[0], np.cumsum([len(e["points"]) for e in flat])]).astype(np.int64)
    out["db_points"] = np.concatenate([e["points"] for e in flat])
    out["sampler_type"] = np.array(stype)
    return out, dict(used=used, overlaps=overlaps, acc=acc, first=first, drawn=by_group)


def gt_obj(r, name, traj, b):
    rows = [b.copy()]
    for t in range(1, T):
        nb = b.copy()
        nb[0:2] += r.normal(0.0, 1.5 * t, 2).astype(np.float32)
        nb[10:12] += np.float32(0.1 * t)
        rows.append(nb)
    return (name, traj, rows)


def spare(r, name, n, k0=20):
    """pool entries that are never drawn first: they sit behind the designed ones in draw order"""
    return [entry(r, name, TRAJ[int(r.integers(0, 3))], box(*far(r, k0 + k))) for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------- the cases
def case_chain(r, variant):
    gt = [gt_obj(r, "car", "static", jitter(r, box(0.0, 0.0))), gt_obj(r, "car", "linear", jitter(r, box(-30.0, 25.0, a10=0.6)))]
    if variant == "a":   # 0 meets only 1, 1 meets the ground truth
        c0, c1 = box(3.0, 0.0), box(1.5, 0.3)
    else:                # 0 meets only 1, 1 is free otherwise
        c0, c1 = box(13.0, 0.0), box(14.5, 0.3)
    pool = [entry(r, "car", "static", jitter(r, c0)), entry(r, "car", "linear", jitter(r, c1)), entry(r, "car", "static", jitter(r, box(*far(r, 0)))),
            entry(r, "car", "nonlinear", jitter(r, box(-1.2, 0.5, a10=0.3)))] + spare(r, "car", 4)
    return dict(gt=gt, pools={"car": pool}, groups=[("car", 6)], rate=1.0, sampler_type="standard")


def check_chain(variant):
    def check(info):
        ov, acc, u = info["overlaps"], info["acc"], info["used"]
        assert len(u) == 4
        assert ov[(0, "slot", 1)] and not any(v for k, v in ov.items() if k[0] == 0 and k[1:] != ("slot", 1))
        if variant == "a":
            assert ov[(1, "gt", 0)] and acc[0] == 0 and acc[1] == 0
        else:
            assert not any(v for k, v in ov.items() if k[0] == 1 and k[1:] != ("slot", 0)) and acc[0] == 0 and acc[1] == 1
        assert acc[2] == 1 and acc[3] == 0
    return check


def case_groups(r):
    gt = [gt_obj(r, "car", "static", jitter(r, box(0.0, 0.0))), gt_obj(r, "pedestrian", "linear", jitter(r, box(-20.0, 0.0, 0.7, 0.7)))]
    cars = [entry(r, "car", "static", jitter(r, box(10.0, 10.0))),           # A: free, accepted
            entry(r, "car", "static", jitter(r, box(1.4, 0.4)))]             # R: meets the ground truth, rejected
    peds = [entry(r, "pedestrian", "static", jitter(r, box(2.6, 0.0, 0.8, 0.8))),     # P1: meets R (rejected) and Q (group 3): accepted
            entry(r, "pedestrian", "linear", jitter(r, box(11.1, 10.0, 0.8, 0.8)))]   # P2: meets A (accepted): rejected
    trucks = [entry(r, "truck", "static", jitter(r, box(4.2, 0.0, 2.8, 7.0))),        # Q: meets P1 (now a ground-truth row): rejected
              entry(r, "truck", "static", jitter(r, box(*far(r, 1)), 0.0, 0.0))]      # free: accepted
    return dict(gt=gt, pools={"car": cars + spare(r, "car", 3), "pedestrian": peds + spare(r, "pedestrian", 3),
                              "truck": trucks + spare(r, "truck", 3)},
                groups=[("car", 3), ("pedestrian", 3), ("truck", 2)], rate=1.0, sampler_type="standard")


def check_groups(info):
    ov, acc, f = info["overlaps"], info["acc"], info["first"]
    A, R, P1, P2, Q, Q2 = f[0], f[0] + 1, f[1], f[1] + 1, f[2], f[2] + 1
    assert info["used"] == [A, R, P1, P2, Q, Q2]
    assert ov[(R, "gt", 0)] and acc[A] == 1 and acc[R] == 0
    assert ov[(P1, "slot", R)] and ov[(Q, "slot", P1)] and acc[P1] == 1
    assert ov[(P2, "slot", A)] and acc[P2] == 0
    assert acc[Q] == 0 and acc[Q2] == 1


def case_angle_cols(r):
    hp = np.pi / 2
    gt = [gt_obj(r, "car", "static", jitter(r, box(0.0, 0.0, 1.0, 6.0, a10=0.0, a11=hp), ang=0.0)),     # column 10: long in y
          gt_obj(r, "car", "static", jitter(r, box(2.5, 30.0, 1.0, 6.0, a10=0.0, a11=0.0), ang=0.0))]
    cars = [entry(r, "car", "static", jitter(r, box(2.5, 0.0, 1.0, 6.0, a10=hp, a11=0.0), ang=0.0)),    # c: free of GT 0 read by column 10
            entry(r, "car", "static", jitter(r, box(0.0, 30.0, 1.0, 6.0, a10=0.0, a11=hp), ang=0.0))]   # d: column 11 lays it across GT 1
    peds = [entry(r, "pedestrian", "static", jitter(r, box(5.4, 0.4, 1.0, 1.0), ang=0.0)),              # e: meets c read by column 10
            entry(r, "pedestrian", "static", jitter(r, box(2.5, 2.0, 0.6, 0.6), ang=0.0))]              # f: inside c read by column 11 only
    return dict(gt=gt, pools={"car": cars + spare(r, "car", 3), "pedestrian": peds + spare(r, "pedestrian", 3)},
                groups=[("car", 4), ("pedestrian", 2)], rate=1.0, sampler_type="standard")


def check_angle_cols(case):
    def check(info):
        acc, f = info["acc"], info["first"]
        c, d, e, fslot = f[0], f[0] + 1, f[1], f[1] + 1
        assert info["used"] == [c, d, e, fslot]
        assert acc[c] == 1 and acc[d] == 0 and acc[e] == 0 and acc[fslot] == 1
        gt0, gt1 = case["gt"][0][2][0], case["gt"][1][2][0]
        bc, bd = case["pools"]["car"][0]["rows"][0], case["pools"]["car"][1]["rows"][0]
        be, bf = case["pools"]["pedestrian"][0]["rows"][0], case["pools"]["pedestrian"][1]["rows"][0]
        # every decision flips with the column
        assert not pair(bc, 11, gt0, 10)[0] and pair(bc, 11, gt0, 11)[0]      # the obstacle's column
        assert pair(bd, 11, gt1, 10)[0] and not pair(bd, 10, gt1, 10)[0]      # the candidate's column
        assert pair(be, 11, bc, 10)[0] and not pair(be, 11, bc, 11)[0]        # an accepted box of an earlier group is an obstacle
        assert not pair(bf, 11, bc, 10)[0] and sat(quad64(bf, 11), quad64(bc, 11))
    return check


def case_short_forecast(r):
    gt = [gt_obj(r, "car", "static", jitter(r, box(0.0, 0.0)))]
    cars = [entry(r, "car", "static", jitter(r, box(*far(r, 0))), steps=1), entry(r, "car", "linear", jitter(r, box(1.5, 0.2)), steps=2),
            entry(r, "car", "linear", jitter(r, box(*far(r, 1))), steps=2), entry(r, "car", "nonlinear", jitter(r, box(*far(r, 2))), steps=3)]
    return dict(gt=gt, pools={"car": cars + spare(r, "car", 3)}, groups=[("car", 5)], rate=1.0, sampler_type="standard")


def check_short_forecast(info):
    assert list(info["acc"][:4]) == [1, 0, 1, 1]


def case_trajectory(r):
    gt = [gt_obj(r, "car", TRAJ[k % 3], jitter(r, box(r.uniform(-30, 30), r.uniform(-30, 30), a10=r.uniform(-3, 3)))) for k in range(3)]
    cars = []
    for k in range(40):
        near = gt[int(r.integers(0, len(gt)))][2][0]
        at = (near[0] + r.uniform(-3, 3), near[1] + r.uniform(-3, 3)) if r.random() < 0.3 else (r.uniform(-45, 45), r.uniform(-45, 45))
        cars.append(entry(r, "car", TRAJ[int(r.integers(0, 3))], box(at[0], at[1], a10=r.uniform(-3, 3), a11=r.uniform(-3, 3))))
    return dict(gt=gt, pools={"car": cars}, groups=[("static_car", 2), ("linear_car", 4), ("nonlinear_car", 6)], rate=1.0,
                sampler_type="trajectory")


def check_trajectory(info):
    d = info["drawn"]
    assert all(len(d.get(k, [])) >= 1 for k in ("static_car", "linear_car", "nonlinear_car"))
    assert sum(len(v) for v in d.values()) >= 8


def case_full(r):
    gt = [gt_obj(r, "car", "static", jitter(r, box(6.0 * k, 0.0))) for k in range(3)]
    gt += [gt_obj(r, "truck", "static", jitter(r, box(6.0 * k, 20.0, 2.8, 7.0))) for k in range(3)]
    peds = [entry(r, "pedestrian", "static", jitter(r, box(1.1, 1.0, 0.8, 0.8))), entry(r, "pedestrian", "static", jitter(r, box(*far(r, 0), 0.8, 0.8)))]
    return dict(gt=gt, pools={"car": spare(r, "car", 4), "pedestrian": peds + spare(r, "pedestrian", 3), "truck": spare(r, "truck", 4)},
                groups=[("car", 3), ("pedestrian", 2), ("truck", 2)], rate=1.0, sampler_type="standard")


def check_full(info):
    assert "car" not in info["drawn"] and "truck" not in info["drawn"] and len(info["drawn"]["pedestrian"]) == 2
    assert list(info["acc"][info["first"][1]:info["first"][2]]) == [0, 1]


def case_rate(r):
    gt = [gt_obj(r, "car", "static", jitter(r, box(0.0, 0.0))), gt_obj(r, "car", "static", jitter(r, box(-30.0, -30.0)))]
    cars = [entry(r, "car", "static", jitter(r, box(1.5, 0.2))), entry(r, "car", "static", jitter(r, box(*far(r, 0)))),
            entry(r, "car", "static", jitter(r, box(*far(r, 1))))]
    peds = [entry(r, "pedestrian", "static", jitter(r, box(*far(r, 2), 0.8, 0.8))), entry(r, "pedestrian", "static", jitter(r, box(*far(r, 3), 0.8, 0.8)))]
    # car: 0.5 (7 - 2) = 2.5 -> 2;  pedestrian: 0.5 (3 - 0) = 1.5 -> 2
    return dict(gt=gt, pools={"car": cars + spare(r, "car", 4), "pedestrian": peds + spare(r, "pedestrian", 3)},
                groups=[("car", 7), ("pedestrian", 3)], rate=0.5, sampler_type="standard")


def check_rate(info):
    assert len(info["drawn"]["car"]) == 2 and len(info["drawn"]["pedestrian"]) == 2
    assert info["first"][1] == 4 and info["first"][2] == 6  # K_g = round(3.5) = 4, round(1.5) = 2
    assert list(info["acc"][:2]) == [0, 1]


def batch_sampler_record(prep):
    """the reference's BatchSampler over 11 entries, drawn across two epoch boundaries"""
    np.random.seed(7)
    bs = prep.BatchSampler(list(range(11)), "x")
    perms, seqs, nums = [bs._indices.copy()], [], [3, 4, 2, 5, 1, 6, 4, 11, 3]
    for n in nums:
        before = bs._idx
        got = np.asarray(bs.sample(n), np.int64)
        if bs._idx == 0 and (before + n >= 11):
            perms.append(bs._indices.copy())
        seqs.append(got)
    flat = np.concatenate(seqs)
    return dict(n=np.int64(11), nums=np.array(nums, np.int64), perms=np.stack(perms), lens=np.array([len(s) for s in seqs], np.int64), seq=flat)


def main():
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    from det3d.core.sampler import preprocess as prep
    from det3d.core.sampler import sample_ops

    makers = [("chain_a", lambda r: case_chain(r, "a"), lambda c: check_chain("a")), ("chain_b", lambda r: case_chain(r, "b"), lambda c: check_chain("b")),
              ("groups", case_groups, lambda c: check_groups), ("angle_cols", case_angle_cols, check_angle_cols),
              ("short_forecast", case_short_forecast, lambda c: check_short_forecast), ("trajectory", case_trajectory, lambda c: check_trajectory),
              ("full", case_full, lambda c: check_full), ("rate", case_rate, lambda c: check_rate)]
    arrays = {"numpy_version": np.array(np.__version__), "names": np.array([m[0] for m in makers]), "grow": np.float64(GROW),
              "class_names": np.array(CLASS_NAMES), "trajectory_names": np.array(TRAJ)}
    r = np.random.default_rng(2025)
    for name, make, checker in makers:
        for attempt in range(200):
            case = make(r)
            with tempfile.TemporaryDirectory() as root:
                res = run_case(sample_ops, root, case, seed=100 + attempt)
            if res is None:
                continue
            out, info = res
            try:
                checker(case)(info)
                assert out["accepted"].sum() >= 1 and any(out["accepted"][i] == 0 for i in info["used"])
            except AssertionError:
                if name == "trajectory":  # a random scene: drawn again until it shows what it is for
                    continue
                raise
            break
        else:
            raise RuntimeError("no robust draw of case " + name)
        print(name, "attempt", attempt, "slots", len(out["cand"]), "used", len(info["used"]), "accepted", int(out["accepted"].sum()),
              "points", len(out["ref_points"]))
        for k, v in out.items():
            arrays["%s/%s" % (name, k)] = v
    for k, v in batch_sampler_record(prep).items():
        arrays["batch_sampler/" + k] = v
    make_golden.save("gt_sample.npz", **arrays)


if __name__ == "__main__":
    main()
