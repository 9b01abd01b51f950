"""Generates tests/golden/targets.npz: the reference's AssignLabel stage (det3d/datasets/pipelines/preprocess.py:336-910, NuScenesDataset
branch) run on seeded post-Preprocess annotation dicts, by IMPORTING the reference with the import shims of make_golden.py.
Run:  python tests/golden/make_golden_targets.py

The fixture holds the inputs (boxes, classes, names, trajectory labels, geometry and assigner settings as JSON) and the reference's
outputs only, plus np.__version__: numpy >= 2 promotes a python float meeting a float32 scalar to float32 (NEP 50), which makes
gaussian_radius, the radius_mult factor and mult * radius float32 computations on float32 annotations (numpy 1.x: float64).
The device kernels follow the numpy 2 rules; the Gaussian itself and limit_period's period constant are float64 / float32 either way.
A case whose reference run raised is recorded by its exception class name (``<case>/raised``).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

def geometry(W, H, osf, vs=(0.075, 0.075, 0.2), x0=-54.0, y0=-54.0):
    """Voxel geometry whose heat map is W x H at out_size_factor osf (as Voxelization writes it: float32 range / size)."""
    vs = np.asarray(vs, np.float32)
    rng = np.array([x0, y0, -5.0, x0 + W * osf * float(vs[0]), y0 + H * osf * float(vs[1]), 3.0], np.float32)
    return dict(shape=np.array([W * osf, H * osf, 40], np.int64), range=rng, size=vs)


def assigner(tasks, osf, traj=False, max_objs=500, min_radius=2):
    return dict(target_assigner=dict(tasks=[dict(num_class=len(t), class_names=list(t)) for t in tasks]), out_size_factor=osf,
                gaussian_overlap=0.1, max_objs=max_objs, min_radius=min_radius, radius_mult=traj,
                sampler_type="trajectory" if traj else "standard")


def f32_center(v, lo, vs, osf):
    return np.float32(np.float32(np.float32(v) - np.float32(lo)) / np.float32(vs)) / osf


def random_boxes(rng, n, geo, osf, dims=(1.9, 4.6, 1.7), speed=3.0):
    W, H = int(geo["shape"][0] // osf), int(geo["shape"][1] // osf)
    r, vs = geo["range"], geo["size"]
    b = np.zeros((n, 12), np.float32)
    b[:, 0] = rng.uniform(r[0] - 1.0, r[0] + (W + 0.5) * osf * vs[0], n)  # a few outside the map
    b[:, 1] = rng.uniform(r[1] - 1.0, r[1] + (H + 0.5) * osf * vs[1], n)
    b[:, 2] = rng.normal(0.0, 1.0, n)
    b[:, 3:6] = np.asarray(dims, np.float32) * rng.uniform(0.5, 1.6, (n, 3))
    b[:, 6:10] = rng.normal(0.0, speed, (n, 4))
    b[:, 10:12] = rng.uniform(-7.0, 7.0, (n, 2))  # rot outside +-pi: limit_period
    return b


def annotations(boxes, classes, names, traj):
    return dict(gt_boxes=[np.asarray(b, np.float32).reshape(-1, 12) for b in boxes], gt_classes=[np.asarray(c, np.int64) for c in classes],
                gt_names=[np.asarray(n) for n in names], gt_trajectory=[np.asarray(t) for t in traj])


def seeded_case(seed, T, tasks, geo, osf, traj=False, n=(8, 20), name="car", max_objs=500, dims=(1.9, 4.6, 1.7)):
    rng = np.random.default_rng(seed)
    nclass = sum(len(t) for t in tasks)
    boxes, classes, names, trajs = [], [], [], []
    for t in range(T):
        k = int(rng.integers(n[0], n[1] + 1))
        boxes.append(random_boxes(rng, k, geo, osf, dims))
        classes.append(rng.integers(1, nclass + 1, k))
        names.append([name] * k)
        trajs.append(list(rng.choice(["static", "linear", "nonlinear"], k)))
    return dict(cfg=assigner(tasks, osf, traj, max_objs), geo=geo, ann=annotations(boxes, classes, names, trajs))


def radius_boundary_l(ref_radius, w_cells, k, vs, osf):
    """Smallest float32 box length l whose int(gaussian_radius) reaches k (w fixed): the boundary and its neighbours are drawn."""
    lo, hi = np.float32(0.01), np.float32(100.0)
    f = lambda l: int(ref_radius((np.float32(np.float32(l / vs) / osf), w_cells), min_overlap=0.1))  # noqa: E731
    a, b = int(lo.view(np.int32)), int(hi.view(np.int32))
    while b - a > 1:
        m = (a + b) // 2
        if f(np.int32(m).view(np.float32)) >= k:
            b = m
        else:
            a = m
    return np.int32(b).view(np.float32)


def edge_case(ref_radius):
    """Hand-placed boxes on a 37 x 23 map at osf 8 (0.6 m cells): edges, w or l = 0, the radius boundary, min_radius, overlaps."""
    osf = 8
    geo = geometry(37, 23, osf)
    r, vs = geo["range"], geo["size"]
    W, H = 37, 23
    cell = float(vs[0]) * osf
    rows = []

    def box(cx, cy, w=1.9, l=4.6, h=1.7, v=(0.5, 0.2), rot=0.3, rrot=-0.2):
        x = np.float32(r[0] + cx * cell)
        y = np.float32(r[1] + cy * cell)
        rows.append([x, y, 0.1, w, l, h, v[0], v[1], 0.05, -0.03, rot, rrot])

    box(-0.5, 5.2)                    # centre column in (-1, 0): kept at column 0
    box(5.3, -0.4)                    # row in (-1, 0): kept at row 0
    box(-1.2, 6.0)                    # left of the map
    box(6.0, -1.3)                    # above the map
    box(W - 0.2, 7.5)                 # last column
    box(8.5, H - 0.3)                 # last row
    box(W + 0.3, 9.5)                 # right of the map
    box(10.5, H + 0.2)                # below the map
    box(12.5, 12.5, w=0.0)            # w = 0: skipped, slot stays zero
    box(13.5, 13.5, l=0.0)            # l = 0
    box(14.2, 10.7, w=0.3, l=0.4)     # min_radius clamp
    box(14.9, 11.1, w=0.35, l=0.5)    # overlapping the previous one, same class
    box(20.0, 4.0, rot=9.5, rrot=-12.0)   # rot outside +-pi
    box(22.0, 5.0, rot=np.pi, rrot=-np.pi)  # exactly +-pi
    box(25.0, 15.0, w=6.0, l=9.0)     # a large window clipped by nothing
    box(35.5, 21.5, w=7.0, l=7.0)     # a large window clipped at two edges
    # radius boundary: l at the smallest float32 with int(radius) = 3, one ulp below, one above
    wc = np.float32(np.float32(np.float32(3.0) / vs[0]) / osf)
    lb = radius_boundary_l(ref_radius, wc, 3, vs[1], osf)
    for j, l in enumerate((np.nextafter(lb, np.float32(0)), lb, np.nextafter(lb, np.float32(100)))):
        box(3.5 + 10 * j, 17.5, w=3.0, l=float(l))
    b0 = np.asarray(rows, np.float32)
    # a centre exactly at column W (dropped): solve in float32
    xw = np.float32(r[0] + W * cell)
    while f32_center(xw, r[0], vs[0], osf) < W:
        xw = np.nextafter(xw, np.float32(1e9))
    while f32_center(np.nextafter(xw, np.float32(-1e9)), r[0], vs[0], osf) >= W:
        xw = np.nextafter(xw, np.float32(-1e9))
    extra = b0[0].copy()
    extra[0], extra[1] = xw, np.float32(r[1] + 3.5 * cell)
    b0 = np.concatenate([b0, extra[None]], 0)
    assert f32_center(xw, r[0], vs[0], osf) == W
    assert f32_center(b0[0, 0], r[0], vs[0], osf) > -1 and f32_center(b0[0, 0], r[0], vs[0], osf) < 0
    n0 = len(b0)
    cls0 = np.ones(n0, np.int64)
    cls0[[1, 5, 9]] = 2               # a second class of the task: regrouping moves them behind the class-1 objects
    cls0[3] = 7                       # a class in no task: left out of every row
    rng = np.random.default_rng(11)
    b2 = random_boxes(rng, 9, geo, osf)
    tasks = [["car", "truck"]]
    ann = annotations([b0, np.zeros((0, 12), np.float32), b2], [cls0, np.zeros(0, np.int64), rng.integers(1, 3, 9)],
                      [["car"] * n0, [], ["car"] * 9], [["static"] * n0, [], ["linear"] * 9])
    return dict(cfg=assigner(tasks, osf, False, max_objs=40), geo=geo, ann=ann)


def cap_case():
    """Trajectory sampler with radius_mult: the factor's cap at 4 and its floor at 1, on a 40 x 30 map."""
    osf = 8
    geo = geometry(40, 30, osf)
    c = seeded_case(21, 4, [["car"]], geo, osf, traj=True, n=(6, 10))
    ann = c["ann"]
    ann["gt_boxes"][3][0, 6:8] = (30.0, 40.0)   # |v| (1 + 3) / 2 = 100: capped at 4
    ann["gt_boxes"][1][0, 6:8] = (0.0, 0.0)     # factor 0: max(1, .) = 1
    ann["gt_boxes"][2][0, 6:8] = (0.6, 0.8)     # |v| = 1: factor (1 + 2) / 2 = 1.5
    return c


def cases():
    out = {}
    out["n0_t7"] = seeded_case(1, 7, [["car"]], geometry(48, 40, 8), 8)
    out["two_task"] = seeded_case(2, 3, [["car"], ["truck", "bus"]], geometry(29, 17, 8), 8, n=(15, 30))
    out["n3dtf"] = seeded_case(3, 7, [["car"]], geometry(64, 56, 8), 8, traj=True)
    out["ped_traj"] = seeded_case(4, 7, [["pedestrian"]], geometry(54, 30, 8, vs=(0.05, 0.05, 0.2)), 8, traj=True, name="pedestrian",
                                  dims=(0.7, 0.8, 1.8))
    out["pp_n3dtf"] = seeded_case(5, 7, [["car"]], geometry(50, 44, 4, vs=(0.2, 0.2, 8.0)), 4, traj=True)
    out["grid180"] = seeded_case(6, 2, [["car"]], geometry(180, 180, 8), 8, n=(40, 60))
    out["swap_xy"] = seeded_case(7, 2, [["car"]], geometry(7, 13, 8), 8, n=(5, 9))
    out["cap4"] = cap_case()
    over = seeded_case(8, 2, [["car"]], geometry(30, 30, 8), 8, n=(12, 12), max_objs=10)
    out["over_limit"] = over
    return out


def main():
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    prep = make_golden._import_ref_pipeline("preprocess")
    from det3d.core.utils.center_utils import gaussian_radius
    import addict

    arrays = {"numpy_version": np.array(np.__version__)}
    cs = cases()
    cs["edges"] = edge_case(gaussian_radius)
    for name, c in cs.items():
        ann = c["ann"]
        T = len(ann["gt_boxes"])
        arrays[name + "/cfg"] = np.array(json.dumps(c["cfg"]))
        for k in ("shape", "range", "size"):
            arrays["%s/geo_%s" % (name, k)] = c["geo"][k]
        arrays[name + "/counts"] = np.array([len(b) for b in ann["gt_boxes"]], np.int32)
        arrays[name + "/boxes"] = np.concatenate(ann["gt_boxes"], 0).astype(np.float32)
        arrays[name + "/classes"] = np.concatenate(ann["gt_classes"]).astype(np.int32)
        arrays[name + "/names"] = np.concatenate([np.asarray(n, dtype="<U16") for n in ann["gt_names"]])
        arrays[name + "/trajectory"] = np.concatenate([np.asarray(n, dtype="<U16") for n in ann["gt_trajectory"]])
        res = dict(mode="train", type="NuScenesDataset", lidar=dict(annotations={k: [np.copy(x) for x in v] for k, v in ann.items()},
                                                                     voxels=dict(c["geo"])))
        stage = prep.AssignLabel(cfg=addict.Dict(c["cfg"]))
        try:
            res, _ = stage(res, None)
        except Exception as e:  # the over-max_objs sample: the reference's assert
            arrays[name + "/raised"] = np.array(type(e).__name__)
            print(name, "raised", type(e).__name__, e)
            continue
        tg = res["lidar"]["targets"]
        for k, v in tg.items():
            assert len(v) == T, (name, k)
            for t in range(T):
                if k.startswith("gt_boxes_and_cls"):
                    arrays["%s/out/%s/%d" % (name, k, t)] = v[t]
                else:
                    for u, a in enumerate(v[t]):
                        arrays["%s/out/%s/%d/%d" % (name, k, t, u)] = a
        print(name, "T=%d" % T, "objects", int(arrays[name + "/counts"].sum()), "keys", sorted(tg))
    make_golden.save("targets.npz", **arrays)


if __name__ == "__main__":
    main()
