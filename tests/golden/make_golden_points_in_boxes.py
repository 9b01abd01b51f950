"""Generates tests/golden/points_in_boxes.npz: the outputs of the reference's own box_np_ops.points_in_rbbox and points_count_rbbox
(det3d/core/bbox/box_np_ops.py:641-647, 15-20) on synthetic clouds and boxes.  The reference runs under make_golden.py's shims (numba.njit is
the identity, so the jitted loops run as plain Python); geometry.py and box_np_ops.py are loaded by path, the rest of the det3d package is
not imported.  Run:  python tests/golden/make_golden_points_in_boxes.py

Cases: 12- and 7-column boxes x 4- and 5-column points; in the 12-column cases column 10 differs from column 11 (the reference reads the
LAST column).  Cases are drawn by REJECTION BEFORE RECORDING, and nothing is excluded afterwards: a point (as the fp32 values that are
recorded) is drawn again until its float64 distance to every face plane of every box is at least MARGIN = 1e-3 m -- two orders above
fp32 rounding error at +-60 m -- so NumPy's fp32 sin / cos and the rounding of its einsum cannot change a decision, and a restatement
that rounds differently must still give the recorded answers exactly.  The generator asserts that every case has points inside and
outside every box, points inside two boxes, and that reading column 10 would change decisions.

Per case the fixture holds ``points`` [n, ndim] fp32, ``boxes`` [m, cols] fp32, ``mask`` [n, m] bool (points_in_rbbox) and ``counts`` [m]
int64 (points_count_rbbox)."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

MARGIN = 1e-3
N_POINTS, N_BOXES = 1200, 8
CORNERS = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)], np.float64)
FACES = ((0, 1, 2), (7, 6, 5), (0, 3, 7), (1, 5, 6), (0, 4, 5), (3, 2, 6))


def load_reference():
    make_golden.install_shims()
    for name in ("det3d", "det3d.core", "det3d.core.bbox"):
        sys.modules.setdefault(name, types.ModuleType(name))
    mods = {}
    for name in ("geometry", "box_np_ops"):
        full = "det3d.core.bbox." + name
        spec = importlib.util.spec_from_file_location(full, os.path.join(make_golden.REF, "det3d", "core", "bbox", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[full] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["box_np_ops"]


def planes64(boxes, angle_col=-1):
    """unit normals [m, 6, 3] and offsets [m, 6] of the face planes, in float64 from the recorded fp32 values"""
    b = boxes.astype(np.float64)
    a = b[:, angle_col]
    s, c = np.sin(a)[:, None], np.cos(a)[:, None]
    o = b[:, None, 3:6] * (CORNERS[None] - 0.5)
    P = np.stack([o[:, :, 0] * c + o[:, :, 1] * s + b[:, None, 0], -o[:, :, 0] * s + o[:, :, 1] * c + b[:, None, 1], o[:, :, 2] + b[:, None, 2]], axis=2)
    n = np.stack([np.cross(P[:, i0] - P[:, i1], P[:, i1] - P[:, i2]) for i0, i1, i2 in FACES], axis=1)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    d = -np.stack([(n[:, f] * P[:, FACES[f][0]]).sum(axis=1) for f in range(6)], axis=1)
    return n, d


def distances(points, boxes, angle_col=-1):
    n, d = planes64(boxes, angle_col)
    return np.einsum("pk,mfk->pmf", points[:, :3].astype(np.float64), n) + d[None]  # signed: negative = the inner side


def draw_boxes(r, cols):
    b = np.zeros((N_BOXES, cols), np.float32)
    b[:, 0:2] = r.uniform(-55, 55, (N_BOXES, 2))
    b[:, 2] = r.uniform(-3, 1, N_BOXES)
    b[:, 3:6] = r.uniform([0.5, 0.6, 0.8], [3.0, 9.0, 3.5], (N_BOXES, 3))
    b[:, 6:] = r.normal(0, 2, (N_BOXES, cols - 6))
    b[:, -1] = r.uniform(-np.pi, np.pi, N_BOXES)
    if cols == 12:
        b[:, 10] = b[:, 11] + r.uniform(0.4, 1.2, N_BOXES).astype(np.float32)
    b[1] = b[0]  # two overlapping boxes: points inside both
    b[1, 0:2] += np.float32(0.4)
    b[1, -1] += np.float32(0.3)
    return b


def draw_point(r, boxes, ndim):
    p = np.zeros((ndim,), np.float32)
    j = int(r.integers(0, len(boxes)))
    kind = r.random()
    if kind < 0.75:  # around a box, in its own frame: inside and just outside
        u = r.uniform(-0.75, 0.75, 3) * boxes[j, 3:6]
        a = float(boxes[j, -1])
        p[0] = u[0] * np.cos(a) + u[1] * np.sin(a) + boxes[j, 0]
        p[1] = -u[0] * np.sin(a) + u[1] * np.cos(a) + boxes[j, 1]
        p[2] = u[2] + boxes[j, 2]
    else:
        p[0:2], p[2] = r.uniform(-60, 60, 2), r.uniform(-5, 3)
    p[3] = r.uniform(0, 255)
    if ndim == 5:
        p[4] = r.integers(0, 10) * 0.05
    return p


def make_case(r, ops, cols, ndim):
    boxes = draw_boxes(r, cols)
    points = np.zeros((N_POINTS, ndim), np.float32)
    redrawn = 0
    for i in range(N_POINTS):
        while True:
            p = draw_point(r, boxes, ndim)
            if np.abs(distances(p[None], boxes)).min() >= MARGIN:
                break
            redrawn += 1
        points[i] = p
    mask = ops.points_in_rbbox(points, boxes)
    counts = ops.points_count_rbbox(points, boxes)
    assert mask.shape == (N_POINTS, N_BOXES) and mask.dtype == np.bool_ and np.array_equal(mask.sum(axis=0), counts)
    assert np.array_equal(mask, (distances(points, boxes) < 0).all(axis=2))  # the float64 geometry agrees, as the margin promises
    assert mask.any(axis=0).all() and (~mask).any(axis=0).all() and (mask.sum(axis=1) >= 2).any()
    flips = 0
    if cols == 12:
        flips = int((mask != (distances(points, boxes, angle_col=10) < 0).all(axis=2)).sum())
        assert flips > 0
    print("cols %d ndim %d: redrawn %d, inside %d of %d, in two boxes %d, column 10 would flip %d" %
          (cols, ndim, redrawn, int(mask.sum()), mask.size, int((mask.sum(axis=1) >= 2).sum()), flips))
    return dict(points=points, boxes=boxes, mask=mask, counts=np.asarray(counts, np.int64))


def main():
    ops = load_reference()
    r = np.random.default_rng(2026)
    arrays = {"numpy_version": np.array(np.__version__), "margin": np.float64(MARGIN)}
    names = []
    for cols in (12, 7):
        for ndim in (5, 4):
            name = "c%d_p%d" % (cols, ndim)
            names.append(name)
            for k, v in make_case(r, ops, cols, ndim).items():
                arrays["%s/%s" % (name, k)] = v
    arrays["names"] = np.array(names)
    make_golden.save("points_in_boxes.npz", **arrays)


if __name__ == "__main__":
    main()
