"""Generates tests/golden/range_filter.npz: the train-mode ground-truth filter of the reference's Voxelization stage
(det3d/datasets/pipelines/preprocess.py:249-255) -- prep.filter_gt_box_outside_range (det3d/core/sampler/preprocess.py:113-127) called
on the boxes of timestep 0, once per timestep, as that stage does -- by IMPORTING the reference with the import shims of make_golden.py.
Run:  python tests/golden/make_golden_range_filter.py

Random cases: [T, n, 12] fp32 boxes drawn by REJECTION so that every BEV corner of every box (evaluated in float64) keeps at least 1e-3 m
from each of the four boundary lines: rounding cannot decide a case, the reference alone does, and nothing is excluded afterwards.
  edges     centres within 6 m of one of the four edges of the nuScenes range, the other coordinate anywhere along it
  corners   centres within 6 m of one of the four corners
  big       boxes larger than the range around centres inside it: the centre is inside while every corner is outside
  small     car-sized boxes around a 4 m x 4 m range: centres inside with all corners outside, centres outside with a corner inside
  asym      a range that is not symmetric (and whose x1 = xmin + (xmax - xmin) is rounded), boxes all over it
Exact cases (angle 0, representable numbers, no margin): per side of the range a box with two corners exactly ON the boundary line and
the others beyond it (dropped: the test is strict), a box with all corners beyond the line (dropped), a box straddling it (kept), and a
box with two corners on the line and two inside (kept).
The fixture holds boxes, the range (fp32, the ``pc_range[[0, 1, 3, 4]]`` the stage passes) and the stage's list of masks, [T, n] bool."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

MARGIN = 1e-3
NUSC = (-54.0, -54.0, 54.0, 54.0)
T = 3


def corners64(box):
    w, l, a = float(box[3]), float(box[4]), float(box[11])
    s, c = np.sin(a), np.cos(a)
    out = []
    for nx, ny in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):
        ox, oy = w * nx, l * ny
        out.append((ox * c + oy * s + float(box[0]), -ox * s + oy * c + float(box[1])))
    return np.array(out)


def clear_of_lines(box, rng):
    c = corners64(box)
    d = np.concatenate([np.abs(c[:, 0] - rng[0]), np.abs(c[:, 0] - rng[2]), np.abs(c[:, 1] - rng[1]), np.abs(c[:, 1] - rng[3])])
    return d.min() >= MARGIN


def draw(rng_np, n, rng, centre, dims=(1.9, 4.6)):
    """n rows [12] fp32; ``centre()`` draws (x, y); rejection on the margin"""
    rows = []
    while len(rows) < n:
        b = np.zeros((12,), np.float32)
        b[0:2] = centre()
        b[2] = rng_np.normal(0.0, 1.0)
        b[3:5] = np.asarray(dims) * rng_np.uniform(0.5, 1.6, 2)
        b[5] = 1.7
        b[6:10] = rng_np.normal(0.0, 3.0, 4)
        b[10:12] = rng_np.uniform(-3.2, 3.2, 2)
        if clear_of_lines(b, rng):
            rows.append(b)
    return np.stack(rows)


def timesteps(rng_np, first):
    """[T, n, 12]: timestep 0 decides; the later ones move on, some far out of the range -- they must not matter"""
    out = [first]
    for t in range(1, T):
        nxt = first.copy()
        nxt[:, 0:2] += rng_np.normal(0.0, 4.0 * t, (len(first), 2)).astype(np.float32)
        nxt[:, 10:12] += rng_np.normal(0.0, 0.5, (len(first), 2)).astype(np.float32)
        out.append(nxt)
    return np.stack(out)


def random_cases():
    r = np.random.default_rng(2024)
    x0, y0, x1, y1 = NUSC
    cases = {}

    def near(v):
        return v + r.uniform(-6.0, 6.0)

    def edge():
        side = r.integers(0, 4)
        along = r.uniform(-60.0, 60.0)
        return [(near(x0), along), (near(x1), along), (along, near(y0)), (along, near(y1))][side]

    def corner():
        return near((x0, x1)[r.integers(0, 2)]), near((y0, y1)[r.integers(0, 2)])

    cases["edges"] = (timesteps(r, draw(r, 96, NUSC, edge)), NUSC)
    cases["corners"] = (timesteps(r, draw(r, 64, NUSC, corner)), NUSC)
    cases["big"] = (timesteps(r, draw(r, 24, NUSC, lambda: r.uniform(-50.0, 50.0, 2), dims=(260.0, 300.0))), NUSC)
    small = (-2.0, -2.0, 2.0, 2.0)
    cases["small"] = (timesteps(r, draw(r, 96, small, lambda: r.uniform(-5.0, 5.0, 2))), small)
    asym = (-10.3, 0.1, 70.7, 40.9)
    cases["asym"] = (timesteps(r, draw(r, 96, asym, lambda: (r.uniform(-18.0, 78.0), r.uniform(-8.0, 49.0)))), asym)
    return cases


def exact_cases():
    x0, y0, x1, y1 = NUSC
    rows = []

    def box(x, y, w=2.0, l=4.0):
        b = np.zeros((12,), np.float32)
        b[0], b[1], b[3], b[4], b[5] = x, y, w, l, 1.5
        b[10] = 0.7  # column 10 is NOT the angle the filter reads
        rows.append(b)

    for x_side, sign in ((x1, 1.0), (x0, -1.0)):  # half width 1: corners at x -+ 1
        box(x_side + sign * 1.0, 3.0)   # two corners ON the line, two beyond: dropped
        box(x_side + sign * 2.0, 3.0)   # all beyond: dropped
        box(x_side, 3.0)                # straddling: kept
        box(x_side - sign * 1.0, 3.0)   # two on the line, two inside: kept
    for y_side, sign in ((y1, 1.0), (y0, -1.0)):  # half length 2: corners at y -+ 2
        box(-7.0, y_side + sign * 2.0)
        box(-7.0, y_side + sign * 4.0)
        box(-7.0, y_side)
        box(-7.0, y_side - sign * 2.0)
    box(x1 + 1.0, y1 + 2.0)  # one corner exactly ON the range's corner, the others outside: dropped
    box(x1 - 1.0, y1 - 2.0)  # one corner ON the range's corner, one strictly inside: kept
    box(0.0, 0.0)
    first = np.stack(rows)
    return {"exact": (np.stack([first] * T), NUSC)}


def main():
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    prep = make_golden._import_ref_pipeline("preprocess").prep
    cases = dict(random_cases(), **exact_cases())
    arrays = {"numpy_version": np.array(np.__version__), "names": np.array(sorted(cases)), "margin": np.float64(MARGIN)}
    for name, (boxes, rng) in cases.items():
        bv_range = np.asarray(rng, np.float32)
        gt = [b.copy() for b in boxes]
        masks = [prep.filter_gt_box_outside_range(gt[0], bv_range) for i in range(len(gt))]  # Voxelization.__call__
        assert all(np.array_equal(g, b) for g, b in zip(gt, boxes)) and all(m.dtype == np.bool_ for m in masks)
        masks = np.stack(masks)
        print(name, boxes.shape, "kept", int(masks[0].sum()), "of", masks.shape[1])
        arrays["%s/boxes" % name], arrays["%s/range" % name], arrays["%s/masks" % name] = boxes, bv_range, masks
    make_golden.save("range_filter.npz", **arrays)


if __name__ == "__main__":
    main()
