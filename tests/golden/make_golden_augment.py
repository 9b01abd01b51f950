"""Generates tests/golden/augment.npz: the reference's four global transforms -- prep.random_flip_both, prep.global_rotation,
prep.global_scaling_v2, prep.global_translate_ (det3d/core/sampler/preprocess.py), called in Preprocess's order
(det3d/datasets/pipelines/preprocess.py:189-192) -- on a seeded 257-point cloud [x, y, z, i, dt] and T = 3 lists of [5, 12] boxes, by
IMPORTING the reference with the import shims of make_golden.py.
Run:  python tests/golden/make_golden_augment.py

The reference draws from the global np.random stream: each case seeds it.  The seeds are searched so that every flip combination
occurs; one more case runs with rotation=[0.0, 0.0].  The fixture holds inputs, the values the four functions returned (flips, angle,
factor, translation) and their outputs, plus np.__version__ (NumPy 2 keeps ``fp32 array op python float`` in fp32, NEP 50).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

ROT, SCALE, STD = [-0.785, 0.785], [0.9, 1.1], 0.5  # every configs/centerpoint/*.py
N_POINTS, T, N_BOXES = 257, 3, 5


def inputs(seed):
    rng = np.random.default_rng(1000 + seed)
    pts = np.zeros((N_POINTS, 5), np.float32)
    pts[:, 0:2] = rng.uniform(-54.0, 54.0, (N_POINTS, 2))
    pts[:, 2] = rng.uniform(-5.0, 3.0, N_POINTS)
    pts[:, 3] = rng.integers(0, 256, N_POINTS)
    pts[:, 4] = rng.integers(0, 10, N_POINTS) * 0.05
    boxes = np.zeros((T, N_BOXES, 12), np.float32)
    boxes[..., 0:2] = rng.uniform(-54.0, 54.0, (T, N_BOXES, 2))
    boxes[..., 2] = rng.normal(0.0, 1.0, (T, N_BOXES))
    boxes[..., 3:6] = np.asarray([1.9, 4.6, 1.7]) * rng.uniform(0.5, 1.6, (T, N_BOXES, 3))
    boxes[..., 6:10] = rng.normal(0.0, 3.0, (T, N_BOXES, 4))
    boxes[..., 10:12] = rng.uniform(-3.2, 3.2, (T, N_BOXES, 2))
    return pts, boxes


def run(prep, seed, rotation):
    pts, boxes = inputs(seed)
    p, gt = pts.copy(), [b.copy() for b in boxes]
    np.random.seed(seed)
    gt, p, flips = prep.random_flip_both(gt, p)
    gt, p, rot = prep.global_rotation(gt, p, rotation=rotation)
    gt, p, scale = prep.global_scaling_v2(gt, p, *SCALE)
    gt, p, trans = prep.global_translate_(gt, p, noise_translate_std=STD)
    assert p.dtype == np.float32 and all(b.dtype == np.float32 for b in gt)
    return dict(points_in=pts, boxes_in=boxes, flips=np.asarray(flips, np.int32), rot=np.float64(rot), scale=np.float64(scale),
                trans=np.asarray(trans, np.float64), points_out=p, boxes_out=np.stack(gt))


def main():
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    prep = make_golden._import_ref_pipeline("preprocess").prep
    cases, seen = {}, set()
    for seed in range(64):  # the first seed of each flip combination, then the next seeds up to six cases
        c = run(prep, seed, list(ROT))
        combo = tuple(int(v) for v in c["flips"])
        if combo not in seen or (len(seen) == 4 and len(cases) < 6):
            seen.add(combo)
            cases["seed%d" % seed] = c
        if len(seen) == 4 and len(cases) >= 6:
            break
    assert len(seen) == 4
    cases["rot0"] = run(prep, 100, [0.0, 0.0])
    assert cases["rot0"]["rot"] == 0.0
    arrays = {"numpy_version": np.array(np.__version__), "names": np.array(sorted(cases))}
    for name, c in cases.items():
        print(name, "flips", c["flips"].tolist(), "rot %.4f scale %.4f" % (c["rot"], c["scale"]), "trans", c["trans"].round(3).tolist())
        for k, v in c.items():
            arrays["%s/%s" % (name, k)] = v
    make_golden.save("augment.npz", **arrays)


if __name__ == "__main__":
    main()
