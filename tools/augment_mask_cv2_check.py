"""Prints the largest absolute difference between the bev-mask warp as this project defines it (include/futuredet_hip.h,
fd_augment_mask; restated in tests/augment_map_ref.py) and a real OpenCV, where somebody has one: the reference's ``get_mask``
(det3d/datasets/pipelines/preprocess.py:75-90) -- np.fliplr / np.flipud, cv2.getRotationMatrix2D, two cv2.warpAffine calls -- run with
cv2 on random and 0/1 maps over a set of parameters.  Nothing here gates anything: the project's tests run without cv2.  The definition
is OpenCV's classic fixed-point linear warp (1/32-pixel coordinates); recent OpenCV releases also ship another linear-warp
implementation, so a difference in the last bits -- or of up to a 1/32-pixel step of the map's slope -- does not mean either side is
wrong.  With a GPU and the built library the kernel's own output is compared as well (--device).

    python tools/augment_mask_cv2_check.py [--device]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_map_ref as am  # noqa: E402

PARAMS = [[0, 0, 0.0, 1.0, 0.0, 0.0], [1, 1, 0.0, 1.0, 3.0, -2.0], [0, 0, 0.0, 1.0, 0.5, 0.0], [1, 0, 0.3, 0.9, -1.37, 2.81],
          [0, 1, -0.78539816, 1.1, 0.25, -0.75], [0, 0, np.pi / 2, 1.0, 0.0, 0.0], [1, 1, -np.pi / 2, 1.05, 7.0, 7.0]]


def cv2_get_mask(cv2, mask, t, angle, flip, scale):
    """get_mask as the reference writes it: mask [180, 180, C] fp32"""
    angle = np.degrees(-angle)
    if flip[0]:
        mask = np.fliplr(mask)
    if flip[1]:
        mask = np.flipud(mask)
    rot_mat = cv2.getRotationMatrix2D((90, 90), angle, scale)
    mask = cv2.warpAffine(np.ascontiguousarray(mask), rot_mat, (180, 180))
    M = np.float32([[1, 0, t[0]], [0, 1, t[1]]])
    return cv2.warpAffine(mask, M, (180, 180))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="also compare fd_augment_mask itself (needs the GPU and the built library)")
    args = ap.parse_args()
    try:
        import cv2
    except ImportError:
        print("cv2 is not installed: nothing to compare against (the project's tests do not need it)")
        return 0
    r = np.random.default_rng(0)
    maps = r.random((180, 180, 6), dtype=np.float32)
    maps[..., 1::2] = (maps[..., 1::2] < 0.5).astype(np.float32)
    worst = 0.0
    for p in PARAMS:
        full = np.array(p + [0.0], np.float64)
        want = cv2_get_mask(cv2, maps, p[4:6], p[2], p[0:2], p[3]).transpose(2, 0, 1)
        mine = am.get_mask(maps.transpose(2, 0, 1)[None], full[None])[0]
        d = float(np.abs(mine - want).max())
        line = "flips %d %d rot %+.4f scale %.2f t (%+.2f, %+.2f): restatement vs cv2 %s max |diff| %.3g, %d of %d pixels differ" % (
            p[0], p[1], p[2], p[3], p[4], p[5], cv2.__version__, d, int((mine != want).sum()), mine.size)
        if args.device:
            import torch

            from futuredet_amd import hip_ops
            from futuredet_amd.augment import GlobalAugment

            src = torch.from_numpy(np.ascontiguousarray(maps.transpose(2, 0, 1)[None])).cuda()
            got = hip_ops.augment_mask(src, GlobalAugment.mask_record(full[None], device=src.device)).cpu().numpy()[0]
            line += "; kernel vs cv2 %.3g, kernel vs restatement %.3g" % (float(np.abs(got - want).max()), float(np.abs(got - mine).max()))
            d = max(d, float(np.abs(got - want).max()))
        worst = max(worst, d)
        print(line)
    print("largest absolute difference against cv2: %.3g" % worst)
    return 0


if __name__ == "__main__":
    sys.exit(main())
