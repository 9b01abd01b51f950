"""NumPy restatement of fd_gt_range_filter (include/futuredet_hip.h): prep.filter_gt_box_outside_range of the reference
(det3d/core/sampler/preprocess.py:113-127) with center_to_corner_box2d / corners_nd / rotation_2d / minmax_to_corner_2d /
points_in_convex_polygon_jit written out in fp32, and the compaction the kernel applies to every timestep."""
import numpy as np

F = np.float32
OFFSETS = ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))  # corners_nd, clockwise from the minimum corner


def corners(boxes):
    """boxes [n, 12] fp32 -> [n, 4, 2] fp32: centre columns 0, 1, dims columns 3, 4, angle the LAST column"""
    b = np.asarray(boxes, F)
    s, c = np.sin(b[:, -1]), np.cos(b[:, -1])
    out = np.zeros((len(b), 4, 2), F)
    for k, (nx, ny) in enumerate(OFFSETS):
        ox, oy = b[:, 3] * F(nx), b[:, 4] * F(ny)
        out[:, k, 0] = (ox * c + oy * s) + b[:, 0]
        out[:, k, 1] = (-(ox * s) + oy * c) + b[:, 1]
    assert out.dtype == F
    return out


def rectangle(rng):
    xmin, ymin, xmax, ymax = (F(v) for v in rng)
    x1, y1 = xmin + (xmax - xmin), ymin + (ymax - ymin)
    return np.array([[xmin, ymin], [xmin, y1], [x1, y1], [x1, ymin]], F)


def inside(points, rng):
    """points [..., 2] fp32 -> bool: strictly inside the rectangle"""
    P = rectangle(rng)
    V = P - P[[3, 0, 1, 2]]
    pts = np.asarray(points, F)
    ok = np.ones(pts.shape[:-1], bool)
    for j in range(4):
        a = V[j, 1] * (P[j, 0] - pts[..., 0])
        b = V[j, 0] * (P[j, 1] - pts[..., 1])
        cross = a.astype(np.float64) - b.astype(np.float64)
        ok &= ~(cross >= 0)
    return ok


def mask(boxes, rng):
    """bool [n]: the keep-mask of boxes [n, 12]"""
    boxes = np.asarray(boxes, F).reshape(-1, 12)
    if len(boxes) == 0:
        return np.zeros((0,), bool)
    return inside(corners(boxes), rng).any(axis=1)


def apply(boxes, counts, classes, trajectory, rng):
    """the kernel's outputs: (boxes, counts, classes, trajectory | None, status) for [B, T, n_max, ...] inputs"""
    boxes, counts, classes = np.asarray(boxes, F), np.asarray(counts, np.int32), np.asarray(classes, np.int32)
    B, T, n_max = boxes.shape[:3]
    ob, oc, ok = np.zeros_like(boxes), np.zeros_like(counts), np.zeros_like(classes)
    ot = np.zeros_like(trajectory) if trajectory is not None else None
    status = np.zeros((B,), np.int32)
    for b in range(B):
        c0 = int(np.clip(counts[b, 0], 0, n_max))
        keep = mask(boxes[b, 0, :c0], rng)
        for t in range(T):
            m = min(int(np.clip(counts[b, t], 0, n_max)), c0)
            idx = np.nonzero(keep[:m])[0]
            k = len(idx)
            ob[b, t, :k], ok[b, t, :k], oc[b, t] = boxes[b, t, idx], classes[b, t, idx], k
            if ot is not None:
                ot[b, t, :k] = trajectory[b, t, idx]
            status[b] += int(counts[b, t] != counts[b, 0])
    return ob, oc, ok, ot, status
