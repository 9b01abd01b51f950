"""NumPy restatement of the point-in-box kernels (include/futuredet_hip.h, "which points of a cloud lie inside which rotated 3-D
boxes"): box_np_ops.points_in_rbbox / points_count_rbbox of the reference, operation by operation in fp32 -- the face planes, the mask,
the counts, the ordered extraction (fd_points_in_boxes_extract), the point-count filter (fd_gt_min_points_filter) and the files
create_gt_database writes.  Every product and sum is a NumPy fp32 operation on its own, so each line below is one IEEE operation, in the
header's order."""
import os

import numpy as np

F32 = np.float32
# corner k -> (bx, by, bz); face f -> (P0, P1, P2)
CORNERS = np.array([(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)], F32)
FACES = ((0, 1, 2), (7, 6, 5), (0, 3, 7), (1, 5, 6), (0, 4, 5), (3, 2, 6))
NO_ROOM = 1


def corners(boxes):
    """[n, 8, 3] fp32: the corners of box rows [n, >= 7]; the angle is the LAST column"""
    b = np.ascontiguousarray(boxes, F32)
    cx, cy, cz, w, l, h, a = (b[:, k:k + 1] for k in (0, 1, 2, 3, 4, 5, b.shape[1] - 1))
    s, c = np.sin(a.astype(np.float64)).astype(F32), np.cos(a.astype(np.float64)).astype(F32)
    half = F32(0.5)
    ox, oy, oz = w * (CORNERS[None, :, 0] - half), l * (CORNERS[None, :, 1] - half), h * (CORNERS[None, :, 2] - half)
    x = (ox * c + oy * s) + cx
    y = (-(ox * s) + oy * c) + cy
    z = oz + cz
    return np.stack([x, y, z], axis=2).astype(F32)


def planes(boxes):
    """(normals [n, 6, 3], d [n, 6]) fp32"""
    P = corners(boxes)
    n = np.zeros((P.shape[0], 6, 3), F32)
    d = np.zeros((P.shape[0], 6), F32)
    for f, (i0, i1, i2) in enumerate(FACES):
        p0, p1, p2 = P[:, i0], P[:, i1], P[:, i2]
        u, v = p0 - p1, p1 - p2
        n[:, f, 0] = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        n[:, f, 1] = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        n[:, f, 2] = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        d[:, f] = ((-(p0[:, 0] * n[:, f, 0])) - p0[:, 1] * n[:, f, 1]) - p0[:, 2] * n[:, f, 2]
    return n, d


def mask(points, boxes, n_boxes=None):
    """bool [n_points, n_boxes_max]: point i inside box j; the rows at or past ``n_boxes`` (clamped) are no boxes and hold nothing"""
    pts = np.ascontiguousarray(points, F32)
    boxes = np.ascontiguousarray(boxes, F32)
    m = boxes.shape[0]
    nb = m if n_boxes is None else min(max(int(n_boxes), 0), m)
    out = np.zeros((pts.shape[0], m), bool)
    if nb == 0 or pts.shape[0] == 0:
        return out
    n, d = planes(boxes[:nb])
    px, py, pz = pts[:, 0:1, None], pts[:, 1:2, None], pts[:, 2:3, None]
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((px * n[None, :, :, 0] + py * n[None, :, :, 1]) + pz * n[None, :, :, 2]) + d[None]
        out[:, :nb] = ~(v >= 0).any(axis=2)
    return out


def counts(points, boxes, n_boxes=None):
    return mask(points, boxes, n_boxes).sum(axis=0).astype(np.int32)


def extract(points, boxes, ncols=None, n_boxes=None, cap_rows=None):
    """(rows [total | cap_rows, ncols] fp32, offsets int64 [n_boxes_max + 1], status): box after box, each box's points in cloud order,
    columns 0..2 minus the box centre, the others copied.  With ``cap_rows`` the rows at or past it are missing."""
    pts = np.ascontiguousarray(points, F32)
    boxes = np.ascontiguousarray(boxes, F32)
    ncols = pts.shape[1] if ncols is None else int(ncols)
    m = mask(pts, boxes, n_boxes)
    offsets = np.concatenate([[0], np.cumsum(m.sum(axis=0))]).astype(np.int64)
    parts = []
    for j in range(boxes.shape[0]):
        sel = pts[m[:, j]].copy()
        with np.errstate(invalid="ignore", over="ignore"):
            sel[:, :3] = sel[:, :3] - boxes[j, :3]
        parts.append(sel[:, :ncols])
    rows = np.concatenate(parts) if parts else np.zeros((0, ncols), F32)
    rows = np.ascontiguousarray(rows.reshape(-1, ncols), F32)
    status = 0
    if cap_rows is not None and len(rows) > cap_rows:
        rows, status = rows[:cap_rows], NO_ROOM
    return rows, offsets, status


def min_points_filter(boxes, gt_counts, classes, trajectory, point_counts, min_points):
    """fd_gt_min_points_filter: boxes [B, T, n, 12], gt_counts [B, T], classes / trajectory (or None) [B, T, n], point_counts [B, n].
    Returns new (boxes, counts, classes, trajectory, status)."""
    boxes, classes = np.asarray(boxes, F32), np.asarray(classes, np.int32)
    B, T, n = boxes.shape[:3]
    ob, oc, ok = np.zeros_like(boxes), np.zeros((B, T), np.int32), np.zeros_like(classes)
    ot = np.zeros_like(trajectory) if trajectory is not None else None
    status = np.zeros((B,), np.int32)
    for b in range(B):
        c0 = min(max(int(gt_counts[b, 0]), 0), n)
        keep = np.zeros((n,), bool)
        keep[:c0] = np.asarray(point_counts[b, :c0]) >= min_points
        for t in range(T):
            m = min(min(max(int(gt_counts[b, t]), 0), n), c0)
            k = keep.copy()
            k[m:] = False
            cnt = int(k.sum())
            ob[b, t, :cnt], ok[b, t, :cnt], oc[b, t] = boxes[b, t][k], classes[b, t][k], cnt
            if ot is not None:
                ot[b, t, :cnt] = trajectory[b, t][k]
            status[b] += int(gt_counts[b, t]) != int(gt_counts[b, 0])
    return ob, oc, ok, ot, status


def database_files(samples, stem, used_classes=None, num_point_features=5):
    """what create_gt_database writes (det3d/datasets/utils/create_gt_database.py:109-176), as data: (files {path relative to the
    database directory's parent: fp32 rows}, infos {name: [entries]}) for samples given as dicts (points, boxes [T, N, 12], names [N],
    trajectory [N], image_idx); ``stem`` is the database directory's name.  Samples without objects are skipped."""
    files, infos, group = {}, {}, 0
    for s in samples:
        boxes = np.asarray(s["boxes"], F32)
        pts = np.ascontiguousarray(np.asarray(s["points"], F32))
        T = boxes.shape[0]
        if boxes.shape[1] == 0:
            continue
        m = mask(pts, boxes[0])
        for i in range(boxes.shape[1]):
            name = s["names"][i]
            if used_classes is not None and name not in used_classes:
                continue
            sel = pts[m[:, i]].copy()
            sel[:, :3] = sel[:, :3] - boxes[0, i, :3]
            sel = np.ascontiguousarray(sel[:, :num_point_features])
            rel = os.path.join(stem, name, "%s_%s_%d.bin" % (s["image_idx"], name, i))
            files[rel] = sel
            infos.setdefault(name, []).append(dict(name=[name] * T, trajectory=[s["trajectory"][i]] * T, path=rel, image_idx=s["image_idx"],
                                                   gt_idx=i, box3d_lidar=[boxes[t, i] for t in range(T)], num_points_in_gt=len(sel),
                                                   difficulty=[0] * T, group_id=group))
            group += 1
    return files, infos
