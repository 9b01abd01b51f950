"""Suppression patterns with answers known by construction, shared by test_nms_edges_host.py (which proves the answers with the host
oracle) and test_gpu_nms_edges.py (which runs them through fd_rotated_nms and the decode).

A scene is a list of yaw-0 squares in score order, placed in units of one BEV cell: the decode computes a centre as
(column + reg) * out_size_factor * voxel_size + pc_range in float32, and with positions that are multiples of 1/8 cell the sum
column + reg is exact, so two candidates of different cells given the same position decode to bit-identical centres.  With
out_size_factor 8 and voxel 0.075 m a cell is 0.6 m: squares of SIDE = 0.15 m at a pitch of 1/8 cell (0.075 m) overlap their neighbours
by IoU 1/3 and touch their second neighbours (IoU 0); squares half a cell apart are 0.15 m clear of each other.  The squared centre
distances are 0.005625 (neighbours), 0.0225 (second neighbours) and >= 0.09 (free): RADIUS = 0.01 separates them for the circular NMS,
whose threshold is compared with the squared distance (circle_nms_jit.py)."""
import numpy as np

SIDE = 0.15
IOU_THR = 0.2
CLEARANCE = 0.05
RADIUS = 0.01
PATTERNS = ("chain", "star", "free", "clusters", "late")
SIZES = (1, 63, 64, 65, 128, 129, 1000)
OSF, VOXEL, PC = np.float32(8.0), np.float32(0.075), np.float32(-54.0)


def _slot(k):
    """free position k (cell units): a 40-wide grid at half-cell pitch, no two slots overlap"""
    k = np.asarray(k)
    return np.stack([20.0 + 0.5 * (k % 40), 20.0 + 0.5 * (k // 40)], -1)


def cluster_lengths(n):
    """runs of identical boxes: 1, 2, 59, 1, 1 put cluster starts at rows 62, 63 and 64; then 63, 64, 65, 1, 2 over and over, cut at n"""
    lens, tail, total, i = [1, 2, 59, 1, 1], [63, 64, 65, 1, 2], 0, 0
    out = []
    while total < n:
        ln = lens[i] if i < len(lens) else tail[(i - len(lens)) % len(tail)]
        ln = min(ln, n - total)
        out.append(ln)
        total += ln
        i += 1
    return out


def pattern(name, n):
    """-> (positions [n,2] float64 in cell units, score order; the kept rows, written down from the construction)"""
    idx = np.arange(n)
    if name == "chain":  # row i overlaps rows i - 1 and i + 1 only: every even row is kept, every odd row falls to the row before it
        return np.stack([10.0 + idx / 8.0, np.full(n, 10.0)], -1), list(range(0, n, 2))
    if name == "star":   # n copies of one box
        return np.tile(_slot(0), (n, 1)), [0] if n else []
    if name == "free":
        return _slot(idx), list(range(n))
    if name == "clusters":
        lens = cluster_lengths(n)
        starts = np.cumsum([0] + lens[:-1]).tolist()
        return np.concatenate([np.tile(_slot(c), (ln, 1)) for c, ln in enumerate(lens)], 0), starts
    if name == "late":
        # row 0 suppresses rows of the LAST 64-column block only (copies of row 0 there: two of every three rows); the rows between are
        # copies of row 1, so few rows are kept before the last block and post_max does not cut the sweep short of it
        lb = 64 * ((n - 1) // 64)
        pos, keep = _slot(idx), []
        for i in range(n):
            if i >= max(lb, 2):
                if (i - lb) % 3 != 1:
                    pos[i] = pos[0]
                    continue
            elif i >= 2:
                pos[i] = pos[1]
                continue
            keep.append(i)
        return pos, keep
    raise KeyError(name)


def centers(pos):
    """the decode's centre arithmetic (center_head.py:641-649) on float32, left to right"""
    p = np.asarray(pos, np.float64).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), np.asarray(pos, np.float64)), "positions must be exact in float32"
    return ((p * OSF) * VOXEL + PC).astype(np.float32)


def boxes(pos, side=SIDE):
    """[n,7] rows x y z dx dy dz yaw as the decode returns them for these positions: z 0, yaw atan2(0, 1) = 0"""
    n = len(pos)
    b = np.zeros((n, 7), np.float32)
    b[:, :2] = centers(pos)
    b[:, 3:6] = np.exp(np.log(np.float32(side)))
    return b


def decode_maps(pos, H, W, cells, logits, side=SIDE):
    """Head maps [1,C,H,W] whose decode is boxes(pos): candidate i sits in cell cells[i] with logit logits[i]; every other cell is far below
    any score threshold."""
    pos = np.asarray(pos, np.float64)
    cells = np.asarray(cells, np.int64)
    hm = np.full((1, 1, H * W), -20.0, np.float32)
    reg = np.zeros((1, 2, H * W), np.float32)
    hm[0, 0, cells] = logits
    reg[0, 0, cells] = pos[:, 0] - cells % W
    reg[0, 1, cells] = pos[:, 1] - cells // W
    # (column + reg is exact: both are multiples of 1/8 below 2^10)
    assert np.array_equal((cells % W).astype(np.float32) + reg[0, 0, cells], pos[:, 0].astype(np.float32))
    assert np.array_equal((cells // W).astype(np.float32) + reg[0, 1, cells], pos[:, 1].astype(np.float32))
    height = np.zeros((1, 1, H * W), np.float32)
    dim = np.full((1, 3, H * W), np.log(np.float32(side)), np.float32)
    rot = np.zeros((1, 2, H * W), np.float32)
    rot[0, 1] = 1.0
    return tuple(a.reshape(1, -1, H, W) for a in (hm, reg, height, dim, rot))


def iou_clear_of_threshold(iou, thr=IOU_THR, clearance=CLEARANCE):
    """every pair's IoU is at least ``clearance`` away from ``thr``: the greedy list has no near-threshold excuse"""
    off = iou[~np.eye(len(iou), dtype=bool)]
    return bool(np.all(np.abs(off - thr) >= clearance))


def radius_clear_of_distances(xy, r=RADIUS):
    """no squared centre distance within 1e-3 (relative) of the circular-NMS threshold"""
    xy = np.asarray(xy, np.float64)
    d = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    return bool(np.all(np.abs(d - r) > 1e-3 * r))


def greedy(suppresses):
    """the reference loop (iou3d_nms.cpp:116-132) on a boolean matrix"""
    n = len(suppresses)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= suppresses[i, i + 1:]
    return keep
