"""NumPy restatement of fd_gt_sample_select / fd_gt_sample_points (include/futuredet_hip.h): DataBaseSamplerV2.sample_all /
sample_class_v2 of the reference (det3d/core/sampler/sample_ops.py:101-253, 275-351) with center_to_corner_box2d and box_collision_test
(det3d/core/sampler/preprocess.py:881-964) written out in fp32, one operation at a time, the sine and cosine taken in float64 and cast;
the containment branch is the one numba compiles (a box wholly inside another collides)."""
import numpy as np

F = np.float32
OFFSETS = ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))
NO_ROW, NO_POINTS, COUNTS_DIFFER, BAD_INDEX = 1, 2, 4, 8
SENTINEL = F(1e30)
MAX_ROWS = 1 << 28


def corners(box, angle_col):
    """one box row [12] -> ([4, 2] fp32 corners, [4] fp32 stand-up box) with the angle read from ``angle_col``"""
    b = np.asarray(box, F)
    a = np.float64(b[angle_col])
    s, c = F(np.sin(a)), F(np.cos(a))
    out = np.zeros((4, 2), F)
    for k, (nx, ny) in enumerate(OFFSETS):
        ox, oy = b[3] * F(nx), b[4] * F(ny)
        out[k, 0] = (ox * c + oy * s) + b[0]
        out[k, 1] = (-(ox * s) + oy * c) + b[1]
    su = np.array([out[:, 0].min(), out[:, 1].min(), out[:, 0].max(), out[:, 1].max()], F)
    return out, su


def _holds(p, q):
    """all corners of q strictly inside the clockwise quadrilateral p"""
    for l in range(4):
        for k in range(4):
            vec = p[k] - p[(k + 1) % 4]
            vec = -vec
            cross = vec[1] * (p[k, 0] - q[l, 0])
            cross = cross - vec[0] * (p[k, 1] - q[l, 1])
            assert cross.dtype == F
            if cross >= 0:
                return False
    return True


def collide(P, Q):
    """box_collision_test(boxes = P, qboxes = Q) for one pair; P, Q = (corners, stand-up box)"""
    p, ps = P
    q, qs = Q
    iw = min(ps[2], qs[2]) - max(ps[0], qs[0])
    if not iw > 0:
        return False
    ih = min(ps[3], qs[3]) - max(ps[1], qs[1])
    if not ih > 0:
        return False
    for k in range(4):
        A, B = p[k], p[(k + 1) % 4]
        for l in range(4):
            C, D = q[l], q[(l + 1) % 4]
            acd = (D[1] - A[1]) * (C[0] - A[0]) > (C[1] - A[1]) * (D[0] - A[0])
            bcd = (D[1] - B[1]) * (C[0] - B[0]) > (C[1] - B[1]) * (D[0] - B[0])
            if acd != bcd:
                abc = (C[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (C[0] - A[0])
                abd = (D[1] - A[1]) * (B[0] - A[0]) > (B[1] - A[1]) * (D[0] - A[0])
                if abc != abd:
                    return True
    if _holds(p, q):
        return True
    return _holds(q, p)


def select_one(boxes, counts, classes, trajectory, db, cand, groups, rate, point_cap):
    """One sample.  boxes [T, n_max, 12], counts [T], classes / trajectory (or None) [T, n_max]; db: dict of numpy arrays boxes
    [M, Tdb, 12], steps, classes, trajectory [M], offsets [M + 1], points [P, ndim]; cand [K]; groups: rows (class_id, trajectory,
    max_num, first, n).  Returns the outputs as a dict; the row arrays are updated COPIES (rows past the new counts keep their input)."""
    boxes, counts, classes = np.array(boxes, F), np.array(counts, np.int32), np.array(classes, np.int32)
    trajectory = np.array(trajectory, np.int32) if trajectory is not None else None
    T, n_max = boxes.shape[:2]
    K, M, P = len(cand), len(db["boxes"]), len(db["points"])
    Tdb = db["boxes"].shape[1]
    c = np.clip(counts, 0, n_max)
    c0 = int(c[0])
    status = 0
    rows = np.zeros((K,), np.int64)
    valid = np.zeros((K,), bool)
    for i, e in enumerate(cand):
        if 0 <= e < M:
            o0, o1 = int(db["offsets"][e]), int(db["offsets"][e + 1])
            if o0 < 0 or o1 < o0 or o1 > P or o1 - o0 > MAX_ROWS:
                status |= BAD_INDEX
            else:
                valid[i], rows[i] = True, o1 - o0
        elif e != -1:
            status |= BAD_INDEX
    if np.any(counts != counts[0]):
        status |= COUNTS_DIFFER
    part = []
    for (cls, tr, max_num, first, n) in groups:
        hit = classes[0, :c0] == cls
        if tr >= 0:
            hit = hit & (trajectory[0, :c0] == tr)
        want = max(0.0, float(np.round(np.float64(rate) * np.float64(int(max_num) - int(hit.sum())))))
        slots = [i for i in range(first, first + n) if valid[i]]
        part.append(slots[:int(min(want, 64.0))])
    cand_q = {i: corners(db["boxes"][cand[i], 0], 11) for g in part for i in g}
    obst_q = {i: corners(db["boxes"][cand[i], 0], 10) for g in part for i in g}
    gt_q = [corners(boxes[0, j], 10) for j in range(c0)]
    accepted, n_pts = [], 0
    max_count = int(c.max())
    for slots in part:
        earlier = list(accepted)
        alive = set(slots)
        for i in slots:
            ok = not any(collide(cand_q[i], g) for g in gt_q)
            ok = ok and not any(collide(cand_q[i], obst_q[j]) for j in earlier)
            ok = ok and not any(collide(cand_q[i], cand_q[j]) for j in sorted(alive) if j != i)
            if ok and max_count + len(accepted) >= n_max:
                ok = False
                status |= NO_ROW
            if ok and rows[i] > point_cap - n_pts:
                ok = False
                status |= NO_POINTS
            if ok:
                accepted.append(i)
                n_pts += int(rows[i])
            else:
                alive.discard(i)
    for t in range(T):
        for r, i in enumerate(accepted):
            e = cand[i]
            at = int(c[t]) + r
            tt = t if t < min(int(db["steps"][e]), Tdb) else 0
            boxes[t, at, :6] = db["boxes"][e, 0, :6]
            boxes[t, at, 6:] = db["boxes"][e, tt, 6:]
            classes[t, at] = db["classes"][e]
            if trajectory is not None:
                trajectory[t, at] = db["trajectory"][e]
    acc = np.zeros((K,), np.int32)
    acc[accepted] = 1
    plan = np.zeros((K, 3), np.int64)  # src_row, rows, dst_row
    run = 0
    for i in range(K):
        if acc[i]:
            plan[i] = (db["offsets"][cand[i]], rows[i], run)
            run += int(rows[i])
        else:
            plan[i] = (0, 0, run)
    return dict(boxes=boxes, counts=(c + len(accepted)).astype(np.int32), classes=classes, trajectory=trajectory, accepted=acc, plan=plan,
                n_points=n_pts, status=status)


def select(boxes, counts, classes, trajectory, db, cand, groups, rate, point_cap):
    """the batch: [B, ...] inputs, a dict of stacked outputs"""
    outs = [select_one(boxes[b], counts[b], classes[b], trajectory[b] if trajectory is not None else None, db, cand[b], groups, rate, point_cap)
            for b in range(len(boxes))]
    res = {k: np.stack([o[k] for o in outs]) for k in ("boxes", "counts", "classes", "accepted", "plan")}
    res["trajectory"] = np.stack([o["trajectory"] for o in outs]) if trajectory is not None else None
    res["n_points"] = np.array([o["n_points"] for o in outs], np.int32)
    res["status"] = np.array([o["status"] for o in outs], np.int32)
    return res


def paste(db, cand, accepted, plan, point_cap):
    """fd_gt_sample_points: the staged rows [point_cap, ndim] of one sample"""
    pts = np.asarray(db["points"], F)
    ndim = pts.shape[1]
    out = np.zeros((point_cap, ndim), F)
    out[:, :3] = SENTINEL
    for i in range(len(cand)):
        src, n, dst = (int(v) for v in plan[i])
        if accepted[i] and n > 0:
            seg = pts[src:src + n].copy()
            seg[:, :3] = seg[:, :3] + np.asarray(db["boxes"][cand[i], 0, :3], F)
            out[dst:dst + n] = seg
    return out


def plan_words(plan32):
    """the kernel's plan [..., 4] int32 -> [..., 3] int64 (src_row, rows, dst_row)"""
    p = np.ascontiguousarray(plan32, np.int32)
    src = p[..., :2].copy().view(np.int64)[..., 0]
    return np.stack([src, p[..., 2].astype(np.int64), p[..., 3].astype(np.int64)], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- random robust cases
def _quad64(box, col, grow=0.0):
    w, l, a = float(box[3]) + 2 * grow, float(box[4]) + 2 * grow, float(box[col])
    s, c = np.sin(a), np.cos(a)
    return np.array([(w * nx * c + l * ny * s + float(box[0]), -(w * nx) * s + l * ny * c + float(box[1])) for nx, ny in OFFSETS])


def _sat64(p, q):
    for poly in (p, q):
        for k in range(4):
            e = poly[(k + 1) % 4] - poly[k]
            axis = np.array([-e[1], e[0]])
            a, b = p @ axis, q @ axis
            if a.max() <= b.min() or b.max() <= a.min():
                return False
    return True


def robust_against(box, others, grow=1e-3):
    """True when a float64 separating-axis test of ``box`` against every row of ``others`` [n, 12] gives the same answer with both
    boxes grown and shrunk by ``grow``, whichever of the two angle columns either box is read with: no rounding decides a pair"""
    if len(others) == 0:
        return True
    reach = 0.5 * np.hypot(box[3], box[4]) + 0.5 * np.hypot(others[:, 3], others[:, 4]) + 0.1
    near = np.nonzero(np.hypot(others[:, 0] - box[0], others[:, 1] - box[1]) < reach)[0]
    for j in near:
        for cp in (10, 11):
            for cq in (10, 11):
                if _sat64(_quad64(box, cp, grow), _quad64(others[j], cq, grow)) != _sat64(_quad64(box, cp, -grow), _quad64(others[j], cq, -grow)):
                    return False
    return True


def random_case(seed, n0, K, T, n_max, ndim=5, Tdb=3, sizes=None, with_trajectory=True):
    """A random sample whose every decision is robust to rounding: (boxes [T, n_max, 12], counts [T], classes, trajectory | None
    [T, n_max], db, cand [K], groups).  About a quarter of the candidates meet something; some boxes lie wholly inside others."""
    r = np.random.default_rng(seed)
    M = K + 8
    side = float(np.sqrt((n0 + M) * 70.0)) + 10.0

    def draw_box():
        b = np.zeros((12,), F)
        b[0:2] = r.uniform(-side / 2, side / 2, 2)
        b[2] = r.normal(0, 1)
        b[3:5] = r.uniform(0.5, 1.5, 2) * (np.array([0.7, 0.7]) if r.random() < 0.25 else np.array([2.0, 4.6]) * (3.0 if r.random() < 0.1 else 1.0))
        b[5] = 1.6
        b[6:10] = r.normal(0, 3, 4)
        b[10:12] = r.uniform(-3.2, 3.2, 2)
        return b

    boxes, cls = np.zeros((T, n_max, 12), F), np.zeros((T, n_max), np.int32)
    traj = np.zeros((T, n_max), np.int32) if with_trajectory else None
    for j in range(n0):
        boxes[0, j] = draw_box()
    for t in range(1, T):
        boxes[t, :n0] = boxes[0, :n0]
        boxes[t, :n0, 0:2] += r.normal(0, 2.0 * t, (n0, 2)).astype(F)
    cls[:, :n0] = r.integers(1, 4, n0)
    if traj is not None:
        traj[:, :n0] = r.integers(0, 3, n0)
    dbb = np.zeros((M, Tdb, 12), F)
    for e in range(M):
        while True:
            b = draw_box()
            if robust_against(b, boxes[0, :n0]) and robust_against(b, dbb[:e, 0]):
                break
        dbb[e, 0] = b
        for t in range(1, Tdb):
            dbb[e, t] = b
            dbb[e, t, 6:] = r.normal(0, 3, 6)
    rows = np.asarray(sizes if sizes is not None else r.integers(1, 30, M), np.int64)
    assert len(rows) == M
    P = int(rows.sum())
    pts = np.zeros((P, ndim), F)
    pts[:, :3] = r.uniform(-2, 2, (P, 3))
    pts[:, 3:] = r.integers(0, 256, (P, ndim - 3))
    db = dict(boxes=dbb, steps=r.integers(1, Tdb + 1, M).astype(np.int32), classes=r.integers(1, 4, M).astype(np.int32),
              trajectory=r.integers(0, 3, M).astype(np.int32), offsets=np.concatenate([[0], np.cumsum(rows)]).astype(np.int64), points=pts)
    cand = r.permutation(M)[:K].astype(np.int32)
    G = 1 if K < 4 else (3 if K < 32 else 4)
    per = K // G
    groups = []
    for g in range(G):
        first, n = g * per, per if g < G - 1 else K - g * per
        tr = 1 if (g == 2 and traj is not None) else -1
        hit = cls[0, :n0] == g % 3 + 1
        if tr >= 0:
            hit = hit & (traj[0, :n0] == tr)
        groups.append((g % 3 + 1, tr, int(hit.sum()) + n - (g % 2), first, n))
    return boxes, np.full((T,), n0, np.int32), cls, traj, db, cand, groups
