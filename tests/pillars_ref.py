"""Plain numpy references of the PointPillars input path -- pillar reader (PillarFeatureNet + PFNLayers), PointPillarsScatter, sweep
assembly -- with the input recipes and the agreement rule shared by tests/test_gpu_pillars_eval.py, tests/test_gpu_sweeps_edges.py
and tests/test_pillars_ref_host.py.  Nothing here calls the HIP library or torch: test_pillars_ref_host.py ties these functions to
the reference's goldens and to the CPU oracle before they judge a kernel."""
import numpy as np

from parity_util import report

GATE_FACTOR = 4.0  # the kernel may be this many times further from the float64 reference than the fp32 restatement is


# ================================================================================================ pillar reader
def decorate_ref(voxels, num_points, coors4, geom, with_distance, dtype=np.float64):
    """pillar_encoder.py:113-149: [raw | raw_xyz - mean | x - cx | y - cy | (||xyz||)] with rows p >= num_points zeroed AFTER the
    decoration (a multiplication by the 0/1 mask, as the reference does it).  The mean is the sum over all P rows (slot order, an
    accumulator started at 0) divided by num_points.  Every operation is evaluated in ``dtype``."""
    v = np.asarray(voxels).astype(dtype)
    M, P, nd = v.shape
    num = np.asarray(num_points).astype(dtype)
    vx, vy, x_off, y_off = (dtype(g) for g in geom)
    acc = np.zeros((M, 3), dtype)
    for p in range(P):
        acc = acc + v[:, p, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = acc / num[:, None]
        cx = np.asarray(coors4)[:, 3].astype(dtype) * vx + x_off
        cy = np.asarray(coors4)[:, 2].astype(dtype) * vy + y_off
        parts = [v, v[:, :, :3] - mean[:, None, :], (v[:, :, 0] - cx[:, None])[..., None], (v[:, :, 1] - cy[:, None])[..., None]]
        if with_distance:
            parts.append(np.sqrt(v[:, :, 0] * v[:, :, 0] + v[:, :, 1] * v[:, :, 1] + v[:, :, 2] * v[:, :, 2])[..., None])
        x = np.concatenate(parts, axis=2)
        mask = (np.arange(P)[None, :] < np.asarray(num_points)[:, None]).astype(dtype)
        x = x * mask[:, :, None]
    assert x.dtype == dtype
    return x


def pfn_layers_ref(x, layers, dtype=np.float64):
    """pillar_encoder.py:38-55 on decorated rows x [M, P, Fin]: per layer Linear (no bias) -> scale * . + shift (eval BatchNorm1d
    folded) -> ReLU, the max over ALL P rows; a layer that is not the last hands [x[p], max] to the next one.  -> [M, U_last]"""
    x = np.asarray(x).astype(dtype)
    for i, (w, scale, shift) in enumerate(layers):
        w, scale, shift = (np.asarray(a).astype(dtype) for a in (w, scale, shift))
        with np.errstate(invalid="ignore"):
            y = np.maximum(np.matmul(x, w.T) * scale + shift, dtype(0))  # (np.maximum and .max propagate NaN, like torch)
            mx = y.max(axis=1, keepdims=True)
        if i == len(layers) - 1:
            assert mx.dtype == dtype
            return mx[:, 0, :]
        x = np.concatenate([y, np.broadcast_to(mx, y.shape)], axis=2)


def pillar_encode_ref(voxels, num_points, coors4, geom, layers, with_distance, dtype=np.float64):
    """PillarFeatureNet.forward (pillar_encoder.py:113-164) as fd_pillars.hip's header states it.  voxels [M, P, ndim], num_points
    [M], coors4 [M, 4] (b, z, y, x), geom = (vx, vy, x_offset, y_offset), layers = [(weight [U, Fin], scale [U], shift [U])] (one or two
    entries; with two, the first has 32 units and the second reads 64 columns).  dtype=np.float32 evaluates the same statement in
    fp32: the yardstick of ``rule``.  A pillar with num_points == 0 comes out NaN, as in the reference."""
    return pfn_layers_ref(decorate_ref(voxels, num_points, coors4, geom, with_distance, dtype), layers, dtype)


def fold_bn(weight, gamma, beta, running_mean, running_var, eps=1e-3):
    """eval BatchNorm1d behind a bias-free Linear as (weight, scale, shift), in float64"""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(running_var, np.float64) + eps)
    return np.asarray(weight, np.float64), scale, np.asarray(beta, np.float64) - np.asarray(running_mean, np.float64) * scale


def rule(name, fused, restated, truth, factor=GATE_FACTOR):
    """solver_util.rule for the reader: the kernel's maximum error against the float64 reference is at most ``factor`` x the fp32
    restatement's own maximum error against it, with a floor of one fp32 ulp of the reference's largest magnitude.  Prints both
    errors and their ratio, then asserts.  -> (kernel error, restatement error)"""
    fused, restated, truth = (np.asarray(a, np.float64).ravel() for a in (fused, restated, truth))
    assert fused.shape == truth.shape == restated.shape, (name, fused.shape, restated.shape, truth.shape)
    assert np.isfinite(truth).all() and truth.size > 0, name
    e_fused = float(np.abs(fused - truth).max())
    e_rest = float(np.abs(restated - truth).max())
    floor = float(np.spacing(np.float32(np.abs(truth).max())))
    bound = max(factor * e_rest, floor)
    report(name, e_fused, bound, "fp32 restatement err %.3e  ratio %s  ulp floor %.3e" % (
        e_rest, "%.2f" % (e_fused / e_rest) if e_rest > 0 else "n/a", floor))
    assert np.isfinite(e_fused) and e_fused <= bound, "%s: kernel err %.3e > bound %.3e (fp32 restatement err %.3e)" % (
        name, e_fused, bound, e_rest)
    return e_fused, e_rest


PILLAR_RANGE = (-50.0, -50.0, -5.0, 50.0, 50.0, 3.0)
PILLAR_VOXEL = (0.25, 0.25)
PILLAR_GEOM = (PILLAR_VOXEL[0], PILLAR_VOXEL[1], PILLAR_VOXEL[0] / 2 + PILLAR_RANGE[0], PILLAR_VOXEL[1] / 2 + PILLAR_RANGE[1])


def make_pillars(rng, M, P, ndim, batch_size=1):
    """Pillars at realistic magnitude: distinct cells of a 400 x 400 grid over +-50 m, every point inside its pillar's cell, z in
    [-5, 3], intensity 0..255, further columns in [0, 1]; padding slots zero.  num_points cycles through 1, P and values in between.
    -> voxels [M, P, ndim] f32, num_points [M] i32, coors4 [M, 4] i32"""
    nx = int(round((PILLAR_RANGE[3] - PILLAR_RANGE[0]) / PILLAR_VOXEL[0]))
    ny = int(round((PILLAR_RANGE[4] - PILLAR_RANGE[1]) / PILLAR_VOXEL[1]))
    cells = rng.choice(batch_size * ny * nx, M, replace=False)
    b, y, x = cells // (ny * nx), (cells // nx) % ny, cells % nx
    coors4 = np.stack([b, np.zeros(M, np.int64), y, x], 1).astype(np.int32)
    num = np.empty(M, np.int32)
    num[0::3] = 1
    num[1::3] = P
    num[2::3] = rng.integers(1, P + 1, len(num[2::3]))
    vox = np.zeros((M, P, ndim), np.float32)
    vox[:, :, 0] = PILLAR_RANGE[0] + (x[:, None] + rng.uniform(0.02, 0.98, (M, P))) * PILLAR_VOXEL[0]
    vox[:, :, 1] = PILLAR_RANGE[1] + (y[:, None] + rng.uniform(0.02, 0.98, (M, P))) * PILLAR_VOXEL[1]
    vox[:, :, 2] = rng.uniform(-5.0, 3.0, (M, P))
    if ndim > 3:
        vox[:, :, 3] = rng.integers(0, 256, (M, P))
    if ndim > 4:
        vox[:, :, 4:] = rng.uniform(0.0, 1.0, (M, P, ndim - 4))
    vox[np.arange(P)[None, :] >= num[:, None]] = 0.0
    return vox, num, coors4


def make_shift(rng, units):
    """A quarter of the units with a large positive shift (a masked row's relu(shift) can win the max), a quarter negative"""
    shift = rng.uniform(-0.2, 0.2, units)
    shift[0::4] = rng.uniform(1.5, 2.5, len(shift[0::4]))
    shift[2::4] = rng.uniform(-1.0, -0.5, len(shift[2::4]))
    return shift


def make_layers(rng, units, fin):
    """[(weight, scale, shift)] float32 for units = [16] / [32] / [64] (one layer) or [32, 64] (two layers).  The first Linear is
    scaled by 0.02 (raw coordinates of tens of metres and intensities up to 255 enter it directly), so activations stay O(1)."""
    layers, cin = [], fin
    for i, u in enumerate(units):
        w = rng.standard_normal((u, cin)) / np.sqrt(cin) * (0.02 if i == 0 else 1.0)
        scale = rng.uniform(0.6, 1.4, u) * np.where(rng.random(u) < 0.2, -1.0, 1.0)
        layers.append((w.astype(np.float32), scale.astype(np.float32), make_shift(rng, u).astype(np.float32)))
        cin = 2 * u
    return layers


# ================================================================================================ scatter
def pillar_scatter_ref(feats, coors4, n, B, ny, nx):
    """PointPillarsScatter.forward (pillar_encoder.py:186-221): canvas[b, :, y, x] = feats[m] for the first n rows, zero elsewhere;
    rows whose b, y or x lies outside the canvas are skipped.  Exact (a copy); callers guarantee unique cells."""
    feats = np.asarray(feats)
    canvas = np.zeros((B, feats.shape[1], ny, nx), feats.dtype)
    for m in range(min(int(n), len(feats))):
        b, _, y, x = (int(c) for c in coors4[m])
        if 0 <= b < B and 0 <= y < ny and 0 <= x < nx:
            canvas[b, :, y, x] = feats[m]
    return canvas


# ================================================================================================ sweep assembly
def assemble_sweeps_ref(raw, rows, transforms, lags, remove_close, keep_cols=4, min_distance=1.0):
    """LoadPointCloudFromFile's NuScenes branch (loading.py:107-141) with read_file's column cut (:31), remove_close (:36-45) and
    read_sweep (:47-60) on in-memory rows.  raw [R, raw_cols] float32; sweep s (in visit order) owns rows[s]:rows[s + 1] (rows past
    rows[-1] belong to nobody); transforms[s] a 4x4 or None; lags[s] a float; remove_close[s] a bool.  -> [N, keep_cols + 1] float32,
    the sweeps' surviving rows in order."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32
    radius = np.float32(min_distance)
    out = []
    for s in range(len(rows) - 1):
        pts = raw[int(rows[s]):int(rows[s + 1]), :keep_cols].T.copy()           # :31, :50  [keep_cols, n]
        if remove_close[s]:
            with np.errstate(invalid="ignore"):
                x_filt = np.abs(pts[0, :]) < radius                             # float32 comparisons, strict
                y_filt = np.abs(pts[1, :]) < radius
            pts = pts[:, np.logical_not(np.logical_and(x_filt, y_filt))]
        n = pts.shape[1]
        if transforms[s] is not None:
            m = np.asarray(transforms[s], np.float64).reshape(4, 4)
            with np.errstate(invalid="ignore", over="ignore"):
                pts[:3, :] = m.dot(np.vstack((pts[:3, :], np.ones(n))))[:3, :]  # float64 product, stored back as float32
        times = (lags[s] * np.ones((1, n))).astype(np.float32)                  # :58, :136
        out.append(np.hstack([pts.T, times.T]))
    if not out:
        return np.zeros((0, keep_cols + 1), np.float32)
    res = np.concatenate(out, axis=0)
    assert res.dtype == np.float32
    return res


def exact_transform(rng):
    """A 4x4 whose entries are multiples of 2^-10 below 64 in magnitude: with coordinates that are multiples of 2^-8 below 128,
    every product and partial sum of the 4x4 . [x y z 1] is exact in float64, whatever the order and with or without fma."""
    m = rng.integers(-(1 << 16) + 1, 1 << 16, (4, 4)).astype(np.float64) / 1024.0
    m[3] = [0.0, 0.0, 0.0, 1.0]
    return m


def exact_coords(rng, shape):
    """float32 multiples of 2^-8 below 128 in magnitude"""
    return (rng.integers(-(1 << 15) + 1, 1 << 15, shape).astype(np.float64) / 256.0).astype(np.float32)
