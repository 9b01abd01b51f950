"""numpy restatement of the arithmetic of fd_augment.hip (include/futuredet_hip.h): flip a, flip b, rotation, scaling, translation of a
cloud and of [.., 12] box rows, every product and every sum one fp32 rounding in the kernels' order; and the same transforms in float64,
the yardstick of the rounding bound.  ``params``: flip_a, flip_b, rot, scale, tx, ty, tz (GlobalAugment.draw's row)."""
import numpy as np

F32 = np.float32
PI32, TWO_PI32 = F32(np.pi), F32(2 * np.pi)
PAIRS = ((0, 1), (6, 7), (8, 9))
U = 2.0 ** -24  # unit roundoff of fp32


def constants(params):
    fa, fb, rot, scale, tx, ty, tz = [float(v) for v in params]
    return bool(fa), bool(fb), F32(np.cos(rot)), F32(np.sin(rot)), F32(rot), F32(scale), (tx, ty, tz)


def _rotate(x, y, c, s):
    xc, ys, xs, yc = x * c, y * s, x * s, y * c  # four rounded products
    return xc + ys, -xs + yc


def _shift(v, t):
    return (v.astype(np.float64) + t).astype(F32)


def points(src, params, perm=None):
    """A(src[perm]) for src [n, 4 | 5] fp32"""
    fa, fb, c, s, _, scale, t = constants(params)
    out = np.array(src if perm is None else src[np.asarray(perm, np.int64)], F32, copy=True)
    x, y, z = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
    if fa:
        y = -y
    if fb:
        x = -x
    x, y = _rotate(x, y, c, s)
    x, y, z = x * scale, y * scale, z * scale
    out[:, 0], out[:, 1], out[:, 2] = _shift(x, t[0]), _shift(y, t[1]), _shift(z, t[2])
    assert out.dtype == F32
    return out


def box_rows(rows, params):
    """A(rows) for rows [n, 12] fp32"""
    fa, fb, c, s, rot, scale, t = constants(params)
    out = np.array(rows, F32, copy=True)
    for k in (10, 11):
        a = out[:, k].copy()
        if fa:
            a = -a + PI32
        if fb:
            a = -a + TWO_PI32
        out[:, k] = a + rot
    for i, j in PAIRS:
        x, y = out[:, i].copy(), out[:, j].copy()
        if fa:
            y = -y
        if fb:
            x = -x
        out[:, i], out[:, j] = _rotate(x, y, c, s)
    out[:, :10] = out[:, :10] * scale
    for k in range(3):
        out[:, k] = _shift(out[:, k].copy(), t[k])
    assert out.dtype == F32
    return out


def boxes(b, counts, params):
    """[B, T, n_max, 12] with counts [B, T] and params [B, 7]: the rows below the count transformed, the others unchanged"""
    out = np.array(b, F32, copy=True)
    B, T = out.shape[:2]
    for bi in range(B):
        for ti in range(T):
            n = max(0, min(int(counts[bi][ti]), out.shape[2]))
            out[bi, ti, :n] = box_rows(out[bi, ti, :n], params[bi])
    return out


def exact(xy, params, t_xy=(0.0, 0.0), flip=True):
    """float64 evaluation of flip, rotation (with the fp32 c and s the reference's matrix holds), scale and shift of xy [n, 2] -> [n, 2]"""
    fa, fb, c, s, _, scale, _ = constants(params)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    if fa:
        y = -y
    if fb:
        x = -x
    c, s, scale = float(c), float(s), float(scale)
    return np.stack([(x * c + y * s) * scale + t_xy[0], (-x * s + y * c) * scale + t_xy[1]], 1)


def bound(xy_in, result, params, t_xy=(0.0, 0.0)):
    """4 u M per entry, M = scale (|x| + |y|) + |t| + |result|: the rotation is three roundings (<= 2 u (|x| + |y|), whichever way the
    products are fused), scale and shift add one each"""
    scale = abs(float(F32(params[3])))
    m = scale * (np.abs(xy_in[:, 0].astype(np.float64)) + np.abs(xy_in[:, 1].astype(np.float64)))
    return 4 * U * (m[:, None] + np.abs(np.asarray(t_xy, np.float64))[None, :] + np.abs(result.astype(np.float64)))
