"""NumPy restatement of fd_augment_mask (include/futuredet_hip.h) and of the host's record building: get_mask of the reference
(det3d/datasets/pipelines/preprocess.py:75-90) with cv2's getRotationMatrix2D and classic fixed-point warpAffine (INTER_LINEAR, constant
border 0) written out.  Every fp32 product and sum is rounded on its own, the coordinates are float64 -> int32 fixed point."""
import numpy as np

SIZE = 180
BITS, TAB = 10, 32  # AB_BITS = 10, INTER_TAB_SIZE = 32


def rotation_matrix(cx, cy, angle_deg, scale):
    """cv2.getRotationMatrix2D, float64 [6]"""
    a = angle_deg * (np.pi / 180.0)
    al, be = np.cos(a) * scale, np.sin(a) * scale
    return np.array([al, be, (1 - al) * cx - be * cy, -be, al, be * cx + (1 - al) * cy], np.float64)


def invert(m):
    """warpAffine's inversion of a forward matrix, float64 [6]"""
    m = np.asarray(m, np.float64).reshape(-1).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def matrices(params):
    """(flip_a, flip_b, m1, m2) of one sample's parameters [7]: the two INVERSE matrices the kernel takes"""
    p = np.asarray(params, np.float64)
    m1 = invert(rotation_matrix(SIZE // 2, SIZE // 2, np.degrees(-p[2]), p[3]))
    m2 = invert([1.0, 0.0, float(np.float32(p[4])), 0.0, 1.0, float(np.float32(p[5]))])
    return bool(p[0]), bool(p[1]), m1, m2


def warp(src, m):
    """src [H, W] fp32, m the inverse matrix [6]"""
    src = np.asarray(src, np.float32)
    H, W = src.shape
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    ax = np.rint(m[0] * x * 1024.0).astype(np.int64)
    bx = np.rint(m[3] * x * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (X0[:, None] + ax[None, :]) >> 5, (Y0[:, None] + bx[None, :]) >> 5
    sx, sy = X >> 5, Y >> 5
    one, n = np.float32(1), np.float32(TAB)
    fx, fy = (X & 31).astype(np.float32) / n, (Y & 31).astype(np.float32) / n
    w00, w01, w10, w11 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok, src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], np.float32(0))

    out = tap(sy, sx) * w00
    out = out + tap(sy, sx + 1) * w01
    out = out + tap(sy + 1, sx) * w10
    out = out + tap(sy + 1, sx + 1) * w11
    assert out.dtype == np.float32
    return out


def get_mask_plane(plane, params):
    fa, fb, m1, m2 = matrices(params)
    p = np.asarray(plane, np.float32)
    if fa:
        p = p[:, ::-1]
    if fb:
        p = p[::-1]
    return warp(warp(p, m1), m2)


def get_mask(maps, params):
    """maps [B, C, H, W] fp32, params [B, 7] -> the warped maps"""
    maps = np.asarray(maps, np.float32)
    return np.stack([np.stack([get_mask_plane(maps[b, c], params[b]) for c in range(maps.shape[1])]) for b in range(maps.shape[0])])
