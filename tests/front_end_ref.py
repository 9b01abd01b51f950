"""Plain numpy references of the input stage (voxel mean, index row order, strided-conv output set, bf16 rounding) and the shared
case lists of tests/test_gpu_front_end.py and tests/test_front_end_ref_host.py.  Nothing here calls the HIP library:
test_front_end_ref_host.py checks these helpers against the C oracle and torch on the CPU."""
import numpy as np

# (ksize, stride, pad) of the backbone's four strided convolutions (SpMiddleResNetFHD)
BACKBONE_GEOMS = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)),
                  ((3, 1, 1), (2, 1, 1), (0, 0, 0))]

# (ksize, stride, pad, submanifold): the four geometries of the backbone, then the rest of the range fill_dp accepts
# (k in 1..3, s in 1..4, p in 0..2).  ((3,3,3),(1,1,1),(2,2,2)) grows the grid by 2: D <= 62.
RULEBOOK_GEOMS = [((3, 3, 3), (1, 1, 1), (1, 1, 1), True), ((3, 3, 3), (2, 2, 2), (1, 1, 1), False),
                  ((3, 3, 3), (2, 2, 2), (0, 1, 1), False), ((3, 1, 1), (2, 1, 1), (0, 0, 0), False),
                  ((1, 1, 1), (1, 1, 1), (0, 0, 0), False), ((2, 2, 2), (2, 2, 2), (0, 0, 0), False),
                  ((3, 3, 3), (3, 3, 3), (1, 1, 1), False), ((3, 3, 3), (4, 4, 4), (0, 0, 0), False),
                  ((3, 3, 3), (1, 1, 1), (2, 2, 2), False), ((1, 2, 3), (4, 1, 2), (0, 1, 2), False),
                  ((2, 1, 3), (1, 3, 1), (1, 0, 2), False), ((3, 1, 1), (1, 1, 1), (1, 0, 0), True),
                  ((1, 3, 3), (1, 1, 1), (0, 1, 1), True)]


def out_shape(in_shape, ks, st, pd):
    return tuple((int(i) + 2 * p - (k - 1) - 1) // s + 1 for i, k, s, p in zip(in_shape, ks, st, pd))


def col_key(B, H, W, b, y, x):
    """Column number of (b, y, x) in the index's tiled order: 8 x 8 tiles, row-major over (b, tile row, tile column), cells of a
    tile row-major (include/futuredet_hip.h: col = ((b*ceil(H/8) + y/8)*ceil(W/8) + x/8)*64 + (y%8)*8 + x%8)."""
    b, y, x = (np.asarray(v, np.int64) for v in (b, y, x))
    ht, wt = -(-int(H) // 8), -(-int(W) // 8)
    return ((b * ht + y // 8) * wt + x // 8) * 64 + (y % 8) * 8 + x % 8


def index_rows(coords, B, D, H, W):
    """The unique coordinates (b, z, y, x) of ``coords`` in index row order: ascending (col_key, z)."""
    c = np.unique(np.asarray(coords, np.int64).reshape(-1, 4), axis=0)
    assert len(c) == 0 or (c.min() >= 0 and (c.max(0) < np.array([B, D, H, W])).all())
    key = col_key(B, H, W, c[:, 0], c[:, 2], c[:, 3])
    return c[np.lexsort((c[:, 1], key))].astype(np.int32)


def down_set(coords, in_shape, ks, st, pd):
    """Output set of a strided sparse convolution: every o with o*s - p + k = i for an active input i and a tap k, inside the
    output grid.  Brute force over the taps; returns unique rows (b, z, y, x) in lexicographic order."""
    c = np.unique(np.asarray(coords, np.int64).reshape(-1, 4), axis=0)
    osh = out_shape(in_shape, ks, st, pd)
    found = [np.zeros((0, 4), np.int64)]
    for kz in range(ks[0]):
        for ky in range(ks[1]):
            for kx in range(ks[2]):
                num = c[:, 1:] + np.array(pd) - np.array([kz, ky, kx])
                o = num // np.array(st)
                ok = ((num % np.array(st)) == 0).all(1) & (o >= 0).all(1) & (o < np.array(osh)).all(1)
                found.append(np.concatenate([c[ok, :1], o[ok]], 1))
    return np.unique(np.concatenate(found), axis=0).astype(np.int32)


def bf16_rne_bits(x):
    """float32 -> bfloat16 bits (uint16), round to nearest, ties to even; NaN keeps its upper half with the quiet bit set."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    hi, lo = (u >> 16).astype(np.uint32), u & np.uint32(0xFFFF)
    up = (lo > 0x8000) | ((lo == 0x8000) & ((hi & 1) == 1))
    r = hi + up.astype(np.uint32)
    nan = ((u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)) & ((u & np.uint32(0x007FFFFF)) != 0)
    return np.where(nan, hi | np.uint32(0x40), r).astype(np.uint16)


def mean_seq(voxels, num):
    """Per-voxel mean in vox_emit's operation order: a float32 accumulator started at +0.0, slots 0..max_points-1 added in
    order (padding slots included), one float32 divide by the point count."""
    voxels = np.asarray(voxels, np.float32)
    acc = np.zeros((voxels.shape[0], voxels.shape[2]), np.float32)
    for k in range(voxels.shape[1]):
        acc = (acc + voxels[:, k, :]).astype(np.float32)
    return (acc / np.asarray(num).astype(np.float32)[:, None]).astype(np.float32)


def bf16_probe_values(rng, n_random=400):
    """float32 values for the bf16 conversion checks: random, exact ties with odd and even upper halves, +-inf, +-0, the canonical
    quiet NaN, the largest finite float."""
    hi = rng.integers(0x0080, 0x7F00, 200).astype(np.uint32)
    hi[::2] &= ~np.uint32(1)
    hi[1::2] |= np.uint32(1)
    hi[::4] |= np.uint32(0x8000)  # some negative
    ties = ((hi << 16) | np.uint32(0x8000)).view(np.float32)
    special = np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x7FC00000, 0x7F7FFFFF], np.uint32).view(np.float32)
    rand = (rng.standard_normal(n_random) * np.exp(rng.uniform(-20, 20, n_random))).astype(np.float32)
    return np.concatenate([rand, ties, special]).astype(np.float32)


def random_coords(rng, B, D, H, W, density, force_z=()):
    """Shuffled active set (b, z, y, x) int32 of a random occupancy, with the given z planes forced active in one cell each."""
    occ = rng.random((B, D, H, W)) < density
    for i, z in enumerate(force_z):
        occ[i % B, z, (3 * i + 1) % H, (5 * i + 2) % W] = True
    idx = np.argwhere(occ).astype(np.int32)
    rng.shuffle(idx)
    return idx
