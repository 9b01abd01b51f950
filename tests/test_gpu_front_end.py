"""-m gpu: the integer-exact input stage -- voxelizer variants, index pyramid, row placement, rulebook geometry range, densify
variants -- against the sequential C oracle (oracle/ops.py) and the numpy references of front_end_ref.py.  Every comparison is
exact (array_equal / set equality); every input comes from a fixed seed."""
import ctypes

import numpy as np
import pytest
import torch

import front_end_ref as fr

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """bf16 tensor -> uint16 bits on the host."""
    return _np(t.contiguous().view(torch.int16)).view(np.uint16)


def _bf16_dev(bits):
    return _dev(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)


def _bf16_as_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ================================================================================================ 1. voxelizer
VOX_RANGE = [-8.0, -8.0, -2.0, 8.0, 8.0, 2.0]
VOX_SIZES = ([0.25, 0.25, 4.0], [0.25, 0.25, 1.0])  # one z cell / four z cells (the key is decoded across z)
# (ndim, max_points, max_voxels, n): both sides of each vox_emit<16/32/64> boundary, every point width
VOX_CASES = [(3, 1, 5000, 20000), (4, 16, 5000, 20000), (5, 17, 3000, 20000), (6, 20, 2500, 20000), (7, 32, 5000, 40000),
             (8, 33, 2000, 40000), (5, 35, 5000, 40000), (4, 64, 5000, 40000)]
VOX_CAPPED = {(6, 20, 2500), (8, 33, 2000)}  # the reference has more distinct cells than max_voxels there


def _mean_layouts(ndim):
    """(mean_stride, coor_cols): rows through LDS (16), and both reasons for the direct writer (not a multiple of 4; above 16)"""
    return [(ndim, 3), (16, 4), (ndim + 1, 4), (20, 3)]


def _cloud(n, ndim, seed):
    rng = np.random.default_rng(seed)
    pts = np.empty((n, ndim), np.float32)
    pts[:, :2] = rng.normal(0.0, 3.0, (n, 2))
    pts[:, 2] = rng.uniform(-2.5, 2.5, n)
    pts[:, 3:] = rng.uniform(0.0, 1.0, (n, ndim - 3))
    hot = np.arange(0, n, 40)  # one hot cell of n / 40 points near (0.1, 0.1, 0.1)
    pts[hot, :3] = 0.1 + rng.uniform(0.0, 0.05, (len(hot), 3))
    return pts


def _raw_cell_counts(pts, vs):
    lo, hi = np.array(VOX_RANGE[:3], np.float32), np.array(VOX_RANGE[3:], np.float32)
    vs = np.array(vs, np.float32)
    grid = np.round((hi - lo) / vs).astype(np.int64)
    c = np.floor((pts[:, :3] - lo) / vs).astype(np.int64)
    c = c[((c >= 0) & (c < grid)).all(1)]
    return np.unique((c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0], return_counts=True)[1]


@pytest.mark.parametrize("vsz", [0, 1])
@pytest.mark.parametrize("case", VOX_CASES, ids=lambda c: "nd%d-mp%d-mv%d" % c[:3])
def test_voxelizer_emit_widths_and_mean_paths_vs_oracle(hip, case, vsz):
    """voxels / coors / num / count identical to the sequential oracle and the fused mean bit-identical to mean_seq, for every
    vox_emit width, point width, mean writer and coordinate width, with and without the voxel output (single-point shortcut)."""
    from oracle import ops as oops

    ndim, mp, mv, n = case
    vs = VOX_SIZES[vsz]
    pts = _cloud(n, ndim, seed=100 + ndim * 64 + mp)
    rv, rc, rn = oops.points_to_voxel(pts, vs, VOX_RANGE, mp, True, mv)
    # the recipe must keep reaching the paths this test is about
    assert rn.max() == mp
    assert (rn == 1).any()
    if mp > 2:
        assert ((rn > 1) & (rn < mp)).any()
    assert _raw_cell_counts(pts, vs).max() > 64
    if case[:3] in VOX_CAPPED:
        assert len(rn) == mv
    m = len(rn)
    ref_mean = fr.mean_seq(rv, rn)
    dpts = _dev(pts)
    for batch_idx, (stride, cols) in enumerate(_mean_layouts(ndim)):
        a = hip.voxelize(dpts, vs, VOX_RANGE, mp, mv, batch_idx=batch_idx, want_voxels=True, want_mean=True, mean_stride=stride, coor_cols=cols)
        b = hip.voxelize(dpts, vs, VOX_RANGE, mp, mv, batch_idx=batch_idx, want_voxels=False, want_mean=True, mean_stride=stride, coor_cols=cols)
        assert "voxels" not in b
        for out in (a, b):
            assert int(out["num_voxels"].cpu()[0]) == m
            co = _np(out["coors"][:m])
            assert co.shape[1] == cols
            if cols == 4:
                assert np.all(co[:, 0] == batch_idx)
            assert np.array_equal(co[:, cols - 3:], rc)
            assert np.array_equal(_np(out["num_points"][:m]), rn)
            mean = _np(out["mean"][:m])
            assert mean.shape[1] == stride
            assert np.array_equal(mean[:, :ndim], ref_mean)
            assert np.all(mean[:, ndim:] == 0)
        assert np.array_equal(_np(a["voxels"][:m]), rv)
        assert np.array_equal(_np(a["mean"][:m]), _np(b["mean"][:m])) and np.array_equal(_np(a["coors"][:m]), _np(b["coors"][:m]))


F_SENT, I_SENT = -7.5, -9


def _sentinel_out(mv, mp, ndim, stride, cols):
    dev = torch.device("cuda")
    return dict(voxels=torch.full((mv, mp, ndim), F_SENT, dtype=torch.float32, device=dev),
                mean=torch.full((mv, stride), F_SENT, dtype=torch.float32, device=dev),
                coors=torch.full((mv, cols), I_SENT, dtype=torch.int32, device=dev),
                num_points=torch.full((mv,), I_SENT, dtype=torch.int32, device=dev),
                num_voxels=torch.full((1,), I_SENT, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("stride,cols", [(16, 4), (5, 3)], ids=["lds", "direct"])
def test_voxelizer_device_point_count(hip, stride, cols):
    """n_points_dev over a padded buffer: the first n rows alone count, rows past num_voxels of every output keep their
    sentinel (also when the mean leaves through LDS), 0 points write nothing but the count, a count above the buffer is clamped."""
    from oracle import ops as oops

    ndim, mp, mv, n, extra = 5, 17, 5000, 20000, 5000
    vs = VOX_SIZES[0]
    rng = np.random.default_rng(77)
    pts = _cloud(n, ndim, seed=5)
    pad = rng.uniform(0.0, 1.0, (extra, ndim)).astype(np.float32)
    pad[:, :2] = rng.uniform(-7.9, 7.9, (extra, 2))  # in range, spread evenly: most land in cells the cloud leaves empty
    pad[:, 2] = rng.uniform(-1.9, 1.9, extra)
    buf = np.concatenate([pts, pad])
    rv, rc, rn = oops.points_to_voxel(pts, vs, VOX_RANGE, mp, True, mv)
    fv, fc, fn = oops.points_to_voxel(buf, vs, VOX_RANGE, mp, True, mv)
    m = len(rn)
    assert m + 500 < len(fn) <= mv, "the padding rows must create new voxels"
    dbuf = _dev(buf)

    def run(count):
        out = _sentinel_out(mv, mp, ndim, stride, cols)
        hip.voxelize(dbuf, vs, VOX_RANGE, mp, mv, batch_idx=1, want_voxels=True, want_mean=True, coor_cols=cols, out=out,
                     n_points_dev=torch.tensor([count], dtype=torch.int32, device="cuda"))
        return {k: _np(v) for k, v in out.items()}

    def check(out, v, c, num):
        k = len(num)
        assert out["num_voxels"][0] == k
        assert np.array_equal(out["voxels"][:k], v) and np.array_equal(out["num_points"][:k], num)
        assert np.array_equal(out["coors"][:k, cols - 3:], c)
        if cols == 4:
            assert np.all(out["coors"][:k, 0] == 1)
        assert np.array_equal(out["mean"][:k, :ndim], fr.mean_seq(v, num)) and np.all(out["mean"][:k, ndim:] == 0)
        assert np.all(out["voxels"][k:] == F_SENT) and np.all(out["mean"][k:] == F_SENT)
        assert np.all(out["coors"][k:] == I_SENT) and np.all(out["num_points"][k:] == I_SENT)

    check(run(n), rv, rc, rn)
    alone = _sentinel_out(mv, mp, ndim, stride, cols)
    hip.voxelize(_dev(pts), vs, VOX_RANGE, mp, mv, batch_idx=1, want_voxels=True, want_mean=True, coor_cols=cols, out=alone)
    check({k: _np(v) for k, v in alone.items()}, rv, rc, rn)
    check(run(0), rv[:0], rc[:0], rn[:0])
    check(run(len(buf) + 12345), fv, fc, fn)
    check(run(2 ** 31 - 1), fv, fc, fn)


def test_voxelizer_all_single_point_voxels(hip, golden):
    """Every voxel holds one point (the placement pass is skipped on the device, vox_emit reads the first points): the mean IS the
    point, bit for bit."""
    from oracle import ops as oops

    g = golden("voxelizer.npz")
    cfg = g["edges_cfg"]
    vs, rg = cfg[:3], cfg[3:9]
    pts = np.ascontiguousarray(g["edges_voxels"][:, 0, :])  # the first point of every voxel of the 'edges' cloud
    rv, rc, rn = oops.points_to_voxel(pts, vs, rg, 10, True, 160000)
    assert len(rn) == len(pts) > 1000 and rn.max() == 1 and np.array_equal(rv[:, 0, :], pts)
    for stride, cols in ((16, 4), (5, 3)):
        out = hip.voxelize(_dev(pts), vs, rg, 10, 160000, batch_idx=2, want_voxels=False, want_mean=True, mean_stride=stride, coor_cols=cols)
        m = int(out["num_voxels"].cpu()[0])
        assert m == len(pts)
        mean = _np(out["mean"][:m])
        assert np.array_equal(mean[:, :5].view(np.uint32), (pts + np.float32(0.0)).view(np.uint32)) and np.all(mean[:, 5:] == 0)
        assert np.array_equal(_np(out["coors"][:m])[:, cols - 3:], rc) and np.all(_np(out["num_points"][:m]) == 1)


@pytest.mark.parametrize("n", [682, 683, 684])
def test_voxelizer_hash_table_boundary(hip, n):
    """vox_layout doubles its 1024-slot table while 2*slots < 3*n: 682 points still share 1024 slots (the highest load factor the
    table ever sees), 683 and 684 get 2048.  All points in distinct cells."""
    from oracle import ops as oops

    rng = np.random.default_rng(n)
    cells = rng.choice(64 * 64, n, replace=False)
    pts = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
    pts[:, 0] = -8.0 + 0.25 * (cells % 64) + rng.uniform(0.05, 0.2, n)
    pts[:, 1] = -8.0 + 0.25 * (cells // 64) + rng.uniform(0.05, 0.2, n)
    pts[:, 2] = rng.uniform(-1.9, 1.9, n)
    vs = VOX_SIZES[0]
    rv, rc, rn = oops.points_to_voxel(pts, vs, VOX_RANGE, 5, True, 1000)
    assert len(rn) == n and rn.max() == 1
    out = hip.voxelize(_dev(pts), vs, VOX_RANGE, 5, 1000, want_voxels=True, want_mean=True, mean_stride=4, coor_cols=3)
    assert int(out["num_voxels"].cpu()[0]) == n
    assert np.array_equal(_np(out["voxels"][:n]), rv) and np.array_equal(_np(out["coors"][:n]), rc)
    assert np.array_equal(_np(out["num_points"][:n]), rn) and np.array_equal(_np(out["mean"][:n]), fr.mean_seq(rv, rn))


# ================================================================================================ 2. build_pyramid
PYR_GRIDS = {"small": (2, 41, 50, 44), "deep": (3, 64, 24, 17)}
PYR_NMAX = 600
PYR_COUNTS = {("small", 0): (500, 317), ("small", 1): (0, 317), ("deep", 0): (300, 450, 123), ("deep", 1): (300, 0, 123)}


def _pyramid_input(grid, variant):
    """coors [B * n_max, 4] and nvox [B] as the voxelizer leaves them: sample b's voxels in rows b * n_max ..., the rows past its count
    hold other in-range cells (which must be ignored).  Columns are reused so that level-0 words hold several bits."""
    B, D, H, W = PYR_GRIDS[grid]
    counts = PYR_COUNTS[(grid, variant)]
    rng = np.random.default_rng(31 + 7 * variant + D)
    coors = np.zeros((B * PYR_NMAX, 4), np.int32)
    for b in range(B):
        cols = rng.choice(H * W, 220, replace=False)
        cell = rng.choice(220 * D, PYR_NMAX, replace=False)  # distinct (column, z)
        col, z = cols[cell // D], cell % D
        if not (z[:max(counts[b], 1)] == 0).any():
            z[0] = 0  # (may duplicate a cell: the index is a set)
        if not (z[:max(counts[b], 1)] == D - 1).any():
            z[min(1, PYR_NMAX - 1)] = D - 1
        coors[b * PYR_NMAX:(b + 1) * PYR_NMAX] = np.stack([np.full(PYR_NMAX, b), z, col // W, col % W], 1)
    live = np.concatenate([coors[b * PYR_NMAX:b * PYR_NMAX + counts[b]] for b in range(B)])
    return coors, np.array(counts, np.int32), live


def _eager_chain(hip, coors, nvox, B, shape0, geoms):
    dev = torch.device("cuda")
    ix = hip.SparseIndex(B, shape0[0], shape0[1], shape0[2], dev)
    for b in range(B):
        ix.mark(coors[b * PYR_NMAX:(b + 1) * PYR_NMAX], n_dev=nvox[b:b + 1], n_max=PYR_NMAX)
    levels = [ix]
    for ks, st, pd in geoms:
        levels.append(levels[-1].downsample(ks, st, pd))
    for ix in levels:
        nd = torch.zeros(1, dtype=torch.int32, device=dev)
        ix.scan(nd)
        ix.finalize(int(nd.cpu()[0]))
    return levels


@pytest.fixture(scope="module")
def cache():
    """Inputs, references and eager indexes shared by the tests of this module: each entry is built by whichever test asks for
    it first and never changed afterwards; the device tensors are dropped with the module."""
    c = {}
    yield c
    c.clear()


def _pyramid_case(hip, cache, grid, variant):
    """Input, oracle row tables and the eager (step-by-step) levels of one case; computed once, read by several tests."""
    key = (grid, variant)
    if key not in cache:
        B, D, H, W = PYR_GRIDS[grid]
        coors, counts, live = _pyramid_input(grid, variant)
        want, shapes, cur = [], [(D, H, W)], live
        for geom in [None] + fr.BACKBONE_GEOMS:
            if geom is not None:
                cur = fr.down_set(cur, shapes[-1], *geom)
                shapes.append(fr.out_shape(shapes[-1], *geom))
            want.append(fr.index_rows(cur, B, *shapes[-1]))
        dcoors, dnvox = _dev(coors), _dev(counts)
        eager = _eager_chain(hip, dcoors, dnvox, B, (D, H, W), fr.BACKBONE_GEOMS)
        cache[key] = dict(coors=dcoors, nvox=dnvox, live=live, want=want, shapes=shapes, eager=eager)
    return cache[key]


@pytest.mark.parametrize("variant", [0, 1], ids=["all", "one-empty"])
@pytest.mark.parametrize("grid", ["small", "deep"])
def test_build_pyramid_matches_eager_chain_and_oracle(hip, cache, grid, variant):
    B, D, H, W = PYR_GRIDS[grid]
    case = _pyramid_case(hip, cache, grid, variant)
    assert (case["live"][:, 1] == 0).any() and (case["live"][:, 1] == D - 1).any()
    idx = hip.build_pyramid(case["coors"], case["nvox"], PYR_NMAX, B, (D, H, W), fr.BACKBONE_GEOMS, torch.device("cuda"), static=False)
    assert len(idx) == 5
    for l, (ix, eg, want) in enumerate(zip(idx, case["eager"], case["want"])):
        assert tuple(ix.spatial_shape) == tuple(eg.spatial_shape) == case["shapes"][l]
        assert ix.n == eg.n == len(want) and int(ix.n_dev.cpu()[0]) == len(want)
        assert torch.equal(ix.words, eg.words) and torch.equal(ix.prefix, eg.prefix) and torch.equal(ix.coords, eg.coords)
        assert np.array_equal(_np(ix.coords), want), "level %d: rows must be the oracle's set in (col_key, z) order" % l
        assert grid != "small" or all(s % 8 != 0 for s in case["shapes"][l][1:])


@pytest.mark.parametrize("grid", ["small", "deep"])
def test_build_pyramid_static_and_row_caps(hip, cache, grid):
    """static=True writes the coordinates inside the scan (idx_scan3_ml<true>) into capacity-sized tables; with a capacity below
    the count the level reports the overflow, keeps its first rows and does not write into the next level's slice."""
    B, D, H, W = PYR_GRIDS[grid]
    case = _pyramid_case(hip, cache, grid, 0)
    true = [len(w) for w in case["want"]]
    dev = torch.device("cuda")
    idx = hip.build_pyramid(case["coors"], case["nvox"], PYR_NMAX, B, (D, H, W), fr.BACKBONE_GEOMS, dev, static=True)
    caps = hip._PyramidPlan(B, (D, H, W), fr.BACKBONE_GEOMS, dev).row_caps(B * PYR_NMAX)
    assert idx[0].level_counts.cpu().tolist() == true
    for ix, eg, cap, n in zip(idx, case["eager"], caps, true):
        assert ix.static and ix.n == cap >= n and tuple(ix.coords.shape) == (cap, 4)
        assert torch.equal(ix.coords[:n], eg.coords) and torch.equal(ix.words, eg.words) and torch.equal(ix.prefix, eg.prefix)
    small = list(true)
    small[2] -= 10
    idx = hip.build_pyramid(case["coors"], case["nvox"], PYR_NMAX, B, (D, H, W), fr.BACKBONE_GEOMS, dev, static=True, row_caps=small)
    counts = idx[0].level_counts.cpu().tolist()
    assert counts == true and counts[2] > idx[2].n == small[2]
    for l, (ix, eg) in enumerate(zip(idx, case["eager"])):
        assert ix.n == small[l]
        assert torch.equal(ix.coords, eg.coords[:small[l]]), "level %d" % l
    # levels 2, 3, 4 are consecutive slices of one allocation: level 3 starts where level 2's capacity ends
    assert idx[3].coords.data_ptr() == idx[2].coords.data_ptr() + 16 * small[2]


def test_index_scan_across_blocks_and_lookup_bounds(hip):
    """541 696 columns = 265 scan blocks (more than one pass of idx_scan2): the prefix must carry across blocks and passes, in the
    step-by-step scan and in the pyramid's fused scan; lookups outside the grid return -1 in every field."""
    B, D, H, W = 1, 4, 733, 736
    dev = torch.device("cuda")
    rng = np.random.default_rng(9)
    cells = rng.choice(B * D * H * W, 20000 + 1000, replace=False)
    allc = np.stack(np.unravel_index(cells, (B, D, H, W)), 1).astype(np.int32)
    act, inactive = allc[:20000], allc[20000:]
    assert hip.SparseIndex(B, D, H, W, dev).ncols == 541696
    want = fr.index_rows(act, B, D, H, W)
    assert len(want) == 20000
    last_col = fr.col_key(B, H, W, want[-1, 0], want[-1, 2], want[-1, 3])
    assert last_col // 2048 > 256, "rows must live past the first 256 scan blocks"
    dact = _dev(act)
    eager = hip.SparseIndex(B, D, H, W, dev)
    eager.mark(dact)
    nd = torch.zeros(1, dtype=torch.int32, device=dev)
    eager.scan(nd)
    eager.finalize(int(nd.cpu()[0]))
    pyr = hip.build_pyramid(dact, _dev(np.array([20000], np.int32)), 20000, B, (D, H, W), [], dev, static=False)[0]
    outside = []
    for b, z, y, x in [(-1, 1, 5, 5), (B, 1, 5, 5), (0, -1, 5, 5), (0, D, 5, 5), (0, 1, 5, -1), (0, 1, 5, W)]:
        outside.append((b, z, y, x))
    outside += [(0, z, y, x) for y in (H, H + 1, 735) for z in (0, 3) for x in (0, 377, W - 1)]
    outside = np.array(outside, np.int32)
    arange = torch.arange(20000, dtype=torch.int32, device=dev)
    for ix in (eager, pyr):
        assert ix.n == 20000
        assert np.array_equal(_np(ix.coords), want)
        assert torch.equal(ix.lookup(ix.coords), arange)
        assert torch.all(ix.lookup(_dev(inactive)) == -1)
        assert torch.all(ix.lookup(_dev(outside)) == -1)
    assert torch.equal(eager.words, pyr.words) and torch.equal(eager.prefix, pyr.prefix)


# ================================================================================================ 3. rulebook geometry range
def _finalized(hip, ix):
    nd = torch.zeros(1, dtype=torch.int32, device="cuda")
    ix.scan(nd)
    ix.finalize(int(nd.cpu()[0]))
    return ix


def _check_rulebook_vs_oracle(hip, geom, grid, idx):
    """The comparison of test_rulebook_matches_oracle_pairs: same (input coord, output coord, tap) triples as the oracle, the output
    shape and count, tail columns == -1; plus the row order of both indexes."""
    from oracle import ops as oops

    ks, st, pd, subm = geom
    B, D, H, W = grid
    o_idx, pairs, pnum, oshape = oops.rulebook(idx, (D, H, W), ks, st, pd, subm)
    src = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    src.mark(_dev(idx))
    _finalized(hip, src)
    assert src.n == len(idx)
    dst = src if subm else _finalized(hip, src.downsample(ks, st, pd))
    assert dst.spatial_shape == list(oshape)
    assert dst.n == len(o_idx)
    co_in, co_out = _np(src.coords), _np(dst.coords)
    assert np.array_equal(co_in, fr.index_rows(idx, B, D, H, W))
    assert np.array_equal(co_out, fr.index_rows(o_idx, B, *dst.spatial_shape))
    nbr = _np(src.rulebook(dst, ks, st, pd))
    assert nbr.shape[0] == ks[0] * ks[1] * ks[2] and np.all(nbr[:, dst.n:] == -1)
    got = set()
    for k in range(nbr.shape[0]):
        for o in np.nonzero(nbr[k, :dst.n] >= 0)[0]:
            got.add((tuple(co_in[nbr[k, o]]), tuple(co_out[o]), k))
    want = set()
    for k in range(len(pnum)):
        for t in range(pnum[k]):
            want.add((tuple(idx[pairs[k, 0, t]]), tuple(o_idx[pairs[k, 1, t]]), k))
    assert len(want) > 0 and got == want


@pytest.mark.parametrize("geom", fr.RULEBOOK_GEOMS, ids=lambda g: "k%d%d%d-s%d%d%d-p%d%d%d%s" % (g[0] + g[1] + g[2] + ("-subm" if g[3] else "",)))
def test_rulebook_geometry_range_deep_grid(hip, geom):
    """D = 62 at 25 % density with z = 0 and z = 61 active: column words with high bits, every accepted (k, s, p) combination of the
    list (the pad-2 geometry fills a 64-deep output)."""
    grid = (2, 62, 9, 8)
    idx = fr.random_coords(np.random.default_rng(13), *grid, 0.25, force_z=(0, 61, 0, 61))
    assert (idx[:, 1] == 0).any() and (idx[:, 1] == 61).any()
    _check_rulebook_vs_oracle(hip, geom, grid, idx)


def test_rulebook_strided_on_64_deep_grid(hip):
    """D = 64: bit 63 of a column word, and idx_down's tap mask shifted to the top of the word."""
    grid = (1, 64, 8, 8)
    idx = fr.random_coords(np.random.default_rng(14), *grid, 0.25, force_z=(63, 0, 63, 62))
    assert (idx[:, 1] == 63).any()
    _check_rulebook_vs_oracle(hip, ((3, 3, 3), (2, 2, 2), (1, 1, 1), False), grid, idx)
    _check_rulebook_vs_oracle(hip, ((3, 3, 3), (1, 1, 1), (1, 1, 1), True), grid, idx)


@pytest.mark.parametrize("geom", [fr.RULEBOOK_GEOMS[0], fr.RULEBOOK_GEOMS[1], fr.RULEBOOK_GEOMS[9]], ids=["subm", "strided", "mixed"])
def test_rulebook_scalar_store_path_through_c_abi(hip, geom):
    """fd_rulebook with a row stride that is no multiple of 4, and with a table that does not start on 16 bytes, takes the 4-byte
    store path: same table as the 16-byte path, tail included."""
    from futuredet_amd import lib

    L = lib.load()
    ks, st, pd, subm = geom
    B, D, H, W = 2, 11, 21, 19
    idx = fr.random_coords(np.random.default_rng(7), B, D, H, W, 0.12)
    src = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    src.mark(_dev(idx))
    _finalized(hip, src)
    dst = src if subm else _finalized(hip, src.downsample(ks, st, pd))
    ref = src.rulebook(dst, ks, st, pd)  # stride a multiple of 64, aligned: the vector path
    K, n_out = ref.shape[0], dst.n
    arr = lambda v: (ctypes.c_int * 3)(*v)  # noqa: E731
    odd = n_out | 1
    for stride, offset in ((odd, 0), (odd, 1), (ref.shape[1], 1)):
        flat = torch.full((K * stride + 8,), 12345, dtype=torch.int32, device="cuda")
        nbr = flat[offset:offset + K * stride]
        assert (nbr.data_ptr() % 16 == 0) == (offset == 0)
        hip.check(L.fd_rulebook(hip._p(src.words), hip._p(src.prefix), B, D, H, W, hip._p(dst.coords), n_out, hip._p(dst.n_dev), stride, 1,
                                arr(ks), arr(st), arr(pd), hip._p(nbr), hip._stream()), "fd_rulebook")
        table = nbr.view(K, stride)
        assert torch.equal(table[:, :n_out], ref[:, :n_out]) and torch.all(table[:, n_out:] == -1)
        assert torch.all(flat[:offset] == 12345) and torch.all(flat[offset + K * stride:] == 12345)


# ================================================================================================ 4. fd_rows_place
PLACE_CASES = [(5, 16), (5, 8), (5, 5), (3, 6), (4, 4)]
BF16_SENT = 0x4242


def _place_setup(hip, cache):
    case = _pyramid_case(hip, cache, "small", 0)
    index = case["eager"][0]
    want = case["want"][0]
    row_of = {tuple(c): i for i, c in enumerate(want)}
    B, D, H, W = PYR_GRIDS["small"]
    rng = np.random.default_rng(21)
    occupied = np.zeros((B, D, H, W), bool)
    occupied[tuple(want.T)] = True
    free = np.argwhere(~occupied).astype(np.int32)
    missing = free[rng.choice(len(free), 40, replace=False)]
    coords = np.concatenate([want, missing])
    rng.shuffle(coords)
    return index, coords, row_of


def _place_reference(coords, src, row_of, n_rows, c_dst, count, sentinel):
    """dst[row_of[c], :c_src] = src[i], padding channels 0, untouched rows keep the sentinel (float32 values; NaN-free sentinel)"""
    ref = np.full((n_rows, c_dst), sentinel, np.float32)
    for i in range(count):
        r = row_of.get(tuple(coords[i]))
        if r is not None:
            ref[r] = 0.0
            ref[r, :src.shape[1]] = src[i]
    return ref


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c_src,c_dst", PLACE_CASES)
def test_rows_place_all_kernels(hip, cache, c_src, c_dst, dtype, offset):
    """rows_place4 (c_dst % 4 == 0, 16-byte aligned rows) and the scalar rows_place (other widths, or a destination view offset by
    one element), fp32 and bf16, with a device count below n_max and coordinates that are not in the index."""
    index, coords, row_of = _place_setup(hip, cache)
    n_max, n_rows = len(coords), index.n + 5
    rng = np.random.default_rng(c_src * 100 + c_dst)
    src = rng.standard_normal((n_max, c_src)).astype(np.float32)
    probe = fr.bf16_probe_values(rng)
    src.reshape(-1)[:2 * len(probe)] = np.concatenate([probe[::-1], probe])  # ties, +-inf, +-0, quiet NaN, max float among the values
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    sent = 77.0 if dtype == "f32" else float(_bf16_as_f32([BF16_SENT])[0])
    for count in (n_max, n_max - 213):
        flat = torch.full((n_rows * c_dst + 8,), sent, dtype=tdt, device="cuda")
        dst = flat[offset:offset + n_rows * c_dst].view(n_rows, c_dst)
        n_dev = None if count == n_max else torch.tensor([count], dtype=torch.int32, device="cuda")
        got = hip.rows_place(index, _dev(coords), _dev(src), c_dst, tdt, n_dev=n_dev, out=dst)
        assert got.data_ptr() == dst.data_ptr()
        ref = _place_reference(coords, src, row_of, n_rows, c_dst, count, sent)
        assert np.isnan(ref).any() and np.isinf(ref).any() and (ref == np.float32(3.4028235e38)).any()  # the special values were placed
        dropped = sum(1 for c in coords[count:] if tuple(c) in row_of)  # index rows whose voxel lies beyond the device count
        assert np.all(ref[index.n:] == sent) and (ref[:index.n, 0] == sent).sum() == dropped and (dropped > 150) == (count < n_max)
        if dtype == "f32":
            assert np.array_equal(_np(dst).view(np.uint32), ref.view(np.uint32))
            assert np.all(_np(flat[:offset]) == sent) and np.all(_np(flat[offset + n_rows * c_dst:]) == sent)
        else:
            assert np.array_equal(_bits(dst), fr.bf16_rne_bits(ref))
            assert np.all(_bits(flat[:offset]) == BF16_SENT) and np.all(_bits(flat[offset + n_rows * c_dst:]) == BF16_SENT)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c_src,c_dst", PLACE_CASES)
def test_rows_permute_after_lookup_matches_rows_place(hip, cache, c_src, c_dst, dtype):
    index, coords, row_of = _place_setup(hip, cache)
    rng = np.random.default_rng(c_src * 100 + c_dst + 1)
    src = rng.standard_normal((len(coords), c_src)).astype(np.float32)
    probe = fr.bf16_probe_values(rng)
    src.reshape(-1)[:2 * len(probe)] = np.concatenate([probe[::-1], probe])
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    rows = index.lookup(_dev(coords))
    want_rows = np.array([row_of.get(tuple(c), -1) for c in coords], np.int32)
    assert np.array_equal(_np(rows), want_rows) and (want_rows < 0).sum() == 40
    got = hip.rows_permute(_dev(src), rows, c_dst, tdt, n_rows=index.n)
    ref = _place_reference(coords, src, row_of, index.n, c_dst, len(coords), 0.0)
    if dtype == "f32":
        assert np.array_equal(_np(got).view(np.uint32), ref.view(np.uint32))
    else:
        assert np.array_equal(_bits(got), fr.bf16_rne_bits(ref))


# ================================================================================================ 5. densify
DENSE_GRIDS = {"d2": (2, 2, 7, 6), "d5": (2, 5, 20, 28)}  # the geometry of the small pyramid's last level; D = 5, H and W no multiples of 8


def _dense_index(hip, cache, which):
    """(index, rows in index order) of a random active set on DENSE_GRIDS[which]; built once"""
    key = ("dense", which)
    if key not in cache:
        B, D, H, W = DENSE_GRIDS[which]
        assert which != "d2" or (D, H, W) == fr.out_shape(fr.out_shape(fr.out_shape(fr.out_shape(
            PYR_GRIDS["small"][1:], *fr.BACKBONE_GEOMS[0]), *fr.BACKBONE_GEOMS[1]), *fr.BACKBONE_GEOMS[2]), *fr.BACKBONE_GEOMS[3])
        idx = fr.random_coords(np.random.default_rng(3), B, D, H, W, 0.4 if which == "d2" else 0.3)
        ix = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
        ix.mark(_dev(idx))
        _finalized(hip, ix)
        assert ix.n == len(idx) > 20
        cache[key] = (ix, fr.index_rows(idx, B, D, H, W))
    return cache[key]


def _dense_feats(n, C, in_dtype, seed):
    """(device rows, float32 host values): bf16 rows hold bf16-representable values, so every result is exact"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, C)).astype(np.float32)
    if in_dtype == "bf16":
        bits = fr.bf16_rne_bits(f)
        return _bf16_dev(bits), _bf16_as_f32(bits)
    return _dev(f), f


def _dense_reference(feats, rows, index):
    from oracle import ops as oops

    d = oops.dense(feats, rows, index.B, index.spatial_shape)  # [B, C, D, H, W]
    return d.reshape(index.B, feats.shape[1] * index.D, index.H, index.W)


def _assert_dense_equal(out, ref):
    if out.dtype == torch.float32:
        assert np.array_equal(_np(out), ref)
    else:
        assert np.array_equal(_bits(out), fr.bf16_rne_bits(ref))


# (index, C): chunks = 2 and 4 of the tile kernel (the 128 x 2 map of the model), D = 5 (not a power of two; two chunks of 80
# channels), and 24 x 5 = one chunk
@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("which,C", [("d2", 128), ("d2", 256), ("d5", 32), ("d5", 24)])
def test_densify_nchw_tile_kernel(hip, cache, which, C, in_dtype):
    index, rows = _dense_index(hip, cache, which)
    feats, host = _dense_feats(index.n, C, in_dtype, seed=C)
    ref = _dense_reference(host, rows, index)
    assert (ref != 0).any()
    out = hip.densify(feats, index, out_dtype=torch.float32)
    assert out.is_contiguous()
    _assert_dense_equal(out, ref)
    # overflow guard: only the first n - 7 rows exist -> the cells of the last 7 rows read as 0, every other cell is unchanged
    cut = host.copy()
    cut[index.n - 7:] = 0
    _assert_dense_equal(hip.densify(feats[:index.n - 7].contiguous(), index, out_dtype=torch.float32), _dense_reference(cut, rows, index))


@pytest.mark.parametrize("out_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("which,C", [("d2", 128), ("d5", 32)])
def test_densify_channels_last_vector_kernels(hip, cache, which, C, in_dtype, out_dtype):
    index, rows = _dense_index(hip, cache, which)
    assert (C * index.D) % 8 == 0
    feats, host = _dense_feats(index.n, C, in_dtype, seed=C + 1)
    odt = torch.float32 if out_dtype == "f32" else torch.bfloat16
    out = hip.densify(feats, index, out_dtype=odt, channels_last=True)
    assert out.is_contiguous(memory_format=torch.channels_last) and out.dtype == odt
    _assert_dense_equal(out, _dense_reference(host, rows, index))
    cut = host.copy()
    cut[index.n - 7:] = 0
    _assert_dense_equal(hip.densify(feats[:index.n - 7].contiguous(), index, out_dtype=odt, channels_last=True), _dense_reference(cut, rows, index))


@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("layout", ["nhwc-cd12-bf16", "nchw-bf16", "slice-f32", "slice-bf16"])
def test_densify_generic_kernel(hip, cache, layout, in_dtype):
    """The element-wise fallback: channels-last with C*D = 12 (no multiple of 8) and bf16 out, NCHW bf16 out, and a pre-allocated
    channel slice of a wider channels-last tensor that does not start on 16 bytes (everything outside the slice keeps a sentinel)."""
    which, C = ("d2", 6) if layout == "nhwc-cd12-bf16" else ("d5", 32)
    index, rows = _dense_index(hip, cache, which)
    feats, host = _dense_feats(index.n, C, in_dtype, seed=C + 2)
    ref = _dense_reference(host, rows, index)
    cut = host.copy()
    cut[index.n - 7:] = 0
    ref_cut = _dense_reference(cut, rows, index)
    short = feats[:index.n - 7].contiguous()
    if layout == "nhwc-cd12-bf16":
        assert C * index.D == 12
        _assert_dense_equal(hip.densify(feats, index, out_dtype=torch.bfloat16, channels_last=True), ref)
        _assert_dense_equal(hip.densify(short, index, out_dtype=torch.bfloat16, channels_last=True), ref_cut)
    elif layout == "nchw-bf16":
        out = hip.densify(feats, index, out_dtype=torch.bfloat16)
        assert out.is_contiguous()
        _assert_dense_equal(out, ref)
        _assert_dense_equal(hip.densify(short, index, out_dtype=torch.bfloat16), ref_cut)
    else:
        odt = torch.float32 if layout == "slice-f32" else torch.bfloat16
        CD = C * index.D
        for f, r in ((feats, ref), (short, ref_cut)):
            wide = torch.full((index.B, CD + 8, index.H, index.W), 3.0, dtype=odt, device="cuda").contiguous(memory_format=torch.channels_last)
            out = wide[:, 1:1 + CD]
            assert out.data_ptr() % 16 != 0 and out.stride(1) == 1
            assert hip.densify(f, index, out=out).data_ptr() == out.data_ptr()
            _assert_dense_equal(out, r)
            assert torch.all(wide[:, :1] == 3.0) and torch.all(wide[:, 1 + CD:] == 3.0)
