"""CPU-only checks of tests/pillars_ref.py, the numpy references of test_gpu_pillars_eval.py and test_gpu_sweeps_edges.py: against
the reference's goldens (pillars.npz, sweeps.npz) and the CPU oracle (oracle/model.py, oracle/ops.py).  No HIP code runs here."""
import numpy as np
import pytest
import torch

import pillars_ref as pr
from parity_util import report

GOLDEN_GEOM = (0.2, 0.2, 0.2 / 2 + -6.4, 0.2 / 2 + -6.4)


def _golden_layers(g, name, n_layers):
    layers = []
    for i in range(n_layers):
        pre = "%s_sd_pfn_layers.%d." % (name, i)
        layers.append(pr.fold_bn(*(g[pre + k] for k in ("linear.weight", "norm.weight", "norm.bias", "norm.running_mean", "norm.running_var"))))
    return layers


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,n_layers,wd", [("two", 2, False), ("one", 1, True)])
def test_pillar_encode_ref_matches_reference_golden(golden, name, n_layers, wd, dtype):
    """The restatement against the reference's own fp32 PillarFeatureNet output, at the suite's gate of 1e-3 of the feature scale (a
    structural mistake -- mean over num_points rows, mask before the decoration, max over the real rows only -- moves values by O(1))."""
    g = golden("pillars.npz")
    want = g[name + "_feats"]
    got = pr.pillar_encode_ref(g["voxels"], g["num"], g["coors"], GOLDEN_GEOM, _golden_layers(g, name, n_layers), wd, dtype=dtype)
    assert got.dtype == dtype and got.shape == want.shape
    assert (g["num"] == g["voxels"].shape[1]).any() and (g["num"] == 1).any()
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    report("pillar_encode_ref(%s) %s vs reference golden" % (np.dtype(dtype).name, name), err, 1e-3 * scale)
    assert err <= 1e-3 * scale


@pytest.mark.parametrize("ndim", [4, 5])
@pytest.mark.parametrize("wd", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("num_filters", [[16], [32], [64], [64, 64]], ids=lambda f: "x".join(map(str, f)))
def test_pillar_encode_ref_matches_float64_oracle(num_filters, wd, ndim):
    """Both sides in float64: agreement to 1e-12 of the scale, on pillars at realistic magnitude with 1, P and in-between points."""
    from futuredet_amd.synth import seeded_state_dict
    from oracle import model as omodel

    rng = np.random.default_rng(100 * ndim + 10 * len(num_filters) + num_filters[0] + int(wd))
    vox, num, coors = pr.make_pillars(rng, 37, 20, ndim, batch_size=2)
    net = omodel.PillarFeatureNet(num_input_features=ndim, num_filters=num_filters, with_distance=wd,
                                  voxel_size=[pr.PILLAR_VOXEL[0], pr.PILLAR_VOXEL[1], 8.0], pc_range=list(pr.PILLAR_RANGE))
    sd = seeded_state_dict(net, 11)
    sd["pfn_layers.0.linear.weight"] = sd["pfn_layers.0.linear.weight"] * 0.02
    net.load_state_dict(sd, strict=False)
    net = net.double().eval()
    layers = []
    for pfn in net.pfn_layers:
        layers.append(pr.fold_bn(pfn.linear.weight.detach().numpy(), pfn.norm.weight.detach().numpy(), pfn.norm.bias.detach().numpy(),
                                 pfn.norm.running_mean.numpy(), pfn.norm.running_var.numpy(), eps=pfn.norm.eps))
    assert [len(l[1]) for l in layers] == ([32, 64] if len(num_filters) == 2 else num_filters)
    with torch.no_grad():
        want = net(torch.from_numpy(vox).double(), torch.from_numpy(num), torch.from_numpy(coors)).numpy()
    got = pr.pillar_encode_ref(vox, num, coors, pr.PILLAR_GEOM, layers, wd)
    assert got.shape == want.shape == (37, num_filters[-1]) and want.dtype == np.float64
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    report("pillar_encode_ref vs float64 oracle %s wd=%d ndim=%d" % (num_filters, wd, ndim), err, 1e-12 * scale)
    assert scale > 0.1 and err <= 1e-12 * scale


def test_pillar_encode_ref_empty_pillar_is_nan_like_the_reference():
    """num_points == 0: the mean divides by zero and the 0/1 mask multiplies NaN -- reference and restatement both give NaN."""
    from oracle import model as omodel

    rng = np.random.default_rng(3)
    vox, num, coors = pr.make_pillars(rng, 3, 4, 5)
    num[1] = 0
    vox[1] = 0
    layers = pr.make_layers(rng, [64], 10)
    got = pr.pillar_encode_ref(vox, num, coors, pr.PILLAR_GEOM, layers, False)
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    net = omodel.PillarFeatureNet(num_input_features=5, num_filters=[64], voxel_size=[0.25, 0.25, 8.0], pc_range=list(pr.PILLAR_RANGE)).eval()
    with torch.no_grad():
        want = net(torch.from_numpy(vox), torch.from_numpy(num), torch.from_numpy(coors))
    assert bool(want[1].isnan().all()) and bool(want[[0, 2]].isfinite().all())


def test_make_layers_lets_masked_rows_win():
    """The recipe of the GPU tests: on the large-shift units relu(shift) of a padding row is the pillar's max for some pillars, and the
    negative-shift units clip to exactly 0 somewhere."""
    rng = np.random.default_rng(1)
    vox, num, coors = pr.make_pillars(rng, 40, 20, 5)
    layers = pr.make_layers(rng, [16], 10)
    x = pr.decorate_ref(vox, num, coors, pr.PILLAR_GEOM, False)
    out = pr.pfn_layers_ref(x, layers)
    masked = np.maximum(layers[0][2].astype(np.float64), 0.0)
    real_only = np.stack([pr.pfn_layers_ref(x[m:m + 1, :num[m]], layers)[0] for m in range(40)])
    padded = num < 20
    assert np.array_equal(out[~padded], real_only[~padded])
    wins = padded[:, None] & (out == masked[None, :]) & (real_only < masked[None, :])
    assert wins[:, 0::4].sum() >= 10 and (out[:, 2::4] == 0).any() and (out > masked[None, :]).any()
    assert np.abs(out).max() < 20


# ------------------------------------------------------------------------------------------------ sweeps
def _sweep_case(g, case):
    """-> raw, rows, transforms, lags, remove_close in the visit order of loading.py:128-129"""
    rows = g[case + "_rows"]
    n = len(rows) - 1
    order = [0] + ([int(i) + 1 for i in np.random.default_rng(0).choice(n - 1, n - 1, replace=False)] if n > 1 else [])
    raw = np.concatenate([g[case + "_raw"][rows[s]:rows[s + 1]] for s in order])
    new_rows = np.cumsum([0] + [int(rows[s + 1] - rows[s]) for s in order])
    mats = [None if s == 0 or not g[case + "_has"][s - 1] else g[case + "_mats"][s - 1] for s in order]
    lags = [0.0 if s == 0 else float(g[case + "_lags"][s - 1]) for s in order]
    return raw, new_rows, mats, lags, [s != 0 for s in order]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_assemble_sweeps_ref_matches_reference_golden(golden, case):
    g = golden("sweeps.npz")
    out = pr.assemble_sweeps_ref(*_sweep_case(g, case), keep_cols=4, min_distance=1.0)
    ref = g[case + "_combined"]
    assert out.shape == ref.shape and out.dtype == ref.dtype
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_assemble_sweeps_ref_matches_oracle_random():
    from oracle import ops as oops

    rng = np.random.default_rng(8)
    S = 5
    raws, mats, lags = [], [], []
    for s in range(S):
        n = 150 + 17 * s
        raw = rng.normal(0, [6.0, 6.0, 1.5, 30.0, 5.0], (n, 5)).astype(np.float32)
        raw[: n // 3, :2] = rng.uniform(-1.5, 1.5, (n // 3, 2))
        raws.append(raw)
        if s:
            a = rng.uniform(-0.3, 0.3)
            m = np.eye(4)
            m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            m[:3, 3] = rng.normal(0, [2.0, 0.5, 0.02])
            mats.append(None if s == 3 else m)
            lags.append(0.05 * s)
    want = oops.assemble_sweeps(raws[0], raws[1:], mats, lags)
    order = [0] + [int(i) + 1 for i in np.random.default_rng(0).choice(S - 1, S - 1, replace=False)]
    rows = np.cumsum([0] + [len(raws[s]) for s in order])
    got = pr.assemble_sweeps_ref(np.concatenate([raws[s] for s in order]), rows, [None if s == 0 else mats[s - 1] for s in order],
                                 [0.0 if s == 0 else lags[s - 1] for s in order], [s != 0 for s in order])
    assert 0 < len(want) < rows[-1] and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_exact_transform_inputs_are_order_independent():
    """The recipe of test_gpu_sweeps_edges.py: with these matrices and coordinates the float64 4x4 product has no rounding, so any
    summation order gives the same bits (checked with Python integers)."""
    rng = np.random.default_rng(4)
    m, xyz = pr.exact_transform(rng), pr.exact_coords(rng, (200, 3))
    assert np.abs(m).max() < 64 and np.abs(xyz).max() < 128
    mi = np.round(m * 1024).astype(np.int64)
    xi = np.round(xyz.astype(np.float64) * 256).astype(np.int64)
    assert np.array_equal(mi / 1024.0, m) and np.array_equal(xi / 256.0, xyz.astype(np.float64))
    exact = (xi @ mi[:3, :3].T + mi[:3, 3] * 256).astype(np.float64) / float(1 << 18)  # |numerator| < 2^33: exact in float64
    out = pr.assemble_sweeps_ref(xyz, [0, 200], [m], [0.5], [False], keep_cols=3)
    assert np.array_equal(out[:, :3], exact.astype(np.float32)) and np.all(out[:, 3] == np.float32(0.5))


# ------------------------------------------------------------------------------------------------ scatter
def test_pillar_scatter_ref_matches_oracle():
    from oracle import model as omodel

    rng = np.random.default_rng(6)
    B, C, ny, nx, M = 2, 7, 5, 9, 31
    cells = rng.choice(B * ny * nx, M, replace=False)
    coors = np.stack([cells // (ny * nx), np.zeros(M, np.int64), (cells // nx) % ny, cells % nx], 1).astype(np.int32)
    feats = rng.standard_normal((M, C)).astype(np.float32)
    want = omodel.pillars_scatter(torch.from_numpy(feats), torch.from_numpy(coors), B, [nx, ny, 1]).numpy()
    got = pr.pillar_scatter_ref(feats, coors, M, B, ny, nx)
    assert got.dtype == want.dtype and np.array_equal(got, want) and (got != 0).sum() == M * C
    # rows past n and rows outside the canvas are skipped
    bad = coors.copy()
    bad[0, 0], bad[1, 2], bad[2, 3] = B, -1, nx
    cut = want.copy()
    for m in (0, 1, 2, M - 1):
        b, _, y, x = coors[m]
        cut[b, :, y, x] = 0
    assert np.array_equal(pr.pillar_scatter_ref(feats, bad, M - 1, B, ny, nx), cut)
