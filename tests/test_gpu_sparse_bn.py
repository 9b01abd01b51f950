"""-m gpu: the fused training-mode BatchNorm of the sparse backbone (futuredet_amd/csrc/fd_sparse_bn.hip over fd_row_bn.h, sparse.batch_norm_act,
SpMiddleResNetFHD.fused_bn) against the formulas in float64 on the same fp32 inputs.

The backward reference is teacher-forced: it takes its ReLU mask from the kernel's own y (a y within rounding of 0 would otherwise flip
a mask and move dx by O(1)).  Gates: |got - ref| <= gate * max |ref| per output; 1e-5 on inputs (a) (x ~ N(0, 0.25^2)), 1e-4 on
inputs (b) (the same plus an offset of +-30 on half the channels -- a mean 120 times the spread)."""
import copy

import numpy as np
import pytest
import torch

from parity_util import report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
EPS = 1e-3
CONST_CH, DEAD_CH = 1, 2  # a constant channel; a channel whose beta drives every output below 0


def _P():
    from futuredet_amd import hip_ops

    return hip_ops.sparse_bn_chunk()


def _inputs(seed, n, C, offset):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.25, (n, C)).astype(np.float32)
    x[:, CONST_CH] = 0.375
    if offset:
        ch = np.arange(C)
        x += np.where(ch % 4 == 0, offset, np.where(ch % 4 == 2, -offset, 0.0)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.normal(0.0, 0.5, C).astype(np.float32)
    beta[DEAD_CH] = -10.0
    dy = rng.normal(0.0, 1.0, (n, C)).astype(np.float32)
    res = rng.normal(0.0, 1.0, (n, C)).astype(np.float32)
    rm = rng.normal(0.0, 1.0, C).astype(np.float32)
    rv = rng.uniform(0.5, 2.0, C).astype(np.float32)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, res=res, rm=rm, rv=rv)


def _ref_forward(x, gamma, beta, res, relu, eps=EPS):
    x = x.astype(np.float64)
    mean, var = x.mean(0), x.var(0)
    invstd = 1.0 / np.sqrt(var + eps)
    pre = gamma.astype(np.float64) * (x - mean) * invstd + beta.astype(np.float64)
    if res is not None:
        pre = pre + res.astype(np.float64)
    return (np.maximum(pre, 0.0) if relu else pre), pre, mean, var, invstd


def _ref_backward(dy, x, y_kernel, gamma, mean, invstd, relu):
    n = x.shape[0]
    g = dy.astype(np.float64)
    if relu:
        g = g * (y_kernel > 0)
    xh = (x.astype(np.float64) - mean) * invstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    dx = gamma.astype(np.float64) * invstd * (g - dbeta / n - xh * dgamma / n)
    return dx, dgamma, dbeta, g


def _gate(name, got, ref, gate):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / max(scale, 1e-30)
    report("sparse bn " + name, err, gate)
    assert np.isfinite(got).all() and err <= gate, "%s: error %.3e of the largest reference value (%.3e) > %.1e" % (name, err, scale, gate)
    return err


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(hip, d, relu, with_res, momentum=0.1, n_dev=None):
    """forward + backward through hip_ops on fresh copies of the running statistics -> dict of device tensors"""
    x, dy = _t(d["x"]), _t(d["dy"])
    res = _t(d["res"]) if with_res else None
    gamma, beta, rm, rv = _t(d["gamma"]), _t(d["beta"]), _t(d["rm"]), _t(d["rv"])
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, saved = hip.sparse_bn_train_forward(x, gamma, beta, rm, rv, nbt, EPS, momentum, residual=res, relu=relu, n_dev=n_dev)
    dx, dres, dgamma, dbeta = hip.sparse_bn_train_backward(dy, x, y, gamma, saved, relu=relu, n_dev=n_dev, want_residual=with_res)
    out = dict(y=y, saved=saved, rm=rm, rv=rv, nbt=nbt, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if dres is not None:
        out["dres"] = dres
    return out


def _check_against_float64(hip, d, relu, with_res, gate, tag, momentum=0.1):
    out = {k: v.cpu().numpy() for k, v in _run(hip, d, relu, with_res, momentum).items()}
    n = d["x"].shape[0]
    res = d["res"] if with_res else None
    y, pre, mean, var, invstd = _ref_forward(d["x"], d["gamma"], d["beta"], res, relu)
    if relu:
        assert (pre[:, DEAD_CH] < 0).all() and (out["y"][:, DEAD_CH] == 0).all(), "the dead channel must be all zero after the ReLU"
    _gate(tag + " y", out["y"], y, gate)
    _gate(tag + " saved mean", out["saved"][0], mean, gate)
    _gate(tag + " saved invstd", out["saved"][1], invstd, gate)
    _gate(tag + " running_mean", out["rm"], (1 - momentum) * d["rm"].astype(np.float64) + momentum * mean, gate)
    _gate(tag + " running_var", out["rv"], (1 - momentum) * d["rv"].astype(np.float64) + momentum * var * n / (n - 1), gate)
    assert int(out["nbt"]) == 1
    dx, dgamma, dbeta, g = _ref_backward(d["dy"], d["x"], out["y"], d["gamma"], mean, invstd, relu)
    _gate(tag + " dx", out["dx"], dx, gate)
    _gate(tag + " dgamma", out["dgamma"], dgamma, gate)
    _gate(tag + " dbeta", out["dbeta"], dbeta, gate)
    if with_res:
        _gate(tag + " d_residual", out["dres"], g, gate)


FORMS = (("relu", True, False), ("relu+residual", True, True), ("plain", False, False))


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 64, 128])
@pytest.mark.parametrize("n_of", [lambda P: 2, lambda P: 63, lambda P: P - 1, lambda P: P, lambda P: P + 1, lambda P: 3 * P + 17],
                         ids=["2", "63", "P-1", "P", "P+1", "3P+17"])
def test_kernels_match_float64(hip, n_of, C):
    n = n_of(_P())
    for name, relu, with_res in FORMS:
        _check_against_float64(hip, _inputs(n * 1000 + C, n, C, 0.0), relu, with_res, 1e-5, "(a) n=%d C=%d %s" % (n, C, name))
        if n >= 63:
            _check_against_float64(hip, _inputs(n * 1000 + C + 1, n, C, 30.0), relu, with_res, 1e-4, "(b) n=%d C=%d %s" % (n, C, name))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset,gate", [(0.0, 1e-5), (30.0, 1e-4)])
def test_running_statistics_over_three_steps(hip, offset, gate):
    P = _P()
    n, C, m = 3 * P + 17, 32, 0.01
    d0 = _inputs(5, n, C, offset)
    gamma, beta, rm, rv = _t(d0["gamma"]), _t(d0["beta"]), _t(d0["rm"]), _t(d0["rv"])
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    rm64, rv64 = d0["rm"].astype(np.float64), d0["rv"].astype(np.float64)
    for step in range(3):
        x = _inputs(50 + step, n, C, offset)["x"] * np.float32(1.0 + step)
        hip.sparse_bn_train_forward(_t(x), gamma, beta, rm, rv, nbt, EPS, m)
        x64 = x.astype(np.float64)
        rm64 = (1 - m) * rm64 + m * x64.mean(0)
        rv64 = (1 - m) * rv64 + m * x64.var(0) * n / (n - 1)
    _gate("3 steps running_mean (offset %g)" % offset, rm.cpu().numpy(), rm64, gate)
    _gate("3 steps running_var (offset %g)" % offset, rv.cpu().numpy(), rv64, gate)
    assert int(nbt) == 3


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 128])
def test_two_runs_are_bit_identical(hip, C):
    d = _inputs(7, 3 * _P() + 17, C, 30.0)
    for name, relu, with_res in FORMS:
        a, b = _run(hip, d, relu, with_res), _run(hip, d, relu, with_res)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits(hip):
    """forward + backward captured once: nothing in the calls allocates device memory outside torch's allocator or synchronises"""
    P = _P()
    n, C = 3 * P + 17, 64
    sets = [_inputs(20 + i, n, C, 0.0) for i in range(2)]
    eager = [_run(hip, d, True, True) for d in sets]
    keys = ("x", "dy", "res", "gamma", "beta", "rm", "rv")
    st = {k: _t(sets[0][k]).clone() for k in keys}
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)

    def step():
        y, saved = hip.sparse_bn_train_forward(st["x"], st["gamma"], st["beta"], st["rm"], st["rv"], nbt, EPS, 0.1, residual=st["res"], relu=True)
        dx, dres, dgamma, dbeta = hip.sparse_bn_train_backward(st["dy"], st["x"], y, st["gamma"], saved, relu=True, want_residual=True)
        return dict(y=y, saved=saved, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up: code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with hip.workspace.scope("test_sparse_bn_graph"):
        with torch.cuda.graph(graph):
            outs = step()
    try:
        for i in (0, 1, 0):
            for k in keys:
                st[k].copy_(_t(sets[i][k]))
            nbt.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for k, v in outs.items():
                assert torch.equal(v, eager[i][k]), (i, k)
            assert torch.equal(st["rm"], eager[i]["rm"]) and torch.equal(st["rv"], eager[i]["rv"]) and int(nbt) == 1
        assert not torch.equal(eager[0]["y"], eager[1]["y"])
    finally:
        del graph
        hip.workspace.release("test_sparse_bn_graph")


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 64])
def test_row_count_from_the_device(hip, C):
    P = _P()
    cap, nv = 2 * P, P + 1
    d = _inputs(9, cap, C, 30.0)
    exact = {k: (v[:nv] if v.ndim == 2 else v) for k, v in d.items()}
    for k in ("x", "dy", "res"):
        d[k][nv:] = np.nan  # a poisoned tail must reach no output and no statistic
    n_dev = torch.tensor([nv], dtype=torch.int32, device=DEV)
    for name, relu, with_res in FORMS:
        a = _run(hip, d, relu, with_res, n_dev=n_dev)
        b = _run(hip, exact, relu, with_res)
        for k in a:
            if a[k].shape == (cap, C):
                assert torch.equal(a[k][:nv], b[k]), (name, k)
                assert torch.count_nonzero(a[k][nv:]) == 0 and bool(torch.isfinite(a[k]).all()), (name, k, "tail")
            else:
                assert torch.equal(a[k], b[k]), (name, k)


# 6, 7 ------------------------------------------------------------------------------------------------------------------------------
def _backbone(seed=5):
    from futuredet_amd.backbones import SpMiddleResNetFHD
    from futuredet_amd.synth import seeded_state_dict

    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, seed), strict=False)
    return bb


@pytest.fixture(scope="module")
def cloud():
    from test_gpu_spconv_grad import _voxels

    cfg, v, c, n = _voxels(3, 4000)
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32))
    coords = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    return feats, coords, np.array([1440, 1440, 40])


def test_eval_path_sees_the_new_statistics(hip, cloud):
    from futuredet_amd.backbones import SpMiddleResNetFHD

    feats, coords, shape = cloud
    f, c = feats.to(DEV), torch.from_numpy(coords).to(DEV)
    bb = _backbone().to(DEV)
    bb.fused_bn = True
    bb.eval()
    with torch.no_grad():
        before = bb(f, c, 1, shape)[0].clone()  # fills the folded-BatchNorm caches
    bb.train()
    bb(f, c, 1, shape)
    stats = {k: v.clone() for k, v in bb.state_dict().items() if "running" in k or "num_batches" in k}
    assert len(stats) == 63 and all(int(v) == 1 for k, v in stats.items() if "num_batches" in k)
    bb.eval()
    fresh = SpMiddleResNetFHD(num_input_features=5)
    fresh.load_state_dict(bb.state_dict())
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        got, want = bb(f, c, 1, shape)[0], fresh(f, c, 1, shape)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want), float((got - want).abs().max())
    assert not torch.equal(got, before), "one training forward must move the eval output"


def test_inside_the_backbone(hip, cloud, monkeypatch):
    """fused_bn=True on a ~4k-point cloud.  (1) Every _SparseBatchNormFunction call, on the features and gradient it met inside the
    backbone, against the float64 formulas (teacher-forced) at 1e-4.  (2) Every parameter gradient and running statistic against the
    float64 restatement of the whole backbone, at the gates of test_gpu_spconv_grad: 1e-2 norm-wise, 1e-4 for the statistics."""
    from futuredet_amd import sparse as spconv
    from test_gpu_spconv_grad import _close, _restated_backbone

    feats, coords, input_shape = cloud
    seen = []
    orig = spconv._SparseBatchNormFunction.apply

    def recording(x, gamma, beta, residual, bn, relu):
        out = orig(x, gamma, beta, residual, bn, relu)
        rec = dict(x=x.detach(), gamma=gamma.detach().clone(), beta=beta.detach().clone(), res=None if residual is None else residual.detach(),
                   relu=relu, eps=bn.eps, y=out.detach())
        out.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        seen.append(rec)
        return out

    monkeypatch.setattr(spconv._SparseBatchNormFunction, "apply", recording)
    bb = _backbone()
    ref_bb = copy.deepcopy(bb)
    bb = bb.to(DEV).train()
    bb.fused_bn = True
    bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
    rng = np.random.default_rng(9)
    G = torch.from_numpy(rng.uniform(-1, 1, tuple(bev.shape)).astype(np.float32))
    (bev * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()

    # (1) the kernels, call by call
    assert len(seen) == 21 and sum(r["res"] is not None for r in seen) == 8 and all(r["relu"] for r in seen)
    for i, r in enumerate(seen):
        n, C = r["x"].shape
        assert n >= 2 and "dy" in r
        tag = "backbone call %d (n=%d C=%d%s)" % (i, n, C, " +res" if r["res"] is not None else "")
        x, gamma, beta, dy = (r[k].cpu().numpy() for k in ("x", "gamma", "beta", "dy"))
        res = None if r["res"] is None else r["res"].cpu().numpy()
        yk = r["y"].cpu().numpy()
        y, pre, mean, var, invstd = _ref_forward(x, gamma, beta, res, True, r["eps"])
        _gate(tag + " y", yk, y, 1e-4)
        leaves = [r[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta")]
        rl = None if r["res"] is None else r["res"].clone().requires_grad_(True)
        twin = torch.nn.BatchNorm1d(C, eps=r["eps"], momentum=0.01).to(DEV).train()
        y2 = orig(leaves[0], leaves[1], leaves[2], rl, twin, True)
        assert torch.equal(y2.detach(), r["y"]), tag
        y2.backward(r["dy"])
        dx, dgamma, dbeta, g = _ref_backward(dy, x, yk, gamma, mean, invstd, True)
        _gate(tag + " dx", leaves[0].grad.cpu().numpy(), dx, 1e-4)
        _gate(tag + " dgamma", leaves[1].grad.cpu().numpy(), dgamma, 1e-4)
        _gate(tag + " dbeta", leaves[2].grad.cpu().numpy(), dbeta, 1e-4)
        if rl is not None:
            _gate(tag + " d_residual", rl.grad.cpu().numpy(), g, 1e-4)

    # (2) the whole backbone
    shape0 = list(np.array(input_shape[::-1]) + [1, 0, 0])
    f, idx, shape, bns = _restated_backbone(ref_bb, feats.double(), coords, shape0)
    Gr = G.double().view(1, 128, shape[0], G.shape[2], G.shape[3])
    ii = torch.from_numpy(idx).long()
    (f * Gr[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]).sum().backward()
    got = dict(bb.named_parameters())
    for name, p in ref_bb.named_parameters():
        assert got[name].grad is not None and bool(torch.isfinite(got[name].grad).all()), name
        ref = p.grad.numpy().astype(np.float64)
        if name.endswith("bias") and "bn" not in name and not name.endswith(".1.bias"):
            continue  # a convolution bias followed by training-mode BatchNorm: its exact gradient is 0, both sides are rounding noise
        e = float(np.linalg.norm(got[name].grad.cpu().numpy() - ref)) / max(float(np.linalg.norm(ref)), 1e-30)
        report("fused_bn backbone grad (norm-wise) " + name, e, 1e-2)
        assert e <= 1e-2, (name, e)
    mods = dict(bb.named_modules())
    n_stats = 0
    for name, m in ref_bb.named_modules():
        if id(m) in bns:
            for stat, want in zip(("running_mean", "running_var"), bns[id(m)]):
                _close("fused_bn backbone %s.%s" % (name, stat), getattr(mods[name], stat).cpu().numpy(), want.numpy(), 1e-4)
            assert int(mods[name].num_batches_tracked) == 1, name
            n_stats += 1
    assert n_stats == 21


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_training_steps_end_to_end(hip, monkeypatch):
    """forecast_n0 with fused_bn and fused_loss through solver.train_steps: finite losses, every parameter moves, same state-dict keys"""
    from futuredet_amd import build_detector, solver
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel
    from test_gpu_loss import _synthetic_gt

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    default_keys = list(net.state_dict())
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    assert net.backbone.fused_bn is False and net.bbox_head.fused_loss is False
    net = net.to(DEV)
    net.backbone.fused_bn = True
    net.bbox_head.fused_loss = True
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    calls = []
    from futuredet_amd import sparse as spconv

    orig = spconv._SparseBatchNormFunction.apply
    monkeypatch.setattr(spconv._SparseBatchNormFunction, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    try:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        losses = [float(sum(out["loss"]).detach()) for out in solver.train_steps(net, [ex, ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2))]
    finally:
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert len(calls) == 42, "every BatchNorm of the backbone goes through the fused kernels, in both steps"
    for k, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if p.requires_grad:
            assert not torch.equal(p.detach(), before[k]), "parameter %s did not move" % k
    assert list(net.state_dict()) == default_keys
