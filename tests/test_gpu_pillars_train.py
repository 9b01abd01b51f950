"""-m gpu: PillarFeatureNet in training mode (csrc/fd_pillars_grad.hip) and the scatter's backward: against the reference's own
reader in .train() (tests/golden/pillars_train.npz, made by tests/golden/make_golden_pillars_train.py), against a float64 torch
restatement at the full train cap, bit-for-bit determinism and graph replay, and one PointPillars training step."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from futuredet_amd import hip_ops  # noqa: E402
from futuredet_amd.readers import PillarFeatureNet  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(HERE, "golden", "pillars_train.npz"))
P0 = np.load(os.path.join(HERE, "golden", "pillars.npz"))
VS, RG = [0.2, 0.2, 8.0], [-6.4, -6.4, -5.0, 6.4, 6.4, 3.0]
GRADS = ("pfn_layers.0.linear.weight", "pfn_layers.0.norm.weight", "pfn_layers.0.norm.bias", "pfn_layers.1.linear.weight",
         "pfn_layers.1.norm.weight", "pfn_layers.1.norm.bias")
CASES = {"plain": False, "distance": True}


def _close(name, got, ref, tol):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= tol, "%s: max |got - ref| = %.3g of max |ref| (tolerance %.0e)" % (name, err, tol)


def _reader(case, pc_range=RG, voxel_size=VS):
    net = PillarFeatureNet(num_input_features=5, num_filters=[64, 64], with_distance=CASES[case], voxel_size=voxel_size,
                           pc_range=pc_range)
    sd = {k.split("/sd/")[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith(case + "/sd/")}
    net.load_state_dict(sd)
    return net.to(DEV).train()


def _inputs():
    return (torch.from_numpy(P0["voxels"]).to(DEV), torch.from_numpy(P0["num"]).to(DEV), torch.from_numpy(P0["coors"]).to(DEV))


def _dout(case, m):
    return torch.from_numpy(np.random.default_rng(43 + int(CASES[case])).standard_normal((m, 64)).astype(np.float32)).to(DEV)


def _params(net):
    l1, l2 = net.pfn_layers
    return (l1.linear.weight.detach(), l1.norm.weight.detach(), l1.norm.bias.detach(), l2.linear.weight.detach(),
            l2.norm.weight.detach(), l2.norm.bias.detach())


def _geom(net):
    return (net.vx, net.vy, net.x_offset, net.y_offset)


def _run_ops(net, voxels, num, coors, dout, workspace=None, out=None):
    w1, g1, b1, w2, g2, b2 = _params(net)
    n1, n2 = net.pfn_layers[0].norm, net.pfn_layers[1].norm
    fwd = hip_ops.pillar_train_forward(voxels, num, coors, _geom(net), w1, g1, b1, n1.eps, w2, g2, b2, n2.eps,
                                       with_distance=net._with_distance, workspace=workspace, out=out)
    grads = hip_ops.pillar_train_backward(dout, voxels, num, coors, _geom(net), w1, g1, b1, w2, g2, b2, fwd[5],
                                          with_distance=net._with_distance)
    return fwd[:5], grads


@pytest.mark.parametrize("case", sorted(CASES))
def test_train_reader_matches_the_reference(case):
    net = _reader(case)
    voxels, num, coors = _inputs()
    dout = _dout(case, voxels.shape[0])
    (_, mean1, var1, mean2, var2), _ = _run_ops(net, voxels, num, coors, dout)
    for name, got in (("mean1", mean1), ("var1", var1), ("mean2", mean2), ("var2", var2)):
        _close(case + " " + name, got.cpu(), G["%s/%s" % (case, name)], 1e-4)
    net = _reader(case)
    out = net(voxels, num, coors)
    out.backward(dout)
    torch.cuda.synchronize()
    _close(case + " out", out.detach().cpu()[::2], G[case + "/out"], 1e-4)
    for i in (1, 2):
        bn = net.pfn_layers[i - 1].norm
        _close("%s running_mean%d" % (case, i), bn.running_mean.cpu(), G["%s/running_mean%d" % (case, i)], 1e-4)
        _close("%s running_var%d" % (case, i), bn.running_var.cpu(), G["%s/running_var%d" % (case, i)], 1e-4)
        assert int(bn.num_batches_tracked) == int(G["%s/num_batches_tracked%d" % (case, i)]) == 1
    params = dict(net.named_parameters())
    for k in GRADS:
        _close("%s grad %s" % (case, k), params[k].grad.cpu(), G["%s/grad/%s" % (case, k)], 1e-3)


def _restatement(voxels, num, coors, net, dout):
    """PillarFeatureNet.train() forward and backward in float64 torch ops (pillar_encoder.py:38-55, :113-164)."""
    f = voxels.double()
    M, P, _ = f.shape
    mean = f[:, :, :3].sum(1, keepdim=True) / num.double().view(-1, 1, 1)
    cx = coors[:, 3].double() * net.vx + net.x_offset
    cy = coors[:, 2].double() * net.vy + net.y_offset
    cols = [f, f[:, :, :3] - mean, (f[:, :, 0] - cx[:, None])[..., None], (f[:, :, 1] - cy[:, None])[..., None]]
    if net._with_distance:
        cols.append(f[:, :, :3].norm(dim=2, keepdim=True))
    x = torch.cat(cols, -1) * (torch.arange(P, device=f.device)[None, :] < num[:, None]).double()[..., None]
    ps = [p.double().clone().requires_grad_(True) for p in _params(net)]
    w1, g1, b1, w2, g2, b2 = ps
    eps1, eps2 = net.pfn_layers[0].norm.eps, net.pfn_layers[1].norm.eps
    z1 = x @ w1.t()
    m1, v1 = z1.mean((0, 1)), z1.var((0, 1), unbiased=False)
    a1 = torch.relu((z1 - m1) / torch.sqrt(v1 + eps1) * g1 + b1)
    in2 = torch.cat([a1, a1.max(1, keepdim=True)[0].expand(-1, P, -1)], -1)
    z2 = in2 @ w2.t()
    m2, v2 = z2.mean((0, 1)), z2.var((0, 1), unbiased=False)
    out = torch.relu((z2 - m2) / torch.sqrt(v2 + eps2) * g2 + b2).max(1)[0]
    out.backward(dout.double())
    return [out.detach(), m1.detach(), v1.detach(), m2.detach(), v2.detach()], [p.grad for p in ps]


def _full_cap_sample(seed):
    from futuredet_amd.configs import pointpillars_config
    from futuredet_amd.synth import synthetic_cloud
    from futuredet_amd.voxelize import points_to_voxel

    vg = pointpillars_config().voxel_generator
    pts = torch.from_numpy(synthetic_cloud(seed=seed, target_points=300000)).to(DEV)
    v, c, n = points_to_voxel(pts, vg["voxel_size"], vg["range"], vg["max_points_in_voxel"], True, vg["max_voxel_num"][0])
    coors = torch.nn.functional.pad(c.int(), (1, 0))
    return v.contiguous(), n.int().contiguous(), coors.contiguous(), vg


@pytest.mark.parametrize("case", sorted(CASES))
def test_full_train_cap_sample_matches_a_float64_restatement(case):
    voxels, num, coors, vg = _full_cap_sample(5)
    assert voxels.shape[0] >= 25000 and voxels.shape[1] == 20, tuple(voxels.shape)
    net = _reader(case, pc_range=vg["range"], voxel_size=vg["voxel_size"])
    with torch.no_grad():  # raw coordinates of a 100 m scene: keep layer 1 in a sane range, as the end-to-end tests do
        net.pfn_layers[0].linear.weight.mul_(0.02)
    dout = torch.randn((voxels.shape[0], 64), generator=torch.Generator(device=DEV).manual_seed(11), device=DEV)
    fwd, grads = _run_ops(net, voxels, num, coors, dout)
    want_fwd, want_grads = _restatement(voxels, num, coors, net, dout)
    for name, got, want in zip(("out", "mean1", "var1", "mean2", "var2"), fwd, want_fwd):
        _close("%s %s" % (case, name), got.cpu(), want.cpu(), 1e-4)
    for name, got, want in zip(GRADS, grads, want_grads):
        _close("%s grad %s" % (case, name), got.cpu(), want.cpu(), 1e-3)


def test_two_runs_are_bit_identical():
    voxels, num, coors, vg = _full_cap_sample(6)
    net = _reader("plain", pc_range=vg["range"], voxel_size=vg["voxel_size"])
    dout = torch.randn((voxels.shape[0], 64), generator=torch.Generator(device=DEV).manual_seed(12), device=DEV)
    a = _run_ops(net, voxels, num, coors, dout)
    b = _run_ops(net, voxels, num, coors, dout)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_graph_replay_gives_the_eager_bytes():
    net = _reader("distance")
    voxels, num, coors = _inputs()
    dout = _dout("distance", voxels.shape[0])
    want = _run_ops(net, voxels, num, coors, dout)
    ws = torch.empty((hip_ops.pillar_train_workspace_bytes(voxels.shape[0], voxels.shape[1]),), dtype=torch.uint8, device=DEV)
    out = torch.empty((voxels.shape[0], 64), dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run_ops(net, voxels, num, coors, dout, workspace=ws, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _run_ops(net, voxels, num, coors, dout, workspace=ws, out=out)
    out.zero_()
    ws.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(want[0] + want[1], got[0] + got[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("channels_last", [False, True])
def test_scatter_backward_is_the_canvas_gradient_at_the_pillars(channels_last):
    from futuredet_amd.backbones import PointPillarsScatter

    rng = np.random.default_rng(3)
    B, C, ny, nx = 2, 64, 48, 40
    cells = [rng.choice(ny * nx, 700, replace=False) for _ in range(B)]
    coors = np.concatenate([np.stack([np.full(700, b), np.zeros(700, int), cells[b] // nx, cells[b] % nx], 1) for b in range(B)]).astype(np.int32)
    coors = torch.from_numpy(coors).to(DEV)
    feats = torch.randn((len(coors), C), device=DEV, requires_grad=True)
    sc = PointPillarsScatter(num_input_features=C)
    sc.dense_channels_last = channels_last
    canvas = sc(feats, coors, B, np.array([nx, ny, 1]))
    assert canvas.is_contiguous(memory_format=torch.channels_last) == channels_last
    dcanvas = torch.randn((B, C, ny, nx), device=DEV)
    if channels_last:
        dcanvas = dcanvas.contiguous(memory_format=torch.channels_last)
    canvas.backward(dcanvas)
    want = dcanvas[coors[:, 0].long(), :, coors[:, 2].long(), coors[:, 3].long()]
    assert torch.equal(feats.grad, want)
    assert torch.equal(hip_ops.pillar_scatter_backward(dcanvas, coors), want)


def test_bf16_reader_refuses_training():
    net = _reader("plain")
    net.compute_dtype = torch.bfloat16
    voxels, num, coors = _inputs()
    with pytest.raises(NotImplementedError, match="fp32"):
        net(voxels, num, coors)


def _gt_boxes(rng, T, n):
    boxes = np.zeros((1, T, n, 12), np.float32)
    for t in range(T):
        b = boxes[0, t]
        b[:, 0:2] = rng.uniform(-45.0, 45.0, (n, 2))
        b[:, 2] = rng.normal(-0.5, 0.3, n)
        b[:, 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * rng.uniform(0.8, 1.2, (n, 3))
        b[:, 6:10] = rng.normal(0.0, 2.0, (n, 4))
        b[:, 10:12] = rng.uniform(-np.pi, np.pi, (n, 2))
    return boxes, np.full((1, T), n, np.int32), np.ones((1, T, n), np.int32), rng.integers(0, 3, (1, T, n)).astype(np.int32)


def test_pointpillars_training_step():
    from futuredet_amd import build_detector
    from futuredet_amd.configs import pointpillars_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel

    cfg = pointpillars_config()
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = tame_box_dims(seeded_state_dict(net, 9))
    sd["reader.pfn_layers.0.linear.weight"] = sd["reader.pfn_layers.0.linear.weight"] * 0.02
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV)
    pts = synthetic_cloud(seed=2, target_points=30000)
    cloud = [torch.from_numpy(pts).to(DEV)]

    def detect(model):
        model.eval()
        with torch.no_grad():
            r = model.forward_points(cloud, vg, padded=False)[0]
        torch.cuda.synchronize()
        return torch.cat([r["box3d_lidar"], r["scores"][:, None]], 1).cpu()

    grid = np.array([512, 512, 1])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    boxes, counts, classes, traj = [torch.from_numpy(a).to(DEV) for a in _gt_boxes(np.random.default_rng(4), cfg.timesteps, 24)]
    targets = ta(boxes, counts, classes, traj if ta.extra_sets else None)
    assert int(sum(m[0].sum() for m in targets["mask"])) > 0
    v, c, n = points_to_voxel(pts, vg["voxel_size"], vg["range"], vg["max_points_in_voxel"], True, vg["max_voxel_num"][0])
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})

    before = detect(net)
    bn_before = [(b.running_mean.clone(), b.running_var.clone()) for b in (p.norm for p in net.reader.pfn_layers)]
    net.train()
    ret = net(ex, return_loss=True)
    loss = sum(ret["loss"])
    assert torch.isfinite(loss)
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    opt.zero_grad()
    loss.backward()
    for name, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            if name.startswith("reader."):
                assert bool((p.grad != 0).any()), name
    for (rm, rv), pfn in zip(bn_before, net.reader.pfn_layers):
        assert not torch.equal(rm, pfn.norm.running_mean) and not torch.equal(rv, pfn.norm.running_var)
        assert int(pfn.norm.num_batches_tracked) == 1
    opt.step()
    after = detect(net)
    assert before.shape != after.shape or not torch.equal(before, after), "one SGD step must change the detections"
    fresh = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    fresh.load_state_dict(net.state_dict())
    fresh = fresh.to(DEV)
    again = detect(fresh)
    assert after.shape == again.shape and torch.equal(after, again), "the stepped model must detect as a fresh load of its state_dict"
