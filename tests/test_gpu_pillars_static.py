"""-m gpu: the sync-free training step for PointPillars and for a bev_map head -- the train-mode pillar reader with its counts on the
device (fd_pillar_train_forward_dev / _backward_dev / _running_stats_dev), the scatter's backward with a device count,
PillarFeatureNet.forward_train_static, PointPillars.forward_points_train, solver.StaticPillarsTrainStep, and the map input of
VoxelNet.forward_points_train / solver.StaticTrainStep.

Exactness rules used below.
  * Device counts against host counts: the same kernels walk the same logical pillars in the same order, so the live rows of ``out``,
    the four batch statistics and the six gradients are the SAME BITS as the host-count entries give on the compacted pillars.
  * Running statistics: the kernel evaluates (1 - f) r + f v [n / (n - 1)] in double precision and rounds once, half an ulp from the
    float64 rule; the bound is 2 fp32 ulp of the result (room for a scale, a multiply and an add in fp32).  torch's own in-place
    update (mul_ by float(1 - f), add_ with alpha) stays within 1.4 ulp of the rule from torch's default buffers (0 and 1), so the two
    module forms are compared under the same 2 ulp.
  * For that reason the reader's running_mean / running_var are the one part of the model state that the static step and the eager
    loop cannot share bit for bit.  From seeded buffers r the two terms may cancel, and torch's fp32 update is then off by ulps of the
    TERMS, not of the result: fl(r a) with a = fl(1 - f) is within 2^-23 |(1 - f) r| of (1 - f) r, alpha v with alpha = fl(f) or
    fl(f n / (n - 1)) within 2^-23 |f v| of its term, the final add within 2^-24 of the result; the kernel is within 2^-24 of the
    result.  With |f v| <= |result| + |(1 - f) r| that gives |static - eager| <= 2^-22 (|r| + |result|), the bound used here.
    Everything else follows test_gpu_train_static's rule (bit-equal when two eager runs are, else 4x their spread)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda")
G = np.load(os.path.join(HERE, "golden", "pillars_train.npz"))
VS, RG = [0.2, 0.2, 8.0], [-6.4, -6.4, -5.0, 6.4, 6.4, 3.0]
CASES = {"plain": False, "distance": True}
P, NDIM = 20, 5
NO_CLIP = dict(max_norm=1.0e6, norm_type=2)  # the norm is computed, the coefficient is exactly 1

# (n_seg, seg_stride, counts)
SEGMENTS = [(1, 64, [37]), (2, 64, [17, 23]), (3, 32, [16, 0, 1]), (2, 64, [64, 64]), (2, 64, [-3, 70]), (2, 9000, [9000, 7421])]


def _ulp_close(got, ref64, ulps, what):
    ref32 = ref64.to(torch.float32)
    tol = ulps * torch.from_numpy(np.spacing(np.abs(ref32.cpu().numpy()))).to(ref64.device).double()
    err = (got.double() - ref64).abs()
    assert bool((err <= tol).all()), "%s: %.3g ulp" % (what, float((err / tol.clamp_min(1e-300)).max()) * ulps)


def _reader(case):
    from futuredet_amd.readers import PillarFeatureNet

    net = PillarFeatureNet(num_input_features=NDIM, num_filters=[64, 64], with_distance=CASES[case], voxel_size=VS, pc_range=RG)
    net.load_state_dict({k.split("/sd/")[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith(case + "/sd/")})
    return net.to(DEV).train()


def _params(net):
    l1, l2 = net.pfn_layers
    return (l1.linear.weight.detach(), l1.norm.weight.detach(), l1.norm.bias.detach(), l2.linear.weight.detach(),
            l2.norm.weight.detach(), l2.norm.bias.detach())


def _geom(net):
    return (net.vx, net.vy, net.x_offset, net.y_offset)


_PILLARS = {}


def _pillars(m):
    """m seeded pillars of the 64 x 64 grid: 1..P points inside their cell, zero slots behind (computed once per size, never changed)"""
    if m not in _PILLARS:
        rng = np.random.default_rng(1000 + m)
        num = rng.integers(1, P + 1, m).astype(np.int32)
        cell = rng.integers(0, 64, (m, 2))
        coors = np.stack([np.zeros(m, np.int64), np.zeros(m, np.int64), cell[:, 0], cell[:, 1]], 1).astype(np.int32)
        pts = np.zeros((m, P, NDIM), np.float32)
        pts[:, :, 0] = RG[0] + (cell[:, 1, None] + rng.uniform(0, 1, (m, P))) * VS[0]
        pts[:, :, 1] = RG[1] + (cell[:, 0, None] + rng.uniform(0, 1, (m, P))) * VS[1]
        pts[:, :, 2] = rng.uniform(RG[2], RG[5], (m, P))
        pts[:, :, 3] = rng.uniform(0, 255, (m, P))
        pts[:, :, 4] = rng.uniform(0, 0.5, (m, P))
        pts *= (np.arange(P)[None, :] < num[:, None])[..., None]
        _PILLARS[m] = tuple(torch.from_numpy(a).to(DEV) for a in (pts, num, coors))
    return _PILLARS[m]


def _segmented(n_seg, stride, counts, width=64):
    """the compacted pillars and douts of a case, and the same laid out in n_seg segments with poisoned rows behind the counts"""
    live = [min(max(c, 0), stride) for c in counts]
    m = sum(live)
    vox, num, coors = _pillars(max(m, 1))
    vox, num, coors = vox[:m], num[:m], coors[:m]
    dout = torch.from_numpy(np.random.default_rng(43 + m).standard_normal((m, width)).astype(np.float32)).to(DEV)
    rows = n_seg * stride
    pv = torch.full((rows, P, NDIM), float("nan"), device=DEV)
    pn = torch.full((rows,), 1 << 30, dtype=torch.int32, device=DEV)
    pc = torch.full((rows, 4), -1, dtype=torch.int32, device=DEV)
    pd = torch.full((rows, width), float("nan"), device=DEV)
    sel, o = [], 0
    for b, c in enumerate(live):
        sel.append(torch.arange(b * stride, b * stride + c, device=DEV))
        o += c
    sel = torch.cat(sel) if sel else torch.zeros((0,), dtype=torch.long, device=DEV)
    pv[sel], pn[sel], pc[sel], pd[sel] = vox, num, coors, dout
    return (vox, num, coors, dout), (pv, pn, pc, pd), sel, torch.tensor(counts, dtype=torch.int32, device=DEV)


def _run_host(hip, net, vox, num, coors, dout):
    w1, g1, b1, w2, g2, b2 = _params(net)
    n1, n2 = net.pfn_layers[0].norm, net.pfn_layers[1].norm
    fwd = hip.pillar_train_forward(vox, num, coors, _geom(net), w1, g1, b1, n1.eps, w2, g2, b2, n2.eps, with_distance=net._with_distance)
    grads = hip.pillar_train_backward(dout, vox, num, coors, _geom(net), w1, g1, b1, w2, g2, b2, fwd[5], with_distance=net._with_distance)
    return list(fwd[:5]), list(grads)


def _run_dev(hip, net, pv, pn, pc, pd, counts, workspace=None, out=None):
    w1, g1, b1, w2, g2, b2 = _params(net)
    n1, n2 = net.pfn_layers[0].norm, net.pfn_layers[1].norm
    fwd = hip.pillar_train_forward_dev(pv, pn, pc, counts, _geom(net), w1, g1, b1, n1.eps, w2, g2, b2, n2.eps,
                                       with_distance=net._with_distance, workspace=workspace, out=out)
    grads = hip.pillar_train_backward_dev(pd, pv, pn, pc, counts, _geom(net), w1, g1, b1, w2, g2, b2, fwd[5], with_distance=net._with_distance)
    return list(fwd[:5]), list(grads)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------ 1: the reader
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n_seg,stride,counts", SEGMENTS, ids=["one", "edge-in-block", "empty-middle", "full", "clamped", "ppb-from-total"])
def test_device_counts_give_the_host_count_bits(hip, case, n_seg, stride, counts):
    net = _reader(case)
    (vox, num, coors, dout), (pv, pn, pc, pd), sel, cdev = _segmented(n_seg, stride, counts)
    want_f, want_g = _run_host(hip, net, vox, num, coors, dout)
    got_f, got_g = _run_dev(hip, net, pv, pn, pc, pd, cdev)
    torch.cuda.synchronize()
    out = got_f[0]
    assert tuple(out.shape) == (n_seg * stride, 64)
    assert torch.equal(_bits(out[sel]), _bits(want_f[0])), "live rows of out"
    behind = torch.ones(out.shape[0], dtype=torch.bool, device=DEV)
    behind[sel] = False
    assert int(behind.sum()) == n_seg * stride - len(sel) and bool((_bits(out[behind]) == 0).all()), "rows behind the counts are +0"
    for name, a, b in zip(("mean1", "var1", "mean2", "var2"), got_f[1:], want_f[1:]):
        assert torch.equal(_bits(a), _bits(b)), name
    for name, a, b in zip(("dw1", "dgamma1", "dbeta1", "dw2", "dgamma2", "dbeta2"), got_g, want_g):
        assert bool(torch.isfinite(a).all()) and torch.equal(_bits(a), _bits(b)), name
    again_f, again_g = _run_dev(hip, net, pv, pn, pc, pd, cdev)
    for a, b in zip(got_f + got_g, again_f + again_g):
        assert torch.equal(_bits(a), _bits(b)), "a second run gives the same bytes"
    if counts == [-3, 70]:  # the clamped counts are [0, 64]
        (_, _, _, _), (qv, qn, qc, qd), _, c2 = _segmented(2, 64, [0, 64])
        f2, g2 = _run_dev(hip, net, qv, qn, qc, qd, c2)
        for a, b in zip(got_f + got_g, f2 + g2):
            assert torch.equal(_bits(a), _bits(b))


def test_empty_batch_is_all_zero(hip):
    net = _reader("plain")
    _, (pv, pn, pc, pd), sel, cdev = _segmented(2, 64, [0, 0])
    assert len(sel) == 0
    fwd, grads = _run_dev(hip, net, pv, pn, pc, pd, cdev)  # (a non-zero status raises)
    for t in fwd + grads:
        assert bool((_bits(t) == 0).all())
    rm, rv = torch.randn(32, device=DEV), torch.rand(32, device=DEV) + 0.5
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    rm0, rv0 = rm.clone(), rv.clone()
    hip.pillar_train_running_stats_dev(fwd[1], fwd[2], 0.01, cdev, 64, P, rm, rv, nbt)
    torch.cuda.synchronize()
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and int(nbt) == 5
    # the module form: zeros out, buffers untouched
    bufs = [b.clone() for b in net.buffers()]
    out = net.forward_train_static(pv.view(2, 64, P, NDIM), pn.view(2, 64), pc.view(2, 64, 4), cdev)
    out.sum().backward()
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and all(torch.equal(a, b) for a, b in zip(bufs, net.buffers()))
    assert all(bool((p.grad == 0).all()) for p in net.parameters())


@pytest.mark.parametrize("case", sorted(CASES))
def test_running_statistics_on_the_device(hip, case):
    net = _reader(case)
    n_seg, stride, counts = 2, 64, [17, 23]
    (vox, num, coors, dout), (pv, pn, pc, pd), sel, cdev = _segmented(n_seg, stride, counts)
    fwd, _ = _run_dev(hip, net, pv, pn, pc, pd, cdev)
    n = float(P * sum(counts))
    g = torch.Generator(device="cpu").manual_seed(3)
    for mean, var, c in ((fwd[1], fwd[2], 32), (fwd[3], fwd[4], 64)):
        for f in (0.01, 0.1, 1.0):
            rm = torch.randn(c, generator=g).to(DEV)
            rv = (torch.rand(c, generator=g) + 0.5).to(DEV)
            nbt = torch.tensor(0, dtype=torch.int64, device=DEV)
            want_m = (1.0 - f) * rm.double() + f * mean.double()
            want_v = (1.0 - f) * rv.double() + f * var.double() * (n / (n - 1.0))
            hip.pillar_train_running_stats_dev(mean, var, f, cdev, stride, P, rm, rv, nbt)
            torch.cuda.synchronize()
            _ulp_close(rm, want_m, 2, "%s running_mean f=%g" % (case, f))
            _ulp_close(rv, want_v, 2, "%s running_var f=%g" % (case, f))
            assert int(nbt) == 1
    # module level: the static form and today's host-count form, from equal (default) buffers
    a, b = _reader(case), _reader(case)
    for net_ in (a, b):
        for pfn in net_.pfn_layers:
            pfn.norm.reset_running_stats()
    out_a = a.forward_train_static(pv.view(n_seg, stride, P, NDIM), pn.view(n_seg, stride), pc.view(n_seg, stride, 4), cdev)
    out_b = b(vox, num, coors)
    out_a.backward(torch.nan_to_num(pd, nan=0.0))
    out_b.backward(dout)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_a[sel]), _bits(out_b))
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(_bits(pa.grad), _bits(pb.grad)), k
    for la, lb in zip(a.pfn_layers, b.pfn_layers):
        assert int(la.norm.num_batches_tracked) == int(lb.norm.num_batches_tracked) == 1
        _ulp_close(la.norm.running_mean, lb.norm.running_mean.double(), 2, "module running_mean")
        _ulp_close(la.norm.running_var, lb.norm.running_var.double(), 2, "module running_var")
        assert not torch.equal(la.norm.running_var, torch.ones_like(la.norm.running_var))


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_scatter_backward_with_a_device_count(hip, channels_last):
    rng = np.random.default_rng(3)
    B, C, ny, nx, cap = 2, 64, 48, 40, 700
    dcanvas = torch.randn((B, C, ny, nx), device=DEV)
    if channels_last:
        dcanvas = dcanvas.contiguous(memory_format=torch.channels_last)
    for b, count in ((0, 437), (1, 0), (1, 700), (0, 1)):
        cells = rng.choice(ny * nx, cap, replace=False)
        coors = torch.from_numpy(np.stack([np.full(cap, b), np.zeros(cap, int), cells // nx, cells % nx], 1).astype(np.int32)).to(DEV)
        want = hip.pillar_scatter_backward(dcanvas, coors[:count].contiguous())
        assert torch.equal(want, dcanvas[coors[:count, 0].long(), :, coors[:count, 2].long(), coors[:count, 3].long()])
        poisoned = coors.clone()
        poisoned[count:] = -1
        got = hip.pillar_scatter_backward(dcanvas, poisoned, n_dev=torch.tensor([count], dtype=torch.int32, device=DEV))
        assert tuple(got.shape) == (cap, C)
        assert torch.equal(got[:count], want) and bool((_bits(got[count:]) == 0).all()), (b, count)


def test_graph_replay_gives_the_eager_bytes(hip):
    """forward, the two running-statistics updates and backward as one linear graph"""
    net = _reader("distance")
    n_seg, stride, counts = 3, 32, [16, 0, 1]
    _, (pv, pn, pc, pd), sel, cdev = _segmented(n_seg, stride, counts)
    bufs0 = [torch.randn(32, device=DEV), torch.rand(32, device=DEV) + 0.5, torch.randn(64, device=DEV), torch.rand(64, device=DEV) + 0.5]

    def run(bufs, nbt, workspace=None, out=None):
        w1, g1, b1, w2, g2, b2 = _params(net)
        n1, n2 = net.pfn_layers[0].norm, net.pfn_layers[1].norm
        f = hip.pillar_train_forward_dev(pv, pn, pc, cdev, _geom(net), w1, g1, b1, n1.eps, w2, g2, b2, n2.eps, with_distance=True,
                                         workspace=workspace, out=out)
        hip.pillar_train_running_stats_dev(f[1], f[2], 0.01, cdev, stride, P, bufs[0], bufs[1], nbt)
        hip.pillar_train_running_stats_dev(f[3], f[4], 0.01, cdev, stride, P, bufs[2], bufs[3], None)
        grads = hip.pillar_train_backward_dev(pd, pv, pn, pc, cdev, _geom(net), w1, g1, b1, w2, g2, b2, f[5], with_distance=True)
        return list(f[:5]) + list(grads)

    eager_bufs, eager_nbt = [b.clone() for b in bufs0], torch.tensor(0, dtype=torch.int64, device=DEV)
    want = run(eager_bufs, eager_nbt)
    ws = torch.empty((hip.pillar_train_workspace_bytes(n_seg * stride, P),), dtype=torch.uint8, device=DEV)
    out = torch.empty((n_seg * stride, 64), dtype=torch.float32, device=DEV)
    bufs, nbt = [b.clone() for b in bufs0], torch.tensor(0, dtype=torch.int64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(bufs, nbt, workspace=ws, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = run(bufs, nbt, workspace=ws, out=out)
    out.zero_()
    ws.zero_()
    for b, b0 in zip(bufs, bufs0):
        b.copy_(b0)
    nbt.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(want + eager_bufs, got + bufs):
        assert torch.equal(_bits(x), _bits(y))
    assert int(nbt) == int(eager_nbt) == 1


# ------------------------------------------------------------------------------------------------------------------- 2: PointPillars
def _flat(losses):
    out = {}
    for k in sorted(losses):
        stack = [(k, losses[k])]
        while stack:
            name, v = stack.pop(0)
            if isinstance(v, torch.Tensor):
                out[name] = v.detach().clone()
            else:
                stack = [("%s.%d" % (name, i), x) for i, x in enumerate(v)] + stack
    return out


LOSS_KEYS = ("loss", "hm_loss", "loc_loss", "num_positive")


@pytest.fixture
def deterministic_convs():
    """torch's own convolutions of the RPN and the head (MIOpen) pick kernels whose sums change from run to run: two passes of ONE path
    differ in every map behind the first convolution, while the canvas in front of it is bit-equal.  A comparison that asks for the same
    bits whatever two eager runs do runs with the deterministic kernel choice.  Those kernels are slow (seconds per backward pass at
    512 x 512) and torch keeps a shape's choice for the rest of the process, so only the B = 2 test uses this, and no other test
    here runs its shapes."""
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


class _Pillars(object):
    """pointpillars_config() with seeded weights (as test_pointpillars_training_step), fused_loss on, and everything a step needs"""

    def __init__(self):
        from futuredet_amd import build_detector, solver
        from futuredet_amd.configs import pointpillars_config
        from futuredet_amd.synth import seeded_state_dict, tame_box_dims
        from futuredet_amd.targets import TargetAssigner

        cfg = pointpillars_config()
        self.cfg = cfg
        self.vg = dict(cfg.voxel_generator, max_voxel_num=[16384, 16384])
        net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        sd = tame_box_dims(seeded_state_dict(net, 9))
        sd["reader.pfn_layers.0.linear.weight"] = sd["reader.pfn_layers.0.linear.weight"] * 0.02
        net.load_state_dict(sd, strict=False)
        self.net = net.to(DEV).train()
        self.net.bbox_head.fused_loss = True
        self.state0 = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.grid = np.array([512, 512, 1])
        self.ta = TargetAssigner(cfg.train_cfg.assigner, self.grid, self.vg["range"], self.vg["voxel_size"])
        self.opt = solver.build_one_cycle_optimizer(self.net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        self.sched = solver.create_learning_rate_scheduler(self.opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0,
                                                                        pct_start=0.4), 10)
        self.solver = solver

    def fresh(self):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.state0[k])
            t = self.opt._table
            t.exp_avg.zero_(), t.exp_avg_sq.zero_(), t.step.zero_()
        self.net.train()

    def state(self):
        t = self.opt._table
        out = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        out.update({"opt.exp_avg": t.exp_avg.clone(), "opt.exp_avg_sq": t.exp_avg_sq.clone(), "opt.step": t.step.clone()})
        return out

    def batch(self, seeds, points):
        from futuredet_amd.synth import synthetic_cloud
        from test_gpu_loss import _synthetic_gt

        gt = _synthetic_gt(np.random.default_rng(100 + seeds[0]), len(seeds), self.cfg.timesteps, 24)
        b = dict(clouds=[torch.from_numpy(synthetic_cloud(seed=s, target_points=p)).to(DEV) for s, p in zip(seeds, points)],
                 gt_boxes=torch.from_numpy(gt[0]).to(DEV), gt_counts=torch.from_numpy(gt[1]).to(DEV), gt_classes=torch.from_numpy(gt[2]).to(DEV))
        if self.ta.extra_sets:
            b["gt_trajectory"] = torch.from_numpy(gt[3]).to(DEV)
        return b

    def targets(self, batch):
        return self.ta(batch["gt_boxes"], batch["gt_counts"], batch["gt_classes"], batch.get("gt_trajectory"))

    def step(self, B, clip=NO_CLIP, **kw):
        return self.solver.StaticPillarsTrainStep(self.net, self.vg, self.ta, self.opt, self.sched, clip, capacity=32768, batch_size=B,
                                                  max_gt=32, **kw)

    def device_example(self, hip, batch):
        """train_steps' collated example from the DEVICE voxeliser's own output, read back and concatenated"""
        vg = self.vg
        cap, mp = vg["max_voxel_num"][0], vg["max_points_in_voxel"]
        parts = []
        for b, pts in enumerate(batch["clouds"]):
            out = dict(voxels=torch.empty((cap, mp, 5), device=DEV), coors=torch.empty((cap, 4), dtype=torch.int32, device=DEV),
                       num_points=torch.empty((cap,), dtype=torch.int32, device=DEV), num_voxels=torch.empty((1,), dtype=torch.int32, device=DEV))
            hip.voxelize(pts, vg["voxel_size"], vg["range"], mp, cap, batch_idx=b, want_voxels=True, coor_cols=4, out=out)
            n = int(out["num_voxels"])
            parts.append((out["voxels"][:n], out["coors"][:n], out["num_points"][:n], n))
        targets = self.targets(batch)
        ex = dict(voxels=torch.cat([p[0] for p in parts]), coordinates=torch.cat([p[1] for p in parts]),
                  num_points=torch.cat([p[2] for p in parts]), num_voxels=torch.tensor([p[3] for p in parts]), shape=np.array([self.grid]),
                  metadata=[None] * len(parts))
        ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
        return ex


@pytest.fixture(scope="module")
def pillars(hip):
    return _Pillars()


def test_forward_points_train_static_against_host_counts(pillars, deterministic_convs):
    w = pillars
    batch = w.batch([2, 3], [30000, 20000])
    clouds, counts = [], []
    for c in batch["clouds"]:
        buf = torch.full((32768, 5), float("nan"), device=DEV)
        buf[: c.shape[0]] = c
        clouds.append(buf)
        counts.append(torch.tensor([c.shape[0]], dtype=torch.int32, device=DEV))
    example = w.targets(batch)

    def run(static):
        w.fresh()
        w.opt.zero_grad()
        losses = w.net.forward_points_train(clouds, w.vg, example, counts=counts, static=static)
        nvox = w.net.last_level_counts
        sum(losses["loss"]).backward()
        torch.cuda.synchronize()
        return _flat({k: losses[k] for k in LOSS_KEYS}), {k: p.grad.clone() for k, p in w.net.named_parameters() if p.requires_grad}, nvox

    la, ga, na = run(True)
    lb, gb, nb = run(False)
    assert isinstance(na, torch.Tensor) and torch.equal(na, nb) and na.dtype == torch.int32 and min(na.tolist()) > 1000
    assert la.keys() == lb.keys() and ga.keys() == gb.keys()
    for k in la:
        assert bool(torch.isfinite(la[k]).all()) and torch.equal(la[k], lb[k]), k
    for k in ga:
        assert torch.equal(_bits(ga[k]), _bits(gb[k])), k
    assert all(bool((ga[k] != 0).any()) for k in ga if k.startswith("reader."))


def test_no_synchronisation_in_the_pillars_step(pillars):
    w = pillars
    w.fresh()
    step = w.step(1)
    b1, b2 = w.batch([1], [3000]), w.batch([3], [4000])
    step.warm_up([b1])
    step(b1)  # first call: scratch allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(b2)
        out = step(b1, check=True)  # nothing is read back
        with pytest.raises(RuntimeError):
            out["loss"][0].item()  # the mode is enforced
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert step.iteration == 3 and not step.overflowed()
    assert bool(torch.isfinite(out["loss"][0])) and bool(torch.isfinite(out["total_norm"]))
    assert [int(b.norm.num_batches_tracked) for b in w.net.reader.pfn_layers] == [3, 3]


def _reader_stat(k):
    return k.startswith("reader.") and k.endswith(("running_mean", "running_var"))


def test_one_pillars_step_against_the_eager_loop(hip, pillars):
    w = pillars
    batch = w.batch([5], [20000])
    ex = w.device_example(hip, batch)
    keys = LOSS_KEYS + ("total_norm",)

    def eager():
        w.fresh()
        losses = next(w.solver.train_steps(w.net, [ex], w.opt, w.sched, grad_clip=NO_CLIP))
        torch.cuda.synchronize()
        return _flat({k: losses[k] for k in keys}), w.state()

    l1, s1 = eager()
    l2, s2 = eager()
    same = all(torch.equal(l1[k], l2[k]) for k in l1) and all(torch.equal(s1[k], s2[k]) for k in s1)

    def group(name):  # one yardstick per kind of number: a gradient norm of 1e5 says nothing about a loss term or a weight
        return "total_norm" if name == "total_norm" else "loss terms" if name in l1 else "state"

    spread = {}
    for name, a, b in [(k, l1[k], l2[k]) for k in l1] + [(k, s1[k], s2[k]) for k in s1 if not k.startswith("opt.")]:
        spread[group(name)] = max(spread.get(group(name), 0.0), float((a.double() - b.double()).abs().max()))
    print("[pillars_static] two eager train_steps runs from one state %s (largest differences %s)" % (
        "agree bit for bit" if same else "differ", ", ".join("%s %.3e" % kv for kv in sorted(spread.items()))))

    w.fresh()
    step = w.step(1)
    step.warm_up([batch])
    before = w.state()
    assert all(torch.equal(before[k], w.state0[k]) for k in w.state0), "warm_up restores the model"
    assert int(w.opt._table.step.max()) == 0 and step.iteration == 0
    out = step(batch)
    torch.cuda.synchronize()
    ls, ss = _flat({k: out[k] for k in keys}), w.state()
    assert step.iteration == 1 and int(w.opt._table.step.min()) == 1 and float(ls["total_norm"]) < NO_CLIP["max_norm"]
    assert l1.keys() == ls.keys() and s1.keys() == ss.keys()
    for name, a, b in [(k, l1[k], ls[k]) for k in l1] + [(k, s1[k], ss[k]) for k in s1]:
        if _reader_stat(name):  # torch's update against the device kernel's: see the module docstring
            tol = 2.0 ** -22 * (w.state0[name].double().abs() + a.double().abs())
            err = (a.double() - b.double()).abs()
            assert bool((err <= tol).all()), "%s: %.3g of the bound" % (name, float((err / tol.clamp_min(1e-300)).max()))
        elif same:
            assert torch.equal(a, b), name
        elif not name.startswith("opt."):
            d = float((a.double() - b.double()).abs().max())
            assert d <= 4.0 * spread[group(name)], "two eager runs differ by up to %.3e in the %s: bound 4x; %s differs by %.3e" % (
                spread[group(name)], group(name), name, d)


# ----------------------------------------------------------------------------------------------------------------------- 3: map head
MAX_VOXELS = 8192
GRID = np.array([1440, 1440, 40])


class _MapWorld(object):
    """forecast_n3dtfm on the geometry of test_gpu_train_static._World: seeded weights, fused_bn and fused_loss on"""

    def __init__(self):
        from futuredet_amd import build_detector, solver
        from futuredet_amd.configs import centerpoint_config
        from futuredet_amd.synth import seeded_state_dict, tame_box_dims
        from futuredet_amd.targets import TargetAssigner

        cfg = centerpoint_config("forecast_n3dtfm")
        self.cfg = cfg
        self.vg = dict(cfg.voxel_generator, max_voxel_num=[MAX_VOXELS, MAX_VOXELS])
        net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
        self.net = net.to(DEV).train()
        self.net.backbone.fused_bn = True
        self.net.bbox_head.fused_loss = True
        self.state0 = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.ta = TargetAssigner(cfg.train_cfg.assigner, GRID, self.vg["range"], self.vg["voxel_size"])
        self.opt = solver.build_one_cycle_optimizer(self.net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        self.sched = solver.create_learning_rate_scheduler(self.opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0,
                                                                        pct_start=0.4), 10)
        self.solver = solver

    def fresh(self, dtype=torch.float32, fused_bn=False):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.state0[k])
            t = self.opt._table
            t.exp_avg.zero_(), t.exp_avg_sq.zero_(), t.step.zero_()
        n = self.net
        n.backbone.train_dtype = n.neck.train_dtype = n.bbox_head.train_dtype = dtype
        n.neck.fused_bn = n.bbox_head.fused_bn = fused_bn
        n.train()

    state = _Pillars.state
    targets = _Pillars.targets

    def batch(self, seed, points, map_seed):
        b = _Pillars.batch(self, [seed], [points])
        g = torch.Generator(device="cpu").manual_seed(map_seed)
        b["bev_map"] = torch.rand((1, 6, self.ta.H, self.ta.W), generator=g).to(DEV)
        return b

    def step(self, **kw):
        return self.solver.StaticTrainStep(self.net, self.vg, self.ta, self.opt, self.sched, NO_CLIP, capacity=8192, batch_size=1, max_gt=32, **kw)

    def host_example(self, batch):
        from front_end_ref import mean_seq
        from futuredet_amd.voxelize import points_to_voxel

        v, c, n = points_to_voxel(batch["clouds"][0].cpu().numpy(), self.vg["voxel_size"], self.vg["range"], 10, True, MAX_VOXELS)
        targets = self.targets(batch)
        ex = dict(voxels=torch.from_numpy(mean_seq(v, n)).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
                  num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([GRID]), metadata=[None],
                  bev_map=[batch["bev_map"][:, i] for i in range(6)])
        ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
        return ex


@pytest.fixture(scope="module")
def mapworld(hip):
    return _MapWorld()


def test_map_head_step_against_the_eager_loop(mapworld):
    from test_gpu_train_static import _compare, _is_block_bias

    w = mapworld
    assert w.net.bbox_head.bev_map and (w.ta.H, w.ta.W) == (180, 180)
    batch = w.batch(5, 4000, 1)
    ex = w.host_example(batch)
    keys = LOSS_KEYS + ("total_norm",)

    def eager():
        w.fresh()
        losses = next(w.solver.train_steps(w.net, [ex], w.opt, w.sched, grad_clip=NO_CLIP))
        torch.cuda.synchronize()
        bias_grads = torch.cat([p.grad.flatten() for k, p in w.net.named_parameters() if _is_block_bias(k)]).clone()
        return _flat({k: losses[k] for k in keys}), w.state(), bias_grads

    l1, s1, g1 = eager()
    l2, s2, _ = eager()
    same = all(torch.equal(l1[k], l2[k]) for k in l1) and all(torch.equal(s1[k], s2[k]) for k in s1)
    spread = max([float((l1[k].double() - l2[k].double()).abs().max()) for k in l1] + [float((s1[k].double() - s2[k].double()).abs().max()) for k in s1])
    print("[map_head] two eager train_steps runs from one state %s (largest difference %.3e)" % ("agree bit for bit" if same else "differ", spread))

    w.fresh()
    step = w.step()
    step.warm_up([batch])
    assert all(torch.equal(v, w.state0[k]) for k, v in w.net.state_dict().items()), "warm_up restores the model"
    out = step(batch)
    torch.cuda.synchronize()
    ls, ss = _flat({k: out[k] for k in keys}), w.state()
    gs = torch.cat([p.grad.flatten() for k, p in w.net.named_parameters() if _is_block_bias(k)])
    lr = w.opt.lr
    assert step.iteration == 1 and int(w.opt._table.step.min()) == 1 and not step.overflowed()
    assert torch.equal(step.bev, batch["bev_map"])
    if same:
        _compare(l1, ls, lr, False, "loss terms")
        _compare(s1, ss, lr, False, "state")
        slack = float((gs.double() - g1.double()).norm()) + 2.0 * float(np.spacing(np.float32(l1["total_norm"].item())))
        assert abs(float(ls["total_norm"]) - float(l1["total_norm"])) <= slack
    else:
        bound = 4.0 * spread
        for name, a, b in [(k, l1[k], ls[k]) for k in l1] + [(k, s1[k], ss[k]) for k in s1 if not k.startswith("opt.")]:
            d = float((a.double() - b.double()).abs().max())
            limit = max(bound, 2.0 * lr * (1.0 + 2.0 ** -20)) if _is_block_bias(name) else bound
            assert d <= limit, "two eager runs differ by up to %.3e: bound 4x = %.3e; %s differs by %.3e" % (spread, bound, name, d)

    # the same cloud with another map: the input reaches the head
    w.fresh()
    other = step(dict(batch, bev_map=w.batch(5, 4000, 2)["bev_map"]))
    torch.cuda.synchronize()
    assert not torch.equal(other["loss"][0], out["loss"][0])
    with pytest.raises(ValueError, match="bev_map"):
        step({k: v for k, v in batch.items() if k != "bev_map"})
    with pytest.raises(ValueError, match="does not fit"):
        step(dict(batch, bev_map=batch["bev_map"][:, :, :90]))


def test_map_head_overflow_is_rerun_with_the_map(mapworld):
    w = mapworld
    batch = w.batch(6, 4000, 3)
    w.fresh()
    step = w.step()
    step.warm_up([batch])
    full = list(step.expected)
    step.row_caps_mode = [MAX_VOXELS] + [max(e // 3, 64) for e in full[1:]]  # too few rows on the deeper levels
    step.reset()
    out = step(batch, check=False)
    torch.cuda.synchronize()
    assert step.overflowed() and int(step.skip) == 1 and int(w.opt._table.step.max()) == 0, "the device skipped the update"
    w.fresh()
    step.iteration = 0
    out = step(batch, check=True)
    torch.cuda.synchronize()
    assert step.iteration == 1 and w.opt._table.step.cpu().tolist() == [1] * w.opt._table.step.numel()
    assert bool(torch.isfinite(out["loss"][0]))
    # the re-run saw the map: against the host-sized step of the same batch with another map
    rerun_loss = out["loss"][0].clone()
    w.fresh()
    step.iteration = 0
    other = step(dict(batch, bev_map=w.batch(6, 4000, 4)["bev_map"]), check=True)
    torch.cuda.synchronize()
    assert not torch.equal(other["loss"][0], rerun_loss)


def test_map_head_step_in_bf16(mapworld):
    w = mapworld
    batch = w.batch(7, 4000, 5)
    w.fresh(torch.bfloat16, fused_bn=True)
    try:
        step = w.step()
        step.warm_up([batch])
        out = step(batch, check=False)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["loss"][0])) and not step.overflowed()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = step(batch, check=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["loss"][0])) and bool(torch.isfinite(out["total_norm"])) and step.iteration == 2
    finally:
        w.fresh()
