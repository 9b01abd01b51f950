"""Mixed-precision training of the dense stride-1 convolutions on the device: the kernels of fd_conv2d_grad_bf16.hip (device weight
packer, weight gradient), the autograd surface dense_train.conv2d_bf16 and the neck's switch RPN.train_dtype, against float64
restatements on the bf16-rounded operands.

Bounds (test_gpu_spconv_grad_bf16.py).  bf16 x bf16 products are exact in fp32, so a result that is not rounded again (dW) differs from
float64 only by the fp32 accumulation: 1e-4 * scale, scale = max(1, max |ref|).  A result that is rounded once to bf16 (y, dX; round to
nearest even, unit roundoff 2^-8 taken generously) gets |got - ref| <= 2^-8 |ref| + 1.01e-4 * scale.

Shapes (B, H, W, Cin, Cout, ks): the smallest that reach every boundary of the forward kernel's 8 x 16 tile, the 32-channel slices and
the weight gradient's pixel chunks."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
U = 2.0 ** -8

CASES = [(1, 3, 5, 32, 32, 3),        # a map smaller than one tile
         (2, 9, 17, 32, 64, 3),       # one pixel past the tile in both directions, two maps
         (2, 20, 28, 64, 96, 3),      # ragged both ways, three output blocks
         (1, 12, 20, 128, 128, 3), (1, 10, 12, 256, 128, 3), (1, 10, 12, 256, 256, 3),  # the shipped channel pairs
         (2, 20, 28, 128, 256, 1),    # the 1 x 1 deblock
         "chunks"]                    # B = 1, H = 1, W = 2 chunk + 1, 32 -> 32, ks 3: two chunks of pixels and one pixel of a third


def _case(case):
    if case == "chunks":
        from futuredet_amd import hip_ops

        return (1, 1, 2 * hip_ops.conv2d_wgrad_bf16_chunk() + 1, 32, 32, 3)
    return case


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(name, got, ref, tol=1e-4):
    """element-wise |got - ref| <= tol * scale, scale = max(1, max |ref|): results that are not rounded to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert_close(name, got / scale, ref / scale, tol)


def _close_rounded(name, got, ref):
    """|got - ref| <= 2^-8 |ref| + 1.01e-4 * scale: results rounded once to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    excess = float(((np.abs(got - ref) - U * np.abs(ref)) / scale).max()) if ref.size else 0.0
    report(name + " (beyond 2^-8 |ref|, / scale)", excess, 1.01e-4)
    assert excess <= 1.01e-4, "%s: |got - ref| - 2^-8 |ref| = %.3e * scale > 1.01e-4 * scale" % (name, excess)


def _bf16_values(rng, shape):
    """uniform (-1, 1), rounded to bf16, as float32"""
    return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(BF).float()


def _reference64(x_nhwc, w, dy_nhwc, ks):
    """float64 F.conv2d and its autograd on the CPU: (y, dx) NHWC, dW OIHW"""
    x = x_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    y = F.conv2d(x, w, padding=ks // 2)
    y.backward(dy_nhwc.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w.grad


def _run(x_nhwc, w, dy_nhwc, ks):
    """conv2d_bf16 forward + backward on the device: (y, dx) bf16 NHWC, dW fp32 OIHW"""
    from futuredet_amd import dense_train

    x = x_nhwc.to(DEV).to(BF).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    y = dense_train.conv2d_bf16(x, w, ks)
    y.backward(dy_nhwc.to(DEV).to(BF))
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad


_problems = {}


def _problem(case):
    """operands (uniform (-1, 1) rounded to bf16) and the float64 reference of a case: computed once, shared, never modified"""
    if case not in _problems:
        B, H, W, cin, cout, ks = _case(case)
        rng = np.random.default_rng(1000 + len(_problems))
        x, w, dy = _bf16_values(rng, (B, H, W, cin)), _bf16_values(rng, (cout, cin, ks, ks)), _bf16_values(rng, (B, H, W, cout))
        _problems[case] = (x, w, dy, ks) + _reference64(x, w, dy, ks)
    return _problems[case]


# ------------------------------------------------------------------------------------------------ 1. the packer
def _tie_weights(rng, shape):
    """fp32 weights of which a third sit exactly half way between two bf16 values (both parities of the lower neighbour), the rest
    have random low bits"""
    v = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))
    bits = v.view(torch.int32)
    kind = torch.from_numpy(rng.integers(0, 3, shape).astype(np.int32))
    tie = (bits & ~0xFFFF) | 0x8000
    return torch.where(kind == 0, tie, bits).view(torch.float32).contiguous()


@pytest.mark.parametrize("cout,cin,ks", sorted({(_c[4], _c[3], _c[5]) for _c in CASES if _c != "chunks"} | {(40, 32, 3), (40, 64, 1)}))
def test_device_pack_is_byte_identical_to_the_host_pack(hip, cout, cin, ks):
    w = _tie_weights(np.random.default_rng(cout * 7 + cin + ks), (cout, cin, ks, ks))
    bits = w.view(torch.int32)
    assert int(((bits & 0xFFFF) == 0x8000).sum()) > w.numel() // 6  # the ties are there, on even and odd neighbours
    assert int((((bits >> 16) & 1) == 1).sum()) > 0 and int((((bits >> 16) & 1) == 0).sum()) > 0
    wd = w.to(DEV)
    assert torch.equal(hip.pack_conv2d_weight_device(wd).cpu(), hip.pack_conv2d_weight(w))
    if cout % 32 == 0:
        want = hip.pack_conv2d_weight(w.flip(2, 3).transpose(0, 1).contiguous())
        got = hip.pack_conv2d_weight_device(wd, transposed=True).cpu()
        assert got.numel() == want.numel() and torch.equal(got, want)
    else:
        with pytest.raises(hip.FutureDetHipError, match="Cout % 32 == 0"):
            hip.pack_conv2d_weight_device(wd, transposed=True)


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv_matches_float64_on_the_rounded_operands(hip, case):
    x, w, dy, ks, y_ref, dx_ref, dw_ref = _problem(case)
    y, dx, dw = _run(x, w, dy, ks)
    assert y.dtype == BF and dx.dtype == BF and dw.dtype == torch.float32 and tuple(dw.shape) == tuple(w.shape)
    name = "conv2d_bf16 %s" % (_case(case),)
    _close_rounded(name + " y", _np(y), y_ref.numpy())
    _close_rounded(name + " dx", _np(dx), dx_ref.numpy())
    _close(name + " dW", _np(dw), dw_ref.numpy())


# ------------------------------------------------------------------------------------------------ 3. exact structure
def test_one_tap_permutation_weight_shifts_and_permutes_exactly(hip):
    """w non-zero at tap (ky, kx) = (0, 2) only, a channel permutation there: y[b, y, x, co] = x[b, y - 1, x + 1, perm[co]] and
    dx[b, y, x, perm[co]] = dy[b, y + 1, x - 1, co], zeros shifted in at the border.  No tolerance."""
    rng = np.random.default_rng(5)
    B, H, W, C = 2, 9, 17, 32
    perm = rng.permutation(C)
    w = torch.zeros((C, C, 3, 3))
    w[torch.arange(C), torch.from_numpy(perm), 0, 2] = 1.0
    x, dy = _bf16_values(rng, (B, H, W, C)), _bf16_values(rng, (B, H, W, C))
    y, dx, _ = _run(x, w, dy, 3)
    want_y = torch.zeros_like(x)
    want_y[:, 1:, :-1, :] = x[:, :-1, 1:, :][..., perm]
    want_dx = torch.zeros_like(x)
    want_dx[:, :-1, 1:, :][..., perm] = dy[:, 1:, :-1, :]
    assert torch.equal(y.float().cpu(), want_y)
    assert torch.equal(dx.float().cpu(), want_dx)


def test_one_hot_pixels_give_exactly_the_expected_weight_gradient(hip):
    """x and dy one-hot at chosen (pixel, channel)s -- a corner, the last pixel of map 0 next to the first of map 1, the end of a row next
    to the start of the following one: dW has one non-zero per in-image tap, each the exact product; neighbours in memory that are not
    neighbours in the image contribute nothing."""
    B, H, W, cin, cout = 2, 9, 17, 32, 64
    xs = [(0, 0, 0, 3, 0.5), (0, 8, 16, 31, 2.0), (1, 0, 0, 0, -1.5), (1, 4, 8, 17, 3.0), (0, 3, 16, 9, -0.75), (0, 4, 0, 12, 1.25)]
    dys = [(0, 0, 0, 5, 1.0), (0, 0, 1, 6, -2.0), (0, 1, 1, 40, 0.5), (0, 8, 16, 63, 4.0), (0, 8, 15, 1, -4.0), (1, 0, 0, 33, 0.25), (1, 0, 1, 32, 8.0),
           (1, 4, 8, 17, -1.0), (1, 5, 9, 0, 2.0), (1, 3, 7, 62, 0.125), (0, 4, 0, 20, 1.5), (0, 3, 16, 21, -0.5), (0, 4, 1, 22, 3.0)]
    x, dy = torch.zeros((B, H, W, cin)), torch.zeros((B, H, W, cout))
    for b, yy, xx, c, v in xs:
        x[b, yy, xx, c] = v
    for b, yy, xx, c, v in dys:
        dy[b, yy, xx, c] = v
    want = torch.zeros((cout, cin, 3, 3))
    n_terms = 0
    for bx, yx, xx_, ci, vx in xs:
        for bd, yd, xd, co, vd in dys:
            ky, kx = yx - yd + 1, xx_ - xd + 1
            if bx == bd and 0 <= ky < 3 and 0 <= kx < 3:
                want[co, ci, ky, kx] += vx * vd
                n_terms += 1
    assert n_terms >= 12 and int((want != 0).sum()) == n_terms  # every term lands in an entry of its own
    got = hip.conv2d_wgrad_bf16(x.to(DEV).to(BF), dy.to(DEV).to(BF), 3)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want.double(), _reference64(x, torch.zeros((cout, cin, 3, 3)), dy, 3)[2])  # (the expectation itself)


def test_border_ring_gradient_is_exact_on_powers_of_two(hip):
    """dy non-zero on the border ring only, all values small powers of two: every partial sum is exact in fp32, so dW equals float64"""
    rng = np.random.default_rng(6)
    B, H, W, cin, cout = 2, 9, 17, 32, 32
    pw = np.array([0.25, 0.5, 1.0, 2.0, -0.25, -0.5, -1.0, -2.0], np.float32)
    x = torch.from_numpy(pw[rng.integers(0, 8, (B, H, W, cin))])
    dy = torch.from_numpy(pw[rng.integers(0, 8, (B, H, W, cout))])
    dy[:, 1:-1, 1:-1, :] = 0.0
    want = _reference64(x, torch.zeros((cout, cin, 3, 3)), dy, 3)[2]
    got = hip.conv2d_wgrad_bf16(x.to(DEV).to(BF), dy.to(DEV).to(BF), 3)
    assert float(want.abs().max()) > 4.0 and torch.equal(got.double().cpu(), want)


# ------------------------------------------------------------------------------------------------ 4. determinism and workspace
@pytest.mark.parametrize("case", [(2, 20, 28, 64, 96, 3), (2, 20, 28, 128, 256, 1), "chunks"], ids=str)
def test_wgrad_is_deterministic_and_reads_only_what_it_wrote(hip, case):
    from futuredet_amd import lib

    x, w, dy, ks = _problem(case)[:4]
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    xd, dyd = x.to(DEV).to(BF), dy.to(DEV).to(BF)
    first = hip.conv2d_wgrad_bf16(xd, dyd, ks)
    second = hip.conv2d_wgrad_bf16(xd, dyd, ks)
    assert torch.equal(first, second)
    L = lib.load()
    need = L.fd_conv2d_wgrad_bf16_workspace_bytes(B, H, W, cin, cout, ks)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.full((cout, cin, ks, ks), float("nan"), dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.fd_conv2d_wgrad_bf16(p(xd), p(dyd), B, H, W, cin, cout, ks, p(ws), need, p(dw), stream), "fd_conv2d_wgrad_bf16")
    torch.cuda.synchronize()
    assert torch.equal(dw, first)  # a workspace full of NaN changes nothing


# ------------------------------------------------------------------------------------------------ 5. no host synchronisation
def test_forward_and_backward_do_not_synchronise(hip):
    from futuredet_amd import dense_train

    x, w, dy, ks = _problem((2, 20, 28, 64, 96, 3))[:4]
    xd, wd, dyd = x.to(DEV).to(BF).requires_grad_(True), w.to(DEV).requires_grad_(True), dy.to(DEV).to(BF)

    def step():
        xd.grad = wd.grad = None
        y = dense_train.conv2d_bf16(xd, wd, ks)
        y.backward(dyd)
        return y

    step()  # warm-up: code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = step()
        with pytest.raises(RuntimeError):  # the mode is enforced on this build
            y.float().sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert xd.grad is not None and wd.grad is not None and bool(torch.isfinite(wd.grad).all())


# ------------------------------------------------------------------------------------------------ 6. the neck
def _small_rpn(seed=0):
    from futuredet_amd.necks import RPN

    torch.manual_seed(seed)
    neck = RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[64, 64],
               num_input_features=32)
    neck.init_weights()
    return neck.to(DEV).train()


def _bev(seed=3):
    return _bf16_values(np.random.default_rng(seed), (2, 32, 16, 24)).to(DEV)


def test_default_train_dtype_is_forward_modules_bit_for_bit(hip, monkeypatch):
    # bit-identical gradients need torch convolutions that repeat their own bits: the deterministic algorithms, for both sides
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    neck = _small_rpn()
    ref = copy.deepcopy(neck)
    assert neck.train_dtype is torch.float32
    xa, xb = _bev().requires_grad_(True), _bev().requires_grad_(True)
    got, want = neck(xa), ref.forward_modules(xb)
    g = _bf16_values(np.random.default_rng(4), tuple(want.shape)).to(DEV)
    got.backward(g)
    want.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(xa.grad, xb.grad)
    for (name, p), q in zip(neck.named_parameters(), ref.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), name
    for (name, b), c in zip(neck.named_buffers(), ref.buffers()):
        assert torch.equal(b, c), name


def _eligible_convs(neck, x):
    from futuredet_amd import dense_train

    n = 0
    for seq in list(neck.blocks) + list(neck.deblocks):
        mods = list(seq.children())
        for i, m in enumerate(mods):
            if dense_train.conv_takes_bf16(m, x) or (i > 0 and dense_train._pad_then_conv_takes_bf16(mods[i - 1], m, x)):
                n += 1
    return n


def test_neck_in_mixed_precision_layer_by_layer(hip):
    """RPN.train_dtype = bfloat16: an fp32 NCHW-contiguous map of the fp32 path's shape, finite fp32 gradients on every parameter, moving
    statistics -- and every conv2d_bf16 call of the walk (x, weight, y, the incoming dy, dx, dW) against its own float64 restatement."""
    from futuredet_amd import dense_train

    neck = _small_rpn()
    want_shape = tuple(copy.deepcopy(neck).forward_modules(_bev()).shape)
    stats = {k: b.clone() for k, b in neck.named_buffers()}
    neck.train_dtype = BF
    x = _bev().requires_grad_(True)
    seen = []
    orig = dense_train.conv2d_bf16

    def recording(x_nhwc, weight, ks):
        if not x_nhwc.requires_grad:
            x_nhwc.requires_grad_(True)
        y = orig(x_nhwc, weight, ks)
        rec = dict(x=x_nhwc.detach(), w=weight, ks=ks, y=y.detach())
        y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
        x_nhwc.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))
        seen.append(rec)
        return y

    dense_train.conv2d_bf16 = recording
    try:
        out = neck(x)
        g = _bf16_values(np.random.default_rng(4), tuple(out.shape)).to(DEV)
        out.backward(g)
        torch.cuda.synchronize()
    finally:
        dense_train.conv2d_bf16 = orig
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == want_shape == (2, 128, 16, 24)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for name, p in neck.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    for k, b in neck.named_buffers():
        assert not torch.equal(b, stats[k]), "BatchNorm buffer %s did not move" % k
    n = _eligible_convs(neck, x)
    assert n == 4 and len(seen) == n, (n, len(seen))  # a stride-1 3 x 3 per stage, stage 0's merged ZeroPad2d + conv, the 1 x 1 deblock
    assert sorted((r["ks"], tuple(r["w"].shape[:2])) for r in seen) == [(1, (64, 32)), (3, (32, 32)), (3, (32, 32)), (3, (64, 64))]
    for i, r in enumerate(seen):
        assert r["x"].dtype == BF and r["y"].dtype == BF and r["dy"].dtype == BF and r["dx"].dtype == BF
        w16 = r["w"].detach().to(BF).float().cpu()  # what the device packer makes of the fp32 master weight
        y_ref, dx_ref, dw_ref = _reference64(r["x"].float().cpu(), w16, r["dy"].float().cpu(), r["ks"])
        name = "neck conv %d (%s, ks %d)" % (i, tuple(r["w"].shape[:2]), r["ks"])
        _close_rounded(name + " y", _np(r["y"]), y_ref.numpy())
        _close_rounded(name + " dx", _np(r["dx"]), dx_ref.numpy())
        _close(name + " dW", _np(r["w"].grad), dw_ref.numpy())


def test_one_training_step_with_the_neck_in_mixed_precision(hip):
    """forecast_n0 with neck.train_dtype = backbone.train_dtype = bfloat16 through solver.train_steps: a finite loss, every neck weight
    moves, same state-dict keys; 12 of the neck's 14 convolutions are on conv2d_bf16"""
    from futuredet_amd import build_detector, dense_train, solver
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel
    from test_gpu_loss import _synthetic_gt

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    keys = list(net.state_dict())
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV)
    assert net.neck.train_dtype is torch.float32
    net.neck.train_dtype = net.backbone.train_dtype = BF
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    before = {k: p.detach().clone() for k, p in net.neck.named_parameters()}
    calls = []
    orig = dense_train.conv2d_bf16

    def counting(x_nhwc, weight, ks):
        calls.append((ks, tuple(weight.shape[:2])))
        return orig(x_nhwc, weight, ks)

    dense_train.conv2d_bf16 = counting
    try:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        out = next(solver.train_steps(net, [ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2)))
    finally:
        dense_train.conv2d_bf16 = orig
    torch.cuda.synchronize()
    assert np.isfinite(float(sum(out["loss"]).detach()))
    assert len(calls) == 12 and sum(1 for ks, _ in calls if ks == 1) == 1, calls
    for k, p in net.neck.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert not torch.equal(p.detach(), before[k]), "neck parameter %s did not move" % k
    assert list(net.state_dict()) == keys
