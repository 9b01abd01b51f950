"""-m gpu: training of the deformable head.  fd_deform_adapt_backward (futuredet_amd/csrc/fd_deform_conv_grad.hip) against float64 autograd
of nn_utils.deform_conv2d_v1 fed the same offsets, the autograd function behind DCNSepHead in .train(), and one training step of a
whole DCN-head detector.

Every gradient test uses offsets that are multiples of 2^-9: exact in fp32 and in float64, so an integer sample coordinate is the same
integer on both sides and the right-hand derivative there is compared, not dodged.  The gate is test_gpu_spconv_grad._close:
|got - ref| <= 1e-4 * max(1, |ref|) on values scaled by the largest reference magnitude.

"Teacher-forced": the kernel takes the forward's output y only as the ReLU mask y > 0, and the float64 oracle applies that same
mask to its own pre-activation (the forward itself is gated in test_gpu_dcn.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
C = 64
CHUNK = 1024  # pixels per dW partial (kChunk of fd_deform_conv_grad.hip)


def _close(name, got, ref, tol=1e-4):
    got, ref = np.asarray(got.detach().cpu(), np.float64), np.asarray(ref.detach().cpu(), np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert float(np.abs(ref).max()) > 0, name
    return assert_close(name, got / scale, ref / scale, tol)


def _quant(t):
    return torch.round(t * 512.0) / 512.0


def _problem(seed, B, H, W, off_std):
    """x, offsets (multiples of 2^-9), the two weights and dy, NHWC fp32 on the device, and the forward's y."""
    from futuredet_amd import hip_ops

    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, C), generator=g)
    off = _quant(torch.randn((B, H, W, 144), generator=g) * off_std)
    wc, wr = torch.randn((C, C, 3, 3), generator=g), torch.randn((C, C, 3, 3), generator=g)
    dy = torch.randn((B, H, W, 2 * C), generator=g)
    x, off, wc, wr, dy = [t.to(DEV).contiguous() for t in (x, off, wc, wr, dy)]
    y = hip_ops.deform_adapt_nhwc(x, hip_ops.pack_deform_adapt_device(wc, wr), offsets=off)
    return x, off, wc, wr, dy, y


def _oracle(x, off, wc, wr, dy, y, conv=None):
    """float64 autograd of deform_conv2d_v1 (or of ``conv``) under the kernel's ReLU mask -> (dx, doffsets, dw [2,64,64,3,3]) NHWC."""
    from futuredet_amd.nn_utils import deform_conv2d_v1

    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    o64 = off.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ws = [w.double().clone().requires_grad_(True) for w in (wc, wr)]
    zs = []
    for br in range(2):
        o = o64[:, 72 * br:72 * (br + 1)]
        zs.append(deform_conv2d_v1(x64, o, ws[br]) if conv is None else conv(x64, ws[br]))
    z = torch.cat(zs, 1).permute(0, 2, 3, 1)
    mask = y > 0
    # the forward's mask is the float64 one wherever the pre-activation is not within rounding of zero
    flips = (mask != (z > 0)) & (z.abs() > 1e-4 * float(z.detach().abs().max()))
    assert not bool(flips.any())
    (z * mask * dy.double()).sum().backward()
    doff = o64.grad.permute(0, 2, 3, 1) if o64.grad is not None else None
    return x64.grad.permute(0, 2, 3, 1), doff, torch.stack([w.grad for w in ws])


# ------------------------------------------------------------------------------------------------ 1. kernel vs float64
@pytest.mark.parametrize("shape", [(2, 13, 11), (2, 40, 37)], ids=lambda s: "%dx%dx%d" % s)
def test_backward_kernel_vs_float64_teacher_forced(hip, shape):
    B, H, W = shape
    npix = B * H * W
    assert npix % 64 != 0 and npix % CHUNK != 0
    if npix > CHUNK:
        assert (npix + CHUNK - 1) // CHUNK >= 3  # several dW chunks, a partial last one
    x, off, wc, wr, dy, y = _problem(11 + H, B, H, W, 1.5)
    dx, doff, dw = hip.deform_adapt_backward(x, off, wc, wr, y, dy)
    torch.cuda.synchronize()
    rdx, rdoff, rdw = _oracle(x, off, wc, wr, dy, y)
    tag = "dcn backward %dx%dx%d " % shape
    _close(tag + "dx", dx, rdx)
    _close(tag + "doffsets", doff, rdoff)
    _close(tag + "dw", dw, rdw)
    # the inputs reach what they are meant to reach: integer coordinates, samples outside the window
    o = off.double().view(B, H, W, 2, 4, 9, 2)
    assert int((o == o.round()).sum()) > 0
    ti = torch.arange(9, device=DEV) // 3
    h = torch.arange(H, device=DEV).view(1, H, 1, 1, 1, 1) - 1 + ti + o[..., 0]
    assert int(((h <= -1) | (h >= H)).sum()) > 0


# ------------------------------------------------------------------------------------------------ 2. zero offsets
def test_backward_with_zero_offsets_is_the_plain_conv(hip):
    B, H, W = 2, 13, 11
    x, off, wc, wr, dy, _ = _problem(5, B, H, W, 0.0)
    assert not bool(off.any())
    y = hip.deform_adapt_nhwc(x, hip.pack_deform_adapt_device(wc, wr), offsets=off)
    dx, doff, dw = hip.deform_adapt_backward(x, off, wc, wr, y, dy)
    torch.cuda.synchronize()
    rdx, _, rdw = _oracle(x, off, wc, wr, dy, y, conv=lambda a, w: F.conv2d(a, w, padding=1))
    _, rdoff, _ = _oracle(x, off, wc, wr, dy, y)
    _close("dcn backward, zero offsets, dx vs conv2d", dx, rdx)
    _close("dcn backward, zero offsets, dw vs conv2d", dw, rdw)
    _close("dcn backward, zero offsets, doffsets", doff, rdoff)


# ------------------------------------------------------------------------------------------------ 3. determinism, capture
def test_backward_is_deterministic_and_replays_in_a_graph(hip):
    B, H, W = 2, 40, 37
    x, off, wc, wr, dy, y = _problem(21, B, H, W, 1.5)
    a = hip.deform_adapt_backward(x, off, wc, wr, y, dy)
    b = hip.deform_adapt_backward(x, off, wc, wr, y, dy)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    _close("dcn backward dx, run to run", b[0], a[0].double())

    def step():
        yy = hip.deform_adapt_nhwc(x, hip.pack_deform_adapt_device(wc, wr), offsets=off)
        return (yy,) + hip.deform_adapt_backward(x, off, wc, wr, yy, dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # scratch of the capture stream exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    for r in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], y), r
        assert torch.equal(out[2], a[1]) and torch.equal(out[3], a[2]), r
        _close("dcn backward dx, graph replay %d vs eager" % r, out[1], a[0].double())


# ------------------------------------------------------------------------------------------------ 4. NULL outputs
def test_backward_null_outputs(hip):
    B, H, W = 2, 13, 11
    x, off, wc, wr, dy, y = _problem(31, B, H, W, 1.5)
    full = hip.deform_adapt_backward(x, off, wc, wr, y, dy)
    for need in [(True, False, False), (False, True, False), (False, False, True)]:
        got = hip.deform_adapt_backward(x, off, wc, wr, y, dy, need=need)
        torch.cuda.synchronize()
        for i in range(3):
            assert (got[i] is not None) == need[i]
        if need[0]:
            _close("dcn backward, dx alone", got[0], full[0].double())
        if need[1]:
            assert torch.equal(got[1], full[1])
        if need[2]:
            assert torch.equal(got[2], full[2])
    assert hip.deform_adapt_backward(x, off, wc, wr, y, dy, need=(False, False, False)) == (None, None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. device packer
def test_device_packer_matches_the_host_packer(hip):
    g = torch.Generator().manual_seed(41)
    wc, wr = torch.randn((C, C, 3, 3), generator=g), torch.randn((C, C, 3, 3), generator=g)
    zw, zb = torch.zeros((72, C, 1, 1)), torch.zeros(72)
    host = hip.pack_deform_adapt(wc.to(DEV), wr.to(DEV), zw, zb, zw, zb, False)[0]
    dev = hip.pack_deform_adapt_device(wc.to(DEV), wr.to(DEV))
    torch.cuda.synchronize()
    assert dev.dtype == torch.uint8 and dev.shape == host.shape and torch.equal(dev, host)


def test_double_backward_is_refused(hip):
    """The backward is kernels, not torch ops: a gradient of the gradient raises, it is not silently wrong."""
    from futuredet_amd.heads import _DeformAdaptFunction

    x, off, wc, wr, dy, _ = _problem(43, 1, 5, 6, 1.5)
    x.requires_grad_(True)
    dy.requires_grad_(True)  # the gradient of x then depends on a tensor that asks for one
    y = _DeformAdaptFunction.apply(x, off, wc, wr)
    (gx,) = torch.autograd.grad((y * dy).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------ 6. module level
def _quantised_head(seed, B, H, W):
    """A DCNSepHead whose conv_offset gives the same offsets, bit for bit, in fp32 and in float64 (multiples of 2^-9), and its input."""
    from futuredet_amd.heads import DCNSepHead

    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    head = DCNSepHead(C, 1, dict(reg=(2, 2), height=(1, 2)), bn=True, final_kernel=3)
    for fa in (head.feature_adapt_cls, head.feature_adapt_reg):
        w = torch.randint(-4, 5, (72, C, 1, 1), generator=g).float() / 64.0
        fa.conv_offset.weight.data.copy_(w * (torch.rand((72, C, 1, 1), generator=g) < 0.25))
        fa.conv_offset.bias.data.copy_(torch.randint(-32, 33, (72,), generator=g).float() / 16.0)
        fa.conv_adaption.weight.data.normal_(0, 1.0, generator=g)
    x = torch.randint(0, 9, (B, C, H, W), generator=g).float() / 8.0 * (torch.rand((B, C, H, W), generator=g) < 0.66)
    return head, x


SEED6 = 1


def test_dcn_sep_head_trains_on_the_kernels(hip):
    B, H, W = 2, 13, 11
    head, x = _quantised_head(SEED6, B, H, W)
    ref = copy.deepcopy(head).double()
    head = head.to(DEV).train()
    fas = (head.feature_adapt_cls, head.feature_adapt_reg)
    rfas = (ref.feature_adapt_cls, ref.feature_adapt_reg)

    # ---- the inputs are what the issue's trap needs: identical offsets, integers, outside samples, exact window edges
    x64 = x.double().requires_grad_(True)
    with torch.no_grad():
        o32 = torch.cat([fa.conv_offset(x.to(DEV)) for fa in fas], 1).cpu()
        o64 = torch.cat([fa.conv_offset(x64) for fa in rfas], 1)
    assert torch.equal(o32.double(), o64) and torch.equal(o64 * 512, (o64 * 512).round())
    o = o64.view(B, 2, 4, 9, 2, H, W)
    tap = torch.arange(9)
    hh = torch.arange(H).view(1, 1, 1, 1, H, 1) - 1 + (tap // 3).view(1, 1, 1, 9, 1, 1) + o[:, :, :, :, 0]
    ww = torch.arange(W).view(1, 1, 1, 1, 1, W) - 1 + (tap % 3).view(1, 1, 1, 9, 1, 1) + o[:, :, :, :, 1]
    counts = dict(integer_offsets=int((o64 == o64.round()).sum()), outside=int(((hh <= -1) | (hh >= H) | (ww <= -1) | (ww >= W)).sum()),
                  on_minus_one=int(((hh == -1) | (ww == -1)).sum()), on_upper_edge=int(((hh == H) | (ww == W)).sum()))
    print("[dcn train] module-level inputs:", counts, "max |offset| %.3f" % float(o64.abs().max()))
    assert all(v > 0 for v in counts.values()), counts

    # ---- device, .train(): the adapted maps are what cls_head / task_head receive
    seen = {}
    hooks = [head.cls_head.register_forward_pre_hook(lambda m, a: seen.__setitem__("cls", a[0])),
             head.task_head.register_forward_pre_hook(lambda m, a: seen.__setitem__("reg", a[0]))]
    xd = x.to(DEV).requires_grad_(True)
    out = head(xd)
    for h_ in hooks:
        h_.remove()
    assert set(out) == {"reg", "height", "hm"} and seen["cls"].grad_fn is not None
    g = torch.Generator().manual_seed(99)
    dyc, dyr = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    ((seen["cls"] * dyc.to(DEV)).sum() + (seen["reg"] * dyr.to(DEV)).sum()).backward()
    torch.cuda.synchronize()

    rc, rr = rfas[0](x64), rfas[1](x64)
    ((rc * dyc.double()).sum() + (rr * dyr.double()).sum()).backward()

    _close("dcn head train: cls adapted map", seen["cls"], rc)
    _close("dcn head train: reg adapted map", seen["reg"], rr)
    _close("dcn head train: dx", xd.grad, x64.grad)
    for name, fa, rfa in (("cls", fas[0], rfas[0]), ("reg", fas[1], rfas[1])):
        _close("dcn head train: %s conv_offset.weight grad" % name, fa.conv_offset.weight.grad, rfa.conv_offset.weight.grad)
        _close("dcn head train: %s conv_offset.bias grad" % name, fa.conv_offset.bias.grad, rfa.conv_offset.bias.grad)
        _close("dcn head train: %s conv_adaption.weight grad" % name, fa.conv_adaption.weight.grad, rfa.conv_adaption.weight.grad)

    # ---- the train-mode maps are the eval kernel's on the same offsets, bit for bit
    with torch.no_grad():
        offs = torch.cat([fa.conv_offset(xd) for fa in fas], 1).permute(0, 2, 3, 1).contiguous()
        wpk = hip.pack_deform_adapt(fas[0].conv_adaption.weight, fas[1].conv_adaption.weight, fas[0].conv_offset.weight, fas[0].conv_offset.bias,
                                    fas[1].conv_offset.weight, fas[1].conv_offset.bias, False)[0]
        want = hip.deform_adapt_nhwc(xd.detach().permute(0, 2, 3, 1).contiguous(), wpk, offsets=offs).permute(0, 3, 1, 2)
    assert torch.equal(seen["cls"], want[:, :C]) and torch.equal(seen["reg"], want[:, C:])


# ------------------------------------------------------------------------------------------------ 7. end to end
def _example(cfg, seed):
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import synthetic_cloud
    from oracle import ops as oops

    vg = centerpoint_config("forecast_n0").voxel_generator
    v, c, n = oops.points_to_voxel(synthetic_cloud(seed=seed, target_points=20000), vg["voxel_size"], vg["range"], 10, True, 160000)
    T = cfg.timesteps
    rng = np.random.default_rng(seed)
    Hh = Wh = 180
    M = 16
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([[1440, 1440, 40]]),
              metadata=[None])
    for key in ("hm", "ind", "mask", "cat", "anno_box"):
        ex[key] = []
    for s in range(T):
        ind = torch.from_numpy(rng.choice(Hh * Wh, M, replace=False)[None].astype(np.int64)).to(DEV)
        hm = torch.from_numpy((rng.uniform(0, 0.9, (1, 1, Hh, Wh)) ** 3).astype(np.float32)).to(DEV)
        hm.view(-1)[ind[0]] = 1.0
        ex["hm"].append([hm])
        ex["ind"].append([ind])
        ex["mask"].append([torch.ones((1, M), dtype=torch.uint8, device=DEV)])
        ex["cat"].append([torch.zeros((1, M), dtype=torch.int64, device=DEV)])
        ex["anno_box"].append([torch.from_numpy(rng.normal(0, 1, (1, M, 10)).astype(np.float32)).to(DEV)])
    return ex


def test_dcn_training_step_end_to_end(hip, monkeypatch):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims

    cfg = centerpoint_config("forecast_n3", dcn_head=True)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV)
    cloud = [torch.from_numpy(synthetic_cloud(seed=1, target_points=20000)).to(DEV)]

    def detect(model):
        model.eval()
        with torch.no_grad():
            r = model.forward_points(cloud, cfg.voxel_generator, padded=False)[0]
        torch.cuda.synchronize()
        return torch.cat([r["box3d_lidar"], r["scores"][:, None]], 1).cpu()

    before = detect(net)
    net.train()
    calls, named = [], []
    backward = hip.deform_adapt_backward
    monkeypatch.setattr(hip, "deform_adapt_backward", lambda *a, **kw: calls.append(1) or backward(*a, **kw))
    ret = net(_example(cfg, 2), return_loss=True)
    loss = sum(ret["loss"])
    assert torch.isfinite(loss)
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    opt.zero_grad()
    loss.backward()
    for name, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            if "conv_offset" in name or "conv_adaption" in name:
                named.append(name)
                assert float(p.grad.abs().max()) > 0, name
    n_tasks = len(net.bbox_head.tasks)
    assert len(named) == 6 * n_tasks and len(calls) == n_tasks, "every DCN task trains through fd_deform_adapt_backward"
    opt.step()
    after = detect(net)
    fresh = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    fresh.load_state_dict(net.state_dict())
    want = detect(fresh.to(DEV))
    assert len(want) > 0 and after.shape == want.shape, (after.shape, want.shape)
    assert torch.allclose(after, want, rtol=0, atol=0, equal_nan=True), float((after - want).nan_to_num().abs().max())
    assert before.shape != want.shape or not torch.equal(before, want), "one SGD step must change the detections"

    # the bf16 head is inference-only
    head = net.bbox_head.train()
    head.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="fp32"):
        head(torch.zeros((1, 8, 8, 8), device=DEV))
