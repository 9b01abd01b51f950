"""-m gpu: CenterHead(dcn_head=True) on the device.  fd_deform_adapt_nhwc (futuredet_amd/csrc/fd_deform_conv.hip) against the float64
torch restatement of DCN v1 (nn_utils.deform_conv2d_v1) in fp32 and teacher-forced bf16, and a whole n3 detector with a DCN head:
device predict vs the float64 head, packed decode vs the per-task path, StaticStep replay vs the eager sweep, four sweeps in flight."""
import copy

import numpy as np
import pytest
import torch

from parity_util import attribute_detection_diffs, report

pytestmark = pytest.mark.gpu

B, H, W, C = 2, 180, 180, 64
BF16_ULP = 8e-3  # one bf16 ulp relative to max(1, |ref|): the gate of the teacher-forced bf16 layers (test_gpu_parity.py)


def _adapt_pair(seed, off_std):
    """Two FeatureAdaption modules with non-zero offset weights: offsets of standard deviation ~ off_std px on ReLU inputs."""
    from futuredet_amd.heads import FeatureAdaption

    torch.manual_seed(seed)
    fa = [FeatureAdaption(C, C) for _ in range(2)]
    for m in fa:
        m.conv_offset.weight.data.normal_(0, off_std / (0.5 * C) ** 0.5)
        m.conv_offset.bias.data.uniform_(-1.0, 1.0)
    return [m.cuda() for m in fa]


def _input(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.relu(torch.randn(B, C, H, W, device="cuda", dtype=torch.float64, generator=g))


def _ref_f64(fa, x64):
    from futuredet_amd.nn_utils import deform_conv2d_v1

    outs = []
    for m in fa:
        off = torch.nn.functional.conv2d(x64, m.conv_offset.weight.double(), m.conv_offset.bias.double())
        outs.append(torch.relu(deform_conv2d_v1(x64, off, m.conv_adaption.weight.double())))
    return torch.cat(outs, 1).permute(0, 2, 3, 1)  # [B, H, W, 128]


def _pack(hip, fa, bf16):
    c, r = fa
    return hip.pack_deform_adapt(c.conv_adaption.weight, r.conv_adaption.weight, c.conv_offset.weight, c.conv_offset.bias,
                                 r.conv_offset.weight, r.conv_offset.bias, bf16)


def _rel(got, want):
    return float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max())


@pytest.mark.parametrize("off_std", [0.5, 2.0])  # trained scale and wide random offsets (every border band samples outside the map)
def test_deform_kernel_fp32_vs_float64(hip, off_std):
    fa = _adapt_pair(3, off_std)
    x64 = _input(4)
    with torch.no_grad():
        want = _ref_f64(fa, x64)
        xn = x64.float().permute(0, 2, 3, 1).contiguous()
        wpk, ow, ob = _pack(hip, fa, False)
        got = hip.deform_adapt_nhwc(xn, wpk, ow, ob)
        # the same kernel reading precomputed fp32 offsets [B,H,W,144] (cls channels first)
        offs = torch.cat([torch.nn.functional.conv2d(x64.float(), m.conv_offset.weight, m.conv_offset.bias) for m in fa], 1)
        got_in = hip.deform_adapt_nhwc(xn, wpk, offsets=offs.permute(0, 2, 3, 1).contiguous())
    torch.cuda.synchronize()
    e, e_in = _rel(got, want), _rel(got_in, want)
    report("deform kernel fp32 (offset std %.1f) vs float64, in-kernel offsets" % off_std, e, 1e-4)
    report("deform kernel fp32 (offset std %.1f) vs float64, offsets input" % off_std, e_in, 1e-4)
    assert e <= 1e-4 and e_in <= 1e-4
    assert float(want.abs().max()) > 1.0 and bool((want[:, 0] != 0).any())


def test_deform_kernel_bf16_teacher_forced(hip):
    """bf16 input, fp32 offsets, samples rounded to bf16 for the bf16 MFMA, bf16 weights, fp32 accumulation, bf16 output: the float64
    restatement of exactly that (same bf16 input) within one bf16 ulp."""
    from futuredet_amd.nn_utils import deform_conv2d_v1

    fa = _adapt_pair(5, 1.0)
    xb = _input(6).to(torch.bfloat16)
    xf = xb.double()
    eye = torch.eye(9 * C, device="cuda", dtype=torch.float64).view(9 * C, C, 3, 3)  # output channel c * 9 + tap = the im2col column
    with torch.no_grad():
        outs = []
        for m in fa:
            off = torch.nn.functional.conv2d(xf, m.conv_offset.weight.double(), m.conv_offset.bias.double())
            col = deform_conv2d_v1(xf, off, eye).to(torch.bfloat16).double().view(B, C, 9, H, W)
            wb = m.conv_adaption.weight.to(torch.bfloat16).double().reshape(C, C, 9)
            outs.append(torch.relu(torch.einsum("bckhw,ock->bohw", col, wb)))
            del col
        want = torch.cat(outs, 1).permute(0, 2, 3, 1).to(torch.bfloat16).double()
        wpk, ow, ob = _pack(hip, fa, True)
        got = hip.deform_adapt_nhwc(xb.permute(0, 2, 3, 1).contiguous(), wpk, ow, ob)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16
    e = _rel(got, want)
    report("deform kernel bf16 teacher-forced vs float64 restatement", e, BF16_ULP)
    assert e <= BF16_ULP


def test_deform_kernel_with_zero_offsets_is_the_plan_conv(hip):
    fa = _adapt_pair(7, 1.0)
    for m in fa:
        m.conv_offset.weight.data.zero_()
        m.conv_offset.bias.data.zero_()
    xn = _input(8).float().permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        wpk, ow, ob = _pack(hip, fa, False)
        got = hip.deform_adapt_nhwc(xn, wpk, ow, ob)
        zero = torch.zeros(C, device="cuda")
        want = torch.cat([hip.conv2d_nhwc_f32(xn, hip.pack_conv2d_weight_f32(m.conv_adaption.weight), zero, C, 3, relu=True) for m in fa], 3)
    torch.cuda.synchronize()
    e = _rel(got, want.double())
    report("deform kernel, zero offsets, vs the fp32 direct 3x3 conv", e, 1e-5)
    assert e <= 1e-5


# ------------------------------------------------------------------------------------------------ a whole detector with a DCN head
def _dcn_net(seed=7):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, tame_box_dims

    cfg = centerpoint_config("forecast_n3", dcn_head=True)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    sd = tame_box_dims(seeded_state_dict(net, seed))
    assert any(k.endswith("conv_offset.weight") and sd[k].abs().max() > 0 for k in sd)
    net.load_state_dict(sd, strict=False)
    return cfg, net.cuda().eval()


def _rows(res):
    return torch.cat([res["box3d_lidar"].float(), res["scores"][:, None].float(), res["label_preds"][:, None].float()], 1).cpu().numpy()


def test_dcn_detector_predict_matches_the_float64_head(hip, monkeypatch):
    from futuredet_amd import detectors
    from futuredet_amd.synth import synthetic_cloud
    from oracle import ops as oops

    monkeypatch.setattr(detectors, "_NO_GRAPH", True)  # neck + head eagerly: the hook below sees the head's input once
    cfg, net = _dcn_net()
    seen = []
    hook = net.bbox_head.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=30000)).cuda() for s in (0, 1)]
    with torch.no_grad():
        got = net.forward_points(clouds, cfg.voxel_generator, padded=False)
        hook.remove()
        assert len(seen) == 1 and net.bbox_head._plan is not None, "the convolution plan must be the path that ran"
        head64 = copy.deepcopy(net.bbox_head).double()
        preds64 = head64.forward_modules(seen[0].double())
        want = net.bbox_head.predict({"metadata": [None] * 2}, [{k: v.float() for k, v in pd.items()} for pd in preds64], cfg.test_cfg)
    tc = cfg.test_cfg
    for b in range(2):
        g, w = _rows(got[b]), _rows(want[b])
        assert len(w) > 50
        n_un = attribute_detection_diffs("dcn n3 detector b%d vs float64 head" % b, g, w, oops.boxes_iou_bev, tc["score_threshold"],
                                         tc["nms"]["nms_iou_threshold"])
        assert n_un == 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dcn_packed_static_step_and_eager_plan_agree_bit_for_bit(hip, precision, monkeypatch):
    from futuredet_amd import detectors
    from futuredet_amd.detectors import StaticStep
    from futuredet_amd.synth import synthetic_cloud

    cfg, net = _dcn_net()
    if precision == "bf16":
        net.set_precision(torch.bfloat16)
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=n)).cuda() for s, n in ((3, 40000), (4, 70000), (5, 9000))]
    step = StaticStep(net, cfg.voxel_generator, capacity=90000)
    seen = []
    with torch.no_grad():
        step.warm_up([clouds[0]])
        for i, c in enumerate(clouds):
            want = net.forward_points([c], cfg.voxel_generator)
            got = step([c])
            torch.cuda.synchronize()
            assert step.graph is not None
            assert torch.equal(want[3], got[3]), i
            cnt = want[3].cpu().numpy()
            assert cnt.sum() > 0
            for s_ in range(cnt.shape[1]):
                k = int(cnt[0, s_])
                for w, g in zip(want[:3], got[:3]):
                    assert torch.equal(w[0, s_, :k], g[0, s_, :k]), (i, s_)
        # the packed decode of the plan's buffer vs the per-task path on the same maps (neck + head run eagerly for the hook)
        monkeypatch.setattr(detectors, "_NO_GRAPH", True)
        hook = net.bbox_head.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
        net.forward_points([clouds[1]], cfg.voxel_generator)
        hook.remove()
        preds = net.bbox_head(seen[-1])
        assert preds[0].raw is not None
        packed = net.bbox_head.predict({"metadata": [None]}, preds, cfg.test_cfg)
        plain = net.bbox_head.predict({"metadata": [None]}, [dict(pd) for pd in preds], cfg.test_cfg)
    assert len(packed[0]["scores"]) > 0 and np.array_equal(_rows(packed[0]), _rows(plain[0]))
    report("dcn head (%s): StaticStep replay, eager sweep, packed and per-task decode bit-identical" % precision, 0.0, 0.0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dcn_sweeps_in_flight_are_deterministic(hip, precision):
    """Four captured sweeps of the DCN detector in flight on four streams, 50 rounds: every replay equals its stream's first."""
    from futuredet_amd.detectors import StaticStep
    from futuredet_amd.synth import synthetic_cloud

    cfg, net = _dcn_net()
    if precision == "bf16":
        net.set_precision(torch.bfloat16)
    NB, NS, rounds = 2, 4, 50
    clouds = [[torch.from_numpy(synthetic_cloud(seed=10 * s + b, target_points=100000)).cuda() for b in range(NB)] for s in range(NS)]
    cap = max(c.shape[0] for cs in clouds for c in cs) + 1024
    streams = [torch.cuda.Stream() for _ in range(NS)]
    steps = []
    with torch.no_grad():
        for s, st in enumerate(streams):
            with torch.cuda.stream(st):
                step = StaticStep(net, cfg.voxel_generator, cap, batch_size=NB, ndim=5, packed=True, row_caps="auto")
                step.warm_up(clouds[s])
                step.capture()
                steps.append(step)
        torch.cuda.synchronize()
        first, differing = [None] * NS, 0
        for r in range(rounds):
            snaps = []
            for s, st in enumerate(streams):
                with torch.cuda.stream(st):
                    packed, counts = steps[s](clouds[s], check=False)
                    snaps.append((packed.clone(), counts.clone(), steps[s].level_counts.clone()))
            torch.cuda.synchronize()
            for s, snap in enumerate(snaps):
                assert not steps[s].overflowed(snap[2].cpu().tolist())
                if first[s] is None:
                    first[s] = snap
                    assert int(snap[1].sum()) > 0
                else:
                    differing += not (torch.equal(snap[0], first[s][0]) and torch.equal(snap[1], first[s][1]))
    report("dcn %s sweeps, %d in flight x %d rounds: replays that differ from the stream's first" % (precision, NS, rounds), float(differing), 0.0)
    assert differing == 0
