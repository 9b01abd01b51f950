"""CenterHead(dcn_head=True) without a GPU: module structure and state_dict keys of the reference's DCNSepHead
(det3d/models/bbox_heads/center_head.py:40-78,176-229,317-373), the configurations it refuses, and the torch restatement of
DCN v1 (nn_utils.deform_conv2d_v1) against convolutions and a float64 loop over deform_conv_cuda_kernel.cu:85-117,191-240."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from futuredet_amd import build_head
from futuredet_amd.nn_utils import deform_conv2d_v1

COMMON = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}

# one DCNSepHead task, written out from the reference modules: FeatureAdaption (conv_offset 1x1 64->72 with bias, conv_adaption
# DeformConv weight only) x 2, cls_head = Sequential(Conv2d, BatchNorm2d, ReLU, Conv2d), task_head = SepHead over the heads without hm
_BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
TASK_KEYS = (["feature_adapt_%s.conv_offset.%s" % (b, k) for b in ("cls", "reg") for k in ("weight", "bias")]
             + ["feature_adapt_%s.conv_adaption.weight" % b for b in ("cls", "reg")]
             + ["cls_head.0.weight", "cls_head.0.bias"] + ["cls_head.1.%s" % k for k in _BN] + ["cls_head.3.weight", "cls_head.3.bias"]
             + ["task_head.%s.0.%s" % (h, k) for h in COMMON for k in ("weight", "bias")]
             + ["task_head.%s.1.%s" % (h, k) for h in COMMON for k in _BN]
             + ["task_head.%s.3.%s" % (h, k) for h in COMMON for k in ("weight", "bias")])
SHARED_KEYS = ["shared_conv.0.weight", "shared_conv.0.bias"] + ["shared_conv.1.%s" % k for k in _BN]
BEV_KEYS = ["bev_conv.%d.%s" % (i, k) for i in (0, 3, 6) for k in ("weight", "bias")] + ["bev_conv.%d.%s" % (i, k) for i in (1, 4, 7) for k in _BN]


def _head(**kw):
    args = dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25,
                code_weights=[1.0] * 10, common_heads=COMMON, share_conv_channel=64, dcn_head=True, timesteps=7, two_stage=False,
                reverse=False, sparse=False, dense=False, bev_map=False, forecast_feature=False, classify=False, wide_head=False)
    args.update(kw)
    return build_head(args)


# mode: (keywords, number of tasks, heat-map classes per task, velocity channels)
MODES = {"standard_n3": (dict(), 1, 1, 14), "reverse": (dict(reverse=True), 1, 1, 14), "sparse": (dict(sparse=True), 2, 1, 14),
         "dense": (dict(dense=True), 7, 1, 2), "classify": (dict(classify=True), 7, 3, 2), "bev_map": (dict(bev_map=True), 1, 1, 14)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_dcn_head_constructs_with_the_reference_state_dict(mode):
    kw, ntask, ncls, nvel = MODES[mode]
    head = _head(**kw)
    want = set(SHARED_KEYS + ["tasks.%d.%s" % (i, k) for i in range(ntask) for k in TASK_KEYS] + (BEV_KEYS if mode == "bev_map" else []))
    sd = head.state_dict()
    assert set(sd) == want, set(sd) ^ want
    for i in range(ntask):
        t = "tasks.%d." % i
        assert sd[t + "feature_adapt_cls.conv_offset.weight"].shape == (72, 64, 1, 1)
        assert sd[t + "feature_adapt_reg.conv_offset.bias"].shape == (72,)
        assert sd[t + "feature_adapt_cls.conv_adaption.weight"].shape == (64, 64, 3, 3)
        assert sd[t + "cls_head.0.weight"].shape == (64, 64, 3, 3) and sd[t + "cls_head.3.weight"].shape == (ncls, 64, 3, 3)
        assert sd[t + "task_head.vel.3.weight"].shape == (nvel, 64, 3, 3)  # the per-timestep widening still applies (center_head.py:353-356)
        assert float(sd[t + "cls_head.3.bias"][0]) == pytest.approx(-2.19)
        assert not sd[t + "feature_adapt_reg.conv_offset.weight"].any()  # FeatureAdaption.init_offset
    head.eval()
    x = torch.randn(1, 512, 12, 10)
    bev = torch.randn(1, 6, 12, 10) if mode == "bev_map" else None
    with torch.no_grad():
        preds = head(x, bev)
    assert len(preds) == ntask
    for pd in preds:
        assert list(pd) == list(COMMON) + ["hm"] and pd["hm"].shape == (1, ncls, 12, 10)


@pytest.mark.parametrize("kw", [dict(forecast_feature=True, dense=True), dict(wide_head=True), dict(share_conv_channel=128)])
def test_dcn_head_refuses_what_the_reference_cannot_run(kw):
    with pytest.raises(ValueError, match="dcn_head"):
        _head(**kw)


def test_dcn_head_from_the_config_builds_a_detector():
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config

    assert centerpoint_config("forecast_n3").model["bbox_head"]["dcn_head"] is False
    cfg = centerpoint_config("forecast_n3", dcn_head=True)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    assert net.bbox_head.dcn_head and type(net.bbox_head.tasks[0]).__name__ == "DCNSepHead"


def test_deform_conv_with_zero_offsets_is_conv2d():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 16, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(5, 16, 3, 3, generator=g, dtype=torch.float64)
    got = deform_conv2d_v1(x, torch.zeros(2, 72, 9, 11, dtype=torch.float64), w)
    assert (got - F.conv2d(x, w, padding=1)).abs().max() <= 1e-12


def test_deform_conv_with_integer_offsets_is_the_shifted_convolution():
    g = torch.Generator().manual_seed(1)
    B, C, H, W = 1, 16, 8, 10
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(4, C, 3, 3, generator=g, dtype=torch.float64)
    shifts = [(1, -2), (-2, 0), (0, 2), (2, 1)]  # (dh, dw) of each deformable group, the same for every tap
    off = torch.zeros(B, 4, 9, 2, H, W, dtype=torch.float64)
    for gi, (a, b) in enumerate(shifts):
        off[:, gi, :, 0], off[:, gi, :, 1] = a, b
    got = deform_conv2d_v1(x, off.view(B, 72, H, W), w)
    want = torch.zeros_like(got)
    for gi, (a, b) in enumerate(shifts):  # out[y, x] = sum w[i, j] x[y - 1 + i + a, x - 1 + j + b], zero outside the map
        sl = slice(4 * gi, 4 * gi + 4)
        full = F.conv2d(F.pad(x[:, sl], (4, 4, 4, 4)), w[:, sl])
        want += full[:, :, 3 + a:3 + a + H, 3 + b:3 + b + W]
    assert (got - want).abs().max() <= 1e-12


def _loop_reference(x, off, w):
    """float64 loops over deform_conv_cuda_kernel.cu:85-117 (bilinear) and :191-240 (im2col), then the GEMM."""
    B, C, H, W = x.shape
    cout = w.shape[0]
    cpg = C // 4
    out = np.zeros((B, cout, H, W))
    for b in range(B):
        col = np.zeros((C, 9, H, W))
        for c in range(C):
            g = c // cpg
            for y in range(H):
                for xx in range(W):
                    for i in range(3):
                        for j in range(3):
                            t = i * 3 + j
                            h = y - 1 + i + off[b, g * 18 + 2 * t, y, xx]
                            ww = xx - 1 + j + off[b, g * 18 + 2 * t + 1, y, xx]
                            val = 0.0
                            if h > -1 and ww > -1 and h < H and ww < W:
                                hl, wl = int(math.floor(h)), int(math.floor(ww))
                                hh_, wh_ = hl + 1, wl + 1
                                lh, lw = h - hl, ww - wl
                                v1 = x[b, c, hl, wl] if (hl >= 0 and wl >= 0) else 0.0
                                v2 = x[b, c, hl, wh_] if (hl >= 0 and wh_ <= W - 1) else 0.0
                                v3 = x[b, c, hh_, wl] if (hh_ <= H - 1 and wl >= 0) else 0.0
                                v4 = x[b, c, hh_, wh_] if (hh_ <= H - 1 and wh_ <= W - 1) else 0.0
                                val = (1 - lh) * (1 - lw) * v1 + (1 - lh) * lw * v2 + lh * (1 - lw) * v3 + lh * lw * v4
                            col[c, t, y, xx] = val
        out[b] = np.einsum("ckhw,ock->ohw", col, w.reshape(cout, C, 9))
    return out


def test_deform_conv_matches_a_float64_loop_at_every_border():
    rng = np.random.default_rng(2)
    B, C, H, W = 2, 8, 6, 7
    x = rng.normal(0, 1, (B, C, H, W))
    w = rng.normal(0, 1, (3, C, 3, 3))
    off = rng.uniform(-3.5, 3.5, (B, 72, H, W))  # fractional: border pixels sample across the edges and outside (-1, H) x (-1, W)
    off[:, 0::2, 0, :] = -0.6  # top row: taps i = 0 and 1 sample at h = -1.6 (outside) and -0.6 (straddling row 0)
    off[:, 1::2, :, -1] = 0.7  # right column: samples at w = W - 1.3 .. W + 0.7, the high corner column outside the map
    got = deform_conv2d_v1(torch.from_numpy(x), torch.from_numpy(off), torch.from_numpy(w)).numpy()
    want = _loop_reference(x, off, w)
    tap_i = np.repeat([0, 1, 2], 3)[None, None, :, None, None]
    tap_j = np.tile([0, 1, 2], 3)[None, None, :, None, None]
    hs = np.arange(H)[:, None] - 1 + tap_i + off[:, 0::2].reshape(B, 4, 9, H, W)
    ws = np.arange(W)[None, :] - 1 + tap_j + off[:, 1::2].reshape(B, 4, 9, H, W)
    for s, n in ((hs, H), (ws, W)):  # the case split is exercised: outside on both sides, straddling the first and the last row / column
        assert (s <= -1).any() and (s >= n).any() and ((s > -1) & (s < 0)).any() and ((s > n - 1) & (s < n)).any()
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
