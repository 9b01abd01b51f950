"""-m gpu: Winograd tile 8 (strips of 32 tiles x 128 output channels, eight consumer waves) against tile 7 (32 tiles x 64 channels)
at the full size of every fp32 RPN / CenterHead Winograd layer, B = 2.  Same packed weights, same MFMAs in the same order per
accumulator: the results must be bit-identical, with and without ReLU, and into a channel window of a wider concat buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (cin, cout, H = W): the RPN blocks and the CenterHead shared / task-branch convs of the fp32 flagship model
LAYERS = ((256, 128, 180), (128, 128, 180), (512, 64, 180), (256, 256, 90), (64, 384, 180))


def _layer(cin, cout, H, W, seed, B=2):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, H, W, cin)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) * (2.0 / (cin * 9)) ** 0.5).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).cuda()
    return x, w, b


@pytest.mark.parametrize("cin,cout,hw", LAYERS)
def test_wino_tile8_matches_tile7(hip, cin, cout, hw):
    x, w, b = _layer(cin, cout, hw, hw, seed=cin + cout + hw)
    wpk = hip.pack_conv2d_weight_wino(w).cuda()
    for relu in (True, False):
        want = hip.conv2d_wino_nhwc_f32(x, wpk, b, cout, relu, tile=7)
        got = hip.conv2d_wino_nhwc_f32(x, wpk, b, cout, relu, tile=8)
        assert torch.equal(want, got), (cin, cout, hw, relu)
        if not relu:
            assert (want < 0).any()  # (the ReLU-off case really differs)


@pytest.mark.parametrize("cin,cout,hw", LAYERS)
def test_wino_tile8_concat_window(hip, cin, cout, hw):
    """co_off > 0 into a wider buffer: the window matches tile 7, every channel outside it keeps its fill."""
    x, w, b = _layer(cin, cout, hw, hw, seed=7 * cin + cout)
    wpk = hip.pack_conv2d_weight_wino(w).cuda()
    co_off, total = 36, cout + 36 + 28
    outs = []
    for tile in (7, 8):
        out = torch.full((2, hw, hw, total), 1234.5, device="cuda")
        hip.conv2d_wino_nhwc_f32(x, wpk, b, cout, True, out=out, co_off=co_off, tile=tile)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert (outs[1][..., :co_off] == 1234.5).all() and (outs[1][..., co_off + cout:] == 1234.5).all()


@pytest.mark.parametrize("cin,cout,H,W", ((128, 70, 30, 26), (32, 200, 9, 63), (64, 70, 37, 77), (16, 130, 13, 65)))
def test_wino_tile8_ragged(hip, cin, cout, H, W):
    """Channel counts that are not a multiple of 128 (a partial last item), odd sizes (partial tiles at the right / bottom edge)
    and images narrower than one strip (W < 63: tile 8 runs tile 6's kernel there); tile 6 is the reference for every shape."""
    x, w, b = _layer(cin, cout, H, W, seed=H * W + cout)
    wpk = hip.pack_conv2d_weight_wino(w).cuda()
    co_off, total = 4, cout + 12
    outs = []
    for tile in (6, 8):
        out = torch.full((2, H, W, total), -7.25, device="cuda")
        hip.conv2d_wino_nhwc_f32(x, wpk, b, cout, True, out=out, co_off=co_off, tile=tile)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), (cin, cout, H, W)
    assert (outs[1][..., :co_off] == -7.25).all() and (outs[1][..., co_off + cout:] == -7.25).all()
