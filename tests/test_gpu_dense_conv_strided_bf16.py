"""Mixed-precision training of the dense convolutions that change resolution, on the device: fd_conv2d_s2_dgrad_bf16, fd_conv2d_down2_bf16,
the 2 x 2 packer, the strided weight gradients, the autograd surfaces dense_train.conv2d_s2_bf16 / conv_transpose2d_k2_bf16 /
conv2d_k2s2_bf16 and their routing in the neck, against float64 restatements on the bf16-rounded operands.

Bounds: the project's rule, derived in test_gpu_dense_conv_train_bf16.py (test_gpu_spconv_grad_bf16.py).  bf16 x bf16 products are exact
in fp32, so a result that is not rounded again (dW) differs from float64 only by the fp32 accumulation: 1e-4 * scale, scale = max(1,
max |ref|).  A result rounded once to bf16 (y, dX) gets |got - ref| <= 2^-8 |ref| + 1.01e-4 * scale.  Operands uniform (-1, 1), rounded to
bf16.

Shapes: the smallest that reach every boundary -- both parities of H and W, the dgrad's 8 x 16 tile of dY cells (one tile exactly, one
cell past it), 128-pixel strips of down2, the 32-channel slices and the shipped channel pairs, the weight gradients' pixel chunks."""
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

# (kind, B, H, W, Cin, Cout): H x W is the layer's INPUT map for "s2"; the COARSE grid for "up2" (its input) and "down2" (its output),
# except the "down2f" rows, whose H x W is the fine input map itself (an odd edge that is not read)
S2_CASES = [(1, 3, 5, 32, 32), (2, 9, 17, 32, 64), (2, 16, 32, 32, 32), (2, 18, 34, 64, 96), (1, 17, 32, 32, 32), (1, 16, 33, 32, 32),
            (1, 12, 20, 128, 256), (1, 12, 20, 64, 128), "chunks"]
K2_CASES = [(1, 3, 5, 32, 32), (2, 9, 17, 64, 96), (1, 10, 12, 256, 256), (1, 8, 8, 256, 128), (1, 8, 8, 64, 128), "chunks"]
ODD_FINE = [(2, 9, 17, 32, 64), (2, 9, 16, 32, 64), (2, 8, 17, 32, 64)]
CASES = ([("s2", c) for c in S2_CASES] + [("up2", c) for c in K2_CASES] + [("down2", c) for c in K2_CASES] + [("down2f", c) for c in ODD_FINE])


def _fn(kind):
    from futuredet_amd import dense_train

    return {"s2": dense_train.conv2d_s2_bf16, "up2": dense_train.conv_transpose2d_k2_bf16, "down2": dense_train.conv2d_k2s2_bf16}[kind[:5]]


def _shapes(kind, case):
    """(x shape NHWC, weight shape, y shape NHWC) of a case"""
    if case == "chunks":
        from futuredet_amd import hip_ops

        chunk = hip_ops.conv2d_wgrad_bf16_chunk()
        case = (1, 1, 4 * chunk + 1, 32, 32) if kind == "s2" else (1, 1, 2 * chunk + 1, 32, 32)  # 2 chunk + 1 pixels of dy / coarse pixels
    B, H, W, cin, cout = case
    if kind == "s2":
        return (B, H, W, cin), (cout, cin, 3, 3), (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout)
    if kind == "up2":
        return (B, H, W, cin), (cin, cout, 2, 2), (B, 2 * H, 2 * W, cout)
    if kind == "down2":
        return (B, 2 * H, 2 * W, cin), (cout, cin, 2, 2), (B, H, W, cout)
    return (B, H, W, cin), (cout, cin, 2, 2), (B, H // 2, W // 2, cout)


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(name, got, ref, tol=1e-4):
    """element-wise |got - ref| <= tol * scale, scale = max(1, max |ref|): results that are not rounded to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
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


def _reference64(kind, x_nhwc, w, dy_nhwc):
    """float64 F.conv2d(stride 2, padding 1) / F.conv_transpose2d(stride 2) / F.conv2d(stride 2) and their autograd on the CPU:
    (y, dx) NHWC, dW in the parameter's layout"""
    x = x_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    if kind == "s2":
        y = F.conv2d(x, w, stride=2, padding=1)
    elif kind == "up2":
        y = F.conv_transpose2d(x, w, stride=2)
    else:
        y = F.conv2d(x, w, stride=2)
    y.backward(dy_nhwc.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), w.grad


def _run(kind, x_nhwc, w, dy_nhwc):
    """the differentiable function forward + backward on the device: (y, dx) bf16 NHWC, dW fp32"""
    x = x_nhwc.to(DEV).to(BF).requires_grad_(True)
    w = w.to(DEV).requires_grad_(True)
    y = _fn(kind)(x, w)
    y.backward(dy_nhwc.to(DEV).to(BF))
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad


_problems = {}


def _problem(kind, case):
    """operands (uniform (-1, 1) rounded to bf16) and the float64 reference of a case: computed once, shared, never modified"""
    key = (kind, case)
    if key not in _problems:
        xs, ws, ys = _shapes(kind, case)
        rng = np.random.default_rng(2000 + len(_problems))
        x, w, dy = _bf16_values(rng, xs), _bf16_values(rng, ws), _bf16_values(rng, ys)
        _problems[key] = (x, w, dy) + _reference64(kind, x, w, dy)
    return _problems[key]


# ------------------------------------------------------------------------------------------------ 1. the packers
def _tie_weights(rng, shape):
    """fp32 weights of which a third sit exactly half way between two bf16 values (both parities of the lower neighbour), the rest
    have random low bits (test_gpu_dense_conv_train_bf16.py)"""
    v = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))
    bits = v.view(torch.int32)
    kind = torch.from_numpy(rng.integers(0, 3, shape).astype(np.int32))
    tie = (bits & ~0xFFFF) | 0x8000
    return torch.where(kind == 0, tie, bits).view(torch.float32).contiguous()


_K2 = [c for c in K2_CASES if c != "chunks"]
UP2_PAIRS = sorted({(c[3], c[4]) for c in _K2} | {(c[4], c[3]) for c in _K2} | {(32, 40)})    # (Ccoarse, Cfine): Cfine is padded
DOWN2_PAIRS = sorted({(c[3], c[4]) for c in _K2} | {(c[4], c[3]) for c in _K2} | {(40, 32)})  # Ccoarse is padded


def _check_ties(w):
    bits = w.view(torch.int32)
    assert int(((bits & 0xFFFF) == 0x8000).sum()) > w.numel() // 6  # the ties are there, on even and odd neighbours
    assert int((((bits >> 16) & 1) == 1).sum()) > 0 and int((((bits >> 16) & 1) == 0).sum()) > 0


@pytest.mark.parametrize("cc,cf", UP2_PAIRS)
def test_up2_device_pack_is_byte_identical_to_the_host_pack(hip, cc, cf):
    w = _tie_weights(np.random.default_rng(cc * 7 + cf), (cc, cf, 2, 2))
    _check_ties(w)
    want = torch.cat([hip.pack_conv2d_weight(w[:, :, dy, dx].t()[..., None, None].contiguous()) for dy in (0, 1) for dx in (0, 1)])
    got = hip.pack_conv2d_weight_2x2_device(w.to(DEV), hip.PACK_UP2).cpu()
    assert got.numel() == want.numel() and torch.equal(got, want)
    twin = hip.pack_conv2d_weight_2x2_device(w.transpose(0, 1).contiguous().to(DEV), hip.PACK_UP2, fine_major=True).cpu()
    assert torch.equal(twin, want)


@pytest.mark.parametrize("cc,cf", DOWN2_PAIRS)
def test_down2_device_pack_is_byte_identical_to_the_host_pack(hip, cc, cf):
    w = _tie_weights(np.random.default_rng(cc * 11 + cf), (cc, cf, 2, 2))
    _check_ties(w)
    want = hip.pack_conv2d_weight(w.permute(0, 2, 3, 1).reshape(cc, 4 * cf, 1, 1).contiguous())
    got = hip.pack_conv2d_weight_2x2_device(w.to(DEV), hip.PACK_DOWN2).cpu()
    assert got.numel() == want.numel() and torch.equal(got, want)
    twin = hip.pack_conv2d_weight_2x2_device(w.transpose(0, 1).contiguous().to(DEV), hip.PACK_DOWN2, fine_major=True).cpu()
    assert torch.equal(twin, want)


def test_packers_refuse_an_unpadded_reduction_side(hip):
    for shape, kind in (((40, 32, 2, 2), hip.PACK_UP2), ((32, 40, 2, 2), hip.PACK_DOWN2), ((32, 32, 3, 3), hip.PACK_UP2)):
        with pytest.raises(hip.FutureDetHipError, match="pack_conv2d_weight_2x2_device"):
            hip.pack_conv2d_weight_2x2_device(torch.zeros(shape, device=DEV), kind)


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("kind,case", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_matches_float64_on_the_rounded_operands(hip, kind, case):
    x, w, dy, y_ref, dx_ref, dw_ref = _problem(kind, case)
    y, dx, dw = _run(kind, x, w, dy)
    assert y.dtype == BF and dx.dtype == BF and dw.dtype == torch.float32 and tuple(dw.shape) == tuple(w.shape)
    assert tuple(y.shape) == tuple(dy.shape) and tuple(dx.shape) == tuple(x.shape)
    name = "%s %s" % (kind, tuple(x.shape) + (w.shape[0 if kind != "up2" else 1],))
    _close_rounded(name + " y", _np(y), y_ref.numpy())
    _close_rounded(name + " dx", _np(dx), dx_ref.numpy())
    _close(name + " dW", _np(dw), dw_ref.numpy())


# ------------------------------------------------------------------------------------------------ 3. exact structure
@pytest.mark.parametrize("H,W", [(9, 17), (10, 18), (9, 18), (10, 17)])
@pytest.mark.parametrize("ky,kx", [(1, 1), (0, 1), (1, 2), (0, 2)])  # one tap of each parity class of dX
def test_stride2_one_tap_permutation_weight_is_exact(hip, ky, kx, H, W):
    """w non-zero at tap (ky, kx) only, a channel permutation there: y[b, oy, ox, co] = x[b, 2 oy + ky - 1, 2 ox + kx - 1, perm[co]] (zero
    outside the image) and dx is dy scattered to exactly those pixels -- the pixels of one parity phase -- with zeros everywhere else,
    the last row and column included.  No tolerance."""
    rng = np.random.default_rng(5 + 3 * ky + kx)
    B, C = 2, 32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    perm = torch.from_numpy(rng.permutation(C))
    w = torch.zeros((C, C, 3, 3))
    w[torch.arange(C), perm, ky, kx] = 1.0
    x, dy = _bf16_values(rng, (B, H, W, C)), _bf16_values(rng, (B, Ho, Wo, C))
    y, dx, _ = _run("s2", x, w, dy)
    oy = torch.tensor([o for o in range(Ho) if 0 <= 2 * o + ky - 1 < H])
    ox = torch.tensor([o for o in range(Wo) if 0 <= 2 * o + kx - 1 < W])
    iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
    want_y = torch.zeros((B, Ho, Wo, C))
    want_y[:, oy[:, None], ox[None, :]] = x[:, iy[:, None], ix[None, :]][..., perm]
    scattered = torch.zeros((B, len(oy), len(ox), C))
    scattered[..., perm] = dy[:, oy[:, None], ox[None, :]]
    want_dx = torch.zeros((B, H, W, C))
    want_dx[:, iy[:, None], ix[None, :]] = scattered
    assert torch.equal(y.float().cpu(), want_y)
    assert torch.equal(dx.float().cpu(), want_dx)
    ref = _reference64("s2", x, w, dy)  # (the expectation itself)
    assert torch.equal(want_y.double(), ref[0]) and torch.equal(want_dx.double(), ref[1])


def _one_hot_maps(shape_a, pts_a, shape_b, pts_b):
    a, b = torch.zeros(shape_a), torch.zeros(shape_b)
    for bb, yy, xx, c, v in pts_a:
        a[bb, yy, xx, c] = v
    for bb, yy, xx, c, v in pts_b:
        b[bb, yy, xx, c] = v
    return a, b


def test_stride2_one_hot_pixels_give_exactly_the_expected_weight_gradient(hip):
    """x and dy one-hot at chosen (pixel, channel)s of a 10 x 17 map (dy: 5 x 9) -- a corner, the last pixel of map 0 next to the first of
    map 1, the end of a row next to the start of the following one, the last output row of the even-H map: dW has one non-zero per
    in-image tap, each the exact product; neighbours in memory that are not neighbours in the image contribute nothing."""
    B, H, W, cin, cout = 2, 10, 17, 32, 64
    Ho, Wo = 5, 9
    xs = [(0, 0, 0, 3, 0.5), (0, 9, 16, 31, 2.0), (1, 0, 0, 0, -1.5), (0, 2, 16, 9, -0.75), (0, 3, 0, 12, 1.25), (1, 9, 5, 17, 3.0), (1, 7, 4, 20, 0.25)]
    dys = [(0, 0, 0, 5, 1.0), (0, 4, 8, 63, 4.0), (1, 0, 0, 33, 0.25), (0, 1, 8, 21, -0.5), (0, 2, 0, 20, 1.5), (1, 4, 2, 40, -2.0), (1, 4, 3, 41, 8.0)]
    x, dy = _one_hot_maps((B, H, W, cin), xs, (B, Ho, Wo, cout), dys)
    want = torch.zeros((cout, cin, 3, 3))
    n_terms = 0
    for bx, yx, xx_, ci, vx in xs:
        for bd, yd, xd, co, vd in dys:
            ky, kx = yx - 2 * yd + 1, xx_ - 2 * xd + 1
            if bx == bd and 0 <= ky < 3 and 0 <= kx < 3:
                want[co, ci, ky, kx] += vx * vd
                n_terms += 1
    assert n_terms >= 8 and int((want != 0).sum()) == n_terms  # every term lands in an entry of its own
    got = hip.conv2d_wgrad_s2_bf16(x.to(DEV).to(BF), dy.to(DEV).to(BF))
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want.double(), _reference64("s2", x, torch.zeros((cout, cin, 3, 3)), dy)[2])  # (the expectation itself)


@pytest.mark.parametrize("ty,tx", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_2x2_one_tap_permutation_weight_is_an_exact_placement_and_gather(hip, ty, tx):
    """a weight that is a channel permutation at tap (ty, tx) and zero elsewhere: up2 places the coarse pixels at (2 y + ty, 2 x + tx) and
    writes zeros to the three other pixels of every block; down2 gathers exactly those pixels.  On an odd fine map for Conv2d(2, 2)."""
    rng = np.random.default_rng(20 + 2 * ty + tx)
    B, Hc, Wc, C = 2, 4, 8, 32
    perm = torch.from_numpy(rng.permutation(C))
    # ConvTranspose2d: w[ci, co]; y[.., co] = x[.., perm[co]]
    w = torch.zeros((C, C, 2, 2))
    w[perm, torch.arange(C), ty, tx] = 1.0
    x, dy = _bf16_values(rng, (B, Hc, Wc, C)), _bf16_values(rng, (B, 2 * Hc, 2 * Wc, C))
    y, dx, _ = _run("up2", x, w, dy)
    want_y = torch.zeros((B, 2 * Hc, 2 * Wc, C))
    want_y[:, ty::2, tx::2] = x[..., perm]
    want_dx = torch.zeros((B, Hc, Wc, C))
    want_dx[..., perm] = dy[:, ty::2, tx::2]
    assert torch.equal(y.float().cpu(), want_y) and torch.equal(dx.float().cpu(), want_dx)
    # Conv2d(2, 2): w[co, ci]; y[.., co] = x[2 y + ty, 2 x + tx, perm[co]], on a 9 x 17 fine map
    H, W = 2 * Hc + 1, 2 * Wc + 1
    w = torch.zeros((C, C, 2, 2))
    w[torch.arange(C), perm, ty, tx] = 1.0
    x, dy = _bf16_values(rng, (B, H, W, C)), _bf16_values(rng, (B, Hc, Wc, C))
    y, dx, _ = _run("down2", x, w, dy)
    want_dx = torch.zeros((B, H, W, C))
    scattered = torch.zeros((B, Hc, Wc, C))
    scattered[..., perm] = dy
    want_dx[:, ty:2 * Hc:2, tx:2 * Wc:2] = scattered
    assert torch.equal(y.float().cpu(), x[:, ty:2 * Hc:2, tx:2 * Wc:2][..., perm]) and torch.equal(dx.float().cpu(), want_dx)


@pytest.mark.parametrize("fine_major", [False, True])
def test_2x2_one_hot_pixels_give_exactly_the_expected_weight_gradient(hip, fine_major):
    """coarse and fine one-hot at chosen pixels of a 9 x 17 fine map (coarse 4 x 8): one exact product per (coarse pixel, fine pixel of
    its block); the fine map's unread last row and column, the neighbouring block and the other map contribute nothing."""
    B, H, W, cc, cf = 2, 9, 17, 64, 32
    coarse_pts = [(0, 0, 0, 5, 1.0), (0, 3, 7, 63, 4.0), (1, 0, 0, 33, 0.25), (0, 1, 7, 21, -0.5), (0, 2, 0, 20, 1.5), (1, 3, 2, 40, -2.0)]
    fine_pts = [(0, 0, 0, 3, 0.5), (0, 1, 1, 4, 2.0), (0, 7, 15, 31, -1.5), (0, 6, 14, 30, 0.75), (1, 0, 1, 0, 3.0), (0, 3, 15, 9, -0.75), (0, 4, 0, 12, 1.25),
                (0, 5, 1, 13, 0.125), (1, 7, 4, 17, 8.0), (1, 6, 5, 18, -4.0), (0, 8, 15, 7, 2.0), (0, 7, 16, 8, 2.0), (1, 7, 6, 19, 1.0), (0, 0, 2, 2, 1.0)]
    coarse, fine = _one_hot_maps((B, H // 2, W // 2, cc), coarse_pts, (B, H, W, cf), fine_pts)
    want = torch.zeros((cc, cf, 2, 2))
    n_terms = 0
    for bc, yc, xc, a, vc in coarse_pts:
        for bf_, yf, xf, f, vf in fine_pts:
            if bc == bf_ and yf // 2 == yc and xf // 2 == xc:
                want[a, f, yf % 2, xf % 2] += vc * vf
                n_terms += 1
    assert n_terms >= 10 and int((want != 0).sum()) == n_terms
    got = hip.conv2d_wgrad_2x2_bf16(coarse.to(DEV).to(BF), fine.to(DEV).to(BF), fine_major=fine_major)
    assert torch.equal(got.cpu(), want.transpose(0, 1).contiguous() if fine_major else want)
    assert torch.equal(want.double(), _reference64("down2", fine, torch.zeros((cc, cf, 2, 2)), coarse)[2])  # (the expectation itself)


@pytest.mark.parametrize("H,W", [(9, 17), (9, 16), (8, 17)])
def test_conv2d_k2s2_gradient_of_the_unread_edge_is_exactly_zero(hip, H, W):
    """the wrapper takes no ``out``: asserted on the returned gradient"""
    x, w, dy = _problem("down2f", (2, H, W, 32, 64))[:3]
    dx = _run("down2f", x, w, dy)[1].float().cpu()
    if H % 2:
        assert bool((dx[:, H - 1] == 0).all())
    if W % 2:
        assert bool((dx[:, :, W - 1] == 0).all())
    assert bool((dx[:, :H // 2 * 2, :W // 2 * 2] != 0).any())


def _powers_of_two(rng, shape):
    pw = np.array([0.25, 0.5, 1.0, 2.0, -0.25, -0.5, -1.0, -2.0], np.float32)
    return torch.from_numpy(pw[rng.integers(0, 8, shape)])


def test_border_ring_gradients_are_exact_on_powers_of_two(hip):
    """the gradient map non-zero on its border ring only, all values small powers of two: every partial sum is exact in fp32, so each new
    dW equals float64 (the border-ring test of test_gpu_dense_conv_train_bf16.py)"""
    rng = np.random.default_rng(6)
    B, cin, cout = 2, 32, 32
    for H, W in ((9, 17), (10, 18)):
        x = _powers_of_two(rng, (B, H, W, cin))
        dy = _powers_of_two(rng, (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, cout))
        dy[:, 1:-1, 1:-1, :] = 0.0
        want = _reference64("s2", x, torch.zeros((cout, cin, 3, 3)), dy)[2]
        got = hip.conv2d_wgrad_s2_bf16(x.to(DEV).to(BF), dy.to(DEV).to(BF))
        assert float(want.abs().max()) > 4.0 and torch.equal(got.double().cpu(), want)
    for H, W in ((10, 18), (11, 19)):
        fine = _powers_of_two(rng, (B, H, W, cin))
        coarse = _powers_of_two(rng, (B, H // 2, W // 2, cout))
        coarse[:, 1:-1, 1:-1, :] = 0.0
        want = _reference64("down2", fine, torch.zeros((cout, cin, 2, 2)), coarse)[2]  # [Ccoarse, Cfine, 2, 2]
        got = hip.conv2d_wgrad_2x2_bf16(coarse.to(DEV).to(BF), fine.to(DEV).to(BF))
        assert float(want.abs().max()) > 4.0 and torch.equal(got.double().cpu(), want)
        got_t = hip.conv2d_wgrad_2x2_bf16(coarse.to(DEV).to(BF), fine.to(DEV).to(BF), fine_major=True)
        assert torch.equal(got_t, got.transpose(0, 1).contiguous())


# ------------------------------------------------------------------------------------------------ 4. determinism and workspace
def _raw():
    from futuredet_amd import lib

    return lib, lib.load(), (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("case", [(2, 18, 34, 64, 96), (1, 12, 20, 128, 256), "chunks"], ids=str)
def test_stride2_gradients_are_deterministic_and_read_only_what_they_wrote(hip, case):
    x, w, dy = _problem("s2", case)[:3]
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    xd, dyd = x.to(DEV).to(BF), dy.to(DEV).to(BF)
    first = hip.conv2d_wgrad_s2_bf16(xd, dyd)
    assert torch.equal(first, hip.conv2d_wgrad_s2_bf16(xd, dyd))
    lib, L, p, stream = _raw()
    need = L.fd_conv2d_wgrad_s2_bf16_workspace_bytes(B, H, W, cin, cout)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.full((cout, cin, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
    lib.check(L.fd_conv2d_wgrad_s2_bf16(p(xd), p(dyd), B, H, W, cin, cout, p(ws), need, p(dw), stream), "fd_conv2d_wgrad_s2_bf16")
    torch.cuda.synchronize()
    assert torch.equal(dw, first)  # a workspace full of NaN changes nothing
    wpk = hip.pack_conv2d_weight_device(w.to(DEV), transposed=True)
    dx = hip.conv2d_s2_dgrad_bf16(dyd, wpk, H, W, cin)
    again = hip.conv2d_s2_dgrad_bf16(dyd, wpk, H, W, cin, out=torch.full((B, H, W, cin), float("nan"), dtype=BF, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int16), again.view(torch.int16))  # every element is written, the same bits


@pytest.mark.parametrize("kind,case", [("up2", (2, 9, 17, 64, 96)), ("down2", (1, 8, 8, 256, 128)), ("down2f", (2, 9, 17, 32, 64)), ("up2", "chunks")], ids=str)
def test_2x2_gradients_are_deterministic_and_read_only_what_they_wrote(hip, kind, case):
    x, w, dy = _problem(kind, case)[:3]
    coarse, fine = (x, dy) if kind == "up2" else (dy, x)
    B, H, W, cf = fine.shape
    cc = coarse.shape[3]
    cd, fd = coarse.to(DEV).to(BF), fine.to(DEV).to(BF)
    first = hip.conv2d_wgrad_2x2_bf16(cd, fd)
    assert torch.equal(first, hip.conv2d_wgrad_2x2_bf16(cd, fd))
    lib, L, p, stream = _raw()
    need = L.fd_conv2d_wgrad_2x2_bf16_workspace_bytes(B, H, W, cc, cf)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    dw = torch.full((cc, cf, 2, 2), float("nan"), dtype=torch.float32, device=DEV)
    lib.check(L.fd_conv2d_wgrad_2x2_bf16(p(cd), p(fd), B, H, W, cc, cf, 0, p(ws), need, p(dw), stream), "fd_conv2d_wgrad_2x2_bf16")
    torch.cuda.synchronize()
    assert torch.equal(dw, first)
    wd = w.to(DEV)  # [Ccoarse, Cfine, 2, 2] for both module kinds
    down = hip.conv2d_down2_bf16(fd, hip.pack_conv2d_weight_2x2_device(wd, hip.PACK_DOWN2), cc)
    again = hip.conv2d_down2_bf16(fd, hip.pack_conv2d_weight_2x2_device(wd, hip.PACK_DOWN2), cc,
                                  out=torch.full((B, H // 2, W // 2, cc), float("nan"), dtype=BF, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(down.view(torch.int16), again.view(torch.int16))


# ------------------------------------------------------------------------------------------------ 5. no host synchronisation
@pytest.mark.parametrize("kind,case", [("s2", (2, 18, 34, 64, 96)), ("up2", (2, 9, 17, 64, 96)), ("down2", (2, 9, 17, 64, 96)), ("down2f", (2, 9, 17, 32, 64))],
                         ids=str)
def test_forward_and_backward_do_not_synchronise(hip, kind, case):
    x, w, dy = _problem(kind, case)[:3]
    xd, wd, dyd = x.to(DEV).to(BF).requires_grad_(True), w.to(DEV).requires_grad_(True), dy.to(DEV).to(BF)
    fn = _fn(kind)

    def step():
        xd.grad = wd.grad = None
        y = fn(xd, wd)
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
def _rpn(pillars, seed=0):
    from futuredet_amd.necks import RPN

    torch.manual_seed(seed)
    if pillars:
        neck = RPN(layer_nums=[1, 1, 1], ds_layer_strides=[2, 2, 2], ds_num_filters=[32, 64, 64], us_layer_strides=[0.5, 1, 2],
                   us_num_filters=[32, 32, 32], num_input_features=32)
    else:  # the small RPN of test_gpu_dense_conv_train_bf16.py
        neck = RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[64, 64],
                   num_input_features=32)
    neck.init_weights()
    return neck.to(DEV).train()


def _bev(seed=3):
    return _bf16_values(np.random.default_rng(seed), (2, 32, 16, 24)).to(DEV)


NAMES = {"conv2d_bf16": "s1", "conv2d_s2_bf16": "s2", "conv_transpose2d_k2_bf16": "up2", "conv2d_k2s2_bf16": "down2"}


class _Recorder(object):
    """wraps the four differentiable functions of dense_train (every call recorded with x, weight, y and, after the backward, dy and dx) and
    counts the calls of nn.Conv2d.forward / nn.ConvTranspose2d.forward: the convolutions that still run as modules"""

    def __init__(self, keep_tensors=True):
        self.seen, self.module_calls, self.keep = [], [], keep_tensors

    def __enter__(self):
        from futuredet_amd import dense_train

        self.saved = {n: getattr(dense_train, n) for n in NAMES}
        self.saved_fwd = (nn.Conv2d.forward, nn.ConvTranspose2d.forward)
        for n, kind in NAMES.items():
            setattr(dense_train, n, self._wrap(self.saved[n], kind))
        rec = self

        def conv_forward(m, x, *a, **k):
            rec.module_calls.append(type(m).__name__)
            return rec.saved_fwd[0](m, x, *a, **k)

        def convt_forward(m, x, *a, **k):
            rec.module_calls.append(type(m).__name__)
            return rec.saved_fwd[1](m, x, *a, **k)

        nn.Conv2d.forward, nn.ConvTranspose2d.forward = conv_forward, convt_forward
        return self

    def __exit__(self, *exc):
        from futuredet_amd import dense_train

        for n, f in self.saved.items():
            setattr(dense_train, n, f)
        nn.Conv2d.forward, nn.ConvTranspose2d.forward = self.saved_fwd

    def _wrap(self, orig, kind):
        def recording(x_nhwc, weight, *args):
            if not self.keep:
                self.seen.append(dict(kind=kind, w=weight))
                return orig(x_nhwc, weight, *args)
            if not x_nhwc.requires_grad:
                x_nhwc.requires_grad_(True)
            y = orig(x_nhwc, weight, *args)
            rec = dict(kind=kind, x=x_nhwc.detach(), w=weight, y=y.detach())
            y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
            x_nhwc.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))
            self.seen.append(rec)
            return y

        return recording

    def count(self, kind):
        return sum(1 for r in self.seen if r["kind"] == kind)


def _check_strided_records(seen):
    n = 0
    for i, r in enumerate(seen):
        if r["kind"] == "s1":
            continue
        assert r["x"].dtype == BF and r["y"].dtype == BF and r["dy"].dtype == BF and r["dx"].dtype == BF
        w16 = r["w"].detach().to(BF).float().cpu()  # what the device packer makes of the fp32 master weight
        y_ref, dx_ref, dw_ref = _reference64(r["kind"], r["x"].float().cpu(), w16, r["dy"].float().cpu())
        name = "neck %s %d %s" % (r["kind"], i, tuple(r["w"].shape))
        _close_rounded(name + " y", _np(r["y"]), y_ref.numpy())
        _close_rounded(name + " dx", _np(r["dx"]), dx_ref.numpy())
        _close(name + " dW", _np(r["w"].grad), dw_ref.numpy())
        n += 1
    return n


@pytest.mark.parametrize("pillars", [False, True], ids=["small", "pointpillars"])
def test_neck_runs_no_module_convolution_in_mixed_precision(hip, pillars):
    """RPN.train_dtype = bfloat16: every convolution of the small neck is one of the bf16 functions -- nn.Conv2d.forward and
    nn.ConvTranspose2d.forward are not called at all -- the result is the fp32 NCHW-contiguous map, every parameter has a finite fp32
    gradient, and every strided call (x, weight, y, the incoming dy, dx, dW) matches its own float64 restatement.

    The PointPillars-shaped neck: 3 stride-2 calls and 1 up2 call.  Its Conv2d(2, stride 2) deblock was measured no faster than the
    module on an fp32 copy beyond that recipe's own spread (profiles/dense_conv_strided_bf16.txt), so run_stack_bf16 does not route it:
    0 down2 calls and exactly that one module convolution.  conv2d_k2s2_bf16 itself is covered by the tests above."""
    neck = _rpn(pillars)
    want_shape = tuple(copy.deepcopy(neck).forward_modules(_bev()).shape)
    neck.train_dtype = BF
    x = _bev().requires_grad_(True)
    with _Recorder() as rec:
        out = neck(x)
        out.backward(_bf16_values(np.random.default_rng(4), tuple(out.shape)).to(DEV))
        torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == want_shape == ((2, 96, 4, 6) if pillars else (2, 128, 16, 24))
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for name, p in neck.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    counts = {k: rec.count(k) for k in ("s1", "s2", "up2", "down2")}
    assert counts == (dict(s1=4, s2=3, up2=1, down2=0) if pillars else dict(s1=4, s2=1, up2=1, down2=0)), counts
    assert rec.module_calls == (["Conv2d"] if pillars else []), rec.module_calls  # (the forward only: the backward is autograd's)
    assert _check_strided_records(rec.seen) == (4 if pillars else 2)


@pytest.mark.parametrize("pillars", [False, True], ids=["small", "pointpillars"])
def test_neck_with_fused_batch_norm_routes_the_same_layers(hip, pillars):
    neck = _rpn(pillars)
    stats = {k: b.clone() for k, b in neck.named_buffers()}
    neck.train_dtype, neck.fused_bn = BF, True
    x = _bev().requires_grad_(True)
    with _Recorder(keep_tensors=False) as rec:
        out = neck(x)
        out.backward(_bf16_values(np.random.default_rng(4), tuple(out.shape)).to(DEV))
        torch.cuda.synchronize()
    counts = {k: rec.count(k) for k in ("s1", "s2", "up2", "down2")}
    assert counts == (dict(s1=4, s2=3, up2=1, down2=0) if pillars else dict(s1=4, s2=1, up2=1, down2=0)), counts
    assert rec.module_calls == (["Conv2d"] if pillars else []), rec.module_calls  # (the unrouted Conv2d(2, stride 2) deblock)
    assert out.dtype == torch.float32 and out.is_contiguous() and bool(torch.isfinite(out).all())
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for name, p in neck.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for k, b in neck.named_buffers():
        assert not torch.equal(b, stats[k]), "BatchNorm buffer %s did not move" % k


# ------------------------------------------------------------------------------------------------ 7. one training step
def test_one_forecast_n0_training_step_with_the_strided_layers_in_bf16(hip):
    """forecast_n0 with backbone, neck and head in bf16 through solver.train_steps: a finite loss, exactly one stride-2 and one up2 call,
    the weights of blocks.1.1 (the stage opener) and deblocks.1.0 (the transposed deblock) move and stay finite, same state-dict keys"""
    from futuredet_amd import build_detector, solver
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
    net.bbox_head.train_dtype = net.neck.train_dtype = net.backbone.train_dtype = BF
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    names = ("blocks.1.1.weight", "deblocks.1.0.weight")
    params = dict(net.neck.named_parameters())
    assert tuple(params[names[0]].shape) == (256, 128, 3, 3) and tuple(params[names[1]].shape) == (256, 256, 2, 2)
    before = {k: params[k].detach().clone() for k in names}
    with _Recorder(keep_tensors=False) as rec:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        out = next(solver.train_steps(net, [ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2)))
        torch.cuda.synchronize()
    assert all(np.isfinite(float(l.detach())) for l in out["loss"])
    neck_calls = [r for r in rec.seen if any(r["w"] is p for p in net.neck.parameters())]
    assert sum(1 for r in neck_calls if r["kind"] == "s2") == 1 and sum(1 for r in neck_calls if r["kind"] == "up2") == 1
    assert sum(1 for r in neck_calls if r["kind"] == "s1") == 12 and rec.count("down2") == 0
    assert any(r["w"] is params[names[0]] and r["kind"] == "s2" for r in rec.seen)
    assert any(r["w"] is params[names[1]] and r["kind"] == "up2" for r in rec.seen)
    for k in names:
        assert bool(torch.isfinite(params[k]).all()) and not torch.equal(params[k].detach(), before[k]), "neck parameter %s did not move" % k
    assert list(net.state_dict()) == keys
