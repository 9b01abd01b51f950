"""Mixed-precision training of the CenterHead on the device: the kernels of fd_head_tail_bf16.hip (the final convolutions of a SepHead's
branches: bf16 NHWC in, fp32 NCHW out, up to 16 output channels, a bias), the autograd surfaces dense_train.head_tail_bf16 and
dense_train.conv2d_bf16 with a bias, and the head's switch CenterHead.train_dtype, against float64 F.conv2d and its autograd on the CPU.

Bounds (test_gpu_dense_conv_train_bf16.py).  bf16 x bf16 products are exact in fp32, so a result that is not rounded again (y of the tail,
dW, dbias) differs from float64 only by the fp32 accumulation: 1e-4 * scale, scale = max(1, max |ref|).  A result that is rounded once to
bf16 (dx; y of conv2d_bf16) gets |got - ref| <= 2^-8 |ref| + 1.01e-4 * scale.

Tiles of the kernels.  Forward and dgrad: one MFMA tile is 16 pixels (flat (b, y, x) order) x 16 output channels, a wave owns 4 tiles, a
workgroup 256 pixels; the forward stages the weights of 64 input channels per round, a dgrad workgroup owns 64 input channels.  Wgrad:
chunks of head_tail_wgrad_chunk() (1024) input pixels, whose 32-pixel steps the four waves take in turn; a workgroup owns 64 input
channels.  A launch
takes head_tail_max_groups() (8) groups.  The shapes below (B, H, W, [(cin, k), ...]) are the smallest that cross each of them."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
U = 2.0 ** -8

CASES = [(1, 3, 5, ((64, 3),), False),                                  # a map smaller than one tile
         (2, 17, 17, ((64, 1), (64, 2)), False),                        # one pixel past the 16-pixel tile in a row, 33 past a workgroup, two maps
         (1, 1, 257, ((32, 16),), False),                               # one pixel past a workgroup
         (2, 20, 28, ((64, 2), (64, 1), (64, 3), (64, 2), (64, 14), (64, 16)), True),   # ragged; 6 slices of one [B, H, W, 384] tensor
         (2, 9, 17, ((128, 2), (64, 3), (64, 16), (128, 14), (64, 1), (64, 2), (32, 3), (64, 5), (64, 2)), False),  # one more than a launch takes
         (1, 12, 20, ((128, 14), (160, 3)), False),                     # two full weight stages; two stages + 32 channels, 2.5 channel blocks
         "chunks"]                                                      # 1 x 1 x (2 chunk + 1): two chunks and one pixel of a third


def _case(case):
    if case == "chunks":
        from futuredet_amd import hip_ops

        return (1, 1, 2 * hip_ops.head_tail_wgrad_chunk() + 1, ((32, 3),), False)
    return case


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(name, got, ref, tol=1e-4):
    """element-wise |got - ref| <= tol * scale, scale = max(1, max |ref|): results that are not rounded to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert_close(name, got / scale, ref / scale, tol)


def _close_rounded(name, got, ref):
    """|got - ref| <= 2^-8 |ref| + 1.01e-4 * scale: results rounded once to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    excess = float(((np.abs(got - ref) - U * np.abs(ref)) / scale).max()) if ref.size else 0.0
    report(name + " (beyond 2^-8 |ref|, / scale)", excess, 1.01e-4)
    assert excess <= 1.01e-4, "%s: |got - ref| - 2^-8 |ref| = %.3e * scale > 1.01e-4 * scale" % (name, excess)


def _bf16_values(rng, shape):
    """uniform (-1, 1), rounded to bf16, as float32"""
    return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(BF).float()


def _tie_values(rng, shape):
    """fp32 values of which a third sit exactly half way between two bf16 values (both parities of the lower neighbour), the rest
    have random low bits"""
    v = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))
    bits = v.view(torch.int32)
    kind = torch.from_numpy(rng.integers(0, 3, shape).astype(np.int32))
    tie = (bits & ~0xFFFF) | 0x8000
    return torch.where(kind == 0, tie, bits).view(torch.float32).contiguous()


def _reference64(x_nhwc, w, b, dy_nchw, dy_for_bias=None):
    """float64 F.conv2d (3 x 3, padding 1, bias) and its autograd on the CPU: y NCHW, dx NHWC, dW OIHW, dbias"""
    x = x_nhwc.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    y = F.conv2d(x, w, b.double(), padding=1)
    y.backward(dy_nchw.double())
    db = (dy_nchw if dy_for_bias is None else dy_for_bias).double().sum((0, 2, 3))
    return y.detach(), x.grad.permute(0, 2, 3, 1), w.grad, db


def _run(xs, ws, bs, dys, strided):
    """dense_train.head_tail_bf16 forward + backward on the device.  strided: the groups read consecutive channel slices of ONE tensor.
    Returns per group (y fp32 NCHW, dx bf16 NHWC, dW, dbias)."""
    from futuredet_amd import dense_train

    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = [b.to(DEV).requires_grad_(True) for b in bs]
    if strided:
        wide = torch.cat(xs, dim=3).to(DEV).to(BF).requires_grad_(True)
        offs = np.cumsum([0] + [x.shape[3] for x in xs])
        ys = dense_train.head_tail_bf16([(wide, w, b, int(o)) for w, b, o in zip(wd, bd, offs)])
    else:
        xd = [x.to(DEV).to(BF).requires_grad_(True) for x in xs]
        ys = dense_train.head_tail_bf16([(x, w, b) for x, w, b in zip(xd, wd, bd)])
    torch.autograd.backward(ys, [dy.to(DEV) for dy in dys])
    torch.cuda.synchronize()
    dxs = [wide.grad[..., offs[i]:offs[i + 1]] for i in range(len(xs))] if strided else [x.grad for x in xd]
    return [(y.detach(), dx, w.grad, b.grad) for y, dx, w, b in zip(ys, dxs, wd, bd)]


_problems = {}


def _problem(case):
    """operands (uniform (-1, 1) rounded to bf16) and the float64 reference of a case: computed once, shared, never modified"""
    if case not in _problems:
        B, H, W, groups, strided = _case(case)
        rng = np.random.default_rng(2000 + len(_problems))
        xs = [_bf16_values(rng, (B, H, W, cin)) for cin, _ in groups]
        ws = [_bf16_values(rng, (k, cin, 3, 3)) for cin, k in groups]
        bs = [_bf16_values(rng, (k,)) for _, k in groups]
        dys = [_bf16_values(rng, (B, k, H, W)) for _, k in groups]
        refs = [_reference64(x, w, b, dy) for x, w, b, dy in zip(xs, ws, bs, dys)]
        _problems[case] = (xs, ws, bs, dys, strided, refs)
    return _problems[case]


def _check_groups(name, got, refs, ws):
    for i, ((y, dx, dw, db), (y_ref, dx_ref, dw_ref, db_ref)) in enumerate(zip(got, refs)):
        assert y.dtype == torch.float32 and y.is_contiguous() and dx.dtype == BF and dw.dtype == torch.float32 and db.dtype == torch.float32
        assert tuple(dw.shape) == tuple(ws[i].shape) and tuple(db.shape) == (ws[i].shape[0],)
        tag = "%s group %d (%d -> %d)" % (name, i, ws[i].shape[1], ws[i].shape[0])
        _close(tag + " y", _np(y), y_ref.numpy())
        _close_rounded(tag + " dx", _np(dx), dx_ref.numpy())
        _close(tag + " dW", _np(dw), dw_ref.numpy())
        _close(tag + " dbias", _np(db), db_ref.numpy())


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("case", CASES, ids=str)
def test_tail_matches_float64(hip, case):
    xs, ws, bs, dys, strided, refs = _problem(case)
    if len(ws) > hip.head_tail_max_groups():
        assert len(ws) == hip.head_tail_max_groups() + 1
    _check_groups("head_tail %s" % (_case(case)[:3],), _run(xs, ws, bs, dys, strided), refs, ws)


def test_weights_and_dy_are_rounded_to_nearest_even_inside(hip):
    """fp32 weights and dy that are not bf16 values, a third of them ties: y, dx and dW equal the float64 results on the operands rounded
    by torch; dbias sums the unrounded dy"""
    rng = np.random.default_rng(7)
    B, H, W, groups = 2, 9, 17, ((64, 3), (64, 14))
    xs = [_bf16_values(rng, (B, H, W, cin)) for cin, _ in groups]
    ws = [_tie_values(rng, (k, cin, 3, 3)) for cin, k in groups]
    bs = [torch.from_numpy(rng.uniform(-1, 1, (k,)).astype(np.float32)) for _, k in groups]
    dys = [_tie_values(rng, (B, k, H, W)) for _, k in groups]
    for t in ws + dys:
        bits = t.view(torch.int32)
        assert int(((bits & 0xFFFF) == 0x8000).sum()) > t.numel() // 6
        assert not torch.equal(t.to(BF).float(), t)
    refs = [_reference64(x, w.to(BF).float(), b, dy.to(BF).float(), dy_for_bias=dy) for x, w, b, dy in zip(xs, ws, bs, dys)]
    got = _run(xs, ws, bs, dys, False)
    _check_groups("head_tail ties", got, refs, ws)
    for (_, _, _, db), dy in zip(got, dys):  # the rounded dy would miss this by far more than the bound
        rounded = dy.to(BF).double().sum((0, 2, 3))
        assert float((rounded - dy.double().sum((0, 2, 3))).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 2. exact structure
def test_zero_dy_gives_exact_zeros(hip):
    xs, ws, bs, dys, strided, _ = _problem(CASES[1])
    for _, dx, dw, db in _run(xs, ws, bs, [torch.zeros_like(dy) for dy in dys], strided):
        for t in (dx, dw, db):
            assert int(torch.count_nonzero(t)) == 0 and bool(torch.isfinite(t).all())


def test_one_hot_operands_reproduce_the_tap_geometry_exactly(hip):
    """Output channel t of 9 has the single weight 1 at tap t = (ky, kx), input channel 5 t + 2: y[b, t, y, x] = x[b, y + ky - 1,
    x + kx - 1, 5 t + 2] and dx[b, y + ky - 1, x + kx - 1, 5 t + 2] = dy[b, t, y, x], zeros shifted in at the border.  x and dy are
    one-hot per pixel at the corners, the ends of rows next to the starts of the following ones and the last pixel of map 0 next to the
    first of map 1.  No tolerance."""
    B, H, W, cin, k = 2, 9, 17, 64, 9
    pix = [(0, 0, 0), (0, 0, 16), (0, 8, 0), (0, 8, 16), (1, 0, 0), (1, 8, 16), (0, 3, 16), (0, 4, 0), (1, 4, 8), (1, 5, 9), (0, 0, 7), (1, 8, 3)]
    w = torch.zeros((k, cin, 3, 3))
    for t in range(9):
        w[t, 5 * t + 2, t // 3, t % 3] = 1.0
    x, dy = torch.zeros((B, H, W, cin)), torch.zeros((B, k, H, W))
    for n, (b, yy, xx) in enumerate(pix):
        for t in range(9):
            x[b, yy, xx, 5 * t + 2] = (2 * n + 1) * 2.0 ** (t - 4)  # an odd number times a power of two: bf16 values, all distinct
            dy[b, t, yy, xx] = -(2 * n + 1) * 2.0 ** (t - 6)
    want_y, want_dx = torch.zeros((B, k, H, W)), torch.zeros((B, H, W, cin))
    for t in range(9):
        sy, sx = t // 3 - 1, t % 3 - 1
        ys, yd = slice(max(sy, 0), H + min(sy, 0)), slice(max(-sy, 0), H + min(-sy, 0))  # source rows y + sy for output rows y
        xs_, xd = slice(max(sx, 0), W + min(sx, 0)), slice(max(-sx, 0), W + min(-sx, 0))
        want_y[:, t, yd, xd] = x[:, ys, xs_, 5 * t + 2]
        want_dx[:, ys, xs_, 5 * t + 2] = dy[:, t, yd, xd]
    (y, dx, dw, db), = _run([x], [w], [torch.zeros((k,))], [dy], False)
    assert torch.equal(x.to(BF).float(), x) and torch.equal(dy.to(BF).float(), dy)
    assert int(torch.count_nonzero(want_y)) == 6 * 4 + 4 * 6 + 2 * 9 == int(torch.count_nonzero(want_dx))  # corners, edges, interior
    assert torch.equal(y.cpu(), want_y)
    assert torch.equal(dx.float().cpu(), want_dx)
    ref = _reference64(x, w, torch.zeros((k,)), dy)
    assert torch.equal(want_y.double(), ref[0]) and torch.equal(want_dx.double(), ref[1])  # (the expectation itself)
    assert torch.equal(dw.double().cpu(), ref[2]) and torch.equal(db.double().cpu(), ref[3])  # small integers and halves: exact in fp32


def test_strided_dgrad_leaves_the_other_channels_alone(hip):
    """dx written into slices 0 and 2 of a [B, H, W, 3 * 64] tensor: slice 1 keeps its canary bits, the written slices equal the
    contiguous run's"""
    xs, ws, bs, dys, _, _ = _problem(CASES[1])
    want = _run(xs, ws, bs, dys, False)
    B, H, W, _ = xs[0].shape
    canary = torch.full((B, H, W, 192), -7.5, dtype=BF, device=DEV)
    wide = canary.clone()
    hip.head_tail_dgrad([(wide, 0, ws[0].to(DEV), dys[0].to(DEV)), (wide, 128, ws[1].to(DEV), dys[1].to(DEV))])
    torch.cuda.synchronize()
    assert torch.equal(wide[..., 64:128], canary[..., 64:128])
    assert torch.equal(wide[..., :64], want[0][1]) and torch.equal(wide[..., 128:], want[1][1])


# ------------------------------------------------------------------------------------------------ 3. determinism and workspace
@pytest.mark.parametrize("case", [CASES[3], "chunks"], ids=str)
def test_two_runs_are_bit_identical_and_the_workspace_is_written_before_it_is_read(hip, case):
    from futuredet_amd import lib

    xs, ws, bs, dys, strided, _ = _problem(case)
    first, second = _run(xs, ws, bs, dys, strided), _run(xs, ws, bs, dys, strided)
    for a, b in zip(first, second):
        for s, t in zip(a, b):
            assert torch.equal(s, t)
    # the weight gradient again through the C ABI, on a workspace full of NaN
    L = lib.load()
    B, H, W, _ = xs[0].shape
    xd = [x.to(DEV).to(BF) for x in xs]
    dyd = [dy.to(DEV) for dy in dys]
    dws = [torch.full(tuple(w.shape), float("nan"), device=DEV) for w in ws]
    dbs = [torch.full((w.shape[0],), float("nan"), device=DEV) for w in ws]
    recs = [hip._head_tail_group("test", x, 0, dw, db, dy)[0] for x, dw, db, dy in zip(xd, dws, dbs, dyd)]
    need = L.fd_head_tail_wgrad_bf16_workspace_bytes(B, H, W, sum(x.shape[3] for x in xs))
    assert need > 0 and need % 4 == 0
    wsb = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    arr = (lib.HeadTailGroup * len(recs))(*recs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.fd_head_tail_wgrad_bf16(arr, len(recs), B, H, W, ctypes.c_void_p(wsb.data_ptr()), need, stream), "fd_head_tail_wgrad_bf16")
    torch.cuda.synchronize()
    for (_, _, dw, db), dw2, db2 in zip(first, dws, dbs):
        assert torch.equal(dw, dw2) and torch.equal(db, db2)


# ------------------------------------------------------------------------------------------------ 4. no host synchronisation
def test_forward_and_backward_do_not_synchronise(hip):
    from futuredet_amd import dense_train

    xs, ws, bs, dys, _, _ = _problem(CASES[1])
    xd = [x.to(DEV).to(BF).requires_grad_(True) for x in xs]
    wd = [w.to(DEV).requires_grad_(True) for w in ws]
    bd = [b.to(DEV).requires_grad_(True) for b in bs]
    dyd = [dy.to(DEV) for dy in dys]
    wc, bc = torch.randn((64, 64, 3, 3), device=DEV).requires_grad_(True), torch.randn((64,), device=DEV).requires_grad_(True)

    def step():
        for t in xd + wd + bd + [wc, bc]:
            t.grad = None
        ys = dense_train.head_tail_bf16([(dense_train.conv2d_bf16(x, wc, 3, bias=bc), w, b) for x, w, b in zip(xd, wd, bd)])
        torch.autograd.backward(ys, dyd)
        return ys

    step()  # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ys = step()
        with pytest.raises(RuntimeError):  # the mode is enforced on this build
            ys[0].sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for t in xd + wd + bd + [wc, bc]:
        assert t.grad is not None and bool(torch.isfinite(t.grad.float()).all())


# ------------------------------------------------------------------------------------------------ 5. conv2d_bf16 with a bias
def test_conv2d_bf16_with_a_bias(hip):
    from futuredet_amd import dense_train

    rng = np.random.default_rng(11)
    B, H, W, cin, cout = 2, 9, 17, 64, 96
    x, w, dy = _bf16_values(rng, (B, H, W, cin)), _bf16_values(rng, (cout, cin, 3, 3)), _bf16_values(rng, (B, H, W, cout))
    bias = _bf16_values(rng, (cout,))

    def run(b):
        xd, wd = x.to(DEV).to(BF).requires_grad_(True), w.to(DEV).requires_grad_(True)
        bd = None if b is None else b.to(DEV).requires_grad_(True)
        y = dense_train.conv2d_bf16(xd, wd, 3) if b is None else dense_train.conv2d_bf16(xd, wd, 3, bias=bd)
        y.backward(dy.to(DEV).to(BF))
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad, None if b is None else bd.grad

    y0, dx0, dw0, _ = run(None)
    y1, dx1, dw1, db1 = run(torch.zeros((cout,)))
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and torch.equal(dw0, dw1)
    y2, dx2, dw2, db2 = run(bias)
    assert torch.equal(dx2, dx0) and torch.equal(dw2, dw0) and torch.equal(db2, db1)
    y_ref, _, _, db_ref = _reference64(x, w, bias, dy.permute(0, 3, 1, 2))
    _close_rounded("conv2d_bf16 + bias y", _np(y2), y_ref.permute(0, 2, 3, 1).numpy())
    assert db2.dtype == torch.float32 and tuple(db2.shape) == (cout,)
    _close("conv2d_bf16 dbias", _np(db2), db_ref.numpy())


# ------------------------------------------------------------------------------------------------ 6. the head
def _small_head(kind, seed=0):
    from futuredet_amd.heads import CenterHead

    torch.manual_seed(seed)
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    kw = dict(in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
              common_heads=common, share_conv_channel=64, classify=False)
    if kind == "standard_t1":
        head = CenterHead(timesteps=1, **kw)
    elif kind == "standard_t3":
        head = CenterHead(timesteps=3, **kw)
    else:
        head = CenterHead(timesteps=3, dense=True, forecast_feature=True, **kw)
    return head.to(DEV).train()


def _head_input(seed=3):
    return _bf16_values(np.random.default_rng(seed), (2, 64, 12, 20)).to(DEV)


def test_default_train_dtype_is_forward_modules_bit_for_bit(hip, monkeypatch):
    from futuredet_amd import dense_train

    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)

    def refuse(*a, **kw):
        raise AssertionError("the fp32 default must not reach the mixed-precision wrappers")

    for name in ("conv2d_bf16", "head_tail_bf16", "sep_head_bf16", "run_head_stack_bf16"):
        monkeypatch.setattr(dense_train, name, refuse)
    head = _small_head("dense_ff")
    ref = copy.deepcopy(head)
    assert head.train_dtype is torch.float32
    xa, xb = _head_input().requires_grad_(True), _head_input().requires_grad_(True)
    got, want = head(xa), ref.forward_modules(xb)
    rng = np.random.default_rng(4)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in g:
            assert torch.equal(g[k], w[k]), k
    outs_g = [d[k] for d in got for k in d if k != "feats"]
    outs_w = [d[k] for d in want for k in d if k != "feats"]
    grads = [_bf16_values(rng, tuple(t.shape)).to(DEV) for t in outs_g]
    torch.autograd.backward(outs_g, grads)
    torch.autograd.backward(outs_w, grads)
    torch.cuda.synchronize()
    assert torch.equal(xa.grad, xb.grad)
    for (name, p), q in zip(head.named_parameters(), ref.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), name
    for (name, b), c in zip(head.named_buffers(), ref.buffers()):
        assert torch.equal(b, c), name


@pytest.mark.parametrize("kind", ["standard_t1", "standard_t3", "dense_ff"])
def test_head_in_mixed_precision_layer_by_layer(hip, kind):
    """CenterHead.train_dtype = bfloat16, teacher-forced: every conv2d_bf16 and head_tail_bf16 call of the walk is recorded with its actual
    input, output and gradients and compared with a float64 restatement of that call on that input.  The leading convolutions of a
    SepHead's branches are ONE conv2d_bf16 call, its final convolutions ONE head_tail_bf16 call."""
    from futuredet_amd import dense_train

    head = _small_head(kind)
    want = copy.deepcopy(head).forward_modules(_head_input())
    stats = {k: b.clone() for k, b in head.named_buffers()}
    keys = list(head.state_dict())
    head.train_dtype = BF
    x = _head_input().requires_grad_(True)
    convs, tails = [], []
    orig_conv, orig_tail = dense_train.conv2d_bf16, dense_train.head_tail_bf16

    def rec_conv(x_nhwc, weight, ks, bias=None):
        if not x_nhwc.requires_grad:
            x_nhwc.requires_grad_(True)
        y = orig_conv(x_nhwc, weight, ks, bias)
        rec = dict(x=x_nhwc.detach(), w=weight.detach(), b=bias.detach(), ks=ks, y=y.detach())
        for t, key in ((y, "dy"), (x_nhwc, "dx"), (weight, "dw"), (bias, "db")):
            t.register_hook(lambda g, rec=rec, key=key: rec.__setitem__(key, g.detach().clone()))
        convs.append(rec)
        return y

    def rec_tail(groups):
        ys = orig_tail(groups)
        recs = []
        for (xg, w, b), y in zip(groups, ys):
            rec = dict(x=xg.detach(), w=w, b=b, y=y.detach())
            y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
            xg.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))
            recs.append(rec)
        tails.append(recs)
        return ys

    dense_train.conv2d_bf16, dense_train.head_tail_bf16 = rec_conv, rec_tail
    try:
        got = head(x)
        outs = [d[k] for d in got for k in d if k != "feats"]
        rng = np.random.default_rng(4)
        torch.autograd.backward(outs, [_bf16_values(rng, tuple(t.shape)).to(DEV) for t in outs])
        torch.cuda.synchronize()
    finally:
        dense_train.conv2d_bf16, dense_train.head_tail_bf16 = orig_conv, orig_tail
    # the surface: the chain's keys and shapes, fp32 NCHW contiguous; finite gradients everywhere; moving statistics; no new state
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in g:
            assert g[k].dtype == torch.float32 and g[k].is_contiguous() and tuple(g[k].shape) == tuple(w[k].shape), k
    assert x.grad is not None and x.grad.dtype == torch.float32 and bool(torch.isfinite(x.grad).all())
    for name, p in head.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    for k, b in head.named_buffers():
        assert not torch.equal(b, stats[k]), "BatchNorm buffer %s did not move" % k
    assert list(head.state_dict()) == keys
    # one batched convolution and one tail call per SepHead (+ shared_conv, + the two forecast_conv layers of a forecast-feature task)
    n_tasks, ff = len(head.tasks), head.forecast_feature
    n_br = len(head.tasks[0].heads)
    assert n_br == 6 and len(tails) == n_tasks and all(len(t) == n_br for t in tails)
    assert len(convs) == 1 + n_tasks * (3 if ff else 1), [tuple(r["w"].shape) for r in convs]
    assert sum(1 for r in convs if r["w"].shape[0] == 64 * n_br) == n_tasks
    for i, r in enumerate(convs):
        assert r["x"].dtype == BF and r["y"].dtype == BF and r["dy"].dtype == BF and r["dx"].dtype == BF
        w16 = r["w"].to(BF).float().cpu()
        y_ref, dx_ref, dw_ref, db_ref = _reference64(r["x"].float().cpu(), w16, r["b"].cpu(), r["dy"].float().permute(0, 3, 1, 2).cpu())
        name = "%s conv %d %s" % (kind, i, tuple(r["w"].shape[:2]))
        _close_rounded(name + " y", _np(r["y"]), y_ref.permute(0, 2, 3, 1).numpy())
        _close_rounded(name + " dx", _np(r["dx"]), dx_ref.numpy())
        _close(name + " dW", _np(r["dw"]), dw_ref.numpy())
        _close(name + " dbias", _np(r["db"]), db_ref.numpy())
    ks = []
    for ti, recs in enumerate(tails):
        for gi, r in enumerate(recs):
            assert r["x"].dtype == BF and r["y"].dtype == torch.float32 and r["dx"].dtype == BF
            ks.append(r["w"].shape[0])
            w16 = r["w"].detach().to(BF).float().cpu()
            dy = r["dy"].float().cpu()
            y_ref, dx_ref, dw_ref, db_ref = _reference64(r["x"].float().cpu(), w16, r["b"].detach().cpu(), dy.to(BF).float(), dy_for_bias=dy)
            name = "%s task %d tail %d (%d)" % (kind, ti, gi, r["w"].shape[0])
            _close(name + " y", _np(r["y"]), y_ref.numpy())
            _close_rounded(name + " dx", _np(r["dx"]), dx_ref.numpy())
            _close(name + " dW", _np(r["w"].grad), dw_ref.numpy())
            _close(name + " dbias", _np(r["b"].grad), db_ref.numpy())
    assert sorted(set(ks)) == ([1, 2, 3, 6] if kind == "standard_t3" else [1, 2, 3])


def test_no_grad_and_eval_ignore_the_switch(hip, monkeypatch):
    from futuredet_amd import dense_train

    head = _small_head("standard_t1")
    head.train_dtype = BF
    ref = copy.deepcopy(head)

    def refuse(*a, **kw):
        raise AssertionError("no_grad must not reach the mixed-precision wrappers")

    monkeypatch.setattr(dense_train, "sep_head_bf16", refuse)
    monkeypatch.setattr(dense_train, "run_head_stack_bf16", refuse)
    with torch.no_grad():
        got, want = head(_head_input()), ref.forward_modules(_head_input())
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k


def test_one_training_step_with_the_whole_net_in_mixed_precision(hip):
    """forecast_n0 with head, neck and backbone in bf16 and the fused loss through solver.train_steps: finite losses, every head parameter
    has a finite gradient and moves, the head's maps are fp32 NCHW contiguous, same state-dict keys"""
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
    assert net.bbox_head.train_dtype is torch.float32
    net.bbox_head.train_dtype = net.neck.train_dtype = net.backbone.train_dtype = BF
    net.bbox_head.fused_loss = True
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    before = {k: p.detach().clone() for k, p in net.bbox_head.named_parameters()}
    maps = []
    handle = net.bbox_head.register_forward_hook(lambda m, a, out: maps.extend(out))
    try:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        out = next(solver.train_steps(net, [ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2)))
    finally:
        handle.remove()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(l.detach())) for l in out["loss"])
    assert len(maps) == len(net.bbox_head.tasks)
    for d in maps:
        for k, t in d.items():
            assert t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous() and t.shape[0] == 1 and tuple(t.shape[2:]) == (180, 180), k
    for k, p in net.bbox_head.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), "head parameter %s did not move" % k
    assert list(net.state_dict()) == keys
