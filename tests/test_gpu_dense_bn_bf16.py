"""-m gpu: the fused training-mode BatchNorm2d (+ ReLU) on bf16 channels-last maps (futuredet_amd/csrc/fd_dense_bn_nhwc.hip over
fd_row_bn.h, dense_bn.batch_norm2d_act_nhwc, RPN.fused_bn / CenterHead.fused_bn with train_dtype = torch.bfloat16) against the formulas in float64
on the bf16-rounded x and dy.

Inputs, references and gates are those of test_gpu_sparse_bn.py: fp32 results (saved, running statistics, dgamma, dbeta) within
1e-5 * max |ref| on inputs (a), 1e-4 * max |ref| on inputs (b) (an offset of +-30 on half the channels; only for n >= 63); y and dx, which
are rounded once to bf16, get 2^-8 |ref| per element on top (test_gpu_sparse_bn_bf16._gate_rounded).  The backward reference is
teacher-forced: it takes its ReLU mask from the kernel's own y.

The two large row counts of test 2 need the float64 formulas on up to 67 M elements: there _ref_forward / _ref_backward are restated
line by line in torch.float64 on the device (_ref_device), and test_device_reference_is_the_numpy_reference ties the restatement to the
numpy functions."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

from parity_util import report
from test_gpu_sparse_bn import DEAD_CH, _gate, _inputs, _ref_backward, _ref_forward
from test_gpu_sparse_bn_bf16 import _gate_rounded, _same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
U = 2.0 ** -8
EPS = 1e-3
INPUTS = (("a", 0.0, 1e-5), ("b", 30.0, 1e-4))
FORMS = (("relu", True), ("plain", False))


def _P():
    from futuredet_amd import hip_ops

    return hip_ops.dense_bn_nhwc_chunk()


def _large(which):
    """the smallest row counts, from the library's own constants, at which (two_chunks) a group of the statistics holds two chunks and the
    last chunk has one row: one chunk more than there are groups, of one row; (two_apply) an apply workgroup covers two chunks: one
    chunk more than there are apply blocks"""
    from futuredet_amd import lib

    L = lib.load()
    P = L.fd_dense_bn_nhwc_chunk()
    return {"two_chunks": L.fd_dense_bn_nhwc_stat_groups() * P + 1, "two_apply": L.fd_dense_bn_nhwc_apply_blocks() * P + 1}[which]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_device_inputs_cache = {}


def _device_inputs(seed, n, C, offset):
    """_inputs on the device, x and dy rounded to bf16; computed once per problem, shared, never modified (of the problems beyond 4 M
    elements only the latest is kept)"""
    key = (seed, n, C, offset)
    if key not in _device_inputs_cache:
        if n * C > 1 << 22:
            for k in [k for k in _device_inputs_cache if k[1] * k[2] > 1 << 22]:
                del _device_inputs_cache[k]
        d = _inputs(seed, n, C, offset)
        _device_inputs_cache[key] = {k: (_t(v).to(BF) if k in ("x", "dy") else _t(v)) for k, v in d.items() if k != "res"}
    return _device_inputs_cache[key]


def _modules(t, sizes, eps=None, momentum=None):
    """fresh BatchNorm2d modules over consecutive channel ranges of the problem ``t``: parameters and running statistics from its vectors"""
    eps = eps or [EPS] * len(sizes)
    momentum = momentum or [0.1] * len(sizes)
    bns, o = [], 0
    for c, e, m in zip(sizes, eps, momentum):
        bn = nn.BatchNorm2d(c, eps=e, momentum=m).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(t["gamma"][o:o + c])
            bn.bias.copy_(t["beta"][o:o + c])
            bn.running_mean.copy_(t["rm"][o:o + c])
            bn.running_var.copy_(t["rv"][o:o + c])
        bns.append(bn)
        o += c
    return bns


def _run(hip, t, relu, sizes=None, eps=None, momentum=None):
    """forward + backward through hip_ops on fresh modules -> dict of device tensors (rm, rv, nbt: the modules' buffers, concatenated)"""
    n, C = t["x"].shape
    bns = _modules(t, sizes or [C], eps, momentum)
    y, saved = hip.dense_bn_nhwc_train_forward(t["x"], bns, relu=relu)
    dx, dgamma, dbeta = hip.dense_bn_nhwc_train_backward(t["dy"], t["x"], y, saved, bns, relu=relu)
    return dict(y=y, saved=saved, dx=dx, dgamma=dgamma, dbeta=dbeta, rm=torch.cat([bn.running_mean for bn in bns]),
                rv=torch.cat([bn.running_var for bn in bns]), nbt=torch.stack([bn.num_batches_tracked for bn in bns]))


def _host(out):
    return {k: (v.float() if v.dtype == BF else v).cpu().numpy() for k, v in out.items()}


def _check_against_float64(hip, t, relu, gate, tag, momentum=0.1):
    """one module over all channels, the numpy reference on the bf16-rounded x and dy"""
    out = _host(_run(hip, t, relu, momentum=[momentum]))
    r = {k: (v.float() if v.dtype == BF else v).cpu().numpy() for k, v in t.items()}
    n = r["x"].shape[0]
    y, pre, mean, var, invstd = _ref_forward(r["x"], r["gamma"], r["beta"], None, relu)
    if relu:
        assert (pre[:, DEAD_CH] < 0).all() and (out["y"][:, DEAD_CH] == 0).all(), "the dead channel must be all zero after the ReLU"
    _gate_rounded(tag + " y", out["y"], y, gate)
    _gate("nhwc " + tag + " saved mean", out["saved"][0], mean, gate)
    _gate("nhwc " + tag + " saved invstd", out["saved"][1], invstd, gate)
    _gate("nhwc " + tag + " running_mean", out["rm"], (1 - momentum) * r["rm"].astype(np.float64) + momentum * mean, gate)
    _gate("nhwc " + tag + " running_var", out["rv"], (1 - momentum) * r["rv"].astype(np.float64) + momentum * var * n / (n - 1), gate)
    assert out["nbt"].tolist() == [1]
    dx, dgamma, dbeta, _ = _ref_backward(r["dy"], r["x"], out["y"], r["gamma"], mean, invstd, relu)
    _gate_rounded(tag + " dx", out["dx"], dx, gate)
    _gate("nhwc " + tag + " dgamma", out["dgamma"], dgamma, gate)
    _gate("nhwc " + tag + " dbeta", out["dbeta"], dbeta, gate)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 64, 128, 160, 256, 384, 512])
@pytest.mark.parametrize("n_of", [lambda P: 2, lambda P: 63, lambda P: P - 1, lambda P: P, lambda P: P + 1, lambda P: 3 * P + 17],
                         ids=["2", "63", "P-1", "P", "P+1", "3P+17"])
def test_kernels_match_float64(hip, n_of, C):
    n = n_of(_P())
    for which, offset, gate in INPUTS:
        if offset and n < 63:
            continue
        t = _device_inputs(n * 1000 + C + (1 if offset else 0), n, C, offset)
        for name, relu in FORMS:
            _check_against_float64(hip, t, relu, gate, "(%s) n=%d C=%d %s" % (which, n, C, name))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _ref_device(t, relu, y_kernel, eps=EPS, momentum=0.1):
    """_ref_forward and _ref_backward of test_gpu_sparse_bn.py, restated in torch.float64 on the device"""
    x, dy = t["x"].double(), t["dy"].double()
    gamma, beta = t["gamma"].double(), t["beta"].double()
    n = x.shape[0]
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mean) * invstd
    pre = gamma * xh + beta
    y = torch.clamp_min(pre, 0.0) if relu else pre
    g = dy * (y_kernel.double() > 0) if relu else dy
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    dx = gamma * invstd * (g - dbeta / n - xh * dgamma / n)
    return dict(y=y, pre=pre, mean=mean, var=var, invstd=invstd, dx=dx, dgamma=dgamma, dbeta=dbeta,
                rm=(1 - momentum) * t["rm"].double() + momentum * mean, rv=(1 - momentum) * t["rv"].double() + momentum * var * n / (n - 1))


def _gate_device(name, got, ref, gate, rounded=False):
    """_gate / _gate_rounded on device tensors"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((((got - ref).abs() - (U * ref.abs() if rounded else 0.0)) / scale).max())
    report("dense bn nhwc " + name, err, gate)
    assert bool(torch.isfinite(got).all()) and err <= gate, "%s: error %.3e of the largest reference value (%.3e) > %.1e" % (name, err, scale, gate)


def test_device_reference_is_the_numpy_reference(hip):
    t = _device_inputs(77, 3 * _P() + 17, 96, 30.0)
    r = {k: (v.float() if v.dtype == BF else v).cpu().numpy() for k, v in t.items()}
    yk = _run(hip, t, True)["y"]
    dev = {k: v.cpu().numpy() for k, v in _ref_device(t, True, yk).items()}
    y, pre, mean, var, invstd = _ref_forward(r["x"], r["gamma"], r["beta"], None, True)
    dx, dgamma, dbeta, _ = _ref_backward(r["dy"], r["x"], yk.float().cpu().numpy(), r["gamma"], mean, invstd, True)
    for k, want in (("y", y), ("pre", pre), ("mean", mean), ("var", var), ("invstd", invstd), ("dx", dx), ("dgamma", dgamma), ("dbeta", dbeta)):
        np.testing.assert_allclose(dev[k], want, rtol=1e-11, atol=1e-11 * float(np.abs(want).max()), err_msg=k)


@pytest.mark.parametrize("which,offset,gate", INPUTS, ids=[i[0] for i in INPUTS])
@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("size", ["two_chunks", "two_apply"])
def test_kernels_match_float64_at_large_n(hip, size, C, which, offset, gate):
    n = _large(size)
    P = _P()
    assert n % P == 1 and n > P, "whole chunks and a last chunk of one row (%d rows, chunk %d)" % (n, P)
    t = _device_inputs(n + C + (1 if offset else 0), n, C, offset)
    tag = "(%s) n=%d C=%d relu" % (which, n, C)
    out = _run(hip, t, True)
    ref = _ref_device(t, True, out["y"])
    assert bool((ref["pre"][:, DEAD_CH] < 0).all()) and int(torch.count_nonzero(out["y"][:, DEAD_CH])) == 0
    _gate_device(tag + " y", out["y"], ref["y"], gate, rounded=True)
    _gate_device(tag + " dx", out["dx"], ref["dx"], gate, rounded=True)
    for k, got in (("mean", out["saved"][0]), ("invstd", out["saved"][1]), ("rm", out["rm"]), ("rv", out["rv"]), ("dgamma", out["dgamma"]),
                   ("dbeta", out["dbeta"])):
        _gate_device(tag + " " + k, got, ref[k], gate)
    assert out["nbt"].tolist() == [1]


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[64] * 6, [32, 64]], ids=["6x64", "32+64"])
def test_groups(hip, sizes):
    C, n = sum(sizes), 3 * _P() + 17
    eps = [(1e-3, 1e-1)[j % 2] for j in range(len(sizes))]
    momentum = [(0.0, 0.1, 1.0)[j % 3] for j in range(len(sizes))]
    for which, offset, gate in INPUTS:
        t = _device_inputs(900 + C + (1 if offset else 0), n, C, offset)
        r = {k: (v.float() if v.dtype == BF else v).cpu().numpy() for k, v in t.items()}
        for name, relu in FORMS:
            dev = _run(hip, t, relu, sizes, eps, momentum)
            out = _host(dev)
            assert out["nbt"].tolist() == [1] * len(sizes)
            o = 0
            for j, c in enumerate(sizes):
                s = slice(o, o + c)
                tag = "(%s) %s group %d of %s (eps %g, momentum %g)" % (which, name, j, sizes, eps[j], momentum[j])
                y, pre, mean, var, invstd = _ref_forward(r["x"][:, s], r["gamma"][s], r["beta"][s], None, relu, eps[j])
                other = 1.0 / np.sqrt(var + eps[1 - j % 2])
                assert float(np.abs(other - invstd).max()) > 100 * gate * float(np.abs(invstd).max()), "the gate must tell the two eps apart"
                _gate_rounded(tag + " y", out["y"][:, s], y, gate)
                _gate("nhwc " + tag + " saved mean", out["saved"][0, s], mean, gate)
                _gate("nhwc " + tag + " saved invstd", out["saved"][1, s], invstd, gate)
                m = momentum[j]
                _gate("nhwc " + tag + " running_mean", out["rm"][s], (1 - m) * r["rm"][s].astype(np.float64) + m * mean, gate)
                _gate("nhwc " + tag + " running_var", out["rv"][s], (1 - m) * r["rv"][s].astype(np.float64) + m * var * n / (n - 1), gate)
                if m == 0.0:
                    assert _same_bits(dev["rm"][s], t["rm"][s]) and _same_bits(dev["rv"][s], t["rv"][s]), tag
                if m == 1.0:
                    assert _same_bits(dev["rm"][s], dev["saved"][0, s]), tag
                dx, dgamma, dbeta, _ = _ref_backward(r["dy"][:, s], r["x"][:, s], out["y"][:, s], r["gamma"][s], mean, invstd, relu)
                _gate_rounded(tag + " dx", out["dx"][:, s], dx, gate)
                _gate("nhwc " + tag + " dgamma", out["dgamma"][s], dgamma, gate)
                _gate("nhwc " + tag + " dbeta", out["dbeta"][s], dbeta, gate)
                o += c


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _raw_run(hip, t, relu, poison):
    """both entry points through ctypes with the workspace, y and dx pre-filled with the NaN pattern ``poison``"""
    from futuredet_amd import lib

    L = lib.load()
    n, C = t["x"].shape
    bns = _modules(t, [C])
    need = L.fd_dense_bn_nhwc_workspace_bytes(n, C)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), poison, dtype=torch.int32, device=DEV)
    y = torch.full((n, C), poison & 0xFFFF, dtype=torch.int16, device=DEV).view(BF)  # (both patterns are positive as int16)
    dx = y.clone()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(ws.view(torch.float32)).all())
    saved = torch.empty((2, C), dtype=torch.float32, device=DEV)
    dgamma, dbeta = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    groups, ng = hip._dense_bn_nhwc_groups(bns, C, True)
    lib.check(L.fd_dense_bn_nhwc_train_forward_bf16(p(t["x"]), groups, ng, n, C, int(relu), p(y), p(saved), p(ws), need, stream), "forward")
    ws.fill_(poison)
    lib.check(L.fd_dense_bn_nhwc_train_backward_bf16(p(t["dy"]), p(t["x"]), p(y), p(saved), groups, ng, n, C, int(relu), p(dx), p(dgamma),
                                                     p(dbeta), p(ws), need, stream), "backward")
    torch.cuda.synchronize()
    return dict(y=y, saved=saved, dx=dx, dgamma=dgamma, dbeta=dbeta, rm=bns[0].running_mean, rv=bns[0].running_var, nbt=bns[0].num_batches_tracked)


@pytest.mark.parametrize("shape", ["3P+17 x 160", "two_apply x 512"])
def test_two_runs_are_bit_identical_and_read_only_what_they_wrote(hip, shape):
    n, C = (3 * _P() + 17, 160) if shape.startswith("3P") else (_large("two_apply"), 512)
    t = _device_inputs(n + C + 1 if n > 4 * _P() else 7, n, C, 30.0)
    for name, relu in FORMS:
        a, b = _raw_run(hip, t, relu, 0x7FC07FC0), _raw_run(hip, t, relu, 0x7FFF7FFF)
        plain = _run(hip, t, relu)
        for k in a:
            assert bool(torch.isfinite(a[k].float()).all()), (name, k)
            assert _same_bits(a[k], b[k]), (name, k)
            assert _same_bits(a[k], plain[k].reshape(a[k].shape)), (name, k, "the front end's bits")


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_bits(hip):
    """forward + backward captured once: nothing in the calls allocates device memory outside torch's allocator or synchronises"""
    n, C = 3 * _P() + 17, 160
    sets = [_device_inputs(20 + i, n, C, 0.0) for i in range(2)]
    eager = [_run(hip, t, True, [32, 128]) for t in sets]
    keys = ("x", "dy", "gamma", "beta", "rm", "rv")
    st = {k: sets[0][k].clone() for k in keys}
    bns = _modules(st, [32, 128])

    def load(t):
        for k in ("x", "dy"):
            st[k].copy_(t[k])
        fresh = _modules(t, [32, 128])
        with torch.no_grad():
            for bn, f in zip(bns, fresh):
                for a, b in zip(list(bn.parameters()) + list(bn.buffers()), list(f.parameters()) + list(f.buffers())):
                    a.copy_(b)

    def step():
        y, saved = hip.dense_bn_nhwc_train_forward(st["x"], bns, relu=True)
        dx, dgamma, dbeta = hip.dense_bn_nhwc_train_backward(st["dy"], st["x"], y, saved, bns, relu=True)
        return dict(y=y, saved=saved, dx=dx, dgamma=dgamma, dbeta=dbeta)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up: code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with hip.workspace.scope("test_dense_bn_nhwc_graph"):
        with torch.cuda.graph(graph):
            outs = step()
    try:
        for i in (0, 1, 0):
            load(sets[i])
            graph.replay()
            torch.cuda.synchronize()
            for k, v in outs.items():
                assert _same_bits(v, eager[i][k]), (i, k)
            assert _same_bits(torch.cat([bn.running_mean for bn in bns]), eager[i]["rm"])
            assert _same_bits(torch.cat([bn.running_var for bn in bns]), eager[i]["rv"])
            assert [int(bn.num_batches_tracked) for bn in bns] == [1, 1]
        assert outs["y"].dtype == BF and not torch.equal(eager[0]["y"], eager[1]["y"])
    finally:
        del graph
        hip.workspace.release("test_dense_bn_nhwc_graph")


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def _map(t, B, H, W):
    """the rows of a problem as an NCHW-shaped view of contiguous NHWC memory"""
    return t.view(B, H, W, t.shape[1]).permute(0, 3, 1, 2)


def test_forward_and_backward_do_not_synchronise(hip):
    from futuredet_amd import dense_bn

    t = _device_inputs(31, 2 * 9 * 20, 96, 0.0)
    bns = _modules(t, [32, 64])
    x, dy = _map(t["x"], 2, 9, 20).requires_grad_(True), _map(t["dy"], 2, 9, 20)

    def step():
        x.grad = None
        for bn in bns:
            bn.weight.grad = bn.bias.grad = None
        y = dense_bn.batch_norm2d_act_nhwc(x, bns)
        y.backward(dy)
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
    assert x.grad is not None and all(bn.weight.grad is not None and bool(torch.isfinite(bn.weight.grad).all()) for bn in bns)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_autograd_surface(hip):
    from futuredet_amd import dense_bn

    B, H, W, sizes = 2, 9, 20, [32, 64]
    n, C = B * H * W, sum(sizes)
    t = _device_inputs(41, n, C, 0.0)
    r = {k: (v.float() if v.dtype == BF else v).cpu().numpy() for k, v in t.items()}
    bns = _modules(t, sizes)
    bufs = [b for bn in bns for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    versions = [b._version for b in bufs]
    x = _map(t["x"], B, H, W).requires_grad_(True)
    y = dense_bn.batch_norm2d_act_nhwc(x, bns)
    assert [b._version for b in bufs] == [v + 1 for v in versions] and [int(bn.num_batches_tracked) for bn in bns] == [1, 1]
    assert y.dtype == BF and tuple(y.shape) == (B, C, H, W) and y.permute(0, 2, 3, 1).is_contiguous()
    y.backward(_map(t["dy"], B, H, W))
    torch.cuda.synchronize()
    assert x.grad.dtype == BF and tuple(x.grad.shape) == (B, C, H, W)
    twin = _modules(t, sizes)
    y2, saved = hip.dense_bn_nhwc_train_forward(t["x"], twin, relu=True)
    dx, dgamma, dbeta = hip.dense_bn_nhwc_train_backward(t["dy"], t["x"], y2, saved, twin, relu=True)
    assert dx.dtype == BF and dgamma.dtype == dbeta.dtype == torch.float32 and tuple(dgamma.shape) == tuple(dbeta.shape) == (C,)
    assert _same_bits(y.detach().permute(0, 2, 3, 1).reshape(n, C), y2) and _same_bits(x.grad.permute(0, 2, 3, 1).reshape(n, C), dx)
    yk, o = y2.float().cpu().numpy(), 0
    for j, (bn, c) in enumerate(zip(bns, sizes)):  # every module's own gradients, against float64
        s = slice(o, o + c)
        assert bn.weight.grad.dtype == bn.bias.grad.dtype == torch.float32 and tuple(bn.weight.grad.shape) == (c,)
        assert _same_bits(bn.weight.grad, dgamma[s]) and _same_bits(bn.bias.grad, dbeta[s])
        _, _, mean, var, invstd = _ref_forward(r["x"][:, s], r["gamma"][s], r["beta"][s], None, True)
        _, dg, db, _ = _ref_backward(r["dy"][:, s], r["x"][:, s], yk[:, s], r["gamma"][s], mean, invstd, True)
        _gate("nhwc autograd module %d weight.grad" % j, bn.weight.grad.cpu().numpy(), dg, 1e-5)
        _gate("nhwc autograd module %d bias.grad" % j, bn.bias.grad.cpu().numpy(), db, 1e-5)
        o += c
    # one module, relu=False, and a gradient that is neither bf16 nor channels-last (an expanded scalar)
    one = _modules(t, [C])[0]
    x3 = _map(t["x"], B, H, W).requires_grad_(True)
    y3 = dense_bn.batch_norm2d_act_nhwc(x3, one, relu=False)
    assert bool((y3 < 0).any())
    y3.float().sum().backward()
    assert x3.grad.dtype == BF and bool(torch.isfinite(x3.grad.float()).all()) and one.weight.grad is not None
    # the wrappers refuse what the predicate refuses
    xd = x.detach()
    frozen = _modules(t, [C])[0].eval()
    for bad, mods in ((xd.float(), one), (xd.contiguous(), one), (xd.cpu(), one), (xd, frozen), (xd, bns[:1]), (xd, [bns[0], frozen]),
                      (xd[:, :48], nn.BatchNorm2d(48).to(DEV).train()), (xd[:1, :, :1, :1], one)):
        if isinstance(mods, nn.Module):
            assert not dense_bn.batch_norm2d_nhwc_fusable(bad, mods)
        with pytest.raises(hip.FutureDetHipError, match="batch_norm2d_act_nhwc"):
            dense_bn.batch_norm2d_act_nhwc(bad, mods)
    with torch.no_grad():
        assert not dense_bn.batch_norm2d_nhwc_fusable(xd, one)
        with pytest.raises(hip.FutureDetHipError, match="batch_norm2d_act_nhwc"):
            dense_bn.batch_norm2d_act_nhwc(xd, one)
    for bad in (t["x"].float(), t["x"][:, ::2], t["x"][:, :48].contiguous()):
        with pytest.raises(hip.FutureDetHipError):
            hip.dense_bn_nhwc_train_forward(bad, one)
    with pytest.raises(hip.FutureDetHipError):
        hip.dense_bn_nhwc_train_forward(t["x"][:1].contiguous(), one)
    assert int(frozen.num_batches_tracked) == 0


# 8, 9 ------------------------------------------------------------------------------------------------------------------------------
def _record_calls(monkeypatch, seen):
    """every dense_bn.batch_norm2d_act_nhwc call with its input, modules, output, incoming gradient and input gradient"""
    from futuredet_amd import dense_bn

    orig = dense_bn.batch_norm2d_act_nhwc

    def recording(x, bns, relu=True):
        if not x.requires_grad:
            x.requires_grad_(True)
        y = orig(x, bns, relu)
        mods = [bns] if isinstance(bns, nn.Module) else list(bns)
        rec = dict(x=x.detach(), bns=mods, relu=relu, y=y.detach(), gamma=[bn.weight.detach().clone() for bn in mods],
                   beta=[bn.bias.detach().clone() for bn in mods])
        y.register_hook(lambda g, rec=rec: rec.__setitem__("dy", g.detach().clone()))
        x.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.detach().clone()))
        seen.append(rec)
        return y

    monkeypatch.setattr(dense_bn, "batch_norm2d_act_nhwc", recording)
    return orig


def _rows(v):
    """an NCHW-shaped map as float64 rows [B H W, C] on the host"""
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1]).double().cpu().numpy()


def _check_recorded_call(tag, rec, gate=1e-4):
    """one recorded call against its own float64 restatement: y and dx with the rounding allowance, every module's parameter gradients"""
    assert rec["x"].dtype == BF and rec["y"].dtype == BF and rec["dy"].dtype == BF and rec["dx"].dtype == BF, tag
    x, yk, dy, dxk = (_rows(rec[k]) for k in ("x", "y", "dy", "dx"))
    o = 0
    for j, bn in enumerate(rec["bns"]):
        c = bn.num_features
        s = slice(o, o + c)
        gamma, beta = rec["gamma"][j].cpu().numpy(), rec["beta"][j].cpu().numpy()
        y, _, mean, var, invstd = _ref_forward(x[:, s], gamma, beta, None, rec["relu"], bn.eps)
        _gate_rounded("%s module %d y" % (tag, j), yk[:, s], y, gate)
        dx, dgamma, dbeta, _ = _ref_backward(dy[:, s], x[:, s], yk[:, s], gamma, mean, invstd, rec["relu"])
        _gate_rounded("%s module %d dx" % (tag, j), dxk[:, s], dx, gate)
        _gate("nhwc %s module %d weight.grad" % (tag, j), bn.weight.grad.cpu().numpy(), dgamma, gate)
        _gate("nhwc %s module %d bias.grad" % (tag, j), bn.bias.grad.cpu().numpy(), dbeta, gate)
        o += c
    assert o == rec["x"].shape[1], tag


def _no_module_forward(monkeypatch, allowed=()):
    entered = []
    orig = nn.BatchNorm2d.forward

    def forward(self, x):
        entered.append(self)
        assert any(self is m for m in allowed), "nn.BatchNorm2d.forward must not be entered with fused_bn"
        return orig(self, x)

    monkeypatch.setattr(nn.BatchNorm2d, "forward", forward)
    return entered


def test_neck(hip, monkeypatch):
    """RPN.train_dtype = bfloat16 with fused_bn: every BatchNorm2d of the neck is one batch_norm2d_act_nhwc call, checked call by call
    against float64 (1e-4 of the largest value, as inside the backbone in test_gpu_sparse_bn.py); the module's forward is never entered"""
    from test_gpu_dense_conv_train_bf16 import _bev, _bf16_values, _small_rpn

    neck = _small_rpn()
    want_shape = tuple(copy.deepcopy(neck).forward_modules(_bev()).shape)
    stats = {k: b.clone() for k, b in neck.named_buffers()}
    neck.train_dtype, neck.fused_bn = BF, True
    n_bn = sum(isinstance(m, nn.BatchNorm2d) for m in neck.modules())
    seen = []
    _record_calls(monkeypatch, seen)
    entered = _no_module_forward(monkeypatch)
    x = _bev().requires_grad_(True)
    out = neck(x)
    out.backward(_bf16_values(np.random.default_rng(4), tuple(out.shape)).to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == want_shape
    assert n_bn == 6 and len(seen) == n_bn and not entered and all(r["relu"] and len(r["bns"]) == 1 for r in seen)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for name, p in neck.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    for k, b in neck.named_buffers():
        assert not torch.equal(b, stats[k]), "BatchNorm buffer %s did not move" % k
    for i, r in enumerate(seen):
        _check_recorded_call("neck call %d %s" % (i, tuple(r["x"].shape)), r)


def test_neck_switch_off_and_frozen_module(hip, monkeypatch):
    from futuredet_amd import dense_bn
    from test_gpu_dense_conv_train_bf16 import _bev, _small_rpn

    def refuse(*a, **kw):
        raise AssertionError("fused_bn = False must not reach batch_norm2d_act_nhwc")

    neck = _small_rpn()
    neck.train_dtype = BF
    assert neck.fused_bn is False
    monkeypatch.setattr(dense_bn, "batch_norm2d_act_nhwc", refuse)
    off = neck(_bev())
    monkeypatch.undo()
    # one module frozen: that layer stays on the module, the others are fused
    neck = _small_rpn()
    neck.train_dtype, neck.fused_bn = BF, True
    frozen = [m for m in neck.modules() if isinstance(m, nn.BatchNorm2d)][1].eval()
    seen = []
    _record_calls(monkeypatch, seen)
    entered = _no_module_forward(monkeypatch, allowed=[frozen])
    out = neck(_bev())
    out.sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(seen) == 5 and len(entered) == 1 and entered[0] is frozen and int(frozen.num_batches_tracked) == 0
    assert all(frozen is not bn for r in seen for bn in r["bns"])
    assert tuple(out.shape) == tuple(off.shape) and bool(torch.isfinite(out).all())


def _small_head():
    from futuredet_amd.heads import CenterHead

    torch.manual_seed(0)
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    head = CenterHead(in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
                      common_heads=common, share_conv_channel=64, classify=False, timesteps=1)
    return head.to(DEV).train()


def test_head(hip, monkeypatch):
    """CenterHead.train_dtype = bfloat16 with fused_bn: shared_conv's BatchNorm2d is one call, the six branch modules ONE grouped call on
    the 384-channel map, and head_tail_bf16 reads six slices of that one tensor"""
    from futuredet_amd import dense_train
    from test_gpu_dense_conv_train_bf16 import _bf16_values

    head = _small_head()
    xin = _bf16_values(np.random.default_rng(3), (2, 64, 16, 24)).to(DEV)
    ref = copy.deepcopy(head)
    ref.train_dtype = BF
    want = ref(xin)  # the un-fused mixed-precision path: keys and shapes
    stats = {k: b.clone() for k, b in head.named_buffers()}
    head.train_dtype, head.fused_bn = BF, True
    seen, tails = [], []
    _record_calls(monkeypatch, seen)
    entered = _no_module_forward(monkeypatch)
    orig_tail = dense_train.head_tail_bf16
    monkeypatch.setattr(dense_train, "head_tail_bf16", lambda groups: (tails.append(list(groups)), orig_tail(groups))[1])
    x = xin.clone().requires_grad_(True)
    got = head(x)
    outs = [d[k] for d in got for k in d]
    rng = np.random.default_rng(4)
    torch.autograd.backward(outs, [_bf16_values(rng, tuple(o.shape)).to(DEV) for o in outs])
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(got) == len(want) == 1 and list(got[0]) == list(want[0])
    for k in got[0]:
        assert got[0][k].dtype == torch.float32 and got[0][k].is_contiguous() and tuple(got[0][k].shape) == tuple(want[0][k].shape), k
    assert not entered and len(seen) == 2, [tuple(r["x"].shape) for r in seen]
    assert len(seen[0]["bns"]) == 1 and tuple(seen[0]["x"].shape) == (2, 64, 16, 24)
    names = list(head.tasks[0].heads)
    assert len(names) == 6 and tuple(seen[1]["x"].shape) == (2, 384, 16, 24) and seen[1]["relu"]
    assert all(a is b for a, b in zip(seen[1]["bns"], [getattr(head.tasks[0], h)[1] for h in names])) and len(seen[1]["bns"]) == 6
    assert len(tails) == 1 and len(tails[0]) == 6 and all(g[0] is tails[0][0][0] for g in tails[0])
    assert [g[3] for g in tails[0]] == [64 * j for j in range(6)] and tuple(tails[0][0][0].shape) == (2, 16, 24, 384)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    for name, p in head.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    for k, b in head.named_buffers():
        assert not torch.equal(b, stats[k]), "BatchNorm buffer %s did not move" % k
    for i, r in enumerate(seen):
        _check_recorded_call("head call %d %s" % (i, tuple(r["x"].shape)), r)


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_one_training_step_with_every_switch_on(hip, monkeypatch):
    """forecast_n0 with backbone, neck and head in bf16 and all three fused_bn through solver.train_steps: a finite loss, every neck and
    head parameter finite and moved, same state-dict keys, and as many fused dense BatchNorm calls as the modules say"""
    from futuredet_amd import build_detector, dense_bn, solver
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
    net.bbox_head.fused_bn = net.neck.fused_bn = net.backbone.fused_bn = True
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    dense = {k: p for part in (net.neck, net.bbox_head) for k, p in part.named_parameters(prefix=type(part).__name__)}
    before = {k: p.detach().clone() for k, p in dense.items()}
    # the count from the modules: every BatchNorm2d of the neck and of shared_conv is a call, the branches of a task are one call together
    want_calls = (sum(isinstance(m, nn.BatchNorm2d) for m in net.neck.modules())
                  + sum(isinstance(m, nn.BatchNorm2d) for m in net.bbox_head.shared_conv.modules()) + len(net.bbox_head.tasks))
    n_modules = sum(isinstance(m, nn.BatchNorm2d) for part in (net.neck, net.bbox_head) for m in part.modules())
    calls = []
    orig = dense_bn.batch_norm2d_act_nhwc
    monkeypatch.setattr(dense_bn, "batch_norm2d_act_nhwc",
                        lambda x, bns, relu=True: (calls.append(1 if isinstance(bns, nn.Module) else len(bns)), orig(x, bns, relu))[1])
    entered = _no_module_forward(monkeypatch)
    try:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        out = next(solver.train_steps(net, [ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2)))
    finally:
        monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(np.isfinite(float(l.detach())) for l in out["loss"])
    assert len(calls) == want_calls and sum(calls) == n_modules and not entered, (calls, want_calls, n_modules)
    for k, p in dense.items():
        assert bool(torch.isfinite(p).all()), k
        assert not torch.equal(p.detach(), before[k]), "parameter %s did not move" % k
    assert list(net.state_dict()) == keys
