"""The host side of the fused dense BatchNorm (csrc/fd_dense_bn.hip): exported symbols, the chunk size, workspace sizes, the argument
checks of both entry points (no device needed: they validate before any device work), the predicate of dense_bn.batch_norm2d_fusable
and the ``fused_bn`` switches of RPN and CenterHead on CPU tensors.  CPU only."""
import copy
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from futuredet_amd import build, hip_ops, lib  # noqa: E402

NAMES = {"fd_dense_bn_chunk", "fd_dense_bn_workspace_bytes", "fd_dense_bn_train_forward", "fd_dense_bn_train_backward"}
HEADS = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}


def small_rpn():
    from futuredet_amd.necks import RPN

    return RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[16, 32], us_layer_strides=[1, 2], us_num_filters=[16, 16],
               num_input_features=16)


def small_head(**kw):
    """the forecast_n0 form of the CenterHead on 32 input channels"""
    from futuredet_amd.heads import CenterHead

    return CenterHead(in_channels=32, tasks=[dict(num_class=1, class_names=["car"])], common_heads=dict(HEADS), share_conv_channel=64,
                      timesteps=1, dense=False, bev_map=False, forecast_feature=False, classify=False, wide_head=False, **kw)


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def test_symbols_header_build_flags_and_chunk(L):
    assert NAMES <= set(lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert getattr(L, name) is not None
    assert "fd_dense_bn.hip" in build.SOURCES and build.EXTRA["fd_dense_bn.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    chunk = int(re.search(r"#define FD_DENSE_BN_CHUNK (\d+)", hdr).group(1))
    assert L.fd_dense_bn_chunk() == chunk == hip_ops.dense_bn_chunk() and chunk > 0 and chunk % 256 == 0


def test_workspace_bytes(L):
    K = L.fd_dense_bn_chunk()
    for C in (1, 3, 16, 64, 130, 256, 4096):
        by_p = [L.fd_dense_bn_workspace_bytes(2, C, P) for P in (1, 2, 63, K - 1, K, K + 1, 3 * K + 17, 180 * 180, 1 << 20, 1 << 30)]
        assert by_p[0] > 0 and all(a <= b for a, b in zip(by_p, by_p[1:])), (C, by_p)
        by_b = [L.fd_dense_bn_workspace_bytes(B, C, K + 1) for B in (1, 2, 3, 4, 7, 8, 64, 1000)]
        assert by_b[0] > 0 and all(a <= b for a, b in zip(by_b, by_b[1:])), (C, by_b)
        assert all(s % 16 == 0 for s in by_p + by_b)
    assert L.fd_dense_bn_workspace_bytes(1000, 1, 5 * K) > L.fd_dense_bn_workspace_bytes(1, 1, K)
    for C in (0, -1, 4097, 1 << 20):
        assert L.fd_dense_bn_workspace_bytes(4, C, 1000) == 0, C
    for B in (0, -1, (1 << 16) + 1):
        assert L.fd_dense_bn_workspace_bytes(B, 16, 1000) == 0, B
    for P in (0, -1, (1 << 30) + 1):
        assert L.fd_dense_bn_workspace_bytes(4, 16, P) == 0, P
    assert L.fd_dense_bn_workspace_bytes(1, 16, 1) == 0  # one value per channel
    assert L.fd_dense_bn_workspace_bytes(1 << 16, 4096, 16) == 0  # B C beyond the plane limit
    assert L.fd_dense_bn_workspace_bytes(2, 16, 1) > 0 and L.fd_dense_bn_workspace_bytes(1, 16, 2) > 0


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    odd = ctypes.c_void_p(0x10004)
    big = 1 << 40

    def fwd(**kw):
        a = dict(x=p, gamma=p, beta=p, B=2, C=16, P=1000, relu=1, eps=1e-3, momentum=0.01, y=p, saved=p, rm=p, rv=p, nbt=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_dense_bn_train_forward(a["x"], a["gamma"], a["beta"], a["B"], a["C"], a["P"], a["relu"], a["eps"], a["momentum"], a["y"],
                                           a["saved"], a["rm"], a["rv"], a["nbt"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(dy=p, x=p, y=p, gamma=p, saved=p, B=2, C=16, P=1000, relu=1, dx=p, dgamma=p, dbeta=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_dense_bn_train_backward(a["dy"], a["x"], a["y"], a["gamma"], a["saved"], a["B"], a["C"], a["P"], a["relu"], a["dx"],
                                            a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for k in ("x", "gamma", "beta"):
        bad(fwd, "fd_dense_bn_train_forward: null x, gamma or beta", **{k: None})
    for k in ("y", "saved"):
        bad(fwd, "fd_dense_bn_train_forward: null y or saved", **{k: None})
    for k in ("rm", "rv", "nbt"):
        bad(fwd, "fd_dense_bn_train_forward: null running statistics", **{k: None})
    for k in ("dy", "x", "gamma", "saved"):
        bad(bwd, "fd_dense_bn_train_backward: null dy, x, gamma or saved", **{k: None})
    bad(bwd, "fd_dense_bn_train_backward: null y (the ReLU mask)", y=None)
    for k in ("dx", "dgamma", "dbeta"):
        bad(bwd, "fd_dense_bn_train_backward: null dx, dgamma or dbeta", **{k: None})
    need = L.fd_dense_bn_workspace_bytes(2, 16, 1000)
    assert need > 0
    for fn, name in ((fwd, "fd_dense_bn_train_forward"), (bwd, "fd_dense_bn_train_backward")):
        for C in (0, -3, 4097):
            bad(fn, name + ": unsupported C %d" % C, C=C)
        for kw in (dict(B=0), dict(B=(1 << 16) + 1), dict(P=0), dict(P=(1 << 30) + 1), dict(B=1 << 16, C=4096)):
            bad(fn, name + ": B or P out of range", **kw)
        bad(fn, name + ": expected more than 1 value per channel", B=1, P=1)
        bad(fn, name + ": relu must be 0 or 1", relu=2)
        bad(fn, name + ": relu must be 0 or 1", relu=-1)
        bad(fn, name + ": null workspace", ws=None)
        bad(fn, name + ": workspace too small", ws_bytes=need - 1)
        bad(fn, name + ": the workspace must be 16-byte aligned", ws=odd)
    bad(fwd, "fd_dense_bn_train_forward: eps must be > 0", eps=0.0)
    bad(fwd, "fd_dense_bn_train_forward: eps must be > 0", eps=-1.0)
    bad(fwd, "fd_dense_bn_train_forward: momentum must be in [0, 1]", momentum=1.5)
    bad(fwd, "fd_dense_bn_train_forward: momentum must be in [0, 1]", momentum=-0.1)
    bad(fwd, "fd_dense_bn_train_forward: x and y must be 16-byte aligned", x=odd)
    bad(fwd, "fd_dense_bn_train_forward: x and y must be 16-byte aligned", y=odd)
    for k in ("dy", "x", "y", "dx"):
        bad(bwd, "fd_dense_bn_train_backward: dy, x, y and dx must be 16-byte aligned", **{k: odd})


def test_front_ends_refuse_cpu_tensors():
    from futuredet_amd import dense_bn

    bn = nn.BatchNorm2d(16).train()
    x = torch.randn(2, 16, 5, 5)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.dense_bn_train_forward(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.dense_bn_train_backward(x, x, x, bn.weight, torch.zeros(2, 16))
    assert not dense_bn.batch_norm2d_fusable(x, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="batch_norm2d_act"):
        dense_bn.batch_norm2d_act(x, bn)
    assert int(bn.num_batches_tracked) == 0


class _OnDevice(object):
    """What batch_norm2d_fusable reads of a tensor, with is_cuda forced on: the predicate's other clauses can then be told apart on a
    machine without a device (a CPU tensor fails the device clause whatever else holds)."""

    def __init__(self, t, device):
        self._t, self.is_cuda, self.device = t, True, device
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def is_contiguous(self):
        return self._t.is_contiguous()


def test_fusable_predicate():
    from futuredet_amd import dense_bn

    dev = torch.device("cpu")

    def ok(x, bn):
        return dense_bn.batch_norm2d_fusable(_OnDevice(x, dev), bn)

    x = torch.randn(2, 16, 5, 5)
    assert ok(x, nn.BatchNorm2d(16).train())  # the stand-in passes every clause: each case below fails for its own reason
    assert not ok(x, nn.BatchNorm2d(16).eval())
    assert not ok(x, nn.BatchNorm2d(16, affine=False).train())
    assert not ok(x, nn.BatchNorm2d(16, momentum=None).train())
    assert not ok(x, nn.BatchNorm2d(16, track_running_stats=False).train())
    assert not ok(x.double(), nn.BatchNorm2d(16).double().train())
    assert not ok(x.double(), nn.BatchNorm2d(16).train()) and not ok(x, nn.BatchNorm2d(16).double().train())
    with torch.no_grad():
        assert not ok(x, nn.BatchNorm2d(16).train())
    assert not ok(x.contiguous(memory_format=torch.channels_last), nn.BatchNorm2d(16).train())
    assert not ok(x[:, :, :, ::2], nn.BatchNorm2d(16).train())
    assert not ok(torch.randn(2, 16, 5), nn.BatchNorm2d(16).train()) and not ok(torch.randn(2, 16), nn.BatchNorm1d(16).train())
    assert not ok(torch.randn(1, 16, 1, 1), nn.BatchNorm2d(16).train()) and ok(torch.randn(2, 16, 1, 1), nn.BatchNorm2d(16).train())
    assert not ok(x, nn.BatchNorm2d(8).train())
    assert not dense_bn.batch_norm2d_fusable(x, nn.BatchNorm2d(16).train())  # a host tensor


def test_fused_bn_defaults_to_false_and_is_no_constructor_state():
    from futuredet_amd.heads import CenterHead
    from futuredet_amd.necks import RPN

    for m, cls in ((small_rpn(), RPN), (small_head(), CenterHead)):
        assert m.fused_bn is False
        keys = list(m.state_dict())
        m.fused_bn = True
        assert list(m.state_dict()) == keys and not any("fused" in k for k in keys)
        assert not any("fused" in p for p in inspect.signature(cls.__init__).parameters)


def _train_once(m, x, G, fused):
    m = copy.deepcopy(m).train()
    m.fused_bn = fused
    xin = x.clone().requires_grad_(True)
    out = m(xin)
    maps = [out] if isinstance(out, torch.Tensor) else [d[k] for d in out for k in sorted(d)]
    sum((o * g).sum() for o, g in zip(maps, G)).backward()
    return maps, xin.grad, {k: p.grad for k, p in m.named_parameters()}, {k: v for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("which", ["rpn", "head", "head_n3dtf", "head_dcn"])
def test_switch_on_gives_the_bits_of_switch_off_on_the_cpu(which):
    """host tensors are not fusable: with the switch on, run_stack walks the same modules in the same order"""
    torch.manual_seed(3)
    if which == "rpn":
        m, x = small_rpn(), torch.randn(2, 16, 12, 12)
    elif which == "head":
        m, x = small_head(), torch.randn(2, 32, 12, 12)
    elif which == "head_dcn":
        m, x = small_head(dcn_head=True), torch.randn(2, 32, 6, 6)
    else:
        from futuredet_amd.heads import CenterHead

        m = CenterHead(in_channels=32, tasks=[dict(num_class=1, class_names=["car"])], common_heads=dict(HEADS), share_conv_channel=64,
                       timesteps=2, dense=True, forecast_feature=True, classify=False)
        x = torch.randn(2, 32, 6, 6)
    m.train()
    probe = m(x)
    shapes = [probe.shape] if isinstance(probe, torch.Tensor) else [d[k].shape for d in probe for k in sorted(d)]
    G = [torch.randn(s) for s in shapes]
    m.zero_grad()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.reset_running_stats()
    off, on = _train_once(m, x, G, False), _train_once(m, x, G, True)
    assert len(off[0]) == len(on[0]) and all(torch.equal(a, b) for a, b in zip(off[0], on[0]))
    assert torch.equal(off[1], on[1])
    for part in (2, 3):
        assert set(off[part]) == set(on[part]) and len(off[part]) > 0
        for k in off[part]:
            assert (off[part][k] is None and on[part][k] is None) or torch.equal(off[part][k], on[part][k]), k
    assert all(int(v) == 1 for k, v in on[3].items() if "num_batches" in k)
