"""The host side of the fused sparse BatchNorm (csrc/fd_sparse_bn.hip): exported symbols, the chunk size, workspace sizes, the argument
checks of both entry points (no device needed: they validate before any device work) and the ``fused_bn`` switch on CPU tensors.
CPU only."""
import copy
import ctypes
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

NAMES = {"fd_sparse_bn_chunk", "fd_sparse_bn_workspace_bytes", "fd_sparse_bn_train_forward", "fd_sparse_bn_train_backward"}


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
    assert "fd_sparse_bn.hip" in build.SOURCES and build.EXTRA["fd_sparse_bn.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    chunk = int(re.search(r"#define FD_SPARSE_BN_CHUNK (\d+)", hdr).group(1))
    assert L.fd_sparse_bn_chunk() == chunk == hip_ops.sparse_bn_chunk() and chunk > 0 and chunk % 64 == 0


def test_workspace_bytes(L):
    P = L.fd_sparse_bn_chunk()
    for C in (16, 32, 48, 64, 128):
        sizes = [L.fd_sparse_bn_workspace_bytes(n, C) for n in (1, 2, 63, P - 1, P, P + 1, 3 * P + 17, 160000, 1 << 30)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (C, sizes)
        assert all(s % 16 == 0 for s in sizes)
    assert L.fd_sparse_bn_workspace_bytes(160000, 128) > L.fd_sparse_bn_workspace_bytes(160000, 16)
    for C in (0, -16, 8, 15, 17, 24, 100, 144, 256):
        assert L.fd_sparse_bn_workspace_bytes(1000, C) == 0, C
        assert not hip_ops.sparse_bn_channels_ok(C)
    for n in (0, -1, (1 << 30) + 1):
        assert L.fd_sparse_bn_workspace_bytes(n, 16) == 0, n
    assert all(hip_ops.sparse_bn_channels_ok(C) for C in range(16, 129, 16))


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    odd = ctypes.c_void_p(0x10004)
    big = 1 << 40

    def fwd(**kw):
        a = dict(x=p, residual=None, gamma=p, beta=p, n=1000, n_dev=None, C=16, relu=1, eps=1e-3, momentum=0.01, y=p, saved=p, rm=p, rv=p,
                 nbt=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_sparse_bn_train_forward(a["x"], a["residual"], a["gamma"], a["beta"], a["n"], a["n_dev"], a["C"], a["relu"], a["eps"],
                                            a["momentum"], a["y"], a["saved"], a["rm"], a["rv"], a["nbt"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(dy=p, x=p, y=p, gamma=p, saved=p, n=1000, n_dev=None, C=16, relu=1, dx=p, dres=None, dgamma=p, dbeta=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_sparse_bn_train_backward(a["dy"], a["x"], a["y"], a["gamma"], a["saved"], a["n"], a["n_dev"], a["C"], a["relu"], a["dx"],
                                             a["dres"], a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for k in ("x", "gamma", "beta"):
        bad(fwd, "fd_sparse_bn_train_forward: null x, gamma or beta", **{k: None})
    for k in ("y", "saved"):
        bad(fwd, "null y or saved", **{k: None})
    for k in ("rm", "rv", "nbt"):
        bad(fwd, "null running statistics", **{k: None})
    for k in ("dy", "x", "gamma", "saved"):
        bad(bwd, "fd_sparse_bn_train_backward: null dy, x, gamma or saved", **{k: None})
    bad(bwd, "null y (the ReLU mask)", y=None)
    for k in ("dx", "dgamma", "dbeta"):
        bad(bwd, "null dx, dgamma or dbeta", **{k: None})
    need = L.fd_sparse_bn_workspace_bytes(1000, 16)
    for fn in (fwd, bwd):
        for C in (0, 8, 24, 144):
            bad(fn, "unsupported C %d" % C, C=C)
        bad(fn, "n out of range", n=0)
        bad(fn, "n out of range", n=(1 << 30) + 1)
        bad(fn, "expected more than 1 value per channel", n=1)
        bad(fn, "relu must be 0 or 1", relu=2)
        bad(fn, "null workspace", ws=None)
        bad(fn, "workspace too small", ws_bytes=need - 1)
        bad(fn, "workspace must be 16-byte aligned", ws=odd)
    bad(fwd, "eps must be > 0", eps=0.0)
    bad(fwd, "momentum must be in [0, 1]", momentum=1.5)
    bad(fwd, "16-byte aligned", x=odd)
    bad(fwd, "16-byte aligned", residual=odd)
    bad(bwd, "16-byte aligned", dy=odd)
    bad(bwd, "16-byte aligned", dres=odd)


def test_front_end_refuses_cpu_tensors():
    bn = nn.BatchNorm1d(16).train()
    x = torch.randn(8, 16)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.sparse_bn_train_forward(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
    from futuredet_amd import sparse as spconv

    assert not spconv.batch_norm_fusable(x, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="batch_norm_act"):
        spconv.batch_norm_act(x, bn)


def test_fused_bn_defaults_to_false_and_is_no_constructor_state():
    from futuredet_amd.backbones import SpMiddleResNetFHD

    bb = SpMiddleResNetFHD(num_input_features=5)
    assert bb.fused_bn is False
    keys = list(bb.state_dict())
    bb.fused_bn = True
    assert list(bb.state_dict()) == keys and not any("fused" in k for k in keys)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_switch_on_keeps_the_module_path_on_the_cpu(dtype):
    """The convolutions have no CPU path, so the switch is exercised where it acts: the backbone's normalisation step on CPU features
    gives exactly what the modules give (values, running statistics, gradients)."""
    from futuredet_amd.backbones import SpMiddleResNetFHD

    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5).to(dtype).train()
    bb.fused_bn = True
    for bn, relu, C, with_res in ((bb.conv_input[1], bb.conv_input[2], 16, False), (bb.conv3[3].bn1, bb.conv3[3].relu, 64, False),
                                  (bb.conv4[4].bn2, bb.conv4[4].relu, 128, True), (bb.extra_conv[1], bb.extra_conv[2], 128, False)):
        ref_bn = copy.deepcopy(bn)
        x = torch.randn(37, C, dtype=dtype)
        res = torch.randn(37, C, dtype=dtype) if with_res else None
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        got = bb._bn_act(xa, bn, relu, res)
        want = ref_bn(xb)
        if with_res:
            want = want + res
        want = torch.relu(want)
        assert torch.equal(got, want)
        assert torch.equal(bn.running_mean, ref_bn.running_mean) and torch.equal(bn.running_var, ref_bn.running_var)
        assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
        g = torch.randn_like(x)
        got.backward(g)
        want.backward(g)
        assert torch.equal(xa.grad, xb.grad) and torch.equal(bn.weight.grad, ref_bn.weight.grad) and torch.equal(bn.bias.grad, ref_bn.bias.grad)
    # one row: torch's own error stays
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bb._bn_act(torch.randn(1, 16, dtype=dtype), bb.conv_input[1], bb.conv_input[2])
