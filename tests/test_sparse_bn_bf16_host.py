"""The host side of the bf16-row form of the fused sparse BatchNorm (csrc/fd_sparse_bn.hip): the two added entry points in the header, in
lib.SIGNATURES and in the library; their argument checks (no device needed: they validate before any device work), which carry the fp32
functions' message texts under the new names; and the ``fused_bn`` switch on CPU bf16 features, where the mixed-precision module chain
stays what it was.  CPU only."""
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

NAMES = {"fd_sparse_bn_train_forward_bf16", "fd_sparse_bn_train_backward_bf16"}
BF = torch.bfloat16


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def test_symbols_header_and_abi_version(L):
    assert NAMES <= set(lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert getattr(L, name) is not None
        assert lib.SIGNATURES[name] == lib.SIGNATURES[name[:-len("_bf16")]]  # the fp32 argument list, pointer for pointer
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    # one workspace size serves both row types: there is no second size function
    assert not any("workspace_bytes_bf16" in n for n in lib.SIGNATURES)


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    odd = ctypes.c_void_p(0x10004)
    half = ctypes.c_void_p(0x10008)  # 8-byte aligned: enough for one bf16 quad, not for the contract
    big = 1 << 40

    def fwd(**kw):
        a = dict(x=p, residual=None, gamma=p, beta=p, n=1000, n_dev=None, C=16, relu=1, eps=1e-3, momentum=0.01, y=p, saved=p, rm=p, rv=p,
                 nbt=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_sparse_bn_train_forward_bf16(a["x"], a["residual"], a["gamma"], a["beta"], a["n"], a["n_dev"], a["C"], a["relu"], a["eps"],
                                                 a["momentum"], a["y"], a["saved"], a["rm"], a["rv"], a["nbt"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(dy=p, x=p, y=p, gamma=p, saved=p, n=1000, n_dev=None, C=16, relu=1, dx=p, dres=None, dgamma=p, dbeta=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_sparse_bn_train_backward_bf16(a["dy"], a["x"], a["y"], a["gamma"], a["saved"], a["n"], a["n_dev"], a["C"], a["relu"], a["dx"],
                                                  a["dres"], a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for k in ("x", "gamma", "beta"):
        bad(fwd, "fd_sparse_bn_train_forward_bf16: null x, gamma or beta", **{k: None})
    for k in ("y", "saved"):
        bad(fwd, "fd_sparse_bn_train_forward_bf16: null y or saved", **{k: None})
    for k in ("rm", "rv", "nbt"):
        bad(fwd, "fd_sparse_bn_train_forward_bf16: null running statistics", **{k: None})
    for k in ("dy", "x", "gamma", "saved"):
        bad(bwd, "fd_sparse_bn_train_backward_bf16: null dy, x, gamma or saved", **{k: None})
    bad(bwd, "fd_sparse_bn_train_backward_bf16: null y (the ReLU mask)", y=None)
    for k in ("dx", "dgamma", "dbeta"):
        bad(bwd, "fd_sparse_bn_train_backward_bf16: null dx, dgamma or dbeta", **{k: None})
    need = L.fd_sparse_bn_workspace_bytes(1000, 16)
    for fn, name in ((fwd, "fd_sparse_bn_train_forward_bf16"), (bwd, "fd_sparse_bn_train_backward_bf16")):
        for C in (0, 8, 24, 144):
            bad(fn, name + ": unsupported C %d: a multiple of 16 in [16, 128]" % C, C=C)
        bad(fn, name + ": n out of range (0)", n=0)
        bad(fn, name + ": n out of range", n=(1 << 30) + 1)
        bad(fn, name + ": expected more than 1 value per channel (n = 1)", n=1)
        bad(fn, name + ": relu must be 0 or 1 (got 2)", relu=2)
        bad(fn, name + ": null workspace", ws=None)
        bad(fn, name + ": workspace too small (%d bytes, %d needed)" % (need - 1, need), ws_bytes=need - 1)
        bad(fn, name + ": the workspace must be 16-byte aligned", ws=odd)
    bad(fwd, "fd_sparse_bn_train_forward_bf16: eps must be > 0", eps=0.0)
    bad(fwd, "fd_sparse_bn_train_forward_bf16: momentum must be in [0, 1]", momentum=1.5)
    for ptr in (odd, half):  # 16 bytes are demanded of bf16 rows too
        bad(fwd, "fd_sparse_bn_train_forward_bf16: x, residual, y and saved must be 16-byte aligned", x=ptr)
        bad(fwd, "fd_sparse_bn_train_forward_bf16: x, residual, y and saved must be 16-byte aligned", residual=ptr)
        bad(bwd, "fd_sparse_bn_train_backward_bf16: dy, x, y, saved, dx and d_residual must be 16-byte aligned", dy=ptr)
        bad(bwd, "fd_sparse_bn_train_backward_bf16: dy, x, y, saved, dx and d_residual must be 16-byte aligned", dres=ptr)
    # y may be null without the ReLU: the next check is reached
    bad(bwd, "null workspace", y=None, relu=0, ws=None)


def test_front_end_refuses_cpu_bf16_tensors():
    from futuredet_amd import sparse as spconv

    bn = nn.BatchNorm1d(16).train()
    x = torch.randn(8, 16).to(BF)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.sparse_bn_train_forward(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.sparse_bn_train_backward(x, x, x, bn.weight, torch.zeros(2, 16))
    assert not spconv.batch_norm_fusable(x, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="batch_norm_act.*fp32 or bf16 device features"):
        spconv.batch_norm_act(x, bn)


@pytest.mark.parametrize("fused_bn", [False, True])
def test_cpu_bf16_features_keep_the_mixed_precision_module_chain(fused_bn):
    """_bn_act on CPU bf16 features, whatever the switch says: relu_to_bf16(bn(x.float()) [+ res.float()]) in values, running statistics
    and gradients"""
    from futuredet_amd import sparse as spconv
    from futuredet_amd.backbones import SpMiddleResNetFHD

    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5).train()
    bb.fused_bn = fused_bn
    bb.train_dtype = BF
    for bn, relu, C, with_res in ((bb.conv_input[1], bb.conv_input[2], 16, False), (bb.conv3[3].bn1, bb.conv3[3].relu, 64, False),
                                  (bb.conv4[4].bn2, bb.conv4[4].relu, 128, True), (bb.extra_conv[1], bb.extra_conv[2], 128, False)):
        ref_bn = copy.deepcopy(bn)
        x = torch.randn(37, C).to(BF)
        res = torch.randn(37, C).to(BF) if with_res else None
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ra = rb = None
        if with_res:
            ra, rb = res.clone().requires_grad_(True), res.clone().requires_grad_(True)
        got = bb._bn_act(xa, bn, relu, ra)
        want = ref_bn(xb.float())
        if with_res:
            want = want + rb.float()
        want = spconv.relu_to_bf16(want)
        assert got.dtype == BF and torch.equal(got, want)
        assert torch.equal(bn.running_mean, ref_bn.running_mean) and torch.equal(bn.running_var, ref_bn.running_var)
        assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
        g = torch.randn(37, C).to(BF)
        got.backward(g)
        want.backward(g)
        assert xa.grad.dtype == BF and torch.equal(xa.grad, xb.grad)
        assert torch.equal(bn.weight.grad, ref_bn.weight.grad) and torch.equal(bn.bias.grad, ref_bn.bias.grad)
        if with_res:
            assert torch.equal(ra.grad, rb.grad)
