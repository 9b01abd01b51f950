"""The host side of the fused BatchNorm2d on bf16 channels-last maps (csrc/fd_dense_bn_nhwc.hip): exported symbols, build flags, the
chunk size, workspace sizes, the ctypes mirror of the group record, the argument checks of both entry points (no device needed: they
validate before any device work), the predicate dense_bn.batch_norm2d_nhwc_fusable, and ``fused_bn`` together with
``train_dtype = torch.bfloat16`` on CPU tensors.  CPU only."""
import copy
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from futuredet_amd import build, hip_ops, lib  # noqa: E402

NAMES = {"fd_dense_bn_nhwc_chunk", "fd_dense_bn_nhwc_stat_groups", "fd_dense_bn_nhwc_apply_blocks", "fd_dense_bn_nhwc_workspace_bytes",
         "fd_dense_bn_nhwc_train_forward_bf16", "fd_dense_bn_nhwc_train_backward_bf16"}
FWD, BWD = "fd_dense_bn_nhwc_train_forward_bf16", "fd_dense_bn_nhwc_train_backward_bf16"
HEADS = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _header():
    return open(os.path.join(REPO, "include", "futuredet_hip.h")).read()


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, _header()).group(1))


def test_symbols_header_build_flags_and_constants(L):
    assert NAMES <= set(lib.SIGNATURES)
    hdr = _header()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert getattr(L, name) is not None
    assert "fd_dense_bn_nhwc.hip" in build.SOURCES
    assert build.EXTRA["fd_dense_bn_nhwc.hip"] == build.EXTRA["fd_dense_bn.hip"] == build.EXTRA["fd_sparse_bn.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    chunk = _define("FD_DENSE_BN_NHWC_CHUNK")
    assert L.fd_dense_bn_nhwc_chunk() == chunk == hip_ops.dense_bn_nhwc_chunk() and chunk > 0 and chunk % 64 == 0
    assert L.fd_dense_bn_nhwc_stat_groups() == _define("FD_DENSE_BN_NHWC_STAT_GROUPS") > 0
    assert L.fd_dense_bn_nhwc_apply_blocks() == _define("FD_DENSE_BN_NHWC_APPLY_BLOCKS") > 0
    assert _define("FD_DENSE_BN_NHWC_MAX_GROUPS") == 8 == hip_ops.dense_bn_nhwc_max_groups()


def test_workspace_bytes(L):
    P = L.fd_dense_bn_nhwc_chunk()
    for C in (32, 64, 96, 128, 160, 256, 384, 448, 512):
        by_n = [L.fd_dense_bn_nhwc_workspace_bytes(n, C) for n in (2, 63, P - 1, P, P + 1, 3 * P + 17, 2 * 180 * 180, 1 << 20, 1 << 30)]
        assert by_n[0] > 0 and all(a <= b for a, b in zip(by_n, by_n[1:])), (C, by_n)
        assert all(s % 16 == 0 for s in by_n)
        # one [mean | M2] pair of fp32 rows per group of chunks
        assert by_n[0] >= 2 * C * 4 and by_n[-1] >= L.fd_dense_bn_nhwc_stat_groups() * 2 * C * 4
    for C in (0, 16, 48, 100, 544, -32):
        assert L.fd_dense_bn_nhwc_workspace_bytes(1000, C) == 0, C
    for n in (0, 1, -1, (1 << 30) + 1):
        assert L.fd_dense_bn_nhwc_workspace_bytes(n, 64) == 0, n


def test_ctypes_record_mirrors_the_header(tmp_path):
    """fd_dense_bn_nhwc_group crosses the C ABI in an array: the mirror holds the header's members in the header's order and gcc gives
    it the same size"""
    bare = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct fd_dense_bn_nhwc_group \{(.*?)\} fd_dense_bn_nhwc_group;", bare, flags=re.S).group(1)
    members = []
    for decl in body.split(";"):
        for part in decl.strip().split(",") if decl.strip() else []:
            members.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1))
    assert members == ["gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "c", "eps", "momentum"]
    assert [n for n, _ in lib.DenseBnNhwcGroup._fields_] == members
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "futuredet_hip.h"\nint main(void) { printf("%zu\\n", sizeof(fd_dense_bn_nhwc_group)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    assert int(subprocess.check_output([exe]).decode()) == ctypes.sizeof(lib.DenseBnNhwcGroup)


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced on the device: every call fails validation before any device work"""
    p, odd, big = 0x10000, 0x10004, 1 << 40

    def records(cs=(64,), **kw):
        a = dict(gamma=p, beta=p, rm=p, rv=p, nbt=p, eps=1e-3, momentum=0.1)
        a.update(kw)
        return (lib.DenseBnNhwcGroup * max(len(cs), 1))(*[lib.DenseBnNhwcGroup(a["gamma"], a["beta"], a["rm"], a["rv"], a["nbt"], c, a["eps"], a["momentum"])
                                                           for c in cs])

    def fwd(**kw):
        a = dict(x=p, groups=records(), n_groups=1, n=1000, C=64, relu=1, y=p, saved=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_dense_bn_nhwc_train_forward_bf16(a["x"], a["groups"], a["n_groups"], a["n"], a["C"], a["relu"], a["y"], a["saved"], a["ws"],
                                                     a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(dy=p, x=p, y=p, saved=p, groups=records(), n_groups=1, n=1000, C=64, relu=1, dx=p, dgamma=p, dbeta=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_dense_bn_nhwc_train_backward_bf16(a["dy"], a["x"], a["y"], a["saved"], a["groups"], a["n_groups"], a["n"], a["C"], a["relu"],
                                                      a["dx"], a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for k in ("x", "y", "saved"):
        bad(fwd, FWD + ": null x, y or saved", **{k: None})
    for k in ("dy", "x", "saved"):
        bad(bwd, BWD + ": null dy, x or saved", **{k: None})
    bad(bwd, BWD + ": null y (the ReLU mask)", y=None)
    for k in ("dx", "dgamma", "dbeta"):
        bad(bwd, BWD + ": null dx, dgamma or dbeta", **{k: None})
    for k in ("gamma", "beta"):
        bad(fwd, FWD + ": group 0: null gamma or beta", groups=records(**{k: None}))
    for k in ("rm", "rv", "nbt"):
        bad(fwd, FWD + ": group 0: null running statistics", groups=records(**{k: None}))
    bad(bwd, BWD + ": group 0: null gamma", groups=records(gamma=None))
    need = L.fd_dense_bn_nhwc_workspace_bytes(1000, 64)
    assert need > 0
    for fn, name in ((fwd, FWD), (bwd, BWD)):
        bad(fn, name + ": null groups", groups=None)
        for ng in (0, -1, 9):
            bad(fn, name + ": n_groups must be in [1, 8]", n_groups=ng)
        for C in (0, 16, 48, 100, 544, -32):
            bad(fn, name + ": unsupported C %d" % C, C=C)
        for c in (0, 16, 48, -32, 1024):
            bad(fn, name + ": group 1: unsupported c %d" % c, C=96, groups=records((32, c)), n_groups=2)
        bad(fn, name + ": the groups' c sum to 96, not to C = 64", groups=records((32, 64)), n_groups=2)
        bad(fn, name + ": the groups' c sum to 32, not to C = 64", groups=records((32,)))
        for n in (0, 1, -5, (1 << 30) + 1):
            bad(fn, name + ": n out of range (%d)" % n, n=n)
        bad(fn, name + ": relu must be 0 or 1", relu=2)
        bad(fn, name + ": relu must be 0 or 1", relu=-1)
        bad(fn, name + ": null workspace", ws=None)
        bad(fn, name + ": workspace too small", ws_bytes=need - 1)
        bad(fn, name + ": the workspace must be 16-byte aligned", ws=odd)
    bad(fwd, FWD + ": group 0: eps must be > 0", groups=records(eps=0.0))
    bad(fwd, FWD + ": group 0: eps must be > 0", groups=records(eps=-1.0))
    bad(fwd, FWD + ": group 0: momentum must be in [0, 1]", groups=records(momentum=1.5))
    bad(fwd, FWD + ": group 0: momentum must be in [0, 1]", groups=records(momentum=-0.1))
    for k in ("x", "y", "saved"):
        bad(fwd, FWD + ": x, y and saved must be 16-byte aligned", **{k: odd})
    for k in ("dy", "x", "y", "saved", "dx"):
        bad(bwd, BWD + ": dy, x, y, saved and dx must be 16-byte aligned", **{k: odd})


def test_front_ends_refuse_cpu_tensors():
    from futuredet_amd import dense_bn

    bn = nn.BatchNorm2d(32).train()
    x = torch.randn(2, 5, 5, 32).to(torch.bfloat16)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.dense_bn_nhwc_train_forward(x, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.dense_bn_nhwc_train_backward(x, x, x, torch.zeros(2, 32), bn)
    view = x.permute(0, 3, 1, 2)
    assert not dense_bn.batch_norm2d_nhwc_fusable(view, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="batch_norm2d_act_nhwc"):
        dense_bn.batch_norm2d_act_nhwc(view, bn)
    with pytest.raises(hip_ops.FutureDetHipError, match="batch_norm2d_act_nhwc"):
        dense_bn.batch_norm2d_act_nhwc(view, [bn])
    assert int(bn.num_batches_tracked) == 0


class _OnDevice(object):
    """What the predicate reads of a tensor, with is_cuda forced on: its other clauses can then be told apart on a machine without a
    device (a CPU tensor fails the device clause whatever else holds)."""

    def __init__(self, t, device):
        self._t, self.is_cuda, self.device = t, True, device
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def permute(self, *dims):
        return self._t.permute(*dims)


def test_fusable_predicate():
    from futuredet_amd import dense_bn

    dev = torch.device("cpu")

    def ok(x, bn):
        return dense_bn.batch_norm2d_nhwc_fusable(_OnDevice(x, dev), bn)

    def cl(B, C, H, W, dtype=torch.bfloat16):
        """an NCHW-shaped view of contiguous NHWC memory"""
        return torch.randn(B, H, W, C).to(dtype).permute(0, 3, 1, 2)

    x = cl(2, 32, 5, 5)
    assert ok(x, nn.BatchNorm2d(32).train())  # the stand-in passes every clause: each case below fails for its own reason
    assert ok(x.contiguous(memory_format=torch.channels_last), nn.BatchNorm2d(32).train())
    assert not ok(x, nn.BatchNorm2d(32).eval())
    with torch.no_grad():
        assert not ok(x, nn.BatchNorm2d(32).train())
    assert not ok(cl(2, 32, 5, 5, torch.float32), nn.BatchNorm2d(32).train())
    assert not ok(x.contiguous(), nn.BatchNorm2d(32).train())  # NCHW-contiguous bf16
    assert not ok(cl(2, 16, 5, 5), nn.BatchNorm2d(16).train())
    assert not ok(x, nn.BatchNorm2d(32, affine=False).train())
    assert not ok(x, nn.BatchNorm2d(32, momentum=None).train())
    assert not ok(x, nn.BatchNorm2d(32, track_running_stats=False).train())
    assert not ok(x, nn.BatchNorm2d(32).double().train())
    assert not ok(x, nn.BatchNorm2d(64).train())
    assert not ok(cl(2, 48, 5, 5), nn.BatchNorm2d(48).train()) and not ok(cl(2, 544, 2, 2), nn.BatchNorm2d(544).train())
    assert ok(cl(2, 512, 2, 2), nn.BatchNorm2d(512).train()) and ok(cl(2, 160, 2, 2), nn.BatchNorm2d(160).train())
    assert not ok(cl(1, 32, 1, 1), nn.BatchNorm2d(32).train()) and ok(cl(2, 32, 1, 1), nn.BatchNorm2d(32).train())
    assert not ok(x[:, :, :, ::2], nn.BatchNorm2d(32).train())
    assert not ok(torch.randn(2, 32, 5).to(torch.bfloat16), nn.BatchNorm2d(32).train())
    assert not dense_bn.batch_norm2d_nhwc_fusable(x, nn.BatchNorm2d(32).train())  # a host tensor
    # the grouped form: the modules partition the channels
    many = [nn.BatchNorm2d(64).train() for _ in range(6)]
    wide = _OnDevice(cl(2, 384, 3, 3), dev)
    assert dense_bn.batch_norm2d_nhwc_group_fusable(wide, many)
    assert not dense_bn.batch_norm2d_nhwc_group_fusable(wide, many[:5])
    assert not dense_bn.batch_norm2d_nhwc_group_fusable(wide, many[:5] + [nn.BatchNorm2d(64).eval()])
    assert not dense_bn.batch_norm2d_nhwc_group_fusable(_OnDevice(cl(2, 288, 3, 3), dev), [nn.BatchNorm2d(32).train() for _ in range(9)])
    assert not dense_bn.batch_norm2d_nhwc_group_fusable(_OnDevice(cl(2, 64, 3, 3), dev), [nn.BatchNorm2d(48).train(), nn.BatchNorm2d(16).train()])


def _rpn():
    from futuredet_amd.necks import RPN

    return RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
               num_input_features=32)


def _head():
    from futuredet_amd.heads import CenterHead

    return CenterHead(in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], common_heads=dict(HEADS), share_conv_channel=64,
                      timesteps=1, dense=False, bev_map=False, forecast_feature=False, classify=False, wide_head=False)


def _train_once(m, x, G, fused, dtype):
    m = copy.deepcopy(m).train()
    m.fused_bn, m.train_dtype = fused, dtype
    xin = x.clone().requires_grad_(True)
    out = m(xin)
    maps = [out] if isinstance(out, torch.Tensor) else [d[k] for d in out for k in sorted(d)]
    sum((o * g).sum() for o, g in zip(maps, G)).backward()
    return maps, xin.grad, {k: p.grad for k, p in m.named_parameters()}, {k: v for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


@pytest.mark.parametrize("which", ["rpn", "head"])
def test_both_switches_on_give_the_bits_of_the_module_chain_on_the_cpu(which):
    """host tensors take neither the mixed-precision path nor the fused kernels: fused_bn = True with train_dtype = bf16 walks the module
    chain"""
    torch.manual_seed(3)
    m, x = (_rpn(), torch.randn(2, 32, 12, 12)) if which == "rpn" else (_head(), torch.randn(2, 64, 12, 12))
    m.train()
    probe = m(x)
    shapes = [probe.shape] if isinstance(probe, torch.Tensor) else [d[k].shape for d in probe for k in sorted(d)]
    G = [torch.randn(s) for s in shapes]
    m.zero_grad()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.reset_running_stats()
    off, on = _train_once(m, x, G, False, torch.float32), _train_once(m, x, G, True, torch.bfloat16)
    assert len(off[0]) == len(on[0]) and all(torch.equal(a, b) for a, b in zip(off[0], on[0]))
    assert torch.equal(off[1], on[1])
    for part in (2, 3):
        assert set(off[part]) == set(on[part]) and len(off[part]) > 0
        for k in off[part]:
            assert (off[part][k] is None and on[part][k] is None) or torch.equal(off[part][k], on[part][k]), k
    assert all(int(v) == 1 for k, v in on[3].items() if "num_batches" in k)


def test_the_walks_take_the_switch():
    """run_stack_bf16, run_head_stack_bf16 and sep_head_bf16 take ``fused_bn`` (off by default); both forward_mixed hand theirs on"""
    import inspect

    from futuredet_amd import dense_train, heads, necks

    for fn in (dense_train.run_stack_bf16, dense_train.run_head_stack_bf16, dense_train.sep_head_bf16):
        assert inspect.signature(fn).parameters["fused_bn"].default is False, fn.__name__
    for cls in (necks.RPN, heads.CenterHead):
        src = inspect.getsource(cls.forward_mixed)
        assert "bool(self.fused_bn)" in src and "has no effect" not in src, cls.__name__
