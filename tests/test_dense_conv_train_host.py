"""The host side of mixed-precision dense-convolution training (csrc/fd_conv2d_grad_bf16.hip, dense_train.py, RPN.train_dtype): exported
symbols, chunk and workspace sizes, the argument checks of the two entry points (they validate before any device work), the predicate
conv_takes_bf16 and the neck's switch on CPU tensors.  CPU only."""
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

NAMES = {"fd_conv2d_pack_weight_dev", "fd_conv2d_wgrad_bf16", "fd_conv2d_wgrad_bf16_workspace_bytes", "fd_conv2d_wgrad_bf16_chunk"}


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def test_symbols_are_declared_and_exported(L):
    assert NAMES <= set(lib.SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert getattr(L, name) is not None
    assert "fd_conv2d_grad_bf16.hip" in build.SOURCES
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    for name in ("pack_conv2d_weight_device", "conv2d_wgrad_bf16"):
        assert callable(getattr(hip_ops, name)), name


def test_chunk_and_workspace_bytes(L):
    chunk = L.fd_conv2d_wgrad_bf16_chunk()
    assert chunk > 0 and chunk % 64 == 0
    assert hip_ops.conv2d_wgrad_bf16_chunk() == chunk
    ws = L.fd_conv2d_wgrad_bf16_workspace_bytes
    for bad in ((2, 8, 8, 48, 64, 3), (2, 8, 8, 64, 48, 3), (2, 8, 8, 64, 64, 2), (0, 8, 8, 64, 64, 3), (2, -1, 8, 64, 64, 3), (2, 8, 0, 64, 64, 3),
                (2, 8, 8, 0, 64, 3), (2, 8, 8, 64, -32, 1)):
        assert ws(*bad) == 0, bad
    # one fp32 [tap][cin][cout] partial per chunk of pixels, so monotone in B H W
    for cin, cout, ks in ((32, 32, 3), (256, 128, 3), (128, 256, 1)):
        sizes = [ws(1, 1, n, cin, cout, ks) for n in (1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1)]
        assert sizes == [c * ks * ks * cin * cout * 4 for c in (1, 1, 2, 2, 3)], (cin, cout, ks, sizes)
    prev = 0
    for B, H, W in ((1, 3, 5), (2, 9, 17), (2, 20, 28), (1, 90, 90), (2, 90, 90), (1, 180, 180), (2, 180, 180), (4, 180, 180)):
        cur = ws(B, H, W, 64, 96, 3)
        assert cur > 0 and cur >= prev, (B, H, W, cur, prev)
        assert cur == ws(1, 1, B * H * W, 64, 96, 3)  # a function of the pixel count only
        prev = cur


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    big = 1 << 40

    def wgrad(**kw):
        a = dict(x=p, dy=p, B=2, H=20, W=28, cin=64, cout=96, ks=3, ws=p, ws_bytes=big, dw=p)
        a.update(kw)
        return L.fd_conv2d_wgrad_bf16(a["x"], a["dy"], a["B"], a["H"], a["W"], a["cin"], a["cout"], a["ks"], a["ws"], a["ws_bytes"], a["dw"], None)

    def pack(**kw):
        a = dict(w=p, cout=64, cin=32, ks=3, mode=0, dst=p)
        a.update(kw)
        return L.fd_conv2d_pack_weight_dev(a["w"], a["cout"], a["cin"], a["ks"], a["mode"], a["dst"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for k in ("x", "dy", "ws", "dw"):
        bad(wgrad, "fd_conv2d_wgrad_bf16: null argument", **{k: None})
    for cin, cout in ((48, 96), (64, 48), (0, 96), (64, 0), (-32, 32), (16, 32)):
        bad(wgrad, "fd_conv2d_wgrad_bf16: cin and cout must be positive multiples of 32", cin=cin, cout=cout)
    for ks in (2, 0, 5, -1):
        bad(wgrad, "fd_conv2d_wgrad_bf16: ks must be 1 or 3", ks=ks)
        bad(pack, "fd_conv2d_pack_weight_dev: ks must be 1 or 3", ks=ks)
    for k in ("B", "H", "W"):
        for v in (0, -3):
            bad(wgrad, "fd_conv2d_wgrad_bf16: bad shape", **{k: v})
    bad(wgrad, "2^31 pixels", B=1 << 11, H=1 << 10, W=1 << 10)
    need = L.fd_conv2d_wgrad_bf16_workspace_bytes(2, 20, 28, 64, 96, 3)
    assert need > 0
    bad(wgrad, "workspace too small", ws_bytes=need - 1)
    bad(wgrad, "workspace too small", ws_bytes=0)
    for k in ("w", "dst"):
        bad(pack, "fd_conv2d_pack_weight_dev: null argument", **{k: None})
    for cin in (48, 16, 0, -32):
        bad(pack, "cin must be a positive multiple of 32", cin=cin)
    bad(pack, "cin must be a positive multiple of 32", cout=0)
    bad(pack, "mode 1 needs cout % 32 == 0", cout=40, mode=1)  # the input gradient would have 40 input channels
    for mode in (-1, 2):
        bad(pack, "mode must be 0 or 1", mode=mode)


def test_front_end_has_no_cpu_path():
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.pack_conv2d_weight_device(torch.zeros((32, 32, 3, 3)))
    x = torch.zeros((1, 4, 4, 32), dtype=torch.bfloat16)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.conv2d_wgrad_bf16(x, x, 3)
    from futuredet_amd import dense_train

    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        dense_train.conv2d_bf16(x, torch.zeros((32, 32, 3, 3)), 3)


def test_conv_takes_bf16_predicate():
    from futuredet_amd.dense_train import conv_takes_bf16

    x = torch.zeros((1, 32, 4, 4))
    assert conv_takes_bf16(nn.Conv2d(32, 64, 3, padding=1, bias=False), x)
    assert conv_takes_bf16(nn.Conv2d(128, 256, 1, bias=False), x)
    for conv in (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False),   # stride 2
                 nn.Conv2d(32, 64, 3, padding=1, bias=True),              # bias
                 nn.Conv2d(32, 64, 3, padding=1, groups=2, bias=False),   # groups
                 nn.Conv2d(48, 64, 3, padding=1, bias=False), nn.Conv2d(64, 48, 3, padding=1, bias=False),  # 48 channels
                 nn.Conv2d(32, 64, 3, padding=0, bias=False), nn.Conv2d(32, 64, 1, padding=1, bias=False),  # the other paddings
                 nn.Conv2d(32, 64, 3, padding=2, dilation=2, bias=False), nn.Conv2d(32, 64, 5, padding=2, bias=False),
                 nn.Conv2d(32, 64, 3, padding=1, bias=False).double(),
                 nn.ConvTranspose2d(64, 64, 2, stride=2, bias=False), nn.ConvTranspose2d(64, 64, 1, bias=False),
                 nn.BatchNorm2d(32), nn.ReLU()):
        assert not conv_takes_bf16(conv, x), conv


def _small_rpn():
    from futuredet_amd.necks import RPN

    torch.manual_seed(0)
    neck = RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[64, 64],
               num_input_features=32)
    neck.init_weights()
    return neck


def test_neck_train_dtype_switch_on_cpu_tensors():
    neck = _small_rpn().train()
    assert neck.train_dtype is torch.float32
    keys = list(neck.state_dict())
    x = torch.randn(2, 32, 16, 24)
    neck.train_dtype = torch.float16
    with pytest.raises(ValueError, match="train_dtype"):
        neck(x)
    neck.train_dtype = torch.bfloat16
    assert list(neck.state_dict()) == keys  # a switch, not state
    ref = copy.deepcopy(neck)
    got, want = neck(x), ref.forward_modules(x)  # a host tensor still runs the module chain
    assert got.dtype == torch.float32 and torch.equal(got, want)
    neck.eval()
    neck.train_dtype = torch.float16  # eval mode does not look at the training switch
    with torch.no_grad():
        assert torch.equal(neck(x), ref.eval().forward_modules(x))
