"""The host side of mixed-precision CenterHead training (csrc/fd_head_tail_bf16.hip, dense_train.head_tail_bf16, the bias of
dense_train.conv2d_bf16, CenterHead.train_dtype): exported symbols, chunk and workspace sizes, the argument checks of the three entry
points (they validate before any device work), the head's two predicates and the switch on CPU tensors.  CPU only."""
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

NAMES = {"fd_head_tail_bf16_max_groups", "fd_head_tail_wgrad_bf16_chunk", "fd_head_tail_wgrad_bf16_workspace_bytes", "fd_head_tail_forward_bf16",
         "fd_head_tail_dgrad_bf16", "fd_head_tail_wgrad_bf16"}
ENTRIES = ("fd_head_tail_forward_bf16", "fd_head_tail_dgrad_bf16", "fd_head_tail_wgrad_bf16")


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
    assert "fd_head_tail_bf16.hip" in build.SOURCES
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    for name in ("head_tail_forward", "head_tail_dgrad", "head_tail_wgrad", "head_tail_max_groups", "head_tail_wgrad_chunk"):
        assert callable(getattr(hip_ops, name)), name
    # the group record: the header's members in the header's order
    body = re.search(r"typedef struct fd_head_tail_group \{(.*?)\} fd_head_tail_group;", hdr, flags=re.S).group(1)
    members = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert members == [n for n, _ in lib.HeadTailGroup._fields_]
    assert ctypes.sizeof(lib.HeadTailGroup) == 4 * 8 + 8 + 4 + 4


def test_chunk_groups_and_workspace_bytes(L):
    chunk = L.fd_head_tail_wgrad_bf16_chunk()
    assert chunk > 0 and hip_ops.head_tail_wgrad_chunk() == chunk
    assert L.fd_head_tail_bf16_max_groups() >= 6 and hip_ops.head_tail_max_groups() == L.fd_head_tail_bf16_max_groups()
    ws = L.fd_head_tail_wgrad_bf16_workspace_bytes
    for bad in ((0, 8, 8, 64), (2, -1, 8, 64), (2, 8, 0, 64), (2, 8, 8, 0), (2, 8, 8, 48), (2, 8, 8, -32)):
        assert ws(*bad) == 0, bad
    # one fp32 [10][cin][16] partial per group and chunk of pixels: nine taps, and a slot for the bias gradient
    for cin in (32, 64, 6 * 64):
        sizes = [ws(1, 1, n, cin) for n in (1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1)]
        assert sizes == [c * 10 * cin * 16 * 4 for c in (1, 1, 2, 2, 3)], (cin, sizes)
    prev = 0
    for B, H, W in ((1, 3, 5), (2, 9, 17), (2, 20, 28), (1, 90, 90), (2, 90, 90), (1, 180, 180), (2, 180, 180), (4, 180, 180)):
        cur = ws(B, H, W, 384)
        assert cur > 0 and cur >= prev, (B, H, W, cur, prev)
        assert cur == ws(1, 1, B * H * W, 384)  # a function of the pixel count only
        prev = cur


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    P = 0x10000
    big = 1 << 40
    max_groups = L.fd_head_tail_bf16_max_groups()

    def call(entry, n=2, groups="default", B=2, H=20, W=28, ws=ctypes.c_void_p(P), ws_bytes=big, **kw):
        g = dict(x=P, w=P, bias=P, y=P, x_stride=128, cin=64, k=3)
        g.update(kw)
        arr = (lib.HeadTailGroup * max(n, 1))(*[lib.HeadTailGroup(P, P, P, P, 64, 64, 2) for _ in range(max(n, 1))])
        arr[max(n, 1) - 1] = lib.HeadTailGroup(g["x"], g["w"], g["bias"], g["y"], g["x_stride"], g["cin"], g["k"])  # the bad one comes last
        gp = arr if groups == "default" else groups
        if entry == "fd_head_tail_wgrad_bf16":
            return getattr(L, entry)(gp, n, B, H, W, ws, ws_bytes, None)
        return getattr(L, entry)(gp, n, B, H, W, None)

    def bad(entry, text, **kw):
        assert call(entry, **kw) == -1, (entry, kw)
        msg = L.fd_last_error().decode()
        assert msg.startswith(entry + ": ") and text in msg, (entry, kw, text, msg)

    for entry in ENTRIES:
        bad(entry, "null argument", groups=None)
        for member in ("x", "w", "y") + (() if entry == "fd_head_tail_dgrad_bf16" else ("bias",)):
            bad(entry, "null argument", **{member: None})
        for k in (0, 17, -1, 32):
            bad(entry, "k must be in [1, 16]", k=k)
        for cin in (48, 16, 0, -32, 72):
            bad(entry, "cin must be a positive multiple of 32", cin=cin)
        bad(entry, "pixel stride below cin", x_stride=56)
        bad(entry, "pixel stride below cin", x_stride=32)
        bad(entry, "16-byte aligned", x_stride=68)
        bad(entry, "16-byte aligned", x=P + 2)
        bad(entry, "too many groups", n=max_groups + 1)
        bad(entry, "too many groups", n=0)
        for dim in ("B", "H", "W"):
            for v in (0, -3):
                bad(entry, "bad shape", **{dim: v})
        bad(entry, "2^31 pixels", B=1 << 11, H=1 << 10, W=1 << 10)
    need = L.fd_head_tail_wgrad_bf16_workspace_bytes(2, 20, 28, 128)  # the two groups of call(): 64 + 64 channels
    assert need > 0
    bad("fd_head_tail_wgrad_bf16", "workspace too small", ws_bytes=need - 1)
    bad("fd_head_tail_wgrad_bf16", "workspace too small", ws_bytes=0)
    bad("fd_head_tail_wgrad_bf16", "null argument", ws=None)


def test_front_end_has_no_cpu_path():
    from futuredet_amd import dense_train

    x = torch.zeros((1, 4, 4, 32), dtype=torch.bfloat16)
    w, b, y = torch.zeros((2, 32, 3, 3)), torch.zeros((2,)), torch.zeros((1, 2, 4, 4))
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.head_tail_forward([(x, 0, w, b)])
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.head_tail_dgrad([(x, 0, w, y)])
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.head_tail_wgrad([(x, 0, 32, y)])
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        dense_train.head_tail_bf16([(x, w, b)])
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        dense_train.conv2d_bf16(x, torch.zeros((32, 32, 3, 3)), 3, bias=torch.zeros((32,)))


def test_head_predicates():
    from futuredet_amd.dense_train import conv_takes_bf16, head_conv_takes_bf16, head_tail_takes_bf16

    x = torch.zeros((1, 64, 4, 4))
    for conv in (nn.Conv2d(64, 64, 3, padding=1, bias=True), nn.Conv2d(128, 64, 3, padding=1, bias=True), nn.Conv2d(512, 64, 3, padding=1),
                 nn.Conv2d(64, 384, 3, padding=1), nn.Conv2d(32, 64, 3, padding=1, bias=False)):
        assert head_conv_takes_bf16(conv, x) and not head_tail_takes_bf16(conv, x), conv
    for k in (1, 2, 3, 14, 16):
        for cin in (32, 64, 128):
            conv = nn.Conv2d(cin, k, 3, padding=1, bias=True)
            assert head_tail_takes_bf16(conv, x) and not head_conv_takes_bf16(conv, x) and not conv_takes_bf16(conv, x), conv
    for conv in (nn.Conv2d(64, 64, 3, stride=2, padding=1), nn.Conv2d(64, 64, 3, padding=1, groups=2), nn.Conv2d(48, 64, 3, padding=1),
                 nn.Conv2d(6, 16, 3, padding=1), nn.Conv2d(16, 32, 3, padding=1), nn.Conv2d(64, 48, 3, padding=1), nn.Conv2d(64, 64, 3, padding=0),
                 nn.Conv2d(64, 64, 1), nn.Conv2d(64, 64, 3, padding=2, dilation=2), nn.Conv2d(64, 64, 5, padding=2),
                 nn.Conv2d(64, 64, 3, padding=1, padding_mode="reflect"), nn.Conv2d(64, 64, 3, padding=1).double(),
                 nn.ConvTranspose2d(64, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU()):
        assert not head_conv_takes_bf16(conv, x), conv
    for conv in (nn.Conv2d(64, 17, 3, padding=1), nn.Conv2d(64, 32, 3, padding=1), nn.Conv2d(64, 3, 3, padding=1, bias=False),
                 nn.Conv2d(48, 3, 3, padding=1), nn.Conv2d(16, 3, 3, padding=1), nn.Conv2d(64, 3, 1), nn.Conv2d(64, 3, 3, padding=0),
                 nn.Conv2d(64, 3, 3, stride=2, padding=1), nn.Conv2d(64, 2, 3, padding=1, groups=2), nn.Conv2d(64, 3, 3, padding=2, dilation=2),
                 nn.Conv2d(64, 3, 3, padding=1).double(), nn.ConvTranspose2d(64, 3, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU()):
        assert not head_tail_takes_bf16(conv, x), conv
    # the neck's predicate still refuses a bias
    assert not conv_takes_bf16(nn.Conv2d(64, 64, 3, padding=1, bias=True), x)


def _small_head(kind):
    from futuredet_amd.heads import CenterHead

    torch.manual_seed(0)
    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    kw = dict(in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
              common_heads=common, share_conv_channel=64, classify=False)
    if kind == "standard":
        return CenterHead(timesteps=1, **kw)
    if kind == "dense_ff":
        return CenterHead(timesteps=3, dense=True, forecast_feature=True, **kw)
    return CenterHead(timesteps=1, dcn_head=True, **kw)


@pytest.mark.parametrize("kind", ["standard", "dense_ff"])
def test_head_train_dtype_switch_on_cpu_tensors(kind):
    head = _small_head(kind).train()
    assert head.train_dtype is torch.float32
    keys = list(head.state_dict())
    x = torch.randn(2, 64, 8, 12)
    head.train_dtype = torch.float16
    with pytest.raises(ValueError, match="train_dtype"):
        head(x)
    head.train_dtype = torch.bfloat16
    assert list(head.state_dict()) == keys  # a switch, not state
    ref = copy.deepcopy(head)
    got, want = head(x), ref.forward_modules(x)  # a host tensor still runs the module chain
    assert len(got) == len(want) == len(head.tasks)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for k in g:
            assert g[k].dtype == torch.float32 and torch.equal(g[k], w[k]), k
    head.eval()
    head.train_dtype = torch.float16  # eval mode does not look at the training switch
    with torch.no_grad():
        for g, w in zip(head(x), ref.eval().forward_modules(x)):
            for k in g:
                assert torch.equal(g[k], w[k]), k


def test_dcn_head_refuses_bf16_training():
    head = _small_head("dcn").train()
    head.train_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="dcn_head"):
        head(torch.randn(1, 64, 8, 12))
