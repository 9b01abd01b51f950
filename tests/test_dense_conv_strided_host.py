"""The host side of mixed-precision training of the dense convolutions that change resolution (csrc/fd_conv2d_strided_grad_bf16.hip, the
strided instantiations in csrc/fd_conv2d_grad_bf16.hip, dense_train.py): exported symbols and ctypes signatures, workspace and pack
sizes, the argument checks of the entry points (they validate before any device work), the four predicates and the neck's switch on
CPU tensors.  CPU only."""
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

from futuredet_amd import build, dense_train, hip_ops, lib  # noqa: E402

c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {
    "fd_conv2d_s2_dgrad_bf16": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p] * 3),
    "fd_conv2d_wgrad_s2_bf16_workspace_bytes": (c_size_t, [c_int] * 5),
    "fd_conv2d_wgrad_s2_bf16": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "fd_conv2d_down2_bf16": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_int, c_void_p, c_void_p]),
    "fd_conv2d_packed_weight_2x2_bytes": (c_size_t, [c_int] * 3),
    "fd_conv2d_pack_weight_2x2_dev": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p] * 2),
    "fd_conv2d_wgrad_2x2_bf16_workspace_bytes": (c_size_t, [c_int] * 5),
    "fd_conv2d_wgrad_2x2_bf16": (c_int, [c_void_p] * 2 + [c_int] * 6 + [c_void_p, c_size_t, c_void_p, c_void_p]),
}


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def test_symbols_are_declared_and_exported(L):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    for name, (res, args) in SIGNATURES.items():
        assert lib.SIGNATURES[name] == (res, args), name
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(args), name  # one ctypes argument per declared parameter
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert "fd_conv2d_strided_grad_bf16.hip" in build.SOURCES
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    for name in ("conv2d_s2_dgrad_bf16", "conv2d_wgrad_s2_bf16", "pack_conv2d_weight_2x2_device", "conv2d_up2_bf16", "conv2d_down2_bf16",
                 "conv2d_wgrad_2x2_bf16"):
        assert callable(getattr(hip_ops, name)), name
    for name in ("conv2d_s2_bf16", "conv_transpose2d_k2_bf16", "conv2d_k2s2_bf16", "conv_s2_takes_bf16", "_pad_then_conv_s2_takes_bf16",
                 "conv_up2_takes_bf16", "conv_down2_takes_bf16"):
        assert callable(getattr(dense_train, name)), name


def test_workspace_and_pack_bytes(L):
    chunk = L.fd_conv2d_wgrad_bf16_chunk()
    s2, k2, pk = L.fd_conv2d_wgrad_s2_bf16_workspace_bytes, L.fd_conv2d_wgrad_2x2_bf16_workspace_bytes, L.fd_conv2d_packed_weight_2x2_bytes
    for bad in ((2, 8, 8, 48, 64), (2, 8, 8, 64, 48), (0, 8, 8, 64, 64), (2, -1, 8, 64, 64), (2, 8, 0, 64, 64), (2, 8, 8, 0, 64), (2, 8, 8, 64, -32)):
        assert s2(*bad) == 0 and k2(*bad) == 0, bad
    assert k2(1, 1, 8, 32, 32) == 0 and k2(1, 8, 1, 32, 32) == 0  # a fine map without one whole 2 x 2 block
    # one fp32 [tap][cin][cout] partial per chunk of OUTPUT pixels: stride 2 over 1 x W has (W - 1) // 2 + 1 of them, 2 x 2 over 2 x W has W // 2
    for cin, cout in ((32, 32), (128, 256), (256, 128)):
        for n_out, chunks in ((1, 1), (chunk, 1), (chunk + 1, 2), (2 * chunk, 2), (2 * chunk + 1, 3)):
            for W in (2 * n_out - 1, 2 * n_out):
                assert s2(1, 1, W, cin, cout) == chunks * 9 * cin * cout * 4, (cin, cout, W)
            for W in (2 * n_out, 2 * n_out + 1):
                assert k2(1, 2, W, cin, cout) == k2(1, 3, W, cin, cout) == chunks * 4 * cin * cout * 4, (cin, cout, W)
    assert s2(2, 9, 17, 64, 96) == s2(1, 1, 2 * 2 * 5 * 9 - 1, 64, 96)  # a function of the output pixel count only
    assert k2(2, 9, 17, 64, 96) == k2(1, 2, 2 * 2 * 4 * 8, 64, 96)
    base = L.fd_conv2d_packed_weight_bytes
    for cc, cf in ((32, 32), (64, 96), (256, 128), (64, 40)):  # up2: the fine side is the output side and is padded to 32
        assert pk(cc, cf, 0) == 4 * base(cf, cc, 1) > 0, (cc, cf)
    for cc, cf in ((32, 32), (96, 64), (128, 256), (40, 64)):  # down2: the coarse side is
        assert pk(cc, cf, 1) == base(cc, 4 * cf, 1) > 0, (cc, cf)
    for bad in ((48, 32, 0), (32, 48, 1), (0, 32, 0), (32, 0, 1), (32, 32, 2), (32, 32, -1), (-32, 32, 0), (32, -32, 1), (0, 32, 1), (32, 0, 0)):
        assert pk(*bad) == 0, bad


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    big = 1 << 40

    def dgrad(**kw):
        a = dict(dy=p, B=2, H=20, W=28, cin=64, cout=96, wpk=p, dx=p)
        a.update(kw)
        return L.fd_conv2d_s2_dgrad_bf16(a["dy"], a["B"], a["H"], a["W"], a["cin"], a["cout"], a["wpk"], a["dx"], None)

    def wgrad_s2(**kw):
        a = dict(x=p, dy=p, B=2, H=20, W=28, cin=64, cout=96, ws=p, ws_bytes=big, dw=p)
        a.update(kw)
        return L.fd_conv2d_wgrad_s2_bf16(a["x"], a["dy"], a["B"], a["H"], a["W"], a["cin"], a["cout"], a["ws"], a["ws_bytes"], a["dw"], None)

    def down2(**kw):
        a = dict(x=p, B=2, H=20, W=28, cin=64, wpk=p, cout=96, y=p)
        a.update(kw)
        return L.fd_conv2d_down2_bf16(a["x"], a["B"], a["H"], a["W"], a["cin"], a["wpk"], a["cout"], a["y"], None)

    def pack(**kw):
        a = dict(w=p, cin=64, cout=96, kind=0, fine_major=0, dst=p)  # (cin: the coarse side, cout: the fine side)
        a.update(kw)
        return L.fd_conv2d_pack_weight_2x2_dev(a["w"], a["cin"], a["cout"], a["kind"], a["fine_major"], a["dst"], None)

    def wgrad_2x2(**kw):
        a = dict(x=p, dy=p, B=2, H=20, W=28, cin=64, cout=96, fine_major=0, ws=p, ws_bytes=big, dw=p)
        a.update(kw)
        return L.fd_conv2d_wgrad_2x2_bf16(a["x"], a["dy"], a["B"], a["H"], a["W"], a["cin"], a["cout"], a["fine_major"], a["ws"], a["ws_bytes"],
                                          a["dw"], None)

    def bad(fn, text, **kw):
        assert fn(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error())

    for fn, name, ptrs in ((dgrad, "fd_conv2d_s2_dgrad_bf16", ("dy", "wpk", "dx")), (wgrad_s2, "fd_conv2d_wgrad_s2_bf16", ("x", "dy", "ws", "dw")),
                           (down2, "fd_conv2d_down2_bf16", ("x", "wpk", "y")), (wgrad_2x2, "fd_conv2d_wgrad_2x2_bf16", ("x", "dy", "ws", "dw")),
                           (pack, "fd_conv2d_pack_weight_2x2_dev", ("w", "dst"))):
        for k in ptrs:
            bad(fn, name + ": null argument", **{k: None})
        if fn is pack:
            continue
        for cin, cout in ((48, 96), (64, 48), (0, 96), (64, 0), (-32, 32), (16, 32)):
            bad(fn, name + ": ", cin=cin, cout=cout)
            assert "multiples of 32" in L.fd_last_error().decode()
        for k in ("B", "H", "W"):
            for v in (0, -3):
                bad(fn, name + ": bad shape", **{k: v})
    for fn in (down2, wgrad_2x2):  # the fine map holds one whole 2 x 2 block at least
        bad(fn, "bad shape", H=1)
        bad(fn, "bad shape", W=1)
    for fn, need in ((wgrad_s2, L.fd_conv2d_wgrad_s2_bf16_workspace_bytes(2, 20, 28, 64, 96)),
                     (wgrad_2x2, L.fd_conv2d_wgrad_2x2_bf16_workspace_bytes(2, 20, 28, 64, 96))):
        assert need > 0
        bad(fn, "workspace too small", ws_bytes=need - 1)
        bad(fn, "workspace too small", ws_bytes=0)
        bad(fn, "2^31 pixels", B=1 << 11, H=1 << 10, W=1 << 10)
    for v in (-1, 2):
        bad(wgrad_2x2, "fine_major must be 0 or 1", fine_major=v)
        bad(pack, "fine_major must be 0 or 1", fine_major=v)
        bad(pack, "kind must be 0 (up2) or 1 (down2)", kind=v)
    for kw in (dict(cin=48), dict(cin=0), dict(cout=0), dict(cout=48, kind=1), dict(cout=-32, kind=1), dict(cin=0, kind=1)):
        bad(pack, "must be a positive multiple of 32", **kw)
    # the existing entry points still refuse what they refused: the new layers did not widen them
    assert L.fd_conv2d_wgrad_bf16(p, p, 2, 20, 28, 64, 96, 2, p, big, p, None) == -1 and "ks must be 1 or 3" in L.fd_last_error().decode()
    assert L.fd_conv2d_pack_weight_dev(p, 64, 32, 2, 0, p, None) == -1 and "ks must be 1 or 3" in L.fd_last_error().decode()


def test_front_end_has_no_cpu_path():
    x = torch.zeros((1, 4, 4, 32), dtype=torch.bfloat16)
    for fn, w in ((dense_train.conv2d_s2_bf16, torch.zeros((32, 32, 3, 3))), (dense_train.conv_transpose2d_k2_bf16, torch.zeros((32, 32, 2, 2))),
                  (dense_train.conv2d_k2s2_bf16, torch.zeros((32, 32, 2, 2)))):
        with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
            fn(x, w)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.pack_conv2d_weight_2x2_device(torch.zeros((32, 32, 2, 2)), hip_ops.PACK_UP2)
    for fn in (hip_ops.conv2d_wgrad_s2_bf16, hip_ops.conv2d_wgrad_2x2_bf16):
        with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
            fn(x, x)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.conv2d_s2_dgrad_bf16(x, torch.zeros(8, dtype=torch.uint8), 7, 7, 32)
    for fn in (hip_ops.conv2d_up2_bf16, hip_ops.conv2d_down2_bf16):
        with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
            fn(x, torch.zeros(8, dtype=torch.uint8), 32)


def test_predicates():
    x = torch.zeros((1, 32, 8, 8))
    s2, pad_s2, up2, down2 = (dense_train.conv_s2_takes_bf16, dense_train._pad_then_conv_s2_takes_bf16, dense_train.conv_up2_takes_bf16,
                              dense_train.conv_down2_takes_bf16)
    pad = nn.ZeroPad2d(1)
    assert s2(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), x)
    assert pad_s2(pad, nn.Conv2d(128, 256, 3, stride=2, bias=False), x)
    assert up2(nn.ConvTranspose2d(256, 128, 2, stride=2, bias=False), x)
    assert down2(nn.Conv2d(64, 128, 2, stride=2, bias=False), x)
    unpadded = nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=False)
    assert not s2(unpadded, x)  # without its ZeroPad2d it is another convolution
    assert not pad_s2(nn.ZeroPad2d(2), unpadded, x) and not pad_s2(nn.ZeroPad2d((1, 0, 1, 0)), unpadded, x) and not pad_s2(nn.ReLU(), unpadded, x)
    assert not pad_s2(pad, nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), x)  # padded twice
    for conv in (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=True), nn.Conv2d(32, 64, 3, stride=2, padding=1, groups=2, bias=False),
                 nn.Conv2d(48, 64, 3, stride=2, padding=1, bias=False), nn.Conv2d(64, 48, 3, stride=2, padding=1, bias=False),
                 nn.Conv2d(32, 64, 3, stride=1, padding=1, bias=False), nn.Conv2d(32, 64, 3, stride=3, padding=1, bias=False),
                 nn.Conv2d(32, 64, 3, stride=2, padding=2, dilation=2, bias=False), nn.Conv2d(32, 64, 5, stride=2, padding=2, bias=False),
                 nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False).double(), nn.Conv2d(32, 64, 2, stride=2, bias=False),
                 nn.ConvTranspose2d(32, 64, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU()):
        assert not s2(conv, x), conv
    for conv in (nn.Conv2d(32, 64, 3, stride=2, bias=True), nn.Conv2d(32, 64, 3, stride=2, groups=2, bias=False),
                 nn.Conv2d(48, 64, 3, stride=2, bias=False), nn.Conv2d(32, 64, 3, stride=1, bias=False),
                 nn.Conv2d(32, 64, 3, stride=2, bias=False).double(), nn.Conv2d(32, 64, 2, stride=2, bias=False)):
        assert not pad_s2(pad, conv, x), conv
    for conv in (nn.ConvTranspose2d(64, 64, 2, stride=2, bias=True), nn.ConvTranspose2d(64, 64, 2, stride=2, groups=2, bias=False),
                 nn.ConvTranspose2d(48, 64, 2, stride=2, bias=False), nn.ConvTranspose2d(64, 48, 2, stride=2, bias=False),
                 nn.ConvTranspose2d(64, 64, 4, stride=4, bias=False), nn.ConvTranspose2d(64, 64, 2, stride=1, bias=False),
                 nn.ConvTranspose2d(64, 64, 2, stride=2, output_padding=1, bias=False), nn.ConvTranspose2d(64, 64, 2, stride=2, padding=1, bias=False),
                 nn.ConvTranspose2d(64, 64, 2, stride=2, bias=False).double(), nn.Conv2d(64, 64, 2, stride=2, bias=False)):
        assert not up2(conv, x), conv
    for conv in (nn.Conv2d(64, 64, 2, stride=2, bias=True), nn.Conv2d(64, 64, 2, stride=2, groups=2, bias=False),
                 nn.Conv2d(48, 64, 2, stride=2, bias=False), nn.Conv2d(64, 48, 2, stride=2, bias=False), nn.Conv2d(64, 64, 4, stride=4, bias=False),
                 nn.Conv2d(64, 64, 2, stride=1, bias=False), nn.Conv2d(64, 64, 2, stride=2, padding=1, bias=False),
                 nn.Conv2d(64, 64, 2, stride=2, bias=False).double(), nn.ConvTranspose2d(64, 64, 2, stride=2, bias=False)):
        assert not down2(conv, x), conv
    assert not down2(nn.Conv2d(64, 128, 2, stride=2, bias=False), torch.zeros((1, 64, 1, 8)))  # no whole 2 x 2 block
    # the stride-1 predicate still refuses all of them
    for conv in (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), nn.ConvTranspose2d(64, 64, 2, stride=2, bias=False),
                 nn.Conv2d(64, 64, 2, stride=2, bias=False)):
        assert not dense_train.conv_takes_bf16(conv, x), conv


def _rpn(pillars):
    from futuredet_amd.necks import RPN

    torch.manual_seed(0)
    if pillars:
        neck = RPN(layer_nums=[1, 1, 1], ds_layer_strides=[2, 2, 2], ds_num_filters=[32, 64, 64], us_layer_strides=[0.5, 1, 2],
                   us_num_filters=[32, 32, 32], num_input_features=32)
    else:
        neck = RPN(layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[64, 64],
                   num_input_features=32)
    neck.init_weights()
    return neck


@pytest.mark.parametrize("pillars", [False, True], ids=["small", "pointpillars"])
def test_neck_train_dtype_switch_on_cpu_tensors(pillars):
    neck = _rpn(pillars).train()
    x = torch.randn(2, 32, 16, 24)
    # the strided layers of this neck are the ones the walk routes
    kinds = []
    for seq in list(neck.blocks) + list(neck.deblocks):
        mods = list(seq.children())
        for i, m in enumerate(mods):
            if i > 0 and dense_train._pad_then_conv_s2_takes_bf16(mods[i - 1], m, x):
                kinds.append("s2")
            elif dense_train.conv_up2_takes_bf16(m, x):
                kinds.append("up2")
            elif dense_train.conv_down2_takes_bf16(m, x):
                kinds.append("down2")
    assert sorted(kinds) == (["down2", "s2", "s2", "s2", "up2"] if pillars else ["s2", "up2"])
    keys = list(neck.state_dict())
    neck.train_dtype = torch.bfloat16
    assert list(neck.state_dict()) == keys  # a switch, not state
    ref = copy.deepcopy(neck)
    got, want = neck(x), ref.forward_modules(x)  # a host tensor still runs the module chain
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert tuple(got.shape) == ((2, 96, 4, 6) if pillars else (2, 128, 16, 24))
