"""The host side of the sync-free training step (csrc/fd_optim.hip's device-record entry, csrc/fd_rows.hip, solver.StaticTrainStep,
SpMiddleResNetFHD.forward_static_train): exported symbols, the argument checks of the three entry points (no device needed: they
validate before any device work), the validation of the optimiser's scalars before they are uploaded, and the refusals of the step's
constructor.  CPU only."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402

NAMES = {"fd_optim_adam_step_dev", "fd_rows_colsum", "fd_levels_overflow"}
HELPERS = {"fd_rows_colsum_chunk", "fd_rows_colsum_workspace_bytes"}


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _table(**kw):
    p = 0x10000
    a = dict(params=p, numel=p, offset=p, flags=p, step=p, coef=p, chunks=p, partials=p, norm=p, grad=p, exp_avg=p, exp_avg_sq=p, total=64,
             n_tensors=2, n_chunks=2, chunk=4096)
    a.update(kw)
    return lib.OptimTable(**a)


def test_symbols_header_build_flags_and_abi(L):
    import subprocess

    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NAMES | HELPERS:
        assert re.search(r"\b%s\s*\(" % name, bare), name
        assert name in lib.SIGNATURES and name in exported, name
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    assert "fd_rows.hip" in build.SOURCES and build.EXTRA["fd_rows.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    chunk = int(re.search(r"#define FD_ROWS_COLSUM_CHUNK (\d+)", hdr).group(1))
    assert L.fd_rows_colsum_chunk() == chunk == hip_ops.rows_colsum_chunk() == 512
    # the device-record entry takes the table by pointer and no scalar by value
    assert lib.SIGNATURES["fd_optim_adam_step_dev"][1] == [ctypes.POINTER(lib.OptimTable), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]


def test_colsum_workspace_bytes(L):
    P = L.fd_rows_colsum_chunk()
    for C in (16, 32, 64, 128):
        sizes = [L.fd_rows_colsum_workspace_bytes(n, C) for n in (0, 1, P - 1, P, P + 1, 4097, 160000, 1 << 30)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes), (C, sizes)
        assert L.fd_rows_colsum_workspace_bytes(160000, C) >= (160000 + P - 1) // P * C * 8
    for C in (0, 8, 24, 48, 96, 256):
        assert L.fd_rows_colsum_workspace_bytes(1000, C) == 0, C
    for n in (-1, (1 << 30) + 1):
        assert L.fd_rows_colsum_workspace_bytes(n, 16) == 0, n


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p, odd4, odd8 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004), ctypes.c_void_p(0x10008)

    def err():
        return L.fd_last_error().decode()

    # fd_optim_adam_step_dev
    assert L.fd_optim_adam_step_dev(None, p, 1, None, None) == -1 and "fd_optim_adam_step_dev: null table" in err()
    for member in ("params", "numel", "offset", "flags", "step", "coef", "chunks", "partials", "norm"):
        assert L.fd_optim_adam_step_dev(ctypes.byref(_table(**{member: None})), p, 1, None, None) == -1
        assert "fd_optim_adam_step_dev: null table member" in err(), member
    for member in ("grad", "exp_avg", "exp_avg_sq"):
        assert L.fd_optim_adam_step_dev(ctypes.byref(_table(**{member: None})), p, 1, None, None) == -1 and "null flat buffer" in err()
    assert L.fd_optim_adam_step_dev(ctypes.byref(_table(chunk=1024)), p, 1, None, None) == -1 and "chunk size" in err()
    assert L.fd_optim_adam_step_dev(ctypes.byref(_table()), None, 1, None, None) == -1 and "fd_optim_adam_step_dev: null hyper record" in err()
    assert L.fd_optim_adam_step_dev(ctypes.byref(_table()), odd4, 1, None, None) == -1 and "8-byte aligned" in err()
    assert L.fd_optim_adam_step_dev(ctypes.byref(_table()), p, 2, None, None) == -1 and "clip must be 0 or 1" in err()

    # fd_rows_colsum
    big = 1 << 40

    def colsum(**kw):
        a = dict(x=p, n=1000, n_dev=None, C=16, dtype=0, out=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_rows_colsum(a["x"], a["n"], a["n_dev"], a["C"], a["dtype"], a["out"], a["ws"], a["ws_bytes"], None)

    def bad(text, **kw):
        assert colsum(**kw) == -1 and text in err(), (kw, text, err())

    for C in (0, 8, 24, 48, 96, 256):
        bad("fd_rows_colsum: C must be 16, 32, 64 or 128", C=C)
    bad("dtype must be 0 (fp32) or 1 (bf16)", dtype=2)
    bad("must lie in [0, 2^30]", n=-1)
    bad("must lie in [0, 2^30]", n=(1 << 30) + 1)
    bad("null out", out=None)
    bad("null rows", x=None)
    bad("workspace must be non-null and 16-byte aligned", ws=None)
    bad("workspace must be non-null and 16-byte aligned", ws=odd8)
    bad("needed", ws_bytes=L.fd_rows_colsum_workspace_bytes(1000, 16) - 1)

    # fd_levels_overflow
    for args in ((None, p, 5, p), (p, None, 5, p), (p, p, 5, None)):
        assert L.fd_levels_overflow(*args, None) == -1 and "fd_levels_overflow: null counts, caps or flag" in err()
    for n in (0, -1, 65):
        assert L.fd_levels_overflow(p, p, n, p, None) == -1 and "n_levels" in err()


def test_scalars_are_validated_before_the_upload():
    good = dict(lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, max_norm=35.0)
    assert hip_ops.check_hyper(**good) == [good[k] for k in hip_ops.HYPER_FIELDS]
    for key, value, text in (("beta1", 1.0, "betas"), ("beta1", -0.1, "betas"), ("beta2", 1.0, "betas"), ("beta1", float("nan"), "betas"),
                             ("eps", 0.0, "eps"), ("eps", float("nan"), "eps"), ("lr", float("nan"), "NaN"), ("wd", float("nan"), "NaN"),
                             ("max_norm", float("nan"), "NaN")):
        with pytest.raises(ValueError, match=text):
            hip_ops.check_hyper(**dict(good, **{key: value}))
    w = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        solver.FusedAdam([[w], []])
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.rows_colsum(torch.zeros(4, 16))
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.levels_overflow(torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32))


def _voxelnet(dcn_head=False):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.targets import TargetAssigner

    cfg = centerpoint_config("forecast_n0", dcn_head=dcn_head)
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    ta = TargetAssigner(cfg.train_cfg.assigner, np.array([1440, 1440, 40]), vg["range"], vg["voxel_size"])
    return net, vg, ta


def test_constructor_names_what_is_missing():
    """every refusal comes before any device work: the models live on the CPU and no optimiser exists"""
    from futuredet_amd import build_detector
    from futuredet_amd.configs import pointpillars_config

    net, vg, ta = _voxelnet()
    assert net.backbone.fused_bn is False and net.bbox_head.fused_loss is False
    with pytest.raises(ValueError, match=r"backbone\.fused_bn"):
        solver.StaticTrainStep(net, vg, ta, None, capacity=1000)
    net.backbone.fused_bn = True
    with pytest.raises(ValueError, match=r"bbox_head\.fused_loss"):
        solver.StaticTrainStep(net, vg, ta, None, capacity=1000)
    net.bbox_head.fused_loss = True
    with pytest.raises(NotImplementedError, match="graph=True"):  # ending the capture of the whole step crashed the HIP runtime
        solver.StaticTrainStep(net, vg, ta, None, capacity=1000, graph=True)
    with pytest.raises(NotImplementedError, match="norm_type"):  # the options train_steps refuses are refused here too
        solver.StaticTrainStep(net, vg, ta, None, grad_clip=dict(max_norm=35, norm_type=1), capacity=1000)

    dcn, vg2, ta2 = _voxelnet(dcn_head=True)
    dcn.backbone.fused_bn, dcn.bbox_head.fused_loss = True, True
    with pytest.raises(NotImplementedError, match="dcn_head"):
        solver.StaticTrainStep(dcn, vg2, ta2, None, capacity=1000)

    cfg = pointpillars_config()
    pp = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    pp.bbox_head.fused_loss = True
    with pytest.raises(NotImplementedError, match="PointPillars"):
        solver.StaticTrainStep(pp, cfg.voxel_generator, ta, None, capacity=1000)
    assert "StaticTrainStep" in solver.__all__


def test_forward_static_train_needs_fused_bn():
    from futuredet_amd.backbones import SpMiddleResNetFHD

    bb = SpMiddleResNetFHD(num_input_features=5).train()
    with pytest.raises(ValueError, match="fused_bn = True"):
        bb.forward_static_train(torch.zeros(4, 16), [])
    bb.fused_bn = True
    bb.eval()
    with pytest.raises(RuntimeError, match="training path"):
        bb.forward_static_train(torch.zeros(4, 16), [])
