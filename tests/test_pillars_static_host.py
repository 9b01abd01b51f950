"""The host side of the sync-free PointPillars / map-head training step (csrc/fd_pillars_grad.hip's device-count entries,
PillarFeatureNet.forward_train_static, solver.StaticPillarsTrainStep, the bev_map input of solver.StaticTrainStep): exported symbols,
ctypes signatures, the argument checks of the new entry points (they validate before any device work) and the refusals of the two
constructors.  CPU only."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402

NAMES = ("fd_pillar_train_forward_dev", "fd_pillar_train_backward_dev", "fd_pillar_train_running_stats_dev")


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def test_symbols_header_and_signatures(L):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, bare), name
        assert name in lib.SIGNATURES and name in exported, name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == lib.SIGNATURES[name][1], name
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    # the header declares as many parameters as the ctypes table passes
    for name in NAMES:
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1]), name
    for name in ("pillar_train_forward_dev", "pillar_train_backward_dev", "pillar_train_running_stats_dev"):
        assert callable(getattr(hip_ops, name)), name
    assert "n_dev" in hip_ops.pillar_scatter_backward.__code__.co_varnames
    assert "StaticPillarsTrainStep" in solver.__all__ and "StaticTrainStep" in solver.__all__


def test_invalid_arguments_are_status_codes_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = ctypes.c_void_p(0x10000)
    big = 1 << 40

    def err():
        return L.fd_last_error().decode()

    def fwd(**kw):
        a = dict(voxels=p, num=p, coors=p, counts=p, n_seg=2, stride=64, P=20, ndim=5, wd=0, u1=32, u2=64, eps1=1e-3, eps2=1e-3, w1=p, out=p,
                 mean1=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_pillar_train_forward_dev(a["voxels"], a["num"], a["coors"], a["counts"], a["n_seg"], a["stride"], a["P"], a["ndim"], a["wd"],
                                             0.2, 0.2, 0.1, 0.1, a["w1"], p, p, a["u1"], a["eps1"], p, p, p, a["u2"], a["eps2"], a["out"],
                                             a["mean1"], p, p, p, a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(voxels=p, counts=p, n_seg=2, stride=64, P=20, ndim=5, u1=32, u2=64, dout=p, dw1=p, ws=p, ws_bytes=big)
        a.update(kw)
        return L.fd_pillar_train_backward_dev(a["voxels"], p, p, a["counts"], a["n_seg"], a["stride"], a["P"], a["ndim"], 0, 0.2, 0.2, 0.1, 0.1,
                                              p, p, p, a["u1"], p, p, p, a["u2"], a["dout"], a["dw1"], p, p, p, p, p, a["ws"], a["ws_bytes"], None)

    need = L.fd_pillar_train_workspace_bytes(2 * 64, 20)
    assert need > 0
    for call, fn in ((fwd, "fd_pillar_train_forward_dev"), (bwd, "fd_pillar_train_backward_dev")):
        for n_seg in (0, -1, 17):
            assert call(n_seg=n_seg) == -1 and fn + ": n_seg must be in [1,16]" in err(), (fn, n_seg, err())
        for stride in (0, -5, 1 << 30):
            assert call(stride=stride) == -1 and fn + ": seg_stride out of range" in err(), (fn, stride, err())
        for P in (0, 33):
            assert call(P=P) == -1 and "max_points must be in [1,32]" in err(), (fn, P)
        for ndim in (2, 9):
            assert call(ndim=ndim) == -1 and "ndim must be in [3,8]" in err(), (fn, ndim)
        assert call(u1=64) == -1 and "unsupported units" in err()
        assert call(u2=32) == -1 and "unsupported units" in err()
        assert call(voxels=None) == -1 and fn + ": null argument" in err()
        assert call(counts=None) == -1 and fn + ": null seg_counts" in err()
        assert call(ws=None) == -1 and "workspace too small" in err()
        assert call(ws_bytes=need - 1) == -1 and "workspace too small" in err()
    assert fwd(out=None) == -1 and "null output" in err()
    assert fwd(mean1=None) == -1 and "null output" in err()
    assert fwd(eps1=0.0) == -1 and "eps must be > 0" in err()
    assert fwd(w1=None) == -1 and "null argument" in err()
    assert bwd(dout=None) == -1 and "null dout" in err()
    assert bwd(dw1=None) == -1 and "null gradient output" in err()

    def rs(**kw):
        a = dict(mean=p, var=p, c=32, mom=0.01, counts=p, n_seg=2, stride=64, P=20, rm=p, rv=p, nbt=p)
        a.update(kw)
        return L.fd_pillar_train_running_stats_dev(a["mean"], a["var"], a["c"], a["mom"], a["counts"], a["n_seg"], a["stride"], a["P"], a["rm"],
                                                   a["rv"], a["nbt"], None)

    fn = "fd_pillar_train_running_stats_dev"
    for key in ("mean", "var", "counts", "rm", "rv"):
        assert rs(**{key: None}) == -1 and fn + ": null argument" in err(), key
    assert rs(c=0) == -1 and "channels" in err()
    for mom in (-0.1, 1.5, float("nan")):
        assert rs(mom=mom) == -1 and "momentum" in err(), mom
    for n_seg in (0, 17):
        assert rs(n_seg=n_seg) == -1 and "n_seg" in err()
    assert rs(stride=0) == -1 and "seg_stride" in err()
    assert rs(P=33) == -1 and "max_points" in err()

    # the workspace is sized by the capacity, with room for the most live blocks any count below it can give (16 pillars a block)
    assert L.fd_pillar_train_workspace_bytes(18000, 20) >= 1024 * (32 + 32 + 32 * 16 + 64 * 64) * 4


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    z = torch.zeros
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.pillar_train_forward_dev(z(2, 8, 20, 5), z(2, 8, dtype=torch.int32), z(2, 8, 4, dtype=torch.int32), z(2, dtype=torch.int32),
                                         (0.2, 0.2, 0.1, 0.1), z(32, 10), z(32), z(32), 1e-3, z(64, 64), z(64), z(64), 1e-3)
    with pytest.raises(hip_ops.FutureDetHipError, match="HIP device"):
        hip_ops.pillar_train_running_stats_dev(z(32), z(32), 0.01, z(2, dtype=torch.int32), 8, 20, z(32), z(32))
    with pytest.raises(NotImplementedError, match="momentum=None"):
        hip_ops.pillar_train_running_stats_dev(z(32), z(32), None, z(2, dtype=torch.int32), 8, 20, z(32), z(32))


def test_momentum_none_is_refused_on_the_static_reader_path():
    from futuredet_amd.readers import PillarFeatureNet

    net = PillarFeatureNet(num_input_features=5, num_filters=[64, 64], norm_cfg=dict(type="BN1d", eps=1e-3, momentum=None)).train()
    assert net.pfn_layers[0].norm.momentum is None
    with pytest.raises(NotImplementedError, match="momentum=None"):
        net.forward_train_static(torch.zeros(2, 8, 20, 5), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8, 4, dtype=torch.int32),
                                 torch.zeros(2, dtype=torch.int32))
    ok = PillarFeatureNet(num_input_features=5, num_filters=[64, 64]).train()
    with pytest.raises(ValueError, match="counts"):
        ok.forward_train_static(torch.zeros(2, 8, 20, 5), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8, 4, dtype=torch.int32),
                                torch.zeros(3, dtype=torch.int32))


def _pointpillars():
    from futuredet_amd import build_detector
    from futuredet_amd.configs import pointpillars_config
    from futuredet_amd.targets import TargetAssigner

    cfg = pointpillars_config()
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    ta = TargetAssigner(cfg.train_cfg.assigner, np.array([512, 512, 1]), vg["range"], vg["voxel_size"])
    return net, vg, ta


def _voxelnet(variant):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.targets import TargetAssigner

    cfg = centerpoint_config(variant)
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    ta = TargetAssigner(cfg.train_cfg.assigner, np.array([1440, 1440, 40]), vg["range"], vg["voxel_size"])
    return net, vg, ta


def test_pillars_step_constructor_names_what_is_missing():
    """every refusal comes before any device work: the models live on the CPU and no optimiser exists"""
    pp, vg, ta = _pointpillars()
    assert pp.bbox_head.fused_loss is False
    with pytest.raises(ValueError, match=r"bbox_head\.fused_loss"):
        solver.StaticPillarsTrainStep(pp, vg, ta, None, capacity=1000)
    pp.bbox_head.fused_loss = True
    with pytest.raises(NotImplementedError, match="graph=True"):
        solver.StaticPillarsTrainStep(pp, vg, ta, None, capacity=1000, graph=True)
    with pytest.raises(NotImplementedError, match="norm_type"):
        solver.StaticPillarsTrainStep(pp, vg, ta, None, grad_clip=dict(max_norm=35, norm_type=1), capacity=1000)
    with pytest.raises(ValueError, match="1 to 16 clouds"):
        solver.StaticPillarsTrainStep(pp, vg, ta, None, capacity=1000, batch_size=17)
    step = solver.StaticPillarsTrainStep(pp, vg, ta, None, capacity=1000, batch_size=2)
    assert step.overflowed() is False and step.bev is None and tuple(step.points.shape) == (2, 1000, 5)

    vn, vg2, ta2 = _voxelnet("forecast_n0")
    vn.backbone.fused_bn, vn.bbox_head.fused_loss = True, True
    with pytest.raises(NotImplementedError, match="not a PointPillars"):
        solver.StaticPillarsTrainStep(vn, vg2, ta2, None, capacity=1000)
    # and the sparse-backbone step still refuses PointPillars, naming the class that takes it
    with pytest.raises(NotImplementedError, match="PointPillars.*StaticPillarsTrainStep"):
        solver.StaticTrainStep(pp, vg, ta, None, capacity=1000)


def test_static_train_step_takes_a_map_head():
    net, vg, ta = _voxelnet("forecast_n3dtfm")
    assert net.bbox_head.bev_map is True
    net.backbone.fused_bn, net.bbox_head.fused_loss = True, True
    step = solver.StaticTrainStep(net, vg, ta, None, capacity=1000, batch_size=2)
    assert tuple(step.bev.shape) == (2, 6, ta.H, ta.W) and step.bev.dtype == torch.float32
    plain, vg0, ta0 = _voxelnet("forecast_n0")
    plain.backbone.fused_bn, plain.bbox_head.fused_loss = True, True
    assert solver.StaticTrainStep(plain, vg0, ta0, None, capacity=1000).bev is None
    # the training path asks for the map instead of refusing the head
    net.train()
    with pytest.raises(ValueError, match="needs the map"):
        net.forward_points_train([torch.zeros(4, 5)], vg, {})
