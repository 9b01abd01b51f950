"""Host side of futuredet_amd.solver (no GPU): the one-cycle schedule and the parameter groups against what the reference's own
code produced (tests/golden/solver.npz, make_golden_solver.py), the fd_optim_* C ABI and its argument checks, and the options the
fused step refuses."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from futuredet_amd import lib, solver
from futuredet_amd.lib import FutureDetHipError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR_CONFIG = dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)


class _Holder(object):
    lr = mom = None


@pytest.mark.parametrize("total_step", [3, 10, 57])
def test_one_cycle_reproduces_the_reference_tables(golden, total_step):
    want = golden("solver.npz")["sched/%d" % total_step]
    h = _Holder()
    s = solver.create_learning_rate_scheduler(h, LR_CONFIG, total_step)
    assert isinstance(s, solver.OneCycle) and (h.lr, h.mom) == (0.001 / 10.0, 0.95)
    got = []
    for i in range(total_step):
        s.step(i)
        got.append((h.lr, h.mom))
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape and np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("total_step", [1, 2])
def test_one_cycle_refuses_a_run_whose_second_phase_starts_at_zero(total_step):
    with pytest.raises(AssertionError):
        solver.OneCycle(_Holder(), total_step, 0.001, [0.95, 0.85], 10.0, 0.4)


def test_scheduler_builder_names_an_unknown_type():
    with pytest.raises(NotImplementedError, match="exponential_decay"):
        solver.create_learning_rate_scheduler(_Holder(), dict(type="exponential_decay"), 10)


def test_groups_of_the_toy_module_follow_the_reference(golden):
    g = golden("solver.npz")
    toy = nn.Module()
    toy.a = nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4))
    toy.b = nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4))
    toy.c = nn.Conv2d(4, 2, 1)
    plain, bn = solver.parameter_groups(toy)
    assert [n for n, _ in plain] == list(g["groups/plain"]) and [n for n, _ in bn] == list(g["groups/bn"])
    named = dict(toy.named_parameters())
    assert all(named[n] is p for n, p in plain + bn)
    toy.a[0].weight.requires_grad_(False)  # only trainable parameters are grouped
    assert [n for n, _ in solver.parameter_groups(toy)[0]] == list(g["groups/plain"])[1:]


@pytest.mark.parametrize("variant,tensors,bn_tensors", [("forecast_n0", 161, 84), ("forecast_n3dtf", 433, 184)])
def test_groups_of_the_shipped_models(variant, tensors, bn_tensors):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config

    cfg = centerpoint_config(variant)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    plain, bn = solver.parameter_groups(net)
    assert (len(plain) + len(bn), len(bn)) == (tensors, bn_tensors)
    trainable = [p for p in net.parameters() if p.requires_grad]
    assert {id(p) for _, p in plain + bn} == {id(p) for p in trainable}, "every trainable parameter sits in a leaf module"
    assert all(p.dim() == 1 for _, p in bn)


def test_optim_layout_segments_and_chunks():
    from futuredet_amd import hip_ops

    C = 4096
    numels = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 1]
    offsets, total, chunks = hip_ops.optim_layout(numels, C)
    assert all(o % 4 == 0 for o in offsets) and offsets[0] == 0
    assert all(offsets[i + 1] - offsets[i] == (n + 3) // 4 * 4 for i, n in enumerate(numels[:-1])) and total == offsets[-1] + (numels[-1] + 3) // 4 * 4
    cover = [0] * len(numels)
    for t, k in chunks:
        assert k * C < numels[t]
        cover[t] += min(C, numels[t] - k * C)
    assert cover == numels and len(chunks) == 5 + 1 + 2 + 3
    with pytest.raises(ValueError):
        hip_ops.optim_layout([4, 0], C)


def test_optim_abi_is_declared_bound_and_exported():
    from futuredet_amd import build

    build.build()
    L = lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "futuredet_hip.h")).read(), flags=re.S)
    names = {"fd_optim_chunk", "fd_optim_zero_grad", "fd_optim_adam_step"}
    assert names <= set(re.findall(r"\b(fd_[a-z0-9_]+)\s*\(", hdr)) and names <= set(lib.SIGNATURES)
    assert "fd_optim.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["fd_optim.hip"]
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert names <= set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION
    assert L.fd_optim_chunk() == 4096 == int(re.search(r"#define FD_OPTIM_CHUNK (\d+)", hdr).group(1))


def test_optim_table_mirrors_the_header(tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "futuredet_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct fd_optim_table \{(.*?)\} fd_optim_table;", hdr, flags=re.S).group(1)
    members = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert [n for n, _ in lib.OptimTable._fields_] == members
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "futuredet_hip.h"\nint main(void) { printf("%zu\\n", sizeof(fd_optim_table)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    assert int(subprocess.check_output([exe]).decode()) == ctypes.sizeof(lib.OptimTable)


def _table(**over):
    """a table whose pointers are non-null but never dereferenced: every call below must fail on the host"""
    fake = 0x1000
    kw = dict({n: fake for n, t in lib.OptimTable._fields_ if t is ctypes.c_void_p}, total=64, n_tensors=2, n_chunks=2, chunk=4096)
    kw.update(over)
    return lib.OptimTable(**kw)


@pytest.mark.parametrize("over,text", [(dict(params=None), "null table member"), (dict(norm=None), "null table member"),
                                       (dict(exp_avg=None), "null flat buffer"), (dict(n_tensors=0), "must be positive"),
                                       (dict(n_chunks=-1), "must be positive"), (dict(total=0), "must be positive"),
                                       (dict(chunk=1024), "chunk size 1024"), (dict(n_chunks=1), "cannot cover"),
                                       (dict(grad=0x1004), "16-byte aligned")])
def test_optim_entry_points_reject_bad_tables_on_the_host(over, text):
    L = lib.load()
    t = _table(**over)
    for rc in (L.fd_optim_adam_step(ctypes.byref(t), 1e-3, 0.9, 0.99, 1e-8, 0.01, 35.0, None), L.fd_optim_zero_grad(ctypes.byref(t), None)):
        assert rc == -1 and text in L.fd_last_error().decode(), L.fd_last_error()


def test_optim_entry_points_reject_null_and_bad_scalars():
    L = lib.load()
    assert L.fd_optim_adam_step(None, 1e-3, 0.9, 0.99, 1e-8, 0.01, 35.0, None) == -1 and b"null table" in L.fd_last_error()
    assert L.fd_optim_zero_grad(None, None) == -1 and b"fd_optim_zero_grad: null table" in L.fd_last_error()
    t = _table()
    assert L.fd_optim_adam_step(ctypes.byref(t), 1e-3, 1.0, 0.99, 1e-8, 0.01, 35.0, None) == -1 and b"betas" in L.fd_last_error()
    assert L.fd_optim_adam_step(ctypes.byref(t), 1e-3, 0.9, 0.99, 0.0, 0.01, 35.0, None) == -1 and b"eps" in L.fd_last_error()
    assert L.fd_optim_adam_step(ctypes.byref(t), float("nan"), 0.9, 0.99, 1e-8, 0.01, 35.0, None) == -1 and b"NaN" in L.fd_last_error()
    with pytest.raises(FutureDetHipError, match="null table member"):
        lib.check(L.fd_optim_zero_grad(ctypes.byref(_table(flags=None)), None), "fd_optim_zero_grad")


def test_fused_adam_has_no_cpu_path():
    net = nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4))
    with pytest.raises(FutureDetHipError, match="no CPU implementation"):
        solver.FusedAdam.for_model(net)
    with pytest.raises(FutureDetHipError, match="no CPU implementation"):
        solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    with pytest.raises(ValueError, match="no parameters"):
        solver.FusedAdam([[], []])


def test_unsupported_options_are_named():
    net = nn.Linear(2, 2)
    assert solver.parse_grad_clip(None) == 0.0 and solver.parse_grad_clip(dict(max_norm=35, norm_type=2)) == 35.0
    with pytest.raises(NotImplementedError, match="norm_type"):
        solver.parse_grad_clip(dict(max_norm=35, norm_type=1))
    with pytest.raises(NotImplementedError, match="norm_type"):
        solver.parse_grad_clip(dict(max_norm=35, norm_type="inf"))
    with pytest.raises(ValueError, match="max_norm"):
        solver.parse_grad_clip(dict(max_norm=0, norm_type=2))
    with pytest.raises(NotImplementedError, match="fixed_wd"):
        solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=False))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=1.0, wd=0.01, fixed_wd=True))
    with pytest.raises(NotImplementedError, match="type"):
        solver.build_one_cycle_optimizer(net, dict(type="sgd", wd=0.01, fixed_wd=True))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        solver.FusedAdam([[net.weight], []], amsgrad=True)
    with pytest.raises(NotImplementedError, match="true_wd"):
        solver.FusedAdam([[net.weight], []], true_wd=False)
    with pytest.raises(NotImplementedError, match="SGD"):
        solver.FusedAdam.create(torch.optim.SGD, 3e-3, [net], wd=0.01, true_wd=True)


def test_det3d_solver_aliases_resolve():
    from futuredet_amd import compat

    assert compat.install_det3d_alias()
    from det3d.solver.fastai_optim import OptimWrapper
    from det3d.solver.learning_schedules_fastai import OneCycle

    assert OptimWrapper is solver.FusedAdam and OneCycle is solver.OneCycle
    assert callable(OptimWrapper.create)
    for name in ("optim_zero_grad", "optim_adam_step", "AdamTable", "optim_layout"):
        from futuredet_amd import hip_ops

        assert hasattr(hip_ops, name), name
