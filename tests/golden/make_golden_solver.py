"""Generates tests/golden/solver.npz by RUNNING the reference's own det3d/solver/fastai_optim.py (OptimWrapper) and
det3d/solver/learning_schedules_fastai.py (OneCycle), loaded by path (the only shim: collections.Iterable, which python >= 3.10
no longer has), plus the two functions flatten_model / get_layer_groups of det3d/torchie/apis/train.py, compiled from that file's
syntax tree because the file itself imports the whole dataset stack.  Nothing of the reference is copied: the fixture holds
inputs and the reference's outputs.  Run:  python tests/golden/make_golden_solver.py

Contents
  sched/<total_step>      [total_step, 2] float64: (lr, mom) that OneCycle sets at every step, shipped lr_config, total_step 3 / 10 / 57
  groups/plain, groups/bn parameter names of the two groups OptimWrapper.create builds for a toy module
  traj/...                a six-step float64 run of OptimWrapper + OneCycle + clip_grad_norm_(max_norm=35) over tensors of
                          1, 3, 4, 5, 63, 64, 65, C-1, C, C+1, 2C+1 elements (C = 4096, the kernels' chunk), spread over both groups:
    numel, group          per tensor, in optimiser order (plain group first)
    p0                    initial parameters, fp32, concatenated in that order
    grad_q, grad_scale    gradients: step s, element e = grad_q[s, e] (int8) * grad_scale[s] (a power of two): exact fp32 values whose
                          norm alternates between about 1500 (clipped) and about 5 (not clipped)
    none_tensor, none_steps  the tensor whose gradient is None in those steps
    lr, mom, total_norm   per step (float64)
    first/..., last/...   p, exp_avg, exp_avg_sq after step 0 and step 5 as <name>_hi (fp32, the rounded float64 value) and <name>_lo
                          (float16: the remainder in units of the fp32 spacing at hi, within +-0.5) -- the float64 value to 2^-12 of
                          an fp32 ulp at three quarters of the bytes; step: per-tensor Adam step counts
"""
import ast
import collections
import collections.abc
import importlib.util
import os
from functools import partial

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
CHUNK = 4096
LR_CONFIG = dict(lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
WD, MAX_NORM, STEPS = 0.01, 35, 6


def load(path, name):
    collections.Iterable = collections.abc.Iterable
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def functions_of(path, names):
    tree = ast.parse(open(os.path.join(REF, path)).read())
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = dict(nn=nn, torch=torch)
    exec(compile(tree, path, "exec"), ns)
    return [ns[n] for n in names]


class Holder(object):
    lr = mom = None


class Plain(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n, dtype=torch.float64))


class Norm(nn.modules.batchnorm._BatchNorm):  # a BatchNorm type to the reference's split, holding one tensor
    def __init__(self, n):
        nn.Module.__init__(self)
        self.weight = nn.Parameter(torch.zeros(n, dtype=torch.float64))


def split64(x):
    hi = x.astype(np.float32)
    lo = (x - hi.astype(np.float64)) / np.spacing(np.abs(hi)).astype(np.float64)
    assert np.all(np.abs(lo) <= 0.5)
    return hi, lo.astype(np.float16)


def main():
    fo = load("det3d/solver/fastai_optim.py", "ref_fastai_optim")
    ls = load("det3d/solver/learning_schedules_fastai.py", "ref_learning_schedules_fastai")
    (get_layer_groups, _) = functions_of("det3d/torchie/apis/train.py", ["get_layer_groups", "flatten_model"])
    out = {}

    for total in (3, 10, 57):
        h = Holder()
        s = ls.OneCycle(h, total, **LR_CONFIG)
        rows = []
        for i in range(total):
            s.step(i)
            rows.append((h.lr, h.mom))
        out["sched/%d" % total] = np.asarray(rows, np.float64)

    toy = nn.Module()
    toy.a = nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4))
    toy.b = nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4))
    toy.c = nn.Conv2d(4, 2, 1)
    opt = fo.OptimWrapper.create(partial(torch.optim.Adam, betas=(0.9, 0.99)), 3e-3, get_layer_groups(toy), wd=WD, true_wd=True, bn_wd=True)
    names = {id(p): n for n, p in toy.named_parameters()}
    out["groups/plain"], out["groups/bn"] = (np.asarray([names[id(p)] for p in g["params"]]) for g in opt.opt.param_groups)
    print("toy groups:", list(out["groups/plain"]), "/", list(out["groups/bn"]))

    numels = [1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    net = nn.Sequential(*[(Norm if i % 2 else Plain)(n) for i, n in enumerate(numels)])
    opt = fo.OptimWrapper.create(partial(torch.optim.Adam, betas=(0.9, 0.99), amsgrad=0.0), 3e-3, get_layer_groups(net), wd=WD, true_wd=True,
                                 bn_wd=True)
    params = [p for g in opt.opt.param_groups for p in g["params"]]
    group = [gi for gi, g in enumerate(opt.opt.param_groups) for _ in g["params"]]
    assert len(opt.opt.param_groups) == 2 and len(params) == len(numels) and 0 < sum(group) < len(group)
    nel = [p.numel() for p in params]
    none_tensor, none_steps = nel.index(CHUNK + 1), (2, 3)
    rng = np.random.default_rng(20261019)
    p0 = (rng.standard_normal(sum(nel)) * 0.1).astype(np.float32)
    q = np.clip(np.rint(rng.standard_normal((STEPS, sum(nel))) * 40.0), -127, 127).astype(np.int8)
    scale = np.asarray([2.0 ** -2 if s % 2 == 0 else 2.0 ** -10 for s in range(STEPS)], np.float32)
    off = np.concatenate([[0], np.cumsum(nel)])
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(torch.from_numpy(p0[off[i]:off[i + 1]].astype(np.float64)))
    sched = ls.OneCycle(opt, STEPS, **LR_CONFIG)
    lr, mom, norms = [], [], []

    def snapshot(tag):
        for name, get in (("p", lambda p: p.detach()), ("exp_avg", lambda p: opt.opt.state[p]["exp_avg"]), ("exp_avg_sq", lambda p: opt.opt.state[p]["exp_avg_sq"])):
            hi, lo = split64(np.concatenate([get(p).numpy().ravel() for p in params]))
            out["traj/%s/%s_hi" % (tag, name)], out["traj/%s/%s_lo" % (tag, name)] = hi, lo
        out["traj/%s/step" % tag] = np.asarray([int(opt.opt.state[p]["step"]) for p in params], np.int32)

    for s in range(STEPS):
        sched.step(s)
        lr.append(opt.lr), mom.append(opt.mom)
        opt.zero_grad()
        for i, p in enumerate(params):
            if i == none_tensor and s in none_steps:
                p.grad = None
            else:
                p.grad = torch.from_numpy((q[s, off[i]:off[i + 1]].astype(np.float32) * scale[s]).astype(np.float64))
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm=MAX_NORM, norm_type=2)))
        opt.step()
        if s == 0:
            snapshot("first")
    snapshot("last")
    print("total_norm per step:", ["%.4g" % n for n in norms], " steps:", list(out["traj/last/step"]))
    assert sum(n > MAX_NORM for n in norms) == 3 and sum(n < MAX_NORM for n in norms) == 3
    out.update({"traj/numel": np.asarray(nel, np.int64), "traj/group": np.asarray(group, np.int32), "traj/p0": p0, "traj/grad_q": q,
                "traj/grad_scale": scale, "traj/none_tensor": np.int32(none_tensor), "traj/none_steps": np.asarray(none_steps, np.int32),
                "traj/lr": np.asarray(lr, np.float64), "traj/mom": np.asarray(mom, np.float64), "traj/total_norm": np.asarray(norms, np.float64),
                "traj/wd": np.float64(WD), "traj/max_norm": np.float64(MAX_NORM), "traj/chunk": np.int32(CHUNK)})
    path = os.path.join(HERE, "solver.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
