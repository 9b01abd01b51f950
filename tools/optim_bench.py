"""Times one optimiser step of the shipped training recipe on the parameter sets of forecast_n0 and forecast_n3dtf with random
gradients: futuredet_amd.solver.FusedAdam (fd_optim.hip) against the reference recipe restated in torch on the same device
(tests/solver_util.TorchRecipe: per-parameter ``mul_(1 - wd * lr)``, ``clip_grad_norm_``, torch.optim.Adam with its defaults over
the same two groups).  Both sides include the OneCycle schedule step and gradient clipping at max_norm 35.

Method: warm-up, then ``--runs`` (>= 20) windows per side, the two sides alternating; a window is ``--iters`` optimiser steps between
two device synchronisations on the host clock, so it holds the launches AND the host work that issues them, which is what a
training loop waits for.  The median window over its step count is reported, with the spread.  The fused side's enqueue time (the
same window without the final synchronise) shows how far the host runs ahead.  Also prints the parity figures of
tests/test_gpu_solver.py (the fixture's six-step trajectory against the float64 reference run).

    python tools/optim_bench.py [--out profiles/optim_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from futuredet_amd import build_detector, solver  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from solver_util import GRAD_CLIP, TorchRecipe, Trajectory  # noqa: E402

DEV = "cuda:0"
LR_CONFIG = dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)


def window(step, iters, first_iter, sync=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first_iter, first_iter + iters):
        step(i)
    if sync:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt / iters * 1e6


def bench_model(variant, runs, iters, warmup, lines):
    cfg = centerpoint_config(variant)
    total = (runs * 3 + warmup) * iters + 16
    sides = {}
    for side in ("fused", "torch"):
        torch.manual_seed(0)
        net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg).to(DEV)
        groups = solver.parameter_groups(net)
        gen = torch.Generator().manual_seed(1)
        grads = [torch.randn(p.shape, generator=gen).to(DEV) for g in groups for _, p in g]
        if side == "fused":
            opt = solver.FusedAdam(groups, wd=0.01)
            opt.zero_grad()
            for p, g in zip(opt.params, grads):
                p.grad.add_(g)
        else:
            opt = TorchRecipe([[p for _, p in g] for g in groups], 0.01)
            for p, g in zip(opt.params, grads):
                p.grad = g.clone()
        sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, total)

        def step(i, opt=opt, sched=sched):
            sched.step(i)
            opt.step(grad_clip=GRAD_CLIP)

        sides[side] = (net, opt, step)
    n_tensors = len(sides["fused"][1].params)
    n_elems = sum(p.numel() for p in sides["fused"][1].params)
    it = 0
    for _ in range(warmup):
        for side in sides:
            window(sides[side][2], iters, it)
        it += iters
    t = {"fused": [], "torch": [], "fused enqueue": []}
    for _ in range(runs):
        for side in ("fused", "torch"):  # alternating: drifts of the host hit both
            t[side].append(window(sides[side][2], iters, it))
        it += iters
        t["fused enqueue"].append(window(sides["fused"][2], iters, it, sync=False))
        it += iters
    lines.append("%s: %d tensors, %d elements; %d windows of %d steps per side after %d warm-up windows" % (variant, n_tensors, n_elems, runs, iters, warmup))
    for k in ("fused", "torch", "fused enqueue"):
        a = np.asarray(t[k])
        lines.append("  %-14s median %9.1f us/step   min %9.1f   max %9.1f" % (k, np.median(a), a.min(), a.max()))
    ratio = float(np.median(t["torch"]) / np.median(t["fused"]))
    # bytes the fused step must move: p, m, v read and written, g read twice (norm pass, step pass)
    mb = n_elems * 4 * 8 / 1e6
    lines.append("  torch / fused = %.1fx;  fused step moves %.0f MB (p, m, v in and out, g twice): %.0f GB/s over the whole window (host work included;"
                 " kernel time alone: not measured)" % (ratio, mb, mb / 1e3 / (np.median(t["fused"]) * 1e-6)))
    return ratio


def parity(lines):
    import test_gpu_solver as tg  # the GPU test's own replay and rule

    traj = Trajectory(dict(np.load(os.path.join(ROOT, "tests", "golden", "solver.npz"), allow_pickle=False)))
    traj.restated, traj.restated_norm = traj.run_restated(torch.float32)
    for label, make in (("trajectory", tg._aligned), ("4-byte aligned parameters", tg._offset_by_one)):
        _, _, snaps, norms = tg._replay(traj, make, replace_grad_of=(1, 4, 8))
        tg._check_trajectory(traj, snaps, norms, label, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.txt"))
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert args.runs >= 20, "the median is taken over at least 20 windows"
    assert torch.cuda.is_available(), "optim_bench needs the MI355X: a CPU timing says nothing about it"
    lines = ["optimiser step: FusedAdam (fd_optim.hip) vs the reference recipe restated in torch, both on %s, torch %s" % (
        torch.cuda.get_device_name(0), torch.__version__),
        "launches per fused step, counted from fd_optim_adam_step: 3 (optim_sumsq, optim_prepare, optim_step) with clipping, 2 without; zero_grad: 1",
        ""]
    ratios = [bench_model(v, args.runs, args.iters, args.warmup, lines) for v in ("forecast_n0", "forecast_n3dtf")]
    lines += ["", "parity (max error against the reference's float64 run; the bound is 4 x the fp32 torch restatement's own error, floor 1 ulp):"]
    parity(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    assert all(r >= 1.0 for r in ratios), "the fused step is slower than the torch restatement: %s" % ratios


if __name__ == "__main__":
    main()
