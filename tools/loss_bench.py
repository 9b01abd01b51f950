"""Times CenterHead.loss forward + backward on the head maps of forecast_n0, forecast_n3 and forecast_n3dtf (B = 4, 180 x 180,
max_objs 1000, 40 objects per step): the torch path against the fused path (``head.fused_loss = True``, fd_loss.hip), the two sides
alternating in one process on the same tensors.  The torch path is the code of the same commit with the switch off.

Method: warm-up, then ``--runs`` (>= 20) windows per side; a window is ``--iters`` steps (loss, then the gradient of the summed loss
w.r.t. every head map).  Each window is timed twice over: with device events around it (what the device spends, gaps included) and
with the host clock around a final synchronise (what a training loop waits for; the torch path is host-bound).  The median window
over its step count is reported with the spread.  Launches per step are counted with torch.profiler on one step per side (device
kernels and memcpy / memset nodes); host synchronisations with torch.cuda.set_sync_debug_mode("warn") on one step per side.

    python tools/loss_bench.py [--out profiles/loss_bench.txt]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loss_util as lu  # noqa: E402
from futuredet_amd import build_head  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402

DEV = "cuda:0"
B, H, W, M, OBJECTS = 4, 180, 180, 1000, 40


def problem(variant):
    cfg = centerpoint_config(variant)
    head = build_head(cfg.model.bbox_head).to(DEV)
    T, dense = cfg.timesteps, bool(head.dense)
    case = lu.make_case(0, B=B, H=H, W=W, M=M, T=T, dense=dense, D=10, classes=(1,), row=14, n_obj=lambda s, u, b: OBJECTS)
    ex = lu.example_of(case, DEV, torch.float32)
    leaves = [{k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in m.items()} for m in case["maps"]]
    flat = [v for m in leaves for v in m.values()]

    def step(fused):
        head.fused_loss = fused
        ret = head.loss(ex, [dict(m) for m in leaves])
        return torch.autograd.grad(sum(ret["loss"]), flat)

    return head, step, len(leaves), T


def window(step, fused, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        step(fused)
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / iters * 1e6
    return e0.elapsed_time(e1) / iters * 1e3, host


def count_launches(step, fused):
    """device activities (kernels, copies, memsets) of one step, or None when the profiler cannot be had"""
    try:
        from torch.profiler import ProfilerActivity, profile

        step(fused)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(fused)
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else None
    except Exception as e:  # noqa: BLE001
        print("launch count: profiler unavailable (%s)" % e)
        return None


def count_syncs(step, fused):
    step(fused)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            step(fused)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in seen if "synchroniz" in str(w.message))


def bench(variant, runs, iters, warmup, lines, table):
    head, step, n_tasks, T = problem(variant)
    for _ in range(warmup):
        for fused in (True, False):
            window(step, fused, iters)
    t = {True: [], False: []}
    for _ in range(runs):
        for fused in (True, False):  # alternating: drifts of the host and the clocks hit both
            t[fused].append(window(step, fused, iters))
    launches = {f: count_launches(step, f) for f in (True, False)}
    syncs = {f: count_syncs(step, f) for f in (True, False)}
    head.fused_loss = False
    lines.append("%s: %d task(s), T = %d, B = %d, %d x %d, max_objs %d, %d objects per step; %d windows of %d steps per side after %d warm-up windows"
                 % (variant, n_tasks, T, B, H, W, M, OBJECTS, runs, iters, warmup))
    med = {}
    for fused, label in ((False, "torch"), (True, "fused")):
        a = np.asarray(t[fused])
        med[fused] = np.median(a, axis=0)
        lines.append("  %-6s device events: median %9.1f us/step  min %9.1f  max %9.1f   host clock + synchronise: median %9.1f us/step  min %9.1f  max %9.1f"
                     % (label, med[fused][0], a[:, 0].min(), a[:, 0].max(), med[fused][1], a[:, 1].min(), a[:, 1].max()))
        lines.append("  %-6s device activities per step (kernels, copies, memsets; torch's own ops around the kernels included): %s;  host synchronisations per step: %d"
                     % (label, launches[fused] if launches[fused] is not None else "not measured", syncs[fused]))
    lines.append("  torch / fused = %.1fx (device events), %.1fx (host clock)" % (med[False][0] / med[True][0], med[False][1] / med[True][1]))
    table.append("| %s | %.0f | %.0f | %.0f | %.0f | %s | %s | %d | %d |" % (
        variant, med[False][0], med[True][0], med[False][1], med[True][1], launches[False] if launches[False] is not None else "not measured",
        launches[True] if launches[True] is not None else "not measured", syncs[False], syncs[True]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--variants", default="forecast_n0,forecast_n3,forecast_n3dtf")
    args = ap.parse_args()
    assert args.runs >= 20, "the median is taken over at least 20 windows"
    assert torch.cuda.is_available(), "loss_bench needs the MI355X: a CPU timing says nothing about it"
    lines = ["CenterHead.loss forward + backward: the torch path vs fused_loss = True (fd_loss.hip), both on %s, torch %s" % (
        torch.cuda.get_device_name(0), torch.__version__),
        "launches of the library per fused step: fd_centerhead_loss_forward 2 (loss_partials, loss_finish), fd_centerhead_loss_backward 2 "
        "(loss_grad_objects, loss_grad_maps); 3 each for more than 8 tasks", ""]
    table = ["| head | torch, device us | fused, device us | torch, host us | fused, host us | torch activities | fused activities | torch syncs | fused syncs |",
             "|---|---|---|---|---|---|---|---|---|"]
    for v in args.variants.split(","):
        bench(v, args.runs, args.iters, args.warmup, lines, table)
    text = "\n".join(lines + [""] + table) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
