"""Training-mode BatchNorm2d + ReLU on bf16 channels-last maps (mixed precision, train_dtype = torch.bfloat16): the fused kernels of
fd_row_bn.h behind fd_dense_bn_nhwc.hip (dense_bn.batch_norm2d_act_nhwc, fused_bn on) against the un-fused recipe they replace
(bn(x.float()), ReLU and one rounding as separate passes, fused_bn off), both sides in one process, alternating inside one timing loop.

Every figure is device time between two events around forward + backward, the median of ``--iters`` samples after a warm-up, with
the spread (min .. max) of each side.  The fused side counts as faster only where the gap between the medians exceeds the spread of the
un-fused side; every other row is marked.

  1. each shipped BatchNorm shape at B = 2: 128 and 256 channels at 180 x 180, 256 at 90 x 90, 64 at 180 x 180, and the six 64-channel
     branch modules of a SepHead on their 384-channel map (one grouped call against .float().split + six modules + torch.cat);
  2. the neck's forward + backward, and the CenterHead's of forecast_n0 and forecast_n3dtf, train_dtype = bf16, fused_bn off / on;
  3. one training iteration of forecast_n0 (the set-up of tools/train_step_bench.py, all three train_dtype = bf16, backbone.fused_bn on
     on both sides): solver.train_steps and solver.StaticTrainStep(check=False), neck and head fused_bn off / on; the host
     synchronisations of the static step are counted with torch's sync debug mode;
  with torch.cuda.max_memory_allocated of each side.

``--kernels N`` instead runs the fused forward + backward N times per shape and nothing else: the run to put under
``rocprofv3 --kernel-trace --stats`` for the kernels' own times; ``--bandwidth`` prints the bytes each kernel moves at those shapes.

    python tools/dense_bn_bf16_bench.py [--iters 20] [--out profiles/dense_bn_bench_bf16.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from futuredet_amd import dense_bn  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.heads import CenterHead  # noqa: E402
from futuredet_amd.necks import RPN  # noqa: E402
from futuredet_amd.sparse import relu_to_bf16  # noqa: E402
from futuredet_amd.synth import seeded_state_dict  # noqa: E402

BF = torch.bfloat16
DEV = torch.device("cuda:0")
B = 2
# (module widths, side, where)
SHAPES = [([128], 180, "RPN stage 1"), ([256], 180, "RPN deblocks"), ([256], 90, "RPN stage 2"), ([64], 180, "CenterHead shared_conv"),
          ([64] * 6, 180, "SepHead branches, grouped")]
# bytes per element of the map that each kernel reads + writes (bf16 rows)
KERNEL_BYTES = (("row_bn_stats", 2), ("row_bn_apply", 4), ("row_bn_grad_sums", 6), ("row_bn_grad_apply", 8))


def timed_each(fns, iters, warmup=3):
    """device time in microseconds of every callable of ``fns`` (a dict), alternating inside one loop -> {key: samples}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1000.0)
    return {k: np.asarray(v) for k, v in ts.items()}


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def row(name, ts, peaks, unit=1.0, what="us"):
    """one table row from the samples {False: un-fused, True: fused}"""
    off, on = ts[False] / unit, ts[True] / unit
    gap, spread = float(np.median(off) - np.median(on)), float(off.max() - off.min())
    verdict = "faster" if gap > spread else "NOT faster (the gap does not exceed the un-fused side's spread)"
    return ("%-44s un-fused %9.1f %s (%.1f .. %.1f)  fused %9.1f %s (%.1f .. %.1f)  x%.2f  peak MiB %8.1f -> %8.1f   %s"
            % (name, np.median(off), what, off.min(), off.max(), np.median(on), what, on.min(), on.max(), np.median(off) / np.median(on),
               peaks[False], peaks[True], verdict))


def shape_problem(widths, side):
    C = sum(widths)
    g = torch.Generator(device="cpu").manual_seed(C + side)
    x = (torch.randn((B, side, side, C), generator=g) * 0.5 + 0.1).to(DEV).to(BF).permute(0, 3, 1, 2).requires_grad_(True)
    dy = torch.randn((B, side, side, C), generator=g).to(DEV).to(BF).permute(0, 3, 1, 2)
    bns = [nn.BatchNorm2d(c, eps=1e-3, momentum=0.01).to(DEV).train() for c in widths]
    params = [p for bn in bns for p in (bn.weight, bn.bias)]

    def run(fused):
        if fused:
            y = dense_bn.batch_norm2d_act_nhwc(x, bns if len(bns) > 1 else bns[0], relu=True)
        elif len(bns) == 1:
            y = relu_to_bf16(bns[0](x.float()))
        else:  # what sep_head_bf16 does without the switch; the cat stands for the six inputs of the final convolutions
            y = torch.cat([relu_to_bf16(bn(p)) for bn, p in zip(bns, x.float().split(widths[0], dim=1))], dim=1)
        return torch.autograd.grad(y, [x] + params, dy)

    return run


def per_shape(args, lines):
    lines.append("1. BatchNorm2d + ReLU forward + backward per shape, B = %d" % B)
    for widths, side, where in SHAPES:
        run = shape_problem(widths, side)
        ts = timed_each({f: (lambda f=f: run(f)) for f in (False, True)}, args.iters)
        peaks = {f: peak_of(lambda f=f: run(f)) for f in (False, True)}
        lines.append(row("%d x %d x %d x %d  %s" % (B, sum(widths), side, side, where), ts, peaks))
        del run
        torch.cuda.empty_cache()


def dense_parts(args, lines):
    lines.append("2. forward + backward of the neck and of the CenterHead, B = %d, 180 x 180, train_dtype = bf16" % B)
    for variant in ("forecast_n0", "forecast_n3dtf"):
        cfg = centerpoint_config(variant)
        nk, hd = dict(cfg.model["neck"]), dict(cfg.model["bbox_head"])
        nk.pop("type"), hd.pop("type")
        torch.manual_seed(0)
        parts = [("CenterHead " + variant, CenterHead(**hd), hd["in_channels"], 4)]
        if variant == "forecast_n0":
            parts.insert(0, ("RPN", RPN(**nk), nk["num_input_features"], 3))
        for name, mod, cin, seed in parts:
            mod.load_state_dict(seeded_state_dict(mod, seed), strict=False)
            mod = mod.to(DEV).train()
            mod.train_dtype = BF
            g = torch.Generator(device="cpu").manual_seed(11)
            xin = torch.randn((B, cin, 180, 180), generator=g).to(DEV)
            weights = {}

            def step(fused, mod=mod, xin=xin, weights=weights):
                mod.fused_bn = fused
                mod.zero_grad(set_to_none=True)
                out = mod(xin)
                maps = [out] if isinstance(out, torch.Tensor) else [p[k] for p in out for k in sorted(p) if k != "feats"]
                loss = 0.0
                for i, m in enumerate(maps):
                    if i not in weights:
                        weights[i] = torch.randn_like(m)
                    loss = loss + (m * weights[i]).sum()
                loss.backward()

            ts = timed_each({f: (lambda f=f: step(f)) for f in (False, True)}, args.iters)
            peaks = {f: peak_of(lambda f=f: step(f)) for f in (False, True)}
            lines.append(row(name, ts, peaks, 1000.0, "ms"))
            del mod, xin, weights, step
            torch.cuda.empty_cache()


def train_step(args, lines):
    import warnings

    import train_step_bench as tsb
    from futuredet_amd import build_detector, solver
    from futuredet_amd.synth import synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel

    lines.append("3. one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, backbone, neck and head in bf16" % (B, args.points))
    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV).train()
    net.backbone.fused_bn = net.bbox_head.fused_loss = True
    net.backbone.train_dtype = net.neck.train_dtype = net.bbox_head.train_dtype = BF
    ta = TargetAssigner(cfg.train_cfg.assigner, tsb.GRID, vg["range"], vg["voxel_size"])
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=args.points)).to(DEV) for s in range(B)]
    gt = [torch.from_numpy(a).to(DEV) for a in tsb.synthetic_gt(np.random.default_rng(2), B, cfg.timesteps, 40)]
    batch = dict(clouds=clouds, gt_boxes=gt[0], gt_counts=gt[1], gt_classes=gt[2])
    vs, cs, ns = [], [], []
    for b, c in enumerate(clouds):
        v, co, n = points_to_voxel(c, vg["voxel_size"], vg["range"], int(vg["max_points_in_voxel"]), True, int(vg["max_voxel_num"][0]))
        vs.append(v), ns.append(n), cs.append(torch.nn.functional.pad(co, (1, 0), value=b))
    targets = ta(gt[0], gt[1], gt[2], None)
    ex = dict(voxels=torch.cat(vs), coordinates=torch.cat(cs), num_points=torch.cat(ns), num_voxels=torch.tensor([len(n) for n in ns]),
              shape=np.array([tsb.GRID] * B), metadata=[None] * B)
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, tsb.LR_CONFIG, 100000)
    it = [0]

    def switch(fused):
        net.neck.fused_bn = net.bbox_head.fused_bn = fused

    def eager(fused):
        switch(fused)
        for _ in solver.train_steps(net, [ex], opt, sched, grad_clip=tsb.GRAD_CLIP, start_iter=it[0]):
            it[0] += 1

    static = solver.StaticTrainStep(net, vg, ta, opt, sched, tsb.GRAD_CLIP, capacity=args.points + 50000, batch_size=B, max_gt=64)
    static.warm_up([batch])
    static(batch)  # derives the capacities

    def fixed(fused):
        switch(fused)
        static(batch, check=False)

    for name, fn in (("solver.train_steps", eager), ("StaticTrainStep(check=False)", fixed)):
        ts = timed_each({f: (lambda f=f: fn(f)) for f in (False, True)}, args.iters)
        peaks = {f: peak_of(lambda f=f: fn(f)) for f in (False, True)}
        lines.append(row(name, ts, peaks, 1000.0, "ms"))
    for fused in (False, True):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                for _ in range(3):
                    fixed(fused)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        lines.append("StaticTrainStep(check=False), neck and head fused_bn=%s: %d host synchronisations in 3 steps"
                     % (fused, sum("synchroniz" in str(w.message).lower() for w in seen)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--kernels", type=int, default=0, help="only run the fused forward + backward this many times per shape (for a kernel trace)")
    ap.add_argument("--bandwidth", action="store_true", help="only print the bytes per kernel at the shipped shapes")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bn_bench_bf16.txt"))
    args = ap.parse_args()
    if args.bandwidth:
        for widths, side, where in SHAPES:
            n, C = B * side * side, sum(widths)
            print("%d x %d rows (%s): %s" % (n, C, where, ", ".join("%s %.2f MB" % (k, b * n * C / 1e6) for k, b in KERNEL_BYTES)))
        return
    if args.kernels:
        for widths, side, where in SHAPES:
            run = shape_problem(widths, side)
            for _ in range(args.kernels):
                run(True)
            torch.cuda.synchronize()
        return
    lines = ["# tools/dense_bn_bf16_bench.py on %s, torch %s: device time between events, median of %d after a warm-up (min .. max); fused_bn "
             "off (un-fused) against on (fused), alternating in one loop" % (torch.cuda.get_device_name(0), torch.__version__, args.iters)]
    per_shape(args, lines)
    dense_parts(args, lines)
    if not args.skip_step:
        train_step(args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
