"""Times one training iteration of forecast_n0 at B = 2 on the bench's synthetic clouds (synth.synthetic_cloud, 300 000 points, the
shipped voxel caps), fp32 and bf16 rows, two ways:

    eager        solver.train_steps on the collated example of the same clouds (voxelised ahead of the clock)
    static       solver.StaticTrainStep: the same launches with every count on the device, nothing waits for the host

(The step replayed as one hipGraph is not measured: StaticTrainStep has no capture, see its docstring.)  Both run with fused_bn and
fused_loss, OneCycle and clipping at max_norm 35.  A sample is one iteration between two device
synchronisations on the host clock (launches and the host work that issues them); the median of ``--runs`` samples is reported with
the spread.  Host synchronisations per step are counted with torch's sync debug mode ("warn": one warning per blocking call) over a
few extra iterations; the static step is run with check=True, so its one read-back of the level counts is in the time and in the
count, and once more with check=False.  No threshold: the file is the record.

    python tools/train_step_bench.py [--out profiles/static_train_step.txt]
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

from futuredet_amd import build_detector, solver  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims  # noqa: E402
from futuredet_amd.targets import TargetAssigner  # noqa: E402
from futuredet_amd.voxelize import points_to_voxel  # noqa: E402

DEV = torch.device("cuda:0")
LR_CONFIG = dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
GRAD_CLIP = dict(max_norm=35, norm_type=2)
GRID = np.array([1440, 1440, 40])


def synthetic_gt(rng, B, T, n):
    boxes = np.zeros((B, T, n, 12), np.float32)
    boxes[..., 0:2] = rng.uniform(-40.0, 40.0, (B, T, n, 2))
    boxes[..., 2] = rng.normal(-0.5, 0.3, (B, T, n))
    boxes[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * rng.uniform(0.8, 1.2, (B, T, n, 3))
    boxes[..., 6:10] = rng.normal(0.0, 2.0, (B, T, n, 4))
    boxes[..., 10:12] = rng.uniform(-np.pi, np.pi, (B, T, n, 2))
    return boxes, np.full((B, T), n, np.int32), np.ones((B, T, n), np.int32)


def timed(fn, runs):
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.asarray(out)


def syncs_per_step(fn, n=3):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for _ in range(n):
                fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(w.message).lower() for w in seen) / float(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_train_step.txt"))
    args = ap.parse_args()
    B = args.batch
    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV).train()
    net.backbone.fused_bn = True
    net.bbox_head.fused_loss = True
    ta = TargetAssigner(cfg.train_cfg.assigner, GRID, vg["range"], vg["voxel_size"])
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=args.points)).to(DEV) for s in range(B)]
    gt = [torch.from_numpy(a).to(DEV) for a in synthetic_gt(np.random.default_rng(2), B, cfg.timesteps, 40)]
    batch = dict(clouds=clouds, gt_boxes=gt[0], gt_counts=gt[1], gt_classes=gt[2])
    # the collated example of the eager loop
    vs, cs, ns = [], [], []
    for b, c in enumerate(clouds):
        v, co, n = points_to_voxel(c, vg["voxel_size"], vg["range"], int(vg["max_points_in_voxel"]), True, int(vg["max_voxel_num"][0]))
        vs.append(v), ns.append(n), cs.append(torch.nn.functional.pad(co, (1, 0), value=b))
    targets = ta(gt[0], gt[1], gt[2], None)
    ex = dict(voxels=torch.cat(vs), coordinates=torch.cat(cs), num_points=torch.cat(ns), num_voxels=torch.tensor([len(n) for n in ns]),
              shape=np.array([GRID] * B), metadata=[None] * B)
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    total = 100000
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, total)
    lines = ["one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, %s, torch %s" % (
        B, args.points, torch.cuda.get_device_name(0), torch.__version__),
        "median of %d samples, ms per step (min .. max); host synchronisations per step from torch's sync debug mode" % args.runs, ""]
    for dtype, tag in ((torch.float32, "fp32 rows"), (torch.bfloat16, "bf16 rows")):
        net.backbone.train_dtype = dtype
        it = [0]

        def eager():
            for _ in solver.train_steps(net, [ex], opt, sched, grad_clip=GRAD_CLIP, start_iter=it[0]):
                it[0] += 1

        rows = [("eager  solver.train_steps", eager)]
        static = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, capacity=args.points + 50000, batch_size=B, max_gt=64)
        static.warm_up([batch])
        rows.append(("static StaticTrainStep", lambda: static(batch)))
        static(batch)  # derives the capacities
        lines.append("%s (level counts of the batch %s, capacities %s)" % (tag, static.expected, static.caps))
        for name, fn in rows:
            for _ in range(args.warmup):
                fn()
            t = timed(fn, args.runs)
            n_sync = syncs_per_step(fn)
            lines.append("  %-38s %8.2f ms  (%.2f .. %.2f)   %4.1f host synchronisations per step" % (name, np.median(t), t.min(), t.max(), n_sync))
        t = timed(lambda: static(batch, check=False), args.runs)
        lines.append("  %-38s %8.2f ms  (%.2f .. %.2f)   check=False: no read-back, the sample ends at the synchronise" % (
            "static, check=False", np.median(t), t.min(), t.max()))
        lines.append("")
        del static
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
