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

``--config pointpillars`` and ``--config forecast_n3dtfm`` time the two steps this tool did not cover -- solver.StaticPillarsTrainStep
(PointPillars; the eager example is the device voxeliser's own output) and solver.StaticTrainStep with the map input of a bev_map
head -- against solver.train_steps on the same weights in ONE alternating loop (eager, static, eager, static, ...), so drift of the
clock or the machine lands on both sides alike; the eager side's own spread is printed next to the medians.

    python tools/train_step_bench.py --config pointpillars --config forecast_n3dtfm --out profiles/static_train_step_pillars.txt
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


def _world(config, B, points):
    """model, voxel config, assigner, the batch of the static step and the collated example of the eager loop for ``config``"""
    from futuredet_amd import hip_ops
    from futuredet_amd.configs import pointpillars_config

    pillars = config == "pointpillars"
    cfg = pointpillars_config() if pillars else centerpoint_config(config)
    vg = cfg.voxel_generator
    grid = np.array([512, 512, 1]) if pillars else GRID
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = tame_box_dims(seeded_state_dict(net, 7))
    if pillars:
        sd["reader.pfn_layers.0.linear.weight"] = sd["reader.pfn_layers.0.linear.weight"] * 0.02  # raw coordinates of a 100 m scene
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    if not pillars:
        net.backbone.fused_bn = True
    net.bbox_head.fused_loss = True
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=points)).to(DEV) for s in range(B)]
    rng = np.random.default_rng(2)
    gt = [torch.from_numpy(a).to(DEV) for a in synthetic_gt(rng, B, cfg.timesteps, 40)]
    batch = dict(clouds=clouds, gt_boxes=gt[0], gt_counts=gt[1], gt_classes=gt[2])
    if ta.extra_sets:
        batch["gt_trajectory"] = torch.from_numpy(rng.integers(0, 3, (B, cfg.timesteps, 40)).astype(np.int32)).to(DEV)
    cap, mp = int(vg["max_voxel_num"][0]), int(vg["max_points_in_voxel"])
    vs, cs, ns = [], [], []
    for b, c in enumerate(clouds):
        if pillars:  # the device voxeliser's own pillars, read back: pillar order is then not in question
            out = dict(voxels=torch.empty((cap, mp, c.shape[1]), device=DEV), coors=torch.empty((cap, 4), dtype=torch.int32, device=DEV),
                       num_points=torch.empty((cap,), dtype=torch.int32, device=DEV), num_voxels=torch.empty((1,), dtype=torch.int32, device=DEV))
            hip_ops.voxelize(c, vg["voxel_size"], vg["range"], mp, cap, batch_idx=b, want_voxels=True, coor_cols=4, out=out)
            n = int(out["num_voxels"])
            vs.append(out["voxels"][:n]), cs.append(out["coors"][:n]), ns.append(out["num_points"][:n])
        else:
            v, co, n = points_to_voxel(c, vg["voxel_size"], vg["range"], mp, True, cap)
            vs.append(v), ns.append(n), cs.append(torch.nn.functional.pad(co, (1, 0), value=b))
    targets = ta(gt[0], gt[1], gt[2], batch.get("gt_trajectory"))
    ex = dict(voxels=torch.cat(vs), coordinates=torch.cat(cs), num_points=torch.cat(ns), num_voxels=torch.tensor([len(n) for n in ns]),
              shape=np.array([grid] * B), metadata=[None] * B)
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    if getattr(net.bbox_head, "bev_map", False):
        batch["bev_map"] = torch.rand((B, 6, ta.H, ta.W), generator=torch.Generator().manual_seed(3)).to(DEV)
        ex["bev_map"] = [batch["bev_map"][:, i] for i in range(6)]
    return net, vg, ta, batch, ex, pillars


def alternating(config, args):
    """eager and static steps of ``config`` on the same weights, alternating in one loop -> report lines"""
    B = args.batch
    net, vg, ta, batch, ex, pillars = _world(config, B, args.points)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, 100000)
    it = [0]

    def eager():
        for _ in solver.train_steps(net, [ex], opt, sched, grad_clip=GRAD_CLIP, start_iter=it[0]):
            it[0] += 1

    cls = solver.StaticPillarsTrainStep if pillars else solver.StaticTrainStep
    static = cls(net, vg, ta, opt, sched, GRAD_CLIP, capacity=args.points + 50000, batch_size=B, max_gt=64)
    static.warm_up([batch])
    rows = [("eager  solver.train_steps", eager), ("static %s" % cls.__name__, lambda: static(batch)),
            ("static, check=False", lambda: static(batch, check=False))]
    for _, fn in rows:
        for _ in range(args.warmup):
            fn()
    samples = [[] for _ in rows]
    for _ in range(args.runs):
        for i, (_, fn) in enumerate(rows):
            samples[i].extend(timed(fn, 1))
    lines = ["%s, B = %d, %d-point synthetic clouds (pillar / level counts %s)" % (
        config, B, args.points, [int(v) for v in net.last_level_counts])]
    for (name, fn), t in zip(rows, samples):
        t = np.asarray(t)
        lines.append("  %-38s %8.2f ms  (%.2f .. %.2f, spread %.2f)   %4.1f host synchronisations per step" % (
            name, np.median(t), t.min(), t.max(), t.max() - t.min(), syncs_per_step(fn)))
    lines.append("")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=["forecast_n0", "pointpillars", "forecast_n3dtfm"],
                    help="forecast_n0 (default): the fp32 / bf16 rows table; pointpillars, forecast_n3dtfm: the alternating comparison")
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="default: profiles/static_train_step.txt, or profiles/static_train_step_pillars.txt "
                                                "for the --config pointpillars / forecast_n3dtfm report")
    args = ap.parse_args()
    configs = args.config or ["forecast_n0"]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "static_train_step.txt" if configs == ["forecast_n0"] else "static_train_step_pillars.txt")
    if configs != ["forecast_n0"]:
        if "forecast_n0" in configs:
            ap.error("--config forecast_n0 is a report of its own; run it separately")
        lines = ["one training iteration, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__),
                 "eager and static steps alternate in one loop on the same weights; median of %d samples each, ms per step (min .. max, "
                 "spread); host synchronisations per step from torch's sync debug mode" % args.runs, ""]
        for config in configs:
            lines += alternating(config, args)
        text = "\n".join(lines)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
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
