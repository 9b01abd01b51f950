"""Times the point-in-box kernels: the three launches alone (fd_points_in_boxes_count = the partial counts + the scan,
fd_points_in_boxes_extract) at 300 000 points x 40 and x 400 boxes, and solver.StaticTrainStep on forecast_n0 at B = 2
(synth.synthetic_cloud, 300 000 points, the shipped voxel caps):

    plain               the batch is copied into the static buffers
    augment             the shipped global augmentation (tools/augment_bench.py's second row)
    augment + filter    the same with min_points_in_gt = 5 (GlobalAugment(..., point_filter=True)): two launches per cloud and one for the
                        batch while the ground truth is loaded

All steps share one model and one optimiser and alternate in ONE loop, so drift of the clock or the machine lands on all sides alike.
A sample is one iteration with check=False between two device synchronisations on the host clock, host work (the draws) included.
No threshold and no speed-up expected: the filter adds launches and removes objects; the file is the record, and the figure to read is
the difference of the medians against the plain side's own spread.

    python tools/points_in_boxes_bench.py [--out profiles/points_in_boxes_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from futuredet_amd import hip_ops, solver  # noqa: E402
from futuredet_amd.augment import GlobalAugment  # noqa: E402
from train_step_bench import DEV, GRAD_CLIP, LR_CONFIG, _world, synthetic_gt, timed  # noqa: E402

TRAIN_PREPROCESSOR = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1],
                          global_translate_std=0.5, db_sampler=dict(enable=False))
MIN_POINTS = 5


def row(name, t, note=""):
    t = np.asarray(t)
    return "  %-44s %8.3f ms  (%.3f .. %.3f, spread %.3f)%s" % (name, np.median(t), t.min(), t.max(), t.max() - t.min(), note)


def kernels_alone(cloud, n_boxes, runs):
    boxes = torch.from_numpy(synthetic_gt(np.random.default_rng(n_boxes), 1, 1, n_boxes)[0][0, 0]).to(DEV)
    n = int(cloud.shape[0])
    ws = hip_ops.points_in_boxes_workspace(n, n_boxes, DEV)
    counts = torch.zeros((n_boxes,), dtype=torch.int32, device=DEV)
    hip_ops.points_in_boxes_count(cloud, boxes, out=counts, workspace=ws)
    total = int(counts.sum())
    rows = torch.empty((total, cloud.shape[1]), device=DEV)
    offsets, status = torch.empty((n_boxes + 1,), dtype=torch.int64, device=DEV), torch.empty((1,), dtype=torch.int32, device=DEV)
    for _ in range(3):
        hip_ops.points_in_boxes_extract(cloud, boxes, ws, rows, offsets=offsets, status=status)
    t_count = timed(lambda: hip_ops.points_in_boxes_count(cloud, boxes, out=counts, workspace=ws), runs)
    t_extract = timed(lambda: hip_ops.points_in_boxes_extract(cloud, boxes, ws, rows, offsets=offsets, status=status), runs)
    note = "   %d points x %d boxes, %d rows extracted" % (n, n_boxes, total)
    return [row("fd_points_in_boxes_count (two launches)", t_count, note), row("fd_points_in_boxes_extract", t_extract, note)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_in_boxes_bench.txt"))
    args = ap.parse_args()
    B = args.batch
    net, vg, ta, batch, _, _ = _world("forecast_n0", B, args.points)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, 100000)
    kw = dict(capacity=args.points + 50000, batch_size=B, max_gt=64)
    plain = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, **kw)
    plain.warm_up([batch])
    aug = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, augment=GlobalAugment(TRAIN_PREPROCESSOR, seed=0), **kw)
    filt = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP,
                                  augment=GlobalAugment(dict(TRAIN_PREPROCESSOR, min_points_in_gt=MIN_POINTS), seed=0, point_filter=True), **kw)
    for step in (aug, filt):
        step.warm_up([batch] * 4)  # four draws: the capacities cover what the transforms do to the level counts
    rows = [("plain   StaticTrainStep", plain), ("augment", aug), ("augment + filter (min_points_in_gt = %d)" % MIN_POINTS, filt)]
    for _, step in rows:
        for _ in range(args.warmup):
            step(batch, check=False)
    samples, overflows = [[] for _ in rows], [0] * len(rows)
    for _ in range(args.runs):
        for i, (_, step) in enumerate(rows):
            samples[i].extend(timed(lambda step=step: step(batch, check=False), 1))
            overflows[i] += bool(step.overflowed())  # (read back after the sample's clock has stopped)
    lines = ["one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, %s, torch %s" % (
        B, args.points, torch.cuda.get_device_name(0), torch.__version__),
        "static steps (check=False) alternate in one loop on the same weights; median of %d samples each, ms per step (min .. max, spread)"
        % args.runs, ""]
    lines += [row(name, t) for (name, _), t in zip(rows, samples)]
    med = [float(np.median(t)) for t in samples]
    lines += ["", "augment + filter - augment = %+.3f ms, - plain = %+.3f ms; the plain side's own spread is %.3f ms" % (
        med[2] - med[1], med[2] - med[0], max(samples[0]) - min(samples[0])),
        "objects kept per sample at timestep 0, last iteration: %s of %s; overflowed iterations (plain, augment, filter): %s of %d" % (
            filt.gt_counts[:, 0].cpu().tolist(), batch["gt_counts"][:, 0].cpu().tolist(), overflows, args.runs),
        "", "the kernels alone (launch + synchronisation on the host clock, median of %d):" % args.runs]
    for n_boxes in (40, 400):
        lines += kernels_alone(batch["clouds"][0].contiguous(), n_boxes, args.runs)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
