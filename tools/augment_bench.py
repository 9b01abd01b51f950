"""Times solver.StaticTrainStep on forecast_n0 at B = 2 (synth.synthetic_cloud, 300 000 points, the shipped voxel caps) with and
without ``augment`` (augment.GlobalAugment with the shipped train_preprocessor values: shuffle, flips, rotation, scaling, translation):

    plain            the batch is copied into the static buffers
    augment          one fd_augment_points per cloud in place of the copy, one fd_augment_boxes, a fresh draw and record upload per step
    transforms only  the same with shuffle_points=False: the rows keep their order
    shuffle only     the same with no_augmentation=True: identity transforms, the rows in the shuffle's order

(The last two split what the augmented step costs beyond its three launches: the transforms change the level counts from draw to draw,
the shuffle changes the order in which the voxeliser meets the points and with it the order of the voxel rows.)

All steps share one model and one optimiser and alternate in ONE loop (plain, augment, transforms only, shuffle only, plain, ...), so
drift of the clock or the machine lands on all sides alike.  A sample is one iteration with check=False between two device synchronisations on the host
clock, host work included.  The augmented step sees another batch every iteration (its level counts move with the draw); an
iteration whose counts overflowed the row capacities is counted and reported.  The last row times GlobalAugment()(batch) alone.
A second leg does the same for forecast_n3dtfm, the bev_map head: the plain step, the augmented step whose batch brings the parameters
and a map warped with them, and the augmented step with ``warp_bev=True`` and ``filter_gt=True`` (map_leg).
No threshold and no speed-up expected: the file is the record, and the figure to read is the difference of the medians against the
plain side's own spread.

    python tools/augment_bench.py [--out profiles/augment_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from futuredet_amd import solver  # noqa: E402
from futuredet_amd.augment import GlobalAugment  # noqa: E402
from train_step_bench import GRAD_CLIP, LR_CONFIG, _world, timed  # noqa: E402

TRAIN_PREPROCESSOR = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1],
                          global_translate_std=0.5, db_sampler=dict(enable=False))


def map_leg(args):
    """forecast_n3dtfm (the bev_map head): the plain step, the augmented step on today's route (the batch brings aug_params and a map
    warped with them) and the augmented step with warp_bev=True and filter_gt=True (a fresh draw, the mask records' upload,
    fd_augment_mask in place of the map's copy, fd_gt_range_filter on the static ground truth), alternating in one loop -> report lines"""
    B = args.batch
    net, vg, ta, batch, _, _ = _world("forecast_n3dtfm", B, args.points)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, 100000)
    kw = dict(capacity=args.points + 50000, batch_size=B, max_gt=64)
    plain = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, **kw)
    plain.warm_up([batch])
    warper = GlobalAugment(TRAIN_PREPROCESSOR, seed=0, warp_bev=True)
    today = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, augment=GlobalAugment(TRAIN_PREPROCESSOR, seed=0), **kw)
    pre = []
    for _ in range(4):  # four draws: the capacities cover what the transforms do to the level counts
        p = warper.draw(B)
        pre.append(dict(batch, aug_params=p, bev_map=warper.warp_map(batch["bev_map"], p)))
    today.warm_up(pre)
    full = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, augment=warper, filter_gt=True, **kw)
    full.warm_up([batch] * 4)
    turn, overflows = [0], [0, 0]

    def today_step():
        turn[0] += 1
        today(pre[turn[0] % len(pre)], check=False)

    rows = [("plain   StaticTrainStep", lambda: plain(batch, check=False)),
            ("augment, batch brings params + warped map", today_step),
            ("augment(warp_bev=True), filter_gt=True", lambda: full(batch, check=False))]
    for _, fn in rows:
        for _ in range(args.warmup):
            fn()
    samples = [[] for _ in rows]
    for _ in range(args.runs):
        for i, (_, fn) in enumerate(rows):
            samples[i].extend(timed(fn, 1))
            if i and (today, full)[i - 1].overflowed():  # (read back after the sample's clock has stopped)
                overflows[i - 1] += 1
    lines = ["one training iteration of forecast_n3dtfm (bev_map head, 180 x 180 map), B = %d, %d-point synthetic clouds, same loop rules; "
             "median of %d samples each, ms per step (min .. max, spread)" % (B, args.points, args.runs), ""]
    med = []
    for (name, _), t in zip(rows, samples):
        t = np.asarray(t)
        med.append((np.median(t), t.max() - t.min()))
        lines.append("  %-42s %8.2f ms  (%.2f .. %.2f, spread %.2f)" % (name, np.median(t), t.min(), t.max(), t.max() - t.min()))
    kept = full.gt_counts[:, 0].cpu().tolist()
    alone = timed(lambda: warper.warp_map(batch["bev_map"], pre[0]["aug_params"]), args.runs)
    lines.append("  %-42s %8.2f ms  (%.2f .. %.2f, spread %.2f)   record build + upload + 1 launch" % (
        "GlobalAugment.warp_map(map) alone", np.median(alone), alone.min(), alone.max(), alone.max() - alone.min()))
    for i, what in ((1, "today's route"), (2, "warp + filter")):
        diff = med[i][0] - med[0][0]
        lines.append("%s - plain = %+.2f ms; the plain side's own spread is %.2f ms: the difference %s it" % (
            what, diff, med[0][1], "exceeds" if abs(diff) > med[0][1] else "lies inside"))
    lines += ["", "warp + filter - today's route = %+.2f ms (no speed-up expected or claimed: the warp and the filter are work the other rows "
              "leave to whoever makes the batch)" % (med[2][0] - med[1][0]),
              "objects kept by the filter in the last iteration: %s of %s per sample; overflowed iterations: today's route %d, warp + filter %d "
              "of %d" % (kept, batch["gt_counts"][:, 0].cpu().tolist(), overflows[0], overflows[1], args.runs)]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    args = ap.parse_args()
    B = args.batch
    net, vg, ta, batch, _, _ = _world("forecast_n0", B, args.points)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, 100000)
    aug = GlobalAugment(TRAIN_PREPROCESSOR, seed=1)
    kw = dict(capacity=args.points + 50000, batch_size=B, max_gt=64)
    plain = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, **kw)
    plain.warm_up([batch])
    overflows = [0]

    def augmented_step(**cfg):
        step = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, augment=GlobalAugment(dict(TRAIN_PREPROCESSOR, **cfg), seed=0), **kw)
        step.warm_up([batch] * 4)  # four draws: the capacities cover what the transforms do to the level counts
        return step

    augmented = augmented_step()
    no_shuffle, shuffle_only = augmented_step(shuffle_points=False), augmented_step(no_augmentation=True)
    rows = [("plain   StaticTrainStep", lambda: plain(batch, check=False)),
            ("augment StaticTrainStep(augment=...)", lambda: augmented(batch, check=False)),
            ("  transforms only (shuffle_points=False)", lambda: no_shuffle(batch, check=False)),
            ("  shuffle only (no_augmentation=True)", lambda: shuffle_only(batch, check=False))]
    for _, fn in rows:
        for _ in range(args.warmup):
            fn()
    samples = [[] for _ in rows]
    for _ in range(args.runs):
        for i, (_, fn) in enumerate(rows):
            samples[i].extend(timed(fn, 1))
            if i == 1 and augmented.overflowed():  # (read back after the sample's clock has stopped)
                overflows[0] += 1
    alone = timed(lambda: aug(batch), args.runs)
    lines = ["one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, %s, torch %s" % (
        B, args.points, torch.cuda.get_device_name(0), torch.__version__),
        "plain and augmented static steps (check=False) alternate in one loop on the same weights; median of %d samples each, ms per step "
        "(min .. max, spread)" % args.runs, ""]
    med = []
    for (name, _), t in zip(rows, samples):
        t = np.asarray(t)
        med.append((np.median(t), t.max() - t.min()))
        lines.append("  %-40s %8.2f ms  (%.2f .. %.2f, spread %.2f)" % (name, np.median(t), t.min(), t.max(), t.max() - t.min()))
    lines.append("  %-40s %8.2f ms  (%.2f .. %.2f, spread %.2f)   %d launches, new tensors allocated" % (
        "GlobalAugment()(batch) alone", np.median(alone), alone.min(), alone.max(), alone.max() - alone.min(), B + 1))
    diff = med[1][0] - med[0][0]
    lines += ["", "augment - plain = %+.2f ms; the plain side's own spread is %.2f ms: the difference %s it" % (
        diff, med[0][1], "exceeds" if abs(diff) > med[0][1] else "lies inside"),
        "row capacities: plain %s, augment %s; %d of %d augmented iterations overflowed them (their optimiser step is skipped on the "
        "device)" % (plain.caps, augmented.caps, overflows[0], args.runs)]
    lines += ["", ""] + map_leg(args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
