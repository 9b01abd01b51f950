"""Times GT-database sampling: the two kernels alone, and solver.StaticTrainStep on forecast_n0 at B = 2 (synth.synthetic_cloud, 300 000
points, the shipped voxel caps) with and without a sampler, over a synthetic database of 200 cars of 50 .. 400 points each:

    plain             the batch is copied into the static buffers
    augment           the shipped global augmentation (tools/augment_bench.py's second row)
    + sampler car=2   the same with GTSampler at the shipped group: the bench's ground truth holds 40 cars, more than max_num, so no
                      entry is ever accepted and every cloud grows by point_cap = 2 x 400 sentinel rows: the fixed cost of the route
    + sampler car=50  a group the ground truth leaves room in: ten of the fifty drawn slots take part, every cloud grows by
                      point_cap = 50 x 400 rows

All steps share one model and one optimiser and alternate in ONE loop, so drift of the clock or the machine lands on all sides alike.
A sample is one iteration with check=False between two device synchronisations on the host clock, host work (the draws) included.
No threshold and no speed-up expected: a sampled step does more work by the added points; the file is the record, and the figure to
read is the difference of the medians against the plain side's own spread.

    python tools/gt_sample_bench.py [--out profiles/gt_sample_bench.txt]
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
from futuredet_amd.augment import GlobalAugment, GTDatabase, GTSampler  # noqa: E402
from train_step_bench import DEV, GRAD_CLIP, LR_CONFIG, _world, timed  # noqa: E402

TRAIN_PREPROCESSOR = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1],
                          global_translate_std=0.5, db_sampler=dict(enable=False))


def synthetic_database(entries=200, seed=11):
    r = np.random.default_rng(seed)
    sizes = r.integers(50, 401, entries)
    boxes = np.zeros((entries, 3, 12), np.float32)
    boxes[:, :, 0:2] = r.uniform(-50, 50, (entries, 1, 2))
    boxes[:, :, 2] = -0.5
    boxes[:, :, 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * r.uniform(0.8, 1.2, (entries, 1, 3))
    boxes[:, :, 6:10] = r.normal(0, 2, (entries, 3, 4))
    boxes[:, :, 10:12] = r.uniform(-np.pi, np.pi, (entries, 1, 2))
    P = int(sizes.sum())
    pts = np.zeros((P, 5), np.float32)
    pts[:, :3] = r.uniform(-0.5, 0.5, (P, 3)) * np.repeat(boxes[:, 0, 3:6], sizes, axis=0)
    pts[:, 3] = r.integers(0, 256, P)
    return GTDatabase.from_arrays(boxes, np.full(entries, 3), np.ones(entries), r.integers(0, 3, entries), pts,
                                  np.concatenate([[0], np.cumsum(sizes)]), DEV, class_names=["car"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_sample_bench.txt"))
    args = ap.parse_args()
    B = args.batch
    net, vg, ta, batch, _, _ = _world("forecast_n0", B, args.points)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, LR_CONFIG, 100000)
    db = synthetic_database()
    kw = dict(capacity=args.points + 50000, batch_size=B, max_gt=64)
    plain = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, **kw)
    plain.warm_up([batch])

    def step_with(groups):
        sampler = GTSampler(db, groups, rate=1.0, seed=0) if groups else None
        step = solver.StaticTrainStep(net, vg, ta, opt, sched, GRAD_CLIP, augment=GlobalAugment(TRAIN_PREPROCESSOR, seed=0, sampler=sampler), **kw)
        step.warm_up([batch] * 4)  # four draws: the capacities cover what the transforms and the pasted points do to the level counts
        return step, sampler

    steps = [step_with(g) for g in (None, [dict(car=2)], [dict(car=50)])]
    rows = [("plain   StaticTrainStep", lambda: plain(batch, check=False))]
    for (step, sampler), name in zip(steps, ("augment", "augment + sampler car=2", "augment + sampler car=50")):
        rows.append((name + (" (point_cap %d)" % sampler.point_cap if sampler else ""), lambda step=step: step(batch, check=False)))
    for _, fn in rows:
        for _ in range(args.warmup):
            fn()
    samples, overflows, accepted = [[] for _ in rows], [0] * len(steps), [[] for _ in steps]
    for _ in range(args.runs):
        for i, (_, fn) in enumerate(rows):
            samples[i].extend(timed(fn, 1))
            if i:  # (read back after the sample's clock has stopped)
                step = steps[i - 1][0]
                overflows[i - 1] += bool(step.overflowed())
                if step.gt_sample is not None:
                    accepted[i - 1].append(step.gt_sample["accepted"].sum(1).cpu().tolist())
    lines = ["one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, %s, torch %s" % (
        B, args.points, torch.cuda.get_device_name(0), torch.__version__),
        "static steps (check=False) alternate in one loop on the same weights; median of %d samples each, ms per step (min .. max, spread)"
        % args.runs, ""]
    med = []
    for (name, _), t in zip(rows, samples):
        t = np.asarray(t)
        med.append((np.median(t), t.max() - t.min()))
        lines.append("  %-44s %8.2f ms  (%.2f .. %.2f, spread %.2f)" % (name, np.median(t), t.min(), t.max(), t.max() - t.min()))
    lines.append("")
    for i in (2, 3):
        lines.append("%s - augment = %+.2f ms, - plain = %+.2f ms; the plain side's own spread is %.2f ms" % (
            rows[i][0], med[i][0] - med[1][0], med[i][0] - med[0][0], med[0][1]))
    lines.append("accepted entries per sample, last iteration: car=2 %s, car=50 %s; overflowed iterations (augment, car=2, car=50): %s of %d" % (
        accepted[1][-1], accepted[2][-1], overflows, args.runs))
    # the kernels alone, on the car=50 sampler's shapes
    step, sampler = steps[2]
    gs, cap = step.gt_sample, sampler.point_cap
    cand = torch.from_numpy(sampler.draw(B)).to(DEV)
    gtb, gtc, gtk = batch["gt_boxes"].contiguous(), batch["gt_counts"].contiguous(), batch["gt_classes"].contiguous()
    wide = torch.zeros((B, gtb.shape[1], 64, 12), device=DEV)
    wide[:, :, :gtb.shape[2]] = gtb
    widek = torch.zeros((B, gtb.shape[1], 64), dtype=torch.int32, device=DEV)
    widek[:, :, :gtb.shape[2]] = gtk
    outs = (torch.empty_like(wide), torch.empty_like(gtc), torch.empty_like(widek), None)
    t_sel = timed(lambda: hip_ops.gt_sample_select(wide, gtc, widek, db, cand, gs["groups"], 1.0, cap, out=outs, accepted=gs["accepted"],
                                                   plan=gs["plan"], n_points=gs["n_points"], status=gs["status"]), args.runs)
    t_pts = timed(lambda: hip_ops.gt_sample_points(db, cand[0], gs["accepted"][0], gs["plan"][0], gs["stage"][0], cap), args.runs)
    lines += ["", "the kernels alone (launch + synchronisation on the host clock):",
              "  %-44s %8.3f ms  (%.3f .. %.3f)   B = %d, T = %d, n_max = 64, K = %d, %d ground-truth objects" % (
                  "fd_gt_sample_select", np.median(t_sel), t_sel.min(), t_sel.max(), B, gtb.shape[1], sampler.K, int(gtc[0, 0])),
              "  %-44s %8.3f ms  (%.3f .. %.3f)   point_cap = %d rows of 5 floats, %d of them entries' points" % (
                  "fd_gt_sample_points (one cloud)", np.median(t_pts), t_pts.min(), t_pts.max(), cap, int(gs["n_points"][0]))]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
