"""A/B of the chunk plan per SubM layer family, on the real rulebooks of one synthetic cloud: fd_spconv_apply_plan with the plan
against the same launch with "spconv_plan" = -1 (in-kernel compaction), alternating, plus the plan build itself.
usage: python tools/spconv_plan_bench.py [--levels 1,2,3] [--iters 50] [--rounds 3] [--points 300000]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from futuredet_amd import build_backbone, hip_ops  # noqa: E402
from futuredet_amd.synth import seeded_state_dict, synthetic_cloud  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--levels", default="1,2,3")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--points", type=int, default=300000)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda")
pts = torch.from_numpy(synthetic_cloud(args.seed, args.points)).to(dev)
out = hip_ops.voxelize(pts, [0.075, 0.075, 0.2], [-54, -54, -5.0, 54, 54, 3.0], 10, 160000, want_voxels=False, want_mean=True,
                       mean_stride=16, coor_cols=4)
m = int(out["num_voxels"].cpu()[0])
bb = build_backbone(dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8))
bb.load_state_dict(seeded_state_dict(bb, 7), strict=False)
bb = bb.to(dev).eval()
idx = bb.build_indexes(lambda i0: i0.mark(out["coors"][:m].contiguous()), 1, [1440, 1440, 40], dev)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


for lvl in [int(v) for v in args.levels.split(",")]:
    C = [16, 32, 64, 128][lvl]
    ix = idx[lvl]
    x = torch.randn((ix.n, C), device=dev)
    wpk = hip_ops.pack_spconv_weight(torch.randn((27, C, C)) * (2.0 / (27 * C)) ** 0.5).to(dev)
    bias = torch.zeros(C, device=dev)
    nbr = ix.rulebook(ix, [3, 3, 3], [1, 1, 1], [1, 1, 1])
    run = lambda: hip_ops.spconv_apply(x, wpk, bias, nbr, ix.n, C, residual=x, relu=True)  # noqa: E731
    y_on = run()
    hip_ops.set_tuning("spconv_plan", -1)
    y_off = run()
    hip_ops.set_tuning("spconv_plan", 0)
    assert torch.equal(y_on, y_off), "the plan changed the result"
    ranges, n_ranges = hip_ops.row_split(nbr, ix.n, C, C)

    def build():
        nbr.plans = {}
        hip_ops.plan_for(nbr, ix.n, ranges, n_ranges)

    for _ in range(3):
        build()
    t_build = timed(build, args.iters)
    on, off = [], []
    for _ in range(args.rounds):
        hip_ops.set_tuning("spconv_plan", -1)
        run()
        off.append(timed(run, args.iters))
        hip_ops.set_tuning("spconv_plan", 0)
        run()
        on.append(timed(run, args.iters))
    print("level %d C=%3d n=%6d: in-kernel compaction %s us | chunk plan %s us | plan build (with its allocation) %.1f us" %
          (lvl, C, ix.n, " ".join("%.1f" % v for v in off), " ".join("%.1f" % v for v in on), t_build), flush=True)
