"""Mixed-precision training of the RPN neck (dense_train.py, RPN.train_dtype = torch.bfloat16) against the fp32 path it can replace.  Every
comparison takes both sides in this one process, alternating inside one timing loop.

  1. per layer, B = 2, the shipped forecast_n0 shapes: forward + backward (dx and dW) of
         ours        dense_train.conv2d_bf16: device packer, fd_conv2d_nhwc_bf16, packer + fd_conv2d_nhwc_bf16 for dx, fd_conv2d_wgrad_bf16
         torch fp32  F.conv2d on fp32 NCHW maps (what the fp32 neck runs)
         torch bf16  F.conv2d on bf16 channels-last maps
     device time between two events, median of --iters samples with (min .. max); then our four launches on their own.
  2. the neck: forward + backward of forecast_n0's RPN at B = 2 on a random BEV map, train_dtype fp32 against bf16, with
     torch.cuda.max_memory_allocated.
  3. the step: one training iteration of forecast_n0 as tools/train_step_bench.py times it (B = 2, bf16 backbone rows, fused_bn,
     fused_loss; eager solver.train_steps and solver.StaticTrainStep), neck fp32 against neck bf16.

No threshold: the file is the record.  Lines are written as they are measured.

    python tools/dense_conv_train_bench.py [--out profiles/dense_conv_train_bf16.txt] [--skip-step]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from futuredet_amd import dense_train, hip_ops  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.necks import RPN  # noqa: E402
from futuredet_amd.synth import seeded_state_dict  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
# (Cin, Cout, side, ks, where)
LAYERS = [(256, 128, 180, 3, "stage 1, first convolution"), (128, 128, 180, 3, "stage 1, repeats"), (256, 256, 90, 3, "stage 2, repeats"),
          (128, 256, 180, 1, "deblock 1 (1 x 1)")]


class Out(object):
    def __init__(self, path):
        self.f = None
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            self.f = open(path, "w")

    def __call__(self, line=""):
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


def timed_each(fns, iters, warmup=3):
    """device time (microseconds) of every callable of ``fns``, the callables alternating inside one loop: {key: samples}"""
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


def fmt(t):
    return "%9.1f (%8.1f .. %8.1f)" % (np.median(t), t.min(), t.max())


def per_layer(args, out):
    out("1. per layer, B = %d: forward + backward (dx, dW), microseconds of device time, median of %d (min .. max)" % (args.batch, args.iters))
    out("%-30s %-32s %-32s %-32s %s" % ("layer", "ours (conv2d_bf16)", "torch fp32 NCHW", "torch bf16 channels-last", "ours / fp32"))
    slower = []
    for cin, cout, side, ks, where in LAYERS:
        B = args.batch
        g = torch.Generator(device="cpu").manual_seed(cin + cout + side)
        x32 = torch.randn((B, cin, side, side), generator=g).to(DEV)
        w32 = (torch.randn((cout, cin, ks, ks), generator=g) * 0.05).to(DEV)
        dy32 = torch.randn((B, cout, side, side), generator=g).to(DEV)
        x_nhwc = x32.permute(0, 2, 3, 1).contiguous().to(BF).requires_grad_(True)
        dy_nhwc = dy32.permute(0, 2, 3, 1).contiguous().to(BF)
        x_f = x32.clone().requires_grad_(True)
        w_a, w_b, w_c = (w32.clone().requires_grad_(True) for _ in range(3))
        x_cl = x32.to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w_cl = w32.to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        dy_cl = dy32.to(BF).contiguous(memory_format=torch.channels_last)

        def ours():
            return torch.autograd.grad(dense_train.conv2d_bf16(x_nhwc, w_a, ks), [x_nhwc, w_a], dy_nhwc)

        def fp32():
            return torch.autograd.grad(F.conv2d(x_f, w_b, padding=ks // 2), [x_f, w_b], dy32)

        def bf16():
            return torch.autograd.grad(F.conv2d(x_cl, w_cl, padding=ks // 2), [x_cl, w_cl], dy_cl)

        t = timed_each({"ours": ours, "fp32": fp32, "bf16": bf16}, args.iters)
        ratio = float(np.median(t["ours"]) / np.median(t["fp32"]))
        name = "%d -> %d, %d x %d, ks %d" % (cin, cout, side, side, ks)
        if ratio >= 1.0:
            slower.append(name)
        out("%-30s %-32s %-32s %-32s %6.2f%s   %s" % (name, fmt(t["ours"]), fmt(t["fp32"]), fmt(t["bf16"]), ratio,
                                                     "  <-- ours is NOT faster" if ratio >= 1.0 else "", where))
        # our launches on their own
        xd, wd = x_nhwc.detach(), w_a.detach()
        wpk, wpk_t = hip_ops.pack_conv2d_weight_device(wd), hip_ops.pack_conv2d_weight_device(wd, transposed=True)
        parts = timed_each({
            "pack": lambda: hip_ops.pack_conv2d_weight_device(wd),
            "forward": lambda: hip_ops.conv2d_nhwc_bf16(xd, wpk, None, cout, ks, stride=1, relu=False),
            "pack^T": lambda: hip_ops.pack_conv2d_weight_device(wd, transposed=True),
            "dx": lambda: hip_ops.conv2d_nhwc_bf16(dy_nhwc, wpk_t, None, cin, ks, stride=1, relu=False),
            "dW": lambda: hip_ops.conv2d_wgrad_bf16(xd, dy_nhwc, ks)}, args.iters)
        out("%-30s %s" % ("", "   ".join("%s %.1f" % (k, np.median(v)) for k, v in parts.items())))
        del x32, w32, dy32, x_nhwc, dy_nhwc, x_f, x_cl, w_cl, dy_cl
        torch.cuda.empty_cache()
    out("layers where conv2d_bf16 is not faster than torch fp32: %s" % (", ".join(slower) if slower else "none"))
    out()


def neck(args, out):
    cfg = centerpoint_config("forecast_n0")
    nk = dict(cfg.model["neck"])
    nk.pop("type")
    torch.manual_seed(0)
    rpn = RPN(**nk)
    rpn.load_state_dict(seeded_state_dict(rpn, 3), strict=False)
    rpn = rpn.to(DEV).train()
    g = torch.Generator(device="cpu").manual_seed(11)
    bev = torch.randn((args.batch, nk["num_input_features"], 180, 180), generator=g).to(DEV)
    dy = torch.randn((args.batch, sum(nk["us_num_filters"]), 180, 180), generator=g).to(DEV)

    def step(dtype):
        rpn.train_dtype = dtype
        rpn.zero_grad(set_to_none=True)
        rpn(bev).backward(dy)

    runs = [timed_each({dt: (lambda dt=dt: step(dt)) for dt in (torch.float32, BF)}, args.model_iters) for _ in range(3)]
    out("2. forecast_n0 RPN, train mode, forward + backward, B = %d, milliseconds of device time (three medians of %d) and max_memory_allocated"
        % (args.batch, args.model_iters))
    med = {}
    for dt in (torch.float32, BF):
        rpn.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        step(dt)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        ms = [float(np.median(r[dt])) / 1000.0 for r in runs]
        med[dt] = float(np.median(ms))
        out("   train_dtype = %-15s %s   median %8.2f ms   peak %8.1f MiB" % (dt, " ".join("%8.2f" % m for m in ms), med[dt], peak / 2 ** 20))
    out("   bf16 / fp32 = %.2f%s" % (med[BF] / med[torch.float32], "" if med[BF] < med[torch.float32] else "   <-- the bf16 neck is NOT faster"))
    out()
    del rpn, bev, dy
    torch.cuda.empty_cache()


def whole_step(args, out):
    import train_step_bench as tsb
    from futuredet_amd import build_detector, solver
    from futuredet_amd.synth import synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel

    B = args.batch
    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV).train()
    net.backbone.fused_bn = True
    net.bbox_head.fused_loss = True
    net.backbone.train_dtype = BF
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
    static = solver.StaticTrainStep(net, vg, ta, opt, sched, tsb.GRAD_CLIP, capacity=args.points + 50000, batch_size=B, max_gt=64)
    static.warm_up([batch])
    static(batch)
    it = [0]

    def eager():
        for _ in solver.train_steps(net, [ex], opt, sched, grad_clip=tsb.GRAD_CLIP, start_iter=it[0]):
            it[0] += 1

    out("3. one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, bf16 backbone rows, fused_bn, fused_loss: ms per step on "
        "the host clock between two synchronisations, median of %d (min .. max)" % (B, args.points, args.step_runs))
    for name, fn in (("eager  solver.train_steps", eager), ("static StaticTrainStep", lambda: static(batch)),
                     ("static, check=False", lambda: static(batch, check=False))):
        res = {}
        for dt in (torch.float32, BF, torch.float32, BF):  # each side twice, alternating; the two samples sets are pooled
            net.neck.train_dtype = dt
            for _ in range(2):
                fn()
            res.setdefault(dt, []).append(tsb.timed(fn, args.step_runs))
        t32, t16 = np.concatenate(res[torch.float32]), np.concatenate(res[BF])
        out("   %-28s neck fp32 %8.2f (%.2f .. %.2f)   neck bf16 %8.2f (%.2f .. %.2f)   bf16 / fp32 = %.2f%s" % (
            name, np.median(t32), t32.min(), t32.max(), np.median(t16), t16.min(), t16.max(), np.median(t16) / np.median(t32),
            "" if np.median(t16) < np.median(t32) else "   <-- the bf16 neck is NOT faster"))
    net.neck.train_dtype = BF
    n_sync = tsb.syncs_per_step(lambda: static(batch, check=False))
    out("   host synchronisations per static step (check=False) with the bf16 neck: %.1f" % n_sync)
    out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-iters", type=int, default=5)
    ap.add_argument("--step-runs", type=int, default=10)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_conv_train_bf16.txt"))
    args = ap.parse_args()
    out = Out(args.out)
    out("# tools/dense_conv_train_bench.py --batch %d, %s, torch %s; weight-gradient chunk %d pixels"
        % (args.batch, torch.cuda.get_device_name(0), torch.__version__, hip_ops.conv2d_wgrad_bf16_chunk()))
    per_layer(args, out)
    neck(args, out)
    if not args.skip_step:
        whole_step(args, out)


if __name__ == "__main__":
    main()
