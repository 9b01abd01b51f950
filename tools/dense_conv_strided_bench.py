"""The resolution-changing convolutions of the bf16 neck (dense_train.conv2d_s2_bf16, conv_transpose2d_k2_bf16, conv2d_k2s2_bf16) against
the recipe they replace in dense_train.run_stack_bf16: the module on an fp32 copy of its bf16 channels-last input, the result rounded to
bf16 -- ``m(x.float()).to(torch.bfloat16)``, torch's fp32 convolution forward and backward between two conversions.  That recipe is the
yardstick, not torch fp32 on fp32 maps.  Every comparison takes both sides in this one process, alternating inside one timing loop.

  1. per layer, B = 2, forward + backward (dx and dW): the two forecast_n0 layers and the five of the PointPillars neck; device time
     between two events, median of --iters samples with (min .. max); then our launches on their own.  A form is a WIN when its
     median is below the recipe's by more than the recipe's own (min .. max) spread in that run.
  2. the forecast_n0 neck and the PointPillars neck, train mode, train_dtype bf16, forward + backward: the routed walk against the
     walk with RECIPE switched on (the routed forms fall through again), with torch.cuda.max_memory_allocated.
  3. one training iteration of forecast_n0 as tools/train_step_bench.py times it (B = 2, bf16 backbone, neck and head, the backbone's
     fused_bn, fused_loss; eager solver.train_steps and solver.StaticTrainStep), each side twice, alternating.

No threshold: the file is the record.  Lines are written as they are measured.

    python tools/dense_conv_strided_bench.py [--out profiles/dense_conv_strided_bf16.txt] [--skip-step]
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

from dense_conv_train_bench import Out, fmt, timed_each  # noqa: E402
from futuredet_amd import dense_train, hip_ops  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.necks import RPN  # noqa: E402
from futuredet_amd.synth import seeded_state_dict  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
# (form, Cin, Cout, input side, where)
LAYERS = [("s2", 128, 256, 180, "forecast_n0 blocks.1: 180^2 -> 90^2"), ("up2", 256, 256, 90, "forecast_n0 deblocks.1: 90^2 -> 180^2"),
          ("s2", 64, 64, 512, "PointPillars blocks.0: 512^2 -> 256^2"), ("s2", 64, 128, 256, "PointPillars blocks.1: 256^2 -> 128^2"),
          ("s2", 128, 256, 128, "PointPillars blocks.2: 128^2 -> 64^2"), ("down2", 64, 128, 256, "PointPillars deblocks.0: 256^2 -> 128^2"),
          ("up2", 256, 128, 64, "PointPillars deblocks.2: 64^2 -> 128^2")]
POINTPILLARS_NECK = dict(layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[0.5, 1, 2],
                         us_num_filters=[128, 128, 128], num_input_features=64)
FORMS = {"s2": dense_train.conv2d_s2_bf16, "up2": dense_train.conv_transpose2d_k2_bf16, "down2": dense_train.conv2d_k2s2_bf16}
_PREDICATES = ("_pad_then_conv_s2_takes_bf16", "conv_s2_takes_bf16", "conv_up2_takes_bf16")  # the forms run_stack_bf16 routes
_ROUTED = {n: getattr(dense_train, n) for n in _PREDICATES}
RECIPE = False  # True: run_stack_bf16 takes the fall-through for the routed forms again (set_recipe)


def set_recipe(on):
    """the switch of sections 2 and 3: with ``on`` the walk's strided predicates all say no, so these layers run the parent's recipe"""
    global RECIPE
    RECIPE = bool(on)
    for n in _PREDICATES:
        setattr(dense_train, n, (lambda *a: False) if on else _ROUTED[n])


def _module(form, cin, cout):
    if form == "s2":
        return nn.Sequential(nn.ZeroPad2d(1), nn.Conv2d(cin, cout, 3, stride=2, bias=False))
    if form == "up2":
        return nn.ConvTranspose2d(cin, cout, 2, stride=2, bias=False)
    return nn.Conv2d(cin, cout, 2, stride=2, bias=False)


def per_layer(args, out):
    out("1. per layer, B = %d: forward + backward (dx, dW), microseconds of device time, median of %d (min .. max)" % (args.batch, args.iters))
    out("%-34s %-32s %-32s %-14s %s" % ("layer", "ours", "recipe m(x.float()).to(bf16)", "ours / recipe", ""))
    verdict = {}
    for form, cin, cout, side, where in LAYERS:
        B = args.batch
        torch.manual_seed(cin + cout + side)
        m = _module(form, cin, cout).to(DEV)
        conv = m[1] if form == "s2" else m
        w = conv.weight
        x_cl = torch.randn((B, cin, side, side), device=DEV).to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        x_nhwc = x_cl.detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)  # the same memory layout, our calling convention
        with torch.no_grad():
            y_shape = tuple(m(x_cl.float()).shape)
        dy_cl = torch.randn(y_shape, device=DEV).to(BF).contiguous(memory_format=torch.channels_last)
        dy_nhwc = dy_cl.permute(0, 2, 3, 1).contiguous()
        fn = FORMS[form]

        def ours():
            return torch.autograd.grad(fn(x_nhwc, w), [x_nhwc, w], dy_nhwc)

        def recipe():  # the parent commit's branch of run_stack_bf16, on the same bf16 channels-last input
            return torch.autograd.grad(m(x_cl.float()).to(torch.bfloat16), [x_cl, w], dy_cl)

        t = timed_each({"ours": ours, "recipe": recipe}, args.iters)
        mo, mr = float(np.median(t["ours"])), float(np.median(t["recipe"]))
        win = mo < mr - float(t["recipe"].max() - t["recipe"].min())
        verdict.setdefault(form, []).append((where, win))
        name = "%s %d -> %d from %d x %d" % (form, cin, cout, side, side)
        out("%-34s %-32s %-32s %6.2f  %-6s %s" % (name, fmt(t["ours"]), fmt(t["recipe"]), mo / mr, "WIN" if win else "no win", where))
        xd, wd = x_nhwc.detach(), w.detach()
        if form == "s2":
            wpk, wpk_t = hip_ops.pack_conv2d_weight_device(wd), hip_ops.pack_conv2d_weight_device(wd, transposed=True)
            parts = {"pack": lambda: hip_ops.pack_conv2d_weight_device(wd),
                     "forward": lambda: hip_ops.conv2d_nhwc_bf16(xd, wpk, None, cout, 3, stride=2, relu=False),
                     "pack^T": lambda: hip_ops.pack_conv2d_weight_device(wd, transposed=True),
                     "dx": lambda: hip_ops.conv2d_s2_dgrad_bf16(dy_nhwc, wpk_t, side, side, cin),
                     "dW": lambda: hip_ops.conv2d_wgrad_s2_bf16(xd, dy_nhwc)}
        else:
            up, down = hip_ops.pack_conv2d_weight_2x2_device(wd, hip_ops.PACK_UP2), hip_ops.pack_conv2d_weight_2x2_device(wd, hip_ops.PACK_DOWN2)
            coarse, fine = (xd, dy_nhwc) if form == "up2" else (dy_nhwc, xd)
            cc, cf = coarse.shape[3], fine.shape[3]
            parts = {"pack up2": lambda: hip_ops.pack_conv2d_weight_2x2_device(wd, hip_ops.PACK_UP2),
                     "pack down2": lambda: hip_ops.pack_conv2d_weight_2x2_device(wd, hip_ops.PACK_DOWN2),
                     ("forward (up2)" if form == "up2" else "dx (up2)"): lambda: hip_ops.conv2d_up2_bf16(coarse, up, cf),
                     ("dx (down2)" if form == "up2" else "forward (down2)"): lambda: hip_ops.conv2d_down2_bf16(fine, down, cc),
                     "dW": lambda: hip_ops.conv2d_wgrad_2x2_bf16(coarse, fine)}
        parts = timed_each(parts, args.iters)
        out("%-34s %s" % ("", "   ".join("%s %.1f" % (k, np.median(v)) for k, v in parts.items())))
        del m, x_cl, x_nhwc, dy_cl, dy_nhwc
        torch.cuda.empty_cache()
    for form, rows in verdict.items():
        out("form %-6s %s" % (form, "; ".join("%s: %s" % (where, "WIN" if win else "no win") for where, win in rows)))
    routed = [form for form in FORMS if "conv_%s_takes_bf16" % form in _PREDICATES]
    out("run_stack_bf16 routes: %s; on the recipe: %s" % (", ".join(routed), ", ".join(f for f in FORMS if f not in routed) or "none"))
    out()


def necks(args, out):
    cfg = centerpoint_config("forecast_n0")
    nk = dict(cfg.model["neck"])
    nk.pop("type")
    out("2. the necks, train mode, train_dtype = bfloat16, forward + backward, B = %d: milliseconds of device time, median of %d (min .. max), "
        "and max_memory_allocated" % (args.batch, args.model_iters))
    for name, kw, side in (("forecast_n0 RPN (180 x 180)", nk, 180), ("PointPillars RPN (512 x 512)", POINTPILLARS_NECK, 512)):
        torch.manual_seed(0)
        rpn = RPN(**kw)
        rpn.load_state_dict(seeded_state_dict(rpn, 3), strict=False)
        rpn = rpn.to(DEV).train()
        rpn.train_dtype = BF
        g = torch.Generator(device="cpu").manual_seed(11)
        bev = torch.randn((args.batch, kw["num_input_features"], side, side), generator=g).to(DEV)
        set_recipe(False)
        with torch.no_grad():
            dy = torch.randn(tuple(rpn(bev).shape), generator=g).to(DEV)

        def step(recipe):
            set_recipe(recipe)
            rpn.zero_grad(set_to_none=True)
            rpn(bev).backward(dy)

        t = timed_each({"ours": lambda: step(False), "recipe": lambda: step(True)}, args.model_iters)
        peak = {}
        for key, recipe in (("ours", False), ("recipe", True)):
            rpn.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            step(recipe)
            torch.cuda.synchronize()
            peak[key] = torch.cuda.max_memory_allocated() / 2 ** 20
        set_recipe(False)
        for key in ("ours", "recipe"):
            ms = t[key] / 1000.0
            out("   %-30s %-8s %8.2f (%.2f .. %.2f) ms   peak %8.1f MiB" % (name, key, np.median(ms), ms.min(), ms.max(), peak[key]))
        r = float(np.median(t["ours"]) / np.median(t["recipe"]))
        out("   %-30s ours / recipe = %.2f%s" % (name, r, "" if r < 1.0 else "   <-- the routed walk is NOT faster"))
        del rpn, bev, dy
        torch.cuda.empty_cache()
    out()


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
    static = solver.StaticTrainStep(net, vg, ta, opt, sched, tsb.GRAD_CLIP, capacity=args.points + 50000, batch_size=B, max_gt=64)
    static.warm_up([batch])
    static(batch)
    it = [0]

    def eager():
        for _ in solver.train_steps(net, [ex], opt, sched, grad_clip=tsb.GRAD_CLIP, start_iter=it[0]):
            it[0] += 1

    out("3. one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, bf16 backbone, neck and head, backbone fused_bn, fused_loss: ms per "
        "step on the host clock between two synchronisations, median of %d (min .. max)" % (B, args.points, args.step_runs))
    for name, fn in (("eager  solver.train_steps", eager), ("static StaticTrainStep", lambda: static(batch))):
        res = {}
        for recipe in (True, False, True, False):  # each side twice, alternating; the two sample sets are pooled
            set_recipe(recipe)
            for _ in range(2):
                fn()
            res.setdefault(recipe, []).append(tsb.timed(fn, args.step_runs))
        tr, to = np.concatenate(res[True]), np.concatenate(res[False])
        out("   %-28s recipe %8.2f (%.2f .. %.2f)   ours %8.2f (%.2f .. %.2f)   ours / recipe = %.3f%s" % (
            name, np.median(tr), tr.min(), tr.max(), np.median(to), to.min(), to.max(), np.median(to) / np.median(tr),
            "" if np.median(to) < np.median(tr) else "   <-- the routed walk is NOT faster"))
    set_recipe(False)
    out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-iters", type=int, default=7)
    ap.add_argument("--step-runs", type=int, default=10)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_conv_strided_bf16.txt"))
    args = ap.parse_args()
    out = Out(args.out)
    out("# tools/dense_conv_strided_bench.py --batch %d, %s, torch %s; weight-gradient chunk %d pixels"
        % (args.batch, torch.cuda.get_device_name(0), torch.__version__, hip_ops.conv2d_wgrad_bf16_chunk()))
    per_layer(args, out)
    necks(args, out)
    if not args.skip_step:
        whole_step(args, out)


if __name__ == "__main__":
    main()
