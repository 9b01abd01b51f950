"""Mixed-precision training of the CenterHead (CenterHead.train_dtype = torch.bfloat16: dense_train.conv2d_bf16 with a bias, the batched
branch convolution, dense_train.head_tail_bf16 on fd_head_tail_bf16.hip) against the fp32 path it can replace.  The method is
tools/dense_conv_train_bench.py's: device time between two events, both sides in this one process, alternating inside one timing loop,
median of the samples with (min .. max).

  a. per layer, B = 2, 180 x 180: forward + backward (dx, dW, dbias) of
         the 512 -> 64 shared convolution            conv2d_bf16 with its bias          against F.conv2d on fp32 NCHW maps
         the 64 -> 384 batched branch convolution    one conv2d_bf16 call               against six 64 -> 64 F.conv2d calls (what the fp32 head runs)
         the 6-group tail (k = 2, 1, 3, 2, 2, 1)     one head_tail_bf16 call            against six 64 -> k F.conv2d calls
     then our tail launches on their own.
  b. the head: forward + backward of the CenterHead of forecast_n0 and of forecast_n3dtf at B = 2 on a random map, train_dtype fp32
     against bf16, with torch.cuda.max_memory_allocated.
  c. the step: one training iteration of forecast_n0 as tools/train_step_bench.py times it (B = 2, backbone and neck in bf16, fused_bn on
     the backbone, fused_loss; eager solver.train_steps and solver.StaticTrainStep), head fp32 against head bf16.

No threshold: the file is the record.  A side counts as faster where the gap between the medians exceeds the other side's own spread
(max - min of its samples, or of its three medians in b).  Lines are written as they are measured.

    python tools/head_train_bench.py [--out profiles/head_train_bf16.txt] [--skip-step]
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

from dense_conv_train_bench import Out, fmt, timed_each  # noqa: E402
from futuredet_amd import dense_train, hip_ops  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.heads import CenterHead  # noqa: E402
from futuredet_amd.synth import seeded_state_dict  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
TAIL_K = (2, 1, 3, 2, 2, 1)  # reg, height, dim, rot, vel, hm of a forecast_n0 SepHead


def verdict(ours, other):
    """(ratio of the medians, note): ours is faster only where the gap exceeds the other side's spread"""
    mo, mt = float(np.median(ours)), float(np.median(other))
    spread = float(other.max() - other.min())
    return mo / mt, "" if mt - mo > spread else "  <-- NOT faster than fp32 by more than its spread (%.1f)" % spread


def per_layer(args, out):
    B, S = args.batch, 180
    out("a. per layer, B = %d, %d x %d: forward + backward (dx, dW, dbias), microseconds of device time, median of %d (min .. max)"
        % (B, S, S, args.iters))
    out("%-44s %-32s %-32s %s" % ("layer", "ours", "torch fp32 NCHW", "ours / fp32"))
    g = torch.Generator(device="cpu").manual_seed(5)

    def rand(*shape, scale=1.0):
        return (torch.randn(shape, generator=g) * scale).to(DEV)

    # ---- the plain and the batched convolution
    for cin, cout, n_split, where in ((512, 64, 1, "shared_conv"), (64, 384, 6, "the leading convolutions of six branches")):
        x32, w32, b32, dy32 = rand(B, cin, S, S), rand(cout, cin, 3, 3, scale=0.05), rand(cout), rand(B, cout, S, S)
        x_nhwc = x32.permute(0, 2, 3, 1).contiguous().to(BF).requires_grad_(True)
        dy_nhwc = dy32.permute(0, 2, 3, 1).contiguous().to(BF)
        w_a, b_a = w32.clone().requires_grad_(True), b32.clone().requires_grad_(True)
        x_f = x32.clone().requires_grad_(True)
        ws = [w.clone().requires_grad_(True) for w in w32.chunk(n_split)]
        bs = [b.clone().requires_grad_(True) for b in b32.chunk(n_split)]
        dys = [d.contiguous() for d in dy32.chunk(n_split, dim=1)]

        def ours():
            return torch.autograd.grad(dense_train.conv2d_bf16(x_nhwc, w_a, 3, bias=b_a), [x_nhwc, w_a, b_a], dy_nhwc)

        def fp32():
            return torch.autograd.grad([F.conv2d(x_f, w, b, padding=1) for w, b in zip(ws, bs)], [x_f] + ws + bs, dys)

        t = timed_each({"ours": ours, "fp32": fp32}, args.iters)
        ratio, note = verdict(t["ours"], t["fp32"])
        out("%-44s %-32s %-32s %6.2f%s   %s" % ("%d -> %d%s" % (cin, cout, "" if n_split == 1 else " (fp32: %d x %d -> %d)" % (n_split, cin, cout // n_split)),
                                                 fmt(t["ours"]), fmt(t["fp32"]), ratio, note, where))
        del x32, w32, dy32, x_nhwc, dy_nhwc, x_f, dys
        torch.cuda.empty_cache()
    # ---- the tail
    G = len(TAIL_K)
    wide = rand(B, S, S, 64 * G).to(BF).requires_grad_(True)
    ws = [rand(k, 64, 3, 3, scale=0.05).requires_grad_(True) for k in TAIL_K]
    bs = [rand(k).requires_grad_(True) for k in TAIL_K]
    dys = [rand(B, k, S, S) for k in TAIL_K]
    xs_f = [wide.detach()[..., 64 * i:64 * i + 64].permute(0, 3, 1, 2).float().contiguous().requires_grad_(True) for i in range(G)]
    ws_f = [w.detach().clone().requires_grad_(True) for w in ws]
    bs_f = [b.detach().clone().requires_grad_(True) for b in bs]

    def ours_tail():
        ys = dense_train.head_tail_bf16([(wide, w, b, 64 * i) for i, (w, b) in enumerate(zip(ws, bs))])
        return torch.autograd.grad(ys, [wide] + ws + bs, dys)

    def fp32_tail():
        ys = [F.conv2d(x, w, b, padding=1) for x, w, b in zip(xs_f, ws_f, bs_f)]
        return torch.autograd.grad(ys, xs_f + ws_f + bs_f, dys)

    t = timed_each({"ours": ours_tail, "fp32": fp32_tail}, args.iters)
    ratio, note = verdict(t["ours"], t["fp32"])
    out("%-44s %-32s %-32s %6.2f%s   %s" % ("tail: 6 x 64 -> %s" % (TAIL_K,), fmt(t["ours"]), fmt(t["fp32"]), ratio, note,
                                             "the final convolutions of a SepHead, one launch per pass"))
    wd, dxw = [w.detach() for w in ws], torch.empty_like(wide.detach())
    parts = timed_each({
        "forward": lambda: hip_ops.head_tail_forward([(wide.detach(), 64 * i, w, b.detach()) for i, (w, b) in enumerate(zip(wd, bs))]),
        "dx": lambda: hip_ops.head_tail_dgrad([(dxw, 64 * i, w, dy) for i, (w, dy) in enumerate(zip(wd, dys))]),
        "dW + dbias": lambda: hip_ops.head_tail_wgrad([(wide.detach(), 64 * i, 64, dy) for i, dy in enumerate(dys)])}, args.iters)
    out("%-44s %s" % ("", "   ".join("%s %.1f" % (k, np.median(v)) for k, v in parts.items())))
    out()
    del wide, xs_f, dys, dxw
    torch.cuda.empty_cache()


def head(args, out, variant):
    cfg = centerpoint_config(variant)
    hd = dict(cfg.model["bbox_head"])
    hd.pop("type")
    torch.manual_seed(0)
    hm = CenterHead(**hd)
    hm.load_state_dict(seeded_state_dict(hm, 4), strict=False)
    hm = hm.to(DEV).train()
    cin = hd["in_channels"] if isinstance(hd["in_channels"], int) else sum(hd["in_channels"])
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn((args.batch, cin, 180, 180), generator=g).to(DEV)
    names = [(i, k) for i, d in enumerate(hm.forward_modules(x)) for k in d if k != "feats"]
    hm.zero_grad(set_to_none=True)
    dys = None

    def step(dtype):
        nonlocal dys
        hm.train_dtype = dtype
        hm.zero_grad(set_to_none=True)
        ret = hm(x)
        outs = [ret[i][k] for i, k in names]
        if dys is None:
            dys = [torch.randn_like(t) for t in outs]
        torch.autograd.backward(outs, dys)

    step(torch.float32)
    runs = [timed_each({dt: (lambda dt=dt: step(dt)) for dt in (torch.float32, BF)}, args.model_iters) for _ in range(3)]
    out("b. %s CenterHead (%d tasks, %d maps), train mode, forward + backward, B = %d, milliseconds of device time (three medians of %d) and "
        "max_memory_allocated" % (variant, len(hm.tasks), len(names), args.batch, args.model_iters))
    med, spread = {}, {}
    for dt in (torch.float32, BF):
        hm.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        step(dt)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        ms = [float(np.median(r[dt])) / 1000.0 for r in runs]
        med[dt], spread[dt] = float(np.median(ms)), max(ms) - min(ms)
        out("   train_dtype = %-15s %s   median %8.2f ms   peak %8.1f MiB" % (dt, " ".join("%8.2f" % m for m in ms), med[dt], peak / 2 ** 20))
    faster = med[torch.float32] - med[BF] > spread[torch.float32]
    out("   bf16 / fp32 = %.2f%s" % (med[BF] / med[torch.float32], "" if faster else "   <-- the bf16 head is NOT faster by more than the spread"))
    out()
    hm.train_dtype = torch.float32
    del hm, x, dys
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
    net.backbone.train_dtype = net.neck.train_dtype = BF
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

    out("c. one training iteration of forecast_n0, B = %d, %d-point synthetic clouds, backbone and neck in bf16, fused_bn on the backbone, "
        "fused_loss: ms per step on the host clock between two synchronisations, median of %d (min .. max)" % (B, args.points, args.step_runs))
    for name, fn in (("eager  solver.train_steps", eager), ("static StaticTrainStep", lambda: static(batch)),
                     ("static, check=False", lambda: static(batch, check=False))):
        res = {}
        for dt in (torch.float32, BF, torch.float32, BF):  # each side twice, alternating; the two sample sets are pooled
            net.bbox_head.train_dtype = dt
            for _ in range(2):
                fn()
            res.setdefault(dt, []).append(tsb.timed(fn, args.step_runs))
        t32, t16 = np.concatenate(res[torch.float32]), np.concatenate(res[BF])
        faster = np.median(t32) - np.median(t16) > t32.max() - t32.min()
        out("   %-28s head fp32 %8.2f (%.2f .. %.2f)   head bf16 %8.2f (%.2f .. %.2f)   bf16 / fp32 = %.2f%s" % (
            name, np.median(t32), t32.min(), t32.max(), np.median(t16), t16.min(), t16.max(), np.median(t16) / np.median(t32),
            "" if faster else "   <-- the bf16 head is NOT faster by more than the spread"))
    net.bbox_head.train_dtype = BF
    n_sync = tsb.syncs_per_step(lambda: static(batch, check=False))
    out("   host synchronisations per static step (check=False) with the bf16 head: %.1f" % n_sync)
    out()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-iters", type=int, default=5)
    ap.add_argument("--step-runs", type=int, default=10)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_bf16.txt"))
    args = ap.parse_args()
    out = Out(args.out)
    out("# tools/head_train_bench.py --batch %d, %s, torch %s; tail weight-gradient chunk %d pixels, %d groups per launch"
        % (args.batch, torch.cuda.get_device_name(0), torch.__version__, hip_ops.head_tail_wgrad_chunk(), hip_ops.head_tail_max_groups()))
    per_layer(args, out)
    for variant in ("forecast_n0", "forecast_n3dtf"):
        head(args, out, variant)
    if not args.skip_step:
        whole_step(args, out)


if __name__ == "__main__":
    main()
