"""Training-path timings of the fp32 sparse convolution at the bench cloud (forecast_n0, 300k synthetic points, one sample).

Per convolution of SpMiddleResNetFHD: forward (fd_spconv_apply on device-packed weights), input gradient (weight re-pack +
fd_spconv_apply on the transposed problem), weight gradient (fd_spconv_wgrad) and, as its A/B partner, the same weight gradient
as a torch gather + mm per tap.  Then one whole training step of the detector: forward, CenterHead.loss, backward.

    python tools/spconv_grad_bench.py [--points 300000] [--iters 20] [--out FILE]

``--dtype bf16`` times the mixed-precision path next to the fp32 one in the same run instead: per layer group forward, input gradient and
weight gradient of both (every figure measured in two separate passes over the layers: the table holds their mean, and the largest
relative difference between the two passes is the run-to-run spread), the peak memory of one backbone forward + backward and the whole
training step in both modes.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from futuredet_amd import build_detector, hip_ops  # noqa: E402
from futuredet_amd import sparse as spconv  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    return float(np.median(ts))


def example(cfg, pts, dev, seed=0):
    from oracle import ops as oops

    vg = cfg.voxel_generator
    v, c, n = oops.points_to_voxel(pts, vg["voxel_size"], vg["range"], vg["max_points_in_voxel"], True, vg["max_voxel_num"][1])
    rng = np.random.default_rng(seed)
    ex = dict(voxels=torch.from_numpy(v).to(dev), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(dev),
              num_points=torch.from_numpy(n).to(dev), num_voxels=torch.tensor([len(n)]), shape=np.array([[1440, 1440, 40]]), metadata=[None])
    M = 64
    for key in ("hm", "ind", "mask", "cat", "anno_box"):
        ex[key] = []
    for _ in range(cfg.timesteps):
        ind = torch.from_numpy(rng.choice(180 * 180, M, replace=False)[None].astype(np.int64)).to(dev)
        hm = torch.from_numpy((rng.uniform(0, 0.9, (1, 1, 180, 180)) ** 3).astype(np.float32)).to(dev)
        hm.view(-1)[ind[0]] = 1.0
        ex["hm"].append([hm])
        ex["ind"].append([ind])
        ex["mask"].append([torch.ones((1, M), dtype=torch.uint8, device=dev)])
        ex["cat"].append([torch.zeros((1, M), dtype=torch.int64, device=dev)])
        ex["anno_box"].append([torch.from_numpy(rng.normal(0, 1, (1, M, 10)).astype(np.float32)).to(dev)])
    return ex


def layer_problem(m, x, dev):
    """(name, feats fp32 [n_in, cin_p], w fp32 [K, cin_p, cout_p], nbr, n_out) of one recorded convolution call"""
    out_index, nbr = m.rulebook_for(x)
    K = nbr.shape[0]
    cin_p, cout_p = spconv.pad_channels(m.in_channels), spconv.pad_channels(m.out_channels)
    feats = x.features.detach().float()
    if feats.shape[1] != cin_p:
        feats = torch.nn.functional.pad(feats, (0, cin_p - feats.shape[1]))
    w = torch.zeros((K, cin_p, cout_p), device=dev)
    w[:, : m.in_channels, : m.out_channels] = m.weight.detach().reshape(K, m.in_channels, m.out_channels)
    return "%s %d->%d K%d" % ("subm" if m.subm else "strided", cin_p, cout_p, K), feats.contiguous(), w, nbr, out_index.n


def compare_dtypes(args, net, ex, seen, dev, lines):
    """fp32 and bf16 training kernels of every layer in one run, summed per layer group"""
    dts = (("fp32", torch.float32), ("bf16", torch.bfloat16))
    passes = []
    order = []
    for _ in range(2):
        t = {}
        for m, x in seen:
            name, feats32, w, nbr, n_out = layer_problem(m, x, dev)
            if name not in order:
                order.append(name)
            n_in, cin_p = feats32.shape
            cout_p = w.shape[2]
            dy32 = torch.randn((n_out, cout_p), device=dev)
            inv = None if m.subm else hip_ops.rulebook_transpose(nbr, n_out, n_in)
            for tag, dt in dts:
                feats, dy = feats32.to(dt), dy32.to(dt)
                wpk = hip_ops.pack_spconv_weight_device(w, hip_ops.PACK_PLAIN, dt)
                fwd = timed(lambda: hip_ops.spconv_apply(feats, wpk, None, nbr, n_out, cout_p), args.iters)
                if m.subm:
                    dgrad = timed(lambda: hip_ops.spconv_apply(dy, hip_ops.pack_spconv_weight_device(w, 2, dt), None, nbr, n_in, cin_p), args.iters)
                else:
                    dgrad = timed(lambda: hip_ops.spconv_apply(dy, hip_ops.pack_spconv_weight_device(w, 1, dt), None, inv, n_in, cin_p), args.iters)
                wgrad = timed(lambda: hip_ops.spconv_wgrad(feats, dy, nbr, n_out), args.iters)
                cur = t.setdefault(name, {"n": 0})
                cur["n"] += tag == "fp32"
                for k_, v_ in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
                    cur[tag + k_] = cur.get(tag + k_, 0.0) + v_
        passes.append(t)
    keys = [tag + k_ for k_ in ("fwd", "dgrad", "wgrad") for tag, _ in dts]
    lines.append("%-24s %3s %9s %9s %9s %9s %9s %9s %7s %8s" % ("layer group", "n", "fwd f32", "fwd bf16", "dgrad f32", "dgrad bf16", "wgrad f32",
                                                                  "wgrad bf16", "wg f/b", "spread"))
    tot = dict.fromkeys(keys, 0.0)
    worst = 0.0
    for name in order:
        a, b = passes[0][name], passes[1][name]
        mean = {k_: 0.5 * (a[k_] + b[k_]) for k_ in keys}
        spread = max(abs(a[k_] - b[k_]) / min(a[k_], b[k_]) for k_ in ("fp32wgrad", "bf16wgrad"))
        worst = max(worst, spread)
        for k_ in keys:
            tot[k_] += mean[k_]
        lines.append("%-24s %3d %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %7.2f %7.1f%%" % ((name, a["n"]) + tuple(mean[k_] for k_ in keys) + (
            mean["fp32wgrad"] / mean["bf16wgrad"], 100.0 * spread)))
    lines.append("%-24s %3d %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %7.2f %7.1f%%" % (("sum", len(seen)) + tuple(tot[k_] for k_ in keys) + (
        tot["fp32wgrad"] / tot["bf16wgrad"], 100.0 * worst)))
    lines.append("(spread: the largest relative difference of a group's weight-gradient time between the two passes)")

    # one backbone forward + backward in both modes: peak memory above what is allocated before it, and the time
    feats_in = net.reader(ex["voxels"], ex["num_points"]).detach()
    for tag, dt in dts:
        net.backbone.train_dtype = dt

        def run():
            net.backbone.zero_grad(set_to_none=True)
            bev, _ = net.backbone(feats_in, ex["coordinates"], 1, ex["shape"][0])
            bev.sum().backward()

        t_bb = timed(run, max(3, args.iters // 4))
        net.backbone.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        lines.append("backbone forward + backward, train_dtype %s: %.2f ms, torch.cuda.max_memory_allocated %.1f MiB above the %.1f MiB held before"
                     % (tag, t_bb / 1000.0, peak / 2.0 ** 20, base / 2.0 ** 20))
    net.backbone.zero_grad(set_to_none=True)
    net.backbone.train_dtype = torch.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--variant", default="forecast_n0")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", default="fp32", choices=("fp32", "bf16"), help="bf16: the mixed-precision path next to the fp32 one, per layer group")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = centerpoint_config(args.variant)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(dev).train()
    ex = example(cfg, synthetic_cloud(seed=0, target_points=args.points), dev)
    lines = ["# tools/spconv_grad_bench.py --variant %s --points %d (%d voxels), fp32, median of %d, microseconds"
             % (args.variant, args.points, int(ex["num_voxels"][0]), args.iters)]

    # capture every sparse convolution's input during one training forward
    seen = []
    hooks = [m.register_forward_pre_hook(lambda m, inp: seen.append((m, inp[0]))) for m in net.backbone.modules()
             if isinstance(m, spconv.SparseConvolution)]
    net(ex, return_loss=True)
    for h in hooks:
        h.remove()
    torch.cuda.synchronize()
    if args.dtype == "bf16":
        lines[0] = "# tools/spconv_grad_bench.py --dtype bf16 --variant %s --points %d (%d voxels), fp32 and bf16 in one run, median of %d, microseconds" % (
            args.variant, args.points, int(ex["num_voxels"][0]), args.iters)
        compare_dtypes(args, net, ex, seen, dev, lines)
    else:
        per_layer_fp32(args, seen, dev, lines)

    opt = torch.optim.SGD(net.parameters(), lr=1e-4)

    def step():
        opt.zero_grad()
        ret = net(ex, return_loss=True)
        sum(ret["loss"]).backward()

    def fwd_loss():
        with torch.no_grad():
            net(ex, return_loss=True)

    for dt in (torch.float32, torch.bfloat16) if args.dtype == "bf16" else (torch.float32,):
        net.backbone.train_dtype = dt
        t_step = timed(step, max(3, args.iters // 4))
        t_fwd = timed(fwd_loss, max(3, args.iters // 4))
        mode = ", backbone train_dtype %s" % str(dt).split(".")[-1] if args.dtype == "bf16" else ""
        lines.append("training step (forward + loss + backward, %s, train mode%s): %.2f ms; forward + loss alone (no_grad): %.2f ms"
                     % (args.variant, mode, t_step / 1000.0, t_fwd / 1000.0))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def per_layer_fp32(args, seen, dev, lines):
    lines.append("%-34s %8s %8s %8s %8s %9s %10s %10s %8s" % ("layer", "n_in", "n_out", "pairs", "fwd", "dgrad", "wgrad", "torch_wg", "wg/fwd"))
    tot = dict(fwd=0.0, dgrad=0.0, wgrad=0.0, torch=0.0)
    for li, (m, x) in enumerate(seen):
        out_index, nbr = m.rulebook_for(x)
        K = nbr.shape[0]
        cin_p, cout_p = spconv.pad_channels(m.in_channels), spconv.pad_channels(m.out_channels)
        feats = x.features.detach()
        if feats.shape[1] != cin_p:
            feats = torch.nn.functional.pad(feats, (0, cin_p - feats.shape[1]))
        feats = feats.contiguous()
        w = torch.zeros((K, cin_p, cout_p), device=dev)
        w[:, : m.in_channels, : m.out_channels] = m.weight.detach().reshape(K, m.in_channels, m.out_channels)
        n_in, n_out = feats.shape[0], out_index.n
        dy = torch.randn((n_out, cout_p), device=dev)
        wpk = hip_ops.pack_spconv_weight_device(w)
        fwd = timed(lambda: hip_ops.spconv_apply(feats, wpk, None, nbr, n_out, cout_p), args.iters)
        if m.subm:
            dgrad = timed(lambda: hip_ops.spconv_apply(dy, hip_ops.pack_spconv_weight_device(w, 2), None, nbr, n_in, cin_p), args.iters)
        else:
            inv = hip_ops.rulebook_transpose(nbr, n_out, n_in)
            dgrad = timed(lambda: hip_ops.spconv_apply(dy, hip_ops.pack_spconv_weight_device(w, 1), None, inv, n_in, cin_p), args.iters)
        wgrad = timed(lambda: hip_ops.spconv_wgrad(feats, dy, nbr, n_out), args.iters)
        tab = nbr[:, :n_out].long()
        lists = [(tab[k][tab[k] >= 0], torch.nonzero(tab[k] >= 0)[:, 0]) for k in range(K)]
        pairs = sum(int(i.numel()) for i, _ in lists)
        ref = torch.stack([feats[i].T @ dy[o] for i, o in lists])
        got = hip_ops.spconv_wgrad(feats, dy, nbr, n_out)
        err = float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))
        tw = timed(lambda: torch.stack([feats[i].T @ dy[o] for i, o in lists]), args.iters)
        name = "%02d %s %d->%d K%d" % (li, "subm" if m.subm else "strided", cin_p, cout_p, K)
        lines.append("%-34s %8d %8d %8d %8.1f %9.1f %10.1f %10.1f %8.2f  (wgrad vs torch: rel err %.1e)"
                     % (name, n_in, n_out, pairs, fwd, dgrad, wgrad, tw, wgrad / fwd, err))
        for k_, v_ in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad), ("torch", tw)):
            tot[k_] += v_
    lines.append("%-34s %8s %8s %8s %8.1f %9.1f %10.1f %10.1f %8.2f" % ("sum", "", "", "", tot["fwd"], tot["dgrad"], tot["wgrad"], tot["torch"],
                                                                       tot["wgrad"] / tot["fwd"]))


if __name__ == "__main__":
    main()
