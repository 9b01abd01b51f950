"""Training-mode BatchNorm of the sparse backbone at the bench cloud (forecast_n0's SpMiddleResNetFHD, 300k synthetic points, one sample):
the fused kernels (sparse.batch_norm_act, fd_row_bn.h behind fd_sparse_bn.hip) against the module chain they replace, in the same run.

Per backbone level, on features of the level's size: forward + backward of  relu(bn(x))  and  relu(bn(x) + identity)  -- fused, and as
nn.BatchNorm1d / add / relu through autograd; each both issued from Python and as one captured graph (device time without launch
gaps).  Then the whole backbone in train mode, forward + backward, with fused_bn off and on: device time and
torch.cuda.max_memory_allocated.  Device events, median; the sides of every comparison alternate inside one timing loop.

--dtype bf16 is the mixed-precision form (train_dtype = torch.bfloat16).  Per level, in one alternating loop: the fused call on bf16
rows, the module chain as SpMiddleResNetFHD._bn_act runs it without fused_bn (bn(x.float()) [+ residual.float()], relu_to_bf16), and the
fused call on fp32 rows of the same count; the bytes the fused bf16 call must move (forward: x twice, the residual, y; backward: dy, y
and x twice, dx, d_residual) over its graph time.  Then the whole mixed-precision backbone with fused_bn off and on.

    python tools/sparse_bn_bench.py [--points 300000] [--iters 20] [--dtype fp32|bf16] [--out profiles/sparse_bn_bench[_bf16].txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from futuredet_amd import hip_ops  # noqa: E402
from futuredet_amd import sparse as spconv  # noqa: E402
from futuredet_amd.backbones import SpMiddleResNetFHD  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.synth import seeded_state_dict, synthetic_cloud  # noqa: E402
from futuredet_amd.voxelize import points_to_voxel  # noqa: E402


def timed_each(fns, iters):
    """median device time of every callable of ``fns`` (a dict), the callables alternating inside one loop so that clocks, caches and the
    allocator's state are shared between the sides"""
    for _ in range(5):
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
    return {k: float(np.median(v)) for k, v in ts.items()}


def levels_bf16(args, dev, levels, lines):
    """per level: fused bf16 | the mixed-precision module chain | fused fp32, without and with the residual, one alternating loop"""
    sides = ("bf16", "chain", "fp32")
    lines.append("bf16 = fused call on bf16 rows; chain = bn(x.float()) [+ res.float()], relu_to_bf16 on the same bf16 rows; fp32 = fused call on fp32 rows")
    lines.append("GB/s = the bytes the fused bf16 call must move (2 rows C (3 [+1 res] forward, 7 [+1 res] backward)) over its graph time")
    lines.append("%-16s %-6s %8s %8s %6s %8s %6s   %8s %8s %6s %8s %6s" % ("level (rows x C)", "", "bf16", "chain", "ratio", "fp32", "GB/s", "bf16+res",
                                                                        "chain+res", "ratio", "fp32+res", "GB/s"))
    for rows, C in levels:
        g = torch.Generator(device="cpu").manual_seed(rows + C)
        x = (torch.randn((rows, C), generator=g) * 0.5 + 0.1).to(dev).to(torch.bfloat16)
        res = torch.randn((rows, C), generator=g).to(dev).to(torch.bfloat16)
        dy = torch.randn((rows, C), generator=g).to(dev).to(torch.bfloat16)
        t16 = dict(x=x.requires_grad_(True), res=res.requires_grad_(True), dy=dy)
        t32 = dict(x=x.detach().float().requires_grad_(True), res=res.detach().float().requires_grad_(True), dy=dy.float())
        bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(dev).train()

        def run(side, with_res):
            t = t32 if side == "fp32" else t16
            r = t["res"] if with_res else None
            if side == "chain":
                y = bn(t["x"].float())
                if with_res:
                    y = y + r.float()
                y = spconv.relu_to_bf16(y)
            else:
                y = spconv.batch_norm_act(t["x"], bn, residual=r, relu=True)
            return torch.autograd.grad(y, [t["x"], bn.weight, bn.bias] + ([r] if with_res else []), t["dy"])

        combos = [(s, r) for s in sides for r in (False, True)]
        eager = timed_each({k: (lambda k=k: run(*k)) for k in combos}, args.iters)
        graphs, keep = {}, []
        for k in combos:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run(*k)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with hip_ops.workspace.scope(("sparse_bn_bench_bf16", rows, C) + k):
                with torch.cuda.graph(graphs[k]):
                    keep.append(run(*k))
        graph = timed_each({k: gr.replay for k, gr in graphs.items()}, args.iters)
        del graphs, keep
        for k in combos:
            hip_ops.workspace.release(("sparse_bn_bench_bf16", rows, C) + k)
        for name, t in (("graph", graph), ("eager", eager)):
            cells = []
            for with_res in (False, True):
                nbytes = 2 * rows * C * (12 if with_res else 10)
                cells += [t["bf16", with_res], t["chain", with_res], t["bf16", with_res] / t["chain", with_res], t["fp32", with_res],
                          nbytes / t["bf16", with_res] / 1e3]
            lines.append("%-16s %-6s %8.1f %8.1f %6.2f %8.1f %6.0f   %8.1f %8.1f %6.2f %8.1f %6.0f" % (("%d x %d" % (rows, C), name) + tuple(cells)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    bf16 = args.dtype == "bf16"
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "sparse_bn_bench_bf16.txt" if bf16 else "sparse_bn_bench.txt")
    dev = torch.device("cuda:0")
    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    v, c, n = points_to_voxel(synthetic_cloud(seed=0, target_points=args.points), vg["voxel_size"], vg["range"], vg["max_points_in_voxel"], True,
                              vg["max_voxel_num"][1])
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32)).to(dev)
    coords = torch.from_numpy(np.pad(c, ((0, 0), (1, 0))).astype(np.int32)).to(dev)
    shape = np.array([1440, 1440, 40])
    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, 5), strict=False)
    bb = bb.to(dev).train()
    lines = ["# tools/sparse_bn_bench.py --points %d%s (%d voxels), %s, median of %d, microseconds of device time (events around forward + backward)"
             % (args.points, " --dtype bf16" if bf16 else "", len(n), args.dtype, args.iters)]

    # the sizes the BatchNorms meet: one per level
    seen = []
    hooks = [m.register_forward_pre_hook(lambda m, inp: seen.append(tuple(inp[0].shape))) for m in bb.modules() if isinstance(m, nn.BatchNorm1d)]
    bb(feats, coords, 1, shape)
    for h in hooks:
        h.remove()
    levels = sorted(set(seen), key=lambda s: -s[0])
    lines.append("graph = the same forward + backward captured once and replayed (device time only); eager = issued from Python (launch gaps included)")
    if bf16:
        levels_bf16(args, dev, levels, lines)
    else:
        lines.append("%-16s %-6s %9s %9s %7s   %9s %9s %7s" % ("level (rows x C)", "", "fused", "modules", "ratio", "fused+res", "mods+res", "ratio"))
    for rows, C in ([] if bf16 else levels):
        g = torch.Generator(device="cpu").manual_seed(rows + C)
        x = (torch.randn((rows, C), generator=g) * 0.5 + 0.1).to(dev).requires_grad_(True)
        res = torch.randn((rows, C), generator=g).to(dev).requires_grad_(True)
        dy = torch.randn((rows, C), generator=g).to(dev)
        bn = nn.BatchNorm1d(C, eps=1e-3, momentum=0.01).to(dev).train()

        def run(fused, with_res):
            r = res if with_res else None
            if fused:
                y = spconv.batch_norm_act(x, bn, residual=r, relu=True)
            else:
                y = bn(x)
                if with_res:
                    y = y + r
                y = torch.relu(y)
            return torch.autograd.grad(y, [x, bn.weight, bn.bias] + ([res] if with_res else []), dy)

        combos = [(f, r) for f in (True, False) for r in (False, True)]
        eager = timed_each({k: (lambda k=k: run(*k)) for k in combos}, args.iters)
        graphs, keep = {}, []
        for k in combos:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run(*k)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with hip_ops.workspace.scope(("sparse_bn_bench", rows, C) + k):
                with torch.cuda.graph(graphs[k]):
                    keep.append(run(*k))
        graph = timed_each({k: g.replay for k, g in graphs.items()}, args.iters)
        del graphs, keep
        for k in combos:
            hip_ops.workspace.release(("sparse_bn_bench", rows, C) + k)
        for name, t in (("graph", graph), ("eager", eager)):
            lines.append("%-16s %-6s %9.1f %9.1f %7.2f   %9.1f %9.1f %7.2f" % ("%d x %d" % (rows, C), name, t[True, False], t[False, False],
                                                                              t[True, False] / t[False, False], t[True, True], t[False, True],
                                                                              t[True, True] / t[False, True]))

    G = None

    if bf16:
        bb.train_dtype = torch.bfloat16

    def step(fused):
        nonlocal G
        bb.fused_bn = fused
        bb.zero_grad(set_to_none=True)
        bev, _ = bb(feats, coords, 1, shape)
        if G is None:
            G = torch.randn_like(bev)
        (bev * G).sum().backward()

    t = timed_each({f: (lambda f=f: step(f)) for f in (False, True)}, max(5, args.iters // 2))
    for fused in (False, True):
        bb.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fused)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        lines.append("backbone train forward + backward%s, fused_bn=%-5s: %8.2f ms   max_memory_allocated %8.1f MiB (%.1f MiB above the %.1f MiB held before the step)"
                     % (", train_dtype=bfloat16" if bf16 else "", fused, t[fused] / 1000.0, peak / 2 ** 20, (peak - base) / 2 ** 20, base / 2 ** 20))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
