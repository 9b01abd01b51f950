"""Training-mode BatchNorm2d + ReLU of the dense half (RPN, CenterHead) at the shipped map shapes, batch 4: the fused kernels
(dense_bn.batch_norm2d_act, fd_dense_bn.hip) against the module chain they replace, in the same run.

Per shape: forward + backward of  relu(bn(x))  -- fused, and as nn.BatchNorm2d / nn.ReLU(inplace=True) through autograd; each both issued
from Python and as one captured graph (device time without launch gaps); the two sides alternate inside one timing loop.  GB/s = the
bytes the fused call must move (4 B C H W (3 forward: x twice and y; 7 backward: dy, y and x twice each, dx)) over its graph time.  A
shape where the fused call does not win is marked.

Then the whole dense half in train mode, RPN + CenterHead forward + backward on a random BEV map, for forecast_n0 and forecast_n3dtf,
with both fused_bn switches off and on: device time, torch.cuda.max_memory_allocated and the peak of the bytes the tensors requested
(torch.cuda.memory_stats: the first counts whole allocator blocks).  The comparison is repeated three times; the
fused side counts as faster where the gap between the medians exceeds the spread of the chain's three medians.

    python tools/dense_bn_bench.py [--batch 4] [--iters 20] [--model-iters 5] [--out profiles/dense_bn_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from futuredet_amd import dense_bn, hip_ops  # noqa: E402
from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.heads import CenterHead  # noqa: E402
from futuredet_amd.necks import RPN  # noqa: E402
from futuredet_amd.synth import seeded_state_dict  # noqa: E402

# (channels, side, where)
SHAPES = [(128, 180, "RPN stage 1"), (256, 90, "RPN stage 2"), (256, 180, "RPN deblocks"), (64, 180, "CenterHead"),
          (64, 256, "PointPillars RPN stage 1"), (128, 128, "PointPillars RPN stage 2, deblocks"), (256, 64, "PointPillars RPN stage 3")]


def timed_each(fns, iters):
    """median device time of every callable of ``fns`` (a dict), the callables alternating inside one loop so that clocks, caches and the
    allocator's state are shared between the sides"""
    for _ in range(3):
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


def per_shape(args, dev, lines):
    lines.append("graph = the same forward + backward captured once and replayed (device time only); eager = issued from Python (launch gaps included)")
    lines.append("%-22s %-6s %9s %9s %7s %7s   %s" % ("shape (B x C x H x W)", "", "fused", "modules", "ratio", "GB/s", "where"))
    losers = []
    for C, side, where in SHAPES:
        B = args.batch
        g = torch.Generator(device="cpu").manual_seed(C + side)
        x = (torch.randn((B, C, side, side), generator=g) * 0.5 + 0.1).to(dev).requires_grad_(True)
        dy = torch.randn((B, C, side, side), generator=g).to(dev)
        bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(dev).train()
        relu = nn.ReLU(inplace=True)

        def run(fused):
            y = dense_bn.batch_norm2d_act(x, bn, relu=True) if fused else relu(bn(x))
            return torch.autograd.grad(y, [x, bn.weight, bn.bias], dy)

        sides = (True, False)
        eager = timed_each({k: (lambda k=k: run(k)) for k in sides}, args.iters)
        graphs, keep = {}, []
        for k in sides:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                run(k)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graphs[k] = torch.cuda.CUDAGraph()
            with hip_ops.workspace.scope(("dense_bn_bench", C, side, k)):
                with torch.cuda.graph(graphs[k]):
                    keep.append(run(k))
        graph = timed_each({k: gr.replay for k, gr in graphs.items()}, args.iters)
        del graphs, keep
        for k in sides:
            hip_ops.workspace.release(("dense_bn_bench", C, side, k))
        nbytes = 4 * B * C * side * side * 10
        name = "%d x %d x %d x %d" % (B, C, side, side)
        for kind, t in (("graph", graph), ("eager", eager)):
            ratio = t[True] / t[False]
            lost = kind == "graph" and ratio >= 1.0
            if lost:
                losers.append(name)
            lines.append("%-22s %-6s %9.1f %9.1f %7.2f %7s   %s%s" % (name, kind, t[True], t[False], ratio,
                                                                   "%.0f" % (nbytes / t[True] / 1e3) if kind == "graph" else "", where,
                                                                   "   <-- the fused call does NOT win" if lost else ""))
        del x, dy
        torch.cuda.empty_cache()
    lines.append("shapes where the fused call does not win (graph time): %s" % (", ".join(losers) if losers else "none"))


def dense_half(args, dev, variant, lines):
    cfg = centerpoint_config(variant)
    nk, hd = dict(cfg.model["neck"]), dict(cfg.model["bbox_head"])
    nk.pop("type"), hd.pop("type")
    torch.manual_seed(0)
    rpn, head = RPN(**nk), CenterHead(**hd)
    rpn.load_state_dict(seeded_state_dict(rpn, 3), strict=False)
    head.load_state_dict(seeded_state_dict(head, 4), strict=False)
    rpn, head = rpn.to(dev).train(), head.to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(11)
    bev = torch.randn((args.batch, nk["num_input_features"], 180, 180), generator=g).to(dev)
    weights = {}

    def step(fused):
        rpn.fused_bn = head.fused_bn = fused
        rpn.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        preds = head(rpn(bev))
        loss = 0.0
        for i, p in enumerate(preds):
            for k in sorted(p):
                if k == "feats":
                    continue
                if (i, k) not in weights:
                    weights[i, k] = torch.randn_like(p[k])
                loss = loss + (p[k] * weights[i, k]).sum()
        loss.backward()

    runs = [timed_each({f: (lambda f=f: step(f)) for f in (False, True)}, args.model_iters) for _ in range(3)]
    chain, fused = [r[False] / 1000.0 for r in runs], [r[True] / 1000.0 for r in runs]
    spread = max(chain) - min(chain)
    gap = float(np.median(chain) - np.median(fused))
    peaks = {}
    for f in (False, True, False, True):  # each side twice: the second reading is reported, a first one that differs is reported too
        rpn.zero_grad(set_to_none=True)
        head.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(f)
        torch.cuda.synchronize()
        now = (torch.cuda.max_memory_allocated(), torch.cuda.memory_stats()["requested_bytes.all.peak"], base)
        if f in peaks and peaks[f] != now:
            lines.append("%s: the peaks of fused_bn=%s did not repeat: %s then %s bytes" % (variant, f, peaks[f], now))
        peaks[f] = now
    for f, ts in ((False, chain), (True, fused)):
        lines.append("%s RPN + CenterHead train forward + backward, batch %d, fused_bn=%-5s: %s ms (three medians of %d), median %8.2f ms   "
                     "max_memory_allocated %8.1f MiB, peak of the requested bytes %8.1f MiB (%.1f MiB held before the step)"
                     % (variant, args.batch, f, " ".join("%8.2f" % t for t in ts), args.model_iters, float(np.median(ts)), peaks[f][0] / 2 ** 20,
                        peaks[f][1] / 2 ** 20, peaks[f][2] / 2 ** 20))
    lines.append("%s: fused - chain = %+.2f ms; spread of the chain's three medians %.2f ms: the fused side is %s"
                 % (variant, -gap, spread, "FASTER by more than the spread" if gap > spread else "NOT faster by more than the spread"))
    for i, what in ((0, "max_memory_allocated (the allocator's blocks, the unsplit remainder of a reused block included)"),
                    (1, "requested bytes (what the tensors asked for)")):
        d = peaks[True][i] - peaks[False][i]
        lines.append("%s: peak %s: fused - chain = %+d bytes: the fused side allocates %s the chain"
                     % (variant, what, d, "no more than" if d <= 0 else "MORE than"))
    del rpn, head, bev, weights
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-iters", type=int, default=5)
    ap.add_argument("--variants", default="forecast_n0,forecast_n3dtf")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_bn_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# tools/dense_bn_bench.py --batch %d, fp32, median of %d, microseconds of device time (events around forward + backward)"
             % (args.batch, args.iters)]
    per_shape(args, dev, lines)
    for variant in [v for v in args.variants.split(",") if v]:
        dense_half(args, dev, variant, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
