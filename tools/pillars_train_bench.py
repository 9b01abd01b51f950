"""Times the train-mode PointPillars reader (fd_pillar_train_forward / _backward) on full train-cap samples: a 300k-point
synthetic_cloud voxelised at the pp geometry with max_voxel_num[0] = 30 000 pillars of 20 slots, B = 1 and B = 4.

Reports device-event medians after warm-up for the reader's forward and backward, the same maths as torch eager fp32 ops (an A/B
partner for this tool only), and one whole PointPillars training step (forward with return_loss, backward, SGD).  FLOPs are
counted from the shapes as the reference evaluates them (layer 1 and layer 2 Linear; in the backward layer 2's weight and input
gradients and layer 1's weight gradient) against the 157 TF/s fp32 peak.

    python tools/pillars_train_bench.py [--out profiles/pillars_train_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from futuredet_amd import hip_ops  # noqa: E402
from futuredet_amd.configs import pointpillars_config  # noqa: E402
from futuredet_amd.readers import PillarFeatureNet  # noqa: E402
from futuredet_amd.synth import seeded_state_dict, synthetic_cloud  # noqa: E402
from futuredet_amd.voxelize import points_to_voxel  # noqa: E402

DEV = "cuda:0"
PEAK = 157.3e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def batch(B, vg):
    vs, cs, ns = [], [], []
    for b in range(B):
        pts = torch.from_numpy(synthetic_cloud(seed=100 + b, target_points=300000)).to(DEV)
        v, c, n = points_to_voxel(pts, vg["voxel_size"], vg["range"], vg["max_points_in_voxel"], True, vg["max_voxel_num"][0])
        vs.append(v)
        cs.append(torch.nn.functional.pad(c.int(), (1, 0), value=b))
        ns.append(n.int())
    return torch.cat(vs).contiguous(), torch.cat(ns).contiguous(), torch.cat(cs).contiguous()


def eager(voxels, num, coors, net, ps, dout):
    """fp32 torch ops restatement (pillar_encoder.py:38-55, :113-164 on batch statistics) with autograd."""
    f = voxels
    M, P, _ = f.shape
    mean = f[:, :, :3].sum(1, keepdim=True) / num.float().view(-1, 1, 1)
    cx = coors[:, 3].float() * net.vx + net.x_offset
    cy = coors[:, 2].float() * net.vy + net.y_offset
    x = torch.cat([f, f[:, :, :3] - mean, (f[:, :, 0] - cx[:, None])[..., None], (f[:, :, 1] - cy[:, None])[..., None]], -1)
    x = x * (torch.arange(P, device=f.device)[None, :] < num[:, None]).float()[..., None]
    w1, g1, b1, w2, g2, b2 = ps
    z1 = x @ w1.t()
    a1 = torch.relu(torch.nn.functional.batch_norm(z1.reshape(-1, 32), None, None, g1, b1, True, 0.0, 1e-3)).view(M, P, 32)
    in2 = torch.cat([a1, a1.max(1, keepdim=True)[0].expand(-1, P, -1)], -1)
    z2 = in2 @ w2.t()
    out = torch.relu(torch.nn.functional.batch_norm(z2.reshape(-1, 64), None, None, g2, b2, True, 0.0, 1e-3)).view(M, P, 64).max(1)[0]
    torch.autograd.backward(out, dout)


def train_step_fn(B, vg):
    from futuredet_amd import build_detector
    from futuredet_amd.synth import tame_box_dims
    from futuredet_amd.targets import TargetAssigner

    cfg = pointpillars_config()
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    sd = tame_box_dims(seeded_state_dict(net, 9))
    sd["reader.pfn_layers.0.linear.weight"] = sd["reader.pfn_layers.0.linear.weight"] * 0.02
    net.load_state_dict(sd, strict=False)
    net = net.to(DEV).train()
    voxels, num, coors = batch(B, vg)
    grid = np.array([512, 512, 1])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    rng = np.random.default_rng(4)
    T, n = cfg.timesteps, 24
    boxes = np.zeros((B, T, n, 12), np.float32)
    boxes[..., 0:2] = rng.uniform(-45, 45, (B, T, n, 2))
    boxes[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32)
    boxes[..., 6:10] = rng.normal(0, 2, (B, T, n, 4))
    args = [torch.from_numpy(a).to(DEV) for a in (boxes, np.full((B, T), n, np.int32), np.ones((B, T, n), np.int32),
                                                    rng.integers(0, 3, (B, T, n)).astype(np.int32))]
    targets = ta(args[0], args[1], args[2], args[3] if ta.extra_sets else None)
    ex = dict(voxels=voxels, coordinates=coors, num_points=num, num_voxels=torch.tensor([int((coors[:, 0] == b).sum()) for b in range(B)]),
              shape=np.array([grid] * B), metadata=[None] * B)
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-6)

    def step():
        opt.zero_grad()
        loss = sum(net(ex, return_loss=True)["loss"])
        loss.backward()
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pillars_train_bench.txt"))
    args = ap.parse_args()
    vg = pointpillars_config().voxel_generator
    lines = ["# tools/pillars_train_bench.py on %s (torch %s): train-mode PillarFeatureNet, median of %d after %d warm-up, device events"
             % (torch.cuda.get_device_name(0), torch.__version__, args.iters, args.warmup)]
    for B in (1, 4):
        voxels, num, coors = batch(B, vg)
        M, P, _ = voxels.shape
        net = PillarFeatureNet(num_input_features=5, num_filters=[64, 64], voxel_size=vg["voxel_size"], pc_range=vg["range"])
        net.load_state_dict(seeded_state_dict(net, 3), strict=False)
        net = net.to(DEV).train()
        l1, l2 = net.pfn_layers
        ps = [t.detach().contiguous() for t in (l1.linear.weight, l1.norm.weight, l1.norm.bias, l2.linear.weight, l2.norm.weight,
                                                 l2.norm.bias)]
        geom = (net.vx, net.vy, net.x_offset, net.y_offset)
        dout = torch.randn((M, 64), device=DEV)
        ws = torch.empty((hip_ops.pillar_train_workspace_bytes(M, P),), dtype=torch.uint8, device=DEV)
        out = torch.empty((M, 64), device=DEV)

        def fwd():
            hip_ops.pillar_train_forward(voxels, num, coors, geom, ps[0], ps[1], ps[2], 1e-3, ps[3], ps[4], ps[5], 1e-3, out=out, workspace=ws)

        def bwd():
            hip_ops.pillar_train_backward(dout, voxels, num, coors, geom, *ps, ws)

        t_f = timed(fwd, args.warmup, args.iters)
        t_b = timed(bwd, args.warmup, args.iters)
        eps = [p.clone().requires_grad_(True) for p in ps]
        t_e = timed(lambda: eager(voxels, num, coors, net, eps, dout), args.warmup, args.iters)
        N, fin = M * P, 10
        flop_f = 2.0 * N * (fin * 32 + 64 * 64)
        flop_b = 2.0 * N * (2 * 64 * 64 + fin * 32)
        lines.append("B=%d  pillars %d x %d slots (N = %d rows, %.0f%% padding)" % (B, M, P, N, 100.0 * (1 - float(num.sum()) / N)))
        lines.append("  reader train forward   %9.1f us   %.2f GFLOP  %.2f%% of fp32 peak" % (t_f, flop_f / 1e9, 100 * flop_f / (t_f * 1e-6) / PEAK))
        lines.append("  reader train backward  %9.1f us   %.2f GFLOP  %.2f%% of fp32 peak" % (t_b, flop_b / 1e9, 100 * flop_b / (t_b * 1e-6) / PEAK))
        lines.append("  forward + backward     %9.1f us   %.2f GFLOP  %.2f%% of fp32 peak" % (t_f + t_b, (flop_f + flop_b) / 1e9,
                                                                                            100 * (flop_f + flop_b) / ((t_f + t_b) * 1e-6) / PEAK))
        lines.append("  torch eager fp32 A/B   %9.1f us   (forward + backward, same maths)" % t_e)
        del eps
        torch.cuda.empty_cache()
        step = train_step_fn(B, vg)
        lines.append("  whole pp training step %9.1f us   (forward with return_loss, backward, SGD)" % timed(step, 2, max(5, args.iters // 2)))
        del step
        torch.cuda.empty_cache()
        print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
