"""Times the DCN head pieces on the device: fd_deform_adapt_nhwc alone (fp32 / bf16, offsets computed in the kernel vs a separate
fp32 1x1 offset convolution feeding the kernel's offsets input), and a whole n3 CenterHead with and without dcn_head on the
convolution plan.  B = 2, 180 x 180, 512 input channels (the n3 configuration).  Prints one JSON line.

    python tools/dcn_bench.py [--iters 50]
    python tools/dcn_bench.py --train [--iters 20] [--out profiles/dcn_train_bench.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/dcn_bench.py --train --trace-only

--train times the training path of one DCNSepHead's FeatureAdaption pair at the same shape, fp32: fd_deform_adapt_backward whole and
by output (dx + doffsets = the data kernel, doffsets alone = the data kernel without its atomic scatter, dw = the partial and the
reduce kernel), the training forward (device weight packing + fd_deform_adapt_nhwc), and forward + backward of the pair through the
kernels (DCNSepHead in .train(), the two torch 1x1 offset convolutions included) against the same pair through
nn_utils.deform_conv2d_v1 on the device (FeatureAdaption.forward, the path before the kernels), with torch's peak allocation of both.
The by-output figures are whole calls: each holds the zero fill of dx and the weight transpose that its kernels need.  The time of
each kernel alone comes from a kernel trace of --trace-only, which runs nothing but the training forward and the full backward
(profiles/dcn_train_kernel_stats.csv).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):  # best of three groups: one disturbed group does not decide
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters)
    return best * 1e3  # us


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20  # MiB above what was live before the step


def train_main(a):
    from futuredet_amd import build, hip_ops, lib
    from futuredet_amd.heads import DCNSepHead

    build.build()
    lib.load()
    B, H, W, C = 2, 180, 180, 64
    out = dict(mode="train", B=B, H=H, W=W)
    torch.manual_seed(0)
    head = DCNSepHead(C, 1, dict(reg=(2, 2), height=(1, 2)), bn=True, final_kernel=3)
    fas = (head.feature_adapt_cls, head.feature_adapt_reg)
    for m in fas:
        m.conv_offset.weight.data.normal_(0, 0.1)
    head = head.cuda().train()
    xc = torch.relu(torch.randn(B, C, H, W, device="cuda"))
    x = xc.permute(0, 2, 3, 1).contiguous()
    wc, wr = fas[0].conv_adaption.weight.detach(), fas[1].conv_adaption.weight.detach()
    with torch.no_grad():
        off = torch.cat([m.conv_offset(xc) for m in fas], 1).permute(0, 2, 3, 1).contiguous()
        y = hip_ops.deform_adapt_nhwc(x, hip_ops.pack_deform_adapt_device(wc, wr), offsets=off)
        dy = torch.randn_like(y)
        if a.trace_only:
            for _ in range(a.iters):
                hip_ops.deform_adapt_nhwc(x, hip_ops.pack_deform_adapt_device(wc, wr), offsets=off)
                hip_ops.deform_adapt_backward(x, off, wc, wr, y, dy)
            torch.cuda.synchronize()
            return
        out["offset_std_px"] = float(off.std())
        out["forward_train_us"] = _time(lambda: hip_ops.deform_adapt_nhwc(x, hip_ops.pack_deform_adapt_device(wc, wr), offsets=off), a.iters)
        for key, need in (("backward_us", (True, True, True)), ("backward_dx_doffsets_us", (True, True, False)),
                          ("backward_doffsets_only_us", (False, True, False)), ("backward_dx_only_us", (True, False, False)),
                          ("backward_dw_us", (False, False, True))):
            out[key] = _time(lambda: hip_ops.deform_adapt_backward(x, off, wc, wr, y, dy, need=need), a.iters)
    atomic_bytes = 2 * 9 * 4 * 256.0 * B * H * W
    out["dx_atomic_gbytes_upper"] = atomic_bytes / 1e9
    out["dx_atomic_floor_us_at_1p3TBps"] = atomic_bytes / 1.3e12 * 1e6
    dyc = torch.randn(B, 2 * C, H, W, device="cuda")
    xg = xc.clone().requires_grad_(True)

    def kernels():
        head.zero_grad(set_to_none=True)
        xg.grad = None
        a_cls, a_reg = head._adapt_pair_train(xg)
        (torch.cat([a_cls, a_reg], 1) * dyc).sum().backward()

    def partner():
        head.zero_grad(set_to_none=True)
        xg.grad = None
        (torch.cat([fas[0](xg), fas[1](xg)], 1) * dyc).sum().backward()

    out["pair_fwd_bwd_kernels_ms"] = _time(kernels, a.iters) / 1e3
    out["pair_fwd_bwd_kernels_peak_mib"] = _peak(kernels)
    out["pair_fwd_bwd_restatement_ms"] = _time(partner, max(a.iters // 10, 2)) / 1e3
    out["pair_fwd_bwd_restatement_peak_mib"] = _peak(partner)
    out["speedup"] = out["pair_fwd_bwd_restatement_ms"] / out["pair_fwd_bwd_kernels_ms"]
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/dcn_bench.py --train --iters %d on %s (torch %s): best of three groups, device events\n%s\n"
                    % (a.iters, torch.cuda.get_device_name(0), torch.__version__, line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--train", action="store_true", help="time the training path of the FeatureAdaption pair")
    ap.add_argument("--trace-only", action="store_true", help="with --train: only run the training forward and the full backward (for a kernel trace)")
    ap.add_argument("--out", default=None, help="with --train: also write the result line to this file")
    a = ap.parse_args()
    if a.train:
        a.iters = a.iters or 20
        return train_main(a)
    a.iters = a.iters or 50
    from futuredet_amd import build, build_head, hip_ops, lib
    from futuredet_amd.heads import FeatureAdaption
    from futuredet_amd.synth import seeded_state_dict

    build.build()
    lib.load()
    B, H, W, C = 2, 180, 180, 64
    out = dict(B=B, H=H, W=W)
    torch.manual_seed(0)
    fa = [FeatureAdaption(C, C) for _ in range(2)]
    for m in fa:
        m.conv_offset.weight.data.normal_(0, 0.1)
    x = torch.relu(torch.randn(B, H, W, C, device="cuda"))
    w_off = torch.cat([m.conv_offset.weight for m in fa], 0).cuda()   # [144, 64, 1, 1]
    b_off = torch.cat([m.conv_offset.bias for m in fa], 0).cuda()
    wpk_off = hip_ops.pack_conv2d_weight_f32(w_off)
    with torch.no_grad():
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            wpk, ow, ob = hip_ops.pack_deform_adapt(fa[0].conv_adaption.weight, fa[1].conv_adaption.weight, fa[0].conv_offset.weight,
                                                    fa[0].conv_offset.bias, fa[1].conv_offset.weight, fa[1].conv_offset.bias, dt == torch.bfloat16)
            wpk, ow, ob = wpk.cuda(), ow.cuda(), ob.cuda()
            xd = x.to(dt).contiguous()
            y = torch.empty((B, H, W, 2 * C), dtype=dt, device="cuda")
            out["deform_fused_us_" + name] = _time(lambda: hip_ops.deform_adapt_nhwc(xd, wpk, ow, ob, out=y), a.iters)
            if dt == torch.float32:  # the alternative: the existing fp32 1x1 conv (64 -> 144) writes the offsets, the kernel reads them
                offs = torch.empty((B, H, W, 144), dtype=torch.float32, device="cuda")

                def split():
                    hip_ops.conv2d_nhwc_f32(x, wpk_off, b_off, 144, 1, relu=False, out=offs)
                    hip_ops.deform_adapt_nhwc(x, wpk, offsets=offs, out=y)

                out["deform_split_us_fp32"] = _time(split, a.iters)
                out["offset_conv1x1_us_fp32"] = _time(lambda: hip_ops.conv2d_nhwc_f32(x, wpk_off, b_off, 144, 1, relu=False, out=offs), a.iters)
        flop = 2.0 * B * H * W * 2 * C * 9 * C  # the two deformable GEMMs (the offset 1x1 adds 2 * B H W * 144 * 64)
        out["deform_gflop"] = flop / 1e9
        out["fp32_mfma_floor_us"] = flop / 157.3e12 * 1e6
        out["fp32_fraction_of_mfma_peak"] = out["fp32_mfma_floor_us"] / out["deform_fused_us_fp32"]
        for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            for dcn in (False, True):
                head = build_head(dict(type="CenterHead", in_channels=512, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes",
                                       weight=0.25, code_weights=[1.0] * 10,
                                       common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
                                       share_conv_channel=64, dcn_head=dcn, timesteps=7, classify=False))
                head.load_state_dict(seeded_state_dict(head, 3), strict=False)
                head = head.cuda().eval()
                head.compute_dtype = dt
                xh = torch.randn(B, 512, H, W, device="cuda")
                out["head_%s_ms_%s" % ("dcn" if dcn else "plain", name)] = _time(lambda: head(xh), a.iters // 5 + 1) / 1e3
            out["dcn_added_ms_" + name] = out["head_dcn_ms_" + name] - out["head_plain_ms_" + name]
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
