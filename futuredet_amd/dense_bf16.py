"""Execution plan of the RPN neck + CenterHead on the hand-written MFMA convolutions: bf16 (fd_conv2d_nhwc_bf16,
v_mfma_f32_32x32x16_bf16) and fp32 (fd_conv2d_nhwc_f32, v_mfma_f32_16x16x4_f32).

Activations are NHWC tensors of the plan's dtype; BatchNorm is folded; the RPN concat is written in place (channel offsets), the
2x2 stride-2 transposed convolution runs as four 1x1 convolutions writing interleaved pixels, and the six branches
of a SepHead run as one 64->384 convolution followed by one block-diagonal 384->(9+2T) convolution.
Built lazily from the torch modules (so state_dict loading is unchanged) and cached until the next load.
"""
import os

import torch

from . import hip_ops
from .nn_utils import fold_stack


USE_WINOGRAD = not os.environ.get("FD_NO_WINOGRAD")  # A/B switch: fp32 3x3 layers on the direct kernel only


def granule(dtype):
    """input-channel granule of the convolution kernel of ``dtype`` (one LDS slice)"""
    return 32 if dtype == torch.bfloat16 else 16


class _Conv(object):
    def __init__(self, w_oihw, bias, stride, relu, dtype):
        self.cout, self.cin, self.ks, _ = w_oihw.shape
        self.stride, self.relu, self.dtype = stride, relu, dtype
        if self.cin % granule(dtype):
            raise ValueError("conv plan: %d input channels are not a multiple of %d" % (self.cin, granule(dtype)))
        self.wpk = hip_ops.pack_conv2d_weight(w_oihw) if dtype == torch.bfloat16 else hip_ops.pack_conv2d_weight_f32(w_oihw)
        self.bias = bias.float().contiguous() if bias is not None else None
        self.fn = hip_ops.conv2d_nhwc_bf16 if dtype == torch.bfloat16 else hip_ops.conv2d_nhwc_f32
        # fp32 3x3 stride 1: the Winograd F(2x2,3x3) kernel is the second formulation; its transformed weights are packed too
        self.wino = (dtype == torch.float32 and self.ks == 3 and stride == 1 and USE_WINOGRAD)
        self.wpk_wino = hip_ops.pack_conv2d_weight_wino(w_oihw) if self.wino else None
        self.choice = {}  # fp32: input shape -> measured-best workgroup tile of the layer's (fixed) formulation

    def _run(self, choice, x, out, co_off, kw):
        kind, tile = choice
        if kind == "wino":
            return hip_ops.conv2d_wino_nhwc_f32(x, self.wpk_wino, self.bias, self.cout, self.relu, out=out, co_off=co_off, tile=tile)
        return self.fn(x, self.wpk, self.bias, self.cout, self.ks, self.stride, self.relu, out=out, co_off=co_off, tile=tile, **kw)

    def _pick(self, x, out, co_off, kw):
        """fp32 only: times the workgroup tile shapes of this layer's formulation once per input shape (eager calls only --
        during a graph capture the default is used) and remembers the fastest.  The FORMULATION is fixed by rule (Winograd
        for every 3x3 stride-1 layer, direct otherwise): Winograd and direct round differently, so a timing-dependent
        choice between them would make the network's output bits depend on noise and differ between ranks.  Tile shapes of
        one formulation give bit-identical results (every output element sums its channels and taps in the same order
        whatever the tile; tests/test_gpu_parity.py::test_dense_conv_tiles_bit_identical), so only speed is tuned."""
        key = tuple(x.shape)
        c = self.choice.get(key)
        if c is not None:
            return c
        default = ("wino", 0) if (self.wino and not kw) else ("direct", 0)
        if torch.cuda.is_current_stream_capturing():
            return default
        if out is None:
            out = self._run(default, x, None, co_off, kw)
        if default[0] == "wino":  # (the Winograd entry point has no pixel-stride placement; 3x3 layers never need it)
            cands = [("wino", t) for t in range(0, hip_ops.conv2d_wino_f32_num_tiles() + 1)]
        else:
            cands = [("direct", t) for t in range(0, hip_ops.conv2d_f32_num_tiles() + 1)]
        best, best_ms = default, float("inf")
        for cand in cands:
            try:
                self._run(cand, x, out, co_off, kw)
                ms = float("inf")
                for _ in range(3):  # the best of three groups of four launches: one disturbed group must not decide the layer's tile
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(4):
                        self._run(cand, x, out, co_off, kw)
                    e1.record()
                    e1.synchronize()
                    ms = min(ms, e0.elapsed_time(e1))
            except hip_ops.FutureDetHipError:
                continue
            if ms < best_ms * 0.98:  # ties go to the earlier candidate
                best, best_ms = cand, ms
        self.choice[key] = best
        return best

    def __call__(self, x, out=None, co_off=0, **kw):
        if self.dtype == torch.float32:
            return self._run(self._pick(x, out, co_off, kw), x, out, co_off, kw)
        return self.fn(x, self.wpk, self.bias, self.cout, self.ks, self.stride, self.relu, out=out, co_off=co_off, **kw)


class _GroupedConv(object):
    """fd_conv2d_grouped_nhwc_f32: the final 3x3 convolutions of a SepHead's branches in one launch (fp32)."""

    def __init__(self, wpk, bias, counts, cin_g):
        self.wpk, self.bias, self.counts, self.cin_g = wpk, bias, counts, cin_g

    def __call__(self, x, out=None):
        return hip_ops.conv2d_grouped_nhwc_f32(x, self.wpk, self.bias, self.counts, self.cin_g, relu=False, out=out)


def _convs_from_stack(modules, dtype):
    out = []
    for f in fold_stack(modules, torch.float32, False):
        assert not f.transposed
        assert (f.weight.shape[-1] == 3 and f.padding == 1) or (f.weight.shape[-1] == 1 and f.padding == 0), \
            "only 3x3 pad 1 / 1x1 pad 0 convolutions appear in the RPN / head"
        out.append(_Conv(f.weight, f.bias, f.stride, f.relu, dtype))
    return out


class RPNPlan(object):
    def __init__(self, rpn, dtype=torch.bfloat16):
        self.dtype = dtype
        self.blocks = [_convs_from_stack(b._modules.values(), dtype) for b in rpn.blocks]
        self.start = rpn.first_up
        self.deblocks = []
        for d in rpn.deblocks:
            mods = list(d._modules.values())
            f = fold_stack(mods, torch.float32, False)[0]
            if f.transposed:  # ConvTranspose2d(k = s): weight [Cin, Cout, k, k] -> k*k 1x1 convs on interleaved pixels
                k = f.weight.shape[-1]
                assert f.stride == k and f.padding == 0
                if dtype == torch.float32 and f.weight.shape[1] % 4 == 0 and f.weight.shape[0] % 16 == 0:
                    # one 1x1 convolution to (dy, dx, co) virtual channels + pixel-shuffle epilogue
                    w = f.weight.permute(2, 3, 1, 0).reshape(-1, f.weight.shape[0])[:, :, None, None].contiguous()
                    self.deblocks.append(("shuffle", k, (hip_ops.pack_conv2d_weight_f32(w), f.bias.float().contiguous(), f.relu), f.weight.shape[1]))
                    continue
                subs = [(_Conv(f.weight[:, :, dy, dx].t().contiguous()[:, :, None, None], f.bias, 1, f.relu, dtype), dy, dx)
                        for dy in range(k) for dx in range(k)]
                self.deblocks.append(("up", k, subs, f.weight.shape[1]))
            elif f.weight.shape[-1] == 1:
                assert f.stride == 1 and f.padding == 0
                self.deblocks.append(("conv", 1, _Conv(f.weight, f.bias, 1, f.relu, dtype), f.weight.shape[0]))
            else:
                # Conv2d(k = s, stride s) of an `us stride` 1/s (rpn.py:95-110, the pp configs): space-to-depth + 1x1 conv
                k = f.weight.shape[-1]
                assert f.stride == k and f.padding == 0
                w = f.weight.permute(0, 2, 3, 1).reshape(f.weight.shape[0], -1)[:, :, None, None].contiguous()
                self.deblocks.append(("down", k, _Conv(w, f.bias, 1, f.relu, dtype), f.weight.shape[0]))
        self.cout_total = sum(d[3] for d in self.deblocks)

    def __call__(self, x):  # x [B,H,W,C] of the plan's dtype
        ups = None
        co = 0
        for i, stack in enumerate(self.blocks):
            for conv in stack:
                x = conv(x)
            j = i - self.start
            if j >= 0:
                kind, k, op, cout = self.deblocks[j]
                B, H, W, C = x.shape
                Ho, Wo = (H // k, W // k) if kind == "down" else (H * k, W * k)
                if ups is None:
                    ups = torch.empty((B, Ho, Wo, self.cout_total), dtype=self.dtype, device=x.device)
                assert ups.shape[1] == Ho and ups.shape[2] == Wo
                if kind == "conv":
                    op(x, out=ups, co_off=co)
                elif kind == "shuffle":
                    hip_ops.conv2d_shuffle_nhwc_f32(x, op[0], op[1], cout, k, op[2], out=ups, co_off=co)
                elif kind == "down":
                    xs = x.view(B, Ho, k, Wo, k, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Ho, Wo, k * k * C)
                    op(xs, out=ups, co_off=co)
                else:
                    for sub, dy, dx in op:
                        sub(x, out=ups, co_off=co, osy=k, osx=k, ooy=dy, oox=dx)
                co += cout
        return ups


class HeadMaps(dict):
    """One task's head maps (NCHW-shaped VIEWS of the plan's NHWC output buffer, in the plan's dtype) plus ``raw`` =
    (buffer [T, B, H, W, C_total], task index, {name: (first channel, channels)}): CenterHead.predict_padded hands the buffer to the
    decode kernels as it is (fd_map_view), without .float() / .contiguous() passes per map."""
    raw = None


class HeadPlan(object):
    """CenterHead: shared conv, then per task one fused first conv and one block-diagonal final conv.  A DCN task (dcn_head,
    center_head.py:176-229) first runs its two FeatureAdaption modules as one fd_deform_adapt_nhwc launch into a [B,H,W,128]
    buffer (cls adaption in channels 0-63, reg in 64-127); its cls_head joins the fused convs as the ``hm`` branch.
    With forecast_feature (n3dtf, center_head.py:119-124,383-386) each task first runs its two forecast convs; task
    i > 0 reads cat[x, feats_{i-1}], which is laid out in place: two ping-pong [B,H,W,2c] buffers hold x in channels
    [0,c) and receive the previous task's feats in [c,2c) (task 0 reads the same buffer through zero weights)."""

    def __init__(self, head, dtype=torch.bfloat16):
        self.dtype = dtype
        self.shared = _convs_from_stack(head.shared_conv, dtype)
        # bev_map branch (center_head.py:336-341,380-381: x = shared_conv(x) + bev_conv(bev_map)): three 3x3 convs from 6 map
        # channels; the 6 channels are padded to the kernel's input granule with zero weights
        self.bev = None
        if head.bev_map:
            st = fold_stack(head.bev_conv, torch.float32, False)
            g = granule(dtype)
            w0 = st[0].weight
            self.bev_cin = w0.shape[1]
            w0 = torch.cat([w0, torch.zeros((w0.shape[0], (-w0.shape[1]) % g) + tuple(w0.shape[2:]), dtype=w0.dtype, device=w0.device)], dim=1)
            self.bev = [_Conv(w0, st[0].bias, 1, True, dtype)] + [_Conv(f.weight, f.bias, f.stride, f.relu, dtype) for f in st[1:]]
        self.ff = bool(head.forecast_feature)
        self.tasks = []
        self.adapt = []  # per task: None, or the packed FeatureAdaption pair of a DCN task (hip_ops.pack_deform_adapt)
        self.pre = []
        for ti, task in enumerate(head.tasks):
            if self.ff:
                st = fold_stack(task.forecast_conv, torch.float32, False)
                assert len(st) == 2
                w0 = st[0].weight
                if ti == 0:  # reads [x | stale feats]: zero weights on the second half
                    w0 = torch.cat([w0, torch.zeros_like(w0)], dim=1)
                self.pre.append((_Conv(w0, st[0].bias, 1, True, dtype), _Conv(st[1].weight, st[1].bias, 1, True, dtype)))
            dcn = getattr(task, "task_head", None) is not None  # DCNSepHead (center_head.py:176-229)
            sep = task.task_head if dcn else task
            names = list(sep.heads)
            stacks = [list(getattr(sep, h)._modules.values()) for h in names]
            if dcn:  # hm last, as DCNSepHead.forward adds it after the task_head's maps
                names.append("hm")
                stacks.append(list(task.cls_head._modules.values()))
            firsts, finals = [], []
            for mods in stacks:
                st = fold_stack(mods, torch.float32, False)
                assert len(st) == 2
                firsts.append(st[0])
                finals.append(st[1])
            w1 = torch.cat([f.weight for f in firsts], 0)
            b1 = torch.cat([f.bias for f in firsts], 0)
            adapt = None
            if dcn:
                # one fd_deform_adapt_nhwc launch writes [cls | reg] adapted maps; the fused first conv reads all 128 channels through
                # block weights: the task_head branches see channels 64-127 only, cls_head's first conv (the last 64 outputs) 0-63
                fc, fr = task.feature_adapt_cls, task.feature_adapt_reg
                adapt = hip_ops.pack_deform_adapt(fc.conv_adaption.weight, fr.conv_adaption.weight, fc.conv_offset.weight, fc.conv_offset.bias,
                                                  fr.conv_offset.weight, fr.conv_offset.bias, dtype == torch.bfloat16)
                cin = w1.shape[1]
                n_hm = firsts[-1].weight.shape[0]
                z = torch.zeros_like(w1)
                w1 = torch.cat([torch.cat([z[:-n_hm], w1[:-n_hm]], 1), torch.cat([w1[-n_hm:], z[-n_hm:]], 1)], 0)
                assert w1.shape[1] == 2 * cin
            hc = firsts[0].weight.shape[0]
            couts = [f.weight.shape[0] for f in finals]
            w2 = torch.zeros((sum(couts), hc * len(names), 3, 3), dtype=torch.float32, device=w1.device)
            o = 0
            for i, f in enumerate(finals):
                w2[o:o + couts[i], i * hc:(i + 1) * hc] = f.weight
                o += couts[i]
            b2 = torch.cat([f.bias for f in finals], 0)
            if dtype == torch.float32 and len(names) <= 8 and max(couts) <= 16 and hc % 16 == 0 and finals[0].weight.shape[-1] == 3:
                # the branches' final 3x3 convs as ONE grouped launch (each branch reads only its own hc channels)
                wg = torch.zeros((16 * len(names), hc, 3, 3), dtype=torch.float32, device=w1.device)
                bg = torch.zeros((16 * len(names),), dtype=torch.float32, device=w1.device)
                for i, f in enumerate(finals):
                    wg[16 * i:16 * i + couts[i]] = f.weight
                    bg[16 * i:16 * i + couts[i]] = f.bias
                c2 = _GroupedConv(hip_ops.pack_conv2d_weight_f32(wg), bg.contiguous(), list(couts), hc)
            else:
                c2 = _Conv(w2, b2, 1, False, dtype)
            self.tasks.append((_Conv(w1, b1, 1, True, dtype), c2, names, couts))
            self.adapt.append(adapt)

    def __call__(self, x, bev_map=None):  # x [B,H,W,C] of the plan's dtype (bev_map [B,6,H,W]) -> list of HeadMaps
        if self.bev is not None:
            assert bev_map is not None, "this head has a bev_map branch"
            for conv in self.shared:
                x = conv(x)
            B, H, W, _ = x.shape
            y = torch.zeros((B, H, W, self.bev[0].cin), dtype=self.dtype, device=x.device)
            y[..., : self.bev_cin] = bev_map.permute(0, 2, 3, 1)
            for conv in self.bev:
                y = conv(y)
            x = x + y
            return self._tasks(x, None)
        for conv in self.shared[:-1]:
            x = conv(x)
        last = self.shared[-1]
        hc = last.cout
        if self.ff:
            B, H, W, _ = x.shape
            # The two concat buffers belong to THIS call: sweeps in flight on other streams (and the graphs captured for
            # them) must not share them -- a capture takes them from its own graph pool, an eager call from the caching
            # allocator on its own stream.
            cat = [torch.empty((B, H, W, 2 * hc), dtype=self.dtype, device=x.device) for _ in range(2)]
            # task 0 reads [x | uninitialised] through zero weights: clear that half (0 * Inf = NaN otherwise)
            cat[0][..., hc:].zero_()
            last(x, out=cat[0], co_off=0)
            cat[1][..., :hc].copy_(cat[0][..., :hc])
        else:
            x = last(x)
            cat = None
        return self._tasks(x, cat)

    def _tasks(self, x, cat):
        hc = self.shared[-1].cout
        if self.ff and cat is None:  # (bev_map head: x is already complete; lay the concat buffers out from it)
            B, H, W, _ = x.shape
            cat = [torch.empty((B, H, W, 2 * hc), dtype=self.dtype, device=x.device) for _ in range(2)]
            cat[0][..., hc:].zero_()
            cat[0][..., :hc].copy_(x)
            cat[1][..., :hc].copy_(x)
        rets = []
        zbuf = None
        for ti, (c1, c2, names, couts) in enumerate(self.tasks):
            d = HeadMaps()
            if self.ff:
                p0, p1 = self.pre[ti]
                x = p1(p0(cat[ti & 1]))                             # feats_i, contiguous for this task's heads
                cat[(ti + 1) & 1][..., hc:].copy_(x)                # and behind x for the next task's concat
                d["feats"] = x.permute(0, 3, 1, 2)
            adapt = self.adapt[ti]
            y1 = c1(x if adapt is None else hip_ops.deform_adapt_nhwc(x, adapt[0], adapt[1], adapt[2]))
            uniform = all(tuple(t[3]) == tuple(self.tasks[0][3]) for t in self.tasks)
            if uniform:
                if zbuf is None:  # all tasks have the same branch widths: one [T, B, H, W, C_total] buffer takes every task's final convs
                    Bz, Hz, Wz, _ = y1.shape
                    zbuf = torch.empty((len(self.tasks), Bz, Hz, Wz, int(sum(couts))), dtype=self.dtype, device=y1.device)
                zt = zbuf[ti]
                c2(y1, out=zt)
            else:
                # tasks of different widths (e.g. the 6-task nuScenes head with 1- and 2-class tasks): a buffer per task, and no packed
                # decode (raw = None: CenterHead.predict takes the per-task path) -- a shared buffer sized by the first task would
                # reject or leave stale channels for the wider ones (advisor, round 3)
                zt = c2(y1)
            z = zt.permute(0, 3, 1, 2)  # [B, sum(couts), H, W] view
            o, where = 0, {}
            for name, cn in zip(names, couts):
                d[name] = z[:, o:o + cn]
                where[name] = (o, cn)
                o += cn
            d.raw = (zbuf, ti, where) if uniform else None
            rets.append(d)
        return rets
