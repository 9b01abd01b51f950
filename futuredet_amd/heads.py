"""CenterHead (det3d/models/bbox_heads/center_head.py:81-174 SepHead, :232-390 CenterHead, :542-747 predict).

Constructor signature and state_dict keys follow the reference (shared_conv.{0,1}.*, tasks.{i}.{reg,height,dim,
rot,vel,hm}.{0,1,3}.*, tasks.{i}.forecast_conv.*, bev_conv.*).  Branches: "standard" (n0 / n3: one task, velocity split
per timestep), "dense" (n3dtf / n3dtfm: one task per timestep, optional chained forecast features and BEV-map branch) and
"classify" (the reference constructor's DEFAULT, center_head.py:253,329-330,589-595: one task per timestep with a three-class
heat-map whose channel maximum is the score map); ``reverse`` (center_head.py:559: decoded exactly like the standard head -- the mode differs in
the training targets only) and ``sparse`` (:322-324,572-587: a forward and a reverse task, each with a velocity pair per timestep; the forward
task's steps first, then the reverse task's) and ``wide_head`` (:332-334,597-604: ONE task on a 512-channel shared convolution whose branches keep that
width and whose heat-map has a channel per timestep; step s decodes channel s with the shared regression maps); ``dcn_head`` (:176-229,358-372:
each task a DCNSepHead -- two deformable FeatureAdaption modules, a cls_head for ``hm`` and a SepHead for the other maps -- on the one
launch of fd_deform_adapt_nhwc) with every mode whose reference forward runs (not forecast_feature / wide_head, 64 shared channels);
``two_stage`` is False in every shipped config and raises.  In eval mode on the device the head runs on the convolution plan of dense_bf16.py
(the only device path; a head it cannot take raises); predict() runs the HIP decode + rotated NMS (fd_centerpoint_decode) for
all (sample, heat-map) groups in one call.  loss() (training, torch ops) covers the standard and dense heads; with ``fused_loss = True`` it runs
on fd_loss.hip (two launches forward, two backward, no host synchronisation).
"""
import copy
import logging
from collections import defaultdict

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import hip_ops
from .nn_utils import Sequential, deform_conv2d_v1, kaiming_init, weights_version
from .registry import HEADS


def _transpose_and_gather_feat(feat, ind):
    """det3d/core/utils/center_utils.py:66-80: [B, C, H, W] maps at flat cells ind [B, M] -> [B, M, C]."""
    feat = feat.permute(0, 2, 3, 1).contiguous()
    feat = feat.view(feat.size(0), -1, feat.size(3))
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def _focal_loss(out, target, ind, mask, cat):
    """FastFocalLoss (det3d/models/losses/centernet_loss.py): CornerNet focal loss, positives gathered at ``ind``."""
    mask = mask.float()
    gt = torch.pow(1 - target, 4)
    neg_loss = (torch.log(1 - out) * torch.pow(out, 2) * gt).sum()
    pos_pred = _transpose_and_gather_feat(out, ind).gather(2, cat.unsqueeze(2))  # B x M x 1
    num_pos = mask.sum()
    pos_loss = (torch.log(pos_pred) * torch.pow(1 - pos_pred, 2) * mask.unsqueeze(2)).sum()
    if num_pos == 0:
        return -neg_loss
    return -(pos_loss + neg_loss) / num_pos


def _reg_loss(output, mask, ind, target):
    """RegLoss (det3d/models/losses/centernet_loss.py): masked L1 per box dimension, normalised by the object count."""
    pred = _transpose_and_gather_feat(output, ind)
    mask = mask.float().unsqueeze(2)
    loss = torch.nn.functional.l1_loss(pred * mask, target * mask, reduction="none")
    loss = loss / (mask.sum() + 1e-4)
    return loss.transpose(2, 0).sum(dim=2).sum(dim=1)


def _stack(modules, x, fused_bn):
    """``modules(x)``; with CenterHead.fused_bn set, through dense_bn.run_stack (fusable BatchNorm2d + ReLU pairs on fd_dense_bn.hip)"""
    if not fused_bn:
        return modules(x)
    from .dense_bn import run_stack

    return run_stack(modules, x, True)


class SepHead(nn.Module):
    def __init__(self, in_channels, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, two_stage=False,
                 forecast_feature=False, wide_head=False, **kwargs):
        super().__init__(**kwargs)
        assert not two_stage, "two_stage is False in every shipped config"
        self.heads = heads
        self.forecast_feature = forecast_feature
        if self.forecast_feature:
            self.forecast_conv = nn.Sequential(
                nn.Conv2d(in_channels, head_conv, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(head_conv),
                nn.ReLU(inplace=True),
                nn.Conv2d(head_conv, head_conv, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(head_conv),
                nn.ReLU(inplace=True))
        if wide_head:  # center_head.py:127-128: the branches keep the width of the shared convolution
            head_conv = in_channels
        for head in self.heads:
            classes, num_conv = self.heads[head]
            fc = Sequential()
            for _ in range(num_conv - 1):
                fc.add(nn.Conv2d(head_conv, head_conv, kernel_size=final_kernel, stride=1, padding=final_kernel // 2,
                                 bias=True))
                if bn:
                    fc.add(nn.BatchNorm2d(head_conv))
                fc.add(nn.ReLU())
            fc.add(nn.Conv2d(head_conv, classes, kernel_size=final_kernel, stride=1, padding=final_kernel // 2, bias=True))
            if "hm" in head:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_init(m)
            self.__setattr__(head, fc)

    def forward_modules(self, x, fused_bn=False):
        ret = {}
        if self.forecast_feature:
            x = _stack(self.forecast_conv, x, fused_bn)
            ret["feats"] = x
        for head in self.heads:
            ret[head] = _stack(self.__getattr__(head), x, fused_bn)
        return ret

    def forward(self, x, fused_bn=False):
        return self.forward_modules(x, fused_bn)


class DeformConv(nn.Module):
    """det3d/ops/dcn/deform_conv.py:192-240 as the reference builds it here: 3x3, stride 1, padding 1, no bias (``weight`` only)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, deformable_groups=4):
        super().__init__()
        self.padding, self.deformable_groups = padding, deformable_groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        n = in_channels * kernel_size * kernel_size  # deform_conv.py:225-230
        stdv = 1.0 / n ** 0.5
        self.weight.data.uniform_(-stdv, stdv)

    def forward(self, x, offset):
        return deform_conv2d_v1(x, offset, self.weight, self.deformable_groups, self.padding)


class _DeformAdaptFunction(torch.autograd.Function):
    """(x [B,H,W,64], offsets [B,H,W,144], w_cls, w_reg [64,64,3,3]) -> y [B,H,W,128] = [ReLU(DCN_cls(x)) | ReLU(DCN_reg(x))], fp32 on the
    device.  Saves x, the offsets, the weights and y (the ReLU mask); the backward re-samples."""

    @staticmethod
    def forward(ctx, x, offsets, w_cls, w_reg):
        y = hip_ops.deform_adapt_nhwc(x, hip_ops.pack_deform_adapt_device(w_cls, w_reg), offsets=offsets)
        ctx.save_for_backward(x, offsets, w_cls, w_reg, y)
        return y

    @staticmethod
    @once_differentiable  # the kernels are not differentiable themselves: a double backward raises here
    def backward(ctx, dy):
        x, offsets, w_cls, w_reg, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, doff, dw = hip_ops.deform_adapt_backward(x, offsets, w_cls, w_reg, y, dy.contiguous(), need=(need[0], need[1], need[2] or need[3]))
        return dx, doff, dw[0] if need[2] else None, dw[1] if need[3] else None


class FeatureAdaption(nn.Module):
    """center_head.py:40-78: ReLU(DeformConv(x, conv_offset(x))), conv_offset a 1x1 conv to dg * 2 * k * k offset channels (zero-initialised)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, deformable_groups=4):
        super().__init__()
        self.conv_offset = nn.Conv2d(in_channels, deformable_groups * kernel_size * kernel_size * 2, 1, bias=True)
        self.conv_adaption = DeformConv(in_channels, out_channels, kernel_size=kernel_size, padding=(kernel_size - 1) // 2,
                                        deformable_groups=deformable_groups)
        self.relu = nn.ReLU(inplace=True)
        self.conv_offset.weight.data.zero_()

    def forward(self, x):
        return self.relu(self.conv_adaption(x, self.conv_offset(x)))


class DCNSepHead(nn.Module):
    """center_head.py:176-229: ``hm`` from cls_head on the cls adaption, the other maps from a SepHead on the reg adaption."""

    def __init__(self, in_channels, num_cls, heads, head_conv=64, final_kernel=1, bn=False, init_bias=-2.19, **kwargs):
        super().__init__(**kwargs)
        self.feature_adapt_cls = FeatureAdaption(in_channels, in_channels, kernel_size=3, deformable_groups=4)
        self.feature_adapt_reg = FeatureAdaption(in_channels, in_channels, kernel_size=3, deformable_groups=4)
        self.cls_head = Sequential(nn.Conv2d(in_channels, head_conv, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(64),
                                   nn.ReLU(inplace=True),
                                   nn.Conv2d(head_conv, num_cls, kernel_size=3, stride=1, padding=1, bias=True))
        self.cls_head[-1].bias.data.fill_(init_bias)
        self.task_head = SepHead(in_channels, heads, head_conv=head_conv, bn=bn, final_kernel=final_kernel)

    def forward_modules(self, x, fused_bn=False):
        if self.training and x.is_cuda:
            a_cls, a_reg = self._adapt_pair_train(x)
        else:
            a_cls, a_reg = self.feature_adapt_cls(x), self.feature_adapt_reg(x)
        ret = self.task_head(a_reg, fused_bn) if fused_bn else self.task_head(a_reg)
        ret["hm"] = _stack(self.cls_head, a_cls, fused_bn)
        return ret

    def _adapt_pair_train(self, x):
        """Both FeatureAdaption modules in training on the device: the offsets from the modules' own 1x1 conv_offset (torch, like every
        other head convolution in training), the deformable pair as one fd_deform_adapt_nhwc launch whose backward is
        fd_deform_adapt_backward.  Nothing of im2col size is computed or saved.  fp32 only: CenterHead.forward_modules refuses a bf16
        compute_dtype, and hip_ops rejects any other tensor dtype."""
        fc, fr = self.feature_adapt_cls, self.feature_adapt_reg
        offsets = torch.cat([fc.conv_offset(x), fr.conv_offset(x)], 1).permute(0, 2, 3, 1).contiguous()
        y = _DeformAdaptFunction.apply(x.permute(0, 2, 3, 1).contiguous(), offsets, fc.conv_adaption.weight, fr.conv_adaption.weight)
        y = y.permute(0, 3, 1, 2)
        c = x.shape[1]
        return y[:, :c], y[:, c:]

    def forward(self, x, fused_bn=False):
        return self.forward_modules(x, fused_bn)


class _FusedLossFunction(torch.autograd.Function):
    """CenterHead.loss on fd_loss.hip: (holder, cfg, per-task targets, per-task map names, *maps) -> one 0-dim loss per task, each a view
    of the terms vector that the call leaves in ``holder``.  The maps are flat: per task its ``hm`` followed by the maps of ``names``."""

    @staticmethod
    def forward(ctx, holder, cfg, targets, names, *maps):
        maps = [m.contiguous() for m in maps]
        ctx.cfg, ctx.targets, ctx.names = cfg, targets, names
        tasks = _FusedLossFunction._tasks(targets, names, maps)
        terms, sigs = hip_ops.centerhead_loss_forward(cfg, tasks)
        holder["terms"], holder["sig"] = terms, sigs
        ctx.terms = terms
        ctx.save_for_backward(*maps)
        stride = hip_ops.loss_terms_layout(cfg)[0]
        return tuple(terms[k * stride] for k in range(len(targets)))

    @staticmethod
    def _tasks(targets, names, maps):
        tasks, at = [], 0
        for tg, nm in zip(targets, names):
            tasks.append(dict(tg, hm=maps[at], maps=dict(zip(nm, maps[at + 1:at + 1 + len(nm)]))))
            at += 1 + len(nm)
        return tasks

    @staticmethod
    @once_differentiable  # the kernels are not differentiable themselves: a double backward raises here
    def backward(ctx, *gos):
        maps = ctx.saved_tensors
        tasks = _FusedLossFunction._tasks(ctx.targets, ctx.names, maps)
        flags = ctx.needs_input_grad[4:]
        need, at = [], 0
        for nm in ctx.names:
            need.append({n for n, f in zip(["hm"] + list(nm), flags[at:at + 1 + len(nm)]) if f})
            at += 1 + len(nm)
        go = torch.stack([g.to(torch.float32) for g in gos])  # on the device: the upstream gradients are never read on the host
        grads = hip_ops.centerhead_loss_backward(ctx.cfg, tasks, ctx.terms, go, need=need)
        out = []
        for g, nm in zip(grads, ctx.names):
            out += [g.get(n) for n in ["hm"] + list(nm)]
        return (None, None, None, None) + tuple(out)


def _drop_caches(module, incompatible_keys=None):
    module._plan = None
    module.__dict__.pop("_wv_tensors", None)


@HEADS.register_module
class CenterHead(nn.Module):
    def __init__(self, in_channels=[128, ], tasks=[], dataset="nuscenes", weight=0.25, code_weights=[], common_heads=dict(),
                 logger=None, init_bias=-2.19, share_conv_channel=64, num_hm_conv=2, dcn_head=False, timesteps=1,
                 two_stage=False, reverse=False, sparse=False, dense=False, bev_map=False, forecast_feature=False,
                 classify=True, wide_head=False):
        super().__init__()
        if two_stage:
            raise NotImplementedError("CenterHead option two_stage is False in every shipped centerpoint config and is not "
                                      "part of the inference hot path")
        if dcn_head:  # the combinations whose reference forward fails (64-channel FeatureAdaption / SepHead in DCNSepHead)
            bad = [k for k, v in (("forecast_feature", forecast_feature), ("wide_head", wide_head)) if v]
            if share_conv_channel != 64:
                bad.append("share_conv_channel=%d" % share_conv_channel)
            if bad:
                raise ValueError("CenterHead(dcn_head=True): %s not supported -- the reference's DCNSepHead (center_head.py:176-229) "
                                 "takes 64 shared channels only" % ", ".join(bad))
        self.dcn_head = bool(dcn_head)
        self.two_stage, self.reverse, self.sparse, self.dense = two_stage, reverse, sparse, dense
        self.bev_map, self.forecast_feature, self.classify, self.wide_head = bev_map, forecast_feature, classify, wide_head
        self.target_timesteps = 7
        self.standard = not (reverse or sparse or dense or classify or wide_head)  # center_head.py:268-271
        num_classes = [len(t["class_names"]) for t in tasks]
        self.class_names = [t["class_names"] for t in tasks]
        self.code_weights = code_weights
        self.box_n_dim = 9 if ("vel" in common_heads and "rot" in common_heads) else 7
        # the loss weights of the forecast steps (center_head.py:278-288): only the velocity terms
        fc_mask = None
        if all(h in common_heads for h in ("vel", "rvel", "rot", "rrot")):
            fc_mask = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]
        elif "vel" in common_heads and "rot" in common_heads:
            fc_mask = [0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
        if fc_mask is not None and len(code_weights) == len(fc_mask):
            self.code_weights_forecast = [float(c) * m for c, m in zip(code_weights, fc_mask)]
        self.weight = weight
        self.dataset = dataset
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.use_direction_classifier = False
        self.timesteps = timesteps
        self.logger = logger or logging.getLogger("CenterHead")
        self.logger.info(f"num_classes: {num_classes}")
        self.tasks = nn.ModuleList()
        if self.sparse:    # center_head.py:322-324: a forward and a reverse task
            self.num_classes = 2 * [1]
        if self.dense:
            self.num_classes = self.timesteps * [1]
        if self.classify:  # center_head.py:329-330 (after the dense rule, as there)
            self.num_classes = self.timesteps * [3]
        if self.wide_head:  # center_head.py:332-334
            self.num_classes = [7]
            share_conv_channel = 512
        if self.bev_map:
            c = share_conv_channel
            self.bev_conv = nn.Sequential(
                nn.Conv2d(6, 16, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(16), nn.ReLU(inplace=True),
                nn.Conv2d(16, 32, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
                nn.Conv2d(32, c, kernel_size=3, padding=1, bias=True), nn.BatchNorm2d(c), nn.ReLU(inplace=True))
        self.shared_conv = nn.Sequential(nn.Conv2d(in_channels, share_conv_channel, kernel_size=3, padding=1, bias=True),
                                         nn.BatchNorm2d(share_conv_channel), nn.ReLU(inplace=True))
        for i, num_cls in enumerate(self.num_classes):
            heads = copy.deepcopy(dict(common_heads))
            for head in heads.keys():
                if not (self.dense or self.classify or self.wide_head) and head in ["vel", "rvel"]:  # center_head.py:355 (standard, reverse, sparse)
                    heads[head] = (self.timesteps * heads[head][0], heads[head][1])
            if self.dcn_head:  # center_head.py:370-372: hm comes from the DCNSepHead's cls_head
                self.tasks.append(DCNSepHead(share_conv_channel, num_cls, heads, bn=True, init_bias=init_bias, final_kernel=3))
                continue
            heads.update(dict(hm=(num_cls, num_hm_conv)))
            cin = 2 * share_conv_channel if (i != 0 and self.forecast_feature) else share_conv_channel
            self.tasks.append(SepHead(cin, heads, bn=True, init_bias=init_bias, final_kernel=3, two_stage=self.two_stage,
                                      forecast_feature=self.forecast_feature, wide_head=self.wide_head))
        self.compute_dtype = torch.float32
        self.fused_loss = False  # True: loss() of a standard / dense head runs on fd_loss.hip for fp32 maps on the device
        self.fused_bn = False  # True: in .train() every fusable BatchNorm2d + ReLU of the head runs on fd_dense_bn.hip, with train_dtype = bfloat16 on fd_dense_bn_nhwc.hip (handed to the tasks)
        self.train_dtype = torch.float32  # training: torch.bfloat16 = mixed precision on the bf16 NHWC convolutions (forward_mixed)
        self._plan = None
        self.register_load_state_dict_post_hook(_drop_caches)
        self.logger.info("Finish CenterHead Initialization")

    invalidate_caches = _drop_caches

    def _apply(self, fn, *a, **kw):
        _drop_caches(self)
        return super()._apply(fn, *a, **kw)

    # ----------------------------------------------------------------------------------------------- forward
    def forward_modules(self, x, bev_map=None):
        ret_dicts = []
        if self.dcn_head and self.training and x.is_cuda and self.compute_dtype != torch.float32:
            raise NotImplementedError("CenterHead(dcn_head=True): training runs in fp32 only; the %s head is inference-only (set "
                                      "compute_dtype = torch.float32 to train)" % self.compute_dtype)
        fused = bool(self.fused_bn)
        x = _stack(self.shared_conv, x, fused)
        if self.bev_map:
            x = x + _stack(self.bev_conv, bev_map, fused)
        for i, task in enumerate(self.tasks):
            xin = torch.cat([x, ret_dicts[i - 1]["feats"]], dim=1) if i != 0 and self.forecast_feature else x
            ret_dicts.append(task(xin, True) if fused else task(xin))
        return ret_dicts

    def forward_mixed(self, x, bev_map=None):
        """Training-mode forward in mixed precision (train_dtype = torch.bfloat16, device maps, gradients enabled): the fp32 NCHW input
        is converted once to bf16 channels-last; shared_conv, forecast_conv and the leading convolution of every branch run on
        dense_train.conv2d_bf16 with their bias (the leading convolutions of one SepHead as ONE convolution on the concatenated weights),
        BatchNorm2d stays each module's own with fp32 statistics (bn(x.float()), ReLU, one rounding), and the final convolutions of a
        SepHead are one dense_train.head_tail_bf16 call (fd_head_tail_bf16.hip) whose maps are fp32 NCHW.  ``feats`` and the
        forecast-feature concat stay bf16 in here; every returned map is fp32 and NCHW-contiguous, what loss() and the fused loss read.
        Layers the kernels do not take (bev_conv's 6- and 16-channel convolutions, more than 16 final channels) run their module on an
        fp32 copy.

        With ``fused_bn`` every BatchNorm2d (+ ReLU) that dense_bn.batch_norm2d_nhwc_fusable accepts runs on fd_dense_bn_nhwc.hip instead
        (dense_bn.batch_norm2d_act_nhwc: bf16 channels-last in and out, fp32 statistics, no fp32 copy of the map), and the BatchNorm2d
        modules of a SepHead's branches are ONE grouped call on the map of their batched convolution, of which the final convolutions
        read their channel slices.  A frozen module and bev_conv's narrow layers keep the recipe above."""
        from .dense_train import run_head_stack_bf16, sep_head_bf16

        fused = bool(self.fused_bn)
        x = run_head_stack_bf16(list(self.shared_conv.children()), x.to(torch.bfloat16, memory_format=torch.channels_last), fused)
        if self.bev_map:
            x = x + run_head_stack_bf16(list(self.bev_conv.children()), bev_map.to(torch.bfloat16, memory_format=torch.channels_last), fused)
        ret_dicts = []
        for i, task in enumerate(self.tasks):
            xin = torch.cat([x, ret_dicts[i - 1]["feats"]], dim=1) if i != 0 and self.forecast_feature else x
            ret_dicts.append(sep_head_bf16(task, xin, fused))
        if self.forecast_feature:
            ret_dicts = [dict((k, v.to(torch.float32, memory_format=torch.contiguous_format) if k == "feats" else v) for k, v in d.items())
                         for d in ret_dicts]
        return ret_dicts

    def forward(self, x, bev_map=None, *kwargs):
        if self.training:
            if self.train_dtype not in (torch.float32, torch.bfloat16):
                raise ValueError("CenterHead: train_dtype must be torch.float32 or torch.bfloat16 (got %s)" % (self.train_dtype,))
            if self.train_dtype == torch.bfloat16 and self.dcn_head:
                raise NotImplementedError("CenterHead(dcn_head=True): train_dtype = torch.bfloat16 is not supported, the deformable head "
                                          "trains in fp32 only")
            if self.train_dtype == torch.bfloat16 and x.is_cuda and torch.is_grad_enabled():
                return self.forward_mixed(x, bev_map)
        if self.training or not x.is_cuda:
            return self.forward_modules(x, bev_map)
        if self.compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("CenterHead: compute_dtype must be float32 or bfloat16, got %s" % (self.compute_dtype,))
        ver = (weights_version(self), self.compute_dtype)
        if self._plan is None or self._plan[0] != ver:
            from .dense_bf16 import HeadPlan

            self._plan = (ver, HeadPlan(self, self.compute_dtype))  # raises ValueError for a head the kernels do not take
        return self._plan[1](x.to(self.compute_dtype).permute(0, 2, 3, 1).contiguous(), bev_map)

    # ----------------------------------------------------------------------------------------------- loss
    def _sigmoid(self, x):
        return torch.clamp(x.sigmoid(), min=1e-4, max=1 - 1e-4)  # center_head.py:392-394 (out of place: the maps may be leaves)

    def loss(self, example, preds_dicts, **kwargs):
        """center_head.py:396-539 for the standard (n0 / n3 / pedestrian) and dense (n3dtf / n3dtfm) heads.  ``example`` carries the
        reference pipeline's targets (hm / ind / mask / cat / anno_box, indexed [timestep][task]).  Returns the reference's dict of
        per-task lists (loss, hm_loss, loc_loss, loc_loss_elem, num_positive); like the reference it replaces preds_dict["hm"] by the
        clamped sigmoid and adds preds_dict["anno_box"].

        ``self.fused_loss = True`` (default False) sends fp32 maps on the device through fd_loss.hip instead (_loss_fused): the same
        dict, with the intended differences listed there.  ``check=True`` then reads the kernels' status word back."""
        for flag in ("reverse", "sparse", "classify", "wide_head"):
            if getattr(self, flag):
                raise NotImplementedError("CenterHead.loss: the %s head's loss is not implemented (standard and dense heads only)" % flag)
        if self.dataset not in ("waymo", "nuscenes"):
            raise NotImplementedError("CenterHead.loss: dataset %r (the reference handles waymo / nuscenes only)" % (self.dataset,))
        if self.fused_loss and preds_dicts and all(p["hm"].is_cuda and p["hm"].dtype == torch.float32 for p in preds_dicts):
            return self._loss_fused(example, preds_dicts, check=kwargs.get("check", False))
        T = self.timesteps
        rets = []
        for task_id, preds_dict in enumerate(preds_dicts):
            preds_dict["hm"] = self._sigmoid(preds_dict["hm"])
            if self.dense:
                hm_loss = _focal_loss(preds_dict["hm"], example["hm"][task_id][0], example["ind"][task_id][0], example["mask"][task_id][0],
                                      example["cat"][task_id][0])
                target_box = example["anno_box"][task_id][0]
            else:
                hm_loss = _focal_loss(preds_dict["hm"], example["hm"][0][task_id], example["ind"][0][task_id], example["mask"][0][task_id],
                                      example["cat"][0][task_id])
                target_box = [example["anno_box"][i][task_id] for i in range(T)]
            p = preds_dict
            if "vel" in p and "rvel" in p and "rot" in p and "rrot" in p:
                if self.dense:
                    p["anno_box"] = torch.cat((p["reg"], p["height"], p["dim"], p["vel"], p["rvel"], p["rot"], p["rrot"]), dim=1)
                else:
                    p["anno_box"] = [torch.cat((p["reg"], p["height"], p["dim"], p["vel"][:, 2 * i:2 * i + 2], p["rvel"][:, 2 * i:2 * i + 2],
                                                p["rot"], p["rrot"]), dim=1) for i in range(T)]
            elif "vel" in p and "rot" in p:
                if self.dense:
                    p["anno_box"] = torch.cat((p["reg"], p["height"], p["dim"], p["vel"], p["rot"]), dim=1)
                    target_box = target_box[..., [0, 1, 2, 3, 4, 5, 6, 7, -2, -1]]
                else:
                    p["anno_box"] = [torch.cat((p["reg"], p["height"], p["dim"], p["vel"][:, 2 * i:2 * i + 2], p["rot"]), dim=1) for i in range(T)]
                    target_box = [target_box[i][..., [0, 1, 2, 3, 4, 5, 6, 7, -2, -1]] for i in range(T)]
            else:
                p["anno_box"] = [torch.cat((p["reg"], p["height"], p["dim"], p["rot"]), dim=1) for i in range(T)]
                target_box = [target_box[i][..., [0, 1, 2, 3, 4, 5, -2, -1]] for i in range(T)]
            loc_loss = []
            if self.dense:
                box_loss = _reg_loss(p["anno_box"], example["mask"][task_id][0], example["ind"][task_id][0], target_box)
                loc_loss.append((box_loss * box_loss.new_tensor(self.code_weights)).sum())
            else:
                box_loss = [_reg_loss(p["anno_box"][i], example["mask"][0][task_id], example["ind"][0][task_id], target_box[i]) for i in range(T)]
                for i in range(T):
                    cw = self.code_weights if i == 0 else self.code_weights_forecast
                    loc_loss.append((box_loss[i] * box_loss[i].new_tensor(cw)).sum())
            loss = hm_loss + self.weight * sum(loc_loss)
            if self.dense:
                ret = {"loss": loss, "hm_loss": hm_loss.detach().cpu(), "loc_loss": loc_loss, "loc_loss_elem": box_loss.detach().cpu(),
                       "num_positive": sum(sum(example["mask"][task_id][0].float()))}
            else:
                ret = {"loss": loss, "hm_loss": hm_loss.detach().cpu(), "loc_loss": loc_loss,
                       "loc_loss_elem": [box_loss[i].detach().cpu() for i in range(T)],
                       "num_positive": sum(sum(sum([example["mask"][i][task_id].float() for i in range(T)])))}
            rets.append(ret)
        merged = defaultdict(list)  # batch-key -> key-batch, as the reference returns it
        for ret in rets:
            for k, v in ret.items():
                merged[k].append(v)
        return merged

    def _loss_fused(self, example, preds_dicts, check=False):
        """loss() on fd_loss.hip (fd_centerhead_loss_forward / _backward): two launches forward and two backward for all tasks and
        timesteps (three each for more than 8 tasks), no atomics, no host synchronisation, so a training step can be captured in a
        graph.  Returns the reference's dict -- the same five keys and list lengths -- with every entry a view of ONE fp32 terms
        vector on the device; only ``loss[k]`` carries a gradient.  Intended differences from the torch path:
          * nothing is copied to the host: hm_loss, loc_loss_elem and num_positive stay device tensors (the torch path, like the
            reference, moves them with .cpu(), a synchronisation per task);
          * preds_dict["hm"] becomes the kernel's clamped sigmoid, a plain tensor without a gradient history;
          * preds_dict["anno_box"] is not built.
        An entry with mask != 0 whose ind / cat is out of range is skipped and counted (torch's gather would device-assert);
        ``check=True`` reads that count back (a synchronisation) and raises AssertionError when it is not 0."""
        T, dense = self.timesteps, bool(self.dense)
        p0 = preds_dicts[0]
        if "vel" in p0 and "rvel" in p0 and "rot" in p0 and "rrot" in p0:
            names = ("reg", "height", "dim", "vel", "rvel", "rot", "rrot")
        elif "vel" in p0 and "rot" in p0:
            names = ("reg", "height", "dim", "vel", "rot")
        else:
            names = ("reg", "height", "dim", "rot")
        D = {7: 14, 5: 10, 4: 8}[len(names)]
        targets = []
        for k in range(len(preds_dicts)):
            if dense:
                targets.append(dict(hm_target=example["hm"][k][0], ind=example["ind"][k][0], cat=example["cat"][k][0],
                                    mask=[example["mask"][k][0]], anno_box=[example["anno_box"][k][0]]))
            else:
                targets.append(dict(hm_target=example["hm"][0][k], ind=example["ind"][0][k], cat=example["cat"][0][k],
                                    mask=[example["mask"][i][k] for i in range(T)], anno_box=[example["anno_box"][i][k] for i in range(T)]))
        B, _, H, W = p0["hm"].shape
        M, row = targets[0]["anno_box"][0].shape[1:]
        key = (B, H, W, M, len(preds_dicts), row, D, T, dense, tuple(self.code_weights), self.weight)
        cached = self.__dict__.get("_loss_cfg")
        if cached is None or cached[0] != key:  # the descriptor of the head mode and batch shape, built once
            cwf = getattr(self, "code_weights_forecast", None) if (not dense and T > 1) else None
            if not dense and T > 1 and cwf is None:
                raise ValueError("CenterHead.loss: a standard head with %d timesteps needs code_weights_forecast (vel and rot heads)" % T)
            cached = (key, hip_ops.make_loss_cfg(B, H, W, M, len(preds_dicts), dense, T, D, row, self.code_weights, cwf, self.weight))
            self.__dict__["_loss_cfg"] = cached
        cfg = cached[1]
        holder = {}
        maps = [p[n] for p in preds_dicts for n in ("hm",) + names]
        losses = _FusedLossFunction.apply(holder, cfg, targets, [names] * len(preds_dicts), *maps)
        terms = holder["terms"]
        for p, sig in zip(preds_dicts, holder["sig"]):
            p["hm"] = sig
        if check:
            bad = hip_ops.loss_status(terms)
            if bad:
                raise AssertionError("CenterHead.loss: %d masked target entries name a cell or class outside the heat map" % bad)
        stride, S = hip_ops.loss_terms_layout(cfg)
        merged = defaultdict(list)
        for k in range(len(preds_dicts)):
            t = terms[k * stride:(k + 1) * stride]
            merged["loss"].append(losses[k])
            merged["hm_loss"].append(t[1])
            merged["loc_loss"].append([t[4 + i] for i in range(S)])
            elem = t[4 + S:].view(S, D)
            merged["loc_loss_elem"].append(elem[0] if dense else [elem[i] for i in range(S)])
            merged["num_positive"].append(t[3])
        return merged

    # ----------------------------------------------------------------------------------------------- predict
    def _groups(self, preds_dicts):
        """-> (list of per-group source dicts, vel tensor per output step, step->group map, num_classes per step)."""
        if self.standard or self.reverse:  # center_head.py:559-570
            pd = preds_dicts[0]
            vels = [pd["vel"][:, 2 * i:2 * i + 2] for i in range(self.timesteps)]
            if len(vels) == 1:
                vels = self.target_timesteps * vels
            return [pd], vels, [0] * len(vels), [1] * len(vels)  # (the reference writes [1] * target_timesteps and can only run 1 or 7 steps)
        if self.sparse:  # center_head.py:572-587: the forward task's steps, then the reverse task's
            fwd, rev = preds_dicts[0], preds_dicts[1]
            vels = [fwd["vel"][:, 2 * i:2 * i + 2] for i in range(self.timesteps)] + [rev["vel"][:, 2 * i:2 * i + 2] for i in range(self.timesteps)]
            return [fwd, rev], vels, [0] * self.timesteps + [1] * self.timesteps, [1] * (2 * self.timesteps)
        if self.wide_head:  # center_head.py:597-604: step s = heat-map channel s of the one task, every other map shared
            pd = preds_dicts[0]
            srcs = [dict(pd, hm=pd["hm"][:, i:i + 1]) for i in range(self.timesteps)]
            return srcs, [pd["vel"]] * self.timesteps, list(range(self.timesteps)), [1] * self.timesteps
        vels = [pd["vel"] for pd in preds_dicts]  # center_head.py:606-607 (dense), :589-595 (classify: one class per step after the channel max)
        return list(preds_dicts), vels, list(range(len(preds_dicts))), [1] * len(preds_dicts) if self.classify else list(self.num_classes)

    @staticmethod
    def _circular(test_cfg):
        """test_cfg.circular_nms (center_head.py:722-725).  ``per_class_nms`` has nothing to reproduce: the reference's branch is ``pass``
        (:668-669), no task's result is collected and predict fails on ``rets[0]`` two lines later."""
        if test_cfg.get("per_class_nms", False):
            raise NotImplementedError("test_cfg.per_class_nms: the reference's branch is empty (center_head.py:668-669) and its predict fails on rets[0]")
        return bool(test_cfg.get("circular_nms", False))

    @staticmethod
    def _group_radius(test_cfg, step_group, G):
        """``test_cfg.min_radius[task_id]`` (center_head.py:724; task_id = output step, :609) per decode group; None when two steps of one
        group differ.  A scalar ``min_radius`` (as every shipped config writes it) fails here as it does in the reference."""
        radii = test_cfg["min_radius"]
        per_step = [float(radii[s]) for s in range(len(step_group))]  # TypeError for a scalar, IndexError for a short list: the reference's own
        out = [None] * G
        for s, g in enumerate(step_group):
            if out[g] is None:
                out[g] = per_step[s]
            elif out[g] != per_step[s]:
                return None
        return [0.0 if r is None else r for r in out]

    @torch.no_grad()
    def predict_packed(self, preds_dicts, test_cfg):
        """Device-only decode straight from the convolution plan's NHWC output buffer: (packed [B,S,post,11] float32 rows
        x y z w l h vx vy yaw score label, counts [B,S] int32) -- five launches (keys + histogram, selection, rank + box decode, IoU mask,
        sweep + gather + assembly: fd_centerpoint_decode_packed), no torch kernel in between.  None when the maps did not come from the plan (torch path, bev_map head)."""
        if self.wide_head:  # (its T groups differ in the heat-map channel only: decoded through the per-group path below)
            return None
        raws = [getattr(pd, "raw", None) for pd in preds_dicts]
        if any(r is None for r in raws) or any(r[0] is not raws[0][0] or r[2] != raws[0][2] for r in raws):
            return None
        circular = self._circular(test_cfg)
        zbuf, _, where = raws[0]
        T, B, H, W, C = zbuf.shape
        hm_channels = where["hm"][1]
        assert hm_channels == 1 or self.classify, "multi-class heat-maps are decoded as their channel maximum only in the classify mode (center_head.py:589-595)"
        if self.sparse:  # center_head.py:572-587: two tasks (forward, reverse), a velocity pair per timestep each; 2 T output steps
            G = 2
            S = 2 * self.timesteps
            assert 2 * self.timesteps <= where["vel"][1], "velocity channels 2 s, 2 s + 1 must exist for every step"
            step_group = [0] * self.timesteps + [1] * self.timesteps
            step_vel = [2 * s for s in range(self.timesteps)] * 2
            num_classes = [1] * S
        elif self.standard or self.reverse:  # center_head.py:559-570: one task, step s = its boxes + velocity channels 2s, 2s+1 (all steps share them when timesteps == 1)
            G = 1
            # center_head.py:559-565 emits one step per velocity pair: ``timesteps`` of them when the head forecasts, else
            # ``target_timesteps`` copies of the single pair (the same rule as _groups above)
            S = self.timesteps if self.timesteps > 1 else self.target_timesteps
            assert self.timesteps <= 1 or 2 * S <= where["vel"][1], "velocity channels 2 s, 2 s + 1 must exist for every step"
            step_group = [0] * S
            step_vel = [2 * s if self.timesteps > 1 else 0 for s in range(S)]
            num_classes = [1] * S
        else:              # :606-607: one task per step
            G = T
            S = T
            step_group = list(range(T))
            step_vel = [0] * T
            num_classes = [1] * T if self.classify else list(self.num_classes)
        labels, acc = [], 0
        for ncls in num_classes:
            labels.append(acc)
            acc += ncls
        cache = self.__dict__.setdefault("_lab_cache", {})
        ck = (zbuf.device, B, S, int(test_cfg["nms"]["nms_post_max_size"]))
        if ck not in cache:  # labels do not depend on the data (built in the eager set-up pass, before any graph capture)
            cache[ck] = torch.as_tensor(labels, dtype=torch.int64, device=zbuf.device).view(1, S, 1).expand(B, S, ck[3]).contiguous()
        group_radius = None
        if circular:
            group_radius = self._group_radius(test_cfg, step_group, G)
            if group_radius is None:  # steps that share a decode group ask for different radii: one group per step (predict_padded)
                return None
        flat = zbuf[:G].reshape(G * B, H, W, C)
        cfg = hip_ops.make_decode_cfg(H, W, test_cfg, hm_channels=hm_channels, group_radius=group_radius)
        views = [hip_ops.nhwc_channel_view(flat, where[k][0]) for k in ("hm", "reg", "height", "dim", "rot")]
        return hip_ops.centerpoint_decode_packed(views, hip_ops.nhwc_channel_view(flat, where["vel"][0]), G * B, B, cfg, zbuf.device, step_group, step_vel, labels)

    @torch.no_grad()
    def predict_padded(self, preds_dicts, test_cfg):
        """Device-only decode: (boxes [B,S,post,9], scores [B,S,post], labels [B,S,post] int64, counts [B,S] int32)
        with S output steps; entries k >= counts[b,s] are padding.  No host synchronisation."""
        fused = self.predict_packed(preds_dicts, test_cfg)
        if fused is not None:
            packed, counts = fused
            B, S, post, _ = packed.shape
            return packed[..., :9], packed[..., 9], self._lab_cache[(packed.device, B, S, post)], counts
        srcs, vels, step_group, num_classes = self._groups(preds_dicts)
        group_radius = None
        if self._circular(test_cfg):
            group_radius = self._group_radius(test_cfg, step_group, len(srcs))
            if group_radius is None:  # a decode group per output step, each with its step's radius
                srcs, step_group = [srcs[g] for g in step_group], list(range(len(step_group)))
                group_radius = self._group_radius(test_cfg, step_group, len(srcs))
        B, hm_channels, H, W = srcs[0]["hm"].shape
        assert all(s["hm"].shape[1] == hm_channels for s in srcs) and (hm_channels == 1 or self.classify), \
            "multi-class heat-maps are decoded as their channel maximum only in the classify mode (center_head.py:589-595)"
        f = lambda k: torch.cat([s[k].float() for s in srcs], 0).contiguous() if len(srcs) > 1 else srcs[0][k].float().contiguous()  # noqa: E731
        cfg = hip_ops.make_decode_cfg(H, W, test_cfg, hm_channels=hm_channels, group_radius=group_radius)
        boxes7, scores, cell, count = hip_ops.centerpoint_decode(f("hm"), f("reg"), f("height"), f("dim"), f("rot"), cfg)
        post = cfg.nms_post_max
        G = len(srcs)
        # group-major [G*B, ...] -> [B, G, ...]
        boxes7 = boxes7.view(G, B, post, 7).transpose(0, 1)
        scores = scores.view(G, B, post).transpose(0, 1)
        cell = cell.view(G, B, post).transpose(0, 1)
        count = count.view(G, B).transpose(0, 1)
        # assemble all S output steps at once (one gather for every step's velocity instead of a Python loop)
        S = len(vels)
        dev = boxes7.device
        ck = (dev, tuple(step_group), tuple(num_classes), B, post)
        cache = self.__dict__.setdefault("_dec_cache", {})
        if ck not in cache:  # small index / label tensors, built once (no per-step host->device copies)
            offs = [0]
            for ncls in num_classes[:-1]:
                offs.append(offs[-1] + ncls)
            cache[ck] = (torch.as_tensor(step_group, device=dev),
                         torch.as_tensor(offs, dtype=torch.int64, device=dev).view(1, S, 1).expand(B, S, post).contiguous())
        gsel, labels = cache[ck]
        b7 = boxes7.index_select(1, gsel)            # [B, S, post, 7]
        idx = cell.index_select(1, gsel).long().clamp_(min=0)  # [B, S, post]
        if all(v is vels[0] for v in vels):          # timesteps == 1: the same two channels for every step
            vstack = vels[0].float().reshape(B, 1, 2, H * W).expand(B, S, 2, H * W)
        else:
            vstack = torch.stack([v.float().reshape(B, 2, H * W) for v in vels], 1)  # [B, S, 2, HW]
        v = torch.gather(vstack, 3, idx.unsqueeze(2).expand(B, S, 2, post)).transpose(2, 3)  # [B, S, post, 2]
        boxes = torch.cat([b7[..., :6], v, b7[..., 6:7]], dim=-1)
        return boxes, scores.index_select(1, gsel), labels, count.index_select(1, gsel)

    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg, **kwargs):
        boxes, scores, labels, counts = self.predict_padded(preds_dicts, test_cfg)
        B, S, post, _ = boxes.shape
        if test_cfg.get("circular_nms", False) and bool((counts < 0).any()):
            raise RuntimeError("circular NMS: a group holds more than %d candidates above the score threshold and keeps fewer than nms_post_max_size of "
                               "them -- the reference's uncut result cannot be reproduced from the candidates taken (raise score_threshold)" % hip_ops.CIRCLE_PRE_MAX)
        valid = torch.arange(post, device=boxes.device).view(1, 1, post) < counts.unsqueeze(-1)
        metas = example.get("metadata") if isinstance(example, dict) else None
        ret = []
        for b in range(B):
            m = valid[b].reshape(-1)
            ret.append({"box3d_lidar": boxes[b].reshape(-1, 9)[m], "scores": scores[b].reshape(-1)[m],
                        "label_preds": labels[b].reshape(-1)[m],
                        "metadata": metas[b] if metas is not None and len(metas) > b else None})
        return ret
