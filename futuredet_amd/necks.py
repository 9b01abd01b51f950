"""RPN neck (det3d/models/necks/rpn.py:22-159).  Same constructor, same state_dict keys
(blocks.{i}.{1,4,...}.weight, deblocks.{i}.0.weight, ...).  In eval mode the stack runs with BatchNorm folded
into the convolutions (ZeroPad2d merged into the conv padding) on the hand-written MFMA convolutions (dense_bf16.py:
NHWC, bf16 or fp32, concat and transposed convolution written in place).  That plan is the ONLY eval-mode device path: a stack
it cannot take (a channel count that is not a multiple of the kernels' granule) raises instead of running anywhere else.
Training mode and host tensors (the CPU tests of the state-dict surface) run the plain nn.Module stack, forward_modules; with
train_dtype = torch.bfloat16 a training-mode device map runs in mixed precision instead (forward_mixed, dense_train.py)."""
import logging

import numpy as np
import torch
from torch import nn

from .nn_utils import Sequential, build_norm_layer, weights_version
from .registry import NECKS



def _drop_caches(module, incompatible_keys=None):
    module._plan = None
    module.__dict__.pop("_wv_tensors", None)


@NECKS.register_module
class RPN(nn.Module):
    def __init__(self, layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides, us_num_filters,
                 num_input_features, norm_cfg=None, name="rpn", logger=None, **kwargs):
        super().__init__()
        # constructor keywords of det3d/models/necks/rpn.py:24-36; the module layout below (blocks.<i>.<j>, deblocks.<i>.<j>) is what
        # fixes the state-dict keys of the reference's checkpoints
        self.stage_strides, self.stage_filters, self.stage_layers = list(ds_layer_strides), list(ds_num_filters), list(layer_nums)
        self.up_strides, self.up_filters = list(us_layer_strides), list(us_num_filters)
        self.norm_cfg = norm_cfg if norm_cfg is not None else dict(type="BN", eps=1e-3, momentum=0.01)
        n_stage, n_up = len(self.stage_layers), len(self.up_strides)
        if not (len(self.stage_strides) == len(self.stage_filters) == n_stage and len(self.up_filters) == n_up <= n_stage):
            raise ValueError("RPN: ds_layer_strides / ds_num_filters / layer_nums need one entry per stage, us_* one per up-sampled stage")
        self.first_up = n_stage - n_up  # stages in front of the first one that has a deblock
        # every deblock must bring its stage to ONE common resolution (their outputs are concatenated)
        scales = {float(self.up_strides[j]) / float(np.prod(self.stage_strides[: self.first_up + j + 1])) for j in range(n_up)}
        if len(scales) > 1:
            raise ValueError("RPN: the deblocks end at different resolutions %s" % sorted(scales))
        blocks, deblocks = [], []
        cin = num_input_features
        for i in range(n_stage):
            blocks.append(self._make_layer(cin, self.stage_filters[i], self.stage_layers[i], stride=self.stage_strides[i]))
            cin = self.stage_filters[i]
            j = i - self.first_up
            if j >= 0:
                up, cout = self.up_strides[j], self.up_filters[j]
                if up > 1:  # transposed convolution up, or (stride < 1, the PointPillars neck) a strided convolution down
                    conv = nn.ConvTranspose2d(cin, cout, up, stride=up, bias=False)
                else:
                    down = int(round(1.0 / up))
                    conv = nn.Conv2d(cin, cout, down, stride=down, bias=False)
                deblocks.append(Sequential(conv, build_norm_layer(self.norm_cfg, cout)[1], nn.ReLU()))
        self.blocks = nn.ModuleList(blocks)
        self.deblocks = nn.ModuleList(deblocks)
        self.compute_dtype = torch.float32
        self.fused_bn = False  # True: in .train() every fusable BatchNorm2d + ReLU of the blocks and deblocks runs on fd_dense_bn.hip
                               # (with train_dtype = torch.bfloat16: on fd_dense_bn_nhwc.hip, bf16 channels-last)
        self.train_dtype = torch.float32  # training: torch.bfloat16 = mixed precision on the bf16 NHWC convolutions (forward_mixed)
        self._plan = None
        self.register_load_state_dict_post_hook(_drop_caches)
        (logger or logging.getLogger("RPN")).info("Finish RPN Initialization")

    @property
    def downsample_factor(self):
        factor = np.prod(self.stage_strides)
        if self.up_strides:
            factor /= self.up_strides[-1]
        return factor

    def _make_layer(self, inplanes, planes, num_blocks, stride=1):
        block = Sequential(nn.ZeroPad2d(1), nn.Conv2d(inplanes, planes, 3, stride=stride, bias=False),
                           build_norm_layer(self.norm_cfg, planes)[1], nn.ReLU())
        for _ in range(num_blocks):
            block.add(nn.Conv2d(planes, planes, 3, padding=1, bias=False))
            block.add(build_norm_layer(self.norm_cfg, planes)[1])
            block.add(nn.ReLU())
        return block

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)

    def _stack(self, modules, x):
        if not self.fused_bn:
            return modules(x)
        from .dense_bn import run_stack

        return run_stack(modules, x, True)

    def forward_modules(self, x):
        ups = []
        for i in range(len(self.blocks)):
            x = self._stack(self.blocks[i], x)
            if i >= self.first_up:
                ups.append(self._stack(self.deblocks[i - self.first_up], x))
        if len(ups) > 0:
            x = torch.cat(ups, dim=1)
        return x

    def forward_mixed(self, x):
        """Training-mode forward in mixed precision (train_dtype = torch.bfloat16, device maps): the BEV map is converted once to bf16
        channels-last, every block and deblock runs through dense_train.run_stack_bf16 -- the stride-1 3 x 3 convolutions and the
        1 x 1 deblock on fd_conv2d_nhwc_bf16 / fd_conv2d_wgrad_bf16 with fp32 master weights and fp32 weight gradients, the 3 x 3 /
        stride 2 convolution that opens a down-sampling stage on dense_train.conv2d_s2_bf16 and the ConvTranspose2d(2, stride 2) deblock
        on dense_train.conv_transpose2d_k2_bf16 (fd_conv2d_strided_grad_bf16.hip), BatchNorm with fp32 statistics -- and the concatenated
        map is returned fp32 and NCHW-contiguous, which is what the head sees from forward_modules.  Any other convolution (a bias, other
        kernel sizes or strides; also the Conv2d(2, stride 2) deblock of the PointPillars neck, which was measured no faster on
        dense_train.conv2d_k2s2_bf16) runs its module on an fp32 copy of its input.
        BatchNorm2d runs the backbone's un-fused recipe, bn(x.float()) + ReLU + one rounding; with ``fused_bn`` every module that
        dense_bn.batch_norm2d_nhwc_fusable accepts (training mode, a multiple of 32 channels up to 512) runs with its ReLU on
        fd_dense_bn_nhwc.hip instead (dense_bn.batch_norm2d_act_nhwc: bf16 channels-last in and out, fp32 statistics, no fp32 copy of the
        map); a frozen module keeps the recipe."""
        from .dense_train import run_stack_bf16

        fused = bool(self.fused_bn)
        x = x.to(torch.bfloat16, memory_format=torch.channels_last)
        ups = []
        for i in range(len(self.blocks)):
            x = run_stack_bf16(self.blocks[i], x, fused)
            if i >= self.first_up:
                ups.append(run_stack_bf16(self.deblocks[i - self.first_up], x, fused))
        if len(ups) > 0:
            x = torch.cat(ups, dim=1)
        return x.to(torch.float32, memory_format=torch.contiguous_format)

    invalidate_caches = _drop_caches

    def _apply(self, fn, *a, **kw):  # .to() / .cuda() / .float(): derived weights live on the old device / dtype
        _drop_caches(self)
        return super()._apply(fn, *a, **kw)

    def forward(self, x):
        if self.training:
            if self.train_dtype not in (torch.float32, torch.bfloat16):
                raise ValueError("RPN: train_dtype must be torch.float32 or torch.bfloat16 (got %s)" % (self.train_dtype,))
            if self.train_dtype == torch.bfloat16 and x.is_cuda:
                return self.forward_mixed(x)
        if self.training or not x.is_cuda:
            return self.forward_modules(x)
        if self.compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("RPN: compute_dtype must be float32 or bfloat16, got %s" % (self.compute_dtype,))
        # hand-written MFMA convolutions on NHWC activations (bf16 or fp32); returned as an NCHW-shaped view of the NHWC buffer
        ver = (weights_version(self), self.compute_dtype)
        if self._plan is None or self._plan[0] != ver:
            from .dense_bf16 import RPNPlan

            self._plan = (ver, RPNPlan(self, self.compute_dtype))  # raises ValueError for a stack the kernels do not take
        xin = x.to(self.compute_dtype).permute(0, 2, 3, 1).contiguous()  # no copy for a channels-last BEV map
        return self._plan[1](xin).permute(0, 3, 1, 2)
