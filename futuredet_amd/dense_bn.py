"""Training-mode BatchNorm2d + ReLU of the dense half (RPN, CenterHead) on the fused kernels of fd_dense_bn.hip: the autograd surface
(batch_norm2d_act), the predicate that says where it applies (batch_norm2d_fusable), and the walk over a Conv2d / BatchNorm2d / ReLU
stack that RPN.fused_bn and CenterHead.fused_bn switch on (run_stack).  These take fp32 NCHW-contiguous device maps.

In mixed precision (train_dtype = torch.bfloat16) the maps are bf16 channels-last, and ``fused_bn`` selects the kernels of
fd_dense_bn_nhwc.hip instead: batch_norm2d_act_nhwc is their autograd surface -- one call for one module, or for the modules that
partition the channels of one map (the branches of a SepHead) -- and batch_norm2d_nhwc_fusable the predicate; the walks that use them
are dense_train.run_stack_bf16, run_head_stack_bf16 and sep_head_bf16.  Everything else keeps the module chain."""
import torch
from torch import nn

from . import hip_ops


class _DenseBatchNormFunction(torch.autograd.Function):
    """Training-mode BatchNorm2d over x [B, C, H, W] fused with the ReLU that follows it (fd_dense_bn.hip):
    y = act(gamma (x - mean) invstd + beta).  ``bn`` is the nn.BatchNorm2d module: the kernel updates its running statistics and
    num_batches_tracked on the device.  Saves x and y: y is what the next convolution saves as its input."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, relu):
        y, saved = hip_ops.dense_bn_train_forward(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps,
                                                  bn.momentum, relu=relu)
        # the kernel wrote through raw pointers: the eval plans key their folded-BN weights on these counters (weights_version)
        for buf in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
            torch.autograd.graph.increment_version(buf)
        ctx.save_for_backward(x, y, gamma, saved)
        ctx.relu = relu
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, gamma, saved = ctx.saved_tensors
        dx, dgamma, dbeta = hip_ops.dense_bn_train_backward(dy.contiguous(), x, y, gamma, saved, relu=ctx.relu)
        return dx, dgamma, dbeta, None, None


def batch_norm2d_fusable(x, bn):
    """True where batch_norm2d_act can take the place of ``bn`` (+ ReLU): a training-mode, affine nn.BatchNorm2d that tracks running
    statistics with a fixed momentum, gradients enabled, an fp32 NCHW-contiguous device map [B, C, H, W] with B H W >= 2, fp32
    parameters on the same device."""
    return (isinstance(bn, nn.BatchNorm2d) and bn.training and torch.is_grad_enabled() and bn.affine and bn.track_running_stats
            and bn.momentum is not None and bn.running_mean is not None and x.is_cuda
            and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.shape[1] == bn.num_features
            and x.shape[0] * x.shape[2] * x.shape[3] >= 2 and bn.weight.dtype == torch.float32 and bn.weight.device == x.device
            and bn.running_mean.dtype == torch.float32 and bn.running_mean.device == x.device)


def batch_norm2d_act(x, bn, relu=True):
    """relu(bn(x)) in training mode on the fused kernels; ``bn`` is the existing nn.BatchNorm2d module (parameters, buffers and
    state-dict keys unchanged).  Raises where batch_norm2d_fusable(x, bn) does not hold: there is no fallback here."""
    if not batch_norm2d_fusable(x, bn):
        raise hip_ops.FutureDetHipError("batch_norm2d_act: needs a training-mode affine BatchNorm2d with running statistics and a momentum, "
                                        "gradients enabled and an fp32 NCHW-contiguous device map [B, C, H, W] with B H W >= 2 (got %s %s)"
                                        % (tuple(x.shape), x.dtype))
    return _DenseBatchNormFunction.apply(x, bn.weight, bn.bias, bn, bool(relu))


def run_stack(modules, x, fused):
    """``modules(x)`` for a Sequential (nn_utils or torch.nn) of convolutions, BatchNorm2d and ReLU.  With ``fused`` set, a BatchNorm2d
    that is directly followed by an nn.ReLU and fusable on its input runs as one batch_norm2d_act call and the ReLU is skipped; every
    other module -- a BatchNorm2d that is not fusable included (frozen with .eval(), a channels-last input, a host tensor, double,
    no_grad) -- is called as before."""
    if not fused:
        return modules(x)
    mods = list(modules.children())
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.BatchNorm2d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) and batch_norm2d_fusable(x, m):
            x = batch_norm2d_act(x, m, relu=True)
            i += 2
        else:
            x = m(x)
            i += 1
    return x


class _DenseBatchNormNhwcFunction(torch.autograd.Function):
    """Training-mode BatchNorm2d over a bf16 channels-last map fused with the ReLU that follows it (fd_dense_bn_nhwc.hip).  ``x`` is the
    NCHW-shaped view of contiguous NHWC memory, and so is the result; ``bns`` the tuple of nn.BatchNorm2d modules whose num_features
    partition the channels; ``params`` their weights, then their biases.  The kernels update every module's running statistics and
    counter on the device.  Saves x, y and saved [2, C]: x is what the convolution in front saved as its output's source, y what the next
    one saves as its input."""

    @staticmethod
    def forward(ctx, x, relu, bns, *params):
        y, saved = hip_ops.dense_bn_nhwc_train_forward(x.permute(0, 2, 3, 1), bns, relu=relu)
        # the kernel wrote through raw pointers: the eval plans key their folded-BN weights on these counters (weights_version)
        for bn in bns:
            for buf in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
                torch.autograd.graph.increment_version(buf)
        y = y.permute(0, 3, 1, 2)
        ctx.save_for_backward(x, y, saved)
        ctx.relu, ctx.bns = relu, bns
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, saved = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()  # (no copy for a bf16 channels-last gradient)
        dx, dgamma, dbeta = hip_ops.dense_bn_nhwc_train_backward(dy, x.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1), saved, ctx.bns,
                                                                 relu=ctx.relu)
        if len(ctx.bns) == 1:
            grads = (dgamma, dbeta)
        else:
            sizes = [bn.num_features for bn in ctx.bns]
            grads = tuple(dgamma.split(sizes)) + tuple(dbeta.split(sizes))
        return (dx.permute(0, 3, 1, 2), None, None) + grads


def _map_takes_nhwc(x):
    """a bf16 device map [B, C, H, W], NCHW-shaped over contiguous NHWC memory, C a multiple of 32 in [32, 512], B H W >= 2"""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()
            and hip_ops.dense_bn_nhwc_channels_ok(x.shape[1]) and x.shape[0] * x.shape[2] * x.shape[3] >= 2)


def _module_takes_nhwc(bn, device):
    """a training-mode, affine nn.BatchNorm2d with running statistics and a fixed momentum, gradients enabled, fp32 parameters and
    buffers on ``device``, a multiple of 32 channels"""
    return (isinstance(bn, nn.BatchNorm2d) and bn.training and torch.is_grad_enabled() and bn.affine and bn.track_running_stats
            and bn.momentum is not None and bn.running_mean is not None and bn.num_features % 32 == 0
            and bn.weight.dtype == torch.float32 and bn.weight.device == device
            and bn.running_mean.dtype == torch.float32 and bn.running_mean.device == device)


def batch_norm2d_nhwc_fusable(x, bn):
    """True where batch_norm2d_act_nhwc can take the place of ``bn`` (+ ReLU): a training-mode, affine nn.BatchNorm2d that tracks running
    statistics with a fixed momentum, gradients enabled, a bf16 device map [B, C, H, W] that is NCHW-shaped over contiguous NHWC memory
    (channels-last), C a multiple of 32 in [32, 512], B H W >= 2, fp32 parameters and buffers on the same device."""
    return batch_norm2d_nhwc_group_fusable(x, [bn])


def batch_norm2d_nhwc_group_fusable(x, bns):
    """True where ONE batch_norm2d_act_nhwc call can take the place of the modules ``bns`` (at most 8) on consecutive channel ranges of
    the map ``x``: the map and every module as in batch_norm2d_nhwc_fusable, every num_features a multiple of 32, together all of x's
    channels."""
    bns = list(bns)
    return (1 <= len(bns) <= hip_ops.dense_bn_nhwc_max_groups() and _map_takes_nhwc(x) and all(_module_takes_nhwc(bn, x.device) for bn in bns)
            and sum(bn.num_features for bn in bns) == x.shape[1])


def batch_norm2d_act_nhwc(x, bns, relu=True):
    """relu(bn(x)) in training mode on the bf16 channels-last kernels.  ``x``: the NCHW-shaped bf16 view of contiguous NHWC device
    memory; ``bns``: the existing nn.BatchNorm2d module, or a list of at most 8 modules whose num_features partition the channels of x in
    order (module j normalises the next num_features channels with its own parameters, eps, momentum and buffers: the branches of a
    SepHead on the map of their batched convolution).  Returns the same kind of view, bf16.  One autograd function, differentiable in
    x and in every module's weight and bias.  Raises where batch_norm2d_nhwc_group_fusable(x, bns) does not hold: there is no fallback
    here."""
    bns = (bns,) if isinstance(bns, nn.Module) else tuple(bns)
    if not (isinstance(x, torch.Tensor) and batch_norm2d_nhwc_group_fusable(x, bns)):
        raise hip_ops.FutureDetHipError("batch_norm2d_act_nhwc: needs training-mode affine BatchNorm2d modules with running statistics and a "
                                        "momentum whose num_features (multiples of 32) partition the channels, gradients enabled and a bf16 "
                                        "channels-last device map [B, C, H, W] with C <= 512 and B H W >= 2 (got %s %s)"
                                        % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x), getattr(x, "dtype", None)))
    return _DenseBatchNormNhwcFunction.apply(x, bool(relu), bns, *([bn.weight for bn in bns] + [bn.bias for bn in bns]))
