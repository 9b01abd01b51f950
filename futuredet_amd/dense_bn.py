"""Training-mode BatchNorm2d + ReLU of the dense half (RPN, CenterHead) on the fused kernels of fd_dense_bn.hip: the autograd surface
(batch_norm2d_act), the predicate that says where it applies (batch_norm2d_fusable), and the walk over a Conv2d / BatchNorm2d / ReLU
stack that RPN.fused_bn and CenterHead.fused_bn switch on (run_stack).  fp32 NCHW-contiguous device maps only; everything else keeps
the module chain."""
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
