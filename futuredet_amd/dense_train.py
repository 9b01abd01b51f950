"""Mixed-precision training of the dense stride-1 convolutions (the RPN neck) on the bf16 NHWC kernels: the autograd surface
(conv2d_bf16), the predicate that says where it applies (conv_takes_bf16), and the walk over a ZeroPad2d / Conv2d / BatchNorm2d / ReLU
stack that RPN.train_dtype = torch.bfloat16 switches on (run_stack_bf16).  The recipe is the sparse backbone's: bf16 activations, fp32
master weights packed to bf16 on the device every step, fp32 accumulation, fp32 weight gradients and BatchNorm statistics."""
import torch
from torch import nn

from . import hip_ops
from .sparse import relu_to_bf16


class _Conv2dBf16Function(torch.autograd.Function):
    """One stride-1 convolution (3 x 3 / padding 1 or 1 x 1 / padding 0, no bias) on x [B, H, W, Cin] bf16 with the fp32 OIHW weight.

    forward:  fd_conv2d_pack_weight_dev (mode 0) + fd_conv2d_nhwc_bf16 (no bias, no ReLU);
    backward: dX on fd_conv2d_nhwc_bf16 again, a Cout -> Cin convolution of dY with the flipped, transposed weights
              (fd_conv2d_pack_weight_dev mode 1); dW on fd_conv2d_wgrad_bf16, fp32.  Saves the inputs only.
    Nothing here reads a value back to the host."""

    @staticmethod
    def forward(ctx, x, weight, ks):
        wpk = hip_ops.pack_conv2d_weight_device(weight)
        y = hip_ops.conv2d_nhwc_bf16(x, wpk, None, weight.shape[0], ks, stride=1, relu=False)
        ctx.save_for_backward(x, weight)
        ctx.ks = ks
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wpk = hip_ops.pack_conv2d_weight_device(weight, transposed=True)
            dx = hip_ops.conv2d_nhwc_bf16(dy, wpk, None, weight.shape[1], ctx.ks, stride=1, relu=False)
        if ctx.needs_input_grad[1]:
            dw = hip_ops.conv2d_wgrad_bf16(x, dy, ctx.ks)
        return dx, dw, None


def conv2d_bf16(x_nhwc, weight, ks):
    """y [B, H, W, Cout] bf16 = the stride-1 convolution of x [B, H, W, Cin] (bf16, contiguous, on the device) with ``weight``, the module's
    fp32 [Cout, Cin, ks, ks] parameter; ks 3 pads by 1, ks 1 by 0.  Differentiable in both.  Raises where the kernels do not apply: there
    is no fallback here."""
    if not (isinstance(x_nhwc, torch.Tensor) and x_nhwc.is_cuda and x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4
            and x_nhwc.is_contiguous()):
        raise hip_ops.FutureDetHipError("conv2d_bf16: x must be a contiguous bf16 [B, H, W, Cin] tensor on the HIP device")
    if not (weight.dtype == torch.float32 and weight.device == x_nhwc.device and weight.dim() == 4 and ks in (1, 3)
            and tuple(weight.shape[1:]) == (x_nhwc.shape[3], ks, ks) and weight.shape[0] % 32 == 0 and weight.shape[1] % 32 == 0):
        raise hip_ops.FutureDetHipError("conv2d_bf16: needs an fp32 [Cout, Cin, %s, %s] weight on x's device with Cin = %d and both channel "
                                        "counts multiples of 32 (got %s %s)" % (ks, ks, x_nhwc.shape[3], tuple(weight.shape), weight.dtype))
    return _Conv2dBf16Function.apply(x_nhwc, weight.contiguous(), ks)


def _conv_takes(conv, x, padding):
    """an nn.Conv2d of kernel size ``ks`` in (1, 3) with ``padding[ks]`` on every side that conv2d_bf16 can run otherwise"""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size in ((1, 1), (3, 3)) and tuple(conv.padding) == (padding[conv.kernel_size[0]],) * 2
            and conv.padding_mode == "zeros" and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0 and conv.weight.dtype == torch.float32
            and conv.weight.device == x.device)


def conv_takes_bf16(conv, x):
    """True where conv2d_bf16 can take the place of ``conv`` on the map ``x``: an nn.Conv2d with a 3 x 3 kernel and padding 1 or a 1 x 1
    kernel and padding 0, stride 1, dilation 1, groups 1, no bias, in_channels and out_channels multiples of 32, an fp32 weight on x's
    device."""
    return _conv_takes(conv, x, {1: 0, 3: 1})


def _pad_then_conv_takes_bf16(pad, conv, x):
    """nn.ZeroPad2d(1) + a 3 x 3 / padding 0 convolution that otherwise satisfies conv_takes_bf16: together one 3 x 3 / padding 1."""
    return isinstance(pad, nn.ZeroPad2d) and tuple(pad.padding) == (1, 1, 1, 1) and _conv_takes(conv, x, {1: None, 3: 0})


def _conv_module_bf16(conv, x):
    """``conv`` through conv2d_bf16 on an NCHW-shaped view of NHWC memory; returns the same kind of view"""
    y = conv2d_bf16(x.permute(0, 2, 3, 1).contiguous(), conv.weight, conv.kernel_size[0])  # (no copy for a channels-last map)
    return y.permute(0, 3, 1, 2)


def run_stack_bf16(modules, x):
    """``modules(x)`` for a Sequential of ZeroPad2d, convolutions, BatchNorm2d and ReLU in mixed precision.  ``x`` is a bf16 device map,
    NCHW-shaped over NHWC memory (channels-last), and so is the result; no permuting copy in between.

      * nn.ZeroPad2d(1) directly followed by a 3 x 3 / padding 0 / stride 1 convolution that otherwise satisfies conv_takes_bf16: the
        pair is one conv2d_bf16 call (the eval plan merges them the same way);
      * a convolution that satisfies conv_takes_bf16: conv2d_bf16;
      * any other convolution (stride 2 behind its ZeroPad2d, ConvTranspose2d): the module on an fp32 copy of its input, the result
        rounded to bf16;
      * BatchNorm2d: the sparse backbone's un-fused mixed-precision recipe -- bn(x.float()) with fp32 batch and running statistics, the
        ReLU that follows, one rounding to bf16."""
    mods = list(modules.children())
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if nxt is not None and _pad_then_conv_takes_bf16(m, nxt, x):
            x = _conv_module_bf16(nxt, x)
            i += 2
        elif conv_takes_bf16(m, x):
            x = _conv_module_bf16(m, x)
            i += 1
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            x = m(x.float()).to(torch.bfloat16)
            i += 1
        elif isinstance(m, nn.BatchNorm2d):
            out = m(x.float())
            if isinstance(nxt, nn.ReLU):
                x = relu_to_bf16(out)
                i += 2
            else:
                x = out.to(torch.bfloat16)
                i += 1
        else:  # ZeroPad2d in front of a strided convolution, a ReLU on its own: exact on bf16
            x = m(x)
            i += 1
    return x
