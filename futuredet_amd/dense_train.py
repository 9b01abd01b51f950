"""Mixed-precision training of the dense convolutions (the RPN neck, the CenterHead) on the bf16 NHWC kernels: the autograd
surfaces (conv2d_bf16 for stride 1; conv2d_s2_bf16, conv_transpose2d_k2_bf16 and conv2d_k2s2_bf16 for the neck's layers that change
resolution; head_tail_bf16 for the head's final convolutions), the predicates that say where they apply (conv_takes_bf16,
conv_s2_takes_bf16, conv_up2_takes_bf16 and conv_down2_takes_bf16 for the neck, head_conv_takes_bf16 / head_tail_takes_bf16 for the
head), and the walk over a ZeroPad2d / Conv2d / BatchNorm2d / ReLU
stack that RPN.train_dtype = torch.bfloat16 switches on (run_stack_bf16).  The recipe is the sparse backbone's: bf16 activations, fp32
master weights packed to bf16 on the device every step, fp32 accumulation, fp32 weight gradients and BatchNorm statistics.  With
``fused_bn`` the walks hand every BatchNorm2d (+ ReLU) that dense_bn.batch_norm2d_nhwc_fusable accepts to
dense_bn.batch_norm2d_act_nhwc (fd_dense_bn_nhwc.hip: bf16 channels-last in and out, no fp32 copy of the map)."""
import torch
from torch import nn

from . import dense_bn, hip_ops
from .sparse import relu_to_bf16


class _Conv2dBf16Function(torch.autograd.Function):
    """One stride-1 convolution (3 x 3 / padding 1 or 1 x 1 / padding 0) on x [B, H, W, Cin] bf16 with the fp32 OIHW weight and, where the
    layer has one, its fp32 bias.

    forward:  fd_conv2d_pack_weight_dev (mode 0) + fd_conv2d_nhwc_bf16 (its bias argument, no ReLU);
    backward: dX on fd_conv2d_nhwc_bf16 again, a Cout -> Cin convolution of dY with the flipped, transposed weights
              (fd_conv2d_pack_weight_dev mode 1); dW on fd_conv2d_wgrad_bf16, fp32; dbias = the column sums of the bf16 dY
              (fd_rows_colsum).  Saves the inputs only.
    Nothing here reads a value back to the host."""

    @staticmethod
    def forward(ctx, x, weight, ks, bias=None):
        wpk = hip_ops.pack_conv2d_weight_device(weight)
        y = hip_ops.conv2d_nhwc_bf16(x, wpk, bias, weight.shape[0], ks, stride=1, relu=False)
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
        if len(ctx.needs_input_grad) == 3:  # the call without a bias
            return dx, dw, None
        db = _colsum(dy.view(-1, dy.shape[3])) if ctx.needs_input_grad[3] else None
        return dx, dw, None, db


def _colsum(rows):
    """fp32 column sums of the bf16 [n, C] rows, C % 32 == 0, on fd_rows_colsum; it takes up to 128 columns, so a wider matrix (the 64 G
    channels of a SepHead's batched branch convolution) goes block of columns by block of columns"""
    c = rows.shape[1]
    if c <= 128 and c & (c - 1) == 0:
        return hip_ops.rows_colsum(rows)
    blk = 128 if c % 128 == 0 else 64 if c % 64 == 0 else 32
    return torch.cat([hip_ops.rows_colsum(rows[:, j:j + blk].contiguous()) for j in range(0, c, blk)])


def conv2d_bf16(x_nhwc, weight, ks, bias=None):
    """y [B, H, W, Cout] bf16 = the stride-1 convolution of x [B, H, W, Cin] (bf16, contiguous, on the device) with ``weight``, the module's
    fp32 [Cout, Cin, ks, ks] parameter, plus ``bias`` (fp32 [Cout], added in fp32 before the one rounding) where given; ks 3 pads by 1,
    ks 1 by 0.  Differentiable in x, weight and bias.  Raises where the kernels do not apply: there is no fallback here."""
    if not (isinstance(x_nhwc, torch.Tensor) and x_nhwc.is_cuda and x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4
            and x_nhwc.is_contiguous()):
        raise hip_ops.FutureDetHipError("conv2d_bf16: x must be a contiguous bf16 [B, H, W, Cin] tensor on the HIP device")
    if not (weight.dtype == torch.float32 and weight.device == x_nhwc.device and weight.dim() == 4 and ks in (1, 3)
            and tuple(weight.shape[1:]) == (x_nhwc.shape[3], ks, ks) and weight.shape[0] % 32 == 0 and weight.shape[1] % 32 == 0):
        raise hip_ops.FutureDetHipError("conv2d_bf16: needs an fp32 [Cout, Cin, %s, %s] weight on x's device with Cin = %d and both channel "
                                        "counts multiples of 32 (got %s %s)" % (ks, ks, x_nhwc.shape[3], tuple(weight.shape), weight.dtype))
    if bias is None:
        return _Conv2dBf16Function.apply(x_nhwc, weight.contiguous(), ks)
    if not (bias.dtype == torch.float32 and bias.device == x_nhwc.device and tuple(bias.shape) == (weight.shape[0],)):
        raise hip_ops.FutureDetHipError("conv2d_bf16: needs an fp32 [%d] bias on x's device (got %s %s)"
                                        % (weight.shape[0], tuple(bias.shape), bias.dtype))
    return _Conv2dBf16Function.apply(x_nhwc, weight.contiguous(), ks, bias.contiguous())


class _Conv2dS2Bf16Function(torch.autograd.Function):
    """The 3 x 3 / stride 2 / padding 1 convolution on x [B, H, W, Cin] bf16 with the fp32 OIHW weight.

    forward:  fd_conv2d_pack_weight_dev (mode 0) + fd_conv2d_nhwc_bf16 with stride 2;
    backward: dX on fd_conv2d_s2_dgrad_bf16 (the mode-1 pack; four parity phases, 9 taps per 2 x 2 block of dX);
              dW on fd_conv2d_wgrad_s2_bf16, fp32.  Saves the inputs only; nothing reads a value back to the host."""

    @staticmethod
    def forward(ctx, x, weight):
        y = hip_ops.conv2d_nhwc_bf16(x, hip_ops.pack_conv2d_weight_device(weight), None, weight.shape[0], 3, stride=2, relu=False)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = hip_ops.conv2d_s2_dgrad_bf16(dy, hip_ops.pack_conv2d_weight_device(weight, transposed=True), x.shape[1], x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1]:
            dw = hip_ops.conv2d_wgrad_s2_bf16(x, dy)
        return dx, dw


class _ConvTranspose2dK2Bf16Function(torch.autograd.Function):
    """ConvTranspose2d(kernel 2, stride 2) on x [B, H, W, Cin] bf16 with the fp32 [Cin, Cout, 2, 2] weight: x is the coarse map.

    forward:  up2 (fd_conv2d_pack_weight_2x2_dev + four placed 1 x 1 launches of fd_conv2d_nhwc_bf16);
    backward: dX = down2 of dY (fd_conv2d_down2_bf16); dW on fd_conv2d_wgrad_2x2_bf16, fp32.  Saves the inputs only."""

    @staticmethod
    def forward(ctx, x, weight):
        y = hip_ops.conv2d_up2_bf16(x, hip_ops.pack_conv2d_weight_2x2_device(weight, hip_ops.PACK_UP2), weight.shape[1])
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = hip_ops.conv2d_down2_bf16(dy, hip_ops.pack_conv2d_weight_2x2_device(weight, hip_ops.PACK_DOWN2), weight.shape[0])
        if ctx.needs_input_grad[1]:
            dw = hip_ops.conv2d_wgrad_2x2_bf16(x, dy)
        return dx, dw


class _Conv2dK2S2Bf16Function(torch.autograd.Function):
    """Conv2d(kernel 2, stride 2) on x [B, H, W, Cin] bf16 with the fp32 [Cout, Cin, 2, 2] weight: x is the fine map.

    forward:  down2 (fd_conv2d_pack_weight_2x2_dev + fd_conv2d_down2_bf16);
    backward: dX = up2 of dY; for an odd H or W it lands in a zero-filled map, whose trailing row or column no output read;
              dW on fd_conv2d_wgrad_2x2_bf16, fp32.  Saves the inputs only."""

    @staticmethod
    def forward(ctx, x, weight):
        y = hip_ops.conv2d_down2_bf16(x, hip_ops.pack_conv2d_weight_2x2_device(weight, hip_ops.PACK_DOWN2), weight.shape[0])
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.to(torch.bfloat16).contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = hip_ops.conv2d_up2_bf16(dy, hip_ops.pack_conv2d_weight_2x2_device(weight, hip_ops.PACK_UP2), weight.shape[1])
            if tuple(dx.shape) != tuple(x.shape):  # (the placed launches address a map of exactly twice the coarse size)
                full = torch.zeros_like(x)
                full[:, :dx.shape[1], :dx.shape[2]] = dx
                dx = full
        if ctx.needs_input_grad[1]:
            dw = hip_ops.conv2d_wgrad_2x2_bf16(dy, x)
        return dx, dw


def _strided_args(name, x_nhwc, weight, kernel, cin_axis, min_hw):
    """the checks the three strided functions share: x a contiguous bf16 [B, H, W, Cin] device map of at least min_hw x min_hw pixels,
    weight fp32 [., ., kernel, kernel] on its device with Cin on ``cin_axis``, both channel counts multiples of 32"""
    if not (isinstance(x_nhwc, torch.Tensor) and x_nhwc.is_cuda and x_nhwc.dtype == torch.bfloat16 and x_nhwc.dim() == 4
            and x_nhwc.is_contiguous()):
        raise hip_ops.FutureDetHipError("%s: x must be a contiguous bf16 [B, H, W, Cin] tensor on the HIP device" % name)
    if not (isinstance(weight, torch.Tensor) and weight.dtype == torch.float32 and weight.device == x_nhwc.device and weight.dim() == 4
            and tuple(weight.shape[2:]) == (kernel, kernel) and weight.shape[cin_axis] == x_nhwc.shape[3] and weight.shape[0] % 32 == 0
            and weight.shape[1] % 32 == 0 and min(x_nhwc.shape[1], x_nhwc.shape[2]) >= min_hw):
        raise hip_ops.FutureDetHipError("%s: needs an fp32 [%s, %d, %d] weight on x's device with Cin = %d, both channel counts multiples of 32, "
                                        "and a map of %d x %d pixels at least (got %s %s, x %s)"
                                        % (name, "Cout, Cin" if cin_axis == 1 else "Cin, Cout", kernel, kernel, x_nhwc.shape[3], min_hw, min_hw,
                                           tuple(weight.shape), weight.dtype, tuple(x_nhwc.shape)))


def conv2d_s2_bf16(x_nhwc, weight):
    """y [B, (H-1)//2+1, (W-1)//2+1, Cout] bf16 = the 3 x 3 / stride 2 / padding 1 convolution of x [B, H, W, Cin] (bf16, contiguous, on the
    device) with ``weight``, the module's fp32 [Cout, Cin, 3, 3] parameter.  Differentiable in x and weight.  Raises where the kernels do
    not apply: there is no fallback here."""
    _strided_args("conv2d_s2_bf16", x_nhwc, weight, 3, 1, 1)
    return _Conv2dS2Bf16Function.apply(x_nhwc, weight.contiguous())


def conv_transpose2d_k2_bf16(x_nhwc, weight):
    """y [B, 2H, 2W, Cout] bf16 = ConvTranspose2d(kernel 2, stride 2) of x [B, H, W, Cin] (bf16, contiguous, on the device) with ``weight``,
    the module's fp32 [Cin, Cout, 2, 2] parameter.  Differentiable in x and weight.  Raises where the kernels do not apply."""
    _strided_args("conv_transpose2d_k2_bf16", x_nhwc, weight, 2, 0, 1)
    return _ConvTranspose2dK2Bf16Function.apply(x_nhwc, weight.contiguous())


def conv2d_k2s2_bf16(x_nhwc, weight):
    """y [B, H//2, W//2, Cout] bf16 = Conv2d(kernel 2, stride 2, padding 0) of x [B, H, W, Cin] (bf16, contiguous, on the device) with
    ``weight``, the module's fp32 [Cout, Cin, 2, 2] parameter.  The trailing row or column of an odd H or W is not read and its gradient is
    exactly zero.  Differentiable in x and weight.  Raises where the kernels do not apply."""
    _strided_args("conv2d_k2s2_bf16", x_nhwc, weight, 2, 1, 2)
    return _Conv2dK2S2Bf16Function.apply(x_nhwc, weight.contiguous())


class _HeadTailBf16Function(torch.autograd.Function):
    """The final convolutions of one SepHead's branches (3 x 3 / padding 1, Cin % 32 == 0, at most 16 output channels, a bias) in one
    launch per pass on fd_head_tail_bf16.hip: bf16 NHWC in, fp32 NCHW out.  ``meta`` holds, per group, (index of its x among the distinct
    x tensors, first channel); the tensors are the distinct xs, then every group's weight, then every group's bias.  Saves the inputs
    only; the input gradient of an x is one bf16 tensor that every group fills its own channel slice of."""

    @staticmethod
    def forward(ctx, meta, n_x, *tensors):
        n = len(meta)
        xs, ws, bs = tensors[:n_x], tensors[n_x:n_x + n], tensors[n_x + n:]
        ys = hip_ops.head_tail_forward([(xs[xi], c0, ws[i], bs[i]) for i, (xi, c0) in enumerate(meta)])
        ctx.save_for_backward(*tensors)
        ctx.meta, ctx.n_x = meta, n_x
        return tuple(ys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dys):
        meta, n_x, n = ctx.meta, ctx.n_x, len(ctx.meta)
        tensors = ctx.saved_tensors
        xs, ws = tensors[:n_x], tensors[n_x:n_x + n]
        dys = [dy.to(torch.float32).contiguous() for dy in dys]
        need = ctx.needs_input_grad[2:]
        dxs = [None] * n_x
        for j in range(n_x):
            if need[j]:
                covered = sum(ws[i].shape[1] for i, (xi, _) in enumerate(meta) if xi == j)
                dxs[j] = (torch.empty_like if covered == xs[j].shape[3] else torch.zeros_like)(xs[j])
        todo = [(dxs[xi], c0, ws[i], dys[i]) for i, (xi, c0) in enumerate(meta) if dxs[xi] is not None]
        if todo:
            hip_ops.head_tail_dgrad(todo)
        dws, dbs = [None] * n, [None] * n
        idx = [i for i in range(n) if need[n_x + i] or need[n_x + n + i]]
        if idx:
            got = hip_ops.head_tail_wgrad([(xs[meta[i][0]], meta[i][1], ws[i].shape[1], dys[i]) for i in idx])
            for i, (dw, db) in zip(idx, got):
                dws[i], dbs[i] = (dw if need[n_x + i] else None), (db if need[n_x + n + i] else None)
        return (None, None) + tuple(dxs) + tuple(dws) + tuple(dbs)


def head_tail_bf16(groups):
    """The final convolutions of a SepHead in one call: ``groups`` is a list of (x, weight, bias) or (x, weight, bias, c0); x a contiguous
    bf16 [B, H, W, C] device tensor of which the group reads channels c0 .. c0 + Cin - 1 (c0 = 0 by default, a multiple of 8; several
    groups may read slices of one x, which must then not overlap), weight fp32 [k, Cin, 3, 3] with Cin % 32 == 0 and 1 <= k <= 16, bias
    fp32 [k].  Returns the list of fp32 NCHW [B, k, H, W] maps: weights rounded to bf16, fp32 accumulation, fp32 bias, no second
    rounding.  Differentiable in every x, weight and bias.  Raises where the kernels do not apply."""
    xs, meta, ws, bs = [], [], [], []
    for g in groups:
        x, w, b = g[0], g[1], g[2]
        c0 = int(g[3]) if len(g) > 3 else 0
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.is_contiguous()):
            raise hip_ops.FutureDetHipError("head_tail_bf16: x must be a contiguous bf16 [B, H, W, C] tensor on the HIP device")
        if not (w.dtype == torch.float32 and w.device == x.device and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.shape[1] % 32 == 0
                and 1 <= w.shape[0] <= 16 and b is not None and b.dtype == torch.float32 and b.device == x.device
                and tuple(b.shape) == (w.shape[0],)):
            raise hip_ops.FutureDetHipError("head_tail_bf16: needs an fp32 [k, Cin, 3, 3] weight with Cin %% 32 == 0 and 1 <= k <= 16 and an "
                                            "fp32 [k] bias on x's device (got %s)" % (tuple(w.shape),))
        for j, other in enumerate(xs):
            if other is x:
                break
        else:
            j = len(xs)
            xs.append(x)
        meta.append((j, c0))
        ws.append(w.contiguous())
        bs.append(b.contiguous())
    return list(_HeadTailBf16Function.apply(tuple(meta), len(xs), *(xs + ws + bs)))


def _conv3_takes(conv, x):
    """an nn.Conv2d with a 3 x 3 kernel, padding 1, stride 1, dilation 1, groups 1, an fp32 weight on x's device, in_channels % 32 == 0"""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (3, 3) and tuple(conv.padding) == (1, 1) and conv.padding_mode == "zeros"
            and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.in_channels % 32 == 0
            and conv.weight.dtype == torch.float32 and conv.weight.device == x.device)


def head_conv_takes_bf16(conv, x):
    """True where conv2d_bf16 (with the layer's bias, if it has one) can take the place of ``conv`` in the head: a 3 x 3 / padding 1 /
    stride 1 nn.Conv2d, dilation 1, groups 1, in_channels and out_channels multiples of 32, an fp32 weight on x's device."""
    return _conv3_takes(conv, x) and conv.out_channels % 32 == 0


def head_tail_takes_bf16(conv, x):
    """True where ``conv`` can be a group of head_tail_bf16: a 3 x 3 / padding 1 / stride 1 nn.Conv2d with a bias, dilation 1, groups 1,
    in_channels a multiple of 32, at most 16 output channels, an fp32 weight on x's device."""
    return _conv3_takes(conv, x) and conv.bias is not None and 1 <= conv.out_channels <= 16


def _to_nhwc(x):
    """contiguous [B, H, W, C] memory of an NCHW-shaped map (no copy for a channels-last one)"""
    return x.permute(0, 2, 3, 1).contiguous()


def _batch_norm_bf16(m, nxt, x, fused_bn):
    """BatchNorm2d ``m`` (+ the nn.ReLU ``nxt`` behind it) on the NCHW-shaped map ``x`` -> (bf16 result, modules consumed).  With
    ``fused_bn`` and a fusable module: one batch_norm2d_act_nhwc call.  Otherwise the un-fused recipe: bn(x.float()) with fp32 batch and
    running statistics, the ReLU, one rounding to bf16."""
    act = isinstance(nxt, nn.ReLU)
    if fused_bn and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4:
        # torch's own convolutions (stride 2, transposed) may hand back NCHW memory: the permuting copy that the next conv2d_bf16 would
        # make moves in front of the BatchNorm2d (no copy for a channels-last map)
        xc = x.contiguous(memory_format=torch.channels_last)
        if dense_bn.batch_norm2d_nhwc_fusable(xc, m):
            return dense_bn.batch_norm2d_act_nhwc(xc, m, relu=act), 1 + act
    out = m(x.float())
    return (relu_to_bf16(out) if act else out.to(torch.bfloat16)), 1 + act


def run_head_stack_bf16(mods, x, fused_bn=False):
    """The modules ``mods`` (a list of Conv2d / BatchNorm2d / ReLU of the CenterHead) on ``x`` in mixed precision.  ``x`` is NCHW-shaped:
    a bf16 channels-last device map, or the fp32 form of one in front of a BatchNorm2d; the result is bf16 channels-last.

      * a convolution that satisfies head_conv_takes_bf16: conv2d_bf16 with its bias;
      * any other convolution (bev_conv's 6- and 16-channel layers): the module on an fp32 copy of its input, rounded to bf16;
      * BatchNorm2d: bn(x.float()) with fp32 batch and running statistics, the ReLU that follows, one rounding to bf16; with
        ``fused_bn``, a module that dense_bn.batch_norm2d_nhwc_fusable accepts on the bf16 channels-last map is one
        batch_norm2d_act_nhwc call instead (relu=False where no ReLU follows)."""
    i = 0
    while i < len(mods):
        m = mods[i]
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if isinstance(m, nn.Conv2d):
            if head_conv_takes_bf16(m, x):
                x = conv2d_bf16(_to_nhwc(x.to(torch.bfloat16)), m.weight, 3, m.bias).permute(0, 3, 1, 2)
            else:
                x = m(x.float()).to(torch.bfloat16)
            i += 1
        elif isinstance(m, nn.BatchNorm2d):
            x, used = _batch_norm_bf16(m, nxt, x, fused_bn)
            i += used
        elif isinstance(m, nn.ReLU):  # out of place: the input may be saved for a backward
            x = torch.relu(x).to(torch.bfloat16)
            i += 1
        else:
            raise NotImplementedError("run_head_stack_bf16: no mixed-precision form of %s" % type(m).__name__)
    return x


def sep_head_bf16(task, x, fused_bn=False):
    """SepHead.forward_modules in mixed precision on the bf16 channels-last device map ``x`` (NCHW-shaped): the dict of the module chain,
    ``feats`` bf16 channels-last, every branch's map fp32 NCHW contiguous.

      * forecast_conv: run_head_stack_bf16;
      * the leading convolutions of the branches, where every branch has one that satisfies head_conv_takes_bf16 and they agree in shape:
        ONE conv2d_bf16 call on torch.cat of their weights and biases (autograd splits the gradients back); otherwise each on its own;
      * each branch's own BatchNorm2d + ReLU on its channels of that result;
      * the final convolutions that satisfy head_tail_takes_bf16: ONE head_tail_bf16 call; any other runs its module on an fp32 copy.

    With ``fused_bn``, where the batched convolution ran, there are at most 8 branches and every branch's middle is exactly a fusable
    BatchNorm2d + ReLU: ONE grouped batch_norm2d_act_nhwc call on the whole map (module j on branch j's channels), no fp32 copy and no
    split, and the final convolutions read their channel slices of that one tensor through head_tail_bf16's c0.  Where the branches
    run on their own, each BatchNorm2d is fused where it can be (run_head_stack_bf16); behind a batched convolution whose branches do
    not qualify together, the un-fused recipe stays."""
    ret = {}
    if task.forecast_feature:
        x = run_head_stack_bf16(list(task.forecast_conv.children()), x, fused_bn)
        ret["feats"] = x
    names = list(task.heads)
    stacks = [list(getattr(task, h).children()) for h in names]
    first = [s[0] for s in stacks]
    whole = None  # the grouped path: every branch's input of its final convolution is a channel slice of this one map
    if (len(names) > 1 and all(len(s) >= 2 and head_conv_takes_bf16(s[0], x) and s[0].bias is not None for s in stacks)
            and len(set((c.in_channels, c.out_channels) for c in first)) == 1):
        y = conv2d_bf16(_to_nhwc(x), torch.cat([c.weight for c in first]), 3, torch.cat([c.bias for c in first])).permute(0, 3, 1, 2)
        width = first[0].out_channels
        if (fused_bn and all(len(s) == 4 and isinstance(s[2], nn.ReLU) for s in stacks)
                and dense_bn.batch_norm2d_nhwc_group_fusable(y, [s[1] for s in stacks])):
            whole = dense_bn.batch_norm2d_act_nhwc(y, [s[1] for s in stacks], relu=True)
            whole_nhwc = _to_nhwc(whole)
            feats = [whole[:, j * width:(j + 1) * width] for j in range(len(names))]
        else:
            parts = y.float().split(width, dim=1)  # one conversion and one split: their backward is one cat
            feats = [run_head_stack_bf16(s[1:-1], p) for s, p in zip(stacks, parts)]
    else:
        feats = [run_head_stack_bf16(s[:-1], x, fused_bn) for s in stacks]
    groups, tails = [], []
    for j, (h, s, f) in enumerate(zip(names, stacks, feats)):
        f = f.to(torch.bfloat16)
        if head_tail_takes_bf16(s[-1], f):
            if whole is not None:  # one x for every group (head_tail_bf16 tells the tensors apart by identity): one input gradient
                groups.append((whole_nhwc, s[-1].weight, s[-1].bias, j * width))
            else:
                groups.append((_to_nhwc(f), s[-1].weight, s[-1].bias))
            tails.append(h)
            ret[h] = None  # keeps the chain's key order
        else:
            ret[h] = s[-1](f.float()).contiguous()
    if groups:
        for h, y in zip(tails, head_tail_bf16(groups)):
            ret[h] = y
    return ret


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


def _strided_takes(conv, x, cls, kernel, padding):
    """a ``cls`` module of kernel size ``kernel``, stride 2 and ``padding`` on every side: no bias, groups 1, dilation 1, zero padding, an
    fp32 weight on x's device, both channel counts multiples of 32"""
    return (isinstance(conv, cls) and conv.kernel_size == (kernel, kernel) and conv.stride == (2, 2) and tuple(conv.padding) == (padding, padding)
            and conv.padding_mode == "zeros" and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is None
            and tuple(getattr(conv, "output_padding", (0, 0))) == (0, 0) and conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0
            and conv.weight.dtype == torch.float32 and conv.weight.device == x.device)


def conv_s2_takes_bf16(conv, x):
    """True where conv2d_s2_bf16 can take the place of ``conv`` on the map ``x``: an nn.Conv2d with a 3 x 3 kernel, stride 2 and padding 1,
    dilation 1, groups 1, no bias, in_channels and out_channels multiples of 32, an fp32 weight on x's device."""
    return _strided_takes(conv, x, nn.Conv2d, 3, 1)


def _pad_then_conv_s2_takes_bf16(pad, conv, x):
    """nn.ZeroPad2d(1) + a 3 x 3 / padding 0 / stride 2 convolution that otherwise satisfies conv_s2_takes_bf16: together one 3 x 3 /
    stride 2 / padding 1 (the eval plan merges them the same way)."""
    return isinstance(pad, nn.ZeroPad2d) and tuple(pad.padding) == (1, 1, 1, 1) and _strided_takes(conv, x, nn.Conv2d, 3, 0)


def conv_up2_takes_bf16(conv, x):
    """True where conv_transpose2d_k2_bf16 can take the place of ``conv``: an nn.ConvTranspose2d with a 2 x 2 kernel, stride 2, no padding
    or output padding, dilation 1, groups 1, no bias, both channel counts multiples of 32, an fp32 weight on x's device."""
    return _strided_takes(conv, x, nn.ConvTranspose2d, 2, 0)


def conv_down2_takes_bf16(conv, x):
    """True where conv2d_k2s2_bf16 can take the place of ``conv``: an nn.Conv2d with a 2 x 2 kernel, stride 2 and padding 0, dilation 1,
    groups 1, no bias, both channel counts multiples of 32, an fp32 weight on x's device, on a map of 2 x 2 pixels at least."""
    return _strided_takes(conv, x, nn.Conv2d, 2, 0) and x.dim() == 4 and min(x.shape[2], x.shape[3]) >= 2


def _strided_module_bf16(fn, conv, x):
    """``conv`` through one of the strided functions on an NCHW-shaped view of NHWC memory; returns the same kind of view"""
    return fn(x.permute(0, 2, 3, 1).contiguous(), conv.weight).permute(0, 3, 1, 2)  # (no copy for a channels-last map)


def _conv_module_bf16(conv, x):
    """``conv`` through conv2d_bf16 on an NCHW-shaped view of NHWC memory; returns the same kind of view"""
    y = conv2d_bf16(x.permute(0, 2, 3, 1).contiguous(), conv.weight, conv.kernel_size[0])  # (no copy for a channels-last map)
    return y.permute(0, 3, 1, 2)


def run_stack_bf16(modules, x, fused_bn=False):
    """``modules(x)`` for a Sequential of ZeroPad2d, convolutions, BatchNorm2d and ReLU in mixed precision.  ``x`` is a bf16 device map,
    NCHW-shaped over NHWC memory (channels-last), and so is the result; no permuting copy in between.

      * nn.ZeroPad2d(1) directly followed by a 3 x 3 / padding 0 / stride 1 convolution that otherwise satisfies conv_takes_bf16: the
        pair is one conv2d_bf16 call (the eval plan merges them the same way);
      * a convolution that satisfies conv_takes_bf16: conv2d_bf16;
      * nn.ZeroPad2d(1) directly followed by a 3 x 3 / padding 0 / stride 2 convolution (_pad_then_conv_s2_takes_bf16), or a convolution
        that satisfies conv_s2_takes_bf16 -- the opener of a down-sampling stage: conv2d_s2_bf16;
      * an nn.ConvTranspose2d(2, stride 2) that satisfies conv_up2_takes_bf16: conv_transpose2d_k2_bf16;
      * any other convolution (a bias, other kernel sizes or strides, channel counts that are no multiples of 32): the module on an
        fp32 copy of its input, the result rounded to bf16.  The nn.Conv2d(2, stride 2) deblock of the PointPillars neck is among them
        although conv2d_k2s2_bf16 can run it (conv_down2_takes_bf16): at its shipped shape its forward + backward was not faster than
        this recipe by more than the recipe's own spread (229 us against 245 us, profiles/dense_conv_strided_bf16.txt), so the walk does
        not route it;
      * BatchNorm2d: the sparse backbone's un-fused mixed-precision recipe -- bn(x.float()) with fp32 batch and running statistics, the
        ReLU that follows, one rounding to bf16; with ``fused_bn``, a module that dense_bn.batch_norm2d_nhwc_fusable accepts is one
        batch_norm2d_act_nhwc call instead (relu=False where no ReLU follows)."""
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
        elif nxt is not None and _pad_then_conv_s2_takes_bf16(m, nxt, x):
            x = _strided_module_bf16(conv2d_s2_bf16, nxt, x)
            i += 2
        elif conv_s2_takes_bf16(m, x):
            x = _strided_module_bf16(conv2d_s2_bf16, m, x)
            i += 1
        elif conv_up2_takes_bf16(m, x):
            x = _strided_module_bf16(conv_transpose2d_k2_bf16, m, x)
            i += 1
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            x = m(x.float()).to(torch.bfloat16)
            i += 1
        elif isinstance(m, nn.BatchNorm2d):
            x, used = _batch_norm_bf16(m, nxt, x, fused_bn)
            i += used
        else:  # ZeroPad2d in front of a convolution that stays on torch, a ReLU on its own: exact on bf16
            x = m(x)
            i += 1
    return x
