"""spconv-1.0 module surface on the HIP kernels.

The reference's backbone (det3d/models/backbones/scn.py:2-3,13-21,37,98-165) is written against spconv 1.0:
``SparseConvTensor(features, indices, spatial_shape, batch_size)``, ``SubMConv3d`` / ``SparseConv3d`` with the
keyword names (in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
indice_key=None), weight ``Parameter(*kernel_size, Cin, Cout)``, ``SparseSequential``, ``.dense()``.  This module
keeps that surface; underneath, an active set is a ``hip_ops.SparseIndex`` (bitmap + prefix, rows spatially
sorted) and a convolution is one ``fd_spconv_apply`` launch on an output-stationary rulebook.

Row order: spconv leaves the output row order unspecified (it differs between its own CPU and GPU paths);
here rows are always in index order.  ``SparseConvTensor`` re-orders the features / indices it is given once,
at construction, so ``.features`` and ``.indices`` always agree.
"""
import math

import numpy as np
import torch
from torch import nn

from . import hip_ops

CH_ALIGN = 16  # MFMA K granularity of fd_spconv_apply; narrower inputs are zero padded


def _triple(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        assert len(v) == 3
        return [int(x) for x in v]
    return [int(v)] * 3


def pad_channels(c):
    return max(CH_ALIGN, (c + CH_ALIGN - 1) // CH_ALIGN * CH_ALIGN)


class SparseConvTensor(object):
    def __init__(self, features, indices, spatial_shape, batch_size, grid=None, _index=None):
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {}
        self.grid = grid
        if _index is not None:  # internal: already in index order
            self.index = _index
            self.features = features
            return
        indices = indices.int().contiguous()
        D, H, W = self.spatial_shape
        idx = hip_ops.SparseIndex(self.batch_size, D, H, W, features.device)
        n_dev = torch.zeros((1,), dtype=torch.int32, device=features.device)
        idx.mark(indices)
        idx.scan(n_dev)
        idx.finalize(int(n_dev.cpu()[0]))
        row_of = idx.lookup(indices)
        self.index = idx
        self._true_channels = features.shape[1]
        src = features.float().contiguous()
        if torch.is_grad_enabled() and src.requires_grad:
            self.features = _RowsPermute.apply(src, row_of, idx.n)
        else:
            self.features = hip_ops.rows_permute(src, row_of, features.shape[1], torch.float32, n_rows=idx.n)

    @property
    def indices(self):
        return self.index.coords

    def find_indice_pair(self, key):
        return self.indice_dict.get(key) if key is not None else None

    def dense(self, channels_first=True):
        feats = self.features.contiguous()
        if torch.is_grad_enabled() and feats.requires_grad:
            out = _Densify.apply(feats, self.index)
        else:
            out = hip_ops.densify(feats, self.index)  # [B, C*D, H, W], channel = c*D + d
        B, C, D = self.batch_size, feats.shape[1], self.index.D
        out = out.view(B, C, D, self.index.H, self.index.W)
        if not channels_first:
            out = out.permute(0, 2, 3, 4, 1).contiguous()
        return out


class SparseModule(nn.Module):
    pass


# ------------------------------------------------------------------------------------------------ autograd (training)
class _RowsPermute(torch.autograd.Function):
    """features (input order) -> rows in index order; backward: the gather by ``row_of``."""

    @staticmethod
    def forward(ctx, src, row_of, n_rows):
        ctx.save_for_backward(row_of)
        return hip_ops.rows_permute(src, row_of, src.shape[1], torch.float32, n_rows=n_rows)

    @staticmethod
    def backward(ctx, grad):
        (row_of,) = ctx.saved_tensors
        keep = row_of >= 0
        g = grad[row_of.long().clamp(min=0)]
        return g * keep[:, None].to(g.dtype), None, None


class _Densify(torch.autograd.Function):
    """SparseConvTensor.dense(): fd_densify forward, fd_dense_gather backward."""

    @staticmethod
    def forward(ctx, feats, index):
        ctx.index, ctx.dtype = index, feats.dtype
        return hip_ops.densify(feats, index)

    @staticmethod
    def backward(ctx, grad):
        g = hip_ops.dense_gather(grad.float(), ctx.index, grad.shape[1] // ctx.index.D)
        return (g if ctx.dtype == torch.float32 else g.to(ctx.dtype)), None


class _ReluToBf16(torch.autograd.Function):
    """relu(x).to(bfloat16) of an fp32 x in one node that saves only its bf16 output -- the tensor the next convolution saves anyway -- where
    the two torch ops would keep the fp32 ReLU output as well.  The mask is y > 0: a positive fp32 value rounds to a positive bf16 value
    (the formats share the exponent range; only values below 2^-134 vanish, and they carry no gradient worth the name)."""

    @staticmethod
    def forward(ctx, x):
        y = torch.relu(x).to(torch.bfloat16)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return dy.float() * (y > 0)


def relu_to_bf16(x):
    return _ReluToBf16.apply(x)


class _SparseConvFunction(torch.autograd.Function):
    """One sparse convolution on channel-padded tensors: feats [n_in, cin_p] fp32 or bf16, weight [K, cin_p, cout_p] and bias [cout_p] (or
    None) always fp32 -- bf16 rows are mixed precision: fp32 master weights packed to bf16 on the device, fp32 accumulation, the fp32 bias
    added before the one rounding of the output, bf16 dX, fp32 dW and dBias.

    forward:  fd_spconv_apply with device-packed weights (no BN folding, no fused ReLU / residual);
    backward: dX on fd_spconv_apply again (SubM: the same table with W[K-1-k]^T; strided: the transposed table with W[k]^T),
              dW on fd_spconv_wgrad / fd_spconv_wgrad_bf16, dBias = sum of dY.  Saves the inputs only (an in-place ReLU follows the output)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, nbr, n_out, subm):
        wpk = hip_ops.pack_spconv_weight_device(weight, hip_ops.PACK_PLAIN, feats.dtype)
        out = hip_ops.spconv_apply(feats, wpk, bias, nbr, n_out, weight.shape[2], plan=False)
        ctx.save_for_backward(feats, weight)
        ctx.nbr, ctx.n_out, ctx.subm, ctx.has_bias = nbr, n_out, subm, bias is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        feats, weight = ctx.saved_tensors
        nbr, n_out = ctx.nbr, ctx.n_out
        n_in, cin_p = feats.shape
        dt = feats.dtype
        dy = dy.to(dt).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.subm:  # the SubM table is symmetric: nbr[k][o] = i <=> nbr[K-1-k][i] = o
                wt = hip_ops.pack_spconv_weight_device(weight, hip_ops.PACK_FLIPPED_TRANSPOSED, dt)
                dx = hip_ops.spconv_apply(dy, wt, None, nbr, n_in, cin_p, plan=False)
            else:
                inv = getattr(nbr, "inv", None)  # cached with the rulebook (indice_key)
                if inv is None:
                    inv = nbr.inv = hip_ops.rulebook_transpose(nbr, n_out, n_in)
                    if getattr(nbr, "n_in_dev", None) is not None:  # static indexes: dX has the INPUT level's rows, n_in is their capacity
                        inv.n_dev, inv.n_expected = nbr.n_in_dev, nbr.n_in_expected
                wt = hip_ops.pack_spconv_weight_device(weight, hip_ops.PACK_TRANSPOSED, dt)
                dx = hip_ops.spconv_apply(dy, wt, None, inv, n_in, cin_p, plan=False)
        if ctx.needs_input_grad[1]:
            dw = hip_ops.spconv_wgrad(feats, dy, nbr, n_out)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if getattr(nbr, "n_dev", None) is not None:  # the count lives on the device; the rows behind it are uninitialised memory
                db = hip_ops.rows_colsum(dy[:n_out], nbr.n_dev)
            else:
                db = dy[:n_out].sum(0) if dt == torch.float32 else dy[:n_out].float().sum(0)
        return dx, dw, db, None, None, None


class _SparseBatchNormFunction(torch.autograd.Function):
    """Training-mode BatchNorm1d over the rows of x [n, C] fused with the residual add and ReLU that follow it (fd_sparse_bn.hip):
    y = act(gamma (x - mean) invstd + beta [+ residual]).  ``bn`` is the nn.BatchNorm1d module: the kernel updates its running
    statistics and num_batches_tracked on the device.  Saves x and y: y is what the next convolution saves as its input.
    x fp32 or bf16 (mixed precision): residual, y and every row gradient have x's dtype; gamma, beta, their gradients and the
    statistics are fp32.  On bf16 rows no fp32 [n, C] tensor exists at any point."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, bn, relu, n_dev=None):
        y, saved = hip_ops.sparse_bn_train_forward(x, gamma, beta, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps,
                                                   bn.momentum, residual=residual, relu=relu, n_dev=n_dev)
        # the kernel wrote through raw pointers: packed_weight keys the eval path's folded-BN cache on these counters
        for buf in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
            torch.autograd.graph.increment_version(buf)
        ctx.save_for_backward(x, y, gamma, saved)
        ctx.relu, ctx.n_dev = relu, n_dev
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y, gamma, saved = ctx.saved_tensors
        want_res = ctx.needs_input_grad[3]
        dx, dres, dgamma, dbeta = hip_ops.sparse_bn_train_backward(dy.to(x.dtype).contiguous(), x, y, gamma, saved, relu=ctx.relu,
                                                                   want_residual=want_res, n_dev=ctx.n_dev)
        return dx, dgamma, dbeta, dres, None, None, None


def batch_norm_fusable(features, bn):
    """True where batch_norm_act can take the place of ``bn`` (+ residual add + ReLU): a training-mode, affine nn.BatchNorm1d that
    tracks running statistics with a fixed momentum, gradients enabled, fp32 or bf16 device features [n >= 2, C] with a supported C
    (the parameters and buffers are fp32 either way)."""
    return (isinstance(bn, nn.BatchNorm1d) and bn.training and torch.is_grad_enabled() and bn.affine and bn.track_running_stats
            and bn.momentum is not None and bn.running_mean is not None and features.is_cuda and features.dtype in (torch.float32, torch.bfloat16)
            and bn.weight.dtype == torch.float32 and bn.weight.device == features.device and features.dim() == 2
            and features.shape[0] >= 2 and hip_ops.sparse_bn_channels_ok(features.shape[1]))


def batch_norm_act(features, bn, residual=None, relu=True, n_dev=None):
    """relu(bn(features) [+ residual]) in training mode on the fused kernels; ``bn`` is the existing nn.BatchNorm1d module (parameters,
    buffers and state-dict keys unchanged).  Raises where batch_norm_fusable(features, bn) does not hold: there is no fallback here.
    ``n_dev`` (int32 [1] on the device): the valid row count of static indexes -- features.shape[0] is then the row capacity; both
    directions take their statistics over the counted rows and write zeros behind them."""
    if not batch_norm_fusable(features, bn):
        raise hip_ops.FutureDetHipError("batch_norm_act: needs a training-mode affine BatchNorm1d with running statistics and a momentum, "
                                        "gradients enabled and fp32 or bf16 device features [n >= 2, C], C a multiple of 16 up to 128 (got %s %s)"
                                        % (tuple(features.shape), features.dtype))
    if residual is not None:
        residual = residual.to(features.dtype).contiguous()
    if n_dev is None:  # (the call as it always was)
        return _SparseBatchNormFunction.apply(features.contiguous(), bn.weight, bn.bias, residual, bn, bool(relu))
    return _SparseBatchNormFunction.apply(features.contiguous(), bn.weight, bn.bias, residual, bn, bool(relu), n_dev)


class SparseConvolution(SparseModule):
    def __init__(self, ndim, in_channels, out_channels, kernel_size=3, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, subm=False, indice_key=None):
        super().__init__()
        assert ndim == 3 and groups == 1 and _triple(dilation) == [1, 1, 1]
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size = _triple(kernel_size)
        self.stride = _triple(stride)
        self.padding = _triple(padding)
        self.subm = subm
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.Tensor(*self.kernel_size, in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self._packed = {}
        self.register_load_state_dict_post_hook(lambda m, keys: m._packed.clear())

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * int(np.prod(self.kernel_size))
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def geometry(self):
        """(ksize, stride, pad) as the kernels use them: SubM forces stride 1 / pad k//2 (spconv 1.0)."""
        if self.subm:
            return self.kernel_size, [1, 1, 1], [k // 2 for k in self.kernel_size]
        return self.kernel_size, self.stride, self.padding

    def packed_weight(self, dtype, bn=None):
        """Fragment-ordered weights (+ fp32 bias) with the eval-mode BatchNorm ``bn`` that follows the conv folded
        in; channel counts are padded to multiples of 16.  Cached per (dtype, bn, device) and re-derived whenever one
        of the source tensors changed (their ``_version`` counters: load_state_dict, init, optimizer step, BN statistics)."""
        key = (dtype, id(bn), self.weight.device)
        ver = self.weight._version + (self.bias._version if self.bias is not None else 0)
        if bn is not None:
            ver += bn.weight._version + bn.bias._version + bn.running_mean._version + bn.running_var._version
        hit = self._packed.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        K = int(np.prod(self.kernel_size))
        w = self.weight.detach().float().reshape(K, self.in_channels, self.out_channels)
        b = self.bias.detach().float() if self.bias is not None else None
        if bn is not None:
            from .nn_utils import fold_bn

            w, b = fold_bn(w, b, bn, 2)
        cin_p, cout_p = pad_channels(self.in_channels), pad_channels(self.out_channels)
        wp = torch.zeros((K, cin_p, cout_p), dtype=torch.float32, device=w.device)
        wp[:, : self.in_channels, : self.out_channels] = w
        bp = None
        if b is not None:
            bp = torch.zeros((cout_p,), dtype=torch.float32, device=w.device)
            bp[: self.out_channels] = b
            bp = bp.contiguous()
        packed = (hip_ops.pack_spconv_weight(wp, dtype), bp, cin_p, cout_p)
        self._packed[key] = (ver, packed)
        return packed

    def rulebook_for(self, x, fp32_layer=None):
        """(output index, rulebook) of this convolution on ``x``, shared under the indice_key.  ``fp32_layer``: see SparseIndex.rulebook."""
        data = x.find_indice_pair(self.indice_key)
        if data is not None:
            return data
        ks, st, pd = self.geometry()
        if self.subm:
            out_index = x.index
        else:
            out_index = x.index.downsample(ks, st, pd)
            n_dev = torch.zeros((1,), dtype=torch.int32, device=x.features.device)
            out_index.scan(n_dev)
            out_index.finalize(int(n_dev.cpu()[0]))
        nbr = x.index.rulebook(out_index, ks, st, pd, fp32_layer=fp32_layer)
        data = (out_index, nbr)
        if self.indice_key is not None:
            x.indice_dict[self.indice_key] = data
        return data

    def forward(self, x):
        assert isinstance(x, SparseConvTensor)
        params = [self.weight] + ([self.bias] if self.bias is not None else [])
        if torch.is_grad_enabled() and (x.features.requires_grad or (self.training and any(p.requires_grad for p in params))):
            return self._forward_autograd(x, *self.rulebook_for(x))
        # an fp32 eval-mode launch: where its kernel reads a chunk plan the plan comes straight from the index, no table is built
        layer = (pad_channels(self.in_channels), pad_channels(self.out_channels)) if x.features.dtype == torch.float32 and not self.training else None
        out_index, nbr = self.rulebook_for(x, fp32_layer=layer)
        feats = x.features
        if feats.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError("sparse convolution takes fp32 or bf16 features (features are %s)" % feats.dtype)
        wpk, bias, cin_p, cout_p = self.packed_weight(feats.dtype)  # the kernel's dtype is the rows': bf16 rows meet a frozen convolution in mixed-precision training
        if feats.shape[1] != cin_p:
            feats = torch.nn.functional.pad(feats, (0, cin_p - feats.shape[1]))
        out = hip_ops.spconv_apply(feats.contiguous(), wpk, bias, nbr, out_index.n, cout_p)
        if cout_p != self.out_channels:
            out = out[:, : self.out_channels].contiguous()
        y = SparseConvTensor(out, None, out_index.spatial_shape, x.batch_size, grid=x.grid, _index=out_index)
        y.indice_dict = x.indice_dict
        return y


    def _forward_autograd(self, x, out_index, nbr):
        """The differentiable path (fp32 rows, or bf16 rows with fp32 parameters): padding and slicing are torch ops around
        _SparseConvFunction."""
        if x.features.dtype not in (torch.float32, torch.bfloat16):
            raise NotImplementedError("sparse convolution training takes fp32 or bf16 features (features are %s)" % x.features.dtype)
        if isinstance(nbr, hip_ops.IndexRulebook):  # (shared under the indice_key by an eval-mode launch: the gradients read the table)
            nbr = nbr.table()
        K = int(np.prod(self.kernel_size))
        cin_p, cout_p = pad_channels(self.in_channels), pad_channels(self.out_channels)
        F = torch.nn.functional
        w = F.pad(self.weight.float().reshape(K, self.in_channels, self.out_channels),
                  (0, cout_p - self.out_channels, 0, cin_p - self.in_channels)).contiguous()
        b = F.pad(self.bias.float(), (0, cout_p - self.out_channels)).contiguous() if self.bias is not None else None
        feats = x.features
        if feats.shape[1] != cin_p:
            feats = F.pad(feats, (0, cin_p - feats.shape[1]))
        out = _SparseConvFunction.apply(feats.contiguous(), w, b, nbr, out_index.n, self.subm)
        if cout_p != self.out_channels:
            out = out[:, : self.out_channels]
        y = SparseConvTensor(out, None, out_index.spatial_shape, x.batch_size, grid=x.grid, _index=out_index)
        y.indice_dict = x.indice_dict
        return y


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias,
                         indice_key=indice_key)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(3, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, subm=True,
                         indice_key=indice_key)


class SparseSequential(SparseModule):
    """SparseModules see the tensor, plain modules see ``.features`` (spconv 1.0 modules.py)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for i, m in enumerate(args):
            self.add_module(str(i), m)
        for k, m in kwargs.items():
            self.add_module(k, m)

    def __getitem__(self, idx):
        return list(self._modules.values())[idx]

    def __len__(self):
        return len(self._modules)

    def add(self, module, name=None):
        self.add_module(str(len(self._modules)) if name is None else name, module)

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                if x.features.shape[0] != 0:
                    x.features = m(x.features)
            else:
                x = m(x)
        return x
