"""Readers (det3d/models/readers).  VoxelFeatureExtractorV3: per-voxel mean of the point slots.  PillarFeatureNet: the PointPillars
reader on fd_pillar_encode (eval) and fd_pillar_train_forward / _backward (train)."""
import torch
from torch import nn

from . import hip_ops
from .nn_utils import bn_affine, build_norm_layer, weights_version
from .registry import READERS


@READERS.register_module
class VoxelFeatureExtractorV3(nn.Module):
    """det3d/models/readers/voxel_encoder.py:8-24.  When the voxelizer already produced means (fused kernel),
    ``features`` arrives as [M, C] and is passed through."""

    def __init__(self, num_input_features=4, norm_cfg=None, name="VoxelFeatureExtractorV3"):
        super().__init__()
        self.name = name
        self.num_input_features = num_input_features

    def forward(self, features, num_voxels, coors=None):
        assert self.num_input_features == features.shape[-1]
        if features.dim() == 2:  # fused voxelizer output: already the mean
            return features
        points_mean = features[:, :, : self.num_input_features].sum(dim=1, keepdim=False) / \
            num_voxels.type_as(features).view(-1, 1)
        return points_mean.contiguous()


class PFNLayer(nn.Module):
    """Parameter holder with the state_dict keys of det3d/models/readers/pillar_encoder.py:15-55 (linear.weight,
    norm.*).  The layer itself (Linear, BatchNorm, ReLU, max over the pillar's points, concat) is evaluated inside
    fd_pillar_encode (eval) or fd_pillar_train_forward / _backward (train); there is no per-layer torch forward."""

    def __init__(self, in_channels, out_channels, norm_cfg=None, last_layer=False):
        super().__init__()
        self.name = "PFNLayer"
        self.last_vfe = last_layer
        if not self.last_vfe:
            out_channels = out_channels // 2
        self.units = out_channels
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        self.norm_cfg = norm_cfg
        self.linear = nn.Linear(in_channels, self.units, bias=False)
        self.norm = build_norm_layer(self.norm_cfg, self.units)[1]


@READERS.register_module
class PillarFeatureNet(nn.Module):
    """det3d/models/readers/pillar_encoder.py:58-164.  In eval mode on the GPU the whole reader is one HIP launch
    (fd_pillar_encode) with BatchNorm folded from the running statistics.  In training mode (the shipped stack, two PFN layers
    32 -> 64, fp32) it runs on fd_pillar_train_forward / fd_pillar_train_backward: BatchNorm on batch statistics over every
    point slot of the batch, gradients for both layers' Linear and BatchNorm parameters, and the running statistics updated
    in place with the BatchNorm modules' own momentum.  ``forward_train_static`` is the same training form for a fixed-capacity batch
    whose pillar counts stay on the device (fd_pillar_train_forward_dev / _backward_dev / _running_stats_dev): no host read, the same
    bits.  The torch modules only define the parameters / state_dict."""

    def __init__(self, num_input_features=4, num_filters=(64,), with_distance=False, voxel_size=(0.2, 0.2, 4),
                 pc_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None):
        super().__init__()
        self.name = "PillarFeatureNet"
        assert len(num_filters) > 0
        self.num_input = num_input_features
        num_input_features += 5
        if with_distance:
            num_input_features += 1
        self._with_distance = with_distance
        num_filters = [num_input_features] + list(num_filters)
        self.pfn_layers = nn.ModuleList([
            PFNLayer(num_filters[i], num_filters[i + 1], norm_cfg=norm_cfg, last_layer=(i >= len(num_filters) - 2))
            for i in range(len(num_filters) - 1)])
        self.vx = voxel_size[0]
        self.vy = voxel_size[1]
        self.x_offset = self.vx / 2 + pc_range[0]
        self.y_offset = self.vy / 2 + pc_range[1]
        self.compute_dtype = torch.float32
        self._packed = None
        self.register_load_state_dict_post_hook(_drop_packed)

    def _layers(self, device):
        key = (device, weights_version(self))
        if self._packed is None or self._packed[0] != key:
            if len(self.pfn_layers) > 2:
                raise NotImplementedError("fd_pillar_encode fuses one or two PFN layers (shipped configs: [64, 64])")
            layers = []
            for pfn in self.pfn_layers:
                scale, shift = bn_affine(pfn.norm)
                layers.append((pfn.linear.weight.detach().float().contiguous().to(device), scale.contiguous().to(device),
                               shift.contiguous().to(device)))
            self._packed = (key, layers)
        return self._packed[1]

    def forward(self, features, num_voxels, coors, n_dev=None):
        if self.training:
            return self._forward_train(features, num_voxels, coors)
        return hip_ops.pillar_encode(features, num_voxels.int(), coors.int().contiguous(), n_dev,
                                     (self.vx, self.vy, self.x_offset, self.y_offset), self._layers(features.device),
                                     with_distance=self._with_distance, out_dtype=self.compute_dtype)


    def _train_spec(self):
        """what both training forms check and hand to the kernels: (layer 1, layer 2, (geometry, eps1, eps2, with_distance))"""
        if self.compute_dtype != torch.float32:
            raise NotImplementedError("PillarFeatureNet: training runs in fp32 only; the %s reader is inference-only (set compute_dtype = "
                                      "torch.float32 to train)" % self.compute_dtype)
        units = [pfn.units for pfn in self.pfn_layers]
        if units != [32, 64]:
            raise NotImplementedError("PillarFeatureNet: training supports the shipped PFN stack num_filters=[64, 64] (units 32 -> 64, "
                                      "fd_pillar_train_forward), not units %s" % units)
        l1, l2 = self.pfn_layers
        geom = (self.vx, self.vy, self.x_offset, self.y_offset)
        return l1, l2, (geom, l1.norm.eps, l2.norm.eps, self._with_distance)

    def _forward_train(self, features, num_voxels, coors):
        l1, l2, spec = self._train_spec()
        n1, n2 = l1.norm, l2.norm
        voxels = features.float().contiguous()
        out, stats = _PillarTrain.apply(voxels, num_voxels.int().contiguous(), coors.int().contiguous(), l1.linear.weight.contiguous(),
                                        n1.weight.contiguous(), n1.bias.contiguous(), l2.linear.weight.contiguous(), n2.weight.contiguous(),
                                        n2.bias.contiguous(), spec)
        n = voxels.shape[0] * voxels.shape[1]
        with torch.no_grad():
            u1 = n1.num_features
            for bn, mean, var in ((n1, stats[:u1], stats[u1:2 * u1]), (n2, stats[2 * u1:2 * u1 + n2.num_features], stats[2 * u1 + n2.num_features:])):
                _update_running_stats(bn, mean, var, n)
        return out

    def forward_train_static(self, features, num_voxels, coors, counts):
        """The training form with the pillar counts on the device, one call for the whole batch: features [B, cap, P, ndim],
        num_voxels [B, cap], coors [B, cap, 4], counts int32[B] on the device (sample b's pillars are its first counts[b] rows; the
        rows behind may hold anything).  Returns [B * cap, 64] with zeros behind the counts -- on the live rows, and in every gradient
        and batch statistic, the bits of ``forward`` on the compacted pillars -- and updates the running statistics on the device
        (fd_pillar_train_running_stats_dev).  Nothing waits for the device."""
        l1, l2, spec = self._train_spec()
        n1, n2 = l1.norm, l2.norm
        for bn in (n1, n2):
            if bn.track_running_stats and bn.running_mean is not None and bn.momentum is None:
                raise NotImplementedError("PillarFeatureNet.forward_train_static: momentum=None (cumulative average) needs "
                                          "num_batches_tracked on the host; set a momentum (every shipped norm_cfg has 0.01)")
        if features.dim() != 4 or counts.dim() != 1 or counts.shape[0] != features.shape[0]:
            raise ValueError("forward_train_static: features [B, cap, P, ndim] with counts [B], got %s and %s"
                             % (tuple(features.shape), tuple(counts.shape)))
        cap, P = features.shape[1], features.shape[2]
        out, stats = _PillarTrainStatic.apply(features.float().contiguous(), num_voxels.int().contiguous(), coors.int().contiguous(),
                                              counts.int().contiguous(), l1.linear.weight.contiguous(), n1.weight.contiguous(),
                                              n1.bias.contiguous(), l2.linear.weight.contiguous(), n2.weight.contiguous(),
                                              n2.bias.contiguous(), spec)
        u1, u2 = n1.num_features, n2.num_features
        for bn, mean, var in ((n1, stats[:u1], stats[u1:2 * u1]), (n2, stats[2 * u1:2 * u1 + u2], stats[2 * u1 + u2:])):
            if bn.track_running_stats and bn.running_mean is not None:
                hip_ops.pillar_train_running_stats_dev(mean, var, bn.momentum, counts, cap, P, bn.running_mean, bn.running_var,
                                                       bn.num_batches_tracked)
        return out


def _update_running_stats(bn, mean, var, n):
    """torch's BatchNorm rule, as in-place ops on the module's buffers (so weights_version sees them): num_batches_tracked += 1,
    running_mean <- (1 - f) running_mean + f mean, running_var <- (1 - f) running_var + f var * n / (n - 1), f = momentum, or
    1 / num_batches_tracked (cumulative average) when momentum is None."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    bn.num_batches_tracked.add_(1)
    f = (1.0 / float(bn.num_batches_tracked)) if bn.momentum is None else bn.momentum
    bn.running_mean.mul_(1.0 - f).add_(mean, alpha=f)
    bn.running_var.mul_(1.0 - f).add_(var, alpha=f * n / (n - 1))


class _PillarTrain(torch.autograd.Function):
    """The train-mode reader over fd_pillar_train_forward / _backward.  Returns (out [M, 64], stats [192] = mean1, var1, mean2,
    var2 with biased variances); the stats carry no gradient."""

    @staticmethod
    def forward(ctx, voxels, num_points, coors4, w1, g1, b1, w2, g2, b2, spec):
        geom, eps1, eps2, wd = spec
        out, mean1, var1, mean2, var2, ws = hip_ops.pillar_train_forward(voxels, num_points, coors4, geom, w1, g1, b1, eps1, w2, g2, b2,
                                                                         eps2, with_distance=wd)
        stats = torch.cat([mean1, var1, mean2, var2])
        ctx.inputs = (voxels, num_points, coors4, w1, g1, b1, w2, g2, b2)
        ctx.ws = ws
        ctx.spec = spec
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, dstats):
        voxels, num_points, coors4, w1, g1, b1, w2, g2, b2 = ctx.inputs
        geom, _, _, wd = ctx.spec
        if dout is None:
            dout = torch.zeros((voxels.shape[0], w2.shape[0]), dtype=torch.float32, device=voxels.device)
        grads = hip_ops.pillar_train_backward(dout.float().contiguous(), voxels, num_points, coors4, geom, w1, g1, b1, w2, g2, b2, ctx.ws,
                                              with_distance=wd)
        ctx.inputs = ctx.ws = None
        return (None, None, None) + tuple(grads) + (None,)


class _PillarTrainStatic(torch.autograd.Function):
    """_PillarTrain over fd_pillar_train_forward_dev / _backward_dev: inputs [B, cap, ...] with the pillar counts [B] on the device.
    Returns (out [B * cap, 64], stats [192])."""

    @staticmethod
    def forward(ctx, voxels, num_points, coors4, counts, w1, g1, b1, w2, g2, b2, spec):
        geom, eps1, eps2, wd = spec
        out, mean1, var1, mean2, var2, ws = hip_ops.pillar_train_forward_dev(voxels, num_points, coors4, counts, geom, w1, g1, b1, eps1,
                                                                             w2, g2, b2, eps2, with_distance=wd)
        stats = torch.cat([mean1, var1, mean2, var2])
        ctx.inputs = (voxels, num_points, coors4, counts, w1, g1, b1, w2, g2, b2)
        ctx.ws = ws
        ctx.spec = spec
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, dstats):
        voxels, num_points, coors4, counts, w1, g1, b1, w2, g2, b2 = ctx.inputs
        geom, _, _, wd = ctx.spec
        if dout is None:
            dout = torch.zeros((voxels.shape[0] * voxels.shape[1], w2.shape[0]), dtype=torch.float32, device=voxels.device)
        grads = hip_ops.pillar_train_backward_dev(dout.float().contiguous(), voxels, num_points, coors4, counts, geom, w1, g1, b1, w2, g2,
                                                  b2, ctx.ws, with_distance=wd)
        ctx.inputs = ctx.ws = None
        return (None, None, None, None) + tuple(grads) + (None,)


def _drop_packed(module, incompatible_keys=None):
    module._packed = None
    module.__dict__.pop("_wv_tensors", None)
