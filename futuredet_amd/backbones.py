"""SpMiddleResNetFHD (det3d/models/backbones/scn.py:37-176) on the HIP sparse-conv kernels.

Module / parameter names reproduce the reference so checkpoints load unchanged
(conv_input.0.weight [3,3,3,5,16], conv1.0.conv1.{weight,bias}, conv1.0.bn1.*, conv2.0.weight, ...).
Two execution paths, both on the HIP kernels:
  * generic: the spconv-surface modules one by one (SparseSequential / SparseBasicBlock.forward), used in
    training mode or when a caller drives sub-modules directly; ``train_dtype = torch.bfloat16`` runs it with bf16 rows
    (mixed precision: fp32 parameters, gradients and BatchNorm statistics);
  * fused (eval): all five sparse indexes are built first (one host read of the five active counts), every
    conv runs as one fd_spconv_apply launch with BatchNorm1d folded into weight/bias and ReLU / residual
    fused in the epilogue, features stay channel-padded and in index order, then fd_densify.
"""
import numpy as np
import torch
from torch import nn

from . import hip_ops, sparse as spconv
from .nn_utils import build_norm_layer
from .registry import BACKBONES
from .sparse import SparseConv3d, SubMConv3d


def conv3x3(in_planes, out_planes, stride=1, indice_key=None, bias=True):
    return spconv.SubMConv3d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=bias,
                             indice_key=indice_key)


class SparseBasicBlock(spconv.SparseModule):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_cfg=None, downsample=None, indice_key=None):
        super().__init__()
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        bias = norm_cfg is not None  # scn.py:54 -- always True, so block convs carry a bias
        self.conv1 = conv3x3(inplanes, planes, stride, indice_key=indice_key, bias=bias)
        self.bn1 = build_norm_layer(norm_cfg, planes)[1]
        self.relu = nn.ReLU()
        self.conv2 = conv3x3(planes, planes, indice_key=indice_key, bias=bias)
        self.bn2 = build_norm_layer(norm_cfg, planes)[1]
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.conv1(x)
        out.features = self.relu(self.bn1(out.features))
        out = self.conv2(out)
        out.features = self.bn2(out.features)
        if self.downsample is not None:
            identity = self.downsample(x)
        out.features = self.relu(out.features + identity.features)
        return out

    def forward_fused_bn(self, x, bn_act):
        """forward with bn1 + relu and bn2 + identity + relu each handed to ``bn_act(features, bn, relu module, residual)``"""
        out = self.conv1(x)
        out.features = bn_act(out.features, self.bn1, self.relu)
        out = self.conv2(out)
        identity = x if self.downsample is None else self.downsample(x)
        out.features = bn_act(out.features, self.bn2, self.relu, identity.features)
        return out


@BACKBONES.register_module
class SpMiddleResNetFHD(nn.Module):
    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleResNetFHD", **kwargs):
        super().__init__()
        self.name = name
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        S = spconv.SparseSequential
        self.conv_input = S(SubMConv3d(num_input_features, 16, 3, bias=False, indice_key="res0"),
                            build_norm_layer(norm_cfg, 16)[1], nn.ReLU(inplace=True))
        self.conv1 = S(SparseBasicBlock(16, 16, norm_cfg=norm_cfg, indice_key="res0"),
                       SparseBasicBlock(16, 16, norm_cfg=norm_cfg, indice_key="res0"))
        self.conv2 = S(SparseConv3d(16, 32, 3, 2, padding=1, bias=False), build_norm_layer(norm_cfg, 32)[1],
                       nn.ReLU(inplace=True), SparseBasicBlock(32, 32, norm_cfg=norm_cfg, indice_key="res1"),
                       SparseBasicBlock(32, 32, norm_cfg=norm_cfg, indice_key="res1"))
        self.conv3 = S(SparseConv3d(32, 64, 3, 2, padding=1, bias=False), build_norm_layer(norm_cfg, 64)[1],
                       nn.ReLU(inplace=True), SparseBasicBlock(64, 64, norm_cfg=norm_cfg, indice_key="res2"),
                       SparseBasicBlock(64, 64, norm_cfg=norm_cfg, indice_key="res2"))
        self.conv4 = S(SparseConv3d(64, 128, 3, 2, padding=[0, 1, 1], bias=False), build_norm_layer(norm_cfg, 128)[1],
                       nn.ReLU(inplace=True), SparseBasicBlock(128, 128, norm_cfg=norm_cfg, indice_key="res3"),
                       SparseBasicBlock(128, 128, norm_cfg=norm_cfg, indice_key="res3"))
        self.extra_conv = S(SparseConv3d(128, 128, (3, 1, 1), (2, 1, 1), bias=False), build_norm_layer(norm_cfg, 128)[1],
                            nn.ReLU())
        self.compute_dtype = torch.float32   # torch.bfloat16 selects the bf16 MFMA path (fp32 accumulate)
        self.dense_channels_last = True
        self.dense_dtype = None              # dtype of the BEV map handed to the neck (default: compute dtype)
        self.profile_hook = None             # callable(tag, algorithmic_bytes, flops, fn) used by bench.py
        self.fused_bn = False                # training: BatchNorm1d (+ residual) + ReLU on the fused kernels (sparse.batch_norm_act),
                                             # on fp32 rows and on the bf16 rows of train_dtype = torch.bfloat16
        self.train_dtype = torch.float32     # training: dtype of the feature rows; torch.bfloat16 = mixed precision (fp32 parameters,
                                             # gradients and BatchNorm statistics).  compute_dtype keeps meaning the eval path

    # ------------------------------------------------------------------------------------------------ generic
    def _bn_act(self, features, bn, relu, residual=None):
        """relu(bn(features) [+ residual]): with fused_bn the fused kernels where they apply (fp32 rows, and the bf16 rows of mixed
        precision), else the modules as SparseSequential / SparseBasicBlock call them (CPU, double, eval, no_grad, affine=False,
        track_running_stats=False, momentum=None, fewer than 2 rows).  Without fused_bn the modules always: mixed precision reaches
        this method with the switch off."""
        if self.fused_bn and spconv.batch_norm_fusable(features, bn):
            return spconv.batch_norm_act(features, bn, residual=residual, relu=True)
        if features.dtype == torch.bfloat16:  # mixed precision: normalise, add and rectify in fp32 (fp32 batch and running statistics), one rounding
            out = bn(features.float())
            if residual is not None:
                out = out + residual.float()
            return spconv.relu_to_bf16(out)  # (saves the bf16 rows only: 6 bytes per element and layer stay alive for backward, against fp32's 8)
        out = bn(features)
        if residual is not None:
            out = out + residual
        return relu(out)

    def _run_stage(self, seq, x):
        """SparseSequential.forward with every BatchNorm1d + ReLU pair and every block's normalisation chain through _bn_act"""
        mods = list(seq._modules.values())
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, SparseBasicBlock):
                x = m.forward_fused_bn(x, self._bn_act)
            elif isinstance(m, spconv.SparseModule):
                x = m(x)
            elif x.features.shape[0] != 0:
                if isinstance(m, nn.BatchNorm1d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
                    x.features = self._bn_act(x.features, m, mods[i + 1])
                    i += 1
                else:
                    x.features = m(x.features)
            i += 1
        return x

    def forward_generic(self, voxel_features, coors, batch_size, input_shape):
        sparse_shape = np.array(input_shape[::-1]) + [1, 0, 0]  # scn.py:151
        ret = spconv.SparseConvTensor(voxel_features, coors.int(), sparse_shape, batch_size)
        stages = (self.conv_input, self.conv1, self.conv2, self.conv3, self.conv4, self.extra_conv)
        mixed = self.train_dtype == torch.bfloat16 and self.training and torch.is_grad_enabled()
        if mixed:  # the rows are bf16 from here to the BEV map; every stage through _run_stage, whose _bn_act normalises them with fp32 statistics
            ret.features = ret.features.to(torch.bfloat16)
        if mixed or (self.fused_bn and self.training and torch.is_grad_enabled()):
            run = [lambda x, seq=seq: self._run_stage(seq, x) for seq in stages]
        else:
            run = stages
        x = run[0](ret)
        x_conv1 = run[1](x)
        x_conv2 = run[2](x_conv1)
        x_conv3 = run[3](x_conv2)
        x_conv4 = run[4](x_conv3)
        ret = run[5](x_conv4).dense()
        if mixed:
            ret = ret.float()  # the neck trains in fp32
        N, C, D, H, W = ret.shape
        ret = ret.view(N, C * D, H, W)
        return ret, {"conv1": x_conv1, "conv2": x_conv2, "conv3": x_conv3, "conv4": x_conv4}

    # ------------------------------------------------------------------------------------------------ fused
    def _stages(self):
        """[(strided conv or None, its bn), [blocks]] per level, in execution order."""
        return [(self.conv_input[0], self.conv_input[1], [self.conv1[0], self.conv1[1]], True),
                (self.conv2[0], self.conv2[1], [self.conv2[3], self.conv2[4]], False),
                (self.conv3[0], self.conv3[1], [self.conv3[3], self.conv3[4]], False),
                (self.conv4[0], self.conv4[1], [self.conv4[3], self.conv4[4]], False),
                (self.extra_conv[0], self.extra_conv[1], [], False)]

    def build_indexes(self, mark_fn, batch_size, input_shape, device, voxels=None, static=False, expected=None, row_caps=None):
        """Builds the five sparse indexes.  ``mark_fn(index0)`` marks the input voxels.  One host read.  With
        ``voxels = (coors [B*n_max,4], nvox [B], n_max)`` the whole pyramid is built by two library calls; with
        ``static=True`` there is no host read at all: every level is sized by its row capacity and the counts stay on the
        device (hip_ops.build_pyramid)."""
        D, H, W = [int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0])]
        if voxels is not None:
            geoms = [self._stages()[lvl][0].geometry() for lvl in range(1, 5)]
            return hip_ops.build_pyramid(voxels[0], voxels[1], voxels[2], batch_size, (D, H, W), geoms, device, static=static,
                                         expected=expected, row_caps=row_caps)
        assert not static, "static indexes are built from the voxelizer's device output (voxels=...)"
        counts = torch.zeros((5,), dtype=torch.int32, device=device)
        idx = [hip_ops.SparseIndex(batch_size, D, H, W, device)]
        mark_fn(idx[0])
        idx[0].scan(counts[0:1])
        for lvl in range(1, 5):
            conv = self._stages()[lvl][0]
            ks, st, pd = conv.geometry()
            nxt = idx[-1].downsample(ks, st, pd)
            nxt.scan(counts[lvl:lvl + 1])
            idx.append(nxt)
        host = counts.cpu()  # the only synchronisation of the backbone
        for i, ix in enumerate(idx):
            ix.finalize(int(host[i]))
        return idx

    def run_fused(self, idx, feats0, dense_out=None, fork=False):
        """feats0: [n0, 16] features already in index order (channel padded).  Returns (dense BEV, per-level
        (features, index)).  ``fork``: the rulebooks (and work-range tables) of levels 1-4 only need the indexes, not the features:
        they are built on a side stream while the first level's convolutions run (inside a captured sweep this forks the graph;
        a sweep's latency loses ~0.1 ms of front-end kernels that used to sit between the convolutions)."""
        dt = self.compute_dtype
        stages = self._stages()
        rb_cache = {}

        # fp32 sweep: the K = 27 layers of levels 1-3 run on chunk plans made straight from the index (hip_ops.IndexRulebook) and
        # their dense tables are never built -- unless a profile hook asks for a launch's pair count, which is counted on the table
        from_index = dt == torch.float32

        def rulebook(src, dst, conv):
            ks, st, pd = conv.geometry()
            key = (id(src), id(dst), tuple(ks), tuple(st), tuple(pd))
            if key not in rb_cache:
                layer = (spconv.pad_channels(conv.in_channels), spconv.pad_channels(conv.out_channels)) if from_index else None
                rb_cache[key] = src.rulebook(dst, ks, st, pd, fp32_layer=layer)
            return rb_cache[key]

        def run(conv, bn, x, src, dst, relu, residual=None, layout=0):
            wpk, bias, cin_p, cout_p = conv.packed_weight(dt, bn)
            assert x.shape[1] == cin_p, (x.shape, cin_p)
            nbr = rulebook(src, dst, conv)
            fn = lambda: hip_ops.spconv_apply(x, wpk, bias, nbr, dst.n, cout_p, residual=residual, relu=relu, layout=layout)  # noqa: E731
            if self.profile_hook is not None:
                s = 4 if dt == torch.float32 else 2
                K = nbr.shape[0]
                table = lambda: nbr.table() if isinstance(nbr, hip_ops.IndexRulebook) else nbr  # noqa: E731
                pairs = lambda: int((table()[:, : dst.n] >= 0).sum().item())  # noqa: E731
                return self.profile_hook("spconv_%dx%d_K%d" % (cin_p, cout_p, K),
                                         dict(s=s, K=K, cin=cin_p, cout=cout_p, n_in=src.n, n_out=dst.n, pairs=pairs), fn)
            return fn()

        def index_plans():
            """The chunk plans of the sweep's index rulebooks, ahead of their first use: one launch for those whose row split is known
            up front (the strided layers, the 32-channel level), the equal-work range tables of the wide levels, one launch for their
            plans -- the tables of a launch overlap their load chains.  Returns the tensors made (cached on the rulebooks)."""
            groups = ([], [])  # (row split known up front, equal-work ranges first)
            for lvl, (conv, bn, blocks, is_subm_in) in enumerate(stages):
                if lvl == 0:
                    continue
                src_l, dst_l = (idx[lvl] if is_subm_in else idx[lvl - 1]), idx[lvl]
                for s_l, cv in [(src_l, conv)] + [(dst_l, b.conv1) for b in blocks[:1]]:  # (a level's blocks share one rulebook)
                    nbr = rulebook(s_l, dst_l, cv)
                    if isinstance(nbr, hip_ops.IndexRulebook):
                        ci, co = spconv.pad_channels(cv.in_channels), spconv.pad_channels(cv.out_channels)
                        groups[int(ci == co and bool(hip_ops._lib.load().fd_spconv_wants_balanced_ranges(ci, co, 0)))].append((nbr, ci, co))
            made = []
            for group in groups:
                splits = [(rb,) + tuple(hip_ops.row_split(rb, rb.n_out, ci, co)) for rb, ci, co in group]
                made += [r for _, r, _ in splits if r is not None]
                made += hip_ops.plans_from_index(splits)
            return made

        main, side = None, None
        if fork and feats0.is_cuda:
            main = torch.cuda.current_stream(feats0.device)
            pool = self.__dict__.setdefault("_side_streams", {})
            side = pool.get(main.cuda_stream)
            if side is None:  # one side stream per launch stream: sweeps in flight on different streams fork independently
                side = pool[main.cuda_stream] = torch.cuda.Stream(device=feats0.device)
            side.wait_stream(main)  # the indexes are complete
            with torch.cuda.stream(side):
                made = []
                for lvl, (conv, bn, blocks, is_subm_in) in enumerate(stages):
                    if lvl == 0:
                        continue
                    src_l, dst_l = (idx[lvl] if is_subm_in else idx[lvl - 1]), idx[lvl]
                    nbr = rulebook(src_l, dst_l, conv)
                    if not isinstance(nbr, hip_ops.IndexRulebook):
                        made.append(nbr)
                    for blk in blocks:
                        nbr = rulebook(dst_l, dst_l, blk.conv1)
                        if isinstance(nbr, hip_ops.IndexRulebook):
                            continue
                        made.append(nbr)
                        cp = spconv.pad_channels(blk.conv1.out_channels)
                        if dt == torch.float32 and nbr.shape[0] == 27 and \
                                hip_ops._lib.load().fd_spconv_wants_balanced_ranges(cp, cp, 0):
                            r = hip_ops.ranges_for(nbr, cp, cp)  # cached on the rulebook tensor; spconv_apply finds it there
                            if r[0] is not None:
                                made.append(r[0])
                        if dt == torch.float32 and nbr.shape[0] == 27 and dst_l.n > 0 and \
                                hip_ops._lib.load().fd_spconv_plan_wanted(cp, cp, 0):
                            # the level's chunk plan, for the row split its convolutions will ask for (cached on the rulebook tensor)
                            made.append(hip_ops.plan_for(nbr, dst_l.n, *hip_ops.row_split(nbr, dst_l.n, cp, cp))[0])
                made += index_plans()
                for t in made:  # allocated on the side stream, consumed by kernels of the main stream
                    t.record_stream(main)
        elif from_index:
            index_plans()
        x = feats0
        levels = {}
        for lvl, (conv, bn, blocks, is_subm_in) in enumerate(stages):
            src = idx[lvl] if is_subm_in else idx[lvl - 1]
            dst = idx[lvl]
            if lvl == 1 and side is not None:
                main.wait_stream(side)  # join: the first level's convolutions are issued, the other levels' rulebooks are needed now
            # The tensors between the strided convolution into a level and the level's last convolution are read by these launches alone:
            # on the fp32 plan route they are stored bank-spread (fd_spconv_apply_layout: 1 input, 2 residual, 4 output), so that their
            # gathers do not queue on one bank.  The level's last output -- levels[lvl], the next strided layer, densify -- stays plain.
            swz = from_index and lvl >= 1 and len(blocks) > 0 and hip_ops.level_layout(
                spconv.pad_channels(conv.in_channels), spconv.pad_channels(conv.out_channels), src.n, dst.n)
            x = run(conv, bn, x, src, dst, relu=True, layout=4 if swz else 0)
            for i, blk in enumerate(blocks):
                y = run(blk.conv1, blk.bn1, x, dst, dst, relu=True, layout=5 if swz else 0)
                last = i + 1 == len(blocks)
                x = run(blk.conv2, blk.bn2, y, dst, dst, relu=True, residual=x, layout=(3 if last else 7) if swz else 0)
            levels[lvl] = (x, dst)
        bev = hip_ops.densify(x, idx[4], out_dtype=self.dense_dtype or dt, channels_last=self.dense_channels_last, out=dense_out)
        return bev, levels

    def forward_static_train(self, feats0, idx):
        """The train-mode walk of _stages() over a finished index pyramid (hip_ops.build_pyramid): what forward_generic computes, with
        no host read.  ``feats0`` [idx[0].n, 16]: the level-0 rows in index order, channel padded (fp32, or already ``train_dtype``);
        ``idx``: the five indexes.  With static indexes (``static=True, row_caps=...``) every ``idx[l].n`` is a row CAPACITY and every
        kernel -- convolutions, weight and bias gradients, BatchNorm in both directions, densify's backward -- takes the level's count
        from the device; with host-sized indexes the calls are forward_generic's own.  The same autograd functions either way, so
        the BEV map, the running statistics and the gradients carry the same bits (bias gradients: fd_rows_colsum's summation
        order instead of torch's).  Single stream; the rulebooks are built where they are first used.
        Needs ``fused_bn = True``: the torch BatchNorm chain cannot honour a device count.  Returns the BEV map [B, 128 * D, H, W]."""
        if not self.fused_bn:
            raise ValueError("SpMiddleResNetFHD.forward_static_train needs fused_bn = True: torch's BatchNorm1d cannot take its row count "
                             "from the device (set backbone.fused_bn = True)")
        if not (self.training and torch.is_grad_enabled()):
            raise RuntimeError("SpMiddleResNetFHD.forward_static_train is the training path: call .train() and enable gradients")
        if self.train_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("SpMiddleResNetFHD: train_dtype must be torch.float32 or torch.bfloat16 (got %s)" % (self.train_dtype,))
        B = idx[0].B
        feats = feats0.to(self.train_dtype)
        rulebooks = {}

        def conv(m, x, src, dst):
            ks, st, pd = m.geometry()
            key = (id(src), id(dst), tuple(ks), tuple(st), tuple(pd))  # a level's SubM convolutions share one table, as under an indice_key
            if key not in rulebooks:
                rulebooks[key] = src.rulebook(dst, ks, st, pd)
            return m._forward_autograd(x, dst, rulebooks[key])

        def bn_act(x, bn, dst, residual=None):
            if dst.n < 2 or not spconv.batch_norm_fusable(x.features, bn):
                raise hip_ops.FutureDetHipError("forward_static_train: BatchNorm over %s %s rows cannot run on the fused kernels"
                                                % (tuple(x.features.shape), x.features.dtype))
            x.features = spconv.batch_norm_act(x.features, bn, residual=residual, relu=True, n_dev=dst.n_dev if dst.static else None)
            return x

        x = spconv.SparseConvTensor(feats, None, idx[0].spatial_shape, B, _index=idx[0])
        for lvl, (head, bn, blocks, is_subm_in) in enumerate(self._stages()):
            src, dst = (idx[lvl] if is_subm_in else idx[lvl - 1]), idx[lvl]
            x = bn_act(conv(head, x, src, dst), bn, dst)
            for blk in blocks:
                y = bn_act(conv(blk.conv1, x, dst, dst), blk.bn1, dst)
                x = bn_act(conv(blk.conv2, y, dst, dst), blk.bn2, dst, residual=x.features)
        ret = x.dense()
        if ret.dtype != torch.float32:
            ret = ret.float()  # the neck trains in fp32
        N, C, D, H, W = ret.shape
        return ret.view(N, C * D, H, W)

    def forward(self, voxel_features, coors, batch_size, input_shape):
        if self.training:
            if self.train_dtype not in (torch.float32, torch.bfloat16):
                raise ValueError("SpMiddleResNetFHD: train_dtype must be torch.float32 or torch.bfloat16 (got %s)" % (self.train_dtype,))
            if self.train_dtype == torch.float32 and self.compute_dtype != torch.float32 and torch.is_grad_enabled():
                raise NotImplementedError("SpMiddleResNetFHD: with train_dtype = torch.float32 training runs the fp32 sparse convolution only; "
                                          "compute_dtype = %s selects the inference path (set train_dtype = torch.bfloat16 for mixed-precision "
                                          "training, or compute_dtype = torch.float32)" % self.compute_dtype)
            return self.forward_generic(voxel_features, coors, batch_size, input_shape)
        coors = coors.int().contiguous()
        dev = voxel_features.device
        idx = self.build_indexes(lambda i0: i0.mark(coors), batch_size, input_shape, dev)
        row_of = idx[0].lookup(coors)
        feats0 = hip_ops.rows_permute(voxel_features.float().contiguous(), row_of,
                                      spconv.pad_channels(voxel_features.shape[1]), self.compute_dtype, n_rows=idx[0].n)
        bev, levels = self.run_fused(idx, feats0)
        multi = {}
        for name, lvl, c in (("conv1", 0, 16), ("conv2", 1, 32), ("conv3", 2, 64), ("conv4", 3, 128)):
            f, ix = levels[lvl]
            multi[name] = spconv.SparseConvTensor(f[:, :c], None, ix.spatial_shape, batch_size, _index=ix)
        return bev, multi


@BACKBONES.register_module
class PointPillarsScatter(nn.Module):
    """det3d/models/readers/pillar_encoder.py:167-221: pillar rows -> [B, C, ny, nx] pseudo image (fd_pillar_scatter:
    cell = y*nx + x as in :204-214; written NCHW, or channels-last for the bf16 convolution path)."""

    def __init__(self, num_input_features=64, norm_cfg=None, name="PointPillarsScatter", **kwargs):
        super().__init__()
        self.name = "PointPillarsScatter"
        self.nchannels = num_input_features
        self.dense_channels_last = True

    def forward(self, voxel_features, coords, batch_size, input_shape, n_dev=None):
        self.nx = int(input_shape[0])
        self.ny = int(input_shape[1])
        coords = coords.int().contiguous()
        if n_dev is None and torch.is_grad_enabled() and voxel_features.requires_grad:
            return _ScatterFn.apply(voxel_features, coords, batch_size, self.ny, self.nx, self.dense_channels_last)
        return hip_ops.pillar_scatter(voxel_features, coords, n_dev, batch_size, self.ny, self.nx,
                                      channels_last=self.dense_channels_last)


    def forward_static(self, voxel_features, coords, counts, batch_size, input_shape):
        """The scatter of a fixed-capacity batch: voxel_features [B * cap, C] and coords [B * cap, 4] hold sample b's pillars in the first
        counts[b] (device int32[B]) rows of segment b; the rows behind are not read, and their gradient is 0.  No host read."""
        self.nx = int(input_shape[0])
        self.ny = int(input_shape[1])
        return _ScatterSegFn.apply(voxel_features, coords.int().contiguous(), counts, batch_size, self.ny, self.nx, self.dense_channels_last)


class _ScatterSegFn(torch.autograd.Function):
    """_ScatterFn for B segments with device counts: one fd_pillar_scatter / fd_dense_gather per segment, each with its count pointer."""

    @staticmethod
    def forward(ctx, feats, coords, counts, batch_size, ny, nx, channels_last):
        B = counts.shape[0]
        cap = feats.shape[0] // B
        ctx.coords, ctx.counts, ctx.cap = coords, counts, cap
        canvas = None
        for b in range(B):
            sl = slice(b * cap, (b + 1) * cap)
            canvas = hip_ops.pillar_scatter(feats[sl], coords[sl], counts[b:b + 1], batch_size, ny, nx, channels_last=channels_last,
                                            out=canvas, zero_first=(b == 0))
        return canvas

    @staticmethod
    def backward(ctx, dcanvas):
        coords, counts, cap = ctx.coords, ctx.counts, ctx.cap
        dcanvas = dcanvas.float()
        d = torch.cat([hip_ops.pillar_scatter_backward(dcanvas, coords[b * cap:(b + 1) * cap], n_dev=counts[b:b + 1])
                       for b in range(counts.shape[0])])
        ctx.coords = ctx.counts = None
        return d, None, None, None, None, None, None


class _ScatterFn(torch.autograd.Function):
    """PointPillarsScatter with its backward: d(pillar row) = dcanvas[b, :, y, x] (fd_dense_gather with D = 1, any canvas strides)."""

    @staticmethod
    def forward(ctx, feats, coords, batch_size, ny, nx, channels_last):
        ctx.coords = coords
        return hip_ops.pillar_scatter(feats, coords, None, batch_size, ny, nx, channels_last=channels_last)

    @staticmethod
    def backward(ctx, dcanvas):
        d = hip_ops.pillar_scatter_backward(dcanvas.float(), ctx.coords)
        ctx.coords = None
        return d, None, None, None, None, None
