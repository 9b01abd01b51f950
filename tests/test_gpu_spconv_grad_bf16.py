"""Mixed-precision training of the sparse backbone on the device: bf16 rows, fp32 master weights.  The kernels of fd_spconv_grad_bf16.hip
(weight gradient, device weight packer), the three transposed shapes of the bf16 forward kernels and the autograd / backbone wiring,
against float64 restatements on the bf16-rounded operands.

Bounds.  bf16 x bf16 products are exact in fp32, so a result that is not rounded again (dW, dBias) differs from float64 only by the fp32
accumulation: the fp32 suite's 1e-4 * scale, scale = max(1, max |ref|).  A result that is rounded once to bf16 (y, dX; round to nearest
even, unit roundoff 2^-8 taken generously) gets |got - ref| <= 2^-8 |ref| + 1.01e-4 * scale."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import assert_close, report
from test_gpu_spconv_grad import LAYERS, WGRAD_TABLES

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
U = 2.0 ** -8


def _coords(rng, B, D, H, W, n_per_batch):
    out = []
    for b in range(B):
        cells = rng.choice(D * H * W, n_per_batch, replace=False)
        z, rem = np.divmod(cells, H * W)
        y, x = np.divmod(rem, W)
        out.append(np.stack([np.full_like(z, b), z, y, x], 1))
    return np.concatenate(out).astype(np.int32)


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(name, got, ref, tol=1e-4):
    """element-wise |got - ref| <= tol * scale, scale = max(1, max |ref|): results that are not rounded to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert_close(name, got / scale, ref / scale, tol)


def _close_rounded(name, got, ref):
    """|got - ref| <= 2^-8 |ref| + 1.01e-4 * scale: results rounded once to bf16"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    excess = float(((np.abs(got - ref) - U * np.abs(ref)) / scale).max()) if ref.size else 0.0
    report(name + " (beyond 2^-8 |ref|, / scale)", excess, 1.01e-4)
    assert excess <= 1.01e-4, "%s: |got - ref| - 2^-8 |ref| = %.3e * scale > 1.01e-4 * scale" % (name, excess)


def _dense64(feats, coords, B, shape):
    D, H, W = shape
    x = torch.zeros((B, feats.shape[1], D, H, W), dtype=torch.float64)
    c = torch.from_numpy(coords).long()
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats
    return x


def _bf16_values(rng, shape):
    """uniform (-1, 1), rounded to bf16, as float32"""
    return torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(BF).float()


def _rulebook(rng, B, shape, nvox, ks, st, pd, subm):
    from futuredet_amd import hip_ops

    coords = torch.from_numpy(_coords(rng, B, *shape, nvox)).to(DEV)
    src = hip_ops.SparseIndex(B, *shape, DEV)
    n_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    src.mark(coords)
    src.scan(n_dev)
    src.finalize(int(n_dev.cpu()[0]))
    if subm:
        dst = src
    else:
        dst = src.downsample(ks, st, pd)
        m = torch.zeros(1, dtype=torch.int32, device=DEV)
        dst.scan(m)
        dst.finalize(int(m.cpu()[0]))
    return src, dst, src.rulebook(dst, ks, st, pd)


def _table_reference(x, w, dy, nbr, n_out):
    """float64 gather / index_add on the table: (y without bias, dX, dW) of x [n_in, cin], w [K, cin, cout], dy [n_out, cout] (any may be None)"""
    t = nbr[:, :n_out].long()
    K = t.shape[0]
    y = torch.zeros((n_out, w.shape[2]), dtype=torch.float64, device=t.device) if x is not None and w is not None else None
    dx = torch.zeros((x.shape[0] if x is not None else int(t.max()) + 1, w.shape[1]), dtype=torch.float64, device=t.device) if dy is not None and w is not None else None
    dw = torch.zeros((K, x.shape[1], dy.shape[1]), dtype=torch.float64, device=t.device) if x is not None and dy is not None else None
    for k in range(K):
        o = torch.nonzero(t[k] >= 0)[:, 0]
        i = t[k][o]
        if y is not None:
            y.index_add_(0, o, x[i] @ w[k])
        if dx is not None:
            dx.index_add_(0, i, dy[o] @ w[k].T)
        if dw is not None:
            dw[k] = x[i].T @ dy[o]
    return y, dx, dw


# ------------------------------------------------------------------------------------------------ 1. per layer, against float64
@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "%d-%d_k%s_s%s_p%s" % (l[0], l[1], l[2], l[3], l[4]))
def test_layer_matches_float64_conv3d_on_the_rounded_operands(layer):
    from futuredet_amd import sparse as spconv

    cin, cout, ks, st, pd, subm, bias, shape, nvox = layer
    rng = np.random.default_rng(cin * 1000 + cout + (0 if subm else 7))
    B = 2
    coords = _coords(rng, B, *shape, nvox - 37)  # row counts that are no multiple of any tile
    feats = _bf16_values(rng, (len(coords), cin))
    torch.manual_seed(cin + cout)
    conv = (spconv.SubMConv3d(cin, cout, ks, bias=bias, indice_key="k") if subm else
            spconv.SparseConv3d(cin, cout, ks, st, padding=pd, bias=bias)).to(DEV).train()
    f = feats.to(DEV).requires_grad_(True)
    x = spconv.SparseConvTensor(f, torch.from_numpy(coords).to(DEV), list(shape), B)
    x.features = x.features.to(BF)  # exact: the values are bf16 already
    y = conv(x)
    assert y.features.dtype == BF
    ycoords = y.indices.cpu().numpy()
    G = _bf16_values(rng, (len(ycoords), cout))
    (y.features.float() * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert f.grad.dtype == torch.float32 and conv.weight.grad.dtype == torch.float32

    # float64 reference: dense conv3d on the rounded features and weights, loss on the active output rows only
    x64 = _dense64(feats.double(), coords, B, shape).requires_grad_(True)
    w64 = conv.weight.detach().cpu().to(BF).double().requires_grad_(True)
    b64 = conv.bias.detach().cpu().double().requires_grad_(True) if bias else None
    ks3, st3, pd3 = conv.geometry()
    out = F.conv3d(x64, w64.permute(4, 3, 0, 1, 2), b64, stride=st3, padding=pd3)
    yc = torch.from_numpy(ycoords).long()
    out_rows = out[yc[:, 0], :, yc[:, 1], yc[:, 2], yc[:, 3]]
    tag = "bf16 spconv %d->%d k%s s%s p%s" % (cin, cout, ks, st, pd)
    _close_rounded(tag + " y", _np(y.features), out_rows.detach().numpy())
    (out_rows * G.double()).sum().backward()
    c = torch.from_numpy(coords).long()
    dx_ref = x64.grad[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]
    _close_rounded(tag + " dX", _np(f.grad), dx_ref.numpy())
    _close(tag + " dW", _np(conv.weight.grad), w64.grad.numpy())
    if bias:
        assert conv.bias.grad.dtype == torch.float32
        _close(tag + " dBias", _np(conv.bias.grad), b64.grad.numpy())


# ------------------------------------------------------------------------------------------------ 2. packer
FORWARD_SHAPES = [(16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
TRANSPOSED_SHAPES = [(32, 16), (64, 32), (128, 64)]


@pytest.mark.parametrize("cin,cout", FORWARD_SHAPES + TRANSPOSED_SHAPES)
def test_device_bf16_pack_is_byte_identical_to_the_host_pack(cin, cout):
    from futuredet_amd import hip_ops

    g = torch.Generator().manual_seed(cin * 7 + cout)
    for K in (27, 3, 1, 2):
        w = torch.randn((K, cin, cout), generator=g)
        # every third value exactly half way between two bf16 neighbours (ties to even, both parities), every seventh one ulp off a tie
        bits = w.view(torch.int32).clone()
        flat = bits.view(-1)
        flat[0::3] = (flat[0::3] & -65536) | 0x8000
        flat[1::7] = (flat[1::7] & -65536) | 0x7fff
        flat[2::7] = (flat[2::7] & -65536) | 0x8001
        w = bits.view(torch.float32)
        assert bool(torch.isfinite(w).all())
        wd = w.to(DEV)
        cases = ((hip_ops.PACK_PLAIN, w), (hip_ops.PACK_TRANSPOSED, w.transpose(1, 2)), (hip_ops.PACK_FLIPPED_TRANSPOSED, w.flip(0).transpose(1, 2)))
        for mode, host_w in cases:
            got = hip_ops.pack_spconv_weight_device(wd, mode, BF).cpu()
            want = hip_ops.pack_spconv_weight(host_w.contiguous(), BF)
            assert got.shape == want.shape and torch.equal(got, want), (K, cin, cout, mode)


# ------------------------------------------------------------------------------------------------ 3. transposed shapes
@pytest.mark.parametrize("geom", [([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0])], ids=["k27_s2", "k3_s211"])
@pytest.mark.parametrize("cbig,csmall", TRANSPOSED_SHAPES)
def test_transposed_shapes_on_a_transposed_table(cbig, csmall, geom):
    """the input gradient of a strided csmall -> cbig layer: fd_spconv_apply(dtype 1) at cbig -> csmall on fd_rulebook_transpose's table"""
    from futuredet_amd import hip_ops

    ks, st, pd = geom
    rng = np.random.default_rng(cbig + csmall + len(ks) * ks[1])
    src, dst, nbr = _rulebook(rng, 2, (21, 40, 40), 3000, ks, st, pd, False)
    K = nbr.shape[0]
    inv = hip_ops.rulebook_transpose(nbr, dst.n, src.n)
    w = (torch.from_numpy(rng.uniform(-1, 1, (K, csmall, cbig)).astype(np.float32)) / np.sqrt(cbig)).to(DEV)
    dy = _bf16_values(rng, (dst.n, cbig)).to(DEV).to(BF)
    wt = hip_ops.pack_spconv_weight_device(w, hip_ops.PACK_TRANSPOSED, BF)
    dx = hip_ops.spconv_apply(dy, wt, None, inv, src.n, csmall)
    torch.cuda.synchronize()
    assert dx.dtype == BF and tuple(dx.shape) == (src.n, csmall)
    x0 = torch.zeros((src.n, csmall), dtype=torch.float64, device=DEV)
    _, dx_ref, _ = _table_reference(x0, w.to(BF).double(), dy.double(), nbr, dst.n)
    _close_rounded("bf16 spconv %d->%d K%d on the transposed table" % (cbig, csmall, K), _np(dx), _np(dx_ref))


# ------------------------------------------------------------------------------------------------ 4. determinism, launch independence
@pytest.mark.parametrize("cin,cout", FORWARD_SHAPES)
def test_wgrad_bf16_is_deterministic_and_independent_of_the_launch(cin, cout):
    from futuredet_amd import hip_ops

    rng = np.random.default_rng(cin + cout)
    grid, nvox = WGRAD_TABLES[(cin, cout) in ((16, 16), (16, 32), (32, 64), (128, 128))]  # the small table: see test_gpu_spconv_grad.py
    src, dst, nbr = _rulebook(rng, 2, grid, nvox, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
    feats = _bf16_values(rng, (src.n, cin)).to(DEV).to(BF)
    dy = _bf16_values(rng, (dst.n, cout)).to(DEV).to(BF)
    a = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
    b = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
    assert a.dtype == torch.float32 and torch.equal(a, b), "two wgrad launches differ"
    _, _, want = _table_reference(feats.double(), None, dy.double(), nbr, dst.n)
    _close("bf16 wgrad %d->%d" % (cin, cout), _np(a), _np(want))
    # the count on the device, n_out a larger capacity: the table's and dY's tail rows hold garbage (indices in range)
    cap = dst.n + 700
    stride = (cap + 63) // 64 * 64
    table = torch.from_numpy(rng.integers(0, src.n, (nbr.shape[0], stride)).astype(np.int32)).to(DEV)
    table[:, : dst.n] = nbr[:, : dst.n]
    dy_cap = _bf16_values(rng, (cap, cout)).to(DEV).to(BF)
    dy_cap[: dst.n] = dy
    table.n_dev = torch.tensor([dst.n], dtype=torch.int32, device=DEV)
    c = hip_ops.spconv_wgrad(feats, dy_cap, table, cap)
    assert torch.equal(a, c), "a capacity launch with the count on the device differs"


# ------------------------------------------------------------------------------------------------ 5. empty level
def test_empty_level_gives_zero_gradients():
    from futuredet_amd import sparse as spconv

    w = torch.randn((27, 16, 32), device=DEV, requires_grad=True)
    b = torch.randn((32,), device=DEV, requires_grad=True)
    f = torch.zeros((0, 16), device=DEV, dtype=BF, requires_grad=True)
    nbr = torch.full((27, 64), -1, dtype=torch.int32, device=DEV)
    for subm in (True, False):
        y = spconv._SparseConvFunction.apply(f, w, b, nbr, 0, subm)
        assert y.shape == (0, 32) and y.dtype == BF
        y.sum().backward()
        torch.cuda.synchronize()
        assert f.grad.shape == (0, 16) and f.grad.dtype == BF
        assert w.grad.dtype == torch.float32 and torch.count_nonzero(w.grad) == 0 and torch.count_nonzero(b.grad) == 0
        w.grad = b.grad = f.grad = None


# ------------------------------------------------------------------------------------------------ 6. graph capture
def test_pack_apply_and_wgrad_replay_bit_identically_from_a_graph():
    from futuredet_amd import hip_ops

    rng = np.random.default_rng(21)
    cin, cout = 32, 64
    src, dst, nbr = _rulebook(rng, 2, (21, 48, 48), 5000, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
    feats = _bf16_values(rng, (src.n, cin)).to(DEV).to(BF)
    dy = _bf16_values(rng, (dst.n, cout)).to(DEV).to(BF)
    w = (torch.from_numpy(rng.uniform(-1, 1, (27, cin, cout)).astype(np.float32)) / 8).to(DEV)

    def run():
        wt = hip_ops.pack_spconv_weight_device(w, hip_ops.PACK_FLIPPED_TRANSPOSED, BF)
        dx = hip_ops.spconv_apply(dy, wt, None, nbr, src.n, cin)
        dw = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
        return wt, dx, dw

    eager = [t.clone() for t in run()]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()  # this stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(("packed weights", "dX", "dW"), outs, eager):
            assert torch.equal(got, want), name


# ------------------------------------------------------------------------------------------------ 7. whole backbone
def _voxels(seed, n_points):
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import synthetic_cloud
    from oracle import ops as oops

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    pts = synthetic_cloud(seed=seed, target_points=n_points)
    v, c, n = oops.points_to_voxel(pts, vg["voxel_size"], vg["range"], 10, True, 160000)
    return cfg, v, c, n


class _RoundBf16(torch.autograd.Function):
    """round to nearest even to bf16, in the tensor's own dtype; the gradient passes unchanged"""

    @staticmethod
    def forward(ctx, x):
        return x.to(BF).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _restated_backbone(bb, feats, coords, shape0, dtype=torch.float64, dev="cpu", rounded=False, cache=None):
    """float64 SpMiddleResNetFHD.forward_generic on oracle.ops.rulebook pairs (gather / index_add); BN on deep copies.  ``rounded``: every
    convolution's input rows, weights and output go through _RoundBf16.  ``cache``: rulebooks shared between calls on the same ``bb``."""
    from oracle import ops as oops

    cache = {} if cache is None else cache
    q = _RoundBf16.apply if rounded else (lambda t: t)

    def conv(m, f, idx, shape):
        ks, st, pd = m.geometry()
        key = (m.indice_key, m.subm) if m.indice_key else id(m)
        if key in cache:
            out_idx, pairs, pnum, out_shape = cache[key]
        else:
            out_idx, pairs, pnum, out_shape = oops.rulebook(idx, shape, ks, st, pd, m.subm)
            pairs = [(torch.from_numpy(pairs[k, 0, : int(pnum[k])].astype(np.int64)).to(dev),
                      torch.from_numpy(pairs[k, 1, : int(pnum[k])].astype(np.int64)).to(dev)) for k in range(len(pnum))]
            cache[key] = (out_idx, pairs, pnum, out_shape)
        K = int(np.prod(ks))
        W = q(m.weight.to(dev, dtype)).reshape(K, m.in_channels, m.out_channels)
        f = q(f)
        out = torch.zeros((len(out_idx), m.out_channels), dtype=dtype, device=dev)
        for k in range(K):
            i, o = pairs[k]
            out = out.index_add(0, o, f[i] @ W[k])
        if m.bias is not None:
            out = out + m.bias.to(dev, dtype)
        return q(out), out_idx, list(out_shape)

    bns = {}

    def bn(m, f):
        if id(m) not in bns:
            bns[id(m)] = (m.running_mean.detach().to(dev, dtype).clone(), m.running_var.detach().to(dev, dtype).clone())
        rm, rv = bns[id(m)]
        return F.batch_norm(f, rm, rv, m.weight.to(dev, dtype), m.bias.to(dev, dtype), training=True, momentum=m.momentum, eps=m.eps)

    def block(blk, f, idx, shape):
        o, _, _ = conv(blk.conv1, f, idx, shape)
        o = torch.relu(bn(blk.bn1, o))
        o, _, _ = conv(blk.conv2, o, idx, shape)
        o = bn(blk.bn2, o)
        return torch.relu(o + f)

    f, idx, shape = feats, coords, list(shape0)
    f, idx, shape = conv(bb.conv_input[0], f, idx, shape)
    f = torch.relu(bn(bb.conv_input[1], f))
    for blk in bb.conv1:
        f = block(blk, f, idx, shape)
    for seq in (bb.conv2, bb.conv3, bb.conv4):
        f, idx, shape = conv(seq[0], f, idx, shape)
        f = torch.relu(bn(seq[1], f))
        f = block(seq[3], f, idx, shape)
        f = block(seq[4], f, idx, shape)
    f, idx, shape = conv(bb.extra_conv[0], f, idx, shape)
    f = torch.relu(bn(bb.extra_conv[1], f))
    return f, idx, shape, bns


def _record_conv_calls(spconv, seen):
    """patches _SparseConvFunction.apply to record what every convolution met; returns the undo"""
    orig = spconv._SparseConvFunction.apply

    def recording(feats, w, b, nbr, n_out, subm):
        out = orig(feats, w, b, nbr, n_out, subm)
        rec = dict(feats=feats.detach(), w=w.detach(), b=None if b is None else b.detach(), nbr=nbr, n_out=n_out, subm=subm)
        if out.requires_grad:
            out.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        seen.append(rec)
        return out

    spconv._SparseConvFunction.apply = recording
    return lambda: setattr(spconv._SparseConvFunction, "apply", orig)


@pytest.fixture(scope="module")
def backbone_run():
    """One mixed-precision forward + backward of SpMiddleResNetFHD at ~30k points, every convolution call recorded, and the float64
    restatement's gradients with and without bf16 rounding of every convolution's rows, weights and output."""
    from futuredet_amd import sparse as spconv
    from futuredet_amd.backbones import SpMiddleResNetFHD
    from futuredet_amd.synth import seeded_state_dict

    cfg, v, c, n = _voxels(3, 30000)
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32))
    coords = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, 5), strict=False)
    ref_bb = copy.deepcopy(bb)
    start = copy.deepcopy(bb)  # the state every run of this module starts from
    bb = bb.to(DEV).train()
    bb.train_dtype = BF
    before = {k: t.detach().clone() for k, t in bb.named_buffers()}
    input_shape = np.array([1440, 1440, 40])
    seen = []
    undo = _record_conv_calls(spconv, seen)
    try:
        bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
        rng = np.random.default_rng(9)
        G = torch.from_numpy(rng.uniform(-1, 1, tuple(bev.shape)).astype(np.float32))
        (bev * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        undo()

    shape0 = list(np.array(input_shape[::-1]) + [1, 0, 0])
    ref_grads, cache = {}, {}
    for rounded in (False, True):
        ref_bb.zero_grad()
        f, idx, shape, _ = _restated_backbone(ref_bb, feats.double().to(DEV), coords, shape0, dev=DEV, rounded=rounded, cache=cache)
        Gr = G.double().view(1, 128, shape[0], G.shape[2], G.shape[3]).to(DEV)
        ii = torch.from_numpy(idx).long().to(DEV)
        (f * Gr[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]).sum().backward()
        ref_grads[rounded] = {name: p.grad.detach().double().cpu().numpy().copy() for name, p in ref_bb.named_parameters()}
        for p in ref_bb.parameters():
            p.grad = None
    def rerun(model):
        """forward + backward (where anything needs a gradient) of ``model`` on the fixture's input and output gradient"""
        out, _ = model(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
        if out.requires_grad:
            (out * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return out

    return dict(bb=bb, bev=bev, seen=seen, before=before, ref_grads=ref_grads, start=start, rerun=rerun)


def test_backbone_runs_all_21_convolutions_on_bf16_rows(backbone_run):
    from futuredet_amd import sparse as spconv

    seen = backbone_run["seen"]
    assert len(seen) == 21
    assert backbone_run["bev"].dtype == torch.float32  # the neck gets an fp32 map
    for li, r in enumerate(seen):
        assert r["feats"].dtype == BF and r["w"].dtype == torch.float32 and r["dy"].dtype == BF, li
        x = r["feats"].clone().requires_grad_(True)
        w = r["w"].clone().requires_grad_(True)
        y = spconv._SparseConvFunction.apply(x, w, None, r["nbr"], r["n_out"], r["subm"])
        y.backward(r["dy"])
        torch.cuda.synchronize()
        assert x.grad.dtype == BF and w.grad.dtype == torch.float32
        _, dx_ref, dw_ref = _table_reference(r["feats"].double(), r["w"].to(BF).double(), r["dy"].double(), r["nbr"], r["n_out"])
        tag = "bf16 backbone layer %d (%s %d->%d K%d, %d rows)" % (li, "subm" if r["subm"] else "strided", w.shape[1], w.shape[2], w.shape[0], r["n_out"])
        _close(tag + " dW", _np(w.grad), _np(dw_ref))
        _close_rounded(tag + " dX", _np(x.grad), _np(dx_ref))


def test_backbone_gradients_are_finite_fp32_and_the_statistics_move(backbone_run):
    bb = backbone_run["bb"]
    for name, p in bb.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
    moved = 0
    for name, buf in bb.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            assert buf.dtype == torch.float32 and bool(torch.isfinite(buf).all()), name
            assert not torch.equal(buf, backbone_run["before"][name]), name + " did not move"
            moved += 1
    assert moved == 2 * 21  # a BatchNorm1d behind each of the 21 convolutions


def test_backbone_gradients_lie_within_twice_the_rounding_distance(backbone_run):
    """Norm-wise error of every parameter gradient against the pure float64 restatement.  No bound can be derived (ReLU masks flip at bf16
    granularity), so the yardstick is measured on the reference alone: E(name) = the norm-wise distance between that restatement and the same
    restatement with every convolution's rows, weights and output rounded to bf16, both in float64.  The device must lie within
    2 E(name) + 1e-2: it rounds at the same places, but from fp32 sums in another order (the factor 2), on top of the fp32 suite's 1e-2."""
    got = dict(backbone_run["bb"].named_parameters())
    pure, rounded = backbone_run["ref_grads"][False], backbone_run["ref_grads"][True]
    worst, fails = None, []
    for name, ref in pure.items():
        if name.endswith("bias") and "bn" not in name and not name.endswith(".1.bias"):
            continue  # a convolution bias followed by training-mode BatchNorm: its exact gradient is 0, both sides are rounding noise
        norm = max(float(np.linalg.norm(ref)), 1e-30)
        E = float(np.linalg.norm(rounded[name] - ref)) / norm
        e = float(np.linalg.norm(got[name].grad.double().cpu().numpy() - ref)) / norm
        report("bf16 backbone grad (norm-wise) " + name, e, 2 * E + 1e-2, "E %.3e" % E)
        if worst is None or e > worst[1]:
            worst = (name, e, E)
        if not e <= 2 * E + 1e-2:
            fails.append((name, e, E))
    report("bf16 backbone grad (norm-wise) largest: " + worst[0], worst[1], 2 * worst[2] + 1e-2, "E %.3e" % worst[2])
    assert not fails, fails


def test_frozen_first_convolution_takes_bf16_rows(backbone_run):
    """conv_input.0 frozen behind a reader without parameters: its rows need no gradient, so it runs outside the autograd function, on
    bf16 rows all the same.  Every other gradient is bit for bit that of the unfrozen run, and so within the same distance of float64."""
    from futuredet_amd import sparse as spconv

    bb = copy.deepcopy(backbone_run["start"]).to(DEV).train()
    bb.train_dtype = BF
    bb.conv_input[0].weight.requires_grad_(False)
    seen = []
    undo = _record_conv_calls(spconv, seen)
    try:
        bev = backbone_run["rerun"](bb)
    finally:
        undo()
    assert len(seen) == 20 and all(r["feats"].dtype == BF for r in seen)  # the frozen one is not among them
    assert bev.dtype == torch.float32 and torch.equal(bev, backbone_run["bev"])
    assert bb.conv_input[0].weight.grad is None
    want = dict(backbone_run["bb"].named_parameters())
    pure, rounded = backbone_run["ref_grads"][False], backbone_run["ref_grads"][True]
    for name, p in bb.named_parameters():
        if name == "conv_input.0.weight":
            continue
        assert p.grad is not None and torch.equal(p.grad, want[name].grad), name
        if name.endswith("bias") and "bn" not in name and not name.endswith(".1.bias"):
            continue  # (as above: exact gradient 0)
        norm = max(float(np.linalg.norm(pure[name])), 1e-30)
        E = float(np.linalg.norm(rounded[name] - pure[name])) / norm
        e = float(np.linalg.norm(p.grad.double().cpu().numpy() - pure[name])) / norm
        assert e <= 2 * E + 1e-2, (name, e, E)


def test_frozen_backbone_in_train_mode_runs_bf16_rows(backbone_run):
    """every parameter frozen, the module left in .train(): all 21 convolutions outside the autograd function, the same BEV map bit for bit"""
    from futuredet_amd import sparse as spconv

    bb = copy.deepcopy(backbone_run["start"]).to(DEV).train()
    bb.train_dtype = BF
    for p in bb.parameters():
        p.requires_grad_(False)
    seen = []
    undo = _record_conv_calls(spconv, seen)
    try:
        bev = backbone_run["rerun"](bb)
    finally:
        undo()
    assert seen == [] and not bev.requires_grad
    assert bev.dtype == torch.float32 and torch.equal(bev, backbone_run["bev"])
    for name, buf in bb.named_buffers():  # the BatchNorms saw the same rows
        assert torch.equal(buf, dict(backbone_run["bb"].named_buffers())[name]), name


# ------------------------------------------------------------------------------------------------ 8. one training step
def _example(cfg, seed):
    cfg_, v, c, n = _voxels(seed, 20000)
    T = cfg.timesteps
    rng = np.random.default_rng(seed)
    Hh = Wh = 180
    M = 16
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([[1440, 1440, 40]]),
              metadata=[None])
    for key in ("hm", "ind", "mask", "cat", "anno_box"):
        ex[key] = []
    for s in range(T):
        ind = torch.from_numpy(rng.choice(Hh * Wh, M, replace=False)[None].astype(np.int64)).to(DEV)
        hm = torch.from_numpy((rng.uniform(0, 0.9, (1, 1, Hh, Wh)) ** 3).astype(np.float32)).to(DEV)
        hm.view(-1)[ind[0]] = 1.0
        mask = torch.ones((1, M), dtype=torch.uint8, device=DEV)
        ex["hm"].append([hm])
        ex["ind"].append([ind])
        ex["mask"].append([mask])
        ex["cat"].append([torch.zeros((1, M), dtype=torch.int64, device=DEV)])
        ex["anno_box"].append([torch.from_numpy(rng.normal(0, 1, (1, M, 10)).astype(np.float32)).to(DEV)])
    return ex


def test_one_mixed_precision_training_step_end_to_end():
    from futuredet_amd import build_detector, solver
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims

    cfg = centerpoint_config("forecast_n0")
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV)
    cloud = [torch.from_numpy(synthetic_cloud(seed=1, target_points=20000)).to(DEV)]

    def detect(model, dtype):
        model.eval()
        model.set_precision(dtype)
        with torch.no_grad():
            r = model.forward_points(cloud, cfg.voxel_generator, padded=False)[0]
        torch.cuda.synchronize()
        model.set_precision(torch.float32)
        return torch.cat([r["box3d_lidar"], r["scores"][:, None]], 1).cpu()

    before = {dt: detect(net, dt) for dt in (torch.float32, BF)}  # fills the folded-BN / packed-weight caches of both eval paths
    opt = solver.FusedAdam.for_model(net, lr=1e-4)
    ex = _example(cfg, 2)

    def step():
        net.train()
        ret = net(ex, return_loss=True)
        loss = sum(ret["loss"])
        assert bool(torch.isfinite(loss))
        opt.zero_grad()
        loss.backward()
        for name, p in net.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
        old = {name: p.detach().clone() for name, p in net.backbone.named_parameters()}
        opt.step()
        torch.cuda.synchronize()
        for name, p in net.backbone.named_parameters():
            assert not torch.equal(old[name], p), "FusedAdam.step left backbone.%s as it was" % name

    net.backbone.train_dtype = BF
    step()
    fresh = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    fresh.load_state_dict(net.state_dict())
    fresh = fresh.to(DEV)
    for dt in (torch.float32, BF):
        after, want = detect(net, dt), detect(fresh, dt)
        # the eval path after the step computes what a fresh model with the stepped weights computes, not the pre-step detections
        assert len(want) > 0 and after.shape == want.shape, (dt, after.shape, want.shape)
        assert torch.allclose(after, want, rtol=0, atol=0, equal_nan=True), (dt, float((after - want).nan_to_num().abs().max()))
        assert before[dt].shape != want.shape or not torch.equal(before[dt], want), "one step must change the %s detections" % dt
    # the eval switch next to the training switch: training takes train_dtype
    net.backbone.compute_dtype = BF
    step()


# ------------------------------------------------------------------------------------------------ 9. fp32 path unchanged
def test_default_train_dtype_keeps_the_fp32_path_bit_for_bit():
    from futuredet_amd import hip_ops
    from futuredet_amd import sparse as spconv
    from futuredet_amd.backbones import SpMiddleResNetFHD
    from futuredet_amd.synth import seeded_state_dict

    cfg, v, c, n = _voxels(4, 8000)
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32))
    coords = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, 5), strict=False)
    bb = bb.to(DEV).train()
    assert bb.train_dtype is torch.float32
    seen = []
    undo = _record_conv_calls(spconv, seen)
    try:
        bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, np.array([1440, 1440, 40]))
        bev.sum().backward()
        torch.cuda.synchronize()
    finally:
        undo()
    assert len(seen) == 21 and bev.dtype == torch.float32
    assert all(r["feats"].dtype == torch.float32 and r["dy"].dtype == torch.float32 for r in seen)
    r = seen[4]  # conv1.1.conv2: SubM 16 -> 16 with a bias
    assert r["subm"] and r["b"] is not None
    x, w = r["feats"].clone().requires_grad_(True), r["w"].clone().requires_grad_(True)
    y = spconv._SparseConvFunction.apply(x, w, r["b"], r["nbr"], r["n_out"], True)
    y.backward(r["dy"])
    y_direct = hip_ops.spconv_apply(r["feats"], hip_ops.pack_spconv_weight_device(r["w"]), r["b"], r["nbr"], r["n_out"], w.shape[2])
    dx_direct = hip_ops.spconv_apply(r["dy"], hip_ops.pack_spconv_weight_device(r["w"], hip_ops.PACK_FLIPPED_TRANSPOSED), None, r["nbr"],
                                     x.shape[0], x.shape[1])
    dw_direct = hip_ops.spconv_wgrad(r["feats"], r["dy"], r["nbr"], r["n_out"])
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and torch.equal(y, y_direct)
    assert torch.equal(x.grad, dx_direct) and torch.equal(w.grad, dw_direct)
