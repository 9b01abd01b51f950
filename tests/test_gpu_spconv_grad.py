"""Training path of the sparse convolution on the device: the backward kernels of fd_spconv_grad.hip behind the autograd surface of
futuredet_amd/sparse.py, checked against float64 torch restatements, and one training step of whole VoxelNet configs."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _coords(rng, B, D, H, W, n_per_batch):
    out = []
    for b in range(B):
        cells = rng.choice(D * H * W, n_per_batch, replace=False)
        z, rem = np.divmod(cells, H * W)
        y, x = np.divmod(rem, W)
        out.append(np.stack([np.full_like(z, b), z, y, x], 1))
    return np.concatenate(out).astype(np.int32)


def _close(name, got, ref, tol=1e-4):
    """element-wise |got - ref| <= tol * max(1, |ref|) on values scaled by the largest reference magnitude (sums of thousands of terms)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    assert_close(name, got / scale, ref / scale, tol)


def _dense64(feats, coords, B, shape):
    D, H, W = shape
    x = torch.zeros((B, feats.shape[1], D, H, W), dtype=torch.float64)
    c = torch.from_numpy(coords).long()
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = feats
    return x


LAYERS = [  # (cin, cout, ksize, stride, pad, subm, bias, grid (D, H, W), voxels per sample)
    (5, 16, 3, 1, 1, True, False, (41, 96, 96), 9000),
    (16, 16, 3, 1, 1, True, True, (41, 96, 96), 9000),
    (16, 32, 3, 2, 1, False, False, (41, 96, 96), 9000),
    (32, 32, 3, 1, 1, True, True, (21, 48, 48), 6000),
    (32, 64, 3, 2, 1, False, False, (21, 48, 48), 6000),
    (64, 64, 3, 1, 1, True, True, (11, 24, 24), 1500),
    (64, 128, 3, 2, [0, 1, 1], False, False, (11, 24, 24), 1500),
    (128, 128, 3, 1, 1, True, True, (5, 12, 12), 300),
    (128, 128, (3, 1, 1), (2, 1, 1), 0, False, False, (5, 12, 12), 300),
]


@pytest.mark.parametrize("layer", LAYERS, ids=lambda l: "%d-%d_k%s_s%s_p%s" % (l[0], l[1], l[2], l[3], l[4]))
def test_layer_gradients_match_float64_conv3d(layer):
    from futuredet_amd import sparse as spconv

    cin, cout, ks, st, pd, subm, bias, shape, nvox = layer
    rng = np.random.default_rng(cin * 1000 + cout + (0 if subm else 7))
    B = 2
    coords = _coords(rng, B, *shape, nvox - 37)  # row counts that are no multiple of any tile
    feats = torch.from_numpy(rng.uniform(-1, 1, (len(coords), cin)).astype(np.float32))
    torch.manual_seed(cin + cout)
    conv = (spconv.SubMConv3d(cin, cout, ks, bias=bias, indice_key="k") if subm else
            spconv.SparseConv3d(cin, cout, ks, st, padding=pd, bias=bias)).to(DEV).train()
    f = feats.to(DEV).requires_grad_(True)
    x = spconv.SparseConvTensor(f, torch.from_numpy(coords).to(DEV), list(shape), B)
    y = conv(x)
    ycoords = y.indices.cpu().numpy()
    G = torch.from_numpy(rng.uniform(-1, 1, (len(ycoords), cout)).astype(np.float32))
    (y.features * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()

    # float64 reference: dense conv3d, loss on the active output rows only
    x64 = _dense64(feats.double(), coords, B, shape).requires_grad_(True)
    w64 = conv.weight.detach().cpu().double().requires_grad_(True)
    b64 = conv.bias.detach().cpu().double().requires_grad_(True) if bias else None
    ks3, st3, pd3 = conv.geometry()
    out = F.conv3d(x64, w64.permute(4, 3, 0, 1, 2), b64, stride=st3, padding=pd3)
    yc = torch.from_numpy(ycoords).long()
    out_rows = out[yc[:, 0], :, yc[:, 1], yc[:, 2], yc[:, 3]]
    _close("spconv fwd", y.features.detach().cpu().numpy(), out_rows.detach().numpy())
    (out_rows * G.double()).sum().backward()
    c = torch.from_numpy(coords).long()
    dx_ref = x64.grad[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]
    tag = "spconv grad %d->%d k%s s%s p%s" % (cin, cout, ks, st, pd)
    _close(tag + " dX", f.grad.cpu().numpy(), dx_ref.numpy())
    _close(tag + " dW", conv.weight.grad.cpu().numpy(), w64.grad.numpy())
    if bias:
        _close(tag + " dBias", conv.bias.grad.cpu().numpy(), b64.grad.numpy())


def test_empty_level_gives_zero_gradients():
    from futuredet_amd import sparse as spconv

    w = torch.randn((27, 16, 32), device=DEV, requires_grad=True)
    b = torch.randn((32,), device=DEV, requires_grad=True)
    f = torch.zeros((0, 16), device=DEV, requires_grad=True)
    nbr = torch.full((27, 64), -1, dtype=torch.int32, device=DEV)
    for subm in (True, False):
        y = spconv._SparseConvFunction.apply(f, w, b, nbr, 0, subm)
        assert y.shape == (0, 32)
        y.sum().backward()
        assert f.grad.shape == (0, 16) and torch.count_nonzero(w.grad) == 0 and torch.count_nonzero(b.grad) == 0
        w.grad = b.grad = f.grad = None


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


def test_rulebook_transpose_inverts_the_table_exactly():
    from futuredet_amd import hip_ops

    rng = np.random.default_rng(5)
    for ks, st, pd in (([3, 3, 3], [2, 2, 2], [1, 1, 1]), ([3, 3, 3], [2, 2, 2], [0, 1, 1]), ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
                       ([3, 3, 3], [1, 1, 1], [1, 1, 1])):
        src, dst, nbr = _rulebook(rng, 2, (21, 40, 40), 3000, ks, st, pd, False)
        inv = hip_ops.rulebook_transpose(nbr, dst.n, src.n).cpu().numpy()
        table = nbr.cpu().numpy()[:, : dst.n]
        want = np.full((table.shape[0], inv.shape[1]), -1, np.int32)
        for k in range(table.shape[0]):
            o = np.nonzero(table[k] >= 0)[0]
            want[k, table[k, o]] = o
        assert np.array_equal(inv, want), (ks, st, pd)


@pytest.mark.parametrize("cin,cout", [(a, b) for a in (16, 32, 64, 128) for b in (16, 32, 64, 128)])
def test_device_pack_is_byte_identical_to_the_host_pack(cin, cout):
    from futuredet_amd import hip_ops

    g = torch.Generator().manual_seed(cin * 7 + cout)
    for K in (27, 3, 1, 2):
        w = torch.randn((K, cin, cout), generator=g)
        wd = w.to(DEV)
        cases = ((hip_ops.PACK_PLAIN, w), (hip_ops.PACK_TRANSPOSED, w.transpose(1, 2)), (hip_ops.PACK_FLIPPED_TRANSPOSED, w.flip(0).transpose(1, 2)))
        for mode, host_w in cases:
            got = hip_ops.pack_spconv_weight_device(wd, mode).cpu()
            want = hip_ops.pack_spconv_weight(host_w.contiguous())
            assert got.shape == want.shape and torch.equal(got, want), (K, cin, cout, mode)


# every instantiation has its own tile split: four on a 10000-row table, the rest on a small one -- about 1300 rows, i.e. three 512-row
# chunks with a partial last one, last batches with a zero-padded tail, and (below) a device count that ends inside the second chunk
WGRAD_TABLES = {True: ((21, 48, 48), 5000), False: ((9, 24, 24), 650)}  # grid, voxels per sample


@pytest.mark.parametrize("cin,cout", [(a, b) for a in (16, 32, 64, 128) for b in (16, 32, 64, 128)])
def test_wgrad_is_deterministic_and_takes_a_device_count(cin, cout):
    from futuredet_amd import hip_ops

    rng = np.random.default_rng(cin + cout)
    grid, nvox = WGRAD_TABLES[(cin, cout) in ((16, 16), (16, 32), (64, 128), (128, 128))]
    src, dst, nbr = _rulebook(rng, 2, grid, nvox, [3, 3, 3], [1, 1, 1], [1, 1, 1], True)
    feats = torch.from_numpy(rng.uniform(-1, 1, (src.n, cin)).astype(np.float32)).to(DEV)
    dy = torch.from_numpy(rng.uniform(-1, 1, (dst.n, cout)).astype(np.float32)).to(DEV)
    a = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
    b = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
    assert torch.equal(a, b), "two wgrad launches differ"
    # float64 restatement on the table
    t = nbr.cpu().long()[:, : dst.n]
    f64, d64 = feats.cpu().double(), dy.cpu().double()
    want = torch.stack([f64[t[k][t[k] >= 0]].T @ d64[torch.nonzero(t[k] >= 0)[:, 0]] for k in range(t.shape[0])])
    _close("wgrad %d->%d" % (cin, cout), a.cpu().numpy(), want.numpy())
    # n_out from a device count (the table and dY keep the capacity): rows past the count contribute nothing
    cut = dst.n - 333
    nbr.n_dev = torch.tensor([cut], dtype=torch.int32, device=DEV)
    c = hip_ops.spconv_wgrad(feats, dy, nbr, dst.n)
    nbr.n_dev = None
    dy_cut = dy.clone()
    dy_cut[cut:] = 0
    d = hip_ops.spconv_wgrad(feats, dy_cut, nbr, dst.n)
    assert torch.equal(c, d)


def test_backward_is_bit_identical_across_runs():
    from futuredet_amd import sparse as spconv

    rng = np.random.default_rng(11)
    coords = torch.from_numpy(_coords(rng, 2, 21, 64, 64, 8000)).to(DEV)
    feats = torch.from_numpy(rng.uniform(-1, 1, (len(coords), 32)).astype(np.float32)).to(DEV)
    conv = spconv.SubMConv3d(32, 64, 3, bias=True, indice_key="d").to(DEV).train()
    grads = []
    for _ in range(2):
        conv.zero_grad()
        x = spconv.SparseConvTensor(feats.clone().requires_grad_(True), coords, [21, 64, 64], 2)
        y = conv(x)
        (y.features ** 2).sum().backward()
        grads.append(conv.weight.grad.clone())
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------------------------------------------ whole backbone
def _voxels(seed, n_points):
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import synthetic_cloud
    from oracle import ops as oops

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    pts = synthetic_cloud(seed=seed, target_points=n_points)
    v, c, n = oops.points_to_voxel(pts, vg["voxel_size"], vg["range"], 10, True, 160000)
    return cfg, v, c, n


def _restated_backbone(bb, feats, coords, shape0, dtype=torch.float64, dev="cpu"):
    """float64 SpMiddleResNetFHD.forward_generic on oracle.ops.rulebook pairs (gather / index_add); BN on deep copies."""
    from oracle import ops as oops

    cache = {}

    def conv(m, f, idx, shape):
        ks, st, pd = m.geometry()
        key = (m.indice_key, m.subm) if m.indice_key else None
        if key is not None and key in cache:
            out_idx, pairs, pnum, out_shape = cache[key]
        else:
            out_idx, pairs, pnum, out_shape = oops.rulebook(idx, shape, ks, st, pd, m.subm)
            if key is not None:
                cache[key] = (out_idx, pairs, pnum, out_shape)
        K = int(np.prod(ks))
        W = m.weight.to(dev, dtype).reshape(K, m.in_channels, m.out_channels)
        out = torch.zeros((len(out_idx), m.out_channels), dtype=dtype, device=dev)
        for k in range(K):
            n = int(pnum[k])
            i = torch.from_numpy(pairs[k, 0, :n].astype(np.int64)).to(dev)
            o = torch.from_numpy(pairs[k, 1, :n].astype(np.int64)).to(dev)
            out = out.index_add(0, o, f[i] @ W[k])
        if m.bias is not None:
            out = out + m.bias.to(dev, dtype)
        return out, out_idx, list(out_shape)

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


def test_backbone_training_gradients_match_a_float64_restatement(monkeypatch):
    """SpMiddleResNetFHD in training mode at ~30k points.  (1) Every convolution, on the features and output gradient it met inside the
    backbone: dX and dW against float64 gather / index_add on its own rulebook (tight: the kernels).  (2) Every parameter's gradient and
    every BN running statistic against a float64 restatement of the whole backbone on oracle.ops.rulebook pairs (the wiring).  Training-mode
    BatchNorm after every convolution makes the deep gradients ill-conditioned -- an fp32 restatement lands ~1e-3 off, and a ReLU mask
    that flips on a last-bit difference moves more -- so (2) is norm-wise at 1e-2: a wrong table, tap order or channel slice is O(1)."""
    from futuredet_amd import sparse as spconv
    from futuredet_amd.backbones import SpMiddleResNetFHD
    from futuredet_amd.synth import seeded_state_dict

    seen = []
    orig = spconv._SparseConvFunction.apply

    def recording(feats, w, b, nbr, n_out, subm):
        out = orig(feats, w, b, nbr, n_out, subm)
        rec = dict(feats=feats.detach(), w=w.detach(), nbr=nbr, n_out=n_out, subm=subm)
        out.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        seen.append(rec)
        return out

    monkeypatch.setattr(spconv._SparseConvFunction, "apply", recording)
    cfg, v, c, n = _voxels(3, 30000)
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32))
    coords = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, 5), strict=False)
    ref_bb = copy.deepcopy(bb)
    bb = bb.to(DEV).train()
    input_shape = np.array([1440, 1440, 40])
    bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
    rng = np.random.default_rng(9)
    G = torch.from_numpy(rng.uniform(-1, 1, tuple(bev.shape)).astype(np.float32))
    (bev * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()

    # (1) the kernels, layer by layer, on what they met in the backbone
    assert len(seen) == 21
    for li, r in enumerate(seen):
        x = r["feats"].clone().requires_grad_(True)
        w = r["w"].clone().requires_grad_(True)
        y = spconv._SparseConvFunction.apply(x, w, None, r["nbr"], r["n_out"], r["subm"])
        y.backward(r["dy"])
        X, W, dy = r["feats"].double(), r["w"].double(), r["dy"].double()
        t = r["nbr"][:, : r["n_out"]].long()
        dw_ref, dx_ref = torch.zeros_like(W), torch.zeros_like(X)
        for k in range(W.shape[0]):
            o = torch.nonzero(t[k] >= 0)[:, 0]
            i = t[k][o]
            dw_ref[k] = X[i].T @ dy[o]
            dx_ref.index_add_(0, i, dy[o] @ W[k].T)
        tag = "backbone layer %d (%s %d->%d K%d, %d rows)" % (li, "subm" if r["subm"] else "strided", W.shape[1], W.shape[2], W.shape[0], r["n_out"])
        _close(tag + " dW", w.grad.cpu().numpy(), dw_ref.cpu().numpy(), 1e-5)
        _close(tag + " dX", x.grad.cpu().numpy(), dx_ref.cpu().numpy(), 1e-5)

    # (2) the whole backbone
    shape0 = list(np.array(input_shape[::-1]) + [1, 0, 0])
    f, idx, shape, bns = _restated_backbone(ref_bb, feats.double(), coords, shape0)
    Gr = G.double().view(1, 128, shape[0], G.shape[2], G.shape[3])
    ii = torch.from_numpy(idx).long()
    (f * Gr[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]).sum().backward()
    got = dict(bb.named_parameters())
    for name, p in ref_bb.named_parameters():
        assert got[name].grad is not None and bool(torch.isfinite(got[name].grad).all()), name
        ref = p.grad.numpy().astype(np.float64)
        if name.endswith("bias") and "bn" not in name and not name.endswith(".1.bias"):
            continue  # a convolution bias followed by training-mode BatchNorm: its exact gradient is 0, both sides are rounding noise
        e = float(np.linalg.norm(got[name].grad.cpu().numpy() - ref)) / max(float(np.linalg.norm(ref)), 1e-30)
        report("backbone grad (norm-wise) " + name, e, 1e-2)
        assert e <= 1e-2, (name, e)
    mods = dict(bb.named_modules())
    for name, m in ref_bb.named_modules():
        if id(m) in bns:
            for stat, want in zip(("running_mean", "running_var"), bns[id(m)]):
                _close("backbone %s.%s" % (name, stat), getattr(mods[name], stat).cpu().numpy(), want.numpy(), 1e-4)


def test_bf16_backbone_refuses_training():
    from futuredet_amd.backbones import SpMiddleResNetFHD

    bb = SpMiddleResNetFHD(num_input_features=5).to(DEV).train()
    bb.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="fp32"):
        bb(torch.zeros((4, 5), device=DEV), torch.zeros((4, 4), dtype=torch.int32, device=DEV), 1, np.array([1440, 1440, 40]))


# ------------------------------------------------------------------------------------------------ end to end
def _example(cfg, seed):
    from futuredet_amd.synth import synthetic_cloud

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


@pytest.mark.parametrize("variant", ["forecast_n0", "forecast_n3dtf"])
def test_training_step_end_to_end(variant):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims

    cfg = centerpoint_config(variant)
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV)
    cloud = [torch.from_numpy(synthetic_cloud(seed=1, target_points=20000)).to(DEV)]

    def detect(model):
        model.eval()
        with torch.no_grad():
            r = model.forward_points(cloud, cfg.voxel_generator, padded=False)[0]
        torch.cuda.synchronize()
        return torch.cat([r["box3d_lidar"], r["scores"][:, None]], 1).cpu()

    before = detect(net)
    net.train()
    ret = net(_example(cfg, 2), return_loss=True)
    loss = sum(ret["loss"])
    assert torch.isfinite(loss)
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    opt.zero_grad()
    loss.backward()
    for name, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    opt.step()
    after = detect(net)
    fresh = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    fresh.load_state_dict(net.state_dict())
    want = detect(fresh.to(DEV))
    # the eval path after the step computes what a fresh model with the stepped weights computes, not the pre-step detections
    assert len(want) > 0 and after.shape == want.shape, (after.shape, want.shape)
    assert torch.allclose(after, want, rtol=0, atol=0, equal_nan=True), float((after - want).nan_to_num().abs().max())
    assert before.shape != want.shape or not torch.equal(before, want), "one SGD step must change the detections"
