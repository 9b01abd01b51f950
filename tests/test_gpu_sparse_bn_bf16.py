"""-m gpu: the bf16-row form of the fused training-mode BatchNorm of the sparse backbone (futuredet_amd/csrc/fd_sparse_bn.hip over
fd_row_bn.h, sparse.batch_norm_act, SpMiddleResNetFHD.fused_bn with train_dtype = torch.bfloat16).

The bf16 kernels are the fp32 kernels with another load and store of a thread's four channels: a bf16 row is widened exactly on load and
rounded to nearest even on store.  So test 1 asks for bits: statistics and parameter gradients equal to those of the fp32 entry points on
the widened rows, y and dx equal to the fp32 results rounded once by torch.  Test 2 ties the fp32 kernels to float64 at the two large row
counts that test 1 adds (more than one chunk per group; apply workgroups of two chunks), test 3 ties the bf16 path to float64 directly.

Gates against float64 are those of test_gpu_sparse_bn.py: 1e-5 * max |ref| on inputs (a), 1e-4 * max |ref| on inputs (b); a result that
is rounded once to bf16 gets 2^-8 |ref| on top (unit roundoff of round-to-nearest-even taken generously, as in
test_gpu_spconv_grad_bf16._close_rounded)."""
import copy

import numpy as np
import pytest
import torch

from parity_util import report
from test_gpu_sparse_bn import DEAD_CH, EPS, FORMS, _check_against_float64, _gate, _inputs, _ref_backward, _ref_forward

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
U = 2.0 ** -8
INPUTS = (("a", 0.0, 1e-5), ("b", 30.0, 1e-4))
ROW_KEYS = ("x", "res", "dy")


def _P():
    from futuredet_amd import hip_ops

    return hip_ops.sparse_bn_chunk()


def _bits(t):
    """the bit patterns of a floating tensor (so that -0 != +0 and a NaN can equal itself); an integer tensor as it is"""
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _device_inputs(d):
    """_inputs on the device, x / res / dy rounded to bf16"""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()}
    for k in ROW_KEYS:
        t[k] = t[k].to(BF)
    return t


def _run(hip, t, relu, with_res, dtype, momentum=0.1, n_dev=None, mask_y=None):
    """forward + backward through hip_ops on rows of ``dtype`` (t holds bf16 rows: .float() widens them exactly) and fresh copies of the
    running statistics.  ``mask_y``: the y handed to the backward as its ReLU mask (default: this run's own)."""
    x, dy = t["x"].to(dtype), t["dy"].to(dtype)
    res = t["res"].to(dtype) if with_res else None
    rm, rv = t["rm"].clone(), t["rv"].clone()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    y, saved = hip.sparse_bn_train_forward(x, t["gamma"], t["beta"], rm, rv, nbt, EPS, momentum, residual=res, relu=relu, n_dev=n_dev)
    dx, dres, dgamma, dbeta = hip.sparse_bn_train_backward(dy, x, y if mask_y is None else mask_y, t["gamma"], saved, relu=relu, n_dev=n_dev,
                                                           want_residual=with_res)
    out = dict(y=y, saved=saved, rm=rm, rv=rv, nbt=nbt, dx=dx, dgamma=dgamma, dbeta=dbeta)
    if dres is not None:
        out["dres"] = dres
    return out


def _check_bf16_is_fp32_rounded_once(hip, d, relu, with_res, tag):
    t = _device_inputs(d)
    lo = _run(hip, t, relu, with_res, BF)
    hi = _run(hip, t, relu, with_res, torch.float32, mask_y=lo["y"].float())
    for k in ("y", "dx") + (("dres",) if with_res else ()):
        assert lo[k].dtype == BF and hi[k].dtype == torch.float32, (tag, k)
    for k in ("saved", "rm", "rv", "dgamma", "dbeta"):
        assert lo[k].dtype == torch.float32 and _same_bits(lo[k], hi[k]), (tag, k, float((lo[k] - hi[k]).abs().max()))
    assert lo["nbt"].dtype == torch.int64 and int(lo["nbt"]) == int(hi["nbt"]) == 1, tag
    assert _same_bits(lo["y"], hi["y"].to(BF)), (tag, "y", int((_bits(lo["y"]) != _bits(hi["y"].to(BF))).sum()))
    assert _same_bits(lo["dx"], hi["dx"].to(BF)), (tag, "dx", int((_bits(lo["dx"]) != _bits(hi["dx"].to(BF))).sum()))
    if relu:
        assert torch.count_nonzero(lo["y"][:, DEAD_CH]) == 0, (tag, "the dead channel must be all zero after the ReLU")
    if with_res:
        want = torch.where(lo["y"] > 0, t["dy"], torch.zeros_like(t["dy"])) if relu else t["dy"]
        assert _same_bits(lo["dres"], want), (tag, "d_residual")


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 32, 64, 128])
@pytest.mark.parametrize("n_of", [lambda P: 2, lambda P: 63, lambda P: P - 1, lambda P: P, lambda P: P + 1, lambda P: 3 * P + 17],
                         ids=["2", "63", "P-1", "P", "P+1", "3P+17"])
def test_bf16_kernels_are_the_fp32_kernels_rounded_once(hip, n_of, C):
    n = n_of(_P())
    for which, offset, _ in INPUTS:
        d = _inputs(n * 1000 + C + (1 if offset else 0), n, C, offset)
        for name, relu, with_res in FORMS:
            _check_bf16_is_fp32_rounded_once(hip, d, relu, with_res, "(%s) n=%d C=%d %s" % (which, n, C, name))


# two chunks per group, a last group of two chunks, a last chunk of one row; apply workgroups of 2 P rows
LARGE = [(lambda P: 256 * P + P + 1, "256P+P+1"), (lambda P: 512 * P + 1, "512P+1")]


@pytest.mark.parametrize("which,offset,gate", INPUTS, ids=[i[0] for i in INPUTS])
@pytest.mark.parametrize("C", [16, 128])
@pytest.mark.parametrize("n_of", [l[0] for l in LARGE], ids=[l[1] for l in LARGE])
def test_bf16_kernels_are_the_fp32_kernels_rounded_once_at_large_n(hip, n_of, C, which, offset, gate):
    n = n_of(_P())
    d = _inputs(n + C + (1 if offset else 0), n, C, offset)
    _check_bf16_is_fp32_rounded_once(hip, d, True, True, "(%s) n=%d C=%d relu+residual" % (which, n, C))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,offset,gate", INPUTS, ids=[i[0] for i in INPUTS])
@pytest.mark.parametrize("C", [16, 128])
@pytest.mark.parametrize("n_of", [l[0] for l in LARGE], ids=[l[1] for l in LARGE])
def test_fp32_kernels_match_float64_at_large_n(hip, n_of, C, which, offset, gate):
    """the fp32 kernels beyond one chunk per group, at the existing file's gates: with test 1 this ties the bf16 form to float64"""
    n = n_of(_P())
    d = _inputs(n + C + (1 if offset else 0), n, C, offset)
    _check_against_float64(hip, d, True, True, gate, "(%s) fp32 n=%d C=%d relu+residual" % (which, n, C))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _gate_rounded(name, got, ref, gate):
    """|got - ref| <= 2^-8 |ref| + gate * max |ref|: one rounding to bf16 on top of the fp32 gate"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-30)
    excess = float(((np.abs(got - ref) - U * np.abs(ref)) / scale).max())
    report("sparse bn bf16 " + name + " (beyond 2^-8 |ref|, / max |ref|)", excess, gate)
    assert np.isfinite(got).all() and excess <= gate, "%s: |got - ref| - 2^-8 |ref| = %.3e of the largest reference value > %.1e" % (name, excess, gate)


@pytest.mark.parametrize("C", [16, 32, 64, 128])
def test_bf16_path_matches_float64(hip, C):
    n, momentum = 3 * _P() + 17, 0.1
    for which, offset, gate in INPUTS:
        d = _inputs(n * 1000 + C + (1 if offset else 0), n, C, offset)
        t = _device_inputs(d)
        r = {k: (t[k].float().cpu().numpy() if k in ROW_KEYS else d[k]) for k in d}  # the reference sees the rounded rows
        for name, relu, with_res in FORMS:
            tag = "(%s) n=%d C=%d %s" % (which, n, C, name)
            out = {k: v.float().cpu().numpy() if v.dtype == BF else v.cpu().numpy() for k, v in _run(hip, t, relu, with_res, BF, momentum).items()}
            y, pre, mean, var, invstd = _ref_forward(r["x"], r["gamma"], r["beta"], r["res"] if with_res else None, relu)
            if relu:
                assert (pre[:, DEAD_CH] < 0).all() and (out["y"][:, DEAD_CH] == 0).all(), "the dead channel must be all zero after the ReLU"
            _gate_rounded(tag + " y", out["y"], y, gate)
            _gate("bf16 " + tag + " saved mean", out["saved"][0], mean, gate)
            _gate("bf16 " + tag + " saved invstd", out["saved"][1], invstd, gate)
            _gate("bf16 " + tag + " running_mean", out["rm"], (1 - momentum) * r["rm"].astype(np.float64) + momentum * mean, gate)
            _gate("bf16 " + tag + " running_var", out["rv"], (1 - momentum) * r["rv"].astype(np.float64) + momentum * var * n / (n - 1), gate)
            assert int(out["nbt"]) == 1
            dx, dgamma, dbeta, g = _ref_backward(r["dy"], r["x"], out["y"], r["gamma"], mean, invstd, relu)  # teacher-forced on the kernel's y
            _gate_rounded(tag + " dx", out["dx"], dx, gate)
            _gate("bf16 " + tag + " dgamma", out["dgamma"], dgamma, gate)
            _gate("bf16 " + tag + " dbeta", out["dbeta"], dbeta, gate)
            if with_res:
                assert np.array_equal(out["dres"], g), tag + ": d_residual is the masked dy, copied"


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 128])
def test_two_bf16_runs_are_bit_identical(hip, C):
    t = _device_inputs(_inputs(7, 3 * _P() + 17, C, 30.0))
    for name, relu, with_res in FORMS:
        a, b = _run(hip, t, relu, with_res, BF), _run(hip, t, relu, with_res, BF)
        assert set(a) == set(b)
        for k in a:
            assert _same_bits(a[k], b[k]), (name, k)


@pytest.mark.parametrize("C", [16, 64])
def test_bf16_row_count_from_the_device(hip, C):
    P = _P()
    cap, nv = 2 * P, P + 1
    d = _inputs(9, cap, C, 30.0)
    exact = _device_inputs({k: (v[:nv] if v.ndim == 2 else v) for k, v in d.items()})
    for k in ROW_KEYS:
        d[k][nv:] = np.nan  # a poisoned tail must reach no output and no statistic
    full = _device_inputs(d)
    assert bool(torch.isnan(full["x"][nv:]).all())
    n_dev = torch.tensor([nv], dtype=torch.int32, device=DEV)
    for name, relu, with_res in FORMS:
        a = _run(hip, full, relu, with_res, BF, n_dev=n_dev)
        b = _run(hip, exact, relu, with_res, BF)
        for k in a:
            if a[k].shape == (cap, C):
                assert a[k].dtype == BF and _same_bits(a[k][:nv].contiguous(), b[k]), (name, k)
                assert torch.count_nonzero(a[k][nv:]) == 0 and bool(torch.isfinite(a[k]).all()), (name, k, "tail")
            else:
                assert _same_bits(a[k], b[k]), (name, k)


def test_bf16_graph_capture_replays_the_eager_bits(hip):
    """forward + backward captured once: nothing in the calls allocates device memory outside torch's allocator or synchronises"""
    P = _P()
    n, C = 3 * P + 17, 64
    sets = [_device_inputs(_inputs(20 + i, n, C, 0.0)) for i in range(2)]
    eager = [_run(hip, t, True, True, BF) for t in sets]
    keys = ("x", "dy", "res", "gamma", "beta", "rm", "rv")
    st = {k: sets[0][k].clone() for k in keys}
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)

    def step():
        y, saved = hip.sparse_bn_train_forward(st["x"], st["gamma"], st["beta"], st["rm"], st["rv"], nbt, EPS, 0.1, residual=st["res"], relu=True)
        dx, dres, dgamma, dbeta = hip.sparse_bn_train_backward(st["dy"], st["x"], y, st["gamma"], saved, relu=True, want_residual=True)
        return dict(y=y, saved=saved, dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up: code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with hip.workspace.scope("test_sparse_bn_bf16_graph"):
        with torch.cuda.graph(graph):
            outs = step()
    try:
        for i in (0, 1, 0):
            for k in keys:
                st[k].copy_(sets[i][k])
            nbt.zero_()
            graph.replay()
            torch.cuda.synchronize()
            for k, v in outs.items():
                assert _same_bits(v, eager[i][k]), (i, k)
            assert _same_bits(st["rm"], eager[i]["rm"]) and _same_bits(st["rv"], eager[i]["rv"]) and int(nbt) == 1
        assert outs["y"].dtype == BF and not torch.equal(eager[0]["y"], eager[1]["y"])
    finally:
        del graph
        hip.workspace.release("test_sparse_bn_bf16_graph")


# 5, 6 ------------------------------------------------------------------------------------------------------------------------------
def _backbone(seed=5):
    from futuredet_amd.backbones import SpMiddleResNetFHD
    from futuredet_amd.synth import seeded_state_dict

    torch.manual_seed(0)
    bb = SpMiddleResNetFHD(num_input_features=5)
    bb.load_state_dict(seeded_state_dict(bb, seed), strict=False)
    return bb


@pytest.fixture(scope="module")
def cloud():
    """the ~4 000-point cloud of test_gpu_sparse_bn.py"""
    from test_gpu_spconv_grad_bf16 import _voxels

    cfg, v, c, n = _voxels(3, 4000)
    feats = torch.from_numpy(v[:, :, :5].sum(1) / n[:, None].astype(np.float32))
    coords = np.pad(c, ((0, 0), (1, 0))).astype(np.int32)
    return feats, coords, np.array([1440, 1440, 40])


def _record_bn_calls(spconv, seen):
    """patches _SparseBatchNormFunction.apply to record what every call met (the module's statistics before the call included) and the
    gradients on both of its sides; returns the undo"""
    orig = spconv._SparseBatchNormFunction.apply

    def recording(x, gamma, beta, residual, bn, relu):
        rec = dict(x=x.detach(), gamma=gamma.detach().clone(), beta=beta.detach().clone(), res=None if residual is None else residual.detach(),
                   relu=relu, bn=bn, rm0=bn.running_mean.clone(), rv0=bn.running_var.clone())
        if x.requires_grad:  # x is the convolution's output and has no other reader: its gradient is this call's dx
            x.register_hook(lambda g: rec.__setitem__("dx", g.detach().clone()))
        out = orig(x, gamma, beta, residual, bn, relu)
        rec.update(y=out.detach(), rm1=bn.running_mean.clone(), rv1=bn.running_var.clone())
        out.register_hook(lambda g: rec.__setitem__("dy", g.detach().clone()))
        seen.append(rec)
        return out

    spconv._SparseBatchNormFunction.apply = recording
    return lambda: setattr(spconv._SparseBatchNormFunction, "apply", orig)


@pytest.fixture(scope="module")
def fused_run(hip, cloud):
    """One forward + backward of SpMiddleResNetFHD with train_dtype = bf16 and fused_bn on the cloud, every fused call recorded."""
    from futuredet_amd import sparse as spconv

    feats, coords, input_shape = cloud
    bb = _backbone()
    ref_bb = copy.deepcopy(bb)
    bb = bb.to(DEV).train()
    bb.train_dtype = BF
    bb.fused_bn = True
    before = {k: t.detach().clone() for k, t in bb.named_buffers()}
    seen = []
    undo = _record_bn_calls(spconv, seen)
    try:
        bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
        rng = np.random.default_rng(9)
        G = torch.from_numpy(rng.uniform(-1, 1, tuple(bev.shape)).astype(np.float32))
        (bev * G.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        undo()
    return dict(bb=bb, ref_bb=ref_bb, bev=bev, G=G, seen=seen, before=before)


def test_switch_off_keeps_the_torch_chain_in_mixed_precision(hip, cloud):
    from futuredet_amd import sparse as spconv

    feats, coords, input_shape = cloud
    bb = _backbone().to(DEV).train()
    bb.train_dtype = BF
    assert bb.fused_bn is False
    seen = []
    undo = _record_bn_calls(spconv, seen)
    try:
        bev, _ = bb(feats.to(DEV), torch.from_numpy(coords).to(DEV), 1, input_shape)
        bev.sum().backward()
        torch.cuda.synchronize()
    finally:
        undo()
    assert len(seen) == 0 and bev.dtype == torch.float32
    assert all(int(b) == 1 for k, b in bb.named_buffers() if k.endswith("num_batches_tracked"))


def test_inside_the_mixed_precision_backbone(hip, fused_run):
    """fused_bn = True with bf16 rows: 21 fused calls, all on bf16 rows, each bit-equal to the fp32 kernels on the widened rows, rounded once"""
    seen, bb = fused_run["seen"], fused_run["bb"]
    assert len(seen) == 21 and sum(r["res"] is not None for r in seen) == 8 and all(r["relu"] for r in seen)
    assert fused_run["bev"].dtype == torch.float32  # the neck gets an fp32 map
    for i, r in enumerate(seen):
        n, C = r["x"].shape
        tag = "bf16 backbone call %d (n=%d C=%d%s)" % (i, n, C, " +res" if r["res"] is not None else "")
        assert n >= 2 and "dy" in r and "dx" in r, tag
        assert r["x"].dtype == BF and r["y"].dtype == BF and (r["res"] is None or r["res"].dtype == BF), tag
        assert r["dx"].dtype == BF and r["dx"].shape == r["x"].shape, tag
        assert r["gamma"].dtype == torch.float32 and r["rm1"].dtype == torch.float32, tag
        # the same call through the fp32 kernels on the widened rows
        rm, rv = r["rm0"].clone(), r["rv0"].clone()
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        res32 = None if r["res"] is None else r["res"].float()
        y32, saved = hip.sparse_bn_train_forward(r["x"].float(), r["gamma"], r["beta"], rm, rv, nbt, r["bn"].eps, r["bn"].momentum, residual=res32,
                                                 relu=True)
        assert _same_bits(r["y"], y32.to(BF)), tag + " y"
        assert _same_bits(r["rm1"], rm) and _same_bits(r["rv1"], rv), tag + " running statistics"
        dy = r["dy"].to(BF)  # what the function's backward makes of the gradient that reaches it
        dx32, dres32, dgamma, dbeta = hip.sparse_bn_train_backward(dy.float(), r["x"].float(), r["y"].float(), r["gamma"], saved, relu=True,
                                                                   want_residual=res32 is not None)
        assert _same_bits(r["dx"], dx32.to(BF)), tag + " dx"
        assert _same_bits(r["bn"].weight.grad, dgamma) and _same_bits(r["bn"].bias.grad, dbeta), tag + " dgamma / dbeta"
        if res32 is not None:
            assert _same_bits(dres32.to(BF), torch.where(r["y"] > 0, dy, torch.zeros_like(dy))), tag + " d_residual"
    moved = 0
    for name, buf in bb.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            assert buf.dtype == torch.float32 and bool(torch.isfinite(buf).all()), name
            assert not torch.equal(buf, fused_run["before"][name]), name + " did not move"
            moved += 1
        elif name.endswith("num_batches_tracked"):
            assert int(buf) == 1, name
    assert moved == 2 * 21


def test_mixed_precision_fused_backbone_gradients_lie_within_twice_the_rounding_distance(hip, cloud, fused_run):
    """Both switches on, against the yardstick of test_gpu_spconv_grad_bf16: E(name) = the norm-wise distance between the float64
    restatement of the backbone and the same restatement with every convolution's rows, weights and output rounded to bf16, on this cloud,
    on the reference alone.  The fused path rounds where that restatement rounds -- a BatchNorm output rounded to bf16 is the next
    convolution's rounded input -- so the device must lie within 2 E(name) + 1e-2."""
    from test_gpu_spconv_grad_bf16 import _restated_backbone

    feats, coords, input_shape = cloud
    ref_bb, G = fused_run["ref_bb"], fused_run["G"]
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
    got = dict(fused_run["bb"].named_parameters())
    pure, rounded = ref_grads[False], ref_grads[True]
    worst, fails = None, []
    for name, ref in pure.items():
        assert got[name].grad is not None and got[name].grad.dtype == torch.float32 and bool(torch.isfinite(got[name].grad).all()), name
        if name.endswith("bias") and "bn" not in name and not name.endswith(".1.bias"):
            continue  # a convolution bias followed by training-mode BatchNorm: its exact gradient is 0, both sides are rounding noise
        norm = max(float(np.linalg.norm(ref)), 1e-30)
        E = float(np.linalg.norm(rounded[name] - ref)) / norm
        e = float(np.linalg.norm(got[name].grad.double().cpu().numpy() - ref)) / norm
        report("bf16 fused_bn backbone grad (norm-wise) " + name, e, 2 * E + 1e-2, "E %.3e" % E)
        if worst is None or e > worst[1]:
            worst = (name, e, E)
        if not e <= 2 * E + 1e-2:
            fails.append((name, e, E))
    report("bf16 fused_bn backbone grad (norm-wise) largest: " + worst[0], worst[1], 2 * worst[2] + 1e-2, "E %.3e" % worst[2])
    assert not fails, fails


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_mixed_precision_training_steps_end_to_end(hip):
    """forecast_n0 with train_dtype = bf16, fused_bn and fused_loss through solver.train_steps: finite losses, 42 fused calls, every
    parameter moves, same state-dict keys"""
    from futuredet_amd import build_detector, solver
    from futuredet_amd import sparse as spconv
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel
    from test_gpu_loss import _synthetic_gt

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    default_keys = list(net.state_dict())
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    assert net.backbone.fused_bn is False and net.bbox_head.fused_loss is False and net.backbone.train_dtype is torch.float32
    net = net.to(DEV)
    net.backbone.train_dtype = BF
    net.backbone.fused_bn = True
    net.bbox_head.fused_loss = True
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    v, c, n = points_to_voxel(synthetic_cloud(seed=1, target_points=4000), vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    calls = []
    orig = spconv._SparseBatchNormFunction.apply

    def counting(*a):
        calls.append(a[0].dtype)
        return orig(*a)

    spconv._SparseBatchNormFunction.apply = counting
    try:
        opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        losses = [float(sum(out["loss"]).detach()) for out in solver.train_steps(net, [ex, ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2))]
    finally:
        spconv._SparseBatchNormFunction.apply = orig
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert len(calls) == 42 and all(dt == BF for dt in calls), "every BatchNorm of the backbone goes through the fused bf16 kernels, in both steps"
    for k, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if p.requires_grad:
            assert not torch.equal(p.detach(), before[k]), "parameter %s did not move" % k
    assert list(net.state_dict()) == default_keys
