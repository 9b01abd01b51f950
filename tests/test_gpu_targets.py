"""-m gpu: AssignLabel's targets on the device (futuredet_amd/targets.py, csrc/fd_targets.hip) against the reference's own stage
(tests/golden/targets.npz, made by tests/golden/make_golden_targets.py), through TargetAssigner and the AssignLabel pipeline stage;
batch / graph / determinism properties; CenterHead.loss and a training step on device-made targets."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_loss as mgl  # noqa: E402
from futuredet_amd.config import ConfigDict  # noqa: E402
from futuredet_amd.targets import AssignLabel, TargetAssigner  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(HERE, "golden", "targets.npz"))
CASES = sorted({k.split("/")[0] for k in G.files if "/" in k})
GOOD = [c for c in CASES if c + "/raised" not in G.files]
TRAJ = ("static", "linear", "nonlinear")
EXACT_COLS = [0, 1, 2, 6, 7, 8, 9]    # ct - ct_int, z, velocities: bit-exact
ULP_COLS = [3, 4, 5, 10, 11, 12, 13]  # log(w, l, h), sin / cos of rot and rrot: numpy's float32 ufuncs against the device's


def _case(name):
    cfg = json.loads(str(G[name + "/cfg"]))
    geo = {k: G["%s/geo_%s" % (name, k)] for k in ("shape", "range", "size")}
    counts = G[name + "/counts"]
    off = np.concatenate([[0], np.cumsum(counts)])
    T = len(counts)
    sl = [slice(off[t], off[t + 1]) for t in range(T)]
    ann = dict(gt_boxes=[G[name + "/boxes"][s] for s in sl], gt_classes=[G[name + "/classes"][s].astype(np.int64) for s in sl],
               gt_names=[G[name + "/names"][s] for s in sl], gt_trajectory=[G[name + "/trajectory"][s] for s in sl])
    return cfg, geo, ann


def _padded(ann, n_max=None):
    T = len(ann["gt_boxes"])
    n_max = n_max or max([len(b) for b in ann["gt_boxes"]] + [1])
    boxes = np.zeros((1, T, n_max, 12), np.float32)
    counts = np.zeros((1, T), np.int32)
    classes = np.zeros((1, T, n_max), np.int32)
    traj = np.full((1, T, n_max), -1, np.int32)
    for t in range(T):
        n = len(ann["gt_boxes"][t])
        counts[0, t] = n
        boxes[0, t, :n] = ann["gt_boxes"][t]
        classes[0, t, :n] = ann["gt_classes"][t]
        traj[0, t, :n] = [TRAJ.index(str(x)) for x in ann["gt_trajectory"][t]]
    return boxes, counts, classes, traj


def _dev(*arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _ulps(a, b):
    ia = a.astype(np.float32).view(np.int32).astype(np.int64)
    ib = b.astype(np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _compare(name, got, worst):
    """got(key, t, u) -> numpy array of sample 0; every reference output of the case is compared."""
    for k in sorted(x for x in G.files if x.startswith(name + "/out/")):
        parts = k.split("/")
        key, t = parts[2], int(parts[3])
        want = G[k]
        if key.startswith("gt_boxes_and_cls"):
            g = got(key, t, None)
            assert g.dtype == want.dtype and g.shape == want.shape, (k, g.dtype, g.shape)
            assert np.array_equal(g.view(np.int32), want.view(np.int32)), (k, np.argwhere(g != want)[:5])
            continue
        u = int(parts[4])
        g = got(key, t, u)
        assert g.dtype == want.dtype and g.shape == want.shape, (k, g.dtype, want.dtype, g.shape, want.shape)
        if key.startswith("hm"):
            bad = np.argwhere(g.view(np.int32) != want.view(np.int32))
            if len(bad):
                rows = ["%s at %s: device %.17g reference %.17g (float64 of both)" % (k, tuple(i), float(g[tuple(i)]), float(want[tuple(i)]))
                        for i in bad[:8]]
                raise AssertionError("%d heat-map elements differ:\n%s" % (len(bad), "\n".join(rows)))
        elif key.startswith("anno_box"):
            assert np.array_equal(g[:, EXACT_COLS].view(np.int32), want[:, EXACT_COLS].view(np.int32)), \
                (k, np.argwhere(g[:, EXACT_COLS] != want[:, EXACT_COLS])[:5])
            d = int(_ulps(g[:, ULP_COLS], want[:, ULP_COLS]).max()) if len(g) else 0
            worst[0] = max(worst[0], d)
            assert d <= 2, (k, d)
        else:
            assert np.array_equal(g, want), (k, np.argwhere(g != want)[:5])


@pytest.mark.parametrize("name", GOOD)
def test_target_assigner_matches_the_reference(name):
    cfg, geo, ann = _case(name)
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    boxes, counts, classes, traj = _dev(*_padded(ann))
    ex = ta(boxes, counts, classes, traj if ta.extra_sets else None)
    torch.cuda.synchronize()

    def got(key, t, u):
        v = ex[key][t] if u is None else ex[key][t][u]
        return v[0].cpu().numpy()

    worst = [0]
    _compare(name, got, worst)
    print("%s: log / sin / cos columns within %d float32 ulp of numpy (numpy %s)" % (name, worst[0], str(G["numpy_version"])))


@pytest.mark.parametrize("name", GOOD)
def test_assign_label_stage_matches_the_reference(name):
    cfg, geo, ann = _case(name)
    res = dict(mode="train", type="NuScenesDataset", lidar=dict(annotations=ann, voxels=dict(geo)))
    res, _ = AssignLabel(cfg=ConfigDict(cfg))(res, None)
    tg = res["lidar"]["targets"]
    want_keys = {k.split("/")[2] for k in G.files if k.startswith(name + "/out/")}
    assert set(tg) == want_keys, (set(tg) ^ want_keys)

    def got(key, t, u):
        return tg[key][t] if u is None else tg[key][t][u]

    _compare(name, got, [0])


def test_over_max_objs_raises_assertion_error():
    name = "over_limit"
    assert str(G[name + "/raised"]) == "AssertionError"
    cfg, geo, ann = _case(name)
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    with pytest.raises(AssertionError, match="max_objs"):
        ta(*_dev(*_padded(ann)[:3]))
    res = dict(mode="train", type="NuScenesDataset", lidar=dict(annotations=ann, voxels=dict(geo)))
    with pytest.raises(AssertionError):
        AssignLabel(cfg=ConfigDict(cfg))(res, None)


def _batch_of_4(name="n3dtf"):
    cfg, geo, ann = _case(name)
    rng = np.random.default_rng(5)
    n_max = max(len(b) for b in ann["gt_boxes"])
    samples = []
    for k in range(4):
        a = {key: [np.copy(x) for x in v] for key, v in ann.items()}
        for t in range(len(a["gt_boxes"])):
            a["gt_boxes"][t][:, :2] += np.float32(0.37 * k)
            keep = rng.random(len(a["gt_boxes"][t])) > 0.2 * k
            for key in a:
                a[key][t] = a[key][t][keep]
        samples.append(_padded(a, n_max))
    return cfg, geo, [np.concatenate(x, 0) for x in zip(*samples)]


def test_a_batch_of_4_equals_4_single_calls():
    cfg, geo, arrays = _batch_of_4()
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    B, T = arrays[0].shape[:2]
    whole = ta.outputs(B, T, torch.device(DEV))
    ta(*_dev(*arrays), out=whole)
    for b in range(B):
        one = ta.outputs(1, T, torch.device(DEV))
        ta(*_dev(*[a[b:b + 1] for a in arrays]), out=one)
        exw, ex1 = ta.example(whole, B, T), ta.example(one, 1, T)
        for key, v in ex1.items():
            if key == "targets_status":
                assert torch.equal(exw[key][b:b + 1], v)
                continue
            for t in range(T):
                if key.startswith("gt_boxes_and_cls"):
                    assert torch.equal(exw[key][t][b:b + 1], v[t]), (key, b, t)
                else:
                    for u in range(len(v[t])):
                        assert torch.equal(exw[key][t][u][b:b + 1], v[t][u]), (key, b, t, u)


def test_graph_replay_with_new_boxes_equals_eager():
    cfg, geo, arrays = _batch_of_4()
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    B, T = arrays[0].shape[:2]
    static_in = _dev(*arrays)
    out = ta.outputs(B, T, torch.device(DEV))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ta(*static_in, out=out, check=False)  # warm-up on the capture stream: the workspace exists before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ta(*static_in, out=out, check=False)
    new = np.copy(arrays[0])
    new[..., 0] -= np.float32(1.3)
    new[..., 10] += np.float32(2.0)
    static_in[0].copy_(torch.from_numpy(new))
    g.replay()
    torch.cuda.synchronize()
    eager = ta.outputs(B, T, torch.device(DEV))
    ta(torch.from_numpy(new).to(DEV), *static_in[1:], out=eager)
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], eager[k]), k
    first = ta.outputs(B, T, torch.device(DEV))
    ta(*_dev(*arrays), out=first)
    assert not torch.equal(first["hm"], eager["hm"]), "the replay must see the new boxes"


def test_two_runs_are_identical():
    cfg, geo, arrays = _batch_of_4()
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    B, T = arrays[0].shape[:2]
    runs = []
    for _ in range(2):
        out = ta.outputs(B, T, torch.device(DEV))
        ta(*_dev(*arrays), out=out)
        runs.append(out)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("case,T,dense", [("n0_t7", 1, False), ("n3dtf", 7, True)])
def test_center_head_loss_on_device_targets_equals_loss_on_reference_targets(case, T, dense):
    from futuredet_amd import build_head

    cfg, geo, ann = _case(case)
    ta = TargetAssigner(ConfigDict(cfg), geo["shape"], geo["range"], geo["size"])
    boxes, counts, classes, traj = _dev(*_padded(ann))
    dev_ex = ta(boxes, counts, classes, traj if ta.extra_sets else None)
    ref_ex = {key: [[torch.from_numpy(G["%s/out/%s/%d/0" % (case, key, t)])[None].to(DEV)] for t in range(len(ann["gt_boxes"]))]
              for key in ("hm", "ind", "mask", "cat", "anno_box")}
    H, W = ta.H, ta.W
    rng = np.random.default_rng(3)
    head = build_head(dict(type="CenterHead", **mgl.head_kwargs(T, dense))).to(DEV)
    maps = []
    for t in range(T if dense else 1):
        m = {"hm": rng.normal(-1.0, 1.5, (1, 1, H, W))}
        for key, c in mgl.MAPS + (("vel", 2 if dense else 2 * T),):
            m[key] = rng.normal(0.0, 1.0, (1, c, H, W))
        maps.append({k: torch.from_numpy(v.astype(np.float32)).to(DEV) for k, v in m.items()})
    losses = []
    for ex in (dev_ex, ref_ex):
        preds = [{k: v.clone() for k, v in m.items()} for m in maps]
        ret = head.loss(ex, preds)
        losses.append(([float(x) for x in ret["loss"]], [float(x) for x in ret["hm_loss"]]))
    (dl, dh), (rl, rh) = losses
    assert dh == rh, (dh, rh)  # heat maps, ind, mask and cat are bit-exact
    np.testing.assert_allclose(dl, rl, rtol=2e-6, atol=0)
    assert all(np.isfinite(dl)) and any(h > 0 for h in dh)


def _synthetic_gt(rng, T, n):
    boxes = np.zeros((1, T, n, 12), np.float32)
    for t in range(T):
        b = boxes[0, t]
        b[:, 0:2] = rng.uniform(-40.0, 40.0, (n, 2)) + np.float32(0.5 * t)
        b[:, 2] = rng.normal(-0.5, 0.3, n)
        b[:, 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * rng.uniform(0.8, 1.2, (n, 3))
        b[:, 6:10] = rng.normal(0.0, 2.0, (n, 4))
        b[:, 10:12] = rng.uniform(-np.pi, np.pi, (n, 2))
    counts = np.full((1, T), n, np.int32)
    return boxes, counts, np.ones((1, T, n), np.int32), rng.integers(0, 3, (1, T, n)).astype(np.int32)


@pytest.mark.parametrize("variant", ["forecast_n0", "forecast_n3dtf"])
def test_training_step_on_device_targets(variant):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.voxelize import points_to_voxel

    cfg = centerpoint_config(variant)
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.to(DEV)
    pts = synthetic_cloud(seed=1, target_points=20000)
    cloud = [torch.from_numpy(pts).to(DEV)]

    def detect(model):
        model.eval()
        with torch.no_grad():
            r = model.forward_points(cloud, vg, padded=False)[0]
        torch.cuda.synchronize()
        return torch.cat([r["box3d_lidar"], r["scores"][:, None]], 1).cpu()

    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    boxes, counts, classes, traj = _dev(*_synthetic_gt(np.random.default_rng(2), cfg.timesteps, 24))
    targets = ta(boxes, counts, classes, traj if ta.extra_sets else None)
    assert int(sum(m[0].sum() for m in targets["mask"])) > 0
    v, c, n = points_to_voxel(pts, vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})

    before = detect(net)
    net.train()
    ret = net(ex, return_loss=True)
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
    assert before.shape != after.shape or not torch.equal(before, after), "one SGD step must change the detections"
