"""-m gpu: the bev-mask warp and the ground-truth range filter -- fd_augment_mask, fd_gt_range_filter (csrc/fd_augment_map.hip),
``GlobalAugment(warp_bev=True)``, ``augment.filter_gt_outside_range`` and the ``filter_gt`` keyword of solver.StaticTrainStep /
StaticPillarsTrainStep.

Exactness rules used below.
  * fd_augment_mask against tests/augment_map_ref.py: the same bits (the same IEEE operations in the same order, no contraction).
  * fd_gt_range_filter against tests/range_filter_ref.py and the reference's recorded masks (tests/golden/range_filter.npz): the same
    rows, counts and status.  The kernel takes fl32(sin(double(a))) where NumPy takes its own fp32 sine (within 1.5 ulp), so every box
    of these tests keeps each corner at least 1e-3 m from each boundary line -- 1000 times what such a difference can move a corner
    at 60 m -- or is one of the exact cases (angle 0, representable numbers), where both sines are exactly 0.
  * A step with the new switches against a step that is handed the batch prepared beforehand: the same launches behind the loaded
    batch, so the same bits -- with torch's own convolutions (MIOpen) held to their deterministic algorithms."""
import numpy as np
import pytest
import torch

import augment_map_ref as am
import range_filter_ref as rf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False))
H = W = 180
NUSC = (-54.0, -54.0, 54.0, 54.0)
MARGIN = 1e-3
ROTS = (0.0, np.pi / 2, -np.pi / 2, 0.3, -0.78539816)
SCALES = (0.9, 1.0, 1.1)
SHIFTS = ((0.0, 0.0), (3.0, -2.0), (0.5, 0.0), (-1.37, 2.81), (400.0, 0.0))
FLIPS = ((0, 0), (1, 0), (0, 1), (1, 1))


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.int32)


def _mrec(params):
    from futuredet_amd.augment import GlobalAugment

    return GlobalAugment.mask_record(np.atleast_2d(params), device=DEV)


# ------------------------------------------------------------------------------------------------------------------ fd_augment_mask
@pytest.fixture(scope="module")
def maps():
    """[3, 6, 180, 180]: random fp32 planes and 0/1 planes, alternating"""
    r = np.random.default_rng(11)
    m = r.random((3, 6, H, W), dtype=np.float32)
    m[:, 1::2] = (m[:, 1::2] < 0.5).astype(np.float32)
    return m


@pytest.fixture(scope="module")
def warp_cases():
    """every flip pair, angle, factor and shift of the issue at least once, in 20 parameter rows (a full product is 300 warps of a
    plane on the host); the restatement of a [180, 180] plane is computed once per (row, plane) and kept"""
    rows = []
    for i in range(20):
        f, rot, s, t = FLIPS[i % 4], ROTS[i % 5], SCALES[(i // 2) % 3], SHIFTS[(i // 4) % 5]
        rows.append([f[0], f[1], rot, s, t[0], t[1], 0.25 * i])
    rows = np.array(rows, np.float64)
    assert {tuple(r[:2]) for r in rows} == set(FLIPS) and set(rows[:, 2]) == set(ROTS) and set(rows[:, 3]) == set(SCALES)
    assert {tuple(r[4:6]) for r in rows} == set(SHIFTS)
    return rows


@pytest.mark.parametrize("B,C", [(1, 1), (1, 6), (3, 1), (3, 6)])
def test_mask_bit_for_bit(hip, maps, warp_cases, B, C):
    cache = test_mask_bit_for_bit.__dict__.setdefault("cache", {})

    def want(b, c, p):
        key = (b, c, p.tobytes())
        if key not in cache:
            cache[key] = am.get_mask_plane(maps[b, c], p)
        return cache[key]

    src_np = np.ascontiguousarray(maps[:B, :C])
    src = torch.from_numpy(src_np).to(DEV)
    for i in range(0, len(warp_cases), B):
        params = np.stack([warp_cases[(i + b) % len(warp_cases)] for b in range(B)])  # the records of one launch differ
        dst = torch.full((B, C, H, W), -7.5, device=DEV)
        out = hip.augment_mask(src, _mrec(params), out=dst)
        assert out is dst
        got = dst.cpu().numpy()
        for b in range(B):
            for c in range(C):
                assert np.array_equal(_bits(got[b, c]), _bits(want(b, c, params[b]))), (B, C, params[b].tolist(), c)
        assert np.array_equal(_bits(src), _bits(src_np)), "src stays"
    # (400, 0) moves everything out of the plane; the identity returns the input
    far = np.array([[0, 0, 0.0, 1.0, 400.0, 0.0, 0.0]] * B)
    assert not bool(hip.augment_mask(src, _mrec(far)).any())
    from futuredet_amd.augment import identity_params

    assert torch.equal(hip.augment_mask(src, _mrec(identity_params(B))).view(torch.int32), src.view(torch.int32))


def test_mask_refusals_and_other_plane_sizes(hip, maps):
    """dst == src and the front end's shape / dtype refusals; a 33 x 47 plane (not the feature's size: the kernel takes any plane that
    fits LDS) against the restatement's warp with the same matrices"""
    from futuredet_amd.augment import MASK_RECORD_DTYPE

    E = hip.FutureDetHipError
    src = torch.from_numpy(maps[:1, :2].copy()).to(DEV)
    rec = _mrec([1, 0, 0.3, 1.1, -1.37, 2.81, 0])
    with pytest.raises(E, match="distinct"):
        hip.augment_mask(src, rec, out=src)
    for kw, text in ((dict(src=src.double()), "float32"), (dict(src=src[:, :, ::2]), "contiguous"), (dict(src=src[0]), r"\[B, C, H, W\]"),
                     (dict(recs=rec.float()), "float64"), (dict(recs=torch.zeros((2, 13), dtype=torch.float64, device=DEV)), "record"),
                     (dict(recs=torch.zeros((1, 6), dtype=torch.float64, device=DEV)), "record"),
                     (dict(out=torch.zeros((1, 2, H, W - 1), device=DEV)), "does not match"),
                     (dict(src=torch.zeros((1, 1, 256, 256), device=DEV)), "does not fit LDS")):
        a = dict(src=src, recs=rec, out=None)
        a.update(kw)
        with pytest.raises(E, match=text):
            hip.augment_mask(a["src"], a["recs"], out=a["out"])
    r = np.random.default_rng(5)
    small = r.random((2, 3, 33, 47), dtype=np.float32)
    recs = np.zeros((2,), MASK_RECORD_DTYPE)
    recs["flip_a"], recs["flip_b"] = [1, 0], [0, 1]
    recs["m1"] = [am.invert(am.rotation_matrix(20, 15, 25.0, 1.05)), am.invert(am.rotation_matrix(23, 16, -100.0, 0.8))]
    recs["m2"] = [am.invert([1, 0, 2.25, 0, 1, -1.5]), am.invert([1, 0, -0.75, 0, 1, 3.0])]
    hip.augment_mask_check(recs, 33, 47)
    got = hip.augment_mask(torch.from_numpy(small).to(DEV), torch.from_numpy(recs.view(np.float64).reshape(2, 13)).to(DEV)).cpu().numpy()
    for b in range(2):
        for c in range(3):
            p = small[b, c]
            p = p[:, ::-1] if recs["flip_a"][b] else p
            p = p[::-1] if recs["flip_b"][b] else p
            assert np.array_equal(_bits(got[b, c]), _bits(am.warp(am.warp(p, recs["m1"][b]), recs["m2"][b]))), (b, c)


def test_mask_graph_replay_with_changed_records(hip, maps):
    """one launch captured on one stream; the records and the map are static buffers whose contents change between replays"""
    src_np = maps[:2, :2].copy()
    src = torch.from_numpy(src_np).to(DEV)
    recs = torch.zeros((2, 13), dtype=torch.float64, device=DEV)
    dst = torch.zeros((2, 2, H, W), device=DEV)
    recs.copy_(_mrec(np.array([[0, 0, 0.0, 1.0, 0, 0, 0], [1, 1, 0.2, 0.95, 1.5, -0.5, 0]])))
    hip.augment_mask(src, recs, out=dst)  # eager once: nothing is configured for the first time inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hip.augment_mask(src, recs, out=dst)
    for k, params in enumerate((np.array([[1, 0, 0.3, 1.1, -1.37, 2.81, 0], [0, 1, -0.6, 0.9, 0.5, 0.0, 0]]),
                                np.array([[0, 1, -0.78539816, 1.0, 3.0, -2.0, 0], [0, 0, np.pi / 2, 1.1, 0.0, 0.0, 0]]))):
        recs.copy_(_mrec(params))
        if k == 1:
            src_np = np.ascontiguousarray(src_np[::-1])
            src.copy_(torch.from_numpy(src_np))
        dst.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dst), _bits(am.get_mask(src_np, params))), k


# --------------------------------------------------------------------------------------------------------------- fd_gt_range_filter
def _clear(boxes, rng):
    """bool [n]: every corner keeps the margin from every boundary line"""
    c = rf.corners(boxes).astype(np.float64)
    d = np.minimum.reduce([np.abs(c[..., 0] - rng[0]), np.abs(c[..., 0] - rng[2]), np.abs(c[..., 1] - rng[1]), np.abs(c[..., 1] - rng[3])])
    return d.min(axis=1) >= MARGIN


def _boxes(r, shape, spread=62.0):
    b = np.zeros(tuple(shape) + (12,), np.float32)
    b[..., 0:2] = r.uniform(-spread, spread, tuple(shape) + (2,))
    b[..., 2] = r.normal(0, 1, shape)
    b[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * r.uniform(0.5, 1.6, tuple(shape) + (3,))
    b[..., 6:10] = r.normal(0, 3, tuple(shape) + (4,))
    b[..., 10:12] = r.uniform(-3.2, 3.2, tuple(shape) + (2,))
    flat = b.reshape(-1, 12)
    bad = ~_clear(flat, NUSC)
    flat[bad, 0:2] = 0.25 * flat[bad, 0:2]  # (pulled well inside: at most 15.5 + 4 m from the centre)
    assert _clear(flat, NUSC).all()
    return b


def _filter_case(B, T, n_max, seed, counts_kind):
    r = np.random.default_rng(seed)
    boxes = _boxes(r, (B, T, n_max))
    classes = r.integers(1, 11, (B, T, n_max)).astype(np.int32)
    traj = r.integers(0, 3, (B, T, n_max)).astype(np.int32)
    if counts_kind == "full":
        counts = np.full((B, T), n_max, np.int32)
    elif counts_kind == "zero":
        counts = np.zeros((B, T), np.int32)
    elif counts_kind == "all_kept":
        counts = np.full((B, T), n_max, np.int32)
        boxes[:, 0, :, 0:2] *= 0.5
    elif counts_kind == "all_dropped":
        counts = np.full((B, T), n_max, np.int32)
        boxes[:, 0, :, 0] = 70.0 + np.abs(boxes[:, 0, :, 0])
    elif counts_kind == "partial":
        counts = np.repeat(r.integers(0, n_max + 1, (B, 1)), T, axis=1).astype(np.int32)
    else:  # "unequal": some timesteps hold fewer or more objects than timestep 0, one count is out of [0, n_max]
        counts = r.integers(0, n_max + 1, (B, T)).astype(np.int32)
        counts[0, 0] = max(1, n_max // 2)
        if T > 1:
            counts[0, T - 1] = n_max + 3
            counts[B - 1, 1] = -2
    return boxes, counts, classes, traj


def _check_filter(hip, boxes, counts, classes, traj, rng, inplace):
    want = rf.apply(boxes, counts, classes, traj, rng)
    t = [torch.from_numpy(a.copy()).to(DEV) if a is not None else None for a in (boxes, counts, classes, traj)]
    out = hip.gt_range_filter(t[0], t[1], t[2], rng, trajectory=t[3], out="inplace" if inplace else None)
    names = ("boxes", "counts", "classes", "trajectory", "status")
    for name, got, ref, src, orig in zip(names, out, want, t + [None], (boxes, counts, classes, traj, None)):
        if ref is None:
            assert got is None, name
            continue
        assert np.array_equal(_bits(got) if name == "boxes" else got.cpu().numpy(), _bits(ref) if name == "boxes" else ref), name
        if name != "status":
            assert (got is src) == inplace, name
            if not inplace:
                assert np.array_equal(src.cpu().numpy(), orig), "out of place: the input stays"
    return want


@pytest.mark.parametrize("n_max", [1, 63, 64, 65, 500])
@pytest.mark.parametrize("T", [1, 3, 7])
def test_range_filter_exact(hip, n_max, T):
    """B = 3 with a different mask per sample; every kind of count; trajectory given and NULL; in place and out of place"""
    seen_status = False
    for k, kind in enumerate(("full", "zero", "all_kept", "all_dropped", "partial", "unequal")):
        boxes, counts, classes, traj = _filter_case(3, T, n_max, 1000 * T + n_max + k, kind)
        for inplace in (False, True):
            for with_traj in (True, False):
                want = _check_filter(hip, boxes, counts, classes, traj if with_traj else None, NUSC, inplace)
        kept0 = want[1][:, 0]
        if kind == "all_kept":
            assert (kept0 == n_max).all() and np.array_equal(want[0], boxes)
        if kind in ("all_dropped", "zero"):
            assert not want[1].any() and not want[0].any()
        if kind == "full" and n_max >= 63:
            assert (0 < kept0).all() and (kept0 < n_max).all() and len({rf.mask(boxes[b, 0], NUSC).tobytes() for b in range(3)}) == 3
        if kind == "unequal" and T > 1:
            assert want[4][0] >= 1 and want[4].sum() == (counts != counts[:, :1]).sum()
            seen_status = True
    assert seen_status or T == 1


def test_range_filter_against_the_reference_golden(hip, golden):
    g = golden("range_filter.npz")
    for name in [str(n) for n in g["names"]]:
        boxes, rng, masks = g["%s/boxes" % name], [float(v) for v in g["%s/range" % name]], g["%s/masks" % name]
        T, n = boxes.shape[:2]
        classes = np.arange(1, T * n + 1, dtype=np.int32).reshape(1, T, n)
        b, c, k, t, status = hip.gt_range_filter(torch.from_numpy(boxes[None]).to(DEV), torch.full((1, T), n, dtype=torch.int32, device=DEV),
                                                 torch.from_numpy(classes).to(DEV), rng)
        assert t is None and int(status[0]) == 0
        kept = int(masks[0].sum())
        assert c.cpu().tolist() == [[kept] * T], name
        for ti in range(T):  # the stage's _dict_select(gt_dict, mask), timestep by timestep
            assert np.array_equal(_bits(b[0, ti, :kept]), _bits(boxes[ti][masks[ti]])), (name, ti)
            assert np.array_equal(k[0, ti, :kept].cpu().numpy(), classes[0, ti][masks[ti]]), (name, ti)
            assert not bool(b[0, ti, kept:].any()) and not bool(k[0, ti, kept:].any()), "padding is zeros"


def test_range_filter_front_end(hip):
    E = hip.FutureDetHipError
    boxes = torch.zeros((2, 3, 5, 12), device=DEV)
    counts = torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    classes = torch.zeros((2, 3, 5), dtype=torch.int32, device=DEV)
    hip.gt_range_filter(boxes, counts, classes, NUSC)
    for kw, text in ((dict(boxes=boxes.double()), "float32"), (dict(boxes=torch.zeros((2, 3, 5, 11), device=DEV)), "n_max, 12"),
                     (dict(boxes=torch.zeros((2, 3, 0, 12), device=DEV)), "n_max, 12"), (dict(counts=counts.long()), "int32"),
                     (dict(counts=counts[:1]), "counts must be"), (dict(classes=classes[:, :, :4].contiguous()), "classes must be"),
                     (dict(trajectory=classes.long()), "int32"), (dict(pc_range=(0, 1, 2)), "pc_range"), (dict(pc_range=(5, 0, 5, 9)), "range"),
                     (dict(out="copy"), "out must be"), (dict(out=(boxes, counts, classes)), "out takes"),
                     (dict(out=(boxes[:1], counts, classes, None)), "does not match"), (dict(status=torch.zeros(3, dtype=torch.int32, device=DEV)), "status"),
                     (dict(boxes=torch.zeros((1, 1, 5000, 12), device=DEV), counts=counts[:1, :1].contiguous(),
                           classes=torch.zeros((1, 1, 5000), dtype=torch.int32, device=DEV)), "n_max")):
        a = dict(boxes=boxes, counts=counts, classes=classes, pc_range=NUSC, trajectory=None, out=None, status=None)
        a.update(kw)
        with pytest.raises(E, match=text):
            hip.gt_range_filter(a["boxes"], a["counts"], a["classes"], a["pc_range"], trajectory=a["trajectory"], out=a["out"], status=a["status"])


def test_range_filter_graph_replay(hip):
    boxes_np, counts_np, classes_np, traj_np = _filter_case(2, 3, 65, 77, "partial")
    src = [torch.from_numpy(a).to(DEV) for a in (boxes_np, counts_np, classes_np, traj_np)]
    work = [torch.zeros_like(t) for t in src]
    status = torch.zeros((2,), dtype=torch.int32, device=DEV)

    def launch():  # the step's form: the static rows in place, the counts from the batch's tensor into the step's
        hip.gt_range_filter(work[0], src[1], work[2], NUSC, trajectory=work[3], out=(work[0], work[1], work[2], work[3]), status=status)

    for w, s in zip(work, src):
        w.copy_(s)
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            launch()
    for seed in (78, 79):
        case = _filter_case(2, 3, 65, seed, "unequal" if seed == 79 else "partial")
        for w, s, a in zip(work, src, case):
            s.copy_(torch.from_numpy(a))
            w.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        want = rf.apply(*case, NUSC)
        assert np.array_equal(_bits(work[0]), _bits(want[0])) and np.array_equal(work[1].cpu().numpy(), want[1])
        assert np.array_equal(work[2].cpu().numpy(), want[2]) and np.array_equal(work[3].cpu().numpy(), want[3])
        assert np.array_equal(status.cpu().numpy(), want[4])


# ---------------------------------------------------------------------------------------------------------------------- the steps
@pytest.fixture
def deterministic_convs():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


MAX_VOXELS = 8192
NO_CLIP = None
SMALL = dict(grid=[768, 768, 40], range=[-28.8, -28.8, -5.0, 28.8, 28.8, 3.0])  # a 96 x 96 map, as test_gpu_augment's world
FULL = dict(grid=[1440, 1440, 40], range=None)  # the shipped 180 x 180 map: the only size the warp has


class _Net(object):
    """a shipped VoxelNet config with seeded weights, fused_bn and fused_loss on, and everything a step needs (the shape of
    test_gpu_train_static._World / test_gpu_pillars_static._MapWorld, for any variant and grid)"""

    def __init__(self, variant, grid, range):
        from futuredet_amd import build_detector, solver
        from futuredet_amd.configs import centerpoint_config
        from futuredet_amd.synth import seeded_state_dict, tame_box_dims
        from futuredet_amd.targets import TargetAssigner

        cfg = centerpoint_config(variant)
        self.cfg = cfg
        self.vg = dict(cfg.voxel_generator, max_voxel_num=[MAX_VOXELS, MAX_VOXELS])
        if range is not None:
            self.vg["range"] = list(range)
        net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
        net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
        self.net = net.to(DEV).train()
        self.net.backbone.fused_bn = True
        self.net.bbox_head.fused_loss = True
        self.state0 = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        self.ta = TargetAssigner(cfg.train_cfg.assigner, np.array(grid), self.vg["range"], self.vg["voxel_size"])
        self.opt = solver.build_one_cycle_optimizer(self.net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        self.sched = solver.create_learning_rate_scheduler(self.opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0,
                                                                        pct_start=0.4), 10)
        self.solver = solver

    def fresh(self):
        with torch.no_grad():
            for k, v in self.net.state_dict().items():
                v.copy_(self.state0[k])
            t = self.opt._table
            t.exp_avg.zero_(), t.exp_avg_sq.zero_(), t.step.zero_()
        self.net.train()

    def state(self):
        t = self.opt._table
        out = {k: v.detach().clone() for k, v in self.net.state_dict().items()}
        out.update({"opt.exp_avg": t.exp_avg.clone(), "opt.exp_avg_sq": t.exp_avg_sq.clone(), "opt.step": t.step.clone()})
        return out

    def batch(self, seed, points, reach):
        """one cloud; 24 objects per timestep whose centres lie within +-reach of the origin"""
        from futuredet_amd.synth import synthetic_cloud

        return _gt_batch(self, [torch.from_numpy(synthetic_cloud(seed=seed, target_points=points)).to(DEV)], seed, reach)

    def step(self, **kw):
        return self.solver.StaticTrainStep(self.net, self.vg, self.ta, self.opt, self.sched, NO_CLIP, capacity=8192, batch_size=1, max_gt=32, **kw)


def _gt_batch(w, clouds, seed, reach):
    r = np.random.default_rng(300 + seed)
    B, T, n = len(clouds), w.cfg.timesteps, 24
    rng = [w.vg["range"][i] for i in (0, 1, 3, 4)]
    boxes = np.zeros((B, T, n, 12), np.float32)
    boxes[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * r.uniform(0.8, 1.2, (B, T, n, 3))
    boxes[..., 2] = r.normal(-0.5, 0.3, (B, T, n))
    boxes[..., 6:10] = r.normal(0.0, 2.0, (B, T, n, 4))
    boxes[..., 10:12] = r.uniform(-np.pi, np.pi, (B, T, n, 2))
    first = boxes[:, 0].reshape(-1, 12)
    todo = np.ones(len(first), bool)
    while todo.any():  # rejection: every corner of the deciding timestep keeps the margin from the boundary lines
        first[todo, 0:2] = r.uniform(-reach, reach, (int(todo.sum()), 2))
        todo = ~_clear_of(first, rng)
    boxes[:, 0] = first.reshape(B, n, 12)
    boxes[:, 1:, :, 0:2] = boxes[:, :1, :, 0:2] + r.normal(0.0, 0.5, (B, T - 1, n, 2)).astype(np.float32)
    b = dict(clouds=clouds, gt_boxes=torch.from_numpy(boxes).to(DEV), gt_counts=torch.full((B, T), n, dtype=torch.int32, device=DEV),
             gt_classes=torch.ones((B, T, n), dtype=torch.int32, device=DEV))
    if w.ta.extra_sets:
        b["gt_trajectory"] = torch.from_numpy(r.integers(0, 3, (B, T, n)).astype(np.int32)).to(DEV)
    return b


def _clear_of(boxes, rng):
    c = rf.corners(boxes).astype(np.float64)
    d = np.minimum.reduce([np.abs(c[..., 0] - rng[0]), np.abs(c[..., 0] - rng[2]), np.abs(c[..., 1] - rng[1]), np.abs(c[..., 1] - rng[3])])
    return d.min(axis=1) >= MARGIN


def _host_filtered(batch, rng):
    """the batch with its ground truth filtered on the host by the restatement"""
    traj = batch.get("gt_trajectory")
    ob, oc, ok, ot, status = rf.apply(batch["gt_boxes"].cpu().numpy(), batch["gt_counts"].cpu().numpy(), batch["gt_classes"].cpu().numpy(),
                                      traj.cpu().numpy() if traj is not None else None, rng)
    out = dict(batch, gt_boxes=torch.from_numpy(ob).to(DEV), gt_counts=torch.from_numpy(oc).to(DEV), gt_classes=torch.from_numpy(ok).to(DEV))
    if traj is not None:
        out["gt_trajectory"] = torch.from_numpy(ot).to(DEV)
    assert not status.any()
    return out


def _flat(losses):
    from test_gpu_train_static import _flat as flat

    return flat(losses)


def _run(w, batch, sync_free=False, **kw):
    """one static step on ``batch`` from the seeded state: loss terms, the state after it and the step.  ``sync_free``: a first call
    lets the step allocate and upload what it keeps, the state is put back, and the measured call runs under torch's sync debug mode.
    With explicit ``row_caps`` (those of an earlier step of the same world) the warm-up is left out: its other effects -- the
    convolutions' kernel choices, the optimiser's pointer table -- are the earlier step's."""
    import time

    t0 = time.perf_counter()
    w.fresh()
    step = w.step(**kw)
    if "row_caps" not in kw:
        step.warm_up([batch])
    if sync_free:
        step(batch, check=False)
        torch.cuda.synchronize()
        w.fresh()
        step.iteration = 0
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = step(batch, check=False)
            with pytest.raises(RuntimeError):
                out["loss"][0].item()  # the mode is enforced
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        out = step(batch)
    torch.cuda.synchronize()
    assert not step.overflowed()
    print("[augment_map] %s %s: %.2f s" % (step.name, sorted(kw), time.perf_counter() - t0))
    return _flat(out), w.state(), step


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _positives(losses):
    return sum(float(v.sum()) for k, v in losses.items() if k.startswith("num_positive"))


@pytest.fixture(scope="module")
def mapnet(hip):
    return _Net("forecast_n3dtfm", **FULL)


def test_warp_in_the_step(mapnet, deterministic_convs):
    """forecast_n3dtfm with warp_bev: the step draws, warps the batch's unwarped map into its static buffer -- without a host
    synchronisation -- and computes what a step computes that is handed the pre-warped map and the parameters.  (The warp exists at
    180 x 180 only, so this is the one test here on the full 1440 x 1440 grid: its first step pays MIOpen's search for the
    deterministic convolution algorithms at that size once per process, about 11 s; the second whole run takes 0.3 s.)"""
    from futuredet_amd.augment import GlobalAugment

    w = mapnet
    assert w.net.bbox_head.bev_map and (w.ta.H, w.ta.W) == (H, W)
    batch = w.batch(5, 4000, 40.0)
    g = torch.Generator(device="cpu").manual_seed(1)
    batch["bev_map"] = torch.rand((1, 6, H, W), generator=g).to(DEV)
    l1, s1, step = _run(w, batch, sync_free=True, augment=GlobalAugment(CFG, seed=3, warp_bev=True))
    params = step.last_aug_params.copy()
    assert params.shape == (1, 7) and params[0, 2] != 0 and params[0, 3] != 1 and params[0, 4] != 0
    want = am.get_mask(batch["bev_map"].cpu().numpy(), params)
    assert np.array_equal(_bits(step.bev), _bits(want)) and not torch.equal(step.bev, batch["bev_map"])
    assert _positives(l1) > 0
    # today's route: a plain augment, the parameters and a map somebody warped (here the library's own warp == the restatement)
    plain = GlobalAugment(CFG, seed=4)
    pre = dict(batch, aug_params=params, bev_map=GlobalAugment(CFG, seed=4, warp_bev=True).warp_map(batch["bev_map"], params))
    assert np.array_equal(_bits(pre["bev_map"]), _bits(want))
    l2, s2, step2 = _run(w, pre, augment=plain, row_caps=list(step.caps))
    assert np.array_equal(step2.last_aug_params, params)
    _same(l1, l2, "warp_bev: loss terms")
    _same(s1, s2, "warp_bev: state")
    # aug(batch) warps a copy for train_steps users; a step built for another map size is refused where it is built
    out = GlobalAugment(CFG, seed=4, warp_bev=True)(batch, params)
    assert np.array_equal(_bits(out["bev_map"]), _bits(want)) and out["bev_map"] is not batch["bev_map"]
    assert GlobalAugment(CFG, seed=4)(batch, params)["bev_map"] is batch["bev_map"]


def test_warp_step_refuses_another_map_size(hip):
    from futuredet_amd.augment import GlobalAugment

    w = _Net("forecast_n3dtfm", **SMALL)
    assert (w.ta.H, w.ta.W) == (96, 96)
    w.step(augment=GlobalAugment(CFG, seed=0))  # without the warp any map size is taken
    with pytest.raises(ValueError, match="180 x 180"):
        w.step(augment=GlobalAugment(CFG, seed=0, warp_bev=True))


def _filter_equivalence(w, batch_of, inside_too=True):
    from futuredet_amd.augment import filter_gt_outside_range

    rng = [w.vg["range"][i] for i in (0, 1, 3, 4)]
    if inside_too:
        inside = batch_of(0.7 * rng[2])   # every box wholly inside: centres within 70 % of the half width, boxes a few metres long
        keep = rf.mask(inside["gt_boxes"][0, 0].cpu().numpy(), rng)
        assert keep.all()
        l0, s0, _ = _run(w, inside)
        assert _positives(l0) > 0, "no box on the map"
        l1, s1, st = _run(w, inside, sync_free=True, filter_gt=True)
        assert torch.equal(st.gt_counts, inside["gt_counts"]) and not bool(st.gt_filter_status.any())
        _same(l0, l1, "nothing out of range: loss terms")
        _same(s0, s1, "nothing out of range: state")
    outside = batch_of(1.5 * rng[2])  # centres up to 1.5 half widths out: a good part of the boxes lies outside
    keep = rf.mask(outside["gt_boxes"][0, 0].cpu().numpy(), rng)
    assert 3 <= keep.sum() <= len(keep) - 3
    host = _host_filtered(outside, rng)
    dev = filter_gt_outside_range(outside, w.vg["range"])
    for k in ("gt_boxes", "gt_counts", "gt_classes") + (("gt_trajectory",) if "gt_trajectory" in outside else ()):
        assert torch.equal(dev[k], host[k]) and dev[k] is not outside[k], k
    assert dev["gt_counts"].is_cuda and int(dev["gt_counts"][0, 0]) == keep.sum() and not bool(dev["gt_filter_status"].any())
    l2, s2, st = _run(w, outside, filter_gt=True)
    assert torch.equal(st.gt_counts, host["gt_counts"]) and torch.equal(st.gt_boxes[:, :, :24], host["gt_boxes"])
    l3, s3, _ = _run(w, host)
    _same(l2, l3, "out of range: loss terms")
    _same(s2, s3, "out of range: state")
    assert _positives(l2) > 0, "no box on the map"


@pytest.mark.parametrize("variant", ["forecast_n0", "forecast_n3dtf"])
def test_filter_in_the_step(hip, deterministic_convs, variant):
    w = _Net(variant, **SMALL)
    _filter_equivalence(w, lambda reach: w.batch(5, 4000, reach))


def test_filter_in_the_pillars_step(hip, deterministic_convs):
    """StaticPillarsTrainStep with filter_gt against its host-filtered twin (test_gpu_augment's 256 x 256 PointPillars world)"""
    from futuredet_amd.synth import synthetic_cloud
    from futuredet_amd.targets import TargetAssigner
    from test_gpu_pillars_static import _Pillars

    w = _Pillars()
    rng = list(w.vg["range"])
    rng[0], rng[1], rng[3], rng[4] = -25.6, -25.6, 25.6, 25.6
    w.vg = dict(w.vg, range=rng)
    w.grid = np.array([256, 256, 1])
    w.ta = TargetAssigner(w.cfg.train_cfg.assigner, w.grid, w.vg["range"], w.vg["voxel_size"])
    step_of = w.step
    w.step = lambda **kw: step_of(1, **kw)
    cloud = torch.from_numpy(synthetic_cloud(seed=2, target_points=6000)).to(DEV)
    _filter_equivalence(w, lambda reach: _gt_batch(w, [cloud], 2, reach), inside_too=False)
