"""-m gpu: the global augmentation -- fd_augment_points, fd_augment_boxes (csrc/fd_augment.hip), augment.GlobalAugment and the ``augment``
keyword of solver.StaticTrainStep / StaticPillarsTrainStep.

Exactness rules used below.
  * The kernels against tests/augment_ref.py: the same bits (the same IEEE operations in the same order, no contraction).
  * The kernels against the reference's recorded outputs (tests/golden/augment.npz): the same bits everywhere but in the rotated
    quantities, which lie within 4 * 2^-24 * M, M = scale (|x| + |y|) + |t| + |result| (derivation: test_augment_host.py).
  * A step with ``augment`` against the plain step: the same launches behind the loaded batch, so the same bits -- with torch's own
    convolutions (MIOpen) held to their deterministic algorithms, since by default they do not repeat their own bits from run to run.
    The step tests run on grids no other test uses (768 x 768 x 40 for the VoxelNet, 256 x 256 for PointPillars): torch keeps a shape's
    kernel choice for the rest of the process."""
import numpy as np
import pytest
import torch

import augment_ref as ar

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False))
POISON = -12345.5
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _params(flips, rot, seed=0):
    r = np.random.default_rng(seed)
    return np.array([flips[0], flips[1], rot, r.uniform(0.9, 1.1), r.normal(0, 0.5), r.normal(0, 0.5), r.normal(0, 0.5)], np.float64)


def _rec(params):
    from futuredet_amd.augment import GlobalAugment

    return GlobalAugment.record(np.atleast_2d(params), device=DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


@pytest.fixture(scope="module")
def clouds():
    """one seeded source cloud per ndim, 1000 rows: xyz across the shipped range, integer-valued intensity, a time column"""
    r = np.random.default_rng(7)
    out = {}
    for ndim in (4, 5):
        c = np.zeros((1000, ndim), np.float32)
        c[:, 0:2] = r.uniform(-54, 54, (1000, 2))
        c[:, 2] = r.uniform(-5, 3, 1000)
        c[:, 3] = r.integers(0, 256, 1000)
        if ndim == 5:
            c[:, 4] = r.integers(0, 10, 1000) * 0.05
        c[3, :3] = (-0.0, 0.0, -0.0)
        out[ndim] = c
    return out


def _perms(n):
    from futuredet_amd.augment import reference_permutation

    return {"none": None, "identity": np.arange(n, dtype=np.int32), "reference": reference_permutation(n),
            "reversed": np.arange(n, dtype=np.int32)[::-1].copy()}


@pytest.mark.parametrize("ndim", [4, 5])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_points_bit_for_bit(hip, clouds, ndim, n):
    src_np = clouds[ndim][:n]
    src = torch.from_numpy(src_np.copy()).to(DEV)
    cases = [(f, rot) for f in FLIPS for rot in (0.0, 0.6137)] + [((1, 0), -0.785)]
    for flips, rot in cases:
        p = _params(flips, rot, seed=n + 3 * flips[0] + flips[1])
        rec = _rec(p)
        got = {}
        for name, perm in _perms(n).items():
            dst = torch.full((1024, ndim), POISON, dtype=torch.float32, device=DEV)
            perm_t = None if perm is None else torch.from_numpy(perm.copy()).to(DEV)
            out = hip.augment_points(src, rec[0], dst, perm=perm_t)
            assert out is dst
            want = ar.points(src_np, p, perm)
            assert np.array_equal(_bits(dst[:n]), want.view(np.int32)), (ndim, n, flips, rot, name)
            assert bool((dst[n:] == POISON).all()), "rows at or past n_rows are not written"
            if n:
                srcrows = src_np if perm is None else src_np[perm]
                assert np.array_equal(_bits(dst[:n, 3:]), srcrows[:, 3:].view(np.int32)), "columns 3 and up pass through"
            got[name] = dst
        assert torch.equal(got["identity"].view(torch.int32), got["none"].view(torch.int32))
    # src is untouched
    assert np.array_equal(_bits(src), src_np.view(np.int32))


@pytest.mark.parametrize("ndim", [4, 5])
def test_points_n_rows_misaligned_buffers_and_a_bad_permutation(hip, clouds, ndim):
    """n_rows below the buffer's rows; views that start 4 bytes into their storage (the 16-byte accesses are not taken); a permutation
    entry outside [0, n): that row is left alone, nothing is read out of bounds"""
    src_np = clouds[ndim]
    p = _params((1, 1), 0.3, seed=5)
    rec = _rec(p)
    src = torch.from_numpy(src_np).to(DEV)
    dst = torch.full((1024, ndim), POISON, dtype=torch.float32, device=DEV)
    hip.augment_points(src, rec[0], dst, n_rows=130)
    assert np.array_equal(_bits(dst[:130]), ar.points(src_np[:130], p).view(np.int32)) and bool((dst[130:] == POISON).all())
    for perm in (None, np.arange(257, dtype=np.int32)[::-1].copy()):
        flat_s = torch.zeros(257 * ndim + 1, device=DEV)
        flat_s[1:] = src[:257].flatten()
        flat_d = torch.full((300 * ndim + 1,), POISON, device=DEV)
        s, d = flat_s[1:].view(257, ndim), flat_d[1:].view(300, ndim)
        assert s.data_ptr() % 16 == 4 and d.data_ptr() % 16 == 4
        hip.augment_points(s, rec[0], d, perm=None if perm is None else torch.from_numpy(perm).to(DEV))
        assert np.array_equal(_bits(d[:257]), ar.points(src_np[:257], p, perm).view(np.int32))
        assert bool((d[257:] == POISON).all()) and float(flat_d[0]) == POISON
    bad = np.arange(65, dtype=np.int32)
    bad[7], bad[20] = 65, -1
    dst.fill_(POISON)
    hip.augment_points(src[:65].contiguous(), rec[0], dst, perm=torch.from_numpy(bad).to(DEV))
    want = ar.points(src_np[:65], p)
    keep = np.ones(65, bool)
    keep[[7, 20]] = False
    assert np.array_equal(_bits(dst[:65])[keep], want.view(np.int32)[keep]) and bool((dst[[7, 20]] == POISON).all())
    with pytest.raises(hip.FutureDetHipError, match="distinct"):
        hip.augment_points(src, rec[0], src)


def test_front_end_refusals(hip):
    E = hip.FutureDetHipError
    rec = _rec(_params((0, 0), 0.0))
    src, dst = torch.zeros((8, 5), device=DEV), torch.zeros((8, 5), device=DEV)
    perm = torch.arange(8, dtype=torch.int32, device=DEV)
    hip.augment_points(src, rec[0], dst, perm=perm)
    for kw, text in ((dict(src=src.double()), "float32"), (dict(src=torch.zeros((8, 10), device=DEV)[:, ::2]), "contiguous"),
                     (dict(src=torch.zeros((8, 3), device=DEV), dst=torch.zeros((8, 3), device=DEV)), r"\[n, 4\] or \[n, 5\]"),
                     (dict(dst=torch.zeros((8, 4), device=DEV)), "one width"), (dict(dst=torch.zeros((7, 5), device=DEV)), "does not fit"),
                     (dict(n_rows=9), "does not fit"), (dict(rec=rec), None), (dict(rec=rec[0].float()), "float64"),
                     (dict(rec=torch.zeros(5, dtype=torch.float64, device=DEV)), "record"), (dict(perm=perm.long()), "int32"),
                     (dict(perm=perm[:7]), "at least n_rows"), (dict(perm=perm.cpu()), "HIP device")):
        a = dict(src=src, rec=rec[0], dst=dst, perm=perm, n_rows=None)
        a.update(kw)
        if text is None:  # a [1, 6] record is one record
            hip.augment_points(a["src"], a["rec"], a["dst"], perm=a["perm"], n_rows=a["n_rows"])
            continue
        with pytest.raises(E, match=text):
            hip.augment_points(a["src"], a["rec"], a["dst"], perm=a["perm"], n_rows=a["n_rows"])
    boxes, counts = torch.zeros((2, 3, 5, 12), device=DEV), torch.zeros((2, 3), dtype=torch.int32, device=DEV)
    recs = _rec(np.stack([_params((0, 0), 0.0)] * 2))
    hip.augment_boxes(boxes, counts, recs)
    for kw, text in ((dict(boxes=torch.zeros((2, 3, 5, 11), device=DEV)), "n_max, 12"), (dict(boxes=torch.zeros((6, 5, 12), device=DEV)), "n_max, 12"),
                     (dict(counts=counts.long()), "int32"), (dict(counts=counts[:1]), "counts must be"), (dict(recs=recs[:1]), "record"),
                     (dict(out=torch.zeros((2, 3, 4, 12), device=DEV)), "does not match"), (dict(boxes=boxes.double()), "float32")):
        a = dict(boxes=boxes, counts=counts, recs=recs, out=None)
        a.update(kw)
        with pytest.raises(E, match=text):
            hip.augment_boxes(a["boxes"], a["counts"], a["recs"], out=a["out"])


def _box_case(T, seed):
    r = np.random.default_rng(seed)
    B, n_max = 2, 5
    b = np.zeros((B, T, n_max, 12), np.float32)
    b[..., 0:2] = r.uniform(-54, 54, (B, T, n_max, 2))
    b[..., 2] = r.normal(0, 1, (B, T, n_max))
    b[..., 3:6] = r.uniform(0.5, 8.0, (B, T, n_max, 3))
    b[..., 6:10] = r.normal(0, 3, (B, T, n_max, 4))
    b[..., 10:12] = r.uniform(-3.2, 3.2, (B, T, n_max, 2))
    counts = r.choice([0, 3, 5], (B, T)).astype(np.int32)
    counts[0, 0], counts[1, T - 1] = 3, 5
    if T == 3:
        counts[0, 1] = 0
    return b, counts


@pytest.mark.parametrize("T", [1, 3])
def test_boxes_bit_for_bit(hip, T):
    b, counts = _box_case(T, 11 + T)
    ct = torch.from_numpy(counts).to(DEV)
    for flips in FLIPS:
        for rot in (0.0, -0.41):
            params = np.stack([_params(flips, rot, seed=1), _params(flips[::-1], rot * 0.5, seed=2)])
            recs = _rec(params)
            want = ar.boxes(b, counts, params)
            bt = torch.from_numpy(b.copy()).to(DEV)
            out = hip.augment_boxes(bt, ct, recs)
            assert np.array_equal(_bits(out), want.view(np.int32)), (T, flips, rot)
            assert np.array_equal(_bits(bt), b.view(np.int32)), "out of place: the input stays"
            again = hip.augment_boxes(bt, ct, recs, out=bt)
            assert again is bt and np.array_equal(_bits(bt), want.view(np.int32)), "in place"
            for bi in range(2):
                for ti in range(T):
                    assert np.array_equal(_bits(out[bi, ti, counts[bi, ti]:]), b[bi, ti, counts[bi, ti]:].view(np.int32)), "padding rows"


def test_kernels_against_the_reference_golden(hip, golden):
    g = golden("augment.npz")
    for name in [str(n) for n in g["names"]]:
        c = {k: g["%s/%s" % (name, k)] for k in ("points_in", "boxes_in", "flips", "rot", "scale", "trans", "points_out", "boxes_out")}
        p = np.array([c["flips"][0], c["flips"][1], c["rot"], c["scale"], *c["trans"]], np.float64)
        rec = _rec(p)
        pts = hip.augment_points(torch.from_numpy(c["points_in"]).to(DEV), rec[0], torch.empty((257, 5), device=DEV)).cpu().numpy()
        T, n = c["boxes_in"].shape[:2]
        boxes = hip.augment_boxes(torch.from_numpy(c["boxes_in"][None]).to(DEV), torch.full((1, T), n, dtype=torch.int32, device=DEV), rec)
        boxes = boxes.cpu().numpy()[0].reshape(-1, 12)
        b_in, b_out = c["boxes_in"].reshape(-1, 12), c["boxes_out"].reshape(-1, 12)
        exact_rot = float(c["rot"]) == 0.0
        assert np.array_equal(pts[:, 2:].view(np.int32), c["points_out"][:, 2:].view(np.int32)), name
        assert np.array_equal(boxes[:, [2, 3, 4, 5, 10, 11]].view(np.int32), b_out[:, [2, 3, 4, 5, 10, 11]].view(np.int32)), name
        pairs = [(pts[:, 0:2], c["points_out"][:, 0:2], c["points_in"][:, 0:2], c["trans"][:2])]
        pairs += [(boxes[:, [i, j]], b_out[:, [i, j]], b_in[:, [i, j]], c["trans"][:2] if i == 0 else (0.0, 0.0)) for i, j in ar.PAIRS]
        for got, ref, xy, t in pairs:
            if exact_rot:
                assert np.array_equal(got.view(np.int32), ref.view(np.int32)), name
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            assert (err <= ar.bound(xy, ref, p, t)).all(), (name, float(err.max()))


def test_determinism_across_two_runs(hip, clouds):
    from futuredet_amd.augment import reference_permutation

    p = _params((1, 0), 0.7, seed=9)
    rec = _rec(p)
    b, counts = _box_case(3, 4)
    recs = _rec(np.stack([p, _params((0, 1), -0.2, seed=8)]))
    runs = []
    for _ in range(2):
        outs = []
        for ndim in (4, 5):
            src = torch.from_numpy(clouds[ndim]).to(DEV)
            for perm in (None, torch.from_numpy(reference_permutation(1000).copy()).to(DEV)):
                outs.append(hip.augment_points(src, rec[0], torch.empty((1000, ndim), device=DEV), perm=perm))
        outs.append(hip.augment_boxes(torch.from_numpy(b).to(DEV), torch.from_numpy(counts).to(DEV), recs))
        runs.append(outs)
    for a, c in zip(*runs):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_graph_capture_and_replay_with_a_changed_record(hip, clouds):
    """both launches captured on one stream (a linear capture, no parallel branches); the record, the cloud and the boxes are static
    buffers whose contents change between replays"""
    from futuredet_amd.augment import reference_permutation

    src_np = clouds[5][:257]
    b, counts = _box_case(3, 21)
    perm = reference_permutation(257)
    src = torch.from_numpy(src_np).to(DEV)
    perm_t = torch.from_numpy(perm.copy()).to(DEV)
    boxes, ct = torch.from_numpy(b).to(DEV), torch.from_numpy(counts).to(DEV)
    recs = torch.zeros((2, 6), dtype=torch.float64, device=DEV)
    dst = torch.full((300, 5), POISON, device=DEV)
    out = torch.zeros_like(boxes)
    p0 = np.stack([_params((0, 0), 0.0, seed=1), _params((1, 1), 0.2, seed=2)])
    recs.copy_(_rec(p0))
    hip.augment_points(src, recs[0], dst, perm=perm_t)  # eager once: nothing is loaded for the first time inside the capture
    hip.augment_boxes(boxes, ct, recs, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            hip.augment_points(src, recs[0], dst, perm=perm_t)
            hip.augment_boxes(boxes, ct, recs, out=out)
    for seed, flips in ((3, (1, 0)), (4, (0, 1))):
        p = np.stack([_params(flips, 0.1 * seed, seed=seed), _params(flips[::-1], -0.1 * seed, seed=seed + 10)])
        recs.copy_(_rec(p))
        dst.fill_(POISON)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dst[:257]), ar.points(src_np, p[0], perm).view(np.int32)) and bool((dst[257:] == POISON).all())
        assert np.array_equal(_bits(out), ar.boxes(b, counts, p).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------- the steps
@pytest.fixture
def deterministic_convs():
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = before


@pytest.fixture(scope="module")
def world(hip):
    """test_gpu_train_static's forecast_n0 world on a 768 x 768 x 40 grid (a 96 x 96 map) of its own"""
    from futuredet_amd.targets import TargetAssigner
    from test_gpu_train_static import MAX_VOXELS, _World

    w = _World()
    w.vg = dict(w.vg, range=[-28.8, -28.8, -5.0, 28.8, 28.8, 3.0], max_voxel_num=[MAX_VOXELS, MAX_VOXELS])
    w.ta = TargetAssigner(w.cfg.train_cfg.assigner, np.array([768, 768, 40]), w.vg["range"], w.vg["voxel_size"])
    return w


@pytest.fixture(scope="module")
def pillars(hip):
    """test_gpu_pillars_static's PointPillars world on a 256 x 256 canvas of its own"""
    from futuredet_amd.targets import TargetAssigner
    from test_gpu_pillars_static import _Pillars

    w = _Pillars()
    rng = list(w.vg["range"])
    rng[0], rng[1], rng[3], rng[4] = -25.6, -25.6, 25.6, 25.6
    w.vg = dict(w.vg, range=rng)
    w.grid = np.array([256, 256, 1])
    w.ta = TargetAssigner(w.cfg.train_cfg.assigner, w.grid, w.vg["range"], w.vg["voxel_size"])
    return w


def _augment(**kw):
    from futuredet_amd.augment import GlobalAugment

    return GlobalAugment(dict(CFG, **kw), seed=3)


def test_no_synchronisation_in_the_augmented_step(world):
    from test_gpu_train_static import _flat

    world.fresh()
    step = world.step(2, augment=_augment())
    b1, b2 = world.batch([1, 2], [3000, 2000]), world.batch([3, 4], [2500, 4000])
    step.warm_up([b2])
    step(b1, check=False)  # first call: capacities uploaded, scratch allocated, the permutations of 3000 and 2000 rows uploaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(b2, check=False)
        first = step.last_aug_params.copy()
        out = step(b1, check=False)
        with pytest.raises(RuntimeError):
            out["loss"][0].item()  # the mode is enforced
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert step.iteration == 3 and not step.overflowed()
    assert step.last_aug_params.shape == (2, 7) and not np.array_equal(first, step.last_aug_params)
    assert all(bool(torch.isfinite(v).all()) for v in _flat(out).values())


def _run(w, batch, **kw):
    """one static step on ``batch`` from the seeded state: loss terms and the state after it"""
    from test_gpu_train_static import _flat

    w.fresh()
    step = w.step(len(batch["clouds"]), **kw)
    step.warm_up([batch])
    out = step(batch)
    torch.cuda.synchronize()
    assert not step.overflowed()
    return _flat(out), w.state(), step


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _step_equivalence(w, batch):
    from futuredet_amd.augment import identity_params

    B = len(batch["clouds"])
    l0, s0, _ = _run(w, batch)
    assert sum(float(v.sum()) for k, v in l0.items() if k.startswith("num_positive")) > 0, "no box on the small map"
    l1, s1, st = _run(w, dict(batch, aug_params=identity_params(B)), augment=_augment(shuffle_points=False))
    assert np.array_equal(st.last_aug_params, identity_params(B))
    _same(l0, l1, "identity: loss terms")
    _same(s0, s1, "identity: state")
    aug = _augment()
    params = aug.draw(B)
    assert params[:, 2].all() and (params[:, 3] != 1).all()
    l2, s2, st = _run(w, dict(batch, aug_params=params), augment=aug)
    assert np.array_equal(st.last_aug_params, params)
    pre = aug(batch, params)
    assert pre["gt_counts"] is batch["gt_counts"] and pre["gt_classes"] is batch["gt_classes"] and pre["clouds"][0] is not batch["clouds"][0]
    l3, s3, _ = _run(w, pre)
    _same(l2, l3, "drawn: loss terms")
    _same(s2, s3, "drawn: state")
    assert not all(torch.equal(l0[k], l2[k]) for k in l0), "the augmented batch is another batch"


def _pad_gt(batch, n):
    """the ground truth padded to n rows per timestep (counts unchanged), so that it fills the step's [B, T, max_gt, 12] buffer"""
    out = dict(batch)
    extra = n - batch["gt_boxes"].shape[2]
    out["gt_boxes"] = torch.nn.functional.pad(batch["gt_boxes"], (0, 0, 0, extra)).contiguous()
    for k in ("gt_classes", "gt_trajectory"):
        if k in batch:
            out[k] = torch.nn.functional.pad(batch[k], (0, extra)).contiguous()
    return out


def test_step_equivalence_voxelnet(world, deterministic_convs):
    """ground truth as wide as the step's buffer (max_gt = 32): fd_augment_boxes writes the static buffer directly"""
    batch = _pad_gt(world.batch([5], [4000]), 32)
    assert batch["gt_boxes"].shape[2] == 32 and int(batch["gt_counts"].max()) == 24
    _step_equivalence(world, batch)


def test_step_equivalence_pillars(pillars, deterministic_convs):
    """ground truth narrower than the buffer (24 of 32 rows): copied, then transformed in place"""
    _step_equivalence(pillars, pillars.batch([2], [6000]))


def test_bev_head_needs_params_and_a_warped_map(world):
    """(the refusal itself needs no device and is also in test_augment_host.py; here on a real step object)"""
    step = world.step(1, augment=_augment())
    step.bev = torch.zeros((1, 6, 4, 4), device=DEV)  # as a bev_map head's step holds it
    with pytest.raises(ValueError, match="aug_params"):
        step._load(dict(world.batch([1], [500]), bev_map=torch.zeros((1, 6, 4, 4), device=DEV)), 0)
