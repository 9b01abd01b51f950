"""-m gpu: GT-database sampling -- fd_gt_sample_select, fd_gt_sample_points (csrc/fd_gt_sample.hip), ``GlobalAugment(sampler=...)`` and
the sampling path of solver.StaticTrainStep / StaticPillarsTrainStep.

Every comparison is exact.  The kernels against tests/gt_sample_ref.py: the same IEEE operations in the same order (no contraction),
the sine and cosine taken in float64 on both sides; the random cases are drawn so that no pair of boxes is decided by the last bits
of those (gt_sample_ref.random_case).  The golden cases also carry the reference's own decisions (tests/golden/gt_sample.npz).  The
steps against ``aug(batch)``: the same launches on the same inputs."""
import types

import numpy as np
import pytest
import torch

import gt_sample_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False))
POISON = -12345.5
IPOISON = -777
CASES = ["chain_a", "chain_b", "groups", "angle_cols", "short_forecast", "trajectory", "full", "rate"]


def _database(db, names=None):
    from futuredet_amd.augment import GTDatabase

    return GTDatabase.from_arrays(db["boxes"], db["steps"], db["classes"], db["trajectory"], db["points"], db["offsets"], DEV, class_names=names)


def _bits(t):
    t = t.detach().cpu().numpy()
    return t.view(np.int32) if t.dtype == np.float32 else t


def _poisoned(boxes, counts, classes, traj):
    """the batch arrays [B, T, n_max, ...] with every row at or past its count poisoned"""
    boxes, classes = boxes.copy(), classes.copy()
    traj = traj.copy() if traj is not None else None
    for b in range(boxes.shape[0]):
        for t in range(boxes.shape[1]):
            c = int(np.clip(counts[b, t], 0, boxes.shape[2]))
            boxes[b, t, c:] = POISON
            classes[b, t, c:] = IPOISON
            if traj is not None:
                traj[b, t, c:] = IPOISON
    return boxes, classes, traj


def _check_select(hip, boxes, counts, classes, traj, db, cand, groups, rate, cap, dbdev=None):
    """fd_gt_sample_select on a batch (numpy, [B, ...]) in place and out of place against the restatement, poisoned tails included;
    returns the restatement's outputs"""
    boxes, classes, traj = _poisoned(boxes, counts, classes, traj)
    want = R.select(boxes, counts, classes, traj, db, cand, groups, rate, cap)
    dbdev = dbdev if dbdev is not None else _database(db)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None
    for mode in ("inplace", "out"):
        ins = [up(boxes), up(counts), up(classes), up(traj)]
        outs = None
        if mode == "out":
            outs = (torch.full_like(ins[0], POISON), torch.full_like(ins[1], IPOISON), torch.full_like(ins[2], IPOISON),
                    torch.full_like(ins[3], IPOISON) if traj is not None else None)
        res = hip.gt_sample_select(ins[0], ins[1], ins[2], dbdev, up(cand), groups, rate, cap, trajectory=ins[3],
                                   out="inplace" if mode == "inplace" else outs)
        assert np.array_equal(_bits(res["accepted"]), want["accepted"]), mode
        assert np.array_equal(_bits(res["status"]), want["status"]) and np.array_equal(_bits(res["n_points"]), want["n_points"]), mode
        assert np.array_equal(R.plan_words(_bits(res["plan"])), want["plan"]), mode
        assert np.array_equal(_bits(res["counts"]), want["counts"]), mode
        # the restatement's copies keep the (poisoned) input behind the new counts: equal everywhere = appended rows right, tails untouched
        assert np.array_equal(_bits(res["boxes"]), want["boxes"].view(np.int32)), mode
        assert np.array_equal(_bits(res["classes"]), want["classes"]), mode
        if traj is not None:
            assert np.array_equal(_bits(res["trajectory"]), want["trajectory"]), mode
        if mode == "inplace":
            assert res["boxes"] is ins[0] and res["counts"] is ins[1]
        else:
            assert np.array_equal(_bits(ins[0]), boxes.view(np.int32)) and np.array_equal(_bits(ins[1]), counts), "the inputs stay"
    return want


def _golden_batch(g, name):
    from test_gt_sample_host import golden_case

    boxes, counts, cls, tr, db, cand, groups, rate, cap = golden_case(g, name)
    return boxes[None], counts[None], cls[None], tr[None], db, cand[None], groups, rate, cap


@pytest.mark.parametrize("name", CASES)
def test_select_on_the_golden_cases(hip, golden, name):
    g = golden("gt_sample.npz")
    boxes, counts, cls, tr, db, cand, groups, rate, cap = _golden_batch(g, name)
    want = _check_select(hip, boxes, counts, cls, tr, db, cand, groups, rate, cap)
    assert np.array_equal(want["accepted"][0], g["%s/accepted" % name]), "the reference's own decisions"
    if all(gr[1] < 0 for gr in groups):  # a standard sampler never looks at the trajectory ids: NULL gives the same
        _check_select(hip, boxes, counts, cls, None, db, cand, groups, rate, cap)


@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("K", [1, 12, 64])
@pytest.mark.parametrize("n0", [0, 1, 63, 64, 65, 500])
def test_select_on_random_robust_cases(hip, n0, K, T):
    """two samples with one database: different ground truth, candidates in different orders; T = 1 runs without trajectory ids"""
    n_max = n0 + K + 3
    a = R.random_case(1000 * n0 + 10 * K + T, n0, K, T, n_max, with_trajectory=T > 1)
    boxes, counts, cls, tr, db, cand, groups = a
    r = np.random.default_rng(n0 + K)
    boxes2 = boxes.copy()
    boxes2[:, :n0] = boxes[:, :n0][:, r.permutation(n0)]
    cand2 = cand[::-1].copy()
    if K > 1:
        cand2[K // 2] = -1
    stack = lambda x, y: np.stack([x, y])
    want = _check_select(hip, stack(boxes, boxes2), stack(counts, counts), stack(cls, cls), stack(tr, tr) if tr is not None else None, db,
                         stack(cand, cand2), groups, 1.0, int(db["offsets"][-1]))
    if K >= 12 and n0 >= 63:
        assert 0 < want["accepted"][0].sum() < K, "a case that decides nothing"


def _limits_case():
    """four far-apart entries of 5, 9, 3 and 2 points, one group, one ground-truth object (test_gt_sample_host's closed-form case)"""
    M = 4
    dbb = np.zeros((M, 2, 12), np.float32)
    for e in range(M):
        dbb[e, :, :6] = (20.0 * e, 50.0, 0.0, 2.0, 4.0, 1.5)
        dbb[e, 1, 6:] = e + 1
    sizes = [5, 9, 3, 2]
    db = dict(boxes=dbb, steps=np.array([2, 1, 2, 2], np.int32), classes=np.full(M, 1, np.int32), trajectory=np.arange(M, dtype=np.int32) % 3,
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), points=np.arange(19 * 4, dtype=np.float32).reshape(19, 4))
    boxes, cls = np.zeros((1, 2, 6, 12), np.float32), np.zeros((1, 2, 6), np.int32)
    boxes[:, :, 0, :6] = (0, 0, 0, 2, 4, 1.5)
    cls[:, :, 0] = 1
    return db, boxes, np.array([[1, 1]], np.int32), cls


def test_select_limits_and_status_bits(hip):
    db, boxes, counts, cls = _limits_case()
    cand, groups = np.array([[0, 1, 2, 3]], np.int32), [(1, -1, 5, 0, 4)]
    dbdev = _database(db)
    run = lambda **kw: _check_select(hip, kw.get("boxes", boxes), kw.get("counts", counts), kw.get("cls", cls), None, db, kw.get("cand", cand),
                                     kw.get("groups", groups), kw.get("rate", 1.0), kw.get("cap", 100), dbdev=dbdev)
    w = run()
    assert list(w["accepted"][0]) == [1, 1, 1, 1] and w["status"][0] == 0 and w["n_points"][0] == 19
    w = run(cap=13)  # entry 1 (9 points) overflows point_cap by one point: rejected, the later smaller ones are accepted
    assert list(w["accepted"][0]) == [1, 0, 1, 1] and w["status"][0] == hip.GT_SAMPLE_NO_POINTS and w["n_points"][0] == 10
    w = run(cap=19)  # exactly filled
    assert list(w["accepted"][0]) == [1, 1, 1, 1] and w["status"][0] == 0
    w = run(boxes=boxes[:, :, :4].copy(), cls=cls[:, :, :4].copy())  # n_max overflows by one row
    assert list(w["accepted"][0]) == [1, 1, 1, 0] and w["status"][0] == hip.GT_SAMPLE_NO_ROW
    w = run(counts=np.array([[1, 2]], np.int32))
    assert w["status"][0] == hip.GT_SAMPLE_COUNTS_DIFFER and list(w["counts"][0]) == [5, 6]
    w = run(cand=np.array([[-1, 7, 2, -5]], np.int32))  # empty and out-of-range slots
    assert list(w["accepted"][0]) == [0, 0, 1, 0] and w["status"][0] == hip.GT_SAMPLE_BAD_INDEX
    w = run(groups=[(1, -1, 3, 0, 4)])
    assert list(w["accepted"][0]) == [1, 1, 0, 0]
    for rate, n in ((0.5, 2), (0.25, 1), (0.125, 0), (0.375, 2)):  # round half to even
        assert int(run(rate=rate)["accepted"][0].sum()) == n, rate


# ---------------------------------------------------------------------------------------------------------------------- the paste
SIZES = [0, 1, 63, 64, 65, 7, 0, 30]


def _paste_case(ndim, seed=5):
    r = np.random.default_rng(seed)
    M, P = len(SIZES), int(np.sum(SIZES))
    pts = np.zeros((P, ndim), np.float32)
    pts[:, :3] = r.uniform(-3, 3, (P, 3))
    pts[:, 3:] = r.integers(0, 256, (P, ndim - 3))
    dbb = np.zeros((M, 2, 12), np.float32)
    dbb[:, :, :3] = r.uniform(-50, 50, (M, 1, 3))
    dbb[:, 1, :3] += 100.0  # not the timestep the centre comes from
    return dict(boxes=dbb, steps=np.full(M, 2, np.int32), classes=np.ones(M, np.int32), trajectory=np.zeros(M, np.int32),
                offsets=np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64), points=pts)


def _plan32(plan):
    out = np.zeros((len(plan), 4), np.int32)
    out[:, :2] = plan[:, 0:1].astype(np.int64).view(np.int32).reshape(-1, 2)
    out[:, 2], out[:, 3] = plan[:, 1], plan[:, 2]
    return out


def _plan(db, cand, accepted):
    plan, run = np.zeros((len(cand), 3), np.int64), 0
    for i, e in enumerate(cand):
        n = int(db["offsets"][e + 1] - db["offsets"][e]) if accepted[i] else 0
        plan[i] = (db["offsets"][e] if accepted[i] else 0, n, run)
        run += n
    return plan, run


@pytest.mark.parametrize("ndim", [4, 5])
def test_points_bit_for_bit(hip, ndim):
    db = _paste_case(ndim)
    dbdev = _database(db)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    r = np.random.default_rng(ndim)
    picks = [(np.arange(8), np.ones(8, np.int32)), (np.array([4, 0, 2, -1, 3, 1]), np.array([1, 1, 0, 0, 1, 1], np.int32)),
             (np.array([5]), np.array([0], np.int32)), (r.permutation(8), r.integers(0, 2, 8).astype(np.int32))]
    for cand, acc in picks:
        cand = cand.astype(np.int32)
        acc = acc * (cand >= 0)
        plan, total = _plan(db, cand, acc)
        for cap in sorted({total, total + 1, total + 300}):  # exactly filled, one sentinel row, many (more than one block)
            want = R.paste(db, cand, acc, plan, cap)
            assert np.all(want[total:, :3] == np.float32(1e30)) and not want[total:, 3:].any()
            dst = torch.full((cap + 5, ndim), POISON, device=DEV)
            out = hip.gt_sample_points(dbdev, up(cand), up(acc), up(_plan32(plan)), dst, cap)
            assert out is dst and np.array_equal(_bits(dst[:cap]), want.view(np.int32)), (ndim, list(cand), cap)
            assert bool((dst[cap:] == POISON).all()), "rows at or past point_cap are not written"
            # misaligned bases: views that start 4 bytes into their storage
            flat_s = torch.zeros(db["points"].size + 1, device=DEV)
            flat_s[1:] = up(db["points"]).flatten()
            flat_d = torch.full(((cap + 5) * ndim + 1,), POISON, device=DEV)
            view = types.SimpleNamespace(boxes=dbdev.boxes, steps=dbdev.steps, classes=dbdev.classes, trajectory=dbdev.trajectory,
                                         offsets=dbdev.offsets, points=flat_s[1:].view(-1, ndim))
            d = flat_d[1:].view(cap + 5, ndim)
            assert view.points.data_ptr() % 16 == 4 and d.data_ptr() % 16 == 4
            hip.gt_sample_points(view, up(cand), up(acc), up(_plan32(plan)), d, cap)
            assert np.array_equal(_bits(d[:cap]), want.view(np.int32)) and bool((d[cap:] == POISON).all()) and float(flat_d[0]) == POISON
    # a plan that does not lie inside db_points: sentinels, nothing read out of bounds
    bad = np.array([[0, 5, 0], [int(db["offsets"][-1]) - 2, 3, 5], [-4, 2, 8]], np.int64)
    dst = torch.full((12, ndim), POISON, device=DEV)
    hip.gt_sample_points(dbdev, up(np.array([1, 2, 3], np.int32)), up(np.ones(3, np.int32)), up(_plan32(bad)), dst, 12)
    got = dst.cpu().numpy()
    assert np.array_equal(got[:5, 3:], db["points"][:5, 3:]) and np.all(got[5:, :3] == np.float32(1e30)) and not got[5:, 3:].any()


def test_both_kernels_in_one_graph_replayed_with_changed_candidates(hip):
    """a linear capture on one stream; the candidates are a static buffer whose contents change between replays"""
    boxes, counts, cls, tr, db, cand, groups = R.random_case(77, 65, 12, 3, 80)
    dbdev = _database(db)
    cap = 200
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    src = [up(boxes[None]), up(counts[None]), up(cls[None]), up(tr[None])]
    work = [torch.empty_like(t) for t in src]
    cand_t = up(cand[None])
    stage = torch.full((cap + 3, 5), POISON, device=DEV)
    rec = hip.gt_sample_groups(groups)

    def launches():
        for w, s in zip(work, src):
            w.copy_(s)
        res = hip.gt_sample_select(work[0], work[1], work[2], dbdev, cand_t, rec, 1.0, cap, trajectory=work[3], out="inplace",
                                   accepted=acc, plan=plan, n_points=n_pts, status=status)
        hip.gt_sample_points(dbdev, cand_t[0], acc[0], plan[0], stage, cap)
        return res

    i32 = dict(dtype=torch.int32, device=DEV)
    acc, plan, n_pts, status = torch.zeros((1, 12), **i32), torch.zeros((1, 12, 4), **i32), torch.zeros((1,), **i32), torch.zeros((1,), **i32)
    launches()  # eager once: nothing is loaded for the first time inside the capture
    torch.cuda.synchronize()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            launches()
    r = np.random.default_rng(0)
    for _ in range(2):
        c = r.permutation(len(db["boxes"]))[:12].astype(np.int32)
        c[r.integers(0, 12)] = -1
        cand_t.copy_(up(c[None]))
        stage.fill_(POISON)
        graph.replay()
        torch.cuda.synchronize()
        want = R.select_one(boxes, counts, cls, tr, db, c, groups, 1.0, cap)
        assert np.array_equal(_bits(acc[0]), want["accepted"]) and int(n_pts[0]) == want["n_points"] and int(status[0]) == want["status"]
        assert np.array_equal(_bits(work[0][0]), want["boxes"].view(np.int32)) and np.array_equal(_bits(work[1][0]), want["counts"])
        assert np.array_equal(_bits(stage[:cap]), R.paste(db, c, want["accepted"], want["plan"], cap).view(np.int32))
        assert bool((stage[cap:] == POISON).all())


def test_determinism_across_two_runs(hip):
    boxes, counts, cls, tr, db, cand, groups = R.random_case(5, 500, 64, 7, 600)
    dbdev = _database(db)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    runs = []
    for _ in range(2):
        res = hip.gt_sample_select(up(boxes[None]), up(counts[None]), up(cls[None]), dbdev, up(cand[None]), groups, 1.0, 400, trajectory=up(tr[None]),
                                   out="inplace")
        stage = torch.zeros((400, 5), device=DEV)
        hip.gt_sample_points(dbdev, up(cand), res["accepted"][0], res["plan"][0], stage, 400)
        runs.append([res[k] for k in ("boxes", "counts", "classes", "trajectory", "accepted", "plan", "n_points", "status")] + [stage])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---------------------------------------------------------------------------------------------------------------------- the sentinel
def _voxel_set(out):
    n = int(out["num_voxels"][0])
    coors = out["coors"][:n].cpu().numpy()
    order = np.lexsort(coors.T[::-1])
    num = out["num_points"][:n].cpu().numpy()[order]
    rows = [coors[order], num]
    if "mean" in out:
        rows.append(out["mean"][:n].cpu().numpy()[order])
    if "voxels" in out:  # the slots behind a voxel's count are not defined
        v = out["voxels"][:n].cpu().numpy()[order]
        v[np.arange(v.shape[1])[None, :] >= num[:, None]] = 0
        rows.append(v)
    return rows


@pytest.mark.parametrize("ndim", [4, 5])
def test_sentinel_rows_are_dropped_by_both_voxelisers(hip, ndim):
    """sentinel rows through fd_augment_points at the extreme of every transform range, then through fd_voxelize as the VoxelNet calls
    it (means, three coordinate columns) and as PointPillars does (point slots, four columns): the voxels of the cloud without them"""
    from futuredet_amd.augment import GlobalAugment
    from futuredet_amd.synth import synthetic_cloud

    scene = synthetic_cloud(seed=3, target_points=3000)[:, :ndim].copy()
    n, cap = len(scene), 777
    sent = np.zeros((cap, ndim), np.float32)
    sent[:, :3] = np.float32(1e30)
    both = torch.from_numpy(np.concatenate([sent, scene])).to(DEV)
    alone = torch.from_numpy(scene).to(DEV)
    voxelnet = dict(voxel_size=[0.075, 0.075, 0.2], coors_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], max_points=10, max_voxels=8192)
    pillars = dict(voxel_size=[0.2, 0.2, 8.0], coors_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], max_points=20, max_voxels=8192)
    for fa in (0, 1):
        for fb in (0, 1):
            for rot in (-0.785, 0.785, -np.pi / 4, np.pi / 4, 0.0):
                for scale in (0.9, 1.1):
                    for shift in (-2.5, 2.5):  # five standard deviations of the shipped 0.5
                        rec = GlobalAugment.record(np.array([[fa, fb, rot, scale, shift, -shift, -abs(shift)]]), device=DEV)
                        a = hip.augment_points(both, rec[0], torch.empty_like(both))
                        b = hip.augment_points(alone, rec[0], torch.empty_like(alone))
                        assert bool((a[:cap, 2] >= 8.9e29).all()) and torch.equal(a[cap:].view(torch.int32), b.view(torch.int32))
                        if (fa, fb, scale, shift) in ((0, 0, 0.9, -2.5), (1, 1, 1.1, 2.5)):
                            for kw in (dict(voxelnet, want_voxels=False, want_mean=True), dict(pillars, want_voxels=True, coor_cols=4)):
                                va, vb = _voxel_set(hip.voxelize(a, **kw)), _voxel_set(hip.voxelize(b, **kw))
                                assert len(va[0]) > 100 and len(va) == len(vb) == 3
                                for x, y in zip(va, vb):
                                    assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), (fa, fb, rot, scale, shift)
    # shuffled in among the scene's points: the same voxel set (the order of a voxel's points is the cloud's)
    from futuredet_amd.augment import reference_permutation

    rec = GlobalAugment.record(np.array([[1, 0, 0.4, 1.05, 0.3, -0.2, 0.1]]), device=DEV)
    perm = torch.from_numpy(reference_permutation(n + cap).copy()).to(DEV)
    a = hip.augment_points(both, rec[0], torch.empty_like(both), perm=perm)
    keep = (perm >= cap).nonzero().flatten()
    kw = dict(pillars, want_voxels=True, coor_cols=4)
    va, vb = _voxel_set(hip.voxelize(a, **kw)), _voxel_set(hip.voxelize(a[keep].contiguous(), **kw))
    for x, y in zip(va, vb):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


# ---------------------------------------------------------------------------------------------------------------------- the steps
@pytest.fixture(scope="module")
def world(hip):
    from test_gpu_train_static import _World

    return _World()


@pytest.fixture(scope="module")
def pillars(hip):
    from test_gpu_pillars_static import _Pillars

    return _Pillars()


def _sampler(seed=0, point_cap=None):
    """a database of twelve cars inside the range, 5-column points, and a sampler of 40 slots (16 of them take part beside 24 cars)"""
    from futuredet_amd.augment import GTSampler

    r = np.random.default_rng(42)
    M = 12
    sizes = r.integers(8, 30, M)
    dbb = np.zeros((M, 3, 12), np.float32)
    dbb[:, :, 0:2] = r.uniform(-20, 20, (M, 1, 2))
    dbb[:, :, 2] = -0.5
    dbb[:, :, 3:6] = (1.9, 4.6, 1.7)
    dbb[:, :, 6:10] = r.normal(0, 2, (M, 3, 4))
    dbb[:, :, 10:12] = r.uniform(-3, 3, (M, 3, 2))
    P = int(sizes.sum())
    pts = np.zeros((P, 5), np.float32)
    pts[:, :3] = r.uniform(-1, 1, (P, 3))
    pts[:, 3] = r.integers(0, 256, P)
    db = dict(boxes=dbb, steps=r.integers(1, 4, M).astype(np.int32), classes=np.ones(M, np.int32), trajectory=r.integers(0, 3, M).astype(np.int32),
              offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), points=pts)
    return GTSampler(_database(db, names=["car"]), [dict(car=40)], rate=1.0, seed=seed, point_cap=point_cap)


def _augment(sampler, **kw):
    from futuredet_amd.augment import GlobalAugment

    return GlobalAugment(dict(CFG, db_sampler=dict(enable=True, sample_groups=[dict(car=40)], global_random_rotation_range_per_object=[0, 0]), **kw),
                         seed=3, sampler=sampler)


def _candidates(B, K, seed):
    r = np.random.default_rng(seed)
    cand = np.full((B, K), -1, np.int32)
    for b in range(B):
        cand[b, :12] = r.permutation(12)
    return cand


def _load_against_aug(w, batch):
    """the static buffers after _load against aug(batch) for the same parameters and candidates"""
    from test_gpu_augment import _pad_gt

    B = len(batch["clouds"])
    sampler = _sampler(point_cap=300)
    aug = _augment(sampler)
    step = w.step(B, augment=aug)
    batch = _pad_gt(batch, step.max_gt)  # aug(batch) appends below the batch's own padded axis: as wide as the step's
    params, cand = aug.draw(B), _candidates(B, sampler.K, 9)
    batch = dict(batch, aug_params=params, gt_sample_candidates=cand)
    pre = aug(batch)
    step._load(batch, 0)
    torch.cuda.synchronize()
    assert np.array_equal(step.last_gt_sample_candidates, cand) and np.array_equal(pre["gt_sample_candidates"], cand)
    acc = pre["gt_sample_accepted"].cpu().numpy()
    assert torch.equal(step.gt_sample["accepted"], pre["gt_sample_accepted"]) and torch.equal(step.gt_sample["status"], pre["gt_sample_status"])
    assert 0 < acc[0].sum() <= 8 and int(pre["gt_sample_status"][0]) & 1, "24 of 32 rows are taken: eight fit, the ninth sets NO_ROW"
    counts = pre["gt_counts"].cpu().numpy()
    assert torch.equal(step.gt_counts, pre["gt_counts"]) and (counts == 24 + acc.sum(1)[:, None]).all()
    for b in range(B):
        n = int(batch["clouds"][b].shape[0]) + 300
        assert int(step.counts[b]) == n and pre["clouds"][b].shape[0] == n
        assert torch.equal(step.points[b, :n].view(torch.int32), pre["clouds"][b].view(torch.int32))
        assert int((pre["clouds"][b][:, 2] >= 8.9e29).sum()) == 300 - int(pre["gt_sample_points"][b]), "what is no entry's point is a sentinel"
        for t in range(counts.shape[1]):
            c = counts[b, t]
            assert torch.equal(step.gt_boxes[b, t, :c].view(torch.int32), pre["gt_boxes"][b, t, :c].view(torch.int32))
            assert torch.equal(step.gt_classes[b, t, :c], pre["gt_classes"][b, t, :c])
            if step.gt_trajectory is not None:
                assert torch.equal(step.gt_trajectory[b, t, :c], pre["gt_trajectory"][b, t, :c])
    # and against the pieces: select on the raw rows, then the transforms
    ref = R.select(batch["gt_boxes"].cpu().numpy(), batch["gt_counts"].cpu().numpy(), batch["gt_classes"].cpu().numpy(), None,
                   {k: getattr(sampler.database, k).cpu().numpy() for k in ("boxes", "steps", "classes", "trajectory", "offsets", "points")},
                   cand, sampler.records, 1.0, 300)
    assert np.array_equal(ref["accepted"], acc) and np.array_equal(ref["counts"], counts)
    return step


def test_load_against_aug_voxelnet(world):
    _load_against_aug(world, world.batch([5, 6], [4000, 2500]))


def test_load_against_aug_pillars(pillars):
    _load_against_aug(pillars, pillars.batch([2], [6000]))


def test_capacity_refusal_on_a_real_step(world):
    step = world.step(1, augment=_augment(_sampler(point_cap=300)))
    before = step.points.clone()
    with pytest.raises(ValueError, match="point_cap = 300"):
        step._load(world.batch([1], [8000]), 0)
    assert torch.equal(step.points, before)


def test_no_synchronisation_in_the_sampled_step(world):
    from test_gpu_train_static import _flat

    world.fresh()
    sampler = _sampler(seed=1)
    step = world.step(2, augment=_augment(sampler))
    b1, b2 = world.batch([1, 2], [3000, 2000]), world.batch([3, 4], [2500, 4000])
    step.warm_up([b2])
    step(b1, check=False)  # first call: capacities uploaded, scratch allocated, the permutations of the grown clouds uploaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step(b2, check=False)
        first = step.last_gt_sample_candidates.copy()
        out = step(b1, check=False)
        with pytest.raises(RuntimeError):
            out["loss"][0].item()  # the mode is enforced
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert step.iteration == 3 and not step.overflowed()
    assert first.shape == (2, sampler.K) and not np.array_equal(first, step.last_gt_sample_candidates)
    assert int(step.gt_sample["accepted"].sum()) > 0 and step.counts.cpu().tolist() == [int(c.shape[0]) + sampler.point_cap for c in b1["clouds"]]
    assert all(bool(torch.isfinite(v).all()) for v in _flat(out).values())


@pytest.mark.parametrize("which", ["world", "pillars"])
def test_a_step_without_a_sampler_loads_what_it_loaded_before(request, hip, which):
    """``sampler=None``: the static buffers are those of the earlier launches -- one fd_augment_points per cloud straight from the
    batch's tensor, one fd_augment_boxes, the batch's counts -- and no sampling buffer exists"""
    from futuredet_amd.augment import GlobalAugment

    w = request.getfixturevalue(which)
    batch = w.batch([2], [3000])
    aug = GlobalAugment(CFG, seed=3)
    step = w.step(1, augment=aug)
    assert step.gt_sample is None and aug.sampler is None and not aug.sampling
    params = aug.draw(1)
    step._load(dict(batch, aug_params=params), 0)
    torch.cuda.synchronize()
    rec = GlobalAugment.record(params, device=DEV)
    c = batch["clouds"][0]
    n = c.shape[0]
    want = hip.augment_points(c, rec[0], torch.empty_like(c), perm=aug.permutation(n, DEV))
    assert int(step.counts[0]) == n and torch.equal(step.points[0, :n].view(torch.int32), want.view(torch.int32))
    boxes = hip.augment_boxes(batch["gt_boxes"], batch["gt_counts"], rec)
    k = batch["gt_boxes"].shape[2]
    assert torch.equal(step.gt_boxes[:, :, :k].view(torch.int32), boxes.view(torch.int32)) and torch.equal(step.gt_counts, batch["gt_counts"])
    assert torch.equal(step.gt_classes[:, :, :k], batch["gt_classes"]) and not step.gt_boxes[:, :, k:].any()
    plain = w.step(1)
    plain._load(batch, 0)
    torch.cuda.synchronize()
    assert torch.equal(plain.points[0, :n], c) and torch.equal(plain.gt_boxes[:, :, :k], batch["gt_boxes"]) and plain.gt_sample is None
