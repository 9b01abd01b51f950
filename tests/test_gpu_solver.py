"""-m gpu: futuredet_amd.solver.FusedAdam (fd_optim.hip) against the reference's float64 trajectory (tests/golden/solver.npz) with the
fp32 torch restatement of the recipe as the yardstick (solver_util.rule), plus addressing, determinism, cache invalidation, the
torch.optim.Adam state format, freedom from host synchronisation, and one step of a real VoxelNet."""
import numpy as np
import pytest
import torch

from solver_util import GRAD_CLIP, TorchRecipe, Trajectory, rule

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def traj(golden):
    t = Trajectory(golden("solver.npz"))
    t.restated, t.restated_norm = t.run_restated(torch.float32)  # computed once, read by every test below
    return t


def _aligned(a):
    return torch.from_numpy(a).to(DEV).requires_grad_(True)


def _offset_by_one(a):
    """a parameter that is a view one element into a larger buffer: its address is 4-byte aligned only"""
    buf = torch.zeros(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(a).to(DEV)
    p = buf[1:].requires_grad_(True)
    assert p.data_ptr() % 16 == 4
    return p


def _flat(tensors):
    return np.concatenate([t.detach().cpu().double().numpy().ravel() for t in tensors])


def _replay(t, make_param, steps=None, replace_grad_of=()):
    """the fixture's steps on the device -> (optimiser, parameters, {(tag, name): flat array}, [total_norm per step])"""
    from futuredet_amd import solver

    params = [make_param(t.initial(i)) for i in range(len(t.numel))]
    opt = solver.FusedAdam(t.groups_of(params), wd=t.wd)
    sched = solver.OneCycle(opt, t.steps, 0.001, [0.95, 0.85], 10.0, 0.4)
    snaps, norms = {}, []
    for s in range(t.steps if steps is None else steps):
        sched.step(s)
        assert (opt.lr, opt.mom) == (t.lr[s], t.mom[s])
        opt.zero_grad()
        given = []
        for i, p in enumerate(params):
            g = t.grad(s, i)
            if g is None:
                p.grad = None
            elif i in replace_grad_of:
                p.grad = torch.from_numpy(g).to(DEV)  # no longer the attached view: step() copies it in
            else:
                p.grad.add_(torch.from_numpy(g).to(DEV))  # in place, as autograd accumulates
            given.append(None if p.grad is None else p.grad.clone())
        norms.append(opt.step(grad_clip=dict(max_norm=t.max_norm, norm_type=2)))
        for p, g in zip(params, given):  # the one intended difference: clipping does not rewrite .grad
            assert (p.grad is None) == (g is None) and (g is None or torch.equal(p.grad, g))
        if steps is None and s in t.snap_at:
            sd = opt.state_dict()
            tag = t.snap_at[s]
            snaps[tag, "p"] = _flat(params)
            snaps[tag, "exp_avg"] = _flat([sd["state"][i]["exp_avg"] for i in range(len(params))])
            snaps[tag, "exp_avg_sq"] = _flat([sd["state"][i]["exp_avg_sq"] for i in range(len(params))])
            snaps[tag, "step"] = np.asarray([int(sd["state"][i]["step"]) for i in range(len(params))], np.int32)
    return opt, params, snaps, norms


def _check_trajectory(t, snaps, norms, label, lines=None):
    for tag in ("first", "last"):
        for name in ("p", "exp_avg", "exp_avg_sq"):
            rule("%s: %s after the %s step" % (label, name, tag), snaps[tag, name], t.restated[tag, name], t.truth[tag, name], lines)
        assert np.array_equal(snaps[tag, "step"], t.truth[tag, "step"]), (tag, snaps[tag, "step"], t.truth[tag, "step"])
    assert all(isinstance(n, torch.Tensor) and n.is_cuda and n.dtype == torch.float32 for n in norms)
    rule("%s: total_norm over the steps" % label, [float(n) for n in norms], t.restated_norm, t.total_norm, lines)
    # the tensor that had no gradient in two steps: two Adam steps fewer, and its parameters still carry those steps' decay
    k = t.none_tensor
    assert t.truth["last", "step"][k] == t.steps - len(t.none_steps)
    a, b = t.off[k], t.off[k + 1]
    rule("%s: p of the tensor that skipped steps" % label, snaps["last", "p"][a:b], t.restated["last", "p"][a:b], t.truth["last", "p"][a:b], lines)
    # without the decay of the skipped steps every element would sit a relative sum(wd * lr) ~ 1.9e-5 away from the truth; six steps
    # of fp32 roundings are a few ulp (1.2e-7 relative each, of values no smaller than the 1e-3 updates) -- element by element, where
    # the parameter is not itself within 1e-3 of zero, the result is far closer to the decayed truth
    want = t.truth["last", "p"][a:b]
    gap = np.abs(want * (1.0 / np.prod([1 - t.wd * t.lr[s] for s in t.none_steps]) - 1.0))
    big = np.abs(want) >= 1e-3
    assert big.sum() > 0.9 * big.size and np.all(np.abs(snaps["last", "p"][a:b] - want)[big] <= 0.25 * gap[big])


def test_trajectory_matches_the_reference_run(hip, traj):
    assert traj.chunk == hip.optim_chunk(), "the fixture's tensor sizes straddle the kernels' chunk"
    _, _, snaps, norms = _replay(traj, _aligned, replace_grad_of=(1, 4, 8))
    _check_trajectory(traj, snaps, norms, "trajectory")


def test_misaligned_parameters_and_contiguity(hip, traj):
    from futuredet_amd import solver

    _, _, snaps, norms = _replay(traj, _offset_by_one)
    _check_trajectory(traj, snaps, norms, "4-byte aligned parameters")
    w = torch.zeros((8, 6), device=DEV).t().requires_grad_(True)
    assert not w.is_contiguous()
    with pytest.raises((ValueError, hip.FutureDetHipError), match="contiguous"):
        solver.FusedAdam([[w], []])
    with pytest.raises(hip.FutureDetHipError, match="float32"):
        solver.FusedAdam([[torch.zeros(4, device=DEV, dtype=torch.float64)], []])


def test_two_runs_are_bit_identical(hip, traj):
    runs = []
    for _ in range(2):
        opt, params, _, norms = _replay(traj, _aligned, steps=3)
        sd = opt.state_dict()
        runs.append(([p.detach().clone() for p in params], [sd["state"][i][k] for i in range(len(params)) for k in ("exp_avg", "exp_avg_sq")], norms))
    for a, b in zip(runs[0], runs[1]):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _step_with_random_grads(module, seed):
    from futuredet_amd import solver

    opt = solver.FusedAdam.for_model(module, lr=1e-2, wd=0.01)
    opt.zero_grad()
    gen = torch.Generator().manual_seed(seed)
    for p in opt.params:
        p.grad.add_(torch.randn(p.shape, generator=gen).to(DEV))
    opt.step(grad_clip=GRAD_CLIP)


def test_center_head_caches_follow_a_step(hip, golden):
    from futuredet_amd import build_head
    from futuredet_amd.nn_utils import weights_version
    from futuredet_amd.synth import seeded_state_dict

    kw = dict(type="CenterHead", in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10,
              common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}, share_conv_channel=64, timesteps=1, classify=False)
    head = build_head(dict(kw))
    head.load_state_dict(seeded_state_dict(head, 12), strict=False)
    head = head.to(DEV).eval()
    x = torch.from_numpy(golden("dense_nets.npz")["rpn_y"]).to(DEV)

    def run(m):
        with torch.no_grad():
            return [{k: v.float().clone() for k, v in pd.items()} for pd in m(x)]

    before, v0 = run(head), weights_version(head)
    _step_with_random_grads(head, 3)
    assert weights_version(head) != v0
    after = run(head)
    fresh = build_head(dict(kw))
    fresh.load_state_dict(head.state_dict())
    want = run(fresh.to(DEV).eval())
    for a, w, b in zip(after, want, before):
        assert set(a) == set(w)
        for k in a:
            assert torch.equal(a[k], w[k]), k
        assert any(not torch.equal(a[k], b[k]) for k in a), "the step must change the head's output"


def test_sparse_conv_caches_follow_a_step(hip):
    from futuredet_amd import sparse as spconv
    from futuredet_amd.nn_utils import weights_version

    rng = np.random.default_rng(5)
    cells = rng.choice(11 * 24 * 24, 1463, replace=False)
    z, rem = np.divmod(cells, 24 * 24)
    coords = torch.from_numpy(np.stack([np.zeros_like(z), z, rem // 24, rem % 24], 1).astype(np.int32)).to(DEV)
    feats = torch.from_numpy(rng.uniform(-1, 1, (len(cells), 32)).astype(np.float32)).to(DEV)
    torch.manual_seed(5)
    conv = spconv.SubMConv3d(32, 64, 3, bias=True, indice_key="s").to(DEV).eval()

    def run(m):
        with torch.no_grad():
            return m(spconv.SparseConvTensor(feats, coords, [11, 24, 24], 1)).features.clone()

    before, v0 = run(conv), weights_version(conv)
    _step_with_random_grads(conv, 4)
    assert weights_version(conv) != v0
    after = run(conv)
    fresh = spconv.SubMConv3d(32, 64, 3, bias=True, indice_key="s")
    fresh.load_state_dict(conv.state_dict())
    assert torch.equal(after, run(fresh.to(DEV).eval())) and not torch.equal(after, before)


def test_state_dict_round_trips_with_torch_adam(hip, traj):
    """FusedAdam.state_dict() loads into torch.optim.Adam over the same two groups and torch's state loads into FusedAdam; one
    further step on each side agrees under the rule, with the float64 truth continued from the fixture's last state."""
    from futuredet_amd import solver

    t = traj
    n = len(t.numel)
    opt, params, snaps, _ = _replay(t, _aligned)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(n)) and [len(g["params"]) for g in sd["param_groups"]] == [t.group.count(0), t.group.count(1)]
    lr, mom = 4e-4, 0.9
    grads = [t.grad(0, i) for i in range(n)]

    def further_step(dtype, p_flat, state):
        ps = [torch.from_numpy(p_flat[t.off[i]:t.off[i + 1]]).to(dtype).clone().requires_grad_(True) for i in range(n)]
        r = TorchRecipe(t.groups_of(ps), t.wd)
        r.opt.load_state_dict(state)
        r.lr, r.mom = lr, mom
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(dtype).clone()  # clip_grad_norm_ scales it in place
        norm = r.step(GRAD_CLIP)
        return _flat(ps), _flat([m[0] for m in r.moments()]), _flat([m[1] for m in r.moments()]), [m[2] for m in r.moments()], float(norm)

    def state_of(dtype, tag_arrays):
        m, v = (tag_arrays[k] for k in ("exp_avg", "exp_avg_sq"))
        return dict(state={i: dict(step=torch.tensor(float(t.truth["last", "step"][i])), exp_avg=torch.from_numpy(m[t.off[i]:t.off[i + 1]]).to(dtype).clone(),
                                   exp_avg_sq=torch.from_numpy(v[t.off[i]:t.off[i + 1]]).to(dtype).clone()) for i in range(n)},
                    param_groups=sd["param_groups"])

    truth = further_step(torch.float64, t.truth["last", "p"], state_of(torch.float64, {k: t.truth["last", k] for k in ("exp_avg", "exp_avg_sq")}))
    # FusedAdam -> torch.optim.Adam: torch continues (in fp32, on the CPU) from the device optimiser's state
    cpu_sd = dict(state={i: {k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for i, st in sd["state"].items()},
                  param_groups=sd["param_groups"])
    from_fused = further_step(torch.float32, snaps["last", "p"].astype(np.float32), cpu_sd)
    # torch.optim.Adam -> FusedAdam: a fresh device optimiser continues from the fp32 restatement's state
    rest = {k: t.restated["last", k].astype(np.float32) for k in ("p", "exp_avg", "exp_avg_sq")}
    fresh_params = [_aligned(rest["p"][t.off[i]:t.off[i + 1]].copy()) for i in range(n)]
    fused = solver.FusedAdam(t.groups_of(fresh_params), wd=t.wd)
    fused.load_state_dict(state_of(torch.float32, rest))
    fused.lr, fused.mom = lr, mom
    fused.zero_grad()
    for p, g in zip(fresh_params, grads):
        p.grad.add_(torch.from_numpy(g).to(DEV))
    norm = fused.step(grad_clip=GRAD_CLIP)
    sd2 = fused.state_dict()
    into_fused = (_flat(fresh_params), _flat([sd2["state"][i]["exp_avg"] for i in range(n)]), _flat([sd2["state"][i]["exp_avg_sq"] for i in range(n)]),
                  [int(sd2["state"][i]["step"]) for i in range(n)], float(norm))
    # the yardstick: the fp32 restatement continuing from its own state
    yard = further_step(torch.float32, rest["p"], state_of(torch.float32, rest))
    for label, got in (("fused state into torch Adam", from_fused), ("torch Adam state into FusedAdam", into_fused)):
        for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
            rule("%s: %s one step on" % (label, name), got[k], yard[k], truth[k])
        assert got[3] == truth[3] == [int(s) + 1 for s in t.truth["last", "step"]]
        rule("%s: total_norm" % label, [got[4]], [yard[4]], [truth[4]])


def test_step_does_not_synchronise(hip, traj):
    from futuredet_amd import solver

    params = [_aligned(traj.initial(i)) for i in range(len(traj.numel))]
    opt = solver.FusedAdam(traj.groups_of(params), wd=traj.wd)
    sched = solver.OneCycle(opt, 10, 0.001, [0.95, 0.85], 10.0, 0.4)
    grads = [torch.from_numpy(traj.grad(0, i)).to(DEV) for i in range(len(params))]

    def one(i):
        sched.step(i)
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad.add_(g)
        return opt.step(grad_clip=GRAD_CLIP)

    one(0)  # warm-up: code objects, the first uploads
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in (1, 2):
            norm = one(i)
        params[-1].grad = None  # a change of the gradient set re-uploads the flags: still without a blocking copy
        sched.step(3)
        opt.step(grad_clip=GRAD_CLIP)
        with pytest.raises(RuntimeError, match="synchroniz"):  # the mode is enforced on this build: a read-back is refused
            norm.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(norm) > 35.0 and int(opt.state_dict()["state"][len(params) - 1]["step"]) == 3


def _example(cfg, seed):
    from futuredet_amd.synth import synthetic_cloud
    from oracle import ops as oops

    vg = cfg.voxel_generator
    v, c, n = oops.points_to_voxel(synthetic_cloud(seed=seed, target_points=8000), vg["voxel_size"], vg["range"], 10, True, 160000)
    rng = np.random.default_rng(seed)
    Hh = Wh = 180
    M = 16
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([[1440, 1440, 40]]), metadata=[None])
    for key in ("hm", "ind", "mask", "cat", "anno_box"):
        ex[key] = []
    for s in range(cfg.timesteps):
        ind = torch.from_numpy(rng.choice(Hh * Wh, M, replace=False)[None].astype(np.int64)).to(DEV)
        hm = torch.from_numpy((rng.uniform(0, 0.9, (1, 1, Hh, Wh)) ** 3).astype(np.float32)).to(DEV)
        hm.view(-1)[ind[0]] = 1.0
        ex["hm"].append([hm])
        ex["ind"].append([ind])
        ex["mask"].append([torch.ones((1, M), dtype=torch.uint8, device=DEV)])
        ex["cat"].append([torch.zeros((1, M), dtype=torch.int64, device=DEV)])
        ex["anno_box"].append([torch.from_numpy(rng.normal(0, 1, (1, M, 10)).astype(np.float32)).to(DEV)])
    return ex


def test_one_training_step_of_a_voxelnet(hip):
    """forecast_n0 (161 tensors: sparse-conv, BatchNorm, RPN and head): one iteration of train_steps on the device against the torch
    restatement (fp32) and the float64 truth on a CPU twin of the model that gets the same gradients."""
    from futuredet_amd import build_detector, solver
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.nn_utils import weights_version
    from futuredet_amd.synth import seeded_state_dict, tame_box_dims

    cfg = centerpoint_config("forecast_n0")
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    twin = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    twin.load_state_dict(net.state_dict())
    net = net.to(DEV)
    opt = solver.build_one_cycle_optimizer(net, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
    sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
    assert opt.group_sizes == [77, 84]
    v0 = weights_version(net)
    out = next(solver.train_steps(net, [_example(cfg, 2)], opt, sched, grad_clip=GRAD_CLIP))
    assert torch.isfinite(sum(out["loss"])) and weights_version(net) != v0
    names = [n for g in solver.parameter_groups(net) for n, _ in g]
    got = dict(zip(names, opt.params))
    grads = {n: p.grad.detach().cpu() for n, p in got.items()}  # clipping left them as backward wrote them
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and sum(bool((g != 0).any()) for g in grads.values()) > 100

    def restated(dtype):
        groups = [[(n, p.detach().clone().to(dtype).requires_grad_(True)) for n, p in g] for g in solver.parameter_groups(twin)]
        r = TorchRecipe([[p for _, p in g] for g in groups], 0.01)
        r.lr, r.mom = opt.lr, opt.mom
        for n, p in groups[0] + groups[1]:
            p.grad = grads[n].to(dtype).clone()  # clip_grad_norm_ scales it in place
        norm = r.step(GRAD_CLIP)
        return {n: p.detach().double().numpy() for n, p in groups[0] + groups[1]}, float(norm)

    (yard, yard_norm), (truth, truth_norm) = restated(torch.float32), restated(torch.float64)
    assert list(yard) == names
    rule("forecast_n0 step: total_norm", [float(out["total_norm"])], [yard_norm], [truth_norm])
    worst = 0.0
    for n in names:
        a = got[n].detach().cpu().double().numpy()
        e_f, e_t = np.abs(a - truth[n]).max(), np.abs(yard[n] - truth[n]).max()
        floor = float(np.spacing(np.float32(np.abs(truth[n]).max())))
        worst = max(worst, e_f / max(4.0 * e_t, floor))
        assert e_f <= max(4.0 * e_t, floor), (n, e_f, e_t, floor)
    rule("forecast_n0 step: all parameters", _flat(got.values()), np.concatenate([yard[n].ravel() for n in names]),
         np.concatenate([truth[n].ravel() for n in names]))
    print("[solver] forecast_n0 step: worst per-tensor error / bound %.3f over %d tensors" % (worst, len(names)))
