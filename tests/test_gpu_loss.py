"""-m gpu: the fused CenterHead loss (futuredet_amd/csrc/fd_loss.hip, CenterHead.fused_loss) against float64 -- the reference's own
terms and gradients (tests/golden/loss.npz) or CenterHead.loss in double on the CPU, which test_loss_golden.py pins to that reference
at 1e-10.  Gate (solver_util.rule, the rule of test_gpu_solver.py): per output tensor the fused path's maximum error is at most
4 x the error of the torch path run in fp32 on the same device tensors, floor one fp32 ulp of the tensor's largest magnitude.

Deliberately absent: entries with mask == 0 and a garbage ind, and out-of-range entries with mask != 0 -- a wrong guard would fault
the device.  The guard's arithmetic (csrc/fd_loss_guard.h) is tested on the host by test_loss_fused_host.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import loss_util as lu  # noqa: E402
import make_golden_loss as mgl  # noqa: E402
from futuredet_amd import build_head, hip_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(HERE, "golden", "loss.npz"))
CHUNK = 2048  # asserted against fd_loss_chunk() below


def _fixture_case(name, T, dense):
    """The fixture's inputs in loss_util's layout, and the reference's float64 outputs under loss_util's names."""
    n_tasks = T if dense else 1
    maps = [{k: GOLD["%s_t%d_%s" % (name, t, k)] for k in lu.HEADS[10] + ("hm",)} for t in range(n_tasks)]
    steps = [[dict(hm=GOLD["%s_s%d_hm_target" % (name, s)], ind=GOLD["%s_s%d_ind" % (name, s)], mask=GOLD["%s_s%d_mask" % (name, s)],
                   cat=GOLD["%s_s%d_cat" % (name, s)], anno_box=GOLD["%s_s%d_anno_box" % (name, s)])] for s in range(T)]
    truth = {}
    for t in range(n_tasks):
        for key in ("loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive"):
            truth["t%d_%s" % (t, key)] = GOLD["%s_out_t%d_%s" % (name, t, key)]
        for k in maps[t]:
            truth["t%d_grad_%s" % (t, k)] = GOLD["%s_grad_t%d_%s" % (name, t, k)]
    return dict(maps=maps, steps=steps, T=T, dense=dense, D=10, classes=[1] * n_tasks), truth


def _three_ways(head, case, truth=None, coeffs=None, wrappers=False):
    """-> (fused, fp32 torch path on the device, float64 truth)"""
    if truth is None:
        truth = lu.run(head, case, "cpu", torch.float64, False, coeffs)
    yard = lu.run(head, case, DEV, torch.float32, False, coeffs)
    fused = lu.run_wrappers(head, case, DEV, coeffs) if wrappers else lu.run(head, case, DEV, torch.float32, True, coeffs)
    return fused, yard, truth


def test_chunk_constant():
    assert hip_ops.loss_chunk() == CHUNK


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["wrappers", "head"])
@pytest.mark.parametrize("name,T,dense", mgl.CASES)
def test_fixture_terms_and_gradients(name, T, dense, how):
    head = build_head(dict(type="CenterHead", **mgl.head_kwargs(T, dense)))
    case, truth = _fixture_case(name, T, dense)
    fused, yard, _ = _three_ways(head, case, truth, wrappers=how == "wrappers")
    lu.gate("%s/%s" % (name, how), fused, yard, truth)
    if how == "wrappers":
        assert fused["status"] == 0


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _six_tasks_objects(s, u, b):
    return 0 if u == 2 else (5 + u + s - b)  # task 2: num_pos == 0 in every step


SHAPES = {
    # 858 heat-map elements: not a multiple of 4, less than one chunk; T = 1
    "odd_small": dict(B=2, H=13, W=11, M=9, T=1, dense=False, classes=(3,)),
    # 2 * chunk + 250 + 41 = 4387 elements: two full chunks, a partial third and a scalar tail of 3
    "three_chunks": dict(B=1, H=41, W=107, M=20, T=2, dense=False, classes=(1,)),
    # six standard tasks with 1 or 2 classes, T = 3, target rows 14 wide as fd_assign_targets writes them; task 2 has no objects
    "six_tasks": dict(B=2, H=12, W=10, M=13, T=3, dense=False, classes=(1, 2, 1, 2, 2, 1), row=14, n_obj=_six_tasks_objects),
    "rvel_rrot": dict(B=2, H=10, W=14, M=8, T=2, dense=False, D=14, classes=(2,)),
    "rvel_rrot_dense": dict(B=2, H=10, W=14, M=8, T=2, dense=True, D=14),
    "no_vel": dict(B=2, H=9, W=15, M=8, T=1, dense=False, D=8, classes=(2,)),
    "one_step": dict(B=3, H=8, W=8, M=6, T=1, dense=False, classes=(1,)),
    # a sample without objects next to a full one; 300 entries take two rounds of the 256-thread compaction
    "empty_next_to_full": dict(B=2, H=24, W=20, M=300, T=2, dense=True, n_obj=lambda s, u, b: 300 if b == 0 else 0),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_generated_shapes(name):
    kw = dict(SHAPES[name])
    assert name != "three_chunks" or kw["B"] * kw["H"] * kw["W"] == 2 * CHUNK + 250 + 41
    head = lu.head_of(kw["T"], kw["dense"], kw.get("D", 10), kw.get("classes", (1,)))
    case = lu.make_case(11, **kw)
    fused, yard, truth = _three_ways(head, case)
    lu.gate(name, fused, yard, truth)
    direct = lu.run_wrappers(head, case, DEV)
    assert direct["status"] == 0
    for k, v in fused.items():
        assert np.array_equal(direct[k], v), k  # the head path and the wrappers are the same launches


def test_unaligned_pointers_take_the_scalar_path_with_the_same_bits():
    kw = dict(SHAPES["three_chunks"])
    head = lu.head_of(kw["T"], kw["dense"])
    case = lu.make_case(11, **kw)
    a, b = lu.run_wrappers(head, case, DEV), lu.run_wrappers(head, case, DEV, shift=1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _duplicates(s, u, b, ind, cat, mask):
    if b == 0:
        ind[0:3] = 37          # three objects on one cell, the same class
        cat[0:3] = 1
        ind[3:5] = 52          # two on one cell, different classes
        cat[3], cat[4] = 0, 1
        ind[5], cat[5] = 0, 0  # one object on cell 0, which the unused slots also name with mask = 0
    else:
        ind[0], ind[2], ind[4] = 5, 5, 5  # duplicates that are not neighbours in the list
        cat[0], cat[2], cat[4] = 0, 1, 0


def test_duplicate_cells_are_summed_in_order_and_deterministic():
    head = lu.head_of(2, False, classes=(2,))
    case = lu.make_case(5, B=2, H=9, W=11, M=10, T=2, dense=False, classes=(2,), n_obj=lambda s, u, b: 7, place=_duplicates)
    assert (case["steps"][0][0]["ind"][0, 7:] == 0).all() and (case["steps"][0][0]["mask"][0, 7:] == 0).all()
    fused, yard, truth = _three_ways(head, case)
    lu.gate("duplicates", fused, yard, truth)
    again = lu.run(head, case, DEV, torch.float32, True)
    for k in fused:
        assert np.array_equal(fused[k], again[k]), k


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _split_logits(rng, shape):
    """A third of the cells at |x| >= 10.5 (sigma clamped on either side), the rest at |x| <= 8, none between: the clamp boundary is
    ln 9999 = 9.21, so no cell's clamp decision depends on the last bit of an exponential."""
    x = rng.uniform(-8.0, 8.0, shape)
    far = rng.random(shape) < 1.0 / 3.0
    return np.where(far, np.sign(rng.normal(size=shape)) * rng.uniform(10.5, 14.0, shape), x)


def test_clamped_cells_have_exactly_zero_gradient():
    head = lu.head_of(1, False, classes=(2,))
    case = lu.make_case(8, B=2, H=12, W=12, M=40, T=1, dense=False, classes=(2,), n_obj=lambda s, u, b: 36, logits=_split_logits)
    x = case["maps"][0]["hm"]
    clamped = np.abs(x) >= 10.5
    assert ((np.abs(x) <= 8.0) | clamped).all() and clamped.mean() > 0.2
    st = case["steps"][0][0]
    pos_clamped = sum(int(clamped[b, st["cat"][b, j]].reshape(-1)[st["ind"][b, j]]) for b in range(2) for j in range(36))
    assert pos_clamped >= 4, "positives must sit on clamped cells too"
    fused, yard, truth = _three_ways(head, case)
    lu.gate("clamp", fused, yard, truth)
    g = fused["t0_grad_hm"]
    assert (g[clamped] == 0.0).all() and (g[~clamped] != 0.0).all()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_upstream_gradients_other_than_one():
    head = lu.head_of(3, True)
    case = lu.make_case(9, B=2, H=10, W=10, M=8, T=3, dense=True)
    coeffs = [0.5, 0.0, -1.75]
    fused, yard, truth = _three_ways(head, case, coeffs=coeffs)
    lu.gate("go", fused, yard, truth)
    for k, v in fused.items():
        if k.startswith("t1_grad_"):
            assert (v == 0.0).all(), k
        elif "_grad_" in k:
            assert (v != 0.0).any(), k


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def _device_problem(head, case):
    ex = lu.example_of(case, DEV, torch.float32)
    leaves = [{k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in m.items()} for m in case["maps"]]
    return ex, leaves


def test_no_host_synchronisation():
    head = lu.head_of(3, True)
    head.fused_loss = True
    case = lu.make_case(9, B=2, H=10, W=10, M=8, T=3, dense=True)
    ex, leaves = _device_problem(head, case)

    def step():
        ret = head.loss(ex, [dict(m) for m in leaves])
        sum(ret["loss"]).backward()
        return ret

    step()  # warm-up: code objects, the workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ret = step()
        with pytest.raises(RuntimeError, match="synchroniz"):  # the mode is enforced on this build
            ret["loss"][0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(v.is_cuda for k in ("loss", "hm_loss", "num_positive") for v in ret[k])
    assert ret["loss"][0].requires_grad and not ret["hm_loss"][0].requires_grad and not ret["loc_loss"][0][0].requires_grad
    assert torch.isfinite(sum(ret["loss"]))
    head.fused_loss = False
    with pytest.raises(RuntimeError, match="synchroniz"):  # what the switch removes: the torch path reads terms back
        torch.cuda.set_sync_debug_mode("error")
        try:
            head.loss(ex, [dict(m) for m in leaves])
        finally:
            torch.cuda.set_sync_debug_mode("default")


def test_check_reads_the_status_word():
    head = lu.head_of(1, False)
    head.fused_loss = True
    case = lu.make_case(3, B=1, H=8, W=8, M=6, T=1, dense=False)
    ex, leaves = _device_problem(head, case)
    ret = head.loss(ex, [dict(m) for m in leaves], check=True)  # every entry in range: no AssertionError
    assert set(ret) == {"loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive"}


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def _synthetic_gt(rng, B, T, n):
    boxes = np.zeros((B, T, n, 12), np.float32)
    boxes[..., 0:2] = rng.uniform(-40.0, 40.0, (B, T, n, 2))
    boxes[..., 2] = rng.normal(-0.5, 0.3, (B, T, n))
    boxes[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * rng.uniform(0.8, 1.2, (B, T, n, 3))
    boxes[..., 6:10] = rng.normal(0.0, 2.0, (B, T, n, 4))
    boxes[..., 10:12] = rng.uniform(-np.pi, np.pi, (B, T, n, 2))
    return boxes, np.full((B, T), n, np.int32), np.ones((B, T, n), np.int32), rng.integers(0, 3, (B, T, n)).astype(np.int32)


def test_targets_loss_and_backward_in_one_graph():
    """fd_assign_targets + loss forward + backward captured on one stream (no parallel branches), replayed twice with new map
    contents: bit for bit the eager result on the same contents."""
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.targets import TargetAssigner

    cfg = centerpoint_config("forecast_n3dtf")
    vg = cfg.voxel_generator
    ta = TargetAssigner(cfg.train_cfg.assigner, np.array([1440, 1440, 40]), vg["range"], vg["voxel_size"])
    B, T = 2, cfg.timesteps
    rng = np.random.default_rng(4)
    static_in = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(rng, B, T, 24)]
    if not ta.extra_sets:
        static_in[3] = None
    head = lu.head_of(T, True)
    head.fused_loss = True
    names = ("hm",) + lu.HEADS[10]
    width = dict(lu.WIDTH, hm=1, vel=2)

    def contents(seed):
        g = np.random.default_rng(seed)
        return [{k: torch.from_numpy(g.normal(-1.0 if k == "hm" else 0.0, 1.2, (B, width[k], ta.H, ta.W)).astype(np.float32)).to(DEV) for k in names}
                for _ in range(T)]

    def problem(maps, out):
        ex = ta(*static_in, out=out, check=False)
        ret = head.loss(ex, [dict(m) for m in maps])
        flat = [m[k] for m in maps for k in names]
        grads = torch.autograd.grad(sum(ret["loss"]), flat)
        return torch.stack([x.detach() for x in ret["loss"] + ret["hm_loss"] + ret["num_positive"]]), grads

    static_maps = [{k: v.requires_grad_(True) for k, v in m.items()} for m in contents(0)]
    out = ta.outputs(B, T, torch.device(DEV))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        problem(static_maps, out)  # warm-up on the capture stream: the workspaces exist before capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        terms, grads = problem(static_maps, out)
    seen = []
    for seed in (1, 2):
        new = contents(seed)
        with torch.no_grad():
            for m, n in zip(static_maps, new):
                for k in names:
                    m[k].copy_(n[k])
        g.replay()
        torch.cuda.synchronize()
        e_terms, e_grads = problem([{k: v.requires_grad_(True) for k, v in m.items()} for m in new], ta.outputs(B, T, torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(terms, e_terms) and bool(torch.isfinite(terms).all())
        for a, b in zip(grads, e_grads):
            assert torch.equal(a, b)
        seen.append(terms.clone())
    assert not torch.equal(seen[0], seen[1]), "the replay must see the new maps"
    assert float(terms[-1]) > 0, "the targets hold objects"


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_training_step_of_a_voxelnet_with_the_switch_on():
    """forecast_n0 on the 20 000-point synthetic cloud: one solver.train_steps iteration with fused_loss gives finite gradients on
    every parameter, and its loss passes the gate against the same step with the switch off.  Truth: CenterHead.loss in double on
    the CPU, on the head maps of the step it is compared with."""
    import copy

    from futuredet_amd import build_detector, solver
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims
    from futuredet_amd.targets import TargetAssigner
    from futuredet_amd.voxelize import points_to_voxel

    cfg = centerpoint_config("forecast_n0")
    vg = cfg.voxel_generator
    net = build_detector(cfg.model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    assert net.bbox_head.fused_loss is False
    nets = {False: net.to(DEV), True: copy.deepcopy(net).to(DEV)}
    grid = np.array([1440, 1440, 40])
    ta = TargetAssigner(cfg.train_cfg.assigner, grid, vg["range"], vg["voxel_size"])
    gt = [torch.from_numpy(a).to(DEV) for a in _synthetic_gt(np.random.default_rng(2), 1, cfg.timesteps, 24)]
    targets = ta(gt[0], gt[1], gt[2], gt[3] if ta.extra_sets else None)
    pts = synthetic_cloud(seed=1, target_points=20000)
    v, c, n = points_to_voxel(pts, vg["voxel_size"], vg["range"], 10, True, 160000)
    ex = dict(voxels=torch.from_numpy(v).to(DEV), coordinates=torch.from_numpy(np.pad(c, ((0, 0), (1, 0)))).to(DEV),
              num_points=torch.from_numpy(n).to(DEV), num_voxels=torch.tensor([len(n)]), shape=np.array([grid]), metadata=[None])
    ex.update({k: targets[k] for k in ("hm", "ind", "mask", "cat", "anno_box")})
    cpu_ex = {k: [[x.cpu().double() if x.dtype == torch.float32 else x.cpu() for x in row] for row in targets[k]]
              for k in ("hm", "ind", "mask", "cat", "anno_box")}
    got, truth = {}, {}
    for on, model in nets.items():
        model.bbox_head.fused_loss = on
        seen = []
        hook = model.bbox_head.register_forward_hook(lambda mod, inp, out: seen.append([{k: v.detach().cpu().double() for k, v in p.items()} for p in out]))
        opt = solver.build_one_cycle_optimizer(model, dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False))
        sched = solver.create_learning_rate_scheduler(opt, dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4), 10)
        out = next(solver.train_steps(model, [ex], opt, sched, grad_clip=dict(max_norm=35, norm_type=2)))
        hook.remove()
        got[on] = np.array([float(x.detach()) for x in out["loss"]])
        for name, p in model.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (on, name)
        twin = lu.head_of(cfg.timesteps, False)
        twin.code_weights, twin.weight = model.bbox_head.code_weights, model.bbox_head.weight
        truth[on] = np.array([float(x) for x in twin.loss(cpu_ex, seen[0])["loss"]])
    e_fused, e_torch = np.abs(got[True] - truth[True]).max(), np.abs(got[False] - truth[False]).max()
    floor = float(np.spacing(np.float32(np.abs(truth[True]).max())))
    print("[loss] forecast_n0 step: fused err %.3e  torch fp32 err %.3e  ulp floor %.3e  loss %r" % (e_fused, e_torch, floor, got[True].tolist()))
    assert np.isfinite(got[True]).all() and e_fused <= max(4.0 * e_torch, floor)
