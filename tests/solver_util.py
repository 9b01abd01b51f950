"""Shared by the solver tests and tools/optim_bench.py: the reference recipe restated in torch, the fixture's float64 trajectory, and
the agreement rule."""
import numpy as np
import torch

GRAD_CLIP = dict(max_norm=35, norm_type=2)


class TorchRecipe(object):
    """The reference's optimiser step restated in torch, on any device and dtype: per-parameter ``mul_(1 - wd * lr)`` on both groups,
    ``clip_grad_norm_``, then torch.optim.Adam (its defaults, betas=(0.9, 0.99)) over the two groups, with lr and beta1 set from
    outside at every iteration as OptimWrapper's properties do."""

    def __init__(self, groups, wd, betas=(0.9, 0.99)):
        self.groups = [list(g) for g in groups]
        self.params = [p for g in self.groups for p in g]
        self.opt = torch.optim.Adam([dict(params=g, lr=0.0) for g in self.groups if g], betas=betas)
        self.wd, self.lr, self.mom, self.beta = wd, 0.0, betas[0], betas[1]

    def zero_grad(self):
        self.opt.zero_grad()

    def step(self, grad_clip=None):
        total_norm = None
        if grad_clip is not None:
            total_norm = torch.nn.utils.clip_grad_norm_([p for p in self.params if p.requires_grad], **grad_clip)
        for g in self.opt.param_groups:
            g["lr"], g["betas"], g["weight_decay"] = self.lr, (self.mom, self.beta), 0
        with torch.no_grad():
            for p in self.params:
                p.mul_(1 - self.wd * self.lr)
        self.opt.step()
        return total_norm

    def moments(self):
        """(exp_avg, exp_avg_sq, step) per parameter; zeros / 0 where torch has created no state yet"""
        out = []
        for p in self.params:
            st = self.opt.state.get(p)
            out.append((st["exp_avg"], st["exp_avg_sq"], int(st["step"])) if st else (torch.zeros_like(p), torch.zeros_like(p), 0))
        return out


class Trajectory(object):
    """tests/golden/solver.npz "traj/...": the reference's float64 six-step run (make_golden_solver.py)"""

    def __init__(self, g):
        self.numel = [int(n) for n in g["traj/numel"]]
        self.group = [int(v) for v in g["traj/group"]]
        self.off = np.concatenate([[0], np.cumsum(self.numel)])
        self.p0 = g["traj/p0"]
        self.q, self.scale = g["traj/grad_q"], g["traj/grad_scale"]
        self.steps = len(self.scale)
        self.none_tensor, self.none_steps = int(g["traj/none_tensor"]), [int(s) for s in g["traj/none_steps"]]
        self.lr, self.mom, self.total_norm = g["traj/lr"], g["traj/mom"], g["traj/total_norm"]
        self.wd, self.max_norm, self.chunk = float(g["traj/wd"]), float(g["traj/max_norm"]), int(g["traj/chunk"])
        self.truth = {}
        for tag in ("first", "last"):
            for name in ("p", "exp_avg", "exp_avg_sq"):
                hi, lo = g["traj/%s/%s_hi" % (tag, name)], g["traj/%s/%s_lo" % (tag, name)]
                self.truth[tag, name] = hi.astype(np.float64) + lo.astype(np.float64) * np.spacing(np.abs(hi)).astype(np.float64)
            self.truth[tag, "step"] = g["traj/%s/step" % tag]
        self.snap_at = {0: "first", self.steps - 1: "last"}

    def initial(self, i):
        return self.p0[self.off[i]:self.off[i + 1]].copy()

    def grad(self, s, i):
        """fp32 gradient of tensor i at step s, or None"""
        if i == self.none_tensor and s in self.none_steps:
            return None
        return self.q[s, self.off[i]:self.off[i + 1]].astype(np.float32) * self.scale[s]

    def groups_of(self, tensors):
        return [[t for t, g in zip(tensors, self.group) if g == 0], [t for t, g in zip(tensors, self.group) if g == 1]]

    def run_restated(self, dtype=torch.float32):
        """the recipe in torch on the CPU -> {(tag, name): flat float64 array}, total_norm per step"""
        params = [torch.from_numpy(self.initial(i)).to(dtype).requires_grad_(True) for i in range(len(self.numel))]
        opt = TorchRecipe(self.groups_of(params), self.wd)
        snaps, norms = {}, []
        for s in range(self.steps):
            opt.lr, opt.mom = float(self.lr[s]), float(self.mom[s])
            for i, p in enumerate(params):
                g = self.grad(s, i)
                p.grad = None if g is None else torch.from_numpy(g).to(dtype)
            norms.append(float(opt.step(dict(max_norm=self.max_norm, norm_type=2))))
            if s in self.snap_at:
                mom = opt.moments()
                snaps[self.snap_at[s], "p"] = np.concatenate([p.detach().double().numpy().ravel() for p in params])
                snaps[self.snap_at[s], "exp_avg"] = np.concatenate([m[0].double().numpy().ravel() for m in mom])
                snaps[self.snap_at[s], "exp_avg_sq"] = np.concatenate([m[1].double().numpy().ravel() for m in mom])
                snaps[self.snap_at[s], "step"] = np.asarray([m[2] for m in mom], np.int32)
        return snaps, np.asarray(norms, np.float64)


def rule(name, fused, restated, truth, lines=None):
    """The agreement rule: the fused result's maximum error against the float64 truth is at most 4 x the fp32 torch restatement's own
    maximum error against it, with a floor of one fp32 ulp of the quantity's largest magnitude.  Prints the figures, then asserts."""
    fused, restated, truth = (np.asarray(a, np.float64).ravel() for a in (fused, restated, truth))
    assert fused.shape == truth.shape == restated.shape, (name, fused.shape, restated.shape, truth.shape)
    e_fused = float(np.abs(fused - truth).max())
    e_torch = float(np.abs(restated - truth).max())
    floor = float(np.spacing(np.float32(np.abs(truth).max())))
    bound = max(4.0 * e_torch, floor)
    line = "%-44s fused err %.3e  torch fp32 err %.3e  ratio %s  ulp floor %.3e" % (
        name, e_fused, e_torch, "%.2f" % (e_fused / e_torch) if e_torch > 0 else "n/a", floor)
    print("[solver] " + line)
    if lines is not None:
        lines.append(line)
    assert np.isfinite(e_fused) and e_fused <= bound, line
    return e_fused, e_torch
