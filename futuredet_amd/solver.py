"""The training recipe of every shipped config on the device:

    optimizer        = dict(type="adam", amsgrad=0.0, wd=0.01, fixed_wd=True, moving_average=False)
    lr_config        = dict(type="one_cycle", lr_max=0.001, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4)
    optimizer_config = dict(grad_clip=dict(max_norm=35, norm_type=2))

In the reference that is fastai's OptimWrapper over torch.optim.Adam(betas=(0.9, 0.99)) with true weight decay on every parameter
(det3d/solver/fastai_optim.py:121-270, det3d/torchie/apis/train.py:161-200), OneCycle moving lr and beta1 at every iteration
(det3d/solver/learning_schedules_fastai.py:7-95) and clip_grad_norm_ from OptimizerHook (det3d/torchie/trainer/hooks/optimizer.py),
in the order of Trainer.train (det3d/torchie/trainer/trainer.py:436-460).  Here one ``FusedAdam.step`` is at most three launches of
fd_optim.hip whatever the number of tensors: gradients live in one flat device buffer (each ``p.grad`` is a view of it), the clip
coefficient stays on the device, and nothing in ``step`` waits for the GPU.

The one intended difference from the reference: clipping scales the gradients on the fly and does NOT rewrite ``p.grad`` (the
reference leaves them scaled in place; nothing reads them before the next ``zero_grad``).

Out of scope: DDP, datasets and loaders, the Trainer hook system and checkpoint writing, ``amsgrad``, ``fixed_wd=False`` and a
``norm_type`` other than 2.  There is no CPU implementation: parameters must be contiguous fp32 tensors on the HIP device.
"""
import functools
import math  # noqa: F401  (in scope for phase functions given as strings, as in the reference's module)

import numpy as np
import torch
from torch import nn

from . import hip_ops

_BN = nn.modules.batchnorm._BatchNorm


# ------------------------------------------------------------------------------------------------ schedule
def annealing_cos(start, end, pct):
    """cosine from ``start`` (pct = 0) to ``end`` (pct = 1), in float64 with the reference's operation order"""
    return end + (start - end) / 2 * (np.cos(np.pi * pct) + 1)


class LRSchedulerStep(object):
    """Piecewise schedules of ``optimizer.lr`` and ``optimizer.mom`` over ``total_step`` iterations.  A phase is (start fraction,
    function of the phase's progress in [0, 1)); phase i runs from int(start_i * total_step) to the next phase's first step, and the
    last phase that has begun sets the value.  A function given as a string is evaluated, as the reference's multi_phase configs
    expect."""

    def __init__(self, optimizer, total_step, lr_phases, mom_phases):
        self.optimizer, self.total_step = optimizer, total_step
        self.lr_phases = self._spans(lr_phases, total_step, fractional_check=False)
        assert self.lr_phases[0][0] == 0
        self.mom_phases = self._spans(mom_phases, total_step, fractional_check=True)
        if self.mom_phases:
            assert self.mom_phases[0][0] == 0

    @staticmethod
    def _spans(phases, total_step, fractional_check):
        phases = list(phases)
        spans = []
        for i, (start, fn) in enumerate(phases):
            first = int(start * total_step)
            if spans:
                # lr phases must begin at increasing STEPS (total_step 1 or 2 fails here for a one-cycle); the reference compares
                # the momentum phases' previous first step with the next start FRACTION, which this keeps
                assert spans[-1][0] < (start if fractional_check else first)
            if isinstance(fn, str):
                fn = eval(fn)
            end = int(phases[i + 1][0] * total_step) if i + 1 < len(phases) else total_step
            spans.append((first, end, fn))
        return spans

    @staticmethod
    def _value(spans, step):
        value = None
        for first, end, fn in spans:
            if step >= first:
                value = fn((step - first) / (end - first))
        return value

    def step(self, step):
        lr, mom = self._value(self.lr_phases, step), self._value(self.mom_phases, step)
        if lr is not None:
            self.optimizer.lr = lr
        if mom is not None:
            self.optimizer.mom = mom


class OneCycle(LRSchedulerStep):
    """lr: lr_max / div_factor -> lr_max over the first pct_start of the run, then -> lr_max / div_factor / 1e4; beta1: moms[0] ->
    moms[1] and back; both on cosines."""

    def __init__(self, optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.lr_max, self.moms, self.div_factor, self.pct_start = lr_max, moms, div_factor, pct_start
        low = lr_max / div_factor
        optimizer.lr, optimizer.mom = low, moms[0]
        up, down = tuple(moms), tuple(moms)[::-1]
        super().__init__(optimizer, total_step,
                         ((0, functools.partial(annealing_cos, low, lr_max)), (pct_start, functools.partial(annealing_cos, lr_max, low / 1e4))),
                         ((0, functools.partial(annealing_cos, *up)), (pct_start, functools.partial(annealing_cos, *down))))


# ------------------------------------------------------------------------------------------------ parameter groups
def parameter_groups(model):
    """The reference's two groups, OptimWrapper.create(..., get_layer_groups(model)): the leaf modules of ``model`` in
    ``model.modules()`` order, split into non-BatchNorm and BatchNorm leaves; each group lists its leaves' trainable parameters.
    Returns two lists of (name, parameter).  (A parameter held directly by a module that also has children is in neither group,
    there and here.)"""
    groups, seen = ([], []), set()
    for mname, m in model.named_modules():
        if next(m.children(), None) is not None:
            continue
        g = groups[1] if isinstance(m, _BN) else groups[0]
        for pname, p in m.named_parameters(recurse=False):
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                g.append(((mname + "." if mname else "") + pname, p))
    return groups


def parse_grad_clip(grad_clip):
    """``optimizer_config.grad_clip`` -> max_norm (0.0: no clipping)"""
    if grad_clip is None:
        return 0.0
    norm_type = grad_clip.get("norm_type", 2)
    if isinstance(norm_type, str) or float(norm_type) != 2.0:
        raise NotImplementedError("grad_clip norm_type=%r: the fused step computes the 2-norm only" % (norm_type,))
    max_norm = float(grad_clip["max_norm"])
    if not max_norm > 0.0:
        raise ValueError("grad_clip max_norm must be positive, got %r" % (grad_clip["max_norm"],))
    return max_norm


# ------------------------------------------------------------------------------------------------ optimiser
class FusedAdam(object):
    """Adam with true weight decay and gradient clipping on fd_optim.hip, with the surface of the reference's OptimWrapper:
    ``lr`` / ``mom`` (beta1) / ``beta`` (beta2) / ``wd`` properties that a scheduler sets, ``step``, ``zero_grad``, ``state_dict`` /
    ``load_state_dict`` in torch.optim.Adam's format over the two groups (what a reference checkpoint's "optimizer" entry holds).

    ``groups``: (non-BatchNorm parameters, BatchNorm parameters), e.g. from ``parameter_groups(model)`` (names are optional)."""

    def __init__(self, groups, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, wd=0.0, true_wd=True, bn_wd=True, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("amsgrad=%r: the fused step keeps no running maximum of exp_avg_sq" % (amsgrad,))
        if not true_wd:
            raise NotImplementedError("fixed_wd / true_wd=False (weight decay folded into the gradient) is not implemented")
        groups = [[e[1] if isinstance(e, (tuple, list)) else e for e in g] for g in groups]
        if len(groups) != 2:
            raise ValueError("FusedAdam takes two groups (non-BatchNorm, BatchNorm), got %d" % len(groups))
        self.group_sizes = [len(g) for g in groups]
        params = groups[0] + groups[1]
        for i, p in enumerate(params):
            if isinstance(p, torch.Tensor) and p.is_cuda and not p.is_contiguous():
                raise ValueError("parameter %d is not contiguous: the fused step addresses parameters as flat arrays" % i)
        self._table = hip_ops.AdamTable(params, [True] * len(groups[0]) + [bool(bn_wd)] * len(groups[1]))
        self._lr, self._mom, self._beta, self._eps, self._wd = float(lr), float(betas[0]), float(betas[1]), float(eps), float(wd)
        self.true_wd, self.bn_wd = True, bool(bn_wd)
        self._views = [self._table.segment(self._table.grad, i) for i in range(len(params))]
        self._attach()

    # -- the two ways the reference builds one
    @classmethod
    def for_model(cls, model, **kwargs):
        return cls(parameter_groups(model), **kwargs)

    @classmethod
    def create(cls, opt_func, lr, layer_groups, wd=0.0, true_wd=False, bn_wd=True):
        """OptimWrapper.create(partial(torch.optim.Adam, betas=..., amsgrad=...), lr, get_layer_groups(model), wd=..., true_wd=...,
        bn_wd=...): ``layer_groups`` is one container of leaf modules."""
        func, kw = getattr(opt_func, "func", opt_func), dict(getattr(opt_func, "keywords", None) or {})
        if func is not torch.optim.Adam:
            raise NotImplementedError("opt_func %r: only torch.optim.Adam has a fused step" % (func,))
        layer_groups = list(layer_groups)
        if len(layer_groups) != 1:
            raise NotImplementedError("%d layer groups: the shipped recipe has one" % len(layer_groups))
        return cls(parameter_groups(layer_groups[0]), lr=lr[-1] if isinstance(lr, (list, tuple)) else lr, betas=kw.get("betas", (0.9, 0.999)),
                   eps=kw.get("eps", 1e-8), wd=wd, true_wd=true_wd, bn_wd=bn_wd, amsgrad=kw.get("amsgrad", False))

    # -- hyper-parameters
    @staticmethod
    def _last(v):
        return float(v[-1] if isinstance(v, (list, tuple)) else v)

    lr = property(lambda self: self._lr, lambda self, v: setattr(self, "_lr", self._last(v)))
    mom = property(lambda self: self._mom, lambda self, v: setattr(self, "_mom", self._last(v)))
    beta = property(lambda self: self._beta, lambda self, v: None if v is None else setattr(self, "_beta", self._last(v)))
    wd = property(lambda self: self._wd, lambda self, v: setattr(self, "_wd", self._last(v)))

    @property
    def params(self):
        return self._table.params

    @property
    def param_groups(self):
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)  # this torch's keys, so the dict loads into its Adam
        defaults.update(lr=self._lr, betas=(self._mom, self._beta), eps=self._eps, weight_decay=0, amsgrad=False)
        n0, n1 = self.group_sizes
        return [dict(defaults, params=list(range(n0))), dict(defaults, params=list(range(n0, n0 + n1)))]

    # -- gradients
    def _attach(self):
        for p, v in zip(self._table.params, self._views):
            if p.grad is not v:
                p.grad = v

    def zero_grad(self):
        """one launch over the flat buffer; every ``p.grad`` is (again) its view of it, so backward accumulates in place"""
        hip_ops.optim_zero_grad(self._table)
        self._attach()

    def step(self, grad_clip=None):
        """Decay, clip (``grad_clip`` = dict(max_norm=..., norm_type=2) or None) and Adam with the current lr / mom.  Returns the
        device tensor of total_norm when clipping is on.  A ``p.grad`` that is no longer the attached view is copied into it; None
        means no gradient this step: the tensor is decayed, its moments and step count stay."""
        max_norm = parse_grad_clip(grad_clip)
        tab = self._table
        tab.sync_pointers()
        has_grad = []
        with torch.no_grad():
            for p, v in zip(tab.params, self._views):
                g = p.grad
                if g is not None and g is not v and (g.data_ptr() != v.data_ptr() or g.shape != v.shape or not g.is_contiguous()):
                    if not g.is_cuda:
                        raise hip_ops.FutureDetHipError("a gradient lives on the CPU; this path has no CPU implementation")
                    v.copy_(g)
                has_grad.append(g is not None)
        tab.set_has_grad(has_grad)
        hip_ops.optim_adam_step(tab, self._lr, self._mom, self._beta, self._eps, self._wd, max_norm)
        # the kernel wrote through raw pointers: weights_version (folded / packed weight caches, captured graphs) looks at _version
        torch.autograd.graph.increment_version(tab.params)
        return tab.norm[0].clone() if max_norm > 0.0 else None

    # -- state
    def state_dict(self):
        tab = self._table
        steps = tab.step.cpu().tolist()
        state = {}
        for i, s in enumerate(steps):
            if s > 0:  # torch creates a parameter's state at its first gradient
                state[i] = dict(step=torch.tensor(float(s)), exp_avg=tab.segment(tab.exp_avg, i).clone(),
                                exp_avg_sq=tab.segment(tab.exp_avg_sq, i).clone())
        return dict(state=state, param_groups=self.param_groups)

    def load_state_dict(self, sd):
        tab = self._table
        sizes = [len(g["params"]) for g in sd["param_groups"]]
        if sizes != self.group_sizes:
            raise ValueError("the state dict has parameter groups of %s tensors, this optimiser %s" % (sizes, self.group_sizes))
        order = [i for g in sd["param_groups"] for i in g["params"]]
        steps = []
        with torch.no_grad():
            for i, key in enumerate(order):
                st = sd["state"].get(key, sd["state"].get(str(key)))
                m, v = tab.segment(tab.exp_avg, i), tab.segment(tab.exp_avg_sq, i)
                if st is None:
                    m.zero_(), v.zero_(), steps.append(0)
                    continue
                if st.get("max_exp_avg_sq") is not None:
                    raise NotImplementedError("the state dict comes from an amsgrad optimiser")
                if tuple(st["exp_avg"].shape) != tuple(m.shape):
                    raise ValueError("state of parameter %d has shape %s, the parameter %s" % (i, tuple(st["exp_avg"].shape), tuple(m.shape)))
                m.copy_(st["exp_avg"]), v.copy_(st["exp_avg_sq"])
                steps.append(int(round(float(st["step"]))))
            tab.step.copy_(torch.tensor(steps, dtype=torch.int32))
        g0 = sd["param_groups"][0]
        self._lr, self._eps = float(g0.get("lr", self._lr)), float(g0.get("eps", self._eps))
        self._mom, self._beta = (float(b) for b in g0.get("betas", (self._mom, self._beta)))

    def __repr__(self):
        return "FusedAdam over %d + %d tensors (%d elements), lr=%g betas=(%g, %g) eps=%g wd=%g" % (
            self.group_sizes[0], self.group_sizes[1], sum(self._table.numel), self._lr, self._mom, self._beta, self._eps, self._wd)


# ------------------------------------------------------------------------------------------------ builders and the loop
def _opt(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def build_one_cycle_optimizer(model, optimizer_cfg):
    """det3d/torchie/apis/train.py:183-200 for the shipped ``optimizer`` dict: Adam(betas=(0.9, 0.99)), true weight decay ``wd`` on
    both groups.  The learning rate is whatever the scheduler sets before the first step."""
    kind = _opt(optimizer_cfg, "type", "adam")
    if kind != "adam":
        raise NotImplementedError("optimizer type=%r: only 'adam' is implemented" % (kind,))
    if not _opt(optimizer_cfg, "fixed_wd", False):
        raise NotImplementedError("optimizer fixed_wd=%r: only fixed_wd=True (true weight decay) is implemented" % (_opt(optimizer_cfg, "fixed_wd"),))
    if _opt(optimizer_cfg, "amsgrad", False):
        raise NotImplementedError("optimizer amsgrad=%r is not implemented" % (_opt(optimizer_cfg, "amsgrad"),))
    return FusedAdam.for_model(model, lr=3e-3, betas=(0.9, 0.99), wd=_opt(optimizer_cfg, "wd", 0.0), true_wd=True, bn_wd=True)


def create_learning_rate_scheduler(optimizer, lr_config, total_step):
    """det3d/builder.py:153-184 for the shipped ``lr_config`` (type one_cycle)"""
    kind = _opt(lr_config, "type")
    if kind != "one_cycle":
        raise NotImplementedError("lr_config type=%r: only 'one_cycle' is implemented" % (kind,))
    return OneCycle(optimizer, total_step, _opt(lr_config, "lr_max"), _opt(lr_config, "moms"), _opt(lr_config, "div_factor"), _opt(lr_config, "pct_start"))


def train_steps(model, batches, optimizer, scheduler, grad_clip=None, start_iter=0):
    """A minimal training loop in the order of Trainer.train + OptimizerHook.after_train_iter: scheduler.step(iter), forward with
    return_loss=True, zero_grad, backward of the summed loss, clip, step.  ``batches``: any iterable of collated examples on the
    device.  Yields the model's loss dict per iteration, with ``total_norm`` (device tensor) added when clipping is on."""
    model.train()
    for i, example in enumerate(batches, start_iter):
        if scheduler is not None:
            scheduler.step(i)
        losses = model(example, return_loss=True)
        optimizer.zero_grad()
        sum(losses["loss"]).backward()
        total_norm = optimizer.step(grad_clip=grad_clip)
        if total_norm is not None:
            losses = dict(losses, total_norm=total_norm)
        yield losses


__all__ = ["FusedAdam", "OneCycle", "LRSchedulerStep", "annealing_cos", "parameter_groups", "parse_grad_clip", "build_one_cycle_optimizer",
           "create_learning_rate_scheduler", "train_steps"]
