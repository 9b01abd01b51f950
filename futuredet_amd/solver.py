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

    def hyper_values(self, grad_clip=None):
        """The six scalars of a step with the current lr / mom, validated: [lr, beta1, beta2, eps, wd, max_norm] (hip_ops.HYPER_FIELDS) --
        what a caller uploads into the device record of ``step(hyper=...)``."""
        return hip_ops.check_hyper(self._lr, self._mom, self._beta, self._eps, self._wd, parse_grad_clip(grad_clip))

    def _gather_gradients(self):
        """The table with this step's pointers, gradients and has-gradient flags in place (uploads only what changed)."""
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
        return tab

    def _step_dev(self, grad_clip, hyper, skip):
        clip = parse_grad_clip(grad_clip) > 0.0
        tab = self._gather_gradients()
        hip_ops.optim_adam_step_dev(tab, hyper, clip, skip)
        torch.autograd.graph.increment_version(tab.params)
        return tab.norm[0].clone() if clip else None

    def step(self, grad_clip=None, hyper=None, skip=None):
        """Decay, clip (``grad_clip`` = dict(max_norm=..., norm_type=2) or None) and Adam with the current lr / mom.  Returns the
        device tensor of total_norm when clipping is on.  A ``p.grad`` that is no longer the attached view is copied into it; None
        means no gradient this step: the tensor is decayed, its moments and step count stay.
        ``hyper`` (float64 [6] on the device, the values of ``hyper_values``): the step reads its scalars from that record when it
        RUNS, not when it is issued (fd_optim_adam_step_dev) -- a captured step follows the schedule; ``grad_clip`` still decides
        whether the norm is computed, its max_norm comes from the record.  ``skip`` (int32 [1] on the device): non-zero leaves
        parameters, moments and step counts as they are.  Without ``hyper`` the call is the one it always was."""
        if hyper is not None:
            return self._step_dev(grad_clip, hyper, skip)
        if skip is not None:
            raise ValueError("FusedAdam.step: skip needs the device record (hyper=...)")
        max_norm = parse_grad_clip(grad_clip)
        tab = self._gather_gradients()
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


class _StaticTrainBase(object):
    """What the sync-free training steps share: the static inputs (clouds and their counts, padded ground truth, the map of a bev_map
    head), the ring of pinned staging buffers, the device record of the optimiser's scalars, the iteration body and the restoring
    warm-up.  A subclass says which detector it takes (_check_model) and how one forward pass is issued (_forward)."""

    name = "_StaticTrainBase"

    def _check_model(self, model):
        raise NotImplementedError

    def _forward(self, clouds, counts, example, static):
        raise NotImplementedError

    def _guard(self, static, level_counts):
        """the device flag that turns this iteration's optimiser step into a no-op, or None"""
        return None

    def _init_common(self, model, voxel_cfg, assigner, optimizer, scheduler, grad_clip, capacity, batch_size, ndim, max_gt, timesteps, graph,
                     augment=None, filter_gt=False):
        name = self.name
        self._check_model(model)
        head = model.bbox_head
        if not getattr(head, "fused_loss", False):
            raise ValueError("%s: bbox_head.fused_loss is off; the torch loss copies its terms to the host "
                             "(set model.bbox_head.fused_loss = True)" % name)
        self.model, self.voxel_cfg, self.assigner, self.optimizer, self.scheduler = model, voxel_cfg, assigner, optimizer, scheduler
        if graph:
            raise NotImplementedError("%s: graph=True is not available -- ending the capture of the whole step crashed the HIP "
                                      "runtime; the step is issued eagerly without host synchronisation (graph=False)" % name)
        self.grad_clip = grad_clip
        parse_grad_clip(grad_clip)
        self.B, self.capacity, self.ndim = int(batch_size), int(capacity), int(ndim)
        self.T = int(timesteps if timesteps is not None else getattr(head, "timesteps", 1))
        self.max_gt = int(max_gt if max_gt is not None else assigner.max_objs)
        dev = next(model.parameters()).device
        self.device = dev
        B, T, n = self.B, self.T, self.max_gt
        self.points = torch.zeros((B, self.capacity, self.ndim), dtype=torch.float32, device=dev)
        self.counts = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.gt_boxes = torch.zeros((B, T, n, 12), dtype=torch.float32, device=dev)
        self.gt_counts = torch.zeros((B, T), dtype=torch.int32, device=dev)
        self.gt_classes = torch.zeros((B, T, n), dtype=torch.int32, device=dev)
        self.gt_trajectory = torch.zeros((B, T, n), dtype=torch.int32, device=dev) if assigner.extra_sets else None
        # the second input of a bev_map head (forecast_n3dtfm): [B, 6, H, W] on the head's feature map, filled from batch["bev_map"]
        self.bev = torch.zeros((B, 6, assigner.H, assigner.W), dtype=torch.float32, device=dev) if getattr(head, "bev_map", False) else None
        self.targets = assigner.outputs(B, T, dev)
        self.hyper = torch.zeros((len(hip_ops.HYPER_FIELDS),), dtype=torch.float64, device=dev)
        # augment (augment.GlobalAugment or None): the records of fd_augment_points / fd_augment_boxes, one per cloud, and the last draw
        self.augment, self.last_aug_params = augment, None
        self.aug_rec = torch.zeros((B, hip_ops.AUGMENT_RECORD_DOUBLES), dtype=torch.float64, device=dev) if augment is not None else None
        # augment.warp_bev: the step warps the batch's unwarped map into self.bev itself (fd_augment_mask), one record per sample
        self.mask_rec = None
        if self.bev is not None and getattr(augment, "warp_bev", False):
            from .augment import check_bev_size

            check_bev_size(self.bev)
            self.mask_rec = torch.zeros((B, hip_ops.AUGMENT_MASK_RECORD_DOUBLES), dtype=torch.float64, device=dev)
        # filter_gt: the reference's train-mode range filter (fd_gt_range_filter) on the static ground truth, over the voxel range
        self.filter_gt, self.gt_range, self.gt_filter_status = bool(filter_gt), None, None
        if self.filter_gt:
            from .augment import bev_range

            self.gt_range = bev_range(voxel_cfg["range"])
            self.gt_filter_status = torch.zeros((B,), dtype=torch.int32, device=dev)
        # augment.sampler (an augment.GTSampler): GT-database sampling while the batch is loaded -- the candidates' device copy, the
        # kernel's reports, and the stage a cloud is assembled in ([the sampled slots ; the scene]) before fd_augment_points reads it
        self.gt_sample = None
        if getattr(augment, "sampling", False):
            s = augment.sampler
            if s.database.points.shape[1] != self.ndim or s.database.points.device != dev:
                raise ValueError("%s: the sampler's database holds %d-column points on %s, the step takes %d columns on %s"
                                 % (name, s.database.points.shape[1], s.database.points.device, self.ndim, dev))
            if s.point_cap >= self.capacity:
                raise ValueError("%s: point_cap = %d leaves no room for a scene in clouds of capacity %d" % (name, s.point_cap, self.capacity))
            i32 = dict(dtype=torch.int32, device=dev)
            self.gt_sample = dict(cand=torch.full((B, s.K), -1, **i32), accepted=torch.zeros((B, s.K), **i32),
                                  plan=torch.zeros((B, s.K, hip_ops.GT_SAMPLE_PLAN_WORDS), **i32), n_points=torch.zeros((B,), **i32),
                                  status=torch.zeros((B,), **i32), groups=hip_ops.gt_sample_groups(s.records),
                                  stage=torch.zeros((B, s.point_cap + self.capacity, self.ndim), dtype=torch.float32, device=dev))
        self.last_gt_sample_candidates = None
        # augment.min_points > 0 (GlobalAugment(..., point_filter=True) on a cfg with min_points_in_gt): the point-count filter while the
        # batch is loaded -- the counts of every cloud's raw timestep-0 boxes, the filter's report, and the workspace of
        # fd_points_in_boxes_count (sized for a cloud of ``capacity`` rows and ``max_gt`` boxes when the first batch is loaded, i.e. at warm_up)
        self.point_filter = None
        if int(getattr(augment, "min_points", 0) or 0) > 0:
            self.point_filter = dict(min_points=int(augment.min_points), counts=torch.zeros((B, n), dtype=torch.int32, device=dev),
                                     status=torch.zeros((B,), dtype=torch.int32, device=dev), workspace=None)
        self._ring, self._slot = None, 0
        self.iteration = 0
        self.outputs, self.level_counts = None, None

    def __del__(self):
        try:
            hip_ops.workspace.release(id(self))
        except Exception:
            pass

    # -- inputs
    def _pinned(self):
        """a slot of the ring of pinned staging buffers (cloud counts, the six scalars, the event of its last copy, the augmentation
        records, the mask records, the GT-sampling candidates), free again once its last copy has run"""
        if self._ring is None:
            self._ring = [[torch.empty((self.B,), dtype=torch.int32).pin_memory(), torch.empty((6,), dtype=torch.float64).pin_memory(), None,
                           torch.empty((self.B, hip_ops.AUGMENT_RECORD_DOUBLES), dtype=torch.float64).pin_memory()
                           if self.augment is not None else None,
                           torch.empty((self.B, hip_ops.AUGMENT_MASK_RECORD_DOUBLES), dtype=torch.float64).pin_memory()
                           if getattr(self, "mask_rec", None) is not None else None,
                           torch.empty(tuple(self.gt_sample["cand"].shape), dtype=torch.int32).pin_memory()
                           if getattr(self, "gt_sample", None) is not None else None]
                          for _ in range(8)]
        slot = self._ring[self._slot % len(self._ring)]
        self._slot += 1
        if slot[2] is not None and not slot[2].query():
            slot[2].synchronize()  # (only when the stream is eight steps behind the host)
        return slot

    def _aug_params(self, batch):
        """this batch's augmentation parameters [B, 7]: batch["aug_params"], else a draw (for a bev_map head only with augment.warp_bev:
        otherwise its map must have been warped with the same parameters by whoever made the batch)"""
        from .augment import PARAM_FIELDS

        params = batch.get("aug_params")
        if params is None:
            if self.bev is not None and not getattr(self.augment, "warp_bev", False):
                raise ValueError("%s: augment with a bev_map head needs batch[\"aug_params\"] [%d, %d] and a \"bev_map\" already warped "
                                 "with them (the map warp, get_mask, is not built)" % (self.name, self.B, len(PARAM_FIELDS)))
            params = self.augment.draw(self.B)
        params = np.asarray(params, np.float64)
        if params.shape != (self.B, len(PARAM_FIELDS)):
            raise ValueError("aug_params %s: expected [%d, %d] (%s)" % (params.shape, self.B, len(PARAM_FIELDS), ", ".join(PARAM_FIELDS)))
        return params

    def _gt_candidates(self, batch):
        """this batch's GT-sampling candidates [B, K]: batch["gt_sample_candidates"], else a draw"""
        s = self.augment.sampler
        cand = batch.get("gt_sample_candidates")
        if cand is None:
            cand = s.draw(self.B)
        cand = np.asarray(cand, np.int32)
        if cand.shape != (self.B, s.K):
            raise ValueError("gt_sample_candidates %s: expected [%d, %d]" % (cand.shape, self.B, s.K))
        return cand

    def _load(self, batch, iteration):
        clouds = batch["clouds"]
        if len(clouds) != self.B:
            raise ValueError("the step was built for batches of %d clouds, got %d" % (self.B, len(clouds)))
        aug = self.augment
        gs = getattr(self, "gt_sample", None)
        grow = aug.sampler.point_cap if gs is not None else 0  # every cloud grows by exactly this many rows
        if gs is not None:
            for c in clouds:  # refused before anything of the step changes
                if int(c.shape[0]) + grow > self.capacity:
                    raise ValueError("cloud of %d rows + point_cap = %d sampled rows does not fit the step's capacity of %d rows"
                                     % (int(c.shape[0]), grow, self.capacity))
        params = self._aug_params(batch) if aug is not None else None  # (drawn or refused before anything of the step changes)
        cand = self._gt_candidates(batch) if gs is not None else None
        warp = getattr(self, "mask_rec", None) is not None
        mask_recs = aug.mask_record(params) if warp else None
        if self.bev is not None:
            bev = batch.get("bev_map")
            if bev is None:
                raise ValueError("the head was built with bev_map=True: the batch needs \"bev_map\" [%d, 6, %d, %d]"
                                 % (self.B, self.bev.shape[2], self.bev.shape[3]))
            if tuple(bev.shape) != tuple(self.bev.shape):
                raise ValueError("bev_map %s does not fit the step's %s buffer" % (tuple(bev.shape), tuple(self.bev.shape)))
        if self.scheduler is not None:
            self.scheduler.step(iteration)
        slot = self._pinned()
        counts_host, hyper_host = slot[0], slot[1]
        hyper_host.numpy()[:] = self.optimizer.hyper_values(self.grad_clip)
        if aug is not None:
            slot[3].numpy()[:] = aug.record(params).view(np.float64).reshape(self.B, -1)
            self.aug_rec.copy_(slot[3], non_blocking=True)
            self.last_aug_params = params
            if warp:
                slot[4].numpy()[:] = mask_recs.view(np.float64).reshape(self.B, -1)
                self.mask_rec.copy_(slot[4], non_blocking=True)
        if gs is not None:  # the ground truth first: the clouds are pasted from what the selection accepts
            slot[5].numpy()[:] = cand
            gs["cand"].copy_(slot[5], non_blocking=True)
            self.last_gt_sample_candidates = cand
            self._load_gt(batch)
        for b, c in enumerate(clouds):
            n = int(c.shape[0])
            if n > self.capacity or c.shape[1] != self.ndim:
                raise ValueError("cloud of %d x %d rows does not fit the step's %d x %d buffer" % (n, c.shape[1], self.capacity, self.ndim))
            if aug is None:
                self.points[b, :n].copy_(c, non_blocking=True)
            elif gs is None:  # the shuffle and the transforms, straight from the batch's tensor
                hip_ops.augment_points(c, self.aug_rec[b], self.points[b], perm=aug.permutation(n, self.device), n_rows=n)
            else:  # [the sampled slots ; the scene] in the stage, then one shuffle-and-transform over all of it
                stage = gs["stage"][b]
                hip_ops.gt_sample_points(aug.sampler.database, gs["cand"][b], gs["accepted"][b], gs["plan"][b], stage, grow)
                stage[grow:grow + n].copy_(c, non_blocking=True)
                hip_ops.augment_points(stage, self.aug_rec[b], self.points[b], perm=aug.permutation(n + grow, self.device), n_rows=n + grow)
            counts_host[b] = n + grow
        self.counts.copy_(counts_host, non_blocking=True)
        self.hyper.copy_(hyper_host, non_blocking=True)
        slot[2] = torch.cuda.Event()
        slot[2].record()
        if gs is None:
            self._load_gt(batch)
        if self.bev is not None:
            if warp:  # the batch's map is the unwarped one
                hip_ops.augment_mask(batch["bev_map"].contiguous(), self.mask_rec, out=self.bev)
            else:
                self.bev.copy_(batch["bev_map"], non_blocking=True)

    def _load_gt(self, batch):
        """the padded ground truth into the static buffers: copy, (point-count filter,) (GT-database sampling,) augmentation, (range
        filter)"""
        aug, gs, pf = self.augment, getattr(self, "gt_sample", None), getattr(self, "point_filter", None)
        boxes, gcounts, classes = batch["gt_boxes"], batch["gt_counts"], batch["gt_classes"]
        n = int(boxes.shape[2])
        if tuple(boxes.shape[:2]) != (self.B, self.T) or n > self.max_gt or boxes.shape[3] != 12:
            raise ValueError("gt_boxes %s do not fit the step's [%d, %d, <= %d, 12] buffer" % (tuple(boxes.shape), self.B, self.T, self.max_gt))
        if gs is not None or pf is not None:  # copy -> filter by points, select: in place (the step's counts from here on) -> transform -> filter
            self.gt_boxes[:, :, :n].copy_(boxes, non_blocking=True)
            if pf is None:
                self.gt_counts.copy_(gcounts, non_blocking=True)
            self.gt_classes[:, :, :n].copy_(classes, non_blocking=True)
            if self.gt_trajectory is not None:
                self.gt_trajectory[:, :, :n].copy_(batch["gt_trajectory"], non_blocking=True)
            if pf is not None:  # the counts: every RAW cloud against its raw timestep-0 boxes, below the batch's device count
                if pf["workspace"] is None:
                    pf["workspace"] = hip_ops.points_in_boxes_workspace(self.capacity, self.max_gt, self.device)
                raw, gc = boxes.contiguous(), gcounts.contiguous()
                for b, c in enumerate(batch["clouds"]):
                    hip_ops.points_in_boxes_count(c, raw[b, 0], n_boxes=gc[b, 0:1], out=pf["counts"][b, :n], workspace=pf["workspace"])
                hip_ops.gt_min_points_filter(self.gt_boxes, gc, self.gt_classes, pf["counts"], pf["min_points"], trajectory=self.gt_trajectory,
                                             out=(self.gt_boxes, self.gt_counts, self.gt_classes, self.gt_trajectory), status=pf["status"])
            if gs is not None:
                s = aug.sampler
                hip_ops.gt_sample_select(self.gt_boxes, self.gt_counts, self.gt_classes, s.database, gs["cand"], gs["groups"], s.rate, s.point_cap,
                                         trajectory=self.gt_trajectory, out="inplace", accepted=gs["accepted"], plan=gs["plan"],
                                         n_points=gs["n_points"], status=gs["status"])
            hip_ops.augment_boxes(self.gt_boxes, self.gt_counts, self.aug_rec, out=self.gt_boxes)
            if getattr(self, "filter_gt", False):
                hip_ops.gt_range_filter(self.gt_boxes, self.gt_counts, self.gt_classes, self.gt_range, trajectory=self.gt_trajectory,
                                        out="inplace", status=self.gt_filter_status)
            return
        if aug is not None and n == self.max_gt and boxes.is_contiguous():
            hip_ops.augment_boxes(boxes, gcounts, self.aug_rec, out=self.gt_boxes)
        else:
            self.gt_boxes[:, :, :n].copy_(boxes, non_blocking=True)
            if aug is not None:  # narrower than the buffer: in place, the counts never reach past column n
                hip_ops.augment_boxes(self.gt_boxes, gcounts, self.aug_rec, out=self.gt_boxes)
        filter_gt = getattr(self, "filter_gt", False)
        if not filter_gt:
            self.gt_counts.copy_(gcounts, non_blocking=True)
        self.gt_classes[:, :, :n].copy_(classes, non_blocking=True)
        if self.gt_trajectory is not None:
            self.gt_trajectory[:, :, :n].copy_(batch["gt_trajectory"], non_blocking=True)
        if filter_gt:  # in place on the static rows; the kernel reads the batch's counts and writes the step's
            hip_ops.gt_range_filter(self.gt_boxes, gcounts.contiguous(), self.gt_classes, self.gt_range, trajectory=self.gt_trajectory,
                                    out=(self.gt_boxes, self.gt_counts, self.gt_classes, self.gt_trajectory), status=self.gt_filter_status)

    # -- the step
    def _body(self, static):
        """every launch of one iteration, in order, on the current stream; nothing in it waits for the device when ``static``"""
        m, opt = self.model, self.optimizer
        if not m.training:
            m.train()
        opt.zero_grad()
        example = self.assigner(self.gt_boxes, self.gt_counts, self.gt_classes, self.gt_trajectory, out=self.targets, check=False)
        clouds = [self.points[b] for b in range(self.B)]
        counts = [self.counts[b:b + 1] for b in range(self.B)]
        losses = self._forward(clouds, counts, example, static)
        level_counts = m.last_level_counts
        skip = self._guard(static, level_counts)
        sum(losses["loss"]).backward()
        total_norm = opt.step(grad_clip=self.grad_clip, hyper=self.hyper, skip=skip)
        losses = dict(losses)
        if total_norm is not None:
            losses["total_norm"] = total_norm
        return losses, level_counts

    def _run_static(self):
        with hip_ops.workspace.scope(id(self)):  # scratch of its own, whatever stream the step is issued on
            return self._body(True)

    def _state(self):
        """every tensor a step changes: parameters and buffers of the model, the optimiser's moments and step counts"""
        tab = self.optimizer._table
        return list(self.model.state_dict(keep_vars=True).values()) + [tab.exp_avg, tab.exp_avg_sq, tab.step]

    def _restoring(self):
        """context: the model, the optimiser and its scheduled lr / mom leave as they came (warm-up steps are not training)"""
        step = self

        class _Restore(object):
            def __enter__(self_):
                self_.saved = [t.detach().clone() for t in step._state()]
                self_.lr_mom = (step.optimizer.lr, step.optimizer.mom)

            def __exit__(self_, *exc):
                with torch.no_grad():
                    for t, s in zip(step._state(), self_.saved):
                        t.detach().copy_(s)
                step.optimizer.lr, step.optimizer.mom = self_.lr_mom

        return _Restore()

    def _warm(self, batches):
        """eager steps (static=False) over ``batches`` inside _restoring(); returns the largest level counts seen, or None"""
        seen = None
        with self._restoring():
            for batch in batches:
                self._load(batch, self.iteration)
                self._body(False)
                counts = [int(v) for v in self.model.last_level_counts]
                seen = counts if seen is None else [max(a, b) for a, b in zip(seen, counts)]
        if seen is None:
            raise ValueError("%s.warm_up needs at least one batch" % self.name)
        return seen


class StaticTrainStep(_StaticTrainBase):
    """One whole training iteration of a VoxelNet -- zero_grad, voxeliser, index pyramid, AssignLabel's targets, sparse backbone, RPN,
    CenterHead, loss, backward, clipping and Adam -- issued without ever waiting for the device: detectors.StaticStep's counterpart for
    training, without its graph (see ``graph`` below).  Shapes are static: the clouds live in fixed-capacity buffers with
    their row counts on the device, the ground truth is padded to [B, T, max_gt, 12], the sparse levels are sized by row capacities
    and every kernel takes its count from device memory (VoxelNet.forward_points_train(static=True)); lr, beta1 and the other four
    scalars of the optimiser reach the kernels through a device record that is refreshed before every step
    (FusedAdam.step(hyper=...)): the launches do not bake the schedule in.

        step = StaticTrainStep(model, cfg.voxel_generator, assigner, optimizer, scheduler, grad_clip, capacity=400000, batch_size=2)
        step.warm_up(batches)                 # eager steps: conv plan choices + level counts; leaves model and optimiser as they were
        for batch in loader:                  # batch: dict(clouds=[B device tensors [N_i, ndim]], gt_boxes=[B, T, n, 12] fp32,
            losses = step(batch)              #             gt_counts=[B, T] int32, gt_classes=[B, T, n] int32[, gt_trajectory])

    ``step(batch)`` runs scheduler.step(iteration), uploads the six scalars, copies the batch into the static inputs and issues the
    launches.  It returns the model's loss dict (device tensors) with ``total_norm`` when clipping is on.  For a bev_map head (the
    forecast_n3dtfm configs) the batch also carries ``bev_map`` [B, 6, H, W] fp32 on the head's feature map; the step keeps it in a
    static buffer (``self.bev``) that the warm-up and the overflow re-run read too, and a batch without it raises ValueError.

    Row capacities (``row_caps="auto"``): ``headroom`` x the largest level counts of the warm-up batches + 4096.  A batch that needs
    more rows on some level sets a flag ON THE DEVICE (fd_levels_overflow) that makes the optimiser step of that iteration a no-op:
    parameters, moments and step counts stay.  With ``check=True`` (default) the level counts are read back after the step -- the one
    synchronisation of the call -- and an overflowed batch is re-run on the host-sized path (forward_points_train(static=False))
    with the same scheduler iteration, so step counts and the iteration advance exactly once.  ``check=False`` keeps the call
    asynchronous; ask ``overflowed()`` later.  What an overflowed step leaves behind: the BatchNorm running statistics (and
    num_batches_tracked) were updated once by its forward pass, on a truncated but valid batch, before the re-run updates them again.

    ``augment`` (an augment.GlobalAugment; None = none, today's launches): the step draws one set of parameters per cloud (or takes
    batch["aug_params"] [B, 7]), keeps them in ``last_aug_params``, uploads their records through the staging ring, and loads the
    batch through fd_augment_points -- one launch per cloud, shuffle and transforms, in place of the copy -- and one fd_augment_boxes.
    The warm-up and the overflow re-run read the static buffers, so they see the augmented batch once.  With a bev_map head and
    ``GlobalAugment(..., warp_bev=True)`` the batch carries the UNWARPED ``bev_map`` [B, 6, 180, 180]: the step uploads one mask record
    per sample through the same ring and warps the map into ``self.bev`` with fd_augment_mask (the reference's ``get_mask``) in place
    of the copy.  With ``warp_bev=False`` the batch must carry ``aug_params`` and a ``bev_map`` already warped with them, else
    ValueError.

    ``filter_gt`` (False = today's launches): after the boxes are loaded (and augmented), fd_gt_range_filter drops, at every
    timestep, the objects whose timestep-0 box has no BEV corner inside the x / y bounds of ``voxel_cfg["range"]`` -- the train-mode
    filter of the reference's Voxelization stage -- in place on the static ground truth; ``gt_counts`` is then written by the kernel
    and ``gt_filter_status`` [B] counts the timesteps of a sample whose count differed from timestep 0's.  Works with ``augment=None``.

    GT-database sampling (``augment=GlobalAugment(..., sampler=GTSampler(...))``; without a sampler today's launches and buffers): the
    step draws the candidates (or takes ``batch["gt_sample_candidates"]`` [B, K]; the last ones are ``last_gt_sample_candidates``),
    uploads them through the same ring, copies the ground truth into the static buffers, runs fd_gt_sample_select in place on them,
    then fd_augment_boxes and the range filter with the step's counts; every cloud is assembled as [the sampled slots ; the scene] in
    a stage of [B, point_cap + capacity, ndim] (fd_gt_sample_points, a copy) and goes through one fd_augment_points over
    n + point_cap rows, so the cloud counts stay host-known.  A cloud with n + point_cap > capacity raises ValueError before anything
    of the step changes.  ``gt_sample["accepted"]`` [B, K], ``["n_points"]`` and ``["status"]`` [B] hold the kernel's reports.

    The point-count filter (``augment=GlobalAugment(..., point_filter=True)`` on a cfg with ``min_points_in_gt > 0``; inactive = today's
    launches and buffers): while the ground truth is loaded, one fd_points_in_boxes_count per cloud -- the batch's RAW cloud against its
    raw timestep-0 boxes, below the batch's device count -- fills ``point_filter["counts"]`` [B, max_gt], and one
    fd_gt_min_points_filter for the batch drops, at every timestep, the objects with fewer points, in place on the static ground
    truth, before the sampler's selection and before the transforms: what ``aug(batch)`` does.  ``point_filter["status"]`` [B] counts
    the timesteps of a sample whose count differed from timestep 0's.  No host synchronisation.

    ``graph``: only False.  Everything in the step is capturable by construction (static shapes, device counts, device scalars, a
    device-side overflow guard, nothing keyed on the weights' version), but capturing it -- MIOpen's convolutions and their backward
    included -- crashed the HIP runtime when the capture was ended (torch 2.10 on ROCm 7, MI355X; DESIGN.md "The sync-free training
    step"), so the capture is not part of the class; ``graph=True`` raises NotImplementedError.  One StaticTrainStep belongs to one stream."""

    name = "StaticTrainStep"

    def __init__(self, model, voxel_cfg, assigner, optimizer, scheduler=None, grad_clip=None, capacity=400000, batch_size=1, ndim=5,
                 max_gt=None, timesteps=None, row_caps="auto", headroom=1.5, graph=False, augment=None, filter_gt=False):
        self._init_common(model, voxel_cfg, assigner, optimizer, scheduler, grad_clip, capacity, batch_size, ndim, max_gt, timesteps, graph,
                          augment, filter_gt)
        self.row_caps_mode, self.headroom = row_caps, float(headroom)
        self.skip = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.expected, self.caps, self.caps_dev = None, None, None

    def _check_model(self, model):
        from .detectors import VoxelNet

        if not isinstance(model, VoxelNet):
            raise NotImplementedError("StaticTrainStep: %s is not a VoxelNet; the static training step covers the sparse-backbone detector "
                                      "only (PointPillars trains through StaticPillarsTrainStep)" % type(model).__name__)
        head, bb = model.bbox_head, model.backbone
        if getattr(head, "dcn_head", False):
            raise NotImplementedError("StaticTrainStep: a dcn_head CenterHead is not covered (dcn_head=True); train it through train_steps")
        if not getattr(bb, "fused_bn", False):
            raise ValueError("StaticTrainStep: backbone.fused_bn is off; torch's BatchNorm1d cannot take its row count from the device "
                             "(set model.backbone.fused_bn = True)")

    def reset(self):
        """drops the row capacities (the next call derives them again from ``row_caps`` and the warm-up counts)"""
        self.caps, self.caps_dev, self.outputs = None, None, None

    def _forward(self, clouds, counts, example, static):
        return self.model.forward_points_train(clouds, self.voxel_cfg, example, counts=counts, static=static,
                                               row_caps=self.caps if static else None, bev_map=self.bev)

    def _guard(self, static, level_counts):
        if not (static and self.caps_dev is not None):
            return None
        hip_ops.levels_overflow(level_counts, self.caps_dev, self.skip)
        return self.skip

    def warm_up(self, batches):
        """Eager steps on the host-sized path (forward_points_train(static=False)) over representative batches: lets the dense
        convolutions pick their kernels, fixes the optimiser's gradient set and pointer table, and records the largest level counts
        (the capacities of row_caps="auto").  The model, the optimiser and the iteration count are restored afterwards."""
        self.expected = self._warm(batches)
        self.reset()

    def _set_caps(self):
        mv = self.voxel_cfg["max_voxel_num"]
        cap0 = self.B * int(mv[0] if isinstance(mv, (list, tuple)) else mv)
        if self.row_caps_mode == "datafree":
            self.caps, self.caps_dev = None, None
            return
        if self.row_caps_mode == "auto":
            if self.expected is None:
                raise RuntimeError("StaticTrainStep.warm_up(batches) must run before the first step (row_caps=\"auto\")")
            self.caps = [cap0] + [int(self.headroom * e) + 4096 for e in self.expected[1:]]  # (level 0 is capped by the voxeliser itself)
        else:
            self.caps = [int(c) for c in self.row_caps_mode]
        if self.model.backbone.train_dtype == torch.float32 and max(self.caps[1:]) >= (1 << 23):
            raise NotImplementedError("StaticTrainStep: a sparse level with a row capacity >= 2^23 (fp32 kernel limit); use a smaller batch")
        self.caps_dev = torch.tensor(self.caps, dtype=torch.int32).to(self.device)

    def __call__(self, batch, check=True):
        """One iteration on ``batch`` (see the class).  ``check``: read the level counts back after the step and re-run an overflowed
        batch on the host-sized path -- one synchronisation, at the end."""
        if self.caps is None and self.row_caps_mode != "datafree":  # first call, or after warm_up() / reset()
            self._set_caps()
        self._load(batch, self.iteration)
        self.outputs, self.level_counts = self._run_static()
        if check and self.caps is not None and self.overflowed():
            self.outputs, _ = self._body(False)  # the device skipped the update; same record of scalars, same iteration
        self.iteration += 1
        return self.outputs

    def overflowed(self, level_counts_host=None):
        """True when the last step needed more rows on some level than its capacities: the device has skipped its optimiser update and
        the batch has to be run again (``step(batch)`` with check=True does).  Synchronises unless the counts are passed in."""
        if self.caps is None or self.level_counts is None:
            return False
        lc = self.level_counts.cpu().tolist() if level_counts_host is None else [int(v) for v in level_counts_host]
        return any(n > c for n, c in zip(lc, self.caps))


class StaticPillarsTrainStep(_StaticTrainBase):
    """StaticTrainStep's counterpart for PointPillars: zero_grad, per-cloud voxeliser with point slots, targets, the train-mode pillar
    reader with its counts on the device, scatter, RPN, CenterHead, loss, backward, clipping and Adam, issued without ever waiting for
    the device (PointPillars.forward_points_train(static=True)).  The batch contract, the staging ring, the device record of the
    optimiser's scalars and ``warm_up`` are StaticTrainStep's:

        step = StaticPillarsTrainStep(model, cfg.voxel_generator, assigner, optimizer, scheduler, grad_clip, capacity=400000, batch_size=2)
        step.warm_up(batches)                 # eager steps (static=False); leaves model and optimiser as they were
        for batch in loader:
            losses = step(batch)

    There are no row capacities and no overflow guard: the voxeliser caps the pillars of a cloud at max_voxel_num[0] and every buffer
    has that size, so ``overflowed()`` is False and ``check`` reads nothing back.  Needs bbox_head.fused_loss; a bev_map head takes
    batch["bev_map"]; neck / bbox_head train_dtype = torch.bfloat16 and the dense fused_bn switches work as in train_steps.  The
    reader trains in fp32.  ``augment``, ``filter_gt``: as for StaticTrainStep.  ``graph``: only False, as for StaticTrainStep."""

    name = "StaticPillarsTrainStep"

    def __init__(self, model, voxel_cfg, assigner, optimizer, scheduler=None, grad_clip=None, capacity=400000, batch_size=1, ndim=5,
                 max_gt=None, timesteps=None, graph=False, augment=None, filter_gt=False):
        self._init_common(model, voxel_cfg, assigner, optimizer, scheduler, grad_clip, capacity, batch_size, ndim, max_gt, timesteps, graph,
                          augment, filter_gt)
        if not 1 <= self.B <= 16:
            raise ValueError("StaticPillarsTrainStep: the pillar reader takes 1 to 16 clouds per batch (got %d)" % self.B)

    def _check_model(self, model):
        from .detectors import PointPillars

        if not isinstance(model, PointPillars):
            raise NotImplementedError("StaticPillarsTrainStep: %s is not a PointPillars detector (a VoxelNet trains through "
                                      "StaticTrainStep)" % type(model).__name__)
        if getattr(model.bbox_head, "dcn_head", False):
            raise NotImplementedError("StaticPillarsTrainStep: a dcn_head CenterHead is not covered (dcn_head=True); train it through "
                                      "train_steps")

    def _forward(self, clouds, counts, example, static):
        return self.model.forward_points_train(clouds, self.voxel_cfg, example, counts=counts, static=static, bev_map=self.bev)

    def warm_up(self, batches):
        """Eager steps on the host-count path (forward_points_train(static=False)) over representative batches: lets the dense convolutions
        pick their kernels and fixes the optimiser's gradient set and pointer table.  The model, the optimiser and the iteration count
        are restored afterwards."""
        self._warm(batches)

    def __call__(self, batch, check=True):
        """One iteration on ``batch``.  ``check`` is accepted for StaticTrainStep's signature: nothing can overflow, nothing is read back."""
        self._load(batch, self.iteration)
        self.outputs, self.level_counts = self._run_static()
        self.iteration += 1
        return self.outputs

    def overflowed(self, level_counts_host=None):
        return False


__all__ = ["FusedAdam", "OneCycle", "LRSchedulerStep", "annealing_cos", "parameter_groups", "parse_grad_clip", "build_one_cycle_optimizer",
           "create_learning_rate_scheduler", "train_steps", "StaticTrainStep", "StaticPillarsTrainStep"]
