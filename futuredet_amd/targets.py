"""Training targets of the CenterHead on the device: the reference's AssignLabel stage (det3d/datasets/pipelines/preprocess.py:336-910,
NuScenesDataset branch) on fd_assign_targets (csrc/fd_targets.hip).

TargetAssigner(assigner_cfg, grid_size, pc_range, voxel_size)(boxes, counts, classes, trajectory)
        padded device annotations of a batch -> the loss-ready batched example, the layout of the reference's collate_kitti_multi
        (det3d/torchie/parallel/collate.py:208-241) that CenterHead.loss reads.
AssignLabel(cfg=assigner_cfg)(res, info)
        the registered pipeline stage: one sample, numpy in, numpy out (res["lidar"]["targets"]).
"""
import numpy as np
import torch

from . import hip_ops
from .lib import TargetsCfg
from .registry import PIPELINES

_TRAJECTORY = ("static", "linear", "nonlinear")  # preprocess.py:368-375: class 1, 2, 3 of the trajectory set
_FORECAST_CLASSES = 7
_ROW_KEYS = ("hm", "anno_box", "ind", "mask", "cat")


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class TargetAssigner(object):
    """Builds heat maps and box rows for a batch [B, T] on the device, every target set in two launches.

    ``assigner_cfg``: cfg.train_cfg.assigner (out_size_factor, gaussian_overlap, max_objs, min_radius, radius_mult, sampler_type,
    target_assigner.tasks); ``grid_size`` / ``pc_range`` / ``voxel_size``: the voxel geometry (what the Voxelization stage writes to
    res["lidar"]["voxels"] as shape / range / size).  A sampler_type other than "standard" adds the trajectory and forecast sets;
    it needs exactly one task (the reference indexes its one-task lists by the task index) and T <= 7."""

    def __init__(self, assigner_cfg, grid_size, pc_range, voxel_size):
        tasks = _get(_get(assigner_cfg, "target_assigner"), "tasks")
        self.class_names = [list(_get(t, "class_names")) for t in tasks]
        for t in tasks:
            if int(_get(t, "num_class")) != len(_get(t, "class_names")):
                raise ValueError("AssignLabel: num_class must equal len(class_names) in every task (preprocess.py:411-451 mixes the two)")
        if not 1 <= len(tasks) <= 16:
            raise ValueError("AssignLabel: 1 to 16 tasks (got %d)" % len(tasks))
        self.sampler_type = _get(assigner_cfg, "sampler_type", "standard")
        self.extra_sets = self.sampler_type != "standard"
        if self.extra_sets and len(tasks) != 1:
            raise ValueError("AssignLabel: the %r sampler builds one-task trajectory / forecast sets and needs one task (got %d); the "
                             "reference fails there with an IndexError" % (self.sampler_type, len(tasks)))
        self.max_objs = int(_get(assigner_cfg, "max_objs"))
        osf = _get(assigner_cfg, "out_size_factor")
        grid = np.asarray(grid_size)
        self.W, self.H = int(grid[0] // osf), int(grid[1] // osf)  # feature_map_size = grid_size[:2] // out_size_factor
        vs = np.asarray(voxel_size, dtype=np.float32)
        pr = np.asarray(pc_range, dtype=np.float32)
        self._cfg = TargetsCfg()
        c = self._cfg
        c.H, c.W, c.max_objs = self.H, self.W, self.max_objs
        c.n_sets = 3 if self.extra_sets else 1
        c.n_tasks = len(tasks)
        for i, names in enumerate(self.class_names):
            c.task_classes[i] = len(names)
        c.radius_mult = 1 if _get(assigner_cfg, "radius_mult", False) else 0
        c.min_radius = int(_get(assigner_cfg, "min_radius"))
        c.out_size_factor = float(np.float32(osf))
        c.voxel_x, c.voxel_y, c.pc_x, c.pc_y = float(vs[0]), float(vs[1]), float(pr[0]), float(pr[1])
        c.gaussian_overlap = float(_get(assigner_cfg, "gaussian_overlap"))
        self.channels = [len(n) for n in self.class_names] + ([3, _FORECAST_CLASSES] if self.extra_sets else [])
        self.sets = [("", 0, len(tasks))] + ([("_trajectory", len(tasks), 1), ("_forecast", len(tasks) + 1, 1)] if self.extra_sets else [])

    def outputs(self, B, T, device):
        """Flat output buffers of one call (fd_assign_targets' layout).  Pass them as ``out`` to reuse storage (a captured graph)."""
        U, mo = len(self.channels), self.max_objs
        n_hm = T * sum(self.channels) * B * self.H * self.W
        return dict(hm=torch.empty(((n_hm + 3) // 4 * 4,), dtype=torch.float32, device=device),
                    ind=torch.empty((T, U, B, mo), dtype=torch.int64, device=device),
                    mask=torch.empty((T, U, B, mo), dtype=torch.uint8, device=device),
                    cat=torch.empty((T, U, B, mo), dtype=torch.int64, device=device),
                    anno_box=torch.empty((T, U, B, mo, 14), dtype=torch.float32, device=device),
                    gt_boxes_and_cls=torch.empty((len(self.sets), T, B, mo, 13), dtype=torch.float32, device=device),
                    status=torch.empty((B, T, len(self.sets)), dtype=torch.int32, device=device))

    def __call__(self, boxes, counts, classes, trajectory=None, out=None, check=True):
        """boxes [B, T, n_max, 12] fp32, counts [B, T] int32, classes [B, T, n_max] int32 (1-based ids over all tasks' class names),
        trajectory [B, T, n_max] int32 (0 static, 1 linear, 2 nonlinear; needed by a non-standard sampler), all on the device.
        Returns the batched example: hm / anno_box / ind / mask / cat (and their _trajectory / _forecast twins) as lists over
        timesteps of lists over tasks of [B, ...] tensors, gt_boxes_and_cls* as lists over timesteps of [B, max_objs, 13], and
        "targets_status" ([B, T, sets] int32).  check=True reads the status back (a synchronisation) and raises AssertionError when
        a set holds more than max_objs objects, as the reference's assert does; check=False leaves that to check_status() (graphs)."""
        B, T, n_max = boxes.shape[:3]
        if self.extra_sets and T > _FORECAST_CLASSES:
            raise KeyError("AssignLabel: the forecast set has %d classes, T = %d (the reference's forecast_map has no key past _7)"
                           % (_FORECAST_CLASSES, T))
        if self.extra_sets and trajectory is None:
            raise ValueError("AssignLabel: the %r sampler needs trajectory ids" % self.sampler_type)
        self._cfg.T, self._cfg.n_max = int(T), int(n_max)
        out = out if out is not None else self.outputs(B, T, boxes.device)
        hip_ops.assign_targets(boxes, counts, classes, trajectory if self.extra_sets else None, self._cfg, out)
        if check:
            self.check_status(out["status"])
        return self.example(out, B, T)

    def example(self, out, B, T):
        """The batched example over the flat buffers of ``out`` (views, no copies)."""
        H, W = self.H, self.W
        csum = sum(self.channels)
        cbase = np.concatenate([[0], np.cumsum(self.channels)])
        ex = {}
        for si, (suffix, u0, nu) in enumerate(self.sets):
            hm, rows = [], {k: [] for k in _ROW_KEYS[1:]}
            for t in range(T):
                maps = []
                for u in range(u0, u0 + nu):
                    off = int((t * csum + cbase[u]) * B * H * W)
                    maps.append(out["hm"][off:off + B * self.channels[u] * H * W].view(B, self.channels[u], H, W))
                hm.append(maps)
                for k in rows:
                    rows[k].append([out[k][t, u] for u in range(u0, u0 + nu)])
            ex["hm" + suffix] = hm
            for k, v in rows.items():
                ex[k + suffix] = v
            ex["gt_boxes_and_cls" + suffix] = [out["gt_boxes_and_cls"][si, t] for t in range(T)]
        ex["targets_status"] = out["status"]
        return ex

    def check_status(self, status):
        bad = torch.nonzero(status.cpu()).tolist()
        if bad:
            b, t, s = bad[0]
            raise AssertionError("AssignLabel: %s set of sample %d, timestep %d holds more than max_objs = %d objects (preprocess.py:562)"
                                 % (("standard", "trajectory", "forecast")[s], b, t, self.max_objs))


@PIPELINES.register_module
class AssignLabel(object):
    """The reference's AssignLabel (preprocess.py:336-910, NuScenesDataset branch) on TargetAssigner with B = 1.

    Reads res["lidar"]["annotations"] as Preprocess (train mode) leaves it -- per annotation timestep gt_boxes [N, 12] float32,
    gt_classes (1-based ids over all tasks' class names), gt_names and gt_trajectory -- and res["lidar"]["voxels"] (shape, range,
    size); writes numpy targets to res["lidar"]["targets"], each key a list over timesteps (of lists over tasks).  Differences from the
    reference, none of which changes the targets:
      * res["lidar"]["annotations"] is left as it is.  The reference rewrites it per task in place; nothing downstream reads that
        (Reformat reads only the targets, formating.py:35).
      * the trajectory / forecast lists are built (and names checked against them, KeyError as in the reference) only for a
        non-standard sampler, the one that uses them.
      * a timestep without objects gives empty targets in every set (the reference raises an IndexError there for a non-standard
        sampler); a non-standard sampler with more than one task raises ValueError (the reference: IndexError).
    mode != "train" gives targets = {}; a dataset type other than NuScenesDataset raises NotImplementedError."""

    def __init__(self, **kwargs):
        self.cfg = kwargs["cfg"]
        self.sampler_type = _get(self.cfg, "sampler_type", "standard")
        self.tasks = _get(_get(self.cfg, "target_assigner"), "tasks")
        self._assigner = {}

    def _assigner_for(self, grid, pc_range, voxel_size):
        key = (tuple(np.asarray(grid).tolist()), tuple(np.asarray(pc_range, np.float32).tolist()), tuple(np.asarray(voxel_size, np.float32).tolist()))
        if key not in self._assigner:
            self._assigner[key] = TargetAssigner(self.cfg, grid, pc_range, voxel_size)
        return self._assigner[key]

    def __call__(self, res, info):
        if res["mode"] != "train":
            res["lidar"]["targets"] = {}
            return res, info
        if res["type"] != "NuScenesDataset":
            raise NotImplementedError("AssignLabel: only NuScenesDataset targets (got %r)" % (res["type"],))
        vox = res["lidar"]["voxels"]
        ta = self._assigner_for(vox["shape"], vox["range"], vox["size"])
        ann = res["lidar"]["annotations"]
        T = len(ann["gt_boxes"])
        n_max = max([len(b) for b in ann["gt_boxes"]] + [1])
        boxes = np.zeros((1, T, n_max, 12), np.float32)
        counts = np.zeros((1, T), np.int32)
        classes = np.zeros((1, T, n_max), np.int32)
        traj = np.zeros((1, T, n_max), np.int32)
        first = ta.class_names[0][0]
        classname = "car" if "car" in first else "pedestrian"  # preprocess.py:368-375
        for t in range(T):
            n = len(ann["gt_boxes"][t])
            counts[0, t] = n
            boxes[0, t, :n] = np.asarray(ann["gt_boxes"][t], np.float32).reshape(n, 12)
            classes[0, t, :n] = np.asarray(ann["gt_classes"][t]).reshape(n)
            if ta.extra_sets:
                for j, (name, tr) in enumerate(zip(ann["gt_names"][t], ann["gt_trajectory"][t])):
                    if name != classname or tr not in _TRAJECTORY:
                        raise KeyError("%s_%s" % (tr, name))  # the reference's trajectory_map lookup
                    traj[0, t, j] = _TRAJECTORY.index(tr)
        dev = torch.device("cuda")
        ex = ta(torch.from_numpy(boxes).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(classes).to(dev),
                torch.from_numpy(traj).to(dev) if ta.extra_sets else None)
        targets = {}
        for k, v in ex.items():
            if k == "targets_status":
                continue
            if k.startswith("gt_boxes_and_cls"):
                targets[k] = [x[0].cpu().numpy() for x in v]
            else:
                targets[k] = [[x[0].cpu().numpy() for x in per_t] for per_t in v]
        res["lidar"]["targets"] = targets
        return res, info
