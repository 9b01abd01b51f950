"""Global training augmentation on the device: the live train-mode path of the reference's ``Preprocess`` stage
(det3d/datasets/pipelines/preprocess.py:189-192, 201-203) for the shipped configs -- the fixed-seed point shuffle, then
``prep.random_flip_both``, ``prep.global_rotation``, ``prep.global_scaling_v2`` and ``prep.global_translate_`` on the cloud and on every
timestep's [N, 12] box rows (fd_augment.hip; include/futuredet_hip.h has the arithmetic) -- and what the reference does between them and
the target assignment (fd_augment_map.hip): the warp of a bev_map head's 180 x 180 mask with the same draw (``get_mask``,
preprocess.py:75-90, 212: two cv2.warpAffine calls, restated in the header) and the ground-truth range filter of the train-mode
``Voxelization`` stage (preprocess.py:249-255, ``prep.filter_gt_box_outside_range``).

    aug = GlobalAugment(cfg.train_preprocessor, seed=0, warp_bev=True)   # warp_bev: also warp batch["bev_map"] (the n3dtfm configs)
    step = StaticTrainStep(..., augment=aug, filter_gt=True)   # the step draws, uploads its records, transforms while it loads the
                                                               # batch, warps the map and filters the ground truth by the voxel range
    batch = filter_gt_outside_range(aug(batch), cfg.voxel_generator["range"])   # or: a new batch dict for train_steps

GT-database sampling ("GT-AUG", the stage's ``db_sampler``: preprocess.py:147-182, DataBaseSamplerV2.sample_all,
det3d/core/sampler/sample_ops.py:101-253) runs before those transforms, as in the reference (fd_gt_sample.hip; the header has the
definition):

    db = GTDatabase.from_dbinfos(cfg.db_sampler["db_info_path"], root, class_names, 5, db_prep_steps=cfg.db_sampler["db_prep_steps"])
    sampler = GTSampler(db, cfg.db_sampler["sample_groups"], rate=cfg.db_sampler["rate"], sampler_type=cfg.sampler_type, seed=0)
    aug = GlobalAugment(cfg.train_preprocessor, seed=0, sampler=sampler)      # accepts db_sampler.enable = True

The host draws the database entries (GTSampler: one BatchSampler restatement per group pool); one launch per batch decides on the
device which of them collide with the sample's ground truth or with one another and appends the accepted entries' rows; one launch per
cloud pastes their points in front of the scene.  A cloud always grows by ``sampler.point_cap`` rows -- what is not an entry's point
is a sentinel row far outside every range, which the voxelisers drop -- so the host knows every size and nothing waits for the device.
GTSampler's docstring names the two intended differences from the reference.

The point-count filter (``min_points_in_gt``, preprocess.py:140-143) and the database itself rest on one primitive, "which points lie
inside which rotated 3-D boxes" (box_np_ops.points_in_rbbox / points_count_rbbox; fd_points_in_boxes.hip, the header has the arithmetic):

    aug = GlobalAugment(cfg.train_preprocessor, seed=0, point_filter=True)    # accepts min_points_in_gt > 0
    counts = points_count_rbbox(cloud, boxes)                                 # int32 [n_boxes], on the device
    rows, offsets = points_in_boxes(cloud, boxes)                             # each box's points, object-centred
    create_gt_database(samples, "gt_database", "dbinfos_train.pkl")           # the reference's files, from device tensors
    db = GTDatabase.from_samples(samples, class_names, device="cuda")         # or the database without the files

Everything is opt-in: with ``warp_bev=False`` / ``filter_gt=False`` / ``sampler=None`` / ``point_filter=False`` the launches are the
earlier ones.  In eval mode
``get_mask`` runs with identity parameters, under which the warp returns its input bit for bit, so that path needs no code.  Not
covered (NotImplementedError where a config asks for it): ``min_points_in_gt`` without ``point_filter=True``, ``npoints``, per-object
rotation noise of the sampler
(``global_random_rotation_range_per_object`` other than [0, 0]) and group sampling; not built: the registered ``Preprocess`` pipeline
stage, which stays a stub, its name-based class filtering (host-side data preparation), and the reference's global ``np.random``
stream (every object here draws from a Generator of its own).
"""
import collections
import threading

import numpy as np
import torch

from . import hip_ops

# struct fd_augment_record
RECORD_DTYPE = np.dtype([("flip_a", "<i4"), ("flip_b", "<i4"), ("c", "<f4"), ("s", "<f4"), ("rot", "<f4"), ("scale", "<f4"),
                         ("tx", "<f8"), ("ty", "<f8"), ("tz", "<f8")])
assert RECORD_DTYPE.itemsize == 8 * hip_ops.AUGMENT_RECORD_DOUBLES
# struct fd_augment_mask_record
MASK_RECORD_DTYPE = np.dtype([("flip_a", "<i4"), ("flip_b", "<i4"), ("m1", "<f8", (6,)), ("m2", "<f8", (6,))])
assert MASK_RECORD_DTYPE.itemsize == 8 * hip_ops.AUGMENT_MASK_RECORD_DOUBLES
PARAM_FIELDS = ("flip_a", "flip_b", "rot", "scale", "tx", "ty", "tz")  # the columns of draw()
BEV_SIZE = 180  # get_mask hard-codes a 180 x 180 map and the centre (90, 90)

_PERM_CACHE_SIZE = 16
_perm_cache = collections.OrderedDict()
_perm_lock = threading.Lock()


def reference_permutation(n):
    """int32 [n]: the order in which Preprocess's ``np.random.default_rng(0).shuffle(points)`` leaves the rows of an n-row cloud
    (shuffled[i] = points[perm[i]]): ``default_rng(0).permutation(n)``, which draws what ``shuffle`` draws.  Read-only and kept in an LRU
    cache keyed by n: one permutation of 300 000 rows costs about 8 ms of host time, a cache hit nothing."""
    n = int(n)
    if n < 0:
        raise ValueError("reference_permutation: n = %d" % n)
    with _perm_lock:
        p = _perm_cache.get(n)
        if p is not None:
            _perm_cache.move_to_end(n)
            return p
    p = np.random.default_rng(0).permutation(n).astype(np.int32)
    p.setflags(write=False)
    with _perm_lock:
        _perm_cache[n] = p
        while len(_perm_cache) > _PERM_CACHE_SIZE:
            _perm_cache.popitem(last=False)
    return p


def _get(cfg, key, default=None):
    v = cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)
    return default if v is None else v


class GlobalAugment(object):
    """The global flip / rotation / scaling / translation and the point shuffle of a ``train_preprocessor`` dict
    (``shuffle_points``, ``global_rot_noise``, ``global_scale_noise``, ``global_translate_std``, ``mode``, ``no_augmentation``).

    ``draw(B)`` draws B samples' parameters from the object's own ``numpy.random.Generator`` (``seed``) in the reference's order of
    draws -- the reference's global ``np.random`` stream is not reproduced; ``record(params)`` turns them into the kernels' records;
    ``aug(batch)`` returns an augmented copy of a device batch.  With ``no_augmentation=True`` or a mode other than "train" the
    transforms are the identity and only the shuffle remains.  ``min_points_in_gt > 0`` (unless ``point_filter=True``) and
    ``npoints > 0`` raise NotImplementedError, and so does an enabled ``db_sampler`` unless a ``sampler`` is given.  (The reference reads
    ``npoints`` and never uses it; it stays refused so that a config that sets it is noticed.)

    ``point_filter`` (False = as before): accepts ``min_points_in_gt > 0``, the reference's point-count filter (preprocess.py:140-143).
    As there, it is active (``min_points`` > 0) only in train mode without ``no_augmentation``; ``aug(batch)`` then applies
    ``filter_gt_by_min_points`` FIRST -- the counts come from the raw cloud and the raw timestep-0 boxes, the same mask goes to every
    timestep -- before sampling and before the transforms, so sampled entries are appended afterwards and are never filtered.  The
    static steps do the same while they load a batch.

    ``sampler`` (a GTSampler; None = no GT-database sampling, the launches of before): ``aug(batch)`` first samples -- the candidates
    are ``batch["gt_sample_candidates"]`` [B, K] if present, else a draw, and are kept in the returned batch -- so the accepted
    entries' rows join ``gt_boxes`` / ``gt_classes`` / ``gt_trajectory`` below the new ``gt_counts`` (the padded axis must have room
    for them: a row that does not fit is a rejected candidate and a bit of ``gt_sample_status``), then transforms the boxes with the
    new counts and builds every cloud as ``augment_points([sampled slots ; scene], perm(n + point_cap))``: each cloud grows by
    exactly ``sampler.point_cap`` rows, the accepted entries' points and sentinel rows (1e30, 1e30, 1e30, 0[, 0]) that every
    voxeliser drops as out of range.  ``gt_sample_status`` [B] (the hip_ops.GT_SAMPLE_* bits), ``gt_sample_accepted`` [B, K] and
    ``gt_sample_points`` [B] stay on the device.

    ``warp_bev`` (False = as before): the mask of a bev_map head is warped with the same parameters (the reference's ``get_mask``):
    ``mask_record(params)`` builds fd_augment_mask's records, ``aug(batch)`` also returns a warped copy of ``batch["bev_map"]`` when the
    batch has one, and the static steps draw for such a head and warp the batch's unwarped map themselves.  The map must be
    [B, C, 180, 180] (ValueError otherwise): the reference hard-codes that size and the centre (90, 90)."""

    def __init__(self, cfg, seed=None, warp_bev=False, sampler=None, point_filter=False):
        self.warp_bev = bool(warp_bev)
        self.point_filter = bool(point_filter)
        self.sampler = sampler
        db = _get(cfg, "db_sampler")
        if db is not None and _get(db, "enable", True):
            if sampler is None:
                raise NotImplementedError("GlobalAugment: an enabled db_sampler (GT-database sampling) needs sampler=GTSampler(...); "
                                          "without one, set db_sampler.enable = False")
            check_db_sampler_cfg(db)
        min_points = int(_get(cfg, "min_points_in_gt", -1))
        if min_points > 0 and not self.point_filter:
            raise NotImplementedError("GlobalAugment: min_points_in_gt > 0 (the point-count filter) needs point_filter=True")
        if _get(cfg, "npoints", -1) > 0:
            raise NotImplementedError("GlobalAugment: npoints > 0 (point sub-sampling) is not built")
        self.shuffle_points = bool(_get(cfg, "shuffle_points", False))
        self.mode = _get(cfg, "mode", "train")
        self.identity = bool(_get(cfg, "no_augmentation", False)) or self.mode != "train"
        rot = _get(cfg, "global_rot_noise", 0.0)
        rot = list(rot) if isinstance(rot, (list, tuple)) else [-rot, rot]  # prep.global_rotation
        scale = _get(cfg, "global_scale_noise", [1.0, 1.0])
        std = _get(cfg, "global_translate_std", 0)
        std = list(std) if isinstance(std, (list, tuple, np.ndarray)) else [std, std, std]  # prep.global_translate_
        if len(rot) != 2 or len(scale) != 2 or len(std) != 3:
            raise ValueError("GlobalAugment: global_rot_noise / global_scale_noise take two values, global_translate_std one or three")
        self.rot_noise, self.scale_noise, self.translate_std = [float(v) for v in rot], [float(v) for v in scale], [float(v) for v in std]
        self.sampling = sampler is not None and not self.identity  # (the reference samples inside its train / augmenting branch only)
        self.min_points = min_points if self.point_filter and min_points > 0 and not self.identity else 0  # 0: the filter is inactive
        self.rng = np.random.default_rng(seed)
        self._perm_dev = collections.OrderedDict()

    # -- parameters
    def draw(self, B):
        """float64 [B, 7]: flip_a, flip_b, rot, scale, tx, ty, tz per sample, drawn in the reference's order (two flips at probability
        0.5, the angle and the factor uniform in their ranges, three normals; z takes ``std[0]`` like x, the reference's quirk)."""
        out = np.zeros((int(B), len(PARAM_FIELDS)), np.float64)
        out[:, 3] = 1.0
        if self.identity:
            return out
        r, std = self.rng, self.translate_std
        for b in range(int(B)):
            out[b, 0] = float(r.random() < 0.5)
            out[b, 1] = float(r.random() < 0.5)
            out[b, 2] = r.uniform(self.rot_noise[0], self.rot_noise[1])
            out[b, 3] = r.uniform(self.scale_noise[0], self.scale_noise[1])
            if any(e != 0 for e in std):
                out[b, 4], out[b, 5], out[b, 6] = r.normal(0, std[0]), r.normal(0, std[1]), r.normal(0, std[0])
        return out

    @staticmethod
    def record(params, device=None):
        """The records of fd_augment_points / fd_augment_boxes for ``params`` [B, 7]: a numpy array [B] of RECORD_DTYPE (c and s are the
        float64 cosine and sine cast to fp32, as the reference builds its matrix), or with ``device`` its upload, float64 [B, 6]."""
        p = np.asarray(params, np.float64).reshape(-1, len(PARAM_FIELDS))
        if not np.all(np.isfinite(p)):
            raise ValueError("augmentation parameters must be finite")
        rec = np.zeros((p.shape[0],), RECORD_DTYPE)
        rec["flip_a"], rec["flip_b"] = p[:, 0] != 0, p[:, 1] != 0
        rec["c"], rec["s"] = np.cos(p[:, 2]).astype(np.float32), np.sin(p[:, 2]).astype(np.float32)
        rec["rot"], rec["scale"] = p[:, 2].astype(np.float32), p[:, 3].astype(np.float32)
        rec["tx"], rec["ty"], rec["tz"] = p[:, 4], p[:, 5], p[:, 6]
        if device is None:
            return rec
        return torch.from_numpy(rec.view(np.float64).reshape(-1, hip_ops.AUGMENT_RECORD_DOUBLES)).to(device)

    @staticmethod
    def mask_record(params, device=None):
        """The records of fd_augment_mask for ``params`` [B, 7]: a numpy array [B] of MASK_RECORD_DTYPE, or with ``device`` its upload,
        float64 [B, 13].  m1 / m2 are the inverses, taken the way cv2.warpAffine takes them, of get_mask's two float64 matrices:
        ``cv2.getRotationMatrix2D((90, 90), np.degrees(-rot), scale)`` and the translation by (float32(tx), float32(ty)) pixels (the
        reference uses the metres as pixels; tz is unused).  ValueError for parameters that are not finite or whose matrices would
        take a pixel of the 180 x 180 map out of the warp's fixed-point range (fd_augment_mask_check)."""
        p = np.asarray(params, np.float64).reshape(-1, len(PARAM_FIELDS))
        if not np.all(np.isfinite(p)):
            raise ValueError("augmentation parameters must be finite")
        rec = np.zeros((p.shape[0],), MASK_RECORD_DTYPE)
        rec["flip_a"], rec["flip_b"] = p[:, 0] != 0, p[:, 1] != 0
        c = float(BEV_SIZE // 2)
        for b in range(p.shape[0]):
            a = np.degrees(-p[b, 2]) * (np.pi / 180.0)  # getRotationMatrix2D: angle *= CV_PI / 180
            alpha, beta = np.cos(a) * p[b, 3], np.sin(a) * p[b, 3]
            rot = [alpha, beta, (1 - alpha) * c - beta * c, -beta, alpha, beta * c + (1 - alpha) * c]
            shift = [1.0, 0.0, float(np.float32(p[b, 4])), 0.0, 1.0, float(np.float32(p[b, 5]))]
            rec["m1"][b], rec["m2"][b] = _invert_affine(rot), _invert_affine(shift)
        try:
            hip_ops.augment_mask_check(rec, BEV_SIZE, BEV_SIZE)
        except hip_ops.FutureDetHipError as e:
            raise ValueError("GlobalAugment.mask_record: %s" % e)
        if device is None:
            return rec
        return torch.from_numpy(rec.view(np.float64).reshape(-1, hip_ops.AUGMENT_MASK_RECORD_DOUBLES)).to(device)

    def warp_map(self, bev, params):
        """a bev_map head's [B, C, 180, 180] fp32 device map warped with ``params`` [B, 7] (get_mask); a new tensor"""
        check_bev_size(bev)
        return hip_ops.augment_mask(bev, self.mask_record(params, device=bev.device))

    def permutation(self, n, device):
        """the shuffle of an n-row cloud as an int32 device tensor, or None when ``shuffle_points`` is off (a small LRU of uploads on top
        of reference_permutation's: a repeated row count costs neither host time nor a copy)"""
        if not self.shuffle_points:
            return None
        key = (int(n), str(device))
        p = self._perm_dev.get(key)
        if p is None:
            p = torch.from_numpy(reference_permutation(n).copy()).to(device, non_blocking=True)  # (the cached array is read-only)
            self._perm_dev[key] = p
            while len(self._perm_dev) > _PERM_CACHE_SIZE:
                self._perm_dev.popitem(last=False)
        else:
            self._perm_dev.move_to_end(key)
        return p

    # -- a batch
    def __call__(self, batch, params=None):
        """A new batch dict: ``clouds`` (list of device tensors [N_i, 4 | 5]) shuffled and transformed, ``gt_boxes`` [B, T, n, 12]
        transformed below ``gt_counts`` [B, T]; every other entry is passed through, and ``aug_params`` holds the parameters used
        (``params``, else batch["aug_params"], else a fresh draw).  With ``warp_bev`` a ``bev_map`` [B, C, 180, 180] entry is replaced by
        its warped copy."""
        if self.min_points > 0:  # on the raw cloud and the raw boxes, before everything else
            batch = filter_gt_by_min_points(batch, self.min_points)
        clouds, boxes = batch["clouds"], batch["gt_boxes"]
        if params is None:
            params = batch.get("aug_params")
        if params is None:
            params = self.draw(len(clouds))
        params = np.asarray(params, np.float64).reshape(-1, len(PARAM_FIELDS))
        if params.shape[0] != len(clouds) or boxes.shape[0] != len(clouds):
            raise ValueError("GlobalAugment: %d clouds, %d rows of parameters, gt_boxes %s" % (len(clouds), params.shape[0], tuple(boxes.shape)))
        recs = self.record(params, device=boxes.device)
        out = dict(batch)
        if not self.sampling:
            pasted = [None] * len(clouds)
            out["gt_boxes"] = hip_ops.augment_boxes(boxes, batch["gt_counts"], recs)
        else:  # sampling comes first: the transforms see the new rows and the new counts
            cand, accepted, plan = self._sample(batch, out)
            pasted = [(cand[b], accepted[b], plan[b]) for b in range(len(clouds))]
            hip_ops.augment_boxes(out["gt_boxes"], out["gt_counts"], recs, out=out["gt_boxes"])
        out["clouds"] = [self._cloud(c, recs[b], pasted[b]) for b, c in enumerate(clouds)]
        out["aug_params"] = params
        if self.warp_bev and batch.get("bev_map") is not None:
            out["bev_map"] = self.warp_map(batch["bev_map"], params)
        return out


    def _sample(self, batch, out):
        """GT-database sampling into ``out``: the new ground truth, the candidates and the kernel's reports; returns the per-sample
        views (cand, accepted, plan) the clouds are pasted from"""
        s = self.sampler
        boxes = batch["gt_boxes"]
        dev = boxes.device
        cand = batch.get("gt_sample_candidates")
        if cand is None:
            cand = s.draw(boxes.shape[0])
        cand = np.ascontiguousarray(cand, np.int32)
        if cand.shape != (boxes.shape[0], s.K):
            raise ValueError("gt_sample_candidates %s: expected [%d, %d]" % (cand.shape, boxes.shape[0], s.K))
        cand_dev = torch.from_numpy(cand).to(dev)
        traj = batch.get("gt_trajectory")
        # on clones: the rows at or past the new counts stay what the batch holds there
        res = hip_ops.gt_sample_select(boxes.clone(), batch["gt_counts"].clone(), batch["gt_classes"].clone(), s.database, cand_dev, s.records,
                                       s.rate, s.point_cap, trajectory=traj.clone() if traj is not None else None, out="inplace")
        out["gt_boxes"], out["gt_counts"], out["gt_classes"] = res["boxes"], res["counts"], res["classes"]
        if traj is not None:
            out["gt_trajectory"] = res["trajectory"]
        out["gt_sample_candidates"], out["gt_sample_status"] = cand, res["status"]
        out["gt_sample_accepted"], out["gt_sample_points"] = res["accepted"], res["n_points"]
        return cand_dev, res["accepted"], res["plan"]

    def _cloud(self, c, rec, pasted):
        """one cloud: [the sampled slots ; the scene], shuffled and transformed"""
        if pasted is None:
            return hip_ops.augment_points(c, rec, torch.empty_like(c), perm=self.permutation(c.shape[0], c.device))
        cand, accepted, plan = pasted
        cap, n = self.sampler.point_cap, int(c.shape[0])
        stage = torch.empty((cap + n, c.shape[1]), dtype=torch.float32, device=c.device)
        hip_ops.gt_sample_points(self.sampler.database, cand, accepted, plan, stage, cap)
        stage[cap:].copy_(c)
        return hip_ops.augment_points(stage, rec, torch.empty_like(stage), perm=self.permutation(cap + n, c.device))


# ------------------------------------------------------------------------------------------------------------------ GT-database sampling
_TRAJECTORY = ("static", "linear", "nonlinear")  # the ids targets.py uses


def check_db_sampler_cfg(db_cfg):
    """NotImplementedError for what a ``db_sampler`` dict can ask for that is not built: per-object rotation noise (a non-empty
    ``global_random_rotation_range_per_object`` whose ends differ by >= 1e-3: noise_per_object_v3_ / rot_transform) and group sampling
    (a group dict with more than one class)."""
    rot = _get(db_cfg, "global_random_rotation_range_per_object")
    if rot is not None:
        rot = list(rot) if isinstance(rot, (list, tuple, np.ndarray)) else [-rot, rot]
        if len(rot) > 0 and (len(rot) != 2 or abs(float(rot[0]) - float(rot[1])) >= 1e-3):
            raise NotImplementedError("db_sampler: global_random_rotation_range_per_object = %r (per-object rotation noise, "
                                      "noise_per_object_v3_ and rot_transform) is not built; every shipped config has [0, 0]" % (rot,))
    for g in _get(db_cfg, "sample_groups", []) or []:
        if len(g) > 1:
            raise NotImplementedError("db_sampler: group sampling (a sample group with more than one class, %r) is not built" % (dict(g),))


class GTDatabase(object):
    """The ground-truth database on the device, as fd_gt_sample_select / fd_gt_sample_points read it: ``boxes`` [M, Tdb, 12] fp32 (an
    entry's box at every timestep it has, zeros behind them), ``steps`` [M] int32 (>= 1), ``classes`` [M] int32 (1-based ids over
    ``class_names``), ``trajectory`` [M] int32 (0 static, 1 linear, 2 nonlinear: targets.py's ids), ``offsets`` [M + 1] int64 and
    ``points`` [P, ndim] fp32 (object-centred, entry e owns the rows offsets[e]..offsets[e + 1]).  ``host`` keeps numpy copies of the
    small arrays for the sampler."""

    def __init__(self, boxes, steps, classes, trajectory, points, offsets, device, class_names=None):
        boxes = np.ascontiguousarray(boxes, np.float32)
        points = np.ascontiguousarray(points, np.float32)
        steps, classes, trajectory = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (steps, classes, trajectory))
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        M = boxes.shape[0]
        if boxes.ndim != 3 or boxes.shape[2] != 12 or M < 1 or boxes.shape[1] < 1:
            raise ValueError("GTDatabase: boxes must be [M, Tdb, 12] with M, Tdb >= 1, got %s" % (boxes.shape,))
        if points.ndim != 2 or points.shape[1] not in (4, 5):
            raise ValueError("GTDatabase: points must be [P, 4] or [P, 5], got %s" % (points.shape,))
        if len(steps) != M or len(classes) != M or len(trajectory) != M or len(offsets) != M + 1:
            raise ValueError("GTDatabase: steps, classes and trajectory take %d values, offsets %d" % (M, M + 1))
        if steps.min() < 1 or steps.max() > boxes.shape[1]:
            raise ValueError("GTDatabase: steps must lie in [1, Tdb = %d]" % boxes.shape[1])
        if offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] != points.shape[0]:
            raise ValueError("GTDatabase: offsets must rise from 0 to the %d rows of points" % points.shape[0])
        self.class_names = list(class_names) if class_names is not None else None
        self.host = dict(steps=steps, classes=classes, trajectory=trajectory, offsets=offsets, rows=np.diff(offsets))
        self.device = torch.device(device)
        self.boxes, self.points = torch.from_numpy(boxes).to(self.device), torch.from_numpy(points).to(self.device)
        self.steps, self.classes, self.trajectory = (torch.from_numpy(v).to(self.device) for v in (steps, classes, trajectory))
        self.offsets = torch.from_numpy(offsets).to(self.device)

    def __len__(self):
        return int(self.boxes.shape[0])

    @classmethod
    def from_arrays(cls, boxes, steps, classes, trajectory, points, offsets, device, class_names=None):
        return cls(boxes, steps, classes, trajectory, points, offsets, device, class_names=class_names)

    @classmethod
    def from_dbinfos(cls, db_infos, root, class_names, num_point_features, db_prep_steps=(), device="cuda"):
        """From the reference's database: ``db_infos`` (the dict create_gt_database.py pickles, class name -> list of entries, or the
        path of that pickle) and the ``.bin`` files its ``path`` entries name below ``root``.  ``db_prep_steps`` as in a config:
        ``filter_by_min_num_points`` (per class, on ``num_points_in_gt``) and ``filter_by_difficulty``, the latter evaluated as the
        reference evaluates it -- ``info["difficulty"] not in removed`` with the list-valued difficulty the database writer stores, so
        the shipped ``[-1]`` removes nothing.  Names and trajectory strings (those of timestep 0) become targets.py's ids; classes
        outside ``class_names`` are left out.  Entries keep the order of the pickle, class after class."""
        import os
        import pickle

        if isinstance(db_infos, (str, bytes, os.PathLike)):
            with open(db_infos, "rb") as f:
                db_infos = pickle.load(f)
        infos = {k: list(v) for k, v in db_infos.items()}
        for step in db_prep_steps or ():
            if "filter_by_difficulty" in step:
                removed = step["filter_by_difficulty"]
                infos = {k: [i for i in v if i["difficulty"] not in removed] for k, v in infos.items()}
            elif "filter_by_min_num_points" in step:
                for name, min_num in dict(step["filter_by_min_num_points"]).items():
                    if name in infos and min_num > 0:
                        infos[name] = [i for i in infos[name] if i["num_points_in_gt"] >= min_num]
            else:
                raise ValueError("unknown database prep type: %r" % (step,))
        class_names = list(class_names)
        first = lambda v: v if isinstance(v, str) else v[0]
        rows, steps, classes, traj, points = [], [], [], [], []
        for name, entries in infos.items():
            if name not in class_names:
                continue
            for info in entries:
                b = np.asarray(info["box3d_lidar"], np.float32).reshape(-1, 12)
                tr = first(info["trajectory"])
                if tr not in _TRAJECTORY:
                    raise KeyError("%s_%s" % (tr, name))
                p = np.fromfile(os.path.join(str(root), info["path"]), dtype=np.float32).reshape(-1, int(num_point_features))
                rows.append(b), steps.append(len(b)), classes.append(class_names.index(first(info["name"])) + 1)
                traj.append(_TRAJECTORY.index(tr)), points.append(p)
        if not rows:
            raise ValueError("GTDatabase.from_dbinfos: no entry of the classes %r is left" % (class_names,))
        boxes = np.zeros((len(rows), max(steps), 12), np.float32)
        for e, b in enumerate(rows):
            boxes[e, :len(b)] = b
        offsets = np.concatenate([[0], np.cumsum([len(p) for p in points])])
        return cls(boxes, steps, classes, traj, np.concatenate(points), offsets, device, class_names=class_names)


    @classmethod
    def from_samples(cls, samples, class_names, device="cuda", num_point_features=None):
        """The database of ``samples`` without the files: what ``from_dbinfos`` returns for what ``create_gt_database`` writes (all
        classes of ``class_names``, no prep steps).  One sample is a dict: ``points`` [n, 4 | 5] fp32 (a device tensor or an array),
        ``boxes`` [T, N, 12], ``names`` (N strings) and ``trajectory`` (N of "static" / "linear" / "nonlinear").  Entries are ordered
        class after class in the order the classes first appear, as the pickle's dict is."""
        by_name, class_names = {}, list(class_names)
        for pts, boxes, names, traj, _ in _database_entries(samples, device, None, num_point_features):
            for i, p in pts.items():
                if traj[i] not in _TRAJECTORY:
                    raise KeyError("%s_%s" % (traj[i], names[i]))
                by_name.setdefault(names[i], []).append((boxes[:, i], class_names.index(names[i]) + 1 if names[i] in class_names else 0,
                                                         _TRAJECTORY.index(traj[i]), p))
        entries = [e for name, lst in by_name.items() if name in class_names for e in lst]
        if not entries:
            raise ValueError("GTDatabase.from_samples: no entry of the classes %r" % (class_names,))
        T = max(len(e[0]) for e in entries)
        boxes = np.zeros((len(entries), T, 12), np.float32)
        for k, e in enumerate(entries):
            boxes[k, :len(e[0])] = e[0]
        offsets = np.concatenate([[0], np.cumsum([len(e[3]) for e in entries])])
        return cls(boxes, [len(e[0]) for e in entries], [e[1] for e in entries], [e[2] for e in entries], np.concatenate([e[3] for e in entries]),
                   offsets, device, class_names=class_names)


def _database_entries(samples, device, used_classes, num_point_features):
    """per sample with objects: (points {object i: fp32 rows, object-centred}, boxes [T, N, 12], names, trajectory, image_idx) -- one
    points_in_boxes per sample on the device, its rows read back once"""
    for index, s in enumerate(samples):
        boxes = np.ascontiguousarray(s["boxes"].cpu().numpy() if isinstance(s["boxes"], torch.Tensor) else s["boxes"], np.float32)
        if boxes.ndim != 3 or boxes.shape[2] != 12:
            raise ValueError("a sample's boxes must be [T, N, 12], got %s" % (boxes.shape,))
        names, traj = [str(v) for v in s["names"]], [str(v) for v in s["trajectory"]]
        if len(names) != boxes.shape[1] or len(traj) != boxes.shape[1]:
            raise ValueError("a sample with %d boxes has %d names and %d trajectory types" % (boxes.shape[1], len(names), len(traj)))
        if boxes.shape[1] == 0:  # (the reference skips a sample without objects)
            continue
        pts = s["points"]
        pts = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts, np.float32))
        pts = pts.to(device=device, dtype=torch.float32).contiguous()
        ncols = None if num_point_features is None else min(int(num_point_features), int(pts.shape[1]))  # (points[:, :point_features])
        rows, offsets = points_in_boxes(pts, torch.from_numpy(boxes[0].copy()).to(pts.device), ncols=ncols)
        rows, offsets = rows.cpu().numpy(), offsets.cpu().numpy()
        keep = {i: rows[offsets[i]:offsets[i + 1]] for i in range(boxes.shape[1]) if used_classes is None or names[i] in used_classes}
        yield keep, boxes, names, traj, s.get("image_idx", index)


def create_gt_database(samples, db_path, dbinfo_path, used_classes=None, num_point_features=5, relative_path=True, device="cuda"):
    """The reference's ground-truth database (det3d/datasets/utils/create_gt_database.py:109-176) from ``samples`` (GTDatabase.from_samples
    names their entries; ``image_idx`` defaults to the sample's position; dataset iteration and sweep loading stay the caller's): per
    object of a used class the file ``<db_path>/<name>/<image_idx>_<name>_<i>.bin`` -- the first ``num_point_features`` columns of the
    cloud's points inside the object's timestep-0 box, minus the box centre, fp32 -- and in the pickle ``dbinfo_path`` a dict class name
    -> entries with ``name`` and ``trajectory`` (one per timestep), ``path`` (relative to db_path's parent, or absolute with
    ``relative_path=False``), ``image_idx``, ``gt_idx``, ``box3d_lidar`` (the rows of every timestep), ``num_points_in_gt``,
    ``difficulty`` (zeros) and ``group_id`` (a running number).  Samples without objects are skipped.  Returns the dict.
    ``GTDatabase.from_dbinfos(dbinfo_path, <db_path's parent>, ...)`` reads it back."""
    import os
    import pickle

    db_path = str(db_path)
    os.makedirs(db_path, exist_ok=True)
    stem = os.path.splitext(os.path.basename(os.path.normpath(db_path)))[0]  # (Path.stem, as the reference builds the relative path)
    infos, group = {}, 0
    for pts, boxes, names, traj, image_idx in _database_entries(samples, device, used_classes, num_point_features):
        T = boxes.shape[0]
        for i, p in pts.items():
            filename = "%s_%s_%d.bin" % (image_idx, names[i], i)
            os.makedirs(os.path.join(db_path, names[i]), exist_ok=True)
            filepath = os.path.join(db_path, names[i], filename)
            np.ascontiguousarray(p, np.float32).tofile(filepath)
            infos.setdefault(names[i], []).append({
                "name": [names[i]] * T, "trajectory": [traj[i]] * T, "path": os.path.join(stem, names[i], filename) if relative_path else filepath,
                "image_idx": image_idx, "gt_idx": i, "box3d_lidar": [boxes[t, i].copy() for t in range(T)], "num_points_in_gt": int(p.shape[0]),
                "difficulty": [np.int32(0)] * T, "group_id": group})
            group += 1
    with open(str(dbinfo_path), "wb") as f:
        pickle.dump(infos, f)
    return infos


class _BatchSampler(object):
    """The reference's BatchSampler (det3d/core/sampler/preprocess.py:19-54) over n indices: a shuffled list read in slices; a draw
    that would reach the end (``idx + num >= n``) returns what is left -- possibly fewer than asked for -- and reshuffles."""

    def __init__(self, n, rng):
        self._indices, self._rng, self._idx, self._n = np.arange(int(n)), rng, 0, int(n)
        rng.shuffle(self._indices)

    def sample(self, num):
        if self._idx + num >= self._n:
            ret = self._indices[self._idx:].copy()
            self._rng.shuffle(self._indices)
            self._idx = 0
        else:
            ret = self._indices[self._idx:self._idx + num].copy()  # (the reference reads its view at once)
            self._idx += num
        return ret


class GTSampler(object):
    """The host half of GT-database sampling: draws, per sample and group, the database entries fd_gt_sample_select chooses from.

    ``sample_groups``: a config's list of one-entry dicts, ``{"car": 2}`` for the standard sampler or ``{"static_car": 2}`` (trajectory
    type + class) for any other ``sampler_type``; ``rate`` as in the config.  Group g owns ``K_g = max(0, round(rate * max_g))`` slots of
    the ``K = sum K_g`` (<= 64) columns of ``draw(B)``; ``records`` are the kernel's group records.  Every group pool (the entries of
    the class, for a typed group those of its trajectory type) has a BatchSampler restatement driven by the object's own
    ``numpy.random.Generator`` (``seed``); the reference's global ``np.random`` stream is not reproduced.

    Two intended differences from the reference.  (1) The host cannot see the per-class ground-truth counts of a batch that lives on
    the device, so it always draws K_g entries and the kernel uses the first ``round(rate * (max_g - count_g))`` of them: the pools
    are consumed faster.  (A typed group also draws from a pool of its own type instead of skipping through the class's pool.)
    (2) The reference mutates a database entry on its first use (``sample["box3d_lidar"] = sample["box3d_lidar"][0]``), so a second
    draw of the same entry has lost its forecasts; here every draw sees all timesteps.

    ``point_cap`` (None: the bound that can never overflow, the sum over groups of K_g x the largest entry of the pool): the rows every
    cloud grows by -- the accepted entries' points and sentinel rows behind them."""

    def __init__(self, database, sample_groups, rate=1.0, sampler_type="standard", seed=None, point_cap=None):
        if database.class_names is None:
            raise ValueError("GTSampler: the database needs class_names to resolve the groups")
        self.database, self.rate, self.sampler_type = database, float(rate), sampler_type
        self.rng = np.random.default_rng(seed)
        host = database.host
        self.records, self._pools, self._entries = [], [], []
        pools, first, bound = {}, 0, 0
        for g in sample_groups:
            if len(g) != 1:
                raise NotImplementedError("GTSampler: group sampling (a sample group with more than one class, %r) is not built" % (dict(g),))
            (key, max_num), = dict(g).items()
            tr = -1
            name = key
            if sampler_type != "standard":
                trs, name = key.split("_")
                if trs not in _TRAJECTORY:
                    raise KeyError(key)
                tr = _TRAJECTORY.index(trs)
            if name not in database.class_names:
                raise ValueError("GTSampler: group %r names a class outside class_names %r" % (key, database.class_names))
            cid = database.class_names.index(name) + 1
            k = max(0, int(np.round(self.rate * max_num)))
            if (cid, tr) not in pools:
                entries = np.nonzero((host["classes"] == cid) & ((host["trajectory"] == tr) | (tr < 0)))[0].astype(np.int32)
                pools[(cid, tr)] = (entries, _BatchSampler(len(entries), self.rng) if len(entries) else None)
            entries, pool = pools[(cid, tr)]
            self._entries.append(entries), self._pools.append(pool)
            self.records.append((cid, tr, int(max_num), first, k))
            first += k
            bound += k * (int(host["rows"][entries].max()) if len(entries) else 0)
        self.K = first
        if not 1 <= self.K <= hip_ops.GT_SAMPLE_MAX_K or len(self.records) > hip_ops.GT_SAMPLE_MAX_GROUPS:
            raise ValueError("GTSampler: %d slots in %d groups; the kernel takes 1..%d slots in at most %d groups"
                             % (self.K, len(self.records), hip_ops.GT_SAMPLE_MAX_K, hip_ops.GT_SAMPLE_MAX_GROUPS))
        self.point_cap = int(bound if point_cap is None else point_cap)
        if self.point_cap < 0:
            raise ValueError("GTSampler: point_cap = %d" % self.point_cap)

    def draw(self, B):
        """int32 [B, K]: per sample, group after group, the drawn entries; -1 where a pool is empty or its draw came up short"""
        cand = np.full((int(B), self.K), -1, np.int32)
        for b in range(int(B)):
            for (_, _, _, first, k), entries, pool in zip(self.records, self._entries, self._pools):
                if pool is None or k == 0:
                    continue
                idx = pool.sample(k)
                cand[b, first:first + len(idx)] = entries[idx]
        return cand


def _invert_affine(m):
    """cv2.warpAffine's inversion of a 2 x 3 float64 matrix, operation by operation (imgwarp.cpp, without WARP_INVERSE_MAP)"""
    m = [float(v) for v in m]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = A11, m[1] * -D, m[3] * -D, A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def check_bev_size(bev):
    """get_mask knows one map size: ValueError for a map that is not [B, C, 180, 180]"""
    if bev.dim() != 4 or tuple(bev.shape[2:]) != (BEV_SIZE, BEV_SIZE):
        raise ValueError("the bev_map warp (get_mask) is defined for %d x %d maps and the centre (%d, %d) only, got %s"
                         % (BEV_SIZE, BEV_SIZE, BEV_SIZE // 2, BEV_SIZE // 2, tuple(bev.shape)))


def filter_gt_outside_range(batch, pc_range):
    """The train-mode ground-truth filter of the reference's Voxelization stage (prep.filter_gt_box_outside_range) for a device batch: a
    new batch dict whose ``gt_boxes`` / ``gt_classes`` / ``gt_trajectory`` keep, at every timestep, the objects whose timestep-0 box has
    a BEV corner strictly inside ``pc_range`` -- (xmin, ymin, xmax, ymax), or a six-value voxel range, whose x and y bounds are taken --
    moved to the front (zeros behind them), with ``gt_counts`` the new counts, still on the device.  ``gt_filter_status`` [B] int32
    counts the timesteps of a sample whose count differed from timestep 0's.  One launch, no synchronisation."""
    rng = bev_range(pc_range)
    out = dict(batch)
    boxes = batch["gt_boxes"]
    if boxes.shape[2] == 0:
        return out
    traj = batch.get("gt_trajectory")
    b, n, c, t, status = hip_ops.gt_range_filter(boxes.contiguous(), batch["gt_counts"].contiguous(), batch["gt_classes"].contiguous(), rng,
                                                 trajectory=traj.contiguous() if traj is not None else None)
    out["gt_boxes"], out["gt_counts"], out["gt_classes"], out["gt_filter_status"] = b, n, c, status
    if traj is not None:
        out["gt_trajectory"] = t
    return out


def points_count_rbbox(points, boxes, n_boxes=None):
    """box_np_ops.points_count_rbbox on device tensors: int32 [n_boxes] = the points of ``points`` [n, 4 | 5] inside each row of ``boxes``
    [n_boxes, >= 7] (the angle is the LAST column).  ``n_boxes``: one int32 on the device, rows at or past it count 0.  Two launches,
    no synchronisation."""
    return hip_ops.points_in_boxes_count(points.contiguous(), boxes.contiguous(), n_boxes=n_boxes)[0]


def points_in_boxes(points, boxes, ncols=None):
    """box_np_ops.points_in_rbbox as rows: (rows [total, ncols] fp32, offsets int64 [n_boxes + 1]) -- box j owns the rows
    offsets[j]..offsets[j + 1], its points in cloud order, columns 0..2 minus the box centre; ``ncols`` (None: all) leading columns.  A
    point inside two boxes appears under both.  The offline path: the totals are read back once to size ``rows`` exactly."""
    points, boxes = points.contiguous(), boxes.contiguous()
    ncols = int(points.shape[1] if ncols is None else ncols)
    counts, ws = hip_ops.points_in_boxes_count(points, boxes)
    total = int(counts.sum().item())
    rows = torch.empty((total, ncols), dtype=torch.float32, device=points.device)
    rows, offsets, _ = hip_ops.points_in_boxes_extract(points, boxes, ws, rows)
    return rows, offsets


def filter_gt_by_min_points(batch, min_points):
    """The reference's ``min_points_in_gt`` filter (preprocess.py:140-143) for a device batch: a new batch dict whose ``gt_boxes`` /
    ``gt_classes`` / ``gt_trajectory`` keep, at every timestep, the objects whose timestep-0 box holds at least ``min_points`` points of
    the sample's cloud, moved to the front (zeros behind them), with ``gt_counts`` the new counts.  ``gt_point_counts`` [B, n] int32 are
    the counts, ``gt_min_points_status`` [B] the timesteps of a sample whose count differed from timestep 0's.  Two launches per cloud
    and one for the batch, no synchronisation."""
    out = dict(batch)
    boxes, counts = batch["gt_boxes"].contiguous(), batch["gt_counts"].contiguous()
    if boxes.shape[2] == 0:
        return out
    pc = torch.empty((boxes.shape[0], boxes.shape[2]), dtype=torch.int32, device=boxes.device)
    for b, c in enumerate(batch["clouds"]):
        hip_ops.points_in_boxes_count(c.contiguous(), boxes[b, 0], n_boxes=counts[b, 0:1], out=pc[b])
    traj = batch.get("gt_trajectory")
    nb, n, c, t, status = hip_ops.gt_min_points_filter(boxes, counts, batch["gt_classes"].contiguous(), pc, int(min_points),
                                                       trajectory=traj.contiguous() if traj is not None else None)
    out["gt_boxes"], out["gt_counts"], out["gt_classes"], out["gt_point_counts"], out["gt_min_points_status"] = nb, n, c, pc, status
    if traj is not None:
        out["gt_trajectory"] = t
    return out


def bev_range(pc_range):
    """(xmin, ymin, xmax, ymax) of a four- or six-value range (``pc_range[[0, 1, 3, 4]]`` of a voxel range), as fp32 values"""
    r = [float(np.float32(v)) for v in pc_range]
    if len(r) == 6:
        r = [r[0], r[1], r[3], r[4]]
    if len(r) != 4:
        raise ValueError("a range takes 4 (xmin, ymin, xmax, ymax) or 6 values, got %d" % len(r))
    return r


def identity_params(B):
    """[B, 7] parameters under which the transforms change nothing (but the sign of a zero)"""
    out = np.zeros((int(B), len(PARAM_FIELDS)), np.float64)
    out[:, 3] = 1.0
    return out


__all__ = ["GlobalAugment", "GTDatabase", "GTSampler", "check_db_sampler_cfg", "reference_permutation", "identity_params", "filter_gt_outside_range", "filter_gt_by_min_points", "points_count_rbbox", "points_in_boxes", "create_gt_database", "bev_range", "check_bev_size",
           "RECORD_DTYPE", "MASK_RECORD_DTYPE", "PARAM_FIELDS", "BEV_SIZE"]
