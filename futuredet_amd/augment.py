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

Everything is opt-in: with ``warp_bev=False`` / ``filter_gt=False`` the launches are the earlier ones.  In eval mode ``get_mask`` runs
with identity parameters, under which the warp returns its input bit for bit, so that path needs no code.  Not covered
(NotImplementedError where a config asks for it): GT-database sampling, ``min_points_in_gt``, ``npoints``; not built: the registered
``Preprocess`` pipeline stage, which stays a stub, and its name-based class filtering (host-side data preparation).
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
    transforms are the identity and only the shuffle remains.  An enabled ``db_sampler``, ``min_points_in_gt > 0`` and ``npoints > 0``
    raise NotImplementedError.

    ``warp_bev`` (False = as before): the mask of a bev_map head is warped with the same parameters (the reference's ``get_mask``):
    ``mask_record(params)`` builds fd_augment_mask's records, ``aug(batch)`` also returns a warped copy of ``batch["bev_map"]`` when the
    batch has one, and the static steps draw for such a head and warp the batch's unwarped map themselves.  The map must be
    [B, C, 180, 180] (ValueError otherwise): the reference hard-codes that size and the centre (90, 90)."""

    def __init__(self, cfg, seed=None, warp_bev=False):
        self.warp_bev = bool(warp_bev)
        db = _get(cfg, "db_sampler")
        if db is not None and _get(db, "enable", True):
            raise NotImplementedError("GlobalAugment: db_sampler (GT-database sampling) is not built; set db_sampler.enable = False")
        if _get(cfg, "min_points_in_gt", -1) > 0:
            raise NotImplementedError("GlobalAugment: min_points_in_gt > 0 (the point-count filter) is not built")
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
        out["clouds"] = [hip_ops.augment_points(c, recs[b], torch.empty_like(c), perm=self.permutation(c.shape[0], c.device))
                         for b, c in enumerate(clouds)]
        out["gt_boxes"] = hip_ops.augment_boxes(boxes, batch["gt_counts"], recs)
        out["aug_params"] = params
        if self.warp_bev and batch.get("bev_map") is not None:
            out["bev_map"] = self.warp_map(batch["bev_map"], params)
        return out


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


__all__ = ["GlobalAugment", "reference_permutation", "identity_params", "filter_gt_outside_range", "bev_range", "check_bev_size",
           "RECORD_DTYPE", "MASK_RECORD_DTYPE", "PARAM_FIELDS", "BEV_SIZE"]
