"""Global training augmentation on the device: the live train-mode path of the reference's ``Preprocess`` stage
(det3d/datasets/pipelines/preprocess.py:189-192, 201-203) for the shipped configs -- the fixed-seed point shuffle, then
``prep.random_flip_both``, ``prep.global_rotation``, ``prep.global_scaling_v2`` and ``prep.global_translate_`` on the cloud and on every
timestep's [N, 12] box rows (fd_augment.hip; include/futuredet_hip.h has the arithmetic).

    aug = GlobalAugment(cfg.train_preprocessor, seed=0)
    step = StaticTrainStep(..., augment=aug)        # the step draws, uploads one record and transforms while it loads the batch
    batch = aug(batch)                              # or: a new batch dict for train_steps

Not covered (NotImplementedError where a config asks for it): GT-database sampling, ``min_points_in_gt``, ``npoints``; not built: the
warp of a bev_map head's mask (``get_mask``), the eval-mode path, and the registered ``Preprocess`` pipeline stage, which stays a stub.
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
PARAM_FIELDS = ("flip_a", "flip_b", "rot", "scale", "tx", "ty", "tz")  # the columns of draw()

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
    raise NotImplementedError."""

    def __init__(self, cfg, seed=None):
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
        (``params``, else batch["aug_params"], else a fresh draw)."""
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
        return out


def identity_params(B):
    """[B, 7] parameters under which the transforms change nothing (but the sign of a zero)"""
    out = np.zeros((int(B), len(PARAM_FIELDS)), np.float64)
    out[:, 3] = 1.0
    return out


__all__ = ["GlobalAugment", "reference_permutation", "identity_params", "RECORD_DTYPE", "PARAM_FIELDS"]
