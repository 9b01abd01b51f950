"""Generates tests/golden/loss.npz: the reference's CenterHead.loss (det3d/models/bbox_heads/center_head.py:396-539 with
FastFocalLoss / RegLoss of det3d/models/losses/centernet_loss.py) on seeded head maps and targets, by IMPORTING the reference
with the import shims of make_golden.py.  Run:  python tests/golden/make_golden_loss.py

The fixture holds inputs (maps, targets) and the reference's outputs (loss terms, gradient of the summed loss w.r.t. each map)
only.  Cases: n0 (standard, T = 1), n3 (standard, T = 7) and n3dtf (dense, 7 tasks), with the shipped configs' code weights.
"""
import logging
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

CASES = (("n0", 1, False), ("n3", 7, False), ("n3dtf", 7, True))
B, H, W, M = 2, 16, 16, 12
MAPS = (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2))


def head_kwargs(T, dense):
    return dict(in_channels=64, tasks=[dict(num_class=1, class_names=["car"])], dataset="nuscenes", weight=0.25,
                code_weights=[1.0] * 10 if dense else [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0],
                common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
                share_conv_channel=64, dcn_head=False, timesteps=T, two_stage=False, reverse=False, sparse=False, dense=dense,
                bev_map=False, forecast_feature=dense, classify=False, wide_head=False)


def inputs(name, T, dense, seed):
    """Seeded maps (per task) and targets (per timestep, one task each) as numpy arrays keyed for the fixture."""
    rng = np.random.default_rng(seed)
    n_tasks = T if dense else 1
    out = {}
    for t in range(n_tasks):
        out["%s_t%d_hm" % (name, t)] = rng.normal(-1.0, 1.5, (B, 1, H, W)).astype(np.float32)
        for m, c in MAPS + (("vel", 2 if dense else 2 * T),):
            out["%s_t%d_%s" % (name, t, m)] = rng.normal(0.0, 1.0, (B, c, H, W)).astype(np.float32)
    for s in range(T):
        hm = rng.uniform(0.0, 0.9, (B, 1, H, W)).astype(np.float32) ** 3
        ind = np.stack([rng.choice(H * W, M, replace=False) for _ in range(B)]).astype(np.int64)
        n_obj = [M - 3, 0] if s == 1 else [M - 3, M - 5]  # a sample without objects in one step
        mask = np.zeros((B, M), np.uint8)
        for b in range(B):
            mask[b, : n_obj[b]] = 1
            hm[b, 0].reshape(-1)[ind[b, : n_obj[b]]] = 1.0
        out["%s_s%d_hm_target" % (name, s)] = hm
        out["%s_s%d_ind" % (name, s)] = ind
        out["%s_s%d_mask" % (name, s)] = mask
        out["%s_s%d_cat" % (name, s)] = np.zeros((B, M), np.int64)
        out["%s_s%d_anno_box" % (name, s)] = rng.normal(0.0, 1.0, (B, M, 10)).astype(np.float32)
    return out


def example_of(d, name, T):
    ex = {"hm": [], "ind": [], "mask": [], "cat": [], "anno_box": []}
    for s in range(T):
        ex["hm"].append([torch.from_numpy(d["%s_s%d_hm_target" % (name, s)])])
        ex["ind"].append([torch.from_numpy(d["%s_s%d_ind" % (name, s)])])
        ex["mask"].append([torch.from_numpy(d["%s_s%d_mask" % (name, s)])])
        ex["cat"].append([torch.from_numpy(d["%s_s%d_cat" % (name, s)])])
        ex["anno_box"].append([torch.from_numpy(d["%s_s%d_anno_box" % (name, s)])])
    return ex


def map_keys(d, name):
    return sorted(k for k in d if k.startswith(name + "_t"))


def run_loss(head, d, name, T, dense):
    """loss(example, preds) on leaf maps; returns (ret, {map key: grad of the summed per-task losses})."""
    leaves = {k: torch.from_numpy(d[k]).double().requires_grad_(True) for k in map_keys(d, name)}
    n_tasks = T if dense else 1
    preds = []
    for t in range(n_tasks):
        pfx = "%s_t%d_" % (name, t)
        # the reference sigmoids hm in place: hand it a non-leaf
        preds.append({k[len(pfx):]: v * 1.0 for k, v in leaves.items() if k.startswith(pfx)})
    ex = example_of(d, name, T)
    ex = {k: [[x.double() if x.dtype == torch.float32 else x for x in row] for row in v] for k, v in ex.items()}
    ret = head.loss(ex, preds)
    sum(ret["loss"]).backward()
    return ret, {k: v.grad.numpy() for k, v in leaves.items()}


def flatten(ret, name, T, dense):
    out = {}
    for t, loss in enumerate(ret["loss"]):
        out["%s_out_t%d_loss" % (name, t)] = np.float64(loss.detach().item())
        out["%s_out_t%d_hm_loss" % (name, t)] = np.float64(ret["hm_loss"][t].item())
        out["%s_out_t%d_loc_loss" % (name, t)] = np.array([x.detach().item() for x in ret["loc_loss"][t]])
        elem = ret["loc_loss_elem"][t]
        out["%s_out_t%d_loc_loss_elem" % (name, t)] = elem.numpy() if dense else np.stack([e.numpy() for e in elem])
        out["%s_out_t%d_num_positive" % (name, t)] = np.float64(ret["num_positive"][t].item())
    return out


def main():
    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    from det3d.models import build_head

    arrays = {}
    for seed, (name, T, dense) in enumerate(CASES):
        d = inputs(name, T, dense, 100 + seed)
        head = build_head(dict(type="CenterHead", logger=logging.getLogger("CenterHead"), **head_kwargs(T, dense))).double()
        ret, grads = run_loss(head, d, name, T, dense)
        arrays.update(d)
        arrays.update(flatten(ret, name, T, dense))
        arrays.update({"%s_grad_%s" % (name, k[len(name) + 1:]): g for k, g in grads.items()})
        print(name, [float(x) for x in ret["loss"]])
    make_golden.save("loss.npz", **arrays)


if __name__ == "__main__":
    main()
