"""Shared by the fused-loss tests and tools/loss_bench.py: seeded CenterHead maps and targets of any head mode, one runner for the
torch path and the fused path (fd_loss.hip) that returns every loss term and map gradient as float64 arrays, and the agreement gate
(solver_util.rule: at most 4 x the fp32 torch path's own error against float64, floor one fp32 ulp)."""
import numpy as np
import torch

from solver_util import rule

HEADS = {8: ("reg", "height", "dim", "rot"), 10: ("reg", "height", "dim", "vel", "rot"),
         14: ("reg", "height", "dim", "vel", "rvel", "rot", "rrot")}
WIDTH = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "rrot": 2}


def head_of(T, dense, D=10, classes=(1,), weight=0.25):
    """A CenterHead of the mode: standard with len(classes) tasks, or dense (T one-class tasks)."""
    from futuredet_amd import build_head

    cw = {8: [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5], 10: [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0],
          14: [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 0.3, 0.3, 1.0, 1.0, 0.7, 0.7]}[D]
    tasks = [dict(num_class=c, class_names=["c%d_%d" % (i, j) for j in range(c)]) for i, c in enumerate(classes)]
    return build_head(dict(type="CenterHead", in_channels=64, tasks=tasks, dataset="nuscenes", weight=weight, code_weights=cw,
                           common_heads={k: (2, 2) if k in ("vel", "rvel") else (WIDTH[k], 2) for k in HEADS[D]},
                           share_conv_channel=64, dcn_head=False, timesteps=T, two_stage=False, reverse=False, sparse=False,
                           dense=dense, bev_map=False, forecast_feature=False, classify=False, wide_head=False))


def make_case(seed, B, H, W, M, T, dense, D=10, classes=(1,), row=None, n_obj=None, logits=None, place=None):
    """Seeded numpy inputs.  ``maps[k]``: the head maps of task k; ``steps[s][u]``: targets (hm, ind, mask, cat, anno_box) of step s,
    task u -- a dense head has T steps of one task, a standard head T steps of len(classes) tasks.  ``n_obj(s, u, b)``: objects of a
    target set (default: M - 3 - b); ``logits(rng, shape)``: raw heat map; ``place(s, u, b, ind, cat)``: edits the entries in place.
    Unused slots name cell 0 / class 0 with mask 0, as both target producers write them."""
    rng = np.random.default_rng(seed)
    row = row or (14 if D == 14 else 10)
    task_classes = [1] * T if dense else list(classes)
    maps = []
    for C in task_classes:
        m = {"hm": (logits(rng, (B, C, H, W)) if logits else rng.normal(-1.0, 1.5, (B, C, H, W))).astype(np.float32)}
        for k in HEADS[D]:
            c = WIDTH.get(k, 2 if dense else 2 * T)
            m[k] = rng.normal(0.0, 1.0, (B, c, H, W)).astype(np.float32)
        maps.append(m)
    steps = []
    for s in range(T):
        sets = []
        for u, C in enumerate([1] if dense else task_classes):
            hm = rng.uniform(0.0, 0.9, (B, C, H, W)).astype(np.float32) ** 3
            ind = np.zeros((B, M), np.int64)
            cat = np.zeros((B, M), np.int64)
            mask = np.zeros((B, M), np.uint8)
            for b in range(B):
                n = n_obj(s, u, b) if n_obj else max(M - 3 - b, 0)
                ind[b, :n] = rng.choice(H * W, n, replace=False)
                cat[b, :n] = rng.integers(0, C, n)
                mask[b, :n] = 1
                if place:
                    place(s, u, b, ind[b], cat[b], mask[b])
                for j in np.nonzero(mask[b])[0]:
                    hm[b, cat[b, j]].reshape(-1)[ind[b, j]] = 1.0
            sets.append(dict(hm=hm, ind=ind, cat=cat, mask=mask, anno_box=rng.normal(0.0, 1.0, (B, M, row)).astype(np.float32)))
        steps.append(sets)
    return dict(maps=maps, steps=steps, T=T, dense=dense, D=D, classes=task_classes)


def example_of(case, device, dtype):
    ex = {k: [] for k in ("hm", "ind", "mask", "cat", "anno_box")}
    for sets in case["steps"]:
        for k in ex:
            ex[k].append([torch.from_numpy(s[k]).to(device) for s in sets])
    for k in ("hm", "anno_box"):
        ex[k] = [[x.to(dtype) for x in row] for row in ex[k]]
    return ex


def collect(ret, preds, grads, dense):
    out = {}
    for t in range(len(ret["loss"])):
        out["t%d_loss" % t] = ret["loss"][t]
        out["t%d_hm_loss" % t] = ret["hm_loss"][t]
        out["t%d_loc_loss" % t] = torch.stack([x for x in ret["loc_loss"][t]])
        out["t%d_loc_loss_elem" % t] = ret["loc_loss_elem"][t] if dense else torch.stack(list(ret["loc_loss_elem"][t]))
        out["t%d_num_positive" % t] = ret["num_positive"][t]
        out["t%d_sig" % t] = preds[t]["hm"]
    out.update(grads)
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def run(head, case, device, dtype, fused, coeffs=None, ex=None):
    """head.loss on leaf maps -> {name: float64 array}: every term, the clamped sigmoid and the gradient of sum_k coeffs[k] loss[k]
    (default 1) w.r.t. every map."""
    leaves = [{k: torch.from_numpy(v).to(device).to(dtype).requires_grad_(True) for k, v in m.items()} for m in case["maps"]]
    preds = [{k: v * 1.0 for k, v in m.items()} for m in leaves]  # the torch path sigmoids hm into the dict: hand it non-leaves
    head.fused_loss = bool(fused)
    try:
        ret = head.loss(ex if ex is not None else example_of(case, device, dtype), preds)
    finally:
        head.fused_loss = False
    coeffs = coeffs or [1.0] * len(ret["loss"])
    sum(a * l for a, l in zip(coeffs, ret["loss"])).backward()
    grads = {"t%d_grad_%s" % (t, k): v.grad for t, m in enumerate(leaves) for k, v in m.items()}
    return collect(ret, preds, grads, case["dense"])


def run_wrappers(head, case, device, coeffs=None, shift=0):
    """The same outputs from hip_ops.centerhead_loss_forward / _backward called directly.  shift > 0 places every float tensor
    ``shift`` elements into a larger buffer: pointers that are not 16-byte aligned (the kernels' scalar path)."""
    from futuredet_amd import hip_ops

    def dev(a):
        t = torch.from_numpy(a).to(device)
        if shift and t.dtype == torch.float32:
            big = torch.zeros(t.numel() + shift + 3, dtype=t.dtype, device=device)
            big[shift:shift + t.numel()] = t.reshape(-1)
            t = big[shift:shift + t.numel()].view(a.shape)
        return t

    T, dense, D = case["T"], case["dense"], case["D"]
    n_tasks = len(case["maps"])
    tasks = []
    for k, m in enumerate(case["maps"]):
        sets = [case["steps"][k][0]] if dense else [case["steps"][i][k] for i in range(T)]
        tasks.append(dict(hm=dev(m["hm"]), hm_target=dev(sets[0]["hm"]), ind=dev(sets[0]["ind"]), cat=dev(sets[0]["cat"]),
                          mask=[dev(s["mask"]) for s in sets], anno_box=[dev(s["anno_box"]) for s in sets],
                          maps={n: dev(m[n]) for n in HEADS[D]}))
    B, _, H, W = case["maps"][0]["hm"].shape
    M, row = case["steps"][0][0]["anno_box"].shape[1:]
    cfg = hip_ops.make_loss_cfg(B, H, W, M, n_tasks, dense, T, D, row, head.code_weights,
                                getattr(head, "code_weights_forecast", None) if (not dense and T > 1) else None, head.weight)
    terms, sigs = hip_ops.centerhead_loss_forward(cfg, tasks)
    go = torch.tensor(coeffs or [1.0] * n_tasks, dtype=torch.float32).to(device)
    grads = hip_ops.centerhead_loss_backward(cfg, tasks, terms, go)
    stride, S = hip_ops.loss_terms_layout(cfg)
    out = {}
    for k in range(n_tasks):
        t = terms[k * stride:(k + 1) * stride]
        out["t%d_loss" % k], out["t%d_hm_loss" % k], out["t%d_num_positive" % k] = t[0], t[1], t[3]
        out["t%d_loc_loss" % k] = t[4:4 + S]
        out["t%d_loc_loss_elem" % k] = t[4 + S:].view(S, D)[0] if dense else t[4 + S:].view(S, D)
        out["t%d_sig" % k] = sigs[k]
        for n, g in grads[k].items():
            out["t%d_grad_%s" % (k, n)] = g
    out = {k: v.detach().double().cpu().numpy() for k, v in out.items()}
    out["status"] = np.float64(terms[-1].item())
    return out


def gate(tag, fused, yard, truth, lines=None):
    """solver_util.rule on every tensor of ``truth``; returns the worst fused error / bound ratio."""
    for k in sorted(truth):
        rule("%s %s" % (tag, k), fused[k], yard[k], truth[k], lines)
