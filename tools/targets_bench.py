"""Device time of the training targets (fd_assign_targets: object pass + heat-map pass) for B = 4, T = 7 on the 180 x 180 map of the
VoxelNet configs, standard and trajectory samplers, about 40 and about 500 objects per timestep.  Each line times graph replays of 20
back-to-back calls (no host work inside the timed region) and reports the heat-map write rate next to densify_nhwc_vec's.

    python tools/targets_bench.py [--reps 20] [--cpu-reference]

--cpu-reference also times the reference's numpy stage on the host running this script (needs the reference tree and the import
shims of tests/golden/make_golden.py; a different machine from the GPU host in general -- the line says which host it ran on)."""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from futuredet_amd.configs import centerpoint_config  # noqa: E402
from futuredet_amd.targets import TargetAssigner  # noqa: E402

# densify_nhwc_vec (DESIGN.md kernel map): 2 x 256 x 180 x 180 fp32 written in 30.4 us
DENSIFY_RATE = 2 * 256 * 180 * 180 * 4 / 30.4e-6
GRID = np.array([1440, 1440, 40])


def inputs(B, T, n, seed, dev):
    rng = np.random.default_rng(seed)
    boxes = np.zeros((B, T, n, 12), np.float32)
    boxes[..., 0:2] = rng.uniform(-54.0, 54.0, (B, T, n, 2))
    boxes[..., 2] = rng.normal(-0.5, 0.5, (B, T, n))
    boxes[..., 3:6] = np.array([1.9, 4.6, 1.7], np.float32) * rng.uniform(0.6, 1.4, (B, T, n, 3))
    boxes[..., 6:10] = rng.normal(0.0, 3.0, (B, T, n, 4))
    boxes[..., 10:12] = rng.uniform(-np.pi, np.pi, (B, T, n, 2))
    counts = rng.integers(int(n * 0.8), n + 1, (B, T)).astype(np.int32)
    return [torch.from_numpy(a).to(dev) for a in (boxes, counts, np.ones((B, T, n), np.int32),
                                                   rng.integers(0, 3, (B, T, n)).astype(np.int32))]


def run(variant, n, reps, B=4, T=7):
    dev = torch.device("cuda:0")
    cfg = centerpoint_config(variant)
    acfg = dict(cfg.train_cfg.assigner)
    if acfg["sampler_type"] != "standard" and T * n > acfg["max_objs"]:
        acfg["max_objs"] = 4096  # the forecast set holds every timestep's objects: T * n would trip the reference's assert at 1000
    vg = cfg.voxel_generator
    ta = TargetAssigner(acfg, GRID, vg["range"], vg["voxel_size"])
    args = inputs(B, T, n, 1, dev)
    traj = args[3] if ta.extra_sets else None
    out = ta.outputs(B, T, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            ta(*args[:3], traj, out=out, check=False)
    torch.cuda.current_stream().wait_stream(s)
    ta.check_status(out["status"])
    g = torch.cuda.CUDAGraph()
    calls = 20
    with torch.cuda.graph(g, stream=s):
        for _ in range(calls):
            ta(*args[:3], traj, out=out, check=False)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / calls)
    us = float(np.median(times))
    hm_bytes = (out["hm"].numel()) * 4
    row_bytes = sum(out[k].numel() * out[k].element_size() for k in ("ind", "mask", "cat", "anno_box", "gt_boxes_and_cls"))
    return dict(sampler=acfg["sampler_type"], variant=variant, B=B, T=T, objects_per_timestep=n, max_objs=acfg["max_objs"],
                maps=len(ta.channels), hm_MB=round(hm_bytes / 1e6, 2), rows_MB=round(row_bytes / 1e6, 2), us_per_call_median=round(us, 2),
                us_min=round(float(min(times)), 2), hm_write_TBps=round(hm_bytes / (us * 1e-6) / 1e12, 2),
                densify_nhwc_vec_TBps=round(DENSIFY_RATE / 1e12, 2), device=torch.cuda.get_device_name(0))


def cpu_reference(n, T=7):
    """The reference's numpy AssignLabel for ONE sample (B = 1), trajectory sampler, on this host's CPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden
    import make_golden_targets as mgt

    make_golden.install_shims()
    sys.path.insert(0, make_golden.REF)
    prep = make_golden._import_ref_pipeline("preprocess")
    import addict

    geo = mgt.geometry(180, 180, 8)
    c = mgt.seeded_case(9, T, [["car"]], geo, 8, traj=True, n=(n, n), max_objs=max(1000, T * n))
    stage = prep.AssignLabel(cfg=addict.Dict(c["cfg"]))
    times = []
    for _ in range(3):
        res = dict(mode="train", type="NuScenesDataset", lidar=dict(annotations={k: [np.copy(x) for x in v] for k, v in c["ann"].items()},
                                                                     voxels=dict(geo)))
        t0 = time.perf_counter()
        stage(res, None)
        times.append(time.perf_counter() - t0)
    return dict(what="reference numpy AssignLabel, one sample, trajectory sampler", host=platform.node(), cpu=platform.processor() or "?",
                objects_per_timestep=n, T=T, ms_per_sample_median=round(float(np.median(times)) * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reference", action="store_true")
    a = ap.parse_args()
    if a.cpu_reference:
        for n in (40, 500):
            print(json.dumps(cpu_reference(n)), flush=True)
        return
    for variant in ("forecast_n0", "forecast_n3dtf"):
        for n in (40, 500):
            print(json.dumps(run(variant, n, a.reps)), flush=True)


if __name__ == "__main__":
    main()
