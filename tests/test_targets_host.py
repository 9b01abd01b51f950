"""-m "not gpu": the host side of the AssignLabel stage (futuredet_amd/targets.py) and the assigner settings of the config builders."""
import json
import os

import numpy as np
import pytest

import futuredet_amd as fa
from futuredet_amd.configs import centerpoint_config, pointpillars_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stage(cfg):
    return fa.build_from_cfg(dict(type="AssignLabel", cfg=cfg), fa.PIPELINES)


def test_assign_label_outside_train_mode_gives_empty_targets():
    cfg = centerpoint_config("forecast_n3dtf").train_cfg.assigner
    res = dict(mode="val", type="NuScenesDataset", lidar=dict(annotations=dict(boxes=[np.zeros((0, 9), np.float32)] * 7)))
    res, info = _stage(cfg)(res, "info")
    assert res["lidar"]["targets"] == {} and info == "info"


def test_assign_label_refuses_other_datasets():
    cfg = centerpoint_config("forecast_n0").train_cfg.assigner
    res = dict(mode="train", type="WaymoDataset", lidar=dict(annotations=dict(gt_boxes=[np.zeros((0, 12), np.float32)])))
    with pytest.raises(NotImplementedError, match="NuScenesDataset"):
        _stage(cfg)(res, None)


def test_trajectory_sampler_needs_one_task():
    from futuredet_amd.targets import TargetAssigner

    cfg = dict(centerpoint_config("forecast_n3dtf").train_cfg.assigner)
    cfg["target_assigner"] = dict(tasks=[dict(num_class=1, class_names=["car"]), dict(num_class=1, class_names=["truck"])])
    with pytest.raises(ValueError, match="one task"):
        TargetAssigner(cfg, np.array([1440, 1440, 40]), [-54, -54, -5, 54, 54, 3], [0.075, 0.075, 0.2])


def test_config_builder_assigner_matches_parsed_reference_configs():
    g = json.load(open(os.path.join(REPO, "tests", "golden", "configs.json")))
    for fname, variant, cls in [("nusc_centerpoint_forecast_n0_detection.py", "forecast_n0", "car"),
                                ("nusc_centerpoint_forecast_n3_detection.py", "forecast_n3", "car"),
                                ("nusc_centerpoint_forecast_n3dtf_detection.py", "forecast_n3dtf", "car"),
                                ("nusc_centerpoint_forecast_n3dtfm_detection.py", "forecast_n3dtfm", "car"),
                                ("nusc_centerpoint_pedestrian_forecast_n0_detection.py", "forecast_n0", "pedestrian"),
                                ("nusc_centerpoint_pedestrian_forecast_n3_detection.py", "forecast_n3", "pedestrian"),
                                ("nusc_centerpoint_pedestrian_forecast_n3dtf_detection.py", "forecast_n3dtf", "pedestrian"),
                                ("nusc_centerpoint_pedestrian_forecast_n3dtfm_detection.py", "forecast_n3dtfm", "pedestrian")]:
        assert _plain(centerpoint_config(variant, cls).train_cfg) == {"assigner": g[fname]["assigner"]}, fname
    for fname, cls in [("nusc_centerpoint_pp_forecast_n3dtf_detection.py", "car"),
                       ("nusc_centerpoint_pp_pedestrian_forecast_n3dtf_detection.py", "pedestrian")]:
        assert _plain(pointpillars_config(cls).train_cfg) == {"assigner": g[fname]["assigner"]}, fname


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v
