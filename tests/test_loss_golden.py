"""CenterHead.loss against the reference's own loss (tests/golden/loss.npz, made by tests/golden/make_golden_loss.py): every loss term
and the gradient of the summed loss w.r.t. every head map, for n0 (standard, T = 1), n3 (standard, T = 7) and n3dtf (dense, 7 tasks).
CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_golden_loss as mgl  # noqa: E402
from futuredet_amd import build_head  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "loss.npz"))


def _head(T, dense):
    return build_head(dict(type="CenterHead", **mgl.head_kwargs(T, dense))).double()


@pytest.mark.parametrize("name,T,dense", mgl.CASES)
def test_loss_matches_the_reference(name, T, dense):
    d = {k: GOLD[k] for k in GOLD.files}
    ret, grads = mgl.run_loss(_head(T, dense), d, name, T, dense)
    got = mgl.flatten(ret, name, T, dense)
    assert len(ret["loss"]) == (T if dense else 1)
    for k, v in got.items():
        np.testing.assert_allclose(v, GOLD[k], rtol=1e-10, atol=1e-12, err_msg=k)
    for k, g in grads.items():
        np.testing.assert_allclose(g, GOLD["%s_grad_%s" % (name, k[len(name) + 1:])], rtol=1e-10, atol=1e-12, err_msg=k)
    assert set(ret) == {"loss", "hm_loss", "loc_loss", "loc_loss_elem", "num_positive"}


def test_loss_of_other_modes_raises_naming_the_mode():
    kw = mgl.head_kwargs(3, False)
    for flag in ("reverse", "sparse", "wide_head"):
        head = build_head(dict(type="CenterHead", **dict(kw, **{flag: True})))
        with pytest.raises(NotImplementedError, match=flag):
            head.loss({}, [])
    head = build_head(dict(type="CenterHead", **dict(kw, classify=True)))
    with pytest.raises(NotImplementedError, match="classify"):
        head.loss({}, [])


def test_forecast_code_weights_keep_the_velocity_terms_only():
    head = _head(7, False)
    assert head.code_weights_forecast == [0.0] * 6 + [0.2, 0.2, 0.0, 0.0]


def test_loss_drives_a_cpu_training_step_of_the_head():
    """The head's torch modules in training mode: loss.backward() reaches every head parameter."""
    torch.manual_seed(0)
    head = build_head(dict(type="CenterHead", **mgl.head_kwargs(7, True))).train()
    d = {k: GOLD[k] for k in GOLD.files}
    ex = mgl.example_of(d, "n3dtf", 7)
    preds = head(torch.randn(2, 64, mgl.H, mgl.W))
    ret = head.loss(ex, preds)
    sum(ret["loss"]).backward()
    for n, p in head.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
