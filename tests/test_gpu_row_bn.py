"""-m gpu: the two APIs over the row-BatchNorm kernels (futuredet_amd/csrc/fd_row_bn.h) give the same bits where their domains
overlap: bf16 rows, C a multiple of 32 up to 128, one set of parameters, no residual, the row count from the host, n >= 2.

fd_sparse_bn_train_forward_bf16 / _backward_bf16 (no residual, no n_dev) against fd_dense_bn_nhwc_train_forward_bf16 / _backward_bf16
with one record, on the same inputs, eps and momentum: y, saved, running_mean, running_var, the counter, dx, dgamma and dbeta agree in
every bit.  Inputs of the kind of test_gpu_sparse_bn.py's inputs (b): an offset of +-30 on half the channels, spread 0.5."""
import numpy as np
import pytest
import torch
from torch import nn

from test_gpu_sparse_bn_bf16 import _same_bits

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BF = torch.bfloat16
EPS, MOMENTUM = 1e-3, 0.1


def _P(hip):
    assert hip.sparse_bn_chunk() == hip.dense_bn_nhwc_chunk()
    return hip.sparse_bn_chunk()


def _two_chunks(hip):
    """the smallest row count at which a group of the statistics holds two chunks (the last chunk has one row)"""
    from futuredet_amd import lib

    return lib.load().fd_dense_bn_nhwc_stat_groups() * _P(hip) + 1


def _inputs(seed, n, C):
    rng = np.random.default_rng(seed)
    ch = np.arange(C)
    x = rng.normal(0.0, 0.5, (n, C)) + np.where(ch % 4 == 0, 30.0, np.where(ch % 4 == 2, -30.0, 0.0))
    d = dict(x=x, dy=rng.normal(0.0, 1.0, (n, C)), gamma=rng.uniform(0.5, 1.5, C), beta=rng.normal(0.0, 0.5, C), rm=rng.normal(0.0, 1.0, C),
             rv=rng.uniform(0.5, 2.0, C))
    t = {k: torch.from_numpy(v.astype(np.float32)).to(DEV) for k, v in d.items()}
    t["x"], t["dy"] = t["x"].to(BF), t["dy"].to(BF)
    return t


def _sparse(hip, t, relu):
    rm, rv, nbt = t["rm"].clone(), t["rv"].clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    y, saved = hip.sparse_bn_train_forward(t["x"], t["gamma"], t["beta"], rm, rv, nbt, EPS, MOMENTUM, relu=relu)
    dx, dres, dgamma, dbeta = hip.sparse_bn_train_backward(t["dy"], t["x"], y, t["gamma"], saved, relu=relu)
    assert dres is None
    return dict(y=y, saved=saved, running_mean=rm, running_var=rv, counter=nbt, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _nhwc(hip, t, relu):
    C = t["x"].shape[1]
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(t["gamma"])
        bn.bias.copy_(t["beta"])
        bn.running_mean.copy_(t["rm"])
        bn.running_var.copy_(t["rv"])
    y, saved = hip.dense_bn_nhwc_train_forward(t["x"], bn, relu=relu)
    dx, dgamma, dbeta = hip.dense_bn_nhwc_train_backward(t["dy"], t["x"], y, saved, bn, relu=relu)
    return dict(y=y, saved=saved, running_mean=bn.running_mean, running_var=bn.running_var, counter=bn.num_batches_tracked, dx=dx,
                dgamma=dgamma, dbeta=dbeta)


CASES = [(C, n_of) for C in (32, 96, 128) for n_of in ("2", "63", "P+1", "3P+17")] + [(32, "two chunks per group")]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("C,n_of", CASES, ids=["C%d n=%s" % c for c in CASES])
def test_sparse_and_nhwc_entry_points_give_the_same_bits(hip, C, n_of, relu):
    P = _P(hip)
    n = {"2": 2, "63": 63, "P+1": P + 1, "3P+17": 3 * P + 17, "two chunks per group": _two_chunks(hip)}[n_of]
    t = _inputs(n * 1000 + C, n, C)
    a, b = _sparse(hip, t, relu), _nhwc(hip, t, relu)
    assert set(a) == set(b)
    for k in ("y", "dx", "dgamma", "saved"):
        assert torch.count_nonzero(a[k].float()) > 0, (k, "all zero")
    assert int(a["counter"]) == 1
    for k in a:
        assert _same_bits(a[k].reshape(-1), b[k].reshape(-1)), "%s differs between the two entry points (n = %d, C = %d, relu = %s)" % (k, n, C, relu)
