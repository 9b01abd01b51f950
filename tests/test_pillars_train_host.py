"""-m "not gpu": the host surface of the train-mode pillar reader (csrc/fd_pillars_grad.hip): exported symbols, the workspace
query, and the argument checks, which return an error before any HIP runtime call."""
import ctypes
import os
import subprocess

import pytest
import torch

from futuredet_amd import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fd_pillar_train_workspace_bytes", "fd_pillar_train_forward", "fd_pillar_train_backward")
FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused by its argument checks


@pytest.fixture(scope="module")
def L():
    from futuredet_amd import build

    build.build()
    return lib.load()


def test_the_library_exports_the_train_reader(L):
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in NAMES:
        assert " T %s\n" % name in nm, name
        assert name in lib.SIGNATURES
    assert L.fd_abi_version() == 8


def test_workspace_query(L):
    assert L.fd_pillar_train_workspace_bytes(30000, 20) > 30000 * 64 * 5
    assert L.fd_pillar_train_workspace_bytes(4 * 30000, 20) > L.fd_pillar_train_workspace_bytes(30000, 20)
    assert L.fd_pillar_train_workspace_bytes(0, 20) == 0
    assert L.fd_pillar_train_workspace_bytes(100, 33) == 0


def _forward(L, m=100, P=20, ndim=5, u1=32, u2=64, voxels=FAKE, ws_bytes=None):
    ws = L.fd_pillar_train_workspace_bytes(m, P) if ws_bytes is None else ws_bytes
    return L.fd_pillar_train_forward(voxels, FAKE, FAKE, m, P, ndim, 0, 0.2, 0.2, -51.1, -51.1, FAKE, FAKE, FAKE, u1, 1e-3, FAKE, FAKE, FAKE,
                                     u2, 1e-3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)


def _backward(L, m=100, P=20, u1=32, u2=64, dout=FAKE, ws_bytes=None):
    ws = L.fd_pillar_train_workspace_bytes(m, P) if ws_bytes is None else ws_bytes
    return L.fd_pillar_train_backward(FAKE, FAKE, FAKE, m, P, 5, 1, 0.2, 0.2, -51.1, -51.1, FAKE, FAKE, FAKE, u1, FAKE, FAKE, FAKE, u2, dout,
                                      FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)


@pytest.mark.parametrize("call", [_forward, _backward])
@pytest.mark.parametrize("kwargs, message", [
    (dict(P=0), b"max_points"),
    (dict(P=33), b"max_points"),
    (dict(u1=64, u2=64), b"unsupported units"),
    (dict(u1=32, u2=32), b"unsupported units"),
    (dict(m=1, P=1), b"more than 1 value per channel"),
    (dict(ws_bytes=1024), b"workspace too small"),
])
def test_invalid_arguments_are_refused(L, call, kwargs, message):
    assert call(L, **kwargs) != 0
    assert message in L.fd_last_error(), L.fd_last_error()


def test_null_pointers_are_refused(L):
    assert _forward(L, voxels=None) != 0
    assert b"null argument" in L.fd_last_error()
    assert _backward(L, dout=None) != 0
    assert b"null dout" in L.fd_last_error()


def test_reader_refuses_other_stacks_in_training():
    from futuredet_amd.readers import PillarFeatureNet

    net = PillarFeatureNet(num_input_features=5, num_filters=[64], with_distance=True).train()
    with pytest.raises(NotImplementedError, match="num_filters=\\[64, 64\\]"):
        net(torch.zeros((4, 20, 5)), torch.ones(4, dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int32))
    net = PillarFeatureNet(num_input_features=5, num_filters=[64, 64]).train()
    net.compute_dtype = torch.bfloat16
    with pytest.raises(NotImplementedError, match="fp32"):
        net(torch.zeros((4, 20, 5)), torch.ones(4, dtype=torch.int32), torch.zeros((4, 4), dtype=torch.int32))
