"""Bit comparison of the fp32 sparse BatchNorm entry points between two builds of the library on one box: the outputs of
fd_sparse_bn_train_forward / _backward on the inputs of tests/test_gpu_sparse_bn.py::test_two_runs_are_bit_identical (n = 3 P + 17,
C = 16 and 128, offset 30, all three forms).  The libraries are opened directly (an older build need not export what lib.SIGNATURES
lists), one process per library, then the comparison:

    python tools/sparse_bn_ab.py dump libA.so a.pt
    python tools/sparse_bn_ab.py dump libB.so b.pt
    python tools/sparse_bn_ab.py compare a.pt b.pt
"""
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

NAMES = ("fd_sparse_bn_chunk", "fd_sparse_bn_workspace_bytes", "fd_sparse_bn_train_forward", "fd_sparse_bn_train_backward")
EPS, MOMENTUM = 1e-3, 0.1


def dump(lib_path, path):
    from futuredet_amd import lib
    from test_gpu_sparse_bn import FORMS, _inputs

    L = ctypes.CDLL(os.path.abspath(lib_path))
    for name in NAMES:
        getattr(L, name).restype, getattr(L, name).argtypes = lib.SIGNATURES[name]
    L.fd_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    out = {"lib": os.path.abspath(lib_path)}
    for C in (16, 128):
        n = 3 * L.fd_sparse_bn_chunk() + 17
        d = {k: torch.from_numpy(v).to(dev) for k, v in _inputs(7, n, C, 30.0).items()}
        ws = torch.empty(L.fd_sparse_bn_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
        for name, relu, with_res in FORMS:
            res = d["res"] if with_res else None
            rm, rv, nbt = d["rm"].clone(), d["rv"].clone(), torch.zeros((), dtype=torch.int64, device=dev)
            y, dx = torch.empty_like(d["x"]), torch.empty_like(d["x"])
            dres = torch.empty_like(d["x"]) if with_res else None
            saved, dgb = torch.empty((2, C), device=dev), torch.empty((2, C), device=dev)
            torch.cuda.synchronize()
            rc = L.fd_sparse_bn_train_forward(p(d["x"]), p(res), p(d["gamma"]), p(d["beta"]), n, None, C, int(relu), EPS, MOMENTUM, p(y), p(saved),
                                              p(rm), p(rv), p(nbt), p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            rc = L.fd_sparse_bn_train_backward(p(d["dy"]), p(d["x"]), p(y), p(d["gamma"]), p(saved), n, None, C, int(relu), p(dx), p(dres),
                                               p(dgb[0]), p(dgb[1]), p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            torch.cuda.synchronize()
            for k, v in dict(y=y, saved=saved, rm=rm, rv=rv, nbt=nbt, dx=dx, dres=dres, dgb=dgb).items():
                if v is not None:
                    out["C%d %s %s" % (C, name, k)] = v.cpu()
    torch.save(out, path)
    print("wrote %d tensors from %s to %s" % (len(out) - 1, out["lib"], path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    print("A: %s\nB: %s" % (a.pop("lib"), b.pop("lib")))
    assert set(a) == set(b) and len(a) > 0

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    bad = [k for k in sorted(a) if not torch.equal(bits(a[k]), bits(b[k]))]
    zero = [k for k in sorted(a) if k.split()[-1] in ("y", "dx", "dgb") and torch.count_nonzero(a[k]) == 0]
    assert not zero, zero
    print("%d tensors compared, %d differ%s" % (len(a), len(bad), (": " + ", ".join(bad)) if bad else ": the fp32 kernels' bits are unchanged"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2], sys.argv[3]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
