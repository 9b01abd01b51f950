"""Bit comparison of the six row-BatchNorm entry points (futuredet_amd/csrc/fd_row_bn.h: fd_sparse_bn_train_forward / _backward, their
_bf16 forms, fd_dense_bn_nhwc_train_forward_bf16 / _backward_bf16) between two builds of the library on one box.  The libraries are
opened directly (an older build need not export what lib.SIGNATURES lists), one process per library, then the comparison; the other
build comes from a worktree of its commit:

    git worktree add ../parent HEAD~1 && python ../parent/futuredet_amd/build.py
    python tools/row_bn_ab.py dump ../parent/futuredet_amd/libfuturedet_hip.so a.pt
    python tools/row_bn_ab.py dump futuredet_amd/libfuturedet_hip.so b.pt
    python tools/row_bn_ab.py compare a.pt b.pt

Inputs are those of tests/test_gpu_sparse_bn.py (seed 7, offset 30), P the chunk.
Sparse, fp32 and bf16 rows, all three forms: C in {16, 48, 128} at n = 3 P + 17 with the row count from the host and with n_dev holding
0, 1, P + 1 and n; n = 256 P + 1 (two chunks per group) at C = 16 and 128; n = 512 P + 1 (two chunks per apply block) at C = 16.
NHWC: C in {32, 96, 160, 512} at n in {2, 3 P + 17}, the record lists [64] * 6 and [32, 64] (each record with its own eps and momentum)
at 3 P + 17, the two large sizes at C = 32; relu on and off.
Every output is compared by bit pattern: y, saved, the running statistics, the counters, dx, d_residual, dgamma, dbeta."""
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SPARSE = ("fd_sparse_bn_chunk", "fd_sparse_bn_workspace_bytes", "fd_sparse_bn_train_forward", "fd_sparse_bn_train_backward",
          "fd_sparse_bn_train_forward_bf16", "fd_sparse_bn_train_backward_bf16")
NHWC = ("fd_dense_bn_nhwc_chunk", "fd_dense_bn_nhwc_workspace_bytes", "fd_dense_bn_nhwc_train_forward_bf16", "fd_dense_bn_nhwc_train_backward_bf16")
EPS, MOMENTUM = 1e-3, 0.1
BF = torch.bfloat16


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dump(lib_path, path):
    from futuredet_amd import lib
    from test_gpu_sparse_bn import FORMS, _inputs

    L = ctypes.CDLL(os.path.abspath(lib_path))
    for name in SPARSE + NHWC:
        getattr(L, name).restype, getattr(L, name).argtypes = lib.SIGNATURES[name]
    L.fd_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda")
    P = L.fd_sparse_bn_chunk()
    assert P == L.fd_dense_bn_nhwc_chunk()
    out = {"lib": os.path.abspath(lib_path)}
    problems = {}

    def problem(n, C):
        if (n, C) not in problems:
            problems[n, C] = {k: torch.from_numpy(v).to(dev) for k, v in _inputs(7, n, C, 30.0).items()}
        return problems[n, C]

    def keep(tag, tensors):
        for k, v in tensors.items():
            if v is not None:
                out["%s %s" % (tag, k)] = v.cpu()

    def sparse(n, C, dtype, nv):
        d = problem(n, C)
        rows = {k: d[k].to(dtype) for k in ("x", "res", "dy")}
        sfx = "_bf16" if dtype == BF else ""
        ws = torch.empty(L.fd_sparse_bn_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
        n_dev = None if nv is None else torch.tensor([nv], dtype=torch.int32, device=dev)
        for name, relu, with_res in FORMS:
            res = rows["res"] if with_res else None
            rm, rv, nbt = d["rm"].clone(), d["rv"].clone(), torch.zeros((), dtype=torch.int64, device=dev)
            y, dx = torch.empty_like(rows["x"]), torch.empty_like(rows["x"])
            dres = torch.empty_like(rows["x"]) if with_res else None
            saved, dgb = torch.empty((2, C), device=dev), torch.empty((2, C), device=dev)
            rc = getattr(L, "fd_sparse_bn_train_forward" + sfx)(p(rows["x"]), p(res), p(d["gamma"]), p(d["beta"]), n, p(n_dev), C, int(relu), EPS,
                                                                MOMENTUM, p(y), p(saved), p(rm), p(rv), p(nbt), p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            rc = getattr(L, "fd_sparse_bn_train_backward" + sfx)(p(rows["dy"]), p(rows["x"]), p(y), p(d["gamma"]), p(saved), n, p(n_dev), C,
                                                                 int(relu), p(dx), p(dres), p(dgb[0]), p(dgb[1]), p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            torch.cuda.synchronize()
            tag = "sparse %s n=%d C=%d n_dev=%s %s%s" % ("bf16" if dtype == BF else "fp32", n, C, nv, name, " (sums)" if nv is None or nv > 1 else "")
            keep(tag, dict(y=y, saved=saved, rm=rm, rv=rv, nbt=nbt, dx=dx, dres=dres, dgb=dgb))

    def nhwc(n, sizes):
        C = sum(sizes)
        d = problem(n, C)
        x, dy = d["x"].to(BF), d["dy"].to(BF)
        ws = torch.empty(L.fd_dense_bn_nhwc_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
        for relu in (1, 0):
            rm, rv, nbt = d["rm"].clone(), d["rv"].clone(), torch.zeros(len(sizes), dtype=torch.int64, device=dev)
            recs, o = [], 0
            for j, c in enumerate(sizes):  # each record its own eps and momentum
                recs.append(lib.DenseBnNhwcGroup(d["gamma"][o:].data_ptr(), d["beta"][o:].data_ptr(), rm[o:].data_ptr(), rv[o:].data_ptr(),
                                                 nbt[j:].data_ptr(), c, EPS * (1 + j), MOMENTUM / (1 + j)))
                o += c
            groups = (lib.DenseBnNhwcGroup * len(recs))(*recs)
            y, dx = torch.empty_like(x), torch.empty_like(x)
            saved, dgb = torch.empty((2, C), device=dev), torch.empty((2, C), device=dev)
            rc = L.fd_dense_bn_nhwc_train_forward_bf16(p(x), groups, len(recs), n, C, relu, p(y), p(saved), p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            rc = L.fd_dense_bn_nhwc_train_backward_bf16(p(dy), p(x), p(y), p(saved), groups, len(recs), n, C, relu, p(dx), p(dgb[0]), p(dgb[1]),
                                                        p(ws), ws.numel(), None)
            assert rc == 0, L.fd_last_error()
            torch.cuda.synchronize()
            keep("nhwc n=%d sizes=%s relu=%d (sums)" % (n, sizes, relu), dict(y=y, saved=saved, rm=rm, rv=rv, nbt=nbt, dx=dx, dgb=dgb))

    n3 = 3 * P + 17
    for dtype in (torch.float32, BF):
        for C in (16, 48, 128):
            for nv in (None, 0, 1, P + 1, n3):
                sparse(n3, C, dtype, nv)
        sparse(256 * P + 1, 16, dtype, None)
        sparse(256 * P + 1, 128, dtype, None)
        sparse(512 * P + 1, 16, dtype, None)
    for C in (32, 96, 160, 512):
        for n in (2, n3):
            nhwc(n, [C])
    nhwc(n3, [64] * 6)
    nhwc(n3, [32, 64])
    nhwc(256 * P + 1, [32])
    nhwc(512 * P + 1, [32])
    torch.save(out, path)
    print("wrote %d tensors from %s to %s" % (len(out) - 1, out["lib"], path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    print("A: %s\nB: %s" % (a.pop("lib"), b.pop("lib")))
    assert set(a) == set(b) and len(a) > 0

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == BF else t

    bad = [k for k in sorted(a) if not torch.equal(bits(a[k]), bits(b[k]))]
    # (with a device row count of 0 or 1 the outputs are zeros by construction: only the other cases carry "(sums)")
    zero = [k for k in sorted(a) if "(sums)" in k and k.split()[-1] in ("y", "dx", "dgb") and torch.count_nonzero(a[k].float()) == 0]
    assert not zero, zero
    print("%d tensors compared, %d differ%s" % (len(a), len(bad), (": " + ", ".join(bad)) if bad else ": the bits of all six entry points are unchanged"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2], sys.argv[3]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
