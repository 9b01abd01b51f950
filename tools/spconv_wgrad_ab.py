"""Bit comparison of the sparse convolution's training kernels between two builds of the library on one box: dW of every instantiation of
fd_spconv_wgrad (16 shapes) and fd_spconv_wgrad_bf16 (7) on a small SubM 3x3x3 table (batch 2, grid 9 x 24 x 24, about 1300 active voxels:
three 512-row chunks with a partial last one), once with the row count on the host and once with a device count below the capacity; and
the bytes of fd_spconv_pack_weight_device / _bf16 in their three modes for every shape they accept (kept as SHA-256 digests).  The weight
gradient's summation order is part of its contract, so the expected outcome is 0 differing tensors.  The libraries are opened directly, one
process per library, then the comparison:

    python tools/spconv_wgrad_ab.py dump libA.so a.pt
    python tools/spconv_wgrad_ab.py dump libB.so b.pt
    python tools/spconv_wgrad_ab.py compare a.pt b.pt
"""
import ctypes
import hashlib
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ("fd_spconv_wgrad_workspace_bytes", "fd_spconv_wgrad", "fd_spconv_wgrad_bf16_workspace_bytes", "fd_spconv_wgrad_bf16",
         "fd_spconv_packed_weight_bytes", "fd_spconv_pack_weight_device", "fd_spconv_pack_weight_device_bf16")
CH = (16, 32, 64, 128)
BF16_SHAPES = ((16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128))
GRID, PER_SAMPLE = (9, 24, 24), 650


def subm_table(rng):
    """nbr [27][stride] of a SubM 3x3x3 convolution over random active cells, rows in (batch, z, y, x) order; -1 = no neighbour"""
    D, H, W = GRID
    cells = np.concatenate([np.sort(rng.choice(D * H * W, PER_SAMPLE, replace=False)) + b * D * H * W for b in range(2)])
    row_of = {int(c): r for r, c in enumerate(cells)}
    b, rem = np.divmod(cells, D * H * W)
    z, rem = np.divmod(rem, H * W)
    y, x = np.divmod(rem, W)
    n = len(cells)
    nbr = np.full((27, (n + 63) // 64 * 64), -1, np.int32)
    for k in range(27):
        dz, dy, dx = k // 9 - 1, k // 3 % 3 - 1, k % 3 - 1
        zz, yy, xx = z + dz, y + dy, x + dx
        ok = (zz >= 0) & (zz < D) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        for r in np.nonzero(ok)[0]:
            nbr[k, r] = row_of.get(int(((b[r] * D + zz[r]) * H + yy[r]) * W + xx[r]), -1)
    return nbr, n


def dump(lib_path, path):
    from futuredet_amd import lib

    L = ctypes.CDLL(os.path.abspath(lib_path))
    for name in NAMES:
        getattr(L, name).restype, getattr(L, name).argtypes = lib.SIGNATURES[name]
    L.fd_last_error.restype = ctypes.c_char_p
    dev = torch.device("cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    out = {"lib": os.path.abspath(lib_path)}
    rng = np.random.default_rng(3)
    table, n = subm_table(rng)
    nbr = torch.from_numpy(table).to(dev)
    assert (n + 511) // 512 == 3 and n % 512 != 0 and int((table[:, :n] >= 0).sum()) > 27 * 64
    cut = torch.tensor([n - 333], dtype=torch.int32, device=dev)  # ends inside the second chunk
    x32 = {c: torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)).to(dev) for c in CH}
    g32 = {c: torch.from_numpy(rng.uniform(-1, 1, (n, c)).astype(np.float32)).to(dev) for c in CH}
    for tag, fn, ws_fn, shapes, cast in (("f32", L.fd_spconv_wgrad, L.fd_spconv_wgrad_workspace_bytes, [(a, b) for a in CH for b in CH], torch.float32),
                                         ("bf16", L.fd_spconv_wgrad_bf16, L.fd_spconv_wgrad_bf16_workspace_bytes, BF16_SHAPES, torch.bfloat16)):
        for cin, cout in shapes:
            x, dy = x32[cin].to(cast), g32[cout].to(cast)
            ws = torch.empty(ws_fn(27, n, cin, cout), dtype=torch.uint8, device=dev)
            for count, n_dev in (("host count", None), ("device count", cut)):
                dw = torch.full((27, cin, cout), float("nan"), device=dev)
                torch.cuda.synchronize()
                rc = fn(p(x), n, p(dy), p(nbr), nbr.shape[1], 27, n, p(n_dev), cin, cout, p(dw), p(ws), ws.numel(), None)
                assert rc == 0, L.fd_last_error()
                torch.cuda.synchronize()
                out["dw %s %d->%d %s" % (tag, cin, cout, count)] = dw.cpu()

    ok16 = (16, 32, 64, 96, 128)  # bf16: the packed problem's input channels
    for tag, fn, dtype in (("f32", L.fd_spconv_pack_weight_device, 0), ("bf16", L.fd_spconv_pack_weight_device_bf16, 1)):
        for cin in range(16, 129, 16):
            for cout in range(16, 129, 16):
                for K in (27, 2):
                    w = torch.from_numpy(rng.standard_normal((K, cin, cout)).astype(np.float32))
                    bits = w.view(torch.int32).view(-1)  # bf16 ties of both parities and their neighbours
                    bits[0::3] = (bits[0::3] & -65536) | 0x8000
                    bits[1::7] = (bits[1::7] & -65536) | 0x7FFF
                    bits[2::7] = (bits[2::7] & -65536) | 0x8001
                    wd = w.to(dev)
                    for mode in (0, 1, 2):
                        ci, co = (cout, cin) if mode else (cin, cout)
                        if dtype == 1 and ci not in ok16:
                            continue
                        dst = torch.full((L.fd_spconv_packed_weight_bytes(K, ci, co, dtype),), 0xA5, dtype=torch.uint8, device=dev)
                        rc = fn(p(wd), K, cin, cout, mode, p(dst), None)
                        assert rc == 0, L.fd_last_error()
                        torch.cuda.synchronize()
                        out["pack %s %d->%d K%d mode %d" % (tag, cin, cout, K, mode)] = hashlib.sha256(dst.cpu().numpy().tobytes()).hexdigest()
    torch.save(out, path)
    print("wrote %d tensors from %s to %s" % (len(out) - 1, out["lib"], path))


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    print("A: %s\nB: %s" % (a.pop("lib"), b.pop("lib")))
    assert set(a) == set(b) and len(a) > 0

    def same(u, v):
        return u == v if isinstance(u, str) else torch.equal(u.view(torch.int32), v.view(torch.int32))

    bad = [k for k in sorted(a) if not same(a[k], b[k])]
    dws = [k for k in a if k.startswith("dw ")]
    empty = [k for k in dws if not bool(torch.isfinite(a[k]).all()) or torch.count_nonzero(a[k]) == 0]
    assert not empty, empty
    assert len(dws) == 2 * (16 + 7) and all(not torch.equal(a[k], a[k.replace("host", "device")]) for k in dws if "host" in k)
    print("%d tensors compared (%d weight gradients, %d packed buffers), %d differ%s"
          % (len(a), len(dws), len(a) - len(dws), len(bad), (": " + ", ".join(bad)) if bad else ": the bits are unchanged"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2], sys.argv[3]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
