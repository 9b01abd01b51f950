"""fd_spconv_pack_weight on the CPU, byte for byte, against a NumPy statement of every section's element order (the packed-weight
buffer of the sparse convolution, csrc/fd_spconv_pack.h).  The statement is the forward one -- "element [k][c][nb][lane][j] of the section
is W[k][a][b]" -- where the library decodes an element index back into (k, a, b): a slip in either shows up as a byte difference.  Every
shape the packer accepts, K odd and even (the zero half of the last tap pair).  CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

from futuredet_amd import build, lib  # noqa: E402

CHANNELS = list(range(16, 129, 16))
TAPS = (1, 2, 3, 27)


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _bf16_rne(v):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _grid(*dims):
    return np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")


def _expected(w, dtype):
    """the buffer's bytes: each section as the array its kernel indexes, filled by the forward rule"""
    K, cin, cout = w.shape
    NB = cout // 16
    if dtype == 0:
        k, c, nb, lane, j = _grid(K, cin // 16, NB, 64, 4)
        out = [w[k, 16 * c + 4 * (lane >> 4) + j, 16 * nb + (lane & 15)]]
        if cin == 32 and cout == 32:  # c32: the 32x32x2 fragments
            k, c, lane, j = _grid(K, cin // 8, 64, 4)
            out.append(w[k, 8 * c + 4 * (lane >> 5) + j, lane & 31])
        return np.concatenate([s.astype(np.float32).ravel() for s in out]).tobytes()
    if cin >= 32:
        k, c, nb, lane, j = _grid(K, cin // 32, NB, 64, 8)
        out = [_bf16_rne(w[k, 32 * c + 8 * (lane >> 4) + j, 16 * nb + (lane & 15)])]
        if (cin, cout) in ((64, 64), (128, 128)):  # win: the 32x32x16 fragments of the LDS-window kernel
            SC = min(cin, 64)
            k, h, s, cb, lane, j = _grid(K, cin // SC, SC // 16, cout // 32, 64, 8)
            out.append(_bf16_rne(w[k, SC * h + 16 * s + 8 * (lane >> 5) + j, 32 * cb + (lane & 31)]))
    else:
        k, nb, lane, j = _grid(K, NB, 64, 4)
        out = [_bf16_rne(w[k, 4 * (lane >> 4) + j, 16 * nb + (lane & 15)])]
        # pair: quads 0, 1 = channels 0..7 / 8..15 of tap 2 u, quads 2, 3 = those of tap 2 u + 1; zeros past K
        u, nb, lane, j = _grid((K + 1) // 2, NB, 64, 8)
        q = lane >> 4
        k = 2 * u + (q >> 1)
        v = _bf16_rne(w[np.minimum(k, K - 1), 8 * (q & 1) + j, 16 * nb + (lane & 15)])
        out.append(np.where(k < K, v, np.uint16(0)))
    return np.concatenate([s.ravel() for s in out]).tobytes()


def _weights(rng, K, cin, cout):
    w = rng.standard_normal((K, cin, cout)).astype(np.float32)
    bits = w.view(np.uint32).reshape(-1)  # every third value a bf16 tie (both parities), every seventh one ulp off a tie
    bits[0::3] = (bits[0::3] & 0xFFFF0000) | 0x8000
    bits[1::7] = (bits[1::7] & 0xFFFF0000) | 0x7FFF
    bits[2::7] = (bits[2::7] & 0xFFFF0000) | 0x8001
    assert np.isfinite(w).all()
    return w


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_host_pack_is_the_forward_order_byte_for_byte(L, dtype):
    rng = np.random.default_rng(17 + dtype)
    cins = CHANNELS if dtype == 0 else [c for c in CHANNELS if c == 16 or c % 32 == 0]
    assert len(cins) == (8 if dtype == 0 else 5)
    for cin in cins:
        for cout in CHANNELS:
            for K in TAPS:
                w = _weights(rng, K, cin, cout)
                want = _expected(w, dtype)
                n = L.fd_spconv_packed_weight_bytes(K, cin, cout, dtype)
                assert n == len(want), (dtype, K, cin, cout, n, len(want))
                got = np.full(n + 64, 0xA5, np.uint8)  # a guard behind the buffer
                assert L.fd_spconv_pack_weight(w.ctypes.data_as(ctypes.c_void_p), K, cin, cout, dtype, got.ctypes.data_as(ctypes.c_void_p)) == 0
                assert got[:n].tobytes() == want, (dtype, K, cin, cout)
                assert (got[n:] == 0xA5).all(), (dtype, K, cin, cout)


def test_host_pack_refuses_what_it_cannot_lay_out(L):
    w = np.zeros((3, 128, 128), np.float32)
    out = np.zeros(2 * w.size, np.float32)
    p, q = w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for cin in (48, 80, 112):  # bf16: 16 input channels or chunks of 32
        assert L.fd_spconv_pack_weight(p, 3, cin, 16, 1, q) == -1
        assert b"fd_spconv_pack_weight: bf16 needs" in L.fd_last_error()
        assert L.fd_spconv_pack_weight(p, 3, cin, 16, 0, q) == 0
    for args, text in (((0, 16, 16, 0), b"K must be in [1,27]"), ((28, 16, 16, 0), b"K must be in [1,27]"), ((3, 16, 144, 0), b"multiples of 16"),
                       ((3, 8, 16, 1), b"multiples of 16"), ((3, 16, 16, 2), b"dtype must be")):
        assert L.fd_spconv_pack_weight(p, *args[:3], args[3], q) == -1
        assert b"fd_spconv_pack_weight: " in L.fd_last_error() and text in L.fd_last_error(), (args, L.fd_last_error())
    assert L.fd_spconv_pack_weight(None, 3, 16, 16, 0, q) == -1 and b"null argument" in L.fd_last_error()
