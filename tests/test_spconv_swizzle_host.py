"""Host side of the bank-spread row layout (no GPU): the permutation as numpy states it and as hip_ops.swizzle_rows states it, the
new symbols in the header and in lib.py, the ABI version, the knob, and the refusals that return before anything is launched."""
import ctypes
import os
import re

import numpy as np
import torch

from futuredet_amd import hip_ops, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def swizzle_np(a):
    """16-byte piece s (4 floats) of row r at piece s ^ (r & 7) of its 128-byte line (32 floats); narrower rows stay"""
    n, c = a.shape
    if c < 32:
        return a.copy()
    out = np.empty_like(a)
    for r in range(n):
        for line in range(c // 32):
            for s in range(8):
                d = s ^ (r & 7)
                out[r, 32 * line + 4 * d:32 * line + 4 * d + 4] = a[r, 32 * line + 4 * s:32 * line + 4 * s + 4]
    return out


def test_the_permutation_is_an_involution_per_line():
    for c in (32, 64, 128):
        a = np.arange(21 * c, dtype=np.float32).reshape(21, c)
        s = swizzle_np(a)
        assert np.array_equal(swizzle_np(s), a)
        for r in range(21):
            for line in range(c // 32):  # a piece never leaves its line, and a line holds a permutation of its own pieces
                assert sorted(s[r, 32 * line:32 * line + 32]) == sorted(a[r, 32 * line:32 * line + 32])
        assert np.array_equal(s[0], a[0]) and np.array_equal(s[8], a[8]) and not np.array_equal(s[9], a[9])
        assert np.array_equal(s[3, 0:4], a[3, 12:16])  # piece 3 of row 3 sits at position 0
        assert np.array_equal(hip_ops.swizzle_rows(torch.from_numpy(a)).numpy(), s), "torch statement differs from numpy's"


def test_16_channel_rows_are_the_identity():
    a = np.arange(19 * 16, dtype=np.float32).reshape(19, 16)
    assert np.array_equal(swizzle_np(a), a)
    assert np.array_equal(hip_ops.swizzle_rows(torch.from_numpy(a)).numpy(), a)


def test_header_declares_the_entry_point_and_lib_mirrors_it():
    header = open(os.path.join(ROOT, "include", "futuredet_hip.h")).read()
    for name in ("fd_spconv_apply_layout", "fd_spconv_layout_wanted"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        n_args = len(m.group(1).split(","))
        fn = getattr(lib.load(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, name
    # fd_spconv_apply_plan's arguments plus the layout word in front of the stream
    L = lib.load()
    assert len(L.fd_spconv_apply_layout.argtypes) == len(L.fd_spconv_apply_plan.argtypes) + 1
    assert L.fd_spconv_apply_layout.argtypes[-2] is ctypes.c_int


def test_abi_version_is_unchanged():
    assert lib.load().fd_abi_version() == 8


def test_knob_and_wanted_bits():
    L = lib.load()
    try:
        assert L.fd_tuning_set(b"spconv_swz", 7) == 0
        want = {(32, 32): 7, (64, 64): 7, (128, 128): 7, (16, 32): 4, (32, 64): 4, (64, 128): 4, (16, 16): 0, (32, 16): 0, (128, 64): 0}
        for (ci, co), w in want.items():
            assert L.fd_spconv_layout_wanted(ci, co, 0) == w, (ci, co)
            assert L.fd_spconv_layout_wanted(ci, co, 1) == 0  # bf16 rows are never spread
        assert L.fd_tuning_set(b"spconv_swz", 1) == 0
        assert [L.fd_spconv_layout_wanted(*s, 0) for s in ((16, 32), (32, 32), (32, 64), (64, 64))] == [4, 7, 0, 0]
        assert L.fd_tuning_set(b"spconv_swz", -1) == 0
        assert all(L.fd_spconv_layout_wanted(ci, co, 0) == 0 for ci, co in want)
        assert not hip_ops.level_layout(16, 32, 1000, 500)
        assert L.fd_tuning_set(b"spconv_swz", 7) == 0
        assert hip_ops.level_layout(16, 32, 1000, 500)
        assert not hip_ops.level_layout(64, 128, 1 << 23, 1000) and not hip_ops.level_layout(64, 128, 1000, 1 << 22)  # the >= 2 GB fallback
    finally:
        assert L.fd_tuning_set(b"spconv_swz", 0) == 0


def test_refusals_return_before_any_launch():
    L = lib.load()
    buf = np.zeros(64 * 28, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    args = (p, 10, p, None, None, 0, p, 64, None, 0, 27, 10, None, 0)
    for cin, cout, dt, lay in [(16, 16, 0, 1), (16, 16, 0, 4), (16, 32, 0, 1), (32, 64, 0, 5), (64, 128, 0, 1), (32, 16, 0, 4), (32, 32, 1, 7),
                               (64, 64, 1, 4), (32, 32, 0, 8), (32, 32, 0, -1)]:
        assert L.fd_spconv_apply_layout(*args, cin, cout, dt, p, None, 0, lay, None) != 0, (cin, cout, dt, lay)
        assert b"fd_spconv_apply_layout" in L.fd_last_error()
    assert L.fd_spconv_apply_layout(*args, 32, 32, 0, p, p, 8, 7, None) != 0 and b"plan_stride" in L.fd_last_error()
