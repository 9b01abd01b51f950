"""Host side of the chunk plan (no GPU): its sizing formula for the data-free row capacities of the bench workload, the argument
checks that return before anything is launched, the tuning knob."""
import ctypes

import numpy as np

from futuredet_amd import hip_ops, lib


# the four strided convolutions of SpMiddleResNetFHD: (kernel, stride, padding)
GEOMS = [((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)), ((3, 1, 1), (2, 1, 1), (0, 0, 0))]


def test_plan_bytes_stay_within_their_bound_for_the_data_free_capacities():
    """A plan is the rulebook's shape plus one row: 28 rows of 4-byte words, each row the capacity + the 8 count words of the last
    chunk, rounded up to 64 words.  So bytes <= 112 * (capacity + 71), never less than 112 * (capacity + 8), and at most 28/27 of
    the level's rulebook table + 112 * 71 bytes -- for every level capacity of a 2 x 330000-voxel sweep (the bench's) and for the
    sizes around a row of 64 words."""
    L = lib.load()
    plan = hip_ops._PyramidPlan(2, (41, 1440, 1440), GEOMS, "cpu")
    caps = plan.row_caps(2 * 330000)
    assert len(caps) == 5 and all(c > 0 for c in caps)
    for cap in list(caps) + [0, 1, 55, 56, 57, 63, 64, 120, 128, (1 << 23) - 1]:
        stride, nbytes = int(L.fd_spconv_plan_stride(cap)), int(L.fd_spconv_plan_bytes(cap))
        assert stride % 64 == 0 and cap + 8 <= stride <= cap + 71
        assert nbytes == 28 * 4 * stride
        assert 112 * (cap + 8) <= nbytes <= 112 * (cap + 71)
        nbr_bytes = 27 * 4 * max(64, (cap + 63) // 64 * 64)  # SparseIndex.rulebook's table
        assert nbytes * 27 <= nbr_bytes * 28 + 27 * 112 * 71
    assert L.fd_spconv_plan_stride(-1) == 0 and L.fd_spconv_plan_bytes(-1) == 0


def test_plan_arguments_are_checked_before_any_launch():
    L = lib.load()
    buf = np.zeros(64 * 28, np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.fd_spconv_plan_build(p, 64, 26, 10, None, None, 0, p, 64, None) != 0 and b"K = 27" in L.fd_last_error()
    assert L.fd_spconv_plan_build(p, 64, 27, 65, None, None, 0, p, 128, None) != 0 and b"n_out" in L.fd_last_error()
    assert L.fd_spconv_plan_build(p, 64, 27, 60, None, None, 0, p, 64, None) != 0 and b"plan_stride" in L.fd_last_error()
    assert L.fd_spconv_plan_build(p, 64, 27, 10, None, p, 0, p, 64, None) != 0 and b"ranges" in L.fd_last_error()
    assert L.fd_spconv_plan_build(None, 64, 27, 0, None, None, 0, None, 0, None) == 0  # an empty level: nothing to do
    args = (p, 10, p, None, None, 0, p, 64, None, 0)
    assert L.fd_spconv_apply_plan(*args, 3, 10, None, 0, 32, 32, 0, p, p, 64, None) != 0 and b"K = 27" in L.fd_last_error()
    assert L.fd_spconv_apply_plan(*args, 27, 10, None, 0, 32, 64, 0, p, p, 64, None) != 0 and b"SubM" in L.fd_last_error()
    assert L.fd_spconv_apply_plan(*args, 27, 60, None, 0, 32, 32, 0, p, p, 64, None) != 0 and b"plan_stride" in L.fd_last_error()


def test_plan_knob_and_the_shapes_that_take_a_plan():
    L = lib.load()
    want = {(16, 16): 0, (32, 32): 1, (64, 64): 1, (128, 128): 1, (16, 32): 0, (32, 64): 0, (64, 128): 0}
    try:
        for (ci, co), w in want.items():
            assert L.fd_spconv_plan_wanted(ci, co, 0) == w, (ci, co)
            assert L.fd_spconv_plan_wanted(ci, co, 1) == 0  # bf16 keeps its own kernels
        assert L.fd_tuning_set(b"spconv_plan", -1) == 0
        assert all(L.fd_spconv_plan_wanted(ci, co, 0) == 0 for ci, co in want)
    finally:
        assert L.fd_tuning_set(b"spconv_plan", 0) == 0
