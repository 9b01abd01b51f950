"""Host side of the chunk plan made straight from the index (no GPU): fd_spconv_apply_plan's refusals of a launch without a rulebook
table, the layer shapes that run on a plan alone and the knob values that keep the table route, the argument checks of the two new
builders, and the agreement of header, bindings and exported symbols."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from futuredet_amd import lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fd_spconv_index_plan_wanted", "fd_spconv_plan_from_index", "fd_spconv_ranges_from_index")
INDEX_SHAPES = {(32, 32), (64, 64), (128, 128), (16, 32), (32, 64), (64, 128)}
EINVAL = -1  # FD_EINVAL
ALL_SHAPES = [(ci, co) for ci in (16, 32, 64, 128) for co in (16, 32, 64, 128)]


def _buf():
    buf = np.zeros(64 * 28, np.int32)
    return buf, buf.ctypes.data_as(ctypes.c_void_p)


def _apply_plan(L, p, nbr, cin, cout, plan, K=27, dtype=0, n_in=10):
    """fd_spconv_apply_plan on 10 output rows; every pointer but nbr / plan is the host buffer (a refusal returns before any is read)"""
    return L.fd_spconv_apply_plan(p, n_in, p, None, None, 0, nbr, 64, None, 0, K, 10, None, 0, cin, cout, dtype, p, plan, 64, None)


def test_apply_plan_refuses_a_missing_table_without_a_plan():
    L = lib.load()
    _, p = _buf()
    for cin, cout in ALL_SHAPES:
        assert _apply_plan(L, p, None, cin, cout, None) == EINVAL, (cin, cout)
        assert b"nbr == NULL" in L.fd_last_error()


def test_apply_plan_refuses_a_missing_table_for_an_unwanted_shape():
    """With a plan but no table: FD_EINVAL for every shape outside fd_spconv_index_plan_wanted, for bf16 rows and for K != 27 --
    before anything is launched (this test runs without a device)."""
    L = lib.load()
    _, p = _buf()
    for cin, cout in ALL_SHAPES:
        if (cin, cout) not in INDEX_SHAPES:
            assert _apply_plan(L, p, None, cin, cout, p) == EINVAL, (cin, cout)
            assert b"nbr == NULL" in L.fd_last_error()
    for cin, cout in sorted(INDEX_SHAPES):
        assert _apply_plan(L, p, None, cin, cout, p, dtype=1) == EINVAL and b"fp32" in L.fd_last_error()
        assert _apply_plan(L, p, None, cin, cout, p, K=3) == EINVAL and b"K = 27" in L.fd_last_error()
    # a wanted shape whose input rows do not fit the plan-reading kernels' 32-bit gather offsets: no kernel left without a table
    assert _apply_plan(L, p, None, 64, 128, p, n_in=1 << 23) == EINVAL and b"plan alone" in L.fd_last_error()


def test_index_plan_shapes_and_knob():
    L = lib.load()
    try:
        for cin, cout in ALL_SHAPES:
            assert L.fd_spconv_index_plan_wanted(cin, cout, 0) == int((cin, cout) in INDEX_SHAPES), (cin, cout)
            assert L.fd_spconv_index_plan_wanted(cin, cout, 1) == 0
        assert L.fd_tuning_set(b"spconv_plan", 1) == 0  # the table route: fd_rulebook + fd_spconv_plan_build
        assert all(L.fd_spconv_index_plan_wanted(ci, co, 0) == 0 for ci, co in ALL_SHAPES)
        assert [L.fd_spconv_plan_wanted(c, c, 0) for c in (16, 32, 64, 128)] == [0, 1, 1, 1]
        _, p = _buf()
        assert _apply_plan(L, p, None, 32, 32, p) == EINVAL and b"nbr == NULL" in L.fd_last_error()
        assert L.fd_tuning_set(b"spconv_plan", 2) == 0  # SubM plans from the index, the strided layers keep their tables
        assert {s for s in ALL_SHAPES if L.fd_spconv_index_plan_wanted(s[0], s[1], 0)} == {(32, 32), (64, 64), (128, 128)}
        assert L.fd_tuning_set(b"spconv_plan", -1) == 0  # no plans at all
        assert all(L.fd_spconv_index_plan_wanted(ci, co, 0) == 0 for ci, co in ALL_SHAPES)
    finally:
        assert L.fd_tuning_set(b"spconv_plan", 0) == 0


def _source(p, **kw):
    s = lib.PlanSource()
    s.in_words = s.in_prefix = s.out_coords = s.plan = p.value
    s.n_out, s.plan_stride, s.Din, s.Hin, s.Win, s.n_ranges = 10, 64, 9, 24, 24, 0
    s.stride[:], s.pad[:] = [1, 1, 1], [1, 1, 1]
    for k, v in kw.items():
        if k in ("stride", "pad"):
            getattr(s, k)[:] = v
        else:
            setattr(s, k, v)
    return s


@pytest.mark.parametrize("kw, word", [(dict(n_out=-1), b"n_out"), (dict(n_out=60), b"plan_stride"), (dict(ranges=1, n_ranges=0), b"ranges"),
                                      (dict(stride=[1, 5, 1]), b"stride"), (dict(pad=[3, 1, 1]), b"stride/pad"), (dict(Din=65), b"D must"),
                                      (dict(plan=None), b"null"), (dict(out_coords=None), b"null")])
def test_plan_from_index_checks_its_sources_before_any_launch(kw, word):
    L = lib.load()
    _, p = _buf()
    if "ranges" in kw:
        kw = dict(kw, ranges=p.value)
    arr = (lib.PlanSource * 2)(_source(p), _source(p, **kw))
    assert L.fd_spconv_plan_from_index(2, 2, arr, None) == EINVAL
    assert word in L.fd_last_error(), L.fd_last_error()


def test_builders_check_counts_and_take_empty_levels():
    L = lib.load()
    _, p = _buf()
    one = (lib.PlanSource * 1)(_source(p, n_out=0, plan=None, out_coords=None))
    assert L.fd_spconv_plan_from_index(2, 1, one, None) == 0  # an empty level: nothing to do, nothing launched
    assert L.fd_spconv_plan_from_index(2, 0, one, None) == EINVAL and L.fd_spconv_plan_from_index(2, 9, one, None) == EINVAL
    assert L.fd_spconv_plan_from_index(2, 1, None, None) == EINVAL
    ws = L.fd_spconv_ranges_workspace_bytes(10)
    assert L.fd_spconv_ranges_from_index(None, 2, 9, 24, 24, p, 10, None, 4, p, p, ws, None) == EINVAL and b"null" in L.fd_last_error()
    assert L.fd_spconv_ranges_from_index(p, 2, 9, 24, 24, p, 10, None, 0, p, p, ws, None) == EINVAL and b"sizes" in L.fd_last_error()
    assert L.fd_spconv_ranges_from_index(p, 2, 65, 24, 24, p, 10, None, 4, p, p, ws, None) == EINVAL and b"D must" in L.fd_last_error()
    assert L.fd_spconv_ranges_from_index(p, 2, 9, 24, 24, p, 10, None, 4, p, p, ws - 1, None) == EINVAL and b"workspace" in L.fd_last_error()


def test_declared_bound_and_exported_symbols_agree():
    """The new entry points are declared in the header, bound in lib.SIGNATURES with the header's argument count, and exported; the
    ABI version did not move (no existing signature changed); fd_plan_source and its ctypes mirror hold the same members in the
    same order."""
    L = lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "futuredet_hip.h")).read(), flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name + " is not declared"
        assert name in lib.SIGNATURES and name in exported, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
    assert L.fd_abi_version() == lib.ABI_VERSION == 8
    body = re.search(r"typedef struct fd_plan_source \{(.*?)\} fd_plan_source;", hdr, flags=re.S).group(1)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            members += [re.sub(r"\[\d+\]", "", w.strip().lstrip("*")) for w in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert members == [n for n, _ in lib.PlanSource._fields_], members
    assert ctypes.sizeof(lib.PlanSource) == 6 * 8 + 2 * 8 + 4 * 4 + 6 * 4
