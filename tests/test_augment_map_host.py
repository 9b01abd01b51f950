"""The host side of the bev-mask warp and the ground-truth range filter (csrc/fd_augment_map.hip, futuredet_amd/augment.py, the
``filter_gt`` keyword and ``GlobalAugment(warp_bev=True)`` of the static steps): the numpy restatements of the kernels' arithmetic
(tests/augment_map_ref.py, tests/range_filter_ref.py) against closed forms and against the reference's recorded masks
(tests/golden/range_filter.npz), exported symbols, the ctypes / numpy mirrors of the new record, argument checks (no device needed: they
come before any device work), mask_record against closed forms and the steps' host-side behaviour.  CPU only."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import augment_map_ref as am  # noqa: E402
import range_filter_ref as rf  # noqa: E402
from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402

NAMES = {"fd_gt_range_filter", "fd_augment_mask", "fd_augment_mask_check"}
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False), class_names=["car"])
H = W = 180


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


@pytest.fixture(scope="module")
def plane():
    return np.random.default_rng(0).random((H, W), dtype=np.float32)


def _mask(plane, fa=0, fb=0, rot=0.0, scale=1.0, tx=0.0, ty=0.0):
    return am.get_mask_plane(plane, [fa, fb, rot, scale, tx, ty, 0.0])


def _same(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the warp restatement: bit for bit, cases that hold for any correct implementation
def test_warp_identity_and_flips(plane):
    assert _same(_mask(plane), plane)
    assert _same(_mask(plane, fa=1), np.ascontiguousarray(plane[:, ::-1]))  # the first flip reverses W (np.fliplr)
    assert _same(_mask(plane, fb=1), np.ascontiguousarray(plane[::-1]))
    assert _same(_mask(plane, fa=1, fb=1), np.ascontiguousarray(plane[::-1, ::-1]))


def test_warp_translations(plane):
    want = np.zeros_like(plane)
    want[:H - 2, 3:] = plane[2:, :W - 3]
    assert _same(_mask(plane, tx=3, ty=-2), want)
    half = np.float32(0.5)
    want = np.zeros_like(plane)
    want[:, 1:] = half * plane[:, :-1] + half * plane[:, 1:]
    want[:, 0] = half * plane[:, 0]  # a zero column to the left
    assert _same(_mask(plane, tx=0.5), want)
    assert not _mask(plane, tx=400.0).any()


def test_warp_quarter_turns_and_scale(plane):
    want = np.zeros_like(plane)
    for x in range(1, W):
        want[:, x] = plane[180 - x, :]
    assert _same(_mask(plane, rot=np.pi / 2), want)
    want = np.zeros_like(plane)
    for y in range(1, H):
        want[y, :] = plane[:, 180 - y]
    assert _same(_mask(plane, rot=-np.pi / 2), want)
    assert _same(np.ascontiguousarray(_mask(plane, scale=2.0)[0::2, 0::2]), np.ascontiguousarray(plane[45:135, 45:135]))


def test_warp_stays_close_to_exact_bilinear(plane):
    """the fixed-point coordinates (1/32 pixel) against float64 bilinear interpolation of the same inverse map: on a [0, 1] map the two
    differ by at most the map's slope times the coordinate error -- two coordinates, each off by at most 1/64 + 2^-10 pixel -- plus fp32
    rounding: 2 x (1/64 + 1/1024) + 1e-6 < 0.034"""
    for rot, scale in ((0.3, 0.9), (-0.78539816, 1.1)):
        m = am.invert(am.rotation_matrix(90, 90, np.degrees(-rot), scale))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        sx, sy = m[0] * xx + m[1] * yy + m[2], m[3] * xx + m[4] * yy + m[5]
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = sx - x0, sy - y0

        def tap(y, x):
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            return np.where(ok, plane[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.float64), 0.0)

        exact = tap(y0, x0) * (1 - fy) * (1 - fx) + tap(y0, x0 + 1) * (1 - fy) * fx + tap(y0 + 1, x0) * fy * (1 - fx) + tap(y0 + 1, x0 + 1) * fy * fx
        err = float(np.abs(am.warp(plane, m) - exact).max())
        print("[augment_map] rot %.3f scale %.2f: fixed point vs exact bilinear max %.4g" % (rot, scale, err))
        assert err < 2 * (1 / 64 + 1 / 1024) + 1e-6


# ---- the range filter: the restatement against the reference's masks
def _golden_cases(golden):
    g = golden("range_filter.npz")
    for name in [str(n) for n in g["names"]]:
        yield name, g["%s/boxes" % name], g["%s/range" % name], g["%s/masks" % name]


def test_range_filter_golden_covers_what_the_issue_asks(golden):
    g = golden("range_filter.npz")
    cases = {n: (b, r, m) for n, b, r, m in _golden_cases(golden)}
    assert {"edges", "corners", "big", "small", "asym", "exact"} <= set(cases) and float(g["margin"]) == 1e-3
    centre_in_dropped = centre_out_kept = 0
    for name, (b, r, m) in cases.items():
        assert b.dtype == np.float32 and b.shape[2] == 12 and r.dtype == np.float32 and m.dtype == np.bool_ and m.shape == b.shape[:2]
        assert (m == m[0]).all()  # the mask of timestep 0, for every timestep
        first = b[0].astype(np.float64)
        cin = (first[:, 0] > r[0]) & (first[:, 0] < r[2]) & (first[:, 1] > r[1]) & (first[:, 1] < r[3])
        centre_in_dropped += int((cin & ~m[0]).sum())
        centre_out_kept += int((~cin & m[0]).sum())
        if name != "exact":  # every corner of every box keeps the margin from every boundary line: nothing is decided by rounding
            c = rf.corners(first.astype(np.float32)).astype(np.float64)
            d = np.concatenate([np.abs(c[..., 0] - r[0]), np.abs(c[..., 0] - r[2]), np.abs(c[..., 1] - r[1]), np.abs(c[..., 1] - r[3])])
            assert d.min() >= 1e-3 - 1e-5, (name, d.min())
            assert 0 < m[0].sum() < m.shape[1] or name == "big", name
    assert centre_in_dropped >= 10 and centre_out_kept >= 10
    # around all four edges and all four corners of the range: kept and dropped boxes in each of the eight regions
    b, r, m = cases["edges"]
    x, y = b[0, :, 0], b[0, :, 1]
    for sel in (np.abs(x - r[0]) < 6.5, np.abs(x - r[2]) < 6.5, np.abs(y - r[1]) < 6.5, np.abs(y - r[3]) < 6.5):
        assert m[0][sel].any() and (~m[0][sel]).any()
    b, r, m = cases["corners"]
    x, y = b[0, :, 0], b[0, :, 1]
    for sx in (x < 0, x > 0):
        for sy in (y < 0, y > 0):
            assert m[0][sx & sy].any() and (~m[0][sx & sy]).any()


def test_range_filter_restatement_reproduces_every_mask(golden):
    for name, b, r, m in _golden_cases(golden):
        assert np.array_equal(rf.mask(b[0], r), m[0]), name


def test_range_filter_boundary_is_strict(golden):
    """the hand-written cases: per side a box with two corners ON the line and the rest beyond (dropped), one wholly beyond (dropped), one
    straddling (kept), one with two corners on the line and two inside (kept); then the range's own corner"""
    _, b, r, m = next(c for c in _golden_cases(golden) if c[0] == "exact")
    assert m[0].astype(int).tolist() == [0, 0, 1, 1] * 4 + [0, 1, 1]
    assert (b[0, :, 11] == 0).all() and (b[0, :, 10] != 0).all()  # the angle is the LAST column
    c = rf.corners(b[0])
    on_line = (c[..., 0] == r[0]) | (c[..., 0] == r[2]) | (c[..., 1] == r[1]) | (c[..., 1] == r[3])
    assert on_line[0::4][:4].any(axis=1).all() and not rf.inside(c[0], r).any()


def test_range_filter_restatement_compacts_every_timestep():
    r = np.random.default_rng(3)
    boxes = r.uniform(-60, 60, (2, 3, 9, 12)).astype(np.float32)
    boxes[..., 3:5] = 2.0
    counts = np.array([[9, 9, 9], [5, 7, 3]], np.int32)
    classes = r.integers(1, 10, (2, 3, 9)).astype(np.int32)
    traj = r.integers(0, 3, (2, 3, 9)).astype(np.int32)
    ob, oc, ok, ot, status = rf.apply(boxes, counts, classes, traj, (-54, -54, 54, 54))
    assert status.tolist() == [0, 2]
    keep0 = rf.mask(boxes[0, 0], (-54, -54, 54, 54))
    assert 0 < keep0.sum() < 9 and (oc[0] == keep0.sum()).all()
    for t in range(3):
        assert np.array_equal(ob[0, t, :oc[0, t]], boxes[0, t][keep0]) and not ob[0, t, oc[0, t]:].any() and not ok[0, t, oc[0, t]:].any()
        assert np.array_equal(ot[0, t, :oc[0, t]], traj[0, t][keep0])
    keep1 = rf.mask(boxes[1, 0, :5], (-54, -54, 54, 54))
    assert oc[1].tolist() == [keep1.sum(), keep1.sum(), keep1[:3].sum()]  # rows at or past counts[b, 0] are dropped


# ---- the C surface
def test_symbols_header_build_flags_and_mirrors(L, tmp_path):
    from futuredet_amd.augment import MASK_RECORD_DTYPE, RECORD_DTYPE

    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fd_[a-z0-9_]+)", nm))
    for name in NAMES:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, bare)
        assert m, name
        assert name in lib.SIGNATURES and name in exported, name
        assert len(m.group(1).split(",")) == len(lib.SIGNATURES[name][1]), name
    assert L.fd_abi_version() == 8 == lib.ABI_VERSION  # purely additive
    assert "fd_augment_map.hip" in build.SOURCES and build.EXTRA["fd_augment_map.hip"] == build.EXTRA["fd_augment.hip"]
    assert "-ffp-contract=off" in build.EXTRA["fd_augment_map.hip"]  # no contraction to fused multiply-adds
    src = tmp_path / "rec.c"
    fields = [n for n, _ in lib.AugmentMaskRecord._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "futuredet_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu", sizeof(fd_augment_mask_record), sizeof(fd_augment_record));\n'
                   + "".join('printf(" %%zu", offsetof(fd_augment_mask_record, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "rec")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got[0] == ctypes.sizeof(lib.AugmentMaskRecord) == MASK_RECORD_DTYPE.itemsize == 104 == 8 * hip_ops.AUGMENT_MASK_RECORD_DOUBLES
    assert got[1] == 48 == RECORD_DTYPE.itemsize == 8 * hip_ops.AUGMENT_RECORD_DOUBLES  # the earlier record has not changed
    assert got[2:] == [getattr(lib.AugmentMaskRecord, f).offset for f in fields] == [MASK_RECORD_DTYPE.fields[f][1] for f in fields]
    assert list(MASK_RECORD_DTYPE.names) == fields == ["flip_a", "flip_b", "m1", "m2"]
    assert MASK_RECORD_DTYPE.fields["m1"][0].shape == (6,) and lib.AugmentMaskRecord.m2.size == 48


def _define(name):
    hdr = open(os.path.join(REPO, "include", "futuredet_hip.h")).read()
    return re.search(r"#define %s (\S+)" % name, hdr).group(1)


def test_range_filter_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work"""
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(9)]
    odd4, odd2 = ctypes.c_void_p(0x100004), ctypes.c_void_p(0x100002)
    max_n = int(_define("FD_RANGE_FILTER_MAX_N"))
    assert max_n >= 500  # what the shipped assigners take (max_objs = 500)

    def call(**kw):
        a = dict(boxes=p[0], counts=p[1], classes=p[2], traj=p[3], rng=(-54.0, -54.0, 54.0, 54.0), boxes_out=p[4], counts_out=p[5],
                 classes_out=p[6], traj_out=p[7], status=p[8], B=2, T=3, n=5)
        a.update(kw)
        return L.fd_gt_range_filter(a["boxes"], a["counts"], a["classes"], a["traj"], *a["rng"], a["boxes_out"], a["counts_out"], a["classes_out"],
                                    a["traj_out"], a["status"], a["B"], a["T"], a["n"], None)

    def bad(text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())

    bad("must be >= 1", B=0)
    bad("must be >= 1", T=0)
    bad("n_max", n=0)
    bad("n_max", n=max_n + 1)
    bad("rows, at most", B=1 << 14, T=1 << 14, n=2)
    for rng in ((-54.0, -54.0, -54.0, 54.0), (-54.0, 54.0, 54.0, -54.0), (float("nan"), -54.0, 54.0, 54.0), (-54.0, -54.0, float("inf"), 54.0)):
        bad("range", rng=rng)
    for k in ("boxes", "counts", "classes", "boxes_out", "counts_out", "classes_out", "status"):
        bad("null", **{k: None})
    bad("needs trajectory_out", traj_out=None)
    bad("16-byte aligned", boxes=odd4)
    bad("16-byte aligned", boxes_out=odd4)
    for k in ("counts", "classes", "traj", "counts_out", "classes_out", "traj_out", "status"):
        bad("4-byte aligned", **{k: odd2})
    bad("not overlap", boxes_out=ctypes.c_void_p(0x100000 + 48))
    bad("not overlap", counts_out=ctypes.c_void_p(0x200000 + 4))
    bad("not overlap", classes_out=ctypes.c_void_p(0x300000 + 4))
    bad("not overlap", traj_out=ctypes.c_void_p(0x400000 + 4))


def test_augment_mask_invalid_arguments_are_einval_without_a_device(L):
    p, q, odd2, odd4 = (ctypes.c_void_p(v) for v in (0x100000, 0x900000, 0x100002, 0x100004))
    max_pixels = int(_define("FD_AUGMENT_MASK_MAX_PIXELS"))
    assert max_pixels * 4 <= 160 * 1024 and max_pixels >= H * W  # the plane is staged in LDS

    def call(**kw):
        a = dict(src=p, recs=p, dst=q, B=2, C=6, H=H, W=W)
        a.update(kw)
        return L.fd_augment_mask(a["src"], a["recs"], a["dst"], a["B"], a["C"], a["H"], a["W"], None)

    def bad(text, **kw):
        assert call(**kw) == -1 and text in L.fd_last_error().decode(), (kw, text, L.fd_last_error().decode())

    for k in ("B", "C", "H", "W"):
        bad("must be >= 1", **{k: 0})
    bad("does not fit LDS", H=1, W=max_pixels + 1)
    bad("does not fit LDS", H=203, W=203)
    bad("elements, at most", B=1 << 10, C=1 << 10, H=H, W=W)
    bad("records must be non-null and 8-byte aligned", recs=None)
    bad("records must be non-null and 8-byte aligned", recs=odd4)
    bad("non-null and 4-byte aligned", src=None)
    bad("non-null and 4-byte aligned", dst=None)
    bad("non-null and 4-byte aligned", src=odd2)
    bad("distinct buffers", dst=p)  # dst == src
    bad("distinct buffers", dst=ctypes.c_void_p(0x100000 + 2 * 6 * H * W * 4 - 4))


def test_augment_mask_check_refuses_coordinates_out_of_range(L):
    from futuredet_amd.augment import MASK_RECORD_DTYPE

    limit = float(_define("FD_AUGMENT_MASK_MAX_COORD"))
    assert limit * 1024 + 17 < 2 ** 31 and limit < 2 ** 15  # the fixed-point sums stay in int32, sx / sy in int16
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def check(m1=ident, m2=ident, h=H, w=W, n=1):
        rec = np.zeros((n,), MASK_RECORD_DTYPE)
        rec["m1"], rec["m2"] = ident, ident
        rec["m1"][-1], rec["m2"][-1] = m1, m2
        return L.fd_augment_mask_check(ctypes.c_void_p(rec.ctypes.data), n, h, w)

    assert check() == 0 and check(m2=[1, 0, -400.0, 0, 1, 0]) == 0
    assert check(m1=[1, 0, limit - 179.5, 0, 1, 0]) == 0
    for kw in (dict(m1=[1, 0, limit - 179.0, 0, 1, 0]), dict(m2=[1, 0, 0, 0, 1, -limit]), dict(m1=[200.0, 0, 0, 0, 1, 0]),
               dict(m2=[1, 0, 0, 0, 200.0, 0]), dict(m1=[1, float("nan"), 0, 0, 1, 0]), dict(m2=[1, 0, 0, float("inf"), 1, 0]),
               dict(m1=[1, 0, limit, 0, 1, 0], n=3)):
        assert check(**kw) == -1 and "fixed-point" in L.fd_last_error().decode(), kw
    assert L.fd_augment_mask_check(None, 1, H, W) == -1 and check(h=0) == -1 and check(w=0) == -1 and L.fd_augment_mask_check(ctypes.c_void_p(8), 0, H, W) == -1
    with pytest.raises(hip_ops.FutureDetHipError, match="mask records"):
        hip_ops.augment_mask_check(np.zeros((2, 13)), H, W)


def test_front_end_argument_checks():
    """CPU tensors raise the project's error (dtype, contiguity and shape refusals: test_gpu_augment_map.py)"""
    E = hip_ops.FutureDetHipError
    with pytest.raises(E, match="HIP device"):
        hip_ops.augment_mask(torch.zeros(1, 1, H, W), torch.zeros((1, 13), dtype=torch.float64))
    with pytest.raises(E, match="HIP device"):
        hip_ops.gt_range_filter(torch.zeros(1, 1, 2, 12), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1, 2), dtype=torch.int32),
                                (-54, -54, 54, 54))


# ---- augment.py
def test_mask_record_against_closed_forms():
    from futuredet_amd.augment import MASK_RECORD_DTYPE, GlobalAugment, identity_params

    rec = GlobalAugment.mask_record(identity_params(2))
    assert rec.dtype == MASK_RECORD_DTYPE and rec.shape == (2,)
    assert (rec["m1"] == [1, 0, 0, 0, 1, 0]).all() and (rec["m2"] == [1, 0, 0, 0, 1, 0]).all() and not rec["flip_a"].any()
    # a translation by (tx, ty) pixels, rounded to fp32 first; tz is unused: the inverse moves back
    rec = GlobalAugment.mask_record(np.array([[1, 0, 0.0, 1.0, 3.0, -2.0, 9.0], [0, 1, 0.0, 1.0, 0.1, 0.5, -9.0]]))
    assert rec["flip_a"].tolist() == [1, 0] and rec["flip_b"].tolist() == [0, 1]
    assert rec["m2"][0].tolist() == [1, 0, -3.0, 0, 1, 2.0] and rec["m2"][1].tolist() == [1, 0, -float(np.float32(0.1)), 0, 1, -0.5]
    assert (rec["m1"] == [1, 0, 0, 0, 1, 0]).all()
    # scale 2 about (90, 90): the inverse is x / 2 + 45
    rec = GlobalAugment.mask_record(np.array([[0, 0, 0.0, 2.0, 0, 0, 0]]))
    assert rec["m1"][0].tolist() == [0.5, 0, 45.0, 0, 0.5, 45.0]
    # a rotation by rot: forward [[a, b, .], [-b, a, .]] with a = cos(-rot) s, b = sin(-rot) s; the inverse is its transpose / s^2 and
    # keeps (90, 90) fixed
    rot, s = 0.3, 1.1
    m = GlobalAugment.mask_record(np.array([[0, 0, rot, s, 0, 0, 0]]))["m1"][0]
    a, b = np.cos(-rot) / s, np.sin(-rot) / s
    assert np.allclose(m[[0, 1, 3, 4]], [a, -b, b, a], rtol=1e-14, atol=0)
    assert np.allclose([m[0] * 90 + m[1] * 90 + m[2], m[3] * 90 + m[4] * 90 + m[5]], [90, 90], rtol=1e-13)
    # the restatement builds the same matrices, bit for bit
    for p in ([1, 0, 0.3, 1.1, -1.37, 2.81, 0.3], [0, 1, -0.78539816, 0.9, 400.0, 0.0, 0.0], [0, 0, np.pi / 2, 1.0, 0.5, 0.0, 0.0]):
        r = GlobalAugment.mask_record(np.array([p]))
        fa, fb, m1, m2 = am.matrices(p)
        assert r["m1"][0].tobytes() == m1.tobytes() and r["m2"][0].tobytes() == m2.tobytes() and (r["flip_a"][0], r["flip_b"][0]) == (fa, fb)
    t = GlobalAugment.mask_record(np.array([[1, 0, 0.3, 1.1, -1.37, 2.81, 0.3]]), device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (1, 13)
    mirror = lib.AugmentMaskRecord.from_buffer_copy(t.numpy().tobytes())
    assert mirror.flip_a == 1 and mirror.flip_b == 0 and list(mirror.m2) == [1, 0, -float(np.float32(-1.37)), 0, 1, -float(np.float32(2.81))]
    with pytest.raises(ValueError, match="finite"):
        GlobalAugment.mask_record(np.array([[0, 0, np.nan, 1, 0, 0, 0]]))
    with pytest.raises(ValueError, match="fixed-point"):
        GlobalAugment.mask_record(np.array([[0, 0, 0.0, 1.0, 1e6, 0, 0]]))
    with pytest.raises(ValueError, match="fixed-point"):
        GlobalAugment.mask_record(np.array([[0, 0, 0.0, 1e-3, 0, 0, 0]]))


def test_no_translation_std_means_no_shift():
    """with every translate std 0 the reference's global_translate_ returns a 2-tuple and get_mask fails; here that case is t = (0, 0)"""
    from futuredet_amd.augment import GlobalAugment

    aug = GlobalAugment(dict(CFG, global_translate_std=0), seed=1, warp_bev=True)
    rec = aug.mask_record(aug.draw(8))
    assert (rec["m2"] == [1, 0, 0, 0, 1, 0]).all()


def test_map_size_refusal():
    from futuredet_amd.augment import BEV_SIZE, GlobalAugment, check_bev_size

    assert BEV_SIZE == 180 and GlobalAugment(CFG).warp_bev is False and GlobalAugment(CFG, 0, True).warp_bev is True
    assert inspect.signature(GlobalAugment.__init__).parameters["warp_bev"].default is False
    check_bev_size(torch.zeros((2, 6, 180, 180)))
    aug = GlobalAugment(CFG, seed=0, warp_bev=True)
    for shape in ((2, 6, 128, 128), (2, 6, 180, 176), (6, 180, 180)):
        with pytest.raises(ValueError, match="180 x 180"):
            aug.warp_map(torch.zeros(shape), np.zeros((2, 7)))


@pytest.mark.parametrize("cls", ["StaticTrainStep", "StaticPillarsTrainStep"])
def test_step_keywords_and_the_bare_step_draws_with_warp_bev(cls):
    """the bare-object step of test_augment_host.py::test_bev_head_without_params_is_refused: with warp_bev the step draws instead of
    raising; without it the refusal and its text are the earlier ones"""
    from futuredet_amd.augment import GlobalAugment

    klass = getattr(solver, cls)
    params = inspect.signature(klass.__init__).parameters
    assert params["filter_gt"].default is False and params["augment"].default is None
    step = object.__new__(klass)
    step.B, step.bev, step.augment = 2, torch.zeros((2, 6, 4, 4)), GlobalAugment(CFG, seed=0, warp_bev=True)
    batch = dict(clouds=[torch.zeros((3, 5)), torch.zeros((4, 5))], bev_map=torch.zeros((2, 6, 4, 4)))
    drawn = step._aug_params(batch)
    assert drawn.shape == (2, 7) and np.array_equal(drawn, GlobalAugment(CFG, seed=0).draw(2))
    given = np.arange(14.0).reshape(2, 7)
    assert np.array_equal(step._aug_params(dict(batch, aug_params=given)), given)
    step.augment = GlobalAugment(CFG, seed=0)
    with pytest.raises(ValueError, match="aug_params.*already warped"):
        step._aug_params(batch)


def test_bev_range_takes_the_voxel_range():
    from futuredet_amd.augment import bev_range

    assert bev_range([-54, -54, -5.0, 54, 54, 3.0]) == [-54.0, -54.0, 54.0, 54.0] == bev_range((-54, -54, 54, 54))
    assert bev_range([-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]) == [float(np.float32(v)) for v in (-51.2, -51.2, 51.2, 51.2)]
    with pytest.raises(ValueError):
        bev_range([0, 1, 2])
