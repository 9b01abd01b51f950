"""The host side of the global augmentation (csrc/fd_augment.hip, futuredet_amd/augment.py, the ``augment`` keyword of the static steps):
the numpy restatement of the kernels' arithmetic (tests/augment_ref.py) against the reference's recorded outputs
(tests/golden/augment.npz), the shuffle's permutation, exported symbols, argument checks (no device needed: they come before any device
work), GlobalAugment's refusals and draws, and the steps' refusal of a bev_map head without parameters.  CPU only.

The bound between the restatement and the reference.  Everything but the rotation is the same sequence of single IEEE operations on both
sides (negation, fp32 products with an fp32 scalar, an fp32 sum with fl32(pi) / fl32(2 pi) / fl32(rot), a float64 sum rounded once), so
with rot = 0 (c = 1, s = 0: products and sums are exact) every entry is equal.  The rotation is x c + y s: three roundings in the
kernels, <= 2 u (|x| + |y|) off the exact value (u = 2^-24); the reference's BLAS product may fuse it, and rotates the velocity pairs
through a float64 copy, both <= 2 u (|x| + |y|) as well (measured on 100 000 points: both forms within 1.5 u (|x| + |y|) of float64,
27-30 % of the entries differing in the last bit).  Scale and shift add one rounding each on values the size of the result.  Hence
|kernel - reference| <= 4 u M, M = scale (|x| + |y|) + |t| + |result|; the golden itself is asserted to lie within that bound of a
float64 evaluation, so the bound is not vacuous on either side."""
import ctypes
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

import augment_ref as ar  # noqa: E402
from futuredet_amd import build, hip_ops, lib, solver  # noqa: E402

NAMES = {"fd_augment_points", "fd_augment_boxes"}
CFG = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
           db_sampler=dict(enable=False), class_names=["car"])


@pytest.fixture(scope="module")
def L():
    build.build()
    return lib.load()


def _cases(golden):
    g = golden("augment.npz")
    for name in [str(n) for n in g["names"]]:
        c = {k: g["%s/%s" % (name, k)] for k in ("points_in", "boxes_in", "flips", "rot", "scale", "trans", "points_out", "boxes_out")}
        c["params"] = np.array([c["flips"][0], c["flips"][1], c["rot"], c["scale"], *c["trans"]], np.float64)
        yield name, c


def test_golden_covers_what_the_issue_asks(golden):
    cs = dict(_cases(golden))
    assert len(cs) >= 6 and str(golden("augment.npz")["numpy_version"]).startswith("2.")
    assert {tuple(int(v) for v in c["flips"]) for c in cs.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sum(float(c["rot"]) == 0.0 for c in cs.values()) == 1 and any(abs(float(c["rot"])) > 0.5 for c in cs.values())
    for c in cs.values():
        assert c["points_in"].shape == (257, 5) and c["boxes_in"].shape == (3, 5, 12) and c["points_out"].dtype == np.float32


def test_restatement_against_the_golden(golden):
    for name, c in _cases(golden):
        p, t = c["params"], c["trans"]
        pts = ar.points(c["points_in"], p)
        b_in, b_ref = c["boxes_in"].reshape(-1, 12), c["boxes_out"].reshape(-1, 12)
        boxes = ar.box_rows(b_in, p)
        # not rotated: z, intensity, time; box z, sizes and the two angles -- every bit
        assert np.array_equal(pts[:, 2:].view(np.int32), c["points_out"][:, 2:].view(np.int32)), name
        assert np.array_equal(boxes[:, [2, 3, 4, 5, 10, 11]].view(np.int32), b_ref[:, [2, 3, 4, 5, 10, 11]].view(np.int32)), name
        pairs = [("points", pts[:, 0:2], c["points_out"][:, 0:2], c["points_in"][:, 0:2], t[:2])]
        pairs += [("boxes %d,%d" % (i, j), boxes[:, [i, j]], b_ref[:, [i, j]], b_in[:, [i, j]], t[:2] if i == 0 else (0.0, 0.0))
                  for i, j in ar.PAIRS]
        for what, got, ref, xy, txy in pairs:
            bound = ar.bound(xy, ref, p, txy)
            f64 = ar.exact(xy, p, txy)
            err_ref = np.abs(ref.astype(np.float64) - f64)
            assert (err_ref <= bound).all(), ("the golden against float64", name, what, float((err_ref / bound).max()))
            err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            print("[augment] %s %s: restatement vs golden max %.3g of the bound, %d of %d entries differ; golden vs float64 max %.3g"
                  % (name, what, float((err / bound).max()), int((got != ref).sum()), got.size, float((err_ref / bound).max())))
            if float(c["rot"]) == 0.0:
                assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (name, what)
            assert (err <= bound).all(), (name, what, float((err / bound).max()))


def test_boxes_restatement_honours_counts():
    r = np.random.default_rng(0)
    b = r.normal(0, 5, (2, 3, 5, 12)).astype(np.float32)
    counts = np.array([[0, 3, 5], [5, 0, 3]], np.int32)
    params = np.array([[1, 0, 0.3, 1.05, 0.1, -0.2, 0.3], [0, 1, -0.2, 0.95, 0.0, 0.4, -0.1]])
    out = ar.boxes(b, counts, params)
    for bi in range(2):
        for ti in range(3):
            n = counts[bi, ti]
            assert np.array_equal(out[bi, ti, n:], b[bi, ti, n:]) and np.array_equal(out[bi, ti, :n], ar.box_rows(b[bi, ti, :n], params[bi]))
            assert n == 0 or not np.array_equal(out[bi, ti, :n], b[bi, ti, :n])


@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_reference_permutation_is_the_reference_shuffle(n):
    from futuredet_amd.augment import reference_permutation

    perm = reference_permutation(n)
    assert perm.dtype == np.int32 and perm.shape == (n,) and sorted(perm.tolist()) == list(range(n))
    pts = np.arange(n * 5, dtype=np.float32).reshape(n, 5)
    shuffled = pts.copy()
    np.random.default_rng(0).shuffle(shuffled)  # preprocess.py:201-203
    assert np.array_equal(shuffled, pts[perm])
    assert reference_permutation(n) is perm and not perm.flags.writeable  # the cache hands the same read-only array back


def test_symbols_header_build_flags_and_abi(L, tmp_path):
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
    assert "fd_augment.hip" in build.SOURCES
    assert build.EXTRA["fd_augment.hip"] == build.EXTRA["fd_loss.hip"] == build.EXTRA["fd_rows.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    # the record: the header's struct, the ctypes mirror and the numpy dtype agree
    from futuredet_amd.augment import RECORD_DTYPE

    src = tmp_path / "rec.c"
    fields = [n for n, _ in lib.AugmentRecord._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "futuredet_hip.h"\nint main(void) { printf("%zu", sizeof(fd_augment_record));\n'
                   + "".join('printf(" %%zu", offsetof(fd_augment_record, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "rec")
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert got[0] == ctypes.sizeof(lib.AugmentRecord) == RECORD_DTYPE.itemsize == 48 == 8 * hip_ops.AUGMENT_RECORD_DOUBLES
    assert got[1:] == [getattr(lib.AugmentRecord, f).offset for f in fields] == [RECORD_DTYPE.fields[f][1] for f in fields]
    assert list(RECORD_DTYPE.names) == fields


def test_invalid_arguments_are_einval_without_a_device(L):
    """pointers that are never dereferenced: every call fails validation before any device work; n_rows = 0 and n_max = 0 are no-ops"""
    p, q, odd4, odd8 = (ctypes.c_void_p(v) for v in (0x10000, 0x900000, 0x10004, 0x10008))
    max_rows = int(re.search(r"#define FD_AUGMENT_MAX_ROWS \(1 << (\d+)\)", open(os.path.join(REPO, "include", "futuredet_hip.h")).read()).group(1))
    max_rows = 1 << max_rows

    def err():
        return L.fd_last_error().decode()

    def points(**kw):
        a = dict(src=p, n=100, ndim=5, perm=None, rec=p, dst=q)
        a.update(kw)
        return L.fd_augment_points(a["src"], a["n"], a["ndim"], a["perm"], a["rec"], a["dst"], None)

    def bad(text, **kw):
        assert points(**kw) == -1 and text in err(), (kw, text, err())

    for ndim in (0, 3, 6):
        bad("ndim must be 4 or 5", ndim=ndim)
    bad("n_rows", n=-1)
    bad("n_rows", n=max_rows + 1)
    bad("record must be non-null and 8-byte aligned", rec=None)
    bad("record must be non-null and 8-byte aligned", rec=odd4)
    bad("null src or dst", src=None)
    bad("null src or dst", dst=None)
    bad("distinct buffers", dst=p)
    bad("distinct buffers", dst=ctypes.c_void_p(0x10000 + 100 * 20 - 4))  # the last float of src
    bad("4-byte aligned", src=ctypes.c_void_p(0x10002))
    assert points(n=0, src=None, dst=None) == 0 and points(n=0, src=p, dst=p) == 0

    def boxes(**kw):
        a = dict(boxes=p, counts=p, recs=p, out=q, B=2, T=3, n=5)
        a.update(kw)
        return L.fd_augment_boxes(a["boxes"], a["counts"], a["recs"], a["out"], a["B"], a["T"], a["n"], None)

    def badb(text, **kw):
        assert boxes(**kw) == -1 and text in err(), (kw, text, err())

    badb("must be >= 1", B=0)
    badb("must be >= 1", T=0)
    badb("must be >= 1", n=-1)
    badb("rows, at most", B=1 << 15, T=1 << 15, n=1)
    badb("records must be non-null and 8-byte aligned", recs=None)
    badb("records must be non-null and 8-byte aligned", recs=odd4)
    badb("null boxes, out or counts", boxes=None)
    badb("null boxes, out or counts", out=None)
    badb("null boxes, out or counts", counts=None)
    badb("16-byte aligned", boxes=odd8)
    badb("16-byte aligned", out=odd8)
    badb("not overlap", out=ctypes.c_void_p(0x10000 + 48))
    assert boxes(n=0, boxes=None, out=None, counts=None) == 0


def test_front_end_argument_checks():
    """CPU tensors raise the project's error (dtype, contiguity and shape refusals: test_gpu_augment.py)"""
    E = hip_ops.FutureDetHipError
    with pytest.raises(E, match="HIP device"):
        hip_ops.augment_points(torch.zeros(4, 5), torch.zeros(6, dtype=torch.float64), torch.zeros(4, 5))
    with pytest.raises(E, match="HIP device"):
        hip_ops.augment_boxes(torch.zeros(1, 1, 2, 12), torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 6), dtype=torch.float64))


def test_global_augment_refusals():
    from futuredet_amd.augment import GlobalAugment

    GlobalAugment(CFG)
    GlobalAugment(dict(CFG, db_sampler=None))
    with pytest.raises(NotImplementedError, match="db_sampler"):
        GlobalAugment(dict(CFG, db_sampler=dict(enable=True, type="GT-AUG")))
    with pytest.raises(NotImplementedError, match="db_sampler"):
        GlobalAugment(dict(CFG, db_sampler=dict(type="GT-AUG")))
    with pytest.raises(NotImplementedError, match="min_points_in_gt"):
        GlobalAugment(dict(CFG, min_points_in_gt=5))
    with pytest.raises(NotImplementedError, match="npoints"):
        GlobalAugment(dict(CFG, npoints=20000))
    GlobalAugment(dict(CFG, min_points_in_gt=-1, npoints=-1))
    with pytest.raises(ValueError):
        GlobalAugment.record(np.array([[0, 0, np.nan, 1, 0, 0, 0]]))


def test_shipped_train_preprocessor_is_accepted():
    """the train_preprocessor every configs/centerpoint/*.py writes: a full db_sampler description with enable=False, no point filter"""
    from futuredet_amd.augment import GlobalAugment
    from futuredet_amd.config import ConfigDict

    db = dict(type="GT-AUG", enable=False, db_info_path="dbinfos_train.pkl", sample_groups=[dict(car=2)],
              db_prep_steps=[dict(filter_by_min_num_points=dict(car=5))], global_random_rotation_range_per_object=[0, 0], rate=1.0)
    tp = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.785, 0.785], global_scale_noise=[0.9, 1.1], global_translate_std=0.5,
              db_sampler=db, class_names=["car"], sampler_type="standard")
    for cfg in (tp, ConfigDict(tp)):
        aug = GlobalAugment(cfg, seed=0)
        assert aug.shuffle_points and not aug.identity
        assert aug.rot_noise == [-0.785, 0.785] and aug.scale_noise == [0.9, 1.1] and aug.translate_std == [0.5, 0.5, 0.5]


def test_draw_ranges_order_and_the_z_quirk():
    from futuredet_amd.augment import PARAM_FIELDS, GlobalAugment, identity_params

    assert PARAM_FIELDS == ("flip_a", "flip_b", "rot", "scale", "tx", "ty", "tz")
    aug = GlobalAugment(CFG, seed=5)
    d = np.concatenate([aug.draw(64) for _ in range(32)])
    assert d.shape == (2048, 7) and d.dtype == np.float64
    assert set(np.unique(d[:, :2])) == {0.0, 1.0} and 0.4 < d[:, 0].mean() < 0.6 and 0.4 < d[:, 1].mean() < 0.6
    assert d[:, 2].min() >= -0.785 and d[:, 2].max() < 0.785 and d[:, 2].std() > 0.4
    assert d[:, 3].min() >= 0.9 and d[:, 3].max() < 1.1
    assert np.allclose(d[:, 4:].std(0), 0.5, atol=0.05) and np.allclose(d[:, 4:].mean(0), 0.0, atol=0.05)
    # the same seed gives the same draws; the order within a sample is the reference's: flips, rot, scale, tx, ty, tz
    a, b = GlobalAugment(CFG, seed=9).draw(3), GlobalAugment(CFG, seed=9).draw(3)
    assert np.array_equal(a, b)
    r = np.random.default_rng(9)
    first = [float(r.random() < 0.5), float(r.random() < 0.5), r.uniform(-0.785, 0.785), r.uniform(0.9, 1.1), r.normal(0, 0.5), r.normal(0, 0.5),
             r.normal(0, 0.5)]
    assert a[0].tolist() == first
    # z is drawn with std[0] (global_translate_'s third draw): y alone follows std[1]
    q = GlobalAugment(dict(CFG, global_translate_std=[2.0, 0.0, 100.0]), seed=1).draw(512)
    assert abs(q[:, 4].std() - 2.0) < 0.3 and (q[:, 5] == 0).all() and abs(q[:, 6].std() - 2.0) < 0.3
    # a scalar angle is a symmetric range; no translation at all draws no normals
    s = GlobalAugment(dict(CFG, global_rot_noise=0.3, global_translate_std=0), seed=1).draw(256)
    assert np.abs(s[:, 2]).max() <= 0.3 and (s[:, 2] < 0).any() and (s[:, 4:] == 0).all()
    # the identity modes: only the shuffle remains
    for kw in (dict(no_augmentation=True), dict(mode="val")):
        g = GlobalAugment(dict(CFG, **kw), seed=1)
        assert np.array_equal(g.draw(4), identity_params(4)) and g.shuffle_points
    assert GlobalAugment(dict(CFG, shuffle_points=False)).permutation(10, "cpu") is None


def test_record_layout():
    from futuredet_amd.augment import RECORD_DTYPE, GlobalAugment

    p = np.array([[1, 0, 0.5, 1.05, 0.25, -0.5, 0.125], [0, 1, -0.785, 0.9, 0.0, 0.0, 0.0]])
    rec = GlobalAugment.record(p)
    assert rec.dtype == RECORD_DTYPE and rec.shape == (2,)
    assert rec["flip_a"].tolist() == [1, 0] and rec["flip_b"].tolist() == [0, 1]
    assert rec["c"][0] == np.float32(np.cos(0.5)) and rec["s"][1] == np.float32(np.sin(-0.785)) and rec["rot"][1] == np.float32(-0.785)
    assert rec["scale"][0] == np.float32(1.05) and rec["tx"][0] == 0.25 and rec["ty"][0] == -0.5 and rec["tz"][0] == 0.125
    t = GlobalAugment.record(p, device="cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (2, 6) and t.numpy().tobytes() == rec.tobytes()
    mirror = lib.AugmentRecord.from_buffer_copy(rec[0].tobytes())
    assert (mirror.flip_a, mirror.flip_b, mirror.tz) == (1, 0, 0.125) and mirror.c == float(np.float32(np.cos(0.5)))


@pytest.mark.parametrize("cls", ["StaticTrainStep", "StaticPillarsTrainStep"])
def test_bev_head_without_params_is_refused(cls):
    """the map warp is not built: with a bev_map head the batch must bring aug_params and a map warped with them.  The refusal comes
    before any device work, so a bare object with the fields _load reads is enough."""
    import inspect

    from futuredet_amd.augment import GlobalAugment

    klass = getattr(solver, cls)
    assert inspect.signature(klass.__init__).parameters["augment"].default is None
    step = object.__new__(klass)
    step.B, step.bev, step.augment = 2, torch.zeros((2, 6, 4, 4)), GlobalAugment(CFG, seed=0)
    batch = dict(clouds=[torch.zeros((3, 5)), torch.zeros((4, 5))], bev_map=torch.zeros((2, 6, 4, 4)))
    with pytest.raises(ValueError, match="aug_params.*already warped"):
        step._load(batch, 0)
    with pytest.raises(ValueError, match=r"expected \[2, 7\]"):
        step._load(dict(batch, aug_params=np.zeros((1, 7))), 0)
    step.bev = None  # no map head: the step draws for itself
    assert step._aug_params(batch).shape == (2, 7)
