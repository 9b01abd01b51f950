"""-m gpu: the rotated BEV IoU on degenerate geometry (tests/golden/iou_edges.npz, values of the compiled reference) and the greedy NMS sweeps
-- nms_sweep, nms_sweep_tail, and the unfused nms_sweep + dec_gather + assemble_kernel path -- on suppression patterns whose answer is known
exactly (nms_edge_cases.py; test_nms_edges_host.py proves the expected lists with the host oracle)."""
import numpy as np
import pytest
import torch

import nms_edge_cases as nec
from parity_util import nms_layout, report

pytestmark = pytest.mark.gpu

H, W = 40, 128  # 5120 cells: more than nms_pre_max_size 4096, so the candidate cut is a cut and not the map size
TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500,
                nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=nec.IOU_THR),
                score_threshold=0.1, pc_range=[-54, -54], out_size_factor=8, voxel_size=[0.075, 0.075], double_flip=False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cfg(hip, pre, post, circular=False, h=H, w=W):
    t = dict(TEST_CFG, nms=dict(TEST_CFG["nms"], nms_pre_max_size=pre, nms_post_max_size=post))
    return hip.make_decode_cfg(h, w, t, group_radius=[nec.RADIUS] if circular else None)


# ------------------------------------------------------------------------------------------------ IoU on the degenerate pairs
def _families(g):
    return [(str(name), np.nonzero(g["family"] == i)[0]) for i, name in enumerate(g["family_names"])]


def _check_iou(tag, g, idx, got):
    """|d| <= 2e-5 * max(1, |ref|) (the bound of test_iou_matches_compiled_reference_golden, scaled for the IoUs above 1 of vanishing extents);
    no NaN; identical boxes within 1e-5 of 1; yaw-0 pairs (no trigonometry in any vertex) bit for bit.  The worst difference of every family
    goes to the parity report before anything is asserted."""
    ref = g["iou"][idx]
    fam = g["family"][idx]
    names = [str(s) for s in g["family_names"]]
    err = np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    failures = []
    for f, name in enumerate(names):
        m = fam == f
        if not m.any():
            continue
        e = np.where(np.isnan(got[m]), np.inf, err[m])
        w = int(np.argmax(e))
        report("iou_edges %s %s (%d pairs)" % (tag, name, int(m.sum())), float(e[w]), 2e-5, "(worst: pair %d, ref %.9g, got %.9g)" % (idx[m][w], ref[m][w], got[m][w]))
        if not e.max() <= 2e-5:
            failures.append("%s: pair %d a=%s b=%s ref %.9g got %.9g" % (name, idx[m][w], g["a"][idx[m][w]].tolist(), g["b"][idx[m][w]].tolist(), ref[m][w], got[m][w]))
        if name == "identical" and not np.all(np.abs(got[m] - 1.0) <= 1e-5):
            failures.append("identical boxes: IoU %s" % got[m][np.abs(got[m] - 1.0) > 1e-5][:5])
        if name == "axis0":
            ne = np.nonzero(got[m].view(np.uint32) != ref[m].view(np.uint32))[0]
            report("iou_edges %s axis0 pairs not bit-equal to the reference" % tag, float(len(ne)), 0.0)
            for k in ne[:5]:
                failures.append("axis0 not bit-exact: pair %d a=%s b=%s ref %.9g got %.9g" % (idx[m][k], g["a"][idx[m][k]].tolist(), g["b"][idx[m][k]].tolist(), ref[m][k], got[m][k]))
    assert not np.isnan(got).any(), "NaN where the reference is finite: pairs %s" % idx[np.isnan(got)][:10]
    assert not failures, "\n".join(failures)


def test_iou_degenerate_pairs_full_matrix_launch(hip, golden):
    g = golden("iou_edges.npz")
    out = hip.boxes_iou_bev(_dev(g["a"]), _dev(g["b"])).cpu().numpy()
    assert out.shape == (len(g["a"]), len(g["b"]))
    _check_iou("[n,n] diagonal", g, np.arange(len(g["a"])), np.ascontiguousarray(np.diagonal(out)))


def test_iou_degenerate_pairs_single_pair_launches(hip, golden):
    """[1,1] launches (thread 0 of a lone workgroup: other index arithmetic than the full matrix), about 20 pairs of every family"""
    g = golden("iou_edges.npz")
    idx = np.concatenate([ids[np.linspace(0, len(ids) - 1, min(20, len(ids))).round().astype(int)] for _, ids in _families(g)])
    a, b = _dev(g["a"]), _dev(g["b"])
    got = torch.cat([hip.boxes_iou_bev(a[i:i + 1], b[i:i + 1]).reshape(1) for i in idx.tolist()]).cpu().numpy()
    _check_iou("[1,1] launches", g, idx, got)


# ------------------------------------------------------------------------------------------------ suppression patterns
_SCENES = {}


def _scene(name, n):
    """pattern -> boxes, expected keep list, and head maps whose decode is those boxes: candidate i in cell (37 i + 11) mod H W (so that the cell
    order is not the score order) with logit 4 - 0.004 i, strictly descending.  The 0.05 clearance from the IoU threshold is asserted with the host
    oracle on the boxes in both layouts the kernels see (as given to fd_rotated_nms; after the decode's swap to [.., d1, d0, .., -yaw - pi/2])."""
    if (name, n) not in _SCENES:
        from oracle import ops as oops

        pos, want = nec.pattern(name, n)
        b = nec.boxes(pos)
        for layout in (b, nms_layout(b)):
            assert nec.iou_clear_of_threshold(oops.boxes_iou_bev(layout, layout)), (name, n)
            assert oops.nms(layout, nec.IOU_THR).tolist() == want
        assert nec.radius_clear_of_distances(b[:, :2])
        cells = (37 * np.arange(n) + 11) % (H * W)
        logits = (4.0 - 0.004 * np.arange(n)).astype(np.float32)
        _SCENES[(name, n)] = dict(pos=pos, want=want, boxes=b, cells=cells, logits=logits, maps=nec.decode_maps(pos, H, W, cells, logits))
    return _SCENES[(name, n)]


@pytest.mark.parametrize("name", nec.PATTERNS)
def test_rotated_nms_on_known_patterns(hip, name):
    """fd_rotated_nms (nms_sweep with post_max = n): keep list and count equal the expected list, no tolerance"""
    for n in nec.SIZES:
        s = _scene(name, n)
        for tag, b in (("yaw 0", s["boxes"]), ("decode layout", nms_layout(s["boxes"]))):
            keep, cnt = hip.rotated_nms(_dev(b), nec.IOU_THR)
            cnt = int(cnt.cpu()[0])
            got = keep.cpu().numpy()
            assert cnt == len(s["want"]) and got[:cnt].tolist() == s["want"], (name, n, tag, cnt, got[:cnt][:10])
            assert not got[cnt:].any()
        report("fd_rotated_nms pattern %s n=%d: kept %d" % (name, n, len(s["want"])), 0.0, 0.0)


_SINGLE = {}


def _decode_single(hip, name, n, pre, post, circular=False):
    """one map through fd_centerpoint_decode -> host copies of (boxes7 [post,7], scores [post], cell [post], count)"""
    key = (name, n, pre, post, circular)
    if key not in _SINGLE:
        maps = [_dev(m) for m in _scene(name, n)["maps"]] if name else [_dev(m) for m in _empty_maps()]
        out = hip.centerpoint_decode(*maps, _cfg(hip, pre, post, circular))
        _SINGLE[key] = tuple(t.cpu().numpy()[0] for t in out)
    return _SINGLE[key]


def _empty_maps():
    return nec.decode_maps(np.zeros((0, 2)), H, W, np.zeros(0, np.int64), np.zeros(0, np.float32))


def _check_decoded(tag, s, post, out):
    boxes, scores, cell, count = out
    want = s["want"][:post]
    k = len(want)
    assert int(count) == k, (tag, int(count), k)
    assert cell[:k].tolist() == s["cells"][want].tolist(), (tag, cell[:k][:10], s["cells"][want][:10])
    hb = s["boxes"][want]
    assert np.array_equal(boxes[:k, :3], hb[:, :3]) and np.array_equal(boxes[:k, 6], hb[:, 6]), tag   # centres: the same float32 operations; yaw atan2f(0, 1)
    assert np.allclose(boxes[:k, 3:6], hb[:, 3:6], rtol=1e-6, atol=0), tag                               # expf(logf(side)) on the device
    assert np.allclose(scores[:k], 1.0 / (1.0 + np.exp(-s["logits"][want].astype(np.float64))), rtol=0, atol=2e-7), tag
    assert not boxes[k:].any() and not scores[k:].any() and np.all(cell[k:] == -1), tag


@pytest.mark.parametrize("name", nec.PATTERNS)
def test_decode_sweeps_on_known_patterns(hip, name):
    """fd_centerpoint_decode on maps crafted to decode to the pattern: nms_pre_max_size 1000 runs the fused nms_sweep_tail (mask in LDS), 4096 the
    unfused nms_sweep + dec_gather.  The kept cells are the cells of the expected rows, in order; count = min(post_max, kept); rows beyond are
    zero with cell -1; both paths return identical tensors."""
    for n in nec.SIZES:
        s = _scene(name, n)
        for post in (83, 128):
            fused = _decode_single(hip, name, n, 1000, post)
            unfused = _decode_single(hip, name, n, 4096, post)
            _check_decoded("%s n=%d post=%d fused" % (name, n, post), s, post, fused)
            _check_decoded("%s n=%d post=%d unfused" % (name, n, post), s, post, unfused)
            for a, b in zip(fused, unfused):
                assert np.array_equal(a, b), (name, n, post)
            report("decode pattern %s n=%d post_max=%d: kept %d of %d, fused == unfused" % (name, n, post, int(fused[3]), len(s["want"])), 0.0, 0.0)


@pytest.mark.parametrize("name", nec.PATTERNS)
def test_decode_circular_nms_on_known_patterns(hip, name):
    """the same scenes under circular NMS (squared centre distance <= 0.01: exact float32 arithmetic, no tolerance)"""
    for n in nec.SIZES:
        s = _scene(name, n)
        for post in (83, 128):
            out = _decode_single(hip, name, n, 1000, post, circular=True)
            _check_decoded("%s n=%d post=%d circular" % (name, n, post), s, post, out)
        report("decode pattern %s n=%d circular NMS: kept %d" % (name, n, len(s["want"])), 0.0, 0.0)


PACKED_SCENES = [("chain", 1000), ("star", 129), ("free", 65), ("clusters", 1000), ("late", 128), (None, 0)]  # decode group g = group * B + sample


@pytest.mark.parametrize("mode,post", [("fused", 83), ("fused", 128), ("unfused", 83), ("unfused", 128), ("circular", 83)])
def test_packed_decode_with_a_pattern_per_group(hip, mode, post):
    """fd_centerpoint_decode_packed, 2 groups x 3 samples in one launch, every (group, sample) map another pattern with another candidate count,
    one of them empty: every (sample, step) block of the packed rows and counts equals what the single-map call gave for that pattern, with the
    velocity read from the step's channels at the kept cells and the step's label.  "unfused" runs assemble_kernel, "fused" the tail of
    nms_sweep_tail, both with per-group counts."""
    from futuredet_amd.lib import MapView

    G, B = 2, 3
    pre, circular = (4096 if mode == "unfused" else 1000), mode == "circular"
    scenes = [_scene(nm, n)["maps"] if nm else _empty_maps() for nm, n in PACKED_SCENES]
    maps = [_dev(np.concatenate([sc[k] for sc in scenes], 0)) for k in range(5)]
    rng = np.random.default_rng(3)
    vel = rng.standard_normal((G * B, 4, H, W)).astype(np.float32)
    vel_d = _dev(vel)

    def view(t):
        return MapView(t.data_ptr(), t.stride(0), t.stride(1), 1, 0)

    step_group, step_vel, step_label = [0, 1, 1], [0, 2, 0], [0, 3, 5]
    packed, counts = hip.centerpoint_decode_packed([view(t) for t in maps], view(vel_d), G * B, B, _cfg(hip, pre, post, circular), maps[0].device,
                                                   step_group, step_vel, step_label)
    packed, counts = packed.cpu().numpy(), counts.cpu().numpy()
    assert packed.shape == (B, 3, post, 11) and counts.shape == (B, 3)
    for b in range(B):
        for st in range(3):
            g = step_group[st] * B + b
            nm, n = PACKED_SCENES[g]
            boxes, scores, cell, count = _decode_single(hip, nm, n, pre, post, circular)
            k = int(count)
            if nm:
                assert k == min(post, len(_scene(nm, n)["want"]))
            else:
                assert k == 0
            want = np.zeros((post, 11), np.float32)
            want[:k, :6] = boxes[:k, :6]
            want[:k, 6] = vel[g, step_vel[st]].reshape(-1)[cell[:k]]
            want[:k, 7] = vel[g, step_vel[st] + 1].reshape(-1)[cell[:k]]
            want[:k, 8] = boxes[:k, 6]
            want[:k, 9] = scores[:k]
            want[:k, 10] = step_label[st]
            assert int(counts[b, st]) == k, (mode, b, st, counts[b, st], k)
            assert np.array_equal(packed[b, st], want), (mode, b, st, nm, n)
    report("packed decode %s post_max=%d: counts %s" % (mode, post, counts.reshape(-1).tolist()), 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ the two selection paths
def _selection_scene():
    """A few hundred candidates in the top-left 40 x 40 cells: clusters of identical boxes (2, 5, 63, 64, 65 copies, in different cells, at
    positions that are multiples of 1/8 cell so that the copies decode bit-identically) and random rotated filler; a filler box is only taken
    if its IoU with every box before it is at least 0.05 away from the threshold.  Scores: strictly descending logits in a random order."""
    from oracle import ops as oops

    rng = np.random.default_rng(11)
    R = 40
    free_cells = rng.permutation(R * R)
    rows = []  # (pos_x, pos_y, dim0, dim1, rot0, rot1)

    def decoded(r):
        r = np.asarray(r, np.float32).reshape(-1, 6)
        b = np.zeros((len(r), 7), np.float32)
        b[:, :2] = (r[:, :2] * nec.OSF) * nec.VOXEL + nec.PC
        b[:, 3:5] = np.exp(r[:, 2:4])
        b[:, 5] = 1.5
        b[:, 6] = np.arctan2(r[:, 4], r[:, 5])
        return b

    def clear(row):
        if not rows:
            return True
        iou = oops.boxes_iou_bev(nms_layout(decoded(row)), nms_layout(decoded(rows)))[0]
        return bool(np.all(np.abs(iou - nec.IOU_THR) >= nec.CLEARANCE + 0.01))  # (the device's expf / atan2f move an IoU by ~1e-6: far inside the margin)

    for ln in (2, 5, 63, 64, 65):
        while True:
            row = (np.round(rng.uniform(2, 38) * 8) / 8, np.round(rng.uniform(2, 38) * 8) / 8, np.float32(rng.normal(0.8, 0.3)), np.float32(rng.normal(0.2, 0.3)),
                   np.float32(rng.standard_normal()), np.float32(rng.standard_normal()))
            if clear(row):
                break
        rows += [row] * ln
    tries = 0
    while len(rows) < 199 + 150:
        tries += 1
        assert tries < 20000
        row = (rng.uniform(1, 39), rng.uniform(1, 39), rng.normal(0.8, 0.4), rng.normal(0.2, 0.4), rng.standard_normal(), rng.standard_normal())
        row = tuple(np.float32(v) for v in row)
        if clear(row):
            rows.append(row)
    n = len(rows)
    rows = np.asarray(rows, np.float64)[rng.permutation(n)]  # score order
    rc = np.stack(np.divmod(free_cells[:n], R), -1)          # (row, column) of candidate i
    logits = (3.0 - 0.01 * np.arange(n)).astype(np.float32)
    b = decoded(rows)
    nb = nms_layout(b)
    iou = oops.boxes_iou_bev(nb, nb)
    assert nec.iou_clear_of_threshold(iou)
    want = oops.nms(nb, nec.IOU_THR).tolist()
    assert want == nec.greedy(iou > nec.IOU_THR)
    return rows, rc, logits, b, want


def _selection_maps(rows, rc, logits, h, w):
    hm = np.full((1, 1, h, w), -20.0, np.float32)
    reg = np.zeros((1, 2, h, w), np.float32)
    height = np.zeros((1, 1, h, w), np.float32)
    dim = np.zeros((1, 3, h, w), np.float32)
    rot = np.zeros((1, 2, h, w), np.float32)
    r, c = rc[:, 0], rc[:, 1]
    hm[0, 0, r, c] = logits
    reg[0, 0, r, c] = rows[:, 0] - c
    reg[0, 1, r, c] = rows[:, 1] - r
    dim[0, 0, r, c], dim[0, 1, r, c], dim[0, 2, r, c] = rows[:, 2], rows[:, 3], np.log(1.5)
    rot[0, 0, r, c], rot[0, 1, r, c] = rows[:, 4], rows[:, 5]
    return hm, reg, height, dim, rot


def test_both_selection_paths_give_the_same_nms(hip):
    """One scene in the top-left corner of a 180 x 180 map (H W = 32400: in-register selection, footprints from dec_rank_decode) and of a
    184 x 184 map (33856: streamed dec_select + footprint_kernel): boxes, scores and counts bit-identical, cells equal through (row, column),
    and both the oracle's greedy list."""
    rows, rc, logits, hb, want = _selection_scene()
    post = 128
    outs = {}
    for side in (180, 184):
        maps = _selection_maps(rows, rc, logits, side, side)
        # clusters: the copies sit in different cells and must still decode to one position
        out = hip.centerpoint_decode(*[_dev(m) for m in maps], _cfg(hip, 1000, post, h=side, w=side))
        outs[side] = tuple(t.cpu().numpy()[0] for t in out)
    k = min(post, len(want))
    for side, (boxes, scores, cell, count) in outs.items():
        assert int(count) == k, (side, int(count), k, len(want))
        got_rc = np.stack(np.divmod(cell[:k], side), -1)
        assert np.array_equal(got_rc, rc[want[:k]]), (side, "kept cells differ from the oracle's greedy list")
        assert np.allclose(boxes[:k], hb[want[:k]], rtol=2e-6, atol=2e-6)
        assert not boxes[k:].any() and np.all(cell[k:] == -1)
    a, b = outs[180], outs[184]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and int(a[3]) == int(b[3])
    assert np.array_equal(np.stack(np.divmod(a[2][:k], 180)), np.stack(np.divmod(b[2][:k], 184)))
    report("selection paths 180x180 vs 184x184: %d candidates, oracle keeps %d, returned %d, bit-identical" % (len(rows), len(want), k), 0.0, 0.0)
