"""The chunk plan of a shared SubM rulebook (fd_spconv_plan_build / fd_spconv_apply_plan): ready-made compacted pair lists instead
of the per-launch compaction.  The plan only moves work: every output must carry the bits of the plan-less launch, for every row
split; the plan itself is compared entry for entry with a numpy restatement of the compaction; a captured sweep replays the same
detections with the plan on and off."""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

PAD = np.int32(-256 + 128)  # 0xffffff00 | 128: the padding entry of a 128-row chunk
CHANNELS = [16, 32, 64, 128]
SPLITS = [None, "tiles", True]  # the layer's own split, one 128-row tile per workgroup, equal-work ranges


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _plan_off(hip, fn):
    hip.set_tuning("spconv_plan", -1)
    try:
        return fn()
    finally:
        hip.set_tuning("spconv_plan", 0)


def _subm_layer(hip, n_target, c, seed):
    """n_target active sites (sorted by the index) of a 2 x 6 x 12 x 16 grid, their SubM rulebook, rows, weights"""
    rng = np.random.default_rng(seed)
    B, D, H, W = 2, 6, 12, 16
    if n_target <= 300:
        flat = rng.choice(B * D * H * W, size=n_target, replace=False)
    else:  # ~1000 rows in two dense clumps and a thin haze: 8-row blocks of very different work -> empty equal-work ranges
        z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
        p = np.where((y < 5) & (x < 7), 0.95, 0.32)
        flat = np.flatnonzero(rng.random((B, D, H, W)) < p[None])
    idx = np.stack(np.unravel_index(flat, (B, D, H, W)), 1).astype(np.int32)
    rng.shuffle(idx)
    feats = rng.standard_normal((len(idx), c)).astype(np.float32)
    src = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    src.mark(_dev(idx))
    src.scan(n_dev)
    src.finalize(int(n_dev.cpu()[0]))
    assert src.n == len(idx)
    x = hip.rows_permute(_dev(feats), src.lookup(_dev(idx)), c, torch.float32, n_rows=src.n)
    w = (rng.standard_normal((27, c, c)) * np.sqrt(2.0 / (27 * c))).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    nbr = src.rulebook(src, (3, 3, 3), (1, 1, 1), (1, 1, 1))
    return dict(src=src, idx=idx, feats=feats, x=x, w=w, wpk=hip.pack_spconv_weight(torch.from_numpy(w)).cuda(), bias=_dev(bias), nbr=nbr,
                n=src.n, dims=(B, D, H, W))


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("n_out", [1, 17, 127, 128, 129, 300, 1000])
def test_layer_outputs_with_and_without_the_plan(hip, c, n_out):
    """One SubM layer (+ bias + residual + ReLU) with the plan on and off, for every row split: torch.equal; and the plan-on
    output against F.conv3d on the densified input (1e-4, the bound of test_sparse_conv_matches_dense_conv3d_directly)."""
    L = _subm_layer(hip, n_out, c, 1000 * c + n_out)
    n, nbr = L["n"], L["nbr"]
    res = _dev(np.random.default_rng(n_out).standard_normal((n, c)).astype(np.float32))
    for split in SPLITS:
        run = lambda: hip.spconv_apply(L["x"], L["wpk"], L["bias"], nbr, n, c, residual=res, relu=True, balanced=split)  # noqa: E731
        y_on = run()
        y_off = _plan_off(hip, run)
        assert torch.equal(y_on, y_off), "%d->%d, %d rows, split %r: the plan changed the output" % (c, c, n, split)
    if n_out == 1000:
        ranges, n_ranges = hip.ranges_for(nbr, c, c)
        r = ranges.cpu().numpy()
        assert (np.diff(r) == 0).any() and (np.diff(r) > 0).any(), "the equal-work table of this case has empty ranges"
    # the arbiter: dense conv3d (MIOpen fp32) at the active sites
    y = hip.spconv_apply(L["x"], L["wpk"], None, nbr, n, c)
    B, D, H, W = L["dims"]
    co = L["src"].coords.long()
    ii = torch.from_numpy(L["idx"].astype(np.int64)).cuda()
    dense_in = torch.zeros((B, c, D, H, W), device="cuda")
    dense_in[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]] = _dev(L["feats"])
    w5 = torch.from_numpy(L["w"]).reshape(3, 3, 3, c, c).permute(4, 3, 0, 1, 2).contiguous().cuda()
    ref = torch.nn.functional.conv3d(dense_in, w5, None, stride=1, padding=1)
    ref_rows = ref[co[:, 0], :, co[:, 1], co[:, 2], co[:, 3]]
    assert_close("spconv with chunk plan vs F.conv3d %d->%d (%d rows)" % (c, c, n), y.cpu().numpy(), ref_rows.cpu().numpy(), 1e-4)


def _edge_table(n, rng):
    """A table made by hand (not a geometry): tap 5 has no pair at all; with one tile per workgroup the two chunks of n = 129 rows
    are rows 0..79 and 80..128, and tap 7 has exactly 16 pairs in the first and exactly 17 in the second (the edges of the 16-pair
    groups); the other taps are random."""
    t = np.where(rng.random((27, n)) < 0.4, rng.integers(0, n, (27, n)), -1).astype(np.int32)
    t[5] = -1
    t[7] = -1
    t[7, rng.choice(80, 16, replace=False)] = rng.integers(0, n, 16)
    t[7, 80 + rng.choice(n - 80, 17, replace=False)] = rng.integers(0, n, 17)
    return t


@pytest.mark.parametrize("c", CHANNELS)
def test_padding_edges_and_an_empty_tap(hip, c):
    rng = np.random.default_rng(77 + c)
    n = 129
    t = _edge_table(n, rng)
    nbr = torch.full((27, 192), -1, dtype=torch.int32, device="cuda")
    nbr[:, :n] = _dev(t)
    nbr.n_out = n
    x = _dev(rng.standard_normal((n, c)).astype(np.float32))
    w = (rng.standard_normal((27, c, c)) * np.sqrt(2.0 / (27 * c))).astype(np.float32)
    wpk = hip.pack_spconv_weight(torch.from_numpy(w)).cuda()
    for split in SPLITS:
        run = lambda: hip.spconv_apply(x, wpk, None, nbr, n, c, balanced=split)  # noqa: E731
        y_on = run()
        assert torch.equal(y_on, _plan_off(hip, run)), (c, split)
    ref = torch.zeros((n, c), dtype=torch.float64, device="cuda")
    for k in range(27):
        m = nbr[k, :n] >= 0
        ref[m] += x.double()[nbr[k, :n][m].long()] @ torch.from_numpy(w[k]).double().cuda()
    assert_close("spconv with chunk plan, hand-made table %d->%d vs float64 definition" % (c, c), y_on.cpu().numpy(), ref.cpu().numpy(), 1e-4)


@pytest.mark.parametrize("c", [32, 64, 128])
def test_two_launches_share_one_plan(hip, c):
    """conv1 -> conv2 of a residual block on one rulebook: one plan build, two launches, the bits of two plan-less launches"""
    L = _subm_layer(hip, 300, c, 5 + c)
    n, nbr = L["n"], L["nbr"]
    w2 = hip.pack_spconv_weight(torch.from_numpy(L["w"][::-1].copy())).cuda()

    def block():
        y = hip.spconv_apply(L["x"], L["wpk"], L["bias"], nbr, n, c, relu=True)
        return hip.spconv_apply(y, w2, L["bias"], nbr, n, c, residual=L["x"], relu=True)

    out = block()
    assert len(nbr.plans) == 1, "both launches of the block read the same plan"
    assert torch.equal(out, _plan_off(hip, block))


def _chunks(n, ranges, n_ranges):
    """(row0, n_rows) of every chunk, restated from the header's description: range b = rows ranges[b] .. ranges[b + 1] (a table) or
    n_ranges equal row counts rounded up to 16 (n_ranges 0: as many ranges as 128-row tiles), each cut into equal chunks of at most
    128 rows, rounded up to 16."""
    if ranges is None:
        nr = n_ranges if n_ranges > 0 else -(-n // 128)
        per = (-(-n // nr) + 15) // 16 * 16
        bounds = [min(n, b * per) for b in range(nr + 1)]
    else:
        bounds = [min(n, int(v)) for v in ranges]
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi <= lo:
            continue
        nc = -(-(hi - lo) // 128)
        rows = (-(-(hi - lo) // nc) + 15) // 16 * 16
        out += [(lo + i * rows, min(rows, hi - lo - i * rows)) for i in range(nc) if hi - lo - i * rows > 0]
    return out


@pytest.mark.parametrize("split", ["tiles", "equal_rows", "table"])
def test_the_plan_itself(hip, split):
    """The plan of the 129-row hand-made table in a capacity-sized buffer (capacity 200, count 129 on the device), copied back and
    compared entry for entry with a numpy restatement of the compaction, written from the table: per chunk and tap the pairs
    (input row << 8 | local row) in row order, then padding entries up to the chunk's rows; the 27 counts as bytes in the count
    row.  Rows past the device's count get no entry: everything the restatement does not name still holds the sentinel."""
    from futuredet_amd import lib

    Lb = lib.load()
    rng = np.random.default_rng(129)
    n, cap = 129, 200
    t = _edge_table(n, rng)
    nbr = torch.full((27, 256), 12345, dtype=torch.int32, device="cuda")  # (the tail of a capacity-sized table is never read)
    nbr[:, :n] = _dev(t)
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    if split == "tiles":
        ranges, n_ranges, want_ranges = None, 0, None
        n_eff = 2  # ranges of a capacity launch are cut over the grid: ceil(200 / 128) workgroups
    elif split == "equal_rows":
        ranges, n_ranges, want_ranges, n_eff = None, 5, None, 5
    else:
        want_ranges = np.array([0, 0, 24, 24, 96, 129, 129], np.int32)  # empty ranges, a 5-row-short last range
        ranges, n_ranges, n_eff = _dev(want_ranges), 6, 6
    stride = int(Lb.fd_spconv_plan_stride(cap))
    assert stride >= cap + 8 and Lb.fd_spconv_plan_bytes(cap) == 28 * stride * 4
    SENT = 0x5a5a5a5a
    plan = torch.full((28, stride), SENT, dtype=torch.int32, device="cuda")
    rc = Lb.fd_spconv_plan_build(_p(nbr), 256, 27, cap, _p(n_dev), _p(ranges), n_ranges, _p(plan), stride, None)
    assert rc == 0, Lb.fd_last_error()
    torch.cuda.synchronize()
    got = plan.cpu().numpy()
    want = np.full((28, stride), SENT, np.int32)
    cnt_bytes = want[27].view(np.uint8)
    got_cnt = got[27].view(np.uint8).copy()
    chunks = _chunks(n, want_ranges, n_eff)
    assert sum(r for _, r in chunks) == n
    for row0, rows in chunks:
        for k in range(27):
            loc = np.flatnonzero(t[k, row0:row0 + rows] >= 0)
            lst = np.full(rows, PAD, np.int32)
            lst[:len(loc)] = (t[k, row0 + loc].astype(np.int64) << 8 | loc).astype(np.int32)
            want[k, row0:row0 + rows] = lst
            cnt_bytes[4 * row0 + k] = len(loc)
        got_cnt[4 * row0 + 27:4 * row0 + 32] = cnt_bytes[4 * row0 + 27:4 * row0 + 32]  # 5 spare bytes of the count block: unspecified
    assert np.array_equal(got[:27], want[:27]), "lists differ from the restated compaction"
    assert np.array_equal(got_cnt, cnt_bytes), "pair counts differ"
    if split == "tiles":
        assert (got[7, 0:16] != PAD).all() and got[7, 16] == PAD and (got[7, 80:97] != PAD).all() and got[7, 97] == PAD
        assert (got[5, :n] == PAD).all()
    assert (got[:27, n:] == SENT).all(), "rows past the device's count must get no entry"
    report("chunk plan (%s): lists and counts equal the numpy restatement" % split, 0.0, 0.0)


def _detector(variant="forecast_n0", seed=7):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, tame_box_dims

    cfg = centerpoint_config(variant, "car")
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, seed)), strict=False)
    return cfg, net.cuda().eval()


def test_captured_static_step_replays_the_same_detections(hip):
    """A whole sweep captured with the plan on and one captured with it off, replayed on the same clouds: a 30k-point cloud and a
    6k-point one whose levels fill a fraction of the captured capacities (rows past the device's count are capacity tail).  With
    data-free capacities and with capacities from a warm-up on the SMALL cloud, which the 30k-point cloud overflows (the step then
    re-runs it eagerly): identical padded detections, counts, level counts and overflow verdicts."""
    from futuredet_amd.detectors import StaticStep
    from futuredet_amd.synth import synthetic_cloud

    cfg, net = _detector()
    small, big = [_dev(synthetic_cloud(seed=s, target_points=p)) for s, p in ((12, 6000), (11, 30000))]

    def sweep(row_caps):
        step = StaticStep(net, cfg.voxel_generator, capacity=32768, row_caps=row_caps)
        outs = []
        with torch.no_grad():
            step.warm_up([small])
            for c in (small, big, small):
                got = step([c])
                torch.cuda.synchronize()
                assert step.graph is not None
                outs.append([t.clone() for t in got[:4]] + [step.level_counts.clone(), step.overflowed()])
        return outs

    for row_caps in ("datafree", "auto"):
        on = sweep(row_caps)
        off = _plan_off(hip, lambda: sweep(row_caps))
        for a, b in zip(on, off):
            for u, v in zip(a[:5], b[:5]):
                assert torch.equal(u, v), row_caps
            assert a[5] == b[5]
        print("[plan] row_caps %s: level counts %s, overflowed %s" % (row_caps, [o[4].cpu().tolist() for o in on], [o[5] for o in on]))
    report("static step: plan on / off replays bit-identical (capacity tails, data-free and warm-up capacities)", 0.0, 0.0)
