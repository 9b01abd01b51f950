"""Chunk plans and equal-work ranges made straight from the sparse index (fd_spconv_plan_from_index / fd_spconv_ranges_from_index)
against the route they replace on the fp32 inference sweep, fd_rulebook -> fd_spconv_plan_build / fd_spconv_ranges: the same
integers.  The strided 16 -> 32, 32 -> 64 and 64 -> 128 layers fed by such a plan against the same layers fed by their table, and a
whole captured sweep with the index route on and off: the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import report

pytestmark = pytest.mark.gpu

SENT = 0x5a5a5a5a
GEOM = {"subm": ((1, 1, 1), (1, 1, 1)), "strided": ((2, 2, 2), (1, 1, 1))}  # (stride, pad) of the 3 x 3 x 3 window


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _i3(v):
    return (ctypes.c_int * 3)(*v)


def _index(hip, B, D, H, W, cells):
    """finalised SparseIndex of the (b, z, y, x) rows ``cells``"""
    ix = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    ix.mark(torch.from_numpy(np.ascontiguousarray(cells)).cuda())
    ix.scan(n_dev)
    ix.finalize(int(n_dev.cpu()[0]))
    return ix


@pytest.fixture(scope="module")
def levels(hip):
    """Three samples on a 9 x 24 x 24 grid: 1505 random active voxels in samples 0 and 2, sample 1 empty; and the level a 3 x 3 x 3
    stride-2 padding-1 convolution makes of it."""
    rng = np.random.default_rng(2024)
    B, D, H, W = 3, 9, 24, 24
    flat = rng.choice(2 * D * H * W, size=1505, replace=False)
    b, z, y, x = np.unravel_index(flat, (2, D, H, W))
    cells = np.stack([b * 2, z, y, x], 1).astype(np.int32)  # samples 0 and 2
    rng.shuffle(cells)
    src = _index(hip, B, D, H, W, cells)
    assert src.n == 1505
    down = src.downsample((3, 3, 3), (2, 2, 2), (1, 1, 1))
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    down.scan(n_dev)
    down.finalize(int(n_dev.cpu()[0]))
    assert down.n > 600 and (down.D, down.H, down.W) == (5, 12, 12)
    return dict(src=src, subm=src, strided=down)


def _chunks(n, ranges, n_ranges):
    """(row0, n_rows) of every chunk, from fd_spconv_chunk.h's description: range b = rows ranges[b] .. ranges[b + 1] (a table) or
    n_ranges equal row counts rounded up to 16, each cut into equal chunks of at most 128 rows, rounded up to 16."""
    if ranges is None:
        per = (-(-n // n_ranges) + 15) // 16 * 16
        bounds = [min(n, b * per) for b in range(n_ranges + 1)]
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


def _both_routes(L, src, dst, kind, n_out, n_dev, split, coords=None):
    """(plan from the table, plan from the index, the range table or None, ranges over which an equal split is cut) for the first
    ``n_out`` rows of ``dst`` (``n_dev``: device count, n_out is then a capacity; ``coords``: a capacity-sized coordinate table)."""
    stride, pad = GEOM[kind]
    coords = dst.coords if coords is None else coords
    count = n_dev if n_dev is not None else torch.tensor([n_out], dtype=torch.int32, device="cuda")
    nstride = max(64, (n_out + 63) // 64 * 64)
    nbr = torch.full((27, nstride), SENT, dtype=torch.int32, device="cuda")
    rc = L.fd_rulebook(_p(src.words), _p(src.prefix), src.B, src.D, src.H, src.W, _p(coords), n_out, _p(count), nstride, 0 if n_dev is not None else 1,
                       _i3((3, 3, 3)), _i3(stride), _i3(pad), _p(nbr), None)
    assert rc == 0, L.fd_last_error()
    ranges, n_ranges = None, split
    if split == "table":
        n_ranges = 5
        ranges = torch.full((n_ranges + 1,), -7, dtype=torch.int32, device="cuda")
        ws = torch.zeros(int(L.fd_spconv_ranges_workspace_bytes(n_out)), dtype=torch.uint8, device="cuda")
        assert L.fd_spconv_ranges(_p(nbr), nstride, 27, n_out, _p(n_dev), n_ranges, _p(ranges), _p(ws), ws.numel(), None) == 0, L.fd_last_error()
    pstride = int(L.fd_spconv_plan_stride(n_out))
    plans = [torch.full((28, pstride), SENT, dtype=torch.int32, device="cuda") for _ in range(2)]
    rc = L.fd_spconv_plan_build(_p(nbr), nstride, 27, n_out, _p(n_dev), _p(ranges), n_ranges, _p(plans[0]), pstride, None)
    assert rc == 0, L.fd_last_error()
    s = (hip_lib().PlanSource * 1)()
    s[0].in_words, s[0].in_prefix, s[0].out_coords = src.words.data_ptr(), src.prefix.data_ptr(), coords.data_ptr()
    s[0].n_out_dev = n_dev.data_ptr() if n_dev is not None else None
    s[0].ranges = ranges.data_ptr() if ranges is not None else None
    s[0].plan, s[0].n_out, s[0].plan_stride = plans[1].data_ptr(), n_out, pstride
    s[0].Din, s[0].Hin, s[0].Win, s[0].n_ranges = src.D, src.H, src.W, n_ranges
    s[0].stride[:], s[0].pad[:] = list(stride), list(pad)
    assert L.fd_spconv_plan_from_index(src.B, 1, s, None) == 0, L.fd_last_error()
    torch.cuda.synchronize()
    return plans[0].cpu().numpy(), plans[1].cpu().numpy(), (ranges.cpu().numpy() if ranges is not None else None), n_ranges


def hip_lib():
    from futuredet_amd import lib

    return lib


def _assert_same_plan(a, b, rows, chunks, what):
    """all 27 list rows at columns < rows, and the 27 count bytes at every chunk start (the other words of row 27 are undefined)"""
    assert sum(r for _, r in chunks) == rows, what
    assert np.array_equal(a[:27, :rows], b[:27, :rows]), what + ": lists differ"
    assert (b[:27, :rows] != SENT).all(), what + ": a column below the row count got no entry"
    ca, cb = a[27].view(np.uint8), b[27].view(np.uint8)
    for row0, _ in chunks:
        assert np.array_equal(ca[4 * row0:4 * row0 + 27], cb[4 * row0:4 * row0 + 27]), what + ": counts differ at row %d" % row0
    assert np.array_equal(a[:27, rows:], b[:27, rows:]), what + ": entries past the row count"


@pytest.mark.parametrize("split", [1, 3, 7, "table"])
@pytest.mark.parametrize("rem", [0, 1, 15])
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_plan_from_index_equals_plan_from_table(hip, levels, kind, rem, split):
    """SubM and strided, n_out % 16 in {0, 1, 15} (the largest such prefix of the level's rows), equal-row splits over 1, 3 and 7
    ranges and an equal-work range table: 1 range = 5-12 chunks behind each other, 7 ranges = chunks of 96-112 rows."""
    L = hip_lib().load()
    src, dst = levels["src"], levels[kind]
    n_out = dst.n - ((dst.n - rem) % 16)
    assert n_out % 16 == rem and n_out > 600
    a, b, ranges, n_eff = _both_routes(L, src, dst, kind, n_out, None, split)
    _assert_same_plan(a, b, n_out, _chunks(n_out, ranges, n_eff), "%s, %d rows, split %r" % (kind, n_out, split))


@pytest.mark.parametrize("split", [3, "table"])
@pytest.mark.parametrize("kind", ["subm", "strided"])
def test_plan_of_a_capacity_sized_level(hip, levels, kind, split):
    """A static index: tables and plan sized by a capacity, the device's count 219 rows below it; an equal split is then cut by the
    kernels from the count.  Nothing is written past the count."""
    L = hip_lib().load()
    src, dst = levels["src"], levels[kind]
    cap = dst.n + 219
    coords = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")  # (rows past the count are never read)
    coords[:dst.n] = dst.coords
    n_dev = torch.tensor([dst.n], dtype=torch.int32, device="cuda")
    a, b, ranges, n_eff = _both_routes(L, src, dst, kind, cap, n_dev, split, coords=coords)
    _assert_same_plan(a, b, dst.n, _chunks(dst.n, ranges, n_eff), "%s, capacity %d, count %d, split %r" % (kind, cap, dst.n, split))
    assert (b[:27, dst.n:] == SENT).all()


def test_empty_level_and_zero_count(hip, levels):
    """n_out = 0 launches nothing; a capacity-sized level whose device count is 0 writes nothing"""
    L = hip_lib().load()
    src = levels["src"]
    s = (hip_lib().PlanSource * 1)()
    s[0].n_out, s[0].n_ranges = 0, 4
    s[0].stride[:], s[0].pad[:] = [1, 1, 1], [1, 1, 1]
    assert L.fd_spconv_plan_from_index(src.B, 1, s, None) == 0, L.fd_last_error()
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    a, b, _, _ = _both_routes(L, src, src, "subm", 200, zero, 3)
    assert (a == SENT).all() and (b == SENT).all()


@pytest.mark.parametrize("static", [False, True])
def test_work_array_and_ranges_from_index(hip, levels, static):
    """block works of the SubM level from the index against block_work_kernel's from the table, and the two range tables"""
    L = hip_lib().load()
    src = levels["src"]
    n = src.n
    cap = n + 219 if static else n
    coords = torch.full((cap, 4), -1, dtype=torch.int32, device="cuda")
    coords[:n] = src.coords
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    nstride = (cap + 63) // 64 * 64
    nbr = torch.full((27, nstride), SENT, dtype=torch.int32, device="cuda")
    assert L.fd_rulebook(_p(src.words), _p(src.prefix), src.B, src.D, src.H, src.W, _p(coords), cap, _p(n_dev), nstride, 0 if static else 1,
                         _i3((3, 3, 3)), _i3((1, 1, 1)), _i3((1, 1, 1)), _p(nbr), None) == 0, L.fd_last_error()
    nb = int(L.fd_spconv_ranges_workspace_bytes(cap))
    for n_ranges in (1, 5, 64):
        ws = [torch.full((nb // 4,), SENT, dtype=torch.int32, device="cuda") for _ in range(2)]
        rg = [torch.full((n_ranges + 1,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        count = n_dev if static else None
        assert L.fd_spconv_ranges(_p(nbr), nstride, 27, cap, _p(count), n_ranges, _p(rg[0]), _p(ws[0]), nb, None) == 0, L.fd_last_error()
        assert L.fd_spconv_ranges_from_index(_p(src.words), src.B, src.D, src.H, src.W, _p(coords), cap, _p(count), n_ranges, _p(rg[1]), _p(ws[1]),
                                             nb, None) == 0, L.fd_last_error()
        torch.cuda.synchronize()
        blocks = (n + 7) // 8
        assert torch.equal(ws[0], ws[1]) and (ws[0][:blocks] != SENT).all() and (ws[0][blocks:] == SENT).all()
        assert torch.equal(rg[0], rg[1]) and int(rg[0][0]) == 0 and int(rg[0][-1]) == n
    assert ws[0][:blocks].min() >= 24 + 3  # (every block holds its own centre taps)


@pytest.fixture(scope="module")
def strided_case(hip):
    """900 random voxels of a 2 x 9 x 48 x 48 grid and the stride-2 level below it: 2-3k output rows"""
    rng = np.random.default_rng(77)
    B, D, H, W = 2, 9, 48, 48
    flat = rng.choice(B * D * H * W, size=900, replace=False)
    cells = np.stack(np.unravel_index(flat, (B, D, H, W)), 1).astype(np.int32)
    src = _index(hip, B, D, H, W, cells)
    down = src.downsample((3, 3, 3), (2, 2, 2), (1, 1, 1))
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    down.scan(n_dev)
    down.finalize(int(n_dev.cpu()[0]))
    assert 2000 <= down.n <= 3000, down.n
    return src, down, n_dev


@pytest.mark.parametrize("static", [False, True])
@pytest.mark.parametrize("cin, cout", [(16, 32), (32, 64), (64, 128)])
def test_strided_layers_fed_by_a_plan(hip, strided_case, cin, cout, static):
    """16 -> 32, 32 -> 64, 64 -> 128 with bias and ReLU: the launch that reads the plan made from the index (no table exists)
    against the launch that compacts its table itself -- torch.equal; ``static``: the level is capacity-sized, 300 rows above the
    device's count."""
    src, down, n_dev = strided_case
    rng = np.random.default_rng(cin)
    dst = down
    if static:
        dst = hip.SparseIndex(down.B, down.D, down.H, down.W, torch.device("cuda"), words=down.words, prefix=down.prefix)
        dst.n, dst.n_dev, dst.static, dst.n_expected = down.n + 300, n_dev, True, down.n
        dst.coords = torch.full((dst.n, 4), -1, dtype=torch.int32, device="cuda")
        dst.coords[:down.n] = down.coords
    x = torch.from_numpy(rng.standard_normal((src.n, cin)).astype(np.float32)).cuda()
    w = (rng.standard_normal((27, cin, cout)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
    wpk = hip.pack_spconv_weight(torch.from_numpy(w)).cuda()
    bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).cuda()
    geom = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
    table = src.rulebook(dst, *geom)
    direct = src.rulebook(dst, *geom, fp32_layer=(cin, cout))
    assert isinstance(table, torch.Tensor) and isinstance(direct, hip.IndexRulebook)
    y_table = hip.spconv_apply(x, wpk, bias, table, dst.n, cout, relu=True)
    y_plan = hip.spconv_apply(x, wpk, bias, direct, dst.n, cout, relu=True)
    torch.cuda.synchronize()
    assert direct._table is None and len(direct.plans) == 1, "the launch must have read the plan, not a table"
    assert torch.equal(y_plan[:down.n], y_table[:down.n]), "%d->%d: the plan-fed launch changed the output" % (cin, cout)
    assert float(y_table[:down.n].abs().max()) > 0.1 and float((y_table[:down.n] == 0).float().mean()) > 0.2  # (ReLU at work on real sums)
    hip.set_tuning("spconv_plan", 1)  # the A/B value: the same call now takes the table route
    try:
        y_knob = hip.spconv_apply(x, wpk, bias, direct, dst.n, cout, relu=True)
        assert direct._table is not None and torch.equal(y_knob[:down.n], y_table[:down.n])
    finally:
        hip.set_tuning("spconv_plan", 0)


def test_whole_pass_with_the_index_route_on_and_off(hip, monkeypatch):
    """One captured two-cloud pass (30k-point clouds) with plans from the index (default) and with the table route ("spconv_plan" = 1):
    identical packed detections, counts and level counts.  Every default sweep builds six index rulebooks (three strided layers, three SubM
    levels) and never falls back to a table."""
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.detectors import StaticStep
    from futuredet_amd.synth import seeded_state_dict, synthetic_cloud, tame_box_dims

    cfg = centerpoint_config("forecast_n0", "car")
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, 7)), strict=False)
    net = net.cuda().eval()
    clouds = [torch.from_numpy(synthetic_cloud(seed=s, target_points=30000)).cuda() for s in (11, 13)]
    made, tables = [], []
    init, table = hip.IndexRulebook.__init__, hip.IndexRulebook.table
    monkeypatch.setattr(hip.IndexRulebook, "__init__", lambda self, *a: (made.append(1), init(self, *a))[1])
    monkeypatch.setattr(hip.IndexRulebook, "table", lambda self: (tables.append(1), table(self))[1])

    def sweep():
        step = StaticStep(net, cfg.voxel_generator, capacity=32768, batch_size=2)
        with torch.no_grad():
            step.warm_up(clouds)
            del made[:]
            got = step(clouds)
            torch.cuda.synchronize()
            assert step.graph is not None
            return [t.clone() for t in got[:4]] + [step.level_counts.clone()], len(made)

    on, n_on = sweep()
    hip.set_tuning("spconv_plan", 1)
    try:
        off, n_off = sweep()
    finally:
        hip.set_tuning("spconv_plan", 0)
    assert n_on > 0 and n_on % 6 == 0 and n_off == 0 and not tables, (n_on, n_off, len(tables))
    for u, v in zip(on, off):
        assert torch.equal(u, v)
    assert int(on[4].min()) > 0
    report("static step: plans from the index / from tables replay bit-identical", 0.0, 0.0)
