"""The item loops of the fp32 pair-compacting sparse convolutions (fd_spconv_c32.hip, fd_spconv_v2.hip) after their bookkeeping moved
off the vector ALU: address arithmetic only, so every output keeps the bits it had.

  * hand-made rulebooks at the edges of the item lists (n_out 1 / 17 / 128 / 129 / 300; a centre tap that holds every row; taps of
    exactly 32 / 33 and 16 / 17 pairs in one chunk; an empty tap; a chunk whose only non-empty tap is the last one), per kernel family,
    table route and plan route, plain and bank-spread: every launch equals the recorded output of the parent build
    (tests/golden/spconv_item_loop.npz, written by tests/golden/make_spconv_item_loop.py), the float64 gather-GEMM within 1e-4 and,
    for 32 -> 32, the 16-pair kernel within 1e-4;
  * one synthetic batch of two small clouds through the index pyramid (about 3000 rows on the finer level: two dozen 128-row chunks
    with taps of 0, 1, 2 and 3+ items and a last chunk that is not full), plan straight from the index against the table route;
  * poisoned capacity tails: NaN behind the input's rows and behind the output's rows.

Bounds.  1e-4 * max(1, |ref|) against float64 is the bound tests/test_gpu_spconv_plan.py uses for the same hand-made-table comparison
(tests/test_gpu_spconv_swizzle.py compares bits only and states no float64 bound); 1e-4 between the 32-pair and the 16-pair kernel is
the bound the existing tests use between kernel families.  Everything else is torch.equal."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from parity_util import assert_close, report

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spconv_item_loop.npz")
# (cin, cout): the 32-pair kernel; the strided 16-pair shapes; the wide SubM 16-pair shapes
FAMILIES = [(32, 32), (16, 32), (32, 64), (64, 128), (64, 64), (128, 128)]
N_OUT = [1, 17, 128, 129, 300]
VARIANTS = ["edges", "last_tap"]
GOLDEN_FULL_ROWS = 129  # cases up to this many rows are recorded whole, all cases by their digest


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _n_in(cin, cout, n_out):
    return n_out if cin == cout else 2 * n_out + 3


def last_chunk_start(n_out):
    """first row of the last chunk when every workgroup takes one 128-row tile (equal chunks, multiples of 16 rows)"""
    n_chunks = (n_out + 127) // 128
    rows = ((n_out + n_chunks - 1) // n_chunks + 15) // 16 * 16
    return (n_chunks - 1) * rows


def hand_table(variant, cin, cout, n_out, seed):
    """K = 27 table made by hand (not a geometry), int32 [27, n_out].
    "edges": tap 13 holds every row, tap 5 none, taps 7 / 8 / 9 / 10 exactly 32 / 33 / 16 / 17 pairs (or all rows, if fewer), all of them
    in the first chunk of the one-tile-per-workgroup split; the other taps are random.
    "last_tap": random, but the last chunk of that split (the whole table up to 128 rows) has pairs in tap 26 only."""
    rng = np.random.default_rng(seed)
    n_in = _n_in(cin, cout, n_out)
    t = np.where(rng.random((27, n_out)) < 0.4, rng.integers(0, n_in, (27, n_out)), -1).astype(np.int32)
    if variant == "edges":
        first = min(n_out, last_chunk_start(n_out) or n_out)
        t[5] = -1
        t[13] = np.arange(n_out) if cin == cout else rng.integers(0, n_in, n_out)
        for tap, count in ((7, 32), (8, 33), (9, 16), (10, 17)):
            t[tap] = -1
            c = min(count, first)
            t[tap, rng.choice(first, c, replace=False)] = rng.integers(0, n_in, c)
    else:
        cut = last_chunk_start(n_out)
        t[:26, cut:] = -1
        t[26, cut:] = rng.integers(0, n_in, n_out - cut)
    return t


def make_case(hip, variant, cin, cout, n_out):
    seed = 100000 * VARIANTS.index(variant) + 1000 * cin + 7 * cout + n_out
    t = hand_table(variant, cin, cout, n_out, seed)
    rng = np.random.default_rng(seed + 1)
    n_in = _n_in(cin, cout, n_out)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n_out, cout)).astype(np.float32)
    stride = max(64, (n_out + 63) // 64 * 64)
    nbr = torch.full((27, stride), -1, dtype=torch.int32, device="cuda")
    nbr[:, :n_out] = _dev(t)
    nbr.n_out = n_out
    return dict(key="%s_%d_%d_%d" % (variant, cin, cout, n_out), t=t, x=x, w=w, bias=bias, res=res, nbr=nbr, n_in=n_in, n_out=n_out, cin=cin,
                cout=cout, xd=_dev(x), wpk=hip.pack_spconv_weight(torch.from_numpy(w)).cuda(), biasd=_dev(bias), resd=_dev(res))


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def input_digest(case):
    h = hashlib.sha256()
    for a in (case["t"], case["x"], case["w"], case["bias"], case["res"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def golden_call(hip, case):
    """the recorded launch: table route, plain rows, bias + residual, no ReLU (every bit of every sum stays visible)"""
    return hip.spconv_apply(case["xd"], case["wpk"], case["biasd"], case["nbr"], case["n_out"], case["cout"], residual=case["resd"], plan=False)


def _plan_only(hip, case, x, residual, layout, split):
    """the plan route of a strided shape on a hand-made table: the plan built from the table, the launch given the plan alone"""
    from futuredet_amd import lib

    L = lib.load()
    nbr, n_out, cin, cout = case["nbr"], case["n_out"], case["cin"], case["cout"]
    ranges, n_ranges = hip.row_split(nbr, n_out, cin, cout, split)
    plan, pstride = hip.plan_for(nbr, n_out, ranges, n_ranges)
    out = torch.empty((n_out, cout), device="cuda")
    rc = L.fd_spconv_apply_layout(_p(x), x.shape[0], _p(case["wpk"]), _p(case["biasd"]), _p(residual), 0, None, nbr.shape[1], _p(ranges), n_ranges,
                                  27, n_out, None, 0, cin, cout, 0, _p(out), _p(plan), pstride, int(layout), None)
    assert rc == 0, L.fd_last_error()
    return out


def routes(hip, case):
    """(name, output in plain rows) of every route of the case: table / plan, layout bits off / on, the family's split / one tile per workgroup"""
    cin, cout, n_out = case["cin"], case["cout"], case["n_out"]
    subm = cin == cout
    x, res = case["xd"], case["resd"]
    xs, res_s = hip.swizzle_rows(x), hip.swizzle_rows(res)
    # SubM from 32 channels: every tensor bank-spread; strided into such a level: residual and output
    lay_on = 7 if subm else 6
    for split in (None, "tiles"):
        for lay in (0, lay_on):
            xi = xs if lay & 1 else x
            ri = res_s if lay & 2 else res
            for plan in (False, True):
                name = "%s split %r layout %d %s" % (case["key"], split, lay, "plan" if plan else "table")
                if plan and not subm:
                    y = _plan_only(hip, case, xi, ri, lay, split)
                else:
                    y = hip.spconv_apply(xi, case["wpk"], case["biasd"], case["nbr"], n_out, cout, residual=ri, plan=plan, layout=lay, balanced=split)
                yield name, (hip.swizzle_rows(y) if lay & 4 else y)


def reference64(case):
    """float64 gather-GEMM on the CPU: bias + residual + sum over taps of x[nbr[k]] @ w[k]"""
    t = torch.from_numpy(case["t"]).long()
    x, w = torch.from_numpy(case["x"]).double(), torch.from_numpy(case["w"]).double()
    ref = torch.from_numpy(case["bias"]).double()[None, :] + torch.from_numpy(case["res"]).double()
    for k in range(27):
        m = t[k] >= 0
        ref[m] += x[t[k][m]] @ w[k]
    return ref.numpy()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n_out", N_OUT)
@pytest.mark.parametrize("cin,cout", FAMILIES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_hand_made_rulebooks_keep_the_parents_bits(hip, golden, variant, cin, cout, n_out):
    case = make_case(hip, variant, cin, cout, n_out)
    key = case["key"]
    assert str(golden["in:" + key]) == input_digest(case), "the generated case is not the recorded one (numpy's streams moved?)"
    want_digest = str(golden["sha:" + key])
    want = torch.from_numpy(golden["out:" + key]).cuda() if "out:" + key in golden else None  # (recorded whole: "edges" up to 129 rows)
    n = 0
    for name, y in routes(hip, case):
        if want is not None:
            assert torch.equal(y, want), name + ": differs from the parent build's output"
        assert digest(y) == want_digest, name + ": differs from the parent build's output (digest)"
        n += 1
    y = golden_call(hip, case)
    assert_close("item loop %s vs float64 gather-GEMM" % key, y.cpu().numpy(), reference64(case), 1e-4)
    if (cin, cout) == (32, 32):
        hip.set_tuning("spconv_c32", -1)
        try:
            y16 = golden_call(hip, case)
        finally:
            hip.set_tuning("spconv_c32", 0)
        assert_close("item loop %s: 32-pair vs 16-pair kernel" % key, y.cpu().numpy(), y16.cpu().numpy(), 1e-4)
    report("item loop %s: %d routes carry the parent's bits" % (key, n), 0.0, 0.0)


@pytest.fixture(scope="module")
def pyramid(hip):
    """two small clouds on a 2 x 9 x 24 x 24 grid and the stride-2 level above them.  Cloud 0: a dense clump (taps of 3 and 4 items per chunk)
    and a lattice of isolated sites (chunks in which only the centre tap has pairs); cloud 1: an even 40 % (taps of 1 and 2 items)"""
    rng = np.random.default_rng(2024)
    B, D, H, W = 2, 9, 24, 24
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    lattice = (y >= 8) & (z % 2 == 0) & (y % 2 == 0) & (x % 2 == 0)
    p = np.stack([np.where((y < 8) & (x < 8), 0.95, np.where(lattice, 0.5, 0.0)), np.full((D, H, W), 0.4)])
    idx = np.argwhere(rng.random((B, D, H, W)) < p).astype(np.int32)
    rng.shuffle(idx)
    src = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    src.mark(_dev(idx))
    src.scan(counts[0:1])
    dst = src.downsample((3, 3, 3), (2, 2, 2), (1, 1, 1))
    dst.scan(counts[1:2])
    host = counts.cpu()
    src.finalize(int(host[0]))
    dst.finalize(int(host[1]))
    assert 1500 <= src.n <= 3000 and src.n % 128 != 0 and dst.n > 257
    tables = dict(subm=src.rulebook(src, (3, 3, 3), (1, 1, 1), (1, 1, 1)).cpu().numpy(),
                  down=src.rulebook(dst, (3, 3, 3), (2, 2, 2), (1, 1, 1)).cpu().numpy())
    per_chunk = np.stack([(tables["subm"][:, r:r + 128][:, : src.n - r] >= 0).sum(1) for r in range(0, src.n, 128)])
    items = (per_chunk + 31) // 32
    assert all((items == v).any() for v in (0, 1, 2)) and (items >= 3).any(), "taps with 0, 1, 2 and 3+ 32-pair items"
    return dict(src=src, dst=dst, tables=tables)


@pytest.mark.parametrize("cin,cout", FAMILIES)
def test_pyramid_level_plan_from_index_and_table_route(hip, pyramid, cin, cout):
    src, dst = pyramid["src"], pyramid["dst"]
    subm = cin == cout
    out_ix = src if subm else dst
    geom = ((3, 3, 3), (1, 1, 1), (1, 1, 1)) if subm else ((3, 3, 3), (2, 2, 2), (1, 1, 1))
    rng = np.random.default_rng(31 * cin + cout)
    x = rng.standard_normal((src.n, cin)).astype(np.float32)
    w = (rng.standard_normal((27, cin, cout)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((out_ix.n, cout)).astype(np.float32)
    xd, wpk, bd, rd = _dev(x), hip.pack_spconv_weight(torch.from_numpy(w)).cuda(), _dev(bias), _dev(res)
    from_index = src.rulebook(out_ix, *geom, fp32_layer=(cin, cout))
    assert isinstance(from_index, hip.IndexRulebook)
    table = src.rulebook(out_ix, *geom)
    n = out_ix.n
    y_table = hip.spconv_apply(xd, wpk, bd, table, n, cout, residual=rd, plan=False)
    y_plan = hip.spconv_apply(xd, wpk, bd, from_index, n, cout, residual=rd)
    assert torch.equal(y_plan, y_table)
    lay = 7 if subm else 6
    y_lay = hip.spconv_apply(hip.swizzle_rows(xd) if lay & 1 else xd, wpk, bd, from_index, n, cout, residual=hip.swizzle_rows(rd), layout=lay)
    assert torch.equal(hip.swizzle_rows(y_lay), y_table)
    y_relu = hip.spconv_apply(xd, wpk, bd, from_index, n, cout, residual=rd, relu=True)
    assert torch.equal(y_relu, y_table.clamp_min(0.0))
    case = dict(t=pyramid["tables"]["subm" if subm else "down"][:, :n], x=x, w=w, bias=bias, res=res)
    assert_close("item loop, pyramid level %d->%d (%d rows) vs float64 gather-GEMM" % (cin, cout, n), y_plan.cpu().numpy(), reference64(case), 1e-4)
    if subm and cin == 32:
        hip.set_tuning("spconv_c32", -1)
        try:
            y16 = hip.spconv_apply(xd, wpk, bd, from_index, n, cout, residual=rd)
        finally:
            hip.set_tuning("spconv_c32", 0)
        assert_close("item loop, pyramid level 32->32: 32-pair vs 16-pair kernel", y_plan.cpu().numpy(), y16.cpu().numpy(), 1e-4)


@pytest.mark.parametrize("n_out", [17, 129, 300])
@pytest.mark.parametrize("cin,cout", FAMILIES)
def test_poisoned_capacity_tails(hip, cin, cout, n_out):
    """NaN in the rows behind the input's n_in rows and behind the output's n_out rows: a padding lane must read zeros (the gather's
    bounds check), never the tail, and nothing may be written past n_out -- table and plan route, plain and bank-spread input"""
    case = make_case(hip, "edges", cin, cout, n_out)
    n_in, subm = case["n_in"], cin == cout
    want = golden_call(hip, case)
    tail = 64
    for lay in ((0, 1) if subm else (0,)):
        x_cap = torch.full((n_in + tail, cin), float("nan"), device="cuda")
        x_cap[:n_in] = hip.swizzle_rows(case["xd"]) if lay & 1 else case["xd"]
        for plan in (False, True):
            out_cap = torch.full((n_out + tail, cout), float("nan"), device="cuda")
            if plan and not subm:
                y = _plan_only(hip, case, x_cap[:n_in], case["resd"], lay, None)
                out_cap[:n_out] = y  # (this route allocates its own output: only the input tail is poisoned)
            else:
                hip.spconv_apply(x_cap[:n_in], case["wpk"], case["biasd"], case["nbr"], n_out, cout, residual=case["resd"], plan=plan, layout=lay,
                                 out=out_cap[:n_out])
            torch.cuda.synchronize()
            assert not bool(torch.isnan(out_cap[:n_out]).any()), (cin, cout, n_out, lay, plan)
            assert bool(torch.isnan(out_cap[n_out:]).all()), "rows >= n_out were written"
            assert torch.equal(out_cap[:n_out], want), (cin, cout, n_out, lay, plan)
