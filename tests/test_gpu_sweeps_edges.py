"""-m gpu: fd_sweep_assemble at its edges -- column widths, row counts around the 64 / 256 boundaries of the ballot-and-scan
compaction, the strict remove_close box, non-finite coordinates, empty sweeps, kMaxSweeps, the device-descriptor form -- bit for bit
against assemble_sweeps_ref (pillars_ref.py).  Matrix entries are multiples of 2^-10 below 64 and coordinates multiples of 2^-8
below 128, so the float64 4x4 product has no rounding and the kernel's fma chain cannot differ from numpy's dot; one case with
random rotations is compared with the oracle's fma chain instead.  A few hundred rows per case."""
import numpy as np
import pytest
import torch

import pillars_ref as pr

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same_bits(a, b, nan_aware=False):
    """bit-for-bit; nan_aware: a NaN matches any NaN (the payload of an invalid operation is the processor's choice)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    if not nan_aware:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _check(hip, raw, rows, mats, lags, close, keep_cols=4, radius=1.0, nan_aware=False, ref=None):
    """Runs the kernel on host descriptors and compares with the reference: count, the kept rows bit for bit, and +inf in every
    column of the tail [count, R).  -> (reference rows, kernel output [R, keep_cols + 1])"""
    if ref is None:
        ref = pr.assemble_sweeps_ref(raw, rows, mats, lags, close, keep_cols=keep_cols, min_distance=radius)
    out, count = hip.assemble_sweeps(_dev(raw), hip.sweep_descriptors(rows, mats, lags, close), keep_cols=keep_cols, min_distance=radius)
    out, n = _np(out), int(count.item())
    assert out.shape == (raw.shape[0], keep_cols + 1)
    assert n == len(ref), (n, len(ref))
    assert _same_bits(out[:n], ref, nan_aware)
    assert np.all(np.isposinf(out[n:]))
    return ref, out


def _cloud(rng, n, raw_cols, keep):
    """n rows with exact coordinates; row i lies inside the 1 m box (both axes) iff not keep[i]; further columns arbitrary floats"""
    raw = (rng.standard_normal((n, raw_cols)) * 20).astype(np.float32)
    raw[:, :3] = pr.exact_coords(rng, (n, 3))
    inside = (rng.integers(-255, 256, (n, 2)).astype(np.float64) / 256.0).astype(np.float32)
    one_axis = np.arange(n) % 5 == 0
    raw[one_axis, 1] = inside[one_axis, 1]              # some kept rows have exactly one axis inside
    both = (np.abs(raw[:, 0]) < 1) & (np.abs(raw[:, 1]) < 1)
    raw[both, 0] += np.float32(2.0)                     # a kept row has at least one axis outside
    drop = ~np.asarray(keep)
    raw[drop, :2] = inside[drop]
    return raw


def _sweep_params(rng, n_sweeps, first_is_key=True):
    """per-sweep (transforms, lags, remove_close): exact matrices, distinct lags; the key frame has neither transform nor filter"""
    mats = [pr.exact_transform(rng) for _ in range(n_sweeps)]
    lags = [0.05 * s + 0.001 for s in range(n_sweeps)]
    close = [True] * n_sweeps
    if first_is_key:
        mats[0], lags[0], close[0] = None, 0.0, False
    if n_sweeps > 2:
        mats[2] = None                                  # a sweep whose transform_matrix is None
    return mats, lags, close


def _split(total, parts):
    cuts = [total * k // parts for k in range(parts + 1)]
    return np.array(cuts, np.int64)


# ================================================================================================ column widths
@pytest.mark.parametrize("keep_cols", [3, 4, 5, 7])
def test_keep_cols_and_raw_cols(hip, keep_cols):
    for raw_cols in sorted({keep_cols, keep_cols + 1, 8}):
        rng = np.random.default_rng(10 * keep_cols + raw_cols)
        keep = rng.random(150) < 0.6
        raw = _cloud(rng, 150, raw_cols, keep)
        mats, lags, close = _sweep_params(rng, 3)
        rows = _split(150, 3)
        ref, out = _check(hip, raw, rows, mats, lags, close, keep_cols=keep_cols)
        assert len(ref) == 50 + int(keep[50:].sum()) and 0 < len(ref) < 150
        assert np.array_equal(ref[:50, 3:keep_cols], raw[:50, 3:keep_cols]) and np.all(ref[:50, keep_cols] == 0)


# ================================================================================================ wave / block boundaries
@pytest.mark.parametrize("pattern", ["mixed", "all", "none"])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 513])
def test_row_counts_at_wave_and_block_boundaries(hip, total, pattern):
    """The rank of a survivor is (block prefix) + (counts of the waves before its own) + (ballot bits below its lane): row counts on
    both sides of 64 and 256, with survivors on both sides of every boundary and a different count in every wave."""
    rng = np.random.default_rng(total)
    if pattern == "mixed":
        keep = rng.random(total) < 0.55
        edge = np.arange(total) % 64
        keep[(edge == 0) | (edge == 63)] = True
        keep[-1] = True
    else:
        keep = np.full(total, pattern == "all")
    raw = _cloud(rng, total, 5, keep)
    n_sweeps = min(3, total)
    mats, lags, close = _sweep_params(rng, n_sweeps, first_is_key=False)
    ref, out = _check(hip, raw, _split(total, n_sweeps), mats, lags, close)
    assert len(ref) == int(keep.sum())
    if pattern == "none":
        assert len(ref) == 0 and np.all(np.isposinf(out))
    if pattern == "mixed" and total >= 64:
        per_wave = [int(keep[w:w + 64].sum()) for w in range(0, total - total % 64, 64)]
        assert 0 < len(ref) < total and (total < 256 or len(set(per_wave)) > 1)


# ================================================================================================ the remove_close box
def _box_rows(radius):
    r = np.float32(radius)
    big = np.float32(np.inf)
    vals = np.array([r, -r, np.nextafter(r, np.float32(0)), np.nextafter(r, big), -np.nextafter(r, np.float32(0)), -np.nextafter(r, big),
                     0.0, -0.0, 0.5 * r, np.nan, np.inf, -np.inf, 3.0 * r], np.float32)
    x, y = np.meshgrid(vals, vals, indexing="ij")
    raw = np.zeros((x.size, 5), np.float32)
    raw[:, 0], raw[:, 1] = x.ravel(), y.ravel()
    raw[:, 2] = np.arange(x.size) / 256.0
    raw[:, 3] = np.arange(x.size)
    inside = lambda v: abs(float(v)) < float(r)  # noqa: E731  (False for NaN)
    keep = np.array([not (inside(a) and inside(b)) for a, b in raw[:, :2]])
    return raw, keep


@pytest.mark.parametrize("radius", [1.0, 2.5])
@pytest.mark.parametrize("flag", [True, False], ids=["remove_close", "flag-off"])
def test_remove_close_box_is_strict_and_handles_non_finite(hip, flag, radius):
    """|x| == r exactly is kept, one ulp inside is dropped (when y is inside too), a row with one axis inside is kept, -0.0 counts as
    inside, NaN and +-inf fail the strict '<' and are kept; with the flag off everything is kept.  Without and with a transform."""
    raw, keep = _box_rows(radius)
    n = len(raw)
    assert n == 169 and keep.sum() == 169 - 25  # 5 values of 13 are strictly inside: 0, -0, r/2, +-(r - 1 ulp)
    rng = np.random.default_rng(17)
    for mat in (None, pr.exact_transform(rng)):
        ref, out = _check(hip, raw, [0, n], [mat], [0.25], [flag], radius=radius, nan_aware=mat is not None)
        want = keep if flag else np.ones(n, bool)
        assert len(ref) == want.sum() and np.array_equal(ref[:, 3], raw[want, 3])
        if mat is None:
            assert _same_bits(ref[:, :4], raw[want, :4])  # -0.0, NaN and inf pass through bit for bit
    # a flagged sweep between two unflagged ones: the flag is the sweep's own
    three = np.concatenate([raw, raw, raw])
    ref, _ = _check(hip, three, [0, n, 2 * n, 3 * n], [None] * 3, [0.0, 0.1, 0.2], [False, flag, False], radius=radius)
    assert len(ref) == 2 * n + (keep.sum() if flag else n)


# ================================================================================================ empty sweeps, many sweeps
@pytest.mark.parametrize("sizes", [[0, 70, 40], [70, 0, 40], [70, 40, 0], [50, 0, 0, 60], [0, 0, 30, 0], [0, 1], [1, 0]], ids=str)
def test_empty_sweeps_first_middle_last_and_adjacent(hip, sizes):
    """Every sweep has its own time lag and matrix: a row attributed to a neighbouring (empty) sweep would carry the wrong ones."""
    rng = np.random.default_rng(sum((i + 1) * s for i, s in enumerate(sizes)))
    total = sum(sizes)
    keep = rng.random(total) < 0.7
    raw = _cloud(rng, total, 5, keep)
    mats, lags, close = _sweep_params(rng, len(sizes), first_is_key=False)
    mats = [pr.exact_transform(rng) for _ in sizes]
    rows = np.cumsum([0] + sizes)
    ref, _ = _check(hip, raw, rows, mats, lags, close)
    assert len(ref) == keep.sum()
    assert set(np.unique(ref[:, 4])) <= {np.float32(lags[s]) for s in range(len(sizes)) if sizes[s]}


def _many_sweeps(rng, n_sweeps):
    sizes = [(7 * s) % 10 for s in range(n_sweeps)]  # 0 .. 9 rows, several empty ones
    total = sum(sizes)
    keep = rng.random(total) < 0.7
    raw = _cloud(rng, total, 5, keep)
    mats = [pr.exact_transform(rng) if s % 3 else None for s in range(n_sweeps)]
    lags = [0.01 * s for s in range(n_sweeps)]
    return raw, np.cumsum([0] + sizes), mats, lags, [s % 4 != 0 for s in range(n_sweeps)]


def test_64_sweeps_and_the_limit(hip):
    rng = np.random.default_rng(64)
    raw, rows, mats, lags, close = _many_sweeps(rng, 64)
    assert 256 < len(raw) < 513 and (np.diff(rows) == 0).sum() >= 6
    ref, _ = _check(hip, raw, rows, mats, lags, close)
    assert 0 < len(ref) < len(raw) and len(np.unique(ref[:, 4])) > 40
    raw, rows, mats, lags, close = _many_sweeps(rng, 65)
    with pytest.raises(hip.FutureDetHipError, match="n_sweeps"):
        hip.assemble_sweeps(_dev(raw), hip.sweep_descriptors(rows, mats, lags, close))


# ================================================================================================ device descriptors
F_CANARY, I_CANARY = -7.5, -9


def test_device_descriptor_form_with_garbage_past_row_end(hip):
    """The static form: a device table with room for 8 records of which n_sweeps = 3 count, R = row_end + 100 as an upper bound with
    NaN in the 100 extra raw rows; ``count`` and ``out`` supplied by the caller, ``out`` longer than R.  The extra rows are dropped and
    come out as +inf, the rows of ``out`` past R stay untouched."""
    rng = np.random.default_rng(33)
    sizes = [120, 90, 101]
    total, extra = sum(sizes), 100
    keep = rng.random(total) < 0.6
    raw = np.concatenate([_cloud(rng, total, 5, keep), np.full((extra, 5), np.nan, np.float32)])
    mats, lags, close = _sweep_params(rng, 3)
    rows = np.cumsum([0] + sizes)
    table = np.zeros((8,), hip.SWEEP_DESC)
    table[:3] = hip.sweep_descriptors(rows, mats, lags, close)
    table[3:] = hip.sweep_descriptors([total, total + 40, total + 60, total + 100, total + 100, 10 ** 6], [pr.exact_transform(rng)] * 5,
                                      [9.0] * 5, [False] * 5)  # records a former, longer cloud left behind
    desc = _dev(table.view(np.uint8).reshape(-1))
    R = total + extra
    out = torch.full((R + 7, 5), F_CANARY, dtype=torch.float32, device="cuda")
    count = torch.full((1,), I_CANARY, dtype=torch.int32, device="cuda")
    got_out, got_count = hip.assemble_sweeps(_dev(raw), desc, out=out, count=count, n_sweeps=3)
    assert got_out.data_ptr() == out.data_ptr() and got_count.data_ptr() == count.data_ptr()
    ref = pr.assemble_sweeps_ref(raw, rows, mats, lags, close)
    n = int(count.item())
    res = _np(out)
    assert n == len(ref) == 120 + int(keep[120:].sum())
    assert _same_bits(res[:n], ref) and np.all(np.isposinf(res[n:R])) and np.all(res[R:] == F_CANARY)
    # the same table read as 5 records: the 4th and 5th sweep now own the first 60 extra rows (NaN passes the filter-less sweeps)
    out.fill_(F_CANARY)
    hip.assemble_sweeps(_dev(raw), desc, out=out, count=count, n_sweeps=5)
    assert int(count.item()) == n + 60 and np.all(_np(out)[R:] == F_CANARY)


# ================================================================================================ random rotations
def test_random_rotations_vs_oracle(hip):
    """Rounding in the float64 product: the kernel's fma chain against the oracle's (bit-exact with the reference's goldens)."""
    from oracle import ops as oops

    rng = np.random.default_rng(21)
    S = 6
    raws, mats, lags = [], [], []
    for s in range(S):
        n = 60 + 11 * s
        raw = rng.normal(0, [6.0, 6.0, 1.5, 30.0, 5.0], (n, 5)).astype(np.float32)
        raw[: n // 3, :2] = rng.uniform(-1.5, 1.5, (n // 3, 2))
        raws.append(raw)
        if s:
            a, b = rng.uniform(-np.pi, np.pi, 2)
            rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            m = np.eye(4)
            m[:3, :3] = rz @ rx
            m[:3, 3] = rng.normal(0, [20.0, 5.0, 0.2])
            mats.append(None if s == 3 else m)
            lags.append(0.05 * s)
    want = oops.assemble_sweeps(raws[0], raws[1:], mats, lags)
    order = [0] + [int(i) + 1 for i in np.random.default_rng(0).choice(S - 1, S - 1, replace=False)]
    rows = np.cumsum([0] + [len(raws[s]) for s in order])
    ref, _ = _check(hip, np.concatenate([raws[s] for s in order]), rows, [None if s == 0 else mats[s - 1] for s in order],
                    [0.0 if s == 0 else lags[s - 1] for s in order], [s != 0 for s in order], ref=want)
    assert 0 < len(ref) < rows[-1]
