"""-m gpu: the eval-mode PointPillars input path -- fd_pillar_encode (all four pillar_encode instantiations) against the float64
numpy restatement of pillars_ref.py under the fp32-restatement rule, and fd_pillar_scatter (all four dtype pairs) exactly.  Every
input comes from a fixed seed; test_pillars_ref_host.py ties the references to the reference's goldens and the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

import front_end_ref as fr
import pillars_ref as pr

pytestmark = pytest.mark.gpu

# units per layer -> the instantiation fd_pillar_encode dispatches: G = 64 / U1 point groups per wave in layer 1
DISPATCH = {"u16": [16], "u32": [32], "u64": [64], "two": [32, 64]}   # <16,false> G=4, <32,false> G=2, <64,false> G=1, <32,true> G=2
P_VALUES = (1, 2, 3, 20, 31, 32)   # below G, no multiple of G, the shipped 20, kMaxP - 1, kMaxP
NDIM_VALUES = (3, 5, 8)            # both limits and the shipped width


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    """bf16 tensor -> uint16 bits on the host."""
    return _np(t.contiguous().view(torch.int16)).view(np.uint16)


def _bf16_dev(bits):
    return _dev(np.ascontiguousarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)


def _bf16_as_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _fin(ndim, wd):
    return ndim + 5 + int(wd)


def _seed(*parts):
    s = 7
    for p in parts:
        s = s * 131 + int(p)
    return s


class _Case(object):
    """One reader input on the host, with its float64 reference and fp32 restatement (computed once)."""

    def __init__(self, units, wd, M, P, ndim, seed):
        rng = np.random.default_rng(seed)
        self.units, self.wd, self.M, self.P, self.ndim = units, wd, M, P, ndim
        self.vox, self.num, self.coors = pr.make_pillars(rng, M, P, ndim)
        self.layers = pr.make_layers(rng, units, _fin(ndim, wd))
        self._truth = self._rest = None

    def truth(self):
        if self._truth is None:
            self._truth = pr.pillar_encode_ref(self.vox, self.num, self.coors, pr.PILLAR_GEOM, self.layers, self.wd)
        return self._truth

    def restated(self):
        if self._rest is None:
            self._rest = pr.pillar_encode_ref(self.vox, self.num, self.coors, pr.PILLAR_GEOM, self.layers, self.wd, dtype=np.float32)
        return self._rest

    def run(self, hip, n_dev=None, out_dtype=torch.float32, rows=None):
        sl = slice(None) if rows is None else rows
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda")
        return hip.pillar_encode(_dev(self.vox[sl]), _dev(self.num[sl]), _dev(self.coors[sl]), nd, pr.PILLAR_GEOM,
                                 [tuple(_dev(a) for a in l) for l in self.layers], with_distance=self.wd, out_dtype=out_dtype)

    def name(self):
        return "pillar_encode %s wd=%d M=%d P=%d ndim=%d" % ("x".join(map(str, self.units)), self.wd, self.M, self.P, self.ndim)


@pytest.fixture(scope="module")
def cache():
    """Cases shared by the tests of this module: each is built by whichever test asks for it first and never changed afterwards."""
    c = {}
    yield c
    c.clear()


def _case(cache, key, wd, M, P=20, ndim=5):
    k = (key, wd, M, P, ndim)
    if k not in cache:
        cache[k] = _Case(DISPATCH[key], wd, M, P, ndim, _seed(len(key), DISPATCH[key][0], wd, M, P, ndim))
    return cache[k]


# ================================================================================================ reader
@pytest.mark.parametrize("wd", [False, True], ids=["plain", "dist"])
@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_every_dispatch_P_by_ndim(hip, cache, key, wd):
    """P x ndim for one instantiation, M = 7 (no multiple of the 4 waves of a workgroup): P below G, P no multiple of G, kMaxP;
    ndim at both limits.  num_points is 1, P and in between; masked rows win the max on the large-shift units."""
    masked_wins = 0
    for P in P_VALUES:
        for ndim in NDIM_VALUES:
            c = _case(cache, key, wd, 7, P, ndim)
            assert set(c.num[:2]) == {1, P} and c.num.min() >= 1 and c.num.max() <= P
            got = _np(c.run(hip))
            pr.rule(c.name(), got, c.restated(), c.truth())
            if len(c.units) == 1:
                relu_shift = np.maximum(c.layers[0][2], 0)
                win = (c.num < P)[:, None] & (got == relu_shift[None, :]) & (relu_shift > 1)[None, :]
                assert np.array_equal(win, (c.num < P)[:, None] & (c.truth() == relu_shift.astype(np.float64)[None, :]) & (relu_shift > 1)[None, :])
                masked_wins += int(win.sum())
                assert (got[:, 2::4] == 0).any()  # negative-shift units clip to exactly 0 somewhere
    assert len(c.units) == 2 or masked_wins > 20


@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_few_pillars(hip, cache, key):
    """M = 1, 4, 5: one live wave, exactly one workgroup, one workgroup and a quarter."""
    for M in (1, 4, 5):
        for wd in (False, True):
            c = _case(cache, key, wd, M)
            pr.rule(c.name(), _np(c.run(hip)), c.restated(), c.truth())


@pytest.mark.parametrize("key", ["two", "u16"])
def test_reader_second_grid_stride_iteration(hip, cache, key):
    """M = 8192 + 5: the grid is capped at 2048 workgroups of 4 waves, so the last 5 pillars are a second loop iteration in which
    workgroup 0 is full, workgroup 1 has one live wave and every other wave only arrives at the barriers.  Every row against the
    reference; rows 8192.. bit for bit against the same pillars placed first in a call of their own; two runs bit-identical."""
    c = _case(cache, key, False, 8192 + 5)
    out = c.run(hip)
    got = _np(out)
    pr.rule(c.name(), got, c.restated(), c.truth())
    pr.rule(c.name() + " rows 8192..", got[8192:], c.restated()[8192:], c.truth()[8192:])
    first = _np(c.run(hip, rows=slice(8192, None)))
    assert first.shape == (5, c.units[-1])
    assert np.array_equal(first.view(np.uint32), got[8192:].view(np.uint32))
    assert torch.equal(out, c.run(hip))


@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_device_count(hip, cache, key):
    """n_dev below M: rows past it stay zero and the rows before it are those of the full call; above M: clamped to M; 0: nothing."""
    c = _case(cache, key, True, 37)
    full = c.run(hip)
    pr.rule(c.name(), _np(full), c.restated(), c.truth())
    assert bool((full != 0).any(1).all())
    for n in (36, 33, 5, 1):
        part = c.run(hip, n_dev=n)
        assert torch.equal(part[:n], full[:n]) and bool((part[n:] == 0).all())
    for n in (38, 37 + 8192, 2 ** 31 - 1):
        assert torch.equal(c.run(hip, n_dev=n), full)
    assert bool((c.run(hip, n_dev=0) == 0).all())
    assert bool((c.run(hip, n_dev=0, out_dtype=torch.bfloat16) == 0).all())


@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_bf16_output_is_the_rounded_fp32_output(hip, cache, key):
    """The bf16 output equals the fp32 output of the same call rounded to nearest-even, bit for bit (rounding built in numpy on the
    uint32 view); also in the second grid-stride iteration's rows of the M = 8197 case."""
    cases = [_case(cache, key, wd, 37) for wd in (False, True)] + [_case(cache, key, False, 7, P, 8) for P in (1, 3, 32)]
    if key in ("two", "u16"):
        cases.append(_case(cache, key, False, 8192 + 5))
    for c in cases:
        f32, bf = c.run(hip), c.run(hip, out_dtype=torch.bfloat16)
        assert bf.dtype == torch.bfloat16 and bf.shape == f32.shape
        assert np.array_equal(_bits(bf), fr.bf16_rne_bits(_np(f32))), c.name()
        assert (_bits(bf) & 1).any() and (_np(f32).view(np.uint32) & 0xFFFF).any()


F_CANARY, BF_CANARY = -7.5, 0x4242


@pytest.mark.parametrize("out_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_out_stride_through_c_abi(hip, cache, key, out_dtype):
    """fd_pillar_encode with out_stride = U + 8 into a canary-filled buffer: the U columns are those of the dense call, the 8 extra
    columns of every row and the rows past a device count stay untouched."""
    from futuredet_amd import lib

    L = lib.load()
    c = _case(cache, key, True, 37)
    U, M = c.units[-1], c.M
    tdt = torch.float32 if out_dtype == "f32" else torch.bfloat16
    dense = c.run(hip, out_dtype=tdt)
    layers = [tuple(_dev(a) for a in l) for l in c.layers] + [(None, None, None)]
    (w1, s1, b1), (w2, s2, b2) = layers[0], layers[1]
    vox, num, coors = _dev(c.vox), _dev(c.num), _dev(c.coors)
    g = pr.PILLAR_GEOM
    for n in (None, 30):
        if out_dtype == "f32":
            buf = torch.full((M, U + 8), F_CANARY, dtype=tdt, device="cuda")
        else:
            buf = _bf16_dev(np.full((M, U + 8), BF_CANARY, np.uint16))
        nd = None if n is None else torch.tensor([n], dtype=torch.int32, device="cuda")
        hip.check(L.fd_pillar_encode(hip._p(vox), hip._p(num), hip._p(coors), hip._p(nd), M, c.P, c.ndim, 1, g[0], g[1], g[2], g[3],
                                     hip._p(w1), hip._p(s1), hip._p(b1), w1.shape[0], hip._p(w2), hip._p(s2), hip._p(b2),
                                     w2.shape[0] if w2 is not None else 0, 0 if out_dtype == "f32" else 1, hip._p(buf), U + 8, hip._stream()),
                  "fd_pillar_encode")
        k = M if n is None else n
        assert torch.equal(buf[:k, :U], dense[:k])
        if out_dtype == "f32":
            assert bool((buf[:, U:] == F_CANARY).all()) and bool((buf[k:] == F_CANARY).all())
        else:
            assert np.all(_bits(buf[:, U:]) == BF_CANARY) and np.all(_bits(buf[k:]) == BF_CANARY)


@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_two_runs_are_bit_identical(hip, cache, key):
    c = _case(cache, key, False, 301, 31, 8)
    a, b = c.run(hip), c.run(hip)
    assert torch.equal(a, b)
    pr.rule(c.name(), _np(a), c.restated(), c.truth())


@pytest.mark.parametrize("key", list(DISPATCH))
def test_reader_empty_pillar_is_the_all_masked_value(hip, key):
    """num_points == 0 (the voxelizer never emits one; the reference gives NaN): the kernel's mean divides by zero, but every row
    is masked by a select, so the pillar comes out finite and equal to what zero rows give: relu(shift) fed through the layers.  With
    one layer that is relu(shift) exactly; the pillars around it are unaffected."""
    rng = np.random.default_rng(_seed(99, DISPATCH[key][0], len(key)))
    units = DISPATCH[key]
    vox, num, coors = pr.make_pillars(rng, 6, 20, 5)
    layers = pr.make_layers(rng, units, 10)
    num[1] = num[4] = 0
    vox[1] = 0.0                       # as a voxelizer would leave an unused slot; pillar 4 keeps its (ignored) rows
    got = _np(hip.pillar_encode(_dev(vox), _dev(num), _dev(coors), None, pr.PILLAR_GEOM, [tuple(_dev(a) for a in l) for l in layers]))
    assert np.isfinite(got).all()
    zeros = np.zeros((2, 20, 10))
    want, rest = pr.pfn_layers_ref(zeros, layers), pr.pfn_layers_ref(zeros, layers, np.float32)
    pr.rule("pillar_encode %s num_points == 0" % key, got[[1, 4]], rest, want)
    if len(units) == 1:
        assert np.array_equal(got[1], np.maximum(layers[0][2], 0)) and np.array_equal(got[4], got[1])
    live = [0, 2, 3, 5]
    truth = pr.pillar_encode_ref(vox[live], num[live], coors[live], pr.PILLAR_GEOM, layers, False)
    rest = pr.pillar_encode_ref(vox[live], num[live], coors[live], pr.PILLAR_GEOM, layers, False, dtype=np.float32)
    pr.rule("pillar_encode %s next to empty pillars" % key, got[live], rest, truth)


# ================================================================================================ scatter
NY, NX = 5, 7
SCATTER_C = (1, 3, 64, 65)


def _scatter_input(C, B, in_dtype, seed, M=23):
    """M rows in distinct cells of a (B, ., NY, NX) canvas, with three rows in their middle that must be skipped (b = B, y = -1,
    x = NX).  The values carry bf16 ties, +-inf, +-0, a quiet NaN and the largest float.  -> (device rows, float32 host values, coors4)"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(B * NY * NX, M, replace=False)
    coors = np.stack([cells // (NY * NX), np.zeros(M, np.int64), (cells // NX) % NY, cells % NX], 1).astype(np.int32)
    coors = np.concatenate([coors[:5], np.array([[B, 0, 1, 1], [0, 0, -1, 2], [B - 1, 0, 2, NX]], np.int32), coors[5:]])
    f = rng.standard_normal((len(coors), C)).astype(np.float32)
    probe = fr.bf16_probe_values(rng, n_random=20)
    k = min(f.size, len(probe))
    f.reshape(-1)[:k] = probe[len(probe) - k:]   # (C = 1: the special values land in the last, valid rows)
    if in_dtype == "bf16":
        bits = fr.bf16_rne_bits(f)
        return _bf16_dev(bits), _bf16_as_f32(bits), coors
    return _dev(f), f, coors


def _canary_canvas(B, C, out_dtype, channels_last):
    """(buf [B + 2, C, NY, NX] canary-filled, canvas = buf[1:1 + B])"""
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    if out_dtype == "f32":
        buf = torch.full((B + 2, C, NY, NX), F_CANARY, dtype=torch.float32, device="cuda").contiguous(memory_format=fmt)
    else:
        buf = _bf16_dev(np.full((B + 2, C, NY, NX), BF_CANARY, np.uint16)).contiguous(memory_format=fmt)
    canvas = buf[1:1 + B]
    assert canvas.is_contiguous(memory_format=fmt)
    return buf, canvas


def _assert_canvas(buf, canvas, ref):
    """canvas == ref bit for bit (bf16: the numpy round-to-nearest-even of ref), the samples around it keep their canary"""
    if canvas.dtype == torch.float32:
        assert np.array_equal(_np(canvas).view(np.uint32), ref.view(np.uint32))
        assert bool((buf[0] == F_CANARY).all()) and bool((buf[-1] == F_CANARY).all())
    else:
        assert np.array_equal(_bits(canvas), fr.bf16_rne_bits(ref))
        assert np.all(_bits(buf[0]) == BF_CANARY) and np.all(_bits(buf[-1]) == BF_CANARY)


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("out_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
def test_scatter_every_dtype_pair_layout_and_width(hip, in_dtype, out_dtype, channels_last):
    """One pillar_scatter instantiation and layout over C = 1, 3, 64, 65 on a (2, C, 5, 7) canvas that is a slice of a canary-filled
    buffer; rows outside the canvas are skipped, cells nobody names are exactly zero.  (1, 3, 5, 7) in bf16 is 210 bytes: the
    hipMemsetAsync branch of the zero fill (every other canvas here is a whole number of words)."""
    for B, C in [(2, c) for c in SCATTER_C] + [(1, 3)]:
        feats, host, coors = _scatter_input(C, B, in_dtype, seed=C + 10 * B)
        nbytes = B * C * NY * NX * (2 if out_dtype == "bf16" else 4)
        assert (nbytes % 4 == 2) == (B == 1 and out_dtype == "bf16")
        buf, canvas = _canary_canvas(B, C, out_dtype, channels_last)
        ref = pr.pillar_scatter_ref(host, coors, len(coors), B, NY, NX)
        assert np.isnan(ref).any() and np.isinf(ref).any() and (ref == 0).any()
        got = hip.pillar_scatter(feats, _dev(coors), None, B, NY, NX, out=canvas)
        assert got.data_ptr() == canvas.data_ptr()
        _assert_canvas(buf, canvas, ref)
    # without ``out``: the wrapper's own allocation, in the asked-for layout and dtype
    feats, host, coors = _scatter_input(64, 2, in_dtype, seed=5)
    tdt = torch.float32 if out_dtype == "f32" else torch.bfloat16
    got = hip.pillar_scatter(feats, _dev(coors), None, 2, NY, NX, out_dtype=tdt, channels_last=channels_last)
    assert got.dtype == tdt and got.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    ref = pr.pillar_scatter_ref(host, coors, len(coors), 2, NY, NX)
    if out_dtype == "f32":
        assert np.array_equal(_np(got).view(np.uint32), ref.view(np.uint32))
    else:
        assert np.array_equal(_bits(got), fr.bf16_rne_bits(ref))


@pytest.mark.parametrize("in_dtype", ["f32", "bf16"])
def test_scatter_rows_of_a_wider_buffer_through_c_abi(hip, in_dtype):
    """feats as columns 2..2+C of a [M, C + 5] buffer (feat_stride > C): the columns around the slice are never read into the canvas."""
    from futuredet_amd import lib

    L = lib.load()
    B = 2
    for C in (3, 64):
        feats, host, coors = _scatter_input(C + 5, B, in_dtype, seed=40 + C)
        for out_dtype in ("f32", "bf16"):
            buf, canvas = _canary_canvas(B, C, out_dtype, False)
            view = feats[:, 2:2 + C]
            assert view.stride(0) == C + 5 and not view.is_contiguous()
            sb, sc, sy, sx = canvas.stride()
            hip.check(L.fd_pillar_scatter(hip._p(view), C, C + 5, 0 if in_dtype == "f32" else 1, hip._p(_dev(coors)), None, len(coors), B, NY, NX,
                                          hip._p(canvas), 0 if out_dtype == "f32" else 1, sb, sc, sy, sx, 1, hip._stream()), "fd_pillar_scatter")
            _assert_canvas(buf, canvas, pr.pillar_scatter_ref(np.ascontiguousarray(host[:, 2:2 + C]), coors, len(coors), B, NY, NX))


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_scatter_sample_by_sample_without_zeroing(hip, channels_last):
    """detectors.py's per-sample calls: zero_first only on the first call, each call with its own rows and device count, into one
    canvas -- equal to the single call over all rows."""
    B, C, cap = 3, 65, 12
    rng = np.random.default_rng(12)
    counts = [9, 0, 12]
    coors = np.zeros((B * cap, 4), np.int32)
    for b in range(B):
        cells = rng.choice(NY * NX, cap, replace=False)
        coors[b * cap:(b + 1) * cap] = np.stack([np.full(cap, b), np.zeros(cap, np.int64), cells // NX, cells % NX], 1)
    feats = rng.standard_normal((B * cap, C)).astype(np.float32)
    live = np.concatenate([np.arange(b * cap, b * cap + counts[b]) for b in range(B)])
    ref = pr.pillar_scatter_ref(feats[live], coors[live], len(live), B, NY, NX)
    buf, canvas = _canary_canvas(B, C, "f32", channels_last)
    dfeats, dcoors, dcounts = _dev(feats), _dev(coors), _dev(np.array(counts, np.int32))
    for b in range(B):
        sl = slice(b * cap, (b + 1) * cap)
        hip.pillar_scatter(dfeats[sl], dcoors[sl], dcounts[b:b + 1], B, NY, NX, out=canvas, zero_first=(b == 0))
    _assert_canvas(buf, canvas, ref)
    single = hip.pillar_scatter(_dev(feats[live]), _dev(coors[live]), None, B, NY, NX, channels_last=channels_last)
    assert torch.equal(single, canvas)
    # zero_first=False alone leaves every cell it does not name as it was
    buf2, canvas2 = _canary_canvas(B, C, "f32", channels_last)
    hip.pillar_scatter(dfeats[:cap], dcoors[:cap], dcounts[:1], B, NY, NX, out=canvas2, zero_first=False)
    keep = pr.pillar_scatter_ref(np.ones((counts[0], C), np.float32), coors[:counts[0]], counts[0], B, NY, NX) == 0
    assert np.all(_np(canvas2)[keep] == F_CANARY) and np.array_equal(_np(canvas2)[~keep], ref[~keep])


@pytest.mark.parametrize("out_dtype", ["f32", "bf16"])
def test_scatter_device_count_and_no_rows(hip, out_dtype):
    B, C = 2, 3
    feats, host, coors = _scatter_input(C, B, "f32", seed=77)
    dcoors = _dev(coors)
    for n in (0, 1, 11, len(coors), len(coors) + 1000, 2 ** 31 - 1):
        buf, canvas = _canary_canvas(B, C, out_dtype, True)
        hip.pillar_scatter(feats, dcoors, torch.tensor([n], dtype=torch.int32, device="cuda"), B, NY, NX, out=canvas)
        _assert_canvas(buf, canvas, pr.pillar_scatter_ref(host, coors, n, B, NY, NX))
    # M = 0: the canvas is zeroed and nothing else happens
    buf, canvas = _canary_canvas(B, C, out_dtype, False)
    hip.pillar_scatter(feats[:0], dcoors[:0], None, B, NY, NX, out=canvas)
    _assert_canvas(buf, canvas, np.zeros((B, C, NY, NX), np.float32))
