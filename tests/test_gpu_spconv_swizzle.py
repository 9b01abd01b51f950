"""Bank-spread rows between two sparse-convolution kernels (fd_spconv_apply_layout): 16-byte piece s of row r is stored at piece
s ^ (r & 7) of its 128-byte line, so that a gather of 16 different rows at one channel offset does not queue on one bank.  The layout
only moves bytes: with the input / residual permuted in torch (hip_ops.swizzle_rows) and the output permuted back, every launch must
carry the bits of the plain launch -- per shape, row count, layout word, with and without residual / ReLU / a device row count; a
level chain and a whole run_fused with the flags it sets equal the plain ones; everything else refuses the word."""
import ctypes

import numpy as np
import pytest
import torch

from parity_util import report

pytestmark = pytest.mark.gpu

# (cin, cout): the SubM shapes take every bit, the strided shapes into a level the residual / output bits
SUBM = [(32, 32), (64, 64), (128, 128)]
STRIDED = [(16, 32), (32, 64), (64, 128)]
N_OUT = [1, 9, 129, 257, 1000]  # one row, the row & 7 wrap, a second chunk, a third chunk, a range of several chunks


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _table(rng, n_in, n_out, cap, n_dev):
    """A K = 27 table made by hand: about half the neighbours missing, capacity columns past n_out hold rows that must never be read"""
    stride = (cap + 63) // 64 * 64
    t = np.where(rng.random((27, stride)) < 0.5, rng.integers(0, n_in, (27, stride)), -1).astype(np.int32)
    nbr = _dev(t)
    nbr.n_out = cap
    if n_dev:
        nbr.n_dev = torch.tensor([n_out], dtype=torch.int32, device="cuda")
        nbr.n_expected = n_out
    return nbr


def _layer(hip, cin, cout, n_in, n_out, seed):
    rng = np.random.default_rng(seed)
    x = _dev(rng.standard_normal((n_in, cin)).astype(np.float32))
    w = (rng.standard_normal((27, cin, cout)) * np.sqrt(2.0 / (27 * cin))).astype(np.float32)
    return rng, x, hip.pack_spconv_weight(torch.from_numpy(w)).cuda(), _dev(rng.standard_normal(cout).astype(np.float32))


def _check_layouts(hip, cin, cout, n_in, n_out, layouts_plain, layouts_res, seed):
    rng, x, wpk, bias = _layer(hip, cin, cout, n_in, n_out, seed)
    xs = hip.swizzle_rows(x)
    n_launch = 0
    for n_dev in (False, True):
        cap = n_out + 37 if n_dev else n_out  # a device row count below the capacity
        nbr = _table(rng, n_in, n_out, cap, n_dev)
        res = _dev(rng.standard_normal((cap, cout)).astype(np.float32))
        res_s = hip.swizzle_rows(res)
        for with_res in (False, True):
            kw = dict(residual=res, relu=True) if with_res else dict()
            ref = hip.spconv_apply(x, wpk, bias, nbr, cap, cout, **kw)
            for lay in (layouts_res if with_res else layouts_plain):
                if with_res:
                    kw["residual"] = res_s if lay & 2 else res
                y = hip.spconv_apply(xs if lay & 1 else x, wpk, bias, nbr, cap, cout, layout=lay, **kw)
                y = hip.swizzle_rows(y) if lay & 4 else y
                assert torch.equal(y[:n_out], ref[:n_out]), "%d->%d, %d rows, layout %d, residual %r, device count %r" % (
                    cin, cout, n_out, lay, with_res, n_dev)
                n_launch += 1
    return n_launch


@pytest.mark.parametrize("n_out", N_OUT)
@pytest.mark.parametrize("c", [c for c, _ in SUBM])
def test_subm_layer_every_layout_word(hip, c, n_out):
    n = _check_layouts(hip, c, c, n_out, n_out, [0, 1, 4, 5], list(range(8)), 100 * c + n_out)
    report("spconv %d->%d, %d rows: %d launches over every layout word equal the plain launch" % (c, c, n_out, n), 0.0, 0.0)


@pytest.mark.parametrize("n_out", N_OUT)
@pytest.mark.parametrize("cin,cout", STRIDED)
def test_strided_layer_output_and_residual_bits(hip, cin, cout, n_out):
    """n_in != n_out; the input of the strided layer is the previous level's plain output, so bit 0 is never valid here"""
    n = _check_layouts(hip, cin, cout, 2 * n_out + 3, n_out, [0, 4], [0, 2, 4, 6], 7 * cin + n_out)
    report("spconv %d->%d, %d rows: %d launches with the output / residual bits equal the plain launch" % (cin, cout, n_out, n), 0.0, 0.0)


def test_the_kernels_really_use_the_layout(hip):
    """A launch told that plain input rows are bank-spread must give something else (the flag is not ignored), for every SubM shape"""
    for c, _ in SUBM:
        rng, x, wpk, bias = _layer(hip, c, c, 300, 300, c)
        nbr = _table(rng, 300, 300, 300, False)
        ref = hip.spconv_apply(x, wpk, bias, nbr, 300, c)
        assert not torch.equal(hip.spconv_apply(x, wpk, bias, nbr, 300, c, layout=1), ref)
        assert not torch.equal(hip.spconv_apply(x, wpk, bias, nbr, 300, c, layout=4), ref)


def _pyramid(hip, n_target, seed):
    """two index levels of a small grid (stride 2) with n_target active input sites"""
    rng = np.random.default_rng(seed)
    B, D, H, W = 2, 9, 24, 24
    flat = rng.choice(B * D * H * W, size=n_target, replace=False)
    idx = np.stack(np.unravel_index(flat, (B, D, H, W)), 1).astype(np.int32)
    src = hip.SparseIndex(B, D, H, W, torch.device("cuda"))
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    src.mark(_dev(idx))
    src.scan(counts[0:1])
    dst = src.downsample((3, 3, 3), (2, 2, 2), (1, 1, 1))
    dst.scan(counts[1:2])
    host = counts.cpu()
    src.finalize(int(host[0]))
    dst.finalize(int(host[1]))
    return rng, src, dst


@pytest.mark.parametrize("cin,cout", STRIDED)
def test_level_chain_with_the_flags_of_run_fused(hip, cin, cout):
    """strided conv + two residual blocks on real rulebooks (plans straight from the index where the library wants them), with the
    layout words run_fused sets -- output only, then input + output, input + residual + output, and the last launch with a plain
    output -- against the plain chain"""
    rng, src, dst = _pyramid(hip, 3000, cin)
    assert src.n != dst.n and dst.n > 257
    x0 = _dev(rng.standard_normal((src.n, cin)).astype(np.float32))
    mk = lambda ci: hip.pack_spconv_weight(torch.from_numpy((rng.standard_normal((27, ci, cout)) * np.sqrt(2.0 / (27 * ci))).astype(np.float32))).cuda()  # noqa: E731
    ws = [mk(cin)] + [mk(cout) for _ in range(4)]
    bias = _dev(rng.standard_normal(cout).astype(np.float32))

    def chain(swz):
        down = src.rulebook(dst, (3, 3, 3), (2, 2, 2), (1, 1, 1), fp32_layer=(cin, cout))
        subm = dst.rulebook(dst, (3, 3, 3), (1, 1, 1), (1, 1, 1), fp32_layer=(cout, cout))
        x = hip.spconv_apply(x0, ws[0], bias, down, dst.n, cout, relu=True, layout=4 if swz else 0)
        for b in range(2):
            y = hip.spconv_apply(x, ws[1 + 2 * b], bias, subm, dst.n, cout, relu=True, layout=5 if swz else 0)
            x = hip.spconv_apply(y, ws[2 + 2 * b], bias, subm, dst.n, cout, residual=x, relu=True, layout=(7 if b == 0 else 3) if swz else 0)
        return x

    assert torch.equal(chain(True), chain(False))
    report("level chain %d->%d (%d -> %d rows): bank-spread inner tensors, plain result" % (cin, cout, src.n, dst.n), 0.0, 0.0)


def _detector(variant="forecast_n0", seed=7):
    from futuredet_amd import build_detector
    from futuredet_amd.configs import centerpoint_config
    from futuredet_amd.synth import seeded_state_dict, tame_box_dims

    cfg = centerpoint_config(variant, "car")
    net = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    net.load_state_dict(tame_box_dims(seeded_state_dict(net, seed)), strict=False)
    return cfg, net.cuda().eval()


def _knob(hip, value, fn):
    hip.set_tuning("spconv_swz", value)
    try:
        return fn()
    finally:
        hip.set_tuning("spconv_swz", 0)


def test_run_fused_knob_on_and_off(hip):
    """run_fused on two small clouds with every level bank-spread (knob 7) and with none (-1): the BEV map and every level's rows
    are the same bits -- what leaves a level is plain either way"""
    from futuredet_amd.synth import synthetic_cloud

    import futuredet_amd.detectors as D

    cfg, net = _detector()
    bb = net.backbone
    clouds = [_dev(synthetic_cloud(seed=s_, target_points=p_)) for s_, p_ in ((3, 4000), (4, 6000))]
    stage, no_graph = {}, D._NO_GRAPH
    net.__dict__["debug_taps"], D._NO_GRAPH = stage, True  # (neck + head eagerly: only the backbone's inputs are wanted)
    try:
        with torch.no_grad():
            net.forward_points(clouds, cfg.voxel_generator, padded="packed")
    finally:
        net.__dict__["debug_taps"], D._NO_GRAPH = None, no_graph
    idx, x0 = stage["idx"], stage["feats0"].clone()
    assert idx[1].n > 257 and idx[3].n > 129, [i.n for i in idx]

    def run():
        with torch.no_grad():
            bev, levels = bb.run_fused(idx, x0)
        return [bev.clone()] + [levels[l][0].clone() for l in sorted(levels)]

    on = _knob(hip, 7, run)
    off = _knob(hip, -1, run)
    assert len(on) == len(off) == 6
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    report("run_fused: bev and %d levels identical with bank-spread inner tensors on / off" % (len(on) - 1), 0.0, 0.0)


def test_captured_static_step_equals_the_eager_pass(hip):
    """A captured sweep with the layout on replays the detections of the same step with it off, and of its own eager re-run: the
    30k-point cloud overflows capacities taken from the small cloud's warm-up, so the step runs it eagerly"""
    from futuredet_amd.detectors import StaticStep
    from futuredet_amd.synth import synthetic_cloud

    cfg, net = _detector()
    small, big = [_dev(synthetic_cloud(seed=s, target_points=p)) for s, p in ((12, 6000), (11, 30000))]

    def sweep():
        step = StaticStep(net, cfg.voxel_generator, capacity=32768, row_caps="auto")
        outs = []
        with torch.no_grad():
            step.warm_up([small])
            for c in (small, big, small):
                got = step([c])
                torch.cuda.synchronize()
                assert step.graph is not None
                outs.append([t.clone() for t in got[:4]] + [step.level_counts.clone(), step.overflowed()])
        return outs

    on = _knob(hip, 7, sweep)
    off = _knob(hip, -1, sweep)
    assert any(o[5] for o in on), "one of the clouds must take the eager re-run"
    for a, b in zip(on, off):
        for u, v in zip(a[:5], b[:5]):
            assert torch.equal(u, v)
        assert a[5] == b[5]
    report("static step: captured and eager passes identical with the layout on / off", 0.0, 0.0)


def test_everything_else_is_unaffected_or_refuses(hip):
    from futuredet_amd import lib

    L = lib.load()
    rng, x, wpk, bias = _layer(hip, 16, 16, 200, 200, 5)
    nbr = _table(rng, 200, 200, 200, False)
    ref = hip.spconv_apply(x, wpk, bias, nbr, 200, 16)
    # layout 0 through the new entry point is the plain launch
    out = torch.empty_like(ref)
    rc = L.fd_spconv_apply_layout(_p(x), 200, _p(wpk), _p(bias), None, 0, _p(nbr), nbr.shape[1], None, 0, 27, 200, None, 0, 16, 16, 0, _p(out),
                                  None, 0, 0, None)
    assert rc == 0 and torch.equal(out, ref)
    # 16-channel rows are never spread; shapes without an instantiation and bf16 refuse, and nothing is written
    for cin, cout, dt, lay in [(16, 16, 0, 1), (16, 16, 0, 4), (16, 32, 0, 1), (32, 64, 0, 1), (64, 128, 0, 5), (32, 16, 0, 4), (32, 32, 1, 7),
                               (64, 64, 1, 1), (32, 32, 0, 8)]:
        xi = torch.zeros((200, cin), dtype=torch.float32 if dt == 0 else torch.bfloat16, device="cuda")
        wi = hip.pack_spconv_weight(torch.zeros((27, cin, cout)), xi.dtype).cuda()
        sentinel = torch.full((200, cout), 7.0, dtype=xi.dtype, device="cuda")
        rc = L.fd_spconv_apply_layout(_p(xi), 200, _p(wi), None, None, 0, _p(nbr), nbr.shape[1], None, 0, 27, 200, None, 0, cin, cout, dt,
                                      _p(sentinel), None, 0, lay, None)
        torch.cuda.synchronize()
        assert rc != 0 and b"fd_spconv_apply_layout" in L.fd_last_error(), (cin, cout, dt, lay)
        assert bool((sentinel == 7.0).all()), "a refused launch must write nothing"
    # the 32-pair kernel switched off: 32 -> 32 has no bank-spread gather left and refuses; the knob answers accordingly
    hip.set_tuning("spconv_c32", -1)
    try:
        assert L.fd_spconv_layout_wanted(32, 32, 0) == 0
        x32 = torch.zeros((200, 32), device="cuda")
        w32 = hip.pack_spconv_weight(torch.zeros((27, 32, 32))).cuda()
        with pytest.raises(Exception):
            hip.spconv_apply(x32, w32, None, nbr, 200, 32, layout=1)
    finally:
        hip.set_tuning("spconv_c32", 0)
    assert L.fd_spconv_layout_wanted(64, 64, 1) == 0 and L.fd_spconv_layout_wanted(16, 16, 0) == 0
    assert _knob(hip, -1, lambda: [L.fd_spconv_layout_wanted(c, c, 0) for c in (32, 64, 128)]) == [0, 0, 0]
    assert _knob(hip, 2, lambda: [L.fd_spconv_layout_wanted(*s, 0) for s in ((32, 32), (64, 64), (32, 64), (16, 32))]) == [0, 7, 4, 0]
