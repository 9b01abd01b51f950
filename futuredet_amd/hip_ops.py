"""Torch-tensor front end of the C ABI (include/futuredet_hip.h).  Tensors are device memory plumbing only:
every function passes raw pointers + the current HIP stream to libfuturedet_hip.so.  No CPU fallbacks."""
import ctypes
import threading

import numpy as np
import torch

from . import lib as _lib
from .lib import DecodeCfg, FutureDetHipError, MapView, check


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter is ~20x cheaper than building a
    torch.cuda.Stream object; this is called once per library launch)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise FutureDetHipError("%s must be a tensor on the HIP device (got %s); this path has no CPU implementation"
                                % (name, "cpu tensor" if isinstance(t, torch.Tensor) else type(t)))
    if dtype is not None and t.dtype != dtype:
        raise FutureDetHipError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise FutureDetHipError("%s must be contiguous" % name)
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Workspace(object):
    """Grow-only per-(tag, device, owner) scratch buffers so steady-state steps do no allocation.  The owner is the current
    stream -- sweeps in flight on different streams (bench.py --inflight, serving) must not share scratch memory -- or, inside
    ``with workspace.scope(token)``, the token: a captured whole-sweep graph keeps scratch of its own whatever stream it was
    captured on (torch hands out streams from a pool, so two captures can meet on one stream handle)."""

    def __init__(self):
        self._bufs = {}
        self._scope = threading.local()

    def scope(self, token):
        ws = self

        class _Scope(object):
            def __enter__(self_):
                self_.prev = getattr(ws._scope, "token", None)
                ws._scope.token = token

            def __exit__(self_, *exc):
                ws._scope.token = self_.prev

        return _Scope()

    def release(self, token):
        """Drops the buffers of a scope (the owner of the token is going away)."""
        for key in [k for k in self._bufs if k[2] == ("scope", token)]:
            del self._bufs[key]

    def get(self, tag, nbytes, device):
        token = getattr(self._scope, "token", None)
        key = (tag, device.index, ("scope", token) if token is not None else _stream().value)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


workspace = _Workspace()
_DT = {torch.float32: 0, torch.bfloat16: 1}


def set_tuning(name, value):
    """fd_tuning_set: kernel-variant knobs for tuning runs and for the tests that compare variants (0 = heuristic)."""
    check(_lib.load().fd_tuning_set(name.encode(), int(value)), "fd_tuning_set")


# ------------------------------------------------------------------------------------------------ voxelizer
def voxelize(points, voxel_size, coors_range, max_points, max_voxels, batch_idx=0, want_voxels=True, want_mean=False,
             mean_stride=None, coor_cols=3, out=None, n_points_dev=None):
    """Runs fd_voxelize on device points [N, ndim] float32.  Returns a dict of capacity-sized device tensors
    (voxels / mean / coors / num_points) plus ``num_voxels`` (device int32[1]); nothing is synchronised.
    ``out`` may supply pre-allocated (sliced) destination tensors with the same keys.  ``n_points_dev`` (device int32[1]):
    only the first min(N, n_points_dev[0]) rows are points, the rest is padding of a fixed-capacity buffer."""
    L = _lib.load()
    points = _dev(points, "points", torch.float32)
    n, ndim = points.shape
    dev = points.device
    rng = (ctypes.c_float * 6)(*[float(np.float32(v)) for v in coors_range])
    vs = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in voxel_size])
    out = dict(out or {})
    if want_voxels and "voxels" not in out:
        out["voxels"] = torch.empty((max_voxels, max_points, ndim), dtype=torch.float32, device=dev)
    if want_mean and "mean" not in out:
        out["mean"] = torch.empty((max_voxels, mean_stride or ndim), dtype=torch.float32, device=dev)
    if "coors" not in out:
        out["coors"] = torch.empty((max_voxels, coor_cols), dtype=torch.int32, device=dev)
    if "num_points" not in out:
        out["num_points"] = torch.empty((max_voxels,), dtype=torch.int32, device=dev)
    if "num_voxels" not in out:
        out["num_voxels"] = torch.zeros((1,), dtype=torch.int32, device=dev)
    mean = out.get("mean") if want_mean else None
    voxels = out.get("voxels") if want_voxels else None
    ws_bytes = L.fd_voxelize_workspace_bytes(n, max_voxels)
    ws = workspace.get("voxelize", ws_bytes, dev)
    check(L.fd_voxelize(_p(points), n, _p(n_points_dev), ndim, rng, vs, int(max_points), int(max_voxels), int(batch_idx), _p(voxels), _p(mean),
                        int(mean.shape[1]) if mean is not None else 0, _p(out["coors"]), int(out["coors"].shape[1]),
                        _p(out["num_points"]), _p(out["num_voxels"]), _p(ws), ws.numel(), _stream()), "fd_voxelize")
    return out


# ------------------------------------------------------------------------------------------------ sparse index
class SparseIndex(object):
    """Active set on a (B, D, H, W) grid: column occupancy words + prefix counts (+ coords once counted)."""

    def __init__(self, B, D, H, W, device, words=None, prefix=None):
        L = _lib.load()
        self.B, self.D, self.H, self.W = int(B), int(D), int(H), int(W)
        self.ncols = L.fd_index_num_cols(self.B, self.H, self.W)
        self.words = torch.zeros((self.ncols,), dtype=torch.int64, device=device) if words is None else words
        self.prefix = torch.empty((self.ncols,), dtype=torch.int32, device=device) if prefix is None else prefix
        self.n_dev = None     # device int32[1] view
        self.n = None         # host int, set by finalize() (static indexes: the row CAPACITY)
        self.coords = None    # [n,4] int32 (b,z,y,x), rows in index order
        self.device = device
        self.static = False   # True: the count stays on the device (n_dev); n is a capacity, n_expected a typical count
        self.n_expected = 0

    @property
    def spatial_shape(self):
        return [self.D, self.H, self.W]

    def mark(self, coords, n_dev=None, n_max=None):
        L = _lib.load()
        coords = _dev(coords, "coords", torch.int32)
        n_max = coords.shape[0] if n_max is None else n_max
        check(L.fd_index_mark(_p(coords), _p(n_dev), n_max, self.B, self.D, self.H, self.W, _p(self.words), _stream()),
              "fd_index_mark")

    def scan(self, n_dev):
        L = _lib.load()
        ws = workspace.get("index_scan", L.fd_index_workspace_bytes(self.ncols), self.device)
        self.n_dev = n_dev
        check(L.fd_index_scan(_p(self.words), self.ncols, _p(self.prefix), _p(n_dev), _p(ws), ws.numel(), _stream()),
              "fd_index_scan")

    def downsample(self, ksize, stride, pad):
        L = _lib.load()
        od = [(i + 2 * p - (k - 1) - 1) // s + 1 for i, k, s, p in zip(self.spatial_shape, ksize, stride, pad)]
        out = SparseIndex(self.B, od[0], od[1], od[2], self.device)
        check(L.fd_index_downsample(_p(self.words), self.B, self.D, self.H, self.W, (ctypes.c_int * 3)(*ksize),
                                    (ctypes.c_int * 3)(*stride), (ctypes.c_int * 3)(*pad), _p(out.words), _stream()),
              "fd_index_downsample")
        return out

    def finalize(self, n):
        """Called once the host knows the active count: materialises coords."""
        L = _lib.load()
        self.n = int(n)
        self.coords = torch.empty((max(self.n, 1), 4), dtype=torch.int32, device=self.device)[: self.n]
        if self.n:
            check(L.fd_index_coords(_p(self.words), _p(self.prefix), self.B, self.D, self.H, self.W, _p(self.coords),
                                    _stream()), "fd_index_coords")

    def lookup(self, coords, n_dev=None):
        L = _lib.load()
        coords = _dev(coords, "coords", torch.int32)
        row_of = torch.empty((coords.shape[0],), dtype=torch.int32, device=self.device)
        check(L.fd_index_lookup(_p(self.words), _p(self.prefix), self.B, self.D, self.H, self.W, _p(coords), _p(n_dev),
                                coords.shape[0], _p(row_of), _stream()), "fd_index_lookup")
        return row_of

    def rulebook(self, out_index, ksize, stride, pad, fp32_layer=None):
        """nbr [K, stride64] int32: input row (in self) feeding each output row of ``out_index`` per tap.
        ``fp32_layer = (cin, cout)``: the table is for fp32 inference launches of that (padded) shape only; where their kernels read
        nothing but a chunk plan (index_plan_wanted) an IndexRulebook comes back instead and no table is built."""
        L = _lib.load()
        assert out_index.n is not None
        if fp32_layer is not None and index_plan_wanted(self, out_index, ksize, *fp32_layer):
            return IndexRulebook(self, out_index, stride, pad)
        K = int(ksize[0] * ksize[1] * ksize[2])
        nstride = max(64, (out_index.n + 63) // 64 * 64)
        nbr = torch.empty((K, nstride), dtype=torch.int32, device=self.device)
        static = getattr(out_index, "static", False)
        if out_index.n == 0:
            nbr.fill_(-1)
            return nbr
        # static indexes: the table has the level's row capacity; only the device's count of rows is written (and read)
        check(L.fd_rulebook(_p(self.words), _p(self.prefix), self.B, self.D, self.H, self.W, _p(out_index.coords), out_index.n,
                            _p(out_index.n_dev), nstride, 0 if static else 1, (ctypes.c_int * 3)(*ksize), (ctypes.c_int * 3)(*stride),
                            (ctypes.c_int * 3)(*pad), _p(nbr), _stream()), "fd_rulebook")
        nbr.n_out = out_index.n
        nbr.n_dev = out_index.n_dev if static else None
        nbr.n_expected = out_index.n_expected if static else 0
        # the INPUT level's count: what the transposed table of a strided layer's input gradient runs on
        src_static = getattr(self, "static", False)
        nbr.n_in_dev = self.n_dev if src_static else None
        nbr.n_in_expected = self.n_expected if src_static else 0
        return nbr


def index_plan_wanted(src, dst, ksize, cin, cout):
    """True when fp32 launches of a cin -> cout layer from index ``src`` to ``dst`` run on a chunk plan made straight from the index
    (fd_spconv_index_plan_wanted; 3 x 3 x 3 windows; input rows within the 32-bit gather offsets of the kernels that read a plan)."""
    return (tuple(int(k) for k in ksize) == (3, 3, 3) and bool(dst.n) and bool(src.n) and src.n < (1 << 23) and src.n * cin * 4 < (1 << 31)
            and bool(_lib.load().fd_spconv_index_plan_wanted(int(cin), int(cout), 0)))


def swizzle_rows(t):
    """The bank-spread layout of fd_spconv_apply_layout, stated in torch: 16-byte piece s of row r of an fp32 [n, c] tensor at piece
    s ^ (r & 7) of its 128-byte line; rows of fewer than 32 channels stay as they are.  Its own inverse.  (Tests and tools: the
    kernels read and write the layout themselves.)"""
    n, c = t.shape
    if c < 32 or n == 0:
        return t.clone()
    assert t.dtype == torch.float32 and c % 32 == 0
    r = torch.arange(n, device=t.device) & 7
    idx = torch.arange(8, device=t.device)[None, :] ^ r[:, None]
    return torch.gather(t.reshape(n, c // 32, 8, 4), 2, idx[:, None, :, None].expand(n, c // 32, 8, 4)).reshape(n, c)


def level_layout(cin, cout, n_in, n_out):
    """True when the inner tensors of a sparse level -- strided cin -> cout convolution from n_in to n_out rows, then cout -> cout SubM
    layers -- are to be stored bank-spread (fd_spconv_layout_wanted; fp32, row counts within the 32-bit gather offsets of the kernels
    that read such rows: the launches of a larger level fall back to kernels that only know plain rows)."""
    L = _lib.load()
    fits = lambda n, c: 0 < n < (1 << 23) and n * c * 4 < (1 << 31)  # noqa: E731
    return bool(fits(n_in, cin) and fits(n_out, cout) and L.fd_spconv_layout_wanted(int(cout), int(cout), 0) == 7
                and L.fd_spconv_layout_wanted(int(cin), int(cout), 0) & 4)


class IndexRulebook(object):
    """Stands where the K = 27 table of SparseIndex.rulebook would on the fp32 inference sweep: the two indexes and the window, from
    which plans_from_index / ranges_for write the chunk plans and the equal-work ranges that the kernels read.  Carries the table's
    attributes (shape, n_out, n_dev, n_expected, ranges, plans), so row_split / plan_for / spconv_apply take it as they take a table;
    ``table()`` builds the dense table after all, for a caller that needs one (a launch no plan-reading kernel takes)."""

    def __init__(self, src, dst, stride, pad):
        static = getattr(dst, "static", False)
        self.src, self.dst, self.stride, self.pad = src, dst, tuple(int(v) for v in stride), tuple(int(v) for v in pad)
        self.shape = (27, max(64, (dst.n + 63) // 64 * 64))
        self.device = src.device
        self.n_out = dst.n
        self.n_dev = dst.n_dev if static else None
        self.n_expected = dst.n_expected if static else 0
        self.ranges, self.plans, self._table = None, {}, None

    def table(self):
        if self._table is None:
            self._table = self.src.rulebook(self.dst, (3, 3, 3), self.stride, self.pad)
        return self._table


def plans_from_index(requests):
    """One fd_spconv_plan_from_index launch for ``requests`` = [(IndexRulebook, ranges, n_ranges)] (the row splits of the launches that
    will read the plans, see row_split); the plans are cached on the rulebooks as plan_for caches them.  Returns the plan tensors."""
    L = _lib.load()
    todo = [(rb, r, int(n), (r.data_ptr() if r is not None else 0, int(n), int(rb.n_out))) for rb, r, n in requests]
    todo = [t for t in todo if t[3] not in t[0].plans]
    out = []
    for at in range(0, len(todo), 8):
        part = todo[at:at + 8]
        srcs = (_lib.PlanSource * len(part))()
        for s, (rb, ranges, n_ranges, key) in zip(srcs, part):
            pstride = int(L.fd_spconv_plan_stride(rb.n_out))
            plan = torch.empty((28, pstride), dtype=torch.int32, device=rb.device)
            s.in_words, s.in_prefix, s.out_coords = rb.src.words.data_ptr(), rb.src.prefix.data_ptr(), rb.dst.coords.data_ptr()
            s.n_out_dev = rb.n_dev.data_ptr() if rb.n_dev is not None else None
            s.ranges = ranges.data_ptr() if ranges is not None else None
            s.plan, s.n_out, s.plan_stride = plan.data_ptr(), rb.n_out, pstride
            s.Din, s.Hin, s.Win, s.n_ranges = rb.src.D, rb.src.H, rb.src.W, n_ranges
            s.stride[:], s.pad[:] = list(rb.stride), list(rb.pad)
            rb.plans[key] = (plan, pstride, ranges)  # (the range table stays alive with the plan cut for it)
            out.append(plan)
        check(L.fd_spconv_plan_from_index(part[0][0].src.B, len(part), srcs, _stream()), "fd_spconv_plan_from_index")
    return out


class _PyramidPlan(object):
    """Static part of build_pyramid for one (B, shape, geometry): level shapes, one words / prefix allocation for all
    levels, the fd_index_level array.  Reused across sweeps so a step pays one memset and two library calls."""

    def __init__(self, B, shape0, geoms, device):
        L = _lib.load()
        self.B, self.geoms, self.device = int(B), geoms, device
        self.shapes = [tuple(int(v) for v in shape0)]
        for ks, st, pd in geoms:
            self.shapes.append(tuple((i + 2 * p - (k - 1) - 1) // s + 1 for i, k, s, p in zip(self.shapes[-1], ks, st, pd)))
        self.ncols = [L.fd_index_num_cols(self.B, sh[1], sh[2]) for sh in self.shapes]
        self.ws_bytes = L.fd_index_workspace_bytes(sum(self.ncols) + 2048 * len(self.ncols))  # block sums of all levels at once

    def row_caps(self, cap0):
        """Upper bounds of the active rows per level given at most ``cap0`` rows on level 0: a strided convolution turns one
        input into at most prod(ceil(k / s)) outputs (the taps k with (p + pad - k) % s == 0), and a level cannot have more
        rows than cells."""
        caps = [min(int(cap0), self.B * int(np.prod(self.shapes[0])))]
        for (ks, st, pd), sh in zip(self.geoms, self.shapes[1:]):
            fan = int(np.prod([-(-k // s) for k, s in zip(ks, st)]))
            caps.append(min(caps[-1] * fan, self.B * int(np.prod(sh))))
        return caps


_pyramid_plans = {}


def build_pyramid(coors, nvox, n_max, B, shape0, geoms, device, static=False, expected=None, row_caps=None):
    """All sparse indexes of the backbone with two library calls and ONE host read: level 0 (D,H,W = shape0) marked
    from the voxelizer output ``coors`` [B*n_max, 4] / ``nvox`` [B]; level l from level l-1 by geoms[l-1] =
    (ksize, stride, pad).  Returns the list of finalised SparseIndex (coords materialised).
    ``static=True``: NO host read -- every level gets its row capacity (_PyramidPlan.row_caps) as ``n``, the counts stay in
    ``n_dev`` and ``expected`` (typical counts, e.g. of an earlier sweep) only steers launch heuristics.  ``row_caps`` (one
    per level) replaces the data-free capacities by smaller ones (a high-water mark with head room): every kernel then works on
    min(capacity, count) rows, and a sweep whose count exceeds a capacity is DETECTABLE -- counts[l] > capacity -- but not
    computed correctly; the caller re-runs it on the eager path (detectors.StaticStep does)."""
    L = _lib.load()
    key = (int(B), tuple(int(v) for v in shape0), tuple((tuple(k), tuple(s), tuple(p)) for k, s, p in geoms), str(device))
    plan = _pyramid_plans.get(key)
    if plan is None:
        plan = _pyramid_plans[key] = _PyramidPlan(B, shape0, geoms, device)
    shapes, ncols = plan.shapes, plan.ncols
    # fresh buffers every sweep (the indexes are handed out and may outlive the call); fd_index_pyramid clears level 0 itself and
    # overwrites the other levels
    words_all = torch.empty((sum(ncols),), dtype=torch.int64, device=device)
    prefix_all = torch.empty((sum(ncols),), dtype=torch.int32, device=device)
    counts = torch.empty((len(shapes),), dtype=torch.int32, device=device)
    idx, off = [], 0
    levels = (_lib.IndexLevel * len(shapes))()
    wp, pp = words_all.data_ptr(), prefix_all.data_ptr()
    for l, (sh, nc) in enumerate(zip(shapes, ncols)):
        ix = SparseIndex.__new__(SparseIndex)
        ix.B, ix.D, ix.H, ix.W, ix.ncols, ix.device = plan.B, sh[0], sh[1], sh[2], nc, device
        ix.words, ix.prefix = words_all[off:off + nc], prefix_all[off:off + nc]
        ix.n_dev, ix.n, ix.coords = counts[l:l + 1], None, None
        ix.level_counts = counts  # all levels' counts in one tensor (n_dev is the slice of this level)
        ix.static, ix.n_expected = False, 0
        lv = levels[l]
        lv.D, lv.H, lv.W = sh
        if l:
            ks, st, pd = geoms[l - 1]
            lv.ksize[:], lv.stride[:], lv.pad[:] = list(ks), list(st), list(pd)
        lv.words, lv.prefix, lv.coords = wp + 8 * off, pp + 4 * off, None
        idx.append(ix)
        off += nc
    ws = workspace.get("index_scan", plan.ws_bytes, device)

    def size_coords(host):
        total = sum(host)
        coords_all = torch.empty((max(total, 1), 4), dtype=torch.int32, device=device)
        o = 0
        for l, ix in enumerate(idx):
            ix.n = int(host[l])
            ix.coords = coords_all[o:o + ix.n]
            levels[l].coords = (coords_all.data_ptr() + 16 * o) if ix.n else None
            levels[l].coords_rows = ix.n
            o += ix.n

    if static:
        host = plan.row_caps(int(B) * int(n_max))
        if row_caps is not None:
            host = [min(int(a), int(b)) for a, b in zip(host, row_caps)]
        for l, ix in enumerate(idx):
            ix.static = True
            ix.n_expected = int(expected[l]) if expected is not None else 0
        # capacities are known before the scan: the coordinate tables go in with the levels and the scan writes them in its last pass
        size_coords(host)
        fused = all(int(h) > 0 for h in host)
        check(L.fd_index_pyramid(_p(coors), _p(nvox), int(n_max), plan.B, len(shapes), levels, _p(counts), _p(ws), ws.numel(), _stream()),
              "fd_index_pyramid")
        if not fused:
            check(L.fd_index_pyramid_coords(plan.B, len(shapes), levels, _stream()), "fd_index_pyramid_coords")
        return idx
    check(L.fd_index_pyramid(_p(coors), _p(nvox), int(n_max), plan.B, len(shapes), levels, _p(counts), _p(ws), ws.numel(), _stream()),
          "fd_index_pyramid")
    size_coords(counts.tolist())  # the only synchronisation of the backbone
    check(L.fd_index_pyramid_coords(plan.B, len(shapes), levels, _stream()), "fd_index_pyramid_coords")
    return idx


def ranges_for(nbr, cin, cout):
    """Work-balanced row ranges of a rulebook for the fp32 kernel (fd_spconv_ranges); computed once per rulebook and
    shared by every convolution that reuses it.  Returns (ranges int32[n+1], n) or (None, n) for an equal-rows split."""
    cached = getattr(nbr, "ranges", None)
    if cached is not None:
        return cached
    L = _lib.load()
    n_out = getattr(nbr, "n_out", None)
    if not n_out:
        return None, 0
    K, nstride = nbr.shape
    n = int(L.fd_spconv_num_ranges(getattr(nbr, "n_expected", 0) or n_out, cin, cout, 0))
    if n <= 0:
        return None, 0
    ranges = torch.empty((n + 1,), dtype=torch.int32, device=nbr.device)
    ws = workspace.get("spconv_ranges", L.fd_spconv_ranges_workspace_bytes(n_out), nbr.device)
    if isinstance(nbr, IndexRulebook):  # (a SubM level's: src is dst)
        ix = nbr.dst
        check(L.fd_spconv_ranges_from_index(_p(ix.words), ix.B, ix.D, ix.H, ix.W, _p(ix.coords), n_out, _p(nbr.n_dev), n, _p(ranges), _p(ws),
                                            ws.numel(), _stream()), "fd_spconv_ranges_from_index")
    else:
        check(L.fd_spconv_ranges(_p(nbr), nstride, K, n_out, _p(getattr(nbr, "n_dev", None)), n, _p(ranges), _p(ws), ws.numel(), _stream()),
              "fd_spconv_ranges")
    nbr.ranges = (ranges, n)
    return nbr.ranges


def row_split(nbr, n_out, cin, cout, balanced=None):
    """(ranges, n_ranges) of an fp32 launch: the kernel walks row ranges.  The MFMA-bound SubM layers (Cout >= 64; their rulebook is
    shared by the 4-5 convolutions of a level) get equal-WORK ranges from fd_spconv_ranges; narrow layers and strided convolutions
    (rulebook used once) take equal row counts -- see fd_spconv_num_ranges for the measurements."""
    L = _lib.load()
    if balanced is None:
        balanced = nbr.shape[0] == 27 and cin == cout and bool(L.fd_spconv_wants_balanced_ranges(cin, cout, 0))
    if balanced == "tiles":      # one 128-row tile per workgroup (tuning comparisons)
        return None, 0
    if balanced:
        return ranges_for(nbr, cin, cout)
    return None, int(L.fd_spconv_num_ranges(getattr(nbr, "n_expected", 0) or n_out, cin, cout, 0))


def plan_for(nbr, n_out, ranges, n_ranges):
    """Chunk plan of a SubM rulebook (fd_spconv_plan_build): the compacted pair lists of every 128-row chunk, written once per
    rulebook and row split and shared by the convolutions that reuse the rulebook.  Sized by the rulebook's row capacity, no host
    read.  Returns (plan int32[28, stride], stride)."""
    key = (ranges.data_ptr() if ranges is not None else 0, int(n_ranges), int(n_out))
    if isinstance(nbr, IndexRulebook):
        assert int(n_out) == nbr.n_out
        plans_from_index([(nbr, ranges, n_ranges)])
        return nbr.plans[key][:2]
    plans = getattr(nbr, "plans", None)
    if plans is None:
        plans = nbr.plans = {}
    if key not in plans:
        L = _lib.load()
        K, nstride = nbr.shape
        pstride = int(L.fd_spconv_plan_stride(n_out))
        plan = torch.empty((28, pstride), dtype=torch.int32, device=nbr.device)
        check(L.fd_spconv_plan_build(_p(nbr), nstride, K, n_out, _p(getattr(nbr, "n_dev", None)), _p(ranges), int(n_ranges), _p(plan), pstride,
                                     _stream()), "fd_spconv_plan_build")
        plans[key] = (plan, pstride, ranges)  # (the range table stays alive with the plan cut for it)
    return plans[key][:2]


def rows_permute(src, row_of, c_dst, dtype=torch.float32, n_rows=None, n_dev=None):
    L = _lib.load()
    src = _dev(src, "src", torch.float32)
    row_of = _dev(row_of, "row_of", torch.int32)
    n_rows = src.shape[0] if n_rows is None else n_rows
    dst = torch.zeros((max(n_rows, 1), c_dst), dtype=dtype, device=src.device)[:n_rows]
    if src.shape[0]:
        check(L.fd_rows_permute(_p(src), src.shape[1], _p(row_of), _p(n_dev), src.shape[0], _p(dst), c_dst,
                                _DT[dtype], _stream()), "fd_rows_permute")
    return dst


def rows_place(index, coords, src, c_dst, dtype=torch.float32, n_dev=None, out=None):
    """fd_rows_place: dst[row of coords[i] in ``index``][:] = src[i][:] (channels >= src.shape[1] zeroed) for the first
    min(len(coords), n_dev[0]) voxels; a coordinate that is not in the index is skipped.  ``out``: pre-allocated [rows, c_dst]
    destination of ``dtype`` (otherwise zeros [index.n, c_dst]); rows that no voxel maps to are left as they are."""
    L = _lib.load()
    coords = _dev(coords, "coords", torch.int32)
    src = _dev(src, "src", torch.float32)
    if out is None:
        out = torch.zeros((max(index.n, 1), c_dst), dtype=dtype, device=src.device)[: index.n]
    _dev(out, "out", dtype)
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise FutureDetHipError("rows_place: coords must be [n, 4] (b, z, y, x), got %s" % (tuple(coords.shape),))
    if src.dim() != 2 or src.shape[0] < coords.shape[0]:
        raise FutureDetHipError("rows_place: src must be [n, c_src] with a row per coordinate")
    if out.dim() != 2 or out.shape[1] != c_dst or index.n is None or out.shape[0] < index.n:
        raise FutureDetHipError("rows_place: out must be [rows >= index.n, %d] (finalised index), got %s" % (c_dst, tuple(out.shape)))
    check(L.fd_rows_place(_p(index.words), _p(index.prefix), index.B, index.D, index.H, index.W, _p(coords), _p(n_dev),
                          coords.shape[0], _p(src), src.shape[1], _p(out), c_dst, _DT[dtype], _stream()), "fd_rows_place")
    return out


# ------------------------------------------------------------------------------------------------ sparse conv
def pack_spconv_weight(w_kio, dtype=torch.float32):
    """[K, Cin, Cout] float32 (host or device) -> fragment-ordered packed weights on the same device."""
    L = _lib.load()
    dev = w_kio.device
    w = w_kio.detach().to("cpu", torch.float32).contiguous()
    K, cin, cout = w.shape
    nbytes = L.fd_spconv_packed_weight_bytes(K, cin, cout, _DT[dtype])
    host = torch.empty((nbytes,), dtype=torch.uint8)
    check(L.fd_spconv_pack_weight(ctypes.c_void_p(w.data_ptr()), K, cin, cout, _DT[dtype], ctypes.c_void_p(host.data_ptr())),
          "fd_spconv_pack_weight")
    return host.to(dev)


PACK_PLAIN, PACK_TRANSPOSED, PACK_FLIPPED_TRANSPOSED = 0, 1, 2  # fd_spconv_pack_weight_device modes: W[k], W[k]^T, W[K-1-k]^T
# per row dtype: the device packer, and (entry point, workspace function, workspace tag) of the weight gradient
_PACK_DEVICE = {torch.float32: "fd_spconv_pack_weight_device", torch.bfloat16: "fd_spconv_pack_weight_device_bf16"}
_WGRAD = {torch.float32: ("fd_spconv_wgrad", "fd_spconv_wgrad_workspace_bytes", "spconv_wgrad"),
          torch.bfloat16: ("fd_spconv_wgrad_bf16", "fd_spconv_wgrad_bf16_workspace_bytes", "spconv_wgrad_bf16")}


def pack_spconv_weight_device(w_kio, mode=PACK_PLAIN, dtype=torch.float32):
    """[K, Cin, Cout] float32 on the device -> fragment-ordered weights of ``dtype`` (fd_spconv_pack_weight byte for byte) of W[k], or, for
    the input gradient, of W[k]^T / W[K-1-k]^T (a Cout -> Cin problem).  No host round trip."""
    L = _lib.load()
    if dtype not in _DT:
        raise FutureDetHipError("pack_spconv_weight_device: dtype must be float32 or bfloat16 (got %s)" % (dtype,))
    w = _dev(w_kio.detach(), "w_kio", torch.float32)
    K, cin, cout = w.shape
    ci, co = (cout, cin) if mode else (cin, cout)
    out = torch.empty((L.fd_spconv_packed_weight_bytes(K, ci, co, _DT[dtype]),), dtype=torch.uint8, device=w.device)
    name = _PACK_DEVICE[dtype]
    check(getattr(L, name)(_p(w), K, cin, cout, int(mode), _p(out), _stream()), name)
    return out


def spconv_wgrad(feats, dy, nbr, n_out):
    """dW[k] = sum_o feats[nbr[k][o]]^T dy[o] -> [K, Cin, Cout] float32 (deterministic; fd_spconv_wgrad for float32 rows,
    fd_spconv_wgrad_bf16 for bfloat16 rows -- feats and dy in the same one of the two)."""
    L = _lib.load()
    if feats.dtype != dy.dtype or feats.dtype not in _DT:
        raise FutureDetHipError("spconv_wgrad: feats and dy must both be float32 or both bfloat16 (got %s and %s)" % (feats.dtype, dy.dtype))
    feats = _dev(feats, "feats")
    dy = _dev(dy, "dy")
    K, nstride = nbr.shape
    cin, cout = feats.shape[1], dy.shape[1]
    assert dy.shape[0] >= n_out
    dw = torch.empty((K, cin, cout), dtype=torch.float32, device=feats.device)
    name, ws_bytes, tag = _WGRAD[feats.dtype]
    ws = workspace.get(tag, getattr(L, ws_bytes)(K, n_out, cin, cout), feats.device)
    check(getattr(L, name)(_p(feats), feats.shape[0], _p(dy), _p(_dev(nbr, "nbr", torch.int32)), nstride, K, n_out,
                           _p(getattr(nbr, "n_dev", None)), cin, cout, _p(dw), _p(ws), ws.numel(), _stream()), name)
    return dw


def assign_targets(boxes, counts, classes, trajectory, cfg, out):
    """AssignLabel's targets of a batch (fd_assign_targets): boxes [B, T, n_max, 12] fp32, counts [B, T] int32, classes / trajectory
    [B, T, n_max] int32 (trajectory None: standard set only, cfg.n_sets must be 1); ``cfg`` a lib.TargetsCfg with T and n_max set;
    ``out`` the flat buffers of TargetAssigner.outputs (hm, ind, mask, cat, anno_box, gt_boxes_and_cls, status), all overwritten."""
    L = _lib.load()
    boxes = _dev(boxes, "boxes", torch.float32)
    B = boxes.shape[0]
    assert tuple(boxes.shape) == (B, cfg.T, cfg.n_max, 12), (tuple(boxes.shape), cfg.T, cfg.n_max)
    assert tuple(counts.shape) == (B, cfg.T) and tuple(classes.shape) == (B, cfg.T, cfg.n_max)
    assert (trajectory is None) == (cfg.n_sets == 1)
    if trajectory is not None:
        assert tuple(trajectory.shape) == (B, cfg.T, cfg.n_max)
        trajectory = _dev(trajectory, "trajectory", torch.int32)
    U = cfg.n_tasks + (2 if cfg.n_sets == 3 else 0)
    ws = workspace.get("targets", L.fd_targets_workspace_bytes(B, cfg.T, U, cfg.max_objs), boxes.device)
    check(L.fd_assign_targets(_p(boxes), _p(_dev(counts, "counts", torch.int32)), _p(_dev(classes, "classes", torch.int32)), _p(trajectory), B,
                              ctypes.byref(cfg), _p(_dev(out["hm"], "hm", torch.float32)), _p(_dev(out["ind"], "ind", torch.int64)),
                              _p(_dev(out["mask"], "mask", torch.uint8)), _p(_dev(out["cat"], "cat", torch.int64)),
                              _p(_dev(out["anno_box"], "anno_box", torch.float32)), _p(_dev(out["gt_boxes_and_cls"], "gt_boxes_and_cls", torch.float32)),
                              _p(_dev(out["status"], "status", torch.int32)), _p(ws), ws.numel(), _stream()), "fd_assign_targets")
    return out


def rulebook_transpose(nbr, n_out, n_in):
    """Input-stationary table inv[k][i] = o of an output-stationary rulebook ([K, stride64(n_in)] int32, -1 where no pair)."""
    L = _lib.load()
    K, nstride = nbr.shape
    istride = max(64, (n_in + 63) // 64 * 64)
    inv = torch.empty((K, istride), dtype=torch.int32, device=nbr.device)
    check(L.fd_rulebook_transpose(_p(_dev(nbr, "nbr", torch.int32)), nstride, K, n_out, _p(getattr(nbr, "n_dev", None)), n_in, _p(inv),
                                  istride, _stream()), "fd_rulebook_transpose")
    return inv


def dense_gather(grad, index, c):
    """Backward of densify: [n, c] rows of ``grad`` ([B, c*D, H, W], any element strides) at the index's active cells."""
    L = _lib.load()
    if not (isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype == torch.float32):
        raise FutureDetHipError("dense_gather: grad must be a float32 tensor on the HIP device")
    n = int(index.n)
    feats = torch.empty((max(n, 1), c), dtype=torch.float32, device=grad.device)[:n]
    sb, sc, sy, sx = grad.stride()
    check(L.fd_dense_gather(_p(grad), sb, sc, sy, sx, index.D, _p(index.coords), n, _p(index.n_dev if index.static else None), c,
                            _p(feats), _stream()), "fd_dense_gather")
    return feats


def spconv_apply(feats, wpacked, bias, nbr, n_out, cout, residual=None, relu=False, out=None, balanced=None, plan=None, layout=0):
    """``layout``: which tensors are stored bank-spread (fd_spconv_apply_layout: 1 the input rows, 2 the residual, 4 the output)."""
    L = _lib.load()
    feats = _dev(feats, "feats")
    dt = _DT[feats.dtype]
    cin = feats.shape[1]
    out_dtype, out_cols = feats.dtype, cout
    from_index = isinstance(nbr, IndexRulebook)
    if from_index and (plan is False or dt != 0 or n_out != nbr.n_out or not index_plan_wanted(nbr.src, nbr.dst, (3, 3, 3), cin, cout)):
        nbr, from_index = nbr.table(), False  # not a launch that runs on a plan alone: the dense table after all
    K, nstride = nbr.shape
    if out is None:
        out = torch.empty((max(n_out, 1), out_cols), dtype=out_dtype, device=feats.device)[:n_out]
    if residual is not None:
        _dev(residual, "residual", out_dtype)
    n_dev, n_expected = getattr(nbr, "n_dev", None), getattr(nbr, "n_expected", 0)  # static index: n_out is a capacity
    ranges, n_ranges = row_split(nbr, n_out, cin, cout, balanced) if dt == 0 and n_out > 0 else (None, 0)
    # fp32 SubM layers from 32 channels up: the rulebook's chunk plan (plan_for), cut for this launch's row split and shared by the
    # convolutions of the level.  ``plan=False`` (the training path) keeps the in-kernel compaction; the results are the same bits.
    # An IndexRulebook has no table at all: its plan comes straight from the index, for the strided 16 -> 32 ... 64 -> 128 layers too.
    if plan is None:
        plan = from_index or (dt == 0 and n_out > 0 and K == 27 and cin == cout and bool(L.fd_spconv_plan_wanted(cin, cout, 0)))
    if layout:
        plan_t, pstride = plan_for(nbr if from_index else _dev(nbr, "nbr", torch.int32), n_out, ranges, n_ranges) if plan else (None, 0)
        check(L.fd_spconv_apply_layout(_p(feats), feats.shape[0], _p(_dev(wpacked, "wpacked")), _p(bias), _p(residual), int(bool(relu)),
                                       None if from_index else _p(_dev(nbr, "nbr", torch.int32)), nstride, _p(ranges), n_ranges, K, n_out,
                                       _p(n_dev), int(n_expected or 0), cin, cout, dt, _p(out), _p(plan_t), pstride, int(layout), _stream()),
              "fd_spconv_apply_layout")
        return out
    if plan:
        plan_t, pstride = plan_for(nbr if from_index else _dev(nbr, "nbr", torch.int32), n_out, ranges, n_ranges)
        check(L.fd_spconv_apply_plan(_p(feats), feats.shape[0], _p(_dev(wpacked, "wpacked")), _p(bias), _p(residual), int(bool(relu)),
                                     None if from_index else _p(nbr), nstride, _p(ranges), n_ranges, K, n_out, _p(n_dev), int(n_expected or 0),
                                     cin, cout, dt, _p(out), _p(plan_t), pstride, _stream()),
              "fd_spconv_apply_plan")
        return out
    check(L.fd_spconv_apply(_p(feats), feats.shape[0], _p(_dev(wpacked, "wpacked")), _p(bias), _p(residual), int(bool(relu)),
                            _p(_dev(nbr, "nbr", torch.int32)), nstride, _p(ranges), n_ranges, K, n_out, _p(n_dev), int(n_expected or 0),
                            cin, cout, dt, _p(out), _stream()),
          "fd_spconv_apply")
    return out


def densify(feats, index, out_dtype=None, channels_last=False, out=None):
    """SparseConvTensor.dense()+view: [B, C*D, H, W] with channel = c*D + d (``out``: pre-allocated destination)."""
    L = _lib.load()
    feats = _dev(feats, "feats")
    C = feats.shape[1]
    shape = (index.B, C * index.D, index.H, index.W)
    if out is None:
        out_dtype = out_dtype or feats.dtype
        out = torch.empty(shape, dtype=out_dtype, device=feats.device,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    else:
        assert tuple(out.shape) == shape and out.is_cuda
        out_dtype = out.dtype
    sb, sc, sy, sx = out.stride()
    check(L.fd_densify(_p(feats), C, _DT[feats.dtype], _p(index.words), _p(index.prefix), index.B, index.D, index.H,
                       index.W, _p(out), _DT[out_dtype], sb, sc, sy, sx, int(feats.shape[0]), _stream()), "fd_densify")
    return out


# ------------------------------------------------------------------------------------------------ dense conv (bf16)
def pack_conv2d_weight(w_oihw):
    """[Cout, Cin, k, k] float32 -> MFMA-fragment-ordered bf16 weights on the same device."""
    L = _lib.load()
    dev = w_oihw.device
    w = w_oihw.detach().to("cpu", torch.float32).contiguous()
    cout, cin, ks, _ = w.shape
    nbytes = L.fd_conv2d_packed_weight_bytes(cout, cin, ks)
    if nbytes == 0:
        raise FutureDetHipError("fd_conv2d: unsupported weight shape %s" % (tuple(w.shape),))
    host = torch.empty((nbytes,), dtype=torch.uint8)
    check(L.fd_conv2d_pack_weight(ctypes.c_void_p(w.data_ptr()), cout, cin, ks, ctypes.c_void_p(host.data_ptr())),
          "fd_conv2d_pack_weight")
    return host.to(dev)


def conv2d_nhwc_bf16(x, wpk, bias, cout, ks, stride=1, relu=True, out=None, co_off=0, osy=1, osx=1, ooy=0, oox=0):
    """x [B,H,W,Cin] bf16 contiguous -> y [B,Ho*osy,Wo*osx,Ctot] bf16 (allocated when ``out`` is None)."""
    L = _lib.load()
    x = _dev(x, "x", torch.bfloat16)
    B, H, W, cin = x.shape
    pad = 1 if ks == 3 else 0
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty((B, Ho * osy, Wo * osx, cout), dtype=torch.bfloat16, device=x.device)
    _dev(out, "out", torch.bfloat16)
    check(L.fd_conv2d_nhwc_bf16(_p(x), B, H, W, cin, _p(wpk), _p(bias), cout, ks, stride, pad, int(bool(relu)), _p(out),
                                out.shape[3], co_off, osy, osx, ooy, oox, _stream()), "fd_conv2d_nhwc_bf16")
    return out


def pack_conv2d_weight_device(w, transposed=False):
    """[Cout, Cin, k, k] float32 on the device -> pack_conv2d_weight's bytes, packed on the device (fd_conv2d_pack_weight_dev: one
    launch, no host round trip).  ``transposed``: the weights of the input gradient, w'[ci][co][k-1-ky][k-1-kx] = w[co][ci][ky][kx]
    (a Cout -> Cin convolution; needs Cout % 32 == 0)."""
    L = _lib.load()
    w = _dev(w.detach(), "w", torch.float32)
    if w.dim() != 4 or w.shape[2] != w.shape[3]:
        raise FutureDetHipError("pack_conv2d_weight_device: need a [Cout, Cin, k, k] weight (got %s)" % (tuple(w.shape),))
    cout, cin, ks, _ = w.shape
    if transposed and cout % 32:
        raise FutureDetHipError("pack_conv2d_weight_device: the transposed weights need Cout %% 32 == 0 (got %s)" % (tuple(w.shape),))
    nbytes = L.fd_conv2d_packed_weight_bytes(cin, cout, ks) if transposed else L.fd_conv2d_packed_weight_bytes(cout, cin, ks)
    if nbytes == 0:
        raise FutureDetHipError("fd_conv2d: unsupported weight shape %s" % (tuple(w.shape),))
    out = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    check(L.fd_conv2d_pack_weight_dev(_p(w), cout, cin, ks, int(bool(transposed)), _p(out), _stream()), "fd_conv2d_pack_weight_dev")
    return out


def conv2d_wgrad_bf16_chunk():
    """Pixels per partial of conv2d_wgrad_bf16: a constant of the library, part of its summation order."""
    return int(_lib.load().fd_conv2d_wgrad_bf16_chunk())


def conv2d_wgrad_bf16(x_nhwc, dy_nhwc, ks):
    """Weight gradient of the stride-1 convolution y = conv(x, w) (padding 1 for ks 3, 0 for ks 1): x [B,H,W,Cin] and dy [B,H,W,Cout] bf16
    contiguous -> dW [Cout, Cin, ks, ks] float32 (fd_conv2d_wgrad_bf16: deterministic, no atomics)."""
    L = _lib.load()
    x = _dev(x_nhwc, "x_nhwc", torch.bfloat16)
    dy = _dev(dy_nhwc, "dy_nhwc", torch.bfloat16)
    if x.dim() != 4 or dy.dim() != 4 or x.shape[:3] != dy.shape[:3]:
        raise FutureDetHipError("conv2d_wgrad_bf16: x [B,H,W,Cin] and dy [B,H,W,Cout] must cover the same pixels (got %s and %s)"
                                % (tuple(x.shape), tuple(dy.shape)))
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    nbytes = L.fd_conv2d_wgrad_bf16_workspace_bytes(B, H, W, cin, cout, ks)
    if nbytes == 0:
        raise FutureDetHipError("conv2d_wgrad_bf16: unsupported problem %s -> %d channels, ks %s" % (tuple(x.shape), cout, ks))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=x.device)
    check(L.fd_conv2d_wgrad_bf16(_p(x), _p(dy), B, H, W, cin, cout, ks, _p(ws), ws.numel(), _p(dw), _stream()), "fd_conv2d_wgrad_bf16")
    return dw


# ------------------------------------------------------------------------------------------------ strided dense conv (bf16 training)
def _map4(t, name):
    t = _dev(t, name, torch.bfloat16)
    if t.dim() != 4:
        raise FutureDetHipError("%s must be a [B, H, W, C] map (got %s)" % (name, tuple(t.shape)))
    return t


def _out_map(out, shape, like, name):
    """``out`` checked against ``shape``, or a new bf16 tensor of that shape on ``like``'s device"""
    if out is None:
        return torch.empty(shape, dtype=torch.bfloat16, device=like.device)
    _dev(out, name, torch.bfloat16)
    if tuple(out.shape) != tuple(shape):
        raise FutureDetHipError("%s must be %s (got %s)" % (name, tuple(shape), tuple(out.shape)))
    return out


def conv2d_s2_dgrad_bf16(dy_nhwc, wpk_t, H, W, cin, out=None):
    """Input gradient of the 3 x 3 / stride 2 / padding 1 convolution of an [B, H, W, cin] map: dy [B, (H-1)//2+1, (W-1)//2+1, Cout] bf16
    and ``wpk_t`` = pack_conv2d_weight_device(w, transposed=True) -> dx [B, H, W, cin] bf16, every element written
    (fd_conv2d_s2_dgrad_bf16)."""
    L = _lib.load()
    dy = _map4(dy_nhwc, "dy_nhwc")
    B, Ho, Wo, cout = dy.shape
    if H < 1 or W < 1 or (Ho, Wo) != ((H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise FutureDetHipError("conv2d_s2_dgrad_bf16: dy %s is not the stride-2 map of %d x %d" % (tuple(dy.shape), H, W))
    _dev(wpk_t, "wpk_t", torch.uint8)
    if wpk_t.numel() != L.fd_conv2d_packed_weight_bytes(cin, cout, 3) or wpk_t.numel() == 0:
        raise FutureDetHipError("conv2d_s2_dgrad_bf16: wpk_t is not the transposed pack of a [%d, %d, 3, 3] weight" % (cout, cin))
    out = _out_map(out, (B, H, W, cin), dy, "out")
    check(L.fd_conv2d_s2_dgrad_bf16(_p(dy), B, H, W, cin, cout, _p(wpk_t), _p(out), _stream()), "fd_conv2d_s2_dgrad_bf16")
    return out


def conv2d_wgrad_s2_bf16(x_nhwc, dy_nhwc):
    """Weight gradient of the 3 x 3 / stride 2 / padding 1 convolution: x [B,H,W,Cin] and dy [B,(H-1)//2+1,(W-1)//2+1,Cout] bf16 contiguous
    -> dW [Cout, Cin, 3, 3] float32 (fd_conv2d_wgrad_s2_bf16: deterministic, no atomics)."""
    L = _lib.load()
    x, dy = _map4(x_nhwc, "x_nhwc"), _map4(dy_nhwc, "dy_nhwc")
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    if tuple(dy.shape[:3]) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise FutureDetHipError("conv2d_wgrad_s2_bf16: dy %s is not the stride-2 map of x %s" % (tuple(dy.shape), tuple(x.shape)))
    nbytes = L.fd_conv2d_wgrad_s2_bf16_workspace_bytes(B, H, W, cin, cout)
    if nbytes == 0:
        raise FutureDetHipError("conv2d_wgrad_s2_bf16: unsupported problem %s -> %d channels" % (tuple(x.shape), cout))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    check(L.fd_conv2d_wgrad_s2_bf16(_p(x), _p(dy), B, H, W, cin, cout, _p(ws), ws.numel(), _p(dw), _stream()), "fd_conv2d_wgrad_s2_bf16")
    return dw


PACK_UP2, PACK_DOWN2 = 0, 1


def pack_conv2d_weight_2x2_device(w, kind, fine_major=False):
    """The packed weights of the 2 x 2 / stride 2 pair from ``w``, fp32 [Ccoarse, Cfine, 2, 2] on the device (the layout of both
    nn.Conv2d(2, 2) and nn.ConvTranspose2d(2, 2); ``fine_major``: [Cfine, Ccoarse, 2, 2]), in one launch (fd_conv2d_pack_weight_2x2_dev).
    PACK_UP2: the four packs of conv2d_up2_bf16, tap 2 dy + dx = pack_conv2d_weight(w[:, :, dy, dx].t()[..., None, None]), back to back;
    PACK_DOWN2: the pack of conv2d_down2_bf16 = pack_conv2d_weight(w.permute(0, 2, 3, 1).reshape(Ccoarse, 4 * Cfine, 1, 1))."""
    L = _lib.load()
    w = _dev(w.detach(), "w", torch.float32)
    if w.dim() != 4 or tuple(w.shape[2:]) != (2, 2) or kind not in (PACK_UP2, PACK_DOWN2):
        raise FutureDetHipError("pack_conv2d_weight_2x2_device: need a [Ccoarse, Cfine, 2, 2] weight and kind PACK_UP2 or PACK_DOWN2 (got %s, %r)"
                                % (tuple(w.shape), kind))
    cc, cf = (w.shape[1], w.shape[0]) if fine_major else (w.shape[0], w.shape[1])
    nbytes = L.fd_conv2d_packed_weight_2x2_bytes(cc, cf, kind)
    if nbytes == 0:
        raise FutureDetHipError("pack_conv2d_weight_2x2_device: unsupported weight shape %s for kind %d" % (tuple(w.shape), kind))
    out = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
    check(L.fd_conv2d_pack_weight_2x2_dev(_p(w), cc, cf, kind, int(bool(fine_major)), _p(out), _stream()), "fd_conv2d_pack_weight_2x2_dev")
    return out


def conv2d_up2_bf16(x_nhwc, wpk4, c_fine, out=None):
    """"up2": coarse x [B, H, W, Ccoarse] bf16 -> fine [B, 2H, 2W, c_fine] bf16, fine[b, 2y+dy, 2x+dx] = x[b, y, x] . W(., ., dy, dx) -- four
    1 x 1 launches of fd_conv2d_nhwc_bf16 with pixel placement on the four packs of PACK_UP2."""
    x = _map4(x_nhwc, "x_nhwc")
    B, H, W, cc = x.shape
    _dev(wpk4, "wpk4", torch.uint8)
    per = _lib.load().fd_conv2d_packed_weight_bytes(c_fine, cc, 1)
    if per == 0 or wpk4.numel() != 4 * per:
        raise FutureDetHipError("conv2d_up2_bf16: wpk4 is not the PACK_UP2 pack of a [%d, %d, 2, 2] weight" % (cc, c_fine))
    out = _out_map(out, (B, 2 * H, 2 * W, c_fine), x, "out")
    for tap in range(4):
        conv2d_nhwc_bf16(x, wpk4[tap * per:(tap + 1) * per], None, c_fine, 1, stride=1, relu=False, out=out, osy=2, osx=2, ooy=tap >> 1, oox=tap & 1)
    return out


def conv2d_down2_bf16(x_nhwc, wpk, c_coarse, out=None):
    """"down2": fine x [B, H, W, Cfine] bf16 -> coarse [B, H//2, W//2, c_coarse] bf16, the sum over the 2 x 2 block of x . W(., ., dy, dx), on
    the PACK_DOWN2 pack (fd_conv2d_down2_bf16).  The trailing row or column of an odd H or W is not read."""
    L = _lib.load()
    x = _map4(x_nhwc, "x_nhwc")
    B, H, W, cf = x.shape
    _dev(wpk, "wpk", torch.uint8)
    if wpk.numel() != L.fd_conv2d_packed_weight_2x2_bytes(c_coarse, cf, PACK_DOWN2) or wpk.numel() == 0:
        raise FutureDetHipError("conv2d_down2_bf16: wpk is not the PACK_DOWN2 pack of a [%d, %d, 2, 2] weight" % (c_coarse, cf))
    out = _out_map(out, (B, H // 2, W // 2, c_coarse), x, "out")
    check(L.fd_conv2d_down2_bf16(_p(x), B, H, W, cf, _p(wpk), c_coarse, _p(out), _stream()), "fd_conv2d_down2_bf16")
    return out


def conv2d_wgrad_2x2_bf16(coarse_nhwc, fine_nhwc, fine_major=False):
    """Weight gradient of the 2 x 2 / stride 2 pair: coarse [B, H//2, W//2, Ccoarse] and fine [B, H, W, Cfine] bf16 contiguous -> dW float32
    [Ccoarse, Cfine, 2, 2] (``fine_major``: [Cfine, Ccoarse, 2, 2]), dW(a, f, dy, dx) = the sum over coarse pixels of
    coarse[b, y, x, a] fine[b, 2y+dy, 2x+dx, f] (fd_conv2d_wgrad_2x2_bf16: deterministic, no atomics)."""
    L = _lib.load()
    co, fi = _map4(coarse_nhwc, "coarse_nhwc"), _map4(fine_nhwc, "fine_nhwc")
    B, H, W, cf = fi.shape
    cc = co.shape[3]
    if tuple(co.shape[:3]) != (B, H // 2, W // 2):
        raise FutureDetHipError("conv2d_wgrad_2x2_bf16: coarse %s is not the 2 x 2 / stride 2 map of fine %s" % (tuple(co.shape), tuple(fi.shape)))
    nbytes = L.fd_conv2d_wgrad_2x2_bf16_workspace_bytes(B, H, W, cc, cf)
    if nbytes == 0:
        raise FutureDetHipError("conv2d_wgrad_2x2_bf16: unsupported problem %s, %s" % (tuple(co.shape), tuple(fi.shape)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=fi.device)
    dw = torch.empty((cf, cc, 2, 2) if fine_major else (cc, cf, 2, 2), dtype=torch.float32, device=fi.device)
    check(L.fd_conv2d_wgrad_2x2_bf16(_p(co), _p(fi), B, H, W, cc, cf, int(bool(fine_major)), _p(ws), ws.numel(), _p(dw), _stream()),
          "fd_conv2d_wgrad_2x2_bf16")
    return dw


# ------------------------------------------------------------------------------------------------ head tail (bf16 training)
def head_tail_max_groups():
    """Group records one launch of the head-tail kernels takes; the wrappers below split longer lists."""
    return int(_lib.load().fd_head_tail_bf16_max_groups())


def head_tail_wgrad_chunk():
    """Input pixels per partial of head_tail_wgrad: a constant of the library, part of its summation order."""
    return int(_lib.load().fd_head_tail_wgrad_bf16_chunk())


def _head_tail_group(what, x, c0, w, bias, y):
    """One fd_head_tail_group: channels c0 .. c0 + cin - 1 of the contiguous bf16 [B, H, W, C] tensor ``x``, the fp32 [k, cin, 3, 3] ``w``,
    the fp32 [k] ``bias`` (None where the entry point does not look at it) and the fp32 [B, k, H, W] ``y``."""
    x = _dev(x, what + ": x", torch.bfloat16)
    w = _dev(w, what + ": weight", torch.float32)
    y = _dev(y, what + ": y", torch.float32)
    if bias is not None:
        bias = _dev(bias, what + ": bias", torch.float32)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or y.dim() != 4:
        raise FutureDetHipError("%s: needs x [B, H, W, C], a [k, cin, 3, 3] weight and y [B, k, H, W] (got %s, %s, %s)"
                                % (what, tuple(x.shape), tuple(w.shape), tuple(y.shape)))
    k, cin = int(w.shape[0]), int(w.shape[1])
    B, H, W, C = x.shape
    if tuple(y.shape) != (B, k, H, W) or (bias is not None and tuple(bias.shape) != (k,)):
        raise FutureDetHipError("%s: y must be [%d, %d, %d, %d] and the bias [%d] (got %s, %s)"
                                % (what, B, k, H, W, k, tuple(y.shape), None if bias is None else tuple(bias.shape)))
    if c0 < 0 or c0 % 8 or c0 + cin > C:
        raise FutureDetHipError("%s: channels %d .. %d are no 16-byte aligned slice of the %d channels of x" % (what, c0, c0 + cin - 1, C))
    rec = _lib.HeadTailGroup(x.data_ptr() + 2 * c0, w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), C, cin, k)
    return rec, (B, H, W)


def _head_tail_launch(what, entry, records, with_workspace=False):
    """``entry`` over the records (rec, (B, H, W)), at most head_tail_max_groups() per launch"""
    L = _lib.load()
    shapes = set(s for _, s in records)
    if len(shapes) != 1:
        raise FutureDetHipError("%s: needs at least one group, all over the same B x H x W pixels (got %s)" % (what, sorted(shapes)))
    B, H, W = shapes.pop()
    step = head_tail_max_groups()
    for i in range(0, len(records), step):
        part = [r for r, _ in records[i:i + step]]
        arr = (_lib.HeadTailGroup * len(part))(*part)
        if with_workspace:
            nbytes = L.fd_head_tail_wgrad_bf16_workspace_bytes(B, H, W, sum(r.cin for r in part))
            if nbytes == 0:
                raise FutureDetHipError("%s: unsupported problem %d x %d x %d, cin %s" % (what, B, H, W, [r.cin for r in part]))
            ws = workspace.get("head_tail_wgrad", nbytes, torch.device("cuda", torch.cuda.current_device()))
            check(getattr(L, entry)(arr, len(part), B, H, W, _p(ws), ws.numel(), _stream()), entry)
        else:
            check(getattr(L, entry)(arr, len(part), B, H, W, _stream()), entry)


def head_tail_forward(groups):
    """fd_head_tail_forward_bf16: for every group (x, c0, weight, bias) the 3 x 3 / padding 1 convolution of channels c0 .. c0 + cin - 1 of
    the contiguous bf16 [B, H, W, C] tensor x with the fp32 [k, cin, 3, 3] weight (k <= 16, rounded to bf16 inside) plus the fp32 bias ->
    a list of fp32 NCHW [B, k, H, W] maps.  One launch per head_tail_max_groups() groups."""
    recs, ys = [], []
    for x, c0, w, bias in groups:
        x = _dev(x, "head_tail_forward: x", torch.bfloat16)
        w = _dev(w, "head_tail_forward: weight", torch.float32)
        if x.dim() != 4 or w.dim() != 4:
            raise FutureDetHipError("head_tail_forward: needs x [B, H, W, C] and a [k, cin, 3, 3] weight (got %s, %s)" % (tuple(x.shape), tuple(w.shape)))
        if bias is None:
            raise FutureDetHipError("head_tail_forward: every group needs a bias")
        y = torch.empty((x.shape[0], w.shape[0], x.shape[1], x.shape[2]), dtype=torch.float32, device=x.device)
        recs.append(_head_tail_group("head_tail_forward", x, c0, w, bias, y))
        ys.append(y)
    _head_tail_launch("head_tail_forward", "fd_head_tail_forward_bf16", recs)
    return ys


def head_tail_dgrad(groups):
    """fd_head_tail_dgrad_bf16: for every group (dx, c0, weight, dy) writes the input gradient of head_tail_forward's convolution, bf16,
    into channels c0 .. c0 + cin - 1 of the contiguous bf16 [B, H, W, C] tensor dx (the other channels are not touched); dy fp32
    [B, k, H, W]."""
    recs = [_head_tail_group("head_tail_dgrad", dx, c0, w, None, dy) for dx, c0, w, dy in groups]
    _head_tail_launch("head_tail_dgrad", "fd_head_tail_dgrad_bf16", recs)


def head_tail_wgrad(groups):
    """fd_head_tail_wgrad_bf16: for every group (x, c0, cin, dy) -> (dW fp32 [k, cin, 3, 3], dbias fp32 [k]) of head_tail_forward's
    convolution; deterministic, no atomics.  dbias sums the unrounded dy."""
    recs, out = [], []
    for x, c0, cin, dy in groups:
        dy = _dev(dy, "head_tail_wgrad: dy", torch.float32)
        if dy.dim() != 4:
            raise FutureDetHipError("head_tail_wgrad: dy must be [B, k, H, W] (got %s)" % (tuple(dy.shape),))
        dw = torch.empty((dy.shape[1], cin, 3, 3), dtype=torch.float32, device=dy.device)
        db = torch.empty((dy.shape[1],), dtype=torch.float32, device=dy.device)
        recs.append(_head_tail_group("head_tail_wgrad", x, c0, dw, db, dy))
        out.append((dw, db))
    _head_tail_launch("head_tail_wgrad", "fd_head_tail_wgrad_bf16", recs, with_workspace=True)
    return out


def pack_conv2d_weight_f32(w_oihw):
    """[Cout, Cin, k, k] float32 -> MFMA-fragment-ordered fp32 weights on the same device (fd_conv2d_f32_pack_weight)."""
    L = _lib.load()
    dev = w_oihw.device
    w = w_oihw.detach().to("cpu", torch.float32).contiguous()
    cout, cin, ks, _ = w.shape
    nbytes = L.fd_conv2d_f32_packed_weight_bytes(cout, cin, ks)
    if nbytes == 0:
        raise FutureDetHipError("fd_conv2d_f32: unsupported weight shape %s" % (tuple(w.shape),))
    host = torch.empty((nbytes,), dtype=torch.uint8)
    check(L.fd_conv2d_f32_pack_weight(ctypes.c_void_p(w.data_ptr()), cout, cin, ks, ctypes.c_void_p(host.data_ptr())),
          "fd_conv2d_f32_pack_weight")
    return host.to(dev)


def conv2d_nhwc_f32(x, wpk, bias, cout, ks, stride=1, relu=True, out=None, co_off=0, osy=1, osx=1, ooy=0, oox=0, tile=0):
    """x [B,H,W,Cin] float32 contiguous -> y [B,Ho*osy,Wo*osx,Ctot] float32 (allocated when ``out`` is None).
    ``tile``: 0 = the library's heuristic, 1..conv2d_f32_num_tiles() = that workgroup tile shape."""
    L = _lib.load()
    x = _dev(x, "x", torch.float32)
    B, H, W, cin = x.shape
    pad = 1 if ks == 3 else 0
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty((B, Ho * osy, Wo * osx, cout), dtype=torch.float32, device=x.device)
    _dev(out, "out", torch.float32)
    check(L.fd_conv2d_nhwc_f32(_p(x), B, H, W, cin, _p(wpk), _p(bias), cout, ks, stride, pad, int(bool(relu)), _p(out),
                               out.shape[3], co_off, osy, osx, ooy, oox, int(tile), _stream()), "fd_conv2d_nhwc_f32")
    return out


def conv2d_f32_num_tiles():
    return int(_lib.load().fd_conv2d_f32_num_tiles())


def conv2d_shuffle_nhwc_f32(x, wpk, bias, cout_sub, k, relu=True, out=None, co_off=0, tile=0):
    """ConvTranspose2d(k, stride k) as one 1x1 convolution + pixel shuffle: x [B,H,W,Cin] -> [B,H*k,W*k,Ctot] float32."""
    L = _lib.load()
    x = _dev(x, "x", torch.float32)
    B, H, W, cin = x.shape
    if out is None:
        out = torch.empty((B, H * k, W * k, cout_sub), dtype=torch.float32, device=x.device)
    _dev(out, "out", torch.float32)
    check(L.fd_conv2d_shuffle_nhwc_f32(_p(x), B, H, W, cin, _p(wpk), _p(bias), int(cout_sub), int(k), int(bool(relu)), _p(out), out.shape[3],
                                       co_off, int(tile), _stream()), "fd_conv2d_shuffle_nhwc_f32")
    return out


def conv2d_grouped_nhwc_f32(x, wpk, bias, counts, cin_g, relu=False, out=None, co_off=0, tile=0):
    """Grouped 3x3 convolution (<= 16 outputs per group): x [B,H,W,groups*cin_g] -> [B,H,W,sum(counts)] float32."""
    L = _lib.load()
    x = _dev(x, "x", torch.float32)
    B, H, W, cin = x.shape
    groups = len(counts)
    assert cin == groups * cin_g
    if out is None:
        out = torch.empty((B, H, W, int(sum(counts))), dtype=torch.float32, device=x.device)
    _dev(out, "out", torch.float32)
    check(L.fd_conv2d_grouped_nhwc_f32(_p(x), B, H, W, groups, int(cin_g), _p(wpk), _p(bias), (ctypes.c_int * groups)(*[int(c) for c in counts]),
                                       int(bool(relu)), _p(out), out.shape[3], co_off, int(tile), _stream()), "fd_conv2d_grouped_nhwc_f32")
    return out


def pack_conv2d_weight_wino(w_oihw):
    """[Cout, Cin, 3, 3] float32 -> Winograd-transformed (G g G^T), fragment-ordered fp32 weights on the same device."""
    L = _lib.load()
    dev = w_oihw.device
    w = w_oihw.detach().to("cpu", torch.float32).contiguous()
    cout, cin, ks, _ = w.shape
    nbytes = L.fd_conv2d_wino_f32_packed_weight_bytes(cout, cin) if ks == 3 else 0
    if nbytes == 0:
        raise FutureDetHipError("fd_conv2d_wino_f32: unsupported weight shape %s" % (tuple(w.shape),))
    host = torch.empty((nbytes,), dtype=torch.uint8)
    check(L.fd_conv2d_wino_f32_pack_weight(ctypes.c_void_p(w.data_ptr()), cout, cin, ctypes.c_void_p(host.data_ptr())),
          "fd_conv2d_wino_f32_pack_weight")
    return host.to(dev)


def conv2d_wino_nhwc_f32(x, wpk, bias, cout, relu=True, out=None, co_off=0, tile=0):
    """3x3 stride-1 pad-1 convolution by Winograd F(2x2,3x3) on MFMA: x [B,H,W,Cin] float32 -> [B,H,W,Ctot] float32."""
    L = _lib.load()
    x = _dev(x, "x", torch.float32)
    B, H, W, cin = x.shape
    if out is None:
        out = torch.empty((B, H, W, cout), dtype=torch.float32, device=x.device)
    _dev(out, "out", torch.float32)
    check(L.fd_conv2d_wino_nhwc_f32(_p(x), B, H, W, cin, _p(wpk), _p(bias), cout, int(bool(relu)), _p(out), out.shape[3], co_off, int(tile),
                                    _stream()), "fd_conv2d_wino_nhwc_f32")
    return out


def conv2d_wino_f32_num_tiles():
    return int(_lib.load().fd_conv2d_wino_f32_num_tiles())


# ------------------------------------------------------------------------------------------------ decode / NMS
CIRCLE_PRE_MAX = 4096  # candidates taken per group under circular NMS (the kernels' bound; the reference applies no cut there)


def pack_deform_adapt(w_cls, w_reg, off_w_cls, off_b_cls, off_w_reg, off_b_reg, bf16):
    """The two FeatureAdaption modules of a DCN task (conv_adaption weights [64, 64, 3, 3], conv_offset weights [72, 64, 1, 1] and
    biases [72]) -> (packed conv_adaption weights for fd_deform_adapt_nhwc, off_w [2, 72, 64] fp32, off_b [2, 72] fp32), on the
    device of w_cls.  The offset weights stay fp32 in the bf16 mode."""
    L = _lib.load()
    dev = w_cls.device
    wc = w_cls.detach().to("cpu", torch.float32).contiguous()
    wr = w_reg.detach().to("cpu", torch.float32).contiguous()
    if tuple(wc.shape) != (64, 64, 3, 3) or tuple(wr.shape) != (64, 64, 3, 3):
        raise FutureDetHipError("fd_deform_adapt: conv_adaption weights must be [64, 64, 3, 3], got %s / %s" % (tuple(wc.shape), tuple(wr.shape)))
    host = torch.empty((L.fd_deform_adapt_packed_weight_bytes(int(bool(bf16))),), dtype=torch.uint8)
    check(L.fd_deform_adapt_pack_weight(ctypes.c_void_p(wc.data_ptr()), ctypes.c_void_p(wr.data_ptr()), int(bool(bf16)),
                                        ctypes.c_void_p(host.data_ptr())), "fd_deform_adapt_pack_weight")
    ow = torch.stack([off_w_cls.detach().float().reshape(72, 64), off_w_reg.detach().float().reshape(72, 64)]).contiguous()
    ob = torch.stack([off_b_cls.detach().float().reshape(72), off_b_reg.detach().float().reshape(72)]).contiguous()
    return host.to(dev), ow.to(dev), ob.to(dev)


def deform_adapt_nhwc(x, wpk, off_w=None, off_b=None, offsets=None, out=None):
    """x [B,H,W,64] fp32 or bf16 -> [B,H,W,128] of x's dtype: ReLU(DCN_cls) in channels 0-63, ReLU(DCN_reg) in 64-127 (fd_deform_adapt_nhwc).
    The offsets come from off_w / off_b (pack_deform_adapt; computed in the kernel) or, when given, from ``offsets`` [B,H,W,144] fp32."""
    L = _lib.load()
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise FutureDetHipError("x must be float32 or bfloat16, got %s" % (x.dtype,))
    x = _dev(x, "x")
    B, H, W, C = x.shape
    bf16 = int(x.dtype == torch.bfloat16)
    if offsets is not None:
        _dev(offsets, "offsets", torch.float32)
        if tuple(offsets.shape) != (B, H, W, 144):
            raise FutureDetHipError("offsets must be [B, H, W, 144], got %s" % (tuple(offsets.shape),))
    else:
        if off_w is None or off_b is None:
            raise FutureDetHipError("deform_adapt_nhwc: off_w and off_b are required without offsets")
        _dev(off_w, "off_w", torch.float32)
        _dev(off_b, "off_b", torch.float32)
        if off_w.numel() != 2 * 72 * C or off_b.numel() != 2 * 72:
            raise FutureDetHipError("off_w must be [2, 72, %d] and off_b [2, 72]" % C)
    if wpk.numel() != L.fd_deform_adapt_packed_weight_bytes(bf16):
        raise FutureDetHipError("deform_adapt_nhwc: packed weights are not of this dtype")
    _dev(wpk, "wpk")
    if out is None:
        out = torch.empty((B, H, W, 2 * C), dtype=x.dtype, device=x.device)
    _dev(out, "out", x.dtype)
    if tuple(out.shape) != (B, H, W, 2 * C):
        raise FutureDetHipError("out must be [B, H, W, %d], got %s" % (2 * C, tuple(out.shape)))
    check(L.fd_deform_adapt_nhwc(_p(x), B, H, W, C, bf16, _p(off_w), _p(off_b), _p(offsets), _p(wpk), _p(out), _stream()),
          "fd_deform_adapt_nhwc")
    return out


def _adapt_weight(w, name):
    w = _dev(w.detach(), name, torch.float32)
    if tuple(w.shape) != (64, 64, 3, 3):
        raise FutureDetHipError("fd_deform_adapt: %s must be [64, 64, 3, 3], got %s" % (name, tuple(w.shape)))
    return w


def pack_deform_adapt_device(w_cls, w_reg):
    """The fp32 packed conv_adaption weights of pack_deform_adapt, from device weights with no host round trip
    (fd_deform_adapt_pack_weight_device; byte-identical to the host packer)."""
    L = _lib.load()
    wc, wr = _adapt_weight(w_cls, "w_cls"), _adapt_weight(w_reg, "w_reg")
    out = torch.empty((L.fd_deform_adapt_packed_weight_bytes(0),), dtype=torch.uint8, device=wc.device)
    check(L.fd_deform_adapt_pack_weight_device(_p(wc), _p(wr), _p(out), _stream()), "fd_deform_adapt_pack_weight_device")
    return out


def deform_adapt_backward(x, offsets, w_cls, w_reg, y, dy, need=(True, True, True)):
    """Gradients of deform_adapt_nhwc(x, pack(w_cls, w_reg), offsets=offsets) = y under dy (fd_deform_adapt_backward), all fp32 NHWC:
    -> (dx [B,H,W,64], doffsets [B,H,W,144], dw [2,64,64,3,3]); an entry of ``need`` = (dx, doffsets, dw) that is False gives None.
    doffsets and dw are bit-identical from run to run; dx is summed with atomic adds."""
    L = _lib.load()
    x = _dev(x, "x", torch.float32)
    B, H, W, C = x.shape
    for t, name, ch in ((offsets, "offsets", 144), (y, "y", 2 * C), (dy, "dy", 2 * C)):
        _dev(t, name, torch.float32)
        if tuple(t.shape) != (B, H, W, ch):
            raise FutureDetHipError("%s must be [B, H, W, %d], got %s" % (name, ch, tuple(t.shape)))
    wc, wr = _adapt_weight(w_cls, "w_cls"), _adapt_weight(w_reg, "w_reg")
    dx = torch.empty_like(x) if need[0] else None
    doff = torch.empty_like(offsets) if need[1] else None
    dw = torch.empty((2, 64, 64, 3, 3), dtype=torch.float32, device=x.device) if need[2] else None
    ws = workspace.get("deform_adapt_backward", L.fd_deform_adapt_backward_workspace_bytes(B, H, W), x.device)
    check(L.fd_deform_adapt_backward(_p(x), _p(offsets), _p(wc), _p(wr), _p(y), _p(dy), B, H, W, C, _p(dx), _p(doff), _p(dw), _p(ws), ws.numel(),
                                     _stream()), "fd_deform_adapt_backward")
    return dx, doff, dw


def make_decode_cfg(H, W, test_cfg, hm_channels=1, group_radius=None):
    """``hm_channels`` > 1: the score of a cell is the maximum over that many heat-map channels (CenterHead's ``classify``
    mode, center_head.py:589-595: torch.max(hm, dim=1) before the sigmoid).  ``group_radius``: test_cfg.circular_nms
    (center_head.py:722-725) -- one ``min_radius`` per decode group; the rotated-IoU predicate is replaced by the centre
    distance and the pre-NMS cut by the kernels' maximum (see fd_decode_cfg in include/futuredet_hip.h)."""
    c = DecodeCfg()
    c.hm_channels = int(hm_channels)
    c.H, c.W = int(H), int(W)
    c.out_size_factor = float(test_cfg["out_size_factor"])
    c.voxel_x, c.voxel_y = float(test_cfg["voxel_size"][0]), float(test_cfg["voxel_size"][1])
    c.pc_x, c.pc_y = float(test_cfg["pc_range"][0]), float(test_cfg["pc_range"][1])
    c.score_threshold = float(test_cfg["score_threshold"])
    for i, v in enumerate(test_cfg["post_center_limit_range"]):
        c.center_range[i] = float(v)
    nms = test_cfg["nms"]
    c.nms_iou_threshold = float(nms["nms_iou_threshold"])
    c.nms_pre_max = int(nms["nms_pre_max_size"])
    c.nms_post_max = int(nms["nms_post_max_size"])
    if group_radius is not None:
        if not 1 <= len(group_radius) <= 16:
            raise ValueError("circular NMS: 1..16 decode groups, got %d radii" % len(group_radius))
        c.nms_kind, c.n_radius = 1, len(group_radius)
        c.nms_pre_max = CIRCLE_PRE_MAX
        for i, r in enumerate(group_radius):
            c.circle_radius[i] = float(r)
    return c


def centerpoint_decode(hm, reg, height, dim, rot, cfg):
    """Inputs are [G, C, H, W] float32 NCHW slices (G groups, C = 1/2/1/3/2).  Returns (boxes7 [G,post,7],
    scores [G,post], cell [G,post] int32, count [G] int32), all on device."""
    L = _lib.load()
    G = hm.shape[0]
    ts = [_dev(t, n, torch.float32) for t, n in ((hm, "hm"), (reg, "reg"), (height, "height"), (dim, "dim"), (rot, "rot"))]
    dev = hm.device
    post = cfg.nms_post_max
    boxes = torch.empty((G, post, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((G, post), dtype=torch.float32, device=dev)
    cell = torch.empty((G, post), dtype=torch.int32, device=dev)
    count = torch.empty((G,), dtype=torch.int32, device=dev)
    ws = workspace.get("decode", L.fd_decode_workspace_bytes(G, ctypes.byref(cfg)), dev)
    args = []
    for t in ts:
        args += [_p(t), t.stride(0)]
    check(L.fd_centerpoint_decode(*args, G, ctypes.byref(cfg), _p(boxes), _p(scores), _p(cell), _p(count), _p(ws),
                                  ws.numel(), _stream()), "fd_centerpoint_decode")
    return boxes, scores, cell, count


def nhwc_channel_view(buf, c0):
    """fd_map_view of channels [c0, ...) of an NHWC buffer [G, H, W, C] (float32 or bf16): the decode reads a head output in place"""
    assert buf.is_cuda and buf.is_contiguous() and buf.dim() == 4 and buf.dtype in (torch.float32, torch.bfloat16)
    G, H, W, C = buf.shape
    return MapView(buf.data_ptr() + int(c0) * buf.element_size(), H * W * C, 1, C, 0 if buf.dtype == torch.float32 else 1)


def centerpoint_decode_views(views, G, cfg, device):
    """fd_centerpoint_decode_maps on five fd_map_view (hm, reg, height, dim, rot); G = groups x samples.  Returns
    (boxes7 [G,post,7], scores [G,post], cell [G,post] int32, count [G] int32)."""
    L = _lib.load()
    post = cfg.nms_post_max
    boxes = torch.empty((G, post, 7), dtype=torch.float32, device=device)
    scores = torch.empty((G, post), dtype=torch.float32, device=device)
    cell = torch.empty((G, post), dtype=torch.int32, device=device)
    count = torch.empty((G,), dtype=torch.int32, device=device)
    ws = workspace.get("decode", L.fd_decode_workspace_bytes(G, ctypes.byref(cfg)), device)
    check(L.fd_centerpoint_decode_maps(*[ctypes.byref(v) for v in views], G, ctypes.byref(cfg), _p(boxes), _p(scores), _p(cell), _p(count), _p(ws),
                                       ws.numel(), _stream()), "fd_centerpoint_decode_maps")
    return boxes, scores, cell, count


def centerpoint_decode_packed(views, vel_view, G, B, cfg, device, step_group, step_vel_channel, step_label):
    """fd_centerpoint_decode_packed: decode + rotated NMS + assembly of the packed result in one call (five launches, the last one
    sweeps, gathers and writes the packed rows).  views = (hm, reg, height, dim, rot) fd_map_view; decode groups are group-major
    (g = group * B + sample).  -> (packed [B, S, post, 11] float32 rows x y z w l h vx vy yaw score label, counts [B, S] int32)"""
    L = _lib.load()
    post, S = cfg.nms_post_max, len(step_group)
    boxes = torch.empty((G, post, 7), dtype=torch.float32, device=device)
    scores = torch.empty((G, post), dtype=torch.float32, device=device)
    cell = torch.empty((G, post), dtype=torch.int32, device=device)
    count = torch.empty((G,), dtype=torch.int32, device=device)
    packed = torch.empty((B, S, post, 11), dtype=torch.float32, device=device)
    counts = torch.empty((B, S), dtype=torch.int32, device=device)
    ws = workspace.get("decode", L.fd_decode_workspace_bytes(G, ctypes.byref(cfg)), device)
    arr = lambda v: (ctypes.c_int32 * S)(*[int(x) for x in v])  # noqa: E731
    check(L.fd_centerpoint_decode_packed(*[ctypes.byref(v) for v in views], ctypes.byref(vel_view), int(G), int(B), ctypes.byref(cfg), S, arr(step_group),
                                         arr(step_vel_channel), arr(step_label), _p(boxes), _p(scores), _p(cell), _p(count), _p(packed), _p(counts), _p(ws),
                                         ws.numel(), _stream()), "fd_centerpoint_decode_packed")
    return packed, counts


def assemble_detections(boxes7, scores, cell, count, vel_view, B, post, step_group, step_vel_channel, step_label):
    """fd_assemble_detections: -> (packed [B, S, post, 11] float32 rows x y z w l h vx vy yaw score label, counts [B, S] int32)"""
    L = _lib.load()
    S = len(step_group)
    dev = boxes7.device
    packed = torch.empty((B, S, post, 11), dtype=torch.float32, device=dev)
    counts = torch.empty((B, S), dtype=torch.int32, device=dev)
    arr = lambda v: (ctypes.c_int32 * S)(*[int(x) for x in v])  # noqa: E731
    check(L.fd_assemble_detections(_p(boxes7), _p(scores), _p(cell), _p(count), ctypes.byref(vel_view), int(B), int(post), S, arr(step_group),
                                   arr(step_vel_channel), arr(step_label), _p(packed), _p(counts), _stream()), "fd_assemble_detections")
    return packed, counts


def rotated_nms(boxes7, thresh):
    """nms_gpu contract on device: boxes [n,7] (pcdet layout, score-sorted) -> (keep int64[n], count int32[1])."""
    L = _lib.load()
    boxes7 = _dev(boxes7, "boxes", torch.float32)
    n = boxes7.shape[0]
    keep = torch.zeros((max(n, 1),), dtype=torch.int64, device=boxes7.device)
    count = torch.zeros((1,), dtype=torch.int32, device=boxes7.device)
    ws = workspace.get("nms", L.fd_nms_workspace_bytes(n), boxes7.device)
    check(L.fd_rotated_nms(_p(boxes7), n, ctypes.c_float(thresh), _p(keep), _p(count), _p(ws), ws.numel(), _stream()),
          "fd_rotated_nms")
    return keep, count


def boxes_iou_bev(a, b):
    L = _lib.load()
    a = _dev(a, "boxes_a", torch.float32)
    b = _dev(b, "boxes_b", torch.float32)
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    check(L.fd_boxes_iou_bev(_p(a), a.shape[0], _p(b), b.shape[0], _p(out), _stream()), "fd_boxes_iou_bev")
    return out


# ------------------------------------------------------------------------------------------------ sweep assembly
SWEEP_DESC = np.dtype([("m", np.float64, (16,)), ("row_begin", np.int64), ("row_end", np.int64), ("time", np.float32),
                       ("flags", np.int32)])  # == struct fd_sweep_desc (include/futuredet_hip.h)
SWEEP_HAS_TRANSFORM, SWEEP_REMOVE_CLOSE = 1, 2


def sweep_descriptors(rows, transforms, time_lags, remove_close):
    """Host side of fd_sweep_assemble: per-sweep records in visit order.  ``rows`` are the cumulative raw-row offsets
    [S+1]; transforms[s] is a 4x4 (any float dtype; promoted to float64 like np.dot with the float64 ones row,
    loading.py:54-56) or None; time_lags[s] a Python/NumPy float; remove_close[s] a bool."""
    S = len(rows) - 1
    d = np.zeros((S,), SWEEP_DESC)
    for s in range(S):
        d["row_begin"][s], d["row_end"][s] = int(rows[s]), int(rows[s + 1])
        flags = 0
        if transforms[s] is not None:
            d["m"][s] = np.asarray(transforms[s], np.float64).reshape(16)
            flags |= SWEEP_HAS_TRANSFORM
        if remove_close[s]:
            flags |= SWEEP_REMOVE_CLOSE
        d["flags"][s] = flags
        d["time"][s] = np.float32(np.float64(time_lags[s]))  # (time_lag * ones).astype(float32), loading.py:58,134
    return d


def assemble_sweeps(raw, desc, keep_cols=4, min_distance=1.0, out=None, count=None, n_sweeps=None):
    """Runs fd_sweep_assemble on device rows ``raw`` [R, raw_cols] float32.  ``desc``: host descriptors (sweep_descriptors; uploaded
    here) or a device uint8 tensor already holding ``n_sweeps`` fd_sweep_desc records (the static form: a captured launch reads
    whatever the caller last copied there; R is then an upper bound, rows past the last descriptor's row_end are dropped).
    Returns (points [R, keep_cols+1] padded with +inf past the count, count int32[1]); ``out`` / ``count`` may be given; no sync."""
    L = _lib.load()
    raw = _dev(raw, "raw", torch.float32)
    R, raw_cols = raw.shape
    dev = raw.device
    if isinstance(desc, torch.Tensor):
        desc_dev = _dev(desc, "desc", torch.uint8)
        n_desc = int(n_sweeps) if n_sweeps is not None else desc_dev.numel() // SWEEP_DESC.itemsize
        assert desc_dev.numel() >= n_desc * SWEEP_DESC.itemsize
    else:
        desc = np.ascontiguousarray(desc)
        assert desc.dtype == SWEEP_DESC
        desc_dev = torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(dev, non_blocking=True)
        n_desc = len(desc)
    if out is None:
        out = torch.empty((R, keep_cols + 1), dtype=torch.float32, device=dev)
    else:
        out = _dev(out, "out", torch.float32)
        assert out.shape[0] >= R and out.shape[1] == keep_cols + 1
    if count is None:
        count = torch.empty((1,), dtype=torch.int32, device=dev)
    ws_bytes = L.fd_sweep_assemble_workspace_bytes(R)
    ws = workspace.get("sweeps", ws_bytes, dev)
    check(L.fd_sweep_assemble(_p(raw), raw_cols, int(keep_cols), R, _p(desc_dev), n_desc, float(min_distance), _p(out),
                              _p(count), _p(ws), ws.numel(), _stream()), "fd_sweep_assemble")
    return out, count


# ------------------------------------------------------------------------------------------------ PointPillars reader
def pillar_encode(voxels, num_points, coors4, n_dev, geom, layers, with_distance=False, out_dtype=torch.float32):
    """fd_pillar_encode: voxels [M,P,ndim] f32, num_points [M] i32, coors4 [M,4] i32 (b,z,y,x), n_dev device int32[1] or
    None; geom = (vx, vy, x_offset, y_offset); layers = [(weight [U,Fin] f32, scale [U], shift [U])] (1 or 2 entries).
    Returns [M, U_last] (rows past the count are left untouched: zero-initialised here)."""
    L = _lib.load()
    voxels = _dev(voxels, "voxels", torch.float32)
    M, P, ndim = voxels.shape
    (w1, s1, b1) = layers[0]
    (w2, s2, b2) = layers[1] if len(layers) > 1 else (None, None, None)
    assert len(layers) in (1, 2)
    U = (w2 if w2 is not None else w1).shape[0]
    out = torch.zeros((M, U), dtype=out_dtype, device=voxels.device)
    check(L.fd_pillar_encode(_p(voxels), _p(num_points), _p(coors4), _p(n_dev), M, P, ndim, int(bool(with_distance)),
                             float(geom[0]), float(geom[1]), float(geom[2]), float(geom[3]), _p(w1), _p(s1), _p(b1), w1.shape[0],
                             _p(w2), _p(s2), _p(b2), (w2.shape[0] if w2 is not None else 0), _DT[out_dtype], _p(out), U, _stream()),
          "fd_pillar_encode")
    return out


def pillar_train_workspace_bytes(m, max_points):
    return int(_lib.load().fd_pillar_train_workspace_bytes(int(m), int(max_points)))


def _pillar_train_args(voxels, num_points, coors4, geom, w1, g1, b1, w2, g2, b2, with_distance):
    voxels = _dev(voxels, "voxels", torch.float32)
    M, P, ndim = voxels.shape
    for t, name in ((w1, "w1"), (g1, "gamma1"), (b1, "beta1"), (w2, "w2"), (g2, "gamma2"), (b2, "beta2")):
        _dev(t, name, torch.float32)
    return [_p(voxels), _p(_dev(num_points, "num_points", torch.int32)), _p(_dev(coors4, "coors4", torch.int32)), M, P, ndim,
            int(bool(with_distance)), float(geom[0]), float(geom[1]), float(geom[2]), float(geom[3])]


def pillar_train_forward(voxels, num_points, coors4, geom, w1, g1, b1, eps1, w2, g2, b2, eps2, with_distance=False, out=None,
                         workspace=None):
    """fd_pillar_train_forward: PillarFeatureNet (two PFN layers, 32 -> 64) on batch statistics.  voxels [M,P,ndim] f32,
    num_points [M] / coors4 [M,4] int32, geom = (vx, vy, x_offset, y_offset), w1 [32, Fin], w2 [64, 64], gamma / beta per layer.
    Returns (out [M, 64], mean1, var1 [32], mean2, var2 [64], workspace); the variances are biased, the workspace (uint8) holds
    what pillar_train_backward needs."""
    L = _lib.load()
    args = _pillar_train_args(voxels, num_points, coors4, geom, w1, g1, b1, w2, g2, b2, with_distance)
    M, P = args[3], args[4]
    dev = voxels.device
    nbytes = L.fd_pillar_train_workspace_bytes(M, P)
    if workspace is None:
        workspace = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((M, w2.shape[0]), dtype=torch.float32, device=dev)
    stats = torch.empty((2 * w1.shape[0] + 2 * w2.shape[0],), dtype=torch.float32, device=dev)
    u1, u2 = w1.shape[0], w2.shape[0]
    mean1, var1, mean2, var2 = stats[:u1], stats[u1:2 * u1], stats[2 * u1:2 * u1 + u2], stats[2 * u1 + u2:]
    check(L.fd_pillar_train_forward(*args, _p(w1), _p(g1), _p(b1), u1, float(eps1), _p(w2), _p(g2), _p(b2), u2, float(eps2),
                                    _p(_dev(out, "out", torch.float32)), _p(mean1), _p(var1), _p(mean2), _p(var2), _p(workspace),
                                    workspace.numel(), _stream()), "fd_pillar_train_forward")
    return out, mean1, var1, mean2, var2, workspace


def pillar_train_backward(dout, voxels, num_points, coors4, geom, w1, g1, b1, w2, g2, b2, workspace, with_distance=False):
    """fd_pillar_train_backward: dout [M, 64] -> (dw1, dgamma1, dbeta1, dw2, dgamma2, dbeta2); ``workspace`` as the matching
    pillar_train_forward left it."""
    L = _lib.load()
    args = _pillar_train_args(voxels, num_points, coors4, geom, w1, g1, b1, w2, g2, b2, with_distance)
    dout = _dev(dout, "dout", torch.float32)
    assert tuple(dout.shape) == (args[3], w2.shape[0]), (tuple(dout.shape), args[3])
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    dg1, db1, dg2, db2 = torch.empty_like(g1), torch.empty_like(b1), torch.empty_like(g2), torch.empty_like(b2)
    check(L.fd_pillar_train_backward(*args, _p(w1), _p(g1), _p(b1), w1.shape[0], _p(w2), _p(g2), _p(b2), w2.shape[0], _p(dout),
                                     _p(dw1), _p(dg1), _p(db1), _p(dw2), _p(dg2), _p(db2), _p(workspace), workspace.numel(), _stream()),
          "fd_pillar_train_backward")
    return dw1, dg1, db1, dw2, dg2, db2


def _pillar_train_dev_args(voxels, num_points, coors4, seg_counts, geom, w1, g1, b1, w2, g2, b2, with_distance):
    """Checks and leading arguments of the device-count entries: voxels [B, cap, P, ndim] (or [B * cap, P, ndim] with
    seg_counts [B]), num_points [B, cap], coors4 [B, cap, 4], seg_counts int32[B] on the device."""
    voxels = _dev(voxels, "voxels", torch.float32)
    seg_counts = _dev(seg_counts, "seg_counts", torch.int32)
    if seg_counts.dim() != 1 or not 1 <= seg_counts.numel() <= 16:
        raise FutureDetHipError("pillar_train (device counts): seg_counts must be int32[B] with 1 <= B <= 16, got %s" % (tuple(seg_counts.shape),))
    B = seg_counts.numel()
    if voxels.dim() == 4:
        voxels = voxels.reshape(-1, voxels.shape[2], voxels.shape[3])
    rows, P, ndim = voxels.shape
    if rows < B or rows % B:
        raise FutureDetHipError("pillar_train (device counts): %d voxel rows are not %d segments of equal size" % (rows, B))
    num_points = _dev(num_points, "num_points", torch.int32)
    coors4 = _dev(coors4, "coors4", torch.int32)
    if num_points.numel() != rows or coors4.numel() != rows * 4:
        raise FutureDetHipError("pillar_train (device counts): num_points %s / coors4 %s do not match %d voxel rows"
                                % (tuple(num_points.shape), tuple(coors4.shape), rows))
    for t, name in ((w1, "w1"), (g1, "gamma1"), (b1, "beta1"), (w2, "w2"), (g2, "gamma2"), (b2, "beta2")):
        _dev(t, name, torch.float32)
    return [_p(voxels), _p(num_points), _p(coors4), _p(seg_counts), B, rows // B, P, ndim, int(bool(with_distance)),
            float(geom[0]), float(geom[1]), float(geom[2]), float(geom[3])]


def pillar_train_forward_dev(voxels, num_points, coors4, seg_counts, geom, w1, g1, b1, eps1, w2, g2, b2, eps2, with_distance=False,
                             out=None, workspace=None):
    """fd_pillar_train_forward_dev: pillar_train_forward on B segments of ``cap`` rows whose pillar counts are on the device
    (seg_counts int32[B]); no host read.  Returns (out [B * cap, 64] with zeros behind the counts, mean1, var1, mean2, var2,
    workspace): the bits of pillar_train_forward on the compacted pillars."""
    L = _lib.load()
    args = _pillar_train_dev_args(voxels, num_points, coors4, seg_counts, geom, w1, g1, b1, w2, g2, b2, with_distance)
    rows, P = args[4] * args[5], args[6]
    dev = voxels.device
    nbytes = L.fd_pillar_train_workspace_bytes(rows, P)
    if workspace is None:
        workspace = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((rows, w2.shape[0]), dtype=torch.float32, device=dev)
    u1, u2 = w1.shape[0], w2.shape[0]
    stats = torch.empty((2 * u1 + 2 * u2,), dtype=torch.float32, device=dev)
    mean1, var1, mean2, var2 = stats[:u1], stats[u1:2 * u1], stats[2 * u1:2 * u1 + u2], stats[2 * u1 + u2:]
    check(L.fd_pillar_train_forward_dev(*args, _p(w1), _p(g1), _p(b1), u1, float(eps1), _p(w2), _p(g2), _p(b2), u2, float(eps2),
                                        _p(_dev(out, "out", torch.float32)), _p(mean1), _p(var1), _p(mean2), _p(var2), _p(workspace),
                                        workspace.numel(), _stream()), "fd_pillar_train_forward_dev")
    return out, mean1, var1, mean2, var2, workspace


def pillar_train_backward_dev(dout, voxels, num_points, coors4, seg_counts, geom, w1, g1, b1, w2, g2, b2, workspace, with_distance=False):
    """fd_pillar_train_backward_dev: dout [B * cap, 64] (rows behind the counts are not read) -> the six gradients; ``workspace``
    as the matching pillar_train_forward_dev left it."""
    L = _lib.load()
    args = _pillar_train_dev_args(voxels, num_points, coors4, seg_counts, geom, w1, g1, b1, w2, g2, b2, with_distance)
    dout = _dev(dout, "dout", torch.float32)
    assert tuple(dout.shape) == (args[4] * args[5], w2.shape[0]), (tuple(dout.shape), args[4] * args[5])
    dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
    dg1, db1, dg2, db2 = torch.empty_like(g1), torch.empty_like(b1), torch.empty_like(g2), torch.empty_like(b2)
    check(L.fd_pillar_train_backward_dev(*args, _p(w1), _p(g1), _p(b1), w1.shape[0], _p(w2), _p(g2), _p(b2), w2.shape[0], _p(dout),
                                         _p(dw1), _p(dg1), _p(db1), _p(dw2), _p(dg2), _p(db2), _p(workspace), workspace.numel(),
                                         _stream()), "fd_pillar_train_backward_dev")
    return dw1, dg1, db1, dw2, dg2, db2


def pillar_train_running_stats_dev(mean, var, momentum, seg_counts, seg_stride, max_points, running_mean, running_var,
                                   num_batches_tracked=None):
    """fd_pillar_train_running_stats_dev: torch's BatchNorm running-statistics rule in place, n = max_points * sum of the clamped
    seg_counts read on the device (nothing happens for n < 2).  ``momentum`` is a number: the cumulative average (None) needs
    num_batches_tracked on the host."""
    L = _lib.load()
    if momentum is None:
        raise NotImplementedError("pillar_train_running_stats_dev: momentum=None (cumulative average) is not implemented on the "
                                  "device-count path")
    mean, var = _dev(mean, "mean", torch.float32), _dev(var, "var", torch.float32)
    seg_counts = _dev(seg_counts, "seg_counts", torch.int32)
    running_mean, running_var = _dev(running_mean, "running_mean", torch.float32), _dev(running_var, "running_var", torch.float32)
    c = mean.numel()
    if not (var.numel() == running_mean.numel() == running_var.numel() == c):
        raise FutureDetHipError("pillar_train_running_stats_dev: mean, var and the running buffers must have one length")
    if num_batches_tracked is not None:
        num_batches_tracked = _dev(num_batches_tracked, "num_batches_tracked", torch.int64)
    check(L.fd_pillar_train_running_stats_dev(_p(mean), _p(var), c, float(momentum), _p(seg_counts), seg_counts.numel(), int(seg_stride),
                                              int(max_points), _p(running_mean), _p(running_var), _p(num_batches_tracked), _stream()),
          "fd_pillar_train_running_stats_dev")
    for buf in (running_mean, running_var, num_batches_tracked):
        if buf is not None:
            torch.autograd.graph.increment_version(buf)  # written behind torch's back: derived-weight caches key on the version


def pillar_scatter_backward(dcanvas, coors4, n_dev=None):
    """Backward of PointPillarsScatter: d(pillar row m) = dcanvas[b, :, y, x] for coors4[m] = (b, 0, y, x) -- fd_dense_gather with D = 1
    on any canvas strides (NCHW or channels-last).  Returns [M, C] float32.  ``n_dev``: device int32[1] count of the live rows of
    coors4; the rows behind it are not read and get gradient 0."""
    L = _lib.load()
    if not (isinstance(dcanvas, torch.Tensor) and dcanvas.is_cuda and dcanvas.dtype == torch.float32):
        raise FutureDetHipError("pillar_scatter_backward: dcanvas must be a float32 tensor on the HIP device")
    coors4 = _dev(coors4, "coors4", torch.int32)
    n, c = coors4.shape[0], dcanvas.shape[1]
    feats = torch.empty((max(n, 1), c), dtype=torch.float32, device=dcanvas.device)[:n]
    sb, sc, sy, sx = dcanvas.stride()
    if n_dev is not None:
        n_dev = _dev(n_dev, "n_dev", torch.int32)
    check(L.fd_dense_gather(_p(dcanvas), sb, sc, sy, sx, 1, _p(coors4), n, _p(n_dev), c, _p(feats), _stream()), "fd_dense_gather")
    return feats


def pillar_scatter(feats, coors4, n_dev, batch_size, ny, nx, out_dtype=None, channels_last=False, out=None, zero_first=True):
    """fd_pillar_scatter -> [B, C, ny, nx] canvas (NCHW, or channels-last memory when asked)."""
    L = _lib.load()
    feats = _dev(feats, "feats")
    M, C = feats.shape
    if out is None:
        out = torch.empty((batch_size, C, ny, nx), dtype=out_dtype or feats.dtype, device=feats.device,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    sb, sc, sy, sx = out.stride()
    check(L.fd_pillar_scatter(_p(feats), C, feats.stride(0), _DT[feats.dtype], _p(coors4), _p(n_dev), M, batch_size, ny, nx,
                              _p(out), _DT[out.dtype], sb, sc, sy, sx, int(bool(zero_first)), _stream()), "fd_pillar_scatter")
    return out


# ------------------------------------------------------------------------------------------------ forecast association
def forecast_chains(centers, velocity, counts, time, reject_thresh):
    """fd_forecast_chains on device tensors: centers/velocity [T,n,3] float64, counts [T] int32, time [T-1] float64."""
    L = _lib.load()
    centers = _dev(centers, "centers", torch.float64)
    velocity = _dev(velocity, "velocity", torch.float64)
    T, n, _ = centers.shape
    dev = centers.device
    i32 = dict(dtype=torch.int32, device=dev)
    out = dict(fwd_idx=torch.zeros((n, T), **i32), fwd_ok=torch.zeros((n,), **i32), bwd_idx=torch.zeros((n, T), **i32),
               bwd_ok=torch.zeros((n,), **i32), match_idx=torch.zeros((T, n), **i32),
               cv_centers=torch.zeros((n, T, 3), dtype=torch.float64, device=dev), status=torch.zeros((1,), **i32))
    check(L.fd_forecast_chains(_p(centers), _p(velocity), _p(counts), _p(time), T, n, float(reject_thresh), _p(out["fwd_idx"]),
                               _p(out["fwd_ok"]), _p(out["bwd_idx"]), _p(out["bwd_ok"]), _p(out["match_idx"]), _p(out["cv_centers"]),
                               _p(out["status"]), _stream()), "fd_forecast_chains")
    return out


def det_to_global_boxes(box3d, cs_record=None, pose_record=None):
    """fd_det_to_global_boxes: box3d [n,9] float32 device tensor; cs_record / pose_record = (rotation wxyz, translation xyz)
    or None.  Returns device tensors (center [n,3] f64, quat [n,4] f64, velocity [n,3] f64, size [n,3] f32)."""
    L = _lib.load()
    box3d = _dev(box3d, "box3d", torch.float32)
    n = box3d.shape[0]
    assert box3d.shape[1] == 9, "box3d_lidar rows are (x,y,z,w,l,h,vx,vy,yaw)"
    dev = box3d.device
    center = torch.empty((n, 3), dtype=torch.float64, device=dev)
    quat = torch.empty((n, 4), dtype=torch.float64, device=dev)
    vel = torch.empty((n, 3), dtype=torch.float64, device=dev)
    size = torch.empty((n, 3), dtype=torch.float32, device=dev)

    def rec(r):
        if r is None:
            return None, None
        q, t = (ctypes.c_double * 4)(*[float(v) for v in r[0]]), (ctypes.c_double * 3)(*[float(v) for v in r[1]])
        return q, t

    cq, ct = rec(cs_record)
    pq, pt = rec(pose_record)
    check(L.fd_det_to_global_boxes(_p(box3d), n, cq, ct, pq, pt, _p(center), _p(quat), _p(vel), _p(size), _stream()), "fd_det_to_global_boxes")
    return center, quat, vel, size


def nearest_rows(library, queries):
    """fd_nearest_rows: library [M, D], queries [N, D] float64 device tensors -> int32 [N] index of the nearest library row"""
    L = _lib.load()
    library, queries = _dev(library, "library", torch.float64), _dev(queries, "queries", torch.float64)
    assert library.shape[1] == queries.shape[1]
    idx = torch.zeros((max(queries.shape[0], 1),), dtype=torch.int32, device=queries.device)[: queries.shape[0]]
    check(L.fd_nearest_rows(_p(library), library.shape[0], _p(queries), queries.shape[0], library.shape[1], _p(idx), _stream()), "fd_nearest_rows")
    return idx


def forecast_groups(centers, match_thresh):
    """fd_forecast_groups: centers [n,3] float64 device tensor -> int32 [n] component ids (multi_future's forecast_id)."""
    L = _lib.load()
    centers = _dev(centers, "centers", torch.float64)
    n = centers.shape[0]
    ids = torch.zeros((max(n, 1),), dtype=torch.int32, device=centers.device)[:n]
    check(L.fd_forecast_groups(_p(centers), n, float(match_thresh), _p(ids), _stream()), "fd_forecast_groups")
    return ids


class ForecastOutputs(object):
    """The device buffers of fd_forecast_from_detections for a batch of B sweeps with T steps of up to ``post`` boxes: allocated once,
    written by every call (fixed shapes: they can be the static outputs of a captured graph).  ``host()`` copies them to numpy."""

    FIELDS = (("center", (-1, -2, 3), torch.float64), ("quat", (-1, -2, 4), torch.float64), ("velocity", (-1, -2, 3), torch.float64),
              ("size", (-1, -2, 3), torch.float32), ("fwd_idx", (-3, -1), torch.int32), ("fwd_ok", (-3,), torch.int32),
              ("bwd_idx", (-3, -1), torch.int32), ("bwd_ok", (-3,), torch.int32), ("match_idx", (-1, -3), torch.int32),
              ("cv_centers", (-3, -1, 3), torch.float64), ("status", (), torch.int32), ("traj_kind", (-4,), torch.int32),
              ("traj_src", (-4,), torch.int32), ("traj_first", (-4,), torch.int32), ("traj_group", (-4,), torch.int32), ("n_traj", (), torch.int32))

    def __init__(self, B, T, post, device):
        self.B, self.T, self.post = int(B), int(T), int(post)
        sub = {-1: self.T, -2: self.post, -3: self.post, -4: 3 * self.post}
        # ONE allocation, every array a 16-byte aligned view of it: the whole result goes to the host in one copy (``blob``)
        layout, off = [], 0
        for name, shape, dt in self.FIELDS:
            shape = (self.B,) + tuple(sub.get(d, d) for d in shape)
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            layout.append((name, shape, dt, off, nbytes))
            off = (off + nbytes + 15) & ~15
        self.layout = layout
        self.blob = torch.zeros((off,), dtype=torch.uint8, device=device)
        for name, shape, dt, o, nbytes in layout:
            setattr(self, name, self.blob[o:o + nbytes].view(dt).view(shape))
        self.c_struct = _lib.ForecastBuffers(**{name: getattr(self, name).data_ptr() for name, _, _ in self.FIELDS})

    def views_of(self, blob_host):
        """the named arrays of a HOST copy of ``blob`` (numpy views, no copy)"""
        a = blob_host.numpy() if isinstance(blob_host, torch.Tensor) else np.asarray(blob_host)
        npdt = {torch.float64: np.float64, torch.float32: np.float32, torch.int32: np.int32}
        return {name: a[o:o + nbytes].view(npdt[dt]).reshape(shape) for name, shape, dt, o, nbytes in self.layout}

    def host(self):
        return self.views_of(self.blob.cpu())


def forecast_from_detections(packed, counts, time, records=None, reject_thresh=2.0, match_thresh=0.25, out=None):
    """fd_forecast_from_detections: packed [B,T,post,F>=9] float32, counts [B,T] int32, time [B,T-1] float64, records [B,14] float64 or
    None (all device tensors) -> ForecastOutputs (``out`` is reused when given).  Three launches, no synchronisation."""
    L = _lib.load()
    packed = _dev(packed, "packed", torch.float32)
    counts = _dev(counts, "counts", torch.int32)
    time = _dev(time, "time", torch.float64)
    B, T, post, F = packed.shape
    assert tuple(counts.shape) == (B, T) and tuple(time.shape) == (B, T - 1)
    if records is not None:
        records = _dev(records, "records", torch.float64)
        assert tuple(records.shape) == (B, 14)
    if out is None:
        out = ForecastOutputs(B, T, post, packed.device)
    assert (out.B, out.T, out.post) == (B, T, post)
    check(L.fd_forecast_from_detections(_p(packed), _p(counts), B, T, post, F, _p(records), _p(time), float(reject_thresh), float(match_thresh),
                                        ctypes.byref(out.c_struct), _stream()), "fd_forecast_from_detections")
    return out


# ---- training: the fused optimiser step (fd_optim.hip) ----------------------------------------------------------------------------
OPTIM_DECAY, OPTIM_HAS_GRAD = 1, 2  # FD_OPTIM_DECAY / FD_OPTIM_HAS_GRAD


def optim_chunk():
    return int(_lib.load().fd_optim_chunk())


def optim_layout(numels, chunk):
    """Host side of fd_optim_table for tensors of ``numels`` elements: (offsets int64 [n] -- each segment starts on a 16-byte boundary --,
    total floats of a flat buffer, chunks int32 [n_chunks, 2] of (tensor, index of the chunk inside the tensor))."""
    offsets, chunks, total = [], [], 0
    for t, n in enumerate(numels):
        n = int(n)
        if n <= 0:
            raise ValueError("tensor %d of the optimiser table is empty" % t)
        offsets.append(total)
        total += (n + 3) // 4 * 4
        chunks += [(t, k) for k in range((n + chunk - 1) // chunk)]
    return np.asarray(offsets, dtype=np.int64), total, np.asarray(chunks, dtype=np.int32).reshape(-1, 2)


class AdamTable(object):
    """The device-side description of a parameter set (struct fd_optim_table) with its flat gradient / exp_avg / exp_avg_sq buffers and
    per-tensor step counts.  Built once; ``sync_pointers`` re-uploads the pointer table only when a parameter's storage has moved and
    ``set_has_grad`` the flags only when the set of tensors with a gradient has changed -- both with non-blocking copies from fresh
    pinned memory, so a step never waits for the device."""

    def __init__(self, params, decay):
        params = list(params)
        if not params:
            raise ValueError("the optimiser got no parameters")
        for i, p in enumerate(params):
            _dev(p, "parameter %d" % i, torch.float32)
            if p.device != params[0].device:
                raise FutureDetHipError("parameter %d lives on %s, the others on %s" % (i, p.device, params[0].device))
        self.params, self.device = params, params[0].device
        self.chunk = optim_chunk()
        self.numel = [p.numel() for p in params]
        offsets, self.total, chunks = optim_layout(self.numel, self.chunk)
        self.offsets = [int(o) for o in offsets]
        n, dev = len(params), self.device
        self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros(self.total, dtype=torch.float32, device=dev) for _ in range(3))
        self.step = torch.zeros(n, dtype=torch.int32, device=dev)
        self._coef = torch.zeros(2 * n, dtype=torch.float32, device=dev)
        self._partials = torch.zeros(len(chunks), dtype=torch.float64, device=dev)
        self.norm = torch.zeros(2, dtype=torch.float32, device=dev)
        self._numel_dev = torch.tensor(self.numel, dtype=torch.int64, device=dev)
        self._offset_dev = torch.from_numpy(offsets).to(dev)
        self._chunks_dev = torch.from_numpy(chunks).to(dev)
        self._ptrs_dev = torch.zeros(n, dtype=torch.int64, device=dev)
        self._flags_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self.decay = [bool(d) for d in decay]
        assert len(self.decay) == n
        self._ptrs, self._has_grad = None, None
        self.sync_pointers()
        self.set_has_grad([True] * n)
        self.c_struct = _lib.OptimTable(
            params=self._ptrs_dev.data_ptr(), numel=self._numel_dev.data_ptr(), offset=self._offset_dev.data_ptr(), flags=self._flags_dev.data_ptr(),
            step=self.step.data_ptr(), coef=self._coef.data_ptr(), chunks=self._chunks_dev.data_ptr(), partials=self._partials.data_ptr(),
            norm=self.norm.data_ptr(), grad=self.grad.data_ptr(), exp_avg=self.exp_avg.data_ptr(), exp_avg_sq=self.exp_avg_sq.data_ptr(),
            total=self.total, n_tensors=n, n_chunks=len(chunks), chunk=self.chunk)

    @staticmethod
    def _upload(dst, values, np_dtype):
        dst.copy_(torch.from_numpy(np.asarray(values, dtype=np_dtype)).pin_memory(), non_blocking=True)

    def segment(self, flat, i):
        """tensor i's view of one of the flat buffers, shaped like the parameter"""
        return flat[self.offsets[i]:self.offsets[i] + self.numel[i]].view(self.params[i].shape)

    def sync_pointers(self):
        ptrs = [p.data_ptr() for p in self.params]
        if ptrs != self._ptrs:
            for i, p in enumerate(self.params):
                if not p.is_contiguous() or p.numel() != self.numel[i]:
                    raise FutureDetHipError("parameter %d changed its shape or is no longer contiguous" % i)
            self._upload(self._ptrs_dev, ptrs, np.int64)  # device addresses lie below 2^63
            self._ptrs = ptrs

    def set_has_grad(self, has_grad):
        if has_grad != self._has_grad:
            self._upload(self._flags_dev, [(OPTIM_DECAY if d else 0) | (OPTIM_HAS_GRAD if h else 0) for d, h in zip(self.decay, has_grad)], np.int32)
            self._has_grad = list(has_grad)


def optim_zero_grad(table):
    """fd_optim_zero_grad: zeroes the flat gradient buffer of an AdamTable (one launch)."""
    check(_lib.load().fd_optim_zero_grad(ctypes.byref(table.c_struct), _stream()), "fd_optim_zero_grad")


def optim_adam_step(table, lr, beta1, beta2, eps, wd, max_norm=0.0):
    """fd_optim_adam_step on an AdamTable: decay, gradient clipping (max_norm > 0; total_norm and the coefficient land in table.norm) and
    Adam for every tensor, in at most three launches.  No allocation, no synchronisation."""
    check(_lib.load().fd_optim_adam_step(ctypes.byref(table.c_struct), float(lr), float(beta1), float(beta2), float(eps), float(wd), float(max_norm),
                                         _stream()), "fd_optim_adam_step")


HYPER_FIELDS = ("lr", "beta1", "beta2", "eps", "wd", "max_norm")  # the device record of fd_optim_adam_step_dev, in this order


def check_hyper(lr, beta1, beta2, eps, wd, max_norm):
    """What fd_optim_adam_step refuses on the host, for values that travel through device memory: -> the six python floats"""
    v = [float(x) for x in (lr, beta1, beta2, eps, wd, max_norm)]
    if not (0.0 <= v[1] < 1.0 and 0.0 <= v[2] < 1.0):
        raise ValueError("optimiser hyper-parameters: betas (%g, %g) must lie in [0, 1)" % (v[1], v[2]))
    if not v[3] > 0.0:
        raise ValueError("optimiser hyper-parameters: eps must be > 0 (got %g)" % v[3])
    if v[0] != v[0] or v[4] != v[4] or v[5] != v[5]:
        raise ValueError("optimiser hyper-parameters: lr, wd or max_norm is NaN")
    return v


def optim_adam_step_dev(table, hyper, clip, skip=None):
    """fd_optim_adam_step_dev on an AdamTable: ``hyper`` float64 [6] on the device (HYPER_FIELDS; validate with check_hyper before the
    upload), ``clip`` a host bool (it fixes the launch count), ``skip`` int32 [1] on the device or None.  No allocation, no
    synchronisation; the same bits as optim_adam_step for the same six values."""
    hyper = _dev(hyper, "hyper", torch.float64)
    if hyper.numel() != len(HYPER_FIELDS):
        raise FutureDetHipError("hyper must hold %d doubles (%s), got %d" % (len(HYPER_FIELDS), ", ".join(HYPER_FIELDS), hyper.numel()))
    if skip is not None:
        _dev(skip, "skip", torch.int32)
    check(_lib.load().fd_optim_adam_step_dev(ctypes.byref(table.c_struct), _p(hyper), int(bool(clip)), _p(skip), _stream()), "fd_optim_adam_step_dev")


def rows_colsum_chunk():
    return int(_lib.load().fd_rows_colsum_chunk())


def rows_colsum(x, n_dev=None):
    """fd_rows_colsum: fp32 [C] = the sum of the first min(n, n_dev[0]) rows of x [n, C] (fp32 or bf16; n_dev None: all rows), summed in
    double in a fixed order.  The rows behind the count are never read."""
    L = _lib.load()
    x = _dev(x, "x")
    if x.dtype not in _DT or x.dim() != 2:
        raise FutureDetHipError("rows_colsum: x must be a float32 or bfloat16 [n, C] tensor (got %s %s)" % (tuple(x.shape), x.dtype))
    n, c = x.shape
    out = torch.empty((c,), dtype=torch.float32, device=x.device)
    ws = workspace.get("rows_colsum", L.fd_rows_colsum_workspace_bytes(n, c), x.device)
    check(L.fd_rows_colsum(_p(x) if n else None, n, _p(n_dev), c, _DT[x.dtype], _p(out), _p(ws), ws.numel(), _stream()), "fd_rows_colsum")
    return out


def levels_overflow(counts, caps, flag=None):
    """fd_levels_overflow: flag[0] (int32 on the device) = any counts[l] > caps[l]; counts / caps int32 device tensors of one length"""
    counts, caps = _dev(counts, "counts", torch.int32), _dev(caps, "caps", torch.int32)
    if counts.numel() != caps.numel():
        raise FutureDetHipError("levels_overflow: %d counts, %d capacities" % (counts.numel(), caps.numel()))
    if flag is None:
        flag = torch.empty((1,), dtype=torch.int32, device=counts.device)
    check(_lib.load().fd_levels_overflow(_p(counts), _p(caps), counts.numel(), _p(_dev(flag, "flag", torch.int32)), _stream()), "fd_levels_overflow")
    return flag


# ---- training: the global augmentation (fd_augment.hip) ---------------------------------------------------------------------------
AUGMENT_RECORD_DOUBLES = ctypes.sizeof(_lib.AugmentRecord) // 8  # a record travels as 6 float64 words (48 bytes, 8-byte aligned)


def _augment_records(rec, name, n):
    rec = _dev(rec, name, torch.float64)
    if rec.numel() != n * AUGMENT_RECORD_DOUBLES:
        raise FutureDetHipError("%s must hold %d record(s) of %d float64 words (augment.GlobalAugment.record), got %s"
                                % (name, n, AUGMENT_RECORD_DOUBLES, tuple(rec.shape)))
    return rec


def augment_points(src, rec, dst, perm=None, n_rows=None):
    """fd_augment_points: dst[i] = A(src[perm[i]]) (perm None: src[i]) for the first ``n_rows`` (default: all) rows of src [n, 4 | 5] fp32;
    dst [>= n_rows, ndim] is another buffer and keeps its rows at or past n_rows.  ``rec``: ONE sample's record on the device (float64
    [6], a row of GlobalAugment.record's upload), ``perm``: int32 [>= n_rows] on the device.  One launch, no allocation, no
    synchronisation.  Returns dst."""
    src, dst = _dev(src, "src", torch.float32), _dev(dst, "dst", torch.float32)
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] not in (4, 5) or dst.shape[1] != src.shape[1]:
        raise FutureDetHipError("augment_points: src and dst must be [n, 4] or [n, 5] rows of one width (got %s and %s)"
                                % (tuple(src.shape), tuple(dst.shape)))
    n = int(src.shape[0]) if n_rows is None else int(n_rows)
    if not 0 <= n <= min(int(src.shape[0]), int(dst.shape[0])):
        raise FutureDetHipError("augment_points: n_rows = %d does not fit src %s and dst %s" % (n, tuple(src.shape), tuple(dst.shape)))
    if src.device != dst.device:
        raise FutureDetHipError("augment_points: src and dst live on different devices")
    rec = _augment_records(rec, "rec", 1)
    if perm is not None:
        perm = _dev(perm, "perm", torch.int32)
        if perm.dim() != 1 or perm.numel() < n:
            raise FutureDetHipError("augment_points: perm must be an int32 vector of at least n_rows = %d entries (got %s)" % (n, tuple(perm.shape)))
    check(_lib.load().fd_augment_points(_p(src), n, int(src.shape[1]), _p(perm), _p(rec), _p(dst), _stream()), "fd_augment_points")
    return dst


def augment_boxes(boxes, counts, recs, out=None):
    """fd_augment_boxes: out [B, T, n_max, 12] = the box rows below counts [B, T] (int32, device) transformed with recs [B] (float64
    [B, 6]), the padding rows copied.  ``out`` None: a new tensor; ``out is boxes``: in place.  One launch, no synchronisation."""
    boxes = _dev(boxes, "boxes", torch.float32)
    if boxes.dim() != 4 or boxes.shape[3] != 12 or boxes.shape[0] < 1 or boxes.shape[1] < 1:
        raise FutureDetHipError("augment_boxes: boxes must be [B, T, n_max, 12] (got %s)" % (tuple(boxes.shape),))
    B, T, n_max = (int(v) for v in boxes.shape[:3])
    counts = _dev(counts, "counts", torch.int32)
    if tuple(counts.shape) != (B, T):
        raise FutureDetHipError("augment_boxes: counts must be int32 [%d, %d] (got %s)" % (B, T, tuple(counts.shape)))
    recs = _augment_records(recs, "recs", B)
    if out is None:
        out = torch.empty_like(boxes)
    out = _dev(out, "out", torch.float32)
    if tuple(out.shape) != tuple(boxes.shape) or out.device != boxes.device:
        raise FutureDetHipError("augment_boxes: out %s does not match boxes %s" % (tuple(out.shape), tuple(boxes.shape)))
    check(_lib.load().fd_augment_boxes(_p(boxes), _p(counts), _p(recs), _p(out), B, T, n_max, _stream()), "fd_augment_boxes")
    return out


# ---- training: the GT range filter and the bev-mask warp (fd_augment_map.hip) -----------------------------------------------------
AUGMENT_MASK_RECORD_DOUBLES = ctypes.sizeof(_lib.AugmentMaskRecord) // 8  # a mask record travels as 13 float64 words (104 bytes)


def _gt_filter_inputs(what, boxes, counts, classes, trajectory):
    """the padded ground truth of the two filters, checked: (ins, names, B, T, n_max)"""
    boxes = _dev(boxes, "boxes", torch.float32)
    if boxes.dim() != 4 or boxes.shape[3] != 12 or min(boxes.shape[:3]) < 1:
        raise FutureDetHipError("%s: boxes must be [B, T, n_max, 12] with B, T, n_max >= 1 (got %s)" % (what, tuple(boxes.shape),))
    B, T, n_max = (int(v) for v in boxes.shape[:3])
    ins = [boxes, _dev(counts, "counts", torch.int32), _dev(classes, "classes", torch.int32),
           _dev(trajectory, "trajectory", torch.int32) if trajectory is not None else None]
    shapes = [tuple(boxes.shape), (B, T), (B, T, n_max), (B, T, n_max)]
    names = ["boxes", "counts", "classes", "trajectory"]
    for t, shape, name in zip(ins, shapes, names):
        if t is not None and (tuple(t.shape) != shape or t.device != boxes.device):
            raise FutureDetHipError("%s: %s must be %s on %s (got %s on %s)" % (what, name, list(shape), boxes.device, tuple(t.shape), t.device))
    return ins, names, B, T, n_max


def _gt_filter_outputs(what, ins, names, out, status):
    """``out`` (None, "inplace" or four tensors) and ``status`` of the two filters, checked: (outs, status)"""
    boxes, B = ins[0], int(ins[0].shape[0])
    if isinstance(out, str):
        if out != "inplace":
            raise FutureDetHipError("%s: out must be None, \"inplace\" or a tuple of four tensors" % what)
        outs = list(ins)
    elif out is None:
        outs = [torch.empty_like(t) if t is not None else None for t in ins]
    else:
        outs = list(out)
        if len(outs) != 4:
            raise FutureDetHipError("%s: out takes (boxes, counts, classes, trajectory | None)" % what)
        for i, (t, src, name) in enumerate(zip(outs, ins, names)):
            if src is None:
                outs[i] = None
                continue
            t = _dev(t, name + "_out", src.dtype)
            if tuple(t.shape) != tuple(src.shape) or t.device != src.device:
                raise FutureDetHipError("%s: %s_out %s does not match %s %s" % (what, name, tuple(t.shape), name, tuple(src.shape)))
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=boxes.device)
    status = _dev(status, "status", torch.int32)
    if status.numel() != B or status.device != boxes.device:
        raise FutureDetHipError("%s: status must be int32 [%d] on %s (got %s)" % (what, B, boxes.device, tuple(status.shape)))
    return outs, status


def gt_range_filter(boxes, counts, classes, pc_range, trajectory=None, out=None, status=None):
    """fd_gt_range_filter: drops, at every timestep, the objects whose timestep-0 box has no BEV corner strictly inside ``pc_range``
    (xmin, ymin, xmax, ymax) and moves the kept rows to the front.  boxes [B, T, n_max, 12] fp32, counts [B, T] int32, classes and
    ``trajectory`` (or None) [B, T, n_max] int32, all on the device.  ``out``: None = new tensors, "inplace" = the inputs themselves, or
    a tuple (boxes, counts, classes, trajectory | None) of tensors shaped like the inputs (each may be its input).  Rows at or past the
    new counts are zeros.  ``status`` int32 [B] (None: new) receives the number of timesteps whose count differs from timestep 0's.
    Returns (boxes, counts, classes, trajectory | None, status).  One launch, no synchronisation."""
    ins, names, B, T, n_max = _gt_filter_inputs("gt_range_filter", boxes, counts, classes, trajectory)
    rng = [float(v) for v in pc_range]
    if len(rng) != 4:
        raise FutureDetHipError("gt_range_filter: pc_range takes (xmin, ymin, xmax, ymax), got %d values" % len(rng))
    outs, status = _gt_filter_outputs("gt_range_filter", ins, names, out, status)
    check(_lib.load().fd_gt_range_filter(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), rng[0], rng[1], rng[2], rng[3], _p(outs[0]), _p(outs[1]),
                                         _p(outs[2]), _p(outs[3]), _p(status), B, T, n_max, _stream()), "fd_gt_range_filter")
    return outs[0], outs[1], outs[2], outs[3], status


def gt_min_points_filter(boxes, counts, classes, point_counts, min_points, trajectory=None, out=None, status=None):
    """fd_gt_min_points_filter: gt_range_filter with another mask -- object i of sample b is kept, at every timestep, iff
    ``point_counts[b, i] >= min_points``; point_counts int32 [B, n_max] on the device (points_in_boxes_count of the sample's cloud and its
    timestep-0 boxes), never an output.  Arguments, ``out``, ``status`` and the return value as for gt_range_filter.  One launch, no
    synchronisation."""
    ins, names, B, T, n_max = _gt_filter_inputs("gt_min_points_filter", boxes, counts, classes, trajectory)
    point_counts = _dev(point_counts, "point_counts", torch.int32)
    if tuple(point_counts.shape) != (B, n_max) or point_counts.device != ins[0].device:
        raise FutureDetHipError("gt_min_points_filter: point_counts must be int32 [%d, %d] on %s (got %s on %s)"
                                % (B, n_max, ins[0].device, tuple(point_counts.shape), point_counts.device))
    outs, status = _gt_filter_outputs("gt_min_points_filter", ins, names, out, status)
    check(_lib.load().fd_gt_min_points_filter(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(point_counts), int(min_points), _p(outs[0]),
                                              _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(status), B, T, n_max, _stream()), "fd_gt_min_points_filter")
    return outs[0], outs[1], outs[2], outs[3], status


def augment_mask_check(recs, H, W):
    """fd_augment_mask_check on host records (a numpy array [B] of augment.MASK_RECORD_DTYPE): raises when a matrix would map a pixel of
    an H x W plane out of the fixed-point range.  No device work."""
    import numpy as np

    recs = np.ascontiguousarray(recs)
    if recs.dtype.itemsize != 8 * AUGMENT_MASK_RECORD_DOUBLES or recs.ndim != 1 or recs.shape[0] < 1:
        raise FutureDetHipError("augment_mask_check: recs must be a vector of %d-byte mask records" % (8 * AUGMENT_MASK_RECORD_DOUBLES))
    check(_lib.load().fd_augment_mask_check(ctypes.c_void_p(recs.ctypes.data), int(recs.shape[0]), int(H), int(W)), "fd_augment_mask_check")


def augment_mask(src, recs, out=None):
    """fd_augment_mask: out [B, C, H, W] fp32 = warp(warp(flip(src), m1), m2) per plane with recs [B] (float64 [B, 13] on the device,
    GlobalAugment.mask_record's upload).  ``out`` None: a new tensor; it must not be src.  One launch, no synchronisation."""
    src = _dev(src, "src", torch.float32)
    if src.dim() != 4 or min(src.shape) < 1:
        raise FutureDetHipError("augment_mask: src must be [B, C, H, W] with no empty axis (got %s)" % (tuple(src.shape),))
    B, C, H, W = (int(v) for v in src.shape)
    recs = _dev(recs, "recs", torch.float64)
    if recs.numel() != B * AUGMENT_MASK_RECORD_DOUBLES or recs.device != src.device:
        raise FutureDetHipError("augment_mask: recs must hold %d record(s) of %d float64 words on %s (augment.GlobalAugment.mask_record), got %s"
                                % (B, AUGMENT_MASK_RECORD_DOUBLES, src.device, tuple(recs.shape)))
    if out is None:
        out = torch.empty_like(src)
    out = _dev(out, "out", torch.float32)
    if tuple(out.shape) != tuple(src.shape) or out.device != src.device:
        raise FutureDetHipError("augment_mask: out %s does not match src %s" % (tuple(out.shape), tuple(src.shape)))
    check(_lib.load().fd_augment_mask(_p(src), _p(recs), _p(out), B, C, H, W, _stream()), "fd_augment_mask")
    return out


# ---- training: GT-database sampling (fd_gt_sample.hip) ----------------------------------------------------------------------------
GT_SAMPLE_MAX_K, GT_SAMPLE_MAX_GROUPS = 64, 16                 # FD_GT_SAMPLE_MAX_K / _MAX_GROUPS
GT_SAMPLE_NO_ROW, GT_SAMPLE_NO_POINTS, GT_SAMPLE_COUNTS_DIFFER, GT_SAMPLE_BAD_INDEX = 1, 2, 4, 8  # the bits of status
GT_SAMPLE_SENTINEL = 1e30                                      # FD_GT_SAMPLE_SENTINEL
GT_SAMPLE_PLAN_WORDS = 4                                       # struct fd_gt_sample_plan as int32 words: src_row (2), rows, dst_row


def _gt_database(db, what):
    """the five device arrays of a database (augment.GTDatabase or anything with these attributes), checked against one another"""
    boxes = _dev(db.boxes, "db.boxes", torch.float32)
    if boxes.dim() != 3 or boxes.shape[2] != 12 or boxes.shape[0] < 1 or boxes.shape[1] < 1:
        raise FutureDetHipError("%s: db.boxes must be [M, Tdb, 12] with M, Tdb >= 1 (got %s)" % (what, tuple(boxes.shape)))
    M = int(boxes.shape[0])
    steps, classes, traj = (_dev(getattr(db, k), "db." + k, torch.int32) for k in ("steps", "classes", "trajectory"))
    offsets = _dev(db.offsets, "db.offsets", torch.int64)
    points = _dev(db.points, "db.points", torch.float32)
    if points.dim() != 2 or points.shape[1] not in (4, 5):
        raise FutureDetHipError("%s: db.points must be [P, 4] or [P, 5] (got %s)" % (what, tuple(points.shape)))
    for t, n, name in ((steps, M, "steps"), (classes, M, "classes"), (traj, M, "trajectory"), (offsets, M + 1, "offsets")):
        if tuple(t.shape) != (n,) or t.device != boxes.device:
            raise FutureDetHipError("%s: db.%s must be [%d] on %s (got %s on %s)" % (what, name, n, boxes.device, tuple(t.shape), t.device))
    if points.device != boxes.device:
        raise FutureDetHipError("%s: db.points lives on %s, db.boxes on %s" % (what, points.device, boxes.device))
    return boxes, steps, classes, traj, offsets, points


def gt_sample_groups(groups):
    """a ctypes array of struct fd_gt_sample_group from rows (class_id, trajectory | -1, max_num, first, n)"""
    rows = [tuple(int(v) for v in g) for g in groups]
    if not 1 <= len(rows) <= GT_SAMPLE_MAX_GROUPS or any(len(r) != 5 for r in rows):
        raise FutureDetHipError("gt_sample_select: 1 to %d group records of (class_id, trajectory, max_num, first, n), got %r"
                                % (GT_SAMPLE_MAX_GROUPS, rows))
    return (_lib.GtSampleGroup * len(rows))(*[_lib.GtSampleGroup(*r) for r in rows])


def gt_sample_select(boxes, counts, classes, db, cand, groups, rate, point_cap, trajectory=None, out=None, accepted=None, plan=None,
                     n_points=None, status=None):
    """fd_gt_sample_select: decides, per sample, which of the drawn database entries ``cand`` [B, K] (int32, -1 = empty) are pasted, and
    appends their rows to the padded ground truth boxes [B, T, n_max, 12] / counts [B, T] / classes / ``trajectory`` (or None)
    [B, T, n_max].  ``db``: the device database (augment.GTDatabase); ``groups``: rows (class_id, trajectory | -1, max_num, first, n) or
    gt_sample_groups' array.  ``out``: None = new tensors (rows at or past the new counts are uninitialised), "inplace" = the inputs
    themselves, or a tuple (boxes, counts, classes, trajectory | None) that overlaps no input.  Returns a dict: boxes, counts, classes,
    trajectory, accepted [B, K] int32, plan [B, K, 4] int32 (src_row as two words, rows, dst_row), n_points [B], status [B] (the
    GT_SAMPLE_* bits).  One launch, no synchronisation."""
    boxes = _dev(boxes, "boxes", torch.float32)
    if boxes.dim() != 4 or boxes.shape[3] != 12 or min(boxes.shape[:3]) < 1:
        raise FutureDetHipError("gt_sample_select: boxes must be [B, T, n_max, 12] with B, T, n_max >= 1 (got %s)" % (tuple(boxes.shape),))
    B, T, n_max = (int(v) for v in boxes.shape[:3])
    dev = boxes.device
    ins = [boxes, _dev(counts, "counts", torch.int32), _dev(classes, "classes", torch.int32),
           _dev(trajectory, "trajectory", torch.int32) if trajectory is not None else None]
    names = ["boxes", "counts", "classes", "trajectory"]
    for t, shape, name in zip(ins, [tuple(boxes.shape), (B, T), (B, T, n_max), (B, T, n_max)], names):
        if t is not None and (tuple(t.shape) != shape or t.device != dev):
            raise FutureDetHipError("gt_sample_select: %s must be %s on %s (got %s on %s)" % (name, list(shape), dev, tuple(t.shape), t.device))
    dbb, dbs, dbc, dbt, dbo, dbp = _gt_database(db, "gt_sample_select")
    if dbb.device != dev:
        raise FutureDetHipError("gt_sample_select: the database lives on %s, the batch on %s" % (dbb.device, dev))
    cand = _dev(cand, "cand", torch.int32)
    if cand.dim() != 2 or cand.shape[0] != B or not 1 <= cand.shape[1] <= GT_SAMPLE_MAX_K or cand.device != dev:
        raise FutureDetHipError("gt_sample_select: cand must be int32 [%d, K] with 1 <= K <= %d on %s (got %s)" % (B, GT_SAMPLE_MAX_K, dev, tuple(cand.shape)))
    K = int(cand.shape[1])
    if not isinstance(groups, ctypes.Array):
        groups = gt_sample_groups(groups)
    if isinstance(out, str):
        if out != "inplace":
            raise FutureDetHipError("gt_sample_select: out must be None, \"inplace\" or a tuple of four tensors")
        outs = list(ins)
    elif out is None:
        outs = [torch.empty_like(t) if t is not None else None for t in ins]
    else:
        outs = list(out)
        if len(outs) != 4:
            raise FutureDetHipError("gt_sample_select: out takes (boxes, counts, classes, trajectory | None)")
        for i, (t, src, name) in enumerate(zip(outs, ins, names)):
            if src is None:
                outs[i] = None
                continue
            t = _dev(t, name + "_out", src.dtype)
            if tuple(t.shape) != tuple(src.shape) or t.device != dev:
                raise FutureDetHipError("gt_sample_select: %s_out %s does not match %s %s" % (name, tuple(t.shape), name, tuple(src.shape)))

    def small(t, shape, name):
        if t is None:
            return torch.empty(shape, dtype=torch.int32, device=dev)
        t = _dev(t, name, torch.int32)
        if tuple(t.shape) != shape or t.device != dev:
            raise FutureDetHipError("gt_sample_select: %s must be int32 %s on %s (got %s)" % (name, list(shape), dev, tuple(t.shape)))
        return t

    accepted, plan = small(accepted, (B, K), "accepted"), small(plan, (B, K, GT_SAMPLE_PLAN_WORDS), "plan")
    n_points, status = small(n_points, (B,), "n_points"), small(status, (B,), "status")
    check(_lib.load().fd_gt_sample_select(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(dbb), _p(dbs), _p(dbc), _p(dbt), _p(dbo),
                                          int(dbb.shape[0]), int(dbb.shape[1]), int(dbp.shape[0]), _p(cand), groups, len(groups), float(rate),
                                          int(point_cap), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(accepted), _p(plan),
                                          _p(n_points), _p(status), B, T, n_max, K, _stream()), "fd_gt_sample_select")
    return dict(boxes=outs[0], counts=outs[1], classes=outs[2], trajectory=outs[3], accepted=accepted, plan=plan, n_points=n_points,
                status=status)


def gt_sample_points(db, cand, accepted, plan, dst, point_cap):
    """fd_gt_sample_points for ONE sample: cand / accepted int32 [K] and plan int32 [K, 4], the sample's rows of gt_sample_select's
    arrays.  Fills the rows [0, point_cap) of dst [>= point_cap, ndim] (ndim = the database's) with the accepted entries' points, moved
    to their boxes' centres, and sentinel rows (1e30, 1e30, 1e30, 0[, 0]) behind them; later rows are not written.  One launch, no
    synchronisation.  Returns dst."""
    dbb, _, _, _, _, dbp = _gt_database(db, "gt_sample_points")
    dst = _dev(dst, "dst", torch.float32)
    point_cap = int(point_cap)
    if dst.dim() != 2 or dst.shape[1] != dbp.shape[1] or not 0 <= point_cap <= dst.shape[0] or dst.device != dbp.device:
        raise FutureDetHipError("gt_sample_points: dst must be [>= point_cap = %d, %d] on %s (got %s on %s)"
                                % (point_cap, dbp.shape[1], dbp.device, tuple(dst.shape), dst.device))
    cand, accepted, plan = _dev(cand, "cand", torch.int32), _dev(accepted, "accepted", torch.int32), _dev(plan, "plan", torch.int32)
    K = int(cand.numel())
    if cand.dim() != 1 or not 1 <= K <= GT_SAMPLE_MAX_K or tuple(accepted.shape) != (K,) or tuple(plan.shape) != (K, GT_SAMPLE_PLAN_WORDS):
        raise FutureDetHipError("gt_sample_points: cand and accepted must be int32 [K], plan int32 [K, %d], 1 <= K <= %d (got %s, %s, %s)"
                                % (GT_SAMPLE_PLAN_WORDS, GT_SAMPLE_MAX_K, tuple(cand.shape), tuple(accepted.shape), tuple(plan.shape)))
    if cand.device != dst.device or accepted.device != dst.device or plan.device != dst.device:
        raise FutureDetHipError("gt_sample_points: cand, accepted and plan must live on %s" % (dst.device,))
    check(_lib.load().fd_gt_sample_points(_p(dbp), int(dbp.shape[0]), int(dbp.shape[1]), _p(dbb), int(dbb.shape[0]), int(dbb.shape[1]), _p(cand),
                                          _p(accepted), _p(plan), K, _p(dst), point_cap, _stream()), "fd_gt_sample_points")
    return dst



# ---- training: points in rotated boxes (fd_points_in_boxes.hip) -------------------------------------------------------------------
POINTS_IN_BOXES_NO_ROOM = 1   # FD_POINTS_IN_BOXES_NO_ROOM
POINTS_IN_BOXES_MAX_N = 4096  # FD_RANGE_FILTER_MAX_N: the boxes of one call


def _points_in_boxes_inputs(what, points, boxes, n_boxes):
    points, boxes = _dev(points, "points", torch.float32), _dev(boxes, "boxes", torch.float32)
    if points.dim() != 2 or points.shape[1] not in (4, 5):
        raise FutureDetHipError("%s: points must be [n, 4] or [n, 5] (got %s)" % (what, tuple(points.shape)))
    if boxes.dim() != 2 or boxes.shape[1] < 7 or boxes.shape[0] > POINTS_IN_BOXES_MAX_N:
        raise FutureDetHipError("%s: boxes must be [n_boxes <= %d, >= 7] (got %s)" % (what, POINTS_IN_BOXES_MAX_N, tuple(boxes.shape)))
    if boxes.device != points.device:
        raise FutureDetHipError("%s: points live on %s, boxes on %s" % (what, points.device, boxes.device))
    if n_boxes is not None:
        n_boxes = _dev(n_boxes, "n_boxes", torch.int32)
        if n_boxes.numel() != 1 or n_boxes.device != points.device:
            raise FutureDetHipError("%s: n_boxes must be ONE int32 on %s (got %s on %s)" % (what, points.device, tuple(n_boxes.shape), n_boxes.device))
    return points, boxes, n_boxes


def points_in_boxes_workspace(n_points, n_boxes_max, device):
    """a new uint8 tensor of fd_points_in_boxes_workspace_bytes(n_points, n_boxes_max) bytes (at least 4) for the two calls below"""
    return torch.empty((max(int(_lib.load().fd_points_in_boxes_workspace_bytes(int(n_points), int(n_boxes_max))), 4),), dtype=torch.uint8, device=device)


def points_in_boxes_count(points, boxes, n_boxes=None, out=None, workspace=None):
    """fd_points_in_boxes_count: int32 [n_boxes_max] = the points of ``points`` [n, 4 | 5] inside each row of ``boxes`` [n_boxes_max, >= 7]
    (centre, dims, ..., the angle in the LAST column); ``n_boxes``: one int32 on the device, the rows at or past it are no boxes (count
    0).  ``out`` int32 [n_boxes_max] and ``workspace`` (uint8, points_in_boxes_workspace) let a step keep static buffers; None = new
    tensors.  Returns (counts, workspace): the workspace is what points_in_boxes_extract reads.  Two launches, no synchronisation."""
    points, boxes, n_boxes = _points_in_boxes_inputs("points_in_boxes_count", points, boxes, n_boxes)
    n, m = int(points.shape[0]), int(boxes.shape[0])
    if out is None:
        out = torch.empty((m,), dtype=torch.int32, device=points.device)
    out = _dev(out, "out", torch.int32)
    if tuple(out.shape) != (m,) or out.device != points.device:
        raise FutureDetHipError("points_in_boxes_count: out must be int32 [%d] on %s (got %s on %s)" % (m, points.device, tuple(out.shape), out.device))
    if workspace is None:
        workspace = points_in_boxes_workspace(n, m, points.device)
    workspace = _dev(workspace, "workspace", torch.uint8)
    check(_lib.load().fd_points_in_boxes_count(_p(points), n, int(points.shape[1]), _p(boxes), m, int(boxes.shape[1]), _p(n_boxes), _p(out),
                                               _p(workspace), workspace.numel(), _stream()), "fd_points_in_boxes_count")
    return out, workspace


def points_in_boxes_extract(points, boxes, workspace, rows, n_boxes=None, offsets=None, status=None):
    """fd_points_in_boxes_extract on the inputs and the workspace of a points_in_boxes_count call: fills ``rows`` [cap_rows, ncols <= ndim]
    fp32 box after box with each box's points in their cloud order, columns 0..2 minus the box centre, and ``offsets`` int64
    [n_boxes_max + 1] (None: new); ``status`` int32 [1] (None: new) gets POINTS_IN_BOXES_NO_ROOM when rows is too short (the rows that
    fit are written).  Returns (rows, offsets, status).  One launch, no synchronisation."""
    points, boxes, n_boxes = _points_in_boxes_inputs("points_in_boxes_extract", points, boxes, n_boxes)
    n, m, dev = int(points.shape[0]), int(boxes.shape[0]), points.device
    workspace, rows = _dev(workspace, "workspace", torch.uint8), _dev(rows, "rows", torch.float32)
    if rows.dim() != 2 or not 1 <= rows.shape[1] <= points.shape[1] or rows.device != dev:
        raise FutureDetHipError("points_in_boxes_extract: rows must be [cap_rows, 1..%d] on %s (got %s on %s)"
                                % (points.shape[1], dev, tuple(rows.shape), rows.device))
    if offsets is None:
        offsets = torch.empty((m + 1,), dtype=torch.int64, device=dev)
    offsets = _dev(offsets, "offsets", torch.int64)
    if status is None:
        status = torch.empty((1,), dtype=torch.int32, device=dev)
    status = _dev(status, "status", torch.int32)
    if tuple(offsets.shape) != (m + 1,) or status.numel() != 1 or offsets.device != dev or status.device != dev:
        raise FutureDetHipError("points_in_boxes_extract: offsets must be int64 [%d] and status int32 [1] on %s (got %s, %s)"
                                % (m + 1, dev, tuple(offsets.shape), tuple(status.shape)))
    check(_lib.load().fd_points_in_boxes_extract(_p(points), n, int(points.shape[1]), _p(boxes), m, int(boxes.shape[1]), _p(n_boxes), _p(workspace),
                                                 workspace.numel(), _p(rows) if rows.shape[0] else None, int(rows.shape[0]), int(rows.shape[1]),
                                                 _p(offsets), _p(status), _stream()), "fd_points_in_boxes_extract")
    return rows, offsets, status

# ---- training: the fused CenterHead loss (fd_loss.hip) ----------------------------------------------------------------------------
LOSS_MAPS = ("reg", "height", "dim", "vel", "rvel", "rot", "rrot")  # fd_loss_task.maps / d_maps, in this order


def loss_chunk():
    """Heat-map elements per workgroup of the loss kernels (fd_loss_chunk())."""
    return int(_lib.load().fd_loss_chunk())


def loss_columns(D, row_stride):
    """Target-row column of every predicted channel, the three branches of CenterHead.loss: 14 channels read the row as it is,
    10 read [0..7, -2, -1] and 8 (no velocity) read [0..5, -2, -1]."""
    if D == 14:
        return list(range(14))
    if D == 10:
        return list(range(8)) + [row_stride - 2, row_stride - 1]
    if D == 8:
        return list(range(6)) + [row_stride - 2, row_stride - 1]
    raise ValueError("CenterHead loss: 8, 10 or 14 box channels (got %d)" % D)


def make_loss_cfg(B, H, W, M, n_tasks, dense, T, D, row_stride, code_weights, code_weights_forecast=None, weight=0.25):
    """lib.LossCfg (struct fd_loss_cfg) of one head mode and batch shape; the code weights are python floats and stay doubles."""
    c = _lib.LossCfg()
    c.B, c.H, c.W, c.M, c.n_tasks, c.dense, c.T, c.D, c.row_stride = int(B), int(H), int(W), int(M), int(n_tasks), int(bool(dense)), int(T), int(D), int(row_stride)
    if D in (8, 10, 14):
        if len(code_weights) != D or (code_weights_forecast is not None and len(code_weights_forecast) != D):
            raise ValueError("CenterHead loss: %d code weights for %d box channels" % (len(code_weights), D))
        for i, col in enumerate(loss_columns(D, row_stride)):
            c.col[i] = col
        for i in range(D):
            c.code_weights[i] = float(code_weights[i])
            c.code_weights_forecast[i] = float(code_weights_forecast[i]) if code_weights_forecast is not None else 0.0
    c.weight = float(weight)
    return c


def loss_terms_layout(cfg):
    """(floats per task, terms per task S) of the terms vector: loss, hm_loss, num_pos, num_positive, loc_loss[S], loc_loss_elem[S][D]
    per task, then one status word."""
    S = 1 if cfg.dense else cfg.T
    return 4 + S + S * cfg.D, S


def _loss_tasks(cfg, tasks, sigs=None, grads=None):
    """The fd_loss_task array of a call.  ``tasks``: per task a dict hm / hm_target / ind / cat, mask and anno_box (lists over the
    task's terms; a standard head's mask list has every step's mask) and maps (name -> tensor).  Returns (array, largest C, keep-alive)."""
    S = 1 if cfg.dense else cfg.T
    arr = (_lib.LossTask * len(tasks))()
    keep, cmax = [], 0
    for k, t in enumerate(tasks):
        hm = _dev(t["hm"], "hm", torch.float32)
        B, C, H, W = hm.shape
        if (B, H, W) != (cfg.B, cfg.H, cfg.W):
            raise FutureDetHipError("CenterHead loss: heat map %s of task %d does not match B, H, W = %d, %d, %d" % (tuple(hm.shape), k, cfg.B, cfg.H, cfg.W))
        cmax = max(cmax, C)
        d = arr[k]
        d.C = C
        d.hm = hm.data_ptr()
        tg = _dev(t["hm_target"], "hm_target", torch.float32)
        assert tuple(tg.shape) == tuple(hm.shape), (tuple(tg.shape), tuple(hm.shape))
        d.hm_target = tg.data_ptr()
        ind, cat = _dev(t["ind"], "ind", torch.int64), _dev(t["cat"], "cat", torch.int64)
        assert tuple(ind.shape) == tuple(cat.shape) == (cfg.B, cfg.M), (tuple(ind.shape), tuple(cat.shape))
        d.ind, d.cat = ind.data_ptr(), cat.data_ptr()
        assert len(t["mask"]) >= S and len(t["anno_box"]) >= S, "a mask and an anno_box per regression term"
        for i in range(S):
            mk = t["mask"][i]
            if mk.dtype == torch.bool:
                mk = mk.view(torch.uint8)
            elif mk.dtype != torch.uint8:
                mk = mk.ne(0).to(torch.uint8)
            mk, an = _dev(mk, "mask", torch.uint8), _dev(t["anno_box"][i], "anno_box", torch.float32)
            assert tuple(mk.shape) == (cfg.B, cfg.M) and tuple(an.shape) == (cfg.B, cfg.M, cfg.row_stride), (tuple(mk.shape), tuple(an.shape))
            d.mask[i], d.anno_box[i] = mk.data_ptr(), an.data_ptr()
            keep += [mk, an]
        for i, name in enumerate(LOSS_MAPS):
            m = t["maps"].get(name)
            if m is None:
                continue
            m = _dev(m, name, torch.float32)
            assert m.dim() == 4 and (m.shape[0], m.shape[2], m.shape[3]) == (B, H, W), (name, tuple(m.shape))
            want = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "rrot": 2}.get(name, 2 if cfg.dense else 2 * cfg.T)
            if m.shape[1] != want:
                raise FutureDetHipError("CenterHead loss: map %s of task %d has %d channels, the head mode needs %d" % (name, k, m.shape[1], want))
            d.maps[i] = m.data_ptr()
            if grads is not None and grads[k].get(name) is not None:
                d.d_maps[i] = grads[k][name].data_ptr()
        if sigs is not None:
            d.sig = sigs[k].data_ptr()
        if grads is not None and grads[k].get("hm") is not None:
            d.d_hm = grads[k]["hm"].data_ptr()
        keep += [hm, tg, ind, cat]
    return arr, cmax, keep


def centerhead_loss_forward(cfg, tasks):
    """fd_centerhead_loss_forward: -> (terms vector fp32 on the device, layout of loss_terms_layout; the clamped sigmoid of every task's
    heat map).  Two launches (three for more than 8 tasks), nothing is synchronised."""
    L = _lib.load()
    sigs = [torch.empty_like(_dev(t["hm"], "hm", torch.float32)) for t in tasks]
    arr, cmax, keep = _loss_tasks(cfg, tasks, sigs=sigs)
    dev = sigs[0].device
    n_terms = L.fd_centerhead_loss_terms(ctypes.byref(cfg))
    terms = torch.empty((max(int(n_terms), 1),), dtype=torch.float32, device=dev)
    ws = workspace.get("loss", L.fd_centerhead_loss_workspace_bytes(ctypes.byref(cfg), cmax), dev)
    check(L.fd_centerhead_loss_forward(ctypes.byref(cfg), arr, _p(terms), _p(ws), ws.numel(), _stream()), "fd_centerhead_loss_forward")
    return terms, sigs


def centerhead_loss_backward(cfg, tasks, terms, go, need=None):
    """fd_centerhead_loss_backward: the gradient of sum_k go[k] * loss[k] w.r.t. every map -> per task a dict hm / reg / ... of new
    tensors, every element written by the call.  ``go``: fp32 [n_tasks] on the device.  ``need``: per task a set of map names to
    compute (default: all the task has)."""
    L = _lib.load()
    grads = []
    for k, t in enumerate(tasks):
        names = ["hm"] + [n for n in LOSS_MAPS if t["maps"].get(n) is not None]
        grads.append({n: torch.empty_like(t["hm"] if n == "hm" else t["maps"][n]) for n in names if need is None or n in need[k]})
    arr, cmax, keep = _loss_tasks(cfg, tasks, grads=grads)
    dev = terms.device
    go = _dev(go, "go", torch.float32)
    assert go.numel() == len(tasks), (go.shape, len(tasks))
    ws = workspace.get("loss", L.fd_centerhead_loss_workspace_bytes(ctypes.byref(cfg), cmax), dev)
    check(L.fd_centerhead_loss_backward(ctypes.byref(cfg), arr, _p(_dev(terms, "terms", torch.float32)), _p(go), _p(ws), ws.numel(), _stream()),
          "fd_centerhead_loss_backward")
    return grads


def loss_status(terms):
    """The status word of a terms vector: the number of masked entries whose ind / cat were out of range (reads it back: a
    synchronisation).  torch's gather would have device-asserted on them."""
    return int(terms[-1].item())


# ------------------------------------------------------------------------------------------------ sparse BatchNorm (training)
def sparse_bn_chunk():
    """Rows per chunk of the sparse BatchNorm's sums (FD_SPARSE_BN_CHUNK): part of the summation order."""
    return int(_lib.load().fd_sparse_bn_chunk())


def sparse_bn_channels_ok(c):
    return c % 16 == 0 and 16 <= c <= 128


def _sparse_bn_ws(L, n, c, device):
    return workspace.get("sparse_bn", L.fd_sparse_bn_workspace_bytes(int(n), int(c)), device)


def _sparse_bn_rows(x, name):
    """the row tensor that sets a call's row type: fp32 or bf16 -> (tensor, entry-point suffix)"""
    x = _dev(x, name)
    if x.dtype == torch.float32:
        return x, ""
    if x.dtype == torch.bfloat16:
        return x, "_bf16"
    raise FutureDetHipError("%s must be torch.float32 or torch.bfloat16, got %s" % (name, x.dtype))


def sparse_bn_train_forward(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, residual=None, relu=True,
                            n_dev=None):
    """fd_sparse_bn_train_forward[_bf16]: y = act(gamma (x - mean) invstd + beta [+ residual]) on batch statistics over the rows of
    x [n, C], fp32 or bf16 (``residual`` and the returned y have x's dtype; parameters, statistics and ``saved`` are always fp32); updates
    running_mean / running_var / num_batches_tracked in place on the device (their ``_version`` is NOT bumped: the caller does that).
    ``n_dev``: int32 [1] on the device, the valid row count (n = x.shape[0] is then the capacity).
    Returns (y, saved [2, C] = mean, invstd).  Two launches, nothing is synchronised."""
    L = _lib.load()
    x, sfx = _sparse_bn_rows(x, "x")
    n, c = x.shape
    for t, name in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if _dev(t, name, torch.float32).numel() != c:
            raise FutureDetHipError("%s must hold %d channels, got %d" % (name, c, t.numel()))
    _dev(num_batches_tracked, "num_batches_tracked", torch.int64)
    if residual is not None and _dev(residual, "residual", x.dtype).shape != x.shape:
        raise FutureDetHipError("residual must be %s, got %s" % (tuple(x.shape), tuple(residual.shape)))
    out = torch.empty_like(x)
    saved = torch.empty((2, c), dtype=torch.float32, device=x.device)
    ws = _sparse_bn_ws(L, n, c, x.device)
    fn = "fd_sparse_bn_train_forward" + sfx
    check(getattr(L, fn)(_p(x), _p(residual), _p(gamma), _p(beta), n, _p(n_dev), c, int(bool(relu)), float(eps), float(momentum), _p(out),
                         _p(saved), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(ws), ws.numel(), _stream()), fn)
    return out, saved


def sparse_bn_train_backward(dy, x, y, gamma, saved, relu=True, want_residual=False, n_dev=None):
    """fd_sparse_bn_train_backward[_bf16]: -> (dx, d_residual or None, dgamma, dbeta).  ``y`` is the forward's output (the ReLU mask; may
    be None with relu=False), ``saved`` what the forward returned.  ``dy`` and ``y`` have x's dtype (fp32 or bf16), and so have dx and
    d_residual; dgamma and dbeta are fp32."""
    L = _lib.load()
    x, sfx = _sparse_bn_rows(x, "x")
    dy = _dev(dy, "dy", x.dtype)
    n, c = x.shape
    if dy.shape != x.shape or (y is not None and _dev(y, "y", x.dtype).shape != x.shape):
        raise FutureDetHipError("dy and y must be %s" % (tuple(x.shape),))
    if _dev(saved, "saved", torch.float32).numel() != 2 * c or _dev(gamma, "gamma", torch.float32).numel() != c:
        raise FutureDetHipError("gamma / saved do not hold %d channels" % c)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual else None
    dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
    ws = _sparse_bn_ws(L, n, c, x.device)
    fn = "fd_sparse_bn_train_backward" + sfx
    check(getattr(L, fn)(_p(dy), _p(x), _p(y), _p(gamma), _p(saved), n, _p(n_dev), c, int(bool(relu)), _p(dx), _p(dres), _p(dgb[0]), _p(dgb[1]),
                         _p(ws), ws.numel(), _stream()), fn)
    return dx, dres, dgb[0], dgb[1]


# ------------------------------------------------------------------------------------------------ dense BatchNorm (training)
def dense_bn_chunk():
    """Elements per chunk of the dense BatchNorm's sums (FD_DENSE_BN_CHUNK): part of the summation order."""
    return int(_lib.load().fd_dense_bn_chunk())


def _dense_bn_map(x, name):
    """an fp32 NCHW-contiguous map on the device -> (tensor, B, C, P)"""
    x = _dev(x, name, torch.float32)
    if x.dim() != 4:
        raise FutureDetHipError("%s must be [B, C, H, W], got %s" % (name, tuple(x.shape)))
    return x, x.shape[0], x.shape[1], x.shape[2] * x.shape[3]


def _dense_bn_ws(L, b, c, p, device):
    return workspace.get("dense_bn", L.fd_dense_bn_workspace_bytes(int(b), int(c), int(p)), device)


def dense_bn_train_forward(x, gamma, beta, running_mean, running_var, num_batches_tracked, eps, momentum, relu=True):
    """fd_dense_bn_train_forward: y = act(gamma (x - mean) invstd + beta) on batch statistics over x [B, C, H, W], fp32 NCHW contiguous;
    updates running_mean / running_var / num_batches_tracked in place on the device (their ``_version`` is NOT bumped: the caller
    does that).  Returns (y, saved [2, C] = mean, invstd).  Two launches, nothing is synchronised."""
    L = _lib.load()
    x, b, c, p = _dense_bn_map(x, "x")
    for t, name in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        if _dev(t, name, torch.float32).numel() != c:
            raise FutureDetHipError("%s must hold %d channels, got %d" % (name, c, t.numel()))
    _dev(num_batches_tracked, "num_batches_tracked", torch.int64)
    out = torch.empty_like(x)
    saved = torch.empty((2, c), dtype=torch.float32, device=x.device)
    ws = _dense_bn_ws(L, b, c, p, x.device)
    check(L.fd_dense_bn_train_forward(_p(x), _p(gamma), _p(beta), b, c, p, int(bool(relu)), float(eps), float(momentum), _p(out), _p(saved),
                                      _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(ws), ws.numel(), _stream()),
          "fd_dense_bn_train_forward")
    return out, saved


def dense_bn_train_backward(dy, x, y, gamma, saved, relu=True):
    """fd_dense_bn_train_backward: -> (dx, dgamma, dbeta).  ``y`` is the forward's output (the ReLU mask; may be None with relu=False),
    ``saved`` what the forward returned."""
    L = _lib.load()
    x, b, c, p = _dense_bn_map(x, "x")
    dy = _dev(dy, "dy", torch.float32)
    if dy.shape != x.shape or (y is not None and _dev(y, "y", torch.float32).shape != x.shape):
        raise FutureDetHipError("dy and y must be %s" % (tuple(x.shape),))
    if _dev(saved, "saved", torch.float32).numel() != 2 * c or _dev(gamma, "gamma", torch.float32).numel() != c:
        raise FutureDetHipError("gamma / saved do not hold %d channels" % c)
    dx = torch.empty_like(x)
    # two tensors, not two rows of one: autograd keeps a gradient that owns its storage and would copy a view
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    ws = _dense_bn_ws(L, b, c, p, x.device)
    check(L.fd_dense_bn_train_backward(_p(dy), _p(x), _p(y), _p(gamma), _p(saved), b, c, p, int(bool(relu)), _p(dx), _p(dgamma), _p(dbeta),
                                       _p(ws), ws.numel(), _stream()), "fd_dense_bn_train_backward")
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ dense BatchNorm on bf16 NHWC maps (training)
def dense_bn_nhwc_chunk():
    """Rows per chunk of the bf16 channels-last BatchNorm's sums (FD_DENSE_BN_NHWC_CHUNK): part of the summation order."""
    return int(_lib.load().fd_dense_bn_nhwc_chunk())


def dense_bn_nhwc_max_groups():
    """BatchNorm2d modules one call of the bf16 channels-last BatchNorm takes (FD_DENSE_BN_NHWC_MAX_GROUPS)."""
    return 8


def dense_bn_nhwc_channels_ok(c):
    return c % 32 == 0 and 32 <= c <= 512


def _dense_bn_nhwc_rows(x, name):
    """a contiguous bf16 [B, H, W, C] (or [n, C]) device tensor -> (tensor, n, C)"""
    x = _dev(x, name, torch.bfloat16)
    if x.dim() not in (2, 4):
        raise FutureDetHipError("%s must be [B, H, W, C] or [n, C], got %s" % (name, tuple(x.shape)))
    return x, x.numel() // x.shape[-1], x.shape[-1]


def _dense_bn_nhwc_groups(bns, c, forward):
    """the fd_dense_bn_nhwc_group array of the modules ``bns`` (their num_features partition the c channels)"""
    bns = [bns] if isinstance(bns, torch.nn.Module) else list(bns)
    if not 1 <= len(bns) <= dense_bn_nhwc_max_groups() or sum(int(bn.num_features) for bn in bns) != c:
        raise FutureDetHipError("dense_bn_nhwc: needs 1 to %d BatchNorm2d modules whose num_features sum to the %d channels (got %s)"
                                % (dense_bn_nhwc_max_groups(), c, [int(bn.num_features) for bn in bns]))
    recs = []
    for bn in bns:
        gamma = _dev(bn.weight, "BatchNorm2d weight", torch.float32)
        if forward:
            for t, name in ((bn.bias, "bias"), (bn.running_mean, "running_mean"), (bn.running_var, "running_var")):
                _dev(t, "BatchNorm2d " + name, torch.float32)
            _dev(bn.num_batches_tracked, "BatchNorm2d num_batches_tracked", torch.int64)
            if bn.momentum is None:
                raise FutureDetHipError("dense_bn_nhwc: needs a fixed momentum (momentum=None is the cumulative average)")
            recs.append(_lib.DenseBnNhwcGroup(gamma.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                              bn.num_batches_tracked.data_ptr(), int(bn.num_features), float(bn.eps), float(bn.momentum)))
        else:
            recs.append(_lib.DenseBnNhwcGroup(gamma.data_ptr(), None, None, None, None, int(bn.num_features), float(bn.eps), 0.0))
    return (_lib.DenseBnNhwcGroup * len(recs))(*recs), len(recs)


def _dense_bn_nhwc_ws(L, n, c, device):
    nbytes = L.fd_dense_bn_nhwc_workspace_bytes(int(n), int(c))
    if nbytes == 0:
        raise FutureDetHipError("dense_bn_nhwc: unsupported size: %d rows of %d channels (C a multiple of 32 in [32, 512], 2 <= n <= 2^30)" % (n, c))
    return workspace.get("dense_bn_nhwc", nbytes, device)


def dense_bn_nhwc_train_forward(x_nhwc, bns, relu=True):
    """fd_dense_bn_nhwc_train_forward_bf16: y = act(gamma (x - mean) invstd + beta) on batch statistics over the rows of the contiguous
    bf16 [B, H, W, C] tensor ``x_nhwc``.  ``bns``: one nn.BatchNorm2d or a list of at most 8 whose num_features partition the channels
    (each a multiple of 32): each module's parameters, eps and momentum apply to its channels and its running_mean / running_var /
    num_batches_tracked are updated in place on the device (their ``_version`` is NOT bumped: the caller does that).
    Returns (y bf16 like x, saved fp32 [2, C] = mean, invstd).  Two launches, nothing is synchronised."""
    L = _lib.load()
    x, n, c = _dense_bn_nhwc_rows(x_nhwc, "x")
    groups, ng = _dense_bn_nhwc_groups(bns, c, True)
    ws = _dense_bn_nhwc_ws(L, n, c, x.device)
    y = torch.empty_like(x)
    saved = torch.empty((2, c), dtype=torch.float32, device=x.device)
    check(L.fd_dense_bn_nhwc_train_forward_bf16(_p(x), groups, ng, n, c, int(bool(relu)), _p(y), _p(saved), _p(ws), ws.numel(), _stream()),
          "fd_dense_bn_nhwc_train_forward_bf16")
    return y, saved


def dense_bn_nhwc_train_backward(dy, x, y, saved, bns, relu=True):
    """fd_dense_bn_nhwc_train_backward_bf16: -> (dx bf16 like x, dgamma fp32 [C], dbeta fp32 [C]; flat over the modules' channels).
    ``y`` is the forward's output (the ReLU mask; may be None with relu=False), ``saved`` what the forward returned."""
    L = _lib.load()
    x, n, c = _dense_bn_nhwc_rows(x, "x")
    dy = _dev(dy, "dy", torch.bfloat16)
    if dy.shape != x.shape or (y is not None and _dev(y, "y", torch.bfloat16).shape != x.shape):
        raise FutureDetHipError("dy and y must be %s" % (tuple(x.shape),))
    if _dev(saved, "saved", torch.float32).numel() != 2 * c:
        raise FutureDetHipError("saved does not hold %d channels" % c)
    groups, ng = _dense_bn_nhwc_groups(bns, c, False)
    ws = _dense_bn_nhwc_ws(L, n, c, x.device)
    dx = torch.empty_like(x)
    dgamma = torch.empty((c,), dtype=torch.float32, device=x.device)
    dbeta = torch.empty((c,), dtype=torch.float32, device=x.device)
    check(L.fd_dense_bn_nhwc_train_backward_bf16(_p(dy), _p(x), _p(y), _p(saved), groups, ng, n, c, int(bool(relu)), _p(dx), _p(dgamma),
                                                 _p(dbeta), _p(ws), ws.numel(), _stream()), "fd_dense_bn_nhwc_train_backward_bf16")
    return dx, dgamma, dbeta
