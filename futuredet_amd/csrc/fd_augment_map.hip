// Between the augmentation and the target assignment: the ground-truth range filter and the warp of a bev_map head's mask
// (include/futuredet_hip.h has the contracts, the arithmetic and the reference lines).  Built with -ffp-contract=off: every product and
// every sum below is one IEEE operation rounded on its own, so every result is bit-defined.
//
//   gt_filter     the range filter and the point-count filter (fd_gt_min_points_filter): one compaction, two keep flags (KeepInRange: the
//                 corner test; KeepMinPoints: point_counts[b, i] >= min_points).
//                 One workgroup per sample.  Phase A: the keep flag of every object of timestep 0 and its exclusive prefix sum, in LDS
//                 (wave ballots, one running total).  Phase B, per timestep: 256 rows at a time, every lane reads its row (box, class,
//                 trajectory) into registers, a barrier, then the kept rows are written to their prefix position.  A kept row never moves
//                 backwards and a chunk only writes below its own end, so rows that are still to be read are never overwritten: that is
//                 what makes the in-place call safe.  The padding rows are zeroed last.
//   mask_planes   one workgroup per [H, W] plane.  Pass 1 warps the flipped source plane with m1 into LDS, a barrier, pass 2 warps the LDS
//                 plane with m2 into dst.  180 x 180 x 4 = 129 600 bytes of the compute unit's 160 KB.
#include <math.h>

#include "fd_common.h"

namespace {

constexpr int kFilterThreads = 256;
constexpr int kMaskThreads = 1024;

struct Rect {
    float px[4], py[4];  // P0..P3 of minmax_to_corner_2d: (x0, y0), (x0, y1), (x1, y1), (x1, y0)
};

// points_in_convex_polygon_jit for one point and the clockwise rectangle
__device__ __forceinline__ bool inside(float x, float y, const Rect &r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = (j + 3) & 3;
        const float vx = r.px[j] - r.px[p], vy = r.py[j] - r.py[p];
        const float a = vy * (r.px[j] - x), b = vx * (r.py[j] - y);
        const double cross = (double)a - (double)b;
        if (cross >= 0) return false;
    }
    return true;
}

// one box row: does any BEV corner lie inside?
__device__ __forceinline__ bool keep_row(const float *row, const Rect &r) {
    const float4 q0 = reinterpret_cast<const float4 *>(row)[0], q1 = reinterpret_cast<const float4 *>(row)[1];
    const float cx = q0.x, cy = q0.y, w = q0.w, l = q1.x, a = row[11];
    const float s = (float)sin((double)a), c = (float)cos((double)a);
    const float hx = w * 0.5f, hy = l * 0.5f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ox = (k < 2) ? -hx : hx, oy = (k == 1 || k == 2) ? hy : -hy;
        const float xc = ox * c, ys = oy * s, xs = ox * s, yc = oy * c;
        const float x = (xc + ys) + cx, y = (-xs + yc) + cy;
        any = any || inside(x, y, r);  // (the reference evaluates all four; the result is their OR)
    }
    return any;
}

__device__ __forceinline__ int clamp_count(int c, int n_max) { return c < 0 ? 0 : (c > n_max ? n_max : c); }

// the keep flag of object i of sample b (row = its timestep-0 box): the range filter's corner test, the point-count filter's threshold
struct KeepInRange {
    Rect rect;
    __device__ __forceinline__ bool operator()(const float *row, int64_t, int) const { return keep_row(row, rect); }
};
struct KeepMinPoints {
    const int *point_counts;  // [B, n_max]
    int min_points;
    __device__ __forceinline__ bool operator()(const float *, int64_t b_n_max, int i) const { return point_counts[b_n_max + i] >= min_points; }
};

template <typename Keep>
__global__ void __launch_bounds__(kFilterThreads) gt_filter(const float *boxes, const int *counts, const int *classes, const int *traj,
                                                            Keep keep_fn, float *boxes_out, int *counts_out, int *classes_out,
                                                            int *traj_out, int *status, int T, int n_max) {  // outputs may be the inputs
    __shared__ int s_pre[FD_RANGE_FILTER_MAX_N + 1];  // s_pre[i] = kept objects below i; object i is kept iff s_pre[i + 1] != s_pre[i]
    __shared__ int s_wave[kFilterThreads / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bt0 = (int64_t)b * T;
    const int c0_raw = counts[bt0], c0 = clamp_count(c0_raw, n_max);

    // phase A
    int running = 0;
    for (int base = 0; base < n_max; base += kFilterThreads) {
        const int i = base + tid;
        const bool keep = i < c0 && keep_fn(boxes + (bt0 * n_max + i) * 12, (int64_t)b * n_max, i);
        const unsigned long long votes = __ballot(keep);
        const int below = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(votes);
        __syncthreads();
        int before = running;
#pragma unroll
        for (int v = 0; v < kFilterThreads / 64; ++v) {
            const int n = s_wave[v];
            if (v < wave) before += n;
            running += n;
        }
        if (i < n_max) s_pre[i] = before + below;
        __syncthreads();
    }
    if (tid == 0) s_pre[n_max] = running;
    __syncthreads();

    // phase B
    int bad = 0;
    for (int t = 0; t < T; ++t) {
        const int64_t bt = bt0 + t;
        const int ct_raw = counts[bt];
        const int ct = clamp_count(ct_raw, n_max), m = ct < c0 ? ct : c0, kept = s_pre[m];
        bad += ct_raw != c0_raw;
        const float4 *src = reinterpret_cast<const float4 *>(boxes) + bt * n_max * 3;
        float4 *dst = reinterpret_cast<float4 *>(boxes_out) + bt * n_max * 3;
        for (int base = 0; base < n_max; base += kFilterThreads) {
            const int i = base + tid;
            int to = -1, cls = 0, tr = 0;
            float4 q0, q1, q2;
            if (i < m && s_pre[i + 1] != s_pre[i]) {
                to = s_pre[i];
                q0 = src[(int64_t)i * 3];
                q1 = src[(int64_t)i * 3 + 1];
                q2 = src[(int64_t)i * 3 + 2];
                cls = classes[bt * n_max + i];
                if (traj) tr = traj[bt * n_max + i];
            }
            __syncthreads();  // every row of this chunk (and of those before it) has been read
            if (to >= 0) {
                dst[(int64_t)to * 3] = q0;
                dst[(int64_t)to * 3 + 1] = q1;
                dst[(int64_t)to * 3 + 2] = q2;
                classes_out[bt * n_max + to] = cls;
                if (traj) traj_out[bt * n_max + to] = tr;
            }
        }
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = kept + tid; i < n_max; i += kFilterThreads) {  // the padding
            dst[(int64_t)i * 3] = zero;
            dst[(int64_t)i * 3 + 1] = zero;
            dst[(int64_t)i * 3 + 2] = zero;
            classes_out[bt * n_max + i] = 0;
            if (traj) traj_out[bt * n_max + i] = 0;
        }
        if (tid == 0) counts_out[bt] = kept;  // (every lane read counts[bt] before the barrier of the first chunk)
    }
    if (tid == 0) status[b] = bad;
}

// ---------------------------------------------------------------------------------------------------------------- the mask warp
typedef fd_augment_mask_record MaskRec;

__device__ __forceinline__ int fix(double v) {  // rint to int32; out-of-contract values are clamped (two of them still add up in int32)
    v = rint(v);
    v = !(v > -536870912.0) ? -536870912.0 : (v > 536870912.0 ? 536870912.0 : v);  // (a NaN takes the first branch)
    return (int)v;
}

template <typename Tap>
__device__ __forceinline__ float warp_pixel(const double *m, int x, int y, Tap tap) {
    const int X0 = fix((m[1] * (double)y + m[2]) * 1024.0) + 16, Y0 = fix((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const int X = (X0 + fix(m[0] * (double)x * 1024.0)) >> 5, Y = (Y0 + fix(m[3] * (double)x * 1024.0)) >> 5;
    const int sx = X >> 5, sy = Y >> 5;
    const float fx = (float)(X & 31) / 32.f, fy = (float)(Y & 31) / 32.f;
    const float one = 1.f;
    const float w00 = (one - fy) * (one - fx), w01 = (one - fy) * fx, w10 = fy * (one - fx), w11 = fy * fx;
    float out = tap(sy, sx) * w00;
    out = out + tap(sy, sx + 1) * w01;
    out = out + tap(sy + 1, sx) * w10;
    out = out + tap(sy + 1, sx + 1) * w11;
    return out;
}

__global__ void __launch_bounds__(kMaskThreads) mask_planes(const float *__restrict__ src, const MaskRec *__restrict__ recs,
                                                            float *__restrict__ dst, int C, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) float s_plane[];  // [H][W]: warp(flip(src), m1)
    const int plane = (int)blockIdx.x, n = H * W;
    const MaskRec r = recs[plane / C];
    const float *s = src + (int64_t)plane * n;
    float *d = dst + (int64_t)plane * n;
    const bool fa = r.flip_a != 0, fb = r.flip_b != 0;
    auto from_src = [&](int yy, int xx) -> float {
        if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return 0.f;
        return s[(fb ? H - 1 - yy : yy) * W + (fa ? W - 1 - xx : xx)];
    };
    auto from_lds = [&](int yy, int xx) -> float {
        if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) return 0.f;
        return s_plane[yy * W + xx];
    };
    for (int p = (int)threadIdx.x; p < n; p += kMaskThreads) s_plane[p] = warp_pixel(r.m1, p % W, p / W, from_src);
    __syncthreads();
    for (int p = (int)threadIdx.x; p < n; p += kMaskThreads) d[p] = warp_pixel(r.m2, p % W, p / W, from_lds);
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool disjoint(const void *a, const void *b, size_t bytes_a, size_t bytes_b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + bytes_a <= y || y + bytes_b <= x;
}
inline bool same_or_disjoint(const void *in, const void *out, size_t bytes) { return in == out || disjoint(in, out, bytes, bytes); }

}  // namespace

// what the two ground-truth filters check alike (``what`` names the entry point); 0 = fine
static int check_filter_args(const char *what, const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory,
                             float *boxes_out, int32_t *counts_out, int32_t *classes_out, int32_t *trajectory_out, int32_t *status, int B, int T,
                             int n_max) {
    FD_REQUIRE(B >= 1 && T >= 1, "%s: B (%d) and T (%d) must be >= 1", what, B, T);
    FD_REQUIRE(n_max >= 1 && n_max <= FD_RANGE_FILTER_MAX_N, "%s: n_max (%d) must lie in [1, %d]", what, n_max, FD_RANGE_FILTER_MAX_N);
    FD_REQUIRE((int64_t)B * T * n_max <= FD_AUGMENT_MAX_ROWS, "%s: B x T x n_max = %lld rows, at most %d", what, (long long)B * T * n_max,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(boxes && counts && classes && boxes_out && counts_out && classes_out && status,
               "%s: null boxes, counts, classes, one of their outputs or status", what);
    FD_REQUIRE(!trajectory || trajectory_out, "%s: a trajectory needs trajectory_out", what);
    FD_REQUIRE(aligned(boxes, 16) && aligned(boxes_out, 16), "%s: boxes and boxes_out must be 16-byte aligned", what);
    FD_REQUIRE(aligned(counts, 4) && aligned(classes, 4) && aligned(trajectory, 4) && aligned(counts_out, 4) && aligned(classes_out, 4) &&
                   aligned(trajectory_out, 4) && aligned(status, 4),
               "%s: the int32 arrays must be 4-byte aligned", what);
    const size_t sets = (size_t)B * T, rows = sets * n_max;
    FD_REQUIRE(same_or_disjoint(boxes, boxes_out, rows * 48) && same_or_disjoint(counts, counts_out, sets * 4) &&
                   same_or_disjoint(classes, classes_out, rows * 4) && (!trajectory || same_or_disjoint(trajectory, trajectory_out, rows * 4)),
               "%s: an output must be its input itself or not overlap it", what);
    return FD_OK;
}

extern "C" int fd_gt_range_filter(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory, float xmin,
                                  float ymin, float xmax, float ymax, float *boxes_out, int32_t *counts_out, int32_t *classes_out,
                                  int32_t *trajectory_out, int32_t *status, int B, int T, int n_max, fd_stream_t stream_) {
    const int rc = check_filter_args("fd_gt_range_filter", boxes, counts, classes, trajectory, boxes_out, counts_out, classes_out, trajectory_out,
                                     status, B, T, n_max);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(isfinite(xmin) && isfinite(ymin) && isfinite(xmax) && isfinite(ymax) && xmax > xmin && ymax > ymin,
               "fd_gt_range_filter: the range (%g, %g, %g, %g) must be finite with xmax > xmin and ymax > ymin", xmin, ymin, xmax, ymax);
    KeepInRange keep;
    Rect &r = keep.rect;
    const float x1 = xmin + (xmax - xmin), y1 = ymin + (ymax - ymin);  // minmax_to_corner_2d: centre + dims, in fp32
    r.px[0] = xmin; r.py[0] = ymin;
    r.px[1] = xmin; r.py[1] = y1;
    r.px[2] = x1;   r.py[2] = y1;
    r.px[3] = x1;   r.py[3] = ymin;
    hipLaunchKernelGGL(gt_filter<KeepInRange>, dim3((unsigned)B), dim3(kFilterThreads), 0, fd::as_stream(stream_), boxes, counts, classes, trajectory,
                       keep, boxes_out, counts_out, classes_out, trajectory ? trajectory_out : nullptr, status, T, n_max);
    return fd::check_launch("fd_gt_range_filter");
}

extern "C" int fd_gt_min_points_filter(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory,
                                       const int32_t *point_counts, int min_points, float *boxes_out, int32_t *counts_out, int32_t *classes_out,
                                       int32_t *trajectory_out, int32_t *status, int B, int T, int n_max, fd_stream_t stream_) {
    const int rc = check_filter_args("fd_gt_min_points_filter", boxes, counts, classes, trajectory, boxes_out, counts_out, classes_out,
                                     trajectory_out, status, B, T, n_max);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(point_counts && aligned(point_counts, 4), "fd_gt_min_points_filter: point_counts must be non-null and 4-byte aligned");
    const size_t sets = (size_t)B * T, rows = sets * n_max, pc = (size_t)B * n_max * 4;
    FD_REQUIRE(disjoint(point_counts, boxes_out, pc, rows * 48) && disjoint(point_counts, counts_out, pc, sets * 4) &&
                   disjoint(point_counts, classes_out, pc, rows * 4) && (!trajectory || disjoint(point_counts, trajectory_out, pc, rows * 4)) &&
                   disjoint(point_counts, status, pc, (size_t)B * 4),
               "fd_gt_min_points_filter: point_counts must not overlap an output");
    KeepMinPoints keep;
    keep.point_counts = point_counts;
    keep.min_points = min_points;
    hipLaunchKernelGGL(gt_filter<KeepMinPoints>, dim3((unsigned)B), dim3(kFilterThreads), 0, fd::as_stream(stream_), boxes, counts, classes,
                       trajectory, keep, boxes_out, counts_out, classes_out, trajectory ? trajectory_out : nullptr, status, T, n_max);
    return fd::check_launch("fd_gt_min_points_filter");
}

extern "C" int fd_augment_mask_check(const fd_augment_mask_record *recs_host, int B, int H, int W) {
    FD_REQUIRE(recs_host && B >= 1 && H >= 1 && W >= 1, "fd_augment_mask_check: null records, or B (%d), H (%d) or W (%d) < 1", B, H, W);
    for (int b = 0; b < B; ++b) {
        const double *ms[2] = {recs_host[b].m1, recs_host[b].m2};
        for (int k = 0; k < 2; ++k)
            for (int row = 0; row < 2; ++row) {
                const double *m = ms[k] + 3 * row;
                const double reach = fabs(m[0]) * (W - 1) + fabs(m[1]) * (H - 1) + fabs(m[2]);
                FD_REQUIRE(isfinite(reach) && reach < FD_AUGMENT_MASK_MAX_COORD,
                           "fd_augment_mask_check: record %d, matrix %d, row %d (%g, %g, %g) maps a pixel of a %d x %d plane beyond %g (or is not "
                           "finite): the fixed-point coordinates would leave their range",
                           b, k + 1, row, m[0], m[1], m[2], H, W, (double)FD_AUGMENT_MASK_MAX_COORD);
            }
    }
    return FD_OK;
}

extern "C" int fd_augment_mask(const float *src, const fd_augment_mask_record *recs, float *dst, int B, int C, int H, int W, fd_stream_t stream_) {
    FD_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "fd_augment_mask: B (%d), C (%d), H (%d) and W (%d) must be >= 1", B, C, H, W);
    FD_REQUIRE((int64_t)H * W <= FD_AUGMENT_MASK_MAX_PIXELS, "fd_augment_mask: a plane of %d x %d pixels does not fit LDS (at most %d pixels)", H, W,
               FD_AUGMENT_MASK_MAX_PIXELS);
    FD_REQUIRE((int64_t)B * C * H * W <= FD_AUGMENT_MAX_ROWS, "fd_augment_mask: B x C x H x W = %lld elements, at most %d", (long long)B * C * H * W,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(recs && aligned(recs, 8), "fd_augment_mask: the records must be non-null and 8-byte aligned");
    FD_REQUIRE(src && dst && aligned(src, 4) && aligned(dst, 4), "fd_augment_mask: src and dst must be non-null and 4-byte aligned");
    const size_t bytes = (size_t)B * C * H * W * sizeof(float);
    FD_REQUIRE(disjoint(src, dst, bytes, bytes), "fd_augment_mask: src and dst must be distinct buffers that do not overlap");
    const size_t lds = (size_t)H * W * sizeof(float);
    static std::atomic<uint64_t> lds_set{0};
    // (configured once per device, so for the largest plane the entry point takes)
    if (lds > 65536 && !fd::ensure_dynamic_lds(reinterpret_cast<const void *>(mask_planes), (size_t)FD_AUGMENT_MASK_MAX_PIXELS * sizeof(float), lds_set)) {
        fd::set_error("fd_augment_mask: the runtime refuses %zu bytes of dynamic LDS for a %d x %d plane", lds, H, W);
        return FD_ELAUNCH;
    }
    hipLaunchKernelGGL(mask_planes, dim3((unsigned)(B * C)), dim3(kMaskThreads), lds, fd::as_stream(stream_), src, recs, dst, C, H, W);
    return fd::check_launch("fd_augment_mask");
}
