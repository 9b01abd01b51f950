// Global training augmentation of one sample: flip, rotation, scaling and translation of a cloud and of its ground-truth box rows
// (include/futuredet_hip.h has the contracts and the reference lines).  Built with -ffp-contract=off: every product and every sum below
// is one IEEE operation rounded on its own, in the order NumPy 2 applies them in the reference, so every result is bit-defined.
//
//   points_rows<NDIM, VEC>  one row per lane: dst[i] = A(src[perm ? perm[i] : i]).  The gather form and the form for buffers that are
//                           not 16-byte aligned.  VEC (NDIM 4 only): the row is one 16-byte access on both sides.
//   points_quads5           no permutation, 5-float rows, 16-byte aligned buffers: a lane takes four consecutive rows = 80 bytes = five
//                           16-byte accesses on each side (a flat float4 sweep whose row phase repeats every four rows, so that x and y of
//                           a row always meet in one lane); the last n % 4 rows take one more lane each.
//   boxes_rows              one [12] box row per lane, three 16-byte accesses on each side; a lane reads its whole row before it writes
//                           it, which is what makes the in-place call safe.
// Elementwise and memory-bound: no LDS, no atomics, no workspace, one launch per entry point.
#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr float kPi = 3.14159274101257324f;     // fl32(pi)
constexpr float kTwoPi = 6.28318548202514648f;  // fl32(2 pi) = 2 fl32(pi)

typedef fd_augment_record Rec;

__device__ __forceinline__ void flip_xy(float &x, float &y, const Rec &r) {
    if (r.flip_a) y = -y;
    if (r.flip_b) x = -x;
}

// [x, y] @ [[c, -s], [s, c]]: products rounded, then the sum
__device__ __forceinline__ void rotate_xy(float &x, float &y, const Rec &r) {
    const float xc = x * r.c, ys = y * r.s, xs = x * r.s, yc = y * r.c;
    x = xc + ys;
    y = -xs + yc;
}

__device__ __forceinline__ float shift(float v, double t) { return (float)((double)v + t); }

__device__ __forceinline__ void point_xyz(float &x, float &y, float &z, const Rec &r) {
    flip_xy(x, y, r);
    rotate_xy(x, y, r);
    x *= r.scale;
    y *= r.scale;
    z *= r.scale;
    x = shift(x, r.tx);
    y = shift(y, r.ty);
    z = shift(z, r.tz);
}

__device__ __forceinline__ float flip_angle(float a, const Rec &r) {
    if (r.flip_a) a = -a + kPi;
    if (r.flip_b) a = -a + kTwoPi;
    return a + r.rot;
}

// b: one box row [x, y, z, w, l, h, vx, vy, rvx, rvy, rot, rrot]
__device__ __forceinline__ void box_row(float *b, const Rec &r) {
    b[10] = flip_angle(b[10], r);
    b[11] = flip_angle(b[11], r);
    flip_xy(b[0], b[1], r);
    flip_xy(b[6], b[7], r);
    flip_xy(b[8], b[9], r);
    rotate_xy(b[0], b[1], r);
    rotate_xy(b[6], b[7], r);
    rotate_xy(b[8], b[9], r);
#pragma unroll
    for (int k = 0; k < 10; ++k) b[k] *= r.scale;
    b[0] = shift(b[0], r.tx);
    b[1] = shift(b[1], r.ty);
    b[2] = shift(b[2], r.tz);
}

template <int NDIM, bool VEC>
__global__ void __launch_bounds__(kThreads) points_rows(const float *__restrict__ src, int n_rows, const int *__restrict__ perm,
                                                        const Rec *__restrict__ rec, float *__restrict__ dst) {
    const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (i >= n_rows) return;
    int j = i;
    if (perm) {
        j = perm[i];
        if ((unsigned)j >= (unsigned)n_rows) return;  // not a permutation of the rows: nothing is read out of bounds, the row stays
    }
    const Rec r = *rec;
    float v[NDIM];
    if (VEC) {
        const float4 q = reinterpret_cast<const float4 *>(src)[j];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < NDIM; ++k) v[k] = src[(int64_t)j * NDIM + k];
    }
    point_xyz(v[0], v[1], v[2], r);
    if (VEC) {
        reinterpret_cast<float4 *>(dst)[i] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < NDIM; ++k) dst[(int64_t)i * NDIM + k] = v[k];
    }
}

__global__ void __launch_bounds__(kThreads) points_quads5(const float *__restrict__ src, int n_rows, const Rec *__restrict__ rec,
                                                          float *__restrict__ dst) {
    const int q = (int)(blockIdx.x * kThreads + threadIdx.x), n_quads = n_rows >> 2;
    if (q >= n_quads + (n_rows & 3)) return;
    const Rec r = *rec;
    if (q >= n_quads) {  // one of the last n % 4 rows
        const int64_t at = ((int64_t)n_quads * 4 + (q - n_quads)) * 5;
        float x = src[at], y = src[at + 1], z = src[at + 2];
        const float a = src[at + 3], b = src[at + 4];
        point_xyz(x, y, z, r);
        dst[at] = x; dst[at + 1] = y; dst[at + 2] = z; dst[at + 3] = a; dst[at + 4] = b;
        return;
    }
    const float4 *s = reinterpret_cast<const float4 *>(src) + (int64_t)q * 5;
    float v[20];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float4 t = s[k];
        v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) point_xyz(v[5 * p], v[5 * p + 1], v[5 * p + 2], r);
    float4 *d = reinterpret_cast<float4 *>(dst) + (int64_t)q * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

__global__ void __launch_bounds__(kThreads) boxes_rows(const float *boxes, const int *__restrict__ counts, const Rec *__restrict__ recs,
                                                       float *out, int T, int n_max, int n_total) {  // out may be boxes: no __restrict__
    const int row = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (row >= n_total) return;
    const int i = row % n_max, bt = row / n_max;
    const bool live = i < counts[bt];
    if (!live && out == boxes) return;
    const float4 *s = reinterpret_cast<const float4 *>(boxes) + (int64_t)row * 3;
    float v[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 t = s[k];
        v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
    if (live) box_row(v, recs[bt / T]);
    float4 *d = reinterpret_cast<float4 *>(out) + (int64_t)row * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool disjoint(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + bytes <= y || y + bytes <= x;
}
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int fd_augment_points(const float *src, int64_t n_rows, int ndim, const int32_t *perm, const fd_augment_record *rec, float *dst,
                                 fd_stream_t stream_) {
    FD_REQUIRE(ndim == 4 || ndim == 5, "fd_augment_points: ndim must be 4 or 5 (got %d)", ndim);
    FD_REQUIRE(n_rows >= 0 && n_rows <= FD_AUGMENT_MAX_ROWS, "fd_augment_points: n_rows (%lld) must lie in [0, %d]", (long long)n_rows,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(rec && ((uintptr_t)rec & 7) == 0, "fd_augment_points: the record must be non-null and 8-byte aligned");
    if (n_rows == 0) return FD_OK;
    FD_REQUIRE(src && dst, "fd_augment_points: null src or dst");
    FD_REQUIRE(disjoint(src, dst, (size_t)n_rows * ndim * sizeof(float)), "fd_augment_points: src and dst must be distinct buffers that do not overlap");
    FD_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "fd_augment_points: src and dst must be 4-byte aligned");
    hipStream_t st = fd::as_stream(stream_);
    const int n = (int)n_rows;
    const bool vec = aligned16(src) && aligned16(dst);
    if (ndim == 4) {
        if (vec)
            hipLaunchKernelGGL((points_rows<4, true>), dim3(blocks_for(n)), dim3(kThreads), 0, st, src, n, perm, rec, dst);
        else
            hipLaunchKernelGGL((points_rows<4, false>), dim3(blocks_for(n)), dim3(kThreads), 0, st, src, n, perm, rec, dst);
    } else if (perm || !vec) {
        hipLaunchKernelGGL((points_rows<5, false>), dim3(blocks_for(n)), dim3(kThreads), 0, st, src, n, perm, rec, dst);
    } else {
        hipLaunchKernelGGL(points_quads5, dim3(blocks_for(n / 4 + n % 4)), dim3(kThreads), 0, st, src, n, rec, dst);
    }
    return fd::check_launch("fd_augment_points");
}

extern "C" int fd_augment_boxes(const float *boxes, const int32_t *counts, const fd_augment_record *recs, float *out, int B, int T, int n_max,
                                fd_stream_t stream_) {
    FD_REQUIRE(B >= 1 && T >= 1 && n_max >= 0, "fd_augment_boxes: B (%d) and T (%d) must be >= 1, n_max (%d) >= 0", B, T, n_max);
    FD_REQUIRE((int64_t)B * T * n_max <= FD_AUGMENT_MAX_ROWS, "fd_augment_boxes: B x T x n_max = %lld rows, at most %d", (long long)B * T * n_max,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(recs && ((uintptr_t)recs & 7) == 0, "fd_augment_boxes: the records must be non-null and 8-byte aligned");
    if (n_max == 0) return FD_OK;
    FD_REQUIRE(boxes && out && counts, "fd_augment_boxes: null boxes, out or counts");
    FD_REQUIRE(aligned16(boxes) && aligned16(out), "fd_augment_boxes: boxes and out must be 16-byte aligned");
    const int total = B * T * n_max;
    FD_REQUIRE(out == boxes || disjoint(boxes, out, (size_t)total * 12 * sizeof(float)), "fd_augment_boxes: out must be boxes itself or not overlap it");
    hipLaunchKernelGGL(boxes_rows, dim3(blocks_for(total)), dim3(kThreads), 0, fd::as_stream(stream_), boxes, counts, recs, out, T, n_max, total);
    return fd::check_launch("fd_augment_boxes");
}
