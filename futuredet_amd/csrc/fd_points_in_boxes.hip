// Which points of a cloud lie inside which rotated 3-D boxes (include/futuredet_hip.h has the contract, the arithmetic and the reference
// lines).  Built with -ffp-contract=off: every product and every sum below is one IEEE operation rounded on its own, so every decision is
// bit-defined and the two kernels that take it (count and extract) take it alike.
//
//   pib_count    one workgroup per 256 points, a point per lane.  The boxes go through LDS a tile of kTile at a time: lane b of the
//                first wave builds the six face planes (and keeps the centre) of box b of the tile, a barrier, then every lane tests its
//                point against the tile's planes -- LDS reads at a wave-uniform address, so broadcasts -- and each wave's ballot +
//                popcount per box lands in LDS; after a second barrier the four waves' numbers are summed into the workspace row of the
//                workgroup.  Boxes at or past the device count are never read: their partial counts are written as zeros.
//   pib_scan     one wave per box: the partial counts of the box over the workgroups, 64 at a time, become their exclusive scan in
//                place (shuffles), the total goes to counts[] and to the head of the workspace.
//   pib_extract  the same decisions again; the destination row of a point is offsets[box] (a running sum over the totals, a tile at a
//                time) + the scan entry of (workgroup, box) + the earlier waves' numbers + the rank in the wave's ballot.  No atomics:
//                two runs write the same rows.  A destination that does not lie in [0, cap_rows) is not written, whatever the workspace
//                holds.
#include <math.h>

#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = FD_POINTS_IN_BOXES_TILE;  // boxes per LDS tile: one bit per box in a lane's 64-bit membership word
static_assert(kTile == 64, "a tile is one 64-bit membership word");

struct Vec3 {
    float x, y, z;
};

// the six face planes of one box row (n.x, n.y, n.z, d) and its centre, into out[0..6]
__device__ __forceinline__ void box_planes(const float *row, int box_cols, float4 *out) {
    const float cx = row[0], cy = row[1], cz = row[2], w = row[3], l = row[4], h = row[5], a = row[box_cols - 1];
    const float s = (float)sin((double)a), c = (float)cos((double)a);
    Vec3 P[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float bx = (k & 4) ? 1.f : 0.f, by = (k & 2) ? 1.f : 0.f, bz = ((k & 3) == 1 || (k & 3) == 2) ? 1.f : 0.f;
        const float ox = w * (bx - 0.5f), oy = l * (by - 0.5f), oz = h * (bz - 0.5f);
        const float xc = ox * c, ys = oy * s, xs = ox * s, yc = oy * c;
        P[k].x = (xc + ys) + cx;
        P[k].y = (-xs + yc) + cy;
        P[k].z = oz + cz;
    }
    constexpr int F[6][3] = {{0, 1, 2}, {7, 6, 5}, {0, 3, 7}, {1, 5, 6}, {0, 4, 5}, {3, 2, 6}};
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const Vec3 p0 = P[F[f][0]], p1 = P[F[f][1]], p2 = P[F[f][2]];
        const float ux = p0.x - p1.x, uy = p0.y - p1.y, uz = p0.z - p1.z;
        const float vx = p1.x - p2.x, vy = p1.y - p2.y, vz = p1.z - p2.z;
        const float a0 = uy * vz, a1 = uz * vy, b0 = uz * vx, b1 = ux * vz, c0 = ux * vy, c1 = uy * vx;
        const float nx = a0 - a1, ny = b0 - b1, nz = c0 - c1;
        const float dx = p0.x * nx, dy = p0.y * ny, dz = p0.z * nz;
        const float d = ((-dx) - dy) - dz;
        out[f] = make_float4(nx, ny, nz, d);
    }
    out[6] = make_float4(cx, cy, cz, 0.f);
}

// a point against the six planes of a box in LDS: outside as soon as one signed distance is >= 0 (a NaN never is)
__device__ __forceinline__ bool inside(float px, float py, float pz, const float4 *pl) {
    bool in = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const float4 q = pl[f];
        const float tx = px * q.x, ty = py * q.y, tz = pz * q.z;
        const float v = ((tx + ty) + tz) + q.w;
        in = in && !(v >= 0.f);
    }
    return in;
}

// fills the tile's planes (boxes tile0 .. tile0 + valid) and, per lane, the 64-bit word of the boxes of the tile that hold its point;
// s_cnt[wave][b] = the wave's number of points in box b.  Ends behind a barrier.
__device__ __forceinline__ unsigned long long tile_membership(const float *boxes, int box_cols, int tile0, int valid, bool has_point, float px,
                                                              float py, float pz, float4 (*s_planes)[7], int (*s_cnt)[kTile]) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < valid) box_planes(boxes + (int64_t)(tile0 + tid) * box_cols, box_cols, s_planes[tid]);
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int b = 0; b < valid; ++b) {
        const bool in = has_point && inside(px, py, pz, s_planes[b]);
        const unsigned long long votes = __ballot(in);
        if (in) mine |= 1ull << b;
        if (lane == 0) s_cnt[wave][b] = __popcll(votes);
    }
    if (lane == 0)
        for (int b = valid; b < kTile; ++b) s_cnt[wave][b] = 0;
    __syncthreads();
    return mine;
}

__global__ void __launch_bounds__(kThreads) pib_count(const float *__restrict__ points, int64_t n, int ndim, const float *__restrict__ boxes,
                                                      int box_cols, int n_boxes_max, const int *__restrict__ n_boxes_dev,
                                                      int *__restrict__ partial /* [gridDim.x, n_boxes_max] */) {
    __shared__ float4 s_planes[kTile][7];
    __shared__ int s_cnt[kWaves][kTile];
    const int tid = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    const int nb = fd::device_count(n_boxes_max, n_boxes_dev);
    const bool has_point = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (has_point) {
        const float *p = points + i * ndim;
        px = p[0], py = p[1], pz = p[2];
    }
    int *mine_row = partial + (int64_t)blockIdx.x * n_boxes_max;
    for (int tile0 = 0; tile0 < n_boxes_max; tile0 += kTile) {
        const int left = nb - tile0, valid = left < 0 ? 0 : (left > kTile ? kTile : left);
        if (valid > 0) {
            tile_membership(boxes, box_cols, tile0, valid, has_point, px, py, pz, s_planes, s_cnt);
            if (tid < kTile && tile0 + tid < n_boxes_max) {
                int sum = 0;
#pragma unroll
                for (int v = 0; v < kWaves; ++v) sum += s_cnt[v][tid];
                mine_row[tile0 + tid] = sum;
            }
            __syncthreads();  // s_cnt and s_planes are free again
        } else if (tid < kTile && tile0 + tid < n_boxes_max) {
            mine_row[tile0 + tid] = 0;
        }
    }
}

// one wave per box; partial [n_wg, n_boxes_max] -> its exclusive scan over the workgroups, totals[box] = counts[box] = the sum
__global__ void __launch_bounds__(kThreads) pib_scan(int *__restrict__ partial, int n_wg, int n_boxes_max, int *__restrict__ totals,
                                                     int *__restrict__ counts) {
    const int lane = (int)threadIdx.x & 63, box = (int)blockIdx.x * kWaves + ((int)threadIdx.x >> 6);
    if (box >= n_boxes_max) return;  // (whole waves leave: no barrier below)
    int running = 0;
    for (int base = 0; base < n_wg; base += 64) {
        const int g = base + lane;
        const int v = g < n_wg ? partial[(int64_t)g * n_boxes_max + box] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (g < n_wg) partial[(int64_t)g * n_boxes_max + box] = running + (incl - v);
        running += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        totals[box] = running;
        counts[box] = running;
    }
}

__global__ void __launch_bounds__(kThreads) pib_extract(const float *__restrict__ points, int64_t n, int ndim, const float *__restrict__ boxes,
                                                        int box_cols, int n_boxes_max, const int *__restrict__ n_boxes_dev,
                                                        const int *__restrict__ totals, const int *__restrict__ scan, int n_wg,
                                                        float *__restrict__ rows, int64_t cap_rows, int ncols_out,
                                                        int64_t *__restrict__ offsets, int *__restrict__ status) {
    __shared__ float4 s_planes[kTile][7];
    __shared__ int s_cnt[kWaves][kTile];
    __shared__ int64_t s_off[kTile];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
    const int nb = fd::device_count(n_boxes_max, n_boxes_dev);
    const bool has_point = i < n;
    const bool has_scan = (int)blockIdx.x < n_wg;  // (n = 0: one workgroup is launched for the offsets alone)
    const float *p = points + i * ndim;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (has_point) px = p[0], py = p[1], pz = p[2];
    const int *scan_row = scan + (int64_t)blockIdx.x * n_boxes_max;
    int64_t running = 0;  // (the first wave's: the totals of the boxes before the tile)
    for (int tile0 = 0; tile0 < n_boxes_max; tile0 += kTile) {
        // offsets of the tile: the running sum + the exclusive scan of the tile's totals (the first wave, shuffles)
        if (wave == 0) {
            const int box = tile0 + lane;
            const int t = box < n_boxes_max ? totals[box] : 0;
            const int64_t v = t < 0 ? 0 : t;
            int64_t incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const int64_t off = running + (incl - v);
            s_off[lane] = off;
            if (blockIdx.x == 0 && box < n_boxes_max) offsets[box] = off;
            running += __shfl(incl, 63, 64);
        }
        const int left = nb - tile0, valid = left < 0 ? 0 : (left > kTile ? kTile : left);
        if (valid == 0) continue;  // (so is every later tile: s_off is not read again)
        const unsigned long long mine = tile_membership(boxes, box_cols, tile0, valid, has_point, px, py, pz, s_planes, s_cnt);
        for (int b = 0; b < valid; ++b) {
            const bool in = (mine >> b) & 1ull;
            const unsigned long long votes = __ballot(in);
            if (!in || !has_scan) continue;
            int before = __popcll(votes & ((1ull << lane) - 1ull));
#pragma unroll
            for (int v = 0; v < kWaves; ++v)
                if (v < wave) before += s_cnt[v][b];
            const int64_t to = s_off[b] + (int64_t)scan_row[tile0 + b] + before;
            if ((uint64_t)to >= (uint64_t)cap_rows) continue;
            const float4 ctr = s_planes[b][6];
            float *dst = rows + to * ncols_out;
            const uint32_t *raw = reinterpret_cast<const uint32_t *>(p);
            for (int col = 0; col < ncols_out; ++col) {
                if (col == 0) dst[0] = px - ctr.x;
                else if (col == 1) dst[1] = py - ctr.y;
                else if (col == 2) dst[2] = pz - ctr.z;
                else reinterpret_cast<uint32_t *>(dst)[col] = raw[col];
            }
        }
        __syncthreads();  // the tile's LDS is free again
    }
    if (blockIdx.x == 0 && tid == 0) {
        offsets[n_boxes_max] = running;
        status[0] = running > cap_rows ? FD_POINTS_IN_BOXES_NO_ROOM : 0;
    }
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool disjoint(const void *a, const void *b, size_t bytes_a, size_t bytes_b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return bytes_a == 0 || bytes_b == 0 || x + bytes_a <= y || y + bytes_b <= x;
}
inline int64_t workgroups(int64_t n) { return (n + kThreads - 1) / kThreads; }

// what count and extract check alike; 0 = fine
int check_inputs(const char *what, const float *points, int64_t n, int ndim, const float *boxes, int n_boxes_max, int box_cols,
                 const int32_t *n_boxes_dev, const void *ws, size_t ws_bytes) {
    FD_REQUIRE(ndim == 4 || ndim == 5, "%s: ndim (%d) must be 4 or 5", what, ndim);
    FD_REQUIRE(n >= 0 && n <= FD_AUGMENT_MAX_ROWS, "%s: n (%lld) must lie in [0, %d]", what, (long long)n, FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(n_boxes_max >= 0 && n_boxes_max <= FD_RANGE_FILTER_MAX_N, "%s: n_boxes_max (%d) must lie in [0, %d]", what, n_boxes_max,
               FD_RANGE_FILTER_MAX_N);
    FD_REQUIRE(box_cols >= 7 && box_cols <= FD_POINTS_IN_BOXES_MAX_COLS, "%s: box_cols (%d) must lie in [7, %d]", what, box_cols,
               FD_POINTS_IN_BOXES_MAX_COLS);
    FD_REQUIRE((points || n == 0) && aligned(points, 4), "%s: points must be non-null (n > 0) and 4-byte aligned", what);
    FD_REQUIRE((boxes || n_boxes_max == 0) && aligned(boxes, 4), "%s: boxes must be non-null (n_boxes_max > 0) and 4-byte aligned", what);
    FD_REQUIRE(aligned(n_boxes_dev, 4), "%s: the device box count must be 4-byte aligned", what);
    const size_t need = fd_points_in_boxes_workspace_bytes(n, n_boxes_max);
    FD_REQUIRE(ws_bytes >= need && (ws || need == 0) && aligned(ws, 4), "%s: the workspace holds %zu bytes, %zu are needed (non-null, 4-byte aligned)",
               what, ws_bytes, need);
    return FD_OK;
}

}  // namespace

extern "C" size_t fd_points_in_boxes_workspace_bytes(int64_t n_points, int n_boxes_max) {
    if (n_points < 0 || n_points > FD_AUGMENT_MAX_ROWS || n_boxes_max < 0 || n_boxes_max > FD_RANGE_FILTER_MAX_N) return 0;
    return (size_t)(workgroups(n_points) + 1) * (size_t)n_boxes_max * sizeof(int32_t);  // the totals, then a row per workgroup
}

extern "C" int fd_points_in_boxes_count(const float *points, int64_t n, int ndim, const float *boxes, int n_boxes_max, int box_cols,
                                        const int32_t *n_boxes_dev, int32_t *counts, void *workspace, size_t workspace_bytes,
                                        fd_stream_t stream_) {
    const int rc = check_inputs("fd_points_in_boxes_count", points, n, ndim, boxes, n_boxes_max, box_cols, n_boxes_dev, workspace, workspace_bytes);
    if (rc != FD_OK) return rc;
    FD_REQUIRE((counts || n_boxes_max == 0) && aligned(counts, 4), "fd_points_in_boxes_count: counts must be non-null (n_boxes_max > 0) and 4-byte aligned");
    const size_t need = fd_points_in_boxes_workspace_bytes(n, n_boxes_max);
    FD_REQUIRE(disjoint(counts, workspace, (size_t)n_boxes_max * 4, need) && disjoint(counts, boxes, (size_t)n_boxes_max * 4, (size_t)n_boxes_max * box_cols * 4) &&
                   disjoint(counts, points, (size_t)n_boxes_max * 4, (size_t)n * ndim * 4) &&
                   disjoint(workspace, boxes, need, (size_t)n_boxes_max * box_cols * 4) && disjoint(workspace, points, need, (size_t)n * ndim * 4),
               "fd_points_in_boxes_count: counts and the workspace must overlap neither each other nor the inputs");
    if (n_boxes_max == 0) return FD_OK;
    const int n_wg = (int)workgroups(n);
    int *totals = static_cast<int *>(workspace), *partial = totals + n_boxes_max;
    hipStream_t stream = fd::as_stream(stream_);
    if (n_wg > 0) {
        hipLaunchKernelGGL(pib_count, dim3((unsigned)n_wg), dim3(kThreads), 0, stream, points, n, ndim, boxes, box_cols, n_boxes_max, n_boxes_dev, partial);
        const int rc1 = fd::check_launch("fd_points_in_boxes_count");
        if (rc1 != FD_OK) return rc1;
    }
    hipLaunchKernelGGL(pib_scan, dim3((unsigned)((n_boxes_max + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, partial, n_wg, n_boxes_max, totals,
                       counts);
    return fd::check_launch("fd_points_in_boxes_count");
}

extern "C" int fd_points_in_boxes_extract(const float *points, int64_t n, int ndim, const float *boxes, int n_boxes_max, int box_cols,
                                          const int32_t *n_boxes_dev, const void *workspace, size_t workspace_bytes, float *rows,
                                          int64_t cap_rows, int ncols_out, int64_t *offsets, int32_t *status, fd_stream_t stream_) {
    const int rc = check_inputs("fd_points_in_boxes_extract", points, n, ndim, boxes, n_boxes_max, box_cols, n_boxes_dev, workspace, workspace_bytes);
    if (rc != FD_OK) return rc;
    FD_REQUIRE(ncols_out >= 1 && ncols_out <= ndim, "fd_points_in_boxes_extract: ncols_out (%d) must lie in [1, ndim = %d]", ncols_out, ndim);
    FD_REQUIRE(cap_rows >= 0 && cap_rows <= FD_AUGMENT_MAX_ROWS, "fd_points_in_boxes_extract: cap_rows (%lld) must lie in [0, %d]", (long long)cap_rows,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE((rows || cap_rows == 0) && aligned(rows, 4), "fd_points_in_boxes_extract: rows must be non-null (cap_rows > 0) and 4-byte aligned");
    FD_REQUIRE(offsets && aligned(offsets, 8) && status && aligned(status, 4),
               "fd_points_in_boxes_extract: offsets (8-byte aligned) and status (4-byte aligned) must be non-null");
    const size_t need = fd_points_in_boxes_workspace_bytes(n, n_boxes_max), rows_bytes = (size_t)cap_rows * ncols_out * 4;
    const size_t off_bytes = ((size_t)n_boxes_max + 1) * 8, pts_bytes = (size_t)n * ndim * 4, box_bytes = (size_t)n_boxes_max * box_cols * 4;
    FD_REQUIRE(disjoint(rows, points, rows_bytes, pts_bytes) && disjoint(rows, boxes, rows_bytes, box_bytes) && disjoint(rows, workspace, rows_bytes, need) &&
                   disjoint(rows, offsets, rows_bytes, off_bytes) && disjoint(rows, status, rows_bytes, 4) && disjoint(offsets, points, off_bytes, pts_bytes) &&
                   disjoint(offsets, boxes, off_bytes, box_bytes) && disjoint(offsets, workspace, off_bytes, need) && disjoint(offsets, status, off_bytes, 4) &&
                   disjoint(status, points, 4, pts_bytes) && disjoint(status, boxes, 4, box_bytes) && disjoint(status, workspace, 4, need),
               "fd_points_in_boxes_extract: rows, offsets and status must overlap neither one another nor the inputs and the workspace");
    const int n_wg = (int)workgroups(n);
    const int *totals = static_cast<const int *>(workspace), *scan = totals + n_boxes_max;
    hipLaunchKernelGGL(pib_extract, dim3((unsigned)(n_wg > 0 ? n_wg : 1)), dim3(kThreads), 0, fd::as_stream(stream_), points, n, ndim, boxes, box_cols,
                       n_boxes_max, n_boxes_dev, totals, scan, n_wg, rows, cap_rows, ncols_out, offsets, status);
    return fd::check_launch("fd_points_in_boxes_extract");
}
