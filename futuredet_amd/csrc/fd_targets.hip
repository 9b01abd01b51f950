// Training targets of the CenterHead: AssignLabel's heat maps and box rows (det3d/datasets/pipelines/preprocess.py:336-910,
// NuScenesDataset branch; gaussian_radius / gaussian2D / draw_umich_gaussian of det3d/core/utils/center_utils.py:17-64) for a
// whole batch [B, T] and every target set (standard; trajectory and forecast for a non-standard sampler) in two launches.
//
// Object pass (targets_objects): workgroup (sample, timestep, set) regroups the set's objects by task and class -- class by class in
// the task's class order, original order within a class, with wave ballots and prefix counts -- and writes every row of the set's
// ind / mask / cat / anno_box and gt_boxes_and_cls (skipped and unused slots as zeros: no memset), one 16-byte draw record per drawn
// object into the caller's workspace and a status word.
// Heat-map pass (targets_heatmap): output-stationary.  The heat maps of a call are one flat array; workgroup i owns its elements
// [1024 i, 1024 i + 1024) -- a strip of one map (or the seam of two), whatever H, W and B -- stages the draw records whose window
// meets the strip in LDS (ballot-compacted) and writes each element once with 16-byte stores: the max over the covering records.
// No atomics: the result does not depend on object order or on the launch shape.
//
// Arithmetic follows numpy 2 (NEP 50: a python float or int meeting a float32 scalar is cast to float32), what the reference
// computes on float32 annotations (loading.py:185) and a float32 voxel_size (voxel_generator.py):
//   * limit_period (box_np_ops.py:360): v - floor(v / f32(2 pi) + 0.5) * f32(2 pi), float32;
//   * w / voxel_size / out_size_factor, gaussian_radius, the radius_mult factor and mult * radius: float32 (the python-float
//     constants of gaussian_radius are rounded to float32 once, on the host); np.linalg.norm of the float32 velocity pair is
//     sqrt(vx * vx + vy * vy) without contraction (the BLAS dot of two elements);
//   * the Gaussian: float64 exp(-(dx^2 + dy^2) / (2 sigma^2)), sigma = (2 r + 1) / 6, rounded once to float32 (np.maximum into the
//     float32 map; rounding is monotone, so the max of the roundings is the rounding of the max).  For r <= 256 every value lies at
//     least 124 float64 ulps from a float32 rounding midpoint, so any faithfully rounded exp gives the same float32.
//     gaussian2D's cut h < eps * h.max() never fires: h.max() = 1 and the smallest value, at a window corner, is
//     exp(-36 r^2 / (2 r + 1)^2) > e^-9, far above eps = 2.2e-16.
// The file is built with -ffp-contract=off: the float32 chains above must not be fused.
#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxU = FD_TARGETS_MAX_TASKS + 2;  // maps per timestep: the standard tasks, trajectory, forecast
constexpr int kMaxQ = 64;                        // classes of one set
constexpr int kTile = kThreads * 4;              // heat-map elements per workgroup
constexpr int kForecastClasses = 7;              // preprocess.py:373-375: car_1 .. car_7
constexpr int kTrajectoryClasses = 3;            // static, linear, nonlinear

struct Plan {
    int B, T, H, W, n_max, max_objs, n_sets, n_tasks, U, Csum, Qstd;
    int radius_mult, min_radius;
    int C[kMaxU], cbase[kMaxU];
    float osf, vsx, vsy, pcx, pcy;
    float k1m, k1p, kb3, kc3, k4a3, period;  // f32(1 - ov), f32(1 + ov), f32(-2 ov), f32(ov - 1), f32(4 (4 ov)), f32(2 pi)
    int64_t hw, total;
};

struct Rec {  // one drawn object: 16 bytes
    int x, y, c, r;
};

__device__ __forceinline__ float limit_period(float v, float period) { return v - floorf(v / period + 0.5f) * period; }

// center_utils.py:17-37 with height = l, width = w, in float32
__device__ float gaussian_radius_f32(float l, float w, const Plan &p) {
    const float b1 = l + w;
    const float c1 = w * l * p.k1m / p.k1p;
    const float r1 = (b1 + sqrtf(b1 * b1 - 4.0f * c1)) / 2.0f;
    const float b2 = 2.0f * (l + w);
    const float c2 = p.k1m * w * l;
    const float r2 = (b2 + sqrtf(b2 * b2 - 16.0f * c2)) / 2.0f;
    const float b3 = p.kb3 * (l + w);
    const float c3 = p.kc3 * w * l;
    const float r3 = (b3 + sqrtf(b3 * b3 - p.k4a3 * c3)) / 2.0f;
    float m = r1;  // python min(): the first of equal values
    if (r2 < m) m = r2;
    if (r3 < m) m = r3;
    return m;
}

__device__ __forceinline__ int wave_rank(unsigned long long bits) {
    const int lane = (int)__lane_id();
    return __popcll(bits & ((1ull << lane) - 1ull));
}

// Object of set s at position e of the set's list: class index q within the set (-1: in no task) and its box row.
__device__ __forceinline__ int object_of(const Plan &p, int s, int b, int t, int e, const int *tpre, const float *__restrict__ boxes,
                                         const int *__restrict__ classes, const int *__restrict__ traj, const float *&row) {
    if (s == 2) {  // forecast: every timestep's objects in timestep order, class = timestep
        int tt = 0;
        while (tt + 1 < p.T && e >= tpre[tt + 1]) ++tt;
        const int64_t o = ((int64_t)b * p.T + tt) * p.n_max + (e - tpre[tt]);
        row = boxes + o * 12;
        return tt < kForecastClasses ? tt : -1;
    }
    const int64_t o = ((int64_t)b * p.T + t) * p.n_max + e;
    row = boxes + o * 12;
    if (s == 1) {
        const int v = traj[o];
        return (v >= 0 && v < kTrajectoryClasses) ? v : -1;
    }
    const int v = classes[o];
    return (v >= 1 && v <= p.Qstd) ? v - 1 : -1;
}

__global__ void __launch_bounds__(kThreads) targets_objects(Plan p, const float *__restrict__ boxes, const int *__restrict__ counts,
                                                            const int *__restrict__ classes, const int *__restrict__ traj,
                                                            int64_t *__restrict__ ind, uint8_t *__restrict__ mask, int64_t *__restrict__ cat,
                                                            float *__restrict__ anno, float *__restrict__ gtbc, int *__restrict__ status,
                                                            Rec *__restrict__ recs, int *__restrict__ rec_count) {
    const int s = blockIdx.x % p.n_sets;
    const int t = (blockIdx.x / p.n_sets) % p.T;
    const int b = blockIdx.x / (p.n_sets * p.T);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    __shared__ int tpre[kForecastClasses + 2];
    __shared__ int cnt[kMaxQ], excl[kMaxQ + 1], run[kMaxQ], wq[kWaves][kMaxQ];
    __shared__ int qtask[kMaxQ], qfirst[kMaxU], drun[kMaxU], wd[kWaves][kMaxU];

    // the set's classes and tasks: set 0 = the config's tasks (class q + 1 = global class id), set 1 / 2 = one task of 3 / 7 classes
    const int u0 = s == 0 ? 0 : p.n_tasks + (s - 1);
    const int nu = s == 0 ? p.n_tasks : 1;
    const int nq = s == 0 ? p.Qstd : (s == 1 ? kTrajectoryClasses : kForecastClasses);
    int n = 0;
    if (s == 2) {
        if (tid == 0) {
            int acc = 0;
            for (int tt = 0; tt < p.T; ++tt) {
                tpre[tt] = acc;
                acc += fd::device_count(p.n_max, counts + (int64_t)b * p.T + tt);
            }
            tpre[p.T] = acc;
        }
        __syncthreads();
        n = tpre[p.T];
    } else {
        n = fd::device_count(p.n_max, counts + (int64_t)b * p.T + t);
    }
    if (tid < nq) {
        int u = 0, acc = 0;
        if (s == 0)
            while (acc + p.C[u] <= tid) acc += p.C[u++];
        qtask[tid] = u0 + u;
        cnt[tid] = 0;
        run[tid] = 0;
    }
    if (tid < nu) drun[tid] = 0;
    __syncthreads();

    // pass A: objects per class
    for (int base = 0; base < n; base += kThreads) {
        const int e = base + tid;
        const float *row;
        const int q = e < n ? object_of(p, s, b, t, e, tpre, boxes, classes, traj, row) : -1;
        for (int k = 0; k < nq; ++k) {
            const unsigned long long bits = __ballot(q == k);
            if (lane == 0) wq[wave][k] = __popcll(bits);
        }
        __syncthreads();
        if (tid < nq) cnt[tid] += wq[0][tid] + wq[1][tid] + wq[2][tid] + wq[3][tid];
        __syncthreads();
    }
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < nq; ++k) {
            excl[k] = acc;
            acc += cnt[k];
        }
        excl[nq] = acc;
        for (int k = nq - 1; k >= 0; --k) qfirst[qtask[k] - u0] = k;
    }
    __syncthreads();
    const int total = excl[nq];

    const int mo = p.max_objs;
    const int64_t list0 = ((int64_t)t * p.U) * p.B + b;  // row list of map u: list0 + u * B
    float *gt_set = gtbc + (((int64_t)s * p.T + t) * p.B + b) * mo * 13;

    // pass B: slots, rows and draw records
    for (int base = 0; base < n; base += kThreads) {
        const int e = base + tid;
        const float *row = nullptr;
        const int q = e < n ? object_of(p, s, b, t, e, tpre, boxes, classes, traj, row) : -1;
        int rank = 0;
        for (int k = 0; k < nq; ++k) {
            const unsigned long long bits = __ballot(q == k);
            if (q == k) rank = wave_rank(bits);
            if (lane == 0) wq[wave][k] = __popcll(bits);
        }
        __syncthreads();
        int u = -1, slot = -1, pos = -1;
        bool drawn = false;
        Rec rec = {0, 0, 0, 0};
        float vals[14];
        float box[12];
        if (q >= 0) {
            for (int w = 0; w < wave; ++w) rank += wq[w][q];
            rank += run[q];
            u = qtask[q];
            pos = excl[q] + rank;                          // row of gt_boxes_and_cls: every task's objects in task order
            slot = excl[q] - excl[qfirst[u - u0]] + rank;  // slot k of the task's rows (preprocess.py:411-451)
            for (int i = 0; i < 12; ++i) box[i] = row[i];
            box[10] = limit_period(box[10], p.period);
            box[11] = limit_period(box[11], p.period);
            for (int i = 0; i < 14; ++i) vals[i] = 0.0f;
            // preprocess.py:485-512
            const float ws = box[3] / p.vsx / p.osf, ls = box[4] / p.vsy / p.osf;
            if (slot < mo && ws > 0.0f && ls > 0.0f) {
                float mult = 1.0f;
                if (p.radius_mult) {
                    const float vn = sqrtf(box[6] * box[6] + box[7] * box[7]);
                    const float m = vn * (float)(1 + t) / 2.0f;
                    mult = m > 1.0f ? m : 1.0f;  // python max(1, m) / min(., 4); a NaN gives 1 like max()
                    mult = 4.0f < mult ? 4.0f : mult;
                }
                const float rf = mult * gaussian_radius_f32(ls, ws, p);
                int r = rf < 1048576.0f ? (int)rf : 1048576;  // int() truncates; the cap only keeps the conversion defined
                r = r > p.min_radius ? r : p.min_radius;
                const float cx = (box[0] - p.pcx) / p.vsx / p.osf, cy = (box[1] - p.pcy) / p.vsy / p.osf;
                // ct.astype(int32) truncates: 0 <= int(c) < W  <=>  -1 < c < W
                if (cx > -1.0f && cx < (float)p.W && cy > -1.0f && cy < (float)p.H) {
                    const int xi = (int)cx, yi = (int)cy;
                    drawn = true;
                    rec.x = xi;
                    rec.y = yi;
                    rec.c = q - qfirst[u - u0];
                    rec.r = r;
                    vals[0] = cx - (float)xi;
                    vals[1] = cy - (float)yi;
                    vals[2] = box[2];
                    vals[3] = logf(box[3]);
                    vals[4] = logf(box[4]);
                    vals[5] = logf(box[5]);
                    vals[6] = box[6];
                    vals[7] = box[7];
                    vals[8] = box[8];
                    vals[9] = box[9];
                    vals[10] = sinf(box[10]);
                    vals[11] = cosf(box[10]);
                    vals[12] = sinf(box[11]);
                    vals[13] = cosf(box[11]);
                }
            }
        }
        // compact draw records per task, in object order
        int drank = 0;
        for (int k = 0; k < nu; ++k) {
            const unsigned long long bits = __ballot(drawn && u - u0 == k);
            if (drawn && u - u0 == k) drank = wave_rank(bits);
            if (lane == 0) wd[wave][k] = __popcll(bits);
        }
        __syncthreads();
        if (q >= 0) {
            const int64_t list = list0 + (int64_t)u * p.B;
            if (slot < mo) {
                const int64_t o = list * mo + slot;
                ind[o] = drawn ? (int64_t)rec.y * p.W + rec.x : 0;
                mask[o] = drawn ? 1 : 0;
                cat[o] = drawn ? rec.c : 0;
                float *a = anno + o * 14;
                for (int i = 0; i < 14; ++i) a[i] = vals[i];
            }
            if (drawn) {
                for (int w = 0; w < wave; ++w) drank += wd[w][u - u0];
                drank += drun[u - u0];
                recs[list * mo + drank] = rec;
            }
            if (pos < mo) {  // preprocess.py:548-567: x y z w l h rot rrot vx vy rvx rvy class
                float *g = gt_set + (int64_t)pos * 13;
                for (int i = 0; i < 6; ++i) g[i] = box[i];
                g[6] = box[10];
                g[7] = box[11];
                for (int i = 6; i < 10; ++i) g[i + 2] = box[i];
                g[12] = (float)(q + 1);
            }
        }
        __syncthreads();
        if (tid < nq) run[tid] += wq[0][tid] + wq[1][tid] + wq[2][tid] + wq[3][tid];
        if (tid < nu) drun[tid] += wd[0][tid] + wd[1][tid] + wd[2][tid] + wd[3][tid];
        __syncthreads();
    }

    // unused slots of every task and unused gt rows: zeros
    for (int k = 0; k < nu; ++k) {
        const int u = u0 + k;
        int used = excl[qfirst[k] + p.C[u]] - excl[qfirst[k]];
        used = used < mo ? used : mo;
        const int64_t list = list0 + (int64_t)u * p.B;
        for (int i = used + tid; i < mo; i += kThreads) {
            const int64_t o = list * mo + i;
            ind[o] = 0;
            mask[o] = 0;
            cat[o] = 0;
        }
        for (int i = used * 14 + tid; i < mo * 14; i += kThreads) anno[list * mo * 14 + i] = 0.0f;
        if (tid == 0) rec_count[list] = drun[k];
    }
    const int used = total < mo ? total : mo;
    for (int i = used * 13 + tid; i < mo * 13; i += kThreads) gt_set[i] = 0.0f;
    if (tid == 0) status[((int64_t)b * p.T + t) * p.n_sets + s] = total > mo ? 1 : 0;  // preprocess.py:562: assert num_obj <= max_objs
}

// (t, u, b) record list and channel of heat-map plane pl (planes: [T][map u][B][C_u])
__device__ __forceinline__ void plane_owner(const Plan &p, int64_t pl, int64_t &list, int &c, int64_t &list_plane0) {
    const int64_t per_t = (int64_t)p.Csum * p.B;
    const int t = (int)(pl / per_t);
    const int r = (int)(pl - t * per_t);
    int u = 0;
    while (u + 1 < p.U && r >= p.cbase[u + 1] * p.B) ++u;
    const int r2 = r - p.cbase[u] * p.B;
    const int b = r2 / p.C[u];
    c = r2 - b * p.C[u];
    list = ((int64_t)t * p.U + u) * p.B + b;
    list_plane0 = pl - c;  // plane of channel 0 of this (t, u, b)
}

__global__ void __launch_bounds__(kThreads) targets_heatmap(Plan p, const Rec *__restrict__ recs, const int *__restrict__ rec_count,
                                                            float *__restrict__ hm) {
    __shared__ int4 srec[kThreads];  // (plane, x, y, r) of the staged records
    __shared__ double sden[kThreads];
    __shared__ int wn[kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t t0 = (int64_t)blockIdx.x * kTile;
    const int64_t t1 = t0 + kTile < p.total ? t0 + kTile : p.total;  // >= t0 + 1
    const int64_t e0 = t0 + tid * 4;

    int64_t epl[4];
    int ex[4], ey[4];
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; ++i) {
        const int64_t e = e0 + i;
        epl[i] = e < p.total ? e / p.hw : -1;
        const int rem = e < p.total ? (int)(e - epl[i] * p.hw) : 0;
        ey[i] = rem / p.W;
        ex[i] = rem - ey[i] * p.W;
    }

    int64_t prev_list = -1;
    for (int64_t pl = t0 / p.hw; pl <= (t1 - 1) / p.hw; ++pl) {
        int64_t list, plane0;
        int c_unused;
        plane_owner(p, pl, list, c_unused, plane0);
        if (list == prev_list) continue;  // the channels of one (t, u, b) share its record list
        prev_list = list;
        const int nrec = rec_count[list];
        const Rec *lr = recs + list * p.max_objs;
        for (int base = 0; base < nrec; base += kThreads) {
            bool keep = false;
            int4 sr = make_int4(0, 0, 0, 0);
            if (base + tid < nrec) {
                const Rec r = lr[base + tid];
                const int64_t rp = plane0 + r.c;
                const int ylo = r.y - r.r > 0 ? r.y - r.r : 0, yhi = r.y + r.r < p.H - 1 ? r.y + r.r : p.H - 1;
                const int xlo = r.x - r.r > 0 ? r.x - r.r : 0, xhi = r.x + r.r < p.W - 1 ? r.x + r.r : p.W - 1;
                const int64_t lo = rp * p.hw + (int64_t)ylo * p.W + xlo, hi = rp * p.hw + (int64_t)yhi * p.W + xhi;
                keep = hi >= t0 && lo < t1;
                sr = make_int4((int)(rp - plane0), r.x, r.y, r.r);
            }
            const unsigned long long bits = __ballot(keep);
            if (lane == 0) wn[wave] = __popcll(bits);
            __syncthreads();
            int at = wave_rank(bits), nkeep = 0;
            for (int w = 0; w < kWaves; ++w) {
                if (w < wave) at += wn[w];
                nkeep += wn[w];
            }
            if (keep) {
                srec[at] = sr;
                const double sigma = (double)(2 * sr.w + 1) / 6.0;
                sden[at] = 2.0 * sigma * sigma;
            }
            __syncthreads();
            for (int k = 0; k < nkeep; ++k) {
                const int4 r = srec[k];
                const int64_t rp = plane0 + r.x;
                for (int i = 0; i < 4; ++i) {
                    const int dx = ex[i] - r.y, dy = ey[i] - r.z;
                    if (epl[i] == rp && dx <= r.w && dx >= -r.w && dy <= r.w && dy >= -r.w) {
                        const float g = (float)exp(-(double)(dx * dx + dy * dy) / sden[k]);
                        v[i] = g > v[i] ? g : v[i];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (e0 < p.total)  // the buffer holds total rounded up to 4 elements; the last tile's tail stops there
        *reinterpret_cast<float4 *>(hm + e0) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

extern "C" size_t fd_targets_workspace_bytes(int B, int T, int maps_per_step, int max_objs) {
    const size_t lists = (size_t)(B > 0 ? B : 0) * (T > 0 ? T : 0) * (maps_per_step > 0 ? maps_per_step : 0);
    return fd::align_up(lists * (size_t)(max_objs > 0 ? max_objs : 0) * sizeof(Rec), 256) + fd::align_up(lists * sizeof(int), 256);
}

extern "C" int fd_assign_targets(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory, int B,
                                 const fd_targets_cfg *cfg, float *hm, int64_t *ind, uint8_t *mask, int64_t *cat, float *anno_box,
                                 float *gt_boxes_and_cls, int32_t *status, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(cfg, "fd_assign_targets: null cfg");
    const fd_targets_cfg &c = *cfg;
    FD_REQUIRE(B >= 1 && c.T >= 1 && c.n_max >= 0 && c.max_objs >= 1 && c.H >= 1 && c.W >= 1, "fd_assign_targets: bad sizes");
    FD_REQUIRE(c.n_sets == 1 || c.n_sets == 3, "fd_assign_targets: n_sets must be 1 (standard) or 3 (+ trajectory, forecast)");
    FD_REQUIRE(c.n_tasks >= 1 && c.n_tasks <= FD_TARGETS_MAX_TASKS, "fd_assign_targets: n_tasks must be in [1, %d]", FD_TARGETS_MAX_TASKS);
    FD_REQUIRE(c.n_sets == 1 || c.T <= kForecastClasses, "fd_assign_targets: the forecast set has %d classes, T = %d", kForecastClasses, c.T);
    FD_REQUIRE(c.out_size_factor > 0.0f && c.voxel_x > 0.0f && c.voxel_y > 0.0f, "fd_assign_targets: bad geometry");
    FD_REQUIRE(boxes && counts && classes && (c.n_sets == 1 || trajectory) && hm && ind && mask && cat && anno_box && gt_boxes_and_cls && status &&
               workspace, "fd_assign_targets: null argument");
    FD_REQUIRE(((uintptr_t)hm & 15) == 0, "fd_assign_targets: hm must be 16-byte aligned");
    Plan p;
    p.B = B; p.T = c.T; p.H = c.H; p.W = c.W; p.n_max = c.n_max; p.max_objs = c.max_objs; p.n_sets = c.n_sets; p.n_tasks = c.n_tasks;
    p.U = c.n_tasks + (c.n_sets == 3 ? 2 : 0);
    p.radius_mult = c.radius_mult ? 1 : 0;
    p.min_radius = c.min_radius;
    int acc = 0;
    for (int u = 0; u < p.U; ++u) {
        const int cu = u < c.n_tasks ? c.task_classes[u] : (u == c.n_tasks ? kTrajectoryClasses : kForecastClasses);
        FD_REQUIRE(cu >= 1, "fd_assign_targets: task %d has no classes", u);
        p.C[u] = cu;
        p.cbase[u] = acc;
        acc += cu;
    }
    p.Csum = acc;
    p.Qstd = 0;
    for (int u = 0; u < c.n_tasks; ++u) p.Qstd += c.task_classes[u];
    FD_REQUIRE(p.Qstd <= kMaxQ, "fd_assign_targets: at most %d classes over the tasks", kMaxQ);
    p.osf = c.out_size_factor; p.vsx = c.voxel_x; p.vsy = c.voxel_y; p.pcx = c.pc_x; p.pcy = c.pc_y;
    const double ov = c.gaussian_overlap;  // the reference's python-float constants, each rounded to float32 where it meets a float32
    p.k1m = (float)(1 - ov);
    p.k1p = (float)(1 + ov);
    p.kb3 = (float)(-2 * ov);
    p.kc3 = (float)(ov - 1);
    p.k4a3 = (float)(4 * (4 * ov));
    p.period = (float)(3.141592653589793 * 2);
    p.hw = (int64_t)c.H * c.W;
    p.total = (int64_t)c.T * p.Csum * B * p.hw;
    const size_t lists = (size_t)B * c.T * p.U;
    FD_REQUIRE(workspace_bytes >= fd_targets_workspace_bytes(B, c.T, p.U, c.max_objs), "fd_assign_targets: workspace too small");
    Rec *recs = (Rec *)workspace;
    int *rec_count = (int *)((char *)workspace + fd::align_up(lists * c.max_objs * sizeof(Rec), 256));
    hipStream_t stream = fd::as_stream(stream_);
    hipLaunchKernelGGL(targets_objects, dim3((unsigned)(B * c.T * c.n_sets)), dim3(kThreads), 0, stream, p, boxes, counts, classes, trajectory,
                       ind, mask, cat, anno_box, gt_boxes_and_cls, status, recs, rec_count);
    const int64_t tiles = (p.total + kTile - 1) / kTile;
    hipLaunchKernelGGL(targets_heatmap, dim3((unsigned)tiles), dim3(kThreads), 0, stream, p, (const Rec *)recs, (const int *)rec_count, hm);
    return fd::check_launch("fd_assign_targets");
}
