// GT-database sampling ("GT-AUG") of a whole batch: which drawn database entries are pasted into a sample, their ground-truth rows, and
// their points (include/futuredet_hip.h has the contracts, the arithmetic and the reference lines).  Built with -ffp-contract=off:
// every product and every sum below is one IEEE operation rounded on its own, so every result is bit-defined.
//
//   sample_select  one workgroup of 256 lanes per sample.
//                  0  the counts of the sample's timesteps and the per-group tallies of its timestep-0 objects go to LDS (a column of
//                     per-lane tallies per group, summed by one lane each: no atomics);
//                  1  lane i < K validates slot i and computes its entry's BEV corners twice: as a candidate (angle = column 11) and as
//                     an obstacle (column 10), with their stand-up boxes, into LDS;
//                  2  every lane takes ground-truth objects (its corners in registers) and tests them against the participating slots;
//                     a wave ballot per slot folds the hits into one 64-bit word per wave;
//                  3  wave w fills rows w, w + 4, ... of the K x K slot matrix, lane j = column j, one ballot per row;
//                  4  every lane walks the groups and slots over those words on its own (wave-uniform, nothing to exchange);
//                  5  the accepted entries' rows are appended (one lane per (slot, timestep)) and the plan is written.
//   sample_points  one lane per staged row; the <= 64 plan offsets live in LDS and a lane finds its slot by a binary search.
#include <math.h>

#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = FD_GT_SAMPLE_MAX_K;
constexpr int kMaxG = FD_GT_SAMPLE_MAX_GROUPS;
constexpr int kMaxT = FD_GT_SAMPLE_MAX_T;
static_assert(kMaxK == 64, "a slot set is one 64-bit word and one wave's ballot");

typedef fd_gt_sample_group Group;
typedef fd_gt_sample_plan Plan;

struct Groups {
    Group g[kMaxG];
};

struct Quad {  // four BEV corners and their stand-up box
    float x[4], y[4];
    float su[4];  // xmin, ymin, xmax, ymax
};

__device__ __forceinline__ float fmin_py(float a, float b) { return b < a ? b : a; }  // Python's min(a, b)
__device__ __forceinline__ float fmax_py(float a, float b) { return b > a ? b : a; }

// center_to_corner_box2d for one box row with the angle given
__device__ __forceinline__ void corners_of(float cx, float cy, float w, float l, float a, Quad &q) {
    const float s = (float)sin((double)a), c = (float)cos((double)a);
    const float hx = w * 0.5f, hy = l * 0.5f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ox = (k < 2) ? -hx : hx, oy = (k == 1 || k == 2) ? hy : -hy;
        const float xc = ox * c, ys = oy * s, xs = ox * s, yc = oy * c;
        q.x[k] = (xc + ys) + cx;
        q.y[k] = (-xs + yc) + cy;
    }
    q.su[0] = q.su[2] = q.x[0];
    q.su[1] = q.su[3] = q.y[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        q.su[0] = fminf(q.su[0], q.x[k]);
        q.su[1] = fminf(q.su[1], q.y[k]);
        q.su[2] = fmaxf(q.su[2], q.x[k]);
        q.su[3] = fmaxf(q.su[3], q.y[k]);
    }
}

// all four corners of q strictly inside p (clockwise): box_collision_test's "complete overlap" loops
__device__ __forceinline__ bool holds(const Quad &p, const Quad &q) {
    for (int l = 0; l < 4; ++l)
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const float vx = -(p.x[k] - p.x[k1]), vy = -(p.y[k] - p.y[k1]);
            float cross = vy * (p.x[k] - q.x[l]);
            cross = cross - vx * (p.y[k] - q.y[l]);
            if (cross >= 0) return false;
        }
    return true;
}

// box_collision_test(boxes = p, qboxes = q) for one pair
__device__ __forceinline__ bool collide(const Quad &p, const Quad &q) {
    const float iw = fmin_py(p.su[2], q.su[2]) - fmax_py(p.su[0], q.su[0]);
    if (!(iw > 0)) return false;
    const float ih = fmin_py(p.su[3], q.su[3]) - fmax_py(p.su[1], q.su[1]);
    if (!(ih > 0)) return false;
    for (int k = 0; k < 4; ++k) {
        const float ax = p.x[k], ay = p.y[k], bx = p.x[(k + 1) & 3], by = p.y[(k + 1) & 3];
        for (int l = 0; l < 4; ++l) {
            const float cx = q.x[l], cy = q.y[l], dx = q.x[(l + 1) & 3], dy = q.y[(l + 1) & 3];
            const bool acd = (dy - ay) * (cx - ax) > (cy - ay) * (dx - ax);
            const bool bcd = (dy - by) * (cx - bx) > (cy - by) * (dx - bx);
            if (acd != bcd) {
                const bool abc = (cy - ay) * (bx - ax) > (by - ay) * (cx - ax);
                const bool abd = (dy - ay) * (bx - ax) > (by - ay) * (dx - ax);
                if (abc != abd) return true;
            }
        }
    }
    if (holds(p, q)) return true;
    return holds(q, p);
}

__device__ __forceinline__ int clamp_count(int c, int n_max) { return c < 0 ? 0 : (c > n_max ? n_max : c); }
__device__ __forceinline__ unsigned long long bit(int i) { return 1ull << i; }

struct SelectArgs {
    const float *boxes;
    const int *counts, *classes, *traj;
    const float *db_boxes;
    const int *db_steps, *db_class, *db_traj;
    const int64_t *db_off;
    const int *cand;
    float *boxes_out;
    int *counts_out, *classes_out, *traj_out, *accepted;
    Plan *plan;
    int *n_points, *status;
    double rate;
    int64_t P;
    int G, T, n_max, K, M, Tdb, point_cap;
};

__global__ void __launch_bounds__(kThreads) sample_select(SelectArgs a, Groups groups) {
    __shared__ Quad s_quad[2][kMaxK];  // [0]: as a candidate (column 11), [1]: as an obstacle (column 10)
    __shared__ int s_tally[kMaxG][kThreads];
    __shared__ unsigned long long s_gmask[kMaxG];
    __shared__ int s_count[kMaxT];
    __shared__ int s_entry[kMaxK], s_rows[kMaxK];
    __shared__ unsigned long long s_row[kMaxK], s_gt_wave[kWaves], s_valid, s_bad;

    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, n_max = a.n_max, K = a.K, G = a.G;
    const int64_t bt0 = (int64_t)b * T;

    // 0: counts and tallies
    if (tid < T) s_count[tid] = a.counts[bt0 + tid];
    const int c0_raw = a.counts[bt0], c0 = clamp_count(c0_raw, n_max);
    {
        int tally[kMaxG];
#pragma unroll
        for (int g = 0; g < kMaxG; ++g) tally[g] = 0;
        for (int i = tid; i < c0; i += kThreads) {
            const int cls = a.classes[bt0 * n_max + i], tr = a.traj ? a.traj[bt0 * n_max + i] : -1;
#pragma unroll
            for (int g = 0; g < kMaxG; ++g)
                if (g < G) tally[g] += cls == groups.g[g].class_id && (groups.g[g].trajectory < 0 || tr == groups.g[g].trajectory);
        }
#pragma unroll
        for (int g = 0; g < kMaxG; ++g) s_tally[g][tid] = tally[g];
    }

    // 1: the slots
    if (tid < kMaxK) {
        const int e = tid < K ? a.cand[(int64_t)b * K + tid] : -1;
        bool valid = e >= 0 && e < a.M, bad = tid < K && !valid && e != -1;
        int rows = 0;
        if (valid) {
            const int64_t o0 = a.db_off[e], o1 = a.db_off[e + 1];
            if (o0 < 0 || o1 < o0 || o1 > a.P || o1 - o0 > FD_AUGMENT_MAX_ROWS) {  // not a row range of db_points: an empty slot
                valid = false;
                bad = true;
            } else {
                rows = (int)(o1 - o0);
            }
        }
        s_entry[tid] = valid ? e : -1;
        s_rows[tid] = rows;
        if (valid) {
            const float *row = a.db_boxes + (int64_t)e * a.Tdb * 12;
            corners_of(row[0], row[1], row[3], row[4], row[11], s_quad[0][tid]);
            corners_of(row[0], row[1], row[3], row[4], row[10], s_quad[1][tid]);
        }
        const unsigned long long v = __ballot(valid), w = __ballot(bad);
        if (tid == 0) {
            s_valid = v;
            s_bad = w;
        }
    }
    __syncthreads();
    if (tid < G) {  // one lane per group: how many of its slots take part, and which
        int n = 0;
        for (int i = 0; i < kThreads; ++i) n += s_tally[tid][i];
        double want = rint(a.rate * (double)(groups.g[tid].max_num - n));  // np.round: half to even
        want = !(want > 0.0) ? 0.0 : (want > (double)kMaxK ? (double)kMaxK : want);
        const unsigned long long valid = s_valid;
        unsigned long long m = 0;
        int taken = 0;
        const int first = groups.g[tid].first, end = first + groups.g[tid].n;
        for (int i = first; i < end && taken < (int)want; ++i)
            if (valid & bit(i)) {
                m |= bit(i);
                ++taken;
            }
        s_gmask[tid] = m;
    }
    __syncthreads();

    // who takes part, and in which group (the same words in every lane)
    unsigned long long part = 0;
    int status = s_bad ? FD_GT_SAMPLE_BAD_INDEX : 0;
    int my_group = -1;  // of slot `lane`
    for (int g = 0; g < G; ++g) {
        part |= s_gmask[g];
        if (s_gmask[g] & bit(lane)) my_group = g;
    }

    // 2: ground truth against the slots
    unsigned long long gt_hits = 0;
    if (part) {
        for (int base = 0; base < c0; base += kThreads) {
            const int j = base + tid;
            const bool live = j < c0;
            Quad q;
            if (live) {
                const float *row = a.boxes + (bt0 * n_max + j) * 12;
                corners_of(row[0], row[1], row[3], row[4], row[10], q);
            }
            for (int i = 0; i < K; ++i) {
                if (!(part & bit(i))) continue;
                const bool hit = live && collide(s_quad[0][i], q);
                if (__ballot(hit)) gt_hits |= bit(i);
            }
        }
    }
    if (lane == 0) s_gt_wave[wave] = gt_hits;

    // 3: the slots against one another; column j is an obstacle for row i when it belongs to i's group (as a candidate) or to an
    //    earlier one (as a ground-truth row)
    for (int i = wave; i < K; i += kWaves) {
        int gi = -1;
        for (int g = 0; g < G; ++g)
            if (s_gmask[g] & bit(i)) gi = g;
        bool hit = false;
        if (gi >= 0 && my_group >= 0 && lane != i && my_group <= gi) hit = collide(s_quad[0][i], s_quad[my_group == gi ? 0 : 1][lane]);
        const unsigned long long votes = __ballot(hit);
        if (lane == 0) s_row[i] = votes;
    }
    __syncthreads();
    gt_hits = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) gt_hits |= s_gt_wave[w];

    // 4: the walk
    int max_count = 0, differ = 0;
    for (int t = 0; t < T; ++t) {
        const int c = clamp_count(s_count[t], n_max);
        max_count = c > max_count ? c : max_count;
        differ |= s_count[t] != c0_raw;
    }
    if (differ) status |= FD_GT_SAMPLE_COUNTS_DIFFER;
    unsigned long long accepted = 0;
    int n_acc = 0, n_pts = 0;
    for (int g = 0; g < G; ++g) {
        unsigned long long obstacles = accepted | s_gmask[g];
        unsigned long long todo = s_gmask[g];
        while (todo) {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            bool ok = !(gt_hits & bit(i)) && !(s_row[i] & obstacles & ~bit(i));
            if (ok && max_count + n_acc >= n_max) {
                ok = false;
                status |= FD_GT_SAMPLE_NO_ROW;
            }
            if (ok && s_rows[i] > a.point_cap - n_pts) {
                ok = false;
                status |= FD_GT_SAMPLE_NO_POINTS;
            }
            if (ok) {
                accepted |= bit(i);
                ++n_acc;
                n_pts += s_rows[i];
            } else {
                obstacles &= ~bit(i);
            }
        }
    }

    // out of place: the rows that were there
    if (a.boxes_out != a.boxes) {
        for (int t = 0; t < T; ++t) {
            const int c = clamp_count(s_count[t], n_max);
            const float4 *src = reinterpret_cast<const float4 *>(a.boxes) + (bt0 + t) * n_max * 3;
            float4 *dst = reinterpret_cast<float4 *>(a.boxes_out) + (bt0 + t) * n_max * 3;
            for (int i = tid; i < c * 3; i += kThreads) dst[i] = src[i];
            for (int i = tid; i < c; i += kThreads) {
                a.classes_out[(bt0 + t) * n_max + i] = a.classes[(bt0 + t) * n_max + i];
                if (a.traj) a.traj_out[(bt0 + t) * n_max + i] = a.traj[(bt0 + t) * n_max + i];
            }
        }
    }

    // 5: the new rows
    for (int item = tid; item < T * K; item += kThreads) {
        const int t = item / K, i = item - t * K;
        if (!(accepted & bit(i))) continue;
        const int e = s_entry[i], r = __popcll(accepted & (bit(i) - 1ull));
        const int64_t at = (bt0 + t) * n_max + clamp_count(s_count[t], n_max) + r;  // < n_max: the walk saw max_count + r < n_max
        const float4 *e0 = reinterpret_cast<const float4 *>(a.db_boxes + (int64_t)e * a.Tdb * 12);
        const int steps = a.db_steps[e], tt = (t < steps && t < a.Tdb) ? t : 0;
        const float *et = a.db_boxes + ((int64_t)e * a.Tdb + tt) * 12;
        float4 *dst = reinterpret_cast<float4 *>(a.boxes_out) + at * 3;
        const float4 q0 = e0[0], q1 = e0[1];
        dst[0] = q0;
        dst[1] = make_float4(q1.x, q1.y, et[6], et[7]);
        dst[2] = make_float4(et[8], et[9], et[10], et[11]);
        a.classes_out[at] = a.db_class[e];
        if (a.traj) a.traj_out[at] = a.db_traj[e];
    }
    if (tid < T) a.counts_out[bt0 + tid] = clamp_count(s_count[tid], n_max) + n_acc;
    if (tid < K) {
        const bool acc = (accepted >> tid) & 1ull;
        int before = 0;
        for (int i = 0; i < tid; ++i)
            if (accepted & bit(i)) before += s_rows[i];
        a.accepted[(int64_t)b * K + tid] = acc ? 1 : 0;
        Plan p;
        p.src_row = acc ? a.db_off[s_entry[tid]] : 0;
        p.rows = acc ? s_rows[tid] : 0;
        p.dst_row = before;
        a.plan[(int64_t)b * K + tid] = p;
    }
    if (tid == 0) {
        a.n_points[b] = n_pts;
        a.status[b] = status;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the paste
template <int NDIM, bool VEC>
__global__ void __launch_bounds__(kThreads) sample_points(const float *__restrict__ db_points, int64_t P, const float *__restrict__ db_boxes,
                                                          int M, int Tdb, const int *__restrict__ cand, const int *__restrict__ accepted,
                                                          const Plan *__restrict__ plan, int K, float *__restrict__ dst, int point_cap) {
    __shared__ int s_dst[kMaxK], s_n[kMaxK];
    __shared__ int64_t s_src[kMaxK];
    __shared__ float s_c[kMaxK][3];
    const int tid = (int)threadIdx.x;
    if (tid < K) {
        const Plan p = plan[tid];
        const int e = cand[tid];
        const bool ok = accepted[tid] != 0 && e >= 0 && e < M && p.rows > 0 && p.src_row >= 0 && p.src_row <= P - p.rows;
        s_dst[tid] = p.dst_row;
        s_n[tid] = ok ? p.rows : 0;
        s_src[tid] = p.src_row;
        const float *c = db_boxes + (int64_t)(ok ? e : 0) * Tdb * 12;
        s_c[tid][0] = ok ? c[0] : 0.f;
        s_c[tid][1] = ok ? c[1] : 0.f;
        s_c[tid][2] = ok ? c[2] : 0.f;
    }
    __syncthreads();
    const int r = (int)(blockIdx.x * kThreads + tid);
    if (r >= point_cap) return;
    int lo = 0, hi = K;  // the last slot whose first row is at or below r (the offsets never decrease)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_dst[mid] <= r) lo = mid; else hi = mid;
    }
    float v[NDIM];
    const int k = r - s_dst[lo];
    if (k >= 0 && k < s_n[lo]) {
        const int64_t j = s_src[lo] + k;
        if (VEC) {
            const float4 q = reinterpret_cast<const float4 *>(db_points)[j];
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int d = 0; d < NDIM; ++d) v[d] = db_points[j * NDIM + d];
        }
        v[0] = v[0] + s_c[lo][0];
        v[1] = v[1] + s_c[lo][1];
        v[2] = v[2] + s_c[lo][2];
    } else {
        v[0] = v[1] = v[2] = FD_GT_SAMPLE_SENTINEL;
#pragma unroll
        for (int d = 3; d < NDIM; ++d) v[d] = 0.f;
    }
    if (VEC) {
        reinterpret_cast<float4 *>(dst)[r] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int d = 0; d < NDIM; ++d) dst[(int64_t)r * NDIM + d] = v[d];
    }
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool disjoint(const void *a, const void *b, size_t bytes_a, size_t bytes_b) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x + bytes_a <= y || y + bytes_b <= x;
}
inline bool same_or_disjoint(const void *in, const void *out, size_t bytes) { return in == out || disjoint(in, out, bytes, bytes); }

}  // namespace

extern "C" int fd_gt_sample_select(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory,
                                   const float *db_boxes, const int32_t *db_steps, const int32_t *db_class, const int32_t *db_traj,
                                   const int64_t *db_point_offset, int M, int Tdb, int64_t P, const int32_t *cand,
                                   const fd_gt_sample_group *groups_host, int G, double rate, int point_cap, float *boxes_out,
                                   int32_t *counts_out, int32_t *classes_out, int32_t *trajectory_out, int32_t *accepted,
                                   fd_gt_sample_plan *plan, int32_t *n_points, int32_t *status, int B, int T, int n_max, int K,
                                   fd_stream_t stream_) {
    FD_REQUIRE(B >= 1 && T >= 1 && T <= FD_GT_SAMPLE_MAX_T, "fd_gt_sample_select: B (%d) must be >= 1 and T (%d) lie in [1, %d]", B, T,
               FD_GT_SAMPLE_MAX_T);
    FD_REQUIRE(n_max >= 1 && n_max <= FD_RANGE_FILTER_MAX_N, "fd_gt_sample_select: n_max (%d) must lie in [1, %d]", n_max, FD_RANGE_FILTER_MAX_N);
    FD_REQUIRE((int64_t)B * T * n_max <= FD_AUGMENT_MAX_ROWS, "fd_gt_sample_select: B x T x n_max = %lld rows, at most %d", (long long)B * T * n_max,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(K >= 1 && K <= FD_GT_SAMPLE_MAX_K, "fd_gt_sample_select: K (%d) must lie in [1, %d]", K, FD_GT_SAMPLE_MAX_K);
    FD_REQUIRE(G >= 1 && G <= FD_GT_SAMPLE_MAX_GROUPS && groups_host, "fd_gt_sample_select: G (%d) must lie in [1, %d] with its records", G,
               FD_GT_SAMPLE_MAX_GROUPS);
    FD_REQUIRE(M >= 1 && Tdb >= 1 && P >= 0, "fd_gt_sample_select: M (%d) and Tdb (%d) must be >= 1, P (%lld) >= 0", M, Tdb, (long long)P);
    FD_REQUIRE(point_cap >= 0 && point_cap <= FD_AUGMENT_MAX_ROWS, "fd_gt_sample_select: point_cap (%d) must lie in [0, %d]", point_cap,
               FD_AUGMENT_MAX_ROWS);
    FD_REQUIRE(isfinite(rate) && rate >= 0, "fd_gt_sample_select: the rate (%g) must be finite and >= 0", rate);
    Groups gs;
    int end = 0;
    for (int g = 0; g < FD_GT_SAMPLE_MAX_GROUPS; ++g) {
        if (g >= G) {
            gs.g[g] = Group{-1, -1, 0, 0, 0};
            continue;
        }
        const Group &r = groups_host[g];
        FD_REQUIRE(r.n >= 0 && r.first >= end && r.first <= K && r.n <= K - r.first,
                   "fd_gt_sample_select: group %d takes the slots [%d, %d + %d): the groups must follow one another without overlap inside K = %d",
                   g, r.first, r.first, r.n, K);
        FD_REQUIRE(trajectory || r.trajectory < 0, "fd_gt_sample_select: group %d counts a trajectory class but trajectory is null", g);
        end = r.first + r.n;
        gs.g[g] = r;
    }
    FD_REQUIRE(boxes && counts && classes && db_boxes && db_steps && db_class && db_traj && db_point_offset && cand && boxes_out && counts_out &&
                   classes_out && accepted && plan && n_points && status,
               "fd_gt_sample_select: a null pointer other than trajectory / trajectory_out");
    FD_REQUIRE(!trajectory || trajectory_out, "fd_gt_sample_select: a trajectory needs trajectory_out");
    FD_REQUIRE(aligned(boxes, 16) && aligned(boxes_out, 16) && aligned(db_boxes, 16) && aligned(plan, 16),
               "fd_gt_sample_select: boxes, boxes_out, db_boxes and plan must be 16-byte aligned");
    FD_REQUIRE(aligned(db_point_offset, 8), "fd_gt_sample_select: db_point_offset must be 8-byte aligned");
    FD_REQUIRE(aligned(counts, 4) && aligned(classes, 4) && aligned(trajectory, 4) && aligned(counts_out, 4) && aligned(classes_out, 4) &&
                   aligned(trajectory_out, 4) && aligned(db_steps, 4) && aligned(db_class, 4) && aligned(db_traj, 4) && aligned(cand, 4) &&
                   aligned(accepted, 4) && aligned(n_points, 4) && aligned(status, 4),
               "fd_gt_sample_select: the int32 arrays must be 4-byte aligned");
    const size_t sets = (size_t)B * T, rows = sets * n_max;
    FD_REQUIRE(same_or_disjoint(boxes, boxes_out, rows * 48) && same_or_disjoint(counts, counts_out, sets * 4) &&
                   same_or_disjoint(classes, classes_out, rows * 4) && (!trajectory || same_or_disjoint(trajectory, trajectory_out, rows * 4)),
               "fd_gt_sample_select: an output must be its input itself or not overlap it");
    FD_REQUIRE((boxes == boxes_out) == (counts == counts_out) && (boxes == boxes_out) == (classes == classes_out) &&
                   (!trajectory || (boxes == boxes_out) == (trajectory == trajectory_out)),
               "fd_gt_sample_select: either every output is its input (in place) or none is");
    SelectArgs a;
    a.boxes = boxes; a.counts = counts; a.classes = classes; a.traj = trajectory;
    a.db_boxes = db_boxes; a.db_steps = db_steps; a.db_class = db_class; a.db_traj = db_traj; a.db_off = db_point_offset;
    a.cand = cand;
    a.boxes_out = boxes_out; a.counts_out = counts_out; a.classes_out = classes_out; a.traj_out = trajectory ? trajectory_out : nullptr;
    a.accepted = accepted; a.plan = plan; a.n_points = n_points; a.status = status;
    a.rate = rate; a.P = P;
    a.G = G; a.T = T; a.n_max = n_max; a.K = K; a.M = M; a.Tdb = Tdb; a.point_cap = point_cap;
    hipLaunchKernelGGL(sample_select, dim3((unsigned)B), dim3(kThreads), 0, fd::as_stream(stream_), a, gs);
    return fd::check_launch("fd_gt_sample_select");
}

extern "C" int fd_gt_sample_points(const float *db_points, int64_t P, int ndim, const float *db_boxes, int M, int Tdb, const int32_t *cand,
                                   const int32_t *accepted, const fd_gt_sample_plan *plan, int K, float *dst, int point_cap,
                                   fd_stream_t stream_) {
    FD_REQUIRE(ndim == 4 || ndim == 5, "fd_gt_sample_points: ndim must be 4 or 5 (got %d)", ndim);
    FD_REQUIRE(K >= 1 && K <= FD_GT_SAMPLE_MAX_K, "fd_gt_sample_points: K (%d) must lie in [1, %d]", K, FD_GT_SAMPLE_MAX_K);
    FD_REQUIRE(M >= 1 && Tdb >= 1 && P >= 0, "fd_gt_sample_points: M (%d) and Tdb (%d) must be >= 1, P (%lld) >= 0", M, Tdb, (long long)P);
    FD_REQUIRE(point_cap >= 0 && point_cap <= FD_AUGMENT_MAX_ROWS, "fd_gt_sample_points: point_cap (%d) must lie in [0, %d]", point_cap,
               FD_AUGMENT_MAX_ROWS);
    if (point_cap == 0) return FD_OK;
    FD_REQUIRE((db_points || P == 0) && db_boxes && cand && accepted && plan && dst, "fd_gt_sample_points: a null pointer");
    FD_REQUIRE(aligned(db_points, 4) && aligned(dst, 4) && aligned(db_boxes, 4) && aligned(cand, 4) && aligned(accepted, 4) && aligned(plan, 8),
               "fd_gt_sample_points: misaligned pointers (plan 8 bytes, the others 4)");
    FD_REQUIRE(disjoint(db_points, dst, (size_t)P * ndim * 4, (size_t)point_cap * ndim * 4), "fd_gt_sample_points: dst must not overlap db_points");
    hipStream_t st = fd::as_stream(stream_);
    const dim3 grid((unsigned)((point_cap + kThreads - 1) / kThreads)), block(kThreads);
    if (ndim == 4) {
        if (aligned(db_points, 16) && aligned(dst, 16))
            hipLaunchKernelGGL((sample_points<4, true>), grid, block, 0, st, db_points, P, db_boxes, M, Tdb, cand, accepted, plan, K, dst, point_cap);
        else
            hipLaunchKernelGGL((sample_points<4, false>), grid, block, 0, st, db_points, P, db_boxes, M, Tdb, cand, accepted, plan, K, dst, point_cap);
    } else {
        hipLaunchKernelGGL((sample_points<5, false>), grid, block, 0, st, db_points, P, db_boxes, M, Tdb, cand, accepted, plan, K, dst, point_cap);
    }
    return fd::check_launch("fd_gt_sample_points");
}
