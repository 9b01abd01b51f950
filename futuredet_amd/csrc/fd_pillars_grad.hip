// Training mode of the PointPillars reader (det3d/models/readers/pillar_encoder.py:15-164): PillarFeatureNet with the shipped
// stack (two PFNLayers, 32 (+32 repeated max) -> 64 units), BatchNorm1d on batch statistics, and its backward.
//
// N = M * P rows (every point slot of every pillar; padded slots are rows: their decorated features are 0).  Layer l:
//   z = W f,  x^ = (z - mean) * invstd,  y = gamma x^ + beta,  a = relu(y),  max over the pillar's P rows.
// Nothing of size [N, 64] is stored: every pass recomputes the decoration and layer 1 from the voxel rows.
//
// Statistics.  z1 = W1 f is linear in the decorated features f (fin <= 16 columns), so layer 1's batch statistics are
// mean1 = W1 mean_f and var1 = diag(W1 C_f W1^T) / N, with C_f the centred co-moment of f.  Layer 2's input in2 = [a1, max1]
// (64 columns) gives mean2 / var2 the same way from C_2.  Both co-moments come from per-block partials centred at the block's
// own mean (two passes over the block's pillars: sum, then the centred Gram on the matrix core, v_mfma_f32_16x16x4_f32),
// combined over blocks in double precision with Chan's rule.  Raw coordinates (tens of metres, intensities up to 255) would
// cancel badly in a plain sum of squares; centred partials do not.
//
// Backward (dout [M, 64]).  The max routes dout to the arg-max row; relu keeps it where the output is > 0: g2[m, v].
//   dbeta2 = sum g2, dgamma2 = sum g2 x^2(arg row);  the batch-stat BN backward dz2 = k (dy2 - dbeta2 / N - x^2 dgamma2 / N),
//   k = gamma2 invstd2, is dense.  Its dense terms are affine in in2, so
//   dW2 = k [SP - dbeta2 mean_in2^T - (dgamma2 / N) invstd2 (W2 C_2)],   SP[v][c] = sum_m g2[m, v] in2[m, arg2[m, v], c]
//   d in2[r] = c0 + A in2[r] + sp[r],   A = -W2^T diag(k dgamma2 invstd2 / N) W2,  c0 = W2^T (k (dgamma2 invstd2 mean2 - dbeta2) / N)
//   (sp[r] = the sparse rows k g2 W2 at the arg-max rows).  The max1 half of d in2 is summed over P and routed to layer 1's
//   arg-max; relu; then dbeta1 = sum dy1, dgamma1 = sum dy1 x^1 and
//   dW1 = k1 [sum dy1 f^T - dbeta1 mean_f^T - (dgamma1 / N) invstd1 (W1 C_f)].
// So the backward is one pass over the rows (layer-1 recompute, a 32 x 32 product per row) plus per-pillar work.
//
// Determinism: block b owns pillars [b * ppb, (b + 1) * ppb) with ppb a function of M only; wave w of the block takes the
// block's pillars w, w + 4, ...; waves are added in wave order; partials are reduced over blocks in 16 fixed slices whose sums
// are added in slice order.  No atomics: two runs give the same bits.
//
// Counts.  The batch is n_seg <= 16 segments of seg_stride rows; segment b's live pillars are its first cnt_b rows.  The logical
// batch is their concatenation in segment order, M = sum cnt_b pillars: every kernel derives M, ppb and the number of live blocks
// from the counts itself and maps logical pillar p to its physical row through the counts' prefix, so the summation order is that
// of M contiguous pillars.  The counts come from the host (fd_pillar_train_forward: one segment of m rows) or from device memory
// (fd_pillar_train_forward_dev: launched for the capacity; blocks behind the last live one leave at once, rows behind a count are
// never read, their `out` rows are written as 0, and a batch of N < 2 rows gives zeros everywhere).
#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxP = 32;          // point slots per pillar (shipped pp configs: 20)
constexpr int kFin = 16;           // decorated columns (ndim + 5 [+1]), zero padded
constexpr int kU1 = 32, kU2 = 64;  // the shipped stack
constexpr int kWaves = 4;
constexpr int kMaxBlocks = 1024;   // blocks (= partials) at most: with the pillars per block, part of the summation order
constexpr int kSlices = 16;        // fixed slices of the block reduction
constexpr int kPartStride = kU1 + kU1 + kU1 * kFin + kU2 * kU2;  // floats per block partial (the largest: the backward's)

// fp64 workspace slots
constexpr int D_SUM1 = 0, D_CM1 = D_SUM1 + kFin, D_SUM2 = D_CM1 + kFin * kFin, D_CM2 = D_SUM2 + kU2, D_WC1 = D_CM2 + kU2 * kU2,
              D_WC2 = D_WC1 + kU1 * kFin, D_BS = D_WC2 + kU2 * kU2, D_BR = D_BS + 2 * kU2, D_END = D_BR + kPartStride;
// fp32 workspace slots
constexpr int F_MU1 = 0, F_IS1 = F_MU1 + kU1, F_MU2 = F_IS1 + kU1, F_IS2 = F_MU2 + kU2, F_A = F_IS2 + kU2, F_C0 = F_A + kU2 * kU2,
              F_K2 = F_C0 + kU2, F_END = F_K2 + kU2;

__host__ __device__ inline int pillars_per_block(long long m) {
    long long ppb = (m + kMaxBlocks - 1) / kMaxBlocks;
    if (ppb < 16) ppb = 16;
    return (int)((ppb + kWaves - 1) / kWaves * kWaves);
}

constexpr int kMaxSegs = 16;

// Where the pillars are.  counts == nullptr: one segment of host_m rows (the host-count entries).
struct Segs {
    const int *counts;  // device int32[n_seg], or nullptr
    long long stride;   // rows per segment
    long long host_m;
    int n_seg;
};

struct Batch {
    long long m;  // live pillars
    int ppb, nb;  // pillars per block, live blocks (0 for the empty batch, N < 2)
};

__device__ __forceinline__ long long seg_count(const Segs &s, int b) {
    if (!s.counts) return s.host_m;
    const long long c = s.counts[b];
    return c < 0 ? 0 : (c > s.stride ? s.stride : c);
}

__device__ __forceinline__ Batch resolve(const Segs &s, int P) {
    Batch B;
    B.m = 0;
    for (int b = 0; b < s.n_seg; ++b) B.m += seg_count(s, b);
    B.ppb = pillars_per_block(B.m);
    B.nb = B.m * P > 1 ? (int)((B.m + B.ppb - 1) / B.ppb) : 0;
    return B;
}

// physical row of logical pillar p < M
__device__ __forceinline__ long long phys_row(const Segs &s, long long p) {
    int b = 0;
    for (; b < s.n_seg - 1; ++b) {
        const long long c = seg_count(s, b);
        if (p < c) break;
        p -= c;
    }
    return (long long)b * s.stride + p;
}

struct Layout {
    int grid;  // blocks launched: the largest number of live blocks any count <= cap can give
    size_t part, arg2, xsel, d64, f32, total;
};

// cap = rows of the buffers (m of the host-count entries, n_seg * seg_stride of the device-count ones)
Layout layout(int64_t m) {
    Layout L;
    const int64_t g = (m + 15) / 16;  // ppb >= 16
    L.grid = (int)(g < kMaxBlocks ? (g < 1 ? 1 : g) : kMaxBlocks);
    size_t o = 0;
    L.part = o; o += fd::align_up((size_t)L.grid * kPartStride * sizeof(float), 256);
    L.arg2 = o; o += fd::align_up((size_t)m * kU2, 256);
    L.xsel = o; o += fd::align_up((size_t)m * kU2 * sizeof(float), 256);
    L.d64 = o;  o += fd::align_up((size_t)D_END * sizeof(double), 256);
    L.f32 = o;  o += fd::align_up((size_t)F_END * sizeof(float), 256);
    L.total = o;
    return L;
}

struct TrainArgs {
    const float *voxels;
    const int *num_points;
    const int *coors;  // [M,4] (b,z,y,x)
    Segs seg;
    int P, ndim, fin, with_distance;
    float vx, vy, x_off, y_off;
    const float *w1, *g1, *b1, *w2, *g2, *b2;
    const float *st;  // fp32 workspace slots
    float *part;
};

struct WaveLds {
    float raw[kMaxP * 8];
    float mean[4];
    __attribute__((aligned(16))) float f[kMaxP][kFin];
    __attribute__((aligned(16))) float x[kMaxP][kU2];  // in2 rows: [a1 (32), max1 (32)]; rows >= P are 0
};

// Decorated, masked features of the pillar in physical row m into w.f (pillar_encoder.py:113-149; rows >= P and dead pillars are 0).  Block-uniform.
__device__ void decorate(const TrainArgs &a, long long m, bool live, WaveLds &w, int lane) {
    const int P = a.P, nd = a.ndim;
    if (live)
        for (int i = lane; i < P * nd; i += 64) w.raw[i] = a.voxels[m * P * nd + i];
    __syncthreads();
    const int cnt = live ? a.num_points[m] : 0;
    if (live && lane < 3) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += w.raw[p * nd + lane];
        w.mean[lane] = s / (float)cnt;
    }
    __syncthreads();
    const float cx = live ? (float)a.coors[m * 4 + 3] * a.vx + a.x_off : 0.f;
    const float cy = live ? (float)a.coors[m * 4 + 2] * a.vy + a.y_off : 0.f;
    for (int i = lane; i < kMaxP * kFin; i += 64) {
        const int p = i / kFin, c = i % kFin;
        float v = 0.f;
        if (live && p < cnt && p < P) {
            const float *r = &w.raw[p * nd];
            if (c < nd) v = r[c];
            else if (c < nd + 3) v = r[c - nd] - w.mean[c - nd];
            else if (c == nd + 3) v = r[0] - cx;
            else if (c == nd + 4) v = r[1] - cy;
            else if (c == nd + 5 && a.with_distance) v = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        }
        w.f[p][c] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ float dot_f(const float (&frow)[kFin], const float (&w1)[kFin]) {
    const float4 *f4 = reinterpret_cast<const float4 *>(frow);
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < kFin / 4; ++q) {
        const float4 f = f4[q];
        acc = fmaf(f.x, w1[4 * q], acc);
        acc = fmaf(f.y, w1[4 * q + 1], acc);
        acc = fmaf(f.z, w1[4 * q + 2], acc);
        acc = fmaf(f.w, w1[4 * q + 3], acc);
    }
    return acc;
}

// Layer 1 on batch statistics: lane = (row group g, unit u).  Writes w.x[p] = [a1[p], max1] for p < P (0 beyond) and returns the
// unit's max and its first arg-max row (both halves of the wave).  Block-uniform.
__device__ void layer1(const TrainArgs &a, bool live, WaveLds &w, const float (&w1)[kFin], float mu, float sc, float beta, int lane, float &mx,
                       int &arg) {
    const int u = lane & 31, g = lane >> 5;
    mx = -INFINITY;
    arg = 0;
    for (int p = g; p < kMaxP; p += 2) {
        float y = 0.f;
        if (live && p < a.P) {
            y = fmaxf(fmaf(dot_f(w.f[p], w1) - mu, sc, beta), 0.f);
            if (y > mx) { mx = y; arg = p; }
        }
        w.x[p][u] = y;
    }
    const float om = __shfl_xor(mx, 32);
    const int oa = __shfl_xor(arg, 32);
    if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
    for (int p = g; p < kMaxP; p += 2) w.x[p][kU1 + u] = (live && p < a.P) ? mx : 0.f;
    __syncthreads();
}

struct Layer1Params {
    float w1[kFin];
    float mu, sc, beta, is;
};

__device__ __forceinline__ void load_layer1(const TrainArgs &a, int u, Layer1Params &l) {
#pragma unroll
    for (int c = 0; c < kFin; ++c) l.w1[c] = c < a.fin ? a.w1[u * a.fin + c] : 0.f;
    l.mu = a.st[F_MU1 + u];
    l.is = a.st[F_IS1 + u];
    l.sc = a.g1[u] * l.is;
    l.beta = a.b1[u];
}

// ---- statistics passes: LAYER 1 = the decorated features (D = 16), LAYER 2 = layer 2's input rows (D = 64).
// Block partial: [n_b, mean_b[D], M2_b[D][D]] (M2 = sum over the block's rows of (x - mean_b)(x - mean_b)^T).
template <int LAYER>
__global__ void __launch_bounds__(kWaves * 64) stats_pass(TrainArgs a) {
    constexpr int D = LAYER == 1 ? kFin : kU2, NT = D / 16;
    __shared__ WaveLds s_w[kWaves];
    __shared__ float s_sum[kWaves][D];
    __shared__ float s_mean[D];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Batch B = resolve(a.seg, a.P);
    if ((int)blockIdx.x >= B.nb) return;  // block-uniform, before any barrier
    const long long p0 = (long long)blockIdx.x * B.ppb, p1 = min(p0 + B.ppb, B.m);
    WaveLds &w = s_w[wave];
    Layer1Params l1;
    if (LAYER == 2) load_layer1(a, lane & 31, l1);
    const int iters = B.ppb / kWaves;
    float colsum = 0.f;  // lane c < D: the wave's column sum
    for (int pass = 0; pass < 2; ++pass) {
        f32x4 acc[NT][NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int it = 0; it < iters; ++it) {
            const long long lp = p0 + wave + (long long)kWaves * it;
            const bool live = lp < p1;
            decorate(a, live ? phys_row(a.seg, lp) : 0, live, w, lane);
            if (LAYER == 2) {
                float mx;
                int arg;
                layer1(a, live, w, l1.w1, l1.mu, l1.sc, l1.beta, lane, mx, arg);
            }
            const float *rows = LAYER == 1 ? &w.f[0][0] : &w.x[0][0];
            if (pass == 0) {
                if (live && lane < D)
                    for (int p = 0; p < a.P; ++p) colsum += rows[p * D + lane];
            } else if (live) {
                const int lr = lane & 15, lq = lane >> 4;
                for (int k0 = 0; k0 < a.P; k0 += 4) {
                    const int p = k0 + lq;
                    float v[NT];
#pragma unroll
                    for (int i = 0; i < NT; ++i) v[i] = p < a.P ? rows[p * D + 16 * i + lr] - s_mean[16 * i + lr] : 0.f;
#pragma unroll
                    for (int i = 0; i < NT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[i], v[j], acc[i][j], 0, 0, 0);
                }
            }
            __syncthreads();
        }
        const float n_b = (float)((p1 - p0) * a.P);
        if (pass == 0) {
            if (lane < D) s_sum[wave][lane] = colsum;
            __syncthreads();
            if (threadIdx.x < D) {
                float s = 0.f;
                for (int q = 0; q < kWaves; ++q) s += s_sum[q][threadIdx.x];
                s_mean[threadIdx.x] = s / n_b;
            }
            __syncthreads();
            continue;
        }
        // waves 1..3 hand their tiles to wave 0 in wave order (the rows of s_w are free now)
        float *scratch = &s_w[0].x[0][0];
        static_assert(D * D <= kWaves * kMaxP * kU2, "scratch");
        for (int q = 1; q < kWaves; ++q) {
            if (wave == q)
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) scratch[((i * NT + j) * 4 + r) * 64 + lane] = acc[i][j][r];
            __syncthreads();
            if (wave == 0)
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[i][j][r] += scratch[((i * NT + j) * 4 + r) * 64 + lane];
            __syncthreads();
        }
        if (wave == 0) {
            float *dst = a.part + (size_t)blockIdx.x * kPartStride;
            if (lane == 0) dst[0] = n_b;
            if (lane < D) dst[1 + lane] = s_mean[lane];
            const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[1 + D + (16 * i + 4 * lq + r) * D + 16 * j + lr] = acc[i][j][r];
        }
    }
}

// out[e] = sum over the blocks' partials, in double precision: slice s of 16 sums blocks [s * per, (s + 1) * per) in order, the
// slices are added in slice order.  mode 0: part[off + e];  1: n_b * mean_b[e];  2: M2_b[e] + n_b (mean_b[i] - mu_i)(mean_b[j] - mu_j),
// e = i * D + j, mu = msum / n_tot (Chan).
__global__ void __launch_bounds__(256) reduce_parts(const float *__restrict__ part, Segs seg, int P, int off, int cnt, int mode, int D,
                                                    const double *__restrict__ msum, double *__restrict__ out) {
    __shared__ double s_acc[256];
    const Batch B = resolve(seg, P);
    const int nb = B.nb;  // (0 for the empty batch: every sum is 0)
    const double n_tot = (double)B.m * P;
    const int el = threadIdx.x & 15, s = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el;
    const int per = (nb + kSlices - 1) / kSlices;
    double acc = 0.0;
    if (e < cnt) {
        int i = 0, j = 0;
        double mi = 0.0, mj = 0.0;
        if (mode == 2) {
            i = e / D;
            j = e - i * D;
            mi = msum[i] / n_tot;
            mj = msum[j] / n_tot;
        }
        const int b1 = min(nb, (s + 1) * per);
        for (int b = s * per; b < b1; ++b) {
            const float *q = part + (size_t)b * kPartStride;
            double v;
            if (mode == 0) v = q[off + e];
            else if (mode == 1) v = (double)q[0] * (double)q[1 + e];
            else v = (double)q[1 + D + e] + (double)q[0] * ((double)q[1 + i] - mi) * ((double)q[1 + j] - mj);
            acc += v;
        }
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (s == 0 && e < cnt) {
        double t = 0.0;
        for (int q = 0; q < kSlices; ++q) t += s_acc[q * 16 + el];
        out[e] = t;
    }
}

// Batch statistics of a layer from its input statistics: mean = W mean_in, var = diag(W C W^T) / N; WC = W C kept for the backward.
template <int U, int D>
__global__ void __launch_bounds__(256) finish_stats(const float *__restrict__ wt, int win, const double *__restrict__ sum, const double *__restrict__ cm,
                                                    Segs seg, int P, float eps, double *__restrict__ wc, float *__restrict__ mean_out,
                                                    float *__restrict__ var_out, float *__restrict__ mu_ws, float *__restrict__ is_ws) {
    const Batch B = resolve(seg, P);
    const double n_tot = (double)B.m * P;
    if (B.nb == 0) {  // the empty batch: no statistics
        for (int t = threadIdx.x; t < U * D; t += 256) wc[t] = 0.0;
        if (threadIdx.x < U) mean_out[threadIdx.x] = var_out[threadIdx.x] = mu_ws[threadIdx.x] = is_ws[threadIdx.x] = 0.f;
        return;
    }
    for (int t = threadIdx.x; t < U * D; t += 256) {
        const int u = t / D, c = t - u * D;
        double s = 0.0;
        for (int k = 0; k < win; ++k) s += (double)wt[u * win + k] * cm[k * D + c];
        wc[t] = s;
    }
    __syncthreads();
    if (threadIdx.x < U) {
        const int u = threadIdx.x;
        double mu = 0.0, var = 0.0;
        for (int c = 0; c < win; ++c) {
            mu += (double)wt[u * win + c] * (sum[c] / n_tot);
            var += wc[u * D + c] * (double)wt[u * win + c];
        }
        var = var > 0.0 ? var / n_tot : 0.0;
        mean_out[u] = (float)mu;
        var_out[u] = (float)var;
        mu_ws[u] = (float)mu;
        is_ws[u] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// ---- forward output: lane = layer-2 unit v.  out = max_p relu(BN2(z2)); arg2 byte = first arg-max row | 0x80 when out > 0;
// xsel = x^2 at that row (dgamma2 of the backward).
__global__ void __launch_bounds__(kWaves * 64) output_pass(TrainArgs a, float *__restrict__ out, unsigned char *__restrict__ arg2,
                                                            float *__restrict__ xsel) {
    __shared__ WaveLds s_w[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Batch B = resolve(a.seg, a.P);
    if (a.seg.counts) {  // device counts: the rows behind a count (every row of the empty batch) are 0
        const long long cells = (long long)a.seg.n_seg * a.seg.stride * kU2;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (long long)gridDim.x * blockDim.x) {
            const long long row = i / kU2;
            const int b = (int)(row / a.seg.stride);
            if (B.nb == 0 || row - (long long)b * a.seg.stride >= seg_count(a.seg, b)) out[i] = 0.f;
        }
    }
    if ((int)blockIdx.x >= B.nb) return;  // block-uniform, before any barrier
    const long long p0 = (long long)blockIdx.x * B.ppb, p1 = min(p0 + B.ppb, B.m);
    WaveLds &w = s_w[wave];
    Layer1Params l1;
    load_layer1(a, lane & 31, l1);
    float w2[2 * kU1];
#pragma unroll
    for (int c = 0; c < 2 * kU1; ++c) w2[c] = a.w2[lane * 2 * kU1 + c];
    const float mu2 = a.st[F_MU2 + lane], is2 = a.st[F_IS2 + lane], sc2 = a.g2[lane] * is2, b2 = a.b2[lane];
    const int iters = B.ppb / kWaves;
    for (int it = 0; it < iters; ++it) {
        const long long lp = p0 + wave + (long long)kWaves * it;
        const bool live = lp < p1;
        const long long m = live ? phys_row(a.seg, lp) : 0;
        decorate(a, m, live, w, lane);
        float mx1;
        int arg1;
        layer1(a, live, w, l1.w1, l1.mu, l1.sc, l1.beta, lane, mx1, arg1);
        if (live) {
            float base = 0.f;
            {
                const float4 *m4 = reinterpret_cast<const float4 *>(&w.x[0][kU1]);
#pragma unroll
                for (int q = 0; q < kU1 / 4; ++q) {
                    const float4 f = m4[q];
                    base = fmaf(f.x, w2[kU1 + 4 * q], base);
                    base = fmaf(f.y, w2[kU1 + 4 * q + 1], base);
                    base = fmaf(f.z, w2[kU1 + 4 * q + 2], base);
                    base = fmaf(f.w, w2[kU1 + 4 * q + 3], base);
                }
            }
            float mx = -INFINITY, zsel = 0.f;
            int arg = 0;
            for (int p = 0; p < a.P; ++p) {
                const float4 *x4 = reinterpret_cast<const float4 *>(&w.x[p][0]);
                float acc = base;
#pragma unroll
                for (int q = 0; q < kU1 / 4; ++q) {
                    const float4 f = x4[q];
                    acc = fmaf(f.x, w2[4 * q], acc);
                    acc = fmaf(f.y, w2[4 * q + 1], acc);
                    acc = fmaf(f.z, w2[4 * q + 2], acc);
                    acc = fmaf(f.w, w2[4 * q + 3], acc);
                }
                const float y = fmaxf(fmaf(acc - mu2, sc2, b2), 0.f);
                if (y > mx) { mx = y; arg = p; zsel = acc; }
            }
            out[m * kU2 + lane] = mx;
            arg2[m * kU2 + lane] = (unsigned char)(arg | (mx > 0.f ? 0x80 : 0));
            xsel[m * kU2 + lane] = (zsel - mu2) * is2;
        }
        __syncthreads();
    }
}

// ---- backward 1: per-block sums of g2 = dout where the output is > 0, and of g2 x^2(arg row).  Partial [dbeta2[64], dgamma2[64]].
__global__ void __launch_bounds__(kWaves * 64) sparse_pass(Segs seg, int P, const float *__restrict__ dout,
                                                            const unsigned char *__restrict__ arg2, const float *__restrict__ xsel,
                                                            float *__restrict__ part) {
    __shared__ float s_red[kWaves][2 * kU2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Batch B = resolve(seg, P);
    if ((int)blockIdx.x >= B.nb) return;  // block-uniform, before any barrier
    const long long p0 = (long long)blockIdx.x * B.ppb, p1 = min(p0 + B.ppb, B.m);
    float sb = 0.f, sg = 0.f;
    for (long long lp = p0 + wave; lp < p1; lp += kWaves) {
        const long long m = phys_row(seg, lp);
        if (arg2[m * kU2 + lane] & 0x80) {
            const float g = dout[m * kU2 + lane];
            sb += g;
            sg += g * xsel[m * kU2 + lane];
        }
    }
    s_red[wave][lane] = sb;
    s_red[wave][kU2 + lane] = sg;
    __syncthreads();
    if (threadIdx.x < 2 * kU2) {
        float s = 0.f;
        for (int q = 0; q < kWaves; ++q) s += s_red[q][threadIdx.x];
        part[(size_t)blockIdx.x * kPartStride + threadIdx.x] = s;
    }
}

// dbeta2 / dgamma2 out; the dense BN-backward terms of layer 2 as A (64 x 64), c0 (64) and k2 = gamma2 invstd2.
__global__ void __launch_bounds__(256) finish_sparse(const float *__restrict__ w2, const float *__restrict__ g2, const double *__restrict__ bs,
                                                     Segs seg, int P, float *__restrict__ st, float *__restrict__ dgamma2, float *__restrict__ dbeta2) {
    __shared__ double s_a[kU2], s_b[kU2];
    const Batch B = resolve(seg, P);
    const double n_tot = (double)B.m * P;
    if (B.nb == 0) {  // the empty batch: no gradient (the rows pass has no live block and reads none of st)
        if (threadIdx.x < kU2) dbeta2[threadIdx.x] = dgamma2[threadIdx.x] = 0.f;
        return;
    }
    if (threadIdx.x < kU2) {
        const int v = threadIdx.x;
        const double is2 = st[F_IS2 + v], mu2 = st[F_MU2 + v];
        const double k = (double)g2[v] * is2, db = bs[v], dg = bs[kU2 + v];
        s_a[v] = k * (dg * is2 * mu2 - db) / n_tot;
        s_b[v] = k * dg * is2 / n_tot;
        st[F_K2 + v] = (float)k;
        dbeta2[v] = (float)db;
        dgamma2[v] = (float)dg;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kU2 * kU2; t += 256) {
        const int c = t / kU2, k = t - c * kU2;
        double s = 0.0;
        for (int v = 0; v < kU2; ++v) s += (double)w2[v * kU2 + c] * s_b[v] * (double)w2[v * kU2 + k];
        st[F_A + t] = (float)-s;
    }
    if (threadIdx.x < kU2) {
        const int c = threadIdx.x;
        double s = 0.0;
        for (int v = 0; v < kU2; ++v) s += (double)w2[v * kU2 + c] * s_a[v];
        st[F_C0 + c] = (float)s;
    }
}

// ---- backward 2: one pass over the rows.  Partial [sum dy1 (32), sum dy1 x^1 (32), sum dy1 f^T (32 x 16), SP (64 x 64)].
__global__ void __launch_bounds__(kWaves * 64) rows_pass(TrainArgs a, const float *__restrict__ dout, const unsigned char *__restrict__ arg2) {
    __shared__ WaveLds s_w[kWaves];
    __shared__ float s_da[kWaves][kMaxP][kU1];
    __shared__ float s_g[kWaves][kU2], s_kg[kWaves][kU2], s_cs[kWaves][kU1], s_dm[kWaves][kU1];
    __shared__ int s_arg[kWaves][kU2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = lane & 31, g = lane >> 5;
    const Batch B = resolve(a.seg, a.P);
    if ((int)blockIdx.x >= B.nb) return;  // block-uniform, before any barrier
    const long long p0 = (long long)blockIdx.x * B.ppb, p1 = min(p0 + B.ppb, B.m);
    WaveLds &w = s_w[wave];
    const float *A = a.st + F_A;
    const float *c0 = a.st + F_C0;
    const float *k2 = a.st + F_K2;
    Layer1Params l1;
    load_layer1(a, u, l1);
    float a11[kU1];
#pragma unroll
    for (int k = 0; k < kU1; ++k) a11[k] = A[u * kU2 + k];
    float E[kFin], sp[kU2];
#pragma unroll
    for (int c = 0; c < kFin; ++c) E[c] = 0.f;
#pragma unroll
    for (int v = 0; v < kU2; ++v) sp[v] = 0.f;
    float sdy = 0.f, sdyx = 0.f;
    const int P = a.P;
    const int iters = B.ppb / kWaves;
    for (int it = 0; it < iters; ++it) {
        const long long lp = p0 + wave + (long long)kWaves * it;
        const bool live = lp < p1;
        const long long m = live ? phys_row(a.seg, lp) : 0;
        decorate(a, m, live, w, lane);
        float mx1;
        int arg1;
        layer1(a, live, w, l1.w1, l1.mu, l1.sc, l1.beta, lane, mx1, arg1);
        if (live) {
            const int ab = arg2[m * kU2 + lane];
            const float gv = (ab & 0x80) ? dout[m * kU2 + lane] : 0.f;
            s_g[wave][lane] = gv;
            s_kg[wave][lane] = k2[lane] * gv;
            s_arg[wave][lane] = ab & 31;
            if (lane < kU1) {
                float cs = 0.f;
                for (int p = 0; p < P; ++p) cs += w.x[p][lane];
                s_cs[wave][lane] = cs;
            }
        }
        __syncthreads();
        if (live) {
            if (g == 0) {
                // d a1 rows: the per-pillar constant c0 + A12 max1, plus the sparse rows k g2 W2 at the arg-max rows (v in order)
                float h = c0[u];
                for (int k = 0; k < kU1; ++k) h = fmaf(A[u * kU2 + kU1 + k], w.x[0][kU1 + k], h);
                for (int p = 0; p < P; ++p) s_da[wave][p][u] = h;
                float smax = 0.f;
                for (int v = 0; v < kU2; ++v) {
                    const float kg = s_kg[wave][v];
                    s_da[wave][s_arg[wave][v]][u] += kg * a.w2[v * kU2 + u];
                    smax = fmaf(kg, a.w2[v * kU2 + kU1 + u], smax);
                }
                // d max1 = sum over the P rows of the max1 half of d in2
                float t1 = 0.f, t2 = 0.f;
                for (int k = 0; k < kU1; ++k) {
                    t1 = fmaf(A[(kU1 + u) * kU2 + k], s_cs[wave][k], t1);
                    t2 = fmaf(A[(kU1 + u) * kU2 + kU1 + k], w.x[0][kU1 + k], t2);
                }
                s_dm[wave][u] = (float)P * c0[kU1 + u] + t1 + (float)P * t2 + smax;
            }
            // SP[v][c] += g2[v] in2[arg2[v]][c]  (lane = c)
#pragma unroll
            for (int v = 0; v < kU2; ++v) sp[v] = fmaf(s_g[wave][v], w.x[s_arg[wave][v]][lane], sp[v]);
        }
        __syncthreads();
        if (live) {
            for (int p = g; p < P; p += 2) {
                const float z = dot_f(w.f[p], l1.w1);
                const float y = fmaf(z - l1.mu, l1.sc, l1.beta);
                float d = s_da[wave][p][u];
                const float4 *x4 = reinterpret_cast<const float4 *>(&w.x[p][0]);
#pragma unroll
                for (int q = 0; q < kU1 / 4; ++q) {
                    const float4 f = x4[q];
                    d = fmaf(a11[4 * q], f.x, d);
                    d = fmaf(a11[4 * q + 1], f.y, d);
                    d = fmaf(a11[4 * q + 2], f.z, d);
                    d = fmaf(a11[4 * q + 3], f.w, d);
                }
                if (p == arg1) d += s_dm[wave][u];
                const float dy = y > 0.f ? d : 0.f;
                sdy += dy;
                sdyx = fmaf(dy, (z - l1.mu) * l1.is, sdyx);
#pragma unroll
                for (int c = 0; c < kFin; ++c) E[c] = fmaf(dy, w.f[p][c], E[c]);
            }
        }
        __syncthreads();
    }
    // the two row groups of a wave, then the waves in order
    sdy += __shfl_xor(sdy, 32);
    sdyx += __shfl_xor(sdyx, 32);
#pragma unroll
    for (int c = 0; c < kFin; ++c) E[c] += __shfl_xor(E[c], 32);
    float *scratch = &s_w[0].x[0][0];
    constexpr int kSpOff = 2 * kU1 + kU1 * kFin;
    static_assert(kPartStride <= kWaves * kMaxP * kU2, "scratch");
    for (int q = 1; q < kWaves; ++q) {
        if (wave == q) {
            if (lane < kU1) {
                scratch[lane] = sdy;
                scratch[kU1 + lane] = sdyx;
#pragma unroll
                for (int c = 0; c < kFin; ++c) scratch[2 * kU1 + lane * kFin + c] = E[c];
            }
#pragma unroll
            for (int v = 0; v < kU2; ++v) scratch[kSpOff + v * kU2 + lane] = sp[v];
        }
        __syncthreads();
        if (wave == 0) {
            if (lane < kU1) {
                sdy += scratch[lane];
                sdyx += scratch[kU1 + lane];
#pragma unroll
                for (int c = 0; c < kFin; ++c) E[c] += scratch[2 * kU1 + lane * kFin + c];
            }
#pragma unroll
            for (int v = 0; v < kU2; ++v) sp[v] += scratch[kSpOff + v * kU2 + lane];
        }
        __syncthreads();
    }
    if (wave == 0) {
        float *dst = a.part + (size_t)blockIdx.x * kPartStride;
        if (lane < kU1) {
            dst[lane] = sdy;
            dst[kU1 + lane] = sdyx;
#pragma unroll
            for (int c = 0; c < kFin; ++c) dst[2 * kU1 + lane * kFin + c] = E[c];
        }
#pragma unroll
        for (int v = 0; v < kU2; ++v) dst[kSpOff + v * kU2 + lane] = sp[v];
    }
}

// dbeta1, dgamma1, dW1 [32, fin], dW2 [64, 64] from the reduced row-pass sums and the forward's statistics.
__global__ void __launch_bounds__(256) finish_rows(const float *__restrict__ g1, const float *__restrict__ g2, int fin, const double *__restrict__ d64,
                                                   const float *__restrict__ st, Segs seg, int P, float *__restrict__ dw1, float *__restrict__ dgamma1,
                                                   float *__restrict__ dbeta1, float *__restrict__ dw2) {
    const Batch B = resolve(seg, P);
    const double n_tot = (double)B.m * P;
    if (B.nb == 0) {  // the empty batch: no gradient
        if (threadIdx.x < kU1) dbeta1[threadIdx.x] = dgamma1[threadIdx.x] = 0.f;
        for (int t = threadIdx.x; t < kU1 * fin; t += 256) dw1[t] = 0.f;
        for (int t = threadIdx.x; t < kU2 * kU2; t += 256) dw2[t] = 0.f;
        return;
    }
    const double *br = d64 + D_BR;
    const double *bs = d64 + D_BS;
    constexpr int kSpOff = 2 * kU1 + kU1 * kFin;
    if (threadIdx.x < kU1) {
        dbeta1[threadIdx.x] = (float)br[threadIdx.x];
        dgamma1[threadIdx.x] = (float)br[kU1 + threadIdx.x];
    }
    for (int t = threadIdx.x; t < kU1 * fin; t += 256) {
        const int u = t / fin, c = t - u * fin;
        const double is1 = st[F_IS1 + u], k1 = (double)g1[u] * is1;
        const double db = br[u], dg = br[kU1 + u];
        dw1[t] = (float)(k1 * (br[2 * kU1 + u * kFin + c] - db * (d64[D_SUM1 + c] / n_tot) - dg / n_tot * is1 * d64[D_WC1 + u * kFin + c]));
    }
    for (int t = threadIdx.x; t < kU2 * kU2; t += 256) {
        const int v = t / kU2, c = t - v * kU2;
        const double is2 = st[F_IS2 + v], k2 = (double)g2[v] * is2;
        const double db = bs[v], dg = bs[kU2 + v];
        dw2[t] = (float)(k2 * (br[kSpOff + t] - db * (d64[D_SUM2 + c] / n_tot) - dg / n_tot * is2 * d64[D_WC2 + t]));
    }
}

void reduce(const float *part, const Segs &seg, int P, int off, int cnt, int mode, int D, const double *msum, double *out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_parts, dim3((unsigned)((cnt + 15) / 16)), dim3(256), 0, st, part, seg, P, off, cnt, mode, D, msum, out);
}

// The running statistics of one BatchNorm1d by torch's rule, n = P * sum cnt_b read here: num_batches_tracked += 1,
// running_mean <- (1 - f) running_mean + f mean, running_var <- (1 - f) running_var + f var n / (n - 1), in double precision and
// rounded once.  n < 2 (the empty batch): nothing.
__global__ void __launch_bounds__(64) running_stats(Segs seg, int P, const float *__restrict__ mean, const float *__restrict__ var, int c,
                                                    double f, float *__restrict__ rmean, float *__restrict__ rvar, long long *__restrict__ nbt) {
    const Batch B = resolve(seg, P);
    if (B.nb == 0) return;
    const double n = (double)B.m * P, unbias = n / (n - 1.0);
    for (int u = threadIdx.x; u < c; u += 64) {
        rmean[u] = (float)((1.0 - f) * (double)rmean[u] + f * (double)mean[u]);
        rvar[u] = (float)((1.0 - f) * (double)rvar[u] + f * unbias * (double)var[u]);
    }
    if (nbt && threadIdx.x == 0) *nbt += 1;
}

}  // namespace

extern "C" size_t fd_pillar_train_workspace_bytes(int64_t m, int max_points) {
    if (m < 1 || m >= (1ll << 30) || max_points < 1 || max_points > kMaxP) return 0;
    return layout(m).total;
}

#define FD_PT_CHECK_COMMON(fn)                                                                                                           \
    FD_REQUIRE(voxels && num_points && coors4 && w1 && gamma1 && beta1 && w2 && gamma2 && beta2, fn ": null argument");                   \
    FD_REQUIRE(max_points >= 1 && max_points <= kMaxP, fn ": max_points must be in [1,%d] (got %d)", kMaxP, max_points);                  \
    FD_REQUIRE(ndim >= 3 && ndim <= 8 && ndim + 5 + (with_distance ? 1 : 0) <= kFin, fn ": ndim must be in [3,8] (got %d)", ndim);        \
    FD_REQUIRE(units1 == kU1 && units2 == kU2,                                                                                           \
               fn ": unsupported units %d -> %d: training supports the shipped stack, two PFN layers of 32 (+32 max) -> 64 units", units1, \
               units2)

#define FD_PT_CHECK(fn)                                                                                                                  \
    FD_PT_CHECK_COMMON(fn);                                                                                                              \
    FD_REQUIRE(m >= 0 && m < (1ll << 30), fn ": m out of range");                                                                         \
    FD_REQUIRE(m * max_points > 1, fn ": expected more than 1 value per channel (N = m * max_points = %lld)", (long long)(m * max_points)); \
    FD_REQUIRE(workspace && workspace_bytes >= fd_pillar_train_workspace_bytes(m, max_points), fn ": workspace too small (%zu < %zu bytes)",  \
               workspace_bytes, fd_pillar_train_workspace_bytes(m, max_points))

#define FD_PT_CHECK_DEV(fn)                                                                                                              \
    FD_PT_CHECK_COMMON(fn);                                                                                                              \
    FD_REQUIRE(seg_counts, fn ": null seg_counts");                                                                                      \
    FD_REQUIRE(n_seg >= 1 && n_seg <= kMaxSegs, fn ": n_seg must be in [1,%d] (got %d)", kMaxSegs, n_seg);                                \
    FD_REQUIRE(seg_stride >= 1 && seg_stride < (1ll << 30) / n_seg, fn ": seg_stride out of range");                                      \
    FD_REQUIRE(workspace && workspace_bytes >= fd_pillar_train_workspace_bytes((int64_t)n_seg * seg_stride, max_points),                  \
               fn ": workspace too small (%zu < %zu bytes)", workspace_bytes,                                                             \
               fd_pillar_train_workspace_bytes((int64_t)n_seg * seg_stride, max_points))

static TrainArgs make_args(const float *voxels, const int32_t *num_points, const int32_t *coors4, const Segs &seg, int max_points, int ndim,
                           int with_distance, float vx, float vy, float x_offset, float y_offset, const float *w1, const float *gamma1,
                           const float *beta1, const float *w2, const float *gamma2, const float *beta2, const Layout &L, char *ws) {
    TrainArgs a;
    a.voxels = voxels;
    a.num_points = num_points;
    a.coors = coors4;
    a.seg = seg;
    a.P = max_points;
    a.ndim = ndim;
    a.fin = ndim + 5 + (with_distance ? 1 : 0);
    a.with_distance = with_distance ? 1 : 0;
    a.vx = vx;
    a.vy = vy;
    a.x_off = x_offset;
    a.y_off = y_offset;
    a.w1 = w1;
    a.g1 = gamma1;
    a.b1 = beta1;
    a.w2 = w2;
    a.g2 = gamma2;
    a.b2 = beta2;
    a.st = (const float *)(ws + L.f32);
    a.part = (float *)(ws + L.part);
    return a;
}

static Segs host_segs(int64_t m) { return Segs{nullptr, (long long)m, (long long)m, 1}; }
static Segs dev_segs(const int32_t *counts, int n_seg, int64_t stride) { return Segs{counts, (long long)stride, 0, n_seg}; }
static int64_t seg_rows(const Segs &s) { return s.counts ? s.n_seg * s.stride : s.host_m; }

// the launches of the forward / backward, for host and device counts alike
static void launch_forward(const TrainArgs &a, const Layout &L, char *ws, float eps1, float eps2, float *out, float *mean1, float *var1,
                           float *mean2, float *var2, hipStream_t st) {
    double *d64 = (double *)(ws + L.d64);
    float *f32 = (float *)(ws + L.f32);
    const Segs &sg = a.seg;
    const int P = a.P;
    const dim3 grid((unsigned)L.grid), block(kWaves * 64);
    // layer 1: statistics of the decorated features
    hipLaunchKernelGGL(stats_pass<1>, grid, block, 0, st, a);
    reduce(a.part, sg, P, 0, kFin, 1, kFin, nullptr, d64 + D_SUM1, st);
    reduce(a.part, sg, P, 0, kFin * kFin, 2, kFin, d64 + D_SUM1, d64 + D_CM1, st);
    hipLaunchKernelGGL((finish_stats<kU1, kFin>), dim3(1), dim3(256), 0, st, a.w1, a.fin, d64 + D_SUM1, d64 + D_CM1, sg, P, eps1, d64 + D_WC1, mean1,
                       var1, f32 + F_MU1, f32 + F_IS1);
    // layer 2: statistics of its input rows [a1, max1]
    hipLaunchKernelGGL(stats_pass<2>, grid, block, 0, st, a);
    reduce(a.part, sg, P, 0, kU2, 1, kU2, nullptr, d64 + D_SUM2, st);
    reduce(a.part, sg, P, 0, kU2 * kU2, 2, kU2, d64 + D_SUM2, d64 + D_CM2, st);
    hipLaunchKernelGGL((finish_stats<kU2, kU2>), dim3(1), dim3(256), 0, st, a.w2, kU2, d64 + D_SUM2, d64 + D_CM2, sg, P, eps2, d64 + D_WC2, mean2,
                       var2, f32 + F_MU2, f32 + F_IS2);
    hipLaunchKernelGGL(output_pass, grid, block, 0, st, a, out, (unsigned char *)(ws + L.arg2), (float *)(ws + L.xsel));
}

static void launch_backward(const TrainArgs &a, const Layout &L, char *ws, const float *dout, float *dw1, float *dgamma1, float *dbeta1, float *dw2,
                            float *dgamma2, float *dbeta2, hipStream_t st) {
    double *d64 = (double *)(ws + L.d64);
    float *f32 = (float *)(ws + L.f32);
    const unsigned char *arg2 = (const unsigned char *)(ws + L.arg2);
    const Segs &sg = a.seg;
    const int P = a.P;
    const dim3 grid((unsigned)L.grid), block(kWaves * 64);
    hipLaunchKernelGGL(sparse_pass, grid, block, 0, st, sg, P, dout, arg2, (const float *)(ws + L.xsel), a.part);
    reduce(a.part, sg, P, 0, 2 * kU2, 0, 0, nullptr, d64 + D_BS, st);
    hipLaunchKernelGGL(finish_sparse, dim3(1), dim3(256), 0, st, a.w2, a.g2, d64 + D_BS, sg, P, f32, dgamma2, dbeta2);
    hipLaunchKernelGGL(rows_pass, grid, block, 0, st, a, dout, arg2);
    reduce(a.part, sg, P, 0, kPartStride, 0, 0, nullptr, d64 + D_BR, st);
    hipLaunchKernelGGL(finish_rows, dim3(1), dim3(256), 0, st, a.g1, a.g2, a.fin, d64, f32, sg, P, dw1, dgamma1, dbeta1, dw2);
}

extern "C" int fd_pillar_train_forward(const float *voxels, const int32_t *num_points, const int32_t *coors4, int64_t m, int max_points, int ndim,
                                       int with_distance, float vx, float vy, float x_offset, float y_offset, const float *w1, const float *gamma1,
                                       const float *beta1, int units1, float eps1, const float *w2, const float *gamma2, const float *beta2,
                                       int units2, float eps2, float *out, float *mean1, float *var1, float *mean2, float *var2, void *workspace,
                                       size_t workspace_bytes, fd_stream_t stream_) {
    FD_PT_CHECK("fd_pillar_train_forward");
    FD_REQUIRE(out && mean1 && var1 && mean2 && var2, "fd_pillar_train_forward: null output");
    FD_REQUIRE(eps1 > 0.f && eps2 > 0.f, "fd_pillar_train_forward: eps must be > 0");
    const Segs sg = host_segs(m);
    const Layout L = layout(seg_rows(sg));
    char *ws = (char *)workspace;
    const TrainArgs a = make_args(voxels, num_points, coors4, sg, max_points, ndim, with_distance, vx, vy, x_offset, y_offset, w1, gamma1, beta1, w2,
                                  gamma2, beta2, L, ws);
    launch_forward(a, L, ws, eps1, eps2, out, mean1, var1, mean2, var2, fd::as_stream(stream_));
    return fd::check_launch("fd_pillar_train_forward");
}

extern "C" int fd_pillar_train_backward(const float *voxels, const int32_t *num_points, const int32_t *coors4, int64_t m, int max_points, int ndim,
                                        int with_distance, float vx, float vy, float x_offset, float y_offset, const float *w1,
                                        const float *gamma1, const float *beta1, int units1, const float *w2, const float *gamma2,
                                        const float *beta2, int units2, const float *dout, float *dw1, float *dgamma1, float *dbeta1, float *dw2,
                                        float *dgamma2, float *dbeta2, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_PT_CHECK("fd_pillar_train_backward");
    FD_REQUIRE(dout, "fd_pillar_train_backward: null dout");
    FD_REQUIRE(dw1 && dgamma1 && dbeta1 && dw2 && dgamma2 && dbeta2, "fd_pillar_train_backward: null gradient output");
    const Segs sg = host_segs(m);
    const Layout L = layout(seg_rows(sg));
    char *ws = (char *)workspace;
    const TrainArgs a = make_args(voxels, num_points, coors4, sg, max_points, ndim, with_distance, vx, vy, x_offset, y_offset, w1, gamma1, beta1, w2,
                                  gamma2, beta2, L, ws);
    launch_backward(a, L, ws, dout, dw1, dgamma1, dbeta1, dw2, dgamma2, dbeta2, fd::as_stream(stream_));
    return fd::check_launch("fd_pillar_train_backward");
}

extern "C" int fd_pillar_train_forward_dev(const float *voxels, const int32_t *num_points, const int32_t *coors4, const int32_t *seg_counts,
                                           int n_seg, int64_t seg_stride, int max_points, int ndim, int with_distance, float vx, float vy,
                                           float x_offset, float y_offset, const float *w1, const float *gamma1, const float *beta1, int units1,
                                           float eps1, const float *w2, const float *gamma2, const float *beta2, int units2, float eps2, float *out,
                                           float *mean1, float *var1, float *mean2, float *var2, void *workspace, size_t workspace_bytes,
                                           fd_stream_t stream_) {
    FD_PT_CHECK_DEV("fd_pillar_train_forward_dev");
    FD_REQUIRE(out && mean1 && var1 && mean2 && var2, "fd_pillar_train_forward_dev: null output");
    FD_REQUIRE(eps1 > 0.f && eps2 > 0.f, "fd_pillar_train_forward_dev: eps must be > 0");
    const Segs sg = dev_segs(seg_counts, n_seg, seg_stride);
    const Layout L = layout(seg_rows(sg));
    char *ws = (char *)workspace;
    const TrainArgs a = make_args(voxels, num_points, coors4, sg, max_points, ndim, with_distance, vx, vy, x_offset, y_offset, w1, gamma1, beta1, w2,
                                  gamma2, beta2, L, ws);
    launch_forward(a, L, ws, eps1, eps2, out, mean1, var1, mean2, var2, fd::as_stream(stream_));
    return fd::check_launch("fd_pillar_train_forward_dev");
}

extern "C" int fd_pillar_train_backward_dev(const float *voxels, const int32_t *num_points, const int32_t *coors4, const int32_t *seg_counts,
                                            int n_seg, int64_t seg_stride, int max_points, int ndim, int with_distance, float vx, float vy,
                                            float x_offset, float y_offset, const float *w1, const float *gamma1, const float *beta1, int units1,
                                            const float *w2, const float *gamma2, const float *beta2, int units2, const float *dout, float *dw1,
                                            float *dgamma1, float *dbeta1, float *dw2, float *dgamma2, float *dbeta2, void *workspace,
                                            size_t workspace_bytes, fd_stream_t stream_) {
    FD_PT_CHECK_DEV("fd_pillar_train_backward_dev");
    FD_REQUIRE(dout, "fd_pillar_train_backward_dev: null dout");
    FD_REQUIRE(dw1 && dgamma1 && dbeta1 && dw2 && dgamma2 && dbeta2, "fd_pillar_train_backward_dev: null gradient output");
    const Segs sg = dev_segs(seg_counts, n_seg, seg_stride);
    const Layout L = layout(seg_rows(sg));
    char *ws = (char *)workspace;
    const TrainArgs a = make_args(voxels, num_points, coors4, sg, max_points, ndim, with_distance, vx, vy, x_offset, y_offset, w1, gamma1, beta1, w2,
                                  gamma2, beta2, L, ws);
    launch_backward(a, L, ws, dout, dw1, dgamma1, dbeta1, dw2, dgamma2, dbeta2, fd::as_stream(stream_));
    return fd::check_launch("fd_pillar_train_backward_dev");
}

extern "C" int fd_pillar_train_running_stats_dev(const float *mean, const float *var, int channels, double momentum, const int32_t *seg_counts,
                                                 int n_seg, int64_t seg_stride, int max_points, float *running_mean, float *running_var,
                                                 int64_t *num_batches_tracked, fd_stream_t stream_) {
    FD_REQUIRE(mean && var && seg_counts && running_mean && running_var, "fd_pillar_train_running_stats_dev: null argument");
    FD_REQUIRE(channels >= 1, "fd_pillar_train_running_stats_dev: channels must be >= 1 (got %d)", channels);
    FD_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "fd_pillar_train_running_stats_dev: momentum must be in [0,1]");
    FD_REQUIRE(n_seg >= 1 && n_seg <= kMaxSegs, "fd_pillar_train_running_stats_dev: n_seg must be in [1,%d] (got %d)", kMaxSegs, n_seg);
    FD_REQUIRE(seg_stride >= 1 && seg_stride < (1ll << 30) / n_seg, "fd_pillar_train_running_stats_dev: seg_stride out of range");
    FD_REQUIRE(max_points >= 1 && max_points <= kMaxP, "fd_pillar_train_running_stats_dev: max_points must be in [1,%d] (got %d)", kMaxP,
               max_points);
    hipLaunchKernelGGL(running_stats, dim3(1), dim3(64), 0, fd::as_stream(stream_), dev_segs(seg_counts, n_seg, seg_stride), max_points, mean, var,
                       channels, momentum, running_mean, running_var, (long long *)num_batches_tracked);
    return fd::check_launch("fd_pillar_train_running_stats_dev");
}
