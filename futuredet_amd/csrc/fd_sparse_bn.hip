// Training-mode BatchNorm1d over the rows of a sparse feature matrix x [n, C] (fp32 or bf16, row-major), fused with what follows it in
// SpMiddleResNetFHD (det3d/models/backbones/scn.py:37-176): y = act(gamma (x - mean) invstd + beta [+ residual]), and its backward.
//
// Statistics.  Rows are cut into chunks of kChunk (= FD_SPARSE_BN_CHUNK) rows: chunk b owns rows [b kChunk, min((b + 1) kChunk, n)).
// Consecutive chunks form at most kMaxGroups groups of G = ceil(chunks / kMaxGroups) chunks.  Pass 1, one workgroup per group: per
// chunk, the column means (summed relative to the chunk's first row, so a mean that is large against the spread costs no digits) and
// M2_b = sum (x - mean_b)^2 centred at that mean; the group's chunks are merged in chunk order, in double, with Chan's rule
// (mean += d n_b / N', M2 += M2_b + d^2 N n_b / N').  Pass 2: EVERY workgroup re-sums the (at most kMaxGroups) group partials itself,
// in double, in a fixed order -- mean = sum n_g mean_g / n, then M2 = sum [M2_g + n_g (mean_g - mean)^2]; the groups are cut into
// slices, a slice adds its groups in order, the slices are added in slice order -- and then applies the normalisation to its rows.
// Workgroup 0 also writes mean / invstd for the backward and updates the running statistics (unbiased variance) and
// num_batches_tracked.  Two launches, no atomics: chunk, group and slice boundaries depend on the valid row count and C only, so two
// runs give the same bits, and a call that reads the row count from the device gives the bits of the exact-size call.
//
// Backward.  g = dy where y > 0 (y is the forward's output: the ReLU mask), x^ = (x - mean) invstd.  Pass 1: sums of g and g x^ per
// chunk, added per group in chunk order in double; pass 2: every workgroup re-sums the group partials in the same fixed order,
// dx = gamma invstd (g - dbeta / n - x^ dgamma / n), d_residual = g.
//
// Thread layout of every pass: a row is C / 4 column quads; thread t takes quad t % (C / 4) of rows t / (C / 4), + 256 / (C / 4), ...
// (a wave reads whole rows).  Row lanes are added in lane order through LDS.
//
// Row type.  Every kernel is a template over the type T of the row tensors (x, residual, y, dy, dx, d_residual): float, a quad is one
// float4 (16 bytes), or bf16_t, a quad is one 8-byte group that ld4 widens exactly to fp32 and st4 rounds to nearest even.  Nothing else
// differs: the bf16 form computes what the fp32 form computes on the widened rows, and rounds once.  Parameters, statistics, saved and the
// workspace partials are fp32 either way.
#include "fd_common.h"

namespace {

constexpr int kChunk = FD_SPARSE_BN_CHUNK;
constexpr int kThreads = 256;
constexpr int kMaxC = 128;
constexpr int kRedFloats = 4 * kThreads;  // lanes * C <= 256 / (C / 4) * C
constexpr int kMaxRows = 1 << 30;
constexpr int kMaxGroups = 256;       // group partials at most: every apply workgroup re-sums them
constexpr int kMaxApplyBlocks = 512;  // apply workgroups at most
static_assert(kChunk % 64 == 0, "chunk");

inline bool channels_ok(int C) { return C >= 16 && C <= kMaxC && C % 16 == 0; }
inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int groups_cap(int64_t n) { return (int)(chunks_of(n) < kMaxGroups ? chunks_of(n) : kMaxGroups); }
// rows per apply workgroup: a function of the capacity only (the apply pass is element-wise: its cut does not touch the sums)
inline int apply_rows(int64_t n) { return (int)((chunks_of(n) + kMaxApplyBlocks - 1) / kMaxApplyBlocks) * kChunk; }

typedef uint16_t bf16_t;  // the bits of a bfloat16

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float ld1(const float *p) { return *p; }

// bf16 -> fp32 is exact: the 16 bits are the upper half of the fp32 pattern
__device__ __forceinline__ float4 ld4(const bf16_t *p) {
    const uint2 u = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float ld1(const bf16_t *p) { return __uint_as_float((unsigned)*p << 16); }
// round to nearest even as fd::bf16_rne (fd_spconv_pack.h) does, and a copy of its own because here a NaN stays a NaN instead of
// carrying into the sign
__device__ __forceinline__ unsigned to_bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void st4(bf16_t *p, float4 v) {
    uint2 u;
    u.x = to_bf16_rne(v.x) | (to_bf16_rne(v.y) << 16);
    u.y = to_bf16_rne(v.z) | (to_bf16_rne(v.w) << 16);
    *reinterpret_cast<uint2 *>(p) = u;
}

// The cut of nv valid rows: chunks, chunks per group, groups.  Device side: everything follows from the valid row count.
struct Cut {
    int nv, nbv, G, ng;
    __device__ __forceinline__ Cut(int n, const int *n_dev) {
        nv = fd::device_count(n, n_dev);
        nbv = (nv + kChunk - 1) / kChunk;
        G = (nbv + kMaxGroups - 1) / kMaxGroups;
        if (G < 1) G = 1;
        ng = (nbv + G - 1) / G;
    }
    __device__ __forceinline__ double rows_in_group(int g) const { return (double)min(G * kChunk, nv - g * G * kChunk); }
};

// Adds the row lanes of a float4 per thread in lane order: thread c < C returns column c's total.  s_red: kRedFloats floats.
__device__ __forceinline__ float lane_sum(float4 v, float *s_red, int rl, int q, int RL, int C) {
    __syncthreads();
    if (rl < RL) st4(&s_red[rl * C + 4 * q], v);
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < C)
        for (int l = 0; l < RL; ++l) t += s_red[l * C + threadIdx.x];
    return t;
}

// ---- forward pass 1: part[g] = [mean_g[C], M2_g[C]]
template <typename T>
__global__ void __launch_bounds__(kThreads) bn_stats(const T *__restrict__ x, int n, const int *__restrict__ n_dev, int C,
                                                      float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kMaxC];
    const Cut cut(n, n_dev);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nbv) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nbv);
    const int QC = C >> 2, RL = kThreads / QC;
    const int q = threadIdx.x % QC, rl = threadIdx.x / QC;
    const bool on = rl < RL;
    double N = 0.0, mean = 0.0, M2 = 0.0;  // threads < C: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, cut.nv);
        const float4 pivot = ld4(x + (int64_t)r0 * C + 4 * q);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
#pragma unroll 4
            for (int r = r0 + rl; r < r1; r += RL) {
                const float4 v = ld4(x + (int64_t)r * C + 4 * q);
                s.x += v.x - pivot.x;
                s.y += v.y - pivot.y;
                s.z += v.z - pivot.z;
                s.w += v.w - pivot.w;
            }
        }
        const float tot = lane_sum(s, red, rl, q, RL, C);
        const float nb = (float)(r1 - r0);
        float mb = 0.f;
        if (threadIdx.x < C) s_mean[threadIdx.x] = mb = ld1(x + (int64_t)r0 * C + threadIdx.x) + tot / nb;
        __syncthreads();
        const float4 m = ld4(&s_mean[4 * q]);
        s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) {
#pragma unroll 4
            for (int r = r0 + rl; r < r1; r += RL) {
                const float4 v = ld4(x + (int64_t)r * C + 4 * q);
                const float dx = v.x - m.x, dy = v.y - m.y, dz = v.z - m.z, dw = v.w - m.w;
                s.x += dx * dx;
                s.y += dy * dy;
                s.z += dz * dz;
                s.w += dw * dw;
            }
        }
        const float m2 = lane_sum(s, red, rl, q, RL, C);
        if (threadIdx.x < C) {  // Chan's rule, chunk b onto the group so far
            const double nbd = (double)nb, N1 = N + nbd, d = (double)mb - mean;
            mean += d * (nbd / N1);
            M2 += (double)m2 + d * d * (N * nbd / N1);
            N = N1;
        }
    }
    if (threadIdx.x < C) {
        float *dst = part + (size_t)blockIdx.x * 2 * C;
        dst[threadIdx.x] = (float)mean;
        dst[C + threadIdx.x] = (float)M2;
    }
}

struct D4 {
    double x, y, z, w;
};

// Slices of the group partials: thread (slice s = t / (C / 4), column quad q) owns groups [s per, (s + 1) per) of the ng.
struct Slices {
    int QC, S, q, s, g0, g1;
    __device__ __forceinline__ Slices(int C, int ng) {
        QC = C >> 2;
        S = kThreads / QC;
        q = threadIdx.x % QC;
        s = threadIdx.x / QC;
        const int per = (ng + S - 1) / S;
        g0 = min(ng, s * per);
        g1 = s < S ? min(ng, g0 + per) : g0;
    }
};

// Adds the slices in slice order: thread c < C returns column c's total.  s_acc: kRedFloats doubles.
__device__ __forceinline__ double slice_total(const D4 &a, double *s_acc, const Slices &sl, int C) {
    __syncthreads();
    if (sl.s < sl.S) {
        double *d = &s_acc[sl.s * C + 4 * sl.q];
        d[0] = a.x;
        d[1] = a.y;
        d[2] = a.z;
        d[3] = a.w;
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < C)
        for (int k = 0; k < sl.S; ++k) t += s_acc[k * C + threadIdx.x];
    return t;
}

// ---- forward pass 2: statistics from the group partials, then y for the workgroup's rows
template <typename T>
__global__ void __launch_bounds__(kThreads) bn_apply(const T *__restrict__ x, const T *__restrict__ residual,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta, int n,
                                                      const int *__restrict__ n_dev, int C, int relu, float eps, double momentum,
                                                      int rows_per_block, const float *__restrict__ part, T *__restrict__ y,
                                                      float *__restrict__ saved, float *__restrict__ running_mean,
                                                      float *__restrict__ running_var, long long *__restrict__ num_batches_tracked) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) double s_mu[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_mean[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_scale[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_beta[kMaxC];
    const Cut cut(n, n_dev);
    const int nv = cut.nv;
    const double cnt = (double)nv;
    const Slices sl(C, cut.ng);
    D4 a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 m = ld4(part + (size_t)g * 2 * C + 4 * sl.q);
        const double w = cut.rows_in_group(g);
        a.x += w * (double)m.x;
        a.y += w * (double)m.y;
        a.z += w * (double)m.z;
        a.w += w * (double)m.w;
    }
    double t = slice_total(a, s_acc, sl, C);
    if (threadIdx.x < C) s_mu[threadIdx.x] = nv > 0 ? t / cnt : 0.0;
    __syncthreads();
    const double mu0 = s_mu[4 * sl.q], mu1 = s_mu[4 * sl.q + 1], mu2 = s_mu[4 * sl.q + 2], mu3 = s_mu[4 * sl.q + 3];
    a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 m = ld4(part + (size_t)g * 2 * C + 4 * sl.q);
        const float4 v = ld4(part + (size_t)g * 2 * C + C + 4 * sl.q);
        const double w = cut.rows_in_group(g);
        const double d0 = (double)m.x - mu0, d1 = (double)m.y - mu1, d2 = (double)m.z - mu2, d3 = (double)m.w - mu3;
        a.x += (double)v.x + w * d0 * d0;
        a.y += (double)v.y + w * d1 * d1;
        a.z += (double)v.z + w * d2 * d2;
        a.w += (double)v.w + w * d3 * d3;
    }
    t = slice_total(a, s_acc, sl, C);
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        const double var = nv > 0 && t > 0.0 ? t / cnt : 0.0;
        const float mean_f = (float)s_mu[c];
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        s_mean[c] = mean_f;
        s_scale[c] = gamma[c] * invstd;
        s_beta[c] = beta[c];
        if (blockIdx.x == 0) {
            saved[c] = mean_f;
            saved[C + c] = invstd;
            if (nv > 0) {
                const double unbiased = var * (cnt / (nv > 1 ? cnt - 1.0 : 1.0));
                running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * s_mu[c]);
                running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
                if (c == 0) num_batches_tracked[0] += 1;
            }
        }
    }
    __syncthreads();
    const int QC = C >> 2, RL = kThreads / QC;
    const int q = threadIdx.x % QC, rl = threadIdx.x / QC;
    if (rl >= RL) return;
    const float4 m = ld4(&s_mean[4 * q]), sc = ld4(&s_scale[4 * q]), be = ld4(&s_beta[4 * q]);
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, n);
#pragma unroll 4
    for (int r = r0 + rl; r < r1; r += RL) {
        const int64_t o = (int64_t)r * C + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nv) {
            const float4 xv = ld4(x + o);
            v.x = (xv.x - m.x) * sc.x + be.x;
            v.y = (xv.y - m.y) * sc.y + be.y;
            v.z = (xv.z - m.z) * sc.z + be.z;
            v.w = (xv.w - m.w) * sc.w + be.w;
            if (residual) {
                const float4 rv = ld4(residual + o);
                v.x += rv.x;
                v.y += rv.y;
                v.z += rv.z;
                v.w += rv.w;
            }
            if (relu) {
                v.x = v.x > 0.f ? v.x : 0.f;
                v.y = v.y > 0.f ? v.y : 0.f;
                v.z = v.z > 0.f ? v.z : 0.f;
                v.w = v.w > 0.f ? v.w : 0.f;
            }
        }
        st4(y + o, v);
    }
}

template <typename T>
__device__ __forceinline__ float4 masked(const T *__restrict__ dy, const T *__restrict__ y, int relu, int64_t o) {
    float4 g = ld4(dy + o);
    if (relu) {
        const float4 yv = ld4(y + o);
        g.x = yv.x > 0.f ? g.x : 0.f;
        g.y = yv.y > 0.f ? g.y : 0.f;
        g.z = yv.z > 0.f ? g.z : 0.f;
        g.w = yv.w > 0.f ? g.w : 0.f;
    }
    return g;
}

// ---- backward pass 1: part[g] = [sum g [C], sum g x^ [C]]
template <typename T>
__global__ void __launch_bounds__(kThreads) bn_grad_sums(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ y,
                                                          const float *__restrict__ saved, int n, const int *__restrict__ n_dev, int C,
                                                          int relu, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    const Cut cut(n, n_dev);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nbv) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nbv);
    const int QC = C >> 2, RL = kThreads / QC;
    const int q = threadIdx.x % QC, rl = threadIdx.x / QC;
    const float4 m = ld4(saved + 4 * q), is = ld4(saved + C + 4 * q);
    double db = 0.0, dg = 0.0;  // threads < C: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, cut.nv);
        float4 sb = make_float4(0.f, 0.f, 0.f, 0.f), sg = sb;
        if (rl < RL) {
#pragma unroll 2
            for (int r = r0 + rl; r < r1; r += RL) {
                const int64_t o = (int64_t)r * C + 4 * q;
                const float4 g = masked(dy, y, relu, o);
                const float4 xv = ld4(x + o);
                sb.x += g.x;
                sb.y += g.y;
                sb.z += g.z;
                sb.w += g.w;
                sg.x += g.x * ((xv.x - m.x) * is.x);
                sg.y += g.y * ((xv.y - m.y) * is.y);
                sg.z += g.z * ((xv.z - m.z) * is.z);
                sg.w += g.w * ((xv.w - m.w) * is.w);
            }
        }
        db += (double)lane_sum(sb, red, rl, q, RL, C);
        dg += (double)lane_sum(sg, red, rl, q, RL, C);
    }
    if (threadIdx.x < C) {
        float *dst = part + (size_t)blockIdx.x * 2 * C;
        dst[threadIdx.x] = (float)db;
        dst[C + threadIdx.x] = (float)dg;
    }
}

// ---- backward pass 2: dbeta / dgamma from the group partials, then dx (and d_residual) for the workgroup's rows
template <typename T>
__global__ void __launch_bounds__(kThreads) bn_grad_apply(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ y,
                                                           const float *__restrict__ gamma, const float *__restrict__ saved, int n,
                                                           const int *__restrict__ n_dev, int C, int relu, int rows_per_block,
                                                           const float *__restrict__ part, T *__restrict__ dx, T *__restrict__ d_residual,
                                                           float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_is[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_k[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_mb[kMaxC];
    __shared__ __attribute__((aligned(16))) float s_mg[kMaxC];
    const Cut cut(n, n_dev);
    const int nv = cut.nv;
    const Slices sl(C, cut.ng);
    D4 ab = {0.0, 0.0, 0.0, 0.0}, ag = ab;
#pragma unroll 4
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 b = ld4(part + (size_t)g * 2 * C + 4 * sl.q);
        const float4 v = ld4(part + (size_t)g * 2 * C + C + 4 * sl.q);
        ab.x += (double)b.x;
        ab.y += (double)b.y;
        ab.z += (double)b.z;
        ab.w += (double)b.w;
        ag.x += (double)v.x;
        ag.y += (double)v.y;
        ag.z += (double)v.z;
        ag.w += (double)v.w;
    }
    const double db = slice_total(ab, s_acc, sl, C);
    const double dg = slice_total(ag, s_acc, sl, C);
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        const double cnt = nv > 0 ? (double)nv : 1.0;
        const float is = saved[C + c];
        s_mean[c] = saved[c];
        s_is[c] = is;
        s_k[c] = gamma[c] * is;
        s_mb[c] = (float)(db / cnt);
        s_mg[c] = (float)(dg / cnt);
        if (blockIdx.x == 0) {
            dbeta[c] = (float)db;
            dgamma[c] = (float)dg;
        }
    }
    __syncthreads();
    const int QC = C >> 2, RL = kThreads / QC;
    const int q = threadIdx.x % QC, rl = threadIdx.x / QC;
    if (rl >= RL) return;
    const float4 m = ld4(&s_mean[4 * q]), is = ld4(&s_is[4 * q]), k = ld4(&s_k[4 * q]), mb = ld4(&s_mb[4 * q]), mg = ld4(&s_mg[4 * q]);
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, n);
#pragma unroll 2
    for (int r = r0 + rl; r < r1; r += RL) {
        const int64_t o = (int64_t)r * C + 4 * q;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), d = g;
        if (r < nv) {
            g = masked(dy, y, relu, o);
            const float4 xv = ld4(x + o);
            d.x = k.x * (g.x - mb.x - (xv.x - m.x) * is.x * mg.x);
            d.y = k.y * (g.y - mb.y - (xv.y - m.y) * is.y * mg.y);
            d.z = k.z * (g.z - mb.z - (xv.z - m.z) * is.z * mg.z);
            d.w = k.w * (g.w - mb.w - (xv.w - m.w) * is.w * mg.w);
        }
        st4(dx + o, d);
        if (d_residual) st4(d_residual + o, g);
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int fd_sparse_bn_chunk(void) { return kChunk; }

extern "C" size_t fd_sparse_bn_workspace_bytes(int64_t n, int C) {
    if (n < 1 || n > kMaxRows || !channels_ok(C)) return 0;
    return fd::align_up((size_t)groups_cap(n) * 2 * C * sizeof(float), 256);
}

#define FD_SBN_CHECK(fn)                                                                                                               \
    FD_REQUIRE(channels_ok(C), fn ": unsupported C %d: a multiple of 16 in [16, %d]", C, kMaxC);                                        \
    FD_REQUIRE(n >= 1 && n <= kMaxRows, fn ": n out of range (%lld)", (long long)n);                                                   \
    FD_REQUIRE(n_dev || n >= 2, fn ": expected more than 1 value per channel (n = %lld)", (long long)n);                                \
    FD_REQUIRE(relu == 0 || relu == 1, fn ": relu must be 0 or 1 (got %d)", relu);                                                      \
    FD_REQUIRE(workspace, fn ": null workspace");                                                                                       \
    FD_REQUIRE(workspace_bytes >= fd_sparse_bn_workspace_bytes(n, C), fn ": workspace too small (%zu bytes, %zu needed)", workspace_bytes, \
               fd_sparse_bn_workspace_bytes(n, C));                                                                                     \
    FD_REQUIRE(aligned16(workspace), fn ": the workspace must be 16-byte aligned")

// The two entry points per row type share their bodies: fn is the name the messages carry, T the row type.
#define FD_SBN_FORWARD(fn, T)                                                                                                          \
    FD_REQUIRE(x && gamma && beta, fn ": null x, gamma or beta");                                                                      \
    FD_REQUIRE(y && saved, fn ": null y or saved");                                                                                    \
    FD_REQUIRE(running_mean && running_var && num_batches_tracked, fn ": null running statistics");                                    \
    FD_SBN_CHECK(fn);                                                                                                                  \
    FD_REQUIRE(eps > 0.f, fn ": eps must be > 0");                                                                                     \
    FD_REQUIRE(momentum >= 0.0 && momentum <= 1.0, fn ": momentum must be in [0, 1]");                                                 \
    FD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(saved) && (!residual || aligned16(residual)),                                 \
               fn ": x, residual, y and saved must be 16-byte aligned");                                                               \
    hipStream_t st = fd::as_stream(stream_);                                                                                           \
    const int rows = apply_rows(n);                                                                                                    \
    float *part = (float *)workspace;                                                                                                  \
    hipLaunchKernelGGL(bn_stats<T>, dim3((unsigned)groups_cap(n)), dim3(kThreads), 0, st, x, (int)n, n_dev, C, part);                  \
    hipLaunchKernelGGL(bn_apply<T>, dim3((unsigned)((n + rows - 1) / rows)), dim3(kThreads), 0, st, x, residual, gamma, beta, (int)n,  \
                       n_dev, C, relu, eps, momentum, rows, (const float *)part, y, saved, running_mean, running_var,                  \
                       (long long *)num_batches_tracked);                                                                              \
    return fd::check_launch(fn)

#define FD_SBN_BACKWARD(fn, T)                                                                                                         \
    FD_REQUIRE(dy && x && gamma && saved, fn ": null dy, x, gamma or saved");                                                          \
    FD_REQUIRE(y || !relu, fn ": null y (the ReLU mask)");                                                                             \
    FD_REQUIRE(dx && dgamma && dbeta, fn ": null dx, dgamma or dbeta");                                                                \
    FD_SBN_CHECK(fn);                                                                                                                  \
    FD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(saved) && aligned16(dx) && aligned16(d_residual),            \
               fn ": dy, x, y, saved, dx and d_residual must be 16-byte aligned");                                                     \
    hipStream_t st = fd::as_stream(stream_);                                                                                           \
    const int rows = apply_rows(n);                                                                                                    \
    float *part = (float *)workspace;                                                                                                  \
    hipLaunchKernelGGL(bn_grad_sums<T>, dim3((unsigned)groups_cap(n)), dim3(kThreads), 0, st, dy, x, y, saved, (int)n, n_dev, C, relu, \
                       part);                                                                                                          \
    hipLaunchKernelGGL(bn_grad_apply<T>, dim3((unsigned)((n + rows - 1) / rows)), dim3(kThreads), 0, st, dy, x, y, gamma, saved,       \
                       (int)n, n_dev, C, relu, rows, (const float *)part, dx, d_residual, dgamma, dbeta);                              \
    return fd::check_launch(fn)

extern "C" int fd_sparse_bn_train_forward(const float *x, const float *residual, const float *gamma, const float *beta, int64_t n,
                                          const int32_t *n_dev, int C, int relu, float eps, double momentum, float *y, float *saved,
                                          float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                                          size_t workspace_bytes, fd_stream_t stream_) {
    FD_SBN_FORWARD("fd_sparse_bn_train_forward", float);
}

extern "C" int fd_sparse_bn_train_forward_bf16(const uint16_t *x, const uint16_t *residual, const float *gamma, const float *beta, int64_t n,
                                               const int32_t *n_dev, int C, int relu, float eps, double momentum, uint16_t *y, float *saved,
                                               float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                                               size_t workspace_bytes, fd_stream_t stream_) {
    FD_SBN_FORWARD("fd_sparse_bn_train_forward_bf16", bf16_t);
}

extern "C" int fd_sparse_bn_train_backward(const float *dy, const float *x, const float *y, const float *gamma, const float *saved, int64_t n,
                                           const int32_t *n_dev, int C, int relu, float *dx, float *d_residual, float *dgamma, float *dbeta,
                                           void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_SBN_BACKWARD("fd_sparse_bn_train_backward", float);
}

extern "C" int fd_sparse_bn_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *gamma, const float *saved,
                                                int64_t n, const int32_t *n_dev, int C, int relu, uint16_t *dx, uint16_t *d_residual,
                                                float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_SBN_BACKWARD("fd_sparse_bn_train_backward_bf16", bf16_t);
}
