// Training-mode BatchNorm2d over a bf16 channels-last map of the dense half (RPN, CenterHead in mixed precision), fused with the ReLU
// that follows it: the map is rows x [n = B H W, C] (bf16, row-major), y = act(gamma (x - mean) invstd + beta), and its backward.  One
// call normalises the channel ranges of up to kMaxRecords BatchNorm2d modules (fd_dense_bn_nhwc_group records, passed by value): record j
// owns the next c_j channels, with its own parameters, eps, momentum, running statistics and counter -- the six or seven 64-channel
// branches of a SepHead are one call on their 384- or 448-channel map.
//
// Statistics: the design of fd_sparse_bn.hip.  Rows are cut into chunks of kChunk (= FD_DENSE_BN_NHWC_CHUNK) rows; consecutive chunks
// form at most kStatGroups groups of G = ceil(chunks / kStatGroups) chunks.  Pass 1, one workgroup per (group, channel block): per
// chunk, the column means (summed relative to the chunk's first row) and M2_b = sum (x - mean_b)^2 centred at that mean; the group's
// chunks are merged in chunk order, in double, with Chan's rule.  Pass 2: EVERY workgroup re-sums the group partials itself, in double,
// in one fixed order (slices of groups, a slice adds its groups in order, the slices are added in slice order), then normalises its rows.
// The workgroups of the first row block also write mean / invstd for the backward and update each record's running statistics (unbiased
// variance, the record's momentum) and counter.  Two launches per direction, no atomics; the cut depends on (n, C) only: two runs give
// the same bits.  Every workspace word that pass 2 reads was written by pass 1 of the same call.
//
// Backward.  g = dy where y > 0 (y is the forward's output: the ReLU mask), x^ = (x - mean) invstd.  Pass 1: sums of g and g x^ per
// chunk, added per group in chunk order in double; pass 2: every workgroup re-sums the partials in the same fixed order,
// dx = gamma invstd (g - dbeta / n - x^ dgamma / n).
//
// What differs from the sparse kernel.  C is any multiple of 32 in [32, 512]: a workgroup owns a channel block of at most kBlockC = 128
// channels (the last block of C = 160 has 32, C = 96 is one block of 96) and grid dimension y runs over the blocks, so the LDS reductions
// keep the sparse kernel's size and a 512-channel map has four times the workgroups of a 128-channel one.  Pass 1 of the forward holds a
// thread's share of the chunk in registers (at most kHold 8-byte groups): the chunk is read from memory once, all its loads are in flight
// together, and the second moment is taken from the registers.
//
// Thread layout of every pass: a block row is cb / 4 column quads; thread t takes quad t % (cb / 4) of rows t / (cb / 4),
// + 256 / (cb / 4), ...  Every access to a map is one 8-byte group per lane (four bf16), widened exactly to fp32 on load and rounded
// once to nearest even on store.  Parameters, statistics, saved, dgamma, dbeta and the workspace are fp32.
#include "fd_common.h"

namespace {

constexpr int kChunk = FD_DENSE_BN_NHWC_CHUNK;
constexpr int kThreads = 256;
constexpr int kBlockC = 128;  // channels of a workgroup at most
constexpr int kMaxC = 512;
constexpr int kMaxRecords = FD_DENSE_BN_NHWC_MAX_GROUPS;
constexpr int kRedFloats = 4 * kThreads;  // lanes * cb <= 256 / (cb / 4) * cb
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kStatGroups = FD_DENSE_BN_NHWC_STAT_GROUPS;    // group partials at most: every apply workgroup re-sums them
constexpr int kApplyBlocks = FD_DENSE_BN_NHWC_APPLY_BLOCKS;  // row blocks of the apply passes at most
constexpr int kHold = kChunk / (kThreads / (kBlockC / 4));   // rows of a chunk per thread at most (the widest block: 8 row lanes)
static_assert(kChunk % 64 == 0 && kHold <= 32, "chunk");
// Rows a thread has in flight in the element-wise loops.  Those loops run a block-uniform number of steps of kBatch rows; a lane whose
// row lies beyond the end loads the last row instead and drops the value, so the loads of a step carry no branch and are issued together.
constexpr int kBatch = 8;

inline bool channels_ok(int C) { return C >= 32 && C <= kMaxC && C % 32 == 0; }
inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int groups_cap(int64_t n) { return (int)(chunks_of(n) < kStatGroups ? chunks_of(n) : kStatGroups); }
inline int channel_blocks(int C) { return (C + kBlockC - 1) / kBlockC; }
// rows per apply workgroup (the apply pass is element-wise: its cut does not touch the sums)
inline int apply_rows(int64_t n) { return (int)((chunks_of(n) + kApplyBlocks - 1) / kApplyBlocks) * kChunk; }

typedef uint16_t bf16_t;  // the bits of a bfloat16

struct Launch {
    fd_dense_bn_nhwc_group g[kMaxRecords];
    int n_groups;
};

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
// bf16 -> fp32 is exact: the 16 bits are the upper half of the fp32 pattern
__device__ __forceinline__ float4 widen(uint2 u) {
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ uint2 ldq(const bf16_t *p) { return *reinterpret_cast<const uint2 *>(p); }
__device__ __forceinline__ float4 ld4(const bf16_t *p) { return widen(ldq(p)); }
__device__ __forceinline__ float ld1(const bf16_t *p) { return __uint_as_float((unsigned)*p << 16); }
// round to nearest even, a NaN stays a NaN (fd_sparse_bn.hip's to_bf16_rne)
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

// The cut of n rows: chunks, chunks per group, groups.  Everything follows from n.
struct Cut {
    int n, nb, G, ng;
    __device__ __forceinline__ Cut(int n_) {
        n = n_;
        nb = (n + kChunk - 1) / kChunk;
        G = (nb + kStatGroups - 1) / kStatGroups;
        ng = (nb + G - 1) / G;
    }
    __device__ __forceinline__ double rows_in_group(int g) const { return (double)min(G * kChunk, n - g * G * kChunk); }
};

// The workgroup's channel block [c0, c0 + cb) and the thread's place in it: column quad q of row lane rl (rl < RL takes rows).
struct Block {
    int c0, cb, QC, RL, q, rl;
    __device__ __forceinline__ Block(int C) {
        c0 = blockIdx.y * kBlockC;
        cb = min(kBlockC, C - c0);
        QC = cb >> 2;
        RL = kThreads / QC;
        q = threadIdx.x % QC;
        rl = threadIdx.x / QC;
    }
};

// Adds the row lanes of a float4 per thread in lane order: thread c < cb returns column c's total.  s_red: kRedFloats floats.
__device__ __forceinline__ float lane_sum(float4 v, float *s_red, const Block &k) {
    __syncthreads();
    if (k.rl < k.RL) st4(&s_red[k.rl * k.cb + 4 * k.q], v);
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < k.cb)
        for (int l = 0; l < k.RL; ++l) t += s_red[l * k.cb + threadIdx.x];
    return t;
}

// ---- forward pass 1: part[g] = [mean_g[C], M2_g[C]]
__global__ void __launch_bounds__(kThreads) bn_nhwc_stats(const bf16_t *__restrict__ x, int n, int C, float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    const Cut cut(n);
    const Block k(C);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nb) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nb);
    const bool on = k.rl < k.RL;
    const bf16_t *xq = x + k.c0 + 4 * k.q;
    double N = 0.0, mean = 0.0, M2 = 0.0;  // threads < cb: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, n);
        const float4 pivot = ld4(xq + (int64_t)r0 * C);
        uint2 hold[kHold];  // the thread's rows of the chunk: rows r0 + rl + i RL
#pragma unroll
        for (int i = 0; i < kHold; ++i) {
            const int r = r0 + k.rl + i * k.RL;
            hold[i] = make_uint2(0u, 0u);
            if (on && r < r1) hold[i] = ldq(xq + (int64_t)r * C);
        }
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < kHold; ++i) {
            if (on && r0 + k.rl + i * k.RL < r1) {
                const float4 v = widen(hold[i]);
                s.x += v.x - pivot.x;
                s.y += v.y - pivot.y;
                s.z += v.z - pivot.z;
                s.w += v.w - pivot.w;
            }
        }
        const float tot = lane_sum(s, red, k);
        const float nbf = (float)(r1 - r0);
        float mb = 0.f;
        if (threadIdx.x < k.cb) s_mean[threadIdx.x] = mb = ld1(x + (int64_t)r0 * C + k.c0 + threadIdx.x) + tot / nbf;
        __syncthreads();
        const float4 m = ld4(&s_mean[4 * k.q]);
        s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < kHold; ++i) {
            if (on && r0 + k.rl + i * k.RL < r1) {
                const float4 v = widen(hold[i]);
                const float dx = v.x - m.x, dy = v.y - m.y, dz = v.z - m.z, dw = v.w - m.w;
                s.x += dx * dx;
                s.y += dy * dy;
                s.z += dz * dz;
                s.w += dw * dw;
            }
        }
        const float m2 = lane_sum(s, red, k);
        if (threadIdx.x < k.cb) {  // Chan's rule, chunk b onto the group so far
            const double nbd = (double)nbf, N1 = N + nbd, d = (double)mb - mean;
            mean += d * (nbd / N1);
            M2 += (double)m2 + d * d * (N * nbd / N1);
            N = N1;
        }
    }
    if (threadIdx.x < k.cb) {
        float *dst = part + (size_t)blockIdx.x * 2 * C + k.c0;
        dst[threadIdx.x] = (float)mean;
        dst[C + threadIdx.x] = (float)M2;
    }
}

struct D4 {
    double x, y, z, w;
};

// Slices of the group partials: thread (slice s = t / (cb / 4), column quad q) owns groups [s per, (s + 1) per) of the ng.
struct Slices {
    int S, q, s, g0, g1;
    __device__ __forceinline__ Slices(const Block &k, int ng) {
        S = k.RL;
        q = k.q;
        s = k.rl;
        const int per = (ng + S - 1) / S;
        g0 = min(ng, s * per);
        g1 = s < S ? min(ng, g0 + per) : g0;
    }
};

// Adds the slices in slice order: thread c < cb returns column c's total.  s_acc: kRedFloats doubles.
__device__ __forceinline__ double slice_total(const D4 &a, double *s_acc, const Slices &sl, int cb) {
    __syncthreads();
    if (sl.s < sl.S) {
        double *d = &s_acc[sl.s * cb + 4 * sl.q];
        d[0] = a.x;
        d[1] = a.y;
        d[2] = a.z;
        d[3] = a.w;
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < cb)
        for (int j = 0; j < sl.S; ++j) t += s_acc[j * cb + threadIdx.x];
    return t;
}

// The record that owns channel ch and the channel's place in it.  The loop is unrolled over the records with constant indices: the
// launch structure stays in the kernel arguments.
struct Owner {
    const float *gamma, *beta;
    float *running_mean, *running_var;
    long long *counter;
    int local;
    float eps;
    double momentum;
    __device__ __forceinline__ Owner(const Launch &L, int ch) {
        gamma = beta = nullptr;
        running_mean = running_var = nullptr;
        counter = nullptr;
        local = 0;
        eps = 1.f;
        momentum = 0.0;
        int off = 0;
#pragma unroll
        for (int j = 0; j < kMaxRecords; ++j) {
            if (j < L.n_groups) {
                const int end = off + L.g[j].c;
                if (ch >= off && ch < end) {
                    gamma = L.g[j].gamma;
                    beta = L.g[j].beta;
                    running_mean = L.g[j].running_mean;
                    running_var = L.g[j].running_var;
                    counter = (long long *)L.g[j].num_batches_tracked;
                    local = ch - off;
                    eps = L.g[j].eps;
                    momentum = L.g[j].momentum;
                }
                off = end;
            }
        }
    }
};

// ---- forward pass 2: statistics from the group partials, then y for the workgroup's rows
__global__ void __launch_bounds__(kThreads) bn_nhwc_apply(const bf16_t *__restrict__ x, const Launch L, int n, int C, int relu,
                                                           int rows_per_block, const float *__restrict__ part, bf16_t *__restrict__ y,
                                                           float *__restrict__ saved) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) double s_mu[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_scale[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_beta[kBlockC];
    const Cut cut(n);
    const Block k(C);
    const double cnt = (double)n;
    const Slices sl(k, cut.ng);
    const float *pq = part + k.c0 + 4 * k.q;
    D4 a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 m = ld4(pq + (size_t)g * 2 * C);
        const double w = cut.rows_in_group(g);
        a.x += w * (double)m.x;
        a.y += w * (double)m.y;
        a.z += w * (double)m.z;
        a.w += w * (double)m.w;
    }
    double t = slice_total(a, s_acc, sl, k.cb);
    if (threadIdx.x < k.cb) s_mu[threadIdx.x] = t / cnt;
    __syncthreads();
    const double mu0 = s_mu[4 * k.q], mu1 = s_mu[4 * k.q + 1], mu2 = s_mu[4 * k.q + 2], mu3 = s_mu[4 * k.q + 3];
    a = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 m = ld4(pq + (size_t)g * 2 * C);
        const float4 v = ld4(pq + (size_t)g * 2 * C + C);
        const double w = cut.rows_in_group(g);
        const double d0 = (double)m.x - mu0, d1 = (double)m.y - mu1, d2 = (double)m.z - mu2, d3 = (double)m.w - mu3;
        a.x += (double)v.x + w * d0 * d0;
        a.y += (double)v.y + w * d1 * d1;
        a.z += (double)v.z + w * d2 * d2;
        a.w += (double)v.w + w * d3 * d3;
    }
    t = slice_total(a, s_acc, sl, k.cb);
    if (threadIdx.x < k.cb) {
        const int c = threadIdx.x, ch = k.c0 + c;
        const Owner o(L, ch);
        const double var = t > 0.0 ? t / cnt : 0.0;
        const float mean_f = (float)s_mu[c];
        const float invstd = (float)(1.0 / sqrt(var + (double)o.eps));
        s_mean[c] = mean_f;
        s_scale[c] = o.gamma[o.local] * invstd;
        s_beta[c] = o.beta[o.local];
        if (blockIdx.x == 0) {
            saved[ch] = mean_f;
            saved[C + ch] = invstd;
            const double unbiased = var * (cnt / (cnt - 1.0));
            o.running_mean[o.local] = (float)((1.0 - o.momentum) * (double)o.running_mean[o.local] + o.momentum * s_mu[c]);
            o.running_var[o.local] = (float)((1.0 - o.momentum) * (double)o.running_var[o.local] + o.momentum * unbiased);
            if (o.local == 0) o.counter[0] += 1;
        }
    }
    __syncthreads();
    if (k.rl >= k.RL) return;
    const float4 m = ld4(&s_mean[4 * k.q]), sc = ld4(&s_scale[4 * k.q]), be = ld4(&s_beta[4 * k.q]);
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, n);
    const int64_t col = k.c0 + 4 * k.q;
    for (int rb = r0 + k.rl; rb < r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
        uint2 xs[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) xs[u] = ldq(x + (int64_t)min(rb + u * k.RL, r1 - 1) * C + col);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int r = rb + u * k.RL;
            if (r >= r1) break;
            const int64_t o = (int64_t)r * C + col;
            const float4 xv = widen(xs[u]);
            float4 v;
            v.x = (xv.x - m.x) * sc.x + be.x;
            v.y = (xv.y - m.y) * sc.y + be.y;
            v.z = (xv.z - m.z) * sc.z + be.z;
            v.w = (xv.w - m.w) * sc.w + be.w;
            if (relu) {
                v.x = v.x > 0.f ? v.x : 0.f;
                v.y = v.y > 0.f ? v.y : 0.f;
                v.z = v.z > 0.f ? v.z : 0.f;
                v.w = v.w > 0.f ? v.w : 0.f;
            }
            st4(y + o, v);
        }
    }
}

// g = dy where y > 0.  RELU is a template parameter of the backward kernels: with a run-time flag the branch around the load of y keeps
// the compiler from issuing the loads of several rows together.
template <bool RELU>
__device__ __forceinline__ float4 masked(const bf16_t *__restrict__ dy, const bf16_t *__restrict__ y, int64_t o) {
    float4 g = ld4(dy + o);
    if (RELU) {
        const float4 yv = ld4(y + o);
        g.x = yv.x > 0.f ? g.x : 0.f;
        g.y = yv.y > 0.f ? g.y : 0.f;
        g.z = yv.z > 0.f ? g.z : 0.f;
        g.w = yv.w > 0.f ? g.w : 0.f;
    }
    return g;
}

// ---- backward pass 1: part[g] = [sum g [C], sum g x^ [C]]
template <bool RELU>
__global__ void __launch_bounds__(kThreads) bn_nhwc_grad_sums(const bf16_t *__restrict__ dy, const bf16_t *__restrict__ x,
                                                               const bf16_t *__restrict__ y, const float *__restrict__ saved, int n, int C,
                                                               float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    const Cut cut(n);
    const Block k(C);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nb) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nb);
    const int64_t col = k.c0 + 4 * k.q;
    const float4 m = ld4(saved + col), is = ld4(saved + C + col);
    double db = 0.0, dg = 0.0;  // threads < cb: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, n);
        float4 sb = make_float4(0.f, 0.f, 0.f, 0.f), sg = sb;
        if (k.rl < k.RL) {
            for (int rb = r0 + k.rl; rb < r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
                float4 gs[kBatch];
                uint2 xs[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    const int64_t o = (int64_t)min(rb + u * k.RL, r1 - 1) * C + col;
                    gs[u] = masked<RELU>(dy, y, o);
                    xs[u] = ldq(x + o);
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {  // (a row beyond the end adds zeros: no branch for the loads to sink into)
                    const bool in = rb + u * k.RL < r1;
                    float4 g = gs[u];
                    g.x = in ? g.x : 0.f;
                    g.y = in ? g.y : 0.f;
                    g.z = in ? g.z : 0.f;
                    g.w = in ? g.w : 0.f;
                    const float4 xv = widen(xs[u]);
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
        }
        db += (double)lane_sum(sb, red, k);
        dg += (double)lane_sum(sg, red, k);
    }
    if (threadIdx.x < k.cb) {
        float *dst = part + (size_t)blockIdx.x * 2 * C + k.c0;
        dst[threadIdx.x] = (float)db;
        dst[C + threadIdx.x] = (float)dg;
    }
}

// ---- backward pass 2: dbeta / dgamma from the group partials, then dx for the workgroup's rows
template <bool RELU>
__global__ void __launch_bounds__(kThreads) bn_nhwc_grad_apply(const bf16_t *__restrict__ dy, const bf16_t *__restrict__ x,
                                                                const bf16_t *__restrict__ y, const Launch L,
                                                                const float *__restrict__ saved, int n, int C, int rows_per_block,
                                                                const float *__restrict__ part, bf16_t *__restrict__ dx,
                                                                float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_is[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_k[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mb[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mg[kBlockC];
    const Cut cut(n);
    const Block k(C);
    const Slices sl(k, cut.ng);
    const float *pq = part + k.c0 + 4 * k.q;
    D4 ab = {0.0, 0.0, 0.0, 0.0}, ag = ab;
#pragma unroll 8
    for (int g = sl.g0; g < sl.g1; ++g) {
        const float4 b = ld4(pq + (size_t)g * 2 * C);
        const float4 v = ld4(pq + (size_t)g * 2 * C + C);
        ab.x += (double)b.x;
        ab.y += (double)b.y;
        ab.z += (double)b.z;
        ab.w += (double)b.w;
        ag.x += (double)v.x;
        ag.y += (double)v.y;
        ag.z += (double)v.z;
        ag.w += (double)v.w;
    }
    const double db = slice_total(ab, s_acc, sl, k.cb);
    const double dg = slice_total(ag, s_acc, sl, k.cb);
    if (threadIdx.x < k.cb) {
        const int c = threadIdx.x, ch = k.c0 + c;
        const Owner o(L, ch);
        const double cnt = (double)n;
        const float is = saved[C + ch];
        s_mean[c] = saved[ch];
        s_is[c] = is;
        s_k[c] = o.gamma[o.local] * is;
        s_mb[c] = (float)(db / cnt);
        s_mg[c] = (float)(dg / cnt);
        if (blockIdx.x == 0) {
            dbeta[ch] = (float)db;
            dgamma[ch] = (float)dg;
        }
    }
    __syncthreads();
    if (k.rl >= k.RL) return;
    const float4 m = ld4(&s_mean[4 * k.q]), is = ld4(&s_is[4 * k.q]), kk = ld4(&s_k[4 * k.q]), mb = ld4(&s_mb[4 * k.q]),
                 mg = ld4(&s_mg[4 * k.q]);
    const int r0 = blockIdx.x * rows_per_block, r1 = min(r0 + rows_per_block, n);
    const int64_t col = k.c0 + 4 * k.q;
    for (int rb = r0 + k.rl; rb < r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
        float4 gs[kBatch];
        uint2 xs[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int64_t o = (int64_t)min(rb + u * k.RL, r1 - 1) * C + col;
            gs[u] = masked<RELU>(dy, y, o);
            xs[u] = ldq(x + o);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int r = rb + u * k.RL;
            if (r >= r1) break;
            const int64_t o = (int64_t)r * C + col;
            const float4 g = gs[u];
            const float4 xv = widen(xs[u]);
            float4 d;
            d.x = kk.x * (g.x - mb.x - (xv.x - m.x) * is.x * mg.x);
            d.y = kk.y * (g.y - mb.y - (xv.y - m.y) * is.y * mg.y);
            d.z = kk.z * (g.z - mb.z - (xv.z - m.z) * is.z * mg.z);
            d.w = kk.w * (g.w - mb.w - (xv.w - m.w) * is.w * mg.w);
            st4(dx + o, d);
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// What both entry points check of the sizes, the records' channel counts and the workspace; fills the launch structure.
int check_call(const char *fn, const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu, const void *workspace,
               size_t workspace_bytes, Launch &L) {
    FD_REQUIRE(groups, "%s: null groups", fn);
    FD_REQUIRE(n_groups >= 1 && n_groups <= kMaxRecords, "%s: n_groups must be in [1, %d] (got %d)", fn, kMaxRecords, n_groups);
    FD_REQUIRE(channels_ok(C), "%s: unsupported C %d: a multiple of 32 in [32, %d]", fn, C, kMaxC);
    int64_t sum = 0;
    for (int j = 0; j < n_groups; ++j) {
        FD_REQUIRE(groups[j].c >= 32 && groups[j].c <= kMaxC && groups[j].c % 32 == 0,
                   "%s: group %d: unsupported c %d: a multiple of 32 in [32, %d]", fn, j, groups[j].c, kMaxC);
        sum += groups[j].c;
    }
    FD_REQUIRE(sum == C, "%s: the groups' c sum to %lld, not to C = %d", fn, (long long)sum, C);
    FD_REQUIRE(n >= 2 && n <= kMaxRows, "%s: n out of range (%lld): more than 1 value per channel, at most 2^30 rows", fn, (long long)n);
    FD_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1 (got %d)", fn, relu);
    FD_REQUIRE(workspace, "%s: null workspace", fn);
    FD_REQUIRE(workspace_bytes >= fd_dense_bn_nhwc_workspace_bytes(n, C), "%s: workspace too small (%zu bytes, %zu needed)", fn,
               workspace_bytes, fd_dense_bn_nhwc_workspace_bytes(n, C));
    FD_REQUIRE(aligned16(workspace), "%s: the workspace must be 16-byte aligned", fn);
    for (int j = 0; j < kMaxRecords; ++j) L.g[j] = groups[j < n_groups ? j : 0];
    L.n_groups = n_groups;
    return FD_OK;
}

}  // namespace

extern "C" int fd_dense_bn_nhwc_chunk(void) { return kChunk; }
extern "C" int fd_dense_bn_nhwc_stat_groups(void) { return kStatGroups; }
extern "C" int fd_dense_bn_nhwc_apply_blocks(void) { return kApplyBlocks; }

extern "C" size_t fd_dense_bn_nhwc_workspace_bytes(int64_t n, int C) {
    if (n < 2 || n > kMaxRows || !channels_ok(C)) return 0;
    return fd::align_up((size_t)groups_cap(n) * 2 * C * sizeof(float), 256);
}

extern "C" int fd_dense_bn_nhwc_train_forward_bf16(const uint16_t *x, const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C,
                                                   int relu, uint16_t *y, float *saved, void *workspace, size_t workspace_bytes,
                                                   fd_stream_t stream_) {
    const char *fn = "fd_dense_bn_nhwc_train_forward_bf16";
    FD_REQUIRE(x && y && saved, "%s: null x, y or saved", fn);
    Launch L;
    if (int e = check_call(fn, groups, n_groups, n, C, relu, workspace, workspace_bytes, L)) return e;
    for (int j = 0; j < n_groups; ++j) {
        const fd_dense_bn_nhwc_group &g = groups[j];
        FD_REQUIRE(g.gamma && g.beta, "%s: group %d: null gamma or beta", fn, j);
        FD_REQUIRE(g.running_mean && g.running_var && g.num_batches_tracked, "%s: group %d: null running statistics", fn, j);
        FD_REQUIRE(g.eps > 0.f, "%s: group %d: eps must be > 0", fn, j);
        FD_REQUIRE(g.momentum >= 0.0 && g.momentum <= 1.0, "%s: group %d: momentum must be in [0, 1]", fn, j);
    }
    FD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(saved), "%s: x, y and saved must be 16-byte aligned", fn);
    hipStream_t st = fd::as_stream(stream_);
    const int rows = apply_rows(n);
    float *part = (float *)workspace;
    const unsigned cblocks = (unsigned)channel_blocks(C);
    hipLaunchKernelGGL(bn_nhwc_stats, dim3((unsigned)groups_cap(n), cblocks), dim3(kThreads), 0, st, x, (int)n, C, part);
    hipLaunchKernelGGL(bn_nhwc_apply, dim3((unsigned)((n + rows - 1) / rows), cblocks), dim3(kThreads), 0, st, x, L, (int)n, C, relu, rows,
                       (const float *)part, y, saved);
    return fd::check_launch(fn);
}

extern "C" int fd_dense_bn_nhwc_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *saved,
                                                    const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu,
                                                    uint16_t *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                                    fd_stream_t stream_) {
    const char *fn = "fd_dense_bn_nhwc_train_backward_bf16";
    FD_REQUIRE(dy && x && saved, "%s: null dy, x or saved", fn);
    FD_REQUIRE(y || relu == 0, "%s: null y (the ReLU mask)", fn);
    FD_REQUIRE(dx && dgamma && dbeta, "%s: null dx, dgamma or dbeta", fn);
    Launch L;
    if (int e = check_call(fn, groups, n_groups, n, C, relu, workspace, workspace_bytes, L)) return e;
    for (int j = 0; j < n_groups; ++j) FD_REQUIRE(groups[j].gamma, "%s: group %d: null gamma", fn, j);
    FD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(saved) && aligned16(dx),
               "%s: dy, x, y, saved and dx must be 16-byte aligned", fn);
    hipStream_t st = fd::as_stream(stream_);
    const int rows = apply_rows(n);
    float *part = (float *)workspace;
    const unsigned cblocks = (unsigned)channel_blocks(C);
    const dim3 sums_grid((unsigned)groups_cap(n), cblocks), apply_grid((unsigned)((n + rows - 1) / rows), cblocks);
    if (relu) {
        hipLaunchKernelGGL(bn_nhwc_grad_sums<true>, sums_grid, dim3(kThreads), 0, st, dy, x, y, saved, (int)n, C, part);
        hipLaunchKernelGGL(bn_nhwc_grad_apply<true>, apply_grid, dim3(kThreads), 0, st, dy, x, y, L, saved, (int)n, C, rows,
                           (const float *)part, dx, dgamma, dbeta);
    } else {
        hipLaunchKernelGGL(bn_nhwc_grad_sums<false>, sums_grid, dim3(kThreads), 0, st, dy, x, y, saved, (int)n, C, part);
        hipLaunchKernelGGL(bn_nhwc_grad_apply<false>, apply_grid, dim3(kThreads), 0, st, dy, x, y, L, saved, (int)n, C, rows,
                           (const float *)part, dx, dgamma, dbeta);
    }
    return fd::check_launch(fn);
}
