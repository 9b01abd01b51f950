// Training-mode BatchNorm over the rows of a row-major matrix x [n, C], fused with what follows it: y = act(gamma (x - mean) invstd +
// beta [+ residual]), and its backward.  One kernel family behind two APIs: fd_sparse_bn.hip (BatchNorm1d over the rows of a sparse
// feature matrix, fp32 or bf16, SpMiddleResNetFHD) and fd_dense_bn_nhwc.hip (BatchNorm2d over a bf16 channels-last map, n = B H W, RPN
// and CenterHead in mixed precision).  Each including file gets its own copy of the kernels (anonymous namespace).
//
// Channels.  A workgroup owns a channel block of at most kBlockC = 128 channels (C = 160: blocks of 128 and 32; C = 96: one block of 96);
// grid dimension y runs over the blocks.  The parameters come in a launch record passed by value: up to kMaxRecords
// fd_dense_bn_nhwc_group records, record j owning the next c_j channels with its own gamma, beta, eps, momentum, running statistics and
// counter (the six or seven 64-channel branches of a SepHead are one call on their 384- or 448-channel map; the sparse API passes one
// record over all C channels).
//
// Statistics.  The valid rows (n, or the device's count n_dev clamped to [0, n]: then n is the capacity) are cut into chunks of kChunk
// rows: chunk b owns rows [b kChunk, min((b + 1) kChunk, nv)).  Consecutive chunks form at most kMaxGroups groups of
// G = ceil(chunks / kMaxGroups) chunks.  Pass 1, one workgroup per (group, channel block): per chunk, the column means (summed relative
// to the chunk's first row, so a mean that is large against the spread costs no digits) and M2_b = sum (x - mean_b)^2 centred at that
// mean; the group's chunks are merged in chunk order, in double, with Chan's rule (mean += d n_b / N', M2 += M2_b + d^2 N n_b / N').  A
// thread holds its rows of the chunk in registers (at most kHold quads): the chunk is read from memory once, all its loads are in flight
// together, and the second moment is taken from the registers.  Pass 2: EVERY workgroup re-sums the (at most kMaxGroups) group partials
// itself, in double, in a fixed order -- mean = sum n_g mean_g / n, then M2 = sum [M2_g + n_g (mean_g - mean)^2]; the groups are cut
// into slices, a slice adds its groups in order, the slices are added in slice order -- and then applies the normalisation to its rows
// (at most kMaxApplyBlocks row blocks of whole chunks).  The workgroups of the first row block also write mean / invstd for the backward
// and update each record's running statistics (unbiased variance) and counter.  Two launches per direction, no atomics: chunk, group and
// slice boundaries depend on the valid row count and C only, so two runs give the same bits, and a call that reads the row count from
// the device gives the bits of the exact-size call.  Every workspace word that pass 2 reads was written by pass 1 of the same call.
//
// Backward.  g = dy where y > 0 (y is the forward's output: the ReLU mask), x^ = (x - mean) invstd.  Pass 1: sums of g and g x^ per
// chunk, added per group in chunk order in double; pass 2: every workgroup re-sums the group partials in the same fixed order,
// dx = gamma invstd (g - dbeta / n - x^ dgamma / n), d_residual = g.
//
// Rows behind the device's count.  The capacity tail [nv, n) of y, dx and d_residual is written as zeros, and no value of such a row
// reaches an output or a sum (template parameter TAIL: only the sparse API's instantiations carry this, the residual and d_residual).
// With nv = 0 the pass-1 workgroups leave at once, mean = 0, invstd = 1 / sqrt(eps), and the running
// statistics and counters stay as they are; with nv = 1 the unbiased factor is 1.
//
// Thread layout of every pass: a block row is cb / 4 column quads; thread t takes quad t % (cb / 4) of rows t / (cb / 4),
// + 256 / (cb / 4), ... (a wave reads whole rows).  Row lanes are added in lane order through LDS.  The element-wise loops run a
// block-uniform number of steps of kBatch rows; a lane whose row lies beyond the end loads the last valid row instead and drops the
// value, so the loads of a step carry no branch and are issued together.
//
// Row type.  Every kernel is a template over the type T of the row tensors (x, residual, y, dy, dx, d_residual): float, a quad is one
// float4 (16 bytes), or bf16_t, a quad is one 8-byte group that is widened exactly to fp32 on load and rounded to nearest even on store.
// Nothing else differs: the bf16 form computes what the fp32 form computes on the widened rows, and rounds once.  Parameters,
// statistics, saved, dgamma, dbeta and the workspace partials are fp32 either way.
#pragma once
#include "fd_common.h"

namespace {
namespace row_bn {

constexpr int kChunk = 256;
constexpr int kMaxGroups = 256;       // group partials at most: every apply workgroup re-sums them
constexpr int kMaxApplyBlocks = 512;  // row blocks of the apply passes at most
static_assert(FD_SPARSE_BN_CHUNK == kChunk && FD_DENSE_BN_NHWC_CHUNK == kChunk && FD_DENSE_BN_NHWC_STAT_GROUPS == kMaxGroups &&
                  FD_DENSE_BN_NHWC_APPLY_BLOCKS == kMaxApplyBlocks,
              "the public header's cut constants are those of the kernels");
constexpr int kThreads = 256;
constexpr int kBlockC = 128;  // channels of a workgroup at most
constexpr int kMaxRecords = FD_DENSE_BN_NHWC_MAX_GROUPS;
constexpr int kRedFloats = 4 * kThreads;  // lanes * cb <= 256 / (cb / 4) * cb
constexpr int64_t kMaxRows = (int64_t)1 << 30;
constexpr int kHold = kChunk / (kThreads / (kBlockC / 4));  // rows of a chunk per thread at most (the widest block: 8 row lanes)
constexpr int kBatch = 8;                                   // rows a thread has in flight in the element-wise loops
static_assert(kChunk % 64 == 0 && kHold <= 32, "chunk");

inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int groups_cap(int64_t n) { return (int)(chunks_of(n) < kMaxGroups ? chunks_of(n) : kMaxGroups); }
inline int channel_blocks(int C) { return (C + kBlockC - 1) / kBlockC; }
// rows per apply workgroup: a function of the capacity only (the apply pass is element-wise: its cut does not touch the sums)
inline int apply_rows(int64_t n) { return (int)((chunks_of(n) + kMaxApplyBlocks - 1) / kMaxApplyBlocks) * kChunk; }
inline size_t workspace_bytes(int64_t n, int C) { return fd::align_up((size_t)groups_cap(n) * 2 * C * sizeof(float), 256); }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

typedef uint16_t bf16_t;  // the bits of a bfloat16

// The row loops have two forms, selected at compile time.  The plain form walks a thread's rows one by one (pass 1 of the forward reads
// a chunk twice); it is kept for the fp32 rows of the sparse API, whose 16-channel level measured slower in the other form (16-byte quads:
// 107-156 registers against 38-64).  Every other instantiation holds the chunk in registers and loads in batches (header comment).
template <typename T, bool TAIL>
constexpr bool kPlain = TAIL && sizeof(T) == 4;

struct Launch {
    fd_dense_bn_nhwc_group g[kMaxRecords];
    int n_groups;
};

// A quad as it lies in memory (ldq), and as four fp32 (widen).  bf16 -> fp32 is exact: the 16 bits are the upper half of the pattern.
__device__ __forceinline__ float4 ldq(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ uint2 ldq(const bf16_t *p) { return *reinterpret_cast<const uint2 *>(p); }
__device__ __forceinline__ float4 widen(float4 v) { return v; }
__device__ __forceinline__ float4 widen(uint2 u) {
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}
template <typename T>
using quad_t = decltype(ldq((const T *)nullptr));
template <typename T>
__device__ __forceinline__ float4 ld4(const T *p) {
    return widen(ldq(p));
}
__device__ __forceinline__ float ld1(const float *p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t *p) { return __uint_as_float((unsigned)*p << 16); }
// round to nearest even as fd::bf16_rne (fd_spconv_pack.h) does, and a copy of its own because here a NaN stays a NaN instead of
// carrying into the sign
__device__ __forceinline__ unsigned to_bf16_rne(float v) {
    const unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void st4(bf16_t *p, float4 v) {
    uint2 u;
    u.x = to_bf16_rne(v.x) | (to_bf16_rne(v.y) << 16);
    u.y = to_bf16_rne(v.z) | (to_bf16_rne(v.w) << 16);
    *reinterpret_cast<uint2 *>(p) = u;
}

// The cut of the nv valid rows: chunks, chunks per group, groups.  Device side: everything follows from the valid row count.
template <bool TAIL>
struct Cut {
    int nv, nbv, G, ng;
    __device__ __forceinline__ Cut(int n, const int *n_dev) {
        nv = TAIL ? fd::device_count(n, n_dev) : n;  // (without TAIL: n >= 2, checked on the host)
        nbv = (nv + kChunk - 1) / kChunk;
        G = (nbv + kMaxGroups - 1) / kMaxGroups;
        if (TAIL && G < 1) G = 1;
        ng = (nbv + G - 1) / G;
    }
    __device__ __forceinline__ double rows_in_group(int g) const { return (double)min(G * kChunk, nv - g * G * kChunk); }
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
template <typename T, bool TAIL>
__global__ void __launch_bounds__(kThreads) row_bn_stats(const T *__restrict__ x, int n, int C, float *__restrict__ part,
                                                          const int *__restrict__ n_dev) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    const Cut<TAIL> cut(n, n_dev);
    const Block k(C);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nbv) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nbv);
    const bool on = k.rl < k.RL;
    const T *xq = x + k.c0 + 4 * k.q;
    double N = 0.0, mean = 0.0, M2 = 0.0;  // threads < cb: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, cut.nv);
        const float4 pivot = ld4(xq + (int64_t)r0 * C);
        quad_t<T> hold[kPlain<T, TAIL> ? 1 : kHold];  // the thread's rows of the chunk: rows r0 + rl + i RL
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (kPlain<T, TAIL>) {
            if (on) {
#pragma unroll 4
                for (int r = r0 + k.rl; r < r1; r += k.RL) {
                    const float4 v = ld4(xq + (int64_t)r * C);
                    s.x += v.x - pivot.x;
                    s.y += v.y - pivot.y;
                    s.z += v.z - pivot.z;
                    s.w += v.w - pivot.w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < kHold; ++i) {
                const int r = r0 + k.rl + i * k.RL;
                hold[i] = quad_t<T>{};
                if (on && r < r1) hold[i] = ldq(xq + (int64_t)r * C);
            }
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
        }
        const float tot = lane_sum(s, red, k);
        const float nbf = (float)(r1 - r0);
        float mb = 0.f;
        if (threadIdx.x < k.cb) s_mean[threadIdx.x] = mb = ld1(x + (int64_t)r0 * C + k.c0 + threadIdx.x) + tot / nbf;
        __syncthreads();
        const float4 m = ld4(&s_mean[4 * k.q]);
        s = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (kPlain<T, TAIL>) {
            if (on) {
#pragma unroll 4
                for (int r = r0 + k.rl; r < r1; r += k.RL) {
                    const float4 v = ld4(xq + (int64_t)r * C);
                    const float dx = v.x - m.x, dy = v.y - m.y, dz = v.z - m.z, dw = v.w - m.w;
                    s.x += dx * dx;
                    s.y += dy * dy;
                    s.z += dz * dz;
                    s.w += dw * dw;
                }
            }
        } else {
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

// The workgroup's rows [r0, r1) of an element-wise pass, and the row a lane loads in place of one at or behind `last + 1` (the end of
// the block or of the valid rows; row 0 when there are none): its value is dropped.
struct RowBlock {
    int r0, r1, last;
    __device__ __forceinline__ RowBlock(int rows_per_block, int n, int nv) {
        r0 = blockIdx.x * rows_per_block;
        r1 = min(r0 + rows_per_block, n);
        last = max(min(r1, nv) - 1, 0);
    }
};

// ---- forward pass 2: statistics from the group partials, then y for the workgroup's rows
template <typename T, bool TAIL>
__global__ void __launch_bounds__(kThreads) row_bn_apply(const T *__restrict__ x, const Launch L, int n, int C, int relu, int rows_per_block,
                                                          const float *__restrict__ part, T *__restrict__ y, float *__restrict__ saved,
                                                          const int *__restrict__ n_dev, const T *__restrict__ residual) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) double s_mu[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_scale[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_beta[kBlockC];
    const Cut<TAIL> cut(n, n_dev);
    const Block k(C);
    const int nv = cut.nv;
    const double cnt = (double)nv;
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
    const bool any = !TAIL || nv > 0;  // (only a device count can be 0 or 1)
    if (threadIdx.x < k.cb) s_mu[threadIdx.x] = any ? t / cnt : 0.0;
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
        const double var = any && t > 0.0 ? t / cnt : 0.0;
        const float mean_f = (float)s_mu[c];
        const float invstd = (float)(1.0 / sqrt(var + (double)o.eps));
        s_mean[c] = mean_f;
        s_scale[c] = o.gamma[o.local] * invstd;
        s_beta[c] = o.beta[o.local];
        if (blockIdx.x == 0) {
            saved[ch] = mean_f;
            saved[C + ch] = invstd;
            if (any) {
                const double unbiased = var * (cnt / (!TAIL || nv > 1 ? cnt - 1.0 : 1.0));
                o.running_mean[o.local] = (float)((1.0 - o.momentum) * (double)o.running_mean[o.local] + o.momentum * s_mu[c]);
                o.running_var[o.local] = (float)((1.0 - o.momentum) * (double)o.running_var[o.local] + o.momentum * unbiased);
                if (o.local == 0) o.counter[0] += 1;
            }
        }
    }
    __syncthreads();
    if (k.rl >= k.RL) return;
    const float4 m = ld4(&s_mean[4 * k.q]), sc = ld4(&s_scale[4 * k.q]), be = ld4(&s_beta[4 * k.q]);
    const RowBlock rows(rows_per_block, n, nv);
    const int64_t col = k.c0 + 4 * k.q;
    if constexpr (kPlain<T, TAIL>) {
#pragma unroll 4
        for (int r = rows.r0 + k.rl; r < rows.r1; r += k.RL) {
            const int64_t o = (int64_t)r * C + col;
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
    } else {
        for (int rb = rows.r0 + k.rl; rb < rows.r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
            quad_t<T> xs[kBatch], rs[kBatch];
    #pragma unroll
            for (int u = 0; u < kBatch; ++u) xs[u] = ldq(x + (int64_t)min(rb + u * k.RL, rows.last) * C + col);
            if (TAIL && residual) {
    #pragma unroll
                for (int u = 0; u < kBatch; ++u) rs[u] = ldq(residual + (int64_t)min(rb + u * k.RL, rows.last) * C + col);
            }
    #pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int r = rb + u * k.RL;
                if (r >= rows.r1) break;
                const float4 xv = widen(xs[u]);
                float4 v;
                v.x = (xv.x - m.x) * sc.x + be.x;
                v.y = (xv.y - m.y) * sc.y + be.y;
                v.z = (xv.z - m.z) * sc.z + be.z;
                v.w = (xv.w - m.w) * sc.w + be.w;
                if (TAIL && residual) {
                    const float4 rv = widen(rs[u]);
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
                if (TAIL && r >= nv) v = make_float4(0.f, 0.f, 0.f, 0.f);
                st4(y + (int64_t)r * C + col, v);
            }
        }
    }
}

// g = dy where y > 0.  RELU is a template parameter of the backward kernels: with a run-time flag the branch around the load of y keeps
// the compiler from issuing the loads of several rows together.
template <bool RELU, typename T>
__device__ __forceinline__ float4 masked(const T *__restrict__ dy, const T *__restrict__ y, int64_t o) {
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
template <typename T, bool TAIL, bool RELU>
__global__ void __launch_bounds__(kThreads) row_bn_grad_sums(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ y,
                                                              const float *__restrict__ saved, int n, int C, float *__restrict__ part,
                                                              const int *__restrict__ n_dev) {
    __shared__ __attribute__((aligned(16))) float red[kRedFloats];
    const Cut<TAIL> cut(n, n_dev);
    const Block k(C);
    const int b0 = blockIdx.x * cut.G;
    if (b0 >= cut.nbv) return;  // block-uniform
    const int b1 = min(b0 + cut.G, cut.nbv);
    const int64_t col = k.c0 + 4 * k.q;
    const float4 m = ld4(saved + col), is = ld4(saved + C + col);
    double db = 0.0, dg = 0.0;  // threads < cb: the group so far
    for (int b = b0; b < b1; ++b) {
        const int r0 = b * kChunk, r1 = min(r0 + kChunk, cut.nv);
        float4 sb = make_float4(0.f, 0.f, 0.f, 0.f), sg = sb;
        if (kPlain<T, TAIL> && k.rl < k.RL) {
#pragma unroll 2
            for (int r = r0 + k.rl; r < r1; r += k.RL) {
                const int64_t o = (int64_t)r * C + col;
                const float4 g = masked<RELU>(dy, y, o);
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
        if (!kPlain<T, TAIL> && k.rl < k.RL) {
            for (int rb = r0 + k.rl; rb < r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
                const int base = __builtin_amdgcn_readfirstlane(rb - k.rl);  // block-uniform, in a scalar register
                float4 gs[kBatch];
                quad_t<T> xs[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {
                    if (TAIL && base + u * k.RL >= r1) break;  // (C = 16: a chunk is half a step)
                    const int64_t o = (int64_t)min(rb + u * k.RL, r1 - 1) * C + col;
                    gs[u] = masked<RELU>(dy, y, o);
                    xs[u] = ldq(x + o);
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {  // (a row beyond the end adds zeros: no branch for the loads to sink into)
                    if (TAIL && base + u * k.RL >= r1) break;
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

// ---- backward pass 2: dbeta / dgamma from the group partials, then dx (and d_residual) for the workgroup's rows
template <typename T, bool TAIL, bool RELU>
__global__ void __launch_bounds__(kThreads) row_bn_grad_apply(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ y,
                                                               const Launch L, const float *__restrict__ saved, int n, int C,
                                                               int rows_per_block, const float *__restrict__ part, T *__restrict__ dx,
                                                               float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                               const int *__restrict__ n_dev, T *__restrict__ d_residual) {
    __shared__ double s_acc[kRedFloats];
    __shared__ __attribute__((aligned(16))) float s_mean[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_is[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_k[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mb[kBlockC];
    __shared__ __attribute__((aligned(16))) float s_mg[kBlockC];
    const Cut<TAIL> cut(n, n_dev);
    const Block k(C);
    const int nv = cut.nv;
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
        const double cnt = !TAIL || nv > 0 ? (double)nv : 1.0;
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
    const RowBlock rows(rows_per_block, n, nv);
    const int64_t col = k.c0 + 4 * k.q;
    if constexpr (kPlain<T, TAIL>) {
#pragma unroll 2
        for (int r = rows.r0 + k.rl; r < rows.r1; r += k.RL) {
            const int64_t o = (int64_t)r * C + col;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f), d = g;
            if (r < nv) {
                g = masked<RELU>(dy, y, o);
                const float4 xv = ld4(x + o);
                d.x = kk.x * (g.x - mb.x - (xv.x - m.x) * is.x * mg.x);
                d.y = kk.y * (g.y - mb.y - (xv.y - m.y) * is.y * mg.y);
                d.z = kk.z * (g.z - mb.z - (xv.z - m.z) * is.z * mg.z);
                d.w = kk.w * (g.w - mb.w - (xv.w - m.w) * is.w * mg.w);
            }
            st4(dx + o, d);
            if (d_residual) st4(d_residual + o, g);
        }
    } else {
        for (int rb = rows.r0 + k.rl; rb < rows.r1 + k.rl; rb += kBatch * k.RL) {  // (rb - rl is block-uniform)
            float4 gs[kBatch];
            quad_t<T> xs[kBatch];
    #pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int64_t o = (int64_t)min(rb + u * k.RL, rows.last) * C + col;
                gs[u] = masked<RELU>(dy, y, o);
                xs[u] = ldq(x + o);
            }
    #pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int r = rb + u * k.RL;
                if (r >= rows.r1) break;
                const int64_t o = (int64_t)r * C + col;
                float4 g = gs[u];
                const float4 xv = widen(xs[u]);
                float4 d;
                d.x = kk.x * (g.x - mb.x - (xv.x - m.x) * is.x * mg.x);
                d.y = kk.y * (g.y - mb.y - (xv.y - m.y) * is.y * mg.y);
                d.z = kk.z * (g.z - mb.z - (xv.z - m.z) * is.z * mg.z);
                d.w = kk.w * (g.w - mb.w - (xv.w - m.w) * is.w * mg.w);
                if (TAIL && r >= nv) g = d = make_float4(0.f, 0.f, 0.f, 0.f);
                st4(dx + o, d);
                if (TAIL && d_residual) st4(d_residual + o, g);
            }
        }
    }
}

// The two launches of a direction.  The callers have checked every argument; fn is the name the launch error carries.  TAIL: the call
// may carry what only the sparse API has -- a row count on the device, a residual, d_residual; without it the kernels take n from the
// host and ignore those three pointers (profiles/row_bn_unify.txt, section 5: the channels-last apply passes with the run-time forms).
template <typename T, bool TAIL>
int forward(const char *fn, const T *x, const T *residual, const Launch &L, int64_t n, const int *n_dev, int C, int relu, T *y, float *saved,
            void *workspace, hipStream_t st) {
    const int rows = apply_rows(n);
    float *part = (float *)workspace;
    const unsigned cblocks = (unsigned)channel_blocks(C);
    hipLaunchKernelGGL((row_bn_stats<T, TAIL>), dim3((unsigned)groups_cap(n), cblocks), dim3(kThreads), 0, st, x, (int)n, C, part, n_dev);
    hipLaunchKernelGGL((row_bn_apply<T, TAIL>), dim3((unsigned)((n + rows - 1) / rows), cblocks), dim3(kThreads), 0, st, x, L, (int)n, C, relu, rows,
                       (const float *)part, y, saved, n_dev, residual);
    return fd::check_launch(fn);
}

template <typename T, bool TAIL>
int backward(const char *fn, const T *dy, const T *x, const T *y, const float *saved, const Launch &L, int64_t n, const int *n_dev, int C,
             int relu, T *dx, T *d_residual, float *dgamma, float *dbeta, void *workspace, hipStream_t st) {
    const int rows = apply_rows(n);
    float *part = (float *)workspace;
    const unsigned cblocks = (unsigned)channel_blocks(C);
    const auto sums = relu ? row_bn_grad_sums<T, TAIL, true> : row_bn_grad_sums<T, TAIL, false>;
    const auto apply = relu ? row_bn_grad_apply<T, TAIL, true> : row_bn_grad_apply<T, TAIL, false>;
    hipLaunchKernelGGL(sums, dim3((unsigned)groups_cap(n), cblocks), dim3(kThreads), 0, st, dy, x, y, saved, (int)n, C, part, n_dev);
    hipLaunchKernelGGL(apply, dim3((unsigned)((n + rows - 1) / rows), cblocks), dim3(kThreads), 0, st, dy, x, y, L, saved, (int)n, C, rows,
                       (const float *)part, dx, dgamma, dbeta, n_dev, d_residual);
    return fd::check_launch(fn);
}

}  // namespace row_bn
}  // namespace
