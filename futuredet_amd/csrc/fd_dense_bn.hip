// Training-mode BatchNorm2d over the maps x [B, C, H, W] (fp32, NCHW contiguous) of the dense half (RPN, CenterHead), fused with the
// ReLU that follows it: y = act(gamma[c] (x - mean[c]) invstd[c] + beta[c]), and its backward.  The sibling of fd_sparse_bn.hip for
// planes: there the reduction runs across rows, here along the contiguous planes.  P = H W values per plane, N = B P per channel.
//
// Statistics.  Every plane (b, c) is cut into pieces = ceil(P / kChunk) chunks of kChunk (= FD_DENSE_BN_CHUNK) elements (the last one
// shorter).  A channel's B pieces chunks are ordered by (b, piece); consecutive chunks form ng groups of G = ceil(chunks / cap) chunks,
// cap = clamp(ceil(kTargetBlocks / C), 1, kMaxGroups) -- a group may cross a sample boundary.  Pass 1, one workgroup per (channel,
// group): per chunk, the mean (summed relative to the chunk's first element, so a mean that is large against the spread costs no
// digits) and M2_j = sum (x - mean_j)^2 centred at that mean, from the chunk held in registers (x is read once); the group's chunks are
// merged in chunk order, in double, with Chan's rule (mean += d n_j / N', M2 += M2_j + d^2 N n_j / N').  Pass 2, element-wise over
// plane pieces: EVERY workgroup re-sums its own channel's (at most kMaxGroups) group partials in group order, in double --
// mean = sum n_g mean_g / N, then M2 = sum [M2_g + n_g (mean_g - mean)^2] -- and then writes its elements.  The workgroup of the first
// piece of plane (0, c) also writes mean / invstd for the backward and updates channel c's running statistics (unbiased variance);
// workgroup 0 alone increments num_batches_tracked.  Two launches, no atomics: chunk, group and piece boundaries depend on (B, C, P)
// only, so two runs give the same bits.
//
// Backward.  g = dy where y > 0 (y is the forward's output: the ReLU mask), x^ = (x - mean) invstd.  Pass 1: the sums of g and g x^ per
// chunk, added per group in chunk order in double; pass 2: every workgroup re-sums its channel's group partials in group order,
// dx = gamma invstd (g - dbeta / N - x^ dgamma / N).
//
// Thread layout.  A chunk is kChunk / 256 elements per thread.  P % 4 == 0 (every plane 16-byte aligned): thread t takes the float4
// t, t + 256, ... of the chunk, all traffic is 16-byte loads and stores.  Any other P: thread t takes the elements t, t + 256, ...
// one by one (plane starts are then unaligned).  A chunk's 256 per-thread sums are added by a butterfly within each wave and the four
// wave totals in wave order: a fixed tree.  Pass 2 cuts a plane into pieces of kApplyChunks chunks or more; the cut does not touch
// the sums.
#include "fd_common.h"

namespace {

constexpr int kChunk = FD_DENSE_BN_CHUNK;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = kChunk / kThreads;  // elements of a chunk per thread
constexpr int kMaxGroups = 64;           // group partials per channel at most: every pass-2 workgroup re-sums them
constexpr int kTargetBlocks = 1024;      // pass-1 workgroups aimed at: C * cap
constexpr int kApplyChunks = 4;          // chunks per pass-2 workgroup at least
constexpr int kMaxApplyPieces = 64;      // pass-2 workgroups per plane at most
constexpr int kMaxC = 4096;
constexpr int64_t kMaxB = 1 << 16, kMaxP = 1 << 30, kMaxPlanes = 1 << 24, kMaxChunks = 1 << 29;
static_assert(kChunk % (4 * kThreads) == 0 && kPer % 4 == 0, "chunk");

// The cut of one channel's N = B P values: chunks, chunks per group, groups.  Host and device agree on it.
struct Cut {
    int pieces, nchunks, G, ng;
    __host__ __device__ Cut(int64_t B, int C, int64_t P) {
        pieces = (int)((P + kChunk - 1) / kChunk);
        nchunks = (int)(B * pieces);
        int cap = (kTargetBlocks + C - 1) / C;
        cap = cap > kMaxGroups ? kMaxGroups : cap;
        G = (nchunks + cap - 1) / cap;
        ng = (nchunks + G - 1) / G;
    }
    // elements in the chunks in front of chunk j
    __host__ __device__ int64_t before(int j, int64_t P) const { return (int64_t)(j / pieces) * P + (int64_t)(j % pieces) * kChunk; }
    __host__ __device__ int64_t count(int g, int64_t P) const {
        const int j0 = g * G, j1 = j0 + G < nchunks ? j0 + G : nchunks;
        return before(j1, P) - before(j0, P);
    }
};

inline bool sizes_ok(int64_t B, int C, int64_t P) {
    return C >= 1 && C <= kMaxC && B >= 1 && B <= kMaxB && P >= 1 && P <= kMaxP && B * C <= kMaxPlanes &&
           B * ((P + kChunk - 1) / kChunk) <= kMaxChunks;
}
// chunks per pass-2 workgroup, pass-2 workgroups per plane
inline int apply_span(int64_t P) {
    const int pieces = (int)((P + kChunk - 1) / kChunk), s = (pieces + kMaxApplyPieces - 1) / kMaxApplyPieces;
    return s > kApplyChunks ? s : kApplyChunks;
}
inline int apply_pieces(int64_t P) {
    const int pieces = (int)((P + kChunk - 1) / kChunk), s = apply_span(P);
    return (pieces + s - 1) / s;
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// Offset within the chunk of a thread's i-th element: float4s (VEC) or single elements, strided by the workgroup.
template <bool VEC>
__device__ __forceinline__ int elem(int i) {
    return VEC ? (((i >> 2) * kThreads + (int)threadIdx.x) << 2) + (i & 3) : i * kThreads + (int)threadIdx.x;
}

// A thread's kPer elements of the chunk p[0, L); VEC: L % 4 == 0 and p 16-byte aligned.  Elements at or beyond L read as 0.
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float *__restrict__ p, int L, float (&v)[kPer]) {
    if (VEC) {
#pragma unroll
        for (int i = 0; i < kPer; i += 4) {
            const int e = elem<true>(i);
            const float4 t = e < L ? ld4(p + e) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[i] = t.x;
            v[i + 1] = t.y;
            v[i + 2] = t.z;
            v[i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int e = elem<false>(i);
            v[i] = e < L ? p[e] : 0.f;
        }
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // both partners add the same two values: every lane ends with the same bits
    return v;
}
// The workgroup's total, the same bits in every thread.  One barrier: callers alternate between two slots s, so a slot is rewritten
// only after a later barrier than the one its readers passed.
__device__ __forceinline__ float block_sum(float v, float *s) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s[0] + s[1]) + s[2]) + s[3];
}

// chunk j of channel c: its start and its length
struct ChunkAt {
    int64_t off;
    int L;
    __device__ __forceinline__ ChunkAt(const Cut &cut, int j, int c, int C, int64_t P) {
        const int b = j / cut.pieces, piece = j % cut.pieces;
        const int64_t e0 = (int64_t)piece * kChunk;
        off = ((int64_t)b * C + c) * P + e0;
        L = (int)(P - e0 < kChunk ? P - e0 : kChunk);
    }
};

// ---- forward pass 1: part[c][g] = (mean_g, M2_g)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) dbn_stats(const float *__restrict__ x, int64_t B, int C, int64_t P, float *__restrict__ part) {
    __shared__ float s_red[2][kWaves];
    const Cut cut(B, C, P);
    const int c = blockIdx.y, g = blockIdx.x;
    if (g >= cut.ng) return;  // block-uniform
    const int j0 = g * cut.G, j1 = min(j0 + cut.G, cut.nchunks);
    double N = 0.0, mean = 0.0, M2 = 0.0;  // the group so far (every thread carries the same values)
    float cur[kPer], nxt[kPer];
    ChunkAt at(cut, j0, c, C, P);
    load_chunk<VEC>(x + at.off, at.L, cur);
    float pivot = x[at.off];
    for (int j = j0; j < j1; ++j) {
        const int L = at.L;
        float pivot_n = 0.f;
        if (j + 1 < j1) {  // the next chunk's loads are in flight during this chunk's sums
            at = ChunkAt(cut, j + 1, c, C, P);
            load_chunk<VEC>(x + at.off, at.L, nxt);
            pivot_n = x[at.off];
        }
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (elem<VEC>(i) < L) s += cur[i] - pivot;
        const float nb = (float)L;
        const float mb = pivot + block_sum(s, s_red[0]) / nb;
        s = 0.f;
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (elem<VEC>(i) < L) {
                const float d = cur[i] - mb;
                s += d * d;
            }
        const float m2 = block_sum(s, s_red[1]);
        {  // Chan's rule, chunk j onto the group so far
            const double nbd = (double)nb, N1 = N + nbd, d = (double)mb - mean;
            mean += d * (nbd / N1);
            M2 += (double)m2 + d * d * (N * nbd / N1);
            N = N1;
        }
        if (j + 1 < j1) {
#pragma unroll
            for (int i = 0; i < kPer; ++i) cur[i] = nxt[i];
            pivot = pivot_n;
        }
    }
    if (threadIdx.x == 0) {
        float *dst = part + ((size_t)c * cut.ng + g) * 2;
        dst[0] = (float)mean;
        dst[1] = (float)M2;
    }
}

// ---- forward pass 2: the channel's statistics from its group partials, then y for the workgroup's piece of its plane
template <bool VEC>
__global__ void __launch_bounds__(kThreads) dbn_apply(const float *__restrict__ x, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, int64_t B, int C, int64_t P, int relu, float eps,
                                                       double momentum, int span, int apieces, const float *__restrict__ part,
                                                       float *__restrict__ y, float *__restrict__ saved, float *__restrict__ running_mean,
                                                       float *__restrict__ running_var, long long *__restrict__ num_batches_tracked) {
    __shared__ double s_n[kMaxGroups], s_a[kMaxGroups], s_b[kMaxGroups];
    const Cut cut(B, C, P);
    const int plane = blockIdx.x / apieces, pi = blockIdx.x % apieces, c = plane % C;
    const float *pc = part + (size_t)c * cut.ng * 2;
    const double cnt = (double)(B * P);
    const int t = threadIdx.x;
    if (t < cut.ng) {
        const double n = (double)cut.count(t, P);
        s_n[t] = n;
        s_a[t] = n * (double)pc[2 * t];
    }
    __syncthreads();
    double mu = 0.0;
    for (int g = 0; g < cut.ng; ++g) mu += s_a[g];
    mu /= cnt;
    if (t < cut.ng) {
        const double d = (double)pc[2 * t] - mu;
        s_b[t] = (double)pc[2 * t + 1] + s_n[t] * d * d;
    }
    __syncthreads();
    double M2 = 0.0;
    for (int g = 0; g < cut.ng; ++g) M2 += s_b[g];
    const double var = M2 > 0.0 ? M2 / cnt : 0.0;
    const float m = (float)mu;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * invstd, be = beta[c];
    if (pi == 0 && plane < C && t == 0) {  // the first piece of plane (0, c)
        saved[c] = m;
        saved[C + c] = invstd;
        const double unbiased = var * (cnt / (cnt - 1.0));
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
        if (blockIdx.x == 0) num_batches_tracked[0] += 1;
    }
    const int64_t e0 = (int64_t)pi * span * kChunk, e1 = e0 + (int64_t)span * kChunk < P ? e0 + (int64_t)span * kChunk : P;
    const float *xp = x + (int64_t)plane * P;
    float *yp = y + (int64_t)plane * P;
    if (VEC) {
#pragma unroll 4
        for (int64_t e = e0 + 4 * t; e < e1; e += 4 * kThreads) {
            const float4 xv = ld4(xp + e);
            float4 v;
            v.x = (xv.x - m) * sc + be;
            v.y = (xv.y - m) * sc + be;
            v.z = (xv.z - m) * sc + be;
            v.w = (xv.w - m) * sc + be;
            if (relu) {
                v.x = v.x > 0.f ? v.x : 0.f;
                v.y = v.y > 0.f ? v.y : 0.f;
                v.z = v.z > 0.f ? v.z : 0.f;
                v.w = v.w > 0.f ? v.w : 0.f;
            }
            st4(yp + e, v);
        }
    } else {
#pragma unroll 4
        for (int64_t e = e0 + t; e < e1; e += kThreads) {
            float v = (xp[e] - m) * sc + be;
            if (relu) v = v > 0.f ? v : 0.f;
            yp[e] = v;
        }
    }
}

// ---- backward pass 1: part[c][g] = (sum g, sum g x^)
template <bool VEC>
__global__ void __launch_bounds__(kThreads) dbn_grad_sums(const float *__restrict__ dy, const float *__restrict__ x,
                                                           const float *__restrict__ y, const float *__restrict__ saved, int64_t B, int C,
                                                           int64_t P, int relu, float *__restrict__ part) {
    __shared__ float s_red[2][2][kWaves];
    const Cut cut(B, C, P);
    const int c = blockIdx.y, g = blockIdx.x;
    if (g >= cut.ng) return;  // block-uniform
    const int j0 = g * cut.G, j1 = min(j0 + cut.G, cut.nchunks);
    const float m = saved[c], is = saved[C + c];
    double db = 0.0, dg = 0.0;  // the group so far
    for (int j = j0; j < j1; ++j) {
        const ChunkAt at(cut, j, c, C, P);
        float gv[kPer], xv[kPer], yv[kPer];
        load_chunk<VEC>(dy + at.off, at.L, gv);
        load_chunk<VEC>(x + at.off, at.L, xv);
        if (relu) load_chunk<VEC>(y + at.off, at.L, yv);
        float sb = 0.f, sg = 0.f;
#pragma unroll
        for (int i = 0; i < kPer; ++i)
            if (elem<VEC>(i) < at.L) {
                const float gi = relu ? (yv[i] > 0.f ? gv[i] : 0.f) : gv[i];
                sb += gi;
                sg += gi * ((xv[i] - m) * is);
            }
        // both totals behind one barrier; the slot pair alternates with the chunk
        float(*s)[kWaves] = s_red[(j - j0) & 1];
        sb = wave_sum(sb);
        sg = wave_sum(sg);
        if ((threadIdx.x & 63) == 0) {
            s[0][threadIdx.x >> 6] = sb;
            s[1][threadIdx.x >> 6] = sg;
        }
        __syncthreads();
        db += (double)(((s[0][0] + s[0][1]) + s[0][2]) + s[0][3]);
        dg += (double)(((s[1][0] + s[1][1]) + s[1][2]) + s[1][3]);
    }
    if (threadIdx.x == 0) {
        float *dst = part + ((size_t)c * cut.ng + g) * 2;
        dst[0] = (float)db;
        dst[1] = (float)dg;
    }
}

// ---- backward pass 2: dbeta / dgamma from the channel's group partials, then dx for the workgroup's piece of its plane
template <bool VEC>
__global__ void __launch_bounds__(kThreads) dbn_grad_apply(const float *__restrict__ dy, const float *__restrict__ x,
                                                            const float *__restrict__ y, const float *__restrict__ gamma,
                                                            const float *__restrict__ saved, int64_t B, int C, int64_t P, int relu,
                                                            int span, int apieces, const float *__restrict__ part, float *__restrict__ dx,
                                                            float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double s_a[kMaxGroups], s_b[kMaxGroups];
    const Cut cut(B, C, P);
    const int plane = blockIdx.x / apieces, pi = blockIdx.x % apieces, c = plane % C;
    const float *pc = part + (size_t)c * cut.ng * 2;
    const double cnt = (double)(B * P);
    const int t = threadIdx.x;
    if (t < cut.ng) {
        s_a[t] = (double)pc[2 * t];
        s_b[t] = (double)pc[2 * t + 1];
    }
    __syncthreads();
    double db = 0.0, dg = 0.0;
    for (int g = 0; g < cut.ng; ++g) {
        db += s_a[g];
        dg += s_b[g];
    }
    const float m = saved[c], is = saved[C + c];
    const float k = gamma[c] * is, mb = (float)(db / cnt), mg = (float)(dg / cnt);
    if (pi == 0 && plane < C && t == 0) {  // the first piece of plane (0, c)
        dbeta[c] = (float)db;
        dgamma[c] = (float)dg;
    }
    const int64_t e0 = (int64_t)pi * span * kChunk, e1 = e0 + (int64_t)span * kChunk < P ? e0 + (int64_t)span * kChunk : P;
    const int64_t po = (int64_t)plane * P;
    const float *dyp = dy + po, *xp = x + po, *yp = relu ? y + po : nullptr;
    float *dxp = dx + po;
    if (VEC) {
#pragma unroll 2
        for (int64_t e = e0 + 4 * t; e < e1; e += 4 * kThreads) {
            float4 gq = ld4(dyp + e);
            const float4 xq = ld4(xp + e);
            if (relu) {
                const float4 yq = ld4(yp + e);
                gq.x = yq.x > 0.f ? gq.x : 0.f;
                gq.y = yq.y > 0.f ? gq.y : 0.f;
                gq.z = yq.z > 0.f ? gq.z : 0.f;
                gq.w = yq.w > 0.f ? gq.w : 0.f;
            }
            float4 d;
            d.x = k * (gq.x - mb - (xq.x - m) * is * mg);
            d.y = k * (gq.y - mb - (xq.y - m) * is * mg);
            d.z = k * (gq.z - mb - (xq.z - m) * is * mg);
            d.w = k * (gq.w - mb - (xq.w - m) * is * mg);
            st4(dxp + e, d);
        }
    } else {
#pragma unroll 2
        for (int64_t e = e0 + t; e < e1; e += kThreads) {
            float gi = dyp[e];
            if (relu) gi = yp[e] > 0.f ? gi : 0.f;
            dxp[e] = k * (gi - mb - (xp[e] - m) * is * mg);
        }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int fd_dense_bn_chunk(void) { return kChunk; }

extern "C" size_t fd_dense_bn_workspace_bytes(int64_t B, int C, int64_t P) {
    if (!sizes_ok(B, C, P) || B * P < 2) return 0;
    // the groups a channel can have, not the groups it has: monotone in B and P
    const int cap = (kTargetBlocks + C - 1) / C < kMaxGroups ? (kTargetBlocks + C - 1) / C : kMaxGroups;
    const int64_t chunks = B * ((P + kChunk - 1) / kChunk);
    return fd::align_up((size_t)C * (size_t)(chunks < cap ? chunks : cap) * 2 * sizeof(float), 256);
}

#define FD_DBN_CHECK(fn)                                                                                                                \
    FD_REQUIRE(C >= 1 && C <= kMaxC, fn ": unsupported C %d: 1 to %d channels", C, kMaxC);                                              \
    FD_REQUIRE(sizes_ok(B, C, P), fn ": B or P out of range (B %lld in [1, %lld], P %lld in [1, %lld], B C <= %lld)", (long long)B,      \
               (long long)kMaxB, (long long)P, (long long)kMaxP, (long long)kMaxPlanes);                                                 \
    FD_REQUIRE(B * P >= 2, fn ": expected more than 1 value per channel (B P = %lld)", (long long)(B * P));                             \
    FD_REQUIRE(relu == 0 || relu == 1, fn ": relu must be 0 or 1 (got %d)", relu);                                                       \
    FD_REQUIRE(workspace, fn ": null workspace");                                                                                        \
    FD_REQUIRE(workspace_bytes >= fd_dense_bn_workspace_bytes(B, C, P), fn ": workspace too small (%zu bytes, %zu needed)",              \
               workspace_bytes, fd_dense_bn_workspace_bytes(B, C, P));                                                                   \
    FD_REQUIRE(aligned16(workspace), fn ": the workspace must be 16-byte aligned")

extern "C" int fd_dense_bn_train_forward(const float *x, const float *gamma, const float *beta, int64_t B, int C, int64_t P, int relu,
                                         float eps, double momentum, float *y, float *saved, float *running_mean, float *running_var,
                                         int64_t *num_batches_tracked, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(x && gamma && beta, "fd_dense_bn_train_forward: null x, gamma or beta");
    FD_REQUIRE(y && saved, "fd_dense_bn_train_forward: null y or saved");
    FD_REQUIRE(running_mean && running_var && num_batches_tracked, "fd_dense_bn_train_forward: null running statistics");
    FD_DBN_CHECK("fd_dense_bn_train_forward");
    FD_REQUIRE(eps > 0.f, "fd_dense_bn_train_forward: eps must be > 0");
    FD_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "fd_dense_bn_train_forward: momentum must be in [0, 1]");
    FD_REQUIRE(aligned16(x) && aligned16(y), "fd_dense_bn_train_forward: x and y must be 16-byte aligned");
    hipStream_t st = fd::as_stream(stream_);
    const Cut cut(B, C, P);
    const int span = apply_span(P), apieces = apply_pieces(P);
    float *part = (float *)workspace;
    const dim3 g1((unsigned)cut.ng, (unsigned)C), g2((unsigned)(B * C * apieces));
    long long *nbt = (long long *)num_batches_tracked;
    if (P % 4 == 0) {
        hipLaunchKernelGGL(dbn_stats<true>, g1, dim3(kThreads), 0, st, x, B, C, P, part);
        hipLaunchKernelGGL(dbn_apply<true>, g2, dim3(kThreads), 0, st, x, gamma, beta, B, C, P, relu, eps, momentum, span, apieces,
                           (const float *)part, y, saved, running_mean, running_var, nbt);
    } else {
        hipLaunchKernelGGL(dbn_stats<false>, g1, dim3(kThreads), 0, st, x, B, C, P, part);
        hipLaunchKernelGGL(dbn_apply<false>, g2, dim3(kThreads), 0, st, x, gamma, beta, B, C, P, relu, eps, momentum, span, apieces,
                           (const float *)part, y, saved, running_mean, running_var, nbt);
    }
    return fd::check_launch("fd_dense_bn_train_forward");
}

extern "C" int fd_dense_bn_train_backward(const float *dy, const float *x, const float *y, const float *gamma, const float *saved, int64_t B,
                                          int C, int64_t P, int relu, float *dx, float *dgamma, float *dbeta, void *workspace,
                                          size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(dy && x && gamma && saved, "fd_dense_bn_train_backward: null dy, x, gamma or saved");
    FD_REQUIRE(y || !relu, "fd_dense_bn_train_backward: null y (the ReLU mask)");
    FD_REQUIRE(dx && dgamma && dbeta, "fd_dense_bn_train_backward: null dx, dgamma or dbeta");
    FD_DBN_CHECK("fd_dense_bn_train_backward");
    FD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(dx), "fd_dense_bn_train_backward: dy, x, y and dx must be 16-byte aligned");
    hipStream_t st = fd::as_stream(stream_);
    const Cut cut(B, C, P);
    const int span = apply_span(P), apieces = apply_pieces(P);
    float *part = (float *)workspace;
    const dim3 g1((unsigned)cut.ng, (unsigned)C), g2((unsigned)(B * C * apieces));
    if (P % 4 == 0) {
        hipLaunchKernelGGL(dbn_grad_sums<true>, g1, dim3(kThreads), 0, st, dy, x, y, saved, B, C, P, relu, part);
        hipLaunchKernelGGL(dbn_grad_apply<true>, g2, dim3(kThreads), 0, st, dy, x, y, gamma, saved, B, C, P, relu, span, apieces,
                           (const float *)part, dx, dgamma, dbeta);
    } else {
        hipLaunchKernelGGL(dbn_grad_sums<false>, g1, dim3(kThreads), 0, st, dy, x, y, saved, B, C, P, relu, part);
        hipLaunchKernelGGL(dbn_grad_apply<false>, g2, dim3(kThreads), 0, st, dy, x, y, gamma, saved, B, C, P, relu, span, apieces,
                           (const float *)part, dx, dgamma, dbeta);
    }
    return fd::check_launch("fd_dense_bn_train_backward");
}
