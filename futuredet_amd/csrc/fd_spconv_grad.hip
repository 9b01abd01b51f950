// Backward pass of the fp32 sparse convolution (training) for gfx950.
//
// The forward (fd_spconv.hip and its variants) is output-stationary: out[o] = sum_k in[nbr[k][o]] @ W[k].  Its gradients:
//
//   dW[k]  = sum_o in[nbr[k][o]]^T . dY[o]                          (fd_spconv_wgrad: this file's GEMM)
//   dIn[i] = sum_k dY[o_k(i)] @ W[k]^T                                (fd_spconv_apply itself, on a transposed problem:)
//            SubM (odd kernel, stride 1, pad k/2): the table is symmetric, nbr[k][o] = i <=> nbr[K-1-k][i] = o, so the
//            same nbr with weights W[K-1-k]^T;  strided: the input-stationary table inv[k][i] = o (fd_rulebook_transpose)
//            with weights W[k]^T.  Both weight forms come from fd_spconv_pack_weight_device (modes 2 and 1).
//   dFeats = the gather of dDense at the active cells                (fd_dense_gather: backward of fd_densify)
//
// fd_spconv_wgrad.  Workgroup (chunk, tap k) owns output rows [chunk * kChunk, +kChunk) of tap k: it compacts the tap's valid
// (input row, output row) pairs of the chunk into LDS with wave ballots (fixed order), then walks them in batches of kBatch
// pairs: the batch's input rows [kBatch][CIN] and gradient rows [kBatch][COUT] are staged in LDS with 16-byte loads, and each
// wave runs v_mfma_f32_16x16x4_f32 over them -- A = in rows (M = input channel), B = dY rows (N = output channel), the pairs
// are the reduction dimension, four per MFMA.  The (CIN/16) x (COUT/16) output tiles are split over the four waves; shapes
// with fewer than four tiles split the pairs instead and add the waves' partial tiles in wave order.  The workgroup's
// [CIN][COUT] partial goes to the caller's workspace; a second kernel sums the partials of a tap in chunk order.  The chunk
// size is a constant, so the summation order -- and the result, bit for bit -- depends only on the rulebook, never on the
// launch.  No atomics.
#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxTaps = 27;
constexpr int kChunk = fd::kSpconvWgradChunk;  // output rows per workgroup (and per partial): part of the summation order, not a tuning knob
constexpr int kBatch = 32;   // pairs staged per LDS round (8 MFMA k-steps)
constexpr int kPadF = 16;    // LDS row padding in floats: the four 16-lane groups of a read land on different bank sets

template <int CIN, int COUT>
__global__ void __launch_bounds__(256) wgrad_partial(const float *__restrict__ in, int64_t n_in, const float *__restrict__ dy,
                                                     const int *__restrict__ nbr, int64_t nbr_stride, int n_out,
                                                     const int *__restrict__ n_out_dev, int n_chunks, float *__restrict__ partial) {
    constexpr int MT = CIN / 16, NT = COUT / 16, T = MT * NT;
    constexpr int NWT = T < 4 ? T : 4;          // wave groups that split the tiles
    constexpr int PS = 4 / NWT;                 // pair splits per tile group
    constexpr int MS = MT < NWT ? MT : NWT;     // tile groups along M
    constexpr int NS = NWT / MS;                // ... and along N
    constexpr int MA = MT / MS, NA = NT / NS;   // tiles of a wave along M and N
    constexpr int XS = CIN + kPadF, YS = COUT + kPadF;
    static_assert(MT % MS == 0 && NT % NS == 0, "tile split");

    __shared__ int s_stage_i[kChunk], s_stage_o[kChunk];
    __shared__ int s_pi[kChunk], s_po[kChunk];
    __shared__ int s_cnt[4];
    __shared__ __attribute__((aligned(16))) float s_x[kBatch * XS];
    __shared__ __attribute__((aligned(16))) float s_y[kBatch * YS];

    const int chunk = blockIdx.x, k = blockIdx.y;
    const int n = fd::device_count(n_out, n_out_dev);
    const int row0 = chunk * kChunk;
    if (row0 >= n) return;  // the reduction reads only the chunks below the count
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // 1. compaction: wave w takes rows [w * kChunk / 4, +kChunk / 4) in steps of 64, in row order
    constexpr int RPW = kChunk / 4;
    int cnt = 0;
    for (int s = 0; s < RPW; s += 64) {
        const int o = row0 + wave * RPW + s + lane;
        int i = -1;
        if (o < n) i = nbr[(int64_t)k * nbr_stride + o];
        const bool ok = i >= 0 && i < n_in;
        const unsigned long long m = __ballot(ok);
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (ok) {
            s_stage_i[wave * RPW + pos] = i;
            s_stage_o[wave * RPW + pos] = o;
        }
        cnt += __popcll(m);
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_cnt[w];
        total += s_cnt[w];
    }
    for (int j = lane; j < cnt; j += 64) {
        s_pi[base + j] = s_stage_i[wave * RPW + j];
        s_po[base + j] = s_stage_o[wave * RPW + j];
    }
    __syncthreads();

    // 2. batches of kBatch pairs through the matrix core
    const int tg = wave / PS, ps = wave % PS;
    const int mg = tg % MS, ng = tg / MS;
    const int lr = lane & 15, lq = lane >> 4;
    f32x4 acc[MA][NA];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int p0 = 0; p0 < total; p0 += kBatch) {
        constexpr int X4 = CIN / 4, Y4 = COUT / 4;
        for (int t = threadIdx.x; t < kBatch * X4; t += 256) {
            const int p = t / X4, c4 = t - p * X4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p0 + p < total) v = reinterpret_cast<const float4 *>(in + (int64_t)s_pi[p0 + p] * CIN)[c4];
            *reinterpret_cast<float4 *>(&s_x[p * XS + c4 * 4]) = v;
        }
        for (int t = threadIdx.x; t < kBatch * Y4; t += 256) {
            const int p = t / Y4, c4 = t - p * Y4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p0 + p < total) v = reinterpret_cast<const float4 *>(dy + (int64_t)s_po[p0 + p] * COUT)[c4];
            *reinterpret_cast<float4 *>(&s_y[p * YS + c4 * 4]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = ps; ks < kBatch / 4; ks += PS) {
            const int p = ks * 4 + lq;
            float av[MA], bv[NA];
#pragma unroll
            for (int a = 0; a < MA; ++a) av[a] = s_x[p * XS + (mg + MS * a) * 16 + lr];
#pragma unroll
            for (int b = 0; b < NA; ++b) bv[b] = s_y[p * YS + (ng + NS * b) * 16 + lr];
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // 3. pair splits: waves ps > 0 hand their tiles to wave ps == 0 of their group through LDS (s_x is free now)
    if (PS > 1) {
        static_assert(PS == 1 || 3 * 64 * 4 * MA * NA <= kBatch * XS, "reduction scratch");
        if (ps > 0) {
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_x[((((tg * (PS - 1) + ps - 1) * MA + a) * NA + b) * 4 + r) * 64 + lane] = acc[a][b][r];
        }
        __syncthreads();
        if (ps > 0) return;
        for (int q = 1; q < PS; ++q)
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][b][r] += s_x[((((tg * (PS - 1) + q - 1) * MA + a) * NA + b) * 4 + r) * 64 + lane];
    }

    // 4. the partial: D layout col = lane & 15, row = 4 * (lane >> 4) + r
    float *dst = partial + ((int64_t)k * n_chunks + chunk) * (CIN * COUT);
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((mg + MS * a) * 16 + lq * 4 + r) * COUT + (ng + NS * b) * 16 + lr] = acc[a][b][r];
}

// dW[k][e] = sum over the tap's chunks, in chunk order
__global__ void __launch_bounds__(256) wgrad_reduce(const float *__restrict__ partial, int K, int cc, int n_out, const int *__restrict__ n_out_dev,
                                                    int n_chunks, float *__restrict__ dw) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)K * cc) return;
    const int k = (int)(t / cc), e = (int)(t - (int64_t)k * cc);
    const int n = fd::device_count(n_out, n_out_dev);
    const int used = (n + kChunk - 1) / kChunk;
    float s = 0.f;
    for (int c = 0; c < used; ++c) s += partial[((int64_t)k * n_chunks + c) * cc + e];
    dw[t] = s;
}

template <int CIN, int COUT>
void launch_wgrad(const float *in, int64_t n_in, const float *dy, const int *nbr, int64_t nbr_stride, int K, int n_out, const int *n_out_dev,
                  int n_chunks, float *partial, hipStream_t stream) {
    hipLaunchKernelGGL((wgrad_partial<CIN, COUT>), dim3((unsigned)n_chunks, (unsigned)K), dim3(256), 0, stream, in, n_in, dy, nbr, nbr_stride,
                       n_out, n_out_dev, n_chunks, partial);
}

__global__ void __launch_bounds__(256) rulebook_transpose(const int *__restrict__ nbr, int64_t nbr_stride, int n_out, const int *__restrict__ n_out_dev,
                                                          int64_t n_in, int *__restrict__ inv, int64_t inv_stride) {
    const int k = blockIdx.y;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= fd::device_count(n_out, n_out_dev)) return;
    const int i = nbr[(int64_t)k * nbr_stride + o];
    if (i >= 0 && i < n_in) inv[(int64_t)k * inv_stride + i] = o;  // unique: o -> o * stride - pad + k is injective per tap
}

// the fp32 fragment order of fd_spconv_pack_weight (fd_spconv.hip) for W'(k, a, b), a < ci (input channel), b < co
__global__ void __launch_bounds__(256) pack_weight_f32(const float *__restrict__ w, int K, int cin, int cout, int mode, int ci, int co, int c32,
                                                       float *__restrict__ dst) {
    const int64_t main_elems = (int64_t)K * ci * co;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= main_elems * (c32 ? 2 : 1)) return;
    int k, a, b;
    if (t < main_elems) {  // [K][ci / 16][co / 16][lane][4]
        const int NC = ci / 16, NB = co / 16;
        int64_t r = t;
        const int j = (int)(r & 3); r >>= 2;
        const int lane = (int)(r & 63); r >>= 6;
        const int nb = (int)(r % NB); r /= NB;
        const int c = (int)(r % NC); r /= NC;
        k = (int)r;
        a = 16 * c + 4 * (lane >> 4) + j;
        b = 16 * nb + (lane & 15);
    } else {  // 32 -> 32: [K][ci / 8][lane][4], channel 8 c + 4 (lane / 32) + j, output channel lane % 32
        int64_t r = t - main_elems;
        const int j = (int)(r & 3); r >>= 2;
        const int lane = (int)(r & 63); r >>= 6;
        const int c = (int)(r % (ci / 8)); r /= (ci / 8);
        k = (int)r;
        a = 8 * c + 4 * (lane >> 5) + j;
        b = lane & 31;
    }
    float v;
    if (mode == 0) v = w[((int64_t)k * cin + a) * cout + b];
    else {
        const int ks = mode == 2 ? K - 1 - k : k;  // transposed: W'(k, a, b) = W(k', b, a)
        v = w[((int64_t)ks * cin + b) * cout + a];
    }
    dst[t] = v;
}

__global__ void __launch_bounds__(256) dense_gather(const float *__restrict__ dense, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int D,
                                                    const int *__restrict__ coords, int64_t n_rows, const int *__restrict__ n_dev, int c,
                                                    float *__restrict__ feats) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_rows * c) return;
    const int64_t row = t / c;
    const int ch = (int)(t - row * c);
    const int64_t n = n_dev ? (int64_t)fd::device_count((int)n_rows, n_dev) : n_rows;
    float v = 0.f;
    if (row < n) {
        const int4 q = reinterpret_cast<const int4 *>(coords)[row];  // (b, z, y, x)
        v = dense[q.x * sb + ((int64_t)ch * D + q.y) * sc + q.z * sy + q.w * sx];
    }
    feats[t] = v;
}

inline bool ok_channels(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

}  // namespace

namespace fd {
void spconv_wgrad_reduce(const float *partial, int K, int cc, int n_out, const int *n_out_dev, int n_chunks, float *dw, hipStream_t stream) {
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)(((int64_t)K * cc + 255) / 256)), dim3(256), 0, stream, partial, K, cc, n_out, n_out_dev, n_chunks, dw);
}
}  // namespace fd

extern "C" size_t fd_spconv_wgrad_workspace_bytes(int K, int64_t n_out, int cin, int cout) {
    if (K <= 0 || n_out < 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)K * (size_t)((n_out + kChunk - 1) / kChunk) * cin * cout * sizeof(float);
}

extern "C" int fd_spconv_wgrad(const float *in_feats, int64_t n_in, const float *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                               const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(K >= 1 && K <= kMaxTaps, "fd_spconv_wgrad: K must be in [1,27]");
    FD_REQUIRE(ok_channels(cin) && ok_channels(cout), "fd_spconv_wgrad: channels must be 16, 32, 64 or 128 (got %d -> %d)", cin, cout);
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31) && n_in >= 0, "fd_spconv_wgrad: bad sizes");
    FD_REQUIRE(dw, "fd_spconv_wgrad: null dw");
    hipStream_t stream = fd::as_stream(stream_);
    const int64_t cc = (int64_t)cin * cout;
    if (n_out == 0 || n_in == 0)  // no pairs: dW = 0
        return fd::fill_words(dw, 0u, (size_t)(K * cc), stream) == 0 ? fd::check_launch("fd_spconv_wgrad(zero)") : FD_ELAUNCH;
    FD_REQUIRE(in_feats && dy && nbr && workspace, "fd_spconv_wgrad: null argument");
    FD_REQUIRE(workspace_bytes >= fd_spconv_wgrad_workspace_bytes(K, n_out, cin, cout), "fd_spconv_wgrad: workspace too small");
    const int n_chunks = (int)((n_out + kChunk - 1) / kChunk);
    float *partial = (float *)workspace;
    const int key = cin * 1000 + cout;
#define FD_W(CI, CO) \
    case CI * 1000 + CO: launch_wgrad<CI, CO>(in_feats, n_in, dy, nbr, nbr_stride, K, (int)n_out, n_out_dev, n_chunks, partial, stream); break;
    switch (key) {
        FD_W(16, 16) FD_W(16, 32) FD_W(16, 64) FD_W(16, 128)
        FD_W(32, 16) FD_W(32, 32) FD_W(32, 64) FD_W(32, 128)
        FD_W(64, 16) FD_W(64, 32) FD_W(64, 64) FD_W(64, 128)
        FD_W(128, 16) FD_W(128, 32) FD_W(128, 64) FD_W(128, 128)
        default: break;
    }
#undef FD_W
    fd::spconv_wgrad_reduce(partial, K, (int)cc, (int)n_out, n_out_dev, n_chunks, dw, stream);
    return fd::check_launch("fd_spconv_wgrad");
}

extern "C" int fd_rulebook_transpose(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, int64_t n_in,
                                     int32_t *inv, int64_t inv_stride, fd_stream_t stream_) {
    FD_REQUIRE(K >= 1 && K <= kMaxTaps, "fd_rulebook_transpose: K must be in [1,27]");
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31) && n_in >= 0 && n_in <= inv_stride, "fd_rulebook_transpose: bad sizes");
    FD_REQUIRE(inv, "fd_rulebook_transpose: null inv");
    hipStream_t stream = fd::as_stream(stream_);
    if (fd::fill_words(inv, 0xffffffffu, (size_t)(K * inv_stride), stream) != 0) return fd::check_launch("fd_rulebook_transpose(fill)");
    if (n_out > 0) {
        FD_REQUIRE(nbr, "fd_rulebook_transpose: null nbr");
        hipLaunchKernelGGL(rulebook_transpose, dim3((unsigned)((n_out + 255) / 256), (unsigned)K), dim3(256), 0, stream, nbr, nbr_stride, (int)n_out,
                           n_out_dev, n_in, inv, inv_stride);
    }
    return fd::check_launch("fd_rulebook_transpose");
}

extern "C" int fd_spconv_pack_weight_device(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream_) {
    FD_REQUIRE(w_kio && wpacked, "fd_spconv_pack_weight_device: null argument");
    FD_REQUIRE(K >= 1 && K <= kMaxTaps, "fd_spconv_pack_weight_device: K must be in [1,27]");
    FD_REQUIRE(cin % 16 == 0 && cout % 16 == 0 && cin >= 16 && cin <= 128 && cout >= 16 && cout <= 128,
               "fd_spconv_pack_weight_device: channels must be multiples of 16 in [16,128] (got %d -> %d)", cin, cout);
    FD_REQUIRE(mode >= 0 && mode <= 2, "fd_spconv_pack_weight_device: mode must be 0 (W[k]), 1 (W[k]^T) or 2 (W[K-1-k]^T)");
    const int ci = mode ? cout : cin, co = mode ? cin : cout;
    const fd::SpconvWeightLayout lay = fd::spconv_weight_layout(K, ci, co, 0);  // the kernel writes base, then c32 right behind it
    const int c32 = lay.c32.bytes != 0;
    const int64_t n = (int64_t)(lay.total / sizeof(float));
    hipLaunchKernelGGL(pack_weight_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fd::as_stream(stream_), w_kio, K, cin, cout, mode, ci, co, c32,
                       (float *)wpacked);
    return fd::check_launch("fd_spconv_pack_weight_device");
}

extern "C" int fd_dense_gather(const float *dense, int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x, int D, const int32_t *coords,
                               int64_t n_rows, const int32_t *n_dev, int c, float *feats, fd_stream_t stream_) {
    FD_REQUIRE(c >= 1 && D >= 1 && n_rows >= 0 && n_rows < (1ll << 31), "fd_dense_gather: bad sizes");
    if (n_rows == 0) return FD_OK;
    FD_REQUIRE(dense && coords && feats, "fd_dense_gather: null argument");
    const int64_t n = n_rows * c;
    hipLaunchKernelGGL(dense_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fd::as_stream(stream_), dense, stride_b, stride_c, stride_y,
                       stride_x, D, coords, n_rows, n_dev, c, feats);
    return fd::check_launch("fd_dense_gather");
}
