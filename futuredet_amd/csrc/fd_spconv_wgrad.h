// The weight gradient of the sparse convolution, dW[k] = sum_o in[nbr[k][o]]^T . dY[o]: the one kernel skeleton and the one
// entry-point body of fd_spconv_wgrad (fp32 rows, fd_spconv_grad.hip) and fd_spconv_wgrad_bf16 (bf16 rows, fd_spconv_grad_bf16.hip).
//
// Workgroup (chunk, tap k) owns output rows [chunk * kSpconvWgradChunk, +kSpconvWgradChunk) of tap k: it compacts the tap's valid
// (input row, output row) pairs of the chunk into LDS with wave ballots, in row order, then walks them in batches: the batch's
// input rows [pairs][CIN] and gradient rows [pairs][COUT] are staged row-major in LDS with 16-byte loads (zero rows past the end of
// the list, so every lane works under a full EXEC mask), and each wave runs MFMAs over them -- A = in rows (M = input channel),
// B = dY rows (N = output channel), the pairs are the reduction dimension.  The (CIN/16) x (COUT/16) output tiles are split over
// the four waves; shapes with fewer than four tiles split the k-steps of a batch instead and add the waves' tiles in wave order.
// The workgroup's fp32 [CIN][COUT] partial goes to the caller's workspace; a second kernel (spconv_wgrad_reduce) sums a tap's
// partials in chunk order.  No atomics.  The chunk size is a constant, so the order of every addition -- pairs in compacted row
// order, k-steps ks = ps, ps + PS, ..., the hand-over q = 1 ... PS - 1, then the chunks -- and with it the result, bit for bit,
// depends only on the rulebook, never on the launch.
//
// What differs between the row types is a traits struct `Rows`:
//   Elem, Piece           the row element (float / unsigned short) and the 16-byte vector a row is staged in (float4 / uint4)
//   kStepPairs            pairs per MFMA k-step
//   batch_pairs(PS)       pairs staged per LDS round
//   row_bytes(C)          LDS row stride of a [pairs][C] image
//   Frag, fragment<ROWB>(), mma()   one operand fragment of a k-step (16 channels from c0) read from an image, and the MFMA
//   shape(cin, cout), kShapes, kLimit2GB   what the entry point accepts
// The staging loops and the k-step loop are written out in the kernel, not behind helpers that take the images as pointers: with
// such helpers the compiler merged the two staging loops and scheduled the fragment reads differently (measured 1-2 % slower on
// 32 -> 32 with tools/spconv_grad_bench.py).  As written, the bf16 instantiations compile to the instruction sequence they had as a
// kernel of their own, 16 -> 16 apart (its hand-over scratch moved into the staging buffer).
#pragma once
#include "fd_common.h"

namespace fd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Output rows per workgroup and per partial: part of the summation order, not a tuning knob; the second kernel derives the number
// of used chunks from it
constexpr int kSpconvWgradChunk = 512;
// fd_spconv_grad.hip: dw[k][e] = the tap's per-chunk partials [K][n_chunks][cc], summed in chunk order
void spconv_wgrad_reduce(const float *partial, int K, int cc, int n_out, const int *n_out_dev, int n_chunks, float *dw, hipStream_t stream);

template <int CIN, int COUT>
struct WgradSplit {
    static constexpr int MT = CIN / 16, NT = COUT / 16, T = MT * NT;
    static constexpr int NWT = T < 4 ? T : 4;         // wave groups that split the tiles
    static constexpr int PS = 4 / NWT;                // k-step splits per tile group
    static constexpr int MS = MT < NWT ? MT : NWT;    // tile groups along M
    static constexpr int NS = NWT / MS;               // ... and along N
    static constexpr int MA = MT / MS, NA = NT / NS;  // tiles of a wave along M and N
    static_assert(MT % MS == 0 && NT % NS == 0, "tile split");
};

template <typename Rows, int CIN, int COUT>
__global__ void __launch_bounds__(256) wgrad_partial(const typename Rows::Elem *__restrict__ in, int64_t n_in, const typename Rows::Elem *__restrict__ dy,
                                                     const int *__restrict__ nbr, int64_t nbr_stride, int n_out,
                                                     const int *__restrict__ n_out_dev, int n_chunks, float *__restrict__ partial) {
    using S = WgradSplit<CIN, COUT>;
    constexpr int PS = S::PS, MS = S::MS, NS = S::NS, MA = S::MA, NA = S::NA;
    constexpr int kChunk = kSpconvWgradChunk;
    constexpr int KB = Rows::batch_pairs(PS);
    constexpr int XB = Rows::row_bytes(CIN), YB = Rows::row_bytes(COUT);

    __shared__ int s_stage_i[kChunk], s_stage_o[kChunk];
    __shared__ int s_pi[kChunk], s_po[kChunk];
    __shared__ int s_cnt[4];
    __shared__ __attribute__((aligned(16))) unsigned char s_x[KB * XB];
    __shared__ __attribute__((aligned(16))) unsigned char s_y[KB * YB];

    const int chunk = blockIdx.x, k = blockIdx.y;
    const int n = device_count(n_out, n_out_dev);
    const int row0 = chunk * kChunk;
    if (row0 >= n) return;  // (uniform) the reduction reads only the chunks below the count
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

    // 2. batches of KB pairs through the matrix core (total, and with it every branch below, is uniform: EXEC stays all ones)
    const int tg = wave / PS, ps = wave % PS;
    const int mg = tg % MS, ng = tg / MS;
    const int lr = lane & 15, lq = lane >> 4;
    f32x4 acc[MA][NA];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NA; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int p0 = 0; p0 < total; p0 += KB) {
        constexpr int X8 = CIN * (int)sizeof(typename Rows::Elem) / 16, Y8 = COUT * (int)sizeof(typename Rows::Elem) / 16;  // 16-byte pieces of a row
        for (int t = threadIdx.x; t < KB * X8; t += 256) {
            const int p = t / X8, c8 = t - p * X8;
            typename Rows::Piece v = {};  // rows past the end of the list: zeros
            if (p0 + p < total) v = reinterpret_cast<const typename Rows::Piece *>(in + (int64_t)s_pi[p0 + p] * CIN)[c8];
            *reinterpret_cast<typename Rows::Piece *>(&s_x[p * XB + c8 * 16]) = v;
        }
        for (int t = threadIdx.x; t < KB * Y8; t += 256) {
            const int p = t / Y8, c8 = t - p * Y8;
            typename Rows::Piece v = {};
            if (p0 + p < total) v = reinterpret_cast<const typename Rows::Piece *>(dy + (int64_t)s_po[p0 + p] * COUT)[c8];
            *reinterpret_cast<typename Rows::Piece *>(&s_y[p * YB + c8 * 16]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = ps; ks < KB / Rows::kStepPairs; ks += PS) {
            typename Rows::Frag av[MA], bv[NA];
#pragma unroll
            for (int a = 0; a < MA; ++a) av[a] = Rows::template fragment<XB>(s_x, ks, (mg + MS * a) * 16, lane);
#pragma unroll
            for (int b = 0; b < NA; ++b) bv[b] = Rows::template fragment<YB>(s_y, ks, (ng + NS * b) * 16, lane);
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b) acc[a][b] = Rows::mma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }

    // 3. k-step splits: waves ps > 0 hand their tiles to wave ps == 0 of their group through LDS (s_x is free after the loop's last
    //    barrier), which adds them in wave order
    if constexpr (PS > 1) {
        static_assert(S::NWT * (PS - 1) * MA * NA * 256 * sizeof(float) <= sizeof(s_x), "hand-over scratch");
        float *s_red = reinterpret_cast<float *>(s_x);
        if (ps > 0) {
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_red[((((tg * (PS - 1) + ps - 1) * MA + a) * NA + b) * 4 + r) * 64 + lane] = acc[a][b][r];
        }
        __syncthreads();
        if (ps > 0) return;
        for (int q = 1; q < PS; ++q)
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][b][r] += s_red[((((tg * (PS - 1) + q - 1) * MA + a) * NA + b) * 4 + r) * 64 + lane];
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

// one fp32 [cin][cout] partial per (chunk, tap)
inline size_t spconv_wgrad_workspace_bytes(int K, int64_t n_out, int cin, int cout) {
    if (K <= 0 || n_out < 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)K * (size_t)((n_out + kSpconvWgradChunk - 1) / kSpconvWgradChunk) * cin * cout * sizeof(float);
}

// the body of an entry point, under its own name
template <typename Rows>
int spconv_wgrad(const char *who, const void *in_feats, int64_t n_in, const void *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                 const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(K >= 1 && K <= kSpconvMaxTaps, "%s: K must be in [1,27]", who);
    FD_REQUIRE(Rows::shape(cin, cout), "%s: channels must be %s (got %d -> %d)", who, Rows::kShapes, cin, cout);
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31) && n_in >= 0, "%s: bad sizes", who);
    FD_REQUIRE(!Rows::kLimit2GB || (n_in * cin * 2 < (1ll << 31) && n_out * cout * 2 < (1ll << 31)),
               "%s: feature matrices of 2 GB and more are not supported (%lld x %d, %lld x %d bf16)", who, (long long)n_in, cin, (long long)n_out, cout);
    FD_REQUIRE(dw, "%s: null dw", who);
    hipStream_t stream = as_stream(stream_);
    const int64_t cc = (int64_t)cin * cout;
    if (n_out == 0 || n_in == 0)  // no pairs: dW = 0
        return fill_words(dw, 0u, (size_t)(K * cc), stream) == 0 ? check_launch(who) : FD_ELAUNCH;
    FD_REQUIRE(in_feats && dy && nbr && workspace, "%s: null argument", who);
    FD_REQUIRE(workspace_bytes >= spconv_wgrad_workspace_bytes(K, n_out, cin, cout), "%s: workspace too small", who);
    const int n_chunks = (int)((n_out + kSpconvWgradChunk - 1) / kSpconvWgradChunk);
    float *partial = (float *)workspace;
    typedef const typename Rows::Elem *rows_t;
#define FD_W(CI, CO)                                                                                                                                \
    case CI * 1000 + CO:                                                                                                                            \
        if constexpr (Rows::shape(CI, CO))                                                                                                          \
            hipLaunchKernelGGL((wgrad_partial<Rows, CI, CO>), dim3((unsigned)n_chunks, (unsigned)K), dim3(256), 0, stream, (rows_t)in_feats, n_in, \
                               (rows_t)dy, nbr, nbr_stride, (int)n_out, n_out_dev, n_chunks, partial);                                             \
        break;
    switch (cin * 1000 + cout) {
        FD_W(16, 16) FD_W(16, 32) FD_W(16, 64) FD_W(16, 128)
        FD_W(32, 16) FD_W(32, 32) FD_W(32, 64) FD_W(32, 128)
        FD_W(64, 16) FD_W(64, 32) FD_W(64, 64) FD_W(64, 128)
        FD_W(128, 16) FD_W(128, 32) FD_W(128, 64) FD_W(128, 128)
        default: break;
    }
#undef FD_W
    spconv_wgrad_reduce(partial, K, (int)cc, (int)n_out, n_out_dev, n_chunks, dw, stream);
    return check_launch(who);
}

}  // namespace fd
