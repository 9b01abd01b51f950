// Mixed-precision training of the sparse convolution on gfx950: the bf16 weight gradient and the device-side bf16 weight packer.
//
// bf16 rows, fp32 master weights.  The forward is fd_spconv_apply(dtype = 1); the input gradient is the same call on the transposed
// problem (fd_spconv_grad.hip's header); this file adds what was missing:
//
// fd_spconv_wgrad_bf16.  dW[k] = sum_o in[nbr[k][o]]^T . dY[o] with bf16 rows and an fp32 result.  The decomposition is
// fd_spconv_wgrad's, so the result is a function of the rulebook only: workgroup (chunk, tap k) owns output rows
// [chunk * kChunk, +kChunk) of tap k, compacts the tap's valid (input row, output row) pairs with wave ballots in row order, walks
// them in batches, writes its [CIN][COUT] fp32 partial to the caller's workspace, and fd_spconv_wgrad's second kernel sums a tap's
// partials in chunk order.  No atomics.
//
// The reduction runs on v_mfma_f32_16x16x32_bf16: A = in rows (M = input channel), B = dY rows (N = output channel), the PAIRS
// are the k dimension, 32 per MFMA.  Both operands are therefore needed pair-major while the rows arrive channel-major: a batch's
// rows are staged row-major in LDS with 16-byte loads and the fragments come out of ds_read_b64_tr_b16, which hands lane i of a
// 16-lane group column i of a 4-row x 16-column block.  Element j = 4 h + q of the fragment of lane group g is pair 16 h + 4 g + q
// of the k-step (the same map for A and B, and the MFMA sums over all of them, so any bijection is right).  With that map a
// 32-lane half of a read touches 8 consecutive rows, 32 bytes of each; LDS rows are 32 * odd bytes long (16 channels: 32; else the
// row plus 32 bytes of padding), so those eight rows start 8 * odd banks apart and the half covers all 64 banks once: the
// transposed reads are conflict-free for every channel count (bank = (byte / 4) % 64, conflicts per 32-lane half).  Every lane
// supplies an in-bounds address under a full EXEC mask -- the last batch of a (chunk, tap) is padded with zero rows, no lane is
// switched off.  The (CIN/16) x (COUT/16) output tiles are split over the four waves; shapes with fewer tiles than waves split
// the k-steps of a batch instead and add the waves' tiles in wave order.
//
// fd_spconv_pack_weight_device_bf16.  The bytes fd_spconv_pack_weight writes for dtype 1 (base section, tap-pair section for 16
// input channels, window section for 64 -> 64 and 128 -> 128; the same round-to-nearest-even) from fp32 weights in device memory,
// of W[k], W[k]^T or W[K-1-k]^T.  One launch, no host round trip.
#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kMaxTaps = 27;
constexpr int kChunk = fd::kSpconvWgradChunk;  // output rows per workgroup (and per partial), shared with fd_spconv_wgrad and its second kernel

// LDS row length in bytes of a [pairs][C] bf16 image: 32 * odd (see the header)
constexpr int lds_row_bytes(int c) { return c == 16 ? 32 : c * 2 + 32; }

// one operand fragment: pairs [32 ks, +32) of the image at `img`, channels [c0, c0 + 16)
template <int ROWB>
__device__ __forceinline__ bf16x8 tr_fragment(const unsigned char *img, int ks, int c0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const unsigned char *a = img + (ks * 32 + 4 * g + q) * ROWB + (c0 + 4 * p) * 2;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(a + 16 * ROWB));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

template <int CIN, int COUT>
__global__ void __launch_bounds__(256) wgrad_bf16_partial(const unsigned short *__restrict__ in, int64_t n_in, const unsigned short *__restrict__ dy,
                                                          const int *__restrict__ nbr, int64_t nbr_stride, int n_out,
                                                          const int *__restrict__ n_out_dev, int n_chunks, float *__restrict__ partial) {
    constexpr int MT = CIN / 16, NT = COUT / 16, T = MT * NT;
    constexpr int NWT = T < 4 ? T : 4;          // wave groups that split the tiles
    constexpr int PS = 4 / NWT;                 // k-step splits per tile group
    constexpr int MS = MT < NWT ? MT : NWT;     // tile groups along M
    constexpr int NS = NWT / MS;                // ... and along N
    constexpr int MA = MT / MS, NA = NT / NS;   // tiles of a wave along M and N
    constexpr int KB = 32 * (PS > 2 ? PS : 2);  // pairs staged per LDS round: every wave has a k-step in it
    constexpr int XB = lds_row_bytes(CIN), YB = lds_row_bytes(COUT);
    constexpr int RED = PS > 1 ? NWT * (PS - 1) * MA * NA * 256 : 1;
    static_assert(MT % MS == 0 && NT % NS == 0, "tile split");

    __shared__ int s_stage_i[kChunk], s_stage_o[kChunk];
    __shared__ int s_pi[kChunk], s_po[kChunk];
    __shared__ int s_cnt[4];
    __shared__ __attribute__((aligned(16))) unsigned char s_x[KB * XB];
    __shared__ __attribute__((aligned(16))) unsigned char s_y[KB * YB];
    __shared__ float s_red[RED];

    const int chunk = blockIdx.x, k = blockIdx.y;
    const int n = fd::device_count(n_out, n_out_dev);
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
        constexpr int X8 = CIN / 8, Y8 = COUT / 8;  // 16-byte pieces of a row
        for (int t = threadIdx.x; t < KB * X8; t += 256) {
            const int p = t / X8, c8 = t - p * X8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);  // rows past the end of the list: zeros
            if (p0 + p < total) v = reinterpret_cast<const uint4 *>(in + (int64_t)s_pi[p0 + p] * CIN)[c8];
            *reinterpret_cast<uint4 *>(&s_x[p * XB + c8 * 16]) = v;
        }
        for (int t = threadIdx.x; t < KB * Y8; t += 256) {
            const int p = t / Y8, c8 = t - p * Y8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (p0 + p < total) v = reinterpret_cast<const uint4 *>(dy + (int64_t)s_po[p0 + p] * COUT)[c8];
            *reinterpret_cast<uint4 *>(&s_y[p * YB + c8 * 16]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = ps; ks < KB / 32; ks += PS) {
            bf16x8 av[MA], bv[NA];
#pragma unroll
            for (int a = 0; a < MA; ++a) av[a] = tr_fragment<XB>(s_x, ks, (mg + MS * a) * 16, lane);
#pragma unroll
            for (int b = 0; b < NA; ++b) bv[b] = tr_fragment<YB>(s_y, ks, (ng + NS * b) * 16, lane);
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NA; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }

    // 3. k-step splits: waves ps > 0 hand their tiles to wave ps == 0 of their group, which adds them in wave order
    if constexpr (PS > 1) {
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

template <int CIN, int COUT>
void launch_wgrad_bf16(const void *in, int64_t n_in, const void *dy, const int *nbr, int64_t nbr_stride, int K, int n_out, const int *n_out_dev,
                       int n_chunks, float *partial, hipStream_t stream) {
    hipLaunchKernelGGL((wgrad_bf16_partial<CIN, COUT>), dim3((unsigned)n_chunks, (unsigned)K), dim3(256), 0, stream, (const unsigned short *)in, n_in,
                       (const unsigned short *)dy, nbr, nbr_stride, n_out, n_out_dev, n_chunks, partial);
}

__device__ inline unsigned short to_bf16_rne(float v) {  // fd_spconv_pack_weight's tobf
    unsigned u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// element t of the dtype-1 buffer of fd_spconv_pack_weight for W'(k, a, b), a < ci (input channel), b < co
__global__ void __launch_bounds__(256) pack_weight_bf16(const float *__restrict__ w, int K, int cin, int cout, int mode, int ci, int co,
                                                        int64_t base_elems, int64_t pair_elems, int64_t win_elems, unsigned short *__restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= base_elems + pair_elems + win_elems) return;
    int k, a, b;
    if (t < base_elems && ci >= 32) {  // [K][ci / 32][co / 16][lane][8]
        const int NC = ci / 32, NB = co / 16;
        int64_t r = t;
        const int j = (int)(r & 7); r >>= 3;
        const int lane = (int)(r & 63); r >>= 6;
        const int nb = (int)(r % NB); r /= NB;
        const int c = (int)(r % NC); r /= NC;
        k = (int)r;
        a = 32 * c + 8 * (lane >> 4) + j;
        b = 16 * nb + (lane & 15);
    } else if (t < base_elems) {  // 16 input channels: [K][co / 16][lane][4]
        const int NB = co / 16;
        int64_t r = t;
        const int j = (int)(r & 3); r >>= 2;
        const int lane = (int)(r & 63); r >>= 6;
        const int nb = (int)(r % NB); r /= NB;
        k = (int)r;
        a = 4 * (lane >> 4) + j;
        b = 16 * nb + (lane & 15);
    } else if (t < base_elems + pair_elems) {  // tap pairs [ceil(K / 2)][co / 16][lane][8]; taps past K are zeros
        const int NB = co / 16;
        int64_t r = t - base_elems;
        const int j = (int)(r & 7); r >>= 3;
        const int lane = (int)(r & 63); r >>= 6;
        const int nb = (int)(r % NB); r /= NB;
        const int q = lane >> 4;
        k = 2 * (int)r + (q >> 1);
        a = 8 * (q & 1) + j;
        b = 16 * nb + (lane & 15);
    } else {  // window section [K][ci / SC][SC / 16][co / 32][lane][8] (fd_spconv_bf16win.hip)
        const int SC = ci < 64 ? ci : 64, H = ci / SC, KS = SC / 16, CB = co / 32;
        int64_t r = t - base_elems - pair_elems;
        const int j = (int)(r & 7); r >>= 3;
        const int lane = (int)(r & 63); r >>= 6;
        const int cb = (int)(r % CB); r /= CB;
        const int s = (int)(r % KS); r /= KS;
        const int h = (int)(r % H); r /= H;
        k = (int)r;
        a = SC * h + 16 * s + 8 * (lane >> 5) + j;
        b = 32 * cb + (lane & 31);
    }
    unsigned short v = 0;
    if (k < K) {
        if (mode == 0) v = to_bf16_rne(w[((int64_t)k * cin + a) * cout + b]);
        else {
            const int ks = mode == 2 ? K - 1 - k : k;  // transposed: W'(k, a, b) = W(k', b, a)
            v = to_bf16_rne(w[((int64_t)ks * cin + b) * cout + a]);
        }
    }
    dst[t] = v;
}

inline bool wgrad_bf16_shape(int cin, int cout) {
    const int key = cin * 1000 + cout;
    return key == 16016 || key == 16032 || key == 32032 || key == 32064 || key == 64064 || key == 64128 || key == 128128;
}

}  // namespace

extern "C" size_t fd_spconv_wgrad_bf16_workspace_bytes(int K, int64_t n_out, int cin, int cout) {
    if (K <= 0 || n_out < 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)K * (size_t)((n_out + kChunk - 1) / kChunk) * cin * cout * sizeof(float);
}

extern "C" int fd_spconv_wgrad_bf16(const void *in_feats, int64_t n_in, const void *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                                    const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes,
                                    fd_stream_t stream_) {
    FD_REQUIRE(K >= 1 && K <= kMaxTaps, "fd_spconv_wgrad_bf16: K must be in [1,27]");
    FD_REQUIRE(wgrad_bf16_shape(cin, cout),
               "fd_spconv_wgrad_bf16: channels must be 16->16, 16->32, 32->32, 32->64, 64->64, 64->128 or 128->128 (got %d -> %d)", cin, cout);
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31) && n_in >= 0, "fd_spconv_wgrad_bf16: bad sizes");
    FD_REQUIRE(n_in * cin * 2 < (1ll << 31) && n_out * cout * 2 < (1ll << 31),
               "fd_spconv_wgrad_bf16: feature matrices of 2 GB and more are not supported (%lld x %d, %lld x %d bf16)", (long long)n_in, cin,
               (long long)n_out, cout);
    FD_REQUIRE(dw, "fd_spconv_wgrad_bf16: null dw");
    hipStream_t stream = fd::as_stream(stream_);
    const int64_t cc = (int64_t)cin * cout;
    if (n_out == 0 || n_in == 0)  // no pairs: dW = 0
        return fd::fill_words(dw, 0u, (size_t)(K * cc), stream) == 0 ? fd::check_launch("fd_spconv_wgrad_bf16(zero)") : FD_ELAUNCH;
    FD_REQUIRE(in_feats && dy && nbr && workspace, "fd_spconv_wgrad_bf16: null argument");
    FD_REQUIRE(workspace_bytes >= fd_spconv_wgrad_bf16_workspace_bytes(K, n_out, cin, cout), "fd_spconv_wgrad_bf16: workspace too small");
    const int n_chunks = (int)((n_out + kChunk - 1) / kChunk);
    float *partial = (float *)workspace;
#define FD_W(CI, CO) \
    case CI * 1000 + CO: launch_wgrad_bf16<CI, CO>(in_feats, n_in, dy, nbr, nbr_stride, K, (int)n_out, n_out_dev, n_chunks, partial, stream); break;
    switch (cin * 1000 + cout) {
        FD_W(16, 16) FD_W(16, 32) FD_W(32, 32) FD_W(32, 64) FD_W(64, 64) FD_W(64, 128) FD_W(128, 128)
        default: break;
    }
#undef FD_W
    fd::spconv_wgrad_reduce(partial, K, (int)cc, (int)n_out, n_out_dev, n_chunks, dw, stream);
    return fd::check_launch("fd_spconv_wgrad_bf16");
}

extern "C" int fd_spconv_pack_weight_device_bf16(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream_) {
    FD_REQUIRE(w_kio && wpacked, "fd_spconv_pack_weight_device_bf16: null argument");
    FD_REQUIRE(K >= 1 && K <= kMaxTaps, "fd_spconv_pack_weight_device_bf16: K must be in [1,27]");
    FD_REQUIRE(cin % 16 == 0 && cout % 16 == 0 && cin >= 16 && cin <= 128 && cout >= 16 && cout <= 128,
               "fd_spconv_pack_weight_device_bf16: channels must be multiples of 16 in [16,128] (got %d -> %d)", cin, cout);
    FD_REQUIRE(mode >= 0 && mode <= 2, "fd_spconv_pack_weight_device_bf16: mode must be 0 (W[k]), 1 (W[k]^T) or 2 (W[K-1-k]^T)");
    const int ci = mode ? cout : cin, co = mode ? cin : cout;
    FD_REQUIRE(ci == 16 || ci % 32 == 0, "fd_spconv_pack_weight_device_bf16: bf16 needs 16 input channels or a multiple of 32 (got %d)", ci);
    const fd::SpconvWeightLayout lay = fd::spconv_weight_layout(K, ci, co, 1);  // base, then pair or win right behind it
    const int64_t n = (int64_t)(lay.total / 2);
    hipLaunchKernelGGL(pack_weight_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fd::as_stream(stream_), w_kio, K, cin, cout, mode, ci, co,
                       (int64_t)(lay.base.bytes / 2), (int64_t)(lay.pair.bytes / 2), (int64_t)(lay.win.bytes / 2), (unsigned short *)wpacked);
    return fd::check_launch("fd_spconv_pack_weight_device_bf16");
}
