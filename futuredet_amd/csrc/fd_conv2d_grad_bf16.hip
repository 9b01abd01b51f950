// Mixed-precision training of the dense convolutions (RPN neck): what fd_conv2d_nhwc_bf16 needs around it to run under autograd.
//
// The forward is fd_conv2d_nhwc_bf16 itself; the input gradient of a stride-1 convolution is the same kernel on the flipped,
// transposed weights.  New here:
//
//   * fd_conv2d_pack_weight_dev: fd_conv2d_pack_weight on the device (the fp32 master weights change every step; the host packer
//     would put a synchronisation into each), of W (mode 0) or of W'[ci][co][ks-1-ky][ks-1-kx] = W[co][ci][ky][kx] (mode 1).
//   * fd_conv2d_wgrad_bf16: dW[co][ci][ky][kx] = sum over pixels (b, y, x) of dy[b, y, x, co] . x[b, y + ky - pad, x + kx - pad, ci]
//     on v_mfma_f32_32x32x16_bf16, M = input channel, N = output channel, the pixels are the reduction dimension.
//
// The weight gradient follows fd_deform_conv_grad.hip and fd_spconv_wgrad.h: the pixels, in their flat (b, y, x) order, are cut into
// chunks of kChunk; workgroup (chunk, kernel row ky, 32 input channels, up to 128 output channels) walks its chunk in batches of
// kBatch pixels and writes one fp32 [ci][co] partial per tap (ky, kx) to the workspace; a second kernel sums the partials of every
// (tap, ci, co) in chunk order and writes dW in the Conv2d layout.  No atomics, and kChunk is a constant: the order of every addition
// depends on the shapes only, so the result is bit-reproducible.
//
// Both MFMA operands reduce over pixels while NHWC keeps channels contiguous, so each lane needs 8 consecutive PIXELS of one channel.
// A batch is staged row-major in LDS -- images of [pixel][32 channels], 64 bytes per pixel, written with 16-byte stores exactly as
// they come from memory -- and the fragments are read with gfx950's transposed LDS read (ds_read_b64_tr_b16: per 16 lanes a block
// of 4 pixels x 16 channels, delivered channel-major).  The 4 pixels x 32 channels that a 32-lane half reads are 256 contiguous
// bytes, one bank row: conflict free, and a k-step or the second half of a fragment is an immediate offset from one per-lane base.
//
// The layers that change resolution (3 x 3 / stride 2, the 2 x 2 / stride 2 pair) take their weight gradient from the same kernel
// template with another staging address: fd_conv2d_wgrad_s2_bf16 and fd_conv2d_wgrad_2x2_bf16 at the end of this file.
//
// Out-of-image taps: the x image of kernel column kx holds, AT THE INDEX OF THE OUTPUT PIXEL p, the input pixel that tap (ky, kx)
// reads for p -- or zeros when that pixel lies outside the image (a zero halo written by the staging, one image per kx; ky is fixed
// per workgroup).  Pixels past the end of the chunk are zeros in every image.  The MFMA loop has no branch and no mask.
#include "fd_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// Pixels per workgroup and per partial: part of the summation order, not a tuning knob
constexpr int kChunk = 2048;
constexpr int kBatch = 128;   // pixels staged per LDS round (8 k-steps of 16)
constexpr int kPixB = 64;     // LDS bytes per pixel of an image: 32 channels
constexpr int kImgB = kBatch * kPixB;
constexpr int kCoBlocks = 4;  // 32-channel output blocks per workgroup: one per wave
static_assert(kChunk % kBatch == 0 && kBatch % 16 == 0 && kChunk % 64 == 0, "chunk shape");

// ---------------------------------------------------------------------------------------------------------------- weight packer
// one thread per 16-byte fragment piece: [cout'_pad/32][cin'/32][tap][ksub][lane] x 8 bf16 (fd_conv2d_pack_weight's loop nest)
__global__ void __launch_bounds__(256) conv2d_pack_weight_dev(const float *__restrict__ w, int cout, int cin, int ks, int mode, uint4 *__restrict__ dst,
                                                              int64_t n_pieces) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n_pieces) return;
    const int taps = ks * ks;
    const int cin_p = mode ? cout : cin, cout_p = mode ? cin : cout;  // the packed problem
    const int nsl = cin_p / 32;
    int64_t t = id;
    const int lane = (int)(t & 63); t >>= 6;
    const int ksub = (int)(t & 1); t >>= 1;
    const int tap = (int)(t % taps); t /= taps;
    const int s = (int)(t % nsl);
    const int nt = (int)(t / nsl);
    const int co = nt * 32 + (lane & 31);
    const int ci0 = s * 32 + ksub * 16 + 8 * (lane >> 5);
    unsigned short h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = 0.0f;
        if (co < cout_p) {
            const int ci = ci0 + j;
            // mode 1: w'[co][ci][tap] = w[ci][co][taps - 1 - tap]
            v = mode ? w[((int64_t)ci * cin + co) * taps + (taps - 1 - tap)] : w[((int64_t)co * cin + ci) * taps + tap];
        }
        unsigned u = __float_as_uint(v);
        u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even: the host packer's arithmetic
        h[j] = (unsigned short)(u >> 16);
    }
    dst[id] = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
struct WgradParams {
    int H, W, cin, cout;  // H x W: the map x
    int Ho, Wo;           // the map dy (stride 1: H x W)
    int n_pix;            // B * Ho * Wo
    int n_chunks;
};

// One MFMA operand of a k-step: for lane (channel lane & 31, k half lane >> 5) the 8 pixels pix0 + 8 (lane >> 5) + 0 .. 7 of its
// channel, from an image of [pixel][32 channels] bf16.  `base` = image + this lane's address of the first read (frag_lane_offset);
// 16-lane group g = lane >> 4 reads channels 16 (g & 1) .. + 15 of pixels 8 (g >> 1) + 4 h + 0 .. 3 in read h; lane 4 q + p of the
// group supplies the address of pixel q, channels 4 p .. 4 p + 3 and receives channel (lane & 15), pixel q in element q.
// EXEC is all ones wherever this is called (whole waves take or skip the k-step loop).
__device__ __forceinline__ unsigned frag_lane_offset(int lane) {
    return (unsigned)((8 * (lane >> 5) + ((lane & 15) >> 2)) * kPixB + ((lane >> 4) & 1) * 32 + (lane & 3) * 8);
}
__device__ __forceinline__ bf16x8 read_frag(const unsigned char *base, int byte_off) {
    typedef __attribute__((address_space(3))) s16x4 *lds_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + byte_off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + byte_off + 4 * kPixB));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// grid: (chunk, kernel row ky, (cin / 32) * ceil(cout / 128)); LDS: KS x images + kCoBlocks dy images of kImgB bytes
//
// ONE template for every geometry, not a copy per layer kind: the stride S and the padding PAD enter the staging address only -- the x
// image of tap (ky, kx) holds, at the index of dy pixel (oy, ox), the x pixel (S oy + ky - PAD, S ox + kx - PAD) or zeros.  <3, 1, 1> and
// <1, 1, 0> are the stride-1 layers (their address arithmetic and every addition are what they were); <3, 2, 1> is the 3 x 3 / stride 2
// / padding 1 layer; <2, 2, 0> is the 2 x 2 / stride 2 pair, x the fine map and dy the coarse one (fd_conv2d_strided_grad_bf16.hip).
template <int KS, int S, int PAD>
__global__ void __launch_bounds__(256) conv2d_wgrad_partial(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dy, WgradParams p,
                                                            float *__restrict__ partial) {
    constexpr int NX = kBatch * 4 / 256;              // 16-byte pieces of one x image per thread
    constexpr int NY = kBatch * 4 * kCoBlocks / 256;  // ... of the dy images
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *s_x = smem, *s_y = smem + KS * kImgB;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = blockIdx.x, ky = blockIdx.y;
    const int n_cog = (p.cout + 32 * kCoBlocks - 1) / (32 * kCoBlocks);
    const int cib = blockIdx.z / n_cog, cog = blockIdx.z - cib * n_cog;
    const int co_blocks = min(kCoBlocks, p.cout / 32 - cog * kCoBlocks);  // (uniform) 32-channel output blocks of this workgroup
    const int p0 = chunk * kChunk;
    const int n = min(kChunk, p.n_pix - p0);  // >= 1: the host launches ceil(n_pix / kChunk) chunks
    const int n_batches = (n + kBatch - 1) / kBatch;
    const int HW = p.Ho * p.Wo;
    const int row_shift = (ky - PAD) * p.W;  // (stride 1)

    uint4 rx[KS][NX], ry[NY];
    auto load_batch = [&](int bt) {
        const int b0 = bt * kBatch;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int id = tid + i * 256, pix = id >> 2, q = id & 3;
            const int pp = p0 + b0 + pix;  // the OUTPUT pixel this slot belongs to
            const bool have = b0 + pix < n;
            const int rem = pp % HW, yy = rem / p.Wo, xx = rem - yy * p.Wo;
            const int iy = S * yy + ky - PAD;
            const bool row_ok = have && (unsigned)iy < (unsigned)p.H;
            // stride 1: x and dy share their pixel index; otherwise the x pixel is addressed by (map, row, column)
            const int64_t row0 = S == 1 ? (int64_t)(pp + row_shift - xx) : ((int64_t)(pp / HW) * p.H + iy) * p.W;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const int ix = S * xx + kx - PAD;
                rx[kx][i] = make_uint4(0u, 0u, 0u, 0u);
                if (row_ok && (unsigned)ix < (unsigned)p.W)
                    rx[kx][i] = *reinterpret_cast<const uint4 *>(x + (row0 + ix) * p.cin + cib * 32 + q * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            const int id = tid + i * 256, pix = id / (4 * kCoBlocks), c = id - pix * (4 * kCoBlocks);  // c: 16-byte piece of the 128 channels
            ry[i] = make_uint4(0u, 0u, 0u, 0u);
            if (b0 + pix < n && (c >> 2) < co_blocks)
                ry[i] = *reinterpret_cast<const uint4 *>(dy + (int64_t)(p0 + b0 + pix) * p.cout + cog * (32 * kCoBlocks) + c * 8);
        }
    };
    auto store_batch = [&]() {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int id = tid + i * 256;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) *reinterpret_cast<uint4 *>(s_x + kx * kImgB + id * 16) = rx[kx][i];
        }
#pragma unroll
        for (int i = 0; i < NY; ++i) {
            const int id = tid + i * 256, pix = id / (4 * kCoBlocks), c = id - pix * (4 * kCoBlocks);
            *reinterpret_cast<uint4 *>(s_y + (c >> 2) * kImgB + pix * kPixB + (c & 3) * 16) = ry[i];
        }
    };

    f32x16 acc[KS];
#pragma unroll
    for (int kx = 0; kx < KS; ++kx)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kx][r] = 0.0f;

    const bool active = wave < co_blocks;  // (wave-uniform) this wave's output block exists
    const unsigned char *xa = s_x + frag_lane_offset(lane);
    const unsigned char *yb = s_y + wave * kImgB + frag_lane_offset(lane);

    load_batch(0);
    for (int bt = 0; bt < n_batches; ++bt) {
        store_batch();
        __syncthreads();
        if (bt + 1 < n_batches) load_batch(bt + 1);  // in flight while this batch's MFMAs run
        if (active) {
#pragma unroll
            for (int k = 0; k < kBatch / 16; ++k) {
                const bf16x8 bfrag = read_frag(yb, k * 16 * kPixB);
                bf16x8 afrag[KS];
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) afrag[kx] = read_frag(xa, kx * kImgB + k * 16 * kPixB);
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag[kx], bfrag, acc[kx], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // the partial [chunk][tap][ci][co]; D layout: col (co) = lane & 31, row (ci) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if (active) {
        const int co = (cog * kCoBlocks + wave) * 32 + (lane & 31);
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            float *dst = partial + ((int64_t)chunk * (KS * KS) + ky * KS + kx) * p.cin * p.cout;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = cib * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                dst[(int64_t)ci * p.cout + co] = acc[kx][r];
            }
        }
    }
}

// dw[co][ci][tap] (ci_major: dw[ci][co][tap]) = sum over chunks, in chunk order, of partial[chunk][tap][ci][co]
__global__ void __launch_bounds__(256) conv2d_wgrad_reduce(const float *__restrict__ partial, int taps, int cin, int cout, int n_chunks, int ci_major,
                                                           float *__restrict__ dw) {
    const int64_t total = (int64_t)taps * cin * cout;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (tap, ci, co), co fastest: coalesced reads
    if (e >= total) return;
    float s = 0.0f;
    for (int c = 0; c < n_chunks; ++c) s += partial[c * total + e];
    const int co = (int)(e % cout);
    const int64_t t = e / cout;
    const int ci = (int)(t % cin), tap = (int)(t / cin);
    dw[(ci_major ? (int64_t)ci * cout + co : (int64_t)co * cin + ci) * taps + tap] = s;
}

// the two launches of a weight gradient; p is complete and the workspace large enough
template <int KS, int S, int PAD>
void launch_wgrad(const void *x, const void *dy, const WgradParams &p, float *partial, int ci_major, float *dw, hipStream_t s) {
    const int n_cog = (p.cout + 32 * kCoBlocks - 1) / (32 * kCoBlocks);
    const dim3 grid((unsigned)p.n_chunks, (unsigned)KS, (unsigned)((p.cin / 32) * n_cog));
    const size_t lds = (size_t)(KS + kCoBlocks) * kImgB;  // 56 KB for 3 x 3: two workgroups per compute unit
    hipLaunchKernelGGL((conv2d_wgrad_partial<KS, S, PAD>), grid, dim3(256), lds, s, (const unsigned short *)x, (const unsigned short *)dy, p, partial);
    const int64_t total = (int64_t)KS * KS * p.cin * p.cout;
    hipLaunchKernelGGL(conv2d_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, KS * KS, p.cin, p.cout, p.n_chunks, ci_major,
                       dw);
}

int64_t channel_blocks(int cin, int cout) { return (int64_t)(cin / 32) * ((cout + 32 * kCoBlocks - 1) / (32 * kCoBlocks)); }

// chunks of dy pixels, or 0 where the shapes are not served
int64_t wgrad_chunks(int64_t B, int64_t Ho, int64_t Wo, int cin, int cout) {
    if (B <= 0 || Ho <= 0 || Wo <= 0 || cin <= 0 || cout <= 0 || cin % 32 || cout % 32) return 0;
    return (B * Ho * Wo + kChunk - 1) / kChunk;
}

}  // namespace

extern "C" int fd_conv2d_wgrad_bf16_chunk(void) { return kChunk; }

extern "C" size_t fd_conv2d_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin, int cout, int ks) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin % 32 || cout % 32 || (ks != 1 && ks != 3)) return 0;
    const int64_t n_pix = (int64_t)B * H * W;
    return (size_t)((n_pix + kChunk - 1) / kChunk) * ks * ks * cin * cout * sizeof(float);
}

extern "C" int fd_conv2d_pack_weight_dev(const float *w, int cout, int cin, int ks, int mode, void *dst, fd_stream_t stream) {
    FD_REQUIRE(w && dst, "fd_conv2d_pack_weight_dev: null argument");
    FD_REQUIRE(ks == 1 || ks == 3, "fd_conv2d_pack_weight_dev: ks must be 1 or 3 (got %d)", ks);
    FD_REQUIRE(mode == 0 || mode == 1, "fd_conv2d_pack_weight_dev: mode must be 0 or 1 (got %d)", mode);
    FD_REQUIRE(cout > 0 && cin > 0 && cin % 32 == 0, "fd_conv2d_pack_weight_dev: cin must be a positive multiple of 32 (got %d -> %d)", cin, cout);
    FD_REQUIRE(mode == 0 || cout % 32 == 0, "fd_conv2d_pack_weight_dev: mode 1 needs cout %% 32 == 0 (got %d)", cout);
    const size_t bytes = mode ? fd_conv2d_packed_weight_bytes(cin, cout, ks) : fd_conv2d_packed_weight_bytes(cout, cin, ks);
    const int64_t n_pieces = (int64_t)(bytes / 16);
    FD_REQUIRE(n_pieces > 0 && (n_pieces + 255) / 256 < (1ll << 31), "fd_conv2d_pack_weight_dev: bad sizes");
    hipLaunchKernelGGL(conv2d_pack_weight_dev, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, fd::as_stream(stream), w, cout, cin, ks, mode,
                       (uint4 *)dst, n_pieces);
    return fd::check_launch("fd_conv2d_pack_weight_dev");
}

extern "C" int fd_conv2d_wgrad_bf16(const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, void *workspace,
                                    size_t workspace_bytes, float *dw, fd_stream_t stream) {
    FD_REQUIRE(x && dy && dw && workspace, "fd_conv2d_wgrad_bf16: null argument");
    FD_REQUIRE(ks == 1 || ks == 3, "fd_conv2d_wgrad_bf16: ks must be 1 or 3 (got %d)", ks);
    FD_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0, "fd_conv2d_wgrad_bf16: cin and cout must be positive multiples of 32 (got %d -> %d)",
               cin, cout);
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_conv2d_wgrad_bf16: bad shape %d x %d x %d", B, H, W);
    const int64_t n_pix = (int64_t)B * H * W;
    FD_REQUIRE(n_pix + kChunk < (1ll << 31), "fd_conv2d_wgrad_bf16: maps of 2^31 pixels and more are not supported");
    const size_t need = fd_conv2d_wgrad_bf16_workspace_bytes(B, H, W, cin, cout, ks);
    FD_REQUIRE(workspace_bytes >= need, "fd_conv2d_wgrad_bf16: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    WgradParams p;
    p.H = p.Ho = H; p.W = p.Wo = W; p.cin = cin; p.cout = cout;
    p.n_pix = (int)n_pix;
    p.n_chunks = (int)((n_pix + kChunk - 1) / kChunk);
    FD_REQUIRE(channel_blocks(cin, cout) <= 65535, "fd_conv2d_wgrad_bf16: too many channel blocks (%d -> %d)", cin, cout);
    hipStream_t s = fd::as_stream(stream);
    if (ks == 3) launch_wgrad<3, 1, 1>(x, dy, p, (float *)workspace, 0, dw, s);
    else launch_wgrad<1, 1, 0>(x, dy, p, (float *)workspace, 0, dw, s);
    return fd::check_launch("fd_conv2d_wgrad_bf16");
}

// ---- the strided layers (include/futuredet_hip.h; the kernels around them: fd_conv2d_strided_grad_bf16.hip).  They live here because
// they are instantiations of conv2d_wgrad_partial, not kernels of their own.
extern "C" size_t fd_conv2d_wgrad_s2_bf16_workspace_bytes(int B, int H, int W, int cin, int cout) {
    if (H <= 0 || W <= 0) return 0;
    return (size_t)wgrad_chunks(B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, cin, cout) * 9 * cin * cout * sizeof(float);
}

extern "C" int fd_conv2d_wgrad_s2_bf16(const void *x, const void *dy, int B, int H, int W, int cin, int cout, void *workspace, size_t workspace_bytes,
                                       float *dw, fd_stream_t stream) {
    FD_REQUIRE(x && dy && dw && workspace, "fd_conv2d_wgrad_s2_bf16: null argument");
    FD_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
               "fd_conv2d_wgrad_s2_bf16: cin and cout must be positive multiples of 32 (got %d -> %d)", cin, cout);
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_conv2d_wgrad_s2_bf16: bad shape %d x %d x %d", B, H, W);
    WgradParams p;
    p.H = H; p.W = W; p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1; p.cin = cin; p.cout = cout;
    FD_REQUIRE((int64_t)B * H * W + kChunk < (1ll << 31), "fd_conv2d_wgrad_s2_bf16: maps of 2^31 pixels and more are not supported");
    const size_t need = fd_conv2d_wgrad_s2_bf16_workspace_bytes(B, H, W, cin, cout);
    FD_REQUIRE(workspace_bytes >= need, "fd_conv2d_wgrad_s2_bf16: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    p.n_pix = B * p.Ho * p.Wo;
    p.n_chunks = (p.n_pix + kChunk - 1) / kChunk;
    FD_REQUIRE(channel_blocks(cin, cout) <= 65535, "fd_conv2d_wgrad_s2_bf16: too many channel blocks (%d -> %d)", cin, cout);
    launch_wgrad<3, 2, 1>(x, dy, p, (float *)workspace, 0, dw, fd::as_stream(stream));
    return fd::check_launch("fd_conv2d_wgrad_s2_bf16");
}

extern "C" size_t fd_conv2d_wgrad_2x2_bf16_workspace_bytes(int B, int H, int W, int c_coarse, int c_fine) {
    if (H < 2 || W < 2) return 0;
    return (size_t)wgrad_chunks(B, H / 2, W / 2, c_fine, c_coarse) * 4 * c_fine * c_coarse * sizeof(float);
}

extern "C" int fd_conv2d_wgrad_2x2_bf16(const void *coarse, const void *fine, int B, int H, int W, int c_coarse, int c_fine, int fine_major,
                                        void *workspace, size_t workspace_bytes, float *dw, fd_stream_t stream) {
    FD_REQUIRE(coarse && fine && dw && workspace, "fd_conv2d_wgrad_2x2_bf16: null argument");
    FD_REQUIRE(fine_major == 0 || fine_major == 1, "fd_conv2d_wgrad_2x2_bf16: fine_major must be 0 or 1 (got %d)", fine_major);
    FD_REQUIRE(c_coarse > 0 && c_fine > 0 && c_coarse % 32 == 0 && c_fine % 32 == 0,
               "fd_conv2d_wgrad_2x2_bf16: both channel counts must be positive multiples of 32 (got %d coarse, %d fine)", c_coarse, c_fine);
    FD_REQUIRE(B > 0 && H >= 2 && W >= 2, "fd_conv2d_wgrad_2x2_bf16: bad shape %d x %d x %d (the fine map; 2 x 2 at least)", B, H, W);
    FD_REQUIRE((int64_t)B * H * W + kChunk < (1ll << 31), "fd_conv2d_wgrad_2x2_bf16: maps of 2^31 pixels and more are not supported");
    const size_t need = fd_conv2d_wgrad_2x2_bf16_workspace_bytes(B, H, W, c_coarse, c_fine);
    FD_REQUIRE(workspace_bytes >= need, "fd_conv2d_wgrad_2x2_bf16: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    WgradParams p;  // x = the fine map (M = its channels), dy = the coarse map: partial [tap][fine channel][coarse channel]
    p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2; p.cin = c_fine; p.cout = c_coarse;
    p.n_pix = B * p.Ho * p.Wo;
    p.n_chunks = (p.n_pix + kChunk - 1) / kChunk;
    FD_REQUIRE(channel_blocks(c_fine, c_coarse) <= 65535, "fd_conv2d_wgrad_2x2_bf16: too many channel blocks (%d, %d)", c_coarse, c_fine);
    launch_wgrad<2, 2, 0>(fine, coarse, p, (float *)workspace, fine_major, dw, fd::as_stream(stream));
    return fd::check_launch("fd_conv2d_wgrad_2x2_bf16");
}
