// Mixed-precision training of the dense convolutions that change resolution (RPN neck): the 3 x 3 / stride 2 / padding 1 convolution that
// opens a down-sampling stage, the ConvTranspose2d(2, stride 2) deblock and the Conv2d(2, stride 2) deblock of the PointPillars neck.
// bf16 NHWC operands, channel counts multiples of 32, fp32 accumulation on v_mfma_f32_32x32x16_bf16, one rounding to bf16; no atomics,
// nothing is read back to the host.
//
// What already exists: the forward of the stride-2 layer (fd_conv2d_nhwc_bf16) and "up2" -- four 1 x 1 convolutions that write the four
// pixels (2 y + dy, 2 x + dx) through fd_conv2d_nhwc_bf16's pixel placement: the forward of ConvTranspose2d(2, 2) and the input gradient
// of Conv2d(2, 2).  New here:
//
//   * fd_conv2d_s2_dgrad_bf16: the input gradient of the stride-2 layer, by parity phase.  dX[iy, ix] sums dY[(iy + 1 - ky) / 2,
//     (ix + 1 - kx) / 2] . W[ky, kx] over the taps whose quotients are integers: an even row takes ky = 1 only, an odd row ky = 0 and 2.
//     So the 2 x 2 block of dX pixels (2 m + {0, 1}, 2 n + {0, 1}) reads the dY cells (m + {0, 1}, n + {0, 1}) through 1 + 2 + 2 + 4 = 9
//     taps (a stride-1 convolution of the zero-inserted dY would spend 36).  A workgroup owns an 8 x 16 tile of cells, stages the 9 x 17
//     cell patch of every 32-channel slice of dY in LDS (fd_conv2d.hip's image: 80-byte pixel pitch, ds_read_b128 fragments) and keeps
//     the four phases' accumulators at once: the four A fragments of a k-step serve all nine taps.
//   * fd_conv2d_down2_bf16: "down2", the forward of Conv2d(2, 2) and the input gradient of ConvTranspose2d(2, 2) -- a 1 x 1 GEMM with
//     K = 4 C over the space-to-depth view of the fine map.  In NHWC the four taps of a coarse pixel are two contiguous runs of 2 C
//     channels (fine rows 2 y and 2 y + 1, from column 2 x), so the view costs nothing: a 32-channel slice of K is 64 contiguous bytes.
//   * fd_conv2d_pack_weight_2x2_dev: the packed weights of both, from the fp32 master weight on the device.  ONE entry point and one
//     launch rather than a device-side rearrangement followed by mode-0 packs of fd_conv2d_pack_weight_dev: the rearranged copy would be
//     a second pass over the weights and a buffer of its own every step, and up2 would take four more launches.
//
// The weight gradients of these layers are instantiations of conv2d_wgrad_partial and live next to it (fd_conv2d_grad_bf16.hip).
#include "fd_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int TH = 8, TW = 16;  // dY cells (dgrad) per workgroup: M = 128
constexpr int PIXB = 80;        // LDS bytes per staged pixel: 64 of data + 16 of padding (fd_conv2d.hip, store_slice)

__device__ inline unsigned short f2bf(float v) {
    unsigned u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// One 32 x 32 accumulator per (wave, j): the wave's 32 pixels x channel block j, rounded to bf16 into s_out [128 pixels][NT channels].
// D layout: col (channel) = lane & 31, row (pixel) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <int WNT>
__device__ __forceinline__ void acc_to_lds(const f32x16 (&acc)[WNT], unsigned short *s_out, int wave, int lane) {
    constexpr int NT = WNT * 32;
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) s_out[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * NT + j * 32 + (lane & 31)] = f2bf(acc[j][r]);
}

// ---------------------------------------------------------------------------------------------------------------- stride-2 dgrad
struct DgradParams {
    int B, H, W, Ho, Wo, cin, cout;  // of the forward layer: dY [B, Ho, Wo, cout] -> dX [B, H, W, cin]
    int tiles_x, tiles_y;
};

// grid: (tiles of 8 x 16 cells x B, cin / (32 WNT)); 256 threads: wave w owns cells 32 w .. 32 w + 31 of the tile (two rows of 16)
template <int WNT>
__global__ void __launch_bounds__(256) conv2d_s2_dgrad(const unsigned short *__restrict__ dy, const bf16x8 *__restrict__ wp, unsigned short *__restrict__ dx,
                                                       DgradParams p) {
    constexpr int PH = TH + 1, PW = TW + 1, PP = PH * PW;  // the cell patch: one halo row below, one halo column to the right
    constexpr int NCHUNK16 = PP * 4, NLOAD = (NCHUNK16 + 255) / 256;
    constexpr int NT = WNT * 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * PP * PIXB];
    static_assert(2 * PP * PIXB >= TH * TW * NT * 2, "the epilogue transposes one phase through the patch buffers");

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = blockIdx.x;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y, b = t / p.tiles_y;
    const int m0 = ty * TH, n0 = tx * TW;
    const int nslices = p.cout / 32;  // the reduction runs over dY's channels

    uint4 stage[NLOAD];
    auto load_slice = [&](int s) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int id = tid + i * 256;
            stage[i] = make_uint4(0u, 0u, 0u, 0u);
            if (id < NCHUNK16) {
                const int pix = id >> 2, q = id & 3;
                const int cy = m0 + pix / PW, cx = n0 + pix % PW;
                if (cy < p.Ho && cx < p.Wo)  // a cell past the map contributes nothing
                    stage[i] = *reinterpret_cast<const uint4 *>(dy + (((int64_t)b * p.Ho + cy) * p.Wo + cx) * p.cout + s * 32 + q * 8);
            }
        }
    };
    auto store_slice = [&](int buf) {
        unsigned char *dst = smem + buf * (PP * PIXB);
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int id = tid + i * 256;
            if (id < NCHUNK16) *reinterpret_cast<uint4 *>(dst + (id >> 2) * PIXB + ((id & 3) << 4)) = stage[i];
        }
    };

    f32x16 acc[4][WNT];  // [phase 2 py + px]
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int j = 0; j < WNT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ph][j][r] = 0.0f;

    // A fragments: lane -> cell (lane & 31) of the wave, k half = lane >> 5; cell (m + sy, n + sx) is an immediate offset away
    const int cell = wave * 32 + (lane & 31);
    const unsigned abase = (unsigned)(((cell / TW) * PW + cell % TW) * PIXB + (lane >> 5) * 16);
    // packed mode-1 weights (fd_conv2d_pack_weight_dev): [cin / 32][cout / 32][tap'][ksub][lane] x 16 bytes, tap' = 8 - (3 ky + kx)
    const int64_t w_nt_stride = (int64_t)nslices * 9 * 2 * 64;
    const bf16x8 *wbase = wp + (int64_t)blockIdx.y * WNT * w_nt_stride + lane;

    load_slice(0);
    store_slice(0);
    __syncthreads();
    if (nslices > 1) load_slice(1);
    for (int s = 0; s < nslices; ++s) {
        const unsigned char *buf = smem + (s & 1) * (PP * PIXB) + abase;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[2][2];
#pragma unroll
            for (int sy = 0; sy < 2; ++sy)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) a[sy][sx] = *reinterpret_cast<const bf16x8 *>(buf + (sy * PW + sx) * PIXB + ks * 32);
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ky = tap / 3, kx = tap % 3;
                    const bf16x8 bw = wbase[j * w_nt_stride + (((int64_t)s * 9 + (8 - tap)) * 2 + ks) * 64];
                    // row parity of the dX pixel: ky = 1 serves the even rows from cell row m; ky = 0 the odd rows from m + 1, ky = 2 from m
                    acc[2 * (ky != 1) + (kx != 1)][j] =
                        __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[ky == 0][kx == 0], bw, acc[2 * (ky != 1) + (kx != 1)][j], 0, 0, 0);
                }
        }
        if (s + 1 < nslices) store_slice((s + 1) & 1);
        if (s + 2 < nslices) load_slice(s + 2);
        __syncthreads();
    }

    // one phase at a time through LDS: 16-byte stores of 8 channels.  Every dX pixel belongs to exactly one (tile, cell, phase).
    unsigned short *s_out = reinterpret_cast<unsigned short *>(smem);
    constexpr int C8 = NT / 8;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
        acc_to_lds<WNT>(acc[ph], s_out, wave, lane);
        __syncthreads();
        for (int id = tid; id < TH * TW * C8; id += 256) {
            const int m = id / C8, c8 = id - m * C8;
            const int iy = 2 * (m0 + m / TW) + (ph >> 1), ix = 2 * (n0 + m % TW) + (ph & 1);
            if (iy < p.H && ix < p.W)
                *reinterpret_cast<uint4 *>(dx + (((int64_t)b * p.H + iy) * p.W + ix) * p.cin + blockIdx.y * NT + c8 * 8) =
                    *reinterpret_cast<const uint4 *>(s_out + m * NT + c8 * 8);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- down2
struct Down2Params {
    int H, W, Hc, Wc, c_fine, c_coarse;  // fine map [B, H, W, c_fine] -> coarse map [B, Hc, Wc, c_coarse], Hc = H / 2, Wc = W / 2
    int n_pix;                           // B * Hc * Wc
};

// grid: (ceil(n_pix / 128), c_coarse / (32 WNT)); a workgroup takes 128 consecutive coarse pixels of the flat (b, y, x) order, wave w
// pixels 32 w .. 32 w + 31.  K = 4 c_fine in slices of 32: slice s lies in run s / (c_fine / 16) (the fine row 2 y + run), 64 s' bytes in.
template <int WNT>
__global__ void __launch_bounds__(256) conv2d_down2(const unsigned short *__restrict__ x, const bf16x8 *__restrict__ wp, unsigned short *__restrict__ y,
                                                    Down2Params p) {
    constexpr int M = 128, NT = WNT * 32;
    constexpr int NLOAD = M * 4 / 256;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * M * PIXB];
    static_assert(2 * M * PIXB >= M * NT * 2, "the epilogue transposes the tile through the slice buffers");

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = blockIdx.x * M;
    const int per_run = p.c_fine / 16;  // 32-channel slices of one run of 2 c_fine channels
    const int nslices = 4 * p.c_fine / 32;

    // this thread's two 16-byte pieces of a slice: element offset of (fine row 2 y, column 2 x, channel 8 q), or -1 past the last pixel
    int64_t src[NLOAD];
#pragma unroll
    for (int i = 0; i < NLOAD; ++i) {
        const int id = tid + i * 256, pp = p0 + (id >> 2);
        src[i] = -1;
        if (pp < p.n_pix) {
            const int xx = pp % p.Wc, rest = pp / p.Wc, yy = rest % p.Hc, b = rest / p.Hc;
            src[i] = (((int64_t)b * p.H + 2 * yy) * p.W + 2 * xx) * p.c_fine + (id & 3) * 8;
        }
    }
    const int64_t row_pitch = (int64_t)p.W * p.c_fine;
    uint4 stage[NLOAD];
    auto load_slice = [&](int s) {
        const int run = s / per_run;
        const int64_t off = run * row_pitch + (s - run * per_run) * 32;
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            stage[i] = make_uint4(0u, 0u, 0u, 0u);
            if (src[i] >= 0) stage[i] = *reinterpret_cast<const uint4 *>(x + src[i] + off);
        }
    };
    auto store_slice = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int id = tid + i * 256;
            *reinterpret_cast<uint4 *>(smem + buf * (M * PIXB) + (id >> 2) * PIXB + ((id & 3) << 4)) = stage[i];
        }
    };

    f32x16 acc[WNT];
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    const unsigned abase = (unsigned)((wave * 32 + (lane & 31)) * PIXB + (lane >> 5) * 16);
    // packed weights of the [c_coarse, 4 c_fine, 1, 1] problem: [c_coarse / 32][slice][ksub][lane] x 16 bytes
    const int64_t w_nt_stride = (int64_t)nslices * 2 * 64;
    const bf16x8 *wbase = wp + (int64_t)blockIdx.y * WNT * w_nt_stride + lane;

    load_slice(0);
    store_slice(0);
    __syncthreads();
    if (nslices > 1) load_slice(1);
    for (int s = 0; s < nslices; ++s) {
        const unsigned char *buf = smem + (s & 1) * (M * PIXB) + abase;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(buf + ks * 32);
#pragma unroll
            for (int j = 0; j < WNT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, wbase[j * w_nt_stride + ((int64_t)s * 2 + ks) * 64], acc[j], 0, 0, 0);
        }
        if (s + 1 < nslices) store_slice((s + 1) & 1);
        if (s + 2 < nslices) load_slice(s + 2);
        __syncthreads();
    }

    unsigned short *s_out = reinterpret_cast<unsigned short *>(smem);
    acc_to_lds<WNT>(acc, s_out, wave, lane);
    __syncthreads();
    constexpr int C8 = NT / 8;
    for (int id = tid; id < M * C8; id += 256) {
        const int m = id / C8, c8 = id - m * C8;
        if (p0 + m < p.n_pix)
            *reinterpret_cast<uint4 *>(y + (int64_t)(p0 + m) * p.c_coarse + blockIdx.y * NT + c8 * 8) = *reinterpret_cast<const uint4 *>(s_out + m * NT + c8 * 8);
    }
}

// ---------------------------------------------------------------------------------------------------------------- 2 x 2 weight packer
// W(a, f, t): the parameter at coarse-side channel a, fine-side channel f, tap t = 2 dy + dx; w is [c_coarse][c_fine][2][2], or
// [c_fine][c_coarse][2][2] with fine_major.
//   kind 0 (up2):   four packs, one per tap t, of the 1 x 1 problem c_coarse -> c_fine: w_t[f][a] = W(a, f, t)
//   kind 1 (down2): one pack of the 1 x 1 problem 4 c_fine -> c_coarse: w'[a][t c_fine + f] = W(a, f, t)
// one thread per 16-byte fragment piece, [out_pad / 32][in / 32][ksub][lane] x 8 bf16 as in fd_conv2d_pack_weight
__global__ void __launch_bounds__(256) conv2d_pack_weight_2x2_dev(const float *__restrict__ w, int c_coarse, int c_fine, int kind, int fine_major,
                                                                  uint4 *__restrict__ dst, int64_t per_pack, int64_t n_pieces) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n_pieces) return;
    const int n_out = kind ? c_coarse : c_fine, n_in = kind ? 4 * c_fine : c_coarse;
    const int nsl = n_in / 32;
    int64_t t = id % per_pack;
    const int pack = (int)(id / per_pack);  // (kind 0: the tap)
    const int lane = (int)(t & 63); t >>= 6;
    const int ksub = (int)(t & 1); t >>= 1;
    const int s = (int)(t % nsl), nt = (int)(t / nsl);
    const int o = nt * 32 + (lane & 31);
    const int i0 = s * 32 + ksub * 16 + 8 * (lane >> 5);
    unsigned short h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = 0.0f;
        if (o < n_out) {
            const int i = i0 + j;
            const int a = kind ? o : i, f = kind ? i % c_fine : o, tap = kind ? i / c_fine : pack;
            v = w[(fine_major ? (int64_t)f * c_coarse + a : (int64_t)a * c_fine + f) * 4 + tap];
        }
        unsigned u = __float_as_uint(v);
        u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even: the host packer's arithmetic
        h[j] = (unsigned short)(u >> 16);
    }
    dst[id] = make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
}

}  // namespace

extern "C" int fd_conv2d_s2_dgrad_bf16(const void *dy, int B, int H, int W, int cin, int cout, const void *wpacked_t, void *dx, fd_stream_t stream) {
    FD_REQUIRE(dy && wpacked_t && dx, "fd_conv2d_s2_dgrad_bf16: null argument");
    FD_REQUIRE(cin > 0 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
               "fd_conv2d_s2_dgrad_bf16: cin and cout must be positive multiples of 32 (got %d -> %d)", cin, cout);
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_conv2d_s2_dgrad_bf16: bad shape %d x %d x %d", B, H, W);
    DgradParams p;
    p.B = B; p.H = H; p.W = W; p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1; p.cin = cin; p.cout = cout;
    p.tiles_x = (p.Wo + TW - 1) / TW;
    p.tiles_y = (p.Ho + TH - 1) / TH;
    const int64_t tiles = (int64_t)p.tiles_x * p.tiles_y * B;
    FD_REQUIRE(tiles < (1ll << 31) && cin / 32 <= 65535, "fd_conv2d_s2_dgrad_bf16: too many tiles or channel blocks");
    hipStream_t s = fd::as_stream(stream);
    if (cin % 64 == 0)
        hipLaunchKernelGGL(conv2d_s2_dgrad<2>, dim3((unsigned)tiles, (unsigned)(cin / 64)), dim3(256), 0, s, (const unsigned short *)dy,
                           (const bf16x8 *)wpacked_t, (unsigned short *)dx, p);
    else
        hipLaunchKernelGGL(conv2d_s2_dgrad<1>, dim3((unsigned)tiles, (unsigned)(cin / 32)), dim3(256), 0, s, (const unsigned short *)dy,
                           (const bf16x8 *)wpacked_t, (unsigned short *)dx, p);
    return fd::check_launch("fd_conv2d_s2_dgrad_bf16");
}

extern "C" int fd_conv2d_down2_bf16(const void *x, int B, int H, int W, int c_fine, const void *wpacked, int c_coarse, void *y, fd_stream_t stream) {
    FD_REQUIRE(x && wpacked && y, "fd_conv2d_down2_bf16: null argument");
    FD_REQUIRE(c_fine > 0 && c_coarse > 0 && c_fine % 32 == 0 && c_coarse % 32 == 0,
               "fd_conv2d_down2_bf16: both channel counts must be positive multiples of 32 (got %d -> %d)", c_fine, c_coarse);
    FD_REQUIRE(B > 0 && H >= 2 && W >= 2, "fd_conv2d_down2_bf16: bad shape %d x %d x %d (the fine map; 2 x 2 at least)", B, H, W);
    Down2Params p;
    p.H = H; p.W = W; p.Hc = H / 2; p.Wc = W / 2; p.c_fine = c_fine; p.c_coarse = c_coarse;
    const int64_t n_pix = (int64_t)B * p.Hc * p.Wc;
    FD_REQUIRE(n_pix + 128 < (1ll << 31) && c_coarse / 32 <= 65535, "fd_conv2d_down2_bf16: maps of 2^31 pixels and more are not supported");
    p.n_pix = (int)n_pix;
    const unsigned gx = (unsigned)((n_pix + 127) / 128);
    hipStream_t s = fd::as_stream(stream);
    if (c_coarse % 64 == 0)
        hipLaunchKernelGGL(conv2d_down2<2>, dim3(gx, (unsigned)(c_coarse / 64)), dim3(256), 0, s, (const unsigned short *)x, (const bf16x8 *)wpacked,
                           (unsigned short *)y, p);
    else
        hipLaunchKernelGGL(conv2d_down2<1>, dim3(gx, (unsigned)(c_coarse / 32)), dim3(256), 0, s, (const unsigned short *)x, (const bf16x8 *)wpacked,
                           (unsigned short *)y, p);
    return fd::check_launch("fd_conv2d_down2_bf16");
}

extern "C" size_t fd_conv2d_packed_weight_2x2_bytes(int c_coarse, int c_fine, int kind) {
    if (kind == 0) return 4 * fd_conv2d_packed_weight_bytes(c_fine, c_coarse, 1);
    if (kind == 1 && c_fine > 0 && c_fine % 32 == 0) return fd_conv2d_packed_weight_bytes(c_coarse, 4 * c_fine, 1);
    return 0;
}

extern "C" int fd_conv2d_pack_weight_2x2_dev(const float *w, int c_coarse, int c_fine, int kind, int fine_major, void *dst, fd_stream_t stream) {
    FD_REQUIRE(w && dst, "fd_conv2d_pack_weight_2x2_dev: null argument");
    FD_REQUIRE(kind == 0 || kind == 1, "fd_conv2d_pack_weight_2x2_dev: kind must be 0 (up2) or 1 (down2) (got %d)", kind);
    FD_REQUIRE(fine_major == 0 || fine_major == 1, "fd_conv2d_pack_weight_2x2_dev: fine_major must be 0 or 1 (got %d)", fine_major);
    const size_t bytes = fd_conv2d_packed_weight_2x2_bytes(c_coarse, c_fine, kind);
    FD_REQUIRE(c_coarse > 0 && c_fine > 0 && bytes > 0,
               "fd_conv2d_pack_weight_2x2_dev: the reduction side (up2: coarse, down2: fine) must be a positive multiple of 32 (got %d coarse, %d fine)",
               c_coarse, c_fine);
    const int64_t n_pieces = (int64_t)(bytes / 16);
    FD_REQUIRE((n_pieces + 255) / 256 < (1ll << 31), "fd_conv2d_pack_weight_2x2_dev: bad sizes");
    hipLaunchKernelGGL(conv2d_pack_weight_2x2_dev, dim3((unsigned)((n_pieces + 255) / 256)), dim3(256), 0, fd::as_stream(stream), w, c_coarse, c_fine, kind,
                       fine_major, (uint4 *)dst, kind ? n_pieces : n_pieces / 4, n_pieces);
    return fd::check_launch("fd_conv2d_pack_weight_2x2_dev");
}
