// Deformable 3x3 convolution (DCN v1) for gfx950: the two FeatureAdaption modules of a CenterHead DCN task in ONE launch.
//
// Reference: det3d/models/bbox_heads/center_head.py:40-78 (FeatureAdaption: conv_offset = 1x1 conv C -> 72 with bias,
// conv_adaption = DeformConv(C, C, 3, padding 1, deformable_groups 4, no bias), output ReLU) and :176-229 (DCNSepHead: a cls and a
// reg FeatureAdaption on the same input); the sampling arithmetic is det3d/ops/dcn/src/deform_conv_cuda_kernel.cu:85-117,191-240.
//
// x [B,H,W,64] NHWC (fp32 or bf16) -> y [B,H,W,128] of the same dtype: channels 0-63 = ReLU(DCN_cls(x)), 64-127 = ReLU(DCN_reg(x)).
//
//   * a workgroup (4 waves) owns a strip of 64 consecutive output pixels (flattened b, y, x); lane m of every wave is pixel m;
//   * prologue: every lane loads its pixel's 64 input channels into registers and computes, in fp32, the 18 offsets
//     (9 taps x (dh, dw)) of the two (branch, group) pairs its wave samples -- wave w: branch w >> 1, groups 2 (w & 1) and
//     2 (w & 1) + 1.  The offset weights are wave-uniform (scalar loads).  Offsets stay fp32 in the bf16 mode too (a bf16 offset
//     misplaces a sample by up to 1/64 px at |d| ~ 4).  Alternatively the caller passes precomputed fp32 offsets [B,H,W,144];
//   * per tap: gather -- every lane blends the four corners of its (pixel, group) sample, each corner a contiguous 16-channel
//     run read with 16-byte loads, in fp32 with the reference's weights and operation order, and writes the 16 sampled channels
//     into the LDS im2col tile [2 branches][64 pixels][64 channels] (rows padded by 16 bytes: conflict-free b128 reads);
//     then MFMA -- wave w multiplies its branch's tile by its half of the branch's packed [64 x 64] tap weights
//     (fp32: v_mfma_f32_16x16x4_f32, bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulators in both), issued transposed (A = weights,
//     B = pixels) so a lane ends up with consecutive output channels of one pixel;
//   * epilogue: ReLU, (bf16: round to nearest even,) store.
// Bound (measured, B = 2, 180 x 180): fp32 194-220 us against a 61 us fp32-MFMA floor, bf16 128-142 us; the ~50 MB of compulsory HBM
// traffic is ~8 us.  Each tap runs gather -> barrier -> MFMA -> barrier without overlap inside the workgroup, and 2-3 waves per SIMD
// do not hide it (DESIGN.md "DCN head").
// Built with -fno-slp-vectorize -ffp-contract=off (build.EXTRA): the coordinate math must stay scalar IEEE operations in the
// written order (the packed-fp32 op_sel form is refused library-wide, tests/test_host_surface.py).
#include <string.h>

#include <type_traits>

#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kC = 64;        // channels of the head (head_conv)
constexpr int kG = 4;         // deformable groups
constexpr int kCG = kC / kG;  // channels per group (16)
constexpr int kTaps = 9;
constexpr int kOffCh = kG * 2 * kTaps;  // 72 offset channels per branch
constexpr int kPix = 64;      // output pixels per workgroup

__device__ inline unsigned short f2bf(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (unsigned short)((u >> 16) | 0x40u);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// 16 consecutive channels at p as fp32
template <bool BF16>
__device__ inline void load16(const void *p, float v[16]) {
    if constexpr (BF16) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint4 u = q[h];
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[8 * h + 2 * k] = __uint_as_float(w[k] << 16);
                v[8 * h + 2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
            }
        }
    } else {
        const float4 *q = reinterpret_cast<const float4 *>(p);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const float4 f = q[h];
            v[4 * h] = f.x; v[4 * h + 1] = f.y; v[4 * h + 2] = f.z; v[4 * h + 3] = f.w;
        }
    }
}

struct DeformParams {
    int B, H, W;
    int64_t npix;  // B * H * W
};

// LDS tile row: 64 channels + 16 bytes of padding
template <bool BF16> struct Tile {
    typedef typename std::conditional<BF16, unsigned short, float>::type T;
    static constexpr int ROW = kC + 16 / (int)sizeof(T);
};

template <bool BF16>
__global__ void __launch_bounds__(256) deform_adapt_nhwc(const void *__restrict__ xv, const float *__restrict__ off_w, const float *__restrict__ off_b,
                                                         const float *__restrict__ off_in, const void *__restrict__ wpv, void *__restrict__ yv,
                                                         DeformParams p) {
    typedef typename Tile<BF16>::T T;
    constexpr int ROW = Tile<BF16>::ROW;
    __shared__ __attribute__((aligned(16))) T tile[2 * kPix * ROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int br = wave >> 1;            // branch of this wave (0 = cls, 1 = reg): gather AND MFMA
    const int g0 = 2 * (wave & 1);       // first of the two groups this wave samples
    const T *x = reinterpret_cast<const T *>(xv);
    const int64_t pix = (int64_t)blockIdx.x * kPix + lane;
    const int64_t pc = pix < p.npix ? pix : p.npix - 1;  // lanes past the end work on the last pixel and store nothing
    const int px = (int)(pc % p.W), py = (int)((pc / p.W) % p.H);
    const int64_t img = pc / ((int64_t)p.H * p.W) * p.H * p.W;  // first pixel of this lane's sample

    // ---- offsets: off[k][tap][0 = dh, 1 = dw] of group g0 + k of branch br (offset channel g * 18 + 2 tap + {0, 1})
    float off[2][kTaps][2];
    if (off_in) {
        const float *o = off_in + pc * (2 * kOffCh) + br * kOffCh + g0 * 2 * kTaps;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                off[k][t][0] = o[k * 2 * kTaps + 2 * t];
                off[k][t][1] = o[k * 2 * kTaps + 2 * t + 1];
            }
    } else {
        float xr[kC];
#pragma unroll
        for (int s = 0; s < kG; ++s) load16<BF16>(x + pc * kC + s * kCG, xr + s * kCG);
        const float *wr = off_w + (int64_t)(br * kOffCh + g0 * 2 * kTaps) * kC;  // wave-uniform rows
        const float *bb = off_b + br * kOffCh + g0 * 2 * kTaps;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int t = 0; t < kTaps; ++t)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int r = k * 2 * kTaps + 2 * t + d;
                    float a = bb[r];
#pragma unroll
                    for (int c = 0; c < kC; ++c) a = __builtin_fmaf(wr[r * kC + c], xr[c], a);
                    off[k][t][d] = a;
                }
    }

    // ---- accumulators and this wave's weight / LDS addressing
    constexpr int NACC = BF16 ? 2 : 8;
    typedef typename std::conditional<BF16, f32x16, f32x4>::type AccT;
    AccT acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = AccT{};

#pragma unroll
    for (int tap = 0; tap < kTaps; ++tap) {
        // ---- gather: (pixel lane, group g0 + k) of branch br -> tile[br][lane][16 (g0 + k) ..]
        const int ti = tap / 3, tj = tap % 3;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int g = g0 + k;
            const float h = (float)(py - 1 + ti) + off[k][tap][0];
            const float w = (float)(px - 1 + tj) + off[k][tap][1];
            float v[kCG];
#pragma unroll
            for (int c = 0; c < kCG; ++c) v[c] = 0.f;
            if (h > -1.f && w > -1.f && h < (float)p.H && w < (float)p.W) {
                const float hf = floorf(h), wf = floorf(w);
                const int hl = (int)hf, wl = (int)wf, hh_i = hl + 1, wh_i = wl + 1;
                const float lh = h - hf, lw = w - wf;
                const float hh = 1.f - lh, hw = 1.f - lw;
                const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
                float c1[kCG], c2[kCG], c3[kCG], c4[kCG];
#pragma unroll
                for (int c = 0; c < kCG; ++c) c1[c] = c2[c] = c3[c] = c4[c] = 0.f;
                const T *base = x + img * kC + g * kCG;
                if (hl >= 0 && wl >= 0) load16<BF16>(base + ((int64_t)hl * p.W + wl) * kC, c1);
                if (hl >= 0 && wh_i <= p.W - 1) load16<BF16>(base + ((int64_t)hl * p.W + wh_i) * kC, c2);
                if (hh_i <= p.H - 1 && wl >= 0) load16<BF16>(base + ((int64_t)hh_i * p.W + wl) * kC, c3);
                if (hh_i <= p.H - 1 && wh_i <= p.W - 1) load16<BF16>(base + ((int64_t)hh_i * p.W + wh_i) * kC, c4);
#pragma unroll
                for (int c = 0; c < kCG; ++c) v[c] = w1 * c1[c] + w2 * c2[c] + w3 * c3[c] + w4 * c4[c];
            }
            T *dst = tile + (br * kPix + lane) * ROW + g * kCG;
            if constexpr (BF16) {
                unsigned u[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) u[c] = (unsigned)f2bf(v[2 * c]) | ((unsigned)f2bf(v[2 * c + 1]) << 16);
                reinterpret_cast<uint4 *>(dst)[0] = make_uint4(u[0], u[1], u[2], u[3]);
                reinterpret_cast<uint4 *>(dst)[1] = make_uint4(u[4], u[5], u[6], u[7]);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) reinterpret_cast<float4 *>(dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            }
        }
        __syncthreads();
        // ---- MFMA over this tap's 64 input channels
        const T *tb = tile + br * kPix * ROW;
        if constexpr (BF16) {
            // weights [br][tap][ks 4][nb 2][lane] x 8 bf16: lane (r, h) = W[32 nb + r][16 ks + 8 h + j]; wave's nb = wave & 1
            const bf16x8 *wp = reinterpret_cast<const bf16x8 *>(wpv) + ((int64_t)(br * kTaps + tap) * 4 * 2 + (wave & 1)) * 64 + lane;
            const int r = lane & 31, hsel = lane >> 5;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 b = wp[ks * 2 * 64];
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(tb + (pb * 32 + r) * ROW + ks * 16 + hsel * 8);
                    acc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, acc[pb], 0, 0, 0);
                }
            }
        } else {
            // weights [br][tap][s 4][nb 4][lane] float4: lane (lm, lq) = W[16 nb + lm][16 s + 4 lq + 0..3]; wave's nb = 2 (wave & 1) + j
            const float4 *wp = reinterpret_cast<const float4 *>(wpv) + (int64_t)(br * kTaps + tap) * 4 * 4 * 64 + lane;
            const int lm = lane & 15, lq = lane >> 4;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float4 bw[2], a[4];
#pragma unroll
                for (int j = 0; j < 2; ++j) bw[j] = wp[(s * 4 + 2 * (wave & 1) + j) * 64];
#pragma unroll
                for (int pb = 0; pb < 4; ++pb) a[pb] = *reinterpret_cast<const float4 *>(tb + (pb * 16 + lm) * ROW + s * 16 + lq * 4);
#define FD_KSTEP(C)                                                                                             \
    _Pragma("unroll") for (int pb = 0; pb < 4; ++pb) _Pragma("unroll") for (int j = 0; j < 2; ++j)              \
        acc[pb * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[j].C, a[pb].C, acc[pb * 2 + j], 0, 0, 0);
                FD_KSTEP(x) FD_KSTEP(y) FD_KSTEP(z) FD_KSTEP(w)
#undef FD_KSTEP
            }
        }
        __syncthreads();  // the tile is rewritten by the next tap's gather
    }

    // ---- epilogue: ReLU, store into y[pixel][64 br + co]
    const int64_t p0 = (int64_t)blockIdx.x * kPix;
    if constexpr (BF16) {
        // lane (r, h), register i: output channel 32 nb + (i & 3) + 8 (i >> 2) + 4 h of pixel 32 pb + r
        unsigned short *y = reinterpret_cast<unsigned short *>(yv);
        const int r = lane & 31, hsel = lane >> 5;
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const int64_t q = p0 + pb * 32 + r;
            if (q >= p.npix) continue;
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                const int co = br * kC + 32 * (wave & 1) + 8 * i4 + 4 * hsel;
                unsigned short o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = f2bf(fmaxf(acc[pb][4 * i4 + e], 0.f));
                *reinterpret_cast<uint2 *>(y + q * (2 * kC) + co) =
                    make_uint2((unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16));
            }
        }
    } else {
        // lane (lm, lq), accumulator (pb, j): output channels 16 (2 (wave & 1) + j) + 4 lq + 0..3 of pixel 16 pb + lm
        float *y = reinterpret_cast<float *>(yv);
        const int lm = lane & 15, lq = lane >> 4;
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
            const int64_t q = p0 + pb * 16 + lm;
            if (q >= p.npix) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int co = br * kC + 16 * (2 * (wave & 1) + j) + 4 * lq;
                const f32x4 v = acc[pb * 2 + j];
                *reinterpret_cast<float4 *>(y + q * (2 * kC) + co) = make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
            }
        }
    }
}

inline uint16_t host_bf16(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

}  // namespace

extern "C" size_t fd_deform_adapt_packed_weight_bytes(int bf16) {
    return (size_t)2 * kTaps * kC * kC * (bf16 ? 2 : 4);
}

extern "C" int fd_deform_adapt_pack_weight(const float *w_cls, const float *w_reg, int bf16, void *dst) {
    FD_REQUIRE(w_cls && w_reg && dst, "fd_deform_adapt_pack_weight: null pointer");
    for (int br = 0; br < 2; ++br) {
        const float *w = br ? w_reg : w_cls;  // [co 64][ci 64][3][3]
        auto W = [&](int co, int ci, int tap) { return w[((int64_t)co * kC + ci) * kTaps + tap]; };
        for (int tap = 0; tap < kTaps; ++tap) {
            if (bf16) {
                uint16_t *d = reinterpret_cast<uint16_t *>(dst) + (int64_t)(br * kTaps + tap) * 4 * 2 * 64 * 8;
                for (int ks = 0; ks < 4; ++ks)
                    for (int nb = 0; nb < 2; ++nb)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 8; ++j)
                                d[((ks * 2 + nb) * 64 + l) * 8 + j] = host_bf16(W(32 * nb + (l & 31), 16 * ks + 8 * (l >> 5) + j, tap));
            } else {
                float *d = reinterpret_cast<float *>(dst) + (int64_t)(br * kTaps + tap) * 4 * 4 * 64 * 4;
                for (int s = 0; s < 4; ++s)
                    for (int nb = 0; nb < 4; ++nb)
                        for (int l = 0; l < 64; ++l)
                            for (int c = 0; c < 4; ++c)
                                d[((s * 4 + nb) * 64 + l) * 4 + c] = W(16 * nb + (l & 15), 16 * s + 4 * (l >> 4) + c, tap);
            }
        }
    }
    return FD_OK;
}

extern "C" int fd_deform_adapt_nhwc(const void *x, int B, int H, int W, int C, int bf16, const float *off_w, const float *off_b,
                                    const float *offsets, const void *wpacked, void *y, fd_stream_t stream) {
    FD_REQUIRE(x && wpacked && y, "fd_deform_adapt_nhwc: null pointer");
    FD_REQUIRE(offsets || (off_w && off_b), "fd_deform_adapt_nhwc: either offsets or both off_w and off_b are required");
    FD_REQUIRE(C == kC, "fd_deform_adapt_nhwc: C = %d, only 64 channels (head_conv) are supported", C);
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "fd_deform_adapt_nhwc: bad shape B=%d H=%d W=%d", B, H, W);
    FD_REQUIRE(bf16 == 0 || bf16 == 1, "fd_deform_adapt_nhwc: bf16 must be 0 or 1");
    FD_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)wpacked & 15) == 0,
               "fd_deform_adapt_nhwc: x, y and wpacked must be 16-byte aligned");
    DeformParams p;
    p.B = B; p.H = H; p.W = W;
    p.npix = (int64_t)B * H * W;
    const int64_t blocks = (p.npix + kPix - 1) / kPix;
    FD_REQUIRE(blocks < (1ll << 31), "fd_deform_adapt_nhwc: %lld pixels is too many", (long long)p.npix);
    hipStream_t s = fd::as_stream(stream);
    if (bf16)
        hipLaunchKernelGGL(deform_adapt_nhwc<true>, dim3((unsigned)blocks), dim3(256), 0, s, x, off_w, off_b, offsets, wpacked, y, p);
    else
        hipLaunchKernelGGL(deform_adapt_nhwc<false>, dim3((unsigned)blocks), dim3(256), 0, s, x, off_w, off_b, offsets, wpacked, y, p);
    return fd::check_launch("fd_deform_adapt_nhwc");
}
