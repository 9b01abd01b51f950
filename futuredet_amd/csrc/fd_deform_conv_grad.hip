// Backward pass of the deformable FeatureAdaption pair (fd_deform_conv.hip) for gfx950: training of the CenterHead dcn_head option.
//
// Reference: det3d/ops/dcn/src/deform_conv_cuda_kernel.cu (deformable_col2im for the input, deformable_col2im_coord /
// get_coordinate_weight for the offsets) under det3d/ops/dcn/deform_conv.py's backward; here for the forward's fixed shape: C = 64,
// 4 deformable groups of 16 channels, 3x3, pad 1, the cls and the reg branch in one call, NHWC, fp32.
//
//   y  = ReLU(sum_t W_br[.][.][t] . col_br[.][t])        col_br[c][t] = bilinear sample of x[.., c] at the tap's deformed position
//   dyr = dy * (y > 0)
//   dcol_br[c][t] = sum_co dyr[br, co] W_br[co][c][t]
//   dx      += w_k dcol[c]  at each in-map corner k of each inside sample            (scatter: fp32 atomic adds)
//   doffset  = sum_{c in group} dcol[c] * d(sample)/d(h, w)                         (one lane per element: deterministic)
//   dW_br[co][ci][t] = sum_pixels dyr[br, co] col_br[ci][t]                          (partials per pixel chunk: deterministic)
//
// deform_adapt_bwd_data (dx, doffsets).  As in the forward a workgroup (4 waves) owns a strip of 64 consecutive pixels; wave w works
// on branch w >> 1 and on the groups 2 (w & 1), 2 (w & 1) + 1 (channels 32 (w & 1) .. + 31).  The wave keeps its branch's dyr strip as
// MFMA B fragments in registers for all nine taps.  Per tap:
//   1. dcol = W^T . dyr on v_mfma_f32_16x16x4_f32 (A = the tap's transposed packed weights, B = dyr, exactly the forward's
//      orientation), written to the LDS tile [branch][pixel][channel];
//   2. lane m = pixel m recomputes, for each of its two groups, the forward's coordinates with the forward's operations in the
//      forward's order (same floor, same in-window and in-map decisions), loads the four corners, reduces the two offset gradients
//      over the group's 16 channels and stores them; it leaves (corner pixel, weight) x 4 in LDS;
//   3. scatter: 16 lanes per (pixel, group, corner), lane = channel: one wave instruction adds four 64-byte runs of dx.
// deform_adapt_bwd_wpartial / deform_adapt_bwd_wreduce (dw).  Workgroup (chunk, tap, branch) walks the chunk's pixels in strips of
// 64: the re-sampled column tile [64 px][64 ci] and dyr [64 px][64 co] go to LDS, and the four waves run v_mfma_f32_16x16x4_f32
// over them with the pixels as the reduction dimension (fd_spconv_wgrad's form).  The [ci][co] partial goes to the workspace; the
// reduce kernel sums a (branch, tap)'s partials in chunk order into OIHW.  kChunk is a constant, so the chunk boundaries and the
// summation order depend on B * H * W only.  No atomics.
// Built with -ffp-contract=off -fno-slp-vectorize like fd_deform_conv.hip: the coordinate arithmetic must be the forward's scalar
// IEEE operations.
#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kC = 64;
constexpr int kG = 4;
constexpr int kCG = kC / kG;
constexpr int kTaps = 9;
constexpr int kOffCh = kG * 2 * kTaps;  // 72 offset channels per branch
constexpr int kPix = 64;                // pixels per strip
constexpr int kRow = kC + 4;            // dcol tile row (floats): 16 bytes of padding, conflict-free b128 accesses
constexpr int kChunk = 1024;            // pixels per dW partial: part of the summation order, not a tuning knob
constexpr int kRowW = kC + 16;          // dW tiles: the four 16-lane groups of a b32 read land on different bank sets
constexpr int kWtElems = 2 * kTaps * kC * kC;

struct GradParams {
    int B, H, W;
    int64_t npix;
};

__device__ inline void load16(const float *p, float v[16]) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        const float4 f = q[h];
        v[4 * h] = f.x; v[4 * h + 1] = f.y; v[4 * h + 2] = f.z; v[4 * h + 3] = f.w;
    }
}

// The forward's sample of (pixel, tap, group): coordinates, weights and the four corners (an out-of-map corner = 0, index -1).
struct Sample {
    bool inside;
    float lh, lw, hh, hw;
    int idx[4];  // pixel index inside the image of corner 1..4, -1 = outside the map
};

__device__ inline Sample locate(int py, int px, int ti, int tj, float dh, float dw, int H, int W) {
    Sample s;
    const float h = (float)(py - 1 + ti) + dh;
    const float w = (float)(px - 1 + tj) + dw;
    s.inside = h > -1.f && w > -1.f && h < (float)H && w < (float)W;
    s.lh = s.lw = s.hh = s.hw = 0.f;
    s.idx[0] = s.idx[1] = s.idx[2] = s.idx[3] = -1;
    if (s.inside) {
        const float hf = floorf(h), wf = floorf(w);
        const int hl = (int)hf, wl = (int)wf, hh_i = hl + 1, wh_i = wl + 1;
        s.lh = h - hf;
        s.lw = w - wf;
        s.hh = 1.f - s.lh;
        s.hw = 1.f - s.lw;
        if (hl >= 0 && wl >= 0) s.idx[0] = hl * W + wl;
        if (hl >= 0 && wh_i <= W - 1) s.idx[1] = hl * W + wh_i;
        if (hh_i <= H - 1 && wl >= 0) s.idx[2] = hh_i * W + wl;
        if (hh_i <= H - 1 && wh_i <= W - 1) s.idx[3] = hh_i * W + wh_i;
    }
    return s;
}

// transposed fragment order for dcol = W^T dyr: [br][tap][s 4][nb 4][lane] float4, lane (lm, lq) = W[16 s + 4 lq + 0..3][16 nb + lm][tap]
__global__ void __launch_bounds__(256) pack_weight_t(const float *__restrict__ w_cls, const float *__restrict__ w_reg, float *__restrict__ dst) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= kWtElems) return;
    int r = t;
    const int c = r & 3; r >>= 2;
    const int l = r & 63; r >>= 6;
    const int nb = r & 3; r >>= 2;
    const int s = r & 3; r >>= 2;
    const int tap = r % kTaps, br = r / kTaps;
    const float *w = br ? w_reg : w_cls;
    const int co = 16 * s + 4 * (l >> 4) + c, ci = 16 * nb + (l & 15);
    dst[t] = w[(co * kC + ci) * kTaps + tap];
}

// the forward's fp32 fragment order (fd_deform_adapt_pack_weight): lane (lm, lq) = W[16 nb + lm][16 s + 4 lq + 0..3][tap]
__global__ void __launch_bounds__(256) pack_weight_fwd(const float *__restrict__ w_cls, const float *__restrict__ w_reg, float *__restrict__ dst) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= kWtElems) return;
    int r = t;
    const int c = r & 3; r >>= 2;
    const int l = r & 63; r >>= 6;
    const int nb = r & 3; r >>= 2;
    const int s = r & 3; r >>= 2;
    const int tap = r % kTaps, br = r / kTaps;
    const float *w = br ? w_reg : w_cls;
    const int co = 16 * nb + (l & 15), ci = 16 * s + 4 * (l >> 4) + c;
    dst[t] = w[(co * kC + ci) * kTaps + tap];
}

__global__ void __launch_bounds__(256, 2) deform_adapt_bwd_data(const float *__restrict__ x, const float *__restrict__ offsets, const float *__restrict__ wt,
                                                                const float *__restrict__ y, const float *__restrict__ dy, float *__restrict__ dx,
                                                                float *__restrict__ doff, GradParams p) {
    __shared__ __attribute__((aligned(16))) float tile[2 * kPix * kRow];  // dcol [br][pixel][channel]
    __shared__ int s_idx[2 * kPix * kG * 4];                              // [br][pixel][group][corner]: global pixel of the corner, -1 = none
    __shared__ float s_wt[2 * kPix * kG * 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int br = wave >> 1, g0 = 2 * (wave & 1);
    const int lm = lane & 15, lq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * kPix;
    const int64_t pix = p0 + lane;
    const bool live = pix < p.npix;
    const int64_t pc = live ? pix : p.npix - 1;
    const int px = (int)(pc % p.W), py = (int)((pc / p.W) % p.H);
    const int64_t img = pc / ((int64_t)p.H * p.W) * p.H * p.W;

    // ---- dyr of this wave's branch as B fragments: b[s][pb] = dyr[pixel 16 pb + lm][16 s + 4 lq + 0..3]; pixels past the end = 0
    float4 b[4][4];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
        const int64_t q = p0 + pb * 16 + lm;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < p.npix) {
                const int64_t o = q * (2 * kC) + br * kC + s * 16 + lq * 4;
                const float4 g = *reinterpret_cast<const float4 *>(dy + o);
                const float4 m = *reinterpret_cast<const float4 *>(y + o);
                v = make_float4(m.x > 0.f ? g.x : 0.f, m.y > 0.f ? g.y : 0.f, m.z > 0.f ? g.z : 0.f, m.w > 0.f ? g.w : 0.f);
            }
            b[s][pb] = v;
        }
    }

    const float *orow = offsets + pc * (2 * kOffCh) + br * kOffCh;

#pragma unroll 1
    for (int tap = 0; tap < kTaps; ++tap) {
        // ---- 1. dcol[c = 16 nb + 4 lq + r][pixel 16 pb + lm], nb = g0 + j
        f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const float4 *wp = reinterpret_cast<const float4 *>(wt) + (int64_t)(br * kTaps + tap) * 4 * 4 * 64 + lane;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float4 a[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) a[j] = wp[(s * 4 + g0 + j) * 64];
#define FD_KSTEP(C)                                                                                \
    _Pragma("unroll") for (int pb = 0; pb < 4; ++pb) _Pragma("unroll") for (int j = 0; j < 2; ++j) \
        acc[pb * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j].C, b[s][pb].C, acc[pb * 2 + j], 0, 0, 0);
            FD_KSTEP(x) FD_KSTEP(y) FD_KSTEP(z) FD_KSTEP(w)
#undef FD_KSTEP
        }
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 v = acc[pb * 2 + j];
                *reinterpret_cast<float4 *>(tile + (br * kPix + pb * 16 + lm) * kRow + (g0 + j) * kCG + lq * 4) = make_float4(v[0], v[1], v[2], v[3]);
            }
        __syncthreads();

        // ---- 2. lane = pixel: the forward's sample of groups g0, g0 + 1; offset gradients; corner list
        const int ti = tap / 3, tj = tap % 3;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int g = g0 + k;
            const float2 o = *reinterpret_cast<const float2 *>(orow + g * 2 * kTaps + 2 * tap);
            const Sample sm = locate(py, px, ti, tj, o.x, o.y, p.H, p.W);
            const float wk[4] = {sm.hh * sm.hw, sm.hh * sm.lw, sm.lh * sm.hw, sm.lh * sm.lw};
            const int e = ((br * kPix + lane) * kG + g) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                s_idx[e + c] = (live && sm.idx[c] >= 0) ? (int)(img + sm.idx[c]) : -1;
                s_wt[e + c] = wk[c];
            }
            if (doff && live) {
                float gh = 0.f, gw = 0.f;
                if (sm.inside) {
                    float d[kCG], c1[kCG], c2[kCG], c3[kCG], c4[kCG];
#pragma unroll
                    for (int c = 0; c < kCG; ++c) c1[c] = c2[c] = c3[c] = c4[c] = 0.f;
                    const float *base = x + img * kC + g * kCG;
                    if (sm.idx[0] >= 0) load16(base + (int64_t)sm.idx[0] * kC, c1);
                    if (sm.idx[1] >= 0) load16(base + (int64_t)sm.idx[1] * kC, c2);
                    if (sm.idx[2] >= 0) load16(base + (int64_t)sm.idx[2] * kC, c3);
                    if (sm.idx[3] >= 0) load16(base + (int64_t)sm.idx[3] * kC, c4);
                    load16(tile + (br * kPix + lane) * kRow + g * kCG, d);
#pragma unroll
                    for (int c = 0; c < kCG; ++c) {
                        gh += d[c] * (sm.hw * (c3[c] - c1[c]) + sm.lw * (c4[c] - c2[c]));
                        gw += d[c] * (sm.hh * (c2[c] - c1[c]) + sm.lh * (c4[c] - c3[c]));
                    }
                }
                *reinterpret_cast<float2 *>(doff + pix * (2 * kOffCh) + br * kOffCh + g * 2 * kTaps + 2 * tap) = make_float2(gh, gw);
            }
        }
        __syncthreads();

        // ---- 3. scatter of this wave's 2 groups x 64 pixels x 4 corners: 16 lanes (channels) per corner
        if (dx) {
            const int ch = lane & 15;
#pragma unroll 4
            for (int it = 0; it < 2 * kPix; ++it) {
                const int k = it >> 6, m = it & 63;  // group g0 + k, pixel m; corner lq
                const int g = g0 + k;
                const int e = ((br * kPix + m) * kG + g) * 4 + lq;
                const int ip = s_idx[e];
                if (ip >= 0) atomicAdd(dx + (int64_t)ip * kC + g * kCG + ch, s_wt[e] * tile[(br * kPix + m) * kRow + g * kCG + ch]);
            }
        }
        __syncthreads();  // tile and corner list are rewritten by the next tap
    }
}

// one (chunk, tap, branch): partial[ci][co] = sum over the chunk's pixels of col[pixel][ci] dyr[pixel][co]
__global__ void __launch_bounds__(256) deform_adapt_bwd_wpartial(const float *__restrict__ x, const float *__restrict__ offsets, const float *__restrict__ y,
                                                                 const float *__restrict__ dy, float *__restrict__ partial, int n_chunks, GradParams p) {
    __shared__ __attribute__((aligned(16))) float s_col[kPix * kRowW];
    __shared__ __attribute__((aligned(16))) float s_dy[kPix * kRowW];

    const int chunk = blockIdx.x, tap = blockIdx.y, br = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int ti = tap / 3, tj = tap % 3;
    const int64_t c0 = (int64_t)chunk * kChunk;
    const int64_t c1 = c0 + kChunk < p.npix ? c0 + kChunk : p.npix;

    f32x4 acc[4];  // wave = ci tile, acc[n] = co tile n
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int64_t s0 = c0; s0 < c1; s0 += kPix) {
        // ---- gather: lane = pixel, wave = group (the forward's sample)
        {
            const int g = wave;
            const int64_t pix = s0 + lane;
            float v[kCG];
#pragma unroll
            for (int c = 0; c < kCG; ++c) v[c] = 0.f;
            if (pix < c1) {
                const int px = (int)(pix % p.W), py = (int)((pix / p.W) % p.H);
                const int64_t img = pix / ((int64_t)p.H * p.W) * p.H * p.W;
                const float2 o = *reinterpret_cast<const float2 *>(offsets + pix * (2 * kOffCh) + br * kOffCh + g * 2 * kTaps + 2 * tap);
                const Sample sm = locate(py, px, ti, tj, o.x, o.y, p.H, p.W);
                if (sm.inside) {
                    const float w1 = sm.hh * sm.hw, w2 = sm.hh * sm.lw, w3 = sm.lh * sm.hw, w4 = sm.lh * sm.lw;
                    float a1[kCG], a2[kCG], a3[kCG], a4[kCG];
#pragma unroll
                    for (int c = 0; c < kCG; ++c) a1[c] = a2[c] = a3[c] = a4[c] = 0.f;
                    const float *base = x + img * kC + g * kCG;
                    if (sm.idx[0] >= 0) load16(base + (int64_t)sm.idx[0] * kC, a1);
                    if (sm.idx[1] >= 0) load16(base + (int64_t)sm.idx[1] * kC, a2);
                    if (sm.idx[2] >= 0) load16(base + (int64_t)sm.idx[2] * kC, a3);
                    if (sm.idx[3] >= 0) load16(base + (int64_t)sm.idx[3] * kC, a4);
#pragma unroll
                    for (int c = 0; c < kCG; ++c) v[c] = w1 * a1[c] + w2 * a2[c] + w3 * a3[c] + w4 * a4[c];
                }
            }
            float *dst = s_col + lane * kRowW + g * kCG;
#pragma unroll
            for (int q = 0; q < 4; ++q) reinterpret_cast<float4 *>(dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
        // ---- dyr strip [64 px][64 co]
#pragma unroll
        for (int t = tid; t < kPix * (kC / 4); t += 256) {
            const int m = t >> 4, c4 = t & 15;
            const int64_t pix = s0 + m;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pix < c1) {
                const int64_t o = pix * (2 * kC) + br * kC + c4 * 4;
                const float4 gq = *reinterpret_cast<const float4 *>(dy + o);
                const float4 mq = *reinterpret_cast<const float4 *>(y + o);
                v = make_float4(mq.x > 0.f ? gq.x : 0.f, mq.y > 0.f ? gq.y : 0.f, mq.z > 0.f ? gq.z : 0.f, mq.w > 0.f ? gq.w : 0.f);
            }
            *reinterpret_cast<float4 *>(s_dy + m * kRowW + c4 * 4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kPix / 4; ++ks) {
            const int m = ks * 4 + lq;
            const float av = s_col[m * kRowW + wave * 16 + lr];
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_dy[m * kRowW + n * 16 + lr], acc[n], 0, 0, 0);
        }
        __syncthreads();
    }

    // D layout: col = lane & 15 (co), row = 4 (lane >> 4) + r (ci)
    float *dst = partial + (((int64_t)br * kTaps + tap) * n_chunks + chunk) * (kC * kC);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(wave * 16 + lq * 4 + r) * kC + n * 16 + lr] = acc[n][r];
}

// dw[br][co][ci][tap] = sum of the (branch, tap)'s partials in chunk order
__global__ void __launch_bounds__(256) deform_adapt_bwd_wreduce(const float *__restrict__ partial, int n_chunks, float *__restrict__ dw) {
    const int t = blockIdx.x * 256 + threadIdx.x;  // (br, tap, ci, co): coalesced partial reads
    if (t >= kWtElems) return;
    const int co = t & 63, ci = (t >> 6) & 63, bt = t >> 12;
    const int tap = bt % kTaps, br = bt / kTaps;
    const float *src = partial + (int64_t)bt * n_chunks * (kC * kC) + ci * kC + co;
    float s = 0.f;
    for (int c = 0; c < n_chunks; ++c) s += src[(int64_t)c * (kC * kC)];
    dw[((br * kC + co) * kC + ci) * kTaps + tap] = s;
}

inline bool shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31) - kChunk; }

}  // namespace

extern "C" size_t fd_deform_adapt_backward_workspace_bytes(int B, int H, int W) {
    if (!shape_ok(B, H, W)) return 0;
    const int64_t npix = (int64_t)B * H * W;
    const int64_t n_chunks = (npix + kChunk - 1) / kChunk;
    return (size_t)kWtElems * sizeof(float) + (size_t)(2 * kTaps * n_chunks) * kC * kC * sizeof(float);
}

extern "C" int fd_deform_adapt_pack_weight_device(const float *w_cls, const float *w_reg, void *wpacked, fd_stream_t stream) {
    FD_REQUIRE(w_cls && w_reg && wpacked, "fd_deform_adapt_pack_weight_device: null pointer");
    FD_REQUIRE(((uintptr_t)wpacked & 15) == 0, "fd_deform_adapt_pack_weight_device: wpacked must be 16-byte aligned");
    hipLaunchKernelGGL(pack_weight_fwd, dim3((kWtElems + 255) / 256), dim3(256), 0, fd::as_stream(stream), w_cls, w_reg, (float *)wpacked);
    return fd::check_launch("fd_deform_adapt_pack_weight_device");
}

extern "C" int fd_deform_adapt_backward(const float *x, const float *offsets, const float *w_cls, const float *w_reg, const float *y, const float *dy, int B,
                                        int H, int W, int C, float *dx, float *doffsets, float *dw, void *workspace, size_t workspace_bytes,
                                        fd_stream_t stream) {
    FD_REQUIRE(x && offsets && w_cls && w_reg && y && dy, "fd_deform_adapt_backward: null input");
    FD_REQUIRE(C == kC, "fd_deform_adapt_backward: C = %d, only 64 channels (head_conv) are supported", C);
    FD_REQUIRE(shape_ok(B, H, W), "fd_deform_adapt_backward: bad shape B=%d H=%d W=%d", B, H, W);
    FD_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)offsets & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)dy & 15) == 0 &&
                   ((uintptr_t)dx & 15) == 0 && ((uintptr_t)doffsets & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
               "fd_deform_adapt_backward: x, offsets, y, dy, dx, doffsets and workspace must be 16-byte aligned");
    if (!dx && !doffsets && !dw) return FD_OK;
    FD_REQUIRE(workspace && workspace_bytes >= fd_deform_adapt_backward_workspace_bytes(B, H, W), "fd_deform_adapt_backward: workspace too small");
    GradParams p;
    p.B = B; p.H = H; p.W = W;
    p.npix = (int64_t)B * H * W;
    hipStream_t s = fd::as_stream(stream);
    float *wt = (float *)workspace;
    float *partial = wt + kWtElems;
    if (dx || doffsets) {
        if (dx) {
            const int rc = fd::fill_words(dx, 0u, (size_t)(p.npix * kC), s);
            if (rc != FD_OK) return rc;
        }
        hipLaunchKernelGGL(pack_weight_t, dim3((kWtElems + 255) / 256), dim3(256), 0, s, w_cls, w_reg, wt);
        const int64_t blocks = (p.npix + kPix - 1) / kPix;
        hipLaunchKernelGGL(deform_adapt_bwd_data, dim3((unsigned)blocks), dim3(256), 0, s, x, offsets, wt, y, dy, dx, doffsets, p);
    }
    if (dw) {
        const int n_chunks = (int)((p.npix + kChunk - 1) / kChunk);
        hipLaunchKernelGGL(deform_adapt_bwd_wpartial, dim3((unsigned)n_chunks, kTaps, 2), dim3(256), 0, s, x, offsets, y, dy, partial, n_chunks, p);
        hipLaunchKernelGGL(deform_adapt_bwd_wreduce, dim3((kWtElems + 255) / 256), dim3(256), 0, s, partial, n_chunks, dw);
    }
    return fd::check_launch("fd_deform_adapt_backward");
}
