// Mixed-precision training of the CenterHead's final convolutions: 3 x 3 / padding 1 / stride 1, cin % 32 == 0 input channels (bf16 NHWC),
// 1 <= k <= 16 output channels with a bias, result fp32 NCHW for the loss.  One launch serves every branch of a SepHead: the caller
// passes up to kMaxGroups group records (fd_head_tail_group), each with its own x (a channel slice of a wider NHWC tensor through the
// pixel stride), cin, weight, bias, k and output.
//
// All three kernels run on v_mfma_f32_16x16x32_bf16 with the k output channels padded to the 16 of the instruction:
//
//   forward  y[b][kk][p] = bias[kk] + sum over (tap, ci) of W[kk][ci][tap] . x[p + tap][ci]
//            A = weights (row kk, reduction ci), B = pixels (column = pixel, reduction ci): a lane's B operand is 8 consecutive channels of
//            one pixel, a 16-byte load straight from NHWC memory (zeros for a tap outside the map); the result leaves with 16 consecutive
//            pixels of one channel plane per 16 lanes.  Weights are rounded to bf16 (nearest even) while they are staged in LDS, kCinStage
//            input channels per round.  A wave owns kTiles tiles of kTilePix pixels; a workgroup kBlockPix pixels in flat (b, y, x) order.
//   dgrad    dx[p][ci] = sum over (tap, kk) of W[kk][ci][tap] . dy[kk][p - tap]
//            the reduction index is (tap, kk16): 9 x 16 = 144 padded to 160 = 5 MFMA steps.  A = weights (row ci), B = dy rounded to bf16
//            (column = pixel); a lane ends with 4 consecutive channels of one pixel: one 8-byte store into the group's slice of dx.
//            A workgroup owns kBlockPix pixels x kCiBlock input channels.
//   wgrad    dW[kk][ci][tap] = sum over pixels e of x[e][ci] . dy[kk][e - tap]
//            the INPUT pixels e, in flat order, are cut into chunks of kChunk; workgroup (chunk, kCiBlock channels, group) walks its chunk
//            in steps of 32 pixels, the four waves taking the steps in turn and adding their accumulators in wave order at the end, and
//            writes one fp32 [tap][ci][16] partial to the workspace; a second kernel sums the partials of every element in chunk order
//            and writes dW in the Conv2d layout.  No atomics; kChunk is a constant: the order of every addition depends on the shapes
//            only.  dbias[kk] sums the unrounded fp32 dy the same way: the centre tap's operand before its rounding, per lane in pixel
//            order, then lanes, waves and chunks in a fixed order (a tenth slot of the partial).
//
// In the forward and the weight gradient, loads under a per-lane condition (a tap outside the map, a pixel past the end) are issued
// unconditionally from an address that is always valid and their value is dropped afterwards, so that no branch stands between two
// loads; the dgrad's dy loads, where most lanes have no channel to read, stay under their condition (30 against 46 us at B = 2, 180 x 180).
//
// The two operands of every MFMA take their reduction index from the same (lane, element) map, so only the documented C/D layout
// (column = lane & 15, row = 4 (lane >> 4) + register) enters the addressing below.
#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kMaxGroups = 8;   // group records per launch
constexpr int kKPad = 16;       // output channels of the MFMA tile: k <= 16
constexpr int kTilePix = 16;    // pixels of one MFMA tile
constexpr int kTiles = 4;       // tiles per wave
constexpr int kBlockPix = 4 * kTiles * kTilePix;  // 256 pixels per workgroup (forward, dgrad)
constexpr int kCinStage = 64;   // forward: input channels of weights staged in LDS per round
constexpr int kCiBlock = 64;    // dgrad, wgrad: input channels per workgroup (16 per wave in wgrad)
constexpr int kChunk = 1024;    // wgrad: input pixels per partial -- part of the summation order, not a tuning knob
constexpr int kSlots = 10;      // wgrad: [ci][16] slots of a partial: the 9 taps, and one whose row 0 holds the bias gradient
constexpr int kStepPix = 32;    // wgrad: pixels per MFMA
static_assert(kChunk % (4 * kStepPix) == 0 && kCinStage % 32 == 0, "chunk shape");

struct Launch {
    fd_head_tail_group g[kMaxGroups];
    int64_t ws_off[kMaxGroups];  // wgrad: the group's first float in the workspace
    int B, H, W, n_pix;
};

// fp32 -> bf16, round to nearest even: gfx950's v_cvt_pk_bf16_f32, the rounding of fd_conv2d_pack_weight
__device__ __forceinline__ unsigned bf16_pair(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 p = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(unsigned, p);
}
__device__ __forceinline__ uint4 pack8(const float *v) {
    return make_uint4(bf16_pair(v[0], v[1]), bf16_pair(v[2], v[3]), bf16_pair(v[4], v[5]), bf16_pair(v[6], v[7]));
}
__device__ __forceinline__ f32x4 mfma(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------------------------------ forward
// grid: (ceil(n_pix / kBlockPix), groups)
__global__ void __launch_bounds__(256) head_tail_forward(Launch L) {
    __shared__ uint4 s_w[9 * (kCinStage / 8) * kKPad];  // [tap][8 channels][kk] x 8 bf16: 18 KB
    const fd_head_tail_group g = L.g[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int HW = L.H * L.W;
    const unsigned short *x = (const unsigned short *)g.x;

    int pix[kTiles], py[kTiles], px[kTiles];
    bool ok[kTiles];
    f32x4 acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        pix[t] = blockIdx.x * kBlockPix + (wave * kTiles + t) * kTilePix + col;
        ok[t] = pix[t] < L.n_pix;
        const int rem = pix[t] % HW;
        py[t] = rem / L.W;
        px[t] = rem - py[t] * L.W;
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    for (int c0 = 0; c0 < g.cin; c0 += kCinStage) {
        const int cs = min(kCinStage, g.cin - c0), c8n = cs >> 3;
        if (c0) __syncthreads();
        for (int id = tid; id < 9 * c8n * kKPad; id += 256) {
            const int kk = id & 15, rest = id >> 4, c8 = rest % c8n, tap = rest / c8n;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float t = g.w[((int64_t)min(kk, g.k - 1) * g.cin + c0 + c8 * 8 + j) * 9 + tap];
                v[j] = kk < g.k ? t : 0.0f;
            }
            s_w[(tap * (kCinStage / 8) + c8) * kKPad + kk] = pack8(v);
        }
        __syncthreads();
        const int ns = cs / 32;  // (uniform) 1 or 2 MFMA steps of 32 channels
        for (int ky = 0; ky < 3; ++ky) {
            // one kernel row: its up to 3 x 2 x kTiles loads are issued before the first MFMA waits for one
            uint4 b[3][kCinStage / 32][kTiles];
#pragma unroll
            for (int t = 0; t < kTiles; ++t) {
                const bool row_ok = ok[t] && (unsigned)(py[t] + ky - 1) < (unsigned)L.H;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    // every load is issued, a tap outside the map from pixel 0, and its value dropped afterwards: no branch per load
                    const bool valid = row_ok && (unsigned)(px[t] + kx - 1) < (unsigned)L.W;
                    const unsigned short *src = x + (int64_t)(valid ? pix[t] + (ky - 1) * L.W + kx - 1 : 0) * g.x_stride + c0 + q * 8;
#pragma unroll
                    for (int s = 0; s < kCinStage / 32; ++s) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(src + (s < ns ? s * 32 : 0));
                        b[kx][s][t] = valid ? v : make_uint4(0u, 0u, 0u, 0u);
                    }
                }
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int s = 0; s < kCinStage / 32; ++s)
                    if (s < ns) {  // (uniform) the LDS rows behind the stage's channels are not written
                        const uint4 a = s_w[((ky * 3 + kx) * (kCinStage / 8) + s * 4 + q) * kKPad + col];
#pragma unroll
                        for (int t = 0; t < kTiles; ++t) acc[t] = mfma(a, b[kx][s][t], acc[t]);
                    }
        }
    }

    float *y = (float *)g.y;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) {
        if (!ok[t]) continue;
        const int b = pix[t] / HW, rem = pix[t] - b * HW;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = 4 * q + r;
            if (kk < g.k) y[((int64_t)b * g.k + kk) * HW + rem] = acc[t][r] + g.bias[kk];
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------------- dgrad
// grid: (ceil(n_pix / kBlockPix), ceil(max cin / kCiBlock), groups)
__global__ void __launch_bounds__(256) head_tail_dgrad(Launch L) {
    __shared__ uint4 s_w[5 * 4 * kCiBlock];  // [step][q][ci] x 8 bf16 (kk = 8 (q & 1) + j of tap 2 step + (q >> 1)): 20 KB
    const fd_head_tail_group g = L.g[blockIdx.z];
    const int c0 = blockIdx.y * kCiBlock;
    if (c0 >= g.cin) return;  // (uniform) a narrower group of this launch
    const int cw = min(kCiBlock, g.cin - c0);  // 32 or 64
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int HW = L.H * L.W;

    for (int id = tid; id < 5 * 4 * cw; id += 256) {
        const int ci = id % cw, sq = id / cw, tap = 2 * (sq >> 2) + ((sq & 3) >> 1), kk0 = 8 * (sq & 1);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = g.w[((int64_t)min(kk0 + j, g.k - 1) * g.cin + c0 + ci) * 9 + min(tap, 8)];
            v[j] = (tap < 9 && kk0 + j < g.k) ? t : 0.0f;
        }
        s_w[sq * kCiBlock + ci] = pack8(v);
    }
    __syncthreads();

    const float *dyp = (const float *)g.y;
    unsigned short *dxp = (unsigned short *)g.x;
    const int kk0 = 8 * (q & 1);
    for (int t = 0; t < kTiles; ++t) {
        const int pix = blockIdx.x * kBlockPix + (wave * kTiles + t) * kTilePix + col;
        const bool ok = pix < L.n_pix;
        const int b = pix / HW, rem = pix - b * HW, py = rem / L.W, px = rem - py * L.W;
        uint4 bfrag[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int tap = 2 * s + (q >> 1);
            const int sy = py - (tap / 3 - 1), sx = px - (tap % 3 - 1);  // the output pixel whose tap `tap` reads this input pixel
            const bool valid = ok && tap < 9 && (unsigned)sy < (unsigned)L.H && (unsigned)sx < (unsigned)L.W;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // (most lanes have no channel here: loading under the condition measured faster than dropping values)
                v[j] = 0.0f;
                if (valid && kk0 + j < g.k) v[j] = dyp[((int64_t)b * g.k + kk0 + j) * HW + sy * L.W + sx];
            }
            bfrag[s] = pack8(v);
        }
        for (int mb = 0; mb < cw / 16; ++mb) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 5; ++s) acc = mfma(s_w[(s * 4 + q) * kCiBlock + mb * 16 + col], bfrag[s], acc);
            if (ok) {
                const uint2 o = make_uint2(bf16_pair(acc[0], acc[1]), bf16_pair(acc[2], acc[3]));
                *reinterpret_cast<uint2 *>(dxp + (int64_t)pix * g.x_stride + c0 + mb * 16 + 4 * q) = o;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------------- wgrad
// grid: (chunks, ceil(max cin / kCiBlock), groups).  The four waves of a workgroup take the chunk's 32-pixel steps in turn (wave w the
// steps w, w + 4, ...), each for all kCiBlock input channels, so dy is read and rounded once per workgroup; their accumulators are then
// added in wave order through LDS.  The centre tap's unrounded dy doubles as the bias gradient's operand (the workgroups of channel
// block 0 write it to row 0 of slot 9 of their chunk).
__global__ void __launch_bounds__(256) head_tail_wgrad_partial(Launch L, float *__restrict__ ws) {
    constexpr int NMB = kCiBlock / 16;
    __shared__ f32x4 s_acc[9 * NMB * 64];  // 36 KB
    __shared__ float s_b[64];
    const fd_head_tail_group g = L.g[blockIdx.z];
    const int c0 = blockIdx.y * kCiBlock;
    if (c0 >= g.cin) return;  // (uniform per workgroup) a narrower group of this launch
    const int n_mb = min(NMB, (g.cin - c0) / 16);  // 2 or 4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, q = lane >> 4;
    const int HW = L.H * L.W, chunk = blockIdx.x;
    const int e_end = min(L.n_pix, (chunk + 1) * kChunk);
    const unsigned short *x = (const unsigned short *)g.x + c0 + col;
    const float *dyp = (const float *)g.y;
    const bool kk_ok = col < g.k;

    f32x4 acc[9][NMB];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) acc[tap][mb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float bsum = 0.0f;

    for (int e0 = chunk * kChunk + wave * kStepPix; e0 < e_end; e0 += 4 * kStepPix) {
        const int e = e0 + 8 * q;  // this lane's 8 pixels: e .. e + 7
        int ey[8], ex[8];
        int64_t plane[8];  // offset of dy[b][col][0][0]
        bool have[8];
        int b = e / HW, rem = e - b * HW, yy = rem / L.W, xx = rem - yy * L.W;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            have[j] = e + j < e_end;
            ey[j] = yy; ex[j] = xx;
            plane[j] = ((int64_t)b * g.k + col) * HW;
            if (++xx == L.W) {
                xx = 0;
                if (++yy == L.H) { yy = 0; ++b; }
            }
        }
        uint4 a[NMB];
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb) {
            unsigned xa[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // every load is issued, from pixel 0 where there is nothing to read, and dropped afterwards
                const unsigned v = (unsigned)x[(int64_t)(have[j] ? e + j : 0) * g.x_stride + (mb < n_mb ? mb * 16 : 0)];
                xa[j] = (have[j] && mb < n_mb) ? v : 0u;
            }
            a[mb] = make_uint4(xa[0] | (xa[1] << 16), xa[2] | (xa[3] << 16), xa[4] | (xa[5] << 16), xa[6] | (xa[7] << 16));
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int sy = ey[j] - dy, sx = ex[j] - dx;
                const bool valid = kk_ok && have[j] && (unsigned)sy < (unsigned)L.H && (unsigned)sx < (unsigned)L.W;
                const float t = dyp[valid ? plane[j] + sy * L.W + sx : 0];
                v[j] = valid ? t : 0.0f;
            }
            if (tap == 4) {
#pragma unroll
                for (int j = 0; j < 8; ++j) bsum += v[j];
            }
            const uint4 bfrag = pack8(v);
#pragma unroll
            for (int mb = 0; mb < NMB; ++mb)
                if (mb < n_mb) acc[tap][mb] = mfma(a[mb], bfrag, acc[tap][mb]);  // (uniform)
        }
    }

    // the four 8-pixel groups of a step, then the four waves, in a fixed order
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int mb = 0; mb < NMB; ++mb) s_acc[(tap * NMB + mb) * 64 + lane] = acc[tap][mb];
            s_b[lane] = bsum;
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int mb = 0; mb < NMB; ++mb) acc[tap][mb] += s_acc[(tap * NMB + mb) * 64 + lane];
            bsum += s_b[lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;

    // the partial [chunk][tap][ci][16]: row (ci) = 4 q + r, column (kk) = lane & 15; columns >= k hold zeros
    float *dst = ws + L.ws_off[blockIdx.z] + (int64_t)chunk * kSlots * g.cin * kKPad;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int mb = 0; mb < NMB; ++mb)
            if (mb < n_mb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[((int64_t)tap * g.cin + c0 + mb * 16 + 4 * q + r) * kKPad + col] = acc[tap][mb][r];
            }
    if (blockIdx.y == 0 && q == 0) dst[(int64_t)9 * g.cin * kKPad + col] = bsum;
}

// grid: (ceil((9 max cin + 1) 16 / 256), groups): dW[kk][ci][tap] = sum over chunks, in chunk order, of partial[chunk][tap][ci][kk];
// dbias[kk] the same sum of partial[chunk][9][0][kk]
__global__ void __launch_bounds__(256) head_tail_wgrad_reduce(Launch L, const float *__restrict__ ws, int n_chunks) {
    const fd_head_tail_group g = L.g[blockIdx.y];
    const int64_t n_dw = (int64_t)9 * g.cin * kKPad, per_chunk = (int64_t)kSlots * g.cin * kKPad;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_dw + kKPad) return;
    const int kk = (int)(e & 15);
    if (kk >= g.k) return;
    const float *src = ws + L.ws_off[blockIdx.y] + e;
    float s = 0.0f;
    for (int c = 0; c < n_chunks; ++c) s += src[c * per_chunk];
    if (e >= n_dw) {
        g.bias[kk] = s;
        return;
    }
    const int64_t t = e >> 4;
    const int ci = (int)(t % g.cin), tap = (int)(t / g.cin);
    g.w[((int64_t)kk * g.cin + ci) * 9 + tap] = s;
}

// Everything an entry point checks before it touches the device; `what` is its name.  need_bias: the bias pointer is read or written.
int validate(const char *what, const fd_head_tail_group *groups, int n_groups, int B, int H, int W, bool need_bias, Launch *L) {
    FD_REQUIRE(groups, "%s: null argument (groups)", what);
    FD_REQUIRE(n_groups >= 1 && n_groups <= kMaxGroups, "%s: too many groups: n_groups must be in [1, %d] (got %d)", what, kMaxGroups, n_groups);
    FD_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape %d x %d x %d", what, B, H, W);
    const int64_t n_pix = (int64_t)B * H * W;
    FD_REQUIRE(n_pix + kChunk < (1ll << 31), "%s: maps of 2^31 pixels and more are not supported", what);
    int max_cin = 0;
    for (int i = 0; i < n_groups; ++i) {
        const fd_head_tail_group &g = groups[i];
        FD_REQUIRE(g.x && g.w && g.y && (g.bias || !need_bias), "%s: null argument (group %d)", what, i);
        FD_REQUIRE(g.k >= 1 && g.k <= kKPad, "%s: k must be in [1, %d] (group %d: %d)", what, kKPad, i, g.k);
        FD_REQUIRE(g.cin > 0 && g.cin % 32 == 0, "%s: cin must be a positive multiple of 32 (group %d: %d)", what, i, g.cin);
        FD_REQUIRE(g.x_stride >= g.cin, "%s: pixel stride below cin (group %d: %lld < %d)", what, i, (long long)g.x_stride, g.cin);
        FD_REQUIRE(g.x_stride % 8 == 0 && ((uintptr_t)g.x & 15) == 0, "%s: x must be 16-byte aligned with a pixel stride that is a multiple of 8 (group %d)",
                   what, i);
        L->g[i] = g;
        max_cin = g.cin > max_cin ? g.cin : max_cin;
    }
    L->B = B; L->H = H; L->W = W;
    L->n_pix = (int)n_pix;
    return max_cin;
}

}  // namespace

extern "C" int fd_head_tail_bf16_max_groups(void) { return kMaxGroups; }

extern "C" int fd_head_tail_wgrad_bf16_chunk(void) { return kChunk; }

extern "C" size_t fd_head_tail_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin_sum) {
    if (B <= 0 || H <= 0 || W <= 0 || cin_sum <= 0 || cin_sum % 32) return 0;
    const int64_t n_pix = (int64_t)B * H * W;
    return (size_t)((n_pix + kChunk - 1) / kChunk) * kSlots * cin_sum * kKPad * sizeof(float);
}

extern "C" int fd_head_tail_forward_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, fd_stream_t stream) {
    Launch L{};
    const int max_cin = validate("fd_head_tail_forward_bf16", groups, n_groups, B, H, W, true, &L);
    if (max_cin < 0) return max_cin;
    const dim3 grid((unsigned)((L.n_pix + kBlockPix - 1) / kBlockPix), (unsigned)n_groups);
    hipLaunchKernelGGL(head_tail_forward, grid, dim3(256), 0, fd::as_stream(stream), L);
    return fd::check_launch("fd_head_tail_forward_bf16");
}

extern "C" int fd_head_tail_dgrad_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, fd_stream_t stream) {
    Launch L{};
    const int max_cin = validate("fd_head_tail_dgrad_bf16", groups, n_groups, B, H, W, false, &L);
    if (max_cin < 0) return max_cin;
    const int gy = (max_cin + kCiBlock - 1) / kCiBlock;
    FD_REQUIRE(gy <= 65535, "fd_head_tail_dgrad_bf16: too many channel blocks (cin %d)", max_cin);
    const dim3 grid((unsigned)((L.n_pix + kBlockPix - 1) / kBlockPix), (unsigned)gy, (unsigned)n_groups);
    hipLaunchKernelGGL(head_tail_dgrad, grid, dim3(256), 0, fd::as_stream(stream), L);
    return fd::check_launch("fd_head_tail_dgrad_bf16");
}

extern "C" int fd_head_tail_wgrad_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, void *workspace, size_t workspace_bytes,
                                       fd_stream_t stream) {
    Launch L{};
    const int max_cin = validate("fd_head_tail_wgrad_bf16", groups, n_groups, B, H, W, true, &L);
    if (max_cin < 0) return max_cin;
    FD_REQUIRE(workspace, "fd_head_tail_wgrad_bf16: null argument (workspace)");
    const int n_chunks = (L.n_pix + kChunk - 1) / kChunk;
    int64_t cin_sum = 0;
    for (int i = 0; i < n_groups; ++i) {
        L.ws_off[i] = (int64_t)n_chunks * kSlots * kKPad * cin_sum;
        cin_sum += groups[i].cin;
    }
    const size_t need = (size_t)n_chunks * kSlots * (size_t)cin_sum * kKPad * sizeof(float);
    FD_REQUIRE(workspace_bytes >= need, "fd_head_tail_wgrad_bf16: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
    const int gy = (max_cin + kCiBlock - 1) / kCiBlock;
    FD_REQUIRE(gy <= 65535, "fd_head_tail_wgrad_bf16: too many channel blocks (cin %d)", max_cin);
    hipStream_t s = fd::as_stream(stream);
    float *ws = (float *)workspace;
    hipLaunchKernelGGL(head_tail_wgrad_partial, dim3((unsigned)n_chunks, (unsigned)gy, (unsigned)n_groups), dim3(256), 0, s, L, ws);
    const int64_t total = ((int64_t)9 * max_cin + 1) * kKPad;
    hipLaunchKernelGGL(head_tail_wgrad_reduce, dim3((unsigned)((total + 255) / 256), (unsigned)n_groups), dim3(256), 0, s, L, (const float *)ws, n_chunks);
    return fd::check_launch("fd_head_tail_wgrad_bf16");
}
