// Sparse convolution apply for gfx950: output-stationary gather + MFMA GEMM, no scatter, no atomics.
//
// Replaces spconv 1.0's indice_conv / indice_subm_conv (gather -> per-tap cuBLAS GEMM -> scatter-add) used by
// the 21 convolutions of det3d/models/backbones/scn.py:99-141, fused with the folded BatchNorm1d, the residual
// add and the ReLU that follow them (scn.py:67-78).
//
//   out[o,:] = act( sum_k in[nbr[k][o],:] @ W[k] + bias (+ residual[o,:]) )
//
// Work decomposition: a wave owns 16*RG consecutive output rows (rows are spatially sorted by the index, so
// the rows a wave gathers are close in memory) and all COUT columns; accumulators stay in registers for all K
// taps.  The rulebook tile of the workgroup ([K][64*RG] int32) is staged once through LDS.  Per tap and per
// 16-row group a wave-wide ballot skips the MFMAs when no row of the group has that neighbour.  A operands are
// gathered straight into MFMA fragment layout with one 16-byte load per lane (row = lane&15, 16-byte chunk =
// lane>>4); B operands come from weights pre-packed in fragment order, one coalesced 1 KiB load per wave
// instruction (L2-resident: at most 1.8 MB per layer).  fp32 uses v_mfma_f32_16x16x4_f32 (exact fp32 fma
// chain), bf16 uses v_mfma_f32_16x16x32_bf16 / 16x16x16 with fp32 accumulation.
#include "fd_spconv_pack.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ inline unsigned short f2bf(float v) {
    unsigned u = __float_as_uint(v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
__device__ inline float bf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }


// ------------------------------------------------------------------------------------------------- fp32
template <int CIN, int COUT, int RG>
__global__ void __launch_bounds__(256) spconv_f32(const float *__restrict__ in, const float4 *__restrict__ wp,
                                                  const float *__restrict__ bias, const float *__restrict__ residual, int relu,
                                                  const int *__restrict__ nbr, int64_t nbr_stride, int K, int n_out,
                                                  const int *__restrict__ n_out_dev, float *__restrict__ out) {
    constexpr int ROWS_B = 64 * RG;  // rows per workgroup
    constexpr int NB = COUT / 16, NC = CIN / 16;
    __shared__ int s_nbr[fd::kSpconvMaxTaps * ROWS_B];
    const int tile = blockIdx.x;  // index order: contiguous XCD chunks concentrate the dense regions on a few XCDs (measured -10%)
    const int row0 = tile * ROWS_B;
    n_out = fd::device_count(n_out, n_out_dev);  // capacity launch (fd_common.h): workgroups past the device's count leave
    if (row0 >= n_out) return;
    for (int t = threadIdx.x; t < K * ROWS_B; t += 256) {
        int k = t / ROWS_B, r = t - k * ROWS_B;
        int64_t o = (int64_t)row0 + r;
        s_nbr[t] = (o < n_out) ? nbr[(int64_t)k * nbr_stride + o] : -1;  // rows >= n_out of the table are never read
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const int wrow = wave * 16 * RG;
    if (row0 + wrow >= n_out) return;

    f32x4 acc[RG][NB];
#pragma unroll
    for (int g = 0; g < RG; ++g)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[g][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int k = 0; k < K; ++k) {
        int idx[RG];
        bool any[RG];
        bool any_all = false;
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            idx[g] = s_nbr[k * ROWS_B + wrow + g * 16 + lrow];
            any[g] = __ballot(idx[g] >= 0) != 0ull;
            any_all = any_all || any[g];
        }
        if (!any_all) continue;
        const float4 *wk = wp + (int64_t)k * NC * NB * 64 + lane;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float4 a[RG];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                a[g] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx[g] >= 0) a[g] = *reinterpret_cast<const float4 *>(in + (int64_t)idx[g] * CIN + c * 16 + lq * 4);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float4 b = wk[(c * NB + nb) * 64];
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    if (any[g]) {
                        acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].x, b.x, acc[g][nb], 0, 0, 0);
                        acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].y, b.y, acc[g][nb], 0, 0, 0);
                        acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].z, b.z, acc[g][nb], 0, 0, 0);
                        acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].w, b.w, acc[g][nb], 0, 0, 0);
                    }
                }
            }
        }
    }
    // epilogue: C/D layout col = lane&15, row = 4*(lane>>4) + reg
#pragma unroll
    for (int g = 0; g < RG; ++g) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lrow;
            const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wrow + g * 16 + lq * 4 + r;
                if (row < n_out) {
                    float v = acc[g][nb][r] + bv;
                    if (residual) v += residual[(int64_t)row * COUT + col];
                    if (relu) v = fmaxf(v, 0.0f);
                    out[(int64_t)row * COUT + col] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- bf16
// CIN >= 32: chunks of 32 channels through v_mfma_f32_16x16x32_bf16 (8 bf16 = 16 B per lane).
// CIN == 16: one chunk of 16 channels through v_mfma_f32_16x16x16_bf16 (4 bf16 = 8 B per lane).
template <int CIN, int COUT, int RG>
__global__ void __launch_bounds__(256) spconv_bf16(const unsigned short *__restrict__ in, const void *__restrict__ wp_,
                                                   const float *__restrict__ bias, const unsigned short *__restrict__ residual,
                                                   int relu, const int *__restrict__ nbr, int64_t nbr_stride, int K, int n_out,
                                                   const int *__restrict__ n_out_dev, unsigned short *__restrict__ out) {
    constexpr int ROWS_B = 64 * RG;
    constexpr int NB = COUT / 16;
    constexpr bool WIDE = CIN >= 32;
    constexpr int NC = WIDE ? CIN / 32 : 1;
    __shared__ int s_nbr[fd::kSpconvMaxTaps * ROWS_B];
    const int tile = blockIdx.x;  // index order: contiguous XCD chunks concentrate the dense regions on a few XCDs (measured -10%)
    const int row0 = tile * ROWS_B;
    n_out = fd::device_count(n_out, n_out_dev);  // capacity launch (fd_common.h): workgroups past the device's count leave
    if (row0 >= n_out) return;
    for (int t = threadIdx.x; t < K * ROWS_B; t += 256) {
        int k = t / ROWS_B, r = t - k * ROWS_B;
        int64_t o = (int64_t)row0 + r;
        s_nbr[t] = (o < n_out) ? nbr[(int64_t)k * nbr_stride + o] : -1;  // rows >= n_out of the table are never read
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lrow = lane & 15, lq = lane >> 4;
    const int wrow = wave * 16 * RG;
    if (row0 + wrow >= n_out) return;

    f32x4 acc[RG][NB];
#pragma unroll
    for (int g = 0; g < RG; ++g)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[g][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int k = 0; k < K; ++k) {
        int idx[RG];
        bool any[RG];
        bool any_all = false;
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            idx[g] = s_nbr[k * ROWS_B + wrow + g * 16 + lrow];
            any[g] = __ballot(idx[g] >= 0) != 0ull;
            any_all = any_all || any[g];
        }
        if (!any_all) continue;
        if constexpr (WIDE) {
            const bf16x8 *wk = reinterpret_cast<const bf16x8 *>(wp_) + (int64_t)k * NC * NB * 64 + lane;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                bf16x8 a[RG];
#pragma unroll
                for (int g = 0; g < RG; ++g) {
                    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
                    if (idx[g] >= 0) raw = *reinterpret_cast<const uint4 *>(in + (int64_t)idx[g] * CIN + c * 32 + lq * 8);
                    a[g] = __builtin_bit_cast(bf16x8, raw);
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const bf16x8 b = wk[(c * NB + nb) * 64];
#pragma unroll
                    for (int g = 0; g < RG; ++g)
                        if (any[g]) acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[g], b, acc[g][nb], 0, 0, 0);
                }
            }
        } else {
            const s16x4 *wk = reinterpret_cast<const s16x4 *>(wp_) + (int64_t)k * NB * 64 + lane;
            s16x4 a[RG];
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                uint2 raw = make_uint2(0u, 0u);
                if (idx[g] >= 0) raw = *reinterpret_cast<const uint2 *>(in + (int64_t)idx[g] * CIN + lq * 4);
                a[g] = __builtin_bit_cast(s16x4, raw);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const s16x4 b = wk[nb * 64];
#pragma unroll
                for (int g = 0; g < RG; ++g)
                    if (any[g]) acc[g][nb] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a[g], b, acc[g][nb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < RG; ++g) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = nb * 16 + lrow;
            const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + wrow + g * 16 + lq * 4 + r;
                if (row < n_out) {
                    float v = acc[g][nb][r] + bv;
                    if (residual) v += bf2f(residual[(int64_t)row * COUT + col]);
                    if (relu) v = fmaxf(v, 0.0f);
                    out[(int64_t)row * COUT + col] = f2bf(v);
                }
            }
        }
    }
}

template <int CIN, int COUT, int RG>
void launch(const fd::SpconvCall &a) {
    const int rows_b = 64 * RG;
    dim3 grid((unsigned)((a.n_out + rows_b - 1) / rows_b));
    const void *wp = (const char *)a.wpacked + fd::spconv_weight_layout(a).base.offset;
    if (a.dtype == 0)
        hipLaunchKernelGGL((spconv_f32<CIN, COUT, RG>), grid, dim3(256), 0, a.stream, (const float *)a.in, (const float4 *)wp, a.bias,
                           (const float *)a.residual, a.relu, a.nbr, a.nbr_stride, a.K, a.n_out, a.n_out_dev, (float *)a.out);
    else
        hipLaunchKernelGGL((spconv_bf16<CIN, COUT, RG>), grid, dim3(256), 0, a.stream, (const unsigned short *)a.in, wp, a.bias,
                           (const unsigned short *)a.residual, a.relu, a.nbr, a.nbr_stride, a.K, a.n_out, a.n_out_dev, (unsigned short *)a.out);
}

template <int CIN, int COUT>
void launch_rg(const fd::SpconvCall &a, int rg) {
    if (rg >= 4) launch<CIN, COUT, 4>(a);
    else if (rg == 2) launch<CIN, COUT, 2>(a);
    else launch<CIN, COUT, 1>(a);
}

int pick_rg(int64_t n_out, int cin, int cout) {
    const int forced = fd::tuning(fd::kTuneSpconvRG);  // tuning / test override (fd_tuning_set)
    if (forced > 0) return forced;
    // Measured on MI355X (tools/spconv_bench.py, 300k-point cloud): the kernel is bound by the L2->L1 weight stream
    // (every wave reads all of W[k] per tap), so more rows per wave (RG) help until the wave count drops below
    // ~2 per SIMD, where gather latency is no longer hidden.  128-wide layers have few rows: RG 1; 64-wide: RG 2.
    const int64_t waves2 = (n_out + 31) / 32;
    int rg = (cin * cout >= 128 * 128) ? 1 : 2;
    if (rg == 2 && waves2 < 256 * 4 * 2) rg = 1;
    return rg;
}

}  // namespace

extern "C" size_t fd_spconv_packed_weight_bytes(int K, int cin, int cout, int dtype) {
    if (K <= 0 || cin <= 0 || cout <= 0) return 0;
    return fd::spconv_weight_layout(K, cin, cout, dtype).total;
}

// the element order: fd_spconv_pack.h
extern "C" int fd_spconv_pack_weight(const float *w, int K, int cin, int cout, int dtype, void *dst) {
    if (const int rc = fd::spconv_pack_check("fd_spconv_pack_weight", w, dst, K, cin, cout, dtype, 0)) return rc;
    fd::spconv_pack_weight_host(w, K, cin, cout, dtype, dst);
    return FD_OK;
}

namespace {
int spconv_apply(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu, const int32_t *nbr,
                 int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out, const int32_t *n_out_dev, int64_t n_expected, int cin,
                 int cout, int dtype, void *out_feats, fd_stream_t stream, const int32_t *plan, int64_t plan_stride, int layout = 0) {
    FD_REQUIRE(K >= 1 && K <= fd::kSpconvMaxTaps, "fd_spconv_apply: K must be in [1,27]");
    FD_REQUIRE(dtype == 0 || dtype == 1, "fd_spconv_apply: dtype must be 0 (f32) or 1 (bf16)");
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31), "fd_spconv_apply: n_out out of range");
    FD_REQUIRE(n_ranges >= 0 && (ranges == nullptr || n_ranges >= 1), "fd_spconv_apply: ranges needs n_ranges >= 1");
    if (n_expected <= 0 || n_expected > n_out) n_expected = n_out;  // only steers launch heuristics
    if (n_out == 0) return FD_OK;  // an empty active set (empty cloud): nothing to compute, buffers may be null
    FD_REQUIRE(in_feats && wpacked && (nbr || plan) && out_feats, "fd_spconv_apply: null argument");
    const fd::SpconvCall c{in_feats, n_in, wpacked, bias, residual, relu, nbr, nbr_stride, ranges, n_ranges, K, (int)n_out, n_out_dev, n_expected,
                           cin, cout, dtype, out_feats, fd::as_stream(stream), plan, plan_stride, layout};
    if (layout) {
        // bank-spread tensors (fd_spconv_apply_layout): only the pair-compacting fp32 kernels read or write them, and only in the
        // instantiations built for it -- every other launch is refused, nothing falls back to a kernel that would read plain rows
        FD_REQUIRE((layout & ~7) == 0, "fd_spconv_apply_layout: layout has bits 0 (input), 1 (residual), 2 (output)");
        int launched = 0;
        if (dtype == 0 && !fd::tuning(fd::kTuneSpconvV1)) {
            if (fd::tuning(fd::kTuneSpconvC32) >= 0) launched = fd::spconv_f32_c32_dispatch(c);
            if (!launched) launched = fd::spconv_f32_compact_dispatch(c);
        }
        if (launched) return fd::check_launch("fd_spconv_apply_layout");
        fd::set_error("fd_spconv_apply_layout: no kernel runs %d -> %d (dtype %d) with layout %d: bank-spread rows are for the fp32 32 -> 32, 64 -> 64 and "
                      "128 -> 128 layers (all bits) and the outputs of 16 -> 32, 32 -> 64 and 64 -> 128 (bit 2)", cin, cout, dtype, layout);
        return FD_EINVAL;
    }
    if (dtype == 0 && !fd::tuning(fd::kTuneSpconvV1) && cin == 16 && fd::tuning(fd::kTuneF32ResRG) >= 0) {
        // the 16-channel level: resident weights + register accumulators + empty-item skipping (fd_spconv_f32r.hip); "f32_res_rg" = -1
        // keeps the pair-compacting kernel for A/B runs
        if (fd::spconv_f32_res16_dispatch(c)) return fd::check_launch("fd_spconv_apply(f32 resident)");
    }
    if (dtype == 0 && !fd::tuning(fd::kTuneSpconvV1) && fd::tuning(fd::kTuneSpconvC32) >= 0) {
        // 32 -> 32: 32-pair items on the 32x32x2 MFMA (fd_spconv_c32.hip)
        if (fd::spconv_f32_c32_dispatch(c)) return fd::check_launch("fd_spconv_apply(c32)");
    }
    if (dtype == 0 && !fd::tuning(fd::kTuneSpconvV1)) {
        // fp32 is MFMA-bound: the pair-compacting kernel (fd_spconv_v2.hip) feeds the matrix core no zero rows
        if (fd::spconv_f32_compact_dispatch(c)) return fd::check_launch("fd_spconv_apply(compact)");
    }
    if (dtype == 1 && fd::tuning(fd::kTuneBf16GP) >= 0) {
        // 64 -> 64, 128 -> 128 (the SubM layers of levels 2 and 3): LDS window of input rows + 32-row register tiles
        // (fd_spconv_bf16win.hip); "bf16_win" = -1 keeps the RING / RESIDENT kernels (A/B runs, variant tests)
        // The window [row - HALO, row + TM + HALO] only holds the neighbours when input rows lie around the output rows, i.e. for a SubM
        // convolution (27 taps over the SAME row set).  The strided 128 -> 128 extra_conv (K = 3, stride (2,1,1)) has the shape but not the
        // property: every lane would take the exec-masked global gather next to a window staged for nothing -> RING kernel.
        const bool subm_like = K == 27 && n_in == n_out;
        if (fd::tuning(fd::kTuneBf16Win) >= 0 && subm_like && fd::spconv_bf16_win_dispatch(c)) return fd::check_launch("fd_spconv_apply(bf16 window)");
        // register accumulators + LDS-shared weights (fd_spconv_bf16.hip)
        if (fd::spconv_bf16_ws_dispatch(c)) return fd::check_launch("fd_spconv_apply(bf16 ws)");
    }
    if (!nbr) {  // (fd_spconv_apply_plan without a table: only the kernels above read a plan)
        fd::set_error("fd_spconv_apply_plan: no kernel runs %d -> %d on %lld input rows from a chunk plan alone: pass the rulebook table", cin, cout,
                      (long long)n_in);
        return FD_EINVAL;
    }
    // what is left below: the register-resident output-stationary kernels of round 1 -- the path for feature matrices of 2 GB and
    // more (the kernels above address rows through 32-bit buffer offsets) and the A/B partner of the variant tests
    const int rg = pick_rg(n_expected, cin, cout);
    const int key = cin * 1000 + cout;
    switch (key) {
        case 16016: launch_rg<16, 16>(c, rg); break;
        case 16032: launch_rg<16, 32>(c, rg); break;
        case 32032: launch_rg<32, 32>(c, rg); break;
        case 32064: launch_rg<32, 64>(c, rg); break;
        case 64064: launch_rg<64, 64>(c, rg); break;
        case 64128: launch_rg<64, 128>(c, rg); break;
        case 128128: launch_rg<128, 128>(c, rg); break;
        default:
            fd::set_error("fd_spconv_apply: unsupported channels %d -> %d", cin, cout);
            return FD_EINVAL;
    }
    return fd::check_launch("fd_spconv_apply");
}
}  // namespace

extern "C" int fd_spconv_apply(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu,
                               const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out,
                               const int32_t *n_out_dev, int64_t n_expected, int cin, int cout, int dtype, void *out_feats, fd_stream_t stream) {
    return spconv_apply(in_feats, n_in, wpacked, bias, residual, relu, nbr, nbr_stride, ranges, n_ranges, K, n_out, n_out_dev, n_expected, cin, cout,
                        dtype, out_feats, stream, nullptr, 0);
}

// fd_spconv_apply with the rulebook's chunk plan (fd_spconv_plan_build): the kernels that take one (fd_spconv_plan_wanted) read their
// chunks' compacted lists from it, every other kernel ignores it.  The same results bit for bit.
// nbr == NULL: the plan came straight from the index (fd_spconv_plan_from_index) and there is no table; only for the shapes of
// fd_spconv_index_plan_wanted, whose kernels read nothing else.
extern "C" int fd_spconv_apply_plan(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu,
                                    const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out,
                                    const int32_t *n_out_dev, int64_t n_expected, int cin, int cout, int dtype, void *out_feats,
                                    const int32_t *plan, int64_t plan_stride, fd_stream_t stream) {
    FD_REQUIRE(nbr || plan, "fd_spconv_apply_plan: nbr == NULL needs a chunk plan (fd_spconv_plan_from_index)");
    if (plan) {
        FD_REQUIRE(K == fd::kSpconvMaxTaps && dtype == 0, "fd_spconv_apply_plan: a chunk plan belongs to an fp32 layer of K = 27 taps");
        FD_REQUIRE(nbr == nullptr || cin == cout, "fd_spconv_apply_plan: next to a rulebook table a chunk plan belongs to an fp32 SubM layer (K = 27)");
        FD_REQUIRE(plan_stride >= fd_spconv_plan_stride(n_out), "fd_spconv_apply_plan: plan_stride below fd_spconv_plan_stride(n_out)");
        if (!nbr) {
            FD_REQUIRE(fd_spconv_index_plan_wanted(cin, cout, dtype),
                       "fd_spconv_apply_plan: nbr == NULL, but no kernel runs this layer shape from a chunk plan alone (fd_spconv_index_plan_wanted)");
        } else if (!fd_spconv_plan_wanted(cin, cout, dtype)) {
            plan = nullptr;  // switched off, or a shape without the path: in-kernel compaction
        }
    }
    return spconv_apply(in_feats, n_in, wpacked, bias, residual, relu, nbr, nbr_stride, ranges, n_ranges, K, n_out, n_out_dev, n_expected, cin, cout,
                        dtype, out_feats, stream, plan, plan_stride);
}

// The layout bits fd_spconv_apply_layout should be given for a layer of this shape inside a level whose inner tensors are ours to lay
// out (0: plain rows): all three for the SubM layers of a bank-spread level, bit 2 for the strided layer that writes the level's first
// tensor.  "spconv_swz": -1 none, 0 the levels that measured faster (kSwzDefaultLevels), > 0 a mask of levels (1: the 32-channel level,
// 2: 64, 4: 128) for A/B runs.  Serial sweeps, layout on against off in one build: the four 32 -> 32 launches 845 -> 837 us,
// the 64 -> 64 launches 1524 -> 1528 us (nothing), the 128 -> 128 launches 2303 -> 2315 us (slower): only the 32-channel level is on.
constexpr int kSwzDefaultLevels = 1;
extern "C" int fd_spconv_layout_wanted(int cin, int cout, int dtype) {
    const int knob = fd::tuning(fd::kTuneSpconvSwz);
    if (dtype != 0 || knob < 0 || fd::tuning(fd::kTuneSpconvV1)) return 0;
    const int levels = knob == 0 ? kSwzDefaultLevels : knob;
    const int level = cout == 32 ? 1 : cout == 64 ? 2 : cout == 128 ? 4 : 0;
    if (!(levels & level)) return 0;
    if (cin == cout) return (cout == 32 && fd::tuning(fd::kTuneSpconvC32) < 0) ? 0 : 7;  // (32 -> 32: only the 32-pair kernel has the gather)
    return 2 * cin == cout ? 4 : 0;
}

// fd_spconv_apply_plan with a layout word: which of the launch's tensors are stored bank-spread (fd_spconv_chunk.h: 16-byte piece s of
// row r at piece s ^ (r & 7) of its 128-byte line) -- bit 0 the input rows, bit 1 the residual, bit 2 the output.  For tensors that only
// these kernels read, i.e. a level's inner tensors; the values are those of the plain launch bit for bit, only where they sit changes.
// layout == 0 is fd_spconv_apply_plan.  A shape without an instantiation for the layout is refused (FD_EINVAL), nothing is launched.
extern "C" int fd_spconv_apply_layout(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu,
                                      const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out,
                                      const int32_t *n_out_dev, int64_t n_expected, int cin, int cout, int dtype, void *out_feats,
                                      const int32_t *plan, int64_t plan_stride, int layout, fd_stream_t stream) {
    if (layout == 0)
        return fd_spconv_apply_plan(in_feats, n_in, wpacked, bias, residual, relu, nbr, nbr_stride, ranges, n_ranges, K, n_out, n_out_dev, n_expected,
                                    cin, cout, dtype, out_feats, plan, plan_stride, stream);
    FD_REQUIRE(nbr || plan, "fd_spconv_apply_layout: nbr == NULL needs a chunk plan (fd_spconv_plan_from_index)");
    if (plan) {
        FD_REQUIRE(K == fd::kSpconvMaxTaps, "fd_spconv_apply_layout: a chunk plan belongs to an fp32 layer of K = 27 taps");
        FD_REQUIRE(nbr == nullptr || cin == cout, "fd_spconv_apply_layout: next to a rulebook table a chunk plan belongs to an fp32 SubM layer (K = 27)");
        FD_REQUIRE(plan_stride >= fd_spconv_plan_stride(n_out), "fd_spconv_apply_layout: plan_stride below fd_spconv_plan_stride(n_out)");
        if (!nbr) {
            FD_REQUIRE(fd_spconv_index_plan_wanted(cin, cout, dtype),
                       "fd_spconv_apply_layout: nbr == NULL, but no kernel runs this layer shape from a chunk plan alone (fd_spconv_index_plan_wanted)");
        } else if (!fd_spconv_plan_wanted(cin, cout, dtype)) {
            plan = nullptr;
        }
    }
    return spconv_apply(in_feats, n_in, wpacked, bias, residual, relu, nbr, nbr_stride, ranges, n_ranges, K, n_out, n_out_dev, n_expected, cin, cout,
                        dtype, out_feats, stream, plan, plan_stride, layout);
}
