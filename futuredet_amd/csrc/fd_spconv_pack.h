// The packed weights of the sparse convolution: which weight goes to which element of the buffer.  The one statement of the
// order: the host packer (fd_spconv_pack_weight) and the device packers (fd_spconv_pack_weight_device, _bf16) all walk the
// buffer's elements and ask spconv_weight_source for each one's source.
//
// The buffer holds W'(k, a, b) -- tap k < K, input channel a < ci, output channel b < co -- as sections of MFMA fragments
// (fd::spconv_weight_layout in fd_common.h has their offsets and sizes; a section of 0 bytes is absent).  A fragment is
// [64 lanes][J elements]; per section, slowest index first:
//   base  every shape; the B operand of the 16x16 MFMAs, b = 16 nb + lane % 16
//           fp32             [K][ci / 16][co / 16][lane][4]   a = 16 c + 4 (lane / 16) + j        (v_mfma_f32_16x16x4_f32, four k-steps)
//           bf16, ci >= 32   [K][ci / 32][co / 16][lane][8]   a = 32 c + 8 (lane / 16) + j        (v_mfma_f32_16x16x32_bf16)
//           bf16, ci == 16   [K][co / 16][lane][4]            a = 4 (lane / 16) + j               (v_mfma_f32_16x16x16_bf16)
//   c32   fp32 32 -> 32: the 32x32x2 fragments of fd_spconv_c32.hip
//           [K][ci / 8][lane][4]                              a = 8 c + 4 (lane / 32) + j, b = lane % 32
//   pair  bf16, ci == 16: two taps stacked along k = 32 (fd_spconv_bf16.hip), ceil(K / 2) tap pairs, zeros for the tap past K
//           [ceil(K / 2)][co / 16][lane][8]                   q = lane / 16: k = 2 u + q / 2, a = 8 (q % 2) + j, b = 16 nb + lane % 16
//   win   bf16 64 -> 64 and 128 -> 128: the A operand of v_mfma_f32_32x32x16_bf16 in the LDS-window kernel (fd_spconv_bf16win.hip),
//         SC = min(ci, 64) input channels per weight stage
//           [K][ci / SC][SC / 16][co / 32][lane][8]           a = SC h + 16 s + 8 (lane / 32) + j, b = 32 cb + lane % 32
// bf16 elements are rounded to nearest even (bf16_rne).  The device packers also write the transposed problems of the input
// gradient: mode 1 is W'(k, a, b) = W(k, b, a), mode 2 is W'(k, a, b) = W(K - 1 - k, b, a), both ci = cout, co = cin of W.
#pragma once
#include "fd_common.h"

namespace fd {

__host__ __device__ inline uint16_t bf16_rne(float v) {  // round to nearest even: torch's .to(torch.bfloat16) on finite values
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

struct WeightSource {
    int k, a, b;  // W'(k, a, b); k >= K: the element is zero
};

// the source of element t (in elements of the dtype, over all sections) of the buffer of spconv_weight_layout(K, ci, co, dtype)
__host__ __device__ inline WeightSource spconv_weight_source(const SpconvWeightLayout &lay, int ci, int co, int dtype, int64_t t) {
    const int64_t elem = dtype == 0 ? 4 : 2;
    const int64_t base_end = (int64_t)lay.base.bytes / elem, c32_end = base_end + (int64_t)lay.c32.bytes / elem,
                  pair_end = c32_end + (int64_t)lay.pair.bytes / elem;
    const int J = dtype == 1 && !(t < base_end && ci == 16) ? 8 : 4;  // elements per lane
    int64_t r = t < base_end ? t : t < c32_end ? t - base_end : t < pair_end ? t - c32_end : t - pair_end;  // index within the section
    const int j = (int)(r & (J - 1));
    r >>= J == 8 ? 3 : 2;
    const int lane = (int)(r & 63);
    r >>= 6;
    auto take = [&r](int n) {
        const int v = (int)(r % n);
        r /= n;
        return v;
    };
    WeightSource s;
    if (t < base_end) {
        const int nb = take(co / 16), c = take(ci / (4 * J));
        s.a = 4 * J * c + J * (lane >> 4) + j;
        s.b = 16 * nb + (lane & 15);
    } else if (t < c32_end) {
        const int c = take(ci / 8);
        s.a = 8 * c + 4 * (lane >> 5) + j;
        s.b = lane & 31;
    } else if (t < pair_end) {
        const int nb = take(co / 16), q = lane >> 4;
        s.a = 8 * (q & 1) + j;
        s.b = 16 * nb + (lane & 15);
        r = 2 * r + (q >> 1);
    } else {
        const int SC = ci < 64 ? ci : 64, cb = take(co / 32), ks = take(SC / 16), h = take(ci / SC);
        s.a = SC * h + 16 * ks + 8 * (lane >> 5) + j;
        s.b = 32 * cb + (lane & 31);
    }
    s.k = (int)r;
    return s;
}

// element t of the buffer from w [K][cin][cout], as T = float (dtype 0) or uint16_t (dtype 1)
template <typename T>
__host__ __device__ inline T spconv_packed_element(const float *w, int K, int cin, int cout, int mode, const SpconvWeightLayout &lay, int64_t t) {
    const WeightSource s = spconv_weight_source(lay, mode ? cout : cin, mode ? cin : cout, sizeof(T) == 4 ? 0 : 1, t);
    if (s.k >= K) return (T)0;
    const float v = mode == 0 ? w[((int64_t)s.k * cin + s.a) * cout + s.b] : w[((int64_t)(mode == 2 ? K - 1 - s.k : s.k) * cin + s.b) * cout + s.a];
    if constexpr (sizeof(T) == 4) return v;
    else return bf16_rne(v);
}

// fd_spconv_pack_weight after its checks: dst of spconv_weight_layout(K, cin, cout, dtype).total bytes, host memory
inline void spconv_pack_weight_host(const float *w, int K, int cin, int cout, int dtype, void *dst) {
    const SpconvWeightLayout lay = spconv_weight_layout(K, cin, cout, dtype);
    const int64_t n = (int64_t)(lay.total / (dtype == 0 ? 4 : 2));
    for (int64_t t = 0; t < n; ++t) {
        if (dtype == 0) ((float *)dst)[t] = spconv_packed_element<float>(w, K, cin, cout, 0, lay, t);
        else ((uint16_t *)dst)[t] = spconv_packed_element<uint16_t>(w, K, cin, cout, 0, lay, t);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) spconv_pack_weight_kernel(const float *__restrict__ w, int K, int cin, int cout, int mode, SpconvWeightLayout lay,
                                                                 T *__restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < (int64_t)(lay.total / sizeof(T))) dst[t] = spconv_packed_element<T>(w, K, cin, cout, mode, lay, t);
}

// what every packer checks, under the entry point's own name (the host packer: mode 0; a device packer: its own dtype)
inline int spconv_pack_check(const char *who, const void *w, const void *dst, int K, int cin, int cout, int dtype, int mode) {
    FD_REQUIRE(w && dst, "%s: null argument", who);
    FD_REQUIRE(K >= 1 && K <= kSpconvMaxTaps, "%s: K must be in [1,27]", who);
    FD_REQUIRE(cin % 16 == 0 && cout % 16 == 0 && cin >= 16 && cin <= 128 && cout >= 16 && cout <= 128,
               "%s: channels must be multiples of 16 in [16,128] (got %d -> %d)", who, cin, cout);
    FD_REQUIRE(dtype == 0 || dtype == 1, "%s: dtype must be 0 (f32) or 1 (bf16)", who);
    FD_REQUIRE(mode >= 0 && mode <= 2, "%s: mode must be 0 (W[k]), 1 (W[k]^T) or 2 (W[K-1-k]^T)", who);
    const int ci = mode ? cout : cin;
    FD_REQUIRE(dtype == 0 || ci == 16 || ci % 32 == 0, "%s: bf16 needs 16 input channels or a multiple of 32 (got %d)", who, ci);
    return FD_OK;
}

// fd_spconv_pack_weight_device (T = float) and fd_spconv_pack_weight_device_bf16 (T = uint16_t): the checks, then one launch
template <typename T>
int spconv_pack_weight_device(const char *who, const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream) {
    constexpr int dtype = sizeof(T) == 4 ? 0 : 1;
    if (const int rc = spconv_pack_check(who, w_kio, wpacked, K, cin, cout, dtype, mode)) return rc;
    const SpconvWeightLayout lay = spconv_weight_layout(K, mode ? cout : cin, mode ? cin : cout, dtype);
    const int64_t n = (int64_t)(lay.total / sizeof(T));
    hipLaunchKernelGGL(spconv_pack_weight_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), w_kio, K, cin, cout, mode, lay,
                       (T *)wpacked);
    return check_launch(who);
}

}  // namespace fd
