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
// fd_spconv_wgrad.  The kernel skeleton, its summation order and the entry point's body: fd_spconv_wgrad.h.  This file has the fp32
// rows: batches of 32 pairs, fragments read from LDS as scalars, v_mfma_f32_16x16x4_f32 with four pairs per k-step.
#include "fd_spconv_pack.h"
#include "fd_spconv_wgrad.h"

namespace {

constexpr int kChunk = fd::kSpconvWgradChunk;

struct RowsF32 {
    typedef float Elem;
    typedef float4 Piece;  // a 16-byte piece of a row
    static constexpr int kStepPairs = 4;
    static constexpr int batch_pairs(int) { return 32; }  // 8 k-steps
    // 16 floats of padding: the four 16-lane groups of a read land on different bank sets
    static constexpr int row_bytes(int c) { return (c + 16) * 4; }
    static constexpr bool channels(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }
    static constexpr bool shape(int cin, int cout) { return channels(cin) && channels(cout); }
    static constexpr const char *kShapes = "16, 32, 64 or 128";
    static constexpr bool kLimit2GB = false;

    typedef float Frag;
    // pair 4 ks + lane / 16 of the image, channel c0 + lane % 16
    template <int ROWB>
    static __device__ __forceinline__ Frag fragment(const unsigned char *img, int ks, int c0, int lane) {
        return reinterpret_cast<const float *>(img)[(ks * 4 + (lane >> 4)) * (ROWB / 4) + c0 + (lane & 15)];
    }
    static __device__ __forceinline__ fd::f32x4 mma(Frag a, Frag b, fd::f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

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

__global__ void __launch_bounds__(256) rulebook_transpose(const int *__restrict__ nbr, int64_t nbr_stride, int n_out, const int *__restrict__ n_out_dev,
                                                          int64_t n_in, int *__restrict__ inv, int64_t inv_stride) {
    const int k = blockIdx.y;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= fd::device_count(n_out, n_out_dev)) return;
    const int i = nbr[(int64_t)k * nbr_stride + o];
    if (i >= 0 && i < n_in) inv[(int64_t)k * inv_stride + i] = o;  // unique: o -> o * stride - pad + k is injective per tap
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

}  // namespace

namespace fd {
void spconv_wgrad_reduce(const float *partial, int K, int cc, int n_out, const int *n_out_dev, int n_chunks, float *dw, hipStream_t stream) {
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)(((int64_t)K * cc + 255) / 256)), dim3(256), 0, stream, partial, K, cc, n_out, n_out_dev, n_chunks, dw);
}
}  // namespace fd

extern "C" size_t fd_spconv_wgrad_workspace_bytes(int K, int64_t n_out, int cin, int cout) { return fd::spconv_wgrad_workspace_bytes(K, n_out, cin, cout); }

extern "C" int fd_spconv_wgrad(const float *in_feats, int64_t n_in, const float *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                               const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes, fd_stream_t stream) {
    return fd::spconv_wgrad<RowsF32>("fd_spconv_wgrad", in_feats, n_in, dy, nbr, nbr_stride, K, n_out, n_out_dev, cin, cout, dw, workspace, workspace_bytes,
                                     stream);
}

extern "C" int fd_rulebook_transpose(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, int64_t n_in,
                                     int32_t *inv, int64_t inv_stride, fd_stream_t stream_) {
    FD_REQUIRE(K >= 1 && K <= fd::kSpconvMaxTaps, "fd_rulebook_transpose: K must be in [1,27]");
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

extern "C" int fd_spconv_pack_weight_device(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream) {
    return fd::spconv_pack_weight_device<float>("fd_spconv_pack_weight_device", w_kio, K, cin, cout, mode, wpacked, stream);
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
