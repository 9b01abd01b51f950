// Mixed-precision training of the sparse convolution on gfx950: the bf16 weight gradient and the device-side bf16 weight packer.
//
// bf16 rows, fp32 master weights.  The forward is fd_spconv_apply(dtype = 1); the input gradient is the same call on the transposed
// problem (fd_spconv_grad.hip's header); this file adds what was missing:
//
// fd_spconv_wgrad_bf16.  dW[k] = sum_o in[nbr[k][o]]^T . dY[o] with bf16 rows and an fp32 result, on the kernel skeleton and in the
// summation order of fd_spconv_wgrad.h; this file has the bf16 rows.
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
// switched off.  A batch is 32 * max(PS, 2) pairs, so every wave of a k-step split has a k-step in it.
//
// fd_spconv_pack_weight_device_bf16.  The bytes fd_spconv_pack_weight writes for dtype 1 (base section, tap-pair section for 16
// input channels, window section for 64 -> 64 and 128 -> 128; the same round-to-nearest-even) from fp32 weights in device memory,
// of W[k], W[k]^T or W[K-1-k]^T.  One launch, no host round trip.
#include "fd_spconv_pack.h"
#include "fd_spconv_wgrad.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

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

struct RowsBf16 {
    typedef unsigned short Elem;
    typedef uint4 Piece;  // a 16-byte piece of a row
    static constexpr int kStepPairs = 32;
    static constexpr int batch_pairs(int ps) { return 32 * (ps > 2 ? ps : 2); }
    static constexpr int row_bytes(int c) { return lds_row_bytes(c); }
    static constexpr bool shape(int cin, int cout) {  // the forward layers
        const int key = cin * 1000 + cout;
        return key == 16016 || key == 16032 || key == 32032 || key == 32064 || key == 64064 || key == 64128 || key == 128128;
    }
    static constexpr const char *kShapes = "16->16, 16->32, 32->32, 32->64, 64->64, 64->128 or 128->128";
    static constexpr bool kLimit2GB = true;

    typedef bf16x8 Frag;
    template <int ROWB>
    static __device__ __forceinline__ Frag fragment(const unsigned char *img, int ks, int c0, int lane) { return tr_fragment<ROWB>(img, ks, c0, lane); }
    static __device__ __forceinline__ fd::f32x4 mma(Frag a, Frag b, fd::f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

}  // namespace

extern "C" size_t fd_spconv_wgrad_bf16_workspace_bytes(int K, int64_t n_out, int cin, int cout) {
    return fd::spconv_wgrad_workspace_bytes(K, n_out, cin, cout);
}

extern "C" int fd_spconv_wgrad_bf16(const void *in_feats, int64_t n_in, const void *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                                    const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes,
                                    fd_stream_t stream) {
    return fd::spconv_wgrad<RowsBf16>("fd_spconv_wgrad_bf16", in_feats, n_in, dy, nbr, nbr_stride, K, n_out, n_out_dev, cin, cout, dw, workspace,
                                      workspace_bytes, stream);
}

extern "C" int fd_spconv_pack_weight_device_bf16(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream) {
    return fd::spconv_pack_weight_device<uint16_t>("fd_spconv_pack_weight_device_bf16", w_kio, K, cin, cout, mode, wpacked, stream);
}
