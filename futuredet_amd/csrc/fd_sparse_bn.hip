// The sparse API of the row BatchNorm kernels (fd_row_bn.h): training-mode BatchNorm1d over the rows of a sparse feature matrix x [n, C]
// (fp32 or bf16), fused with what follows it in SpMiddleResNetFHD (det3d/models/backbones/scn.py:37-176): y = act(gamma (x - mean) invstd
// + beta [+ residual]), and its backward.  One channel block (C a multiple of 16, at most 128), one parameter record filled from the
// scalar arguments, an optional residual / d_residual, and an optional row count on the device (n_dev; n is then the capacity).
#include "fd_row_bn.h"

namespace {

using row_bn::aligned16;
using row_bn::bf16_t;

inline bool channels_ok(int C) { return C >= 16 && C <= row_bn::kBlockC && C % 16 == 0; }

// What both directions check of the sizes and the workspace.
int check_sizes(const char *fn, int64_t n, const int32_t *n_dev, int C, int relu, const void *workspace, size_t workspace_bytes) {
    FD_REQUIRE(channels_ok(C), "%s: unsupported C %d: a multiple of 16 in [16, %d]", fn, C, row_bn::kBlockC);
    FD_REQUIRE(n >= 1 && n <= row_bn::kMaxRows, "%s: n out of range (%lld)", fn, (long long)n);
    FD_REQUIRE(n_dev || n >= 2, "%s: expected more than 1 value per channel (n = %lld)", fn, (long long)n);
    FD_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1 (got %d)", fn, relu);
    FD_REQUIRE(workspace, "%s: null workspace", fn);
    FD_REQUIRE(workspace_bytes >= fd_sparse_bn_workspace_bytes(n, C), "%s: workspace too small (%zu bytes, %zu needed)", fn, workspace_bytes,
               fd_sparse_bn_workspace_bytes(n, C));
    FD_REQUIRE(aligned16(workspace), "%s: the workspace must be 16-byte aligned", fn);
    return FD_OK;
}

// the one record of a call: all C channels (the backward reads gamma only)
row_bn::Launch one_record(const float *gamma, const float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked, int C,
                          float eps, double momentum) {
    row_bn::Launch L = {};
    L.g[0] = {gamma, beta, running_mean, running_var, num_batches_tracked, C, eps, momentum};
    L.n_groups = 1;
    return L;
}

// The two entry points per row type share their bodies: fn is the name the messages carry, T the row type.
template <typename T>
int forward(const char *fn, const T *x, const T *residual, const float *gamma, const float *beta, int64_t n, const int32_t *n_dev, int C,
            int relu, float eps, double momentum, T *y, float *saved, float *running_mean, float *running_var, int64_t *num_batches_tracked,
            void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(x && gamma && beta, "%s: null x, gamma or beta", fn);
    FD_REQUIRE(y && saved, "%s: null y or saved", fn);
    FD_REQUIRE(running_mean && running_var && num_batches_tracked, "%s: null running statistics", fn);
    if (int e = check_sizes(fn, n, n_dev, C, relu, workspace, workspace_bytes)) return e;
    FD_REQUIRE(eps > 0.f, "%s: eps must be > 0", fn);
    FD_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "%s: momentum must be in [0, 1]", fn);
    FD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(saved) && (!residual || aligned16(residual)),
               "%s: x, residual, y and saved must be 16-byte aligned", fn);
    return row_bn::forward<T, true>(fn, x, residual, one_record(gamma, beta, running_mean, running_var, num_batches_tracked, C, eps, momentum), n, n_dev,
                           C, relu, y, saved, workspace, fd::as_stream(stream_));
}

template <typename T>
int backward(const char *fn, const T *dy, const T *x, const T *y, const float *gamma, const float *saved, int64_t n, const int32_t *n_dev, int C,
             int relu, T *dx, T *d_residual, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(dy && x && gamma && saved, "%s: null dy, x, gamma or saved", fn);
    FD_REQUIRE(y || !relu, "%s: null y (the ReLU mask)", fn);
    FD_REQUIRE(dx && dgamma && dbeta, "%s: null dx, dgamma or dbeta", fn);
    if (int e = check_sizes(fn, n, n_dev, C, relu, workspace, workspace_bytes)) return e;
    FD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(saved) && aligned16(dx) && aligned16(d_residual),
               "%s: dy, x, y, saved, dx and d_residual must be 16-byte aligned", fn);
    return row_bn::backward<T, true>(fn, dy, x, y, saved, one_record(gamma, nullptr, nullptr, nullptr, nullptr, C, 1.f, 0.0), n, n_dev, C, relu, dx,
                            d_residual, dgamma, dbeta, workspace, fd::as_stream(stream_));
}

}  // namespace

extern "C" int fd_sparse_bn_chunk(void) { return row_bn::kChunk; }

extern "C" size_t fd_sparse_bn_workspace_bytes(int64_t n, int C) {
    if (n < 1 || n > row_bn::kMaxRows || !channels_ok(C)) return 0;
    return row_bn::workspace_bytes(n, C);
}

extern "C" int fd_sparse_bn_train_forward(const float *x, const float *residual, const float *gamma, const float *beta, int64_t n,
                                          const int32_t *n_dev, int C, int relu, float eps, double momentum, float *y, float *saved,
                                          float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                                          size_t workspace_bytes, fd_stream_t stream_) {
    return forward("fd_sparse_bn_train_forward", x, residual, gamma, beta, n, n_dev, C, relu, eps, momentum, y, saved, running_mean, running_var,
                   num_batches_tracked, workspace, workspace_bytes, stream_);
}

extern "C" int fd_sparse_bn_train_forward_bf16(const uint16_t *x, const uint16_t *residual, const float *gamma, const float *beta, int64_t n,
                                               const int32_t *n_dev, int C, int relu, float eps, double momentum, uint16_t *y, float *saved,
                                               float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                                               size_t workspace_bytes, fd_stream_t stream_) {
    return forward<bf16_t>("fd_sparse_bn_train_forward_bf16", x, residual, gamma, beta, n, n_dev, C, relu, eps, momentum, y, saved, running_mean,
                           running_var, num_batches_tracked, workspace, workspace_bytes, stream_);
}

extern "C" int fd_sparse_bn_train_backward(const float *dy, const float *x, const float *y, const float *gamma, const float *saved, int64_t n,
                                           const int32_t *n_dev, int C, int relu, float *dx, float *d_residual, float *dgamma, float *dbeta,
                                           void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    return backward("fd_sparse_bn_train_backward", dy, x, y, gamma, saved, n, n_dev, C, relu, dx, d_residual, dgamma, dbeta, workspace,
                    workspace_bytes, stream_);
}

extern "C" int fd_sparse_bn_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *gamma, const float *saved,
                                                int64_t n, const int32_t *n_dev, int C, int relu, uint16_t *dx, uint16_t *d_residual,
                                                float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    return backward<bf16_t>("fd_sparse_bn_train_backward_bf16", dy, x, y, gamma, saved, n, n_dev, C, relu, dx, d_residual, dgamma, dbeta,
                            workspace, workspace_bytes, stream_);
}
