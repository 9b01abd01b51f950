// The channels-last API of the row BatchNorm kernels (fd_row_bn.h): training-mode BatchNorm2d over a bf16 channels-last map of the dense
// half (RPN, CenterHead in mixed precision), fused with the ReLU that follows it: the map is rows x [n = B H W, C] (bf16, row-major),
// y = act(gamma (x - mean) invstd + beta), and its backward.  C is any multiple of 32 in [32, 512] (up to four channel blocks); one call
// normalises the channel ranges of up to kMaxRecords BatchNorm2d modules (fd_dense_bn_nhwc_group records).  No residual, and the row
// count comes from the host.
#include "fd_row_bn.h"

namespace {

using row_bn::aligned16;
using row_bn::kMaxRecords;
using row_bn::kMaxRows;
using row_bn::Launch;

constexpr int kMaxC = 512;

inline bool channels_ok(int C) { return C >= 32 && C <= kMaxC && C % 32 == 0; }

// What both entry points check of the sizes, the records' channel counts and the workspace; fills the launch structure.
int check_call(const char *fn, const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu, const void *workspace,
               size_t workspace_bytes, Launch &L) {
    FD_REQUIRE(groups, "%s: null groups", fn);
    FD_REQUIRE(n_groups >= 1 && n_groups <= kMaxRecords, "%s: n_groups must be in [1, %d] (got %d)", fn, kMaxRecords, n_groups);
    FD_REQUIRE(channels_ok(C), "%s: unsupported C %d: a multiple of 32 in [32, %d]", fn, C, kMaxC);
    int64_t sum = 0;
    for (int j = 0; j < n_groups; ++j) {
        FD_REQUIRE(groups[j].c >= 32 && groups[j].c <= kMaxC && groups[j].c % 32 == 0,
                   "%s: group %d: unsupported c %d: a multiple of 32 in [32, %d]", fn, j, groups[j].c, kMaxC);
        sum += groups[j].c;
    }
    FD_REQUIRE(sum == C, "%s: the groups' c sum to %lld, not to C = %d", fn, (long long)sum, C);
    FD_REQUIRE(n >= 2 && n <= kMaxRows, "%s: n out of range (%lld): more than 1 value per channel, at most 2^30 rows", fn, (long long)n);
    FD_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1 (got %d)", fn, relu);
    FD_REQUIRE(workspace, "%s: null workspace", fn);
    FD_REQUIRE(workspace_bytes >= fd_dense_bn_nhwc_workspace_bytes(n, C), "%s: workspace too small (%zu bytes, %zu needed)", fn,
               workspace_bytes, fd_dense_bn_nhwc_workspace_bytes(n, C));
    FD_REQUIRE(aligned16(workspace), "%s: the workspace must be 16-byte aligned", fn);
    for (int j = 0; j < kMaxRecords; ++j) L.g[j] = groups[j < n_groups ? j : 0];
    L.n_groups = n_groups;
    return FD_OK;
}

}  // namespace

extern "C" int fd_dense_bn_nhwc_chunk(void) { return row_bn::kChunk; }
extern "C" int fd_dense_bn_nhwc_stat_groups(void) { return row_bn::kMaxGroups; }
extern "C" int fd_dense_bn_nhwc_apply_blocks(void) { return row_bn::kMaxApplyBlocks; }

extern "C" size_t fd_dense_bn_nhwc_workspace_bytes(int64_t n, int C) {
    if (n < 2 || n > kMaxRows || !channels_ok(C)) return 0;
    return row_bn::workspace_bytes(n, C);
}

extern "C" int fd_dense_bn_nhwc_train_forward_bf16(const uint16_t *x, const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C,
                                                   int relu, uint16_t *y, float *saved, void *workspace, size_t workspace_bytes,
                                                   fd_stream_t stream_) {
    const char *fn = "fd_dense_bn_nhwc_train_forward_bf16";
    FD_REQUIRE(x && y && saved, "%s: null x, y or saved", fn);
    Launch L;
    if (int e = check_call(fn, groups, n_groups, n, C, relu, workspace, workspace_bytes, L)) return e;
    for (int j = 0; j < n_groups; ++j) {
        const fd_dense_bn_nhwc_group &g = groups[j];
        FD_REQUIRE(g.gamma && g.beta, "%s: group %d: null gamma or beta", fn, j);
        FD_REQUIRE(g.running_mean && g.running_var && g.num_batches_tracked, "%s: group %d: null running statistics", fn, j);
        FD_REQUIRE(g.eps > 0.f, "%s: group %d: eps must be > 0", fn, j);
        FD_REQUIRE(g.momentum >= 0.0 && g.momentum <= 1.0, "%s: group %d: momentum must be in [0, 1]", fn, j);
    }
    FD_REQUIRE(aligned16(x) && aligned16(y) && aligned16(saved), "%s: x, y and saved must be 16-byte aligned", fn);
    return row_bn::forward<row_bn::bf16_t, false>(fn, x, nullptr, L, n, nullptr, C, relu, y, saved, workspace, fd::as_stream(stream_));
}

extern "C" int fd_dense_bn_nhwc_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *saved,
                                                    const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu,
                                                    uint16_t *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                                    fd_stream_t stream_) {
    const char *fn = "fd_dense_bn_nhwc_train_backward_bf16";
    FD_REQUIRE(dy && x && saved, "%s: null dy, x or saved", fn);
    FD_REQUIRE(y || relu == 0, "%s: null y (the ReLU mask)", fn);
    FD_REQUIRE(dx && dgamma && dbeta, "%s: null dx, dgamma or dbeta", fn);
    Launch L;
    if (int e = check_call(fn, groups, n_groups, n, C, relu, workspace, workspace_bytes, L)) return e;
    for (int j = 0; j < n_groups; ++j) FD_REQUIRE(groups[j].gamma, "%s: group %d: null gamma", fn, j);
    FD_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(saved) && aligned16(dx),
               "%s: dy, x, y, saved and dx must be 16-byte aligned", fn);
    return row_bn::backward<row_bn::bf16_t, false>(fn, dy, x, y, saved, L, n, nullptr, C, relu, dx, nullptr, dgamma, dbeta, workspace,
                                            fd::as_stream(stream_));
}
