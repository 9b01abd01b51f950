// Two small pieces of the sync-free training step (include/futuredet_hip.h has the contracts).
//
//   fd_rows_colsum      out[c] = sum of x[r][c] over the first min(n, *n_dev) rows of a row tensor [n, C], fp32 or bf16 rows, fp32 result:
//                       the bias gradient of a block convolution when the row count lives on the device (the rows behind the count
//                       are uninitialised memory there and are never read).
//   fd_levels_overflow  flag[0] = any counts[l] > caps[l]: the `skip` input of fd_optim_adam_step_dev.
//
// colsum_partial  chunk k (kChunk rows) -> partial[k][c] in double.  A workgroup is kThreads / C row lanes of C channel threads:
//                 consecutive threads read consecutive channels of a row; lane r adds rows r, r + R, ... of the chunk in that order,
//                 then the lanes are added in lane order.  Chunks at or behind the count leave at once.
//   colsum_finish   one workgroup, same shape: lane r adds the partials of chunks r, r + R, ... below ceil(count / kChunk) in that
//                   order, the lanes are added in lane order, one rounding to fp32.
// Every sum is a double addition in one fixed order that depends on (count, C) alone: no atomics, the same bits on
// every run.
#include "fd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = FD_ROWS_COLSUM_CHUNK;
constexpr int kMaxLevels = 64;

template <bool kBf16>
__device__ __forceinline__ double load_elem(const void *x, int64_t i) {
    if (kBf16) return (double)__uint_as_float((uint32_t) reinterpret_cast<const uint16_t *>(x)[i] << 16);
    return (double)reinterpret_cast<const float *>(x)[i];
}

// sum over the row lanes of a workgroup, lane order; valid in the threads of lane 0
__device__ __forceinline__ double lanes_sum(double v, double *lds, int lanes, int C) {
    lds[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    if ((int)threadIdx.x < C)
        for (int r = 0; r < lanes; ++r) s += lds[r * C + threadIdx.x];
    return s;
}

template <bool kBf16>
__global__ void __launch_bounds__(kThreads) colsum_partial(const void *__restrict__ x, int n, const int *__restrict__ n_dev, int C,
                                                           double *__restrict__ partial) {
    __shared__ double lds[kThreads];
    const int count = fd::device_count(n, n_dev);
    const int64_t first = (int64_t)blockIdx.x * kChunk;
    if (first >= count) return;  // uniform over the workgroup
    const int rows = count - first < kChunk ? (int)(count - first) : kChunk;
    const int lanes = kThreads / C, c = threadIdx.x % C, r0 = threadIdx.x / C;
    double acc = 0.0;
    for (int r = r0; r < rows; r += lanes) acc += load_elem<kBf16>(x, (first + r) * C + c);
    const double s = lanes_sum(acc, lds, lanes, C);
    if ((int)threadIdx.x < C) partial[(int64_t)blockIdx.x * C + threadIdx.x] = s;
}

__global__ void __launch_bounds__(kThreads) colsum_finish(const double *__restrict__ partial, int n, const int *__restrict__ n_dev, int C,
                                                          float *__restrict__ out) {
    __shared__ double lds[kThreads];
    const int count = fd::device_count(n, n_dev);
    const int chunks = (count + kChunk - 1) / kChunk;
    const int lanes = kThreads / C, c = threadIdx.x % C, r0 = threadIdx.x / C;
    double acc = 0.0;
    for (int k = r0; k < chunks; k += lanes) acc += partial[(int64_t)k * C + c];
    const double s = lanes_sum(acc, lds, lanes, C);
    if ((int)threadIdx.x < C) out[threadIdx.x] = (float)s;
}

__global__ void __launch_bounds__(64) levels_overflow(const int *__restrict__ counts, const int *__restrict__ caps, int n_levels,
                                                      int *__restrict__ flag) {
    const int l = threadIdx.x;
    const int over = l < n_levels && counts[l] > caps[l];
    const unsigned long long any = __ballot(over);
    if (l == 0) flag[0] = any ? 1 : 0;
}

bool colsum_channels_ok(int C) { return C == 16 || C == 32 || C == 64 || C == 128; }

}  // namespace

extern "C" int fd_rows_colsum_chunk(void) { return kChunk; }

extern "C" size_t fd_rows_colsum_workspace_bytes(int64_t n, int C) {
    if (n < 0 || n > ((int64_t)1 << 30) || !colsum_channels_ok(C)) return 0;
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    return fd::align_up((size_t)(chunks > 0 ? chunks : 1) * C * sizeof(double), 256);
}

extern "C" int fd_rows_colsum(const void *x, int64_t n, const int32_t *n_dev, int C, int dtype, float *out, void *workspace, size_t workspace_bytes,
                              fd_stream_t stream_) {
    FD_REQUIRE(colsum_channels_ok(C), "fd_rows_colsum: C must be 16, 32, 64 or 128 (got %d)", C);
    FD_REQUIRE(dtype == 0 || dtype == 1, "fd_rows_colsum: dtype must be 0 (fp32) or 1 (bf16), got %d", dtype);
    FD_REQUIRE(n >= 0 && n <= ((int64_t)1 << 30), "fd_rows_colsum: n (%lld) must lie in [0, 2^30]", (long long)n);
    FD_REQUIRE(out, "fd_rows_colsum: null out");
    FD_REQUIRE(x || n == 0, "fd_rows_colsum: null rows");
    FD_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "fd_rows_colsum: the workspace must be non-null and 16-byte aligned");
    FD_REQUIRE(workspace_bytes >= fd_rows_colsum_workspace_bytes(n, C), "fd_rows_colsum: workspace of %zu bytes, %zu needed", workspace_bytes,
               fd_rows_colsum_workspace_bytes(n, C));
    hipStream_t st = fd::as_stream(stream_);
    const unsigned chunks = (unsigned)((n + kChunk - 1) / kChunk);
    double *partial = reinterpret_cast<double *>(workspace);
    if (chunks) {
        if (dtype == 1)
            hipLaunchKernelGGL(colsum_partial<true>, dim3(chunks), dim3(kThreads), 0, st, x, (int)n, n_dev, C, partial);
        else
            hipLaunchKernelGGL(colsum_partial<false>, dim3(chunks), dim3(kThreads), 0, st, x, (int)n, n_dev, C, partial);
    }
    hipLaunchKernelGGL(colsum_finish, dim3(1), dim3(kThreads), 0, st, partial, (int)n, n_dev, C, out);
    return fd::check_launch("fd_rows_colsum");
}

extern "C" int fd_levels_overflow(const int32_t *counts, const int32_t *caps, int n_levels, int32_t *flag, fd_stream_t stream_) {
    FD_REQUIRE(counts && caps && flag, "fd_levels_overflow: null counts, caps or flag");
    FD_REQUIRE(n_levels >= 1 && n_levels <= kMaxLevels, "fd_levels_overflow: n_levels (%d) must lie in [1, %d]", n_levels, kMaxLevels);
    hipLaunchKernelGGL(levels_overflow, dim3(1), dim3(64), 0, fd::as_stream(stream_), counts, caps, n_levels, flag);
    return fd::check_launch("fd_levels_overflow");
}
