// One optimiser step for a whole model: the training recipe of every shipped config -- Adam under fastai's OptimWrapper with true
// weight decay (det3d/solver/fastai_optim.py:158-174), clip_grad_norm_ (det3d/torchie/trainer/hooks/optimizer.py:9-19) and the
// beta1 / lr that OneCycle sets per iteration -- in three launches, whatever the number of tensors.  include/futuredet_hip.h has the
// table layout and the arithmetic.
//
// Work items are chunks: at most kChunk elements of one tensor, listed as (tensor, index) pairs by the host, so a workgroup finds
// its tensor without a search.  The median tensor of the shipped models has 64-128 elements (BatchNorm vectors): such a tensor is
// one chunk of its own and most of its workgroup idles; the few convolution weights that hold nearly all elements are cut into
// kChunk pieces that 256 threads walk with 16-byte accesses (4 per thread and buffer).
//
//   optim_sumsq    chunk c -> partials[c] = sum of g^2 over the chunk, in double (the squares of fp32 values are exact in double),
//                  0 for a tensor without a gradient.  Thread-strided accumulation, then a fixed shuffle tree and the four waves
//                  added in wave order.
//   optim_prepare  one workgroup: thread j adds partials j, j + 256, ... in that order, the same tree finishes; total_norm and the
//                  clip coefficient go to norm[0..1] in fp32 with clip_grad_norm_'s roundings.  Then, per tensor with a gradient:
//                  step += 1 and the two bias-correction scalars, computed in double and rounded to fp32 as torch rounds the python
//                  floats it hands to addcdiv_ / div.
//   optim_step     chunk c: decay, moments, update.
// Every sum has one fixed order that depends on the table alone: no atomics, the same bits on every run.
// fd_optim_adam_step_dev launches the same three kernels with the scalars behind a device pointer and an optional device skip flag
// (a step captured into a graph: the schedule changes lr and beta1 at every replay, and an overflowed replay must not train).
//
// Built with -ffp-contract=off: the fp32 expression of the header is what runs (torch's kernels do not contract either).
#include <math.h>

#include "fd_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = FD_OPTIM_CHUNK;
static_assert(kChunk % (kThreads * 4) == 0, "a chunk is a whole number of 16-byte accesses per thread");

struct Hyper {  // launch argument: lr and beta1 change at every iteration
    double lr, beta1, beta2, eps, wd, max_norm;
};

// Where a launch finds its scalars: in its arguments (fd_optim_adam_step), or in a device record of six doubles in Hyper's order
// (fd_optim_adam_step_dev: a captured launch bakes its arguments in, the record is read at every replay).  Both ways hand the kernels the
// same doubles, so both round them alike.  `skip` (device, may be null): non-zero = the call leaves everything but norm as it is.
struct HyperSource {
    Hyper h;
    const double *dev;
    const int32_t *skip;
};
__device__ __forceinline__ Hyper load_hyper(const HyperSource &s) {
    if (!s.dev) return s.h;
    Hyper h;
    h.lr = s.dev[0]; h.beta1 = s.dev[1]; h.beta2 = s.dev[2]; h.eps = s.dev[3]; h.wd = s.dev[4]; h.max_norm = s.dev[5];
    return h;
}
__device__ __forceinline__ bool skipped(const HyperSource &s) { return s.skip && *s.skip != 0; }

struct Table {  // fd_optim_table with its types
    const uint64_t *params;
    const int64_t *numel, *offset;
    const int32_t *flags;
    int32_t *step;
    float *coef;
    const int32_t *chunks;
    double *partials;
    float *norm;
    float *grad, *exp_avg, *exp_avg_sq;
    int n_tensors, n_chunks;
};

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ double block_sum(double v, double *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kWaves; ++w) s += lds[w];
    return s;
}

__global__ void __launch_bounds__(kThreads) optim_sumsq(Table T) {
    __shared__ double lds[kWaves];
    const int c = blockIdx.x;
    const int t = T.chunks[2 * c];
    const int64_t first = (int64_t)T.chunks[2 * c + 1] * kChunk;
    double acc = 0.0;
    if ((unsigned)t < (unsigned)T.n_tensors && (T.flags[t] & FD_OPTIM_HAS_GRAD)) {  // uniform over the workgroup
        const int64_t left = T.numel[t] - first;
        const int n = left < kChunk ? (int)left : kChunk;
        const float *__restrict__ g = T.grad + T.offset[t] + first;
        for (int i = threadIdx.x * 4; i < n; i += kThreads * 4) {
            const f32x4 G = *reinterpret_cast<const f32x4 *>(g + i);  // the segment is padded to a multiple of 4
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < n) acc += (double)G[j] * (double)G[j];
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) T.partials[c] = s;
}

__global__ void __launch_bounds__(kThreads) optim_prepare(Table T, HyperSource src, int clip) {
    __shared__ double lds[kWaves];
    const Hyper h = load_hyper(src);
    if (clip) {
        double acc = 0.0;
        for (int c = threadIdx.x; c < T.n_chunks; c += kThreads) acc += T.partials[c];
        const double s = block_sum(acc, lds);
        if (threadIdx.x == 0) {
            const float total_norm = (float)sqrt(s);
            float coef = (float)h.max_norm / (total_norm + 1e-6f);
            if (coef > 1.f) coef = 1.f;  // clamp(max = 1): a NaN norm stays a NaN coefficient, as in torch
            T.norm[0] = total_norm;
            T.norm[1] = coef;
        }
    } else if (threadIdx.x == 0) {
        T.norm[0] = 0.f;
        T.norm[1] = 1.f;
    }
    if (skipped(src)) return;  // uniform; norm is written, step counts and coefficients stay
    for (int t = threadIdx.x; t < T.n_tensors; t += kThreads) {
        if (!(T.flags[t] & FD_OPTIM_HAS_GRAD)) continue;
        const int s = T.step[t] + 1;
        T.step[t] = s;
        const double bc1 = 1.0 - pow(h.beta1, (double)s), bc2 = 1.0 - pow(h.beta2, (double)s);
        T.coef[2 * t] = (float)(h.lr / bc1);
        T.coef[2 * t + 1] = (float)sqrt(bc2);
    }
}

struct StepScalars {
    float decay, b1, omb1, b2, omb2, eps, clip, step_size, bc2_sqrt;
    bool has_grad, decays;
};

// kVec: the parameter side takes 16-byte accesses too.  The flat buffers always do: a thread's 4 elements may reach into the
// segment's zero padding, where moments are written back as zeros.
template <bool kVec>
__device__ __forceinline__ void step_chunk(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                           int n, const StepScalars &k) {
    for (int i = threadIdx.x * 4; i < n; i += kThreads * 4) {
        const int cnt = n - i < 4 ? n - i : 4;
        f32x4 P, G, M, V;
        if (kVec) {
            P = *reinterpret_cast<const f32x4 *>(p + i);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) P[j] = j < cnt ? p[i + j] : 0.f;
        }
        if (k.has_grad) {
            G = *reinterpret_cast<const f32x4 *>(g + i);
            M = *reinterpret_cast<const f32x4 *>(m + i);
            V = *reinterpret_cast<const f32x4 *>(v + i);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x = P[j];
            if (k.decays) x = x * k.decay;
            if (k.has_grad) {
                const float gc = G[j] * k.clip;
                float mj = k.b1 * M[j] + k.omb1 * gc;
                float vj = k.b2 * V[j] + (k.omb2 * gc) * gc;
                const float denom = sqrtf(vj) / k.bc2_sqrt + k.eps;
                x = x - k.step_size * (mj / denom);
                if (j >= cnt) mj = 0.f, vj = 0.f;
                M[j] = mj;
                V[j] = vj;
            }
            P[j] = x;
        }
        if (kVec) {
            *reinterpret_cast<f32x4 *>(p + i) = P;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) p[i + j] = P[j];
        }
        if (k.has_grad) {
            *reinterpret_cast<f32x4 *>(m + i) = M;
            *reinterpret_cast<f32x4 *>(v + i) = V;
        }
    }
}

__global__ void __launch_bounds__(kThreads) optim_step(Table T, HyperSource src) {
    if (skipped(src)) return;
    const Hyper h = load_hyper(src);
    const int c = blockIdx.x;
    const int t = T.chunks[2 * c];
    if ((unsigned)t >= (unsigned)T.n_tensors) return;
    const int flags = T.flags[t];
    StepScalars k;
    k.has_grad = (flags & FD_OPTIM_HAS_GRAD) != 0;
    k.decays = (flags & FD_OPTIM_DECAY) != 0;
    if (!k.has_grad && !k.decays) return;
    const int64_t first = (int64_t)T.chunks[2 * c + 1] * kChunk;
    const int64_t numel = T.numel[t];
    const int64_t left = numel - first;
    const int n = left < kChunk ? (int)left : kChunk;
    k.decay = (float)(1.0 - h.wd * h.lr);
    k.b1 = (float)h.beta1;
    k.omb1 = (float)(1.0 - h.beta1);
    k.b2 = (float)h.beta2;
    k.omb2 = (float)(1.0 - h.beta2);
    k.eps = (float)h.eps;
    k.clip = T.norm[1];
    k.step_size = T.coef[2 * t];
    k.bc2_sqrt = T.coef[2 * t + 1];
    const uint64_t base = T.params[t];
    float *p = reinterpret_cast<float *>(base) + first;  // first is a multiple of kChunk: the alignment class of `base` holds
    const int64_t off = T.offset[t] + first;
    if ((base & 15) == 0 && (numel & 3) == 0)
        step_chunk<true>(p, T.grad + off, T.exp_avg + off, T.exp_avg_sq + off, n, k);
    else
        step_chunk<false>(p, T.grad + off, T.exp_avg + off, T.exp_avg_sq + off, n, k);
}

int make_table(const char *who, const fd_optim_table *tab, Table &T) {
    FD_REQUIRE(tab, "%s: null table", who);
    FD_REQUIRE(tab->params && tab->numel && tab->offset && tab->flags && tab->step && tab->coef && tab->chunks && tab->partials && tab->norm,
               "%s: null table member", who);
    FD_REQUIRE(tab->grad && tab->exp_avg && tab->exp_avg_sq, "%s: null flat buffer", who);
    FD_REQUIRE(tab->n_tensors > 0 && tab->n_chunks > 0 && tab->total > 0, "%s: n_tensors (%d), n_chunks (%d) and total (%lld) must be positive", who,
               tab->n_tensors, tab->n_chunks, (long long)tab->total);
    FD_REQUIRE(tab->n_chunks >= tab->n_tensors, "%s: %d chunks cannot cover %d tensors", who, tab->n_chunks, tab->n_tensors);
    FD_REQUIRE(tab->chunk == kChunk, "%s: chunk size %d, the kernels take %d (fd_optim_chunk())", who, tab->chunk, kChunk);
    FD_REQUIRE(((uintptr_t)tab->grad & 15) == 0 && ((uintptr_t)tab->exp_avg & 15) == 0 && ((uintptr_t)tab->exp_avg_sq & 15) == 0,
               "%s: the flat buffers must be 16-byte aligned", who);
    T.params = (const uint64_t *)tab->params;
    T.numel = (const int64_t *)tab->numel;
    T.offset = (const int64_t *)tab->offset;
    T.flags = (const int32_t *)tab->flags;
    T.step = (int32_t *)tab->step;
    T.coef = (float *)tab->coef;
    T.chunks = (const int32_t *)tab->chunks;
    T.partials = (double *)tab->partials;
    T.norm = (float *)tab->norm;
    T.grad = tab->grad;
    T.exp_avg = tab->exp_avg;
    T.exp_avg_sq = tab->exp_avg_sq;
    T.n_tensors = tab->n_tensors;
    T.n_chunks = tab->n_chunks;
    return FD_OK;
}

}  // namespace

extern "C" int fd_optim_chunk(void) { return kChunk; }

extern "C" int fd_optim_zero_grad(const fd_optim_table *table, fd_stream_t stream_) {
    Table T;
    if (int rc = make_table("fd_optim_zero_grad", table, T)) return rc;
    fd::fill_words(T.grad, 0u, (size_t)table->total, fd::as_stream(stream_));
    return fd::check_launch("fd_optim_zero_grad");
}

extern "C" int fd_optim_adam_step(const fd_optim_table *table, double lr, double beta1, double beta2, double eps, double wd, double max_norm,
                                  fd_stream_t stream_) {
    Table T;
    if (int rc = make_table("fd_optim_adam_step", table, T)) return rc;
    FD_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "fd_optim_adam_step: betas (%g, %g) must lie in [0, 1)", beta1, beta2);
    FD_REQUIRE(eps > 0.0, "fd_optim_adam_step: eps must be > 0");
    FD_REQUIRE(lr == lr && wd == wd && max_norm == max_norm, "fd_optim_adam_step: lr, wd or max_norm is NaN");
    HyperSource src{};
    src.h.lr = lr; src.h.beta1 = beta1; src.h.beta2 = beta2; src.h.eps = eps; src.h.wd = wd; src.h.max_norm = max_norm;
    hipStream_t st = fd::as_stream(stream_);
    const int clip = max_norm > 0.0 ? 1 : 0;
    const dim3 grid((unsigned)T.n_chunks), block(kThreads);
    if (clip) hipLaunchKernelGGL(optim_sumsq, grid, block, 0, st, T);
    hipLaunchKernelGGL(optim_prepare, dim3(1), block, 0, st, T, src, clip);
    hipLaunchKernelGGL(optim_step, grid, block, 0, st, T, src);
    return fd::check_launch("fd_optim_adam_step");
}

extern "C" int fd_optim_adam_step_dev(const fd_optim_table *table, const double *hyper, int clip, const int32_t *skip, fd_stream_t stream_) {
    Table T;
    if (int rc = make_table("fd_optim_adam_step_dev", table, T)) return rc;
    FD_REQUIRE(hyper, "fd_optim_adam_step_dev: null hyper record");
    FD_REQUIRE(((uintptr_t)hyper & 7) == 0, "fd_optim_adam_step_dev: the hyper record must be 8-byte aligned");
    FD_REQUIRE(clip == 0 || clip == 1, "fd_optim_adam_step_dev: clip must be 0 or 1 (got %d)", clip);
    HyperSource src{};
    src.dev = hyper;
    src.skip = skip;
    hipStream_t st = fd::as_stream(stream_);
    const dim3 grid((unsigned)T.n_chunks), block(kThreads);
    if (clip) hipLaunchKernelGGL(optim_sumsq, grid, block, 0, st, T);
    hipLaunchKernelGGL(optim_prepare, dim3(1), block, 0, st, T, src, clip);
    hipLaunchKernelGGL(optim_step, grid, block, 0, st, T, src);
    return fd::check_launch("fd_optim_adam_step_dev");
}
