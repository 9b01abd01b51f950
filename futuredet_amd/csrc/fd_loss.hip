// CenterHead.loss on the device: FastFocalLoss + RegLoss (det3d/models/losses/centernet_loss.py) as center_head.py:396-539 combines
// them for the standard and dense heads, forward terms and the gradient of every head map, in a fixed number of launches whatever
// the number of tasks and timesteps.  include/futuredet_hip.h has the layouts and the arithmetic.
//
// Forward (2 launches for up to 8 tasks, 3 for 9-16: the descriptors of 8 tasks travel as one launch's arguments):
//   loss_partials  grid (chunks + B, tasks).  Chunk workgroups own at most kChunk elements of one heat map: 16-byte loads where the
//                  three pointers allow it, a scalar tail otherwise; each writes the clamped sigmoid and its negative sum as a
//                  double.  Object workgroups own one (task, sample): they compact the sample's valid entries in object order
//                  (ballots, like fd_targets.hip), then the positive sum, the mask counts of every step and, one thread per
//                  (term, channel), the L1 sums over the valid entries in object order.
//   loss_finish    one workgroup: per task the chunk partials in a fixed order, the samples in sample order, all in double; writes
//                  the terms vector in fp32 and the status word.
// Backward (2 launches, 3 for 9-16 tasks):
//   loss_grad_objects  one workgroup per (task, sample): the same compaction, then per valid entry the first-occurrence flags
//                  and duplicate links (a scan over the sample's entries in LDS).  The first entry of a (cell, class) carries the
//                  number of its duplicates for the heat map; the first entry of a cell carries, per box-map channel, the sum of
//                  sign(p - t) * coefficient over the terms in step order and the duplicates in object order.
//   loss_grad_maps     output-stationary, grid (chunks, tasks * 8 maps): a workgroup owns kChunk elements of one gradient map, places
//                  the records that fall into it in LDS (records have distinct cells: plain stores) and writes every element once,
//                  zeros included.  No atomics, no memset; the same bits on every run.
//
// Element arithmetic runs in double from the raw logit (sigma = 1 / (1 + exp(-x)); the clamp decision is taken on sigma rounded to
// fp32 against the fp32 bounds, which is what torch's fp32 clamp decides) and is rounded to fp32 once, at the store.
// Built with -ffp-contract=off.
#include <math.h>

#include "fd_common.h"
#include "fd_loss_guard.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = FD_LOSS_CHUNK;
constexpr int kMaxTasks = FD_LOSS_MAX_TASKS;
constexpr int kMaxSteps = FD_LOSS_MAX_STEPS;
constexpr int kMaxObjs = FD_LOSS_MAX_OBJS;
constexpr int kMaxD = 14;
constexpr int kMaps = 7;       // reg, height, dim, vel, rvel, rot, rrot
constexpr int kGroup = 8;      // tasks whose descriptors fit one object launch
constexpr int kPartStride = 112;  // doubles per (task, sample): pos, bad, count[7], l1[7][14]
constexpr int kPartCount = 2, kPartL1 = 2 + kMaxSteps;
static_assert(kPartL1 + kMaxSteps * kMaxD <= kPartStride, "object partials");
static_assert(kChunk % (kThreads * 4) == 0, "a chunk is a whole number of 16-byte accesses per thread");

struct Geom {
    int B, HW, M, n_tasks, dense, S, D, row, K;
    int nchunk_fwd, nchunk_bwd;
    int col[kMaxD];
    int ch[kMaps], choff[kMaps];
};

struct Weights {
    double cw[kMaxD], cwf[kMaxD], weight;
};

struct Work {  // the caller's workspace, cut up
    double *partials;  // [n_tasks][nchunk_fwd]
    double *objpart;   // [n_tasks][B][kPartStride]
    int *nvalid;       // [n_tasks][B]
    int4 *rec;         // [n_tasks][B][M]: cell, class * HW + cell, duplicates of (cell, class) or 0, first of its cell
    float *rec_val;    // [n_tasks][B][M][K]
};

struct FwdTask {
    const float *hm, *target;
    float *sig;
    const int64_t *ind, *cat;
    const uint8_t *mask[kMaxSteps];
    const float *maps[kMaps];
    const float *anno[kMaxSteps];
    int C;
};
struct FwdTasks { FwdTask t[kGroup]; };

struct ObjTask {
    const int64_t *ind, *cat;
    const uint8_t *mask;
    const float *maps[kMaps];
    const float *anno[kMaxSteps];
    int C;
};
struct ObjTasks { ObjTask t[kGroup]; };

struct MapTask {
    const float *hm, *target;
    float *d_hm;
    float *d_maps[kMaps];
    int C;
};
struct MapTasks { MapTask t[kMaxTasks]; };

struct FinishArgs { int nchunks[kMaxTasks]; };

// sum over the workgroup in a fixed order; the result is valid in thread 0.  Safe to call repeatedly.
__device__ double block_sum(double v, double *lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kWaves; ++w) s += lds[w];
    __syncthreads();
    return s;
}

struct Sig {
    double sd;  // sigma
    double s;   // clamped
    float sf;   // clamped, fp32: what the forward stores
    bool pass;  // clamp's backward: 1e-4 <= sigma <= 1 - 1e-4 in fp32
};

__device__ __forceinline__ Sig clamped_sigmoid(float x) {
    const float lo = 1e-4f, hi = (float)(1.0 - 1e-4);
    Sig r;
    r.sd = 1.0 / (1.0 + exp(-(double)x));
    const float f = (float)r.sd;
    r.pass = f >= lo && f <= hi;
    r.sf = f < lo ? lo : (f > hi ? hi : f);  // a NaN stays a NaN
    r.s = r.pass ? r.sd : (double)r.sf;
    return r;
}

// RegLoss divides by mask.float().sum() + 1e-4: an fp32 sum (exact) plus an fp32 constant, rounded to fp32 -- in the reference's
// double run too, because the mask is cast to float there.  Everything around it stays in double.
__device__ __forceinline__ double reg_denominator(float num_pos) { return (double)(num_pos + 1e-4f); }

__device__ __forceinline__ int wave_rank(unsigned long long bits) {
    const int lane = (int)__lane_id();
    return __popcll(bits & ((1ull << lane) - 1ull));
}

// (map, channel within the map) of predicted channel c of regression term i; the channel order is reg, height, dim, vel[, rvel],
// rot[, rrot] and term i of a standard head reads velocity channels 2i, 2i + 1
__device__ __forceinline__ void term_channel(const Geom &g, int i, int c, int &map, int &ch) {
    const int vstep = g.dense ? 0 : 2 * i;
    if (c < 2) { map = 0; ch = c; return; }
    if (c == 2) { map = 1; ch = 0; return; }
    if (c < 6) { map = 2; ch = c - 3; return; }
    if (g.D == 8) { map = 5; ch = c - 6; return; }
    if (c < 8) { map = 3; ch = vstep + c - 6; return; }
    if (g.D == 10) { map = 5; ch = c - 8; return; }
    if (c < 10) { map = 4; ch = vstep + c - 8; return; }
    if (c < 12) { map = 5; ch = c - 10; return; }
    map = 6; ch = c - 12;
}

struct ObjLds {
    int m[kMaxObjs], ind[kMaxObjs], cat[kMaxObjs];
    int wn[kWaves], wb[kWaves];
};

// The valid entries of one sample, in object order, into LDS.  Returns their number; n_mask counts mask != 0, n_bad the masked
// entries whose ind / cat are out of range.  An entry with mask == 0 is dropped before its ind / cat are looked at.
__device__ int compact_objects(ObjLds &L, const uint8_t *__restrict__ mask, const int64_t *__restrict__ ind, const int64_t *__restrict__ cat,
                               int M, int64_t hw, int C, int &n_mask, int &n_bad) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int n = 0;
    n_mask = 0;
    n_bad = 0;
    for (int base = 0; base < M; base += kThreads) {
        const int m = base + tid;
        int kind = kLossSkip;
        int64_t iv = 0, cv = 0;
        if (m < M) {
            const uint8_t mk = mask[m];
            if (mk) {
                iv = ind[m];
                cv = cat[m];
            }
            kind = fd_loss_entry_kind(mk, iv, cv, hw, C);
        }
        const unsigned long long take = __ballot(kind == kLossTake), bad = __ballot(kind == kLossBad);
        if (lane == 0) {
            L.wn[wave] = __popcll(take);
            L.wb[wave] = __popcll(bad);
        }
        __syncthreads();
        int at = n + wave_rank(take), tot = 0, totb = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) at += L.wn[w];
            tot += L.wn[w];
            totb += L.wb[w];
        }
        if (kind == kLossTake && at < kMaxObjs) {
            L.m[at] = m;
            L.ind[at] = (int)iv;
            L.cat[at] = (int)cv;
        }
        n += tot;
        n_bad += totb;
        n_mask += tot + totb;
        __syncthreads();
    }
    return n < kMaxObjs ? n : kMaxObjs;
}

// ------------------------------------------------------------------------------------------------------------------ forward
__device__ void forward_chunk(const Geom &g, const FwdTask &t, int task, int chunk, const Work &ws, double *red) {
    const int64_t n_all = (int64_t)g.B * t.C * g.HW;
    const int64_t first = (int64_t)chunk * kChunk;
    if (first >= n_all) return;  // uniform over the workgroup
    const int n = n_all - first < kChunk ? (int)(n_all - first) : kChunk;
    const float *__restrict__ x = t.hm + first;
    const float *__restrict__ tg = t.target + first;
    float *__restrict__ sg = t.sig + first;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)tg) | ((uintptr_t)sg)) & 15) == 0;  // first is a multiple of kChunk
    double acc = 0.0;
    for (int i = threadIdx.x * 4; i < n; i += kThreads * 4) {
        const int cnt = n - i < 4 ? n - i : 4;
        f32x4 X, T, S;
        if (vec && cnt == 4) {
            X = *reinterpret_cast<const f32x4 *>(x + i);
            T = *reinterpret_cast<const f32x4 *>(tg + i);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                X[j] = j < cnt ? x[i + j] : 0.f;
                T[j] = j < cnt ? tg[i + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Sig s = clamped_sigmoid(X[j]);
            const double u = 1.0 - (double)T[j], u2 = u * u;
            const double term = log(1.0 - s.s) * (s.s * s.s) * (u2 * u2);
            if (j < cnt) acc += term;
            S[j] = s.sf;
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<f32x4 *>(sg + i) = S;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) sg[i + j] = S[j];
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) ws.partials[(int64_t)task * g.nchunk_fwd + chunk] = s;
}

__device__ void forward_objects(const Geom &g, const FwdTask &t, int task, int b, const Work &ws, ObjLds &L, double *red) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)b * g.M;
    int n_mask, n_bad;
    const int n = compact_objects(L, t.mask[0] + row0, t.ind + row0, t.cat + row0, g.M, g.HW, t.C, n_mask, n_bad);
    double *out = ws.objpart + ((int64_t)task * g.B + b) * kPartStride;

    double acc = 0.0;
    for (int j = tid; j < n; j += kThreads) {
        const int64_t e = fd_loss_cell(b, g.B, L.cat[j], t.C, L.ind[j], g.HW);
        if (e >= 0) {
            const Sig s = clamped_sigmoid(t.hm[e]);
            const double om = 1.0 - s.s;
            acc += log(s.s) * (om * om);
        }
    }
    const double pos = block_sum(acc, red);
    if (tid == 0) {
        out[0] = pos;
        out[1] = (double)n_bad;
        out[kPartCount] = (double)n_mask;
    }
    for (int i = 1; i < g.S; ++i) {  // standard head: num_positive counts the masks of every step
        const uint8_t *__restrict__ mk = t.mask[i] + row0;
        double c = 0.0;
        for (int m = tid; m < g.M; m += kThreads) c += mk[m] ? 1.0 : 0.0;
        const double s = block_sum(c, red);
        if (tid == 0) out[kPartCount + i] = s;
    }
    if (tid < g.S * g.D) {
        const int i = tid / g.D, c = tid - i * g.D;
        int map, ch;
        term_channel(g, i, c, map, ch);
        const float *__restrict__ pm = t.maps[map];
        const float *__restrict__ an = t.anno[i];
        const int col = g.col[c];
        double l1 = 0.0;
        for (int j = 0; j < n; ++j) {
            const int64_t e = fd_loss_cell(b, g.B, ch, g.ch[map], L.ind[j], g.HW);
            if (e < 0) continue;
            const double p = (double)pm[e], tv = (double)an[(row0 + L.m[j]) * g.row + col];
            l1 += fabs(p - tv);
        }
        out[kPartL1 + tid] = l1;
    }
}

__global__ void __launch_bounds__(kThreads) loss_partials(Geom g, FwdTasks tasks, int task0, Work ws) {
    __shared__ ObjLds L;
    __shared__ double red[kWaves];
    const FwdTask &t = tasks.t[blockIdx.y];
    const int task = task0 + blockIdx.y;
    if ((int)blockIdx.x < g.nchunk_fwd)
        forward_chunk(g, t, task, blockIdx.x, ws, red);
    else
        forward_objects(g, t, task, blockIdx.x - g.nchunk_fwd, ws, L, red);
}

__global__ void __launch_bounds__(kThreads) loss_finish(Geom g, Weights wt, FinishArgs fa, Work ws, float *__restrict__ terms) {
    __shared__ double red[kWaves];
    __shared__ double sh[kPartStride];
    const int tid = threadIdx.x;
    const int stride = 4 + g.S + g.S * g.D;
    double bad = 0.0;
    for (int k = 0; k < g.n_tasks; ++k) {
        double acc = 0.0;
        for (int c = tid; c < fa.nchunks[k]; c += kThreads) acc += ws.partials[(int64_t)k * g.nchunk_fwd + c];
        const double neg = block_sum(acc, red);
        if (tid < kPartStride) {
            double v = 0.0;
            for (int b = 0; b < g.B; ++b) v += ws.objpart[((int64_t)k * g.B + b) * kPartStride + tid];
            sh[tid] = v;
        }
        __syncthreads();
        float *out = terms + (int64_t)k * stride;
        const double num_pos = sh[kPartCount], denom = reg_denominator((float)num_pos);
        if (tid < g.S * g.D) out[4 + g.S + tid] = (float)(sh[kPartL1 + tid] / denom);
        if (tid == 0) {
            const double hm_loss = num_pos == 0.0 ? -neg : -(sh[0] + neg) / num_pos;
            double loc_sum = 0.0, num_positive = 0.0;
            for (int i = 0; i < g.S; ++i) {
                const double *w = (i == 0) ? wt.cw : wt.cwf;
                double loc = 0.0;
                for (int c = 0; c < g.D; ++c) loc += sh[kPartL1 + i * g.D + c] / denom * w[c];
                out[4 + i] = (float)loc;
                loc_sum += loc;
                num_positive += sh[kPartCount + i];
            }
            out[0] = (float)(hm_loss + wt.weight * loc_sum);
            out[1] = (float)hm_loss;
            out[2] = (float)num_pos;
            out[3] = (float)num_positive;
            bad += sh[1];
        }
        __syncthreads();
    }
    if (tid == 0) terms[(int64_t)g.n_tasks * stride] = (float)bad;
}

// ----------------------------------------------------------------------------------------------------------------- backward
__global__ void __launch_bounds__(kThreads) loss_grad_objects(Geom g, Weights wt, ObjTasks tasks, int task0, Work ws,
                                                              const float *__restrict__ terms, const float *__restrict__ go) {
    __shared__ ObjLds L;
    __shared__ int nxt[kMaxObjs];
    __shared__ unsigned char first_cell[kMaxObjs];
    __shared__ double coef[kMaxSteps * kMaxD];
    const ObjTask &t = tasks.t[blockIdx.y];
    const int task = task0 + blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    const int64_t row0 = (int64_t)b * g.M;
    const int64_t list = (int64_t)task * g.B + b;
    const int stride = 4 + g.S + g.S * g.D;
    if (tid < g.S * g.D) {
        const int i = tid / g.D, c = tid - i * g.D;
        const double w = i == 0 ? wt.cw[c] : wt.cwf[c];
        coef[tid] = (double)go[task] * wt.weight * w / reg_denominator(terms[(int64_t)task * stride + 2]);
    }
    int n_mask, n_bad;
    const int n = compact_objects(L, t.mask + row0, t.ind + row0, t.cat + row0, g.M, g.HW, t.C, n_mask, n_bad);  // ends on a barrier
    int4 *rec = ws.rec + list * g.M;
    for (int j = tid; j < n; j += kThreads) {
        const int ij = L.ind[j], cj = L.cat[j];
        bool first_pair = true, first = true;
        int dup = 0, next = -1;
        for (int q = 0; q < n; ++q) {
            if (L.ind[q] != ij) continue;
            if (q < j) first = false;
            if (q > j && next < 0) next = q;
            if (L.cat[q] == cj) {
                if (q < j) first_pair = false;
                if (q >= j) ++dup;
            }
        }
        nxt[j] = next;
        first_cell[j] = first ? 1 : 0;
        rec[j] = make_int4(ij, cj * g.HW + ij, first_pair ? dup : 0, first ? 1 : 0);
    }
    if (tid == 0) ws.nvalid[list] = n;
    __syncthreads();
    float *val = ws.rec_val + list * g.M * g.K;
    for (int it = tid; it < n * g.K; it += kThreads) {
        const int j = it / g.K, q = it - j * g.K;
        if (!first_cell[j]) continue;
        int map = 0;
        while (map + 1 < kMaps && q >= g.choff[map] + g.ch[map]) ++map;
        const int ch = q - g.choff[map];
        int i0 = 0, i1 = g.S, c;
        const int rot0 = g.D == 8 ? 6 : (g.D == 10 ? 8 : 10);
        switch (map) {
            case 0: c = ch; break;
            case 1: c = 2; break;
            case 2: c = 3 + ch; break;
            case 3: c = 6 + (ch & 1); break;
            case 4: c = 8 + (ch & 1); break;
            case 5: c = rot0 + ch; break;
            default: c = 12 + ch; break;
        }
        if ((map == 3 || map == 4) && !g.dense) {
            i0 = ch >> 1;
            i1 = i0 + 1;
        }
        const int64_t e = fd_loss_cell(b, g.B, ch, g.ch[map], L.ind[j], g.HW);
        double acc = 0.0;
        if (e >= 0 && c < g.D) {
            const float p = t.maps[map][e];
            const int col = g.col[c];
            for (int i = i0; i < i1 && i < g.S; ++i) {
                const float *__restrict__ an = t.anno[i];
                const double k = coef[i * g.D + c];
                for (int jj = j; jj >= 0; jj = nxt[jj]) {
                    const float d = p - an[(row0 + L.m[jj]) * g.row + col];
                    acc += d > 0.f ? k : (d < 0.f ? -k : 0.0);
                }
            }
        }
        val[(int64_t)j * g.K + q] = (float)acc;
    }
}

__global__ void __launch_bounds__(kThreads) loss_grad_maps(Geom g, MapTasks tasks, Work ws, const float *__restrict__ terms,
                                                           const float *__restrict__ go) {
    __shared__ float buf[kChunk];
    const int task = blockIdx.y >> 3, mu = blockIdx.y & 7, tid = threadIdx.x;
    const MapTask &t = tasks.t[task];
    const int chn = mu == 0 ? t.C : g.ch[mu - 1];
    float *__restrict__ out = mu == 0 ? t.d_hm : t.d_maps[mu - 1];
    if (!out || chn <= 0) return;
    const int64_t per = (int64_t)chn * g.HW, n_all = per * g.B;
    const int64_t first = (int64_t)blockIdx.x * kChunk;
    if (first >= n_all) return;
    const int n = n_all - first < kChunk ? (int)(n_all - first) : kChunk;
    int *bufi = reinterpret_cast<int *>(buf);
    for (int i = tid; i < kChunk; i += kThreads) bufi[i] = 0;  // 0 and 0.0f share their bits
    __syncthreads();
    const int b0 = (int)(first / per), b1 = (int)((first + n - 1) / per);
    for (int b = b0; b <= b1 && b < g.B; ++b) {
        const int64_t list = (int64_t)task * g.B + b;
        int nv = ws.nvalid[list];
        nv = nv < g.M ? (nv > 0 ? nv : 0) : g.M;
        const int4 *__restrict__ rec = ws.rec + list * g.M;
        for (int j = tid; j < nv; j += kThreads) {
            const int4 r = rec[j];
            if (mu == 0) {
                const int64_t e = (int64_t)b * per + r.y - first;
                if (r.z > 0 && r.y >= 0 && r.y < per && e >= 0 && e < n) bufi[e] = r.z;
            } else if (r.w && r.x >= 0 && r.x < g.HW) {
                const float *__restrict__ v = ws.rec_val + (list * g.M + j) * g.K + g.choff[mu - 1];
                for (int ch = 0; ch < chn; ++ch) {
                    const int64_t e = ((int64_t)b * chn + ch) * g.HW + r.x - first;
                    if (e >= 0 && e < n) buf[e] = v[ch];
                }
            }
        }
    }
    __syncthreads();
    float *__restrict__ o = out + first;
    if (mu != 0) {
        const bool vec = (((uintptr_t)o) & 15) == 0;
        for (int i = tid * 4; i < n; i += kThreads * 4) {
            if (vec && n - i >= 4) {
                *reinterpret_cast<f32x4 *>(o + i) = *reinterpret_cast<const f32x4 *>(buf + i);
            } else {
                for (int j = 0; j < 4 && i + j < n; ++j) o[i + j] = buf[i + j];
            }
        }
        return;
    }
    const int stride = 4 + g.S + g.S * g.D;
    const double num_pos = (double)terms[(int64_t)task * stride + 2];
    const double scale = num_pos == 0.0 ? -(double)go[task] : -(double)go[task] / num_pos;
    const float *__restrict__ x = t.hm + first;
    const float *__restrict__ tg = t.target + first;
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)tg) | ((uintptr_t)o)) & 15) == 0;
    for (int i = tid * 4; i < n; i += kThreads * 4) {
        const int cnt = n - i < 4 ? n - i : 4;
        f32x4 X, T, G;
        if (vec && cnt == 4) {
            X = *reinterpret_cast<const f32x4 *>(x + i);
            T = *reinterpret_cast<const f32x4 *>(tg + i);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                X[j] = j < cnt ? x[i + j] : 0.f;
                T[j] = j < cnt ? tg[i + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Sig s = clamped_sigmoid(X[j]);
            const double u = 1.0 - (double)T[j], u2 = u * u, om = 1.0 - s.s;
            double d = (u2 * u2) * (2.0 * s.s * log(om) - s.s * s.s / om);
            const int dup = j < cnt ? bufi[i + j] : 0;
            if (dup > 0) d += (double)dup * (om * om / s.s - 2.0 * om * log(s.s));
            G[j] = s.pass ? (float)(scale * d * (s.sd * (1.0 - s.sd))) : 0.f;
        }
        if (vec && cnt == 4) {
            *reinterpret_cast<f32x4 *>(o + i) = G;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) o[i + j] = G[j];
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- host
int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

int channels_of(const fd_loss_cfg &c, int ch[kMaps]) {
    const int v = c.dense ? 2 : 2 * c.T;
    ch[0] = 2; ch[1] = 1; ch[2] = 3;
    ch[3] = c.D >= 10 ? v : 0;
    ch[4] = c.D == 14 ? v : 0;
    ch[5] = 2;
    ch[6] = c.D == 14 ? 2 : 0;
    int k = 0;
    for (int i = 0; i < kMaps; ++i) k += ch[i];
    return k;
}

bool sizes_ok(const fd_loss_cfg *c, int max_classes) {
    if (!c) return false;
    if (c->B <= 0 || c->H <= 0 || c->W <= 0 || c->M <= 0 || max_classes <= 0) return false;
    if (c->n_tasks < 1 || c->n_tasks > kMaxTasks) return false;
    if (!c->dense && (c->T < 1 || c->T > kMaxSteps)) return false;
    if (c->D != 8 && c->D != 10 && c->D != 14) return false;
    if (c->M > kMaxObjs) return false;
    const int64_t hw = (int64_t)c->H * c->W;
    const int64_t widest = max_classes > 2 * kMaxSteps ? max_classes : 2 * kMaxSteps;
    return hw * c->B * widest < ((int64_t)1 << 31);
}

struct Layout {
    size_t partials, objpart, nvalid, rec, rec_val, total;
};

Layout layout_of(const fd_loss_cfg &c, int max_classes) {
    int ch[kMaps];
    const int K = channels_of(c, ch);
    const size_t lists = (size_t)c.n_tasks * c.B;
    const size_t nchunk = (size_t)chunks_of((int64_t)c.B * max_classes * c.H * c.W);
    Layout l;
    size_t at = 0;
    l.partials = at; at += fd::align_up((size_t)c.n_tasks * nchunk * sizeof(double), 256);
    l.objpart = at;  at += fd::align_up(lists * kPartStride * sizeof(double), 256);
    l.nvalid = at;   at += fd::align_up(lists * sizeof(int), 256);
    l.rec = at;      at += fd::align_up(lists * c.M * sizeof(int4), 256);
    l.rec_val = at;  at += fd::align_up(lists * c.M * K * sizeof(float), 256);
    l.total = at;
    return l;
}

// everything both entry points check before any device work; fills the launch-argument structs
int prepare(const char *who, const fd_loss_cfg *cfg, const fd_loss_task *tasks, void *workspace, size_t workspace_bytes, Geom &g, Weights &wt,
            Work &ws, int &max_classes) {
    FD_REQUIRE(cfg, "%s: null cfg", who);
    FD_REQUIRE(tasks, "%s: null tasks", who);
    FD_REQUIRE(workspace, "%s: null workspace", who);
    const fd_loss_cfg &c = *cfg;
    FD_REQUIRE(c.B > 0 && c.H > 0 && c.W > 0 && c.M > 0, "%s: B (%d), H (%d), W (%d) and M (%d) must be positive", who, c.B, c.H, c.W, c.M);
    FD_REQUIRE(c.n_tasks >= 1 && c.n_tasks <= kMaxTasks, "%s: n_tasks (%d) must be in [1, %d]", who, c.n_tasks, kMaxTasks);
    FD_REQUIRE(c.dense || (c.T >= 1 && c.T <= kMaxSteps), "%s: T (%d) must be in [1, %d] for a standard head", who, c.T, kMaxSteps);
    FD_REQUIRE(c.D == 8 || c.D == 10 || c.D == 14, "%s: D (%d) must be 8, 10 or 14", who, c.D);
    FD_REQUIRE(c.M <= kMaxObjs, "%s: M (%d) above %d objects per sample", who, c.M, kMaxObjs);
    FD_REQUIRE(c.row_stride >= 1, "%s: row_stride (%d) must be positive", who, c.row_stride);
    for (int i = 0; i < c.D; ++i)
        FD_REQUIRE(c.col[i] >= 0 && c.col[i] < c.row_stride, "%s: column %d of the map (%d) outside a target row of %d", who, i, c.col[i], c.row_stride);
    max_classes = 0;
    for (int k = 0; k < c.n_tasks; ++k) {
        FD_REQUIRE(tasks[k].C > 0, "%s: C (%d) of task %d must be positive", who, tasks[k].C, k);
        max_classes = tasks[k].C > max_classes ? tasks[k].C : max_classes;
    }
    FD_REQUIRE(sizes_ok(cfg, max_classes), "%s: a map of B * channels * H * W elements must stay below 2^31", who);
    FD_REQUIRE(workspace_bytes >= layout_of(c, max_classes).total, "%s: workspace too small (%zu bytes, %zu needed)", who, workspace_bytes,
               layout_of(c, max_classes).total);
    FD_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    g.B = c.B; g.HW = c.H * c.W; g.M = c.M; g.n_tasks = c.n_tasks; g.dense = c.dense ? 1 : 0; g.S = c.dense ? 1 : c.T; g.D = c.D;
    g.row = c.row_stride;
    fd_loss_cfg cc = c;
    cc.dense = g.dense;
    g.K = channels_of(cc, g.ch);
    int off = 0;
    for (int i = 0; i < kMaps; ++i) {
        g.choff[i] = off;
        off += g.ch[i];
    }
    for (int i = 0; i < kMaxD; ++i) g.col[i] = i < c.D ? c.col[i] : 0;
    int widest = max_classes;
    for (int i = 0; i < kMaps; ++i) widest = g.ch[i] > widest ? g.ch[i] : widest;
    g.nchunk_fwd = (int)chunks_of((int64_t)c.B * max_classes * g.HW);
    g.nchunk_bwd = (int)chunks_of((int64_t)c.B * widest * g.HW);
    for (int i = 0; i < kMaxD; ++i) {
        wt.cw[i] = i < c.D ? c.code_weights[i] : 0.0;
        wt.cwf[i] = i < c.D ? c.code_weights_forecast[i] : 0.0;
    }
    wt.weight = c.weight;
    const Layout l = layout_of(cc, max_classes);
    char *base = (char *)workspace;
    ws.partials = (double *)(base + l.partials);
    ws.objpart = (double *)(base + l.objpart);
    ws.nvalid = (int *)(base + l.nvalid);
    ws.rec = (int4 *)(base + l.rec);
    ws.rec_val = (float *)(base + l.rec_val);
    for (int k = 0; k < c.n_tasks; ++k) {
        const fd_loss_task &t = tasks[k];
        FD_REQUIRE(t.hm && t.hm_target && t.ind && t.cat, "%s: task %d: null hm, hm_target, ind or cat", who, k);
        for (int i = 0; i < g.S; ++i) FD_REQUIRE(t.mask[i] && t.anno_box[i], "%s: task %d: null mask or anno_box of step %d", who, k, i);
        for (int i = 0; i < kMaps; ++i) FD_REQUIRE(g.ch[i] == 0 || t.maps[i], "%s: task %d: null map %d", who, k, i);
    }
    return FD_OK;
}

}  // namespace

extern "C" int fd_loss_chunk(void) { return kChunk; }

extern "C" size_t fd_centerhead_loss_terms(const fd_loss_cfg *cfg) {
    if (!sizes_ok(cfg, 1)) return 0;
    const size_t S = cfg->dense ? 1 : cfg->T;
    return (size_t)cfg->n_tasks * (4 + S + S * cfg->D) + 1;
}

extern "C" size_t fd_centerhead_loss_workspace_bytes(const fd_loss_cfg *cfg, int max_classes) {
    if (!sizes_ok(cfg, max_classes)) return 0;
    fd_loss_cfg c = *cfg;
    c.dense = c.dense ? 1 : 0;
    return layout_of(c, max_classes).total;
}

extern "C" int fd_centerhead_loss_forward(const fd_loss_cfg *cfg, const fd_loss_task *tasks, float *terms, void *workspace,
                                          size_t workspace_bytes, fd_stream_t stream_) {
    const char *who = "fd_centerhead_loss_forward";
    Geom g;
    Weights wt;
    Work ws;
    int max_classes;
    if (int rc = prepare(who, cfg, tasks, workspace, workspace_bytes, g, wt, ws, max_classes)) return rc;
    FD_REQUIRE(terms, "%s: null terms", who);
    for (int k = 0; k < g.n_tasks; ++k) FD_REQUIRE(tasks[k].sig, "%s: task %d: null sig", who, k);
    hipStream_t st = fd::as_stream(stream_);
    FinishArgs fa;
    for (int k = 0; k < kMaxTasks; ++k) fa.nchunks[k] = k < g.n_tasks ? (int)chunks_of((int64_t)g.B * tasks[k].C * g.HW) : 0;
    for (int k0 = 0; k0 < g.n_tasks; k0 += kGroup) {
        const int nk = g.n_tasks - k0 < kGroup ? g.n_tasks - k0 : kGroup;
        FwdTasks ft;
        for (int k = 0; k < kGroup; ++k) {
            const fd_loss_task &s = tasks[k0 + (k < nk ? k : 0)];
            FwdTask &d = ft.t[k];
            d.hm = s.hm; d.target = s.hm_target; d.sig = s.sig; d.ind = s.ind; d.cat = s.cat; d.C = s.C;
            for (int i = 0; i < kMaxSteps; ++i) {
                d.mask[i] = (const uint8_t *)s.mask[i];
                d.anno[i] = s.anno_box[i];
            }
            for (int i = 0; i < kMaps; ++i) d.maps[i] = s.maps[i];
        }
        hipLaunchKernelGGL(loss_partials, dim3((unsigned)(g.nchunk_fwd + g.B), (unsigned)nk), dim3(kThreads), 0, st, g, ft, k0, ws);
    }
    hipLaunchKernelGGL(loss_finish, dim3(1), dim3(kThreads), 0, st, g, wt, fa, ws, terms);
    return fd::check_launch(who);
}

extern "C" int fd_centerhead_loss_backward(const fd_loss_cfg *cfg, const fd_loss_task *tasks, const float *terms, const float *go,
                                           void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    const char *who = "fd_centerhead_loss_backward";
    Geom g;
    Weights wt;
    Work ws;
    int max_classes;
    if (int rc = prepare(who, cfg, tasks, workspace, workspace_bytes, g, wt, ws, max_classes)) return rc;
    FD_REQUIRE(terms && go, "%s: null terms or go", who);
    hipStream_t st = fd::as_stream(stream_);
    for (int k0 = 0; k0 < g.n_tasks; k0 += kGroup) {
        const int nk = g.n_tasks - k0 < kGroup ? g.n_tasks - k0 : kGroup;
        ObjTasks ot;
        for (int k = 0; k < kGroup; ++k) {
            const fd_loss_task &s = tasks[k0 + (k < nk ? k : 0)];
            ObjTask &d = ot.t[k];
            d.ind = s.ind; d.cat = s.cat; d.mask = (const uint8_t *)s.mask[0]; d.C = s.C;
            for (int i = 0; i < kMaxSteps; ++i) d.anno[i] = s.anno_box[i];
            for (int i = 0; i < kMaps; ++i) d.maps[i] = s.maps[i];
        }
        hipLaunchKernelGGL(loss_grad_objects, dim3((unsigned)g.B, (unsigned)nk), dim3(kThreads), 0, st, g, wt, ot, k0, ws, terms, go);
    }
    MapTasks mt;
    for (int k = 0; k < kMaxTasks; ++k) {
        const fd_loss_task &s = tasks[k < g.n_tasks ? k : 0];
        MapTask &d = mt.t[k];
        d.hm = s.hm; d.target = s.hm_target; d.d_hm = s.d_hm; d.C = s.C;
        for (int i = 0; i < kMaps; ++i) d.d_maps[i] = s.d_maps[i];
    }
    hipLaunchKernelGGL(loss_grad_maps, dim3((unsigned)g.nchunk_bwd, (unsigned)(g.n_tasks * 8)), dim3(kThreads), 0, st, g, mt, ws, terms, go);
    return fd::check_launch(who);
}
