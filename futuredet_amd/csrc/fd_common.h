// Shared helpers for the gfx950 kernels of libfuturedet_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/futuredet_hip.h"

namespace fd {

void set_error(const char *fmt, ...);

// ---- sparse convolution: one call record, one description of the packed-weight buffer ---------------------------
// fd_spconv_apply validates its arguments, fills this record once and offers it to the kernel families in turn.
struct SpconvCall {
    const void *in;
    int64_t n_in;         // rows of `in` (bound of the rulebook entries)
    const void *wpacked;  // start of the whole packed buffer: a family finds its section through spconv_weight_layout
    const float *bias;
    const void *residual;
    int relu;
    const int *nbr;
    int64_t nbr_stride;
    const int *ranges;  // null: equal-row ranges
    int n_ranges;
    int K, n_out;
    const int *n_out_dev;
    int64_t n_expected;  // only steers launch heuristics
    int cin, cout, dtype;
    void *out;
    hipStream_t stream;
    const int *plan;  // null, or the rulebook's chunk plan (fd_spconv_plan_build for the same n_out / ranges / n_ranges): fd_spconv_chunk.h
    int64_t plan_stride;
    int layout;  // which tensors are stored bank-spread (fd_spconv_apply_layout; skeleton::kLayoutIn / Residual / Out), 0 = none
};

constexpr int kSpconvMaxTaps = 27;  // 3 x 3 x 3: the largest kernel of every sparse-convolution entry point

// The byte sections of the packed-weight buffer (bytes 0 = absent); what they hold and in which order: fd_spconv_pack.h
struct WeightSection {
    size_t offset, bytes;
};
struct SpconvWeightLayout {
    WeightSection base, c32, pair, win;
    size_t total;
};
inline SpconvWeightLayout spconv_weight_layout(int K, int cin, int cout, int dtype) {
    const size_t elem = dtype == 0 ? 4 : 2, main_bytes = (size_t)K * cin * cout * elem;
    SpconvWeightLayout l{};
    size_t end = 0;
    auto section = [&](bool present, size_t bytes) {
        const WeightSection s{end, present ? bytes : 0};
        end += s.bytes;
        return s;
    };
    l.base = section(true, main_bytes);
    l.c32 = section(dtype == 0 && cin == 32 && cout == 32, main_bytes);
    l.pair = section(dtype == 1 && cin == 16, (size_t)((K + 1) / 2) * 32 * cout * elem);
    l.win = section(dtype == 1 && ((cin == 64 && cout == 64) || (cin == 128 && cout == 128)), main_bytes);
    l.total = end;
    return l;
}
inline SpconvWeightLayout spconv_weight_layout(const SpconvCall &c) { return spconv_weight_layout(c.K, c.cin, c.cout, c.dtype); }

// The kernel families of fd_spconv_apply, in the order it tries them: 1 = launched, 0 = not this family's shape.
int spconv_f32_res16_dispatch(const SpconvCall &c);    // fd_spconv_f32r.hip: fp32, 16 input channels (weights resident in LDS, register accumulators)
int spconv_f32_c32_dispatch(const SpconvCall &c);      // fd_spconv_c32.hip: fp32 32 -> 32 on the 32x32x2 MFMA
int spconv_f32_compact_dispatch(const SpconvCall &c);  // fd_spconv_v2.hip: fp32, pair compaction
int spconv_bf16_win_dispatch(const SpconvCall &c);     // fd_spconv_bf16win.hip: 64 -> 64, 128 -> 128 with an LDS window of input rows and 32-row MFMA tiles
int spconv_bf16_ws_dispatch(const SpconvCall &c);      // fd_spconv_bf16.hip: RESIDENT / RING kernels

// fd_conv2d_wino_pc.hip: 0 = launched, 1 = shape not supported by the variant, -1 = dynamic LDS refused; wide_items: work items of 128
// output channels (tile 8) instead of 64 (tile 7)
int wino_pc_launch(const float *x, const void *wp, const float *bias, float *y, int B, int H, int W, int cin, int cout, int relu, int cout_total,
                   int co_off, int wide_items, hipStream_t stream);

// Element counts that only the device knows (voxels of a sweep, rows of a sparse level): entry points take the host-side
// CAPACITY plus an optional device pointer to the actual count; kernels are launched for the capacity and work on
// min(capacity, *count).  This is what lets a whole sweep be issued (or captured into one hipGraph) without reading a
// count back to the host.
__device__ __forceinline__ int device_count(int capacity, const int *count_dev) {
    if (!count_dev) return capacity;
    const int n = *count_dev;
    return n < capacity ? (n > 0 ? n : 0) : capacity;
}

inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return FD_ELAUNCH;
    }
    return FD_OK;
}

#define FD_REQUIRE(cond, ...)           \
    do {                                \
        if (!(cond)) {                  \
            fd::set_error(__VA_ARGS__); \
            return FD_EINVAL;           \
        }                               \
    } while (0)

inline hipStream_t as_stream(fd_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Fills n_words 32-bit words (p 4-byte aligned) with a kernel (fd_error.hip).  Used instead of hipMemsetAsync wherever the
// call may be captured into a hipGraph: measured on ROCm 7.2 / MI355X, a captured graph whose memset nodes reset the
// voxelizer's hash table hangs on its second replay (the table is not reset, the probe loop never finds a free slot).
int fill_words(void *p, uint32_t value, size_t n_words, hipStream_t stream);
// the same for up to three regions in one launch (a null pointer = no region)
int fill_words3(void *p0, uint32_t v0, size_t n0, void *p1, uint32_t v1, size_t n1, void *p2, uint32_t v2, size_t n2, hipStream_t stream);

// ---- per-process state (fd_error.hip).  The library keeps NO per-call mutable state; what it caches is
//      keyed by device ordinal and published with atomics, so calls from several threads / for several
//      devices of one process are safe.
constexpr int kMaxDevices = 64;
int current_device();   // hipGetDevice (0 when the runtime cannot tell)
int device_cu_count();  // compute units of the current device, cached per device
// Kernels that need more than 64 KB of dynamic LDS must be told so once per (kernel, device).  `done` is the
// kernel instantiation's own bit mask of devices already configured.  Returns false when the runtime refuses.
bool ensure_dynamic_lds(const void *kernel, size_t bytes, std::atomic<uint64_t> &done);
// Tuning / test knobs (fd_tuning_set; initial values are read ONCE from the environment when the library is loaded: the
// variable of a knob is FD_ + its upper-case name).  0 = the built-in heuristic.  This list is the only one: the enum, the
// names fd_tuning_set accepts and the environment variables all come from it.
#define FD_TUNE_KNOBS(X)                                                                                                       \
    X(kTuneSpconvRG, "spconv_rg") X(kTuneSpconvV1, "spconv_v1") X(kTuneConvNT, "conv_nt") X(kTuneV2RangesPerCU, "v2_ranges_per_cu") \
    X(kTuneSpconvC32, "spconv_c32") X(kTuneBf16GP, "bf16_gp") X(kTuneBf16RG, "bf16_rg") X(kTuneBf16Depth, "bf16_depth")        \
    X(kTuneBf16NW, "bf16_nw") X(kTuneBf16Win, "bf16_win") X(kTuneF32ResRG, "f32_res_rg") X(kTuneConvStrip, "conv_strip")       \
    X(kTuneF32ResNW, "f32_res_nw") X(kTuneSpconvPlan, "spconv_plan") X(kTuneSpconvSwz, "spconv_swz")
#define FD_TUNE_ENUM(key, name) key,
enum TuneKey { FD_TUNE_KNOBS(FD_TUNE_ENUM) kTuneCount };
#undef FD_TUNE_ENUM
int tuning(TuneKey key);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- sparse index addressing (see include/futuredet_hip.h) ------------------------------------------
struct IndexGeom {
    int B, D, H, W, Ht, Wt;
    __host__ __device__ int64_t num_cols() const { return (int64_t)B * Ht * Wt * 64; }
};
__host__ __device__ inline IndexGeom make_geom(int B, int D, int H, int W) {
    IndexGeom g;
    g.B = B; g.D = D; g.H = H; g.W = W;
    g.Ht = (H + 7) >> 3; g.Wt = (W + 7) >> 3;
    return g;
}
__host__ __device__ inline int64_t col_of(const IndexGeom &g, int b, int y, int x) {
    return ((((int64_t)b * g.Ht + (y >> 3)) * g.Wt + (x >> 3)) << 6) + ((y & 7) << 3) + (x & 7);
}
__device__ inline void col_to_byx(const IndexGeom &g, int64_t col, int &b, int &y, int &x) {
    int in = (int)(col & 63);
    int64_t t = col >> 6;
    int tx = (int)(t % g.Wt);
    t /= g.Wt;
    int ty = (int)(t % g.Ht);
    b = (int)(t / g.Ht);
    y = ty * 8 + (in >> 3);
    x = tx * 8 + (in & 7);
}

// XCD-aware block remap (8 XCDs, round-robin dispatch): consecutive logical tiles land on one XCD so
// spatially adjacent tiles share an L2.  Bijective for any grid size.
__device__ inline unsigned xcd_swizzle(unsigned bid, unsigned nblocks) {
    const unsigned nx = 8;
    unsigned per = nblocks / nx, rem = nblocks % nx;
    unsigned xcd = bid % nx, loc = bid / nx;
    // XCD x owns per(+1 if x<rem) logical tiles
    unsigned start = xcd * per + (xcd < rem ? xcd : rem);
    return start + loc;
}

}  // namespace fd
