/*
 * futuredet_hip.h -- C ABI of libfuturedet_hip.so, the MI355X (gfx950) implementation of the
 * FutureDet LiDAR inference hot path.  Plain pointers and sizes only (no torch types); every buffer is
 * caller-owned DEVICE memory unless marked host; every call is asynchronous on `stream` (a hipStream_t
 * passed as void*), performs no allocation and no device synchronisation, and returns 0 on success or a
 * negative FD_E* code (never exit()).  fd_last_error() returns a thread-local description of the last
 * failure.  Calls are re-entrant across threads, streams and devices: a call works on the device that is
 * current on the calling thread (the one `stream` belongs to); the only process-level state is a per-device
 * cache of device attributes / kernel LDS limits (atomics) and the fd_tuning_set knobs.  Sizes that the GPU decides (voxel count, active rows per level, detections) are written to
 * device int32 counters supplied by the caller; host code reads them when it needs them.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference tree).
 */
#ifndef FUTUREDET_HIP_H
#define FUTUREDET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_EINVAL (-1)    /* bad argument (null pointer, unsupported channel count, ...) */
#define FD_EWORKSPACE (-2) /* workspace too small */
#define FD_ELAUNCH (-3)   /* hipLaunch / runtime error (text in fd_last_error) */

typedef void *fd_stream_t; /* hipStream_t */

int fd_abi_version(void); /* 8 (round 6.  7: + fd_forecast_from_detections / fd_forecast_buffers; fd_sweep_assemble takes n_rows as an upper
                             * bound -- rows past the last descriptor's row_end are dropped.  8: struct fd_decode_cfg grew by nms_kind /
                             * n_radius / circle_radius (circular NMS) -- callers must zero-initialise the struct) */
const char *fd_last_error(void);
/* Tuning / test knobs (no reference counterpart): the reference paths the tests compare bit for bit and against the oracle.
 * 0 = built-in heuristic; any other name is FD_EINVAL.  Names: "spconv_rg" (rows per wave of the register sparse-conv
 * kernel: 1|2|4), "spconv_v1" (1: fp32 on the register kernel instead of the compacting one), "spconv_c32" (-1: fp32 32 -> 32 on
 * the 16-pair compacting kernel instead of the 32-pair one), "v2_ranges_per_cu" (row ranges per compute unit of the compacting
 * kernels), "f32_res_rg" (-1: 16-channel fp32 layers on the pair-compacting kernel instead of the resident-weights one; 2: two row
 * groups per wave; 32: 16 -> 32 on it as well), "f32_res_nw" (1: that kernel on XCD-contiguous tile chunks instead of interleaved
 * tiles), "spconv_plan" (-1: fd_spconv_apply_plan ignores the chunk plan), "spconv_swz" (-1: fd_spconv_layout_wanted answers 0, no bank-spread rows),
 * "bf16_gp" (-1: bf16 on the register kernel), "bf16_rg" / "bf16_depth" (row groups per wave / gather-ring depth of the bf16
 * kernels), "bf16_win" (-1: the 64 -> 64 / 128 -> 128 bf16 layers on the RING / RESIDENT kernels instead of the LDS-window
 * kernel), "bf16_nw" (1: RESIDENT bf16 kernels walk XCD-contiguous tile chunks instead of tiles interleaved over the grid),
 * "conv_nt" (output channels per workgroup of the bf16 dense conv: 64 | 32), "conv_strip" (1: stride-1 bf16 dense layers on strips
 * of 128 consecutive pixels instead of 8 x 16 tiles: faster alone, slower with several sweeps in flight; -1: the ragged grid of 8 x 16
 * tiles instead of the default mixed tiling -- whole 8 x 16 tiles plus edge tiles of other shapes; results identical in all three).
 * Initial values come from the environment variable FD_ + the upper-case name (FD_SPCONV_RG, ...), read once when the library is
 * loaded; nothing on the launch path calls getenv(). */
int fd_tuning_set(const char *name, int value);

/* ---------------------------------------------------------------------------------------------------
 * Device-side counts.  The number of voxels of a sweep and the number of active rows of every sparse level exist only
 * on the device.  Every entry point on the sweep path therefore takes a host-side CAPACITY (n_points, n_max, n_out,
 * nbr_stride ...) and, optionally, a device pointer to the actual count (n_points_dev, n_dev, n_out_dev): kernels are
 * launched for the capacity (or a bounded grid) and work on min(capacity, *count).  With the counts left on the device a
 * whole sweep -- voxelizer to NMS -- is issued without a host read-back and can be captured into one hipGraph
 * (futuredet_amd.detectors.VoxelNet.forward_points_static).  Passing NULL keeps the plain host-count behaviour.
 * ------------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------------
 * Voxelizer (+ fused mean reader).
 * Replaces points_to_voxel(points, voxel_size, coors_range, max_points, reverse_index=True, max_voxels)
 *   det3d/ops/point_cloud/point_cloud_ops.py:112-184 (kernel :7-55), called from
 *   det3d/core/input/voxel_generator.py:19-30 <- det3d/datasets/pipelines/preprocess.py:244-271,
 * and, when out_mean != NULL, VoxelFeatureExtractorV3.forward (det3d/models/readers/voxel_encoder.py:17-24)
 * and the batch-index prefix of collate_kitti_multi (det3d/torchie/parallel/collate.py:199-206).
 * Semantics are the reference's sequential ones, computed deterministically in parallel: voxels are numbered
 * in first-occurrence order of the input points, the first max_voxels voxels survive, each keeps its first
 * max_points points in input order; c = floor((p - lo) / vs) in float32 with a true division.
 *   points      [n, ndim] float32 rows (x,y,z,...)          ndim <= 8
 *   n_points_dev  NULL, or device int32[1]: the cloud has min(n_points, *n_points_dev) rows and n_points is the capacity of
 *                 a padded buffer (futuredet_amd.loading.assemble_device) -- see "Device-side counts" below
 *   out_voxels  [max_voxels, max_points, ndim] or NULL      (zero padded, as the reference returns)
 *   out_mean    [max_voxels, mean_stride] or NULL           (sum of kept points / count; cols >= ndim zeroed)
 *   out_coors   [max_voxels, coor_cols]; coor_cols 3 -> (z,y,x); 4 -> (batch_idx,z,y,x)
 *   out_num_points [max_voxels] int32, out_num_voxels device int32[1]
 * ------------------------------------------------------------------------------------------------- */
size_t fd_voxelize_workspace_bytes(int64_t n_points, int64_t max_voxels);
int fd_voxelize(const float *points, int64_t n_points, const int32_t *n_points_dev, int ndim, const float *range6_host,
                const float *voxel_size3_host, int max_points, int64_t max_voxels, int batch_idx,
                float *out_voxels, float *out_mean, int mean_stride, int32_t *out_coors, int coor_cols,
                int32_t *out_num_points, int32_t *out_num_voxels, void *workspace, size_t workspace_bytes,
                fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Sparse index + rulebook.  Replaces spconv 1.0's get_indice_pairs (invoked implicitly by every
 * SubMConv3d / SparseConv3d with a new indice_key: det3d/models/backbones/scn.py:99,110,115,120,125,130,
 * 135,141) and SparseConvTensor's coordinate bookkeeping (scn.py:154).
 *
 * Native layout (not spconv's pair lists): an active set on a grid (B, D<=64, H, W) is one 64-bit
 * occupancy word per (b,y,x) column (bit z) plus an exclusive prefix count per column; columns are
 * linearised in 8x8 tiles, so row numbers are spatially sorted:
 *     col(b,y,x) = ((b*ceil(H/8) + y/8)*ceil(W/8) + x/8)*64 + (y%8)*8 + x%8
 *     row(b,z,y,x) = prefix[col] + popcount(words[col] & ((1<<z)-1))
 * The rulebook is OUTPUT-stationary: nbr[k][o] = input row feeding output row o through kernel tap k
 * (k row-major over (kz,ky,kx), cross-correlation: input = o*stride - pad + k) or -1.
 * ------------------------------------------------------------------------------------------------- */
int64_t fd_index_num_cols(int B, int H, int W);                 /* length of words[] / prefix[] */
size_t fd_index_workspace_bytes(int64_t num_cols);
/* words must be zeroed by the caller (hipMemsetAsync) before fd_index_mark. */
int fd_index_mark(const int32_t *coords /*[n,4] (b,z,y,x)*/, const int32_t *n_dev /*device count, or NULL*/,
                  int64_t n_max, int B, int D, int H, int W, uint64_t *words, fd_stream_t stream);
/* marks the output set of a strided conv: o = (p + pad - k)/stride where integral and inside out grid; every word of out_words is
 * OVERWRITTEN (gather form, no atomics: nothing is OR-ed into what out_words held before) */
int fd_index_downsample(const uint64_t *in_words, int B, int D, int H, int W, const int *ksize3,
                        const int *stride3, const int *pad3, uint64_t *out_words, fd_stream_t stream);
/* exclusive scan of popcounts -> prefix[], total -> n_active_dev[0] */
int fd_index_scan(const uint64_t *words, int64_t num_cols, int32_t *prefix, int32_t *n_active_dev,
                  void *workspace, size_t workspace_bytes, fd_stream_t stream);
/* coords[row] = (b,z,y,x) for every active row */
int fd_index_coords(const uint64_t *words, const int32_t *prefix, int B, int D, int H, int W,
                    int32_t *coords /*[n_active,4]*/, fd_stream_t stream);
/* row_of[j] = row of coords_in[j] in the index (or -1) */
int fd_index_lookup(const uint64_t *words, const int32_t *prefix, int B, int D, int H, int W,
                    const int32_t *coords_in, const int32_t *n_dev, int64_t n_max, int32_t *row_of,
                    fd_stream_t stream);
/* dst[row_of[j], 0:c_dst] = src[j, 0:c_src] (zero padded to c_dst); rows with row_of<0 skipped */
int fd_rows_permute(const float *src, int c_src, const int32_t *row_of, const int32_t *n_dev, int64_t n_max,
                    void *dst, int c_dst, int dst_bf16, fd_stream_t stream);
/* nbr [K, nbr_stride] int32; out_coords holds out_rows (<= nbr_stride) rows, the kernel works on min(out_rows, *n_out_dev).
 * fill_tail != 0: rows o >= that count are filled with -1 up to nbr_stride;
 * fill_tail == 0: rows >= the count are left untouched (capacity-sized tables whose consumers are given the same device count) */
int fd_rulebook(const uint64_t *in_words, const int32_t *in_prefix, int B, int Din, int Hin, int Win,
                const int32_t *out_coords, int64_t out_rows, const int32_t *n_out_dev, int64_t nbr_stride, int fill_tail, const int *ksize3,
                const int *stride3, const int *pad3, int32_t *nbr, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Sparse convolution apply (gather - GEMM - no scatter).  Replaces spconv 1.0 indice_conv /
 * indice_subm_conv as used by the 21 convolutions of SpMiddleResNetFHD (scn.py:99-141) together with the
 * eval-mode BatchNorm1d / ReLU / residual add that follow them (scn.py:67-78,100-101,...): BN is folded
 * into weight/bias by the caller.
 *   out[o,:] = act( sum_k in[nbr[k][o],:] @ W[k] + bias (+ residual[o,:]) )
 *   in_feats  [n_in, cin]  float32 (dtype 0) or bfloat16 (dtype 1);  cin, cout in {16,32,64,128}
 *   wpacked   weights in MFMA fragment order, produced by fd_spconv_pack_weight from [K,cin,cout] float32
 *   bias      [cout] float32 or NULL; residual [n_out,cout] same dtype as out or NULL; relu 0/1
 * ------------------------------------------------------------------------------------------------- */
size_t fd_spconv_packed_weight_bytes(int K, int cin, int cout, int dtype);
int fd_spconv_pack_weight(const float *w_kio_host, int K, int cin, int cout, int dtype, void *wpacked_host);
int fd_spconv_apply(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual,
                    int relu, const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges /* [n_ranges+1] or NULL */,
                    int n_ranges, int K, int64_t n_out, const int32_t *n_out_dev /* NULL, or the device's row count */,
                    int64_t n_expected /* 0, or a typical row count that steers the launch heuristics when n_out is a capacity */,
                    int cin, int cout, int dtype, void *out_feats, fd_stream_t stream);
/* Work distribution of fd_spconv_apply (fp32; no reference counterpart -- spconv launches one GEMM per tap).  Workgroup b
 * computes output rows ranges[b] .. ranges[b+1]-1 (consecutive rows = neighbouring voxels), in chunks of <= 128 rows.
 *   ranges == NULL, n_ranges == 0 : one 128-row tile per workgroup
 *   ranges == NULL, n_ranges  > 0 : n_ranges equal row counts
 *   ranges != NULL                : device table from fd_spconv_ranges: equal WORK (16-pair MFMA groups, counted per
 *                                   8-row block of the rulebook) per range; boundaries are multiples of 8 rows.
 * fd_spconv_num_ranges returns the count the kernel prefers for a layer shape on the current device (a whole number of
 * ranges per compute unit).  The table depends only on the rulebook, so the 4-5 convolutions that share an indice_key
 * share it.  Results never depend on the distribution (fixed summation order per output row). */
int fd_spconv_num_ranges(int64_t n_out, int cin, int cout, int dtype);
int fd_spconv_wants_balanced_ranges(int cin, int cout, int dtype); /* 1: use fd_spconv_ranges; 0: equal rows (ranges = NULL) */
size_t fd_spconv_ranges_workspace_bytes(int64_t n_out);
int fd_spconv_ranges(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, int n_ranges,
                     int32_t *ranges /*[n_ranges+1]*/, void *workspace, size_t workspace_bytes, fd_stream_t stream);
/* Chunk plan of a SubM rulebook (K = 27; fp32; no reference counterpart).  The fp32 kernels compact every 128-row chunk of the
 * rulebook into per-tap pair lists before they compute; the lists depend only on the rulebook and on the row ranges, so the 4-5
 * convolutions that share an indice_key can share them.  fd_spconv_plan_build writes them once, in one launch, with no host read
 * (graph-capturable): plan is int32 [28, plan_stride], plan_stride >= fd_spconv_plan_stride(n_out), fd_spconv_plan_bytes(n_out) bytes
 * at that stride; n_out may be a capacity (n_out_dev as in fd_spconv_apply: rows past the device's count get no entry and are never
 * read).  fd_spconv_apply_plan is fd_spconv_apply with that plan: it must be given the n_out, n_out_dev, ranges and n_ranges the plan
 * was built with (range boundaries multiples of 8 rows, as fd_spconv_ranges makes them).  Layer shapes for which
 * fd_spconv_plan_wanted is 0 (and plan == NULL) run exactly fd_spconv_apply; results are bit-identical either way. */
int64_t fd_spconv_plan_stride(int64_t n_out);
size_t fd_spconv_plan_bytes(int64_t n_out);
int fd_spconv_plan_wanted(int cin, int cout, int dtype);
int fd_spconv_plan_build(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, const int32_t *ranges,
                         int n_ranges, int32_t *plan, int64_t plan_stride, fd_stream_t stream);
int fd_spconv_apply_plan(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu,
                         const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out,
                         const int32_t *n_out_dev, int64_t n_expected, int cin, int cout, int dtype, void *out_feats, const int32_t *plan,
                         int64_t plan_stride, fd_stream_t stream);
/* The chunk plan straight from the sparse index, without the rulebook table in between (fp32; 3 x 3 x 3 windows only: SubM, and
 * the strided convolutions into the next level).  fd_spconv_plan_from_index writes, in ONE launch, the plans of up to 8 sources:
 * source i is the table fd_rulebook would make from (in_words, in_prefix, Din/Hin/Win, out_coords, n_out_dev, {3,3,3}, stride, pad),
 * cut for the row split (ranges, n_ranges) as fd_spconv_plan_build cuts it -- the same int32 [28, plan_stride] words for every
 * column below the row count.  out_coords holds n_out rows.  fd_spconv_ranges_from_index is fd_spconv_ranges for a SubM level
 * (stride 1, pad 1; words / coords of the level itself): the same table bit for bit, same workspace size.
 * fd_spconv_index_plan_wanted: 1 for the layer shapes whose kernels read nothing but such a plan -- fd_spconv_apply_plan then takes
 * nbr == NULL (nbr_stride is ignored).  For every other shape, or without a plan, nbr == NULL is FD_EINVAL. */
typedef struct fd_plan_source {
    const uint64_t *in_words; /* index of the INPUT level */
    const int32_t *in_prefix;
    const int32_t *out_coords; /* [n_out, 4] (b, z, y, x): rows of the output level */
    const int32_t *n_out_dev;  /* NULL, or the device's row count (n_out is then a capacity) */
    const int32_t *ranges;     /* the row split of the convolution launch, as for fd_spconv_plan_build */
    int32_t *plan;             /* [28, plan_stride] */
    int64_t n_out, plan_stride;
    int32_t Din, Hin, Win, n_ranges;
    int32_t stride[3], pad[3];
} fd_plan_source;
int fd_spconv_index_plan_wanted(int cin, int cout, int dtype);
/* Bank-spread rows between two of our own kernels.  fd_spconv_apply_layout is fd_spconv_apply_plan plus a layout word that says which
 * of the launch's tensors are stored with 16-byte piece s of row r at piece s ^ (r & 7) of its 128-byte line (pieces keep their line
 * in 256- and 512-byte rows; 64-byte rows are never spread): bit 0 the input rows, bit 1 the residual, bit 2 the output.  The values
 * are those of the plain launch bit for bit; a gather of 16 different rows at one channel offset then spreads over the 8 positions
 * of a line instead of queueing on one.  For tensors nothing else reads: a level's inner tensors.  layout == 0 is
 * fd_spconv_apply_plan.  fp32 only: all bits for 32 -> 32, 64 -> 64 and 128 -> 128, bits 1 and 2 for every shape of 32 output channels
 * and up on the pair-compacting kernels; any other launch is FD_EINVAL and launches nothing.  fd_spconv_layout_wanted: the bits a layer
 * of this shape should get inside such a level (SubM layers 7, the strided layer into the level 4, else 0), 0 under
 * fd_tuning_set("spconv_swz", -1); a positive "spconv_swz" is a mask of levels for A/B runs (1: 32 channels, 2: 64, 4: 128). */
int fd_spconv_layout_wanted(int cin, int cout, int dtype);
int fd_spconv_apply_layout(const void *in_feats, int64_t n_in, const void *wpacked, const float *bias, const void *residual, int relu,
                           const int32_t *nbr, int64_t nbr_stride, const int32_t *ranges, int n_ranges, int K, int64_t n_out,
                           const int32_t *n_out_dev, int64_t n_expected, int cin, int cout, int dtype, void *out_feats,
                           const int32_t *plan, int64_t plan_stride, int layout, fd_stream_t stream);
int fd_spconv_plan_from_index(int B, int n_sources, const fd_plan_source *sources_host, fd_stream_t stream);
int fd_spconv_ranges_from_index(const uint64_t *words, int B, int D, int H, int W, const int32_t *coords, int64_t n_out,
                                const int32_t *n_out_dev, int n_ranges, int32_t *ranges /*[n_ranges+1]*/, void *workspace,
                                size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Densify.  Replaces SparseConvTensor.dense() + view (scn.py:165-168): out[b, c*D + d, y, x] = feats[row, c].
 * Every output element is written exactly once (zeros where inactive); element strides let the caller
 * choose NCHW or channels-last memory.  out_dtype 0 float32, 1 bfloat16.
 * ------------------------------------------------------------------------------------------------- */
int fd_densify(const void *feats, int c, int dtype, const uint64_t *words, const int32_t *prefix, int B, int D,
               int H, int W, void *out, int out_dtype, int64_t stride_b, int64_t stride_c, int64_t stride_y,
               int64_t stride_x, int64_t n_rows /* rows of feats: an index row >= n_rows (a capacity-sized level that overflowed) reads as zero */,
               fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Dense 2-D convolution, bf16 NHWC, fp32 accumulate, fused bias + ReLU (hand-written MFMA implicit GEMM).
 * Replaces the cuDNN convolutions of the RPN neck and CenterHead in the bf16 configuration
 * (det3d/models/necks/rpn.py:81-140, det3d/models/bbox_heads/center_head.py:104-143,344-349) with eval-mode
 * BatchNorm folded into weight/bias by the caller.
 *   x [B,H,W,cin] bf16; wpacked from fd_conv2d_pack_weight([cout][cin][ks][ks] float32 host); bias [cout] f32 or NULL
 *   supported: 3x3 stride 1|2 pad 1, 1x1 stride 1 pad 0; cin % 32 == 0
 *   y element (b, oy*osy+ooy, ox*osx+oox, co_off+co) of a [B, Ho*osy, Wo*osx, cout_total] bf16 tensor -- channel
 *   offsets express a concat, pixel strides/offsets express a 2x2 stride-2 transposed conv as four 1x1 convs.
 * ------------------------------------------------------------------------------------------------- */
size_t fd_conv2d_packed_weight_bytes(int cout, int cin, int ks);
int fd_conv2d_pack_weight(const float *w_oihw_host, int cout, int cin, int ks, void *wpacked_host);
int fd_conv2d_nhwc_bf16(const void *x, int B, int H, int W, int cin, const void *wpacked, const float *bias, int cout,
                        int ks, int stride, int pad, int relu, void *y, int cout_total, int co_off, int osy, int osx,
                        int ooy, int oox, fd_stream_t stream);
/* The same convolution in fp32 (fp32 activations / weights / output, v_mfma_f32_16x16x4_f32): the RPN / CenterHead layers of
 * the fp32 configurations, where the reference runs cuDNN (det3d/models/necks/rpn.py:124-159,
 * det3d/models/bbox_heads/center_head.py:129-143,344-349).  cin must be a multiple of 16; same placement arguments. */
size_t fd_conv2d_f32_packed_weight_bytes(int cout, int cin, int ks);
int fd_conv2d_f32_pack_weight(const float *w_oihw_host, int cout, int cin, int ks, void *wpacked_host);
int fd_conv2d_f32_num_tiles(void); /* number of workgroup tile shapes instantiated (valid `tile` values are 1..n) */
int fd_conv2d_nhwc_f32(const float *x, int B, int H, int W, int cin, const void *wpacked, const float *bias, int cout, int ks,
                       int stride, int pad, int relu, float *y, int cout_total, int co_off, int osy, int osx, int ooy, int oox,
                       int tile /* 0 = library heuristic, else 1..fd_conv2d_f32_num_tiles() */, fd_stream_t stream);
/* ConvTranspose2d(k, stride k) -- the RPN's upsampling deblock (det3d/models/necks/rpn.py:98-110) -- as ONE 1x1 convolution to
 * k*k*cout_sub virtual channels with a pixel-shuffle epilogue.  Weights: fd_conv2d_f32_pack_weight of [(dy,dx,co), cin, 1, 1];
 * bias [cout_sub]; y [B, H*k, W*k, cout_total]. */
int fd_conv2d_shuffle_nhwc_f32(const float *x, int B, int H, int W, int cin, const void *wpacked, const float *bias, int cout_sub, int k,
                               int relu, float *y, int cout_total, int co_off, int tile, fd_stream_t stream);
/* Grouped 3x3 stride-1 pad-1 convolution, <= 16 outputs per group: the final convolutions of the six CenterHead branches
 * (det3d/models/bbox_heads/center_head.py:129-143) in one launch.  x [B,H,W,groups*cin_g]; weights: fd_conv2d_f32_pack_weight of
 * [groups*16, cin_g, 3, 3] (each group padded to 16 outputs); bias [groups*16]; counts_host[g] = real outputs of group g,
 * written back to back from channel co_off of y. */
int fd_conv2d_grouped_nhwc_f32(const float *x, int B, int H, int W, int groups, int cin_g, const void *wpacked, const float *bias,
                               const int *counts_host, int relu, float *y, int cout_total, int co_off, int tile, fd_stream_t stream);
/* 3x3 stride-1 pad-1 only: Winograd F(2x2,3x3) with the 16 element-wise products as MFMA GEMMs over the input channels
 * (2.25x fewer multiplies than the direct form).  Weights are transformed (U = G g G^T) and packed by
 * fd_conv2d_wino_f32_pack_weight; cin must be a multiple of 16; output placement: channel offset only.  Every tile gives the
 * same bits.  Tile 7 (strips of 32 Winograd tiles x 64 channels, producer + consumer waves) needs W >= 63 and tensors below
 * 2 GB and fails with FD_EINVAL otherwise; tile 8 (the same strips x 128 channels) runs tile 6's kernel on those shapes. */
int fd_conv2d_wino_f32_num_tiles(void);
size_t fd_conv2d_wino_f32_packed_weight_bytes(int cout, int cin);
int fd_conv2d_wino_f32_pack_weight(const float *w_oihw_host, int cout, int cin, void *wpacked_host);
int fd_conv2d_wino_nhwc_f32(const float *x, int B, int H, int W, int cin, const void *wpacked, const float *bias, int cout, int relu,
                            float *y, int cout_total, int co_off, int tile /* 0 = default, else 1..num_tiles */, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * CenterPoint decode + rotated NMS.  Replaces CenterHead.predict's per-step decode
 * (det3d/models/bbox_heads/center_head.py:609-673), post_processing (:699-747), rotate_nms_pcdet
 * (det3d/core/bbox/box_torch_ops.py:248-277) and iou3d_nms_cuda.nms_gpu (det3d/ops/iou3d_nms/src/
 * iou3d_nms.cpp:90-135, iou3d_nms_kernel.cu:104-311) -- including the greedy sweep, which runs on the device.
 * One "group" = one (sample, heat-map) pair; G groups are decoded in one call.
 *   hm     [G, HW] float32 logits (single class)           reg [G,2,HW] height [G,1,HW] dim [G,3,HW] rot [G,2,HW]
 *   (channel-planar NCHW slices; *_gstride = element stride between groups)
 *   out_boxes7 [G, post_max, 7]  (x,y,z,w,l,h,yaw as predict emits them, vel excluded)
 *   out_scores [G, post_max], out_cell [G, post_max] int32 (BEV cell index, for gathering vel), out_count [G]
 * ------------------------------------------------------------------------------------------------- */
typedef struct fd_decode_cfg {
    int H, W;
    float out_size_factor, voxel_x, voxel_y, pc_x, pc_y; /* test_cfg.out_size_factor / voxel_size / pc_range */
    float score_threshold;
    float center_range[6];                               /* post_center_limit_range */
    float nms_iou_threshold;
    int nms_pre_max, nms_post_max;
    int hm_channels; /* 0 / 1: one heat-map channel; n > 1: score = max over n channels (center_head.py:589-595, the `classify` head) */
    /* test_cfg.circular_nms (center_head.py:722-725 -> _circle_nms :750-758 -> core/utils/circle_nms_jit.py): nms_kind 1 replaces the
     * rotated-IoU predicate by "squared centre distance <= min_radius" (the reference compares min_radius with the SQUARED distance, in
     * float32); decode group g takes circle_radius[g / (G / n_radius)] (test_cfg.min_radius[task_id]: one entry per group, n_radius must
     * divide G).  The reference applies no pre-NMS cut in this mode; here the nms_pre_max (<= 4096) best candidates are taken, which gives
     * the reference's result whenever a group has no more candidates than that OR nms_post_max boxes are kept among them (the greedy
     * order makes the first kept boxes independent of later candidates).  A group for which neither holds reports count -1 and no rows
     * (out_count and counts_out): never a silently different answer.  Equal scores: the reference's order among them is numpy's
     * unstable argsort reversed, here the lower cell index first. */
    int nms_kind; /* 0: rotated BEV IoU > nms_iou_threshold (rotate_nms_pcdet); 1: circular */
    int n_radius; /* nms_kind 1: entries of circle_radius in use, 1..16 */
    float circle_radius[16];
} fd_decode_cfg;

/* A head map as the decode reads it: element (group g, channel ch, BEV cell) of a float32 (dtype 0) or bf16 (dtype 1) tensor at
 * data[g * group_stride + ch * channel_stride + cell * cell_stride] (strides in elements).  NCHW planes: channel_stride = H*W,
 * cell_stride = 1.  A channel slice of an NHWC convolution output: channel_stride = 1, cell_stride = C_total, data = base + c0 --
 * the decode then reads the head's output in place (center_head.py:559-697 works on the permuted NHWC tensors the same way). */
typedef struct fd_map_view {
    const void *data;
    int64_t group_stride, channel_stride, cell_stride;
    int dtype;
} fd_map_view;

size_t fd_decode_workspace_bytes(int G, const fd_decode_cfg *cfg);
/* fd_centerpoint_decode on map views (any layout / float32 or bf16); the group index of a view is g = group * B + sample */
int fd_centerpoint_decode_maps(const fd_map_view *hm, const fd_map_view *reg, const fd_map_view *height, const fd_map_view *dim,
                               const fd_map_view *rot, int G, const fd_decode_cfg *cfg_host, float *out_boxes7, float *out_scores,
                               int32_t *out_cell, int32_t *out_count, void *workspace, size_t workspace_bytes, fd_stream_t stream);
/* Final assembly of CenterHead.predict's output (center_head.py:559-570 standard head: step s = the shared boxes + velocity
 * channels 2s, 2s+1; :606-607 dense head: step s = task s; :672-697 label offsets and concatenation): for sample b and output step s
 * the kept boxes of decode group step_group[s] * B + b with the velocity read from ``vel`` (a map view whose group index is
 * group * B + sample) at channels step_vel_channel[s], +1 and the label step_label[s], as packed rows
 * [B, S, post_max, 11] = x y z w l h vx vy yaw score label (rows >= count zero) and counts_out [B, S].  step_* are HOST arrays (S <= 16). */
int fd_assemble_detections(const float *boxes7, const float *scores, const int32_t *cell, const int32_t *count, const fd_map_view *vel,
                           int B, int post_max, int S, const int32_t *step_group, const int32_t *step_vel_channel,
                           const int32_t *step_label, float *packed, int32_t *counts_out, fd_stream_t stream);
/* fd_centerpoint_decode_maps + fd_assemble_detections in ONE call: the last kernel of the decode (greedy sweep from LDS, gather of the kept
 * boxes) also writes the packed rows of every output step (arguments as in the two calls above; G = groups * B, decode group
 * g = group * B + sample; step_* are HOST arrays, S <= 16).  out_boxes7 / out_scores / out_cell / out_count receive what
 * fd_centerpoint_decode_maps would write. */
int fd_centerpoint_decode_packed(const fd_map_view *hm, const fd_map_view *reg, const fd_map_view *height, const fd_map_view *dim,
                                 const fd_map_view *rot, const fd_map_view *vel, int G, int B, const fd_decode_cfg *cfg_host, int S,
                                 const int32_t *step_group, const int32_t *step_vel_channel, const int32_t *step_label, float *out_boxes7,
                                 float *out_scores, int32_t *out_cell, int32_t *out_count, float *packed, int32_t *counts_out, void *workspace,
                                 size_t workspace_bytes, fd_stream_t stream);
int fd_centerpoint_decode(const float *hm, int64_t hm_gstride, const float *reg, int64_t reg_gstride,
                          const float *height, int64_t height_gstride, const float *dim, int64_t dim_gstride,
                          const float *rot, int64_t rot_gstride, int G, const fd_decode_cfg *cfg_host,
                          float *out_boxes7, float *out_scores, int32_t *out_cell, int32_t *out_count,
                          void *workspace, size_t workspace_bytes, fd_stream_t stream);

/* Stand-alone rotated NMS with nms_gpu's contract (boxes [n,7] pcdet layout, already score-sorted):
 * keep[0:count] = kept indices (int64), count -> out_count (device int32).  Replaces
 * iou3d_nms_cuda.nms_gpu (iou3d_nms_api.cpp:11-17, iou3d_nms.cpp:90-135). */
size_t fd_nms_workspace_bytes(int n);
int fd_rotated_nms(const float *boxes7, int n, float thresh, int64_t *keep, int32_t *out_count,
                   void *workspace, size_t workspace_bytes, fd_stream_t stream);
/* pairwise rotated BEV IoU, replaces boxes_iou_bev_gpu (iou3d_nms.cpp:49-69) */
int fd_boxes_iou_bev(const float *a7, int na, const float *b7, int nb, float *out, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Sweep assembly (the step in front of the voxelizer).  Replaces the NuScenes branch of
 * LoadPointCloudFromFile.__call__ (det3d/datasets/pipelines/loading.py:107-141) together with read_file's
 * column cut (:31), remove_close (:36-45) and read_sweep (:47-60): the raw rows of the key frame and of the
 * sweeps (in the order the reference visits them) are filtered, moved into the key frame's coordinates and
 * given their time column, in input order.
 *   raw          [n_rows, raw_cols] float32, the concatenated contents of the .bin files (raw_cols = 5)
 *   sweeps_dev   [n_sweeps] descriptors IN DEVICE MEMORY, consecutive row ranges starting at row 0.  n_rows is an UPPER BOUND
 *                (ABI 7): rows at or past the last descriptor's row_end are dropped, so a fixed-capacity buffer whose fill is only
 *                known to the descriptors can be assembled by a launch captured once (FullSweepStep, detectors.py)
 *                m = transform_matrix (row-major 4x4, float64 as the reference's np.dot evaluates it; ignored
 *                unless FD_SWEEP_HAS_TRANSFORM), time = float32(time_lag) (0 for the key frame)
 *   out_points   [n_rows, keep_cols + 1] float32; rows [0, *out_count) are the reference's
 *                res["lidar"]["combined"]; rows [*out_count, n_rows) are filled with +inf (outside any range)
 *   out_count    device int32[1]
 * ------------------------------------------------------------------------------------------------- */
#define FD_SWEEP_HAS_TRANSFORM 1 /* sweep["transform_matrix"] is not None (loading.py:53) */
#define FD_SWEEP_REMOVE_CLOSE 2  /* read_sweep's remove_close (loading.py:50); not applied to the key frame (:113) */
typedef struct fd_sweep_desc {
    double m[16];
    int64_t row_begin, row_end;
    float time;
    int32_t flags;
} fd_sweep_desc;
size_t fd_sweep_assemble_workspace_bytes(int64_t n_rows);
int fd_sweep_assemble(const float *raw, int raw_cols, int keep_cols, int64_t n_rows, const fd_sweep_desc *sweeps_dev,
                      int n_sweeps, float min_distance, float *out_points, int32_t *out_count, void *workspace,
                      size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * PointPillars reader.  Replaces PillarFeatureNet.forward (det3d/models/readers/pillar_encoder.py:113-164) and
 * its PFNLayers (:38-55: Linear(bias=False) -> eval BatchNorm1d -> ReLU -> max over the pillar's points
 * [-> concat with the repeated max]) in one launch; nothing of shape [M, P, C] is written to memory.
 *   voxels      [m_max, max_points, ndim] float32 zero padded (fd_voxelize's out_voxels)
 *   num_points  [m_max] int32;  coors4 [m_max, 4] int32 (b,z,y,x);  n_dev: device pillar count or NULL (= m_max)
 *   vx, vy, x_offset, y_offset : PillarFeatureNet.vx/.vy/.x_offset/.y_offset (:107-110)
 *   w1 [units1, ndim+5(+1)] = pfn_layers[0].linear.weight; scale/shift = the eval BatchNorm1d as y = x*scale+shift
 *   w2 [units2, 2*units1]   = pfn_layers[1].linear.weight or NULL for a single layer (num_filters=(64,))
 *   out         [m_max, out_stride] float32 (out_dtype 0) or bf16 (1); rows >= the pillar count are not written
 * ------------------------------------------------------------------------------------------------- */
int fd_pillar_encode(const float *voxels, const int32_t *num_points, const int32_t *coors4, const int32_t *n_dev,
                     int64_t m_max, int max_points, int ndim, int with_distance, float vx, float vy, float x_offset,
                     float y_offset, const float *w1, const float *scale1, const float *shift1, int units1,
                     const float *w2, const float *scale2, const float *shift2, int units2, int out_dtype, void *out,
                     int out_stride, fd_stream_t stream);

/* PointPillarsScatter.forward (pillar_encoder.py:186-221): out[b, c, y, x] = feats[row, c] for coors4[row] = (b,_,y,x),
 * zero elsewhere (zero_first != 0 clears the dense B*c*H*W canvas first).  Strides are in elements, so the same call
 * writes an NCHW float32 canvas (reference layout) or an NHWC bf16 one (hand-written conv path). */
int fd_pillar_scatter(const void *feats, int c, int feat_stride, int dtype, const int32_t *coors4, const int32_t *n_dev,
                      int64_t m_max, int B, int H, int W, void *out, int out_dtype, int64_t stride_b, int64_t stride_c,
                      int64_t stride_y, int64_t stride_x, int zero_first, fd_stream_t stream);


/* ---------------------------------------------------------------------------------------------------
 * Forecast association: the numeric core of `tracker` (det3d/datasets/nuscenes/nuscenes.py:125-257), `match_boxes`
 * (:112-123) and `distance_matrix` (:100-110) for one sweep: T forecast steps with counts[t] <= n_max boxes each.
 *   centers, velocity [T, n_max, 3] float64 (Box.center / Box.velocity);  time_dev [T-1] float64 (seconds between steps)
 *   fwd_idx [n_max, T], fwd_ok [n_max] : forward chain of step-0 box i (index per step) and "not void" flag
 *                                        (every hop <= reject_thresh, :160-173)
 *   bwd_idx [n_max, T], bwd_ok [n_max] : back-cast chain of last-step box i, hop s goes from step T-1-s to T-2-s (:222-237)
 *   match_idx [T, n_max]               : match_boxes: nearest step-t box to step-0 box i
 *   cv_centers [n_max, T, 3]           : constant-velocity forward trajectory of step-0 box i (:183-193)
 *   status int32[1]                    : 1 when some step has no box (the reference then returns no trajectory); a negative
 *                                        count is an empty step
 * ------------------------------------------------------------------------------------------------- */
int fd_forecast_chains(const double *centers, const double *velocity, const int32_t *counts, const double *time_dev, int T,
                       int n_max, double reject_thresh, int32_t *fwd_idx, int32_t *fwd_ok, int32_t *bwd_idx, int32_t *bwd_ok,
                       int32_t *match_idx, double *cv_centers, int32_t *status, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Head output -> global-frame boxes: _second_det_to_nusc_box (det3d/datasets/nuscenes/nusc_common.py:167-189: yaw ->
 * -yaw - pi/2 in float32, Quaternion(axis z, that angle), velocity (vx, vy, 0)) followed by _lidar_nusc_box_to_global
 * (:192-216: rotate + translate by the calibrated_sensor record, then by the ego_pose record).  The two records are host
 * arrays (rotation w,x,y,z / translation x,y,z, float64) instead of devkit table look-ups; pass NULL pairs to stay in
 * the lidar frame.  Outputs: center [n,3], quat [n,4] (w,x,y,z), velocity [n,3] float64 (Box.center / .orientation /
 * .velocity), size [n,3] float32 (Box.wlh).
 * ------------------------------------------------------------------------------------------------- */
int fd_det_to_global_boxes(const float *box3d9, int n, const double *cs_rotation4_host, const double *cs_translation3_host,
                           const double *pose_rotation4_host, const double *pose_translation3_host, double *center,
                           double *quat, double *velocity, float *size, fd_stream_t stream);
/* multi_future's grouping (det3d/datasets/nuscenes/nuscenes.py:299-339 with network_split :283-297): boxes whose centres
 * (all three coordinates, distance_matrix :100-110) are closer than match_thresh are linked; ids[i] = index of box i's
 * connected component, components numbered by their smallest member (networkx's enumeration order).  n <= 8192. */
int fd_forecast_groups(const double *centers3, int n, double match_thresh, int32_t *ids, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The three calls above for a whole batch, device-resident and capturable (ABI 7): from the head's packed output
 * (fd_centerpoint_decode_packed: packed [B, T, post, row_floats] float32 rows = box 9 + score + label, counts [B, T]) to what
 * `forecast_boxes` + `tracker` + `multi_future` produce for each sweep (det3d/datasets/nuscenes/nuscenes.py:384-494 with
 * forecast_mode "velocity_dense", :125-257, :299-339; nusc_common.py:167-216), as arrays:
 *   records_dev  [B][14] float64 in DEVICE memory: calibrated_sensor rotation (w,x,y,z), translation (x,y,z), ego_pose rotation,
 *                translation of every sample (the devkit look-ups of nuscenes.py:385-398 are the caller's); NULL = lidar frame.
 *                Device memory, because a captured graph is replayed for other samples: nothing of a sample is a kernel argument
 *   time_dev     [B][T-1] float64: seconds between consecutive forecast steps (get_time, nuscenes.py:399-406)
 *   counts       [B][T] int32 in device memory: a step holds min(count, post) boxes.  A negative count (circular NMS's undecided
 *                group, -1) is an empty step, like 0: status = 1, n_traj = 0, no trajectory of that sample
 *   out->center / quat / velocity [B,T,post,3|4|3] float64, size [B,T,post,3] float32: every slot's global-frame box
 *   out->fwd_idx ... status: fd_forecast_chains' outputs per sample ([B, ...] in front of the shapes documented there, n_max = post)
 *   out->traj_kind / traj_src / traj_first / traj_group [B, 3*post] int32, n_traj [B] (all five or none): the sweep's trajectories in
 *                tracker's order -- kind 0 = forward chain of step-0 box src (fwd_idx[src][:]), 1 = constant-velocity roll-out of
 *                step-0 box src (cv_centers[src][:]), 2 = back-cast chain of last-step box src (bwd_idx[src][::-1]); first = the
 *                step-0 box the trajectory begins with; group = multi_future's forecast_id among the sweep's trajectories (components
 *                of "first boxes closer than match_thresh", numbered by their smallest member).  Entries past n_traj are -1.
 * Three launches (boxes, association, trajectories); bit-identical to the three single-sweep calls.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fd_forecast_buffers {
    double *center, *quat, *velocity;
    float *size;
    int32_t *fwd_idx, *fwd_ok, *bwd_idx, *bwd_ok, *match_idx;
    double *cv_centers;
    int32_t *status;
    int32_t *traj_kind, *traj_src, *traj_first, *traj_group, *n_traj;
} fd_forecast_buffers;
int fd_forecast_from_detections(const float *packed, const int32_t *counts, int B, int T, int post, int row_floats,
                                const double *records_dev, const double *time_dev, double reject_thresh, double match_thresh,
                                const fd_forecast_buffers *out, fd_stream_t stream);

/* The search of process_trajectories (det3d/datasets/nuscenes/nuscenes.py:341-382, forecast_boxes with postprocess=True :465-467):
 * idx[i] = argmin_j || library[j] - queries[i] || over the rows of a trajectory library [n_library, dim] (float64, row =
 * [vx, vy, q0..q3, centre_1 - centre_0, ...]); the first minimum wins like np.argmin.  Exact squared differences instead of the
 * reference's |a|^2 + |b|^2 - 2ab expansion: the two can only disagree between library rows that are equidistant to 1e-15. */
int fd_nearest_rows(const double *library, int n_library, const double *queries, int n_queries, int dim, int32_t *idx, fd_stream_t stream);

/* The whole index pyramid of the backbone in one call (the same launches as fd_index_mark / _downsample / _scan /
 * _coords above, issued back to back): level 0 is marked from the voxelizer's coords of every sample
 * (coords [B * n_max_per_sample, 4], n_dev[b] = voxel count of sample b or NULL), level l > 0 is derived from
 * level l-1 with its ksize/stride/pad (the strided SparseConv3d of scn.py:110,120,130,141); counts_dev[l] receives
 * the active count of level l.  The caller need not initialise any level's words (level 0 is cleared by this call, the other
 * levels are overwritten); all levels are scanned by one
 * set of launches: workspace >= fd_index_workspace_bytes(sum of the levels' fd_index_num_cols + 2048 * n_levels).  fd_index_pyramid_coords materialises coords for the levels whose pointer is
 * set (after the host has read the counts and allocated them).  When EVERY level passed to fd_index_pyramid already has its
 * coords pointer set (capacity-sized tables, coords_rows = capacity), the coordinates are written in the same pass and
 * fd_index_pyramid_coords need not be called. */
typedef struct fd_index_level {
    int32_t D, H, W;
    int32_t ksize[3], stride[3], pad[3]; /* how this level derives from the previous one (unused for level 0) */
    uint64_t *words;
    int32_t *prefix;
    int32_t *coords; /* [n_l, 4] or NULL */
    int64_t coords_rows; /* rows of ``coords``: an active voxel whose row index is >= coords_rows is not written (capacity-sized
                          * levels of the sync-free step; 0 = unbounded, the caller sized coords from the counts) */
} fd_index_level;
int fd_index_pyramid(const int32_t *coords, const int32_t *n_dev, int64_t n_max_per_sample, int B, int n_levels,
                     const fd_index_level *levels_host, int32_t *counts_dev, void *workspace, size_t workspace_bytes,
                     fd_stream_t stream);
int fd_index_pyramid_coords(int B, int n_levels, const fd_index_level *levels_host, fd_stream_t stream);

/* fd_index_lookup + fd_rows_permute in one launch: dst[row(coords_in[i])][:] = src[i][:] (channels >= c_src zeroed) for
 * the first n_dev[0] (<= n_max) voxels; this is how the voxelizer's per-voxel features become rows of the level-0
 * SparseConvTensor (scn.py:154) in index order. */
int fd_rows_place(const uint64_t *words, const int32_t *prefix, int B, int D, int H, int W, const int32_t *coords_in,
                  const int32_t *n_dev, int64_t n_max, const float *src, int c_src, void *dst, int c_dst, int dst_bf16,
                  fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Deformable 3x3 convolution (DCN v1) of the CenterHead dcn_head option: the cls and the reg FeatureAdaption of one DCNSepHead
 * in ONE launch (det3d/models/bbox_heads/center_head.py:40-78,176-229; module det3d/ops/dcn/deform_conv.py:192-240, arithmetic
 * det3d/ops/dcn/src/deform_conv_cuda_kernel.cu:85-117,191-240).  Purely additive: fd_abi_version() stays 8.
 * x [B,H,W,C] NHWC, C = 64, fp32 (bf16 = 0) or bf16 (bf16 = 1); y [B,H,W,128] of the same dtype: channels 0-63 =
 * ReLU(DeformConv_cls(x, offset_cls)), 64-127 = ReLU(DeformConv_reg(x, offset_reg)); deformable groups 4, padding 1, no bias.
 * Offsets are fp32 in both dtypes: either computed in the kernel from x by the 1x1 conv_offset of both branches (off_w
 * [2][72][64] fp32 = [branch][offset channel][input channel], off_b [2][72]; `offsets` NULL) or read from `offsets` [B,H,W,144]
 * fp32 (branch-major, the reference's channel order within a branch: group * 18 + 2 * tap + {0 = dh, 1 = dw}; off_w / off_b
 * ignored).  Weights: fd_deform_adapt_pack_weight of the two [64, 64, 3, 3] conv_adaption weights (host buffers of
 * fd_deform_adapt_packed_weight_bytes(bf16) bytes).  x, y and wpacked 16-byte aligned. */
size_t fd_deform_adapt_packed_weight_bytes(int bf16);
int fd_deform_adapt_pack_weight(const float *w_cls_oihw_host, const float *w_reg_oihw_host, int bf16, void *wpacked_host);
int fd_deform_adapt_nhwc(const void *x, int B, int H, int W, int C, int bf16, const float *off_w, const float *off_b, const float *offsets,
                         const void *wpacked, void *y, fd_stream_t stream);

/* Training of the pair (fd_deform_conv_grad.hip): the reference's deformable_col2im / deformable_col2im_coord
 * (deform_conv_cuda_kernel.cu) for the shapes above, fp32 only.  Purely additive: fd_abi_version() stays 8.
 * Inputs: x [B,H,W,64], offsets [B,H,W,144] as the forward reads them, the two conv_adaption weights [64,64,3,3] (OIHW) in
 * DEVICE memory, the forward's output y [B,H,W,128] (only its sign is used: the ReLU mask y > 0) and dy [B,H,W,128].
 * Outputs, each skipped when NULL: dx [B,H,W,64] (zeroed here on the stream, then fp32 atomic adds: equal from run to run only
 * up to the summation order), doffsets [B,H,W,144] and dw [2][64][64][3][3] (cls, reg; OIHW) -- both bit-identical from run to
 * run.  At an integer sample coordinate the offset gradient is the right-hand derivative (get_coordinate_weight).  The call
 * neither allocates nor synchronises; workspace of fd_deform_adapt_backward_workspace_bytes(B, H, W) bytes (0 = bad shape).
 * All tensor pointers and the workspace 16-byte aligned.
 * fd_deform_adapt_pack_weight_device: the fp32 form of fd_deform_adapt_pack_weight from device weights into device memory,
 * byte-identical to the host packer's output (fd_deform_adapt_packed_weight_bytes(0) bytes). */
size_t fd_deform_adapt_backward_workspace_bytes(int B, int H, int W);
int fd_deform_adapt_backward(const float *x, const float *offsets, const float *w_cls_oihw, const float *w_reg_oihw, const float *y, const float *dy,
                             int B, int H, int W, int C, float *dx, float *doffsets, float *dw, void *workspace, size_t workspace_bytes,
                             fd_stream_t stream);
int fd_deform_adapt_pack_weight_device(const float *w_cls_oihw, const float *w_reg_oihw, void *wpacked, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: the backward pass of the fp32 sparse convolution (fd_spconv_grad.hip) -- spconv 1.0's indice_conv_backward /
 * indice_subm_conv_backward (gradients of scn.py:99-141 under loss.backward()).  Purely additive: fd_abi_version() stays 8.
 * fp32 only; cin, cout in {16, 32, 64, 128}.  The weight gradient's kernel and entry-point body are shared with the bf16 rows below
 * (fd_spconv_wgrad.h); the element order of the packed weights, for the host packer and both device packers: fd_spconv_pack.h.
 *   fd_spconv_wgrad:  dw[k] = sum_o in[nbr[k][o]]^T . dy[o]  ([K, cin, cout] fp32, overwritten) for the output-stationary table of
 *                     fd_rulebook; dy [n_out, cout].  Deterministic: per-(512-row chunk, tap) partials in `workspace`
 *                     (fd_spconv_wgrad_workspace_bytes), summed in chunk order -- bit-identical whatever the launch.  n_out_dev as in
 *                     fd_spconv_apply (rows >= the device count contribute nothing).  The input gradient is fd_spconv_apply itself:
 *                     SubM: the same nbr with fd_spconv_pack_weight_device mode 2 (W[K-1-k]^T); strided: the table of
 *                     fd_rulebook_transpose with mode 1 (W[k]^T), n_out = n_in.
 *   fd_rulebook_transpose: inv[k][i] = o where nbr[k][o] = i, else -1 ([K, inv_stride], inv_stride >= n_in, every entry written).
 *   fd_spconv_pack_weight_device: fd_spconv_pack_weight (dtype 0) on the device, byte for byte, of W'[k] = W[k] (mode 0),
 *                     W[k]^T (mode 1: a [K, cout, cin] problem) or W[K-1-k]^T (mode 2); w_kio [K, cin, cout] fp32 device memory,
 *                     wpacked fd_spconv_packed_weight_bytes(K, cin', cout', 0) bytes.
 *   fd_dense_gather:  the backward of fd_densify: feats[row, ch] = dense[b * stride_b + (ch * D + z) * stride_c + y * stride_y + x *
 *                     stride_x] for coords[row] = (b, z, y, x); rows >= min(n_rows, *n_dev) are written as 0.
 * ------------------------------------------------------------------------------------------------- */
size_t fd_spconv_wgrad_workspace_bytes(int K, int64_t n_out, int cin, int cout);
int fd_spconv_wgrad(const float *in_feats, int64_t n_in, const float *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                    const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_rulebook_transpose(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, int64_t n_in, int32_t *inv,
                          int64_t inv_stride, fd_stream_t stream);
int fd_spconv_pack_weight_device(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream);
int fd_dense_gather(const float *dense, int64_t stride_b, int64_t stride_c, int64_t stride_y, int64_t stride_x, int D, const int32_t *coords,
                    int64_t n_rows, const int32_t *n_dev, int c, float *feats, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mixed-precision training of the sparse convolution (fd_spconv_grad_bf16.hip): bf16 rows, fp32 master weights and gradients.
 * Purely additive: fd_abi_version() stays 8.  The forward is fd_spconv_apply(dtype 1); the input gradient is fd_spconv_apply(dtype 1)
 * on the transposed problem exactly as above, for which the bf16 kernels also take 32 -> 16, 64 -> 32 and 128 -> 64.
 *   fd_spconv_wgrad_bf16:  fd_spconv_wgrad (the same kernel skeleton and summation order, fd_spconv_wgrad.h) with bf16 in_feats [n_in, cin]
 *                     and dy [n_out, cout]; dw [K, cin, cout] stays FP32 (overwritten).
 *                     bf16 x bf16 products accumulated in fp32 on the matrix core.  (cin, cout) in {16->16, 16->32, 32->32, 32->64, 64->64,
 *                     64->128, 128->128}.  The same per-(512-row chunk, tap) partials in `workspace`
 *                     (fd_spconv_wgrad_bf16_workspace_bytes; 0 = bad sizes), summed in chunk order: bit-identical whatever the launch, no
 *                     atomics.  n_out_dev as in fd_spconv_apply; n_out == 0 writes zeros.  Feature matrices of 2 GB and more: FD_EINVAL.
 *                     Neither allocates nor synchronises.
 *   fd_spconv_pack_weight_device_bf16: fd_spconv_pack_weight (dtype 1) on the device, byte for byte (every section of the buffer, the same
 *                     round-to-nearest-even), of W'[k] = W[k] (mode 0), W[k]^T (mode 1: a [K, cout, cin] problem) or W[K-1-k]^T (mode 2);
 *                     w_kio [K, cin, cout] fp32 device memory, wpacked fd_spconv_packed_weight_bytes(K, cin', cout', 1) bytes.  One launch,
 *                     no host round trip.
 * ------------------------------------------------------------------------------------------------- */
size_t fd_spconv_wgrad_bf16_workspace_bytes(int K, int64_t n_out, int cin, int cout);
int fd_spconv_wgrad_bf16(const void *in_feats, int64_t n_in, const void *dy, const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out,
                         const int32_t *n_out_dev, int cin, int cout, float *dw, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_spconv_pack_weight_device_bf16(const float *w_kio, int K, int cin, int cout, int mode, void *wpacked, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mixed-precision training of the dense stride-1 convolutions (fd_conv2d_grad_bf16.hip): bf16 NHWC activations, fp32 master weights
 * and gradients.  Purely additive: fd_abi_version() stays 8.  The forward is fd_conv2d_nhwc_bf16; the input gradient is
 * fd_conv2d_nhwc_bf16 on dy with the mode-1 weights below (a cout -> cin convolution of the same kernel size and padding).
 *   fd_conv2d_pack_weight_dev: replaces fd_conv2d_pack_weight (a host loop + upload, i.e. a synchronisation per step) in training.
 *                     w_oihw [cout][cin][ks][ks] fp32 DEVICE memory, ks 1 or 3, cin % 32 == 0.  mode 0: byte for byte what
 *                     fd_conv2d_pack_weight writes ([cout_pad/32][cin/32][tap][ksub][lane][8] bf16, the same round-to-nearest-even,
 *                     zeros for co >= cout).  mode 1: the packed form of w'[ci][co][ks-1-ky][ks-1-kx] = w[co][ci][ky][kx], the
 *                     cin' = cout, cout' = cin problem; needs cout % 32 == 0; fd_conv2d_packed_weight_bytes(cin, cout, ks) bytes.
 *                     One launch, no host copy.
 *   fd_conv2d_wgrad_bf16: replaces the fp32 NCHW weight gradient torch runs for these layers.  x [B,H,W,cin] bf16, dy [B,H,W,cout]
 *                     bf16 (stride 1; padding 1 for ks 3, 0 for ks 1), cin and cout multiples of 32 -> dw [cout][cin][ks][ks] FP32
 *                     (overwritten).  bf16 x bf16 products accumulated in fp32 on the matrix core.  The pixels, in (b, y, x) order,
 *                     are cut into chunks of fd_conv2d_wgrad_bf16_chunk() (a constant of the library); one fp32 partial per (chunk,
 *                     tap) goes to `workspace` (fd_conv2d_wgrad_bf16_workspace_bytes; 0 = bad arguments) and the partials are summed
 *                     in chunk order: bit-identical from run to run, no atomics.  The workspace need not be initialised: every word
 *                     that is read has been written by the same call.  Maps of 2^31 pixels and more: FD_EINVAL.  Neither allocates
 *                     nor synchronises.
 * ------------------------------------------------------------------------------------------------- */
int fd_conv2d_pack_weight_dev(const float *w_oihw, int cout, int cin, int ks, int mode, void *wpacked, fd_stream_t stream);
int fd_conv2d_wgrad_bf16_chunk(void);
size_t fd_conv2d_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin, int cout, int ks);
int fd_conv2d_wgrad_bf16(const void *x, const void *dy, int B, int H, int W, int cin, int cout, int ks, void *workspace,
                         size_t workspace_bytes, float *dw, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mixed-precision training of the CenterHead's final convolutions (fd_head_tail_bf16.hip): 3 x 3, padding 1, stride 1, cin % 32 == 0
 * input channels, 1 <= k <= 16 output channels, a bias; bf16 NHWC input, fp32 NCHW output for the loss.  Purely additive:
 * fd_abi_version() stays 8.  One launch serves up to fd_head_tail_bf16_max_groups() group records (a longer array is FD_EINVAL: the
 * caller splits it); all groups cover the same B x H x W pixels.  A record (fd_head_tail_group): x, bf16, channel c of pixel p at
 * x[p * x_stride + c] with x_stride >= cin, x_stride % 8 == 0 and x 16-byte aligned -- so a group can read, and its input gradient fill,
 * a cin-channel slice of a wider NHWC tensor; w [k][cin][3][3] fp32; bias [k] fp32; y [B][k][H][W] fp32.  What each entry point does
 * with them:
 *   fd_head_tail_forward_bf16: reads x, w (rounded to bf16 inside, nearest even) and bias; writes y = fp32 accumulation on the matrix
 *                     core + bias, not rounded again.
 *   fd_head_tail_dgrad_bf16: reads w and y (= dy, rounded to bf16 as the operand); WRITES x (= dx: fp32 accumulation rounded once to
 *                     bf16, channels 0 .. cin - 1 of every pixel and nothing else); bias is not looked at and may be null.
 *   fd_head_tail_wgrad_bf16: reads x and y (= dy); WRITES w (= dW fp32, dy rounded to bf16 as the operand) and bias (= dbias fp32, the
 *                     sum of the unrounded dy in a fixed order).
 *   fd_head_tail_wgrad_bf16: the input pixels, in (b, y, x) order, are cut into chunks of fd_head_tail_wgrad_bf16_chunk() (a constant of
 *                     the library); one fp32 [10][cin][16] partial per (group, chunk) -- nine taps and the bias gradient -- goes to `workspace`
 *                     (fd_head_tail_wgrad_bf16_workspace_bytes with cin_sum = the sum of the groups' cin; 0 = bad arguments) and the
 *                     partials are summed in chunk order: bit-identical from run to run, no atomics.  The workspace need not be
 *                     initialised: every word that is read has been written by the same call.
 * Every entry point validates before any device work (FD_EINVAL + fd_last_error), neither allocates nor synchronises.
 * ------------------------------------------------------------------------------------------------- */
typedef struct fd_head_tail_group {
    void *x;
    float *w;
    float *bias;
    void *y;
    int64_t x_stride;
    int cin;
    int k;
} fd_head_tail_group;
int fd_head_tail_bf16_max_groups(void);
int fd_head_tail_wgrad_bf16_chunk(void);
size_t fd_head_tail_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin_sum);
int fd_head_tail_forward_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, fd_stream_t stream);
int fd_head_tail_dgrad_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, fd_stream_t stream);
int fd_head_tail_wgrad_bf16(const fd_head_tail_group *groups, int n_groups, int B, int H, int W, void *workspace, size_t workspace_bytes,
                            fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training targets: AssignLabel's heat maps and box rows (fd_targets.hip) -- det3d/datasets/pipelines/preprocess.py:336-910
 * (NuScenesDataset branch) with gaussian_radius / draw_umich_gaussian of det3d/core/utils/center_utils.py:17-64, for a whole batch
 * [B, T] and every target set in two launches.  Purely additive: fd_abi_version() stays 8.
 * Inputs: boxes [B, T, n_max, 12] fp32 (x y z w l h vx vy rvx rvy rot rrot, as LoadPointCloudAnnotations leaves them: rot / rrot are
 * passed through limit_period here), counts [B, T] int32 (objects per (sample, timestep); a count <= 0 is an empty timestep, a count
 * above n_max reads n_max), classes [B, T, n_max] int32 (1-based class id over all tasks' class names, anything else: in no task),
 * trajectory [B, T, n_max] int32 (0 static, 1 linear, 2 nonlinear, anything else: not in the trajectory set; read only when
 * n_sets = 3).
 * Sets (n_sets = 1: standard; 3: + trajectory (one task of 3 classes, preprocess.py:571-733) + forecast (one task of 7 classes: every
 * timestep's objects in timestep order, class = timestep + 1, preprocess.py:737-897; needs T <= 7)).  Maps per timestep
 * U = n_tasks (+ 2); map u has C_u channels (task_classes[u], then 3, then 7); Csum = their sum.
 * Outputs, every element written by the call:
 *   hm               fp32, one array of T * Csum * B * H * W elements (16-byte aligned, room for that count rounded up to 4):
 *                    [T][map u: [B][C_u][H][W]], map (t, u) starting at element (t * Csum + sum_{u' < u} C_u') * B * H * W;
 *   ind / cat        int64 [T][U][B][max_objs], mask uint8 and anno_box fp32 [.., 14] of the same shape (preprocess.py:519-531);
 *   gt_boxes_and_cls fp32 [n_sets][T][B][max_objs][13] (preprocess.py:548-567);
 *   status           int32 [B][T][n_sets]: 0, or 1 = the set holds more than max_objs objects (the reference's assert, :562).
 * workspace >= fd_targets_workspace_bytes(B, T, U, max_objs).  gaussian_overlap is the config's python float: the constants of
 * gaussian_radius are derived from it as numpy derives them. */
#define FD_TARGETS_MAX_TASKS 16
typedef struct fd_targets_cfg {
    int H, W;        /* heat-map rows and columns: grid[1] // out_size_factor, grid[0] // out_size_factor */
    int T, n_max, max_objs;
    int n_sets;      /* 1 or 3 */
    int n_tasks;     /* tasks of the standard set */
    int task_classes[FD_TARGETS_MAX_TASKS];
    int radius_mult; /* 0 / 1 */
    int min_radius;
    float out_size_factor, voxel_x, voxel_y, pc_x, pc_y;
    double gaussian_overlap;
} fd_targets_cfg;
size_t fd_targets_workspace_bytes(int B, int T, int maps_per_step, int max_objs);
int fd_assign_targets(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory, int B,
                      const fd_targets_cfg *cfg, float *hm, int64_t *ind, uint8_t *mask, int64_t *cat, float *anno_box,
                      float *gt_boxes_and_cls, int32_t *status, void *workspace, size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: PillarFeatureNet in train mode (fd_pillars_grad.hip) -- det3d/models/readers/pillar_encoder.py:15-164 with
 * BatchNorm1d on batch statistics, and its backward.  Purely additive: fd_abi_version() stays 8.  fp32; the shipped stack only:
 * two PFN layers, units1 = 32 (+32 repeated max) -> units2 = 64; max_points (P) in [1, 32]; N = m * max_points > 1 rows, every
 * point slot of every pillar (padded slots included, as torch's BatchNorm1d counts them).
 *   inputs as fd_pillar_encode (voxels [m, P, ndim], num_points [m], coors4 [m, 4], geometry); w1 [32, ndim+5(+1)],
 *   w2 [64, 64] (the linear weights), gamma / beta the BatchNorm weight / bias, eps1 / eps2 their eps.
 *   fd_pillar_train_forward: out [m, 64] fp32 (the reader's output), mean1 / var1 [32] and mean2 / var2 [64]: each layer's batch
 *                     mean and BIASED variance (the caller updates the running statistics).  Leaves in `workspace` what the
 *                     backward needs (per-pillar arg-max bytes, statistics): keep it untouched until the backward has run.
 *   fd_pillar_train_backward: dout [m, 64] -> dw1 [32, ndim+5(+1)], dgamma1 / dbeta1 [32], dw2 [64, 64], dgamma2 / dbeta2 [64],
 *                     all overwritten; same inputs and workspace as the forward call it follows.
 * workspace >= fd_pillar_train_workspace_bytes(m, max_points) (0 = invalid sizes).  No allocation, no synchronisation: both calls
 * can be captured into a graph.  Deterministic: fixed-order block partials and a fixed-order double-precision combine, no atomics.
 * ------------------------------------------------------------------------------------------------- */
size_t fd_pillar_train_workspace_bytes(int64_t m, int max_points);
int fd_pillar_train_forward(const float *voxels, const int32_t *num_points, const int32_t *coors4, int64_t m, int max_points, int ndim,
                            int with_distance, float vx, float vy, float x_offset, float y_offset, const float *w1, const float *gamma1,
                            const float *beta1, int units1, float eps1, const float *w2, const float *gamma2, const float *beta2, int units2,
                            float eps2, float *out, float *mean1, float *var1, float *mean2, float *var2, void *workspace,
                            size_t workspace_bytes, fd_stream_t stream);
int fd_pillar_train_backward(const float *voxels, const int32_t *num_points, const int32_t *coors4, int64_t m, int max_points, int ndim,
                             int with_distance, float vx, float vy, float x_offset, float y_offset, const float *w1, const float *gamma1,
                             const float *beta1, int units1, const float *w2, const float *gamma2, const float *beta2, int units2,
                             const float *dout, float *dw1, float *dgamma1, float *dbeta1, float *dw2, float *dgamma2, float *dbeta2,
                             void *workspace, size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * The same reader with its pillar counts in device memory (fd_pillars_grad.hip), for a training step that never waits for the
 * device.  Purely additive: fd_abi_version() stays 8.  The same kernels as the pair above, which are their one-segment,
 * host-count case.
 *   The buffers hold n_seg segments (1 <= n_seg <= 16) of seg_stride rows: voxels [n_seg * seg_stride, P, ndim], num_points and
 *   coors4 alike.  Segment b owns rows [b * seg_stride, b * seg_stride + cnt_b), cnt_b = clamp(seg_counts[b], 0, seg_stride),
 *   seg_counts a device int32[n_seg].  Rows behind a count may hold anything: they are neither read nor used as an address.
 *   The logical batch is the segments' live pillars in segment order, M = sum cnt_b pillars, N = M * P rows.
 *   fd_pillar_train_forward_dev / _backward_dev: the SAME BITS (out's live rows, the four statistics, the six gradients) as
 *                     fd_pillar_train_forward / _backward with m = M on those pillars in one contiguous buffer: pillars per block and
 *                     the live blocks come from the device total, the launch is sized by the capacity.  out [n_seg * seg_stride, 64]
 *                     is defined everywhere: rows behind a count are 0; dout has the same shape (its rows behind a count are not
 *                     read).  N < 2 (the empty batch): out, the statistics and every gradient are 0.
 *   fd_pillar_train_running_stats_dev: torch's BatchNorm rule for one layer, with n = P * sum cnt_b read on the device:
 *                     num_batches_tracked (int64, may be NULL) += 1, running_mean <- (1 - momentum) running_mean + momentum mean,
 *                     running_var <- (1 - momentum) running_var + momentum var n / (n - 1); evaluated in double precision, rounded
 *                     once.  n < 2: nothing is written.
 * workspace >= fd_pillar_train_workspace_bytes(n_seg * seg_stride, max_points): sized by the capacity.  No atomics, no allocation,
 * no synchronisation; deterministic and capturable like the pair above.
 * ------------------------------------------------------------------------------------------------- */
int fd_pillar_train_forward_dev(const float *voxels, const int32_t *num_points, const int32_t *coors4, const int32_t *seg_counts, int n_seg,
                                int64_t seg_stride, int max_points, int ndim, int with_distance, float vx, float vy, float x_offset,
                                float y_offset, const float *w1, const float *gamma1, const float *beta1, int units1, float eps1,
                                const float *w2, const float *gamma2, const float *beta2, int units2, float eps2, float *out, float *mean1,
                                float *var1, float *mean2, float *var2, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_pillar_train_backward_dev(const float *voxels, const int32_t *num_points, const int32_t *coors4, const int32_t *seg_counts, int n_seg,
                                 int64_t seg_stride, int max_points, int ndim, int with_distance, float vx, float vy, float x_offset,
                                 float y_offset, const float *w1, const float *gamma1, const float *beta1, int units1, const float *w2,
                                 const float *gamma2, const float *beta2, int units2, const float *dout, float *dw1, float *dgamma1,
                                 float *dbeta1, float *dw2, float *dgamma2, float *dbeta2, void *workspace, size_t workspace_bytes,
                                 fd_stream_t stream);
int fd_pillar_train_running_stats_dev(const float *mean, const float *var, int channels, double momentum, const int32_t *seg_counts, int n_seg,
                                      int64_t seg_stride, int max_points, float *running_mean, float *running_var,
                                      int64_t *num_batches_tracked, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: one optimiser step for a whole model (fd_optim.hip).  Purely additive: fd_abi_version() stays 8.  fp32.
 * Replaces, for the recipe of every shipped config (adam, fixed_wd, one_cycle, grad_clip max_norm / norm_type 2):
 *   the true weight decay of OptimWrapper.step, p.data.mul_(1 - wd * lr) on every parameter of both groups
 *     (det3d/solver/fastai_optim.py:158-174),
 *   clip_grad_norm_ of OptimizerHook.after_train_iter (det3d/torchie/trainer/hooks/optimizer.py:9-19),
 *   torch.optim.Adam(betas=(0.9, 0.99)).step() below it (det3d/torchie/apis/train.py:183-200), with the beta1 that OneCycle set for
 *     this iteration (det3d/solver/learning_schedules_fastai.py:53-67),
 *   and optimizer.zero_grad() (det3d/torchie/trainer/trainer.py:436-460 gives the order).
 * The parameter set is described once, on the device.  Tensor t (n_tensors of them):
 *   params[t]  uint64: address of the parameter's first element (contiguous fp32; any 4-byte alignment -- a tensor whose address is
 *              not 16-byte aligned or whose numel is not a multiple of 4 takes a scalar path on the parameter side);
 *   numel[t], offset[t]  int64: its length and where its segment starts in the three flat buffers grad / exp_avg / exp_avg_sq
 *              (`total` floats each, 16-byte aligned; every offset a multiple of 4; the padding between segments stays zero);
 *   flags[t]   int32: FD_OPTIM_DECAY (weight decay applies) | FD_OPTIM_HAS_GRAD (the tensor has a gradient this step);
 *   step[t]    int32: the tensor's own Adam step count, advanced by the call for tensors with a gradient;
 *   coef[2t..] fp32 scratch: lr / (1 - beta1^step), sqrt(1 - beta2^step), written by the call.
 * Work is cut into chunks of at most `chunk` (= fd_optim_chunk() = FD_OPTIM_CHUNK) elements of ONE tensor: chunks[2c] = tensor,
 * chunks[2c + 1] = index of the chunk inside the tensor (elements [index * chunk, ...)), n_chunks of them covering every tensor.
 * partials: double[n_chunks] scratch;  norm: fp32[2], written by a clipping call: total_norm, min(1, max_norm / (total_norm + 1e-6)).
 *
 * fd_optim_adam_step, per element of a tensor with a gradient g (clipped on the fly, g <- g * norm[1]; grad is NOT rewritten):
 *   p *= 1 - wd * lr (FD_OPTIM_DECAY);  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * in fp32 without contraction, the scalars rounded from double as torch rounds its python floats.  A tensor without a gradient is
 * decayed only: moments and step stay.  max_norm > 0: three launches (per-chunk sums of squares of the gradients in double, a
 * fixed-order finish in double, the step); max_norm <= 0: no clipping, two launches.  No atomics: the same bits on every run.
 * fd_optim_zero_grad: zeroes the flat gradient buffer (one launch).
 * Both validate on the host before any device work: a null table / member, n_tensors, n_chunks or total <= 0, chunk != FD_OPTIM_CHUNK,
 * beta outside [0, 1), eps <= 0 are FD_EINVAL.  No allocation, no synchronisation.
 * ------------------------------------------------------------------------------------------------- */
#define FD_OPTIM_CHUNK 4096
#define FD_OPTIM_DECAY 1
#define FD_OPTIM_HAS_GRAD 2
typedef struct fd_optim_table {
    const void *params;
    const void *numel, *offset;
    const void *flags;
    void *step;
    void *coef;
    const void *chunks;
    void *partials;
    void *norm;
    float *grad, *exp_avg, *exp_avg_sq;
    int64_t total;
    int32_t n_tensors, n_chunks, chunk;
} fd_optim_table;
int fd_optim_chunk(void);
int fd_optim_zero_grad(const fd_optim_table *table, fd_stream_t stream);
int fd_optim_adam_step(const fd_optim_table *table, double lr, double beta1, double beta2, double eps, double wd, double max_norm,
                       fd_stream_t stream);
/* fd_optim_adam_step_dev: the same kernels with the six scalars read from DEVICE memory at run time -- hyper[0..5] = lr, beta1, beta2,
 * eps, wd, max_norm (doubles, 8-byte aligned) -- so a launch captured into a graph follows a schedule that changes lr and beta1 at every
 * iteration.  Given the same six values it writes the same bits as fd_optim_adam_step (parameters, both moments, step, coef, norm):
 * both hand the kernels the same doubles.  clip (0 or 1) is a host argument because it fixes the launch count (1: three launches,
 * hyper[5] is max_norm; 0: two launches, norm = (0, 1), hyper[5] is not read).  skip (device int32[1], may be NULL): when non-zero at run
 * time the call changes nothing but norm (and the partials scratch): no decay, no moments, no step counts, no parameter update.
 * Host validation: the table as above, a null or misaligned hyper, clip not 0 or 1 are FD_EINVAL; the VALUES of the record cannot be
 * checked on the host -- the caller validates them before it uploads them (betas in [0, 1), eps > 0, no NaN). */
int fd_optim_adam_step_dev(const fd_optim_table *table, const double *hyper, int clip, const int32_t *skip, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: two small pieces of a step that never waits for the host (fd_rows.hip).  Purely additive: fd_abi_version() stays 8.
 * fd_rows_colsum: out[c] (fp32 [C]) = the sum over the first min(n, max(*n_dev, 0)) rows (n_dev NULL: n rows) of the row-major
 *   contiguous x [n, C], dtype 0 = fp32 rows, 1 = bf16 rows (widened exactly).  Rows at or behind the count are never read (they may
 *   be uninitialised).  C in {16, 32, 64, 128}; n in [0, 2^30]; n = 0 or a count of 0 gives zeros.  Rows are cut into chunks of
 *   fd_rows_colsum_chunk() (= FD_ROWS_COLSUM_CHUNK) rows; a chunk's 256 / C row lanes add their rows in row order and are added in lane
 *   order, the chunk partials likewise; all in double, rounded to fp32 once.  No atomics: the same bits on every run, and they depend
 *   on the count and C only, not on the capacity n.  Two launches (one for n = 0); no allocation, no synchronisation.
 *   workspace >= fd_rows_colsum_workspace_bytes(n, C) (0 = invalid sizes), 16-byte aligned.  FD_EINVAL for: an unsupported C or dtype,
 *   n out of range, null out, null x with n > 0, a workspace that is null, misaligned or too small.
 * fd_levels_overflow: one launch; flag[0] = 1 if counts[l] > caps[l] for any l < n_levels, else 0 (all three in device memory, int32;
 *   n_levels in [1, 64]).  FD_EINVAL for a null pointer or n_levels out of range.
 * ------------------------------------------------------------------------------------------------- */
#define FD_ROWS_COLSUM_CHUNK 512
int fd_rows_colsum_chunk(void);
size_t fd_rows_colsum_workspace_bytes(int64_t n, int C);
int fd_rows_colsum(const void *x, int64_t n, const int32_t *n_dev, int C, int dtype, float *out, void *workspace, size_t workspace_bytes,
                   fd_stream_t stream);
int fd_levels_overflow(const int32_t *counts, const int32_t *caps, int n_levels, int32_t *flag, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: the global augmentation of one sample (fd_augment.hip) -- the train-mode transforms of Preprocess
 * (det3d/datasets/pipelines/preprocess.py:189-192, 201-203): prep.random_flip_both, prep.global_rotation, prep.global_scaling_v2 and
 * prep.global_translate_ (det3d/core/sampler/preprocess.py:815-857, 776-799, 860-868, 967-992; the rotation itself is
 * box_np_ops.rotation_points_single_angle, det3d/core/bbox/box_np_ops.py:182-204) and the fixed-seed point shuffle, as a permutation.
 * Purely additive: fd_abi_version() stays 8.  One launch each, graph-capturable, no allocation, no workspace, no synchronisation.
 * fd_augment_record: one sample's draw.  flip_a / flip_b: the reference's first / second flip (non-zero = on); c, s: the float64
 *   cos / sin of the angle cast to fp32; rot, scale: the angle and the factor cast to fp32; tx, ty, tz: the float64 translation.
 * The arithmetic A, every product and sum rounded once in fp32 unless said otherwise (NumPy 2 on fp32 arrays), in this order:
 *   flip a   y = -y; boxes also columns 7 and 9, and columns 10, 11: a = -a + fl32(pi)
 *   flip b   x = -x; boxes also columns 6 and 8, and columns 10, 11: a = -a + fl32(2 pi)
 *   rotate   x' = x c + y s, y' = -(x s) + y c (z untouched); boxes: the column pairs (0, 1), (6, 7), (8, 9), and columns 10, 11 += rot.
 *            (The reference rotates the pairs (6, 7) and (8, 9) through a float64 copy and its BLAS product fuses as it likes: its
 *            rotated values lie within 4 ulp-sized steps of these, see tests/test_augment_host.py.)
 *   scale    xyz of a point, columns 0..9 of a box, times scale
 *   shift    fl32(double(v) + t) on x, y, z of points and boxes
 * fd_augment_points: dst[i] = A(src[perm ? perm[i] : i]) for i < n_rows, rows of ndim (4 or 5) fp32; columns 3 and up pass through bit
 *   for bit; dst rows at or past n_rows are not written.  perm: int32 [>= n_rows] in device memory, a permutation of 0..n_rows-1 (a
 *   row whose index lies outside that range is left unwritten; nothing is read out of bounds), or NULL.  rec: ONE record in device
 *   memory.  n_rows = 0 is a no-op.  16-byte accesses are used when src and dst are 16-byte aligned (ndim 5: and perm is NULL).
 *   FD_EINVAL for: ndim not 4 or 5, n_rows outside [0, FD_AUGMENT_MAX_ROWS], a null or misaligned record, null or misaligned (4 bytes)
 *   src / dst with n_rows > 0, src == dst or overlapping ranges.
 * fd_augment_boxes: boxes / out [B, T, n_max, 12] fp32, 16-byte aligned; counts int32 [B, T] and recs [B] in device memory.  Row i of
 *   (b, t) becomes A(row) with recs[b] when i < counts[b, t] and is copied unchanged otherwise.  out == boxes (in place) is allowed,
 *   any other overlap is not.  n_max = 0 is a no-op.  FD_EINVAL for: B or T < 1, n_max < 0, more than FD_AUGMENT_MAX_ROWS rows, null
 *   or misaligned pointers, partially overlapping boxes and out.
 * ------------------------------------------------------------------------------------------------- */
#define FD_AUGMENT_MAX_ROWS (1 << 28)
typedef struct fd_augment_record {
    int32_t flip_a, flip_b;
    float c, s, rot, scale;
    double tx, ty, tz;
} fd_augment_record;
int fd_augment_points(const float *src, int64_t n_rows, int ndim, const int32_t *perm, const fd_augment_record *rec, float *dst,
                      fd_stream_t stream);
int fd_augment_boxes(const float *boxes, const int32_t *counts, const fd_augment_record *recs, float *out, int B, int T, int n_max,
                     fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: what the reference does between the augmentation and AssignLabel (fd_augment_map.hip) -- the ground-truth range filter of
 * the train-mode Voxelization stage (det3d/datasets/pipelines/preprocess.py:249-255, prep.filter_gt_box_outside_range,
 * det3d/core/sampler/preprocess.py:113-127) and the warp of a bev_map head's mask (get_mask, preprocess.py:75-90, 212).
 * Purely additive: fd_abi_version() stays 8.  One launch each, graph-capturable, no atomics, no allocation, no workspace, no
 * synchronisation.
 *
 * fd_gt_range_filter: boxes [B, T, n_max, 12] fp32 (16-byte aligned), counts [B, T] int32, classes [B, T, n_max] int32, trajectory
 *   [B, T, n_max] int32 or NULL (then trajectory_out is ignored), all in device memory; the range (xmin, ymin, xmax, ymax) by value.
 *   The mask of sample b comes from the rows of timestep 0: with c0 = clamp(counts[b, 0], 0, n_max), object i < c0 is KEPT iff at
 *   least one of the four BEV corners of boxes[b, 0, i] lies strictly inside the range rectangle.  Every operation below is one fp32
 *   IEEE operation rounded on its own unless said otherwise (box_np_ops.center_to_corner_box2d -> corners_nd / rotation_2d):
 *     w, l = columns 3, 4; angle a = column 11 (the LAST column); s = fl32(sin(double(a))), c = fl32(cos(double(a))) (the reference
 *       takes NumPy's fp32 sin / cos, which lie within 1.5 ulp of these);
 *     corner k = 0..3, in the reference's order, has the offsets (ox, oy) = (-w/2, -l/2), (-w/2, +l/2), (+w/2, +l/2), (+w/2, -l/2);
 *     x_k = (ox c + oy s) + column 0,  y_k = (-(ox s) + oy c) + column 1   (rotation_2d: clockwise for a positive angle);
 *     the rectangle's vertices, as minmax_to_corner_2d builds them: x0 = xmin, x1 = xmin + (xmax - xmin), y0 = ymin,
 *       y1 = ymin + (ymax - ymin); P0 = (x0, y0), P1 = (x0, y1), P2 = (x1, y1), P3 = (x1, y0), edge vector V_j = P_j - P_(j-1 mod 4);
 *     inside (points_in_convex_polygon_jit, geometry.py:280): for every j, double(V_j.y (P_j.x - x_k)) - double(V_j.x (P_j.y - y_k))
 *       is NOT >= 0.  A corner exactly on a boundary line is therefore outside; a NaN corner counts as inside, as in the reference.
 *   The same mask is applied to every timestep t: with m = min(clamp(counts[b, t], 0, n_max), c0), the kept rows i < m of boxes,
 *   classes and trajectory move to the front in their order, counts_out[b, t] = their number, and every row at or past that number is
 *   PADDING, written as zeros (boxes 0.0f, classes 0, trajectory 0) up to n_max.  status[b] = the number of timesteps t with
 *   counts[b, t] != counts[b, 0] (the reference fails there: a boolean index of the wrong length); rows i >= c0 of such a step are
 *   dropped.  Each output may be its input (in place) or must not overlap it; outputs must not overlap one another.
 *   FD_EINVAL for: B or T < 1, n_max outside [1, FD_RANGE_FILTER_MAX_N], more than FD_AUGMENT_MAX_ROWS rows, a null pointer other
 *   than trajectory / trajectory_out, a trajectory without trajectory_out, boxes not 16-byte or int arrays not 4-byte aligned, a
 *   partial overlap of an output with its input, a range that is not finite or has xmax <= xmin or ymax <= ymin.
 *
 * fd_augment_mask: src, dst [B, C, H, W] fp32, recs [B] in device memory (8-byte aligned); dst must not overlap src.  Per plane
 *   dst = warp(warp(flip(src), m1), m2): flip_a reverses the W axis (np.fliplr of the reference's HWC mask), flip_b the H axis, both
 *   before the warps; m1, m2 are the INVERSE 2x3 matrices of the two warps, row-major.  warp(s, m) is OpenCV's classic warpAffine with
 *   INTER_LINEAR and a constant border of 0 on fp32; for the destination pixel (x, y):
 *     X = (rint((m[1] y + m[2]) 1024) + 16 + rint(m[0] x 1024)) >> 5,  Y = (rint((m[4] y + m[5]) 1024) + 16 + rint(m[3] x 1024)) >> 5
 *       (float64 products and sums rounded one by one, rint = round half to even, int32 with arithmetic shifts);
 *     sx = X >> 5, sy = Y >> 5, fx = float(X & 31) / 32, fy = float(Y & 31) / 32;
 *     w00 = (1 - fy)(1 - fx), w01 = (1 - fy) fx, w10 = fy (1 - fx), w11 = fy fx  (fp32);
 *     out = s[sy][sx] w00 + s[sy][sx + 1] w01 + s[sy + 1][sx] w10 + s[sy + 1][sx + 1] w11  (fp32, left to right, no fused
 *       multiply-add); every tap outside the plane reads 0.
 *   The intermediate plane lives in LDS (H W 4 bytes, one workgroup per plane).  The kernel reads nothing out of bounds whatever a
 *   record holds (a float64 coordinate is clamped to +-2^29 before it becomes an int32, which only moves taps that lie far outside
 *   the plane anyway), but the definition above holds only for records that fd_augment_mask_check accepts.
 *   FD_EINVAL for: B, C, H or W < 1, H W > FD_AUGMENT_MASK_MAX_PIXELS, B C H W > FD_AUGMENT_MAX_ROWS, null or misaligned pointers
 *   (src / dst 4 bytes, recs 8), overlapping src and dst.  FD_ELAUNCH when the runtime refuses the LDS allocation.
 * fd_augment_mask_check: host-only, recs_host [B] in HOST memory.  FD_EINVAL when a coefficient is not finite or when, for some
 *   pixel of an H x W plane, a fixed-point coordinate could leave int32 or sx / sy could leave int16 (OpenCV's own map format):
 *   accepted iff |m[0]| (W - 1) + |m[1]| (H - 1) + |m[2]| < FD_AUGMENT_MASK_MAX_COORD, and likewise for m[3], m[4], m[5], for both
 *   matrices.
 * ------------------------------------------------------------------------------------------------- */
#define FD_RANGE_FILTER_MAX_N 4096
#define FD_AUGMENT_MASK_MAX_PIXELS 40960
#define FD_AUGMENT_MASK_MAX_COORD 32000.0
typedef struct fd_augment_mask_record {
    int32_t flip_a, flip_b;
    double m1[6], m2[6];
} fd_augment_mask_record;
int fd_gt_range_filter(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory, float xmin, float ymin,
                       float xmax, float ymax, float *boxes_out, int32_t *counts_out, int32_t *classes_out, int32_t *trajectory_out,
                       int32_t *status, int B, int T, int n_max, fd_stream_t stream);
int fd_augment_mask(const float *src, const fd_augment_mask_record *recs, float *dst, int B, int C, int H, int W, fd_stream_t stream);
int fd_augment_mask_check(const fd_augment_mask_record *recs_host, int B, int H, int W);

/* ---------------------------------------------------------------------------------------------------
 * Training: ground-truth database sampling, "GT-AUG" (fd_gt_sample.hip) -- what Preprocess does with its db_sampler before the global
 * transforms (det3d/datasets/pipelines/preprocess.py:147-182; DataBaseSamplerV2.sample_all / sample_class_v2,
 * det3d/core/sampler/sample_ops.py:101-253, 275-351; box_collision_test, det3d/core/sampler/preprocess.py:881-964).  The host draws the
 * database entries (augment.GTSampler); which of them are pasted is decided here, per sample, from the sample's own ground truth.
 * Purely additive: fd_abi_version() stays 8.  Graph-capturable, no atomics, no allocation, no workspace, no synchronisation.
 *
 * The database, in device memory: db_boxes [M, Tdb, 12] fp32 (16-byte aligned; an entry's box rows, timestep 0 first), db_steps [M]
 *   (valid timesteps of an entry, >= 1), db_class [M], db_traj [M] int32, db_point_offset [M + 1] int64 (entry e owns the rows
 *   [offset[e], offset[e + 1]) of db_points [P, ndim] fp32, object-centred).
 *
 * fd_gt_sample_select: one launch for the batch, one workgroup per sample.  boxes [B, T, n_max, 12] fp32, counts [B, T], classes and
 *   trajectory (or NULL) [B, T, n_max] int32 as for fd_gt_range_filter; cand [B, K] int32 holds the drawn entries, -1 = an empty slot;
 *   groups_host [G] in HOST memory (copied into the launch): group g owns the slots [first, first + n), the groups follow one another in
 *   slot order.  Per sample, with c_t = clamp(counts[b, t], 0, n_max):
 *   1. count_g = the objects i < c_0 of timestep 0 with classes == class_id and (trajectory < 0 or trajectory[b, 0, i] == trajectory);
 *      num_g = max(0, rint(rate * double(max_num - count_g))), round half to even (np.round).  The first num_g slots of the group that
 *      hold an entry TAKE PART.  A slot holds an entry when its index e lies in [0, M) and offset[e] <= offset[e + 1] <= P; any other
 *      value but -1 makes it an empty slot and sets FD_GT_SAMPLE_BAD_INDEX.
 *   2. BEV corners, in the form fd_gt_range_filter's text defines (every operation one fp32 operation): s = fl32(sin(double(a))),
 *      c = fl32(cos(double(a))); corner k has the offsets (-w/2, -l/2), (-w/2, +l/2), (+w/2, +l/2), (+w/2, -l/2);
 *      x_k = (ox c + oy s) + x, y_k = (-(ox s) + oy c) + y.  The angle a is column 11 for a slot among the slots of its own group (a
 *      CANDIDATE) and column 10 for a ground-truth row and for an accepted slot of an earlier group (an OBSTACLE): the reference reads
 *      gt_boxes[:, -2] for the one and [:, -1] for the other.  A stand-up box is the min / max of the four corners.
 *   3. collide(p, q) = box_collision_test(boxes = p, qboxes = q) for one pair, p always the candidate whose row is being judged:
 *      iw = min(p.xmax, q.xmax) - max(p.xmin, q.xmin) must be > 0, then ih likewise; then, for the edges AB of p (k = 0..3, B = corner
 *      k + 1 mod 4) and CD of q (l = 0..3): acd = (Dy - Ay)(Cx - Ax) > (Cy - Ay)(Dx - Ax), bcd likewise with B, and when they differ
 *      abc = (Cy - Ay)(Bx - Ax) > (By - Ay)(Cx - Ax), abd = (Dy - Ay)(Bx - Ax) > (By - Ay)(Dx - Ax); abc != abd is a collision.
 *      Otherwise containment: q lies inside p when for all corners Q of q and all k, with V = -(P_k - P_(k + 1 mod 4)),
 *      cross = V.y (P_k.x - Q.x), cross = cross - V.x (P_k.y - Q.y) is NOT >= 0; then p inside q the same way.  Either is a collision.
 *      (This is the function as numba compiles it; see DESIGN.md on `ret[i, j] is False`.)  A slot never collides with itself.
 *   4. The walk: group after group, slot after slot among those that take part.  The obstacles of a slot are the ground-truth rows
 *      i < c_0 of timestep 0, the ACCEPTED slots of earlier groups, and the slots of its own group that take part and have not been
 *      rejected (accepted ones and those still to come).  A slot that collides with an obstacle is rejected.  So is one that would
 *      not fit: max_t c_t + (accepted so far) >= n_max sets FD_GT_SAMPLE_NO_ROW, rows(e) > point_cap - (points accepted so far) sets
 *      FD_GT_SAMPLE_NO_POINTS (tested in this order, after the collision).  Every other slot is accepted.
 *   5. The r-th accepted slot (slot order), entry e, becomes row c_t + r of every timestep t: columns 0..5 of db_boxes[e, 0], columns
 *      6..11 of db_boxes[e, t < min(db_steps[e], Tdb) ? t : 0], classes = db_class[e], trajectory = db_traj[e]; counts_out[b, t] =
 *      c_t + accepted.  A sample with counts[b, t] != counts[b, 0] for some t sets FD_GT_SAMPLE_COUNTS_DIFFER.  Rows at or past the new
 *      counts are not written.  Either every output is its input (in place) or none overlaps an input; out of place the rows below c_t
 *      are copied.
 *   6. accepted [B, K] = 0 / 1; plan [B, K] (16-byte aligned): src_row = offset[e], rows = rows(e) for an accepted slot and 0, 0 for
 *      any other, dst_row = the rows of the accepted slots before it; n_points [B] = their total (<= point_cap); status [B] = the bits.
 *   FD_EINVAL for: B < 1, T outside [1, FD_GT_SAMPLE_MAX_T], n_max outside [1, FD_RANGE_FILTER_MAX_N], K outside [1, FD_GT_SAMPLE_MAX_K],
 *   G outside [1, FD_GT_SAMPLE_MAX_GROUPS], M or Tdb < 1, P < 0, point_cap outside [0, FD_AUGMENT_MAX_ROWS], a rate that is negative or
 *   not finite, group records that overlap, are out of slot order or run past K, a group with trajectory >= 0 while trajectory is
 *   NULL, null or misaligned pointers, partially overlapping or mixed in-place / out-of-place outputs.
 *
 * fd_gt_sample_points: one launch per cloud.  cand, accepted, plan: the sample's rows [K] of the arrays above.  Fills the rows
 *   [0, point_cap) of dst [>= point_cap, ndim], ndim 4 or 5: row dst_row + k of an accepted slot = db_points[src_row + k] with
 *   fl32(x + cx), fl32(y + cy), fl32(z + cz), (cx, cy, cz) = columns 0..2 of db_boxes[e, 0], the other columns bit for bit; every
 *   other row is the SENTINEL (FD_GT_SAMPLE_SENTINEL x 3, 0[, 0]): a point no voxeliser keeps under any shipped transform.  Rows at or
 *   past point_cap are not written.  A plan entry that does not lie inside db_points writes sentinels; nothing is read out of bounds.
 *   ndim 4 with 16-byte aligned db_points and dst moves a row as one 16-byte access; otherwise scalar accesses.
 *   FD_EINVAL for: ndim not 4 or 5, K out of range, M or Tdb < 1, P < 0, point_cap outside [0, FD_AUGMENT_MAX_ROWS], null or misaligned
 *   pointers (plan 8 bytes, the others 4), dst overlapping db_points.  point_cap = 0 is a no-op.
 * ------------------------------------------------------------------------------------------------- */
#define FD_GT_SAMPLE_MAX_K 64
#define FD_GT_SAMPLE_MAX_GROUPS 16
#define FD_GT_SAMPLE_MAX_T 64
#define FD_GT_SAMPLE_SENTINEL 1e30f
#define FD_GT_SAMPLE_NO_ROW 1
#define FD_GT_SAMPLE_NO_POINTS 2
#define FD_GT_SAMPLE_COUNTS_DIFFER 4
#define FD_GT_SAMPLE_BAD_INDEX 8
typedef struct fd_gt_sample_group {
    int32_t class_id, trajectory /* -1: any */, max_num, first, n;
} fd_gt_sample_group;
typedef struct fd_gt_sample_plan {
    int64_t src_row;
    int32_t rows, dst_row;
} fd_gt_sample_plan;
int fd_gt_sample_select(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory, const float *db_boxes,
                        const int32_t *db_steps, const int32_t *db_class, const int32_t *db_traj, const int64_t *db_point_offset, int M, int Tdb,
                        int64_t P, const int32_t *cand, const fd_gt_sample_group *groups_host, int G, double rate, int point_cap,
                        float *boxes_out, int32_t *counts_out, int32_t *classes_out, int32_t *trajectory_out, int32_t *accepted,
                        fd_gt_sample_plan *plan, int32_t *n_points, int32_t *status, int B, int T, int n_max, int K, fd_stream_t stream);
int fd_gt_sample_points(const float *db_points, int64_t P, int ndim, const float *db_boxes, int M, int Tdb, const int32_t *cand,
                        const int32_t *accepted, const fd_gt_sample_plan *plan, int K, float *dst, int point_cap, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: which points of a cloud lie inside which rotated 3-D boxes (fd_points_in_boxes.hip) -- box_np_ops.points_in_rbbox and
 * points_count_rbbox (det3d/core/bbox/box_np_ops.py:641-647, 15-20: center_to_corner_box3d -> corner_to_surfaces_3d ->
 * geometry.surface_equ_3d_jitv2 and points_in_convex_polygon_3d_jit, det3d/core/bbox/geometry.py:215-276, 352-378), what the reference's
 * ``min_points_in_gt`` filter (det3d/datasets/pipelines/preprocess.py:140-143) and its ground-truth database writer
 * (det3d/datasets/utils/create_gt_database.py:125-169) are built on.  Purely additive: fd_abi_version() stays 8.  Graph-capturable, no
 * atomics, no allocation, no synchronisation; every argument is checked on the host before any device work.
 *
 * The arithmetic.  Every operation below is one fp32 IEEE operation rounded on its own unless said otherwise.
 *   A box row has box_cols >= 7 columns: the centre = columns 0, 1, 2; (w, l, h) = columns 3, 4, 5; the angle a = the LAST column, as
 *     the reference reads it (rbbox[:, -1]: column 11 of our 12-column rows, not column 10); s = fl32(sin(double(a))),
 *     c = fl32(cos(double(a))) (the reference takes NumPy's fp32 sin / cos, which lie within 1.5 ulp of these).
 *   Corner k = 0..7 has the unit offsets (bx, by, bz) = (0,0,0), (0,0,1), (0,1,1), (0,1,0), (1,0,0), (1,0,1), (1,1,1), (1,1,0); with
 *     ox = w (bx - 0.5), oy = l (by - 0.5), oz = h (bz - 0.5):  x_k = (ox c + oy s) + cx,  y_k = (-(ox s) + oy c) + cy,  z_k = oz + cz.
 *   Face f = 0..5 uses the corners (P0, P1, P2) = (0,1,2), (7,6,5), (0,3,7), (1,5,6), (0,4,5), (3,2,6); with u = P0 - P1, v = P1 - P2:
 *     n = (u.y v.z - u.z v.y,  u.z v.x - u.x v.z,  u.x v.y - u.y v.x),  d = ((-(P0.x n.x)) - P0.y n.y) - P0.z n.z.
 *   A point p is INSIDE iff for all six faces ((p.x n.x + p.y n.y) + p.z n.z) + d is NOT >= 0: a point on a face is outside, a NaN
 *     counts as inside (as in the reference), a box whose three dimensions are zero holds no finite point (n = 0 and d = 0 on every
 *     face, and 0 >= 0).
 *
 * points [n, ndim] fp32, ndim 4 or 5; boxes [n_boxes_max, box_cols] fp32; n_boxes_dev: NULL, or one int32 in device memory -- the rows
 *   at or past nb = clamp(*n_boxes_dev, 0, n_boxes_max) are never read as boxes and hold no point.  workspace: device memory of
 *   fd_points_in_boxes_workspace_bytes(n, n_boxes_max) bytes, 4-byte aligned (0 bytes for invalid sizes).
 * fd_points_in_boxes_count: counts [n_boxes_max] int32 = the points inside each box.  Two launches: the partial counts of every
 *   (workgroup of 256 points, box) -- box planes in LDS, FD_POINTS_IN_BOXES_TILE boxes at a time whatever n_boxes_max is, one wave
 *   ballot + popcount per box -- then one pass that sums them per box and leaves their exclusive scan over the workgroups, and the
 *   totals, in the workspace.  n = 0 writes zeros; n_boxes_max = 0 is a no-op.
 * fd_points_in_boxes_extract: one more launch, on the SAME inputs and the workspace fd_points_in_boxes_count filled for them.
 *   offsets [n_boxes_max + 1] int64: offsets[j] = the points in the boxes before j, offsets[n_boxes_max] = the total.  rows
 *   [cap_rows, ncols_out] fp32, 1 <= ncols_out <= ndim: box after box, each box's points in their cloud order -- row offsets[j] + r is
 *   the r-th point of the cloud that lies inside box j, columns 0..2 minus the box centre (one fp32 subtraction each), the other
 *   columns copied bit for bit.  A point inside two boxes appears under both.  A row at or past cap_rows is not written and sets
 *   FD_POINTS_IN_BOXES_NO_ROOM in status[0] (0 otherwise); rows at or past the total are not written.  The order comes from the scan
 *   and ballot ranks: two runs write the same bytes.  With a workspace that was not filled for these inputs the result is undefined,
 *   but nothing is written outside rows [0, cap_rows).
 *   FD_EINVAL (both) for: ndim not 4 or 5, n outside [0, FD_AUGMENT_MAX_ROWS], n_boxes_max outside [0, FD_RANGE_FILTER_MAX_N],
 *   box_cols outside [7, FD_POINTS_IN_BOXES_MAX_COLS], a null (for a non-empty array) or misaligned pointer (offsets 8 bytes, the
 *   others 4), a workspace that is too small, outputs or workspace overlapping one another or an input; extract also: ncols_out outside
 *   [1, ndim], cap_rows outside [0, FD_AUGMENT_MAX_ROWS].
 *
 * fd_gt_min_points_filter (fd_augment_map.hip): fd_gt_range_filter with another mask -- the same arguments but the range, the same
 *   outputs, padding rule, in-place rule and status.  Object i < c0 of sample b is KEPT iff point_counts[b, i] >= min_points;
 *   point_counts [B, n_max] int32 in device memory (fd_points_in_boxes_count of the sample's cloud and its timestep-0 boxes) must not
 *   overlap an output.  FD_EINVAL as for fd_gt_range_filter (without the range), and for a null, misaligned or overlapping point_counts.
 * ------------------------------------------------------------------------------------------------- */
#define FD_POINTS_IN_BOXES_TILE 64
#define FD_POINTS_IN_BOXES_MAX_COLS 64
#define FD_POINTS_IN_BOXES_NO_ROOM 1
size_t fd_points_in_boxes_workspace_bytes(int64_t n_points, int n_boxes_max);
int fd_points_in_boxes_count(const float *points, int64_t n, int ndim, const float *boxes, int n_boxes_max, int box_cols,
                             const int32_t *n_boxes_dev, int32_t *counts, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_points_in_boxes_extract(const float *points, int64_t n, int ndim, const float *boxes, int n_boxes_max, int box_cols,
                               const int32_t *n_boxes_dev, const void *workspace, size_t workspace_bytes, float *rows, int64_t cap_rows,
                               int ncols_out, int64_t *offsets, int32_t *status, fd_stream_t stream);
int fd_gt_min_points_filter(const float *boxes, const int32_t *counts, const int32_t *classes, const int32_t *trajectory,
                            const int32_t *point_counts, int min_points, float *boxes_out, int32_t *counts_out, int32_t *classes_out,
                            int32_t *trajectory_out, int32_t *status, int B, int T, int n_max, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: CenterHead.loss for the standard and dense heads (fd_loss.hip) -- FastFocalLoss + RegLoss of
 * det3d/models/losses/centernet_loss.py as center_head.py:396-539 combines them, forward terms and the gradient of every head map.
 * Purely additive: fd_abi_version() stays 8.  fp32 maps, contiguous [B, channels, H, W].
 * Per task, x the raw heat map [B, C, H, W], sigma = sigmoid(x), s = clamp(sigma, 1e-4, 1 - 1e-4):
 *   neg = sum log(1 - s) s^2 (1 - target)^4 over the map;  pos = sum_{b,m} log(s[b, cat, ind]) (1 - s[b, cat, ind])^2 mask[b, m];
 *   num_pos = sum mask;  hm_loss = -(pos + neg) / num_pos, or -neg when num_pos == 0;
 *   regression term i, predicted channel c:  elem[i][c] = sum_{b,m} mask |p_c[b, ind] - t_i[b, m, col[c]]| / (num_pos + 1e-4), the
 *     divisor rounded to fp32 (RegLoss casts the mask to float, whatever the dtype of the maps);
 *   loc_loss[i] = sum_c elem[i][c] cw_i[c];  loss = hm_loss + weight sum_i loc_loss[i].
 * The predicted channels are reg(2), height(1), dim(3), vel(2)[, rvel(2)], rot(2)[, rrot(2)]: D = 8 (no vel), 10 or 14 of them;
 * col[c] is the column of a target row (row_stride floats) that channel c is compared with.
 *   standard head (dense = 0): one focal term on the targets of step 0 and T regression terms, all on ind / mask[0] of step 0; term i
 *     reads anno_box[i] and velocity channels 2i, 2i + 1 (vel / rvel have 2T channels); cw_0 = code_weights, cw_{i>0} =
 *     code_weights_forecast; num_positive = sum_i sum mask[i].  S = T terms.
 *   dense head (dense = 1): task k is given the targets of its own step as mask[0] / anno_box[0]; one term with code_weights (vel /
 *     rvel have 2 channels); num_positive = num_pos.  S = 1; T is ignored.
 * mask holds 0 or 1 (any non-zero byte counts as 1).  An entry with mask == 0 contributes nothing and its ind / cat are never used;
 * an entry with mask != 0 whose ind is outside [0, H W) or whose cat is outside [0, C) contributes nothing to pos / elem / the
 * gradients and is counted in the status word (torch's gather would device-assert).  Objects that share a cell add their
 * gradients in object order.
 *
 * fd_centerhead_loss_forward writes sig (the clamped sigmoid of every task's heat map) and the terms vector, fp32, per task
 *   loss, hm_loss, num_pos, num_positive, loc_loss[S], loc_loss_elem[S][D]
 * followed by ONE status word (the number of out-of-range entries over all tasks, as a float):
 * fd_centerhead_loss_terms(cfg) = n_tasks (4 + S + S D) + 1 floats.
 * fd_centerhead_loss_backward reads the same maps and targets, the terms vector of the forward call (num_pos) and go[n_tasks] (the
 * upstream gradient of every task's loss, DEVICE memory) and writes d_hm / d_maps: every element exactly once, zeros where no
 * object sits; a NULL output pointer skips that map.  Gradients of the clamped cells are exactly 0 (clamp's backward).
 * Sums run in double in a fixed order (chunks of fd_loss_chunk() elements, samples in order, objects in order): no atomics, the same
 * bits on every run.  Launches: 2 per call for up to 8 tasks, 3 for 9 to 16.  Descriptors travel as launch arguments: no
 * allocation, no copy, no synchronisation; nothing is cached between calls.
 * workspace >= fd_centerhead_loss_workspace_bytes(cfg, largest C of the tasks) (0 = invalid sizes), 16-byte aligned; the backward
 * does not need the forward's contents.  Both entry points validate on the host before any device work; FD_EINVAL for: a null cfg /
 * tasks / terms / go / workspace or a null member that the mode needs; B, H, W, M or a task's C <= 0; n_tasks outside [1, 16]; T
 * outside [1, 7] (standard); D not 8, 10 or 14; M above FD_LOSS_MAX_OBJS; a column outside the target row; a map of 2^31 elements or
 * more; a workspace that is too small.
 * ------------------------------------------------------------------------------------------------- */
#define FD_LOSS_CHUNK 2048
#define FD_LOSS_MAX_TASKS 16
#define FD_LOSS_MAX_STEPS 7
#define FD_LOSS_MAX_OBJS 2048
typedef struct fd_loss_cfg {
    int32_t B;
    int32_t H;
    int32_t W;
    int32_t M;
    int32_t n_tasks;
    int32_t dense;
    int32_t T;
    int32_t D;
    int32_t row_stride;
    int32_t col[14];
    double code_weights[14];
    double code_weights_forecast[14];
    double weight;
} fd_loss_cfg;
typedef struct fd_loss_task {
    const float *hm;        /* raw heat map [B, C, H, W] */
    const float *hm_target; /* [B, C, H, W] */
    const int64_t *ind;     /* [B, M] */
    const int64_t *cat;     /* [B, M] */
    const void *mask[7];    /* uint8 [B, M] per step (standard: T of them; dense: [0]) */
    const float *maps[7];   /* reg, height, dim, vel, rvel, rot, rrot; NULL where D has no such channels */
    const float *anno_box[7]; /* fp32 [B, M, row_stride] per term */
    int32_t C;
    float *sig;             /* forward: clamped sigmoid [B, C, H, W] */
    float *d_hm;            /* backward outputs (NULL: skipped) */
    float *d_maps[7];
} fd_loss_task;
int fd_loss_chunk(void);
size_t fd_centerhead_loss_terms(const fd_loss_cfg *cfg);
size_t fd_centerhead_loss_workspace_bytes(const fd_loss_cfg *cfg, int max_classes);
int fd_centerhead_loss_forward(const fd_loss_cfg *cfg, const fd_loss_task *tasks, float *terms, void *workspace, size_t workspace_bytes,
                               fd_stream_t stream);
int fd_centerhead_loss_backward(const fd_loss_cfg *cfg, const fd_loss_task *tasks, const float *terms, const float *go, void *workspace,
                                size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: BatchNorm1d on batch statistics over the rows of a sparse feature matrix, fused with the ReLU and the residual add that
 * follow it in SpMiddleResNetFHD (fd_sparse_bn.hip; the kernels are those of fd_row_bn.h).  Purely additive: fd_abi_version() stays 8.
 * fp32, row-major contiguous x [n, C]; C a multiple of 16 in [16, 128]; relu 0 or 1; residual [n, C] or NULL.
 * The _bf16 entry points take bf16 rows (the bits, as uint16_t) for x, residual, y, dy, dx and d_residual; gamma, beta, saved, the
 * running statistics, dgamma, dbeta and the workspace stay fp32 (one workspace size serves both).  A row is widened exactly on load
 * and rounded to nearest even on store: the bf16 form computes what the fp32 form computes on the widened rows, rounded once.  The
 * ReLU mask is y > 0 on the bf16 y; d_residual is the masked dy, copied.
 *   forward:  y = act(gamma (x - mean) invstd + beta [+ residual]);  mean and the biased variance over the valid rows,
 *             invstd = 1 / sqrt(var + eps);  saved = [mean[C], invstd[C]] fp32 for the backward;
 *             running_mean <- (1 - momentum) running_mean + momentum mean, running_var the same with the unbiased variance
 *             var n / (n - 1), num_batches_tracked (int64) += 1 -- all on the device.
 *   backward: g = dy where y > 0 (relu = 1; y is the forward's output) or dy;  dbeta = sum g;  dgamma = sum g x^,
 *             x^ = (x - mean) invstd;  dx = gamma invstd (g - dbeta / n - x^ dgamma / n);  d_residual = g (NULL: skipped).
 * Sums: rows are cut into chunks of fd_sparse_bn_chunk() (= FD_SPARSE_BN_CHUNK) rows; a chunk's partial is centred at the chunk's own
 * mean; partials are combined in double, in a fixed order, with Chan's rule.  No atomics: the same bits on every run.
 * n_dev (may be NULL): the valid row count in device memory; n is then the capacity, the statistics use min(n, max(*n_dev, 0)) rows, and
 * the rows at or beyond it are written as zeros in y, dx and d_residual and never read.  A device count of 0 leaves the running
 * statistics and num_batches_tracked as they are; a device count of 1 gives a variance of 0 (torch raises; a kernel cannot).
 * Two launches per call; no allocation, no synchronisation.  workspace >= fd_sparse_bn_workspace_bytes(n, C) (0 = invalid sizes),
 * 16-byte aligned like every tensor; the backward does not need the forward's contents.
 * Both entry points validate on the host before any device work; FD_EINVAL for: a null pointer (other than residual, n_dev,
 * d_residual, and y when relu = 0), an unsupported C, n outside [1, 2^30], n < 2 without n_dev, relu not 0 or 1, eps <= 0, momentum
 * outside [0, 1], a misaligned tensor, a workspace that is too small.
 * ------------------------------------------------------------------------------------------------- */
#define FD_SPARSE_BN_CHUNK 256
int fd_sparse_bn_chunk(void);
size_t fd_sparse_bn_workspace_bytes(int64_t n, int C);
int fd_sparse_bn_train_forward(const float *x, const float *residual, const float *gamma, const float *beta, int64_t n, const int32_t *n_dev,
                               int C, int relu, float eps, double momentum, float *y, float *saved, float *running_mean, float *running_var,
                               int64_t *num_batches_tracked, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_sparse_bn_train_backward(const float *dy, const float *x, const float *y, const float *gamma, const float *saved, int64_t n,
                                const int32_t *n_dev, int C, int relu, float *dx, float *d_residual, float *dgamma, float *dbeta,
                                void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_sparse_bn_train_forward_bf16(const uint16_t *x, const uint16_t *residual, const float *gamma, const float *beta, int64_t n,
                                    const int32_t *n_dev, int C, int relu, float eps, double momentum, uint16_t *y, float *saved,
                                    float *running_mean, float *running_var, int64_t *num_batches_tracked, void *workspace,
                                    size_t workspace_bytes, fd_stream_t stream);
int fd_sparse_bn_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *gamma, const float *saved,
                                     int64_t n, const int32_t *n_dev, int C, int relu, uint16_t *dx, uint16_t *d_residual, float *dgamma,
                                     float *dbeta, void *workspace, size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Training: BatchNorm2d on batch statistics over the maps of the dense half (RPN, CenterHead), fused with the ReLU that follows it
 * (fd_dense_bn.hip).  Purely additive: fd_abi_version() stays 8.
 * fp32, NCHW contiguous x [B, C, H, W], passed as (B, C, P = H W); N = B P values per channel.  C in [1, 4096] (no multiple-of-16
 * rule: the channel is not the vectorised axis), B in [1, 2^16], P in [1, 2^30], B C <= 2^24, B ceil(P / chunk) <= 2^29, N >= 2;
 * relu 0 or 1.  Element offsets are 64-bit.  No residual input, no bf16 form.
 *   forward:  y = act(gamma[c] (x - mean[c]) invstd[c] + beta[c]);  saved [2, C] = (mean, invstd) for the backward;
 *             running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with the unbiased variance
 *             var N / (N - 1), num_batches_tracked (int64) += 1 -- all on the device.
 *   backward: g = dy where y > 0 (relu = 1; y is the forward's output) or dy;  dbeta = sum g;  dgamma = sum g x^,
 *             x^ = (x - mean) invstd;  dx = gamma invstd (g - dbeta / N - x^ dgamma / N).
 * Sums: every plane (b, c) is cut into chunks of fd_dense_bn_chunk() (= FD_DENSE_BN_CHUNK) elements; a channel's chunks, ordered by
 * (b, piece), form groups of consecutive chunks; a chunk's partial is centred at the chunk's own mean; partials are combined in double,
 * in a fixed order, with Chan's rule.  No atomics, and every boundary follows from (B, C, P): the same bits on every run.
 * P % 4 == 0: all traffic is 16-byte loads and stores; any other P runs element by element (plane starts are then unaligned).
 * Two launches per call; no allocation, no synchronisation.  workspace >= fd_dense_bn_workspace_bytes(B, C, P) (0 = unsupported
 * sizes), 16-byte aligned; the backward does not need the forward's contents.
 * Both entry points validate on the host before any device work; FD_EINVAL for: a null pointer (other than y when relu = 0), C, B or P
 * out of range, B P < 2, relu not 0 or 1, eps <= 0, momentum outside [0, 1], a workspace that is null, too small or misaligned,
 * x, y, dy or dx not 16-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
#define FD_DENSE_BN_CHUNK 2048
int fd_dense_bn_chunk(void);
size_t fd_dense_bn_workspace_bytes(int64_t B, int C, int64_t P);
int fd_dense_bn_train_forward(const float *x, const float *gamma, const float *beta, int64_t B, int C, int64_t P, int relu, float eps,
                              double momentum, float *y, float *saved, float *running_mean, float *running_var,
                              int64_t *num_batches_tracked, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_dense_bn_train_backward(const float *dy, const float *x, const float *y, const float *gamma, const float *saved, int64_t B, int C,
                               int64_t P, int relu, float *dx, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                               fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mixed-precision training: BatchNorm2d on batch statistics over a bf16 channels-last map of the dense half, fused with the ReLU that
 * follows it (fd_dense_bn_nhwc.hip; the kernels are those of fd_row_bn.h).  Purely additive: fd_abi_version() stays 8.
 * The map is rows x [n = B H W, C], bf16 (the bits, as uint16_t), row-major contiguous; C a multiple of 32 in [32, 512]; n in [2, 2^30];
 * relu 0 or 1.  y, dy and dx are bf16 rows like x: a row is widened exactly on load and rounded once, to nearest even (a NaN stays a NaN),
 * on store.  saved [2, C], dgamma [C], dbeta [C], the parameters, the running statistics and the workspace are fp32.
 * One call serves the channel ranges of up to FD_DENSE_BN_NHWC_MAX_GROUPS BatchNorm2d modules: record j of `groups`
 * (fd_dense_bn_nhwc_group, read on the host and passed to the kernels by value) owns the next c channels -- c a multiple of 32, the c
 * of all records summing to C -- with its own gamma [c], beta [c], eps, momentum, running_mean [c], running_var [c] and counter.
 *   forward:  y = act(gamma (x - mean) invstd + beta);  mean and the biased variance over the n rows, invstd = 1 / sqrt(var + eps) with
 *             the record's eps;  saved = [mean[C], invstd[C]];  per record running_mean <- (1 - momentum) running_mean + momentum mean,
 *             running_var the same with the unbiased variance var n / (n - 1), num_batches_tracked (int64) += 1 -- all on the device.
 *   backward: g = dy where y > 0 (relu = 1; y is the forward's output) or dy;  dbeta = sum g;  dgamma = sum g x^,
 *             x^ = (x - mean) invstd;  dx = gamma invstd (g - dbeta / n - x^ dgamma / n).  Reads only gamma of a record.
 * Sums: the design of fd_row_bn.h, shared with fd_sparse_bn_*.  Rows are cut into chunks of fd_dense_bn_nhwc_chunk() (= FD_DENSE_BN_NHWC_CHUNK) rows;
 * consecutive chunks form at most fd_dense_bn_nhwc_stat_groups() groups; a chunk's partial is centred at the chunk's own mean; partials are
 * combined in double, in a fixed order, with Chan's rule.  The element-wise passes cut the rows into at most
 * fd_dense_bn_nhwc_apply_blocks() blocks of whole chunks.  No atomics, and every boundary follows from (n, C): the same bits on every run.
 * Two launches per call; no allocation, no synchronisation.  workspace >= fd_dense_bn_nhwc_workspace_bytes(n, C) (0 = unsupported
 * sizes), 16-byte aligned; it need not be initialised and the backward does not need the forward's contents.
 * Both entry points validate on the host before any device work; FD_EINVAL for: a null pointer (other than y when relu = 0, and in the
 * backward every member of a record but gamma), C or a record's c out of range or no multiple of 32, c not summing to C, n_groups
 * outside [1, FD_DENSE_BN_NHWC_MAX_GROUPS], n outside [2, 2^30], relu not 0 or 1, (forward) a record's eps <= 0 or momentum outside
 * [0, 1], a workspace that is null, too small or misaligned, x, y, dy, dx or saved not 16-byte aligned.
 * ------------------------------------------------------------------------------------------------- */
#define FD_DENSE_BN_NHWC_CHUNK 256
#define FD_DENSE_BN_NHWC_MAX_GROUPS 8
#define FD_DENSE_BN_NHWC_STAT_GROUPS 256
#define FD_DENSE_BN_NHWC_APPLY_BLOCKS 512
typedef struct fd_dense_bn_nhwc_group {
    const float *gamma, *beta;
    float *running_mean, *running_var;
    int64_t *num_batches_tracked;
    int c;
    float eps;
    double momentum;
} fd_dense_bn_nhwc_group;
int fd_dense_bn_nhwc_chunk(void);
int fd_dense_bn_nhwc_stat_groups(void);
int fd_dense_bn_nhwc_apply_blocks(void);
size_t fd_dense_bn_nhwc_workspace_bytes(int64_t n, int C);
int fd_dense_bn_nhwc_train_forward_bf16(const uint16_t *x, const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu,
                                        uint16_t *y, float *saved, void *workspace, size_t workspace_bytes, fd_stream_t stream);
int fd_dense_bn_nhwc_train_backward_bf16(const uint16_t *dy, const uint16_t *x, const uint16_t *y, const float *saved,
                                         const fd_dense_bn_nhwc_group *groups, int n_groups, int64_t n, int C, int relu, uint16_t *dx,
                                         float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, fd_stream_t stream);

/* ---------------------------------------------------------------------------------------------------
 * Mixed-precision training of the dense convolutions that change resolution (fd_conv2d_strided_grad_bf16.hip; the weight gradients
 * are instantiations of fd_conv2d_wgrad_bf16's kernel in fd_conv2d_grad_bf16.hip).  Purely additive: fd_abi_version() stays 8.
 * They replace the fp32 torch convolutions, forward and backward, of det3d/models/necks/rpn.py:124-128 (ZeroPad2d(1) + Conv2d(3,
 * stride 2): the opener of a down-sampling stage), rpn.py:82-86 (the ConvTranspose2d(k = stride = 2) deblock) and rpn.py:96-102 (the
 * Conv2d(k = stride = 2) deblock of us_layer_strides 0.5).  All maps are bf16 NHWC, all channel counts multiples of 32, sums are fp32
 * on the matrix core, a bf16 result is rounded once (to nearest even); no atomics, no allocation, no synchronisation.
 *
 * 3 x 3 / stride 2 / padding 1, x [B,H,W,cin] -> y [B,Ho,Wo,cout], Ho = (H - 1) / 2 + 1 (H and W even or odd).  The forward is
 * fd_conv2d_nhwc_bf16 with stride 2.
 *   fd_conv2d_s2_dgrad_bf16: dx[b,iy,ix,ci] = sum over (ky, kx, co) of dy[b,(iy+1-ky)/2,(ix+1-kx)/2,co] w[co][ci][ky][kx] over the taps
 *                     whose quotients are integers inside Ho x Wo.  wpacked_t: the mode-1 pack of fd_conv2d_pack_weight_dev (ks 3).
 *                     Every element of dx is written.
 *   fd_conv2d_wgrad_s2_bf16: dw[co][ci][ky][kx] = sum over (b, oy, ox) of dy[b,oy,ox,co] x[b,2oy+ky-1,2ox+kx-1,ci] (in-image terms), fp32,
 *                     overwritten.  fd_conv2d_wgrad_bf16's design over the pixels of dy: chunks of fd_conv2d_wgrad_bf16_chunk(), one
 *                     fp32 partial per (chunk, tap) in `workspace` (fd_conv2d_wgrad_s2_bf16_workspace_bytes; 0 = bad arguments), summed in
 *                     chunk order: the same bits on every run; the workspace need not be initialised.
 *
 * The 2 x 2 / stride 2 pair between a fine map [B,H,W,c_fine] and a coarse map [B,H/2,W/2,c_coarse] (the trailing row or column of an
 * odd H or W is not read), with W(a, f, dy, dx) the parameter at coarse-side channel a and fine-side channel f -- both nn.Conv2d(2, 2)
 * ([cout = coarse][cin = fine][2][2]) and nn.ConvTranspose2d(2, 2) ([cin = coarse][cout = fine][2][2]) store [c_coarse][c_fine][2][2];
 * fine_major = 1 reads or writes the other order, [c_fine][c_coarse][2][2]:
 *   "up2":   fine[b,2y+dy,2x+dx,f] = sum over a of coarse[b,y,x,a] W(a,f,dy,dx) -- the forward of ConvTranspose2d(2, 2), the input
 *            gradient of Conv2d(2, 2): four fd_conv2d_nhwc_bf16 launches (ks 1, osy = osx = 2, ooy = dy, oox = dx), tap 2 dy + dx with
 *            the pack at offset (2 dy + dx) fd_conv2d_packed_weight_bytes(c_fine, c_coarse, 1) of the kind-0 pack below.
 *   fd_conv2d_down2_bf16: "down2", coarse[b,y,x,a] = sum over (dy, dx, f) of fine[b,2y+dy,2x+dx,f] W(a,f,dy,dx) -- the forward of
 *            Conv2d(2, 2), the input gradient of ConvTranspose2d(2, 2); wpacked: the kind-1 pack below.
 *   fd_conv2d_pack_weight_2x2_dev: w fp32 DEVICE memory -> kind 0: the four up2 packs, back to back, each byte for byte
 *            fd_conv2d_pack_weight of the [c_fine][c_coarse][1][1] weight W(., ., dy, dx) transposed (c_coarse % 32 == 0, c_fine padded
 *            to 32); kind 1: fd_conv2d_pack_weight of the [c_coarse][4 c_fine][1][1] weight with input channel (2 dy + dx) c_fine + f
 *            (c_fine % 32 == 0, c_coarse padded to 32).  fd_conv2d_packed_weight_2x2_bytes: the size (0 = bad arguments).  One launch.
 *   fd_conv2d_wgrad_2x2_bf16: dw(a,f,dy,dx) = sum over coarse pixels of coarse[b,y,x,a] fine[b,2y+dy,2x+dx,f], fp32, overwritten, in
 *            the layout fine_major selects; chunks of coarse pixels, partials and reduction as above
 *            (fd_conv2d_wgrad_2x2_bf16_workspace_bytes; H and W are the fine map's).
 * ------------------------------------------------------------------------------------------------- */
int fd_conv2d_s2_dgrad_bf16(const void *dy, int B, int H, int W, int cin, int cout, const void *wpacked_t, void *dx, fd_stream_t stream);
size_t fd_conv2d_wgrad_s2_bf16_workspace_bytes(int B, int H, int W, int cin, int cout);
int fd_conv2d_wgrad_s2_bf16(const void *x, const void *dy, int B, int H, int W, int cin, int cout, void *workspace, size_t workspace_bytes,
                            float *dw, fd_stream_t stream);
int fd_conv2d_down2_bf16(const void *x, int B, int H, int W, int c_fine, const void *wpacked, int c_coarse, void *y, fd_stream_t stream);
size_t fd_conv2d_packed_weight_2x2_bytes(int c_coarse, int c_fine, int kind);
int fd_conv2d_pack_weight_2x2_dev(const float *w, int c_coarse, int c_fine, int kind, int fine_major, void *wpacked, fd_stream_t stream);
size_t fd_conv2d_wgrad_2x2_bf16_workspace_bytes(int B, int H, int W, int c_coarse, int c_fine);
int fd_conv2d_wgrad_2x2_bf16(const void *coarse, const void *fine, int B, int H, int W, int c_coarse, int c_fine, int fine_major,
                             void *workspace, size_t workspace_bytes, float *dw, fd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FUTUREDET_HIP_H */
