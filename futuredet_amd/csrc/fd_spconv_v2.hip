// fp32 sparse convolution, second formulation: tile-level pair compaction.
//
// fp32 MFMA (v_mfma_f32_16x16x4_f32) runs at the fp32 vector rate, so the fp32 layers are MFMA-bound and
// every zero row fed to the matrix core is lost time.  With 27 taps only 18-63 % of the (output row, tap)
// pairs exist, and a 16-row output group almost never lacks a tap entirely, so the register-resident
// output-stationary kernel (fd_spconv.hip) spends 40-80 % of its MFMAs on zeros.  This kernel removes them:
//
//   * a workgroup owns one RANGE of consecutive output rows (spatially sorted, so their inputs are close) and walks it
//     in chunks of at most TM = 128 rows.  Ranges are either equal row counts or, for rulebooks shared by several
//     convolutions, equal WORK (fd_spconv_ranges: MFMA groups per 32-row block, prefix sum, quantiles), and there is a
//     whole number of them per compute unit: no tail round, no heavy / light tile lottery, and -- unlike a work-sorted
//     tile permutation -- neighbouring workgroups still gather neighbouring input rows.  While a chunk's MFMAs run,
//     the next chunk's rulebook slice is already on its way into registers;
//   * the rulebook tile [K][TM] is staged in LDS and compacted IN PLACE per tap with wave ballots /
//     prefix popcounts into lists of (input row << 8 | local output row) entries, tails filled with -1 --
//     the "LDS-staged rulebook tile";
//   * accumulators for the whole chunk live in LDS ([TM + 1][COUT] fp32, 64 KB at COUT = 128; row TM is a
//     scratch row that absorbs the padding lanes so the accumulator traffic needs no exec masking).  The MFMA is
//     issued TRANSPOSED (A operand = weight fragment, B operand = gathered rows): lane (pair j, quad q) then holds four
//     consecutive output channels of pair j's row, so one 16-byte LDS read and one 16-byte write per 16-column block
//     move the accumulators (the untransposed layout needs four 4-byte accesses each way and four row addresses);
//     16-byte slots are XOR-swizzled by the row so the 16 rows of a lane group land on distinct banks;
//   * each wave owns a column slice of the tile (and, for narrow COUT, a row subset) and walks a flattened
//     work list of (tap, 16-pair group) items: gather the 16 input rows straight into MFMA A-fragment layout
//     (one 16-byte bounds-checked buffer load per lane and 16-channel chunk, prefetched DEPTH items ahead with
//     exact vmcnt accounting), read the 16 accumulator rows from LDS as the MFMA C operand, run the
//     CIN/4 x NBW MFMAs, write D back.  The wave's slice of W[tap] stays in registers for the whole tap
//     (double buffered one tap ahead when it is small).  A wave never shares an accumulator element with another
//     wave: no atomics, no barriers in the main loop, fixed summation order (taps ascending) -> deterministic.
//   * epilogue: bias (+ residual) (+ ReLU) on the LDS tile, written out with 16-byte row-contiguous stores.
//
// What happens per chunk around the item loop -- LDS layout, list-entry encoding, accumulator swizzle, range / chunk resolution,
// slice prefetch and staging, tile init, compaction, work list, epilogue -- is shared with the 32-pair kernel (fd_spconv_c32.hip)
// and lives in fd_spconv_chunk.h.  This file owns the 16-pair unit of work (wave -> column slice / tap split / row set mapping,
// gather, weight slice in registers and its in-place reload, the 16x16x4 MFMA loop with its scheduling barriers), its dispatch
// table, the phase trace (FD_V2_TRACE), the work-balanced ranges and the chunk plan of a shared rulebook (chunk_plan_kernel), and the
// kernels that make plan and block works straight from the sparse index, without the table (index_plan_kernel, index_work_kernel).
#include "fd_spconv_chunk.h"

namespace {

namespace sk = fd::skeleton;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Phase timeline for tuning builds only (tools/probes/build_trace.sh compiles this file with -DFD_V2_TRACE into a
// separate library; the product library contains none of it): thread 0 of every workgroup stamps s_memtime at the
// phase boundaries of its first chunk.
#ifdef FD_V2_TRACE
__device__ unsigned long long *g_trace;
#define FD_T(i)                                                                                  \
    do {                                                                                         \
        if (threadIdx.x == 0 && g_trace) g_trace[(size_t)blockIdx.x * 16 + (i)] = __builtin_readcyclecounter(); \
    } while (0)
#define FD_TV(i, v)                                                                    \
    do {                                                                               \
        if (threadIdx.x == 0 && g_trace) g_trace[(size_t)blockIdx.x * 16 + (i)] = (v); \
    } while (0)
#else
#define FD_T(i)
#define FD_TV(i, v)
#endif


// tap splits of a COUT-column tile (the kernel's TS; the host sizes the LDS request with it).  32 / 64 columns: instead of two row
// halves (whose separately compacted lists pad 17 % more MFMA rows) the two waves of a column slice split the TAPS (even / odd)
// over the full tile and accumulate into private copies of the tile that the epilogue adds up; the LDS for the second copy is
// there anyway (these layers run two workgroups per CU).  16 columns keep four row quarters: measured faster.
constexpr int tap_splits(int cout) { return (cout == 32 || cout == 64) ? 2 : 1; }

// PLAN: nbr / nbr_stride are a chunk plan (fd_spconv_chunk.h) instead of the rulebook: the lists arrive compacted
// SWZ: the input rows are stored bank-spread (fd_spconv_chunk.h); `relu` carries skeleton::kernel_flags
template <int CIN, int COUT, int TM, int DEPTH, bool PLAN, bool SWZ>
__global__ void __launch_bounds__(256) spconv_f32_compact(const float *__restrict__ in, const float4 *__restrict__ wp,
                                                          const float *__restrict__ bias, const float *__restrict__ residual, int relu,
                                                          const int *__restrict__ nbr, int64_t nbr_stride, int K, int n_out,
                                                          const int *__restrict__ n_out_dev, float *__restrict__ out, unsigned in_bytes,
                                                          const int *__restrict__ ranges, int rows_per_range) {
    constexpr int NB = COUT / 16, NC = CIN / 16;
    constexpr int WC = NB == 8 ? 4 : (NB >= 2 ? 2 : 1);  // column splits across the 4 waves (64 columns: 2 x 32)
    constexpr int NBW = NB / WC;          // 16-column blocks per wave
    constexpr int TS = tap_splits(COUT);
    constexpr int WR = 4 / (WC * TS);             // row splits
    constexpr int NACC = NBW;  // one accumulator chain per column block (dependent 16x16x4 MFMAs issue back to back at full rate)
    static_assert((TM == 128 || TM == 64) && TM / WR >= 16, "local row uses 8 bits (0..TM, TM = scratch row)");
    static_assert(!PLAN || (TM == sk::kPlanTM && WR == 1), "the chunk plan holds the lists of 128-row chunks with one row set");
    static_assert(!SWZ || CIN >= 32, "rows of fewer than 128 bytes are never bank-spread");
    constexpr int kPad = sk::pad_entry(TM);
    constexpr sk::Layout L = sk::layout(TM, COUT, TS, 16);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *s_list = reinterpret_cast<int *>(smem + L.list);
    unsigned short *s_items = reinterpret_cast<unsigned short *>(smem + L.items);
    unsigned char *s_cnt = smem + L.cnt;
    int *s_pad = reinterpret_cast<int *>(smem + L.pad);
    float *s_acc = reinterpret_cast<float *>(smem + L.acc);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: what derives from it stays in SGPRs
    int r_begin, r_end, n_chunks, chunk_rows;
    sk::resolve_range(n_out, n_out_dev, ranges, rows_per_range, r_begin, r_end);
    if (r_begin >= r_end) return;
    FD_T(0);
    sk::cut_chunks<TM>(r_begin, r_end, n_chunks, chunk_rows);
    int pre[sk::kSliceRegs<TM>];
    const int k_fetch = PLAN ? sk::kPlanRows : K;
    sk::fetch_slice<TM>(pre, nbr, nbr_stride, k_fetch, r_begin);

    const int lrow = lane & 15, lq = lane >> 4;
    const int wc = wave % WC, wr = TS == 1 ? wave / WC : 0, ts = TS == 1 ? 0 : wave / WC;
    const int cb = wc * NBW * 16;
    unsigned char *acc_bytes = reinterpret_cast<unsigned char *>(s_acc + ts * L.acc_copy);  // this wave's tile copy
    const unsigned slot0 = (unsigned)(cb >> 2) + (unsigned)lq;  // 16-byte slot of this lane's 4 channels in block nw = 0
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)in_bytes, 0x00020000);
    constexpr int kTapBytes = NC * NB * 64 * 16;  // packed weights: [K][NC][NB][64 lanes] float4
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(wp), 0, K * kTapBytes, 0x00020000);
    const unsigned w_lane = (unsigned)(lane * 16 + wc * NBW * 64 * 16);
    unsigned short *items = s_items + wave * L.item_slot;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
    int row0, n_rows;
    if (!sk::chunk_span(r_begin, r_end, chunk_rows, chunk, row0, n_rows)) break;
    if constexpr (PLAN) {
        sk::stage_plan_chunk<TM, COUT, TS, 16>(pre, s_list, s_cnt, s_pad, s_acc, bias, residual, relu, row0, n_rows);
    } else {
        sk::stage_chunk<TM, COUT, TS, 16>(pre, s_list, s_pad, s_acc, bias, residual, relu, K, row0, n_rows);
        __syncthreads();
        if (chunk == 0) FD_T(1);
        sk::compact_taps<TM, WR>(s_list, s_cnt, K);
    }
    __syncthreads();
    if (chunk == 0) FD_T(2);
    // the next chunk's slice travels while this chunk computes
    if (chunk + 1 < n_chunks) sk::fetch_slice<TM>(pre, nbr, nbr_stride, k_fetch, row0 + chunk_rows);
    const int n_items = sk::build_items<TS, 16>(s_cnt, items, K, ts, wr);

    // ring of DEPTH prefetched items.  Gathers are buffer loads with hardware bounds checking: a padding lane / a
    // slot past the end of the work list gets an out-of-range offset and reads zeros, so prefetch AND compute are
    // branch-free (exec-masked loads forced vmcnt(0), i.e. no overlap at all; branches around the MFMAs kept the
    // compiler from interleaving the bookkeeping VALU/LDS work with them).
    int k_r[DEPTH];
    int row_r[DEPTH];  // list entry of pair `lrow` of the item: input row << 8 | local output row
    u32x4 a_r[DEPTH][NC];
    // Bookkeeping is kept off the vector ALU (it competes with the MFMAs for issue slots): the item code is
    // wave-uniform (scalar registers), and a list entry needs no compare/select -- the padding entry kPad has all
    // high bits set, so its byte offset lands beyond the buffer (hardware returns zeros) and its row field is the
    // scratch row TM.
    // Bookkeeping is software pipelined so that no LDS round trip sits between two MFMA blocks of a wave (in-order
    // issue: a dependent ds_read chain costs ~1.3k cycles per item under load, as much as the gather itself):
    //   stage A0 (item i+DEPTH+1): read the item code          -> consumed one iteration later
    //   stage A1 (item i+DEPTH)  : read its 16 list entries     -> consumed one iteration later
    //   stage B  (item i+DEPTH-1): issue its gather (buffer loads; a padding entry / a slot past the end of the work list
    //                              has an out-of-range offset: the hardware returns zeros, no branch, no exec mask)
    //   item i                   : request the old accumulator values, run the MFMAs from a zero accumulator, then add
    //                              and write back -- nothing waits in front of the MFMAs.  (LDS float atomics would
    //                              drop the read altogether but ds_add_f32 measured 2-4x slower for the whole kernel.)
    // A wave owns its accumulator elements and LDS operations of a wave execute in order, so the sums are formed in a
    // fixed order (taps ascending): deterministic.
    auto stage_a0 = [&](int it) -> int { return sk::stage_a0(items, n_items, it); };
    auto stage_a1 = [&](int it, int code_v, int &kk, int &e) { sk::stage_a1<TM, WR, 16>(s_list, s_pad, n_items, wr, lrow, it, code_v, kk, e); };
    // bank-spread rows: the lane's piece of 16-channel chunk c is lq + 4 (c & 1) of line c / 2, stored at piece ^ (row & 7).  The
    // row's bits go into the offset once per item; the odd chunks read from that offset ^ 64 (one XOR per item, which the compiler
    // shares between them), and the line stays an immediate
    auto gather_offset = [&](int e) -> unsigned {
        const unsigned o = sk::entry_row_bytes<CIN>(e) + (unsigned)(lq * 16);
        return SWZ ? o ^ sk::entry_swz_bits(e) : o;
    };
    auto gather_chunk = [&](unsigned voff, int c) {
        return SWZ ? __builtin_amdgcn_raw_buffer_load_b128(rsrc, (voff ^ (unsigned)((c & 1) * 64)) + (c >> 1) * 128, 0, 0)
                   : __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + c * 64, 0, 0);
    };
    // weight fragments through a buffer resource: the lane's part of the address is set once (w_lane), tap and (c, nw) go into the scalar
    // offset -- a tap switch costs scalar adds, no 64-bit address arithmetic on the vector ALU
    auto load_w = [&](int k, int c, int nw) {
        return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, w_lane, k * kTapBytes + (c * NB + nw) * 64 * 16, 0));
    };
    auto load_b = [&](int k, float4(&dst)[NC][NBW]) {
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int nw = 0; nw < NBW; ++nw) dst[c][nw] = load_w(k, c, nw);
    };
    // One weight slice in registers.  It is replaced IN PLACE during the last item of a tap: as soon as the MFMAs of a
    // 16-channel chunk have consumed b[c], the same registers are reloaded with the next tap's chunk, so the weights
    // of the next tap arrive under the matrix work of the current one without a second buffer.  (A double buffer
    // swapped at the tap switch costs hipcc a full register copy plus an s_waitcnt vmcnt(0) per switch -- the loop-
    // carried swap cannot be allocated copy-free -- which also drained the gather prefetch ring one item in five.)
    float4 b[NC][NBW];
    static_assert(DEPTH >= 2, "the slot freed by the previous item is refilled during the current item's MFMAs");
    int k_s, e_s, code_s;
#pragma unroll
    for (int d = 0; d < DEPTH - 1; ++d) {
        stage_a1(d, stage_a0(d), k_s, e_s);
        const unsigned vo = gather_offset(e_s);
#pragma unroll
        for (int c = 0; c < NC; ++c) a_r[d][c] = gather_chunk(vo, c);
        k_r[d] = k_s;
        row_r[d] = e_s;
    }
    k_r[DEPTH - 1] = -1;
    row_r[DEPTH - 1] = kPad;
    stage_a1(DEPTH - 1, stage_a0(DEPTH - 1), k_s, e_s);  // staged for the first loop iteration
    code_s = stage_a0(DEPTH);
    if (n_items > 0) load_b(k_r[0], b);  // weights of the first tap (the only exposed weight latency of the chunk)
    if (chunk == 0) { FD_T(3); FD_TV(8, (unsigned long long)n_items); FD_TV(9, (unsigned long long)n_chunks); FD_TV(10, (unsigned long long)n_rows);
                      FD_TV(11, (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11))); FD_TV(12, (unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11))); }
    FD_TV(13, (unsigned long long)(g_trace ? g_trace[(size_t)blockIdx.x * 16 + 13] : 0) + (unsigned long long)n_items);

    // transposed product: A operand = weight fragment (row index = output channel), B operand = gathered rows (column
    // index = pair), so acc[nw] of lane (pair lrow, quad lq) = out[pair][cb + 16 nw + 4 lq .. + 3]
    auto mfma_chunk = [&](const u32x4 &a4, const float4(&bc)[NBW], f32x4(&acc)[NACC]) {
        const float4 av = __builtin_bit_cast(float4, a4);
#pragma unroll
        for (int nw = 0; nw < NBW; ++nw) acc[nw] = __builtin_amdgcn_mfma_f32_16x16x4f32(bc[nw].x, av.x, acc[nw], 0, 0, 0);
#pragma unroll
        for (int nw = 0; nw < NBW; ++nw) acc[nw] = __builtin_amdgcn_mfma_f32_16x16x4f32(bc[nw].y, av.y, acc[nw], 0, 0, 0);
#pragma unroll
        for (int nw = 0; nw < NBW; ++nw) acc[nw] = __builtin_amdgcn_mfma_f32_16x16x4f32(bc[nw].z, av.z, acc[nw], 0, 0, 0);
#pragma unroll
        for (int nw = 0; nw < NBW; ++nw) acc[nw] = __builtin_amdgcn_mfma_f32_16x16x4f32(bc[nw].w, av.w, acc[nw], 0, 0, 0);
    };

    for (int i0 = 0; i0 < n_items; i0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            // accumulator row of this lane's pair (the row field of a padding entry is the scratch row TM): one swizzled
            // 16-byte slot per 16-column block
            const unsigned arow = sk::entry_local_row(row_r[d]);
            unsigned aoff[NBW];
#pragma unroll
            for (int nw = 0; nw < NBW; ++nw) aoff[nw] = sk::acc_slot_bytes<COUT>(arow, slot0 + 4u * nw);
            // The old accumulator values are requested first and are the C operand of the MFMA chain: the matrix pipe
            // does the accumulation and D goes back to LDS untouched -- no vector-ALU work on the accumulators at all
            // (VALU instructions of one wave barely overlap the MFMAs of the other waves of its SIMD, so every VALU
            // instruction saved per item is matrix-pipe time gained).  The bookkeeping below covers the LDS latency.
            f32x4 acc[NACC];
#pragma unroll
            for (int nw = 0; nw < NBW; ++nw) acc[nw] = *reinterpret_cast<const f32x4 *>(acc_bytes + aoff[nw]);
            // refill the slot freed by the previous item BEFORE this item's MFMAs (left to itself hipcc sinks the loads
            // below the MFMA block and waits vmcnt(0) for them at the top of the next item), then advance the two
            // bookkeeping stages; their results are first touched in the next iteration.
            const int dn = (d + DEPTH - 1) % DEPTH;  // compile-time after unrolling
            unsigned vo;
            {
                const int it = i0 + d + DEPTH - 1;
                vo = gather_offset(e_s);
                k_r[dn] = k_s;
                row_r[dn] = e_s;
                stage_a1(it + 1, code_s, k_s, e_s);
                code_s = stage_a0(it + 2);
            }
            const int knext = k_r[(d + 1) % DEPTH];                 // tap of the next item (-1 past the end), wave-uniform
            const bool reload = knext >= 0 && knext != k_r[d];      // this is the last item of its tap
            // narrow layers (fewer than 16 MFMAs per item) have too little matrix work between the loads for the
            // interleaving to pay: their gather goes out in one piece in front of the MFMAs
            constexpr bool kSpread = NC * 4 * NBW >= 16;
            if constexpr (!kSpread) {
#pragma unroll
                for (int c = 0; c < NC; ++c) a_r[dn][c] = gather_chunk(vo, c);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (reload) {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    mfma_chunk(a_r[d][c], b[c], acc);
                    if constexpr (kSpread) a_r[dn][c] = gather_chunk(vo, c);  // the gather of item i+DEPTH-1 is spread between the MFMAs
#pragma unroll
                    for (int nw = 0; nw < NBW; ++nw) b[c][nw] = load_w(knext, c, nw);
                    __builtin_amdgcn_sched_group_barrier(0x008, 4 * NBW, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, (kSpread ? 1 : 0) + NBW, 0);
                }
            } else {
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    mfma_chunk(a_r[d][c], b[c], acc);
                    if constexpr (kSpread) {
                        a_r[dn][c] = gather_chunk(vo, c);
                        __builtin_amdgcn_sched_group_barrier(0x008, 4 * NBW, 0);
                        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    }
                }
            }
#pragma unroll
            for (int nw = 0; nw < NBW; ++nw) *reinterpret_cast<f32x4 *>(acc_bytes + aoff[nw]) = acc[nw];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (chunk == 0) FD_T(4);
    __syncthreads();
    if (chunk == 0) FD_T(5);
    sk::epilogue<TM, COUT, TS>(s_acc, bias, residual, relu, out, row0, n_rows);
    __syncthreads();  // the next chunk re-uses the list and the accumulator tile
    if (chunk == 0) FD_T(6);
    }  // chunk loop
    FD_T(7);
}

// LDS request of one workgroup.  Occupancy is not a lever here: MFMA and non-MFMA instructions of the waves sharing a
// SIMD execute almost serially (128 channels: one workgroup per CU is only 9 % slower than two), and for the 64->64
// layers two workgroups per CU beat the three that would fit (300 -> 278 us: less contention in the gather path), so
// their request is rounded up to just over a third of the CU's 160 KB.
inline size_t lds_request(int cin, int cout, int tm) {
    const size_t lds = (size_t)sk::layout(tm, cout, tap_splits(cout), 16).bytes;
    return (cin == 64 && cout == 64 && tm == 128 && lds < 56 * 1024) ? (size_t)56 * 1024 : lds;
}

// the shapes with a bank-spread gather: 64 -> 64 and 128 -> 128 (32 -> 32 has its own kernel, fd_spconv_c32.hip)
constexpr bool has_swz_gather(int cin, int cout, int tm) { return cin == cout && (cin == 64 || cin == 128) && tm == sk::kPlanTM; }

template <int CIN, int COUT, int TM, int DEPTH, bool PLAN = false, bool SWZ = false>
int launch_compact(const fd::SpconvCall &c) {
    if constexpr (!PLAN && !SWZ) {
        // a bank-spread tensor: the input only where the gather is instantiated, output / residual rows of 128 bytes and more
        if ((c.layout & sk::kLayoutIn) && !has_swz_gather(CIN, COUT, TM)) return 0;
        if ((c.layout & (sk::kLayoutResidual | sk::kLayoutOut)) && COUT < 32) return 0;
        if constexpr (has_swz_gather(CIN, COUT, TM)) {
            if (c.layout & sk::kLayoutIn) return launch_compact<CIN, COUT, TM, DEPTH, false, true>(c);
        }
    }
    // the layers that read a chunk plan: SubM at 32 channels and up, and the strided 16 -> 32, 32 -> 64, 64 -> 128 (one row set per
    // 128-row chunk each)
    if constexpr (!PLAN && ((CIN == COUT && COUT >= 32) || COUT == 2 * CIN) && TM == sk::kPlanTM) {
        if (c.plan) return launch_compact<CIN, COUT, TM, DEPTH, true, SWZ>(c);
    }
    const size_t lds_req = lds_request(CIN, COUT, TM);
    static std::atomic<uint64_t> lds_set{0};  // devices on which this instantiation has its LDS limit raised
    auto kern = spconv_f32_compact<CIN, COUT, TM, DEPTH, PLAN, SWZ>;
    if (!fd::ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds_req, lds_set)) return 0;
    const unsigned in_bytes = (unsigned)(c.n_in * CIN * 4);
    int n_ranges = c.n_ranges, rows_per = 0;
    if (!c.ranges) sk::equal_rows_split(c.n_out, TM, c.n_out_dev != nullptr, n_ranges, rows_per);
    const void *wp = (const char *)c.wpacked + fd::spconv_weight_layout(c).base.offset;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_ranges), dim3(256), lds_req, c.stream, (const float *)c.in, (const float4 *)wp, c.bias,
                       (const float *)c.residual, sk::kernel_flags(c.relu, c.layout), PLAN ? c.plan : c.nbr, PLAN ? c.plan_stride : c.nbr_stride, c.K, c.n_out, c.n_out_dev,
                       (float *)c.out, in_bytes, c.ranges, rows_per);
    return 1;
}

// ---------------------------------------------------------------------------------------------- work-balanced ranges
// work of an 8-row block in 1/32 of a 16-pair MFMA group: 2 per pair, + 1 per (block, tap) that has pairs (its share of
// the list padding: half a group per tap and 128-row chunk), + kRowCost for the per-row cost of prologue / compaction /
// epilogue: the phase trace puts those at ~10 groups per 128-row chunk = 20 units per block (swept 4 ... 48: 20-32 is the
// flat optimum, 128->128 -2.5 %, 64->64 -1 % against the 4 of the first version, which let sparse regions grow ranges past
// 128 rows, i.e. into a second chunk with its own padding and prologue).  An iterative refinement with the kernel's exact
// group count per range was tried and is worse (98 ... 156 groups per wave instead of 120 ... 151): the cost of a range
// jumps by ~23 groups when it crosses 128 rows, which a boundary interpolation cannot follow; with the ranges capped at
// 128 rows (one chunk each) the refinement converges but the layer time does not move (348 vs 352 us): the group count per
// workgroup is not what sets the kernel's duration.
// One wave covers 64 rows = 8 blocks with one ballot per tap; lane i < 8 accumulates block i.
constexpr int kWorkRows = 8;
constexpr int kRowCost = 24;
__global__ void __launch_bounds__(256) block_work_kernel(const int *__restrict__ nbr, int64_t nbr_stride, int K, int n_out,
                                                         const int *__restrict__ n_out_dev, unsigned row_cost, unsigned *__restrict__ work) {
    n_out = fd::device_count(n_out, n_out_dev);
    const int n_blocks = (n_out + kWorkRows - 1) / kWorkRows;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t o = wave * 64 + lane;
    if (wave * 8 >= n_blocks) return;
    unsigned w = row_cost;
    for (int k = 0; k < K; ++k) {
        const bool v = o < n_out && nbr[(int64_t)k * nbr_stride + o] >= 0;
        const unsigned long long m = __ballot(v);
        const unsigned byte = (unsigned)(m >> (8 * (lane & 7))) & 0xffu;
        w += (unsigned)__popc(byte) * 2u + (byte ? 1u : 0u);
    }
    if (lane < 8 && wave * 8 + lane < n_blocks) work[wave * 8 + lane] = w;
}

// single workgroup: prefix over the block works, range j = blocks whose work midpoint falls into the j-th of n_ranges
// equal slices of the total.  Boundaries are multiples of 8 rows; a range may be empty (one block heavier than a slice).
// Round 6: every pass over the works is coalesced -- the 16 waves own contiguous segments and walk them 64 blocks at a time with a
// shuffle scan (the round 2-5 form gave each of the 1024 threads ~40 CONSECUTIVE blocks: 40 strided load instructions per thread, twice,
// between two 1024-wide Hillis-Steele scans; 28 us per launch for a 150-KB table).  Same table bit for bit.
__global__ void __launch_bounds__(1024) range_split_kernel(const unsigned *__restrict__ work, int n_out, const int *__restrict__ n_out_dev,
                                                           int n_ranges, int *__restrict__ ranges) {
    n_out = fd::device_count(n_out, n_out_dev);
    const int n_blocks = (n_out + kWorkRows - 1) / kWorkRows;
    __shared__ unsigned long long s_seg[16];
    __shared__ unsigned long long s_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n_blocks == 0) {
        for (int j = tid; j <= n_ranges; j += 1024) ranges[j] = 0;
        return;
    }
    const int seg = (((n_blocks + 15) / 16) + 63) & ~63;  // blocks per wave (whole 64-block steps)
    const int b_lo = wave * seg, b_hi = min(n_blocks, b_lo + seg);
    // ---- segment sums (coalesced), their exclusive scan, the total
    constexpr int kU = 16;  // loads in flight per lane (a dependent load per 64 blocks costs a memory round trip each: 38 of them per pass before)
    unsigned long long sum = 0;
    for (int c0 = b_lo; c0 < b_hi; c0 += 64 * kU) {
        unsigned wv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int bb = c0 + 64 * u + lane;
            wv[u] = work[bb < b_hi ? bb : b_hi - 1];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) sum += (c0 + 64 * u + lane < b_hi) ? wv[u] : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s_seg[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int w = 0; w < 16; ++w) { const unsigned long long v = s_seg[w]; s_seg[w] = run; run += v; }
        s_total = run;
    }
    __syncthreads();
    const unsigned long long total = s_total > 0 ? s_total : 1ull;
    // range of a block = floor(midpoint * n_ranges / total), as one double multiply (monotone in the midpoint, the same function in
    // every thread: all the table needs -- results do not depend on the ranges, tests/test_gpu_parity.py)
    const double scale = (double)n_ranges / (2.0 * (double)total);
    auto range_of = [&](unsigned long long ex, unsigned w) -> int {
        const int r = (int)((double)(2ull * ex + w) * scale);
        return r < n_ranges ? r : n_ranges - 1;
    };
    unsigned long long run = s_seg[wave];  // exclusive prefix of this wave's first block
    int prev = -1;                         // range of the block in front of the current one (-1 in front of block 0)
    if (b_lo > 0 && b_lo < n_blocks) {
        const unsigned wp = work[b_lo - 1];
        prev = range_of(run - wp, wp);
    }
    // 512 blocks per step: loaded coalesced into this wave's LDS slice, then lane l walks blocks 8 l .. 8 l + 7 on its own -- one shuffle scan
    // (of the lanes' 8-block sums) per 512 blocks instead of one per 64
    constexpr int kB = 8;
    __shared__ unsigned s_buf[16][64 * (kB + 1)];
    unsigned *buf = s_buf[wave];
    for (int c0 = b_lo; c0 < b_hi; c0 += 64 * kB) {
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int e = 64 * u + lane, bb = c0 + e;
            buf[(e / kB) * (kB + 1) + e % kB] = bb < b_hi ? work[bb] : 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        unsigned w[kB];
        unsigned tot = 0;
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            w[i] = buf[lane * (kB + 1) + i];
            tot += w[i];
        }
        unsigned inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        unsigned long long ex = run + (inc - tot);
        // the range of the block in front of this lane's first one: the previous lane's last block (lane 0: the carry)
        const int first = c0 + lane * kB;
        int last_rg = prev;
        {
            unsigned long long e2 = ex;
#pragma unroll
            for (int i = 0; i < kB; ++i) {
                if (first + i < b_hi) last_rg = range_of(e2, w[i]);
                e2 += w[i];
            }
        }
        int before = __shfl_up(last_rg, 1);
        if (lane == 0) before = prev;
        // (a lane whose blocks all lie past the segment end keeps the carry: its last_rg is its predecessor's, handed on below)
        if (first >= b_hi) last_rg = before;
#pragma unroll
        for (int i = 0; i < kB; ++i) {
            const int bb = first + i;
            if (bb < b_hi) {
                const int rg = range_of(ex, w[i]);
                for (int j = before + 1; j <= rg; ++j) ranges[j] = bb * kWorkRows;
                before = rg;
                if (bb == n_blocks - 1)  // the thread owning the last block closes the table
                    for (int j = rg + 1; j <= n_ranges; ++j) ranges[j] = n_out;
            }
            ex += w[i];
        }
        // carry into the next step: the range of the step's last valid block, the step's total
        const int n_valid = min(64 * kB, b_hi - c0);
        prev = __shfl(last_rg, (n_valid - 1) / kB);
        run += __shfl(inc, 63);
        __builtin_amdgcn_wave_barrier();  // (the slice is rewritten by the next step)
    }
}

// ------------------------------------------------------------------------------------------------------- chunk plan
// The compacted lists of every (range, chunk) of a shared rulebook, written once (layout: fd_spconv_chunk.h).  Workgroup
// (x, y) of a grid of n_ranges x kPlanSplit resolves range x exactly as the convolution's workgroup x does (the same
// resolve_range / cut_chunks / chunk_span, the same grid width) and takes its chunks y, y + kPlanSplit, ...; wave w compacts
// the taps w, w + 4, ... of a chunk straight from global memory with compact_taps' ballots: the same entries in the same order.
// No LDS, no barrier, nothing shared between workgroups.  Bound: reads the 4 K N_out bytes of the rulebook once, writes 4 (K + 1) N_out.
constexpr int kPlanSplit = 4;
__global__ void __launch_bounds__(256) chunk_plan_kernel(const int *__restrict__ nbr, int64_t nbr_stride, int n_out, const int *__restrict__ n_out_dev,
                                                         const int *__restrict__ ranges, int rows_per_range, int *__restrict__ plan, int64_t plan_stride) {
    constexpr int TM = sk::kPlanTM, K = sk::kMaxTaps, NT = (K + 3) / 4, NH = TM / 64;
    constexpr int kPad = sk::pad_entry(TM);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int r_begin, r_end, n_chunks, chunk_rows;
    sk::resolve_range(n_out, n_out_dev, ranges, rows_per_range, r_begin, r_end);
    if (r_begin < 0 || r_begin >= r_end) return;
    sk::cut_chunks<TM>(r_begin, r_end, n_chunks, chunk_rows);
    for (int chunk = blockIdx.y; chunk < n_chunks; chunk += kPlanSplit) {
        int row0, n_rows;
        if (!sk::chunk_span(r_begin, r_end, chunk_rows, chunk, row0, n_rows)) break;
        // all of the wave's loads first (one memory round trip per chunk), rows past the chunk's end as "no pair"
        int v[NT][NH];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int k = wave + 4 * j < K ? wave + 4 * j : K - 1;
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int r = h * 64 + lane;
                const int rr = r < n_rows ? r : n_rows - 1;  // (clamped address, selected on use)
                v[j][h] = nbr[(int64_t)k * nbr_stride + row0 + rr];
                if (r >= n_rows) v[j][h] = -1;
            }
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int k = wave + 4 * j;
            if (k >= K) break;
            int *list = plan + (int64_t)k * plan_stride + row0;  // [n_rows]
            int count = 0;
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const unsigned long long m = __ballot(v[j][h] >= 0);
                const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
                if (v[j][h] >= 0) list[pos] = sk::pack_entry(v[j][h], h * 64 + lane);
                count += __popcll(m);
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int p = h * 64 + lane;
                if (p >= count && p < n_rows) list[p] = kPad;
            }
            if (lane == 0) reinterpret_cast<unsigned char *>(plan + (int64_t)K * plan_stride + row0)[k] = (unsigned char)count;
        }
    }
}

// -------------------------------------------------------------------------------- plan and block works from the index
// On the fp32 inference sweep the dense [27][N] tables of levels 1-3 only carried data from rulebook_kernel to the kernels above
// (and, strided, to a convolution workgroup that compacted its slice while it held a compute unit's matrix pipe): 27 x 4 bytes per
// row written, read back once or twice.  The entries depend on nothing but the index (bit words + prefix), the output rows'
// coordinates and the row split, so these kernels make plan and works from those: rulebook_kernel's bit tests feed
// chunk_plan_kernel's ballots directly.  The same entries in the same order, so the convolutions' sums keep their order.
struct PlanSource {
    const unsigned long long *words;  // the INPUT level's index
    const int *prefix;
    const int *out_coords;            // [n_out][4] (b, z, y, x): the output level's rows
    const int *n_out_dev;
    const int *ranges;                // the convolution launch's row split (resolve_range)
    int *plan;
    int64_t plan_stride;
    fd::IndexGeom gi;
    int n_out, n_ranges, rows_per_range;
    int s[3], p[3];                   // stride and padding of the 3 x 3 x 3 window (z, y, x)
};
constexpr int kMaxPlanSources = 8;
struct PlanSources {
    PlanSource t[kMaxPlanSources];
};

// rulebook_kernel's test of one tap: the input row at height iz of a column (bit word w, first row `base`), -1 when there is none
__device__ __forceinline__ int tap_row(unsigned long long w, int base, int iz, int D) {
    return (iz >= 0 && iz < D && ((w >> iz) & 1ull)) ? base + __popcll(w & ((1ull << iz) - 1ull)) : -1;
}

// chunk_plan_kernel with the table read replaced by the index lookup.  grid = (widest table's ranges, kPlanSplit, tables): one
// launch serves several tables, so that their dependent load chains (coordinates -> words / prefixes) overlap instead of running one
// launch behind the other.  A wave takes the (ky, kx) columns w, w + 4, w + 8 of the window and their three kz taps: a column's word
// and prefix are loaded once for its taps, all of a chunk's loads are requested before any is used.  No LDS, nothing shared
// between workgroups.
__global__ void __launch_bounds__(256) index_plan_kernel(const PlanSources S) {
    constexpr int TM = sk::kPlanTM, K = sk::kMaxTaps, NH = TM / 64, NCOL = 3;
    constexpr int kPad = sk::pad_entry(TM);
    const PlanSource &t = S.t[blockIdx.z];
    if ((int)blockIdx.x >= t.n_ranges) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int r_begin, r_end, n_chunks, chunk_rows;
    sk::resolve_range_of((int)blockIdx.x, t.n_ranges, t.n_out, t.n_out_dev, t.ranges, t.rows_per_range, r_begin, r_end);
    if (r_begin < 0 || r_begin >= r_end) return;
    sk::cut_chunks<TM>(r_begin, r_end, n_chunks, chunk_rows);
    const fd::IndexGeom gi = t.gi;
    for (int chunk = blockIdx.y; chunk < n_chunks; chunk += kPlanSplit) {
        int row0, n_rows;
        if (!sk::chunk_span(r_begin, r_end, chunk_rows, chunk, row0, n_rows)) break;
        int4 c[NH];  // (b, z, y, x)
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int r = h * 64 + lane;
            c[h] = reinterpret_cast<const int4 *>(t.out_coords)[row0 + (r < n_rows ? r : n_rows - 1)];  // (clamped address, selected on use)
        }
        unsigned long long w[NCOL][NH];
        int base[NCOL][NH];
#pragma unroll
        for (int j = 0; j < NCOL; ++j) {
            const int c9 = wave + 4 * j, ky = c9 / 3, kx = c9 - 3 * ky;
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int iy = c[h].z * t.s[1] - t.p[1] + ky;
                const int ix = c[h].w * t.s[2] - t.p[2] + kx;
                const bool ok = c9 < 9 && h * 64 + lane < n_rows && iy >= 0 && iy < gi.H && ix >= 0 && ix < gi.W;
                const int64_t col = ok ? fd::col_of(gi, c[h].x, iy, ix) : 0;  // (unconditional loads at a clamped address)
                const unsigned long long wv = t.words[col];
                base[j][h] = t.prefix[col];
                w[j][h] = ok ? wv : 0ull;  // rows past the chunk's end as "no pair"
            }
        }
#pragma unroll
        for (int j = 0; j < NCOL; ++j) {
            const int c9 = wave + 4 * j;
            if (c9 >= 9) break;
            for (int kz = 0; kz < 3; ++kz) {
                const int k = kz * 9 + c9;
                int *list = t.plan + (int64_t)k * t.plan_stride + row0;  // [n_rows]
                int v[NH];
#pragma unroll
                for (int h = 0; h < NH; ++h) v[h] = tap_row(w[j][h], base[j][h], c[h].y * t.s[0] - t.p[0] + kz, gi.D);
                int count = 0;
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    const unsigned long long m = __ballot(v[h] >= 0);
                    const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
                    if (v[h] >= 0) list[pos] = sk::pack_entry(v[h], h * 64 + lane);
                    count += __popcll(m);
                }
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    const int p = h * 64 + lane;
                    if (p >= count && p < n_rows) list[p] = kPad;
                }
                if (lane == 0) reinterpret_cast<unsigned char *>(t.plan + (int64_t)K * t.plan_stride + row0)[k] = (unsigned char)count;
            }
        }
    }
}

// block_work_kernel for a SubM level (stride 1, padding 1), the table's "entry >= 0" replaced by the bit test: the same work array.
__global__ void __launch_bounds__(256) index_work_kernel(const unsigned long long *__restrict__ words, fd::IndexGeom g, const int *__restrict__ coords,
                                                         int n_out, const int *__restrict__ n_out_dev, unsigned row_cost, unsigned *__restrict__ work) {
    n_out = fd::device_count(n_out, n_out_dev);
    const int n_blocks = (n_out + kWorkRows - 1) / kWorkRows;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t o = wave * 64 + lane;
    if (wave * 8 >= n_blocks) return;
    const bool in = o < n_out;
    const int4 c = reinterpret_cast<const int4 *>(coords)[in ? o : n_out - 1];  // (b, z, y, x); clamped address
    unsigned long long wv[9];
#pragma unroll
    for (int c9 = 0; c9 < 9; ++c9) {
        const int iy = c.z - 1 + c9 / 3, ix = c.w - 1 + c9 % 3;
        const bool ok = in && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
        const unsigned long long x = words[ok ? fd::col_of(g, c.x, iy, ix) : 0];
        wv[c9] = ok ? x : 0ull;
    }
    unsigned w = row_cost;
#pragma unroll
    for (int c9 = 0; c9 < 9; ++c9) {
        for (int kz = 0; kz < 3; ++kz) {
            const int iz = c.y - 1 + kz;
            const bool v = iz >= 0 && iz < g.D && ((wv[c9] >> iz) & 1ull);
            const unsigned long long m = __ballot(v);
            const unsigned byte = (unsigned)(m >> (8 * (lane & 7))) & 0xffu;
            w += (unsigned)__popc(byte) * 2u + (byte ? 1u : 0u);
        }
    }
    if (lane < 8 && wave * 8 + lane < n_blocks) work[wave * 8 + lane] = w;
}

}  // namespace

// ---- the chunk plan of a shared rulebook (see fd_spconv_chunk.h and chunk_plan_kernel)
extern "C" int64_t fd_spconv_plan_stride(int64_t n_out) { return n_out < 0 ? 0 : sk::plan_stride_for(n_out); }
extern "C" size_t fd_spconv_plan_bytes(int64_t n_out) { return n_out < 0 ? 0 : sizeof(int32_t) * (size_t)sk::kPlanRows * (size_t)sk::plan_stride_for(n_out); }

// 1 when fd_spconv_apply_plan reads a plan for this layer shape: the fp32 SubM layers whose kernels cut 128-row chunks with one row
// set.  "spconv_plan" = -1 switches the plan off for A/B runs.
extern "C" int fd_spconv_plan_wanted(int cin, int cout, int dtype) {
    if (dtype != 0 || cin != cout || fd::tuning(fd::kTuneSpconvV1) || fd::tuning(fd::kTuneSpconvPlan) < 0) return 0;
    return cin == 32 || cin == 64 || cin == 128;
}

extern "C" int fd_spconv_plan_build(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, const int32_t *ranges,
                                    int n_ranges, int32_t *plan, int64_t plan_stride, fd_stream_t stream_) {
    FD_REQUIRE(K == sk::kMaxTaps, "fd_spconv_plan_build: a chunk plan belongs to a SubM rulebook (K = 27)");
    FD_REQUIRE(n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31), "fd_spconv_plan_build: n_out out of range");
    FD_REQUIRE(n_ranges >= 0 && (ranges == nullptr || n_ranges >= 1), "fd_spconv_plan_build: ranges needs n_ranges >= 1");
    if (n_out == 0) return FD_OK;
    FD_REQUIRE(nbr && plan, "fd_spconv_plan_build: null argument");
    FD_REQUIRE(plan_stride >= sk::plan_stride_for(n_out), "fd_spconv_plan_build: plan_stride below fd_spconv_plan_stride(n_out)");
    int rows_per = 0;  // the split of the convolution launches (launch_compact / launch_c32)
    if (!ranges) sk::equal_rows_split((int)n_out, sk::kPlanTM, n_out_dev != nullptr, n_ranges, rows_per);
    hipLaunchKernelGGL(chunk_plan_kernel, dim3((unsigned)n_ranges, kPlanSplit), dim3(256), 0, fd::as_stream(stream_), nbr, nbr_stride, (int)n_out,
                       n_out_dev, ranges, rows_per, plan, plan_stride);
    return fd::check_launch("fd_spconv_plan_build");
}

// 1 when the layer shape takes its chunk plan straight from the index (fd_spconv_plan_from_index) and runs without a rulebook table:
// the SubM shapes of fd_spconv_plan_wanted plus the strided 16 -> 32, 32 -> 64 and 64 -> 128 (K = 27, one row set per 128-row chunk).
// "spconv_plan" = 1 keeps the table route (fd_rulebook + fd_spconv_plan_build) for A/B runs, 2 keeps it for the strided layers only.
extern "C" int fd_spconv_index_plan_wanted(int cin, int cout, int dtype) {
    const int knob = fd::tuning(fd::kTuneSpconvPlan);
    if (knob == 1) return 0;
    if (cin == cout) return fd_spconv_plan_wanted(cin, cout, dtype);
    if (dtype != 0 || knob < 0 || knob == 2 || fd::tuning(fd::kTuneSpconvV1)) return 0;
    if (cin == 16 && fd::tuning(fd::kTuneF32ResRG) >= 32) return 0;  // (16 -> 32 forced onto the resident kernel, which reads the table)
    return (cin == 16 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 128);
}

extern "C" int fd_spconv_plan_from_index(int B, int n_sources, const fd_plan_source *sources, fd_stream_t stream_) {
    FD_REQUIRE(sources && n_sources >= 1 && n_sources <= kMaxPlanSources && B >= 1, "fd_spconv_plan_from_index: need 1 <= n_sources <= 8 and B >= 1");
    PlanSources S{};
    int n = 0, width = 0;
    for (int i = 0; i < n_sources; ++i) {
        const fd_plan_source &s = sources[i];
        FD_REQUIRE(s.n_out >= 0 && s.n_out < (1ll << 31), "fd_spconv_plan_from_index: n_out out of range");
        FD_REQUIRE(s.n_ranges >= 0 && (s.ranges == nullptr || s.n_ranges >= 1), "fd_spconv_plan_from_index: ranges needs n_ranges >= 1");
        for (int a = 0; a < 3; ++a)
            FD_REQUIRE(s.stride[a] >= 1 && s.stride[a] <= 4 && s.pad[a] >= 0 && s.pad[a] <= 2, "fd_spconv_plan_from_index: unsupported stride/pad");
        if (s.n_out == 0) continue;  // an empty level: nothing to write
        FD_REQUIRE(s.in_words && s.in_prefix && s.out_coords && s.plan, "fd_spconv_plan_from_index: null argument");
        FD_REQUIRE(s.Din > 0 && s.Din <= 64 && s.Hin > 0 && s.Win > 0, "fd_spconv_plan_from_index: bad grid (D must be <= 64)");
        FD_REQUIRE(s.plan_stride >= sk::plan_stride_for(s.n_out), "fd_spconv_plan_from_index: plan_stride below fd_spconv_plan_stride(n_out)");
        PlanSource &t = S.t[n++];
        t.words = (const unsigned long long *)s.in_words;
        t.prefix = s.in_prefix;
        t.out_coords = s.out_coords;
        t.n_out_dev = s.n_out_dev;
        t.ranges = s.ranges;
        t.plan = s.plan;
        t.plan_stride = s.plan_stride;
        t.gi = fd::make_geom(B, s.Din, s.Hin, s.Win);
        t.n_out = (int)s.n_out;
        t.n_ranges = s.n_ranges;
        t.rows_per_range = 0;  // the split of the convolution launches (launch_compact / launch_c32)
        if (!s.ranges) sk::equal_rows_split(t.n_out, sk::kPlanTM, s.n_out_dev != nullptr, t.n_ranges, t.rows_per_range);
        for (int a = 0; a < 3; ++a) { t.s[a] = s.stride[a]; t.p[a] = s.pad[a]; }
        width = t.n_ranges > width ? t.n_ranges : width;
    }
    if (n == 0) return FD_OK;
    hipLaunchKernelGGL(index_plan_kernel, dim3((unsigned)width, kPlanSplit, (unsigned)n), dim3(256), 0, fd::as_stream(stream_), S);
    return fd::check_launch("fd_spconv_plan_from_index");
}

// fd_spconv_ranges for a SubM level (3 x 3 x 3, stride 1, padding 1) without its table: the block works come from the index
extern "C" int fd_spconv_ranges_from_index(const uint64_t *words, int B, int D, int H, int W, const int32_t *coords, int64_t n_out,
                                           const int32_t *n_out_dev, int n_ranges, int32_t *ranges, void *workspace, size_t workspace_bytes,
                                           fd_stream_t stream_) {
    FD_REQUIRE(words && coords && ranges && workspace, "fd_spconv_ranges_from_index: null argument");
    FD_REQUIRE(B >= 1 && D > 0 && D <= 64 && H > 0 && W > 0, "fd_spconv_ranges_from_index: bad grid (D must be <= 64)");
    FD_REQUIRE(n_ranges >= 1 && n_out >= 0 && n_out < (1ll << 31), "fd_spconv_ranges_from_index: bad sizes");
    FD_REQUIRE(workspace_bytes >= fd_spconv_ranges_workspace_bytes(n_out), "fd_spconv_ranges_from_index: workspace too small");
    hipStream_t stream = fd::as_stream(stream_);
    const int n_blocks = (int)((n_out + kWorkRows - 1) / kWorkRows);
    unsigned *work = (unsigned *)workspace;
    if (n_blocks > 0)
        hipLaunchKernelGGL(index_work_kernel, dim3((unsigned)((n_blocks + 31) / 32)), dim3(256), 0, stream, (const unsigned long long *)words,
                           fd::make_geom(B, D, H, W), coords, (int)n_out, n_out_dev, (unsigned)kRowCost, work);
    hipLaunchKernelGGL(range_split_kernel, dim3(1), dim3(1024), 0, stream, work, (int)n_out, n_out_dev, n_ranges, ranges);
    return fd::check_launch("fd_spconv_ranges_from_index");
}

#ifdef FD_V2_TRACE
extern "C" int fd_debug_set_trace(void *p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &p, sizeof(p)) == hipSuccess ? 0 : -1; }
#endif

// How many ranges fd_spconv_apply wants for a layer shape (measured on MI355X, 300k-point cloud, tools/spconv_bench.py):
//   * Cout >= 64 (MFMA-bound, two workgroups resident per CU): exactly one range per resident workgroup slot, equal
//     WORK -- every CU gets the same number of MFMA groups and finishes together (64->64: 229 -> 200 us, 128->128:
//     320 -> 308 us); more, shorter ranges lose that (greedy dispatch leaves up to one range of imbalance per CU);
//   * narrower layers are bound by the per-row skeleton (prologue / compaction / epilogue), three to six workgroups
//     are resident per CU and overlap each other's phases: about one 128-row chunk per range, rounded up to a whole
//     number of ranges per CU, equal ROWS (equal-work ranges put several chunks of a sparse region behind each other
//     in one workgroup: 16->16 28 -> 56 us).
extern "C" int fd_spconv_num_ranges(int64_t n_out, int cin, int cout, int dtype) {
    if (n_out <= 0 || dtype != 0) return 0;
    const int n_cu = fd::device_cu_count();
    const int64_t tiles = (n_out + 127) / 128;
    const int mult = fd::tuning(fd::kTuneV2RangesPerCU);  // tuning override
    int64_t per_cu;
    if (mult) per_cu = mult;
    else if (cout >= 64) per_cu = (int64_t)((160 * 1024) / lds_request(cin, cout, 128));
    else per_cu = (tiles + n_cu - 1) / n_cu;
    if (per_cu < 1) per_cu = 1;
    return (int)(per_cu * n_cu);
}

// 1 when the layer shape profits from equal-work ranges (fd_spconv_ranges), 0 when equal rows are the better split
extern "C" int fd_spconv_wants_balanced_ranges(int cin, int cout, int dtype) { return dtype == 0 && cout >= 64; }

extern "C" size_t fd_spconv_ranges_workspace_bytes(int64_t n_out) {
    return fd::align_up(sizeof(unsigned) * (size_t)((n_out + kWorkRows - 1) / kWorkRows + 8), 256);
}

extern "C" int fd_spconv_ranges(const int32_t *nbr, int64_t nbr_stride, int K, int64_t n_out, const int32_t *n_out_dev, int n_ranges,
                                int32_t *ranges, void *workspace, size_t workspace_bytes, fd_stream_t stream_) {
    FD_REQUIRE(nbr && ranges && workspace, "fd_spconv_ranges: null argument");
    FD_REQUIRE(n_ranges >= 1 && n_out >= 0 && n_out <= nbr_stride && n_out < (1ll << 31), "fd_spconv_ranges: bad sizes");
    FD_REQUIRE(workspace_bytes >= fd_spconv_ranges_workspace_bytes(n_out), "fd_spconv_ranges: workspace too small");
    hipStream_t stream = fd::as_stream(stream_);
    const int n_blocks = (int)((n_out + kWorkRows - 1) / kWorkRows);
    unsigned *work = (unsigned *)workspace;
    if (n_blocks > 0)
        hipLaunchKernelGGL(block_work_kernel, dim3((unsigned)((n_blocks + 31) / 32)), dim3(256), 0, stream, nbr, nbr_stride, K, (int)n_out, n_out_dev,
                           (unsigned)kRowCost, work);
    hipLaunchKernelGGL(range_split_kernel, dim3(1), dim3(1024), 0, stream, work, (int)n_out, n_out_dev, n_ranges, ranges);
    return fd::check_launch("fd_spconv_ranges");
}

namespace fd {
// returns 1 when launched, 0 when this shape is not covered (caller falls back to the register kernel)
int spconv_f32_compact_dispatch(const SpconvCall &c) {
    if (!sk::entries_fit(c.n_in, c.cin)) return 0;
    // <CIN, COUT, chunk height, gather ring depth>: 128-row chunks everywhere; the ring is as deep as the gathered rows leave
    // registers for (4 up to 32 input channels, 3 at 64, 2 at 128)
    switch (c.cin * 1000 + c.cout) {
        case 16016: return launch_compact<16, 16, 128, 4>(c);
        case 16032: return launch_compact<16, 32, 128, 4>(c);
        case 32032: return launch_compact<32, 32, 128, 4>(c);
        case 32064: return launch_compact<32, 64, 128, 4>(c);
        case 64064: return launch_compact<64, 64, 128, 3>(c);
        case 64128: return launch_compact<64, 128, 128, 3>(c);
        case 128128: return launch_compact<128, 128, 128, 2>(c);
        // the transposed shapes: input gradients of the strided 16 -> 32, 32 -> 64 and 64 -> 128 layers (fd_spconv_grad.hip)
        case 32016: return launch_compact<32, 16, 128, 4>(c);
        case 64032: return launch_compact<64, 32, 128, 4>(c);
        case 128064: return launch_compact<128, 64, 128, 2>(c);
    }
    return 0;
}
}  // namespace fd
