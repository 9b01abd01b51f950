// fp32 sparse convolution for the 32 -> 32 layers: 32-pair items on v_mfma_f32_32x32x2_f32.
//
// Same formulation as fd_spconv_v2.hip (row ranges walked in chunks of <= 128 rows, rulebook tile compacted in LDS per tap,
// accumulator tile in LDS, transposed product, no atomics, fixed summation order) with a different unit of work.  The per-chunk
// skeleton both kernels run around their item loops -- LDS layout, list entries, accumulator swizzle, range / chunk resolution,
// slice prefetch and staging, tile init, compaction, work list, epilogue -- is fd_spconv_chunk.h; this file owns the 32-pair unit
// of work: wave -> tap split mapping, gather, weight registers, the 32x32x2 MFMA loop, and its dispatch.  The SQ
// counters of the 16x16x4 kernel on 32 -> 32 (profiles/round2_spconv_sq_counters.txt): 3.0 VALU + 3.9 SALU + 0.7 LDS + 0.4
// VMEM instructions per MFMA, waves stalled on a dependency 47 % of their cycles, and no VALU instruction ever co-executes
// with an MFMA on a SIMD -- a 16-pair x 16-column item carries 8 MFMAs (256 matrix-pipe cycles) for ~50 instructions of item
// decode, gather addressing and accumulator hand-over.  Here an item is 32 pairs x all 32 columns: CIN/2 MFMAs of 64 cycles
// (1024 cycles at CIN = 32) for about the same bookkeeping.  Measured (300k-point cloud, 268k rows, 3.17 M pairs): 146 -> 141 us
// per 32 -> 32 layer, +0.8 % on the whole sweep -- far less than the instruction count suggests.  The item's own bookkeeping does
// bind a little: with it taken off the vector ALU (about 30 -> 18 VALU instructions and four branches -> one per item: slots in
// XOR-linear form, item codes held in a register, weights through a buffer resource, one reload branch; DESIGN.md, "item
// bookkeeping off the vector ALU") the four launches of a two-cloud pass went from 832-836 to 823-826 us, -1.1 %, every run
// below every parent run -- far less than one 64-cycle MFMA slot per removed instruction would have given.  With the rows split between two waves (64-row halves, 28 pairs per tap and half on
// average) half of the 32-pair slots were padding and the kernel was slower (158 us); the 16 -> 32 strided layer (2.4 pairs
// per row) stays on the 16-pair kernel (54 vs 70 us).
//   * waves: wave ts handles the taps k with k % 4 == ts over all rows of the chunk and accumulates into its own copy of the
//     tile; the epilogue adds the four copies (80 KB of LDS per workgroup, two workgroups per CU);
//   * B operand (gathered rows): lane (pair n = lane % 32, k-half h = lane / 32) loads the four consecutive channels
//     8 c + 4 h .. + 3 of its pair's input row per 8-channel step c; A operand: the same channels of W[tap] for output
//     channel lane % 32 (fd_spconv_pack_weight appends this layout for Cout = 32);
//   * D: lane (n, h) register v holds output channel 8 (v / 4) + 4 h + v % 4 of pair n -> four 16-byte accumulator slots
//     per lane, the same slots as the 32-column tile of the v2 kernel (skeleton::acc_slot_bytes), addressed in XOR-linear form
//     (skeleton::acc_row_term): one row term per item, one XOR per slot.
#include "fd_spconv_chunk.h"

namespace {

namespace sk = fd::skeleton;
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 lds_f4;
constexpr int TM = 128, COUT = 32, TS = 4, WR = 1;
constexpr sk::Layout L = sk::layout(TM, COUT, TS, 32);
static_assert(((sk::kMaxTaps + TS - 1) / TS) * (TM / WR / 32) <= L.item_slot, "item list slot");

// PLAN: nbr / nbr_stride are a chunk plan (fd_spconv_chunk.h) instead of the rulebook: the lists arrive compacted
// SWZ: the input rows are stored bank-spread (fd_spconv_chunk.h); `relu` carries skeleton::kernel_flags
template <int CIN, int DEPTH, bool PLAN, bool SWZ>
__global__ void __launch_bounds__(256) spconv_f32_c32(const float *__restrict__ in, const float4 *__restrict__ wp, const float *__restrict__ bias,
                                                      const float *__restrict__ residual, int relu, const int *__restrict__ nbr, int64_t nbr_stride,
                                                      int K, int n_out, const int *__restrict__ n_out_dev, float *__restrict__ out, unsigned in_bytes,
                                                      const int *__restrict__ ranges, int rows_per_range) {
    constexpr int NCH = CIN / 8;  // 8-channel steps = float4 loads per lane and item
    constexpr int kPad = sk::pad_entry(TM);
    extern __shared__ __attribute__((aligned(256))) unsigned char smem[];  // (a multiple of the accumulator swizzle's span, see tile_off)
    int *s_list = reinterpret_cast<int *>(smem + L.list);
    unsigned short *s_items = reinterpret_cast<unsigned short *>(smem + L.items);
    unsigned char *s_cnt = smem + L.cnt;
    int *s_pad = reinterpret_cast<int *>(smem + L.pad);
    float *s_acc = reinterpret_cast<float *>(smem + L.acc);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: what derives from it stays in SGPRs
    int r_begin, r_end, n_chunks, chunk_rows;
    sk::resolve_range(n_out, n_out_dev, ranges, rows_per_range, r_begin, r_end);
    if (r_begin >= r_end) return;
    sk::cut_chunks<TM>(r_begin, r_end, n_chunks, chunk_rows);
    int pre[sk::kSliceRegs<TM>];
    const int k_fetch = PLAN ? sk::kPlanRows : K;
    sk::fetch_slice<TM>(pre, nbr, nbr_stride, k_fetch, r_begin);

    const int ln = lane & 31, lh = lane >> 5;
    const int ts = wave, wr = 0;
    // accumulator slots in XOR-linear form (skeleton::acc_row_term): the wave's tile copy starts at a multiple of the swizzle's span, so its
    // LDS address adds into the row term, and slot q of the lane is that term ^ (lh * 16) ^ (q * 32).  The slots are addressed as LDS
    // integers: added to the generic `smem` the compiler must assume an unknown base behind the XOR and spends an add per slot
    static_assert(L.acc % sk::acc_span(COUT) == 0 && (L.acc_copy * 4) % sk::acc_span(COUT) == 0, "tile copies start at multiples of the swizzle span");
    const unsigned tile_off = (unsigned)(__UINTPTR_TYPE__)(lds_u8 *)smem + (unsigned)(L.acc + ts * L.acc_copy * 4);  // (scalar)
    const unsigned acc_c0 = (unsigned)lh * 16u;                         // column slot 2 q + lh: lh here, q as an XOR of bits 5..6
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)in_bytes, 0x00020000);
    // the weight fragments come through a buffer resource too: tap and step go into the scalar offset, and the
    // lane's part of the address is set once (no 64-bit address arithmetic on the vector ALU per tap switch)
    constexpr int kTapBytes = NCH * 64 * 16;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(wp), 0, K * kTapBytes, 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    unsigned short *items = s_items + wave * L.item_slot;

    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        int row0, n_rows;
        if (!sk::chunk_span(r_begin, r_end, chunk_rows, chunk, row0, n_rows)) break;
        if constexpr (PLAN) {
            sk::stage_plan_chunk<TM, COUT, TS, 32>(pre, s_list, s_cnt, s_pad, s_acc, bias, residual, relu, row0, n_rows);
        } else {
            sk::stage_chunk<TM, COUT, TS, 32>(pre, s_list, s_pad, s_acc, bias, residual, relu, K, row0, n_rows);
            __syncthreads();
            sk::compact_taps<TM, WR>(s_list, s_cnt, K);
        }
        __syncthreads();
        if (chunk + 1 < n_chunks) sk::fetch_slice<TM>(pre, nbr, nbr_stride, k_fetch, row0 + chunk_rows);  // the next chunk's slice travels while this chunk computes
        const int n_items = sk::build_items<TS, 32>(s_cnt, items, K, ts, wr);
        const int codes = sk::item_codes<L.item_slot>(items);  // lane i: code i; the item loop never goes back to LDS for a code

        // software pipeline as in the v2 kernel: item code one iteration ahead of the list entry, the list entry one ahead
        // of the gather, the gather DEPTH - 1 items ahead of the MFMAs; everything branch-free (a slot past the end of the
        // list reads padding entries: out-of-range gather offset -> zeros, accumulator row TM = scratch row)
        int k_r[DEPTH], row_r[DEPTH];
        u32x4 a_r[DEPTH][NCH];
        auto stage_a0 = [&](int it) -> int { return sk::stage_a0_reg(codes, n_items, it); };
        auto stage_a1 = [&](int it, int code, int &kk, int &e) { sk::stage_a1_s<TM, WR, 32>(s_list, s_pad, n_items, wr, ln, it, code, kk, e); };
        // bank-spread rows: the lane's piece is lh + 2 c of the row's one line, stored at piece ^ (row & 7): the row's bits go into
        // the offset once per item, the step's bits with one XOR per load (they no longer add)
        auto gather_offset = [&](int e) -> unsigned {
            const unsigned o = sk::entry_row_bytes<CIN>(e) + (unsigned)(lh * 16);
            return SWZ ? o ^ sk::entry_swz_bits(e) : o;
        };
        auto gather_step = [&](unsigned voff, int c) {
            return SWZ ? __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff ^ (unsigned)(c * 32), 0, 0) : __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + c * 32, 0, 0);
        };
        float4 b[NCH];  // this tap's weights: channels 8 c + 4 lh .. + 3, output channel ln
        auto load_b_step = [&](int k, int c) {
            return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane, k * kTapBytes + c * 64 * 16, 0));
        };
        auto load_b = [&](int k) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) b[c] = load_b_step(k, c);
        };
        int k_s, e_s, code_s;
#pragma unroll
        for (int d = 0; d < DEPTH - 1; ++d) {
            stage_a1(d, stage_a0(d), k_s, e_s);
            const unsigned vo = gather_offset(e_s);
#pragma unroll
            for (int c = 0; c < NCH; ++c) a_r[d][c] = gather_step(vo, c);
            k_r[d] = k_s;
            row_r[d] = e_s;
        }
        k_r[DEPTH - 1] = -1;
        row_r[DEPTH - 1] = kPad;
        stage_a1(DEPTH - 1, stage_a0(DEPTH - 1), k_s, e_s);
        code_s = stage_a0(DEPTH);
        if (n_items > 0) load_b(k_r[0]);

        for (int i0 = 0; i0 < n_items; i0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                // accumulator row of this lane's pair: four swizzled 16-byte slots (channels 8 q + 4 lh .. + 3, q = 0..3)
                const unsigned aterm = (tile_off + sk::acc_row_term<COUT>(sk::entry_local_row(row_r[d]))) ^ acc_c0;
                unsigned aoff[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) aoff[q] = aterm ^ (unsigned)(q * 32);
                f32x16 acc;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const lds_f4 *>((__UINTPTR_TYPE__)aoff[q]);
                    acc[4 * q + 0] = v.x; acc[4 * q + 1] = v.y; acc[4 * q + 2] = v.z; acc[4 * q + 3] = v.w;
                }
                // refill the ring slot freed by the previous item and advance the bookkeeping stages before the MFMAs
                const int dn = (d + DEPTH - 1) % DEPTH;
                {
                    const int it = i0 + d + DEPTH - 1;
                    const unsigned vo = gather_offset(e_s);
                    k_r[dn] = k_s;
                    row_r[dn] = e_s;
#pragma unroll
                    for (int c = 0; c < NCH; ++c) a_r[dn][c] = gather_step(vo, c);
                    stage_a1(it + 1, code_s, k_s, e_s);
                    code_s = stage_a0(it + 2);
                }
                const int knext = k_r[(d + 1) % DEPTH];
                const bool reload = knext >= 0 && knext != k_r[d];  // last item of its tap (wave-uniform)
                __builtin_amdgcn_sched_barrier(0);
                auto mfma_step = [&](int c) {
                    const float4 av = __builtin_bit_cast(float4, a_r[d][c]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c].x, av.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c].y, av.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c].z, av.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[c].w, av.w, acc, 0, 0, 0);
                };
                auto write_back = [&]() {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<lds_f4 *>((__UINTPTR_TYPE__)aoff[q]) = f32x4{acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
                };
                // one wave-uniform branch per item, two copies of the chain (the v2 kernel's shape): a branch per step cut the chain into
                // four blocks, each with its own conservative wait.  Each copy writes its own result back: merged behind the branch, the
                // two chains' accumulators cost a register copy each
                if (reload) {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        mfma_step(c);
                        b[c] = load_b_step(knext, c);  // next tap's step c, under the remaining MFMAs
                    }
                    write_back();
                    asm volatile("; c32 item, reload copy");  // (keeps the compiler from merging the two write-backs again)
                } else {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) mfma_step(c);
                    write_back();
                    asm volatile("; c32 item, plain copy");
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
        sk::epilogue<TM, COUT, TS>(s_acc, bias, residual, relu, out, row0, n_rows);
        __syncthreads();  // the next chunk re-uses the list and the accumulator tile
    }
}

template <int CIN, int DEPTH, bool PLAN, bool SWZ>
int launch_c32(const fd::SpconvCall &c) {
    const unsigned in_bytes = (unsigned)(c.n_in * CIN * 4);
    int n_ranges = c.n_ranges, rows_per = 0;
    if (!c.ranges) sk::equal_rows_split(c.n_out, TM, c.n_out_dev != nullptr, n_ranges, rows_per);
    static std::atomic<uint64_t> lds_set{0};  // devices on which this instantiation has its dynamic-LDS limit raised (> 64 KB)
    if (!fd::ensure_dynamic_lds(reinterpret_cast<const void *>(spconv_f32_c32<CIN, DEPTH, PLAN, SWZ>), (size_t)L.bytes, lds_set)) return 0;
    // the 32x32x2 fragment layout ([K][CIN / 8][64 lanes] float4, see fd_spconv_pack_weight)
    const void *wp = (const char *)c.wpacked + fd::spconv_weight_layout(c).c32.offset;
    hipLaunchKernelGGL((spconv_f32_c32<CIN, DEPTH, PLAN, SWZ>), dim3((unsigned)n_ranges), dim3(256), (size_t)L.bytes, c.stream, (const float *)c.in, (const float4 *)wp,
                       c.bias, (const float *)c.residual, sk::kernel_flags(c.relu, c.layout), PLAN ? c.plan : c.nbr, PLAN ? c.plan_stride : c.nbr_stride, c.K, c.n_out, c.n_out_dev, (float *)c.out, in_bytes, c.ranges, rows_per);
    return 1;
}

}  // namespace

namespace fd {
// Returns 1 when launched.
int spconv_f32_c32_dispatch(const SpconvCall &c) {
    if (c.cout != 32 || c.cin != 32) return 0;
    if (!sk::entries_fit(c.n_in, c.cin)) return 0;
    if (c.layout & sk::kLayoutIn) return c.plan ? launch_c32<32, 3, true, true>(c) : launch_c32<32, 3, false, true>(c);
    return c.plan ? launch_c32<32, 3, true, false>(c) : launch_c32<32, 3, false, false>(c);
}
}  // namespace fd
