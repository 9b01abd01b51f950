// The per-chunk skeleton of the fp32 pair-compacting sparse convolutions: everything fd_spconv_v2.hip (16-pair items) and
// fd_spconv_c32.hip (32-pair items) do around their item loops, defined once.
//
//   * a workgroup (256 threads, 4 waves) owns one RANGE of consecutive output rows and walks it in chunks of at most TM rows;
//     while a chunk's MFMAs run, the next chunk's rulebook slice is already on its way into registers;
//   * the rulebook tile [K][TM] is staged in LDS and compacted IN PLACE per tap with wave ballots / prefix popcounts into lists
//     of (input row << 8 | local output row) entries, tails filled with the padding entry;
//     a kernel given the rulebook's chunk plan finds those lists ready-made in global memory and only stages them ("chunk plan" below);
//   * accumulators for the whole chunk live in LDS: TS copies (one per tap split) of [TM + 1][COUT] fp32; row TM is a scratch
//     row that absorbs the padding lanes so the accumulator traffic needs no exec masking; 16-byte slots are XOR-swizzled by the
//     row so the 16 rows of a lane group land on distinct banks;
//   * each wave walks a flattened work list of (tap, ITEM-pair group) items over its taps and row set;
//   * epilogue: sum of the tile copies, bias (+ residual) (+ ReLU), written out with 16-byte row-contiguous stores.
//
// Template parameters: TM rows per chunk, COUT output channels, TS tap splits (tile copies), WR row splits (row sets of TM / WR
// rows), ITEM pairs per work item (16 or 32).  Everything here inlines into the kernels: no state, no indirection, all sizes
// compile-time.  The phases read threadIdx themselves instead of taking tid / lane / wave: the compiler optimises a helper on its
// own before it inlines it, and only from threadIdx does it know the index's range there (with tid handed in as an int most kernels
// came out 2-4 VGPRs larger and spconv_f32_compact<32,16,128,2> lost a wave of occupancy).  The kernel files keep their unit of work -- wave mapping, gather, weight registers, MFMA loop.
#pragma once
#include "fd_common.h"

namespace fd {
namespace skeleton {

constexpr int kMaxTaps = 27;

// ---------------------------------------------------------------------------------------------------- list entries
// (input row << 8) | local output row.  The padding entry has all high bits set, so its gather byte offset lands beyond the
// buffer (the hardware returns zeros) and its row field is the scratch row TM: a padding lane needs no compare / select.
constexpr int pad_entry(int tm) { return (int)(0xffffff00u | (unsigned)tm); }
__device__ __forceinline__ int pack_entry(int in_row, int local_row) { return (in_row << 8) | local_row; }
__device__ __forceinline__ unsigned entry_local_row(int e) { return (unsigned)e & 255u; }
// byte offset of the entry's input row = (e >> 8) * CIN * 4, computed on the masked entry without a multiply
template <int CIN>
__device__ __forceinline__ unsigned entry_row_bytes(int e) {
    static_assert(CIN == 16 || CIN == 32 || CIN == 64 || CIN == 128, "shift per CIN");
    const unsigned hi = (unsigned)e & 0xffffff00u;
    return CIN >= 64 ? hi << (CIN == 128 ? 1 : 0) : hi >> (CIN == 32 ? 1 : 2);
}

// ---------------------------------------------------------------------------------------------- bank-spread row layout
// A b128 gather is served in passes of 16 lanes, and a pass takes as long as its fullest 16-byte position of a 128-byte line.  The
// MFMA operand layout puts 16 different rows at ONE channel offset in the lanes of a pass: all 16 on one position.  A tensor that
// only these kernels read (a level's inner tensors) may therefore be stored bank-spread: 16-byte piece s of row r sits at piece
// s ^ (r & 7) of its 128-byte line, so the rows of a pass spread over the 8 positions.  Pieces keep their line (256- and 512-byte
// rows), the positions of one line are a permutation (row-contiguous stores stay row-contiguous), and rows of fewer than 128 bytes
// (16 channels) are never spread.  The layout word of a launch (fd_spconv_apply_layout) says which of its tensors are stored so:
constexpr int kLayoutIn = 1, kLayoutResidual = 2, kLayoutOut = 4;
// The kernels take the residual / output bits in their `relu` word, above the ReLU bit (no further kernel argument); the input bit
// is a compile-time switch of the gather (SWZ).
constexpr int kFlagRelu = 1, kFlagResidualSwz = kLayoutResidual, kFlagOutSwz = kLayoutOut;
constexpr int kernel_flags(int relu, int layout) { return (relu ? kFlagRelu : 0) | (layout & (kLayoutResidual | kLayoutOut)); }
// byte position of 16-byte piece `s` (0..7) of row `r` within the piece's 128-byte line
__host__ __device__ constexpr unsigned swz_piece_bytes(unsigned s, unsigned r) { return (s ^ (r & 7u)) << 4; }
// float4 column c4 of row `row` of a COLS-channel tensor, as stored: `on` = the tensor is bank-spread (wave-uniform)
template <int COLS>
__device__ __forceinline__ int swz_col4(int c4, int row, bool on) {
    if constexpr (COLS < 32) return c4;
    return c4 ^ (row & (on ? 7 : 0));
}
// the row-dependent term of a bank-spread gather offset, from the list entry (bits 8..10 = input row & 7): XORed into the byte offset
// of the lane's piece once per item.  The padding entry keeps all its high bits: still out of range.
__device__ __forceinline__ unsigned entry_swz_bits(int e) { return ((unsigned)e >> 4) & 0x70u; }

// host: the entry must fit an int32 and the feature matrix a 31-bit buffer range
inline bool entries_fit(int64_t n_in_bound, int cin) { return n_in_bound < (1ll << 23) && n_in_bound * cin * 4 < (1ll << 31); }

// ------------------------------------------------------------------------------------------------------ LDS layout
// Byte offsets of a workgroup's dynamic LDS; the kernels' pointers and the hosts' requests both come from here.
struct Layout {
    int list;       // int [kMaxTaps][TM]: raw rulebook slice, then the compacted entries
    int items;      // unsigned short [4 waves][item_slot]: the waves' work lists
    int item_slot;  //   entries per wave
    int cnt;        // unsigned char [kMaxTaps][4]: pairs per (tap, row set), each <= 128
    int pad;        // int [ITEM]: padding entries, the list block of a slot past the end of the work list
    int acc;        // float [TS][TM + 1][COUT], 16-byte aligned
    int acc_copy;   //   floats per tile copy
    int bytes;
};
constexpr int acc_copy_floats(int tm, int cout) { return (tm + 1) * cout; }  // TM rows + the scratch row
constexpr int acc_span(int cout) { return cout >= 64 ? 256 : cout * 4; }     // bytes within which the slot swizzle permutes (acc_swizzle)
constexpr Layout layout(int tm, int cout, int ts, int item) {
    Layout l{};
    l.list = 0;
    l.items = l.list + (int)sizeof(int) * kMaxTaps * tm;
    // 16-pair kernels: taps x 16-row groups of the chunk, whatever the wave's share of them; 32-pair kernel: 7 taps x 4 groups
    l.item_slot = item == 16 ? kMaxTaps * (tm / 16) : 32;
    l.cnt = l.items + (int)sizeof(unsigned short) * 4 * l.item_slot;
    l.pad = l.cnt + 112;  // kMaxTaps * 4 counts, rounded up to 16 bytes
    l.acc = l.pad + (int)sizeof(int) * item;
    // the 32-pair kernel addresses its slots in XOR-linear form (acc_row_term): its tile copies start at multiples of the swizzle's span
    if (item == 32) l.acc = (l.acc + acc_span(cout) - 1) / acc_span(cout) * acc_span(cout);
    l.acc_copy = acc_copy_floats(tm, cout);
    l.bytes = l.acc + (int)sizeof(float) * ts * l.acc_copy;
    return l;
}

// 16-byte slot swizzle of the accumulator tile: column slot `col` (4 channels) of local row `row` lives in slot col ^ f(row) of
// the row, so that 16 different rows at one column slot spread over the 16 slots of a 256-byte bank row (COUT 64/128: row & 15;
// 32: two rows per bank row; 16: four).
template <int COUT>
__device__ __forceinline__ unsigned acc_swizzle(unsigned row) {
    static_assert(COUT == 16 || COUT == 32 || COUT == 64 || COUT == 128, "whole bank rows");
    constexpr int kSwzShift = COUT >= 64 ? 0 : COUT == 32 ? 1 : 2;
    constexpr unsigned kSwzMask = COUT >= 64 ? 15u : COUT == 32 ? 7u : 3u;
    return (row >> kSwzShift) & kSwzMask;
}
// slot index in a tile copy (a float4 index: init and epilogue) ...
template <int COUT>
__device__ __forceinline__ int acc_slot(int row, int col) {
    return row * (COUT / 4) + (col ^ (int)acc_swizzle<COUT>((unsigned)row));
}
// ... and the same slot as a byte offset, 16 * acc_slot, for the item loops: row base and swizzled slot stay two shifts and one
// add, so the row part is shared by the slots of an item (shifting the summed index costs an instruction per slot)
template <int COUT>
__device__ __forceinline__ unsigned acc_slot_bytes(unsigned row, unsigned col) {
    return row * (COUT * 4) + ((col ^ acc_swizzle<COUT>(row)) << 4);
}

// The same bytes in XOR-linear form: the row's term has its low log2(acc_span) bits from the swizzle alone and a column slot is less
// than a span, so slot `col` of the row is acc_row_term(row) ^ (col << 4) -- and stays so with a tile offset that is a multiple of
// the span added to the term.  A lane's column constants are set once per kernel, the term once per item: one XOR per slot.
template <int COUT>
__device__ __forceinline__ unsigned acc_row_term(unsigned row) {
    return row * (COUT * 4) + (acc_swizzle<COUT>(row) << 4);
}

// -------------------------------------------------------------------------------------------- row range and chunks
// This workgroup's row range: an entry of the `ranges` table, or the equal-rows split (made here from the device's count when
// there is one, see equal_rows_split).  The range may be empty.
// Range `block` of `n_blocks`: what resolve_range gives workgroup `block` of a launch that is n_blocks wide (the plan builder of
// several tables in one launch, whose grid is as wide as its widest table, resolves each table's ranges with that table's width).
__device__ __forceinline__ void resolve_range_of(int block, int n_blocks, int n_out, const int *n_out_dev, const int *ranges, int rows_per_range,
                                                 int &r_begin, int &r_end) {
    if (n_out_dev) n_out = fd::device_count(n_out, n_out_dev);  // capacity launch (see fd_common.h)
    if (ranges) {
        r_begin = ranges[block];
        r_end = ranges[block + 1];
    } else {
        if (n_out_dev) rows_per_range = (((n_out + n_blocks - 1) / n_blocks) + 15) & ~15;
        const int64_t b = (int64_t)block * rows_per_range;
        r_begin = (int)(b < n_out ? b : n_out);
        r_end = (int)(b + rows_per_range < n_out ? b + rows_per_range : n_out);
    }
    if (r_end > n_out) r_end = n_out;
}
__device__ __forceinline__ void resolve_range(int n_out, const int *n_out_dev, const int *ranges, int rows_per_range,
                                              int &r_begin, int &r_end) {
    resolve_range_of((int)blockIdx.x, (int)gridDim.x, n_out, n_out_dev, ranges, rows_per_range, r_begin, r_end);
}
// the range is cut into equal chunks of at most TM rows (multiples of 16)
template <int TM>
__device__ __forceinline__ void cut_chunks(int r_begin, int r_end, int &n_chunks, int &chunk_rows) {
    n_chunks = (r_end - r_begin + TM - 1) / TM;
    chunk_rows = (((r_end - r_begin + n_chunks - 1) / n_chunks) + 15) & ~15;
}
__device__ __forceinline__ bool chunk_span(int r_begin, int r_end, int chunk_rows, int chunk, int &row0, int &n_rows) {
    row0 = r_begin + chunk * chunk_rows;
    n_rows = (r_end - row0) < chunk_rows ? (r_end - row0) : chunk_rows;
    return n_rows > 0;
}
// host: equal row counts per range (multiples of 16); n_ranges <= 0 -> one TM-row tile per workgroup.  With a device count the
// kernel makes the split over n_ranges itself (resolve_range).
inline void equal_rows_split(int n_out, int tm, bool device_count, int &n_ranges, int &rows_per) {
    if (n_ranges <= 0) n_ranges = (n_out + tm - 1) / tm;
    rows_per = (((n_out + n_ranges - 1) / n_ranges) + 15) & ~15;
    if (!device_count) n_ranges = (n_out + rows_per - 1) / rows_per;
}

// -------------------------------------------------------------------------------------------------- rulebook slice
// rulebook slice of a chunk, one register per 256 entries; loads are branch-free (clamped address, select on use)
template <int TM>
constexpr int kSliceRegs = (kMaxTaps * TM + 255) / 256;

template <int TM>
__device__ __forceinline__ void fetch_slice(int (&pre)[kSliceRegs<TM>], const int *nbr, int64_t nbr_stride, int K, int row0) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < kSliceRegs<TM>; ++i) {
        const int t = tid + i * 256;
        int k = t / TM;
        const int r = t - k * TM;
        k = k < K ? k : K - 1;
        int64_t o = (int64_t)row0 + r;
        o = o < nbr_stride ? o : nbr_stride - 1;
        pre[i] = nbr[(int64_t)k * nbr_stride + o];
    }
}

// Accumulator tile.  For COUT <= 64 the tile starts from bias + residual instead of zero: the epilogue then has no global
// load left (it used to issue one dependent residual load per 256 rows x 4 channels -- 4 to 8 exposed memory round trips per
// chunk, as long as the chunk's whole MFMA loop on the 32-channel layers: the "unexplained" 47 % dependency stall of round 2).
// All loads of a chunk go out back to back here and land during the list staging.  (128 columns: 64 registers per thread
// would be needed; that layer is MFMA-bound and keeps the epilogue form.)
template <int COUT>
constexpr bool kInitAcc = COUT <= 64;

template <int TM, int COUT, int TS>
__device__ __forceinline__ void init_acc(float *s_acc, const float *bias, const float *residual, int flags, int row0, int n_rows) {
    const int tid = threadIdx.x;
    if constexpr (kInitAcc<COUT>) {
        constexpr int C4i = COUT / 4, NINIT = TM * C4i / 256;
        static_assert(TM * C4i % 256 == 0, "whole passes");
        float4 iv[NINIT];
#pragma unroll
        for (int i = 0; i < NINIT; ++i) {
            const int t = tid + i * 256, c4 = t % C4i;
            iv[i] = bias ? reinterpret_cast<const float4 *>(bias)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (residual) {
            float4 rv[NINIT];
#pragma unroll
            for (int i = 0; i < NINIT; ++i) {
                const int t = tid + i * 256, r = t / C4i, c4 = t - r * C4i;
                const int rr = r < n_rows ? r : n_rows - 1;  // (clamped address, selected on use)
                rv[i] = reinterpret_cast<const float4 *>(residual + (int64_t)(row0 + rr) * COUT)[swz_col4<COUT>(c4, row0 + rr, flags & kFlagResidualSwz)];
            }
#pragma unroll
            for (int i = 0; i < NINIT; ++i) { iv[i].x += rv[i].x; iv[i].y += rv[i].y; iv[i].z += rv[i].z; iv[i].w += rv[i].w; }
        }
#pragma unroll
        for (int i = 0; i < NINIT; ++i) {
            const int t = tid + i * 256, r = t / C4i, c4 = t - r * C4i;
            reinterpret_cast<float4 *>(s_acc)[acc_slot<COUT>(r, c4)] = r < n_rows ? iv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // the scratch row of copy 0 and the other tile copies start from zero
        for (int t = TM * C4i + tid; t < TS * acc_copy_floats(TM, COUT) / 4; t += 256) reinterpret_cast<float4 *>(s_acc)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int t = tid; t < TS * acc_copy_floats(TM, COUT) / 4; t += 256) reinterpret_cast<float4 *>(s_acc)[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// stage the prefetched slice (rows past the chunk's end as "no pair"), start the accumulators, write the padding block
template <int TM, int COUT, int TS, int ITEM>
__device__ __forceinline__ void stage_chunk(const int (&pre)[kSliceRegs<TM>], int *s_list, int *s_pad, float *s_acc, const float *bias,
                                            const float *residual, int flags, int K, int row0, int n_rows) {
    const int tid = threadIdx.x;
    static_assert(256 % TM == 0, "a thread stages the same local row in every pass");
    const bool in_chunk = tid % TM < n_rows;
#pragma unroll
    for (int i = 0; i < kSliceRegs<TM>; ++i) {
        const int t = tid + i * 256;
        if (t < K * TM) s_list[t] = in_chunk ? pre[i] : -1;
    }
    init_acc<TM, COUT, TS>(s_acc, bias, residual, flags, row0, n_rows);
    if (tid < ITEM) s_pad[tid] = pad_entry(TM);
}

// ------------------------------------------------------------------------------------------------------ chunk plan
// A SubM rulebook is shared by the 4-5 convolutions of its level, and the compacted lists of a chunk depend on nothing but the
// rulebook and the chunk boundaries.  The chunk plan (chunk_plan_kernel in fd_spconv_v2.hip, one launch per rulebook) holds them
// ready-made in the rulebook's own shape, so that a kernel fetches a chunk's lists with the very code that fetches its rulebook slice:
//   rows 0 .. 26 of int [kPlanRows][plan_stride]: entry i of tap k's list of the chunk that starts at output row row0 is
//     plan[k][row0 + i], i < n_rows; entries past the tap's count are the padding entry (what compact_taps<128, 1> leaves in LDS);
//   row 27: the chunk's 27 pair counts as bytes, in the 8 words from plan[27][row0] (chunks start at multiples of 8 rows and
//     never share a block of 8: the equal-rows split cuts at multiples of 16, fd_spconv_ranges at multiples of 8).
// 128-row chunks with one row set (WR = 1) only: the 32 -> 32, 64 -> 64 and 128 -> 128 layers, and the strided 16 -> 32, 32 -> 64 and
// 64 -> 128 layers, whose plan comes straight from the index (index_plan_kernel) since nothing else reads their table.
constexpr int kPlanRows = kMaxTaps + 1;
constexpr int kPlanTM = 128;
constexpr int kPlanCountWords = (kMaxTaps + 3) / 4;
// host: words per plan row for n_out output rows (the count words of the last chunk end before n_out + 8)
inline int64_t plan_stride_for(int64_t n_out) { return (n_out + 8 + 63) / 64 * 64; }

// stage_chunk for a kernel that fetched its slice from the plan (fetch_slice with K = kPlanRows): the lists go to LDS as they are
// (positions past the chunk's rows belong to the next chunk: padding), the counts are unpacked; no compaction pass follows.
template <int TM, int COUT, int TS, int ITEM>
__device__ __forceinline__ void stage_plan_chunk(const int (&pre)[kSliceRegs<TM>], int *s_list, unsigned char *s_cnt, int *s_pad, float *s_acc,
                                                 const float *bias, const float *residual, int flags, int row0, int n_rows) {
    const int tid = threadIdx.x;
    static_assert(TM == kPlanTM && 256 % TM == 0, "the plan is cut for 128-row chunks");
    static_assert(kSliceRegs<TM> * 256 >= kMaxTaps * TM + kPlanCountWords, "the count words ride in the slice's last register");
    const bool in_chunk = tid % TM < n_rows;
#pragma unroll
    for (int i = 0; i < kSliceRegs<TM>; ++i) {
        const int t = tid + i * 256;
        if (t < kMaxTaps * TM) {
            s_list[t] = in_chunk ? pre[i] : pad_entry(TM);
        } else if (t < kMaxTaps * TM + kPlanCountWords) {
            const int k0 = (t - kMaxTaps * TM) * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (k0 + q < kMaxTaps) s_cnt[(k0 + q) * 4] = (unsigned char)((unsigned)pre[i] >> (8 * q));
        }
    }
    init_acc<TM, COUT, TS>(s_acc, bias, residual, flags, row0, n_rows);
    if (tid < ITEM) s_pad[tid] = pad_entry(TM);
}

// ------------------------------------------------------------------------------------------------------ compaction
// in place, per (tap, row set): wave w takes taps w, w + 4, ...; tails are filled with the padding entry
template <int TM, int WR>
__device__ __forceinline__ void compact_taps(int *s_list, unsigned char *s_cnt, int K) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int RW = TM / WR, NH = (RW + 63) / 64;
    for (int k = wave; k < K; k += 4) {
#pragma unroll
        for (int wr = 0; wr < WR; ++wr) {
            const int base = k * TM + wr * RW;
            int count = 0;
            int v[NH];
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int r = h * 64 + lane;
                v[h] = (r < RW) ? s_list[base + r] : -1;
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int r = h * 64 + lane;
                if (r < RW) s_list[base + r] = pad_entry(TM);
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int r = h * 64 + lane;
                const unsigned long long m = __ballot(v[h] >= 0);
                const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
                if (v[h] >= 0) s_list[base + pos] = pack_entry(v[h], wr * RW + r);
                count += __popcll(m);
            }
            if (lane == 0) s_cnt[k * 4 + wr] = (unsigned char)count;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- work list
// flattened work list of a wave (tap split ts, row set wr): one item = ITEM compacted pairs of one tap, code = (tap << 3) | group.
// Returns the number of items (wave-uniform, in a scalar register).
template <int TS, int ITEM>
__device__ __forceinline__ int build_items(const unsigned char *s_cnt, unsigned short *items, int K, int ts, int wr) {
    const int lane = threadIdx.x & 63;
    const int ng = (lane < K && (lane % TS) == ts) ? ((int)s_cnt[lane * 4 + wr] + ITEM - 1) / ITEM : 0;
    int inc = ng;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(inc, off);
        if (lane >= off) inc += u;
    }
    const int n_items = __builtin_amdgcn_readfirstlane(__shfl(inc, 63));
    for (int g = 0; g < ng; ++g) items[inc - ng + g] = (unsigned short)((lane << 3) | g);
    // wave-local LDS hand-off (items written above are read below by other lanes of the same wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return n_items;
}

// The two bookkeeping stages of the kernels' software pipelines (see the item loop of fd_spconv_v2.hip).
// stage A0: the item code of slot `it` (a slot past the end reads item 0; stage A1 discards it)
__device__ __forceinline__ int stage_a0(const unsigned short *items, int n_items, int it) { return (int)items[it < n_items ? it : 0]; }
// stage A1: the item's tap (-1 past the end) and the list entry of pair `lp` of the item
template <int TM, int WR, int ITEM>
__device__ __forceinline__ void stage_a1(const int *s_list, const int *s_pad, int n_items, int wr, int lp, int it, int code_v, int &kk, int &e) {
    const bool v = it < n_items;  // uniform (n_items is in a scalar register)
    const int code = __builtin_amdgcn_readfirstlane(code_v);
    const int ks = v ? (code >> 3) : 0;
    kk = v ? ks : -1;
    // past the end of the work list the (scalar) list pointer selects the block of padding entries: no per-lane select
    const int *lst = v ? s_list + ks * TM + wr * (TM / WR) + (code & 7) * ITEM : s_pad;
    e = lst[lp];
}

// A work list of at most 64 items (the 32-pair kernel's: 32) needs no LDS round trip per item: after build_items lane i holds code i
// in a register (one read per chunk), and stage A0 is a v_readlane with a scalar lane index: the code arrives in a scalar register.
template <int SLOT>
__device__ __forceinline__ int item_codes(const unsigned short *items) {
    static_assert(SLOT <= 64 && (SLOT & (SLOT - 1)) == 0, "one code per lane");
    return (int)items[threadIdx.x & (SLOT - 1)];
}
__device__ __forceinline__ int stage_a0_reg(int codes, int n_items, int it) { return __builtin_amdgcn_readlane(codes, it < n_items ? it : 0); }
// stage A1 on a code that is scalar already
template <int TM, int WR, int ITEM>
__device__ __forceinline__ void stage_a1_s(const int *s_list, const int *s_pad, int n_items, int wr, int lp, int it, int code, int &kk, int &e) {
    const bool v = it < n_items;
    const int ks = v ? (code >> 3) : 0;
    kk = v ? ks : -1;
    const int *lst = v ? s_list + ks * TM + wr * (TM / WR) + (code & 7) * ITEM : s_pad;
    e = lst[lp];
}

// -------------------------------------------------------------------------------------------------------- epilogue
// whole chunk, float4 per thread, rows contiguous in global memory (swizzled slots in LDS)
template <int TM, int COUT, int TS>
// `flags`: kFlagRelu, and whether `residual` / `out` are stored bank-spread
__device__ __forceinline__ void epilogue(float *s_acc, const float *bias, const float *residual, int flags,
                                         float *out, int row0, int n_rows) {
    const int tid = threadIdx.x;
    constexpr int C4 = COUT / 4;
    for (int t = tid; t < n_rows * C4; t += 256) {
        const int r = t / C4, c4 = t - r * C4;
        const int row = row0 + r;
        const int slot = acc_slot<COUT>(r, c4);
        float4 v = reinterpret_cast<const float4 *>(s_acc)[slot];
#pragma unroll
        for (int q = 1; q < TS; ++q) {
            const float4 v2 = reinterpret_cast<const float4 *>(s_acc + q * acc_copy_floats(TM, COUT))[slot];
            v.x += v2.x; v.y += v2.y; v.z += v2.z; v.w += v2.w;
        }
        if constexpr (!kInitAcc<COUT>) {
            if (bias) {
                const float4 bv = reinterpret_cast<const float4 *>(bias)[c4];
                v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            }
            if (residual) {
                const float4 rv = reinterpret_cast<const float4 *>(residual + (int64_t)row * COUT)[swz_col4<COUT>(c4, row, flags & kFlagResidualSwz)];
                v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
            }
        }
        if (flags & kFlagRelu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        reinterpret_cast<float4 *>(out + (int64_t)row * COUT)[swz_col4<COUT>(c4, row, flags & kFlagOutSwz)] = v;
    }
}

}  // namespace skeleton
}  // namespace fd
