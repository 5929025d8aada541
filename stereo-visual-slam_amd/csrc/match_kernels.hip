// match_kernels.hip -- K7: brute-force cross-checked Hamming matcher + distance gate.
//
// Replaces cv::BFMatcher(NORM_HAMMING, crossCheck=true)::match + the gate of VO::feature_matching
// (/root/reference/src/stereo_visual_slam_main/visual_odometry.cpp:219-251).  Semantics (OpenCV 3.2
// batchDistance with crosscheck): (i) every TRAIN row j takes its nearest QUERY row i*(j), first minimum in
// ascending i; (ii) for j ascending, query i*(j) takes train j if d < dist[i*].  Both steps are order-free
// minima of packed keys, so they map to atomicMin without changing the result:
//   step (i)  : key = d << 16 | i   -> min over i  = smallest d, then smallest i   (first minimum)
//   step (ii) : key = d << 16 | j   -> min over {j : i*(j) = i} = smallest d, then smallest j (strict '<').
//
// gfx950 mapping.  The all-pairs Hamming table is the one dense contraction of the pipeline: with the descriptor bits
// recoded as +-1, <a, b> = 256 - 2 hamming(a, b).  +-1 is exact in FP4 (e2m1: 0x2 / 0xA), so a 32 x 32 block of distances is four
// v_mfma_f32_32x32x64_f8f6f4 with FP4 operands (four VGPRs each; 32.5 cycles per instruction, the cycles of v_mfma_i32_32x32x32_i8 at
// twice the K -- tools/scratch/mfma_fp4_layout.hip), exact in the f32 accumulator.  The +-1 form never exists in HBM:
// `match_train_nearest_kernel` reads the raw 32-B descriptors and expands bits to nibbles in registers (a shift and a masked merge per operand
// dword) -- the 128 train columns of a wave once, into the 64 VGPRs that stay resident as MFMA B operands; every 32-row query tile
// cooperatively (one dword -> 16 bytes per thread) on its way into LDS (row stride 144 B: conflict-free ds_read_b128), shared by the four
// waves of the workgroup.  The fold needs no key arithmetic: the tie-break enters as the C operand of a tile's first MFMA
// (C = (31 - local row) * 2^-12), so the accumulator IS the key dot + row fraction (largest dot, then smallest row; exact in f32, see the
// kernel's comment) and the column maxima are v_max3_f32 over the accumulator registers, two values per instruction.
// 164 VGPRs, no scratch: three waves per SIMD.  (Before: eight v_mfma_i32_32x32x32_i8 per block on +-1 bytes and v_lshl_add + v_max per value
// on packed integer keys, 219 VGPRs, 0.50 ms per 1024 items of 1500 x 1500; now 0.20 ms.)
#include "vslam_internal.h"

namespace vslam {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// 32 descriptor bits -> 32 e2m1 nibbles of +-1 (bit clear -> 0x2 = +1, set -> 0xA = -1) = the 16 operand bytes of one lane for one
// K = 64 step.  Operand dword i, nibble n holds bit 4 n + i: a shift and a masked merge per dword.  (A Hamming dot product does not care
// which k a bit lands on, only that the query side and the train side agree -- both go through this function.)
__device__ inline v4i expand32(uint32_t x) {
    return v4i{(int)(((x << 3) & 0x88888888u) | 0x22222222u), (int)(((x << 2) & 0x88888888u) | 0x22222222u),
               (int)(((x << 1) & 0x88888888u) | 0x22222222u), (int)((x & 0x88888888u) | 0x22222222u)};
}
// one K = 64 step of a 32 x 32 block: FP4 operands (cbsz = blgp = 4, four VGPRs each).  kBlockScale = 0 on both sides selects the instruction's
// form without block scales, v_mfma_f32_32x32x64_f8f6f4 (products unscaled; half the encoding and no scale VGPR); 0x7F7F7F7F would be the scaled form
// with E8M0 127 = 2^0.  tools/scratch/mfma_fp4_layout.hip checks both on the device.
constexpr int kBlockScale = 0;
__device__ inline v16f mma_fp4(v4i a, v4i b, v16f c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{a[0], a[1], a[2], a[3], 0, 0, 0, 0}, v8i{b[0], b[1], b[2], b[3], 0, 0, 0, 0}, c, 4, 4, 0,
                                                           kBlockScale, 0, kBlockScale);
}

// threadIdx.x behind a compiler barrier: lane arithmetic that is needed only after (or rarely inside) the tile loop is recomputed from it there
// instead of staying in registers across the loop -- the loop runs at the 168-VGPR limit of three waves per SIMD
__device__ inline int fresh_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

constexpr int kMatchBlock = 256;             // 4 waves
constexpr int kColTiles = 4;                 // 32-column MFMA tiles per wave held in registers (one A read from LDS feeds four tiles)
constexpr int kColsPerWave = 32 * kColTiles;
constexpr int kColsPerBlock = (kMatchBlock / 64) * kColsPerWave;
constexpr int kQRows = 32;                   // query rows per LDS tile
constexpr int kQStride = 144;                // bytes per staged query row (128 + 16: conflict-free 16-B reads)
constexpr float kRowUnit = 1.f / 4096.f;     // one row of tie-break in the f32 key (kMaxRows = 4096 rows fit the 12 fraction bits)
constexpr float kNoRow = -4194304.f;         // C of a row past nq: dot + kNoRow is exact and below every real key
static_assert(kMaxRows <= 4096, "the f32 key holds the row in 12 fraction bits");

// Work items are numbered column-block-major (w = (colblock * qsplit + split) * B + item): the items' live column blocks
// come first in the grid and spread evenly over the XCDs / CUs, the blocks beyond an item's train rows (capacity padding)
// sit at the end and exit at once.  (With the item as the slow index the live blocks of every item landed on the same few XCDs.)
// kSel (vslam_feature_matching_subset_dev): the query set of item b is the ascending row list d_qsel[b][0 .. d_nqsel[b]).  The list is COMPACTED on the
// way into LDS -- staged tile row r is Q[qsel[r]] -- so a selection of n rows costs n / 32 tiles, the MFMA / fold path is untouched (the exact
// 256 - 2 hamming identity holds) and the packed key carries the row's RANK in the list; match_finalize_kernel maps rank -> row.  The list ascends,
// so ascending rank = ascending original row and the first-minimum tie rule is the unmasked kernel's.
// d_qitem (vslam_feature_matching_pairs_dev; null: item b's own block): the QUERY side of item b -- descriptor block, d_nq entry, d_qsel row and
// d_nqsel entry -- is block d_qitem[b] of n_qitems; the train side, d_gap and the outputs stay item b's.  An index outside [0, n_qitems) empties the
// item.  One uniform load ahead of the address arithmetic: the resident operands, the tile pipeline and the register budget are untouched.
//
// The f32 key.  Within the tiles tile0 .. tile1 - 1 of this workgroup, row i (of tile T, local row i % 32) competes with
//   key = dot + (32 (tile1 - T) - 1 - i % 32) * 2^-12 = dot + (32 tile1 - 1 - i) * 2^-12:  largest dot, then smallest row;
// |dot| <= 256 and the fraction has 12 bits, so every key is exact in f32 and distinct per row.  The MFMA forms it: the first instruction of a
// tile takes C = (31 - i % 32) * 2^-12 (constant per lane and register), and the running maxima gain 32 * 2^-12 before each tile.
template <bool kSel>
__global__ __launch_bounds__(kMatchBlock, 3) void match_train_nearest_kernel(
    const uint8_t* __restrict__ d_q, size_t q_stride, const int32_t* __restrict__ d_nq, const uint8_t* __restrict__ d_t, size_t t_stride,
    const int32_t* __restrict__ d_nt, int max_rows, int qsplit, int B, uint32_t* __restrict__ d_train_best, const int32_t* __restrict__ d_qsel,
    int sel_cap, const int32_t* __restrict__ d_nqsel, const int32_t* __restrict__ d_qitem, int n_qitems) {
    const int w = blockIdx.x;
    const int b = w % B, split = (w / B) % qsplit, cb = w / (B * qsplit);
    const int qb = d_qitem ? d_qitem[b] : b; // the block the query side comes from
    if (d_qitem && (qb < 0 || qb >= n_qitems)) return;
    const int nrows = min(d_nq[qb], max_rows), nt = min(d_nt[b], max_rows);
    const int nq = kSel ? min(max(d_nqsel[qb], 0), min(sel_cap, nrows)) : nrows; // the rows that compete: all of them, or the selection's length
    const int32_t* sel = kSel ? d_qsel + (size_t)qb * sel_cap : nullptr;
    const int c0 = cb * kColsPerBlock;
    if (c0 >= nt || nq <= 0) return;
    // query range of this split, in whole tiles
    const int ntiles = (nq + kQRows - 1) / kQRows, per = (ntiles + qsplit - 1) / qsplit;
    const int tile0 = split * per, tile1 = min(ntiles, tile0 + per);
    if (tile0 >= tile1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    __shared__ alignas(16) int8_t sq[2][kQRows * kQStride];
    const uint8_t* Q = d_q + (size_t)qb * q_stride;
    const uint8_t* T = d_t + (size_t)b * t_stride;
    // B operands: this wave's 128 train columns, expanded once and resident for the whole kernel.  K step s of lane (r, h) holds
    // dword 4 h + s of the descriptor (one 16-B load per column and lane).
    v4i breg[kColTiles][4];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) {
        const int j = min(c0 + wave * kColsPerWave + 32 * t + r, nt - 1);
        const uint4 d = *reinterpret_cast<const uint4*>(T + (size_t)j * 32 + 16 * h);
        breg[t][0] = expand32(d.x); breg[t][1] = expand32(d.y); breg[t][2] = expand32(d.z); breg[t][3] = expand32(d.w);
    }
    // staging: a tile is 32 rows x 8 dwords of raw descriptor = one dword per thread, expanded to 16 operand bytes into LDS
    const int srow = threadIdx.x >> 3, sword = threadIdx.x & 7;
    auto gload = [&](int tile, uint32_t& x) {
        int r0 = min(tile * kQRows + srow, nq - 1);
        if (kSel) r0 = min(max(sel[r0], 0), nrows - 1); // rank -> row (the clamp keeps a list that breaks the precondition inside the item)
        x = *reinterpret_cast<const uint32_t*>(Q + ((uint32_t)r0 * 32u + (uint32_t)sword * 4u)); // (32-bit offset from the item's base)
    };
    auto sstore = [&](int buf, uint32_t x) { *reinterpret_cast<v4i*>(&sq[buf][srow * kQStride + sword * 16]) = expand32(x); };
    // tie-break C of this lane's 16 accumulator slots (slot v = local row 8 (v / 4) + v % 4 + 4 h)
    v16f ctie;
#pragma unroll
    for (int v = 0; v < 16; ++v) ctie[v] = (float)(31 - (8 * (v / 4) + (v % 4) + 4 * h)) * kRowUnit;
    uint32_t x;
    gload(tile0, x);
    sstore(0, x);
    if (tile0 + 1 < tile1) gload(tile0 + 1, x);
    __syncthreads();
    float m[kColTiles];
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) m[t] = -INFINITY;
    // four column tiles per wave: one set of accumulators; a query tile read from LDS once feeds 16 MFMAs; the other waves of the SIMD
    // fill the MFMA pipe while this one folds
    v16f acc[kColTiles];
    for (int tile = tile0; tile < tile1; ++tile) {
        const int buf = (tile - tile0) & 1;
        if (tile + 1 < tile1) { sstore(buf ^ 1, x); if (tile + 2 < tile1) gload(tile + 2, x); } // (buffer buf ^ 1 was released by the barrier below)
        if (tile * kQRows + kQRows > nq) { // the item's last, partial tile (nothing follows it): rows >= nq must not compete
            const int row0 = tile * kQRows + 4 * ((fresh_tid() >> 5) & 1);
#pragma unroll
            for (int v = 0; v < 16; ++v)
                if (row0 + 8 * (v / 4) + (v % 4) >= nq) ctie[v] = kNoRow;
        }
        v4i a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = *reinterpret_cast<const v4i*>(&sq[buf][r * kQStride + (4 * h + s) * 16]);
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) acc[t] = mma_fp4(a[0], breg[t][0], ctie);
#pragma unroll
        for (int s = 1; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < kColTiles; ++t) acc[t] = mma_fp4(a[s], breg[t][s], acc[t]);
        // fold: the accumulators ARE the keys -- one v_max3_f32 per two values
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            float mm = m[t] + 32.f * kRowUnit;
#pragma unroll
            for (int v = 0; v < 16; v += 2) mm = __builtin_fmaxf(__builtin_fmaxf(acc[t][v], acc[t][v + 1]), mm);
            m[t] = mm;
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < kColTiles; ++t) m[t] = __builtin_fmaxf(m[t], __shfl_xor(m[t], 32));
    const int tid = fresh_tid();
    if ((tid & 32) == 0) {
#pragma unroll
        for (int t = 0; t < kColTiles; ++t) {
            const float mm = m[t];
            const int j = c0 + (tid >> 6) * kColsPerWave + 32 * t + (tid & 31);
            if (j < nt && mm >= -256.f) {
                const float fl = __builtin_floorf(mm); // = dot; the fraction is (32 tile1 - 1 - row) * 2^-12
                const uint32_t d = (uint32_t)(256 - (int)fl) >> 1, i = (uint32_t)(32 * tile1 - 1 - (int)((mm - fl) * 4096.f));
                const uint32_t key = (d << 16) | i;
                if (qsplit == 1) d_train_best[(size_t)b * max_rows + j] = key;
                else atomicMin(&d_train_best[(size_t)b * max_rows + j], key);
            }
        }
    }
}

// ordered compaction helper: returns the exclusive rank of `flag` among the block's threads, and the block total
__device__ inline int block_rank(bool flag, int* s_wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave_tot[wave] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int c = s_wave_tot[w];
        if (w < wave) base += c;
        tot += c;
    }
    total = tot;
    return base + rank;
}

constexpr int kFinBlock = 1024;

__global__ __launch_bounds__(kFinBlock) void match_finalize_kernel(
    const int32_t* __restrict__ d_nq, const int32_t* __restrict__ d_nt, const double* __restrict__ d_gap, int gate,
    double ratio, double gap_thr, int max_rows, const uint32_t* __restrict__ d_train_best, vslam_dmatch* __restrict__ d_out,
    int out_capacity, int32_t* __restrict__ d_nout, const int32_t* __restrict__ d_qsel, int sel_cap, const int32_t* __restrict__ d_nqsel,
    const int32_t* __restrict__ d_qitem, int n_qitems) {
    const int b = blockIdx.x;
    const int qraw = d_qitem ? d_qitem[b] : b;
    const bool live = !d_qitem || (qraw >= 0 && qraw < n_qitems); // (an item without a query block: nq = 0, d_nout[b] = 0)
    const int qb = live ? qraw : 0;
    const int nrows = live ? min(d_nq[qb], max_rows) : 0, nt = min(d_nt[b], max_rows);
    // a selection (d_qsel non-null): the keys carry ranks in the list, nq is its length and queryIdx is the list's entry
    const int32_t* sel = d_qsel ? d_qsel + (size_t)qb * sel_cap : nullptr;
    const int nq = sel ? min(max(d_nqsel[qb], 0), min(sel_cap, nrows)) : nrows;
    __shared__ uint32_t qbest[kMaxRows];
    __shared__ int s_wave_tot[kFinBlock / 64];
    __shared__ uint32_t s_min[kFinBlock / 64];
    for (int i = threadIdx.x; i < kMaxRows; i += kFinBlock) qbest[i] = 0xFFFFFFFFu;
    __syncthreads();
    if (nq > 0)
        for (int j = threadIdx.x; j < nt; j += kFinBlock) {
            const uint32_t key = d_train_best[(size_t)b * max_rows + j];
            if (key != 0xFFFFFFFFu) atomicMin(&qbest[key & 0xFFFFu], (key & 0xFFFF0000u) | (uint32_t)j);
        }
    __syncthreads();
    // d_min over the matches (visual_odometry.cpp:229-234)
    uint32_t dmin = 0xFFFFu;
    for (int i = threadIdx.x; i < nq; i += kFinBlock) {
        const uint32_t key = qbest[i];
        if (key != 0xFFFFFFFFu) dmin = min(dmin, key >> 16);
    }
    for (int o = 32; o > 0; o >>= 1) dmin = min(dmin, (uint32_t)__shfl_xor((int)dmin, o));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = dmin;
    __syncthreads();
    dmin = 0xFFFFu;
    for (int w = 0; w < kFinBlock / 64; ++w) dmin = min(dmin, s_min[w]);
    // threshold (visual_odometry.cpp:242), evaluated in double like the reference
    const double a = ratio * (double)(float)dmin, g = gap_thr * d_gap[b];
    const double thr = a > g ? a : g;
    vslam_dmatch* out = d_out + (size_t)b * out_capacity;
    int written = 0;
    for (int base = 0; base < nq; base += kFinBlock) {
        const int i = base + threadIdx.x;
        uint32_t key = 0xFFFFFFFFu;
        if (i < nq) key = qbest[i];
        bool keep = key != 0xFFFFFFFFu;
        const uint32_t d = key >> 16;
        if (keep && gate) keep = (double)(float)d <= thr;
        int total;
        const int r = block_rank(keep, s_wave_tot, total);
        if (keep && written + r < out_capacity) {
            vslam_dmatch m;
            m.queryIdx = sel ? sel[i] : i; m.trainIdx = (int)(key & 0xFFFFu); m.imgIdx = 0; m.distance = (float)d;
            out[written + r] = m;
        }
        written += total;
    }
    if (threadIdx.x == 0) d_nout[b] = min(written, out_capacity);
}

int launch_match(const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, const uint8_t* d_t, size_t t_stride,
                 const int32_t* d_nt, const double* d_gap, int gate, double ratio, double gap_thr, int B, int max_rows,
                 uint32_t* d_train_best, vslam_dmatch* d_out, int out_capacity, int32_t* d_nout, hipStream_t stream, const int32_t* d_qsel, int sel_cap,
                 const int32_t* d_nqsel, const int32_t* d_qitem, int n_qitems) {
    if (B <= 0) return VSLAM_OK;
    if (max_rows > kMaxRows || max_rows <= 0) { set_error("matcher: max_rows %d out of range (<= %d)", max_rows, kMaxRows); return VSLAM_ERR_ARG; }
    // fill the chip: ~>= 1024 workgroups.  Split the query range when the batch is small.
    const int tblocks = (max_rows + kColsPerBlock - 1) / kColsPerBlock;
    int qsplit = 1;
    while (qsplit < 16 && (long)tblocks * qsplit * B < 1024 && max_rows / (qsplit * 2) >= 4 * kQRows) qsplit *= 2;
    // every in-range train row is written exactly once when the query range is not split
    if (qsplit > 1) VS_HIP(hipMemsetAsync(d_train_best, 0xFF, (size_t)B * max_rows * sizeof(uint32_t), stream));
    if (d_qsel) {
        ProfScope prof__(stream, "match_train_nearest_sel_kernel");
        hipLaunchKernelGGL(match_train_nearest_kernel<true>, dim3(tblocks * qsplit * B), dim3(kMatchBlock), 0, stream, d_q, q_stride, d_nq, d_t, t_stride,
                           d_nt, max_rows, qsplit, B, d_train_best, d_qsel, sel_cap, d_nqsel, d_qitem, n_qitems);
    } else {
        ProfScope prof__(stream, "match_train_nearest_kernel");
        hipLaunchKernelGGL(match_train_nearest_kernel<false>, dim3(tblocks * qsplit * B), dim3(kMatchBlock), 0, stream, d_q, q_stride, d_nq, d_t, t_stride,
                           d_nt, max_rows, qsplit, B, d_train_best, nullptr, 0, nullptr, d_qitem, n_qitems);
    }
    ProfScope prof__(stream, "match_finalize_kernel");
    hipLaunchKernelGGL(match_finalize_kernel, dim3(B), dim3(kFinBlock), 0, stream, d_nq, d_nt, d_gap, gate, ratio, gap_thr,
                       max_rows, d_train_best, d_out, out_capacity, d_nout, d_qsel, sel_cap, d_nqsel, d_qitem, n_qitems);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
