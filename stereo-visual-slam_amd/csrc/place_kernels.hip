// place_kernels.hip -- loop-closure detection: a database of keyframe descriptor blocks and the place score between its entries
// (include/vslam_hip.h "place database").
//
//   score(i, j) = #{ r < n_i : min_c hamming(D_i[r], D_j[c]) <= tau },   -1 for a pair that is not eligible, 0 when n_j = 0.
//
// The arithmetic is the matcher's (match_kernels.hip): descriptor bits recoded to +-1 in FP4 inside the kernel, <a, b> = 256 - 2 hamming(a, b), four
// v_mfma_f32_32x32x64_f8f6f4 per 32 x 32 block, exact in f32; "nearest <= tau" is "largest dot >= 256 - 2 tau".  The +-1 form never exists in HBM.
// What differs is the blocking.  The matcher serves one pair per item; here one query entry meets every database entry, so a workgroup expands 512 rows
// of ITS QUERY ENTRY once (four waves x four 32-column MFMA tiles = 64 VGPRs per lane of B operands, resident for the whole kernel: the expanded form
// of 1500 rows would be 192 KB, more than the LDS; 500 rows are one workgroup) and the database entries stream past it as A operands: 32-row tiles,
// expanded on their way into LDS (row stride 144 B, double buffered), one continuous tile stream across entry boundaries.  A tile's sixteen
// accumulator registers per lane are rows of the DATABASE entry, so the maximum over them (v_max3_f32) followed by one exchange between the lane halves
// at the end of an entry is every query row's largest dot: per pair only a count of lanes survives.  No match list, no cross-check, no keys.
// Padding: a partial tile repeats the entry's last row (a repeated row changes no maximum); query rows past n_i are staged the same way and never
// counted.  Counts of a query's column blocks (n_i > 512) meet in the table by integer atomicAdd on the zero the init kernel wrote: exact in any order.
#include <algorithm>

#include "vslam_internal.h"

namespace vslam {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// (match_kernels.hip's expand32 / mma_fp4: both operands of a dot go through the same recoding)
__device__ inline v4i place_expand32(uint32_t x) {
    return v4i{(int)(((x << 3) & 0x88888888u) | 0x22222222u), (int)(((x << 2) & 0x88888888u) | 0x22222222u),
               (int)(((x << 1) & 0x88888888u) | 0x22222222u), (int)((x & 0x88888888u) | 0x22222222u)};
}
__device__ inline v16f place_mma_fp4(v4i a, v4i b, v16f c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{a[0], a[1], a[2], a[3], 0, 0, 0, 0}, v8i{b[0], b[1], b[2], b[3], 0, 0, 0, 0}, c, 4, 4, 0, 0, 0, 0);
}

constexpr int kPlaceBlock = 256;             // 4 waves
constexpr int kPlaceColTiles = 4;            // 32-column MFMA tiles per wave: the query rows a wave keeps in registers
constexpr int kPlaceColsPerWave = 32 * kPlaceColTiles;
constexpr int kPlaceColsPerBlock = (kPlaceBlock / 64) * kPlaceColsPerWave;
constexpr int kPlaceRows = 32;               // database rows per LDS tile
constexpr int kPlaceStride = 144;            // bytes per staged row (128 + 16: conflict-free 16-B reads)

__device__ inline bool place_eligible(const PlaceView& v, int sq, int fq, int min_gap, int j) {
    return v.seq[j] == sq && (long long)v.frame[j] <= (long long)fq - (long long)min_gap;
}

// -1 for a pair that is not eligible, 0 for one that is: the score kernel adds its counts to the zeros
__global__ __launch_bounds__(256) void place_score_init_kernel(PlaceView v, int q0, int nq, int min_gap, int32_t* __restrict__ d_score, int ld) {
    const int i = blockIdx.y;
    const int sq = v.seq[q0 + i], fq = v.frame[q0 + i];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < v.n_entries; j += gridDim.x * 256)
        d_score[(size_t)i * ld + j] = place_eligible(v, sq, fq, min_gap, j) ? 0 : -1;
}

// the tile stream of a workgroup: entry j in [j, j1) that is eligible and not empty, tile of ntiles
struct PlaceCursor { int j, tile, ntiles, n; };

__device__ inline void place_seek(const PlaceView& v, int sq, int fq, int min_gap, int j1, PlaceCursor& c) { // first entry at or after c.j that has work
    c.tile = 0;
    for (; c.j < j1; ++c.j) {
        if (!place_eligible(v, sq, fq, min_gap, c.j)) continue;
        c.n = min(max(v.n[c.j], 0), v.rows);
        if (c.n > 0) { c.ntiles = (c.n + kPlaceRows - 1) / kPlaceRows; return; }
    }
    c.n = 0; c.ntiles = 0;
}
__device__ inline void place_advance(const PlaceView& v, int sq, int fq, int min_gap, int j1, PlaceCursor& c) {
    if (c.j >= j1) return;
    if (++c.tile < c.ntiles) return;
    ++c.j;
    place_seek(v, sq, fq, min_gap, j1, c);
}

// grid: x = query entry (of nq), y = column block of the query's rows, z = slice of the database entries
__global__ __launch_bounds__(kPlaceBlock, 3) void place_score_kernel(PlaceView v, int q0, int thr_dot, int min_gap, int per_slice, int32_t* __restrict__ d_score, int ld) {
    const int qi = blockIdx.x, e = q0 + qi;
    const int ni = min(max(v.n[e], 0), v.rows);
    const int c0 = blockIdx.y * kPlaceColsPerBlock;
    if (c0 >= ni) return;
    const int j0 = blockIdx.z * per_slice, j1 = min(v.n_entries, j0 + per_slice);
    const int sq = v.seq[e], fq = v.frame[e];
    PlaceCursor cur{j0, 0, 0, 0};
    place_seek(v, sq, fq, min_gap, j1, cur);
    if (cur.j >= j1) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    __shared__ alignas(16) int8_t sq_tile[2][kPlaceRows * kPlaceStride];
    const size_t entry_bytes = (size_t)v.stride_rows * 32;
    // B operands: this wave's 128 query rows, expanded once.  K step s of lane (r, h) holds dword 4 h + s of the descriptor.
    const uint8_t* Q = v.desc + (size_t)e * entry_bytes;
    v4i breg[kPlaceColTiles][4];
#pragma unroll
    for (int t = 0; t < kPlaceColTiles; ++t) {
        const int col = min(c0 + wave * kPlaceColsPerWave + 32 * t + r, ni - 1);
        const uint4 d = *reinterpret_cast<const uint4*>(Q + (size_t)col * 32 + 16 * h);
        breg[t][0] = place_expand32(d.x); breg[t][1] = place_expand32(d.y); breg[t][2] = place_expand32(d.z); breg[t][3] = place_expand32(d.w);
    }
    const bool wave_live = c0 + wave * kPlaceColsPerWave < ni;   // (a wave whose columns are all padding still stages tiles and meets the barriers)
    // staging: a tile is 32 rows x 8 dwords of raw descriptor = one dword per thread, expanded to 16 operand bytes into LDS
    const int srow = threadIdx.x >> 3, sword = threadIdx.x & 7;
    auto gload = [&](const PlaceCursor& c, uint32_t& x) {
        const int row = min(c.tile * kPlaceRows + srow, c.n - 1);   // (a partial tile repeats the last row: no maximum changes)
        x = *reinterpret_cast<const uint32_t*>(v.desc + (size_t)c.j * entry_bytes + ((uint32_t)row * 32u + (uint32_t)sword * 4u));
    };
    auto sstore = [&](int buf, uint32_t x) { *reinterpret_cast<v4i*>(&sq_tile[buf][srow * kPlaceStride + sword * 16]) = place_expand32(x); };
    // pipeline: LDS holds the tile at `cur`, register x the tile at `nxt`, and the load of the tile at `ahead` is issued while `cur` computes
    PlaceCursor nxt = cur;
    place_advance(v, sq, fq, min_gap, j1, nxt);
    PlaceCursor ahead = nxt;
    uint32_t x = 0;
    gload(cur, x);
    sstore(0, x);
    if (nxt.j < j1) gload(nxt, x);
    __syncthreads();
    const float thr = (float)thr_dot;
    float m[kPlaceColTiles];
#pragma unroll
    for (int t = 0; t < kPlaceColTiles; ++t) m[t] = -1024.f;
    const v16f zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    while (cur.j < j1) {
        if (nxt.j < j1) {   // (buffer buf ^ 1 was released by the barrier that ended the previous tile)
            sstore(buf ^ 1, x);
            ahead = nxt;
            place_advance(v, sq, fq, min_gap, j1, ahead);
            if (ahead.j < j1) gload(ahead, x);
        }
        if (wave_live) {
            v4i a[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = *reinterpret_cast<const v4i*>(&sq_tile[buf][r * kPlaceStride + (4 * h + s) * 16]);
            v16f acc[kPlaceColTiles];
#pragma unroll
            for (int t = 0; t < kPlaceColTiles; ++t) acc[t] = place_mma_fp4(a[0], breg[t][0], zero);
#pragma unroll
            for (int s = 1; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < kPlaceColTiles; ++t) acc[t] = place_mma_fp4(a[s], breg[t][s], acc[t]);
            // fold: the largest dot of every query row (= lane column) over this tile's database rows (= accumulator registers)
#pragma unroll
            for (int t = 0; t < kPlaceColTiles; ++t) {
                float mm = m[t];
#pragma unroll
                for (int k = 0; k < 16; k += 2) mm = __builtin_fmaxf(__builtin_fmaxf(acc[t][k], acc[t][k + 1]), mm);
                m[t] = mm;
            }
            if (cur.tile + 1 == cur.ntiles) {   // the entry's last tile: count the query rows whose nearest is within tau
                int cnt = 0;
#pragma unroll
                for (int t = 0; t < kPlaceColTiles; ++t) {
                    const float mm = __builtin_fmaxf(m[t], __shfl_xor(m[t], 32));
                    const bool hit = h == 0 && c0 + wave * kPlaceColsPerWave + 32 * t + r < ni && mm >= thr;
                    cnt += __popcll(__ballot(hit));
                    m[t] = -1024.f;
                }
                if (lane == 0 && cnt > 0) atomicAdd(&d_score[(size_t)qi * ld + cur.j], cnt);
            }
        }
        __syncthreads();
        cur = nxt; nxt = ahead; buf ^= 1;
    }
}

// ordered compaction helper: the exclusive rank of `flag` among the block's threads, and the block total
__device__ inline int place_block_rank(bool flag, int* s_wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const unsigned long long mk = __ballot(flag);
    const int rank = __popcll(mk & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave_tot[wave] = __popcll(mk);
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

// item b of the batch -> entry d_dst[b] (< 0: not added): descriptor rows (the tail of the block zeroed) and n / seq / frame
__global__ __launch_bounds__(256) void place_add_kernel(PlaceView v, const int32_t* __restrict__ d_dst, const uint8_t* __restrict__ d_desc, size_t desc_stride,
                                                        const int32_t* __restrict__ d_n, const int32_t* __restrict__ d_seq, const int32_t* __restrict__ d_frame) {
    const int b = blockIdx.x, e = d_dst[b];
    if (e < 0 || e >= v.capacity) return;
    const int n = min(max(d_n[b], 0), v.rows);
    const uint4* src = reinterpret_cast<const uint4*>(d_desc + (size_t)b * desc_stride);
    uint4* dst = reinterpret_cast<uint4*>(v.desc + (size_t)e * v.stride_rows * 32);
    for (int k = threadIdx.x; k < v.stride_rows * 2; k += 256) dst[k] = k < n * 2 ? src[k] : uint4{0u, 0u, 0u, 0u};
    if (threadIdx.x == 0) { v.n[e] = n; v.seq[e] = d_seq[b]; v.frame[e] = d_frame[b]; }
}

// ... and, with geometry, the keypoints' pixels, points, valid flags and the ascending list of the rows that own a valid point
// (eleven table pointers: the SGPR cap keeps the kernel inside the eight-wave budget of DESIGN.md 5.6)
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(72))) void place_add_geometry_kernel(float2* __restrict__ o_xy, float* __restrict__ o_xyz, uint8_t* __restrict__ o_valid,
                                                                 int32_t* __restrict__ o_qsel, int32_t* __restrict__ o_nqsel, int rows, int capacity,
                                                                 const int32_t* __restrict__ d_dst, const int32_t* __restrict__ d_n,
                                                                 const vslam_keypoint* __restrict__ d_kps, const float* __restrict__ d_xyz,
                                                                 const uint8_t* __restrict__ d_valid, int kp_capacity) {
    const int b = blockIdx.x, e = d_dst[b];
    if (e < 0 || e >= capacity) return;
    __shared__ int s_wave_tot[4];
    const int ng = min(min(max(d_n[b], 0), rows), kp_capacity);   // (rows past the caller's keypoint capacity own no point)
    int written = 0;
    for (int base = 0; base < rows; base += 256) {
        const int k = base + threadIdx.x;
        bool ok = false;
        if (k < rows) {
            float2 xy = {0.f, 0.f}; float px = 0.f, py = 0.f, pz = 0.f;
            if (k < ng) {
                const size_t s = (size_t)b * kp_capacity + k;
                xy = float2{d_kps[s].x, d_kps[s].y}; px = d_xyz[3 * s]; py = d_xyz[3 * s + 1]; pz = d_xyz[3 * s + 2];
                ok = d_valid[s] != 0;
            }
            const size_t o = (size_t)e * rows + k;
            o_xy[o] = xy; o_xyz[3 * o] = px; o_xyz[3 * o + 1] = py; o_xyz[3 * o + 2] = pz; o_valid[o] = ok ? 1 : 0;
        }
        int total;
        const int rk = place_block_rank(ok, s_wave_tot, total);
        if (ok) o_qsel[(size_t)e * rows + written + rk] = k;
        written += total;
    }
    if (threadIdx.x == 0) o_nqsel[e] = written;
}

// per query the K eligible entries with the highest score that reach min_score: descending score, ties to the smaller entry id; unused slots -1 / 0.
// K rounds of an arg-max over key = score << 32 | (2^31 - 1 - id), each below the previous round's key.
__global__ __launch_bounds__(256) void place_select_kernel(int n_entries, const int32_t* __restrict__ d_score, int ld, int K, int min_score,
                                                           int32_t* __restrict__ d_cand, int32_t* __restrict__ d_cand_score) {
    const int i = blockIdx.x;
    const int32_t* row = d_score + (size_t)i * ld;
    __shared__ long long s_best[4];
    const int floor_score = max(min_score, 0);   // (a pair that is not eligible holds -1)
    long long prev = 0x7FFFFFFFFFFFFFFFll;
    for (int k = 0; k < K; ++k) {
        long long best = -1;
        for (int j = threadIdx.x; j < n_entries; j += 256) {
            const int s = row[j];
            if (s < floor_score) continue;
            const long long key = ((long long)s << 32) | (long long)(0x7FFFFFFF - j);
            if (key < prev && key > best) best = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        __syncthreads();   // (s_best of the previous round has been read)
        if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
        __syncthreads();
        best = s_best[0];
        for (int w = 1; w < 4; ++w) best = s_best[w] > best ? s_best[w] : best;
        if (threadIdx.x == 0) {
            d_cand[(size_t)i * K + k] = best < 0 ? -1 : 0x7FFFFFFF - (int)(best & 0xFFFFFFFFll);
            d_cand_score[(size_t)i * K + k] = best < 0 ? 0 : (int)(best >> 32);
        }
        prev = best;   // (-1 once the eligible entries are used up: nothing is below it)
    }
}

// verification, before the matcher: item b's query block = its rank-`rank` candidate (-1 when there is none or it is out of range), gap 1.0
__global__ __launch_bounds__(256) void place_verify_prep_kernel(int n_entries, int nq, const int32_t* __restrict__ d_cand, int K, int rank, int32_t* __restrict__ d_qitem,
                                                                double* __restrict__ d_gap) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nq) return;
    const int c = d_cand[(size_t)b * K + rank];
    d_qitem[b] = (c >= 0 && c < n_entries) ? c : -1;
    d_gap[b] = 1.0;
}

// verification, between the matcher and RANSAC: in match order, (point of candidate c at queryIdx, pixel of the query entry at trainIdx).  An item
// without a candidate, or with fewer matches than min_inliers (it cannot be accepted), hands RANSAC no points: identity / 0 inliers.
__global__ __launch_bounds__(256) void place_gather_kernel(PlaceView v, int q0, const int32_t* __restrict__ d_qitem, const vslam_dmatch* __restrict__ d_m,
                                                           const int32_t* __restrict__ d_nm, int min_inliers, float* __restrict__ d_xyz, float* __restrict__ d_uv,
                                                           int32_t* __restrict__ d_n, int32_t* __restrict__ d_n_matches) {
    const int b = blockIdx.x, c = d_qitem[b];
    const int nm = c < 0 ? 0 : min(max(d_nm[b], 0), v.rows);
    if (threadIdx.x == 0) { d_n_matches[b] = nm; d_n[b] = nm >= min_inliers ? nm : 0; }
    if (nm < min_inliers) return;
    for (int k = threadIdx.x; k < nm; k += 256) {
        const vslam_dmatch mt = d_m[(size_t)b * v.rows + k];
        const int qi = min(max(mt.queryIdx, 0), v.rows - 1), ti = min(max(mt.trainIdx, 0), v.rows - 1);
        const size_t s = (size_t)c * v.rows + qi, t = (size_t)(q0 + b) * v.rows + ti, o = (size_t)b * v.rows + k;
        d_xyz[3 * o] = v.xyz[3 * s]; d_xyz[3 * o + 1] = v.xyz[3 * s + 1]; d_xyz[3 * o + 2] = v.xyz[3 * s + 2];
        d_uv[2 * o] = v.xy[t].x; d_uv[2 * o + 1] = v.xy[t].y;
    }
}

int launch_place_add(const PlaceView& v, const int32_t* d_dst, const uint8_t* d_desc, size_t desc_stride, const int32_t* d_n, const int32_t* d_seq,
                     const int32_t* d_frame, const vslam_keypoint* d_kps, const float* d_xyz, const uint8_t* d_valid, int kp_capacity, int B, hipStream_t stream) {
    if (B <= 0) return VSLAM_OK;
    ProfScope prof__(stream, "place_add_kernel", 2);
    hipLaunchKernelGGL(place_add_kernel, dim3(B), dim3(256), 0, stream, v, d_dst, d_desc, desc_stride, d_n, d_seq, d_frame);
    if (v.xy)
        hipLaunchKernelGGL(place_add_geometry_kernel, dim3(B), dim3(256), 0, stream, v.xy, v.xyz, v.valid, v.qsel, v.nqsel, v.rows, v.capacity, d_dst, d_n, d_kps, d_xyz,
                           d_valid, kp_capacity);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_place_score(const PlaceView& v, int q0, int nq, int tau, int min_gap, int32_t* d_score, int ld, hipStream_t stream) {
    if (nq <= 0 || v.n_entries <= 0) return VSLAM_OK;
    {
        ProfScope prof__(stream, "place_score_init_kernel");
        hipLaunchKernelGGL(place_score_init_kernel, dim3(std::min((v.n_entries + 255) / 256, 1024), nq), dim3(256), 0, stream, v, q0, nq, min_gap, d_score, ld);
    }
    // fill the chip: about 1024 workgroups or more; slice the database when the queries alone do not give them
    const int cblocks = (v.rows + kPlaceColsPerBlock - 1) / kPlaceColsPerBlock;
    int slices = 1;
    while (slices < 64 && (long)nq * slices < 1024 && v.n_entries / (slices * 2) >= 8) slices *= 2;
    const int per_slice = (v.n_entries + slices - 1) / slices;
    ProfScope prof__(stream, "place_score_kernel");
    hipLaunchKernelGGL(place_score_kernel, dim3(nq, cblocks, slices), dim3(kPlaceBlock), 0, stream, v, q0, 256 - 2 * tau, min_gap, per_slice, d_score, ld);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_place_select(const PlaceView& v, int nq, const int32_t* d_score, int ld, int K, int min_score, int32_t* d_cand, int32_t* d_cand_score,
                        hipStream_t stream) {
    if (nq <= 0) return VSLAM_OK;
    ProfScope prof__(stream, "place_select_kernel");
    hipLaunchKernelGGL(place_select_kernel, dim3(nq), dim3(256), 0, stream, v.n_entries, d_score, ld, K, min_score, d_cand, d_cand_score);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_place_verify_prep(const PlaceView& v, int nq, const int32_t* d_cand, int K, int rank, int32_t* d_qitem, double* d_gap, hipStream_t stream) {
    ProfScope prof__(stream, "place_verify_prep_kernel");
    hipLaunchKernelGGL(place_verify_prep_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, v.n_entries, nq, d_cand, K, rank, d_qitem, d_gap);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_place_gather(const PlaceView& v, int q0, int nq, const int32_t* d_qitem, const vslam_dmatch* d_m, const int32_t* d_nm, int min_inliers, float* d_xyz,
                        float* d_uv, int32_t* d_n, int32_t* d_n_matches, hipStream_t stream) {
    ProfScope prof__(stream, "place_gather_kernel");
    hipLaunchKernelGGL(place_gather_kernel, dim3(nq), dim3(256), 0, stream, v, q0, d_qitem, d_m, d_nm, min_inliers, d_xyz, d_uv, d_n, d_n_matches);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
