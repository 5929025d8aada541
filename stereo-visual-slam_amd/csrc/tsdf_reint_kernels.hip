// tsdf_reint_kernels.hip -- re-integration of the surface map (include/vslam_hip.h "RE-INTEGRATION"): a call's frames taken out of the field at the
// poses they went in with and put in at corrected ones, in one pass.  A voxel is four plain integer sums, so taking a frame out is INTEGRATION's
// rule subtracted: the same tsdf_sample (tsdf_device.h), evaluated at the old pose into `sub` and at the new pose into `add`, and one
// read-modify-write `stored + add - sub` per voxel and call.  A frame is subtracted only from the blocks it was added to: list positions below
// its reach (the claimed-block count after the allocation of the call that integrated it) and below n0, the count before this call.
//
//   tsdf_reint_frames_kernel     both frame tables: the new sides into the map's own table (ALLOCATION then reads it), the old sides into the second; n0
//   (tsdf_alloc_kernel           tsdf_kernels.hip's allocation, over the new sides)
//   tsdf_reint_cull_kernel       (form 1) one lane per (block, frame): two 64-bit frame masks per block, the old one with the reach test folded in
//   tsdf_reint_kernel<k>         one workgroup per claimed block, one lane per voxel: sub over the old sides, add over the new ones, the update
// A pose that is not finite switches its side off and is not counted as a skipped frame.  A voxel whose stored sums are below `sub` keeps its value
// and sets status bit 3.  Compiled with FMA contraction off (the Makefile's default): every sum is bit-exact against tests/tsdf_reintegrate_ref.py.
#include "vslam_internal.h"

#include "se3_device.h"
#include "tsdf_device.h"

namespace vslam {

constexpr u64 kTsdfStatusUnderflow = 8ull;

// One workgroup.  Row b of either table carries the frame's map id when the id is in 0 .. 1022 and that side's pose is finite, else -1.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_reint_frames_kernel(TsdfTable t, TsdfReint r, const double* __restrict__ T_old, const double* __restrict__ T_new,
                                                                        const int32_t* __restrict__ map_ids, int B) {
    if (threadIdx.x == 0) *r.n0 = (uint32_t)t.counters[0]; // (the allocation of this call runs after this kernel)
    for (int b = threadIdx.x; b < B; b += kVoxelBlock) {
        const int m = map_ids[b];
        tsdf_frame_row(T_new + 7 * (size_t)b, m, t.frames + (size_t)kTsdfFrameDoubles * b);
        tsdf_frame_row(T_old + 7 * (size_t)b, m, r.frames_old + (size_t)kTsdfFrameDoubles * b);
    }
}

// (form 1) one wave per (list entry, word of 64 frames), one lane per frame.  New side: the frames whose map is the block's and that the cull keeps.
// Old side: those of them whose reach and n0 lie above the block's list position.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_reint_cull_kernel(TsdfTable t, TsdfReint r, TsdfCull cu, int B) {
    const u64 n_list = t.counters[0], n0 = (u64)*r.n0;
    const int lane = threadIdx.x & 63, words = (B + 63) >> 6;
    const double vs = (double)t.vs;
    uint32_t visited = 0u, kept = 0u;
    for (u64 it = (u64)blockIdx.x * (kVoxelBlock / 64) + (threadIdx.x >> 6); it < n_list * (u64)words; it += (u64)gridDim.x * (kVoxelBlock / 64)) {
        const u64 i = it / (u64)words;
        const int wd = (int)(it - i * (u64)words), b = wd * 64 + lane;
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        bool mine_new = false, keep_new = false, mine_old = false, keep_old = false;
        if (b < B) {
            const double* __restrict__ fn = t.frames + (size_t)kTsdfFrameDoubles * b;
            const double* __restrict__ fo = r.frames_old + (size_t)kTsdfFrameDoubles * b;
            const u64 reach = (u64)r.reach[b];
            mine_new = (int)fn[15] == id.map;
            keep_new = mine_new && tsdf_may_pass(fn, id, vs, cu);
            mine_old = (int)fo[15] == id.map && i < (reach < n0 ? reach : n0);
            keep_old = mine_old && tsdf_may_pass(fo, id, vs, cu);
        }
        const u64 m_new = __ballot(keep_new), m_old = __ballot(keep_old);
        visited += (uint32_t)(__popcll(__ballot(mine_new)) + __popcll(__ballot(mine_old))); kept += (uint32_t)(__popcll(m_new) + __popcll(m_old));
        if (lane == 0) { t.pairs[(size_t)s * t.frame_words + wd] = m_new; r.pairs_old[(size_t)s * t.frame_words + wd] = m_old; }
    }
    if (lane == 0 && visited) { atomicAdd(&t.counters[6], (u64)visited); atomicAdd(&t.counters[7], (u64)kept); }
}

// The eight sums stay in registers over the frames; a voxel with nothing to apply is neither read nor written.
// (form 1: 57 VGPRs, and uncapped 88 SGPRs -- two tables, the camera, the gates and the cull; eight waves per SIMD need <= 80)
template <bool kMasks>
__global__ __launch_bounds__(kTsdfLanes) __attribute__((amdgpu_num_sgpr(72))) void tsdf_reint_kernel(TsdfTable t, TsdfReint r, VoxelImages a, TsdfCull cu,
                                                                                                     const uint8_t* __restrict__ gray, size_t img_bytes, int pitch) {
    const u64 n_list = t.counters[0], n0 = (u64)*r.n0;
    const int l = threadIdx.x, words = (a.B + 63) >> 6;
    const double vs = (double)t.vs, tau = (double)t.J * vs, kq = 1024.0 / tau;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        const int ix = id.bx * 8 + (l & 7), iy = id.by * 8 + ((l >> 3) & 7), iz = id.bz * 8 + (l >> 6);
        const double X0 = ((double)ix + 0.5) * vs, X1 = ((double)iy + 0.5) * vs, X2 = ((double)iz + 0.5) * vs;
        TsdfSums add, sub;
        if (kMasks) {
            for (int wd = 0; wd < words; ++wd) {
                u64 m = r.pairs_old[(size_t)s * t.frame_words + wd]; // (workgroup-uniform)
                while (m) {
                    const int b = wd * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    tsdf_sample(r.frames_old + (size_t)kTsdfFrameDoubles * b, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, sub);
                }
            }
            for (int wd = 0; wd < words; ++wd) {
                u64 m = t.pairs[(size_t)s * t.frame_words + wd];
                while (m) {
                    const int b = wd * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    tsdf_sample(t.frames + (size_t)kTsdfFrameDoubles * b, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, add);
                }
            }
        } else {
            uint32_t visited = 0u, kept = 0u;
            for (int b = 0; b < a.B; ++b) {
                const double* __restrict__ f = r.frames_old + (size_t)kTsdfFrameDoubles * b;
                if ((int)f[15] != id.map) continue; // (workgroup-uniform, as are the reach test and the cull)
                const u64 reach = (u64)r.reach[b];
                if (!(i < (reach < n0 ? reach : n0))) continue;
                visited += 1u;
                if (!tsdf_may_pass(f, id, vs, cu)) continue;
                kept += 1u;
                tsdf_sample(f, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, sub);
            }
            for (int b = 0; b < a.B; ++b) {
                const double* __restrict__ f = t.frames + (size_t)kTsdfFrameDoubles * b;
                if ((int)f[15] != id.map) continue;
                visited += 1u;
                if (!tsdf_may_pass(f, id, vs, cu)) continue;
                kept += 1u;
                tsdf_sample(f, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, add);
            }
            if (l == 0 && visited) { atomicAdd(&t.counters[6], (u64)visited); atomicAdd(&t.counters[7], (u64)kept); }
        }
        bool under = false;
        if (add.W | sub.W) { // (a side that saw the voxel counted it in W; the lane owns the voxel: a plain read-modify-write)
            uint4* p = t.pool + (size_t)s * kTsdfLanes + l;
            const uint4 o = *p;
            under = o.x < sub.W || o.y < sub.Sq || o.z < sub.Wc || o.w < sub.I;
            if (!under) *p = make_uint4(o.x + add.W - sub.W, o.y + add.Sq - sub.Sq, o.z + add.Wc - sub.Wc, o.w + add.I - sub.I);
        }
        if (__ballot(under) != 0ull && (l & 63) == 0) atomicOr(&t.counters[4], kTsdfStatusUnderflow);
    }
}

// ------------------------------------------------------------------------------------------------------------------- launchers
// the tables of the old sides: frame table | frame masks | n0 (every part a multiple of 8 bytes)
size_t tsdf_reint_table_bytes(const TsdfTable& t, int max_batch) {
    return (size_t)max_batch * kTsdfFrameDoubles * 8 + ((size_t)t.frame_words << t.log2_blocks) * 8 + 8;
}
TsdfReint tsdf_reint_tables(const TsdfTable& t, int max_batch, uint8_t* base, const uint32_t* d_reach) {
    TsdfReint r;
    r.frames_old = reinterpret_cast<double*>(base); base += (size_t)max_batch * kTsdfFrameDoubles * 8;
    r.pairs_old = reinterpret_cast<unsigned long long*>(base); base += ((size_t)t.frame_words << t.log2_blocks) * 8;
    r.n0 = reinterpret_cast<uint32_t*>(base);
    r.reach = d_reach;
    return r;
}

int launch_tsdf_reintegrate(const TsdfTable& t, const TsdfReint& r, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const double* d_T_old,
                            const int32_t* d_map_id, int form, hipStream_t stream) {
    {
        ProfScope ps(stream, "tsdf_reint_frames_kernel");
        hipLaunchKernelGGL(tsdf_reint_frames_kernel, dim3(1), dim3(kVoxelBlock), 0, stream, t, r, d_T_old, a.T, d_map_id, a.B);
        VS_HIP(hipGetLastError());
    }
    if (int rc = launch_tsdf_alloc(t, a, stream)) return rc;
    const TsdfCull cu = tsdf_cull_of(t, a);
    if (form == 1) {
        ProfScope ps(stream, "tsdf_reint_cull_kernel");
        hipLaunchKernelGGL(tsdf_reint_cull_kernel, dim3(tsdf_list_grid(t)), dim3(kVoxelBlock), 0, stream, t, r, cu, a.B);
        VS_HIP(hipGetLastError());
    }
    ProfScope ps(stream, "tsdf_reint_kernel");
    if (form == 1) hipLaunchKernelGGL(tsdf_reint_kernel<true>, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, r, a, cu, d_gray, img_bytes, pitch);
    else hipLaunchKernelGGL(tsdf_reint_kernel<false>, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, r, a, cu, d_gray, img_bytes, pitch);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
