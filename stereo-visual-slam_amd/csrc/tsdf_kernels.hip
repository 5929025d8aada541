// tsdf_kernels.hip -- the surface map stage (include/vslam_hip.h "surface map"): the SGBM disparity maps of a call's keyframes fused, at their
// poses, into a truncated signed distance field over 8 x 8 x 8 voxel blocks, and the surface read back as one surfel per zero-crossing voxel edge.
// Everything a voxel holds is an integer sum and every voxel has ONE owner lane, so the field depends neither on the order of the frames nor on
// the order the blocks were claimed in, and the integration needs no atomics.
//
//   tsdf_clear_kernel           every slot empty, every voxel zero
//   tsdf_frames_kernel          the call's frame table: R, t, the inverse translation, the map id (-1: the frame takes no part)
//   tsdf_alloc_kernel           every sample along every wanted pixel's ray -> the block that holds it, claimed if it is new
//   tsdf_cull_kernel            (form 1) one lane per (block, frame): a 64-bit frame mask per block
//   tsdf_integrate_kernel<k>    one workgroup per claimed block, one lane per voxel, every frame of the call (form 0) or of the block's mask (form 1)
//   tsdf_extract_kernel         one lane per voxel: its three edges towards +x, +y, +z; the crossing ones leave as surfels, one counter add per wave
//   tsdf_blocks_kernel          the raw blocks, for tests and tools
// The hash slot is the storage (slot s owns block s of the pool) and a claimed slot is appended to a list the later kernels walk, so no lane ever
// waits for another to publish an index: claiming is a relaxed key load, a 64-bit compare-and-swap only on "empty", linear probing over at most
// kTsdfMaxProbe slots.  A sample that finds no slot is dropped and counted.
// Compiled with FMA contraction off (the Makefile's default): every sum is bit-exact against tests/tsdf_ref.py.
// The key, the claim, the lookup, the voxel predicates and the surfel arithmetic are in tsdf_device.h, shared with tsdf_mesh_kernels.hip; the frame
// row, the cull and the per-sample rule of INTEGRATION lie there too, shared with tsdf_reint_kernels.hip.
#include "vslam_internal.h"

#include "se3_device.h"
#include "tsdf_device.h"

namespace vslam {

__global__ __launch_bounds__(kVoxelBlock) void tsdf_clear_kernel(TsdfTable t) {
    const size_t n_slots = (size_t)1 << t.log2_blocks, n_vox = n_slots * kTsdfLanes, stride = (size_t)gridDim.x * kVoxelBlock;
    for (size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x; i < n_vox; i += stride) t.pool[i] = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x; i < n_slots; i += stride) t.keys[i] = kVoxelEmpty;
    if (blockIdx.x == 0 && threadIdx.x < kTsdfCounters) t.counters[threadIdx.x] = 0ull;
}

// ------------------------------------------------------------------------------------------------------------------- the frame table
// One workgroup.  A frame takes part when its map id is in 0 .. 1022 and its seven pose numbers, the rotation matrix and the inverse translation
// formed from them are finite; a frame with a map id and a pose that is not finite is counted and sets status bit 2.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_frames_kernel(TsdfTable t, const double* __restrict__ T, const int32_t* __restrict__ map_ids, int B) {
    uint32_t skipped = 0u;
    for (int b = threadIdx.x; b < B; b += kVoxelBlock) {
        const double* Tb = T + 7 * (size_t)b;
        const int m = map_ids[b];
        const bool fin = tsdf_frame_row(Tb, m, t.frames + (size_t)kTsdfFrameDoubles * b);
        skipped += (m >= 0 && m <= kVoxelMaxMap && !fin) ? 1u : 0u;
    }
    if (skipped) { atomicAdd(&t.counters[5], (u64)skipped); atomicOr(&t.counters[4], 4ull); }
}

// ------------------------------------------------------------------------------------------------------------------- allocation
// The tile mapping of the dense map's fused pass.  A lane walks the 2 J + 1 samples of each of its four pixels in order, so samples of one block
// follow each other: it merges such a run before anything leaves it.  A block that exists already costs its run one key load and no atomic.
// (42 VGPRs: eight waves per SIMD need <= 80 SGPRs on this device; the camera, the gates and the pose are 50 of them)
__global__ __launch_bounds__(kVoxelBlock) __attribute__((amdgpu_num_sgpr(72))) void tsdf_alloc_kernel(TsdfTable t, VoxelImages a, int vec) {
    const double* __restrict__ f = t.frames + (size_t)kTsdfFrameDoubles * blockIdx.z;
    const int map_id = (int)f[15];
    if (map_id < 0) return; // (workgroup-uniform)
    VoxelLane l;
    voxel_lane_load(a, vec, l);
    TsdfTally tally;
    if (l.r < a.h && (l.c[0] >= 0 || l.c[1] >= 0 || l.c[2] >= 0 || l.c[3] >= 0)) {
        const double Rinv[9] = {f[0], f[3], f[6], f[1], f[4], f[7], f[2], f[5], f[8]}, tinv[3] = {f[12], f[13], f[14]};
        const double vs = (double)t.vs;
        u64 run_key = kVoxelEmpty;
        uint32_t run_n = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (l.c[j] < 0) continue;
            const double depth = a.fx * a.b / (double)l.d[j];
            if (!(depth > a.z_min && depth < a.z_max)) continue; // (reproject_pixel's gate)
            for (int k = -t.J; k <= t.J; ++k) {
                const double Z = depth + (double)k * vs;
                if (Z <= 0) continue;
                float px, py, pz;
                reproject_ray(a, Rinv, tinv, l.c[j], l.r, Z, px, py, pz);
                uint32_t cx, cy, cz, off;
                const bool okx = voxel_axis(px, t.inv, cx, off), oky = voxel_axis(py, t.inv, cy, off), okz = voxel_axis(pz, t.inv, cz, off);
                if (!(okx && oky && okz)) { tally.range += 1u; continue; }
                const u64 key = tsdf_key(map_id, cx, cy, cz);
                if (key == run_key) { run_n += 1u; continue; }
                if (run_n) tsdf_claim(t, run_key, run_n, tally);
                run_key = key; run_n = 1u;
            }
        }
        if (run_n) tsdf_claim(t, run_key, run_n, tally);
    }
    for (int o = 32; o > 0; o >>= 1) {
        tally.samples += __shfl_xor(tally.samples, o); tally.range += __shfl_xor(tally.range, o); tally.full += __shfl_xor(tally.full, o);
    }
    if ((threadIdx.x & 63) != 0) return;
    if (tally.samples) atomicAdd(&t.counters[1], (u64)tally.samples);
    if (tally.range) atomicAdd(&t.counters[2], (u64)tally.range);
    if (tally.full) { atomicAdd(&t.counters[3], (u64)tally.full); atomicOr(&t.counters[4], 1ull); }
}

// ------------------------------------------------------------------------------------------------------------------- integration
// (form 1) one wave per (list entry, word of 64 frames), one lane per frame: the frames whose map is the block's and that the cull keeps
__global__ __launch_bounds__(kVoxelBlock) void tsdf_cull_kernel(TsdfTable t, TsdfCull cu, int B) {
    const u64 n_list = t.counters[0];
    const int lane = threadIdx.x & 63, words = (B + 63) >> 6;
    const double vs = (double)t.vs;
    uint32_t visited = 0u, kept = 0u;
    for (u64 it = (u64)blockIdx.x * (kVoxelBlock / 64) + (threadIdx.x >> 6); it < n_list * (u64)words; it += (u64)gridDim.x * (kVoxelBlock / 64)) {
        const u64 i = it / (u64)words;
        const int wd = (int)(it - i * (u64)words), b = wd * 64 + lane;
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        bool mine = false, keep = false;
        if (b < B) {
            const double* __restrict__ f = t.frames + (size_t)kTsdfFrameDoubles * b;
            mine = (int)f[15] == id.map;
            keep = mine && tsdf_may_pass(f, id, vs, cu);
        }
        const u64 m = __ballot(keep);
        visited += (uint32_t)__popcll(__ballot(mine)); kept += (uint32_t)__popcll(m);
        if (lane == 0) t.pairs[(size_t)s * t.frame_words + wd] = m;
    }
    if (lane == 0 && visited) { atomicAdd(&t.counters[6], (u64)visited); atomicAdd(&t.counters[7], (u64)kept); }
}

template <bool kMasks>
__global__ __launch_bounds__(kTsdfLanes) void tsdf_integrate_kernel(TsdfTable t, VoxelImages a, TsdfCull cu, const uint8_t* __restrict__ gray, size_t img_bytes, int pitch) {
    const u64 n_list = t.counters[0];
    const int l = threadIdx.x, words = (a.B + 63) >> 6;
    const double vs = (double)t.vs, tau = (double)t.J * vs, kq = 1024.0 / tau;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        const int ix = id.bx * 8 + (l & 7), iy = id.by * 8 + ((l >> 3) & 7), iz = id.bz * 8 + (l >> 6);
        const double X0 = ((double)ix + 0.5) * vs, X1 = ((double)iy + 0.5) * vs, X2 = ((double)iz + 0.5) * vs;
        TsdfSums v;
        if (kMasks) {
            for (int wd = 0; wd < words; ++wd) {
                u64 m = t.pairs[(size_t)s * t.frame_words + wd]; // (workgroup-uniform)
                while (m) {
                    const int b = wd * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    tsdf_sample(t.frames + (size_t)kTsdfFrameDoubles * b, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, v);
                }
            }
        } else {
            uint32_t visited = 0u, kept = 0u;
            for (int b = 0; b < a.B; ++b) {
                const double* __restrict__ f = t.frames + (size_t)kTsdfFrameDoubles * b;
                if ((int)f[15] != id.map) continue; // (workgroup-uniform, as is the cull)
                visited += 1u;
                if (!tsdf_may_pass(f, id, vs, cu)) continue;
                kept += 1u;
                tsdf_sample(f, b, X0, X1, X2, a, gray, img_bytes, pitch, vs, tau, kq, v);
            }
            if (l == 0 && visited) { atomicAdd(&t.counters[6], (u64)visited); atomicAdd(&t.counters[7], (u64)kept); }
        }
        if (v.W) { // the lane owns the voxel: a plain read-modify-write
            uint4* p = t.pool + (size_t)s * kTsdfLanes + l;
            const uint4 o = *p;
            *p = make_uint4(o.x + v.W, o.y + v.Sq, o.z + v.Wc, o.w + v.I);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- extraction
__global__ __launch_bounds__(kTsdfLanes) void tsdf_extract_kernel(TsdfTable t, int map_id, uint32_t min_w, vslam_surfel* __restrict__ out, int32_t* __restrict__ map_out,
                                                                  u64 capacity, u64* __restrict__ n_out) {
#pragma clang fp contract(off)
    __shared__ uint4 lv[kTsdfLanes];
    const u64 n_list = t.counters[0];
    const int l = threadIdx.x, lane = l & 63;
    const double vs = (double)t.vs;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        if (map_id >= 0 && id.map != map_id) continue; // (workgroup-uniform)
        __syncthreads(); // (the readers of the last block are done)
        const uint4 va = t.pool[(size_t)s * kTsdfLanes + l];
        lv[l] = va;
        __syncthreads();
        if (va.x >= kTsdfMaxW) atomicOr(&t.counters[4], 2ull);
        const int ia[3] = {id.bx * 8 + (l & 7), id.by * 8 + ((l >> 3) & 7), id.bz * 8 + (l >> 6)};
        const bool good_a = tsdf_good(va, min_w);
        const double Da = good_a ? tsdf_D(va) : 0.0;
#pragma unroll 1
        for (int e = 0; e < 3; ++e) {
            const int e0 = e == 0, e1 = e == 1, e2 = e == 2;
            bool take = false;
            uint4 vb = make_uint4(0u, 0u, 0u, 0u);
            if (good_a) {
                vb = tsdf_fetch(t, lv, id, ia[0] + e0, ia[1] + e1, ia[2] + e2);
                take = tsdf_good(vb, min_w) && ((tsdf_num(va) > 0) != (tsdf_num(vb) > 0));
            }
            const u64 ballot = __ballot(take);
            if (ballot == 0) continue; // (wave-uniform)
            u64 first = 0;
            if (lane == 0) first = atomicAdd(n_out, (u64)__popcll(ballot));
            first = __shfl(first, 0);
            const u64 pos = first + (u64)__popcll(ballot & ((1ull << lane) - 1ull));
            if (!take || pos >= capacity) continue;
            tsdf_surfel(t, lv, id, ia, e, va, vb, Da, min_w, vs, out + pos);
            if (map_out) map_out[pos] = id.map;
        }
    }
}

// the claimed blocks of map map_id (-1: all): (map, bx, by, bz) and the block's 512 x 4 uint32; the counter runs on past `capacity`
__global__ __launch_bounds__(kTsdfLanes) void tsdf_blocks_kernel(TsdfTable t, int map_id, int32_t* __restrict__ block_out, uint4* __restrict__ voxels_out, u64 capacity,
                                                                 u64* __restrict__ n_out) {
    __shared__ u64 spos;
    const u64 n_list = t.counters[0];
    const int l = threadIdx.x;
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const uint32_t s = t.list[i];
        const TsdfBlockId id = tsdf_unpack(t.keys[s]);
        if (map_id >= 0 && id.map != map_id) continue; // (workgroup-uniform)
        __syncthreads();
        if (l == 0) spos = atomicAdd(n_out, 1ull);
        __syncthreads();
        const u64 pos = spos;
        if (pos >= capacity) continue;
        voxels_out[pos * kTsdfLanes + l] = t.pool[(size_t)s * kTsdfLanes + l];
        if (l == 0) reinterpret_cast<int4*>(block_out)[pos] = make_int4(id.map, id.bx, id.by, id.bz);
    }
}

// ------------------------------------------------------------------------------------------------------------------- launchers
int launch_tsdf_clear(const TsdfTable& t, hipStream_t stream) {
    ProfScope ps(stream, "tsdf_clear_kernel");
    const size_t need = (((size_t)kTsdfLanes << t.log2_blocks) + kVoxelBlock - 1) / kVoxelBlock;
    hipLaunchKernelGGL(tsdf_clear_kernel, dim3((unsigned)(need > 256 * 16 ? 256 * 16 : need)), dim3(kVoxelBlock), 0, stream, t);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

// ALLOCATION of the frames of t.frames (a.T is not read: the poses are the table's)
int launch_tsdf_alloc(const TsdfTable& t, const VoxelImages& a, hipStream_t stream) {
    const int vec = voxel_vec(a), hs = (a.h + a.step - 1) / a.step;
    const dim3 grid(voxel_tiles_x(a, vec), (hs + kVoxelTileRows - 1) / kVoxelTileRows, a.B);
    ProfScope ps(stream, "tsdf_alloc_kernel");
    hipLaunchKernelGGL(tsdf_alloc_kernel, grid, dim3(kVoxelBlock), 0, stream, t, a, vec);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_tsdf_integrate(const TsdfTable& t, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const int32_t* d_map_id, int form,
                          hipStream_t stream) {
    {
        ProfScope ps(stream, "tsdf_frames_kernel");
        hipLaunchKernelGGL(tsdf_frames_kernel, dim3(1), dim3(kVoxelBlock), 0, stream, t, a.T, d_map_id, a.B);
        VS_HIP(hipGetLastError());
    }
    if (int rc = launch_tsdf_alloc(t, a, stream)) return rc;
    const TsdfCull cu = tsdf_cull_of(t, a);
    if (form == 1) {
        ProfScope ps(stream, "tsdf_cull_kernel");
        hipLaunchKernelGGL(tsdf_cull_kernel, dim3(tsdf_list_grid(t)), dim3(kVoxelBlock), 0, stream, t, cu, a.B);
        VS_HIP(hipGetLastError());
    }
    ProfScope ps(stream, "tsdf_integrate_kernel");
    if (form == 1) hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, a, cu, d_gray, img_bytes, pitch);
    else hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, a, cu, d_gray, img_bytes, pitch);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_tsdf_extract(const TsdfTable& t, int map_id, int min_weight, vslam_surfel* d_out, int32_t* d_map_out, size_t capacity, unsigned long long* d_n_out,
                        hipStream_t stream) {
    VS_HIP(hipMemsetAsync(d_n_out, 0, sizeof(u64), stream));
    ProfScope ps(stream, "tsdf_extract_kernel");
    hipLaunchKernelGGL(tsdf_extract_kernel, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, map_id, (uint32_t)(min_weight < 1 ? 1 : min_weight), d_out, d_map_out,
                       (u64)capacity, d_n_out);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_tsdf_blocks(const TsdfTable& t, int map_id, int32_t* d_block_out, uint32_t* d_voxels_out, size_t capacity, unsigned long long* d_n_out,
                       hipStream_t stream) {
    VS_HIP(hipMemsetAsync(d_n_out, 0, sizeof(u64), stream));
    ProfScope ps(stream, "tsdf_blocks_kernel");
    hipLaunchKernelGGL(tsdf_blocks_kernel, dim3(tsdf_list_grid(t)), dim3(kTsdfLanes), 0, stream, t, map_id, d_block_out, reinterpret_cast<uint4*>(d_voxels_out),
                       (u64)capacity, d_n_out);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
