// voxel_kernels.hip -- the dense map stage (include/vslam_hip.h "dense map"): the SGBM disparity of every pixel, reprojected at its keyframe's pose,
// summed into a sparse voxel grid that lives in a device hash table.  Everything a voxel holds is an integer sum, so the table does not depend on
// the order its points arrive in.
//
//   voxel_clear_kernel          every slot empty
//   reproject_kernel            disparity maps -> points (B x ceil(h / step) x ceil(w / step) x 3 f32) and their depth-gate flags
//   voxel_insert_points_kernel  a point list -> the table
//   voxel_fuse_kernel<kLds>     both in one pass, no point written to memory: <false> every point straight into the table, <true> a workgroup
//                               sums its image tile in an LDS hash table first and adds each distinct voxel of the tile to the table once
//   voxel_extract_kernel        occupied slots -> a compact list of centroids, one counter add per wave
// Insertion: a 64-bit compare-and-swap claims an empty slot for a key, linear probing over at most kVoxelMaxProbe slots; the sums are added with
// no-return atomics.  No loop waits for another lane or workgroup: a point that finds no slot within the probe limit is dropped and counted.
// This file is compiled with FMA contraction off (the Makefile's default): the key arithmetic is bit-exact against tests/voxel_ref.py, and the
// reprojection of reproject_kernel and voxel_fuse_kernel is ONE device function, so the two give the same points.
#include "vslam_internal.h"

#include "se3_device.h"
#include "voxel_device.h"

namespace vslam {

constexpr int kVoxelMaxProbe = 128;   // slots a point may probe in the global table before it counts as dropped
constexpr int kVoxelLdsSlots = 512;   // LDS table of voxel_fuse_kernel<true>: 512 x (8 + 20) bytes = 14 KiB for a tile of 1024 pixels
constexpr int kVoxelLdsProbe = 8;     // ... and the slots a point probes there before it goes to the global table itself

struct VoxelSlot { u64 key; uint32_t count, sox, soy, soz, sint, pad; };
static_assert(sizeof(VoxelSlot) == 32, "a slot is 32 bytes");

// what a lane did, summed over its wave at the end of the kernel: one counter add per wave and counter
struct VoxelTally { uint32_t occupied = 0, points = 0, range = 0, full = 0; };

struct VoxelKey { u64 key; uint32_t ox, oy, oz; bool ok; }; // ok false: the point is out of range on some axis
__device__ __forceinline__ VoxelKey voxel_key(float x, float y, float z, float inv, int map_id) {
    VoxelKey k;
    uint32_t cx, cy, cz;
    const bool okx = voxel_axis(x, inv, cx, k.ox), oky = voxel_axis(y, inv, cy, k.oy), okz = voxel_axis(z, inv, cz, k.oz);
    k.ok = okx && oky && okz;
    k.key = (u64)(uint32_t)map_id << 54 | (u64)cx << 36 | (u64)cy << 18 | (u64)cz;
    return k;
}

// n points of one voxel, already summed, into the global table.  (count, sum_ox) and (sum_oy, sum_oz) go out as one 64-bit add each: a carry out
// of the lower word needs a count of 2^32 resp. 2^24, beyond the limit the sums are documented for.
__device__ __forceinline__ void voxel_add(const VoxelTable& t, u64 key, uint32_t hash, uint32_t n, uint32_t sox, uint32_t soy, uint32_t soz, uint32_t sint,
                                          VoxelTally& tally) {
    VoxelSlot* slots = reinterpret_cast<VoxelSlot*>(t.slots);
    const uint32_t mask = (1u << t.log2_capacity) - 1u;
    uint32_t s = hash & mask, claimed = 0u, added = 0u;
    for (int p = 0; p < kVoxelMaxProbe; ++p, s = (s + 1) & mask) {
        u64 k = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVoxelEmpty) {
            k = atomicCAS(&slots[s].key, kVoxelEmpty, key);
            if (k == kVoxelEmpty) { claimed = 1u; k = key; }
        }
        if (k == key) {
            atomicAdd(reinterpret_cast<u64*>(&slots[s].count), (u64)n | (u64)sox << 32);
            atomicAdd(reinterpret_cast<u64*>(&slots[s].soy), (u64)soy | (u64)soz << 32);
            if (sint) atomicAdd(&slots[s].sint, sint);
            added = n;
            break;
        }
    }
    // (branch-free: the tally stays in registers)
    tally.occupied += claimed; tally.points += added; tally.full += n - added;
}

// every lane of every wave of the workgroup calls this once, converged
__device__ __forceinline__ void voxel_tally_flush(const VoxelTable& t, VoxelTally v) {
    for (int o = 32; o > 0; o >>= 1) {
        v.occupied += __shfl_xor(v.occupied, o); v.points += __shfl_xor(v.points, o); v.range += __shfl_xor(v.range, o); v.full += __shfl_xor(v.full, o);
    }
    if ((threadIdx.x & 63) != 0) return;
    if (v.occupied) atomicAdd(&t.counters[0], (u64)v.occupied);
    if (v.points) atomicAdd(&t.counters[1], (u64)v.points);
    if (v.range) atomicAdd(&t.counters[2], (u64)v.range);
    if (v.full) { atomicAdd(&t.counters[3], (u64)v.full); atomicOr(&t.counters[4], 1ull); }
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_clear_kernel(VoxelTable t) {
    uint4* p = reinterpret_cast<uint4*>(t.slots);
    const size_t n = (size_t)2 << t.log2_capacity;
    for (size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kVoxelBlock)
        p[i] = (i & 1) ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(~0u, ~0u, 0u, 0u);
}

__global__ __launch_bounds__(kVoxelBlock) void voxel_insert_points_kernel(VoxelTable t, const float* __restrict__ xyz, const uint8_t* __restrict__ valid,
                                                                          const uint8_t* __restrict__ intensity, size_t n, int map_id) {
    VoxelTally tally;
    for (size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kVoxelBlock) {
        if (valid && !valid[i]) continue;
        const VoxelKey k = voxel_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], t.inv, map_id);
        tally.range += k.ok ? 0u : 1u;
        if (!k.ok) continue;
        voxel_add(t, k.key, voxel_hash(k.key), 1u, k.ox, k.oy, k.oz, intensity ? (uint32_t)intensity[i] : 0u, tally);
    }
    voxel_tally_flush(t, tally);
}

// ------------------------------------------------------------------------------------------------------------------- reprojection
__global__ __launch_bounds__(kVoxelBlock) void reproject_kernel(VoxelImages a, int vec, float* __restrict__ xyz, uint8_t* __restrict__ valid) {
    VoxelLane l;
    voxel_lane_load(a, vec, l);
    if (l.r >= a.h) return;
    double Rinv[9], tinv[3];
    voxel_inverse_pose(a.T + 7 * (size_t)blockIdx.z, Rinv, tinv);
    const int ws = (a.w + a.step - 1) / a.step, hs = (a.h + a.step - 1) / a.step;
    const size_t row = ((size_t)blockIdx.z * hs + l.rs) * ws;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (l.c[j] < 0) continue;
        float px, py, pz;
        const bool ok = reproject_pixel(a, Rinv, tinv, l.c[j], l.r, l.d[j], px, py, pz);
        const size_t i = row + l.c[j] / a.step;
        xyz[3 * i] = px; xyz[3 * i + 1] = py; xyz[3 * i + 2] = pz;
        valid[i] = ok;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the fused pass
// Neighbouring pixels share voxels (at 20 m a 0.2 m voxel is about 7 pixels wide), so the question of this kernel is contention, not bytes.
// Both forms: a lane merges the run of equal keys among its own four adjacent pixels before anything leaves it.
//   <false>: each run goes straight to the global table.
//   <true>:  each run goes into the workgroup's LDS table (same key, same five sums, LDS atomics); after a barrier every occupied LDS slot is
//            added to the global table once.  A run that finds no LDS slot within kVoxelLdsProbe goes to the global table itself.
// Integer sums commute: the two forms leave identical tables.
template <bool kLds>
__global__ __launch_bounds__(kVoxelBlock) void voxel_fuse_kernel(VoxelTable t, VoxelImages a, int vec, const uint8_t* __restrict__ gray, size_t img_bytes, int pitch,
                                                                 const int32_t* __restrict__ map_ids) {
    __shared__ u64 lkey[kLds ? kVoxelLdsSlots : 1];
    __shared__ uint32_t lsum[kLds ? kVoxelLdsSlots : 1][5];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int map_id = map_ids[b];
    if (map_id < 0 || map_id > kVoxelMaxMap) return; // (workgroup-uniform: before any barrier)
    if (kLds) {
        for (int i = tid; i < kVoxelLdsSlots; i += kVoxelBlock) {
            lkey[i] = kVoxelEmpty;
#pragma unroll
            for (int k = 0; k < 5; ++k) lsum[i][k] = 0u;
        }
        __syncthreads();
    }
    VoxelLane l;
    voxel_lane_load(a, vec, l);
    VoxelTally tally;
    if (l.r < a.h && (l.c[0] >= 0 || l.c[1] >= 0 || l.c[2] >= 0 || l.c[3] >= 0)) {
        double Rinv[9], tinv[3];
        voxel_inverse_pose(a.T + 7 * (size_t)b, Rinv, tinv);
        const uint8_t* grow = gray ? gray + (size_t)b * img_bytes + (size_t)l.r * pitch : nullptr;
        u64 run_key = kVoxelEmpty; // the lane's pending run: n points of one voxel and their sums
        uint32_t run_n = 0u, run_x = 0u, run_y = 0u, run_z = 0u, run_g = 0u;
#pragma unroll
        for (int j = 0; j <= 4; ++j) {
            u64 key = kVoxelEmpty;
            uint32_t ox = 0u, oy = 0u, oz = 0u, g = 0u;
            if (j < 4 && l.c[j] >= 0) {
                float px, py, pz;
                if (reproject_pixel(a, Rinv, tinv, l.c[j], l.r, l.d[j], px, py, pz)) {
                    const VoxelKey k = voxel_key(px, py, pz, t.inv, map_id);
                    tally.range += k.ok ? 0u : 1u;
                    if (k.ok) { key = k.key; ox = k.ox; oy = k.oy; oz = k.oz; g = grow ? (uint32_t)grow[l.c[j]] : 0u; }
                }
            }
            if (key == run_key) { // (also "no point" after "no point")
                if (key != kVoxelEmpty) { run_n += 1u; run_x += ox; run_y += oy; run_z += oz; run_g += g; }
                continue;
            }
            if (run_key != kVoxelEmpty) { // the run ends here (j == 4 ends the last one)
                const uint32_t hash = voxel_hash(run_key);
                bool done = false;
                if (kLds) {
                    uint32_t s = (hash >> 16) & (kVoxelLdsSlots - 1);
                    for (int p = 0; p < kVoxelLdsProbe && !done; ++p, s = (s + 1) & (kVoxelLdsSlots - 1)) {
                        u64 k = __hip_atomic_load(&lkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (k == kVoxelEmpty) {
                            k = atomicCAS(&lkey[s], kVoxelEmpty, run_key);
                            if (k == kVoxelEmpty) k = run_key;
                        }
                        if (k == run_key) {
                            atomicAdd(&lsum[s][0], run_n); atomicAdd(&lsum[s][1], run_x); atomicAdd(&lsum[s][2], run_y); atomicAdd(&lsum[s][3], run_z);
                            if (run_g) atomicAdd(&lsum[s][4], run_g);
                            done = true;
                        }
                    }
                }
                if (!done) voxel_add(t, run_key, hash, run_n, run_x, run_y, run_z, run_g, tally);
            }
            run_key = key; run_n = 1u; run_x = ox; run_y = oy; run_z = oz; run_g = g;
        }
    }
    if (kLds) {
        __syncthreads();
        for (int i = tid; i < kVoxelLdsSlots; i += kVoxelBlock) {
            const u64 k = lkey[i];
            if (k != kVoxelEmpty) voxel_add(t, k, voxel_hash(k), lsum[i][0], lsum[i][1], lsum[i][2], lsum[i][3], lsum[i][4], tally);
        }
    }
    voxel_tally_flush(t, tally);
}

// ------------------------------------------------------------------------------------------------------------------- extraction
// One lane per slot; the lanes of a wave that hold a wanted voxel take their output positions from ONE add to the counter.  The counter runs on
// past `capacity`: it is the full count, only the writes stop.
__global__ __launch_bounds__(kVoxelBlock) void voxel_extract_kernel(VoxelTable t, int map_id, uint32_t min_count, vslam_voxel* __restrict__ out,
                                                                    int32_t* __restrict__ map_out, u64 capacity, u64* __restrict__ n_out) {
    const uint4* slots = reinterpret_cast<const uint4*>(t.slots);
    const u64 n_slots = 1ull << t.log2_capacity; // (a multiple of the workgroup: every wave runs the loop converged)
    const int lane = threadIdx.x & 63;
    const double vs = (double)t.vs;
    for (u64 i = (u64)blockIdx.x * kVoxelBlock + threadIdx.x; i < n_slots; i += (u64)gridDim.x * kVoxelBlock) {
        const uint4 lo = slots[2 * i], hi = slots[2 * i + 1];
        const u64 key = (u64)lo.x | (u64)lo.y << 32;
        const uint32_t count = lo.z;
        const bool occupied = key != kVoxelEmpty && count > 0u;
        if (occupied && count >= (1u << 24)) atomicOr(&t.counters[4], 2ull);
        const int m = (int)(key >> 54);
        const bool take = occupied && count >= min_count && (map_id < 0 || m == map_id);
        const u64 ballot = __ballot(take);
        if (ballot == 0) continue;
        u64 first = 0;
        if (lane == 0) first = atomicAdd(n_out, (u64)__popcll(ballot));
        first = __shfl(first, 0);
        const u64 pos = first + (u64)__popcll(ballot & ((1ull << lane) - 1ull));
        if (!take || pos >= capacity) continue;
        const int ix = (int)((key >> 36) & 0x3FFFFu) - kVoxelHalf, iy = (int)((key >> 18) & 0x3FFFFu) - kVoxelHalf, iz = (int)(key & 0x3FFFFu) - kVoxelHalf;
        const double n = (double)count;
        const float x = (float)(((double)ix + ((double)lo.w / n + 0.5) / 256.0) * vs);
        const float y = (float)(((double)iy + ((double)hi.x / n + 0.5) / 256.0) * vs);
        const float z = (float)(((double)iz + ((double)hi.y / n + 0.5) / 256.0) * vs);
        const float g = (float)((double)hi.z / n);
        uint4* o = reinterpret_cast<uint4*>(out + pos);
        o[0] = make_uint4((uint32_t)ix, (uint32_t)iy, (uint32_t)iz, count);
        o[1] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(g));
        if (map_out) map_out[pos] = m;
    }
}

// ------------------------------------------------------------------------------------------------------------------- launchers
static unsigned voxel_stream_grid(size_t items) { // a grid-stride kernel: enough workgroups to fill the device, no more than the work
    const size_t need = (items + kVoxelBlock - 1) / kVoxelBlock;
    return (unsigned)(need < 1 ? 1 : (need > 256 * 16 ? 256 * 16 : need));
}

int launch_voxel_clear(const VoxelTable& t, hipStream_t stream) {
    VS_HIP(hipMemsetAsync(t.counters, 0, sizeof(u64) * kVoxelCounters, stream));
    ProfScope ps(stream, "voxel_clear_kernel");
    hipLaunchKernelGGL(voxel_clear_kernel, dim3(voxel_stream_grid((size_t)2 << t.log2_capacity)), dim3(kVoxelBlock), 0, stream, t);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_reproject(const VoxelImages& a, float* d_xyz, uint8_t* d_valid, hipStream_t stream) {
    const int vec = voxel_vec(a), hs = (a.h + a.step - 1) / a.step;
    const dim3 grid(voxel_tiles_x(a, vec), (hs + kVoxelTileRows - 1) / kVoxelTileRows, a.B);
    ProfScope ps(stream, "reproject_kernel");
    hipLaunchKernelGGL(reproject_kernel, grid, dim3(kVoxelBlock), 0, stream, a, vec, d_xyz, d_valid);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_voxel_insert_points(const VoxelTable& t, const float* d_xyz, const uint8_t* d_valid, const uint8_t* d_intensity, size_t n, int map_id, hipStream_t stream) {
    if (n == 0) return VSLAM_OK;
    ProfScope ps(stream, "voxel_insert_points_kernel");
    hipLaunchKernelGGL(voxel_insert_points_kernel, dim3(voxel_stream_grid(n)), dim3(kVoxelBlock), 0, stream, t, d_xyz, d_valid, d_intensity, n, map_id);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_voxel_fuse(const VoxelTable& t, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const int32_t* d_map_id, int form,
                      hipStream_t stream) {
    const int vec = voxel_vec(a), hs = (a.h + a.step - 1) / a.step;
    const dim3 grid(voxel_tiles_x(a, vec), (hs + kVoxelTileRows - 1) / kVoxelTileRows, a.B);
    ProfScope ps(stream, "voxel_fuse_kernel");
    if (form == 1) hipLaunchKernelGGL(voxel_fuse_kernel<true>, grid, dim3(kVoxelBlock), 0, stream, t, a, vec, d_gray, img_bytes, pitch, d_map_id);
    else hipLaunchKernelGGL(voxel_fuse_kernel<false>, grid, dim3(kVoxelBlock), 0, stream, t, a, vec, d_gray, img_bytes, pitch, d_map_id);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_voxel_extract(const VoxelTable& t, int map_id, int min_count, vslam_voxel* d_out, int32_t* d_map_out, size_t capacity, unsigned long long* d_n_out,
                         hipStream_t stream) {
    VS_HIP(hipMemsetAsync(d_n_out, 0, sizeof(u64), stream));
    ProfScope ps(stream, "voxel_extract_kernel");
    hipLaunchKernelGGL(voxel_extract_kernel, dim3(voxel_stream_grid((size_t)1 << t.log2_capacity)), dim3(kVoxelBlock), 0, stream, t, map_id,
                       (uint32_t)(min_count < 1 ? 1 : min_count), d_out, d_map_out, (u64)capacity, d_n_out);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
