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
// The key, the claim, the lookup, the voxel predicates and the surfel arithmetic are in tsdf_device.h, shared with tsdf_mesh_kernels.hip.
#include "vslam_internal.h"

#include "se3_device.h"
#include "tsdf_device.h"

namespace vslam {

// what the cull needs of the camera: the slopes of the image rectangle grown by half a pixel and the lengths of the four side planes' normals
struct TsdfCull { double al, ar, at, ab, nl, nr, nt, nb, rad; };

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
        double R[9], Rinv[9], tinv[3];
        se3::rotmat(Tb, R);
        voxel_inverse_pose(Tb, Rinv, tinv);
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 7; ++i) fin = fin && isfinite(Tb[i]);
#pragma unroll
        for (int i = 0; i < 9; ++i) fin = fin && isfinite(R[i]);
#pragma unroll
        for (int i = 0; i < 3; ++i) fin = fin && isfinite(tinv[i]);
        const int m = map_ids[b];
        const bool mapped = m >= 0 && m <= kVoxelMaxMap;
        skipped += (mapped && !fin) ? 1u : 0u;
        double* f = t.frames + (size_t)kTsdfFrameDoubles * b;
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { f[9 + i] = Tb[4 + i]; f[12 + i] = tinv[i]; }
        f[15] = (mapped && fin) ? (double)m : -1.0;
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
// The cull, an optimisation only: false when NO voxel of the block can pass the rule in frame f.  Every voxel centre lies within 3.5 sqrt(3) < 6.07
// voxels of the block's centre C; cu.rad is 7 voxels.  A voxel passes only with P[2] > vs and -0.5 <= u < w - 0.5, that is x >= al z and x < ar z
// for z > 0 (fx > 0), likewise in y: a sphere wholly on the outer side of one of these five planes holds no such voxel.  (With fx or fy <= 0 the
// launcher sets rad to infinity and nothing is culled.)
__device__ __forceinline__ bool tsdf_may_pass(const double* __restrict__ f, const TsdfBlockId& b, double vs, const TsdfCull& cu) {
    const double C0 = ((double)(8 * b.bx) + 4.0) * vs, C1 = ((double)(8 * b.by) + 4.0) * vs, C2 = ((double)(8 * b.bz) + 4.0) * vs;
    const double P0 = f[0] * C0 + f[1] * C1 + f[2] * C2 + f[9], P1 = f[3] * C0 + f[4] * C1 + f[5] * C2 + f[10], P2 = f[6] * C0 + f[7] * C1 + f[8] * C2 + f[11];
    if (!(P2 + cu.rad > vs)) return false;
    if (P0 - cu.al * P2 < -cu.rad * cu.nl) return false;
    if (cu.ar * P2 - P0 < -cu.rad * cu.nr) return false;
    if (P1 - cu.at * P2 < -cu.rad * cu.nt) return false;
    if (cu.ab * P2 - P1 < -cu.rad * cu.nb) return false;
    return true;
}

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

struct TsdfSums { uint32_t W = 0, Sq = 0, Wc = 0, I = 0; };

// one voxel (centre X in the world) in one frame: the rule of include/vslam_hip.h, f64 in the written order
__device__ __forceinline__ void tsdf_sample(const double* __restrict__ f, int b, double X0, double X1, double X2, const VoxelImages& a, const uint8_t* __restrict__ gray,
                                            size_t img_bytes, int pitch, double vs, double tau, double kq, TsdfSums& v) {
#pragma clang fp contract(off)
    const double P0 = f[0] * X0 + f[1] * X1 + f[2] * X2 + f[9], P1 = f[3] * X0 + f[4] * X1 + f[5] * X2 + f[10], P2 = f[6] * X0 + f[7] * X1 + f[8] * X2 + f[11];
    if (!(P2 > vs)) return;
    const double u = a.fx * (P0 / P2) + a.cx, w = a.fy * (P1 / P2) + a.cy;
    const double cf = floor(u + 0.5), rf = floor(w + 0.5);
    if (!(cf >= 0.0 && cf < (double)a.w && rf >= 0.0 && rf < (double)a.h)) return;
    const int c = (int)cf, r = (int)rf;
    const double z = a.fx * a.b / (double)a.disp[((size_t)b * a.h + r) * a.w + c];
    if (!(z > a.z_min && z < a.z_max)) return;
    const double sdf = z - P2;
    if (sdf < -tau) return;
    const int q = (int)rint(fmin(sdf, tau) * kq);
    v.W += 1u; v.Sq += (uint32_t)(q + 1024);
    if (sdf <= tau) { v.Wc += 1u; v.I += gray ? (uint32_t)gray[(size_t)b * img_bytes + (size_t)r * pitch + c] : 0u; }
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

int launch_tsdf_integrate(const TsdfTable& t, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const int32_t* d_map_id, int form,
                          hipStream_t stream) {
    {
        ProfScope ps(stream, "tsdf_frames_kernel");
        hipLaunchKernelGGL(tsdf_frames_kernel, dim3(1), dim3(kVoxelBlock), 0, stream, t, a.T, d_map_id, a.B);
        VS_HIP(hipGetLastError());
    }
    {
        const int vec = voxel_vec(a), hs = (a.h + a.step - 1) / a.step;
        const dim3 grid(voxel_tiles_x(a, vec), (hs + kVoxelTileRows - 1) / kVoxelTileRows, a.B);
        ProfScope ps(stream, "tsdf_alloc_kernel");
        hipLaunchKernelGGL(tsdf_alloc_kernel, grid, dim3(kVoxelBlock), 0, stream, t, a, vec);
        VS_HIP(hipGetLastError());
    }
    TsdfCull cu;
    cu.al = (-0.5 - a.cx) / a.fx; cu.ar = ((double)a.w - 0.5 - a.cx) / a.fx; cu.at = (-0.5 - a.cy) / a.fy; cu.ab = ((double)a.h - 0.5 - a.cy) / a.fy;
    cu.nl = sqrt(1.0 + cu.al * cu.al); cu.nr = sqrt(1.0 + cu.ar * cu.ar); cu.nt = sqrt(1.0 + cu.at * cu.at); cu.nb = sqrt(1.0 + cu.ab * cu.ab);
    cu.rad = (a.fx > 0 && a.fy > 0) ? 7.0 * (double)t.vs : (double)INFINITY;
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
