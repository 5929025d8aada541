// tsdf_device.h -- what the surface map's two files share (tsdf_kernels.hip: allocation, integration, extraction; tsdf_mesh_kernels.hip: mesh and
// block loader): the block key, the claim and the lookup in the pool's hash table, the voxel predicates of EXTRACTION and the surfel of a crossing
// edge.  One definition each, so an extracted surfel and a mesh vertex are the same bits.  Include it from a file compiled with FMA contraction off.
#pragma once
#include "vslam_internal.h"

#include "voxel_device.h"

namespace vslam {

constexpr int kTsdfMaxProbe = 128;        // slots a key may probe before it counts as absent (lookup) or dropped (claim)
constexpr int kTsdfLanes = 512;           // the voxels of a block = the lanes of its workgroup
constexpr uint32_t kTsdfMaxW = 1u << 20;  // the sums are exact below this weight (2048 * 2^20 < 2^32)
constexpr int kTsdfBHalf = 1 << 14;       // block coordinates per axis: [-2^14, 2^14)
constexpr int kTsdfGrid = 4096;           // workgroups of the kernels that walk the block list

struct TsdfTally { uint32_t samples = 0, range = 0, full = 0; };

// block key of a voxel whose indices + 2^17 are (cx, cy, cz)
__device__ __forceinline__ u64 tsdf_key(int map_id, uint32_t cx, uint32_t cy, uint32_t cz) {
    return (u64)(uint32_t)map_id << 45 | (u64)(cx >> 3) << 30 | (u64)(cy >> 3) << 15 | (u64)(cz >> 3);
}
__device__ __forceinline__ uint32_t tsdf_probes(const TsdfTable& t) { return t.log2_blocks < 7 ? (1u << t.log2_blocks) : (uint32_t)kTsdfMaxProbe; }

// n samples of one block: the block is claimed if no slot holds it yet
__device__ __forceinline__ void tsdf_claim(const TsdfTable& t, u64 key, uint32_t n, TsdfTally& tally) {
    const uint32_t mask = (1u << t.log2_blocks) - 1u, probes = tsdf_probes(t);
    uint32_t s = voxel_hash(key) & mask, found = 0u;
    for (uint32_t p = 0; p < probes; ++p, s = (s + 1) & mask) {
        u64 k = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == kVoxelEmpty) {
            k = atomicCAS(&t.keys[s], kVoxelEmpty, key);
            if (k == kVoxelEmpty) { // this lane claimed the slot: it enters the list (each slot is claimed once, so the list cannot overflow)
                const u64 i = atomicAdd(&t.counters[0], 1ull);
                t.list[i] = s;
                k = key;
            }
        }
        if (k == key) { found = n; break; }
    }
    tally.samples += found; tally.full += n - found;
}

// read-only: the slot of a block, false if no slot holds it
__device__ __forceinline__ bool tsdf_find(const TsdfTable& t, u64 key, uint32_t& slot) {
    const uint32_t mask = (1u << t.log2_blocks) - 1u, probes = tsdf_probes(t);
    uint32_t s = voxel_hash(key) & mask;
    for (uint32_t p = 0; p < probes; ++p, s = (s + 1) & mask) {
        const u64 k = t.keys[s];
        if (k == key) { slot = s; return true; }
        if (k == kVoxelEmpty) return false;
    }
    return false;
}

struct TsdfBlockId { int map, bx, by, bz; };
__device__ __forceinline__ TsdfBlockId tsdf_unpack(u64 key) {
    TsdfBlockId b;
    b.map = (int)(key >> 45);
    b.bx = (int)((key >> 30) & 0x7FFFu) - kTsdfBHalf; b.by = (int)((key >> 15) & 0x7FFFu) - kTsdfBHalf; b.bz = (int)(key & 0x7FFFu) - kTsdfBHalf;
    return b;
}

__device__ __forceinline__ bool tsdf_good(const uint4& v, uint32_t min_w) { return v.x >= min_w && v.x < kTsdfMaxW && v.z >= 1u; }
__device__ __forceinline__ long long tsdf_num(const uint4& v) { return (long long)v.y - 1024ll * (long long)v.x; }
__device__ __forceinline__ double tsdf_D(const uint4& v) { return (double)tsdf_num(v) / (double)v.x; }

// the sums of voxel (ix, iy, iz) of the map of block `id`: from the staged block if it lies there, else through the table; all zero if no block holds it
__device__ __forceinline__ uint4 tsdf_fetch(const TsdfTable& t, const uint4* lv, const TsdfBlockId& id, int ix, int iy, int iz) {
    if ((ix >> 3) == id.bx && (iy >> 3) == id.by && (iz >> 3) == id.bz) return lv[(iz & 7) << 6 | (iy & 7) << 3 | (ix & 7)];
    if (ix < -kVoxelHalf || ix >= kVoxelHalf || iy < -kVoxelHalf || iy >= kVoxelHalf || iz < -kVoxelHalf || iz >= kVoxelHalf) return make_uint4(0u, 0u, 0u, 0u);
    uint32_t s;
    if (!tsdf_find(t, tsdf_key(id.map, (uint32_t)(ix + kVoxelHalf), (uint32_t)(iy + kVoxelHalf), (uint32_t)(iz + kVoxelHalf)), s)) return make_uint4(0u, 0u, 0u, 0u);
    return t.pool[(size_t)s * kTsdfLanes + ((iz & 7) << 6 | (iy & 7) << 3 | (ix & 7))];
}

// The surfel of the crossing edge from voxel a = ia (sums va, D = Da, staged block lv of block `id`) to b = a + e^ (sums vb): EXTRACTION's arithmetic,
// f64 in the written order, stored as three 16-byte rows
__device__ __forceinline__ void tsdf_surfel(const TsdfTable& t, const uint4* lv, const TsdfBlockId& id, const int* ia, int e, const uint4& va, const uint4& vb, double Da,
                                            uint32_t min_w, double vs, vslam_surfel* __restrict__ dst) {
#pragma clang fp contract(off)
    const int e0 = e == 0, e1 = e == 1, e2 = e == 2;
    const double Db = tsdf_D(vb), tt = Da / (Da - Db);
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll 1
    for (int k = 1; k <= 2; ++k) { // the two axes across the edge: central differences at a and at b where both neighbours are good
        const int fa = (e + k) % 3, f0 = fa == 0, f1 = fa == 1, f2 = fa == 2;
        double sum = 0.0;
        int n = 0;
#pragma unroll 1
        for (int c = 0; c < 2; ++c) {
            const int c0 = ia[0] + c * e0, c1 = ia[1] + c * e1, c2 = ia[2] + c * e2;
            const uint4 vp = tsdf_fetch(t, lv, id, c0 + f0, c1 + f1, c2 + f2), vm = tsdf_fetch(t, lv, id, c0 - f0, c1 - f1, c2 - f2);
            if (tsdf_good(vp, min_w) && tsdf_good(vm, min_w)) { sum += (tsdf_D(vp) - tsdf_D(vm)) / 2.0; n += 1; }
        }
        const double g = n ? sum / (double)n : 0.0;
        if (f0) g0 = g; else if (f1) g1 = g; else g2 = g;
    }
    const double ge = Db - Da;
    if (e0) g0 = ge; else if (e1) g1 = ge; else g2 = ge;
    const double norm = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
    const float x = (float)(e0 ? ((double)ia[0] + 0.5 + tt) * vs : ((double)ia[0] + 0.5) * vs);
    const float y = (float)(e1 ? ((double)ia[1] + 0.5 + tt) * vs : ((double)ia[1] + 0.5) * vs);
    const float z = (float)(e2 ? ((double)ia[2] + 0.5 + tt) * vs : ((double)ia[2] + 0.5) * vs);
    const float inten = (float)(((double)va.w + (double)vb.w) / ((double)va.z + (double)vb.z));
    uint4* o = reinterpret_cast<uint4*>(dst);
    o[0] = make_uint4((uint32_t)ia[0], (uint32_t)ia[1], (uint32_t)ia[2], (uint32_t)e);
    o[1] = make_uint4(va.x < vb.x ? va.x : vb.x, __float_as_uint(x), __float_as_uint(y), __float_as_uint(z));
    o[2] = make_uint4(__float_as_uint((float)(g0 / norm)), __float_as_uint((float)(g1 / norm)), __float_as_uint((float)(g2 / norm)), __float_as_uint(inten));
}

static unsigned tsdf_list_grid(const TsdfTable& t) { // a kernel that walks the block list: no more workgroups than there are slots
    const size_t n_slots = (size_t)1 << t.log2_blocks;
    return (unsigned)(n_slots < (size_t)kTsdfGrid ? n_slots : (size_t)kTsdfGrid);
}

} // namespace vslam
