// tsdf_device.h -- what the surface map's two files share (tsdf_kernels.hip: allocation, integration, extraction; tsdf_mesh_kernels.hip: mesh and
// block loader): the block key, the claim and the lookup in the pool's hash table, the voxel predicates of EXTRACTION and the surfel of a crossing
// edge.  One definition each, so an extracted surfel and a mesh vertex are the same bits.  Include it from a file compiled with FMA contraction off.
// Also the frame row, the cull and the per-sample rule of INTEGRATION, which tsdf_kernels.hip adds with and tsdf_reint_kernels.hip adds and subtracts with.
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

// One row of a frame table (kTsdfFrameDoubles doubles: R, t, the inverse translation, the map id or -1) from a pose and a map id; true when the pose
// is finite by ALLOCATION's test: its seven numbers, the rotation matrix and the inverse translation formed from them
__device__ __forceinline__ bool tsdf_frame_row(const double* Tb, int m, double* f) {
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
    const bool mapped = m >= 0 && m <= kVoxelMaxMap;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { f[9 + i] = Tb[4 + i]; f[12 + i] = tinv[i]; }
    f[15] = (mapped && fin) ? (double)m : -1.0;
    return fin;
}

// what the cull needs of the camera: the slopes of the image rectangle grown by half a pixel and the lengths of the four side planes' normals
struct TsdfCull { double al, ar, at, ab, nl, nr, nt, nb, rad; };

// the cull of a call's camera (fx or fy <= 0: rad is infinite and nothing is culled)
static inline TsdfCull tsdf_cull_of(const TsdfTable& t, const VoxelImages& a) {
    TsdfCull cu;
    cu.al = (-0.5 - a.cx) / a.fx; cu.ar = ((double)a.w - 0.5 - a.cx) / a.fx; cu.at = (-0.5 - a.cy) / a.fy; cu.ab = ((double)a.h - 0.5 - a.cy) / a.fy;
    cu.nl = sqrt(1.0 + cu.al * cu.al); cu.nr = sqrt(1.0 + cu.ar * cu.ar); cu.nt = sqrt(1.0 + cu.at * cu.at); cu.nb = sqrt(1.0 + cu.ab * cu.ab);
    cu.rad = (a.fx > 0 && a.fy > 0) ? 7.0 * (double)t.vs : (double)INFINITY;
    return cu;
}

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

static unsigned tsdf_list_grid(const TsdfTable& t) { // a kernel that walks the block list: no more workgroups than there are slots
    const size_t n_slots = (size_t)1 << t.log2_blocks;
    return (unsigned)(n_slots < (size_t)kTsdfGrid ? n_slots : (size_t)kTsdfGrid);
}

} // namespace vslam
