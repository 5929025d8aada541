// voxel_device.h -- what the two map stages share (voxel_kernels.hip "dense map", tsdf_kernels.hip "surface map"): the voxel index of a coordinate,
// the hash, the reprojection of a pixel and the image tile a workgroup of 256 lanes walks.  One definition each, so the two stages give the same
// bits.  Include it from a file compiled with FMA contraction off.
#pragma once
#include "vslam_internal.h"

#include "se3_device.h"

namespace vslam {

typedef unsigned long long u64;

constexpr u64 kVoxelEmpty = ~0ull;
constexpr int kVoxelHalf = 1 << 17;   // voxel indices per axis: [-2^17, 2^17)
constexpr int kVoxelBlock = 256;
constexpr int kVoxelTileCols = 64, kVoxelTileRows = 16; // the image tile of a workgroup: a lane holds 4 adjacent pixels of one row

// one axis of the key: cell index + 2^17 and the offset inside the cell in 1/256; false = out of range (a non-finite product included)
__device__ __forceinline__ bool voxel_axis(float x, float inv, uint32_t& cell, uint32_t& off) {
    const float t = __fmul_rn(x, inv);
    const float c = floorf(t);
    cell = 0u; off = 0u;
    if (!(c >= -(float)kVoxelHalf && c < (float)kVoxelHalf)) return false;
    const int o = (int)__fmul_rn(__fsub_rn(t, c), 256.0f); // (t - c rounds to 1.0f for a tiny negative t: the offset saturates at 255)
    cell = (uint32_t)((int)c + kVoxelHalf);
    off = (uint32_t)(o > 255 ? 255 : o);
    return true;
}

__device__ __forceinline__ uint32_t voxel_hash(u64 k) { // (the 64-bit finaliser of MurmurHash3)
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return (uint32_t)k;
}

// ------------------------------------------------------------------------------------------------------------------- reprojection
// T^-1 = (R^T, -R^T t), as geom_kernels.hip's find3d kernels form it
__device__ __forceinline__ void voxel_inverse_pose(const double* T, double Rinv[9], double tinv[3]) {
    double R[9];
    se3::rotmat(T, R);
    Rinv[0] = R[0]; Rinv[1] = R[3]; Rinv[2] = R[6];
    Rinv[3] = R[1]; Rinv[4] = R[4]; Rinv[5] = R[7];
    Rinv[6] = R[2]; Rinv[7] = R[5]; Rinv[8] = R[8];
#pragma unroll
    for (int a = 0; a < 3; ++a) tinv[a] = -(Rinv[3 * a] * T[4] + Rinv[3 * a + 1] * T[5] + Rinv[3 * a + 2] * T[6]);
}

// Frame::find_3d (types_def.cpp:9-18) for a keypoint at ((float)c, (float)r) with disparity d, into the world: f64 math, f32 at rest.
// Returns the depth gate z_min < Z < z_max (false for a disparity that is negative, zero or NaN: the depth is then negative, infinite or NaN).
__device__ __forceinline__ bool reproject_pixel(const VoxelImages& a, const double Rinv[9], const double tinv[3], int c, int r, float d, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    const float u = (float)c, v = (float)r;
    const double x = ((double)u - a.cx) / a.fx, y = ((double)v - a.cy) / a.fy;
    const double depth = a.fx * a.b / (double)d;
    const double X = x * depth, Y = y * depth, Z = depth;
    px = (float)(Rinv[0] * X + Rinv[1] * Y + Rinv[2] * Z + tinv[0]);
    py = (float)(Rinv[3] * X + Rinv[4] * Y + Rinv[5] * Z + tinv[1]);
    pz = (float)(Rinv[6] * X + Rinv[7] * Y + Rinv[8] * Z + tinv[2]);
    return Z > a.z_min && Z < a.z_max;
}
// ... and the same expression for a point at depth Z along the pixel's ray (the surface map's samples before and behind the measured depth)
__device__ __forceinline__ void reproject_ray(const VoxelImages& a, const double Rinv[9], const double tinv[3], int c, int r, double Z, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    const float u = (float)c, v = (float)r;
    const double x = ((double)u - a.cx) / a.fx, y = ((double)v - a.cy) / a.fy;
    const double X = x * Z, Y = y * Z;
    px = (float)(Rinv[0] * X + Rinv[1] * Y + Rinv[2] * Z + tinv[0]);
    py = (float)(Rinv[3] * X + Rinv[4] * Y + Rinv[5] * Z + tinv[1]);
    pz = (float)(Rinv[6] * X + Rinv[7] * Y + Rinv[8] * Z + tinv[2]);
}

// A workgroup's tile of item blockIdx.z: kVoxelTileRows wanted rows x kVoxelTileCols wanted columns, a lane = 4 adjacent wanted pixels of one row.
// With step 1 and a 16-byte aligned base (`vec`) the lane's four disparities are ONE 16-byte load: the tile's columns are then counted from the
// row's last 16-byte boundary (`mis` elements before its first pixel), so every load is aligned whatever w is; a chunk that reaches across the
// row's ends holds the neighbouring rows' pixels, which the lane ignores (c < 0 or c >= w), and the one chunk that would reach past the last
// map's end is read pixel by pixel.
struct VoxelLane { int r, rs; int c[4]; float d[4]; }; // image row, wanted-row index, image columns (-1: none) and their disparities
__device__ __forceinline__ void voxel_lane_load(const VoxelImages& a, int vec, VoxelLane& l) {
    const int tid = threadIdx.x, b = blockIdx.z;
    l.rs = blockIdx.y * kVoxelTileRows + (tid >> 4);
    l.r = l.rs * a.step;
    const int first = blockIdx.x * kVoxelTileCols + (tid & 15) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { l.c[j] = -1; l.d[j] = 0.f; }
    if (l.r >= a.h) return;
    const size_t e0 = ((size_t)b * a.h + l.r) * a.w, total = (size_t)a.B * a.h * a.w;
    const int mis = vec ? (int)(e0 & 3) : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long c = (long long)(first + j) * a.step - mis;
        l.c[j] = (c >= 0 && c < a.w) ? (int)c : -1;
    }
    if (l.c[0] < 0 && l.c[1] < 0 && l.c[2] < 0 && l.c[3] < 0) return;
    const size_t flat = e0 - mis + first; // (vec: the chunk's first element, a multiple of 4)
    if (vec && flat + 4 <= total) {
        const float4 q = *reinterpret_cast<const float4*>(a.disp + flat);
        l.d[0] = q.x; l.d[1] = q.y; l.d[2] = q.z; l.d[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (l.c[j] >= 0) l.d[j] = a.disp[e0 + l.c[j]];
    }
}
static inline int voxel_tiles_x(const VoxelImages& a, int vec) {
    const int ws = (a.w + a.step - 1) / a.step;
    return ((vec ? a.w + 3 : ws) + kVoxelTileCols - 1) / kVoxelTileCols;
}
static inline int voxel_vec(const VoxelImages& a) { return a.step == 1 && reinterpret_cast<uintptr_t>(a.disp) % 16 == 0; }

} // namespace vslam
