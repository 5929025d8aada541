// tsdf_render_kernels.hip -- the surface map's ray-cast views (include/vslam_hip.h "RENDER"): what a camera at a given pose sees of the field, as a
// depth image and, per pixel, the surface normal and intensity.  A ray is parametrised by the camera's z; it walks the samples Z_k = z_min + k hs,
// reads the field by trilinear interpolation of D over the eight voxels around a sample, and ends at the first known sample that is not positive: a
// hit if the sample before it was known and positive, a miss otherwise (a back face, or a surface entered from unobserved space).
//
//   tsdf_views_kernel        the call's view table, in the frame table's layout and by its test: R, t, the inverse translation, the map id (-1: no part)
//   tsdf_range_init_kernel   (form 1) every (view, tile) range empty; the whole march for a view whose rotation is not orthonormal
//   tsdf_ray_range_kernel    (form 1) one lane per (claimed block, view): the block's sphere projected onto the view's 16 x 16 tiles, each tile's sample
//                            range [k_lo, k_hi] narrowed with integer atomicMin / atomicMax (order-independent)
//   tsdf_render_kernel       one lane per pixel, a wave an 8 x 8 patch, a workgroup a 16 x 16 tile: the march, the hit, the attributes
// Form 1 skips only samples that cannot be known, so both forms write the same bytes.  No lane waits on another: a lane keeps the last block its
// samples' first corner fell into, as (key, slot or absent), in registers, and a sample in a block known to be absent costs no memory access.
// Compiled with FMA contraction off (the Makefile's default): every value is bit-exact against tests/tsdf_render_ref.py.
#include "vslam_internal.h"

#include "se3_device.h"
#include "tsdf_device.h"

namespace vslam {

constexpr uint32_t kRenderAbsent = 0xFFFFFFFFu; // the cached block has no slot
constexpr int kRenderTile = 16;

struct RenderCache { u64 key = kVoxelEmpty; uint32_t slot = kRenderAbsent; };
struct RenderSample { double D, gx, gy, gz, inten; };

__device__ __forceinline__ double render_lerp(double a, double b, double t) { return a + t * (b - a); }

// ------------------------------------------------------------------------------------------------------------------- the view table
__global__ __launch_bounds__(kVoxelBlock) void tsdf_views_kernel(double* __restrict__ views, const double* __restrict__ T, const int32_t* __restrict__ map_ids, int V) {
    const int v = blockIdx.x * kVoxelBlock + threadIdx.x;
    if (v >= V) return;
    const double* Tb = T + 7 * (size_t)v;
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
    const int m = map_ids[v];
    double* f = views + (size_t)kTsdfFrameDoubles * v;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { f[9 + i] = Tb[4 + i]; f[12 + i] = tinv[i]; }
    f[15] = (m >= 0 && m <= kVoxelMaxMap && fin) ? (double)m : -1.0;
}

// ------------------------------------------------------------------------------------------------------------------- the sample
// The sample at depth Z of the ray (x, y): false = unknown.  kAttr: the gradient and the intensity too, else D alone.
template <bool kAttr>
__device__ __forceinline__ bool render_sample(const TsdfTable& t, const double* __restrict__ f, int map_id, uint32_t min_w, double vs, double x, double y, double Z,
                                              RenderCache& cache, RenderSample& out) {
#pragma clang fp contract(off)
    const double P0 = x * Z, P1 = y * Z;
    // (the view table holds R row-major: Rinv[3a + b] = R[3b + a])
    const double g0 = (f[0] * P0 + f[3] * P1 + f[6] * Z + f[12]) / vs - 0.5;
    const double g1 = (f[1] * P0 + f[4] * P1 + f[7] * Z + f[13]) / vs - 0.5;
    const double g2 = (f[2] * P0 + f[5] * P1 + f[8] * Z + f[14]) / vs - 0.5;
    const double i0 = floor(g0), i1 = floor(g1), i2 = floor(g2);
    const double lo = -(double)kVoxelHalf, hi = (double)kVoxelHalf;
    if (!(i0 >= lo && i0 + 1.0 < hi && i1 >= lo && i1 + 1.0 < hi && i2 >= lo && i2 + 1.0 < hi)) return false; // (a NaN fails every comparison)
    const double f0 = g0 - i0, f1 = g1 - i1, f2 = g2 - i2;
    const uint32_t c0 = (uint32_t)((int)i0 + kVoxelHalf), c1 = (uint32_t)((int)i1 + kVoxelHalf), c2 = (uint32_t)((int)i2 + kVoxelHalf); // each + 1 < 2^18
    const u64 base = tsdf_key(map_id, c0, c1, c2);
    if (base != cache.key) {
        uint32_t s;
        cache.slot = tsdf_find(t, base, s) ? s : kRenderAbsent;
        cache.key = base;
    }
    if (cache.slot == kRenderAbsent) return false; // corner (0, 0, 0) must be good
    double D[8], I[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t vx = c0 + (c & 1), vy = c1 + ((c >> 1) & 1), vz = c2 + (c >> 2);
        const u64 key = tsdf_key(map_id, vx, vy, vz);
        uint32_t slot = cache.slot;
        if (key != base && !tsdf_find(t, key, slot)) return false;
        const uint4 v = t.pool[(size_t)slot * kTsdfLanes + ((vz & 7u) << 6 | (vy & 7u) << 3 | (vx & 7u))];
        if (!tsdf_good(v, min_w)) return false;
        D[c] = tsdf_D(v);
        if (kAttr) I[c] = (double)v.w / (double)v.z;
    }
    out.D = render_lerp(render_lerp(render_lerp(D[0], D[1], f0), render_lerp(D[2], D[3], f0), f1),
                        render_lerp(render_lerp(D[4], D[5], f0), render_lerp(D[6], D[7], f0), f1), f2);
    if (kAttr) {
        out.inten = render_lerp(render_lerp(render_lerp(I[0], I[1], f0), render_lerp(I[2], I[3], f0), f1),
                                render_lerp(render_lerp(I[4], I[5], f0), render_lerp(I[6], I[7], f0), f1), f2);
        // the gradient of the interpolant: the differences along an axis, lerped over the other two axes in the order x, y, z
        out.gx = render_lerp(render_lerp(D[1] - D[0], D[3] - D[2], f1), render_lerp(D[5] - D[4], D[7] - D[6], f1), f2);
        out.gy = render_lerp(render_lerp(D[2] - D[0], D[3] - D[1], f0), render_lerp(D[6] - D[4], D[7] - D[5], f0), f2);
        out.gz = render_lerp(render_lerp(D[4] - D[0], D[5] - D[1], f0), render_lerp(D[6] - D[2], D[7] - D[3], f0), f1);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------------------- the march
struct RenderArgs {
    double fx, fy, cx, cy, z_min, hs;
    int w, h, V, K, tiles_x, tiles_y;
    uint32_t min_w;
    const double* views;   // V x kTsdfFrameDoubles
    const int2* ranges;    // (form 1) V x tiles_y x tiles_x of (k_lo, k_hi); null: every tile walks 0 .. K-1
    float* depth; float4* attr; u64* counts;
};

// blockIdx.x + tile0 = the tile, blockIdx.z + view0 = the view (the launcher cuts grids beyond the device's limits into several)
__global__ __launch_bounds__(kVoxelBlock) void tsdf_render_kernel(TsdfTable t, RenderArgs a, unsigned tile0, int view0) {
#pragma clang fp contract(off)
    const int view = view0 + (int)blockIdx.z;
    const unsigned tile = tile0 + blockIdx.x;
    const int ty = (int)(tile / (unsigned)a.tiles_x), tx = (int)(tile - (unsigned)ty * (unsigned)a.tiles_x);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = tx * kRenderTile + (wave & 1) * 8 + (lane & 7), r = ty * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
    const double* __restrict__ f = a.views + (size_t)kTsdfFrameDoubles * view;
    const int map_id = (int)f[15]; // (workgroup-uniform)
    int k_lo = 0, k_hi = a.K - 1;
    if (a.ranges) {
        const int2 rg = a.ranges[((size_t)view * a.tiles_y + ty) * a.tiles_x + tx]; // (workgroup-uniform)
        k_lo = rg.x > 0 ? rg.x : 0; k_hi = rg.y < a.K - 1 ? rg.y : a.K - 1;
    }
    const bool inside = c < a.w && r < a.h;
    float depth = 0.f;
    float4 attr = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t n_samples = 0u, n_hit = 0u;
    if (inside && map_id >= 0) {
        const double vs = (double)t.vs;
        const double x = ((double)c - a.cx) / a.fx, y = ((double)r - a.cy) / a.fy;
        RenderCache cache;
        RenderSample s;
        bool prev = false, hit = false;
        double D_prev = 0.0;
        int k = k_lo;
        for (; k <= k_hi; ++k) { // (everything outside k_lo .. k_hi is unknown: `prev` is clear there)
            n_samples += 1u;
            if (!render_sample<false>(t, f, map_id, a.min_w, vs, x, y, a.z_min + (double)k * a.hs, cache, s)) { prev = false; continue; }
            if (s.D > 0.0) { prev = true; D_prev = s.D; continue; }
            hit = prev; // the first known sample that is not positive ends the ray
            break;
        }
        if (hit) {
            const double Zs = (a.z_min + (double)(k - 1) * a.hs) + (D_prev / (D_prev - s.D)) * a.hs;
            depth = (float)Zs;
            n_hit = 1u;
            if (a.attr) {
                if (!render_sample<true>(t, f, map_id, a.min_w, vs, x, y, Zs, cache, s))
                    render_sample<true>(t, f, map_id, a.min_w, vs, x, y, a.z_min + (double)k * a.hs, cache, s); // (sample k is known)
                const double norm = sqrt(s.gx * s.gx + s.gy * s.gy + s.gz * s.gz);
                const bool flat = !(isfinite(norm) && norm > 0.0);
                attr = make_float4(flat ? 0.f : (float)(s.gx / norm), flat ? 0.f : (float)(s.gy / norm), flat ? 0.f : (float)(s.gz / norm), (float)s.inten);
            }
        }
    }
    if (inside) {
        const size_t px = ((size_t)view * a.h + r) * a.w + c;
        a.depth[px] = depth;
        if (a.attr) a.attr[px] = attr;
    }
    if (!a.counts) return;
    for (int o = 32; o > 0; o >>= 1) { n_samples += __shfl_xor(n_samples, o); n_hit += __shfl_xor(n_hit, o); }
    if (lane != 0) return;
    if (n_hit) atomicAdd(&a.counts[0], (u64)n_hit);
    if (n_samples) atomicAdd(&a.counts[1], (u64)n_samples);
}

// ------------------------------------------------------------------------------------------------------------------- form 1: the tile ranges
// A view's R is used as the inverse of the sampling map X = R^T P + tinv below; that holds for a unit quaternion only.  A view whose R R^T is not
// the identity to 1e-9 gets the whole march on every tile and no narrowing can widen it further.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_range_init_kernel(RenderArgs a, int2* __restrict__ ranges) {
    const size_t tiles = (size_t)a.tiles_x * a.tiles_y, n = tiles * a.V;
    for (size_t i = (size_t)blockIdx.x * kVoxelBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kVoxelBlock) {
        const double* __restrict__ f = a.views + (size_t)kTsdfFrameDoubles * (i / tiles);
        double dev = 0.0;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) dev = fmax(dev, fabs(f[3 * p] * f[3 * q] + f[3 * p + 1] * f[3 * q + 1] + f[3 * p + 2] * f[3 * q + 2] - (p == q ? 1.0 : 0.0)));
        ranges[i] = dev <= 1e-9 ? make_int2(0x7FFFFFFF, -1) : make_int2(0, a.K - 1);
    }
}

// A sample can be known only if its first corner floor(p / vs - 0.5) lies in a claimed block of the view's map, that is if p lies in the cube of side
// 8 vs around C = (8 b + 4.5) vs: within 4 sqrt(3) vs < 6.93 vs of C.  The sphere used has 7.25 vs plus 4e-9 of the coordinates' magnitude for the
// rounding of the two transforms.  A sample's camera z IS its Z_k, so the sphere bounds k through P2 -+ rad (one more sample either side), and its
// bounding box at the depths z_min or deeper bounds the pixel, widened by one pixel either side.
__global__ __launch_bounds__(kVoxelBlock) void tsdf_ray_range_kernel(TsdfTable t, RenderArgs a, int2* __restrict__ ranges) {
    const u64 n_list = t.counters[0], n = n_list * (u64)a.V;
    const double vs = (double)t.vs;
    for (u64 it = (u64)blockIdx.x * kVoxelBlock + threadIdx.x; it < n; it += (u64)gridDim.x * kVoxelBlock) {
        const u64 i = it / (u64)a.V;
        const int view = (int)(it - i * (u64)a.V);
        const double* __restrict__ f = a.views + (size_t)kTsdfFrameDoubles * view;
        const TsdfBlockId id = tsdf_unpack(t.keys[t.list[i]]);
        if ((int)f[15] != id.map) continue;
        const double C0 = ((double)(8 * id.bx) + 4.5) * vs, C1 = ((double)(8 * id.by) + 4.5) * vs, C2 = ((double)(8 * id.bz) + 4.5) * vs;
        const double P0 = f[0] * C0 + f[1] * C1 + f[2] * C2 + f[9], P1 = f[3] * C0 + f[4] * C1 + f[5] * C2 + f[10], P2 = f[6] * C0 + f[7] * C1 + f[8] * C2 + f[11];
        const double rad = 7.25 * vs + 4e-9 * (fabs(C0) + fabs(C1) + fabs(C2) + fabs(f[9]) + fabs(f[10]) + fabs(f[11]));
        const double zn = fmax(P2 - rad, a.z_min), zf = P2 + rad;
        if (!(zf >= zn)) continue; // wholly in front of z_min (or behind the camera)
        const double kl = floor((zn - a.z_min) / a.hs) - 1.0, kh = ceil((zf - a.z_min) / a.hs) + 1.0;
        if (!(kl <= (double)(a.K - 1))) continue; // wholly beyond z_max
        const int k_lo = kl > 0.0 ? (int)kl : 0, k_hi = kh < (double)(a.K - 1) ? (int)kh : a.K - 1;
        const double xl = P0 - rad, xr = P0 + rad, yt = P1 - rad, yb = P1 + rad;
        const double cl = floor((xl >= 0.0 ? xl / zf : xl / zn) * a.fx + a.cx) - 1.0, cr = ceil((xr >= 0.0 ? xr / zn : xr / zf) * a.fx + a.cx) + 1.0;
        const double rt = floor((yt >= 0.0 ? yt / zf : yt / zn) * a.fy + a.cy) - 1.0, rb = ceil((yb >= 0.0 ? yb / zn : yb / zf) * a.fy + a.cy) + 1.0;
        if (!(cl <= (double)(a.w - 1) && cr >= 0.0 && rt <= (double)(a.h - 1) && rb >= 0.0)) continue; // off the image
        const int tx0 = (cl > 0.0 ? (int)cl : 0) / kRenderTile, tx1 = (cr < (double)(a.w - 1) ? (int)cr : a.w - 1) / kRenderTile;
        const int ty0 = (rt > 0.0 ? (int)rt : 0) / kRenderTile, ty1 = (rb < (double)(a.h - 1) ? (int)rb : a.h - 1) / kRenderTile;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) {
                int2* rg = ranges + ((size_t)view * a.tiles_y + ty) * a.tiles_x + tx;
                atomicMin(&rg->x, k_lo);
                atomicMax(&rg->y, k_hi);
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------- launcher
size_t tsdf_render_table_bytes(int V, int w, int h, int form) {
    const size_t tiles = (size_t)((w + kRenderTile - 1) / kRenderTile) * (size_t)((h + kRenderTile - 1) / kRenderTile);
    return (size_t)V * kTsdfFrameDoubles * sizeof(double) + (form == 1 ? (size_t)V * tiles * sizeof(int2) : 0);
}

int launch_tsdf_render(const TsdfTable& t, const TsdfRenderCall& rc, uint8_t* d_tables, int form, hipStream_t stream) {
    RenderArgs a;
    a.fx = rc.fx; a.fy = rc.fy; a.cx = rc.cx; a.cy = rc.cy; a.z_min = rc.z_min; a.hs = rc.hs;
    a.w = rc.w; a.h = rc.h; a.V = rc.V; a.K = rc.K;
    a.tiles_x = (rc.w + kRenderTile - 1) / kRenderTile; a.tiles_y = (rc.h + kRenderTile - 1) / kRenderTile;
    a.min_w = (uint32_t)(rc.min_weight < 1 ? 1 : rc.min_weight);
    double* views = reinterpret_cast<double*>(d_tables);
    int2* ranges = form == 1 ? reinterpret_cast<int2*>(d_tables + (size_t)rc.V * kTsdfFrameDoubles * sizeof(double)) : nullptr;
    a.views = views; a.ranges = ranges; a.depth = rc.d_depth; a.attr = reinterpret_cast<float4*>(rc.d_attr); a.counts = rc.d_counts;
    if (rc.d_counts) VS_HIP(hipMemsetAsync(rc.d_counts, 0, 2 * sizeof(u64), stream));
    {
        ProfScope ps(stream, "tsdf_views_kernel");
        hipLaunchKernelGGL(tsdf_views_kernel, dim3((unsigned)((rc.V + kVoxelBlock - 1) / kVoxelBlock)), dim3(kVoxelBlock), 0, stream, views, rc.d_T, rc.d_map_id, rc.V);
        VS_HIP(hipGetLastError());
    }
    const size_t tiles = (size_t)a.tiles_x * a.tiles_y;
    if (form == 1) {
        {
            const size_t need = (tiles * rc.V + kVoxelBlock - 1) / kVoxelBlock;
            ProfScope ps(stream, "tsdf_range_init_kernel");
            hipLaunchKernelGGL(tsdf_range_init_kernel, dim3((unsigned)(need > (size_t)kTsdfGrid ? (size_t)kTsdfGrid : need)), dim3(kVoxelBlock), 0, stream, a, ranges);
            VS_HIP(hipGetLastError());
        }
        ProfScope ps(stream, "tsdf_ray_range_kernel");
        hipLaunchKernelGGL(tsdf_ray_range_kernel, dim3(tsdf_list_grid(t)), dim3(kVoxelBlock), 0, stream, t, a, ranges);
        VS_HIP(hipGetLastError());
    }
    ProfScope ps(stream, "tsdf_render_kernel");
    constexpr size_t kMaxTiles = (size_t)1 << 22; // 2^30 lanes a launch
    constexpr int kMaxViews = 65535;
    for (int v0 = 0; v0 < rc.V; v0 += kMaxViews)
        for (size_t t0 = 0; t0 < tiles; t0 += kMaxTiles) {
            const dim3 grid((unsigned)(tiles - t0 < kMaxTiles ? tiles - t0 : kMaxTiles), 1, (unsigned)(rc.V - v0 < kMaxViews ? rc.V - v0 : kMaxViews));
            hipLaunchKernelGGL(tsdf_render_kernel, grid, dim3(kVoxelBlock), 0, stream, t, a, (unsigned)t0, v0);
            VS_HIP(hipGetLastError());
        }
    return VSLAM_OK;
}

} // namespace vslam
