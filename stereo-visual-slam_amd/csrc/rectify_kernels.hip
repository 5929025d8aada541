// rectify_kernels.hip -- the stereo rectification stage: raw 8-bit camera images through a fixed-point (x, y, fraction) map into the rectified,
// undistorted images every other stage assumes (include/vslam_hip.h "rectification").  The arithmetic is the published one of OpenCV's
// initUndistortRectifyMap(CV_16SC2) + remap(INTER_LINEAR, BORDER_CONSTANT 0); parity with OpenCV itself is unpinned (tests/rectify_ref.py is the yardstick).
//
//   rectify_build_map   host, double, once per rig: the CV_16SC2 map (xy int16 pairs + 5 + 5 fraction bits)
//   rectify_pack_map    host: map -> the device entry format below
//   rectify_kernel      the gather: one lane = 4 adjacent destination pixels of one row, decoded ONCE and applied to a group of images
#include <algorithm>
#include <cmath>

#include "vslam_internal.h"

namespace vslam {

// ------------------------------------------------------------------------------------------------------------------- host: the map
static void mat3_mul(const double a[9], const double b[9], double c[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

static double mat3_det(const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

static void mat3_inv(const double m[9], double o[9]) {
    const double id = 1.0 / mat3_det(m);
    o[0] = (m[4] * m[8] - m[5] * m[7]) * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = (m[5] * m[6] - m[3] * m[8]) * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = (m[3] * m[7] - m[4] * m[6]) * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// max |R R^T - I| and det R (vslam_rectify_params_check)
void rectify_rotation_error(const double R[9], double* ortho_err, double* det) {
    double e = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
            e = std::fmax(e, std::fabs(d));
        }
    *ortho_err = e; *det = mat3_det(R);
}

// 32 x coordinate -> fixed point: round half to even, integer part saturated to int16, 5 fraction bits
static void rectify_fix(double c32, int16_t* s, int* a) {
    const double lim = 1099511627776.0; // 2^40: a multiple of 32 far outside int16 * 32, so the clip changes no entry that can touch an image
    double t = std::nearbyint(c32);     // (default rounding mode: ties to even)
    t = t < -lim ? -lim : (t > lim ? lim : t);
    const long long i = (long long)t;
    const long long q = i >> 5;
    *s = (int16_t)(q < -32768 ? -32768 : (q > 32767 ? 32767 : q));
    *a = (int)(i & 31);
}

void rectify_build_map(const vslam_rectify_cam& cam, int dst_w, int dst_h, int16_t* xy, uint16_t* frac) {
    const double P3[9] = {cam.P[0], 0, cam.P[2], 0, cam.P[1], cam.P[3], 0, 0, 1};
    double PR[9], M[9];
    mat3_mul(P3, cam.R, PR);
    mat3_inv(PR, M);
    const double fx = cam.K[0], fy = cam.K[1], cx = cam.K[2], cy = cam.K[3];
    const double k1 = cam.D[0], k2 = cam.D[1], p1 = cam.D[2], p2 = cam.D[3], k3 = cam.D[4], k4 = cam.D[5], k5 = cam.D[6], k6 = cam.D[7];
    for (int y = 0; y < dst_h; ++y)
        for (int x = 0; x < dst_w; ++x) {
            const double X = M[0] * x + M[1] * y + M[2], Y = M[3] * x + M[4] * y + M[5], W = M[6] * x + M[7] * y + M[8];
            const double xn = X / W, yn = Y / W, r2 = xn * xn + yn * yn;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = xn * kr + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn);
            const double yd = yn * kr + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn;
            const double u = fx * xd + cx, v = fy * yd + cy;
            const size_t i = (size_t)y * dst_w + x;
            if (!std::isfinite(u) || !std::isfinite(v)) { xy[2 * i] = xy[2 * i + 1] = -32768; frac[i] = 0; continue; } // "outside"
            int ax, ay;
            rectify_fix(32 * u, &xy[2 * i], &ax);
            rectify_fix(32 * v, &xy[2 * i + 1], &ay);
            frac[i] = (uint16_t)(ay * 32 + ax);
        }
}

// Device entry of one destination pixel (8 bytes), everything that does not depend on the image decoded ahead:
//   .x = col0 | row0 << 12 | dx << 24 | dy << 25   the top-left tap CLAMPED into the source, and whether the right / lower tap is one further
//   .y = wx0 | wx1 << 8 | wy0 << 16 | wy1 << 24    the separable weights (32 - ax, ax, 32 - ay, ay), ZERO for a column / row outside the source
// A tap outside the source then reads some pixel inside it with weight 0: "0 per tap" with no branch and no address outside the image.
// Rows are padded to map_pitch = dst_w rounded up to 4 entries with all-zero entries (they write the destination's padding bytes).
int rectify_map_pitch(int dst_w) { return (dst_w + 3) & ~3; }

void rectify_pack_map(const int16_t* xy, const uint16_t* frac, int dst_w, int dst_h, int src_w, int src_h, uint2* out) {
    const int mp = rectify_map_pitch(dst_w);
    auto clampi = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    for (int y = 0; y < dst_h; ++y)
        for (int x = 0; x < mp; ++x) {
            uint2 e = make_uint2(0u, 0u);
            if (x < dst_w) {
                const size_t i = (size_t)y * dst_w + x;
                const int sx = xy[2 * i], sy = xy[2 * i + 1], ax = frac[i] & 31, ay = (frac[i] >> 5) & 31;
                const int c0 = clampi(sx, src_w - 1), c1 = clampi(sx + 1, src_w - 1), r0 = clampi(sy, src_h - 1), r1 = clampi(sy + 1, src_h - 1);
                const uint32_t wx0 = (sx >= 0 && sx < src_w) ? 32 - ax : 0, wx1 = (sx + 1 >= 0 && sx + 1 < src_w) ? ax : 0;
                const uint32_t wy0 = (sy >= 0 && sy < src_h) ? 32 - ay : 0, wy1 = (sy + 1 >= 0 && sy + 1 < src_h) ? ay : 0;
                e.x = (uint32_t)c0 | (uint32_t)r0 << 12 | (uint32_t)(c1 - c0) << 24 | (uint32_t)(r1 - r0) << 25;
                e.y = wx0 | wx1 << 8 | wy0 << 16 | wy1 << 24;
            }
            out[(size_t)y * mp + x] = e;
        }
}

// Source-side form (b): which source box a 256 x 4 destination tile reads, for staging it in LDS.  Per tile {bx0 (a multiple of 16), by0, 16-byte
// chunks per row, rows}, all zero = "gather directly": the tile has no tap with a weight, its box exceeds the LDS slot, or staging would move more
// than kRectifyStageBytesPerPixel bytes per destination pixel (a map without locality: the gathers touch less).
constexpr int kRectifyBoxChunks = 1024;            // 16 KiB of LDS per workgroup: eight workgroups per CU
constexpr int kRectifyStageBytesPerPixel = 8;
void rectify_tile_boxes(const uint2* packed, int dst_w, int dst_h, int4* tiles) {
    const int mp = rectify_map_pitch(dst_w), tx = rectify_tiles_x(dst_w), ty = (dst_h + 3) / 4;
    for (int j = 0; j < ty; ++j)
        for (int i = 0; i < tx; ++i) {
            int cmin = 1 << 30, cmax = -1, rmin = 1 << 30, rmax = -1, npx = 0;
            for (int y = 4 * j; y < std::min(4 * j + 4, dst_h); ++y)
                for (int x = 256 * i; x < std::min(256 * i + 256, dst_w); ++x) {
                    const uint2 e = packed[(size_t)y * mp + x];
                    if (((e.y & 0xFFu) + ((e.y >> 8) & 0xFFu)) == 0 || (((e.y >> 16) & 0xFFu) + (e.y >> 24)) == 0) continue; // no tap has a weight
                    const int c0 = e.x & 0xFFF, r0 = (e.x >> 12) & 0xFFF, c1 = c0 + ((e.x >> 24) & 1), r1 = r0 + ((e.x >> 25) & 1);
                    cmin = std::min(cmin, c0); cmax = std::max(cmax, c1); rmin = std::min(rmin, r0); rmax = std::max(rmax, r1); ++npx;
                }
            int4 t = make_int4(0, 0, 0, 0);
            if (npx > 0) {
                const int bx0 = cmin & ~15, bw16 = (cmax + 1 - bx0 + 15) / 16, bh = rmax - rmin + 1;
                if (bw16 * bh <= kRectifyBoxChunks && bw16 * 16 * bh <= kRectifyStageBytesPerPixel * npx) t = make_int4(bx0, rmin, bw16, bh);
            }
            tiles[(size_t)j * tx + i] = t;
        }
}
int rectify_tiles_x(int dst_w) { return (dst_w + 255) / 256; }

// ------------------------------------------------------------------------------------------------------------------- device: the gather
// Grid: x = 256-pixel strips of a destination row (pitch included), y = 4 rows per workgroup (one wave per row: a wave's stores are 256
// contiguous bytes of one row), z = side x image group.  A lane decodes its four entries once (16 tap offsets, 16 weights) and applies them to
// the kRectifyGroup images of its group: the map's 8 bytes per pixel and the address arithmetic are paid once per group, not once per image.
// Source side, two forms (Tuning::rectify_form):
//   (a) kLds = false: direct byte gathers through the vector cache; neighbouring lanes read neighbouring source bytes, so the four loads of a
//       pixel hit the lines its neighbours fetched.  Image bases are wave-uniform (scalar registers), the offsets 32-bit.
//   (b) kLds = true: per image the tile's source box (rectify_tile_boxes) goes into LDS with 16-byte row loads -- every thread's chunks and
//       their addresses are fixed before the image loop -- and the taps are LDS byte reads.  A tile without a box runs form (a)'s loop.
struct RectifySide { const uint2* map; const int4* tiles; const uint8_t* src; uint8_t* dst; };
struct RectifyArgs {
    RectifySide side[2];
    int groups;                 // image groups per side: ceil(B / kRectifyGroup)
    int B, w_pitch4, h, map_pitch, tiles_x;
    uint32_t src_pitch, dst_pitch;
    size_t src_img_bytes, dst_img_bytes;
    int dword_stores;           // destination base, pitch and image stride are multiples of 4: one dword per lane; else four byte stores
};

template <bool kLds>
__global__ __launch_bounds__(256) void rectify_kernel(const RectifyArgs a) {
    __shared__ uint4 box[kLds ? kRectifyBoxChunks : 1];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + threadIdx.y;
    const bool live = x0 < (int)a.dst_pitch && y < a.h;
    const int s = blockIdx.z >= (unsigned)a.groups ? 1 : 0;
    const int g = blockIdx.z - s * a.groups;
    const uint2* map = s ? a.side[1].map : a.side[0].map;
    const uint8_t* src = s ? a.side[1].src : a.side[0].src;
    uint8_t* dst = s ? a.side[1].dst : a.side[0].dst;
    int4 tile = make_int4(0, 0, 0, 0); // {bx0, by0, chunks per row, rows}
    if (kLds && (int)blockIdx.x < a.tiles_x) tile = (s ? a.side[1].tiles : a.side[0].tiles)[blockIdx.y * a.tiles_x + blockIdx.x];
    const bool staged = kLds && tile.w > 0;          // workgroup-uniform
    if (!staged && !live) return;                    // (no barrier on the gather path)

    uint2 e[4] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
    if (live && x0 < a.map_pitch) { // (map_pitch is a multiple of 4: all four entries exist; beyond it the lane only writes padding zeros)
        const uint4* m = reinterpret_cast<const uint4*>(map + (size_t)y * a.map_pitch + x0);
        const uint4 m0 = m[0], m1 = m[1];
        e[0] = make_uint2(m0.x, m0.y); e[1] = make_uint2(m0.z, m0.w); e[2] = make_uint2(m1.x, m1.y); e[3] = make_uint2(m1.z, m1.w);
    }
    // tap offsets: into the source image (pitch src_pitch, origin 0) or into the staged box (pitch 16 x chunks, origin bx0, by0)
    const uint32_t tp = staged ? 16u * (uint32_t)tile.z : a.src_pitch;
    uint32_t o00[4], o10[4], o01[4], o11[4], w00[4], w10[4], w01[4], w11[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t wx0 = e[k].y & 0xFFu, wx1 = (e[k].y >> 8) & 0xFFu, wy0 = (e[k].y >> 16) & 0xFFu, wy1 = e[k].y >> 24;
        w00[k] = wx0 * wy0; w10[k] = wx1 * wy0; w01[k] = wx0 * wy1; w11[k] = wx1 * wy1;
        uint32_t dx = (e[k].x >> 24) & 1u, dyp = (e[k].x >> 25) & 1u ? tp : 0u;
        uint32_t col = e[k].x & 0xFFFu, row = (e[k].x >> 12) & 0xFFFu;
        if (staged) {
            if ((w00[k] | w10[k] | w01[k] | w11[k]) == 0) { col = row = dx = dyp = 0; } // no weight: the entry lies outside the box; read its origin
            else { col -= (uint32_t)tile.x; row -= (uint32_t)tile.y; }
        }
        o00[k] = row * tp + col;
        o10[k] = o00[k] + dx; o01[k] = o00[k] + dyp; o11[k] = o01[k] + dx;
    }
    // form (b): the chunks of the box this thread stages for every image (at most kRectifyBoxChunks / 256 = 4), fixed before the loop
    uint32_t goff[kRectifyBoxChunks / 256];
    const int n_chunks = tile.z * tile.w;
    if (staged) {
#pragma unroll
        for (int j = 0; j < kRectifyBoxChunks / 256; ++j) {
            const int i = tid + 256 * j, r = i / tile.z, c = i - r * tile.z;
            goff[j] = (uint32_t)(tile.y + r) * a.src_pitch + (uint32_t)tile.x + 16u * (uint32_t)c;
        }
    }
    const int b0 = g * kRectifyGroup, b1 = min(b0 + kRectifyGroup, a.B);
    const uint8_t* sp = src + (size_t)b0 * a.src_img_bytes;
    uint8_t* dp = dst + (size_t)b0 * a.dst_img_bytes + (size_t)y * a.dst_pitch + x0;
    for (int b = b0; b < b1; ++b, sp += a.src_img_bytes, dp += a.dst_img_bytes) {
        uint32_t out = 0;
        if (staged) {
            __syncthreads(); // (the previous image's taps are read)
#pragma unroll
            for (int j = 0; j < kRectifyBoxChunks / 256; ++j)
                if (tid + 256 * j < n_chunks) box[tid + 256 * j] = *reinterpret_cast<const uint4*>(sp + goff[j]);
            __syncthreads();
            const uint8_t* lb = reinterpret_cast<const uint8_t*>(box);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (w00[k] * lb[o00[k]] + w10[k] * lb[o10[k]] + w01[k] * lb[o01[k]] + w11[k] * lb[o11[k]] + 512u) >> 10;
                out |= v << (8 * k);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (w00[k] * sp[o00[k]] + w10[k] * sp[o10[k]] + w01[k] * sp[o01[k]] + w11[k] * sp[o11[k]] + 512u) >> 10;
                out |= v << (8 * k);
            }
        }
        if (!live) continue;
        if (a.dword_stores) *reinterpret_cast<uint32_t*>(dp) = out;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < (int)a.dst_pitch) dp[k] = (uint8_t)(out >> (8 * k));
        }
    }
}

int launch_rectify(const RectifyLaunch& L, hipStream_t stream) {
    RectifyArgs a;
    int n = 0;
    for (int s = 0; s < 2; ++s)
        if (L.map[s] && L.src[s] && L.dst[s]) { a.side[n].map = L.map[s]; a.side[n].tiles = L.tiles[s]; a.side[n].src = L.src[s]; a.side[n].dst = L.dst[s]; ++n; }
    if (n == 0 || L.B <= 0) return VSLAM_OK;
    if (n == 1) a.side[1] = a.side[0];
    a.groups = (L.B + kRectifyGroup - 1) / kRectifyGroup;
    if (n * a.groups > 65535) { set_error("rectify: %d images per side exceed the launch grid (%d)", L.B, 65535 * kRectifyGroup / 2); return VSLAM_ERR_ARG; }
    a.B = L.B; a.h = L.h; a.map_pitch = rectify_map_pitch(L.w); a.tiles_x = rectify_tiles_x(L.w);
    a.src_pitch = (uint32_t)L.src_pitch; a.dst_pitch = (uint32_t)L.dst_pitch;
    a.src_img_bytes = L.src_img_bytes; a.dst_img_bytes = L.dst_img_bytes;
    a.w_pitch4 = (L.dst_pitch + 3) / 4;
    a.dword_stores = 1;
    if (L.dst_pitch % 4 || L.dst_img_bytes % 4) a.dword_stores = 0;
    // form (b) loads 16-byte chunks of source rows: it needs 16-byte aligned rows (then a chunk never crosses a row's end either)
    bool lds = L.form == 1 && L.src_pitch % 16 == 0 && L.src_img_bytes % 16 == 0;
    for (int s = 0; s < n; ++s) {
        if (reinterpret_cast<uintptr_t>(a.side[s].dst) % 4) a.dword_stores = 0;
        if (reinterpret_cast<uintptr_t>(a.side[s].src) % 16 || !a.side[s].tiles) lds = false;
    }
    const dim3 grid((a.w_pitch4 + 63) / 64, (L.h + 3) / 4, n * a.groups), block(64, 4);
    ProfScope ps(stream, "rectify_kernel");
    if (lds) hipLaunchKernelGGL(rectify_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(rectify_kernel<false>, grid, block, 0, stream, a);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
