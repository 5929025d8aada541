// projmatch_kernels.hip -- match by projection (include/vslam_hip.h "match by projection"): one 256-lane workgroup per item.
// The workgroup bins its target image's keypoints into a grid of 32 x 32 px cells in LDS (histogram with ds atomics, scan, scatter of 16-bit
// indices), then walks the item's landmarks with stride 256, a lane per landmark: f64 projection, the cells the window touches, XOR + popcount
// on each candidate's 32 bytes (two 16-byte loads, L2-resident), best and second distance in registers, a 64-bit ds minimum of
// (distance << 32 | index inside the item) into a per-keypoint claims table, and after a barrier a second walk that turns the losers into CONTESTED.
// The order inside a cell cannot reach an output: every reduction is a minimum over integer keys or a count.  No floating-point atomics.
// This translation unit is compiled without contraction (the Makefile's default): the projection is the header's arithmetic, operation by operation.
#include "vslam_internal.h"

namespace vslam {
namespace {

constexpr int kPmBlock = 256;
constexpr float kPmInvCell = 1.0f / 32.0f;   // cells of 32 x 32 px
constexpr unsigned long long kPmFree = ~0ull;

struct PmArgs {
    const int32_t* lm_off; const int32_t* item_img; const double* item_T; const double* lm_xyz; const int32_t* lm_desc_row;
    const uint8_t* src_desc; const vslam_keypoint* kps; const uint8_t* desc; const int32_t* d_n;
    int32_t* match; int32_t* dist; int32_t* n_cand; uint8_t* status;
    size_t desc_stride;
    double fx, fy, cx, cy, r, z_min, z_max, u_max, v_max;
    int n_items, n_landmarks, B, cap, n_src_rows, gw, gh, tau, ratio_pct;
};

__device__ __forceinline__ bool pm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

// clamp(floor(c), 0, n - 1) of a cell coordinate that may be anything, NaN included (-> 0)
__device__ __forceinline__ int pm_clamp_cell(float c, int n) { return c >= (float)n ? n - 1 : (c >= 0.f ? (int)c : 0); }
__device__ __forceinline__ int pm_clamp_cell(double c, int n) { return c >= (double)n ? n - 1 : (c >= 0.0 ? (int)c : 0); }

__device__ __forceinline__ void pm_write(const PmArgs& a, int i, int status, int match, int dist, int n_cand) {
    a.match[i] = match; a.dist[i] = dist; a.status[i] = (uint8_t)status;
    if (a.n_cand) a.n_cand[i] = n_cand;
}

// R (row-major) and t of the item's pose, the header's arithmetic, into rt[12]
__device__ __forceinline__ void pm_pose(const double* q, double* rt) {
#pragma clang fp contract(off)
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    rt[0] = 1 - 2 * (y * y + z * z); rt[1] = 2 * (x * y - z * w); rt[2] = 2 * (x * z + y * w);
    rt[3] = 2 * (x * y + z * w); rt[4] = 1 - 2 * (x * x + z * z); rt[5] = 2 * (y * z - x * w);
    rt[6] = 2 * (x * z - y * w); rt[7] = 2 * (y * z + x * w); rt[8] = 1 - 2 * (x * x + y * y);
    rt[9] = q[4]; rt[10] = q[5]; rt[11] = q[6];
}

// steps 1 and 2 of the rule; returns the status reached (MATCHED = go on to the candidates).  rt lives in LDS: every lane reads the same words
// (a broadcast), and no lane holds the pose in registers across the candidate loops.
__device__ __forceinline__ int pm_project(const PmArgs& a, const double* rt, double X, double Y, double Z, double* u, double* v) {
#pragma clang fp contract(off)
    const double Pz = ((rt[6] * X + rt[7] * Y) + rt[8] * Z) + rt[11];
    if (!(Pz >= a.z_min && Pz <= a.z_max)) return VSLAM_PM_BEHIND;
    const double Px = ((rt[0] * X + rt[1] * Y) + rt[2] * Z) + rt[9];
    const double Py = ((rt[3] * X + rt[4] * Y) + rt[5] * Z) + rt[10];
    *u = (a.fx * Px) / Pz + a.cx;
    *v = (a.fy * Py) / Pz + a.cy;
    if (!(*u >= 0.0 && *u <= a.u_max && *v >= 0.0 && *v <= a.v_max)) return VSLAM_PM_OUTSIDE;
    return VSLAM_PM_MATCHED;
}

// kStage: the image's descriptors are copied into LDS first (32 bytes per keypoint slot more) and the candidates read them there, not from L2
template <bool kStage>
__global__ __launch_bounds__(kPmBlock) void project_match_kernel(const PmArgs a) {
    extern __shared__ __align__(16) unsigned char pm_smem[];
    uint4* sdesc = reinterpret_cast<uint4*>(pm_smem);                              // kStage: cap x 2
    unsigned long long* claims = reinterpret_cast<unsigned long long*>(pm_smem + (kStage ? (size_t)a.cap * 32 : 0));   // cap: min over the item of (d << 32 | index inside the item)
    float2* xy = reinterpret_cast<float2*>(claims + a.cap);                        // cap: pixel of keypoint j
    uint32_t* cell = reinterpret_cast<uint32_t*>(xy + a.cap);                      // gw x gh: count, then start, then end of the cell's list
    uint16_t* list = reinterpret_cast<uint16_t*>(cell + a.gw * a.gh);              // cap: keypoint indices, cell by cell
    __shared__ int s_pm;
    __shared__ double s_rt[12];
    __shared__ uint32_t s_scan[kPmBlock];
    const int m = blockIdx.x, tid = threadIdx.x;

    // the offsets: pm = max(0, lm_off[0 .. m-1]); the item writes [max(lo, pm), min(hi, n_landmarks)) and nothing else
    if (tid == 0) s_pm = 0;
    __syncthreads();
    {
        int mx = 0;
        for (int k = tid; k < m; k += kPmBlock) mx = max(mx, a.lm_off[k]);
        if (mx > 0) atomicMax(&s_pm, mx);
    }
    __syncthreads();
    const int pm = s_pm, lo = a.lm_off[m], hi = a.lm_off[m + 1];
    const int wlo = max(lo, pm), whi = min(hi, a.n_landmarks);
    const int img = a.item_img[m];
    bool ok = pm <= lo && lo <= hi && hi <= a.n_landmarks && img >= 0 && img < a.B;
    {
        double q[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { q[k] = a.item_T[(size_t)m * 7 + k]; ok = ok && pm_finite(q[k]); }
        if (tid == 0) pm_pose(q, s_rt);   // (read after the barriers of the grid build)
    }
    if (!ok) {   // (uniform over the workgroup)
        for (int i = wlo + tid; i < whi; i += kPmBlock) pm_write(a, i, VSLAM_PM_INVALID, -1, -1, 0);
        return;
    }
    if (lo >= hi) return;

    // the target image's keypoints into the grid
    const int n = min(max(a.d_n[img], 0), a.cap), ncell = a.gw * a.gh;
    const vslam_keypoint* kps = a.kps + (size_t)img * a.cap;
    const uint8_t* desc = a.desc + (size_t)img * a.desc_stride;
    for (int c = tid; c < ncell; c += kPmBlock) cell[c] = 0;
    for (int j = tid; j < n; j += kPmBlock) claims[j] = kPmFree;
    if (kStage)
        for (int k = tid; k < 2 * n; k += kPmBlock) sdesc[k] = reinterpret_cast<const uint4*>(desc)[k];
    __syncthreads();
    for (int j = tid; j < n; j += kPmBlock) {
        const float x = kps[j].x, y = kps[j].y;
        xy[j] = make_float2(x, y);
        atomicAdd(&cell[pm_clamp_cell(y * kPmInvCell, a.gh) * a.gw + pm_clamp_cell(x * kPmInvCell, a.gw)], 1u);
    }
    __syncthreads();
    {   // exclusive scan of the counts: a run of cells per lane, the lanes' sums scanned through LDS
        const int per = (ncell + kPmBlock - 1) / kPmBlock, c0 = min(tid * per, ncell), c1 = min(c0 + per, ncell);
        uint32_t sum = 0;
        for (int c = c0; c < c1; ++c) sum += cell[c];
        s_scan[tid] = sum;
        __syncthreads();
        for (int d = 1; d < kPmBlock; d <<= 1) {
            const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        uint32_t run = s_scan[tid] - sum;
        for (int c = c0; c < c1; ++c) { const uint32_t cnt = cell[c]; cell[c] = run; run += cnt; }
    }
    __syncthreads();
    for (int j = tid; j < n; j += kPmBlock) {
        const float2 p = xy[j];
        const uint32_t pos = atomicAdd(&cell[pm_clamp_cell(p.y * kPmInvCell, a.gh) * a.gw + pm_clamp_cell(p.x * kPmInvCell, a.gw)], 1u);
        list[pos] = (uint16_t)j;   // (pos < n: the counts sum to n)
    }
    __syncthreads();   // cell[c] is now the END of cell c's list; its start is cell[c - 1] (0 for c = 0)

    // first walk: steps 1-4, the claim, provisional results
    for (int i = lo + tid; i < hi; i += kPmBlock) {
        const double X = a.lm_xyz[(size_t)i * 3], Y = a.lm_xyz[(size_t)i * 3 + 1], Z = a.lm_xyz[(size_t)i * 3 + 2];
        const int row = a.lm_desc_row[i];
        int status = VSLAM_PM_INVALID, n_cand = 0, best_d = -1, best_j = -1;
        double u, v;
        if (pm_finite(X) && pm_finite(Y) && pm_finite(Z) && row >= 0 && row < a.n_src_rows) status = pm_project(a, s_rt, X, Y, Z, &u, &v);
        if (status == VSLAM_PM_MATCHED) {
            const uint4* dp = reinterpret_cast<const uint4*>(a.src_desc + (size_t)row * 32);
            const uint4 da = dp[0], db = dp[1];
            // the cells the window touches, a 64th of a pixel wider than the window (the exact test below decides; a wider visit costs nothing but time)
            const int cx0 = pm_clamp_cell(((u - a.r) - 0.015625) * (double)kPmInvCell, a.gw), cx1 = pm_clamp_cell(((u + a.r) + 0.015625) * (double)kPmInvCell, a.gw);
            const int cy0 = pm_clamp_cell(((v - a.r) - 0.015625) * (double)kPmInvCell, a.gh), cy1 = pm_clamp_cell(((v + a.r) + 0.015625) * (double)kPmInvCell, a.gh);
            int second = 0x7fffffff;
            best_d = 0x7fffffff; best_j = 0x7fffffff;
            for (int cy = cy0; cy <= cy1; ++cy) {
                // the cells of one grid row are neighbours in the list: one run
                const int c_first = cy * a.gw + cx0, c_last = cy * a.gw + cx1;
                const uint32_t k1 = cell[c_last];
#pragma unroll 1
                for (uint32_t k = c_first ? cell[c_first - 1] : 0u; k < k1; ++k) {
                    const int j = list[k];
                    const float2 p = xy[j];
                    if (!(fabs((double)p.x - u) <= a.r && fabs((double)p.y - v) <= a.r)) continue;
                    ++n_cand;
                    const uint4* cp = kStage ? sdesc + 2 * j : reinterpret_cast<const uint4*>(desc + (size_t)j * 32);
                    const uint4 ca = cp[0], cb = cp[1];
                    const int d = __popc(da.x ^ ca.x) + __popc(da.y ^ ca.y) + __popc(da.z ^ ca.z) + __popc(da.w ^ ca.w) + __popc(db.x ^ cb.x) + __popc(db.y ^ cb.y) +
                                  __popc(db.z ^ cb.z) + __popc(db.w ^ cb.w);
                    if (d < best_d || (d == best_d && j < best_j)) { second = best_d; best_d = d; best_j = j; }
                    else second = min(second, d);
                }
            }
            if (n_cand == 0) { status = VSLAM_PM_NO_CANDIDATE; best_d = -1; }
            else if (best_d > a.tau) status = VSLAM_PM_TOO_FAR;
            else if (a.ratio_pct > 0 && n_cand > 1 && 100 * best_d > a.ratio_pct * second) status = VSLAM_PM_AMBIGUOUS;
            else atomicMin(&claims[best_j], ((unsigned long long)(uint32_t)best_d << 32) | (uint32_t)(i - lo));
        }
        pm_write(a, i, status, status == VSLAM_PM_MATCHED ? best_j : -1, best_d, n_cand);
    }
    __syncthreads();
    // second walk (every lane revisits the landmarks it wrote): a claim that lost is CONTESTED
    for (int i = lo + tid; i < hi; i += kPmBlock) {
        if (a.status[i] != VSLAM_PM_MATCHED) continue;
        const int j = a.match[i];
        if (j < 0 || j >= a.cap) continue;   // (never so after the first walk; nothing but a slot of the table is ever indexed)
        if (claims[j] != (((unsigned long long)(uint32_t)a.dist[i] << 32) | (uint32_t)(i - lo))) { a.status[i] = VSLAM_PM_CONTESTED; a.match[i] = -1; }
    }
}

} // namespace

size_t project_match_lds_bytes(int cap, int gw, int gh, bool stage) { return (size_t)cap * (stage ? 50 : 18) + (size_t)gw * gh * 4; }

int launch_project_match(const vslam_project_match& in, const vslam_project_match_params& p, const double K4[4], int img_w, int img_h, int stage,
                         hipStream_t stream) {
    PmArgs a;
    a.lm_off = in.d_lm_off; a.item_img = in.d_item_img; a.item_T = in.d_item_T; a.lm_xyz = in.d_lm_xyz; a.lm_desc_row = in.d_lm_desc_row;
    a.src_desc = in.d_src_desc; a.kps = in.d_kps; a.desc = in.d_desc; a.d_n = in.d_n;
    a.match = in.d_match; a.dist = in.d_dist; a.n_cand = in.d_n_cand; a.status = in.d_status;
    a.desc_stride = in.desc_stride_bytes ? in.desc_stride_bytes : (size_t)in.kp_capacity * 32;
    a.fx = K4[0]; a.fy = K4[1]; a.cx = K4[2]; a.cy = K4[3]; a.r = (double)p.radius_px; a.z_min = p.z_min; a.z_max = p.z_max;
    a.u_max = (double)(img_w - 1); a.v_max = (double)(img_h - 1);
    a.n_items = in.n_items; a.n_landmarks = in.n_landmarks; a.B = in.B; a.cap = in.kp_capacity; a.n_src_rows = in.n_src_rows;
    a.gw = (img_w + 31) / 32; a.gh = (img_h + 31) / 32; a.tau = p.tau; a.ratio_pct = p.ratio_pct;
    // the staged form only where its LDS leaves room for two workgroups per CU
    const bool staged = stage == 1 && project_match_lds_bytes(a.cap, a.gw, a.gh, true) <= 78 * 1024;
    const size_t smem = project_match_lds_bytes(a.cap, a.gw, a.gh, staged);
    static bool attr_set[16] = {false}; // per device
    int dev = 0;
    VS_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16 || !attr_set[dev]) {
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(project_match_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)project_match_lds_bytes(VSLAM_PROJECT_MATCH_MAX_KP, 128, 128, false)));
        VS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(project_match_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 78 * 1024));
        if (dev >= 0 && dev < 16) attr_set[dev] = true;
    }
    ProfScope prof__(stream, "project_match_kernel");
    if (staged) hipLaunchKernelGGL(project_match_kernel<true>, dim3(in.n_items), dim3(kPmBlock), smem, stream, a);
    else hipLaunchKernelGGL(project_match_kernel<false>, dim3(in.n_items), dim3(kPmBlock), smem, stream, a);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
