// vslam_internal.h -- private declarations shared by the HIP translation units of libvslam_hip.so.
// gfx950 (MI355X / CDNA4) only: wave64, 160 KiB LDS per CU, 256 CUs in 8 XCDs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/vslam_hip.h"

namespace vslam {

void set_error(const char* fmt, ...);

#define VS_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            ::vslam::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
            return VSLAM_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)

// ----------------------------------------------------------------------------------------------- stage profiler
// Optional hipEvent brackets around every kernel family (SURVEY.md section 5 "Tracing / profiling").  Enabled per
// context by vslam_profile_enable(); launch functions call PROF_BEGIN/PROF_END, which are no-ops when disabled.
struct Prof;
Prof* prof_current();
void prof_set_current(Prof* p);
void prof_begin(hipStream_t s, const char* name, int launches);
void prof_end(hipStream_t s);
struct ProfScope {
    hipStream_t s;
    ProfScope(hipStream_t st, const char* name, int launches = 1) : s(st) { prof_begin(s, name, launches); }
    ~ProfScope() { prof_end(s); }
};

// ----------------------------------------------------------------------------------------------- device scratch
// Slots bumped over a device buffer, each a whole number of 256-byte units.  With a null base it only measures.
struct Layout {
    uint8_t* base; size_t off = 0;
    explicit Layout(uint8_t* b = nullptr) : base(b) {}
    template <typename T> T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// A growable device buffer of a context, accounted to the context's byte counter.  It only grows, on the first call that needs more,
// after a synchronise of the stream that may still use it.
struct DevBuf {
    const char* name;      // for error messages
    size_t* acct;          // the owning context's dev_bytes
    size_t min_bytes;      // smallest allocation
    uint8_t* p = nullptr; size_t bytes = 0;
    DevBuf(const char* n, size_t* a, size_t min = 0) : name(n), acct(a), min_bytes(min) {}
    int reserve(size_t need, hipStream_t stream);
    void release();
};

// `layout(L&)` states the slots once: it runs against a null base to measure, `buf` grows to fit, and it runs again on `a` to carve `buf`
template <typename L, typename F>
int carve(DevBuf& buf, hipStream_t stream, L& a, F&& layout) {
    L m(nullptr);
    layout(m);
    if (int rc = buf.reserve(m.off, stream)) return rc;
    a.base = buf.p; a.off = 0;
    layout(a);
    if (a.off > buf.bytes) { set_error("%s layout uses %zu bytes of %zu reserved", buf.name, a.off, buf.bytes); return VSLAM_ERR_CAPACITY; }
    return VSLAM_OK;
}
template <typename F>
int carve(DevBuf& buf, hipStream_t stream, F&& layout) { Layout a; return carve(buf, stream, a, layout); }

constexpr int kWave = 64;
constexpr int kNLevels = VSLAM_ORB_NLEVELS;
constexpr int kEdge = 31;            // ORB edgeThreshold
constexpr int kMaxRows = 4096;       // max descriptors per matcher item / keypoints per image through ANMS

// ----------------------------------------------------------------------------------------------- ORB
struct OrbLevel {
    int w, h;          // level size
    float scale;       // (float)pow(1.2, l)
    int nfeat;         // per-level budget
    int pyr_off;       // byte offset of this level inside one image's pyramid buffer (level 0: unused)
    int corner_cap;    // capacity of the FAST corner list of this level
    int corner_off;    // offset (entries) of this level's corner list inside one image's corner buffer
    int tiles_x, tiles_y, tile_off; // FAST tiling of this level
    int tab_off;       // offset into the resize tables (xofs/ialpha) for this level
};

struct OrbPlan {
    OrbLevel lv[kNLevels];
    int w, h;
    int pyr_bytes;        // per image, levels 1..7
    int corner_total;     // per image
    int total_tiles;      // FAST tiles per image, all levels
    int sel_cap;          // per (image, level) capacity of the selected keypoint staging list
    int blur_off[kNLevels]; // byte offset of each level inside one image's blurred pyramid (level 0 included); a level holds pitch x tiled_rows(h) bytes
    int blur_bytes;       // per image
};

// Line-tiled level layout (the blurred pyramid as orb_pyrblur_kernel writes it for orb_describe_kernel<true>): the level is cut into tiles of
// 16 columns x 8 rows, tile (tx, ty) is the 128 contiguous bytes -- one cache line -- at (ty * tiles_per_row + tx) * 128, row r of it the 16 bytes at
// 16 * (r & 7).  tiles_per_row = pitch / 16 (pitches are multiples of 64), and there are ceil(h / 8) tile rows: a level occupies
// pitch * tiled_rows(h) bytes in EITHER layout, so one plan serves both.
// No tiled access leaves the level's allocation: x < pitch and y < tiled_rows(h) give tx < tiles_per_row and ty < tiled_rows(h) / 8, i.e. an offset
// below pitch * tiled_rows(h) -- the last, partial tile row is allocated in full.  The producer stores 16-byte chunks that start at a pixel (x, y)
// of the level (x < w <= pitch, y < h); the consumers read whole chunks of tiles that hold a pixel of a patch which passed the kernel's `inside`
// test, i.e. lies inside the level, or single pixels inside the level.  Bytes of a tile beyond the level's width or height (padding) are
// never written by anyone and may hold anything: no result depends on them.
constexpr int kTileCols = 16, kTileRows = 8, kTileBytes = kTileCols * kTileRows;
__host__ __device__ inline int tiled_rows(int h) { return (h + kTileRows - 1) & ~(kTileRows - 1); }
__host__ __device__ inline uint32_t tiled_offset(int x, int y, int tiles_per_row) {
    return (uint32_t)(((y >> 3) * tiles_per_row + (x >> 4)) * kTileBytes + ((y & 7) << 4) + (x & 15));
}

struct Ctx;

// resize tables (host-computed, OpenCV arithmetic) live in device memory: per level xofs[w], ialpha[2w], yofs[h], ibeta[2h]
struct OrbTables {
    int* d_xofs;      // concatenated over levels 1..7
    short* d_ialpha;
    int* d_yofs;
    short* d_ibeta;
    int x_off[kNLevels], y_off[kNLevels];
    // orb_pyrblur_kernel: source level l is cut into 256 x 64 tiles; tile column tx OWNS the output columns dx of level l + 1 whose
    // left source pixel xofs[dx] falls into it: [tile_dx[tdx_off[l] + tx], tile_dx[tdx_off[l] + tx + 1]); rows likewise
    int* d_tile_dx;
    int* d_tile_dy;
    int tdx_off[kNLevels], tdy_off[kNLevels];
    size_t bytes;     // device memory of the tables above
};

void orb_debug_enable();
void orb_debug_dump(hipStream_t stream);
int orb_plan_init(OrbPlan* plan, int w, int h, int nfeatures, int kp_capacity);
int orb_tables_init(const OrbPlan* plan, OrbTables* t);
void orb_tables_free(OrbTables* t);

struct OrbBuffers {
    uint8_t* d_pyr;        // B x pyr_bytes
    uint32_t* d_corners;   // B x corner_total packed (x | y<<12 | score<<24)
    int32_t* d_corner_cnt; // B x 8
    vslam_keypoint* d_sel; // B x 8 x sel_cap  (per level, raster order, level coords scaled to L0, with angle)
    int32_t* d_sel_cnt;    // B x 8
    int32_t* d_status;     // B  (bit flags: overflow conditions)
    vslam_keypoint* d_det; // B x kp_capacity: detect output (level asc, raster) when ANMS is run as a separate call
    uint8_t* d_blur;       // B x blur_bytes: Gaussian-blurred pyramid (rBRIEF samples these)
    uint8_t* d_rawt;       // B x blur_bytes: line-tiled copy of the raw levels 0..7 (orb_orient_kernel<true> samples these); written only together with a tiled d_blur
    bool blur_tiled;       // layout of d_blur as its most recent producer wrote it: line-tiled (orb_pyrblur_kernel under Tuning::orb_tiled) or row-major
    float2* d_cs;          // B x kp_capacity: per-keypoint (cos, sin) of the rBRIEF rotation
    int32_t* d_order;      // B x kp_capacity: the output slots in (octave, raster) order -- the walk order of orient / describe
    double* d_rad;         // B x kMaxRows: ANMS suppression radii (f64)
    int32_t* d_anms_path;  // B: VSLAM_ANMS_PATH_* of the most recent orb_anms_kernel launch
};

// launches (all asynchronous on `stream`)
int launch_orb_pyramid(const OrbPlan& plan, const OrbTables& tab, const uint8_t* d_imgs, size_t img_bytes, int pitch,
                       int B, uint8_t* d_pyr, hipStream_t stream);
// pyramid level l + 1 AND the blurred level l from ONE staging of the level-l tile (8 launches: the levels depend on each other)
// [r6] ... and, with d_corners != nullptr, FAST + NMS of level l from the same tile (then launch_orb_fast is not called)
// tiled: the blurred levels are written line-tiled (tiled_offset) instead of row-major; launch_orb_describe must be told the same.
// tiled and d_rawt != nullptr: a line-tiled copy of raw levels 0..7 goes to d_rawt as well (B x blur_bytes, the blurred pyramid's plan), for launch_orb_orient
int launch_orb_pyrblur(const OrbPlan& plan, const OrbTables& tab, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, uint8_t* d_pyr,
                       uint8_t* d_blur, bool tiled, uint8_t* d_rawt, int fast_thr, uint32_t* d_corners, int32_t* d_corner_cnt, int32_t* d_status, hipStream_t stream);
int launch_orb_fast(const OrbPlan& plan, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, const uint8_t* d_pyr,
                    int fast_thr, uint32_t* d_corners, int32_t* d_corner_cnt, int32_t* d_status, hipStream_t stream);
int launch_orb_select(const OrbPlan& plan, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, const uint8_t* d_pyr,
                      const uint32_t* d_corners, const int32_t* d_corner_cnt, vslam_keypoint* d_sel, int32_t* d_sel_cnt,
                      int32_t* d_status, hipStream_t stream);
// gather per-level lists (level asc) -> ANMS(num) -> regroup by octave -> d_kps (B x kp_capacity), d_count
// anms_num <= 0: no ANMS (detect order).  regroup: apply cv::ORB::compute's border cull + octave regrouping.
// anms_cap: Tuning::anms_cap as it stands (-1 = one grid cell).  d_path[b]: which way image b went (VSLAM_ANMS_PATH_*).
int launch_orb_anms(const OrbPlan& plan, int B, const vslam_keypoint* d_sel, const int32_t* d_sel_cnt, int sel_cap,
                    int anms_num, int regroup, vslam_keypoint* d_kps, float2* d_cs, int32_t* d_order, int kp_capacity, int32_t* d_count, int32_t* d_status,
                    double* d_rad, int anms_cap, int32_t* d_path, hipStream_t stream);
// same ANMS kernel on a flat list per image (d_in: B x in_capacity, d_nin[b]) for the stand-alone vslam_anms call
int launch_anms_flat(int B, const vslam_keypoint* d_in, const int32_t* d_nin, int in_capacity, int anms_num, int regroup,
                     int img_w, int img_h, vslam_keypoint* d_kps, float2* d_cs, int32_t* d_order, int kp_capacity, int32_t* d_count, int32_t* d_status,
                     double* d_rad, int anms_cap, int32_t* d_path, hipStream_t stream);
int launch_orb_blur(const OrbPlan& plan, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, const uint8_t* d_pyr, uint8_t* d_blur,
                    hipStream_t stream);
int launch_orb_orient(const OrbPlan& plan, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, const uint8_t* d_pyr, vslam_keypoint* d_kps,
                      float2* d_cs, const int32_t* d_order, int kp_capacity, const int32_t* d_count, const uint8_t* d_rawt, hipStream_t stream);
int launch_orb_describe(const OrbPlan& plan, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, const uint8_t* d_pyr,
                        const uint8_t* d_blur, const vslam_keypoint* d_kps, const float2* d_cs, const int32_t* d_order, int kp_capacity, const int32_t* d_count,
                        uint8_t* d_desc, bool tiled, hipStream_t stream);

// ----------------------------------------------------------------------------------------------- matcher
struct MatchBuffers {
    uint32_t* d_train_best; // B x max_rows : (dist << 16 | query index) per train row
};
int launch_match(const uint8_t* d_q, size_t q_stride, const int32_t* d_nq, const uint8_t* d_t, size_t t_stride,
                 const int32_t* d_nt, const double* d_gap, int gate, double ratio, double gap_thr, int B, int max_rows,
                 uint32_t* d_train_best, vslam_dmatch* d_out, int out_capacity, int32_t* d_nout, hipStream_t stream,
                 const int32_t* d_qsel = nullptr, int sel_cap = 0, const int32_t* d_nqsel = nullptr, const int32_t* d_qitem = nullptr, int n_qitems = 0);

// ----------------------------------------------------------------------------------------------- geometry
struct CamParams { double fx, fy, cx, cy, b, dmin, dmax, drel, row_tol; };
// item b's disparity map starts at d_disp + b * item_stride, its rows are dstride elements apart
int launch_find3d_disparity_batch(const vslam_keypoint* d_kps, const int32_t* d_n, int kp_capacity, int B, const float* d_disp, int w, int h,
                                  int dstride, size_t item_stride, const double* d_T, CamParams cam, float* d_xyz, uint8_t* d_valid, uint8_t* d_rel,
                                  hipStream_t stream);
int launch_triangulate(const float* d_uvL, const float* d_uvR, const int32_t* d_n, int capacity, int B, const double* d_T,
                       CamParams cam, float* d_xyz, uint8_t* d_valid, uint8_t* d_rel, hipStream_t stream);
// f2f matches + per-keypoint 3-D points of the query frame -> compact (xyz, uv) PnP inputs (ordered, valid only)
int launch_build_pnp_inputs(const vslam_dmatch* d_m, const int32_t* d_nm, int match_capacity, const vslam_dmatch* d_lr,
                            const int32_t* d_nlr, int lr_capacity, const float* d_xyz_lr, const uint8_t* d_valid_lr,
                            const vslam_keypoint* d_kpsT, int kp_capacity, int B, int32_t* d_kp2lr, float* d_xyz_out, float* d_uv_out,
                            int32_t* d_nout, int out_capacity, hipStream_t stream, const int32_t* d_seg_start = nullptr);
int launch_gather_uv(const vslam_keypoint* d_kpsQ, const vslam_keypoint* d_kpsT, int kp_capacity, const vslam_dmatch* d_m,
                     const int32_t* d_nm, int match_capacity, int B, float* d_uvQ, float* d_uvT, hipStream_t stream);

int launch_hbm_copy_probe(const void* src, void* dst, size_t bytes, int variant, hipStream_t stream);
int hbm_copy_probe_variants();
const char* hbm_copy_probe_name(int variant);

// ----------------------------------------------------------------------------------------------- LM
struct LmWindowArgs {
    int n_windows, n_kf;
    const int32_t* n_kf_w;  // n_windows: keyframes of window w (<= n_kf, the pose stride), or null
    const int32_t* lm_off;
    const int32_t* edge_off;
    double* T;              // n_windows x n_kf x 7
    float* xyz;             // total_lm x 3
    const uint8_t* reliable;
    uint8_t* lm_inlier;
    const int32_t* kf_idx;
    const int32_t* lm_idx;
    const float* uv;
    double* chi2;
    vslam_lm_stats* stats;
    // scratch (sized by total_lm / total_edge)
    double* P;      // total_lm x 3   current landmark estimates
    double* Ptrial; // total_lm x 3
    double* Hll;    // total_lm x 6 (only the first trial of a call stores it: its lambda comes out of the same pass)
    double* bl;     // total_lm x 3
    double* Dinv;   // total_lm x 6
    double* lin;    // total_edge x 2 : Huber weight per edge at the current / at the trial state, keyframe-major
    int32_t* lm_ptr;   // total_lm + n_windows (CSR by landmark, window-local edge ids, built in-kernel)
    int32_t* kf_ptr;   // n_windows x (MAX_KF + 1)
    int32_t* kf_edges; // total_edge: landmark id of the edge stored at keyframe-major position j
    int32_t* pair_ptr; // n_windows x (NPAIR + 1)
    int32_t* pair_hits;// Schur hit records of the off-diagonal keyframe pairs: {pos1 | pos2 << 16, landmark} (8 B each)
    int32_t hit_capacity_per_edge; // UNUSED (nobody sets or reads it): kept because the kernels take this struct by value
    double K[4];
    double huber_delta;
    double* chi2_thr; // n_windows: final adaptive threshold of the last pass
    size_t total_lm, total_edge;
};
// mode 0 = optimize_map (EdgeProjection + Schur), 1 = optimize_pose_only.
// Kernel-choice overrides of a context (tuning aid / tests): -1 = the library's batch-size rule.  Seeded ONCE at vslam_create from the
// VSLAM_* environment variables of the same names (validated there), changed afterwards only through vslam_set_tuning -- no getenv on
// the call path (it races with a host that mutates its environment).
constexpr int kPoseOnlyNarrowWaves = 4; // the narrow form of pose_only_wave_kernel that the library builds next to VSLAM_MAX_KF waves per window
struct Tuning {
    int orb_fuse_min = -1;    // VSLAM_ORB_FUSE_MIN: images per call from which orb_pyrblur_kernel replaces resize + blur
    int orb_tiled = -1;       // VSLAM_ORB_TILED: 0 = orb_pyrblur_kernel writes the blurred pyramid row-major and orb_describe_kernel gathers rows (the form before the
                              // line-tiled layout, kept for before / after measurements); default / 1: line-tiled whenever the fused kernel runs.  Same bits either way
    int anms_cap = -1;        // VSLAM_ANMS_CAP: pixels of cleared distance at which orb_anms_kernel's radius walk stops early (0 = never: the full walk;
                              // default: one cell of its grid).  Same bits either way: a selection the cap could have changed is redone without it
    int sgbm_fuse_min = -1;   // VSLAM_SGBM_FUSE_MIN: pairs per call from which sgbm_down_kernel replaces hsum / vsum / path<0,1>
    int sgbm_fwd_min = -1;    // VSLAM_SGBM_FWD_MIN: pairs per call from which sgbm_forward_kernel replaces three path kernels
    int sgbm_fw_rows = -1;    // VSLAM_SGBM_FW_ROWS: 32 or 64 image rows per slab of the forward sweep
    int pose_only_window = -1; // VSLAM_POSE_ONLY_WINDOW: 1 = the schedule's pose-only pass on lm_window_kernel instead of pose_only_wave_kernel
    int pose_only_waves = -1; // VSLAM_POSE_ONLY_WAVES: waves per window of pose_only_wave_kernel -- VSLAM_MAX_KF (one keyframe per wave) or kPoseOnlyNarrowWaves (a wave runs a list of
                              // keyframes, two windows share a CU); 0 = default: VSLAM_MAX_KF when a launch has at most as many windows as the device has CUs, else the narrow form; same bits either way
    int pnp_window = -1;      // VSLAM_PNP_WINDOW: 1 = single-pose problems on lm_window_kernel<pnp> instead of pnp_wave_kernel
    int ba_lanes = -1;        // VSLAM_BA_LANES: 256 | 512 = lanes per window of ba_resident_kernel (default: 512 when a launch has at most as many windows as the device has CUs, else 256 -- two windows per CU; same bits either way)
    int ba_resident = -1;     // VSLAM_BA_RESIDENT: 0 = optimize_map windows always on lm_window_kernel; 1 = on ba_resident_kernel whenever they fit its LDS budget;
                              // default: ba_resident_kernel for the windows that fit and have at most 2.2 observations per landmark (the windows of a real sequence)
    int track_rule = -1;      // VSLAM_TRACK_RULE: which frame-to-frame matches continue a track in vslam_build_windows_dev.  1 (default) = the reference's tracking()
                              // (visual_odometry.cpp:568-599): whenever the last-frame keypoint is a feature -- created there or tracked into it; one without a depth of its own
                              // is judged by the pose stage's inlier rule on its landmark's map position (:260-270, :277).  0 = the convention of rounds 4-5: only when the
                              // last-frame keypoint owns a valid depth (kept for before / after measurements)
    int rectify_form = -1;    // VSLAM_RECTIFY_FORM: source side of rectify_kernel -- 0 = direct byte gathers, 1 = each tile's source box staged in LDS (default 1; tiles whose box does not pay gather either way)
    int pg_precond = -1;      // VSLAM_PG_PRECOND: preconditioner of pose_graph_kernel's conjugate gradients -- 0 = block-Jacobi, 1 = chain (block-tridiagonal); default: the rule of DESIGN.md 5.10
    int voxel_form = -1;      // VSLAM_VOXEL_FORM: voxel_fuse_kernel -- 0 = every point straight into the global table, 1 = a workgroup sums its image tile in an LDS hash table first (same table either way)
    int tsdf_render_form = -1; // VSLAM_TSDF_RENDER_FORM: vslam_tsdf_render_dev -- 0 = every ray walks all K samples, 1 = tsdf_ray_range_kernel narrows each tile's sample range first (same bytes either way); default: DESIGN.md 5.15
    int tsdf_dist_form = -1;  // VSLAM_TSDF_DIST_FORM: vslam_tsdf_distance_dev -- 0 = tsdf_dist_brute_kernel walks the site masks around every voxel, 1 = the separable transform in three passes (same bytes either way); default: DESIGN.md 5.17
    int tsdf_form = -1;       // VSLAM_TSDF_FORM: tsdf_integrate_kernel -- 0 = every block walks all frames of the call, 1 = tsdf_cull_kernel writes a frame mask per block first (same sums either way); default: DESIGN.md 5.13
    int ba_adaptive = -1;     // VSLAM_BA_ADAPTIVE: 0 = the BA schedule runs all three optimize_map passes for every window (default: a pass that flags nothing new is continued instead of repeated)
    int pm_stage = -1;        // VSLAM_PM_STAGE: project_match_kernel -- 1 = the target image's descriptors staged in LDS (where two workgroups per CU still fit), 0 = read from L2; default: DESIGN.md 5.12
    int fba_store = -1;       // VSLAM_FBA_STORE: 1 = full_ba_kernel keeps (P, B) of every observation from the linearisation (default), 0 = recomputes them in every conjugate-gradient phase
};
// scratch: the context's SGBM buffer.  Its first 256-byte slot is a header of int32 words: the forward sweep's ticket pools, then its error word.
constexpr int kSgbmTicketPools = 8;
constexpr int kSgbmErrorWord = kSgbmTicketPools; // error word of the most recent launch (vslam_sgbm_status_dev)
// sp: a set that vslam_sgbm_params_check accepts for (w, h).  The reference's set keeps its batch-size dispatch (fused sweeps), any other runs the line kernels at every batch size.
int launch_sgbm(const Tuning& tune, const vslam_sgbm_params& sp, const uint8_t* d_left, const uint8_t* d_right, size_t img_bytes, int pitch, int w, int h, int B,
                float* d_disp_f32, int16_t* d_disp_i16, int16_t* d_disp_raw, DevBuf& scratch, hipStream_t stream);

// ba_resident_kernel's arguments (ba_resident.hip: optimize_map / the BA schedule on windows whose landmark state fits the LDS of one CU; the rest is
// marked in `defer`).  launch_lm_windows fills them: the scratch pointers are slices of lm_window_kernel's own scratch (carve_lm), so that both kernels
// run in one launch set on one buffer.  ba_resident_kernel's slice <- lm_window_kernel's, and who owns it when:
//   tab   <- Hll     (6 x total_lm doubles)  ba_resident_kernel: perm / mstat / working positions;  lm_window_kernel: H_ll of the first trial
//   xin   <- Ptrial  (3 x total_lm doubles)  input positions as f32, sorted;                        trial landmark estimates
//   Pbak  <- P       (3 x total_lm doubles)  accepted positions while a trial sits in LDS;          current landmark estimates
//   Dc    <- Dinv    (6 x total_lm doubles)  D^-1 of the multi-observation landmarks;               D^-1 of every landmark
//   blc   <- bl      (3 x total_lm doubles)  their b_l;                                             b_l of every landmark
//   uv_s  <- uvk     (2 x total_edge floats) observations slot-major;                               observations keyframe-major
//   epos  <- kf_pos  (total_edge int32)      caller's edge id per slot-major position;              keyframe-major position per edge
// Sharing is safe because every one of them is cut into PER-WINDOW slices (by lm_off / edge_off) that only the workgroup of that window touches, and
// within a launch set a window's optimize_map passes run on exactly one of the two kernels: ba_resident_kernel comes first on the stream and writes
// defer[w]; lm_window_kernel returns at once for defer[w] == 0 and, for a window left to it (even one given up half-way), rebuilds its slices from the
// caller's arrays.  The schedule's pose-only pass, after both, takes every window and also reads nothing that the passes left in scratch.
struct RsArgs {
    LmWindowArgs a;
    float2* uv_s;          // total_edge: observations, slot-major per window: slot q of sorted landmark s at [slotoff[q] + s]
    int32_t* epos;         // total_edge: caller's edge id (window-local) at the same position
    double* tab;           // 6 x total_lm doubles of scratch; window slice [6 lm0, 6 (lm0 + nl)) holds, as u16: perm[nl] (sorted position ->
                           // landmark id, window-local), mstat[nl] (keyframe set (12 bits) | slot of the landmark's last edge << 12, sorted order)
    double* xin;           // 3 x total_lm doubles of scratch; window slice holds, as f32, the input positions in sorted order (3 nl floats)
    double* Pbak;          // 3 x total_lm: the accepted positions while a trial sits in LDS
    double* Dc;            // 6 x total_lm: D^-1 = (H_ll + lambda I)^-1 of the multi-observation landmarks, sorted order, 48 B records (hit-major phase)
    double* blc;           // 3 x total_lm: their b_l, 24 B records
    int32_t* status;
    int32_t* passes;
    int32_t* defer;        // n_windows: 1 = window left to lm_window_kernel
    const int32_t* order;
    long long* dbg;
    int dyn_bytes;
    int dyn_narrow;        // the dynamic LDS of the 256-lane form: WHICH windows the kernel takes and on which path (hit-major / row-wise) is decided against it in both widths, so that a window's bits do not depend on the width
    int want_chi2;
    int dense_to_general;  // 1: windows with more than 2.2 observations per landmark are left to lm_window_kernel (Tuning::ba_resident = 1 forces them here)
};

// Every decision of one launch_lm_windows call, taken once (plan_lm_windows, lm_kernels.hip) from the call's shape, the context's Tuning and the
// device's CU count; the launchers only execute it.  The reasons for the rules stand at the Tuning fields.
struct LmPlan {
    bool schedule;         // the BA schedule of run_vslam.cpp:58-71 (else one pass of the caller's mode)
    bool resident;         // ba_resident_kernel runs first and takes the optimize_map passes of the windows it does not mark in `defer`
    bool adaptive;         // schedule: one launch per kernel runs a window's passes back to back (else three launches, every pass for every window)
    bool dense_to_general; // resident: windows above 2.2 observations per landmark are deferred too
    bool order;            // lm_order_kernel deals the windows largest first
    bool po_window;        // schedule: the pose-only pass on lm_window_kernel, else on pose_only_wave_kernel ...
    int po_waves;          // ... with this many waves per window
    int ba_lanes;          // resident: 256 | 512 lanes per window
    int launches;          // what the stage profiler is told: 1, 2 (adaptive) or 4 (plain schedule), + resident; lm_order_kernel and lm_fill_kernel are not counted
};

// What the most recent launch on a context's LmScratch left for vslam_ba_status_dev / _schedule_passes_dev / _deferred_dev.  Replaced whole by
// every launcher that carves the scratch (launch_lm_windows, launch_pnp's window form) and by vslam_ba_chain_dev, never field by field.
struct LmLast {
    int32_t* status = nullptr; int n = 0; // per window: VSLAM_OK or why the kernel rejected its graph; windows of that launch
    int32_t* passes = nullptr;  // optimize_map passes executed per window -- written by a schedule only: after any other launch the slot holds whatever it held
    int32_t* defer = nullptr;   // per window: 1 = left to lm_window_kernel by ba_resident_kernel ...
    bool defer_valid = false;   // ... written by that launch (it involved ba_resident_kernel); false: every window ran on lm_window_kernel
    // after a chain: the caller's windows with the status of the step that ran each; the per-launch diagnostics describe single steps and are not available
    static LmLast of_chain(int32_t* status, int n) { LmLast l; l.status = status; l.n = n; return l; }
};
// device scratch of the LM kernels: owned by the context (two contexts / streams must not share it), grown on demand
struct LmScratch {
    DevBuf buf, cyc; // the kernels' scratch; the phase clocks of the LM kernels (VSLAM_LM_PROFILE), kDbgSlots per window
    const Tuning* tune; // the owning context's overrides
    // tuning aids, read from the environment ONCE by vslam_create: VSLAM_LM_PROFILE (phase clocks of the window kernels to stderr), with it
    // VSLAM_RS_PROFILE (those of ba_resident_kernel first) and VSLAM_PO_PROFILE (the clocks are cleared before the pose-only pass: only that pass shows)
    bool prof_lm = false, prof_rs = false, prof_po = false;
    // lm_device_ready, on the first LM launch of the context: every instance of lm_window_kernel and ba_resident_kernel may use more than 64 KB of
    // dynamic LDS on this context's device; ba_resident_kernel's dynamic LDS at 256 lanes (two windows per CU) and at 512 (the whole CU); the CU count
    bool dev_ready = false;
    int rs_narrow_bytes = 0, rs_full_bytes = 0, cu_count = 0;
    LmLast last;
    LmScratch(size_t* acct, const Tuning* t) : buf("LM scratch", acct), cyc("LM clock buffer", acct), tune(t) {}
};
int rs_device_ready(int device, LmScratch& s); // ba_resident.hip's half of lm_device_ready
// iters / update_poses / update_lms: of a single pass (plan.schedule false)
int launch_ba_resident(const RsArgs& ra, const LmPlan& plan, int iters, int update_poses, int update_lms, hipStream_t stream);
int launch_lm_windows(const LmWindowArgs& a, int schedule, int mode, int iters, int update_poses, int update_lms, LmScratch* scratch,
                      hipStream_t stream);
// The fetchers synchronise the stream.  Kept as they were (bench.py relies on them): lm_fetch_status does NOT compare n_windows with the last launch's
// count (asking for more reads past the status words), the other two refuse n_windows beyond it; lm_fetch_passes after a launch that was no schedule
// returns whatever the slot holds; lm_fetch_deferred after a launch without ba_resident_kernel returns all 1.
int lm_fetch_status(const LmScratch* scratch, int n_windows, int32_t* h_status, hipStream_t stream);
int lm_fetch_passes(const LmScratch* scratch, int n_windows, int32_t* h_passes, hipStream_t stream);
int lm_fetch_deferred(const LmScratch* scratch, int n_windows, int32_t* h_defer, hipStream_t stream);

struct PnpArgs {
    const float* xyz; const float* uv; const int32_t* n; int capacity; int B;
    double* T; int iters; double K[4]; double huber_delta; double reproj_thr;
    uint8_t* inlier; int32_t* n_inliers; vslam_lm_stats* stats;
    int n_hint; // points per problem when the host knows it (0 = unknown): picks the kernel in launch_pnp
};
int launch_pnp(const PnpArgs& a, LmScratch* scratch, hipStream_t stream);
int launch_edge_jacobians(int n, const float* d_xyz, const float* d_uv, const double* d_T, const double K[4], double delta, double* d_err, double* d_Jp, double* d_Jl,
                          double* d_chi2, double* d_hw, hipStream_t stream);
// pnp_kernels.hip: cv::solvePnPRansac for B problems of up to `capacity` points -- H 5-point subsets each, EPnP per subset (one wave each), f32 inlier
// scoring, the sequential acceptance rule replayed per problem.  tables (optional): where the B x H hypothesis tables lie in `scratch` -- [R | t]
// (12 doubles), ok flag, inlier count (0 where ok == 0) -- valid until the next launch on that scratch
struct RansacTables { const double* Rt; const int32_t* ok; const int32_t* counts; };
int launch_pnp_ransac_batch(const float* d_xyz, const float* d_uv, const int32_t* d_n, int capacity, int B, int H, const double K[4], double reproj_err,
                            double confidence, DevBuf& scratch, double* d_T, uint8_t* d_inlier, int32_t* d_n_inl, int32_t* d_iters, hipStream_t stream,
                            RansacTables* tables = nullptr);
// track_kernels.hip: BA windows of a batch of consecutive keyframes from the front end's device-resident output.  launch_build_windows and
// launch_map_pnp_inputs share one front half (dims, node tables, pairing, init, link, walk); KfPolicy says what the window builder adds to it.
// Which keyframes a window holds (vslam_build_windows_kf_dev): policy -1 = the sliding window with no set outputs (vslam_build_windows_dev),
// 0 = the sliding window with its sets written to kf_frame / evicted, 1 = the reference's culling (needs extra scratch).
// gate (vslam_build_windows_gated_dev): insert_key_frame's keyframe gate on num_inliers (n_frames - 1) and T_rel, states to frame_state; policy 0 / 1.
// map (vslam_build_windows_map_dev): the poses G (n_frames x 7) come from the caller instead of the chain of d_T_rel, and when in_of_match is set
// ((n_frames - 1) x match_capacity) the links are decided through it: match k of item i holds when in_of_match >= 0 and that input's d_pose_inlier flag is set.
// gate with state_in (vslam_build_windows_map_gated_dev): the frame states are the caller's (n_frames), not computed from num_inliers / T_rel.
struct KfPolicy { int policy; double near_dist; int32_t* kf_frame; int32_t* evicted; bool gate = false; const int32_t* num_inliers = nullptr; int32_t* frame_state = nullptr;
                  const double* G = nullptr; const int32_t* in_of_match = nullptr; const int32_t* state_in = nullptr;
                  // recover (vslam_build_windows_map_recover_dev; with gate, G, state_in): the states also give the pairing of every frame with its last
                  // accepted predecessor; pred_table (n_frames) is the pairing in.d_f2f was built on -- a pair's links hold only where the two agree
                  bool recover = false; const int32_t* pred_table = nullptr;
                  // vslam_set_window_ids: per landmark of the concatenated array, the root node of its track (frame x kp_capacity + keypoint); null: not written
                  int32_t* lm_id = nullptr; };
// The segment table of a context as the launchers see it (vslam_set_segments; all null / 0: the batch is one sequence): start[f] = first frame of
// f's segment (n_frames), first (n_seg + 1), qitem[i] = i, or -1 for the item before a segment's first frame (n_frames - 1).
struct SegView { const int32_t* start = nullptr; const int32_t* first = nullptr; const int32_t* qitem = nullptr; int n_seg = 0; };
int launch_seg_expand(int n_frames, int n_seg, const int32_t* d_first, int32_t* d_start, int32_t* d_qitem, hipStream_t stream);
// What both builders' walk takes from the context: K4 = {fx, fy, cx, cy}, reproj_thr (pixels), track_rule resolved to 0 / 1 (see Tuning::track_rule)
struct TrackParams { double K4[4]; double reproj_thr; int track_rule; };
// out: the caller's batch -- n_kf the pose stride, total_lm / total_edge the capacities of its arrays, every array written -- and its status word
int launch_build_windows(const vslam_tracks_in& in, const vslam_ba_batch& out, int32_t* d_status, const TrackParams& tp, const KfPolicy& kp, DevBuf& scratch, hipStream_t stream,
                         const SegView& seg);
int launch_chain_poses(int n_frames, const double* d_T_rel, double* d_G, hipStream_t stream, const SegView& seg);
// insert_key_frame's gate per frame (vslam_gate_states_dev): absolute 0 on T_rel (n_frames - 1 rows), 1 on absolute poses (n_frames rows)
int launch_gate_states(int n_frames, const double* d_T, int absolute, const int32_t* d_num_inliers, int32_t* d_state, hipStream_t stream, const SegView& seg);
// the reference's failure handling: every frame's last accepted predecessor / gap / Lost from the states (vslam_frame_pairs_dev), and the gate taken
// against that predecessor at that gap followed by the Lost scan (vslam_gate_states_pairs_dev)
int launch_frame_pairs(int n_frames, const int32_t* d_state, int32_t* d_pred, double* d_gap, hipStream_t stream, const SegView& seg);
int launch_gate_states_pairs(int n_frames, const double* d_G, const int32_t* d_pred, const int32_t* d_num_inliers, int32_t* d_state, DevBuf& scratch,
                             hipStream_t stream, const SegView& seg);
// the recover entries: the pairing in.d_f2f was built on (null: adjacent frames) and where the pairing of this call's states goes (the caller's
// arrays in vslam_build_map_pnp_inputs_recover_dev, scratch in the window builder)
struct MapRecover { const int32_t* d_pred_prev; int32_t* d_pred; double* d_gap; };
// the re-match of vslam_build_map_pnp_inputs_requery_dev: frame f's descriptors at d_desc + f * desc_stride; outputs the feature lists (n_frames x kp_capacity,
// n_frames) and the new frame-to-frame table ((n_frames - 1) x match_capacity); the matcher's gate parameters and scratch
struct MapRequery { const uint8_t* d_desc; size_t desc_stride; int32_t* d_feat; int32_t* d_nfeat; vslam_dmatch* d_f2f_out; int32_t* d_nf2f_out;
                    double ratio, gap_thr; uint32_t* d_train_best; };
// the inputs of every frame pair (xyz / uv: (n_frames - 1) x capacity, n), the input index of every match and the status word
struct MapInputsOut { float* xyz; float* uv; int32_t* n; int32_t* in_of_match; int capacity; int32_t* status; };
// one refinement pass's pose inputs against the map (vslam_build_map_pnp_inputs_dev): the builders' walk on the caller's poses d_G and the previous
// pass's links.  d_state non-null: the gated walk (*_gated_dev); rq non-null: the pairs are re-matched on their feature sets between the walk and
// the emit (*_requery_dev); rv non-null (with rq and d_state): the pairing of the states decides who is matched against whom (*_recover_dev)
int launch_map_pnp_inputs(const vslam_tracks_in& in, const double* d_G, const int32_t* d_in_of_match_prev, const int32_t* d_state, const TrackParams& tp, const MapInputsOut& out,
                          const MapRequery* rq, const MapRecover* rv, DevBuf& scratch, hipStream_t stream, const SegView& seg);

// chain_kernels.hip: the chained BA of vslam_ba_chain_dev.  Step j stages the j-th window of every sequence that has one into a batch of its own
// (offsets, then gather with the carried poses and flags substituted), the schedule runs on it, and scatter takes the results back to the caller's
// arrays and into the chain state.  Every index read from a caller's array is range-checked before it addresses memory.
struct ChainArgs {
    int n_windows, n_kf, min_kf; long long total_lm, total_edge;   // the caller's batch
    const int32_t* lm_off; const int32_t* edge_off; const int32_t* n_kf_w; // (n_kf_w null: every window holds n_kf keyframes)
    double* T; const float* xyz; const uint8_t* reliable; uint8_t* lm_inlier; const int32_t* kf_idx; const int32_t* lm_idx; const float* uv;
    double* chi2; vslam_lm_stats* stats;                             // (null: not wanted)
    const int32_t* lm_id; const int32_t* kf_frame; int32_t* ran;     // (kf_frame null: the sliding window; ran null: not wanted)
    const int32_t* first; int n_seg;                                 // the segment table (first null: one sequence, n_seg = 1)
    // chain state: pose per frame (x 7) with its "some window left one" byte, the is_inlier byte per root, the status word per caller window
    double* pose; uint8_t* pose_set; uint8_t* bit; long long n_roots; int32_t* status;
    // the staging batch of one step (at most n_seg windows; landmark / edge arrays sized by the caller's totals) and slot -> caller window
    int32_t* s_lm_off; int32_t* s_edge_off; int32_t* s_n_kf; int32_t* s_win;
    double* s_T; float* s_xyz; uint8_t* s_rel; uint8_t* s_inl; int32_t* s_kf; int32_t* s_lm; float* s_uv; double* s_chi2; vslam_lm_stats* s_stats;
};
int launch_chain_stage(const ChainArgs& a, int step, int n_slots, hipStream_t stream);
int launch_chain_scatter(const ChainArgs& a, int n_slots, const int32_t* step_status, hipStream_t stream);

// ----------------------------------------------------------------------------------------------- rectification
// rectify_kernels.hip: the map builder (host, double, once per rig), the device entry format and the gather kernel
constexpr int kRectifyGroup = 8;   // images of the batch one lane applies its decoded map entries to
void rectify_rotation_error(const double R[9], double* ortho_err, double* det);
void rectify_build_map(const vslam_rectify_cam& cam, int dst_w, int dst_h, int16_t* xy, uint16_t* frac);
int rectify_map_pitch(int dst_w);  // entries per row of a device map: dst_w rounded up to 4
void rectify_pack_map(const int16_t* xy, const uint16_t* frac, int dst_w, int dst_h, int src_w, int src_h, uint2* out);
int rectify_tiles_x(int dst_w);    // 256 x 4 destination tiles per tile row
void rectify_tile_boxes(const uint2* packed, int dst_w, int dst_h, int4* tiles); // per tile the source box to stage in LDS, or zeros: gather directly
// side s (0 left, 1 right) is skipped when any of its three pointers is null; w x h: the destination size the maps were built for
// form: 0 = direct gathers, 1 = the tiles' source boxes staged in LDS (tiles[s] required; falls back to 0 for sources that are not 16-byte aligned)
struct RectifyLaunch { const uint2* map[2]; const int4* tiles[2]; const uint8_t* src[2]; uint8_t* dst[2]; int w, h, B, src_pitch, dst_pitch, form;
                       size_t src_img_bytes, dst_img_bytes; };
int launch_rectify(const RectifyLaunch& L, hipStream_t stream);
struct RectifyState { uint2* d_map[2]; int4* d_tiles[2]; int src_w[2], src_h[2]; };  // the two maps of a context (null until set), counted in dev_bytes

// ----------------------------------------------------------------------------------------------- dense map
// voxel_kernels.hip: disparity maps reprojected at their keyframes' poses and summed into a sparse voxel grid (include/vslam_hip.h "dense map").
// A slot is 32 bytes: the key, then count / sum_ox / sum_oy / sum_oz / sum_intensity as uint32 and 4 unused bytes.
constexpr int kVoxelMaxMap = 1022;       // map ids 0 .. 1022: the key's top ten bits, all-ones left to the empty slot
constexpr int kVoxelCounters = 8;        // uint64 words behind a table: occupied, points, dropped for range, dropped full, status (the rest unused)
struct VoxelTable { uint8_t* slots; unsigned long long* counters; int log2_capacity; float vs, inv; };
// What a context hands out and takes back -- VoxelMap, TsdfMap, PlaceDb -- starts with this: the context, the object's one device allocation and its
// size, counted in the context's dev_bytes.  `noun`: what the messages of owned_by() call the object.
struct Owned {
    Ctx* ctx = nullptr; uint8_t* base = nullptr; size_t bytes = 0;
    int alloc(Ctx* c, size_t n, const char* who);   // on `who`'s behalf; a failure leaves nothing allocated and nothing counted
    void free();                                    // after everything queued on the context's stream; the object's DevBufs are its own to release
};
struct VoxelMap : Owned { static constexpr const char* noun = "map"; VoxelTable t; };
// B disparity maps (B x h x w f32, tightly packed), their poses (B x 7) and the pixels wanted: every step-th column and row, depth gate (z_min, z_max)
struct VoxelImages { const float* disp; int w, h, B, step; const double* T; double z_min, z_max, fx, fy, cx, cy, b; };
int launch_voxel_clear(const VoxelTable& t, hipStream_t stream);
int launch_reproject(const VoxelImages& a, float* d_xyz, uint8_t* d_valid, hipStream_t stream);
int launch_voxel_insert_points(const VoxelTable& t, const float* d_xyz, const uint8_t* d_valid, const uint8_t* d_intensity, size_t n, int map_id, hipStream_t stream);
// form: 0 = direct insertion, 1 = tile sums in LDS first
int launch_voxel_fuse(const VoxelTable& t, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const int32_t* d_map_id, int form,
                      hipStream_t stream);
int launch_voxel_extract(const VoxelTable& t, int map_id, int min_count, vslam_voxel* d_out, int32_t* d_map_out, size_t capacity, unsigned long long* d_n_out,
                         hipStream_t stream);

// ----------------------------------------------------------------------------------------------- surface map
// tsdf_kernels.hip: disparity maps fused into a truncated signed distance field over 8 x 8 x 8 voxel blocks (include/vslam_hip.h "surface map").
// The hash slot IS the storage: slot s of `keys` owns block s of `pool` (512 voxels of W, Sq, Wc, I as one uint4 each; voxel (x, y, z) of a block
// at (z & 7) << 6 | (y & 7) << 3 | (x & 7)).  `list` holds the claimed slots in the order they were claimed, counters[0] of them.
constexpr int kTsdfCounters = 8;         // uint64 words: blocks, samples, dropped for range, dropped full, status, frames skipped, pairs visited, pairs kept
constexpr int kTsdfFrameDoubles = 16;    // a frame of the frame table: R (9), t (3), the inverse pose's translation (3), the map id (-1: takes no part)
struct TsdfTable { unsigned long long* keys; uint32_t* list; uint4* pool; unsigned long long* counters; double* frames; unsigned long long* pairs;
                   int log2_blocks, J, frame_words; float vs, inv; };
struct TsdfMap : Owned { static constexpr const char* noun = "map"; TsdfTable t;
                 DevBuf mesh; // the vertex-id table of vslam_tsdf_mesh_dev: vid (3 x 512 int32 per claimed block) | pos_of_slot (one uint32 per slot); grown by the first mesh call
                 DevBuf render; // the tables of vslam_tsdf_render_dev: the view table (16 doubles per view) | (form 1) one (k_lo, k_hi) per view and 16 x 16 tile; grown on demand
                 DevBuf reint; // the old sides of vslam_tsdf_reintegrate_dev: a second frame table | a second frame mask per slot | n0; grown by the first such call
                 DevBuf dist; // the clearance layer of vslam_tsdf_distance_dev (TsdfLayer below); grown by the first build or a larger request
                 // epoch: bumped by integrate, reintegrate, load_blocks and clear; the layer serves readers only while dist_epoch == epoch
                 unsigned long long epoch = 0, dist_epoch = 0; bool dist_built = false; int dist_log2 = 0;
                 TsdfMap(size_t* acct) : mesh("mesh vertex-id table", acct), render("render view and range tables", acct), reint("re-integration tables", acct),
                                         dist("distance layer", acct) {} };
int launch_tsdf_clear(const TsdfTable& t, hipStream_t stream);
int launch_tsdf_alloc(const TsdfTable& t, const VoxelImages& a, hipStream_t stream); // ALLOCATION of the frames of t.frames
// form: 0 = every block walks all frames, 1 = a cull kernel writes a frame mask per block first
int launch_tsdf_integrate(const TsdfTable& t, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const int32_t* d_map_id, int form,
                          hipStream_t stream);
int launch_tsdf_extract(const TsdfTable& t, int map_id, int min_weight, vslam_surfel* d_out, int32_t* d_map_out, size_t capacity, unsigned long long* d_n_out,
                        hipStream_t stream);
int launch_tsdf_blocks(const TsdfTable& t, int map_id, int32_t* d_block_out, uint32_t* d_voxels_out, size_t capacity, unsigned long long* d_n_out,
                       hipStream_t stream);
// tsdf_dist_kernels.hip: the clearance layer (include/vslam_hip.h "DISTANCE").  A key table of its own of 2^log2_blocks slots, slot s owning block s of
// `cells` (512 uint16 cell words in the pool's voxel order), of `tmp` (the separable form's second buffer), of `masks` (three 512-bit masks: site, free,
// occupied) and of `kind` (bit 0: claimed in the pool for a map the build covered, bit 1: holds a voxel within R of a site; 0: not emitted).  `list`
// holds the claimed slots, `site_list` those whose block holds a site.
constexpr int kDistCounters = 8;         // uint64 words; the indices follow
constexpr int kDistNList = 0, kDistSites = 1, kDistNSiteBlocks = 2, kDistVoid = 3, kDistNLayer = 4, kDistNKindB = 5;
constexpr int kDistMaskWords = 24;
constexpr size_t kDistBlockBytes = 8 + 8 * kDistMaskWords + 1024 + 1024 + 4 + 4 + 1;   // per slot: key, masks, cells, tmp, list, site_list, kind
struct TsdfLayer { unsigned long long* counters; unsigned long long* keys; unsigned long long* masks; uint16_t* cells; uint16_t* tmp; uint32_t* list;
                   uint32_t* site_list; uint8_t* kind; int log2_blocks; };
size_t tsdf_dist_layer_bytes(int log2_layer_blocks);
TsdfLayer tsdf_dist_layer(uint8_t* base, int log2_layer_blocks);
// R = radius_voxels in [1, 16]; form: 0 = every voxel walks the site masks around it, 1 = the separable transform, three passes (same bytes);
// d_counts null or 3 words: sites, layer blocks, layer blocks the pool does not hold
int launch_tsdf_distance(const TsdfTable& t, const TsdfLayer& L, int map_id, int min_weight, int R, int form, unsigned long long* d_counts, hipStream_t stream);
int launch_tsdf_distance_blocks(const TsdfLayer& L, int map_id, int32_t* d_block_out, uint16_t* d_cells_out, size_t capacity, unsigned long long* d_n_out,
                                hipStream_t stream);
int launch_tsdf_distance_query(const TsdfTable& t, const TsdfLayer& L, const double* d_xyz_w, const int32_t* d_map_id, size_t N, float* d_dist, uint8_t* d_class,
                               hipStream_t stream);
// tsdf_reint_kernels.hip: frames taken out at their old poses and put in at their new ones (include/vslam_hip.h "RE-INTEGRATION").  The new sides use
// the map's own frame table and masks (t.frames, t.pairs); the old sides the tables of TsdfMap::reint, laid out alike.  n0 = the blocks claimed before the call.
struct TsdfReint { double* frames_old; unsigned long long* pairs_old; uint32_t* n0; const uint32_t* reach; };
size_t tsdf_reint_table_bytes(const TsdfTable& t, int max_batch);
TsdfReint tsdf_reint_tables(const TsdfTable& t, int max_batch, uint8_t* base, const uint32_t* d_reach);
// a.T: the new poses; form as launch_tsdf_integrate
int launch_tsdf_reintegrate(const TsdfTable& t, const TsdfReint& r, const VoxelImages& a, const uint8_t* d_gray, size_t img_bytes, int pitch, const double* d_T_old,
                            const int32_t* d_map_id, int form, hipStream_t stream);
// tsdf_mesh_kernels.hip: the triangle mesh of the field (include/vslam_hip.h "MESH") and the block loader
int launch_tsdf_mesh(const TsdfTable& t, int32_t* d_vid, uint32_t* d_pos_of_slot, size_t vid_blocks, int map_id, int min_weight, vslam_surfel* d_vertices,
                     int32_t* d_vertex_map, size_t vertex_capacity, vslam_triangle* d_triangles, size_t triangle_capacity, unsigned long long* d_counts,
                     hipStream_t stream);
int launch_tsdf_load(const TsdfTable& t, const int32_t* d_block_ids, const uint32_t* d_voxels, size_t n, hipStream_t stream);
// tsdf_render_kernels.hip: depth, normal and intensity views ray-cast from the field (include/vslam_hip.h "RENDER")
struct TsdfRenderCall { int w, h, V, K, min_weight; double fx, fy, cx, cy, z_min, hs; const double* d_T; const int32_t* d_map_id;
                        float* d_depth; float* d_attr; unsigned long long* d_counts; };  // (d_attr, d_counts null: not wanted)
size_t tsdf_render_table_bytes(int V, int w, int h, int form);
// form: 0 = every ray walks all K samples, 1 = a range kernel narrows each 16 x 16 tile's samples to those near a claimed block first (same bytes)
int launch_tsdf_render(const TsdfTable& t, const TsdfRenderCall& rc, uint8_t* d_tables, int form, hipStream_t stream);

// ----------------------------------------------------------------------------------------------- place database
// place_kernels.hip: keyframe descriptor blocks kept across steps and the place score between them (include/vslam_hip.h "place database").
// Entry e owns stride_rows x 32 bytes of descriptors (stride_rows = rows rounded up to 32: every block 16-byte aligned, the tail zeroed), n / seq / frame
// and, with geometry (xy non-null), `rows` slots of pixel, camera-frame point, valid flag and the ascending list qsel[0 .. nqsel) of the valid rows.
struct PlaceView { uint8_t* desc; int32_t* n; int32_t* seq; int32_t* frame; float2* xy; float* xyz; uint8_t* valid; int32_t* qsel; int32_t* nqsel;
                   int rows, stride_rows, capacity, n_entries; };
struct PlaceDb : Owned { static constexpr const char* noun = "database"; PlaceView v; unsigned long long n_refused; DevBuf dst, work;
                 PlaceDb(size_t* acct) : dst("place add table", acct), work("place verify scratch", acct) {} };
int launch_place_add(const PlaceView& v, const int32_t* d_dst, const uint8_t* d_desc, size_t desc_stride, const int32_t* d_n, const int32_t* d_seq,
                     const int32_t* d_frame, const vslam_keypoint* d_kps, const float* d_xyz, const uint8_t* d_valid, int kp_capacity, int B, hipStream_t stream);
// d_score (nq x ld int32): -1 / the count of section "place database" for queries [q0, q0 + nq) against every entry
int launch_place_score(const PlaceView& v, int q0, int nq, int tau, int min_gap, int32_t* d_score, int ld, hipStream_t stream);
int launch_place_select(const PlaceView& v, int nq, const int32_t* d_score, int ld, int K, int min_score, int32_t* d_cand, int32_t* d_cand_score,
                        hipStream_t stream);
int launch_place_verify_prep(const PlaceView& v, int nq, const int32_t* d_cand, int K, int rank, int32_t* d_qitem, double* d_gap, hipStream_t stream);
int launch_place_gather(const PlaceView& v, int q0, int nq, const int32_t* d_qitem, const vslam_dmatch* d_m, const int32_t* d_nm, int min_inliers, float* d_xyz,
                        float* d_uv, int32_t* d_n, int32_t* d_n_matches, hipStream_t stream);

// ----------------------------------------------------------------------------------------------- pose graph
// posegraph_kernels.hip: one persistent workgroup per graph through all LM iterations (include/vslam_hip.h "pose-graph optimisation").  The per-graph
// state is carved from `buf`; d_status (n_graphs words, the library's own copy for vslam_pose_graph_status_dev) is its first slot.  precond: -1 / 0 / 1.
int launch_pose_graph(const vslam_pose_graph& g, const vslam_pose_graph_params& p, int precond, double* d_T_out, vslam_pose_graph_stats* d_stats, DevBuf& buf,
                      hipStream_t stream);

// ----------------------------------------------------------------------------------------------- full bundle adjustment
// fullba_kernels.hip: one persistent workgroup per problem through all LM iterations (include/vslam_hip.h "full bundle adjustment").  The state is
// carved from `buf`; the status words (n_problems, the library's own copy for vslam_full_ba_status_dev) are its first slot.  store: 1 = the observations'
// (P, B) are kept from the linearisation, 0 = recomputed in every conjugate-gradient phase.
int launch_full_ba(const vslam_full_ba& b, const vslam_full_ba_params& p, int store, double* d_T_out, double* d_xyz_out, vslam_full_ba_stats* d_stats,
                   DevBuf& buf, hipStream_t stream);

// ----------------------------------------------------------------------------------------------- match by projection
// projmatch_kernels.hip: one workgroup per item (include/vslam_hip.h "match by projection").  K4 = the call's camera, img_w x img_h the context's image.
// stage: 1 = the image's descriptors are staged in LDS where that leaves two workgroups per CU, 0 = the candidates read them from L2.
size_t project_match_lds_bytes(int cap, int gw, int gh, bool stage);
int launch_project_match(const vslam_project_match& in, const vslam_project_match_params& p, const double K4[4], int img_w, int img_h, int stage,
                         hipStream_t stream);

// ----------------------------------------------------------------------------------------------- context
struct Ctx {
    vslam_params p;
    int device;
    hipStream_t stream;
    bool own_stream;
    size_t dev_bytes;
    OrbPlan plan;
    OrbTables tab;
    OrbBuffers orb;
    MatchBuffers match;
    DevBuf stage{"staging", &dev_bytes, (size_t)1 << 20}; // staging for the host-buffer API (sized for one item)
    uint8_t* h_pinned; size_t pinned_bytes;
    DevBuf sgbm{"SGBM scratch", &dev_bytes}; // cost volumes of vslam_disparity_map*
    bool sgbm_unchecked;  // an asynchronous SGBM launch whose error word nobody has read yet (vslam_sync / vslam_sgbm_status_dev do)
    DevBuf ransac{"RANSAC scratch", &dev_bytes}; // hypothesis tables of vslam_pnp_ransac_dev
    DevBuf track{"track scratch", &dev_bytes};   // chain tables of vslam_build_windows_dev
    Tuning tune;
    LmScratch lm{&dev_bytes, &tune};
    Prof* prof;           // stage profiler of this context (vslam_profile_enable); null until first enabled
    bool prof_orb;        // VSLAM_ORB_PROFILE was set when the context was created: every ORB call dumps the phase clocks of its kernels
    RectifyState rect;    // vslam_rectify_set / vslam_rectify_set_maps
    DevBuf segbuf{"segment table", &dev_bytes}; // vslam_set_segments: first, start, qitem
    SegView seg;          // ... as the launchers take it (all null: no table)
    int seg_frames;       // first[n_seg] of the table in place (0: none)
    std::vector<int32_t> seg_first_h; // ... and its `first` on the host (vslam_ba_chain_dev walks the sequences step by step)
    int32_t* ids; int ids_cap;  // vslam_set_window_ids: the caller's landmark-id buffer the window builders also fill (null: none)
    int ids_kp_cap;       // kp_capacity of the most recent builder call that wrote ids (the stride of the ids' frame index)
    DevBuf chain{"chain scratch", &dev_bytes};   // state and staging batch of vslam_ba_chain_dev
    DevBuf pgraph{"pose-graph state", &dev_bytes}; // status words and per-graph state of vslam_pose_graph_dev
    int pgraph_n;         // graphs of the most recent vslam_pose_graph_dev call (0: none yet)
    bool orb_ok;          // img_w, img_h >= 64: the ORB entry points serve this context (a smaller one is a rectification target only)
    DevBuf fullba{"full-BA state", &dev_bytes};    // status words and per-problem state of vslam_full_ba_dev
    int fullba_n;         // problems of the most recent vslam_full_ba_dev call (0: none yet)
};

} // namespace vslam
