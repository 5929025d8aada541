// api.hip -- the C-ABI of libvslam_hip.so (declared in include/vslam_hip.h).
// Host-buffer entry points (`vslam_*`) stage through a growable device arena and call the same launches as the
// device-resident batched entry points (`vslam_*_dev`).  No CPU fallback anywhere: without a HIP device every
// compute call fails with VSLAM_ERR_HIP / VSLAM_ERR_NO_DEVICE.
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "se3_device.h"
#include "vslam_internal.h"

#include <mutex>

namespace vslam {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- stage profiler (hipEvent brackets; see vslam_internal.h)
struct Prof {
    struct Rec { const char* name; int launches; hipEvent_t e0, e1; };
    bool on = false;
    std::vector<Rec> recs, open;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
static thread_local Prof* g_prof = nullptr;
// time origin shared by the brackets of every context ON ONE DEVICE (vslam_profile_intervals; events of different devices have no common clock):
// one event per device, created under a mutex by the first context of that device that profiles
static hipEvent_t g_prof_origin[16] = {nullptr};
static std::mutex g_prof_origin_mu;
Prof* prof_current() { return g_prof; }
void prof_set_current(Prof* p) { g_prof = p; }
void prof_begin(hipStream_t s, const char* name, int launches) {
    Prof* p = g_prof;
    if (!p || !p->on) return;
    Prof::Rec r{name, launches, p->get(), p->get()};
    (void)hipEventRecord(r.e0, s);
    p->open.push_back(r);
}
void prof_end(hipStream_t s) {
    Prof* p = g_prof;
    if (!p || !p->on || p->open.empty()) return;
    Prof::Rec r = p->open.back();
    p->open.pop_back();
    (void)hipEventRecord(r.e1, s);
    p->recs.push_back(r);
}
// every entry point makes its context's device current and routes the stage profiler to that context's recorder
#define VS_ENTER(c)                                                                         \
    do {                                                                                    \
        VS_HIP(hipSetDevice((c)->device));                                                  \
        prof_set_current(((c)->prof && (c)->prof->on) ? (c)->prof : nullptr);               \
    } while (0)

int DevBuf::reserve(size_t need, hipStream_t stream) {
    if (bytes >= need) return VSLAM_OK;
    VS_HIP(hipStreamSynchronize(stream));
    release();
    const size_t want = std::max(need, min_bytes);
    if (hipMalloc((void**)&p, want) != hipSuccess) { p = nullptr; set_error("%s hipMalloc(%zu) failed", name, want); return VSLAM_ERR_HIP; }
    bytes = want; *acct += want;
    return VSLAM_OK;
}
void DevBuf::release() {
    if (p) { (void)hipFree(p); *acct -= bytes; }
    p = nullptr; bytes = 0;
}

int Owned::alloc(Ctx* c, size_t n, const char* who) {
    ctx = c;
    if (hipMalloc((void**)&base, n) != hipSuccess) { base = nullptr; set_error("%s: hipMalloc(%zu) failed", who, n); return VSLAM_ERR_HIP; }
    bytes = n; c->dev_bytes += n;
    return VSLAM_OK;
}
void Owned::free() {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipFree(base);
    ctx->dev_bytes -= bytes;
    base = nullptr; bytes = 0;
}
// the object behind a handle (a VoxelMap, TsdfMap or PlaceDb), or null and a message when it is not one of context c
template <typename T, typename H>
static T* owned_by(const Ctx* c, H* handle, const char* who) {
    T* m = reinterpret_cast<T*>(handle);
    if (!c || !m || m->ctx != c) { set_error("%s: null context or %s, or a %s of another context", who, T::noun, T::noun); return nullptr; }
    return m;
}

// Staging layout of one host-buffer call over the context's staging buffer: in() also queues the host -> device copy of its slot.
struct Arena : Layout {
    struct Upload { void* d; const void* h; size_t bytes; };
    std::vector<Upload> uploads;
    explicit Arena(uint8_t* b = nullptr) : Layout(b) {}
    template <typename T> T* in(const T* h, size_t n) { T* d = take<T>(n); if (base) uploads.push_back({d, h, n * sizeof(T)}); return d; }
};
// `layout(Arena&)` carves the staging buffer (carve()); the queued uploads go out on the context stream in take order
template <typename F>
static int arena_stage(Ctx* c, F&& layout) {
    Arena a;
    if (int rc = carve(c->stage, c->stream, a, layout)) return rc;
    for (const Arena::Upload& u : a.uploads) VS_HIP(hipMemcpyAsync(u.d, u.h, u.bytes, hipMemcpyHostToDevice, c->stream));
    return VSLAM_OK;
}

static CamParams cam_of(const Ctx* c) {
    CamParams cam;
    cam.fx = c->p.cam[0]; cam.fy = c->p.cam[1]; cam.cx = c->p.cam[2]; cam.cy = c->p.cam[3]; cam.b = c->p.cam[4];
    cam.dmin = c->p.depth_min; cam.dmax = c->p.depth_max; cam.drel = c->p.depth_reliable; cam.row_tol = c->p.stereo_row_tol;
    return cam;
}
static void fill_K(const Ctx* c, double K[4]) { K[0] = c->p.cam[0]; K[1] = c->p.cam[1]; K[2] = c->p.cam[2]; K[3] = c->p.cam[3]; }
// launch_pnp's view of B single-pose problems under the context's intrinsics, Huber delta and inlier threshold; no outputs besides the poses and
// no n_hint until the caller sets them
static PnpArgs pnp_args_of(const Ctx* c, const float* d_xyz, const float* d_uv, const int32_t* d_n, int capacity, int B, double* d_T, int iters) {
    PnpArgs p;
    memset(&p, 0, sizeof(p));
    p.xyz = d_xyz; p.uv = d_uv; p.n = d_n; p.capacity = capacity; p.B = B; p.T = d_T; p.iters = iters;
    fill_K(c, p.K); p.huber_delta = c->p.huber_delta; p.reproj_thr = c->p.pnp_reproj_thr;
    return p;
}

template <typename T>
static int dev_alloc(Ctx* c, T** p, size_t n) {
    VS_HIP(hipMalloc((void**)p, n * sizeof(T)));
    c->dev_bytes += n * sizeof(T);
    return VSLAM_OK;
}

// ---- kernel-choice overrides (struct Tuning): table of {name, environment variable, field, allowed range}
struct TuneKey { const char* name; const char* env; int Tuning::*field; int lo, hi; };
static const TuneKey kTuneKeys[] = {
    {"orb_fuse_min", "VSLAM_ORB_FUSE_MIN", &Tuning::orb_fuse_min, 0, 1 << 30},
    {"orb_tiled", "VSLAM_ORB_TILED", &Tuning::orb_tiled, 0, 1},
    {"anms_cap", "VSLAM_ANMS_CAP", &Tuning::anms_cap, 0, 1 << 30},
    {"sgbm_fuse_min", "VSLAM_SGBM_FUSE_MIN", &Tuning::sgbm_fuse_min, 0, 1 << 30},
    {"sgbm_fwd_min", "VSLAM_SGBM_FWD_MIN", &Tuning::sgbm_fwd_min, 0, 1 << 30},
    {"sgbm_fw_rows", "VSLAM_SGBM_FW_ROWS", &Tuning::sgbm_fw_rows, 32, 64},
    {"pose_only_window", "VSLAM_POSE_ONLY_WINDOW", &Tuning::pose_only_window, 0, 1},
    {"pose_only_waves", "VSLAM_POSE_ONLY_WAVES", &Tuning::pose_only_waves, 0, VSLAM_MAX_KF},
    {"ba_resident", "VSLAM_BA_RESIDENT", &Tuning::ba_resident, 0, 1},
    {"pnp_window", "VSLAM_PNP_WINDOW", &Tuning::pnp_window, 0, 1},
    {"ba_adaptive", "VSLAM_BA_ADAPTIVE", &Tuning::ba_adaptive, 0, 1},
    {"ba_lanes", "VSLAM_BA_LANES", &Tuning::ba_lanes, 256, 512},
    {"track_rule", "VSLAM_TRACK_RULE", &Tuning::track_rule, 0, 1},
    {"rectify_form", "VSLAM_RECTIFY_FORM", &Tuning::rectify_form, 0, 1},
    {"voxel_form", "VSLAM_VOXEL_FORM", &Tuning::voxel_form, 0, 1},
    {"tsdf_form", "VSLAM_TSDF_FORM", &Tuning::tsdf_form, 0, 1},
    {"tsdf_dist_form", "VSLAM_TSDF_DIST_FORM", &Tuning::tsdf_dist_form, 0, 1},
    {"tsdf_render_form", "VSLAM_TSDF_RENDER_FORM", &Tuning::tsdf_render_form, 0, 1},
    {"pg_precond", "VSLAM_PG_PRECOND", &Tuning::pg_precond, 0, 1},
    {"fba_store", "VSLAM_FBA_STORE", &Tuning::fba_store, 0, 1},
    {"pm_stage", "VSLAM_PM_STAGE", &Tuning::pm_stage, 0, 1},
};
static int tune_set(Tuning& t, const TuneKey& k, long v) {
    if (v == -1) { t.*(k.field) = -1; return VSLAM_OK; } // back to the library's rule
    if (v < k.lo || v > k.hi || (k.field == &Tuning::sgbm_fw_rows && v != 32 && v != 64) || (k.field == &Tuning::ba_lanes && v != 256 && v != 512) ||
        (k.field == &Tuning::pose_only_waves && v != 0 && v != VSLAM_MAX_KF && v != kPoseOnlyNarrowWaves)) {
        set_error("tuning value %s = %ld out of range (%d..%d%s, or -1 = default)", k.name, v, k.lo, k.hi, k.field == &Tuning::sgbm_fw_rows ? ", 32 or 64" : "");
        return VSLAM_ERR_ARG;
    }
    t.*(k.field) = (int)v;
    return VSLAM_OK;
}
// the environment seeds the overrides ONCE, at context creation; an unparsable value is an error there, not a silent 0
static int tune_from_env(Tuning& t) {
    for (const TuneKey& k : kTuneKeys) {
        const char* e = getenv(k.env);
        if (!e || !*e) continue;
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        if (end == e || *end != 0) { set_error("environment variable %s = \"%s\" is not an integer", k.env, e); return VSLAM_ERR_ARG; }
        int rc = tune_set(t, k, v);
        if (rc) return rc;
    }
    return VSLAM_OK;
}

static int orb_status_check(Ctx* c, int B) {
    std::vector<int32_t> st(B);
    VS_HIP(hipMemcpyAsync(st.data(), c->orb.d_status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < B; ++b)
        if (st[b]) { set_error("ORB capacity exceeded on image %d (status bits 0x%x)", b, st[b]); return VSLAM_ERR_CAPACITY; }
    return VSLAM_OK;
}

// Images per call from which orb_pyrblur_kernel replaces the separate resize + blur (+ FAST) kernels; Tuning::orb_fuse_min overrides it
constexpr int kOrbFuseMinDefault = 96;
static int orb_fuse_min(const Ctx* c) { return c->tune.orb_fuse_min >= 0 ? c->tune.orb_fuse_min : kOrbFuseMinDefault; }
// The fused kernel writes the blurred pyramid line-tiled for orb_describe_kernel<true> unless Tuning::orb_tiled = 0; the separate blur kernel is row-major always
static bool orb_tiled(const Ctx* c, bool fused) { return fused && c->tune.orb_tiled != 0; }

// detect + (ANMS) + (describe) on device-resident images
static int orb_pipeline(Ctx* c, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, int anms_num, int regroup, bool describe,
                        vslam_keypoint* d_kps, uint8_t* d_desc, int32_t* d_count) {
    if (B <= 0) return VSLAM_OK;
    if (B > c->p.max_batch) { set_error("batch %d exceeds context max_batch %d", B, c->p.max_batch); return VSLAM_ERR_ARG; }
    int rc;
    // With descriptors wanted and a LARGE batch, every level is staged once for both its successor and its blurred copy
    // (orb_pyrblur_kernel: 3 % faster at 512 images, a third less pyramid traffic).  Small batches keep the separate kernels: eight
    // dependent launches that each do resize AND blur are slower than seven short resize launches + one blur launch over all levels
    // (0.36 vs 0.43 ms for two images).  [r6] With FAST inside the tile pass and the blur on the matrix cores the fused kernel wins from ~64 images on
    // (128 images: 0.89 vs 0.96 ms, 256: 1.35 vs 1.55; round 5's break-even was ~300).  Tuning::orb_fuse_min overrides the threshold (tests run both paths).
    const bool fused = describe && B >= orb_fuse_min(c);
    if (describe) c->orb.blur_tiled = orb_tiled(c, fused);
    if (fused) { // [r6] ... and FAST + NMS of every level from the same staged tile
        if ((rc = launch_orb_pyrblur(c->plan, c->tab, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->orb.d_blur, c->orb.blur_tiled, c->orb.d_rawt, c->p.fast_threshold, c->orb.d_corners,
                                     c->orb.d_corner_cnt, c->orb.d_status, c->stream))) return rc;
    } else {
        if ((rc = launch_orb_pyramid(c->plan, c->tab, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->stream))) return rc;
        if ((rc = launch_orb_fast(c->plan, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->p.fast_threshold, c->orb.d_corners,
                                  c->orb.d_corner_cnt, c->orb.d_status, c->stream))) return rc;
    }
    if ((rc = launch_orb_select(c->plan, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->orb.d_corners, c->orb.d_corner_cnt, c->orb.d_sel,
                                c->orb.d_sel_cnt, c->orb.d_status, c->stream))) return rc;
    if ((rc = launch_orb_anms(c->plan, B, c->orb.d_sel, c->orb.d_sel_cnt, c->plan.sel_cap, anms_num, regroup, d_kps, nullptr, c->orb.d_order, c->p.kp_capacity,
                              d_count, c->orb.d_status, c->orb.d_rad, c->tune.anms_cap, c->orb.d_anms_path, c->stream))) return rc;
    // orientation (and the rBRIEF rotation) only for the keypoints the ANMS kept
    if ((rc = launch_orb_orient(c->plan, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, d_kps, c->orb.d_cs, c->orb.d_order, c->p.kp_capacity, d_count,
                                fused && c->orb.blur_tiled ? c->orb.d_rawt : nullptr, c->stream))) return rc; // (the tiled raw copy exists when this call's fused kernel wrote it)
    if (describe) {
        if (!fused && (rc = launch_orb_blur(c->plan, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->orb.d_blur, c->stream))) return rc;
        if ((rc = launch_orb_describe(c->plan, d_imgs, img_bytes, pitch, B, c->orb.d_pyr, c->orb.d_blur, d_kps, c->orb.d_cs, c->orb.d_order, c->p.kp_capacity, d_count,
                                      d_desc, c->orb.blur_tiled, c->stream))) return rc;
    }
    if (c->prof_orb) orb_debug_dump(c->stream);
    return VSLAM_OK;
}

static int check_img(Ctx* c, const void* img, int w, int h, int stride) {
    if (!c || !img) { set_error("null context or image"); return VSLAM_ERR_ARG; }
    if (!c->orb_ok) { set_error("the context's %dx%d image is below ORB's 64x64: it serves the rectification stage and the image-free entry points only", c->p.img_w, c->p.img_h); return VSLAM_ERR_ARG; }
    if (w != c->p.img_w || h != c->p.img_h || stride < w) { set_error("image %dx%d (stride %d) does not match the context's %dx%d", w, h, stride, c->p.img_w, c->p.img_h); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

// ---- the two LM / PCG solvers (pose graph, full BA): their parameter structs have the same fields, and both leave a status word per problem at the
// front of their state buffer
template <class Params>
static void solver_default_params(Params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(Params);
    p->max_iters = 50; p->pcg_max_iters = 4000; p->pcg_tol = 1e-10; p->step_tol = 1e-9; p->lambda_init = 1e-4;
}
// p = the caller's parameters, or the defaults without any, checked (`me` is the entry's name, `type` the struct's)
template <class Params>
static int solver_params(const char* me, const char* type, const Params* params, Params& p) {
    solver_default_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(Params)) { set_error("%s: %s struct_size %d, the library has %d", me, type, params->struct_size, (int)sizeof(Params)); return VSLAM_ERR_ARG; }
        p = *params;
    }
    if (p.max_iters < 0 || p.pcg_max_iters < 1 || !(p.pcg_tol >= 0) || !(p.step_tol >= 0) || !(p.lambda_init > 0) || !(p.lambda_init <= 1e12)) {
        set_error("%s: parameters out of range (max_iters >= 0, pcg_max_iters >= 1, pcg_tol >= 0, step_tol >= 0, 0 < lambda_init <= 1e12)", me);
        return VSLAM_ERR_ARG;
    }
    return VSLAM_OK;
}
// the first n status words of buf, where the most recent call of entry `solver` left `last_n` of them (`what`: graphs / problems)
static int solver_status(Ctx* c, const char* me, const char* what, const char* solver, const DevBuf Ctx::*buf, const int Ctx::*last_n, int n, int32_t* h_status) {
    if (!h_status) { set_error("%s: null h_status", me); return VSLAM_ERR_ARG; }
    if (n < 0) { set_error("%s: negative n_%s %d", me, what, n); return VSLAM_ERR_ARG; }
    if (!c) { set_error("%s: null context", me); return VSLAM_ERR_ARG; }
    if (n > c->*last_n) { set_error("%s: %d %s asked for, the most recent %s call had %d", me, n, what, solver, c->*last_n); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    if (n > 0) VS_HIP(hipMemcpyAsync(h_status, (c->*buf).p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

} // namespace vslam

using namespace vslam;

extern "C" {

void vslam_default_params(vslam_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->img_w = 1241; p->img_h = 376; p->max_batch = 1;
    p->orb_nfeatures = 3000; p->anms_num = 500; p->fast_threshold = 20; p->kp_capacity = 4096;
    p->cam[0] = 718.856; p->cam[1] = 718.856; p->cam[2] = 607.1928; p->cam[3] = 185.2157; p->cam[4] = 0.573;
    p->depth_min = 10; p->depth_max = 400; p->depth_reliable = 40;
    p->match_ratio = 2.0; p->match_gap_thr = 30.0; p->huber_delta = 5.991; p->pnp_reproj_thr = 4.0; p->stereo_row_tol = 2.0;
    p->struct_size = (int32_t)sizeof(vslam_params); p->abi_version = VSLAM_ABI_VERSION;
}

const char* vslam_last_error(void) { return g_err; }
const char* vslam_version(void) { return "vslam_hip 0.3 (gfx950, ABI 3)"; }
int vslam_abi_version(void) { return VSLAM_ABI_VERSION; }
const char* vslam_kernel_names(void) { // the ProfScope names of csrc/*.hip (tests/test_abi.py checks the list against the sources)
    return "orb_resize_kernel orb_pyrblur_kernel orb_fast_kernel orb_select_kernel orb_anms_kernel orb_orient_kernel orb_blur_kernel orb_describe_kernel "
           "match_train_nearest_kernel match_finalize_kernel sgbm_prefilter_kernel sgbm_down_kernel sgbm_forward_kernel sgbm_hsum_kernel sgbm_vsum_kernel sgbm_path_kernel "
           "sgbm_wta_kernel sgbm_lrcheck_kernel sgbm_median3_kernel sgbm_ccl_rows_kernel sgbm_ccl_union_kernel sgbm_ccl_count_kernel "
           "sgbm_ccl_apply_kernel sgbm_ccl_kernels triangulate_kernel find3d_disparity_kernel gather_uv_kernel build_pnp_inputs_kernel lm_window_kernel pose_only_wave_kernel "
           "lm_window_kernel<pnp> pnp_wave_kernel pnp_inlier_kernel pnp_epnp_kernels epnp_front_kernel epnp_jacobi_kernel epnp_back_kernel hbm_copy_probe_kernel "
           "pnp_ransac_subsets_kernel pnp_ransac_count_kernel pnp_ransac_select_kernel "
           "build_windows_kernels track_init_kernel track_pose_chain_kernel track_link_kernel track_chain_kernel window_count_kernel window_scan_kernel window_rank_kernel window_emit_kernel "
           "track_ends_kernel kf_band_kernel kf_set_kernel kf_sliding_kernel kf_gate_kernel map_pnp_inputs_kernels track_map_inputs_kernel "
           "match_train_nearest_sel_kernel track_features_kernel frame_pairs_kernel kf_gate_pairs_kernel rectify_kernel ba_chain_kernels "
           "voxel_clear_kernel reproject_kernel voxel_insert_points_kernel voxel_fuse_kernel voxel_extract_kernel "
           "tsdf_clear_kernel tsdf_frames_kernel tsdf_alloc_kernel tsdf_cull_kernel tsdf_integrate_kernel tsdf_extract_kernel tsdf_blocks_kernel tsdf_mesh_vertex_kernel tsdf_mesh_tri_kernel tsdf_load_kernel "
           "tsdf_reint_frames_kernel tsdf_reint_cull_kernel tsdf_reint_kernel "
           "tsdf_views_kernel tsdf_range_init_kernel tsdf_ray_range_kernel tsdf_render_kernel "
           "tsdf_dist_clear_kernel tsdf_dist_classify_kernel tsdf_dist_dilate_kernel tsdf_dist_brute_kernel tsdf_dist_row_kernel tsdf_dist_pass_kernel tsdf_dist_counts_kernel "
           "tsdf_dist_blocks_kernel tsdf_dist_query_kernel "
           "place_add_kernel place_score_init_kernel place_score_kernel place_select_kernel place_verify_prep_kernel place_gather_kernel "
           "pose_graph_kernel full_ba_kernel project_match_kernel";
}

int vslam_create(const vslam_params* p, int device, void* stream, vslam_ctx** out) {
    if (!p || !out) { set_error("null argument"); return VSLAM_ERR_ARG; }
    *out = nullptr;
    // (the ABI guard comes first: nothing else of *p may be read from a struct of another revision, and it needs no device)
    if (p->struct_size != (int32_t)sizeof(vslam_params) || p->abi_version != VSLAM_ABI_VERSION) {
        set_error("vslam_params from a different ABI (struct_size %d / abi_version %d, library has %d / %d): rebuild the caller against include/vslam_hip.h and "
                  "fill the struct with vslam_default_params", p->struct_size, p->abi_version, (int)sizeof(vslam_params), VSLAM_ABI_VERSION);
        return VSLAM_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device visible (libvslam_hip has no CPU path)"); return VSLAM_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (0..%d)", device, ndev - 1); return VSLAM_ERR_ARG; }
    if (p->max_batch <= 0 || p->kp_capacity < 64 || p->kp_capacity > kMaxRows || p->orb_nfeatures <= 0) { set_error("bad params (max_batch>0, 64<=kp_capacity<=%d)", kMaxRows); return VSLAM_ERR_ARG; }
    VS_HIP(hipSetDevice(device));
    Ctx* c = new Ctx(); // (value-initialised: zeroes, then the members' default initialisers -- Tuning's -1, LmScratch's)
    c->p = *p; c->device = device;
    { int rc_t = tune_from_env(c->tune); if (rc_t) { delete c; return rc_t; } }
    // the profile switches (tuning aids) are read here as well, once: nothing below vslam_create calls getenv
    c->prof_orb = getenv("VSLAM_ORB_PROFILE") != nullptr;
    c->lm.prof_lm = getenv("VSLAM_LM_PROFILE") != nullptr; c->lm.prof_rs = getenv("VSLAM_RS_PROFILE") != nullptr; c->lm.prof_po = getenv("VSLAM_PO_PROFILE") != nullptr;
    if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete c; return VSLAM_ERR_HIP; }
        c->own_stream = true;
    }
    if (c->prof_orb) orb_debug_enable();
    // An image below ORB's 64 x 64 (a small rectification target): the ORB plan and buffers are laid out for the 64 x 64 minimum so that every
    // pointer of the context exists, and the ORB entry points refuse the context (check_img, vslam_feature_detection_dev, vslam_orb_level).
    c->orb_ok = p->img_w >= 64 && p->img_h >= 64;
    if (p->img_w < 2 || p->img_h < 2) { set_error("image size %dx%d unsupported (2..4095; ORB needs 64..4095)", p->img_w, p->img_h); vslam_destroy(reinterpret_cast<vslam_ctx*>(c)); return VSLAM_ERR_ARG; }
    int rc = orb_plan_init(&c->plan, std::max(p->img_w, 64), std::max(p->img_h, 64), p->orb_nfeatures, p->kp_capacity);
    if (rc == VSLAM_OK) { rc = orb_tables_init(&c->plan, &c->tab); c->dev_bytes += c->tab.bytes; }
    const size_t B = (size_t)p->max_batch;
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_pyr, B * c->plan.pyr_bytes);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_corners, B * c->plan.corner_total);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_corner_cnt, B * kNLevels);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_sel, B * kNLevels * c->plan.sel_cap);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_sel_cnt, B * kNLevels);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_status, B);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_blur, B * c->plan.blur_bytes);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_rawt, B * c->plan.blur_bytes);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_cs, B * (size_t)p->kp_capacity);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_order, B * (size_t)p->kp_capacity);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_rad, B * (size_t)kMaxRows);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->orb.d_anms_path, B);
    if (rc == VSLAM_OK) rc = dev_alloc(c, &c->match.d_train_best, B * kMaxRows);
    if (rc != VSLAM_OK) { vslam_destroy(reinterpret_cast<vslam_ctx*>(c)); return rc; }
    *out = reinterpret_cast<vslam_ctx*>(c);
    return VSLAM_OK;
}

void vslam_destroy(vslam_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    orb_tables_free(&c->tab);
    for (DevBuf* b : {&c->stage, &c->sgbm, &c->ransac, &c->track, &c->lm.buf, &c->lm.cyc, &c->segbuf, &c->chain, &c->pgraph, &c->fullba}) b->release();
    if (c->h_pinned) hipHostFree(c->h_pinned);
    void* ptrs[] = {c->orb.d_pyr, c->orb.d_corners, c->orb.d_corner_cnt, c->orb.d_sel, c->orb.d_sel_cnt, c->orb.d_status, c->orb.d_det, c->orb.d_blur, c->orb.d_rawt, c->orb.d_cs, c->orb.d_order, c->orb.d_rad, c->orb.d_anms_path,
                    c->match.d_train_best, c->rect.d_map[0], c->rect.d_map[1], c->rect.d_tiles[0], c->rect.d_tiles[1]};
    for (void* q : ptrs) if (q) hipFree(q);
    if (c->prof) {
        if (prof_current() == c->prof) prof_set_current(nullptr);
        for (Prof::Rec& r : c->prof->recs) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
        for (hipEvent_t e : c->prof->pool) hipEventDestroy(e);
        delete c->prof;
    }
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}

int vslam_sync(vslam_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    if (c->sgbm_unchecked) { int32_t st = 0; return vslam_sgbm_status_dev(ctx, &st); } // (synchronises; a fired backstop voids the maps: VSLAM_ERR_HIP)
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

size_t vslam_device_bytes(const vslam_ctx* ctx) { return ctx ? reinterpret_cast<const Ctx*>(ctx)->dev_bytes : 0; }

// ---------------------------------------------------------------------------------------------- ORB, host buffers
// Host image -> device image with a 64-byte row pitch.  The rows are repacked on the host into a pinned staging buffer and
// sent as ONE linear copy: hipMemcpy2DAsync from pageable memory degenerates into a copy per row (measured 2.8 ms for a
// 1241x376 image against 0.03 ms for the same bytes as one block).  Several images of one call use consecutive slots.
static int img_pitch(int w) { return (w + 63) & ~63; }
static int upload_image(Ctx* c, uint8_t* d_img, const uint8_t* img, int w, int h, int stride, int slot = 0) {
    const int pitch = img_pitch(w);
    const size_t bytes = (size_t)pitch * h;
    const size_t need = bytes * (size_t)(slot + 1);
    if (c->pinned_bytes < need) {
        VS_HIP(hipStreamSynchronize(c->stream));
        if (c->h_pinned) (void)hipHostFree(c->h_pinned);
        c->h_pinned = nullptr; c->pinned_bytes = 0;
        const size_t want = std::max(need, 2 * bytes);
        VS_HIP(hipHostMalloc((void**)&c->h_pinned, want, hipHostMallocDefault));
        c->pinned_bytes = want;
    }
    uint8_t* stage = c->h_pinned + bytes * (size_t)slot;
    for (int y = 0; y < h; ++y) {
        memcpy(stage + (size_t)y * pitch, img + (size_t)y * stride, (size_t)w);
        memset(stage + (size_t)y * pitch + w, 0, (size_t)(pitch - w)); // deterministic padding
    }
    VS_HIP(hipMemcpyAsync(d_img, stage, bytes, hipMemcpyHostToDevice, c->stream));
    return VSLAM_OK;
}

static int orb_host_call(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride, int anms_num, int regroup, bool describe,
                         vslam_keypoint* kps, uint8_t* desc, int cap, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = check_img(c, img, w, h, stride);
    if (rc) return rc;
    if (!kps || !n_out || cap <= 0 || (describe && !desc)) { set_error("null output"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    const int kc = c->p.kp_capacity, dp = img_pitch(w);
    uint8_t *d_img, *d_desc; vslam_keypoint* d_kps; int32_t* d_cnt;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_img = a.take<uint8_t>((size_t)dp * h);
             d_kps = a.take<vslam_keypoint>(kc);
             d_desc = a.take<uint8_t>((size_t)kc * 32);
             d_cnt = a.take<int32_t>(1);
         }))) return rc;
    if ((rc = upload_image(c, d_img, img, w, h, stride))) return rc;
    if ((rc = orb_pipeline(c, d_img, (size_t)dp * h, dp, 1, anms_num, regroup, describe, d_kps, d_desc, d_cnt))) return rc;
    int32_t n = 0;
    VS_HIP(hipMemcpyAsync(&n, d_cnt, sizeof(n), hipMemcpyDeviceToHost, c->stream));
    if ((rc = orb_status_check(c, 1))) return rc;
    if (n > cap) { *n_out = 0; set_error("caller capacity %d < %d keypoints", cap, n); return VSLAM_ERR_CAPACITY; }
    VS_HIP(hipMemcpyAsync(kps, d_kps, sizeof(vslam_keypoint) * n, hipMemcpyDeviceToHost, c->stream));
    if (describe) VS_HIP(hipMemcpyAsync(desc, d_desc, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    *n_out = n;
    return VSLAM_OK;
}

int vslam_feature_detection(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride, vslam_keypoint* kps, uint8_t* desc, int cap, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("null context"); return VSLAM_ERR_ARG; }
    return orb_host_call(ctx, img, w, h, stride, c->p.anms_num, 1, true, kps, desc, cap, n_out);
}

int vslam_orb_detect(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride, vslam_keypoint* kps, int cap, int* n_out) {
    return orb_host_call(ctx, img, w, h, stride, 0, 0, false, kps, nullptr, cap, n_out);
}

int vslam_anms(vslam_ctx* ctx, vslam_keypoint* kps, int n, int num, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !kps || !n_out || n < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n > kMaxRows) { set_error("ANMS input %d > %d", n, kMaxRows); return VSLAM_ERR_CAPACITY; }
    if (n == 0) { *n_out = 0; return VSLAM_OK; }
    VS_ENTER(c);
    int rc;
    vslam_keypoint *d_in, *d_out; int32_t *d_n, *d_cnt;
    const int32_t nn = n;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_in = a.take<vslam_keypoint>(kMaxRows);
             d_out = a.take<vslam_keypoint>(kMaxRows);
             d_n = a.take<int32_t>(1);
             d_cnt = a.take<int32_t>(1);
         }))) return rc;
    VS_HIP(hipMemcpyAsync(d_in, kps, sizeof(vslam_keypoint) * n, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemcpyAsync(d_n, &nn, sizeof(nn), hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemsetAsync(c->orb.d_status, 0, sizeof(int32_t), c->stream));
    if ((rc = launch_anms_flat(1, d_in, d_n, kMaxRows, num, 0, c->p.img_w, c->p.img_h, d_out, nullptr, nullptr, kMaxRows, d_cnt, c->orb.d_status, c->orb.d_rad, c->tune.anms_cap, c->orb.d_anms_path, c->stream))) return rc;
    int32_t m = 0;
    VS_HIP(hipMemcpyAsync(&m, d_cnt, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    VS_HIP(hipMemcpy(kps, d_out, sizeof(vslam_keypoint) * m, hipMemcpyDeviceToHost));
    *n_out = m;
    return VSLAM_OK;
}

int vslam_orb_compute(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride, vslam_keypoint* kps, int n, uint8_t* desc, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    int rc = check_img(c, img, w, h, stride);
    if (rc) return rc;
    if (!kps || !desc || !n_out || n < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n > c->p.kp_capacity) { set_error("compute input %d > kp_capacity %d", n, c->p.kp_capacity); return VSLAM_ERR_CAPACITY; }
    if (n == 0) { *n_out = 0; return VSLAM_OK; }
    for (int i = 0; i < n; ++i)
        if (kps[i].octave < 0 || kps[i].octave >= kNLevels) { set_error("keypoint %d: octave %d out of range", i, kps[i].octave); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    const int kc = c->p.kp_capacity, dp = img_pitch(w);
    uint8_t *d_img, *d_desc; vslam_keypoint *d_in, *d_kps; int32_t *d_n, *d_cnt;
    const int32_t nn = n;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_img = a.take<uint8_t>((size_t)dp * h);
             d_in = a.take<vslam_keypoint>(kc);
             d_kps = a.take<vslam_keypoint>(kc);
             d_desc = a.take<uint8_t>((size_t)kc * 32);
             d_n = a.take<int32_t>(1);
             d_cnt = a.take<int32_t>(1);
         }))) return rc;
    if ((rc = upload_image(c, d_img, img, w, h, stride))) return rc;
    VS_HIP(hipMemcpyAsync(d_in, kps, sizeof(vslam_keypoint) * n, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemcpyAsync(d_n, &nn, sizeof(nn), hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemsetAsync(c->orb.d_status, 0, sizeof(int32_t), c->stream));
    const bool fused = 1 >= orb_fuse_min(c); // (one image: the separate kernels unless a test forces the fused one)
    c->orb.blur_tiled = orb_tiled(c, fused);
    if (fused) { if ((rc = launch_orb_pyrblur(c->plan, c->tab, d_img, (size_t)dp * h, dp, 1, c->orb.d_pyr, c->orb.d_blur, c->orb.blur_tiled, nullptr, 0, nullptr, nullptr, nullptr, c->stream))) return rc; }
    else {
        if ((rc = launch_orb_pyramid(c->plan, c->tab, d_img, (size_t)dp * h, dp, 1, c->orb.d_pyr, c->stream))) return rc;
        if ((rc = launch_orb_blur(c->plan, d_img, (size_t)dp * h, dp, 1, c->orb.d_pyr, c->orb.d_blur, c->stream))) return rc;
    }
    if ((rc = launch_anms_flat(1, d_in, d_n, kc, 0, 1, w, h, d_kps, c->orb.d_cs, nullptr, kc, d_cnt, c->orb.d_status, c->orb.d_rad, c->tune.anms_cap, c->orb.d_anms_path, c->stream))) return rc;
    if ((rc = launch_orb_describe(c->plan, d_img, (size_t)dp * h, dp, 1, c->orb.d_pyr, c->orb.d_blur, d_kps, c->orb.d_cs, nullptr, kc, d_cnt, d_desc, c->orb.blur_tiled, c->stream))) return rc;
    int32_t m = 0;
    VS_HIP(hipMemcpyAsync(&m, d_cnt, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    VS_HIP(hipMemcpy(kps, d_kps, sizeof(vslam_keypoint) * m, hipMemcpyDeviceToHost));
    VS_HIP(hipMemcpy(desc, d_desc, (size_t)m * 32, hipMemcpyDeviceToHost));
    *n_out = m;
    return VSLAM_OK;
}

int vslam_feature_detection_dev(vslam_ctx* ctx, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B, vslam_keypoint* d_kps,
                                uint8_t* d_desc, int32_t* d_count) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_imgs || !d_kps || !d_desc || !d_count || pitch < c->p.img_w || img_bytes < (size_t)pitch * c->p.img_h || !c->orb_ok) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return orb_pipeline(c, d_imgs, img_bytes, pitch, B, c->p.anms_num, 1, true, d_kps, d_desc, d_count);
}

int vslam_orb_status_dev(vslam_ctx* ctx, int B, int32_t* h_status) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_status || B <= 0 || B > c->p.max_batch) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    VS_HIP(hipMemcpyAsync(h_status, c->orb.d_status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

int vslam_orb_anms_path_dev(vslam_ctx* ctx, int B, int32_t* h_path) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_path || B <= 0 || B > c->p.max_batch) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    VS_HIP(hipMemcpyAsync(h_path, c->orb.d_anms_path, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

int vslam_orb_level(vslam_ctx* ctx, int item, int level, int blurred, uint8_t* out, int out_stride, int out_rows, int* w, int* h) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out || !w || !h || item < 0 || item >= c->p.max_batch || level < 0 || level >= kNLevels || (level == 0 && !blurred) || !c->orb_ok) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    const OrbLevel& L = c->plan.lv[level];
    if (out_stride < L.w || out_rows < L.h) { set_error("vslam_orb_level: level %d is %d x %d", level, L.w, L.h); return VSLAM_ERR_CAPACITY; }
    const uint8_t* src = blurred ? c->orb.d_blur + (size_t)item * c->plan.blur_bytes + c->plan.blur_off[level]
                                 : c->orb.d_pyr + (size_t)item * c->plan.pyr_bytes + L.pyr_off;
    VS_HIP(hipStreamSynchronize(c->stream));
    if (blurred && c->orb.blur_tiled) { // the last producer wrote the level line-tiled: fetch it as it lies and de-tile here (a diagnostic: no kernel for it)
        const int pitch = (L.w + 63) & ~63;
        std::vector<uint8_t> lv((size_t)pitch * tiled_rows(L.h));
        VS_HIP(hipMemcpy(lv.data(), src, lv.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < L.h; ++y)
            for (int x = 0; x < L.w; ++x) out[(size_t)y * out_stride + x] = lv[tiled_offset(x, y, pitch / kTileCols)];
        *w = L.w; *h = L.h;
        return VSLAM_OK;
    }
    VS_HIP(hipMemcpy2D(out, (size_t)out_stride, src, (size_t)((L.w + 63) & ~63), (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
    *w = L.w; *h = L.h;
    return VSLAM_OK;
}

// ---------------------------------------------------------------------------------------------- matcher
// vslam_feature_matching{,_subset,_pairs}_dev: the three entries' argument checks in their one order, then the launch.  subset: the entry takes
// d_qsel / d_nqsel / sel_capacity; pairs: it also takes d_qitem / n_qitems (an entry that lacks them passes null / 0, the launch's defaults)
static int feature_matching_dev(const char* entry, bool subset, bool pairs, vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq,
                                const int32_t* d_qsel, const int32_t* d_nqsel, int sel_capacity, const int32_t* d_qitem, int n_qitems, const uint8_t* d_t,
                                size_t t_stride_bytes, const int32_t* d_nt, const double* d_gap, int gate, int B, int max_rows, vslam_dmatch* d_out,
                                int out_capacity, int32_t* d_nout) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_q || !d_t || !d_nq || !d_nt || !d_gap || !d_out || !d_nout || out_capacity <= 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (subset && (!d_qsel || !d_nqsel)) { set_error("%s: d_qsel and d_nqsel are required", entry); return VSLAM_ERR_ARG; }
    if (pairs && (!d_qitem || n_qitems < 1)) { set_error("%s: d_qitem (B query-block indices) and n_qitems >= 1 are required", entry); return VSLAM_ERR_ARG; }
    if (subset && (sel_capacity < 1 || sel_capacity > kMaxRows)) { set_error("sel_capacity %d outside 1..%d (the matcher's row limit)", sel_capacity, kMaxRows); return VSLAM_ERR_ARG; }
    if (B > c->p.max_batch) { set_error("batch %d exceeds context max_batch %d", B, c->p.max_batch); return VSLAM_ERR_ARG; }
    if ((((uintptr_t)d_q | (uintptr_t)d_t | (uintptr_t)q_stride_bytes | (uintptr_t)t_stride_bytes) & 15) != 0) {
        set_error("%s: d_q, d_t and both strides must be multiples of 16 bytes (the matcher reads descriptors with 16-byte loads)", entry);
        return VSLAM_ERR_ARG;
    }
    VS_ENTER(c);
    return launch_match(d_q, q_stride_bytes, d_nq, d_t, t_stride_bytes, d_nt, d_gap, gate, c->p.match_ratio, c->p.match_gap_thr, B, max_rows,
                        c->match.d_train_best, d_out, out_capacity, d_nout, c->stream, d_qsel, sel_capacity, d_nqsel, d_qitem, n_qitems);
}

int vslam_feature_matching_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq, const uint8_t* d_t,
                               size_t t_stride_bytes, const int32_t* d_nt, const double* d_gap, int gate, int B, int max_rows,
                               vslam_dmatch* d_out, int out_capacity, int32_t* d_nout) {
    return feature_matching_dev("vslam_feature_matching_dev", false, false, ctx, d_q, q_stride_bytes, d_nq, nullptr, nullptr, 0, nullptr, 0, d_t, t_stride_bytes, d_nt,
                                d_gap, gate, B, max_rows, d_out, out_capacity, d_nout);
}

int vslam_feature_matching_subset_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq, const int32_t* d_qsel,
                                      const int32_t* d_nqsel, int sel_capacity, const uint8_t* d_t, size_t t_stride_bytes, const int32_t* d_nt,
                                      const double* d_gap, int gate, int B, int max_rows, vslam_dmatch* d_out, int out_capacity, int32_t* d_nout) {
    return feature_matching_dev("vslam_feature_matching_subset_dev", true, false, ctx, d_q, q_stride_bytes, d_nq, d_qsel, d_nqsel, sel_capacity, nullptr, 0, d_t,
                                t_stride_bytes, d_nt, d_gap, gate, B, max_rows, d_out, out_capacity, d_nout);
}

int vslam_feature_matching_pairs_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq, const int32_t* d_qsel,
                                     const int32_t* d_nqsel, int sel_capacity, const int32_t* d_qitem, int n_qitems, const uint8_t* d_t, size_t t_stride_bytes,
                                     const int32_t* d_nt, const double* d_gap, int gate, int B, int max_rows, vslam_dmatch* d_out, int out_capacity,
                                     int32_t* d_nout) {
    return feature_matching_dev("vslam_feature_matching_pairs_dev", true, true, ctx, d_q, q_stride_bytes, d_nq, d_qsel, d_nqsel, sel_capacity, d_qitem, n_qitems, d_t,
                                t_stride_bytes, d_nt, d_gap, gate, B, max_rows, d_out, out_capacity, d_nout);
}

int vslam_feature_matching(vslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double frame_gap, int gate,
                           vslam_dmatch* out, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !n_out || nq < 0 || nt < 0 || (nq > 0 && (!q || !out)) || (nt > 0 && !t)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (nq > kMaxRows || nt > kMaxRows) { set_error("matcher supports at most %d rows per side", kMaxRows); return VSLAM_ERR_CAPACITY; }
    *n_out = 0;
    if (nq == 0 || nt == 0) return VSLAM_OK; // empty set: no matches (reference: UB, quirk Q7)
    VS_ENTER(c);
    int rc;
    const int rows = std::max(nq, nt);
    const int32_t hn[3] = {nq, nt, 0};
    uint8_t *d_q, *d_t; vslam_dmatch* d_out; int32_t* d_n; double* d_gap;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_q = a.in(q, (size_t)nq * 32);
             d_t = a.in(t, (size_t)nt * 32);
             d_out = a.take<vslam_dmatch>(nq);
             d_n = a.in(hn, 3);
             d_gap = a.in(&frame_gap, 1);
         }))) return rc;
    if ((rc = launch_match(d_q, 0, d_n, d_t, 0, d_n + 1, d_gap, gate, c->p.match_ratio, c->p.match_gap_thr, 1, rows, c->match.d_train_best,
                           d_out, nq, d_n + 2, c->stream))) return rc;
    int32_t m = 0;
    VS_HIP(hipMemcpyAsync(&m, d_n + 2, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    if (m > 0) VS_HIP(hipMemcpy(out, d_out, sizeof(vslam_dmatch) * m, hipMemcpyDeviceToHost));
    *n_out = m;
    return VSLAM_OK;
}

// ---------------------------------------------------------------------------------------------- geometry
// ---------------------------------------------------------------------------------------------- SGBM
void vslam_default_sgbm_params(vslam_sgbm_params* p) {
    if (!p) return;
    p->num_disparities = 96; p->block_size = 9; p->P1 = 8 * 9 * 9; p->P2 = 32 * 9 * 9; p->disp12_max_diff = 1; p->pre_filter_cap = 63; // visual_odometry.cpp:163-164
    p->uniqueness_ratio = 10; p->speckle_window_size = 100; p->speckle_range = 32; p->struct_size = (int32_t)sizeof(vslam_sgbm_params);
}

int vslam_sgbm_params_check(const vslam_sgbm_params* p, int w, int h) {
    if (!p) { set_error("vslam_sgbm_params: null pointer"); return VSLAM_ERR_ARG; }
    auto refuse = [](const char* field, long v, const char* rule) { set_error("vslam_sgbm_params.%s = %ld: %s", field, v, rule); return VSLAM_ERR_ARG; };
    if (p->struct_size != (int32_t)sizeof(vslam_sgbm_params)) return refuse("struct_size", p->struct_size, "not this library's sizeof(vslam_sgbm_params)");
    if (p->num_disparities < 16 || p->num_disparities > 256 || p->num_disparities % 16) return refuse("num_disparities", p->num_disparities, "need a multiple of 16 in [16, 256]");
    if (p->block_size < 1 || p->block_size % 2 == 0) return refuse("block_size", p->block_size, "need an odd size >= 1");
    if (p->P1 <= 0) return refuse("P1", p->P1, "need 0 < P1 < P2");
    if (p->P2 <= p->P1) return refuse("P2", p->P2, "need 0 < P1 < P2");
    if (p->disp12_max_diff < 0) return refuse("disp12_max_diff", p->disp12_max_diff, "need >= 0");
    if (p->pre_filter_cap < 1 || p->pre_filter_cap > 63) return refuse("pre_filter_cap", p->pre_filter_cap, "need a cap in [1, 63]");
    if (p->uniqueness_ratio < 0 || p->uniqueness_ratio > 100) return refuse("uniqueness_ratio", p->uniqueness_ratio, "need a ratio in [0, 100]");
    if (p->speckle_window_size < 0) return refuse("speckle_window_size", p->speckle_window_size, "need >= 0");
    if (p->speckle_range < 0) return refuse("speckle_range", p->speckle_range, "need >= 0");
    // the 16-bit range rule (include/vslam_hip.h): three path values plus the offset 3 * P2 in a u16
    const long ftzero = (p->pre_filter_cap > 15 ? p->pre_filter_cap : 15) | 1;
    const long bs = p->block_size < 255 ? p->block_size : 255; // (255^2 * 93 is far outside already: no overflow for any int32 field)
    const long cmax = bs * bs * (2 * ftzero + 63);
    if (3 * (cmax + (long)p->P2) > 65535) {
        set_error("vslam_sgbm_params: block_size %d, pre_filter_cap %d and P2 %d leave the 16-bit range: need 3 * (block_size^2 * (2 * ftzero + 63) + P2) <= 65535, have %ld",
                  p->block_size, p->pre_filter_cap, p->P2, 3 * (cmax + (long)p->P2));
        return VSLAM_ERR_ARG;
    }
    if (w > 4096) { set_error("vslam_sgbm_params: image width %d > 4096", w); return VSLAM_ERR_ARG; }
    if (w - p->num_disparities <= p->block_size / 2) {
        set_error("vslam_sgbm_params.num_disparities = %d with block_size %d needs an image wider than %d (have %d)", p->num_disparities, p->block_size,
                  p->num_disparities + p->block_size / 2, w);
        return VSLAM_ERR_ARG;
    }
    if (h <= p->block_size) { set_error("vslam_sgbm_params.block_size = %d needs more than %d image rows (have %d)", p->block_size, p->block_size, h); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

// NULL = the reference's set; anything else must pass the check before a launch
static int sgbm_set_of(const vslam_sgbm_params* sgbm, int w, int h, vslam_sgbm_params& sp) {
    if (sgbm) sp = *sgbm; else vslam_default_sgbm_params(&sp);
    return vslam_sgbm_params_check(&sp, w, h);
}

int vslam_disparity_map_ex_dev(vslam_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride_bytes, int pitch, int w, int h,
                               int B, const vslam_sgbm_params* sgbm, float* d_disparity, int16_t* d_disp_i16, int16_t* d_disp_raw_i16) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_left || !d_right || w <= 0 || h <= 0 || pitch < w || B < 0 || img_stride_bytes < (size_t)pitch * h ||
        (!d_disparity && !d_disp_i16 && !d_disp_raw_i16)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    vslam_sgbm_params sp;
    if (int rc = sgbm_set_of(sgbm, w, h, sp)) return rc;
    VS_ENTER(c);
    c->sgbm_unchecked = true; // (asynchronous: the forward sweep's error word is looked at by the next vslam_sync / vslam_sgbm_status_dev)
    return launch_sgbm(c->tune, sp, d_left, d_right, img_stride_bytes, pitch, w, h, B, d_disparity, d_disp_i16, d_disp_raw_i16, c->sgbm, c->stream);
}

int vslam_disparity_map_dev(vslam_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride_bytes, int pitch, int w, int h,
                            int B, float* d_disparity, int16_t* d_disp_i16, int16_t* d_disp_raw_i16) {
    return vslam_disparity_map_ex_dev(ctx, d_left, d_right, img_stride_bytes, pitch, w, h, B, nullptr, d_disparity, d_disp_i16, d_disp_raw_i16);
}

int vslam_disparity_map_ex(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride, const vslam_sgbm_params* sgbm,
                           float* disparity, int16_t* disp_i16, int16_t* disp_raw_i16) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !left || !right || w <= 0 || h <= 0 || stride < w || (!disparity && !disp_i16 && !disp_raw_i16)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    vslam_sgbm_params sp;
    if (int rc0 = sgbm_set_of(sgbm, w, h, sp)) return rc0;
    VS_ENTER(c);
    int rc;
    const size_t npix = (size_t)w * h;
    const int pl = img_pitch(w);
    uint8_t *d_l, *d_r; float* d_f; int16_t *d_i, *d_raw;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_l = a.take<uint8_t>((size_t)pl * h);
             d_r = a.take<uint8_t>((size_t)pl * h);
             d_f = a.take<float>(npix);
             d_i = a.take<int16_t>(npix);
             d_raw = a.take<int16_t>(npix);
         }))) return rc;
    if ((rc = upload_image(c, d_l, left, w, h, stride))) return rc;
    if ((rc = upload_image(c, d_r, right, w, h, stride, 1))) return rc;
    if ((rc = launch_sgbm(c->tune, sp, d_l, d_r, (size_t)pl * h, pl, w, h, 1, d_f, d_i, disp_raw_i16 ? d_raw : nullptr, c->sgbm, c->stream))) return rc;
    if (disparity) VS_HIP(hipMemcpyAsync(disparity, d_f, npix * 4, hipMemcpyDeviceToHost, c->stream));
    if (disp_i16) VS_HIP(hipMemcpyAsync(disp_i16, d_i, npix * 2, hipMemcpyDeviceToHost, c->stream));
    if (disp_raw_i16) VS_HIP(hipMemcpyAsync(disp_raw_i16, d_raw, npix * 2, hipMemcpyDeviceToHost, c->stream));
    int32_t st = 0;
    return vslam_sgbm_status_dev(ctx, &st); // synchronises; VSLAM_ERR_HIP if the forward sweep's backstop fired
}

int vslam_disparity_map(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride, float* disparity, int16_t* disp_i16,
                        int16_t* disp_raw_i16) {
    return vslam_disparity_map_ex(ctx, left, right, w, h, stride, nullptr, disparity, disp_i16, disp_raw_i16);
}

int vslam_set_tuning(vslam_ctx* ctx, const char* name, int value) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !name) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    for (const TuneKey& k : kTuneKeys)
        if (!strcmp(k.name, name)) return tune_set(c->tune, k, value);
    set_error("unknown tuning key \"%s\"", name);
    return VSLAM_ERR_ARG;
}

int vslam_sgbm_status_dev(vslam_ctx* ctx, int32_t* h_status) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_status) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    *h_status = 0;
    c->sgbm_unchecked = false;
    if (!c->sgbm.p) { VS_HIP(hipStreamSynchronize(c->stream)); return VSLAM_OK; } // no SGBM launch yet
    VS_HIP(hipMemcpyAsync(h_status, reinterpret_cast<const int32_t*>(c->sgbm.p) + kSgbmErrorWord, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    if (*h_status != 0) { set_error("sgbm_forward_kernel: a slab waited for its predecessor beyond the spin limit; the disparity maps of this call are void"); return VSLAM_ERR_HIP; }
    return VSLAM_OK;
}

// ---------------------------------------------------------------------------------------------- rectification
void vslam_default_rectify_params(vslam_rectify_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->src_w = 1241; p->src_h = 376;
    for (vslam_rectify_cam& c : p->cam) {
        c.K[0] = c.P[0] = 718.856; c.K[1] = c.P[1] = 718.856; c.K[2] = c.P[2] = 607.1928; c.K[3] = c.P[3] = 185.2157; // vslam_default_params' cam
        c.R[0] = c.R[4] = c.R[8] = 1.0;
    }
    p->struct_size = (int32_t)sizeof(vslam_rectify_params);
}

int vslam_rectify_params_check(const vslam_rectify_params* p, int dst_w, int dst_h) {
    if (!p) { set_error("vslam_rectify_params: null pointer"); return VSLAM_ERR_ARG; }
    if (p->struct_size != (int32_t)sizeof(vslam_rectify_params)) {
        set_error("vslam_rectify_params.struct_size = %d: not this library's sizeof(vslam_rectify_params) = %d", p->struct_size, (int)sizeof(vslam_rectify_params));
        return VSLAM_ERR_ARG;
    }
    auto size_ok = [](const char* field, int v) {
        if (v >= 2 && v <= 4096) return true;
        set_error("vslam_rectify_params: %s = %d outside [2, 4096]", field, v);
        return false;
    };
    if (!size_ok("src_w", p->src_w) || !size_ok("src_h", p->src_h) || !size_ok("dst_w", dst_w) || !size_ok("dst_h", dst_h)) return VSLAM_ERR_ARG;
    for (int s = 0; s < 2; ++s) {
        const vslam_rectify_cam& c = p->cam[s];
        const struct { const char* name; const double* v; int n; } arrays[] = {{"K", c.K, 4}, {"D", c.D, 8}, {"R", c.R, 9}, {"P", c.P, 4}};
        for (const auto& a : arrays)
            for (int i = 0; i < a.n; ++i)
                if (!std::isfinite(a.v[i])) { set_error("vslam_rectify_params.cam[%d].%s[%d] is not finite", s, a.name, i); return VSLAM_ERR_ARG; }
        for (int i = 0; i < 2; ++i) {
            if (!(c.K[i] > 0)) { set_error("vslam_rectify_params.cam[%d].K[%d] = %g: the focal length must be > 0", s, i, c.K[i]); return VSLAM_ERR_ARG; }
            if (!(c.P[i] > 0)) { set_error("vslam_rectify_params.cam[%d].P[%d] = %g: the rectified focal length must be > 0", s, i, c.P[i]); return VSLAM_ERR_ARG; }
        }
        double err, det;
        rectify_rotation_error(c.R, &err, &det);
        if (err > 1e-6 || !(det > 0)) {
            set_error("vslam_rectify_params.cam[%d].R is not a rotation: max |R R^T - I| = %g (need <= 1e-6), det = %g (need > 0)", s, err, det);
            return VSLAM_ERR_ARG;
        }
    }
    return VSLAM_OK;
}

int vslam_rectify_build_maps(const vslam_rectify_params* p, int cam, int dst_w, int dst_h, int16_t* xy, uint16_t* frac) {
    if (int rc = vslam_rectify_params_check(p, dst_w, dst_h)) return rc;
    if ((cam != 0 && cam != 1) || !xy || !frac) { set_error("vslam_rectify_build_maps: cam must be 0 or 1, xy and frac non-null"); return VSLAM_ERR_ARG; }
    rectify_build_map(p->cam[cam], dst_w, dst_h, xy, frac);
    return VSLAM_OK;
}

// Source side of rectify_kernel: 0 = direct gathers, 1 = LDS-staged boxes (0.93 vs 2.87 ms per 1024 raw pairs; tiles without a box and
// unaligned sources gather); Tuning::rectify_form overrides it (tests and tools/bench_rectify.py run both)
constexpr int kRectifyFormDefault = 1;
static int rectify_form(const Ctx* c) { return c->tune.rectify_form >= 0 ? c->tune.rectify_form : kRectifyFormDefault; }

// pack + upload one camera's map (allocates the context's slot on first use; the stream is idle when the old entries are overwritten)
static int rectify_upload(Ctx* c, int cam, const std::vector<uint2>& packed, int src_w, int src_h) {
    std::vector<int4> tiles((size_t)rectify_tiles_x(c->p.img_w) * ((c->p.img_h + 3) / 4));
    rectify_tile_boxes(packed.data(), c->p.img_w, c->p.img_h, tiles.data());
    VS_HIP(hipStreamSynchronize(c->stream));
    if (!c->rect.d_map[cam]) { int rc = dev_alloc(c, &c->rect.d_map[cam], packed.size()); if (rc) return rc; }
    if (!c->rect.d_tiles[cam]) { int rc = dev_alloc(c, &c->rect.d_tiles[cam], tiles.size()); if (rc) return rc; }
    VS_HIP(hipMemcpy(c->rect.d_map[cam], packed.data(), packed.size() * sizeof(uint2), hipMemcpyHostToDevice));
    VS_HIP(hipMemcpy(c->rect.d_tiles[cam], tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice));
    c->rect.src_w[cam] = src_w; c->rect.src_h[cam] = src_h;
    return VSLAM_OK;
}

int vslam_rectify_set(vslam_ctx* ctx, const vslam_rectify_params* p) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("null context"); return VSLAM_ERR_ARG; }
    const int w = c->p.img_w, h = c->p.img_h;
    if (int rc = vslam_rectify_params_check(p, w, h)) return rc;
    VS_ENTER(c);
    std::vector<uint2> packed[2];
    std::vector<int16_t> xy((size_t)w * h * 2);
    std::vector<uint16_t> frac((size_t)w * h);
    for (int s = 0; s < 2; ++s) { // (both maps exist on the host before the first one replaces anything on the device)
        rectify_build_map(p->cam[s], w, h, xy.data(), frac.data());
        packed[s].resize((size_t)rectify_map_pitch(w) * h);
        rectify_pack_map(xy.data(), frac.data(), w, h, p->src_w, p->src_h, packed[s].data());
    }
    for (int s = 0; s < 2; ++s)
        if (int rc = rectify_upload(c, s, packed[s], p->src_w, p->src_h)) return rc;
    return VSLAM_OK;
}

int vslam_rectify_set_maps(vslam_ctx* ctx, int cam, const int16_t* xy, const uint16_t* frac, int src_w, int src_h) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !xy || !frac || (cam != 0 && cam != 1)) { set_error("vslam_rectify_set_maps: null argument or cam outside 0 | 1"); return VSLAM_ERR_ARG; }
    if (src_w < 2 || src_w > 4096 || src_h < 2 || src_h > 4096) { set_error("vslam_rectify_set_maps: source size %d x %d outside [2, 4096]", src_w, src_h); return VSLAM_ERR_ARG; }
    const int w = c->p.img_w, h = c->p.img_h;
    for (size_t i = 0; i < (size_t)w * h; ++i)
        if (frac[i] >= 1024) { set_error("vslam_rectify_set_maps: frac[%zu] = %d is not ay * 32 + ax with ax, ay < 32", i, (int)frac[i]); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    std::vector<uint2> packed((size_t)rectify_map_pitch(w) * h);
    rectify_pack_map(xy, frac, w, h, src_w, src_h, packed.data());
    return rectify_upload(c, cam, packed, src_w, src_h);
}

int vslam_rectify_dev(vslam_ctx* ctx, const uint8_t* d_src_left, const uint8_t* d_src_right, size_t src_img_bytes, int src_pitch, int B,
                      uint8_t* d_dst_left, uint8_t* d_dst_right, size_t dst_img_bytes, int dst_pitch) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("null context"); return VSLAM_ERR_ARG; }
    const uint8_t* src[2] = {d_src_left, d_src_right};
    uint8_t* dst[2] = {d_dst_left, d_dst_right};
    if ((!src[0] != !dst[0]) || (!src[1] != !dst[1]) || (!src[0] && !src[1])) {
        set_error("vslam_rectify_dev: a side is its source AND its destination pointer (both NULL = skipped), and at least one side is needed"); return VSLAM_ERR_ARG;
    }
    if (B < 1 || B > c->p.max_batch) { set_error("batch %d outside 1..max_batch %d", B, c->p.max_batch); return VSLAM_ERR_ARG; }
    RectifyLaunch L{};
    for (int s = 0; s < 2; ++s) {
        if (!src[s]) continue;
        if (!c->rect.d_map[s]) { set_error("vslam_rectify_dev: no map set for camera %d (vslam_rectify_set / vslam_rectify_set_maps)", s); return VSLAM_ERR_ARG; }
        if (src_pitch < c->rect.src_w[s] || src_img_bytes < (size_t)src_pitch * c->rect.src_h[s] || (uint64_t)src_pitch * c->rect.src_h[s] > 0xFFFFFFFFull) {
            set_error("vslam_rectify_dev: src_pitch %d / src_img_bytes %zu do not hold camera %d's %d x %d source", src_pitch, src_img_bytes, s, c->rect.src_w[s], c->rect.src_h[s]);
            return VSLAM_ERR_ARG;
        }
        L.map[s] = c->rect.d_map[s]; L.tiles[s] = c->rect.d_tiles[s]; L.src[s] = src[s]; L.dst[s] = dst[s];
    }
    if (dst_pitch < c->p.img_w || dst_img_bytes < (size_t)dst_pitch * c->p.img_h) {
        set_error("vslam_rectify_dev: dst_pitch %d / dst_img_bytes %zu do not hold the context's %d x %d image", dst_pitch, dst_img_bytes, c->p.img_w, c->p.img_h);
        return VSLAM_ERR_ARG;
    }
    VS_ENTER(c);
    L.form = rectify_form(c);
    L.w = c->p.img_w; L.h = c->p.img_h; L.B = B; L.src_pitch = src_pitch; L.dst_pitch = dst_pitch; L.src_img_bytes = src_img_bytes; L.dst_img_bytes = dst_img_bytes;
    return launch_rectify(L, c->stream);
}

int vslam_rectify(vslam_ctx* ctx, int cam, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !src || !dst || (cam != 0 && cam != 1)) { set_error("vslam_rectify: null argument or cam outside 0 | 1"); return VSLAM_ERR_ARG; }
    if (!c->rect.d_map[cam]) { set_error("vslam_rectify: no map set for camera %d (vslam_rectify_set / vslam_rectify_set_maps)", cam); return VSLAM_ERR_ARG; }
    const int sw = c->rect.src_w[cam], sh = c->rect.src_h[cam], w = c->p.img_w, h = c->p.img_h;
    if (src_stride < sw || dst_stride < w) { set_error("vslam_rectify: src_stride %d < %d or dst_stride %d < %d", src_stride, sw, dst_stride, w); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    int rc;
    const int sp = img_pitch(sw), dp = img_pitch(w);
    uint8_t *d_s, *d_d;
    if ((rc = arena_stage(c, [&](Arena& a) { d_s = a.take<uint8_t>((size_t)sp * sh); d_d = a.take<uint8_t>((size_t)dp * h); }))) return rc;
    if ((rc = upload_image(c, d_s, src, sw, sh, src_stride))) return rc;
    RectifyLaunch L{};
    L.map[cam] = c->rect.d_map[cam]; L.tiles[cam] = c->rect.d_tiles[cam]; L.src[cam] = d_s; L.dst[cam] = d_d; L.form = rectify_form(c);
    L.w = w; L.h = h; L.B = 1; L.src_pitch = sp; L.dst_pitch = dp; L.src_img_bytes = (size_t)sp * sh; L.dst_img_bytes = (size_t)dp * h;
    if ((rc = launch_rectify(L, c->stream))) return rc;
    std::vector<uint8_t> out((size_t)dp * h);
    VS_HIP(hipMemcpyAsync(out.data(), d_d, out.size(), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    for (int y = 0; y < h; ++y) memcpy(dst + (size_t)y * dst_stride, out.data() + (size_t)y * dp, (size_t)w);
    return VSLAM_OK;
}

int vslam_find_3d_disparity(vslam_ctx* ctx, const vslam_keypoint* kps, int n, const float* disparity, int w, int h, int dstride,
                            const double T_c_w[7], float* xyz_w, uint8_t* valid, uint8_t* reliable, int* n_valid) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n < 0 || !disparity || !T_c_w || w <= 0 || h <= 0 || dstride < w || (n > 0 && (!kps || !xyz_w || !valid || !reliable))) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n_valid) *n_valid = 0;
    if (n == 0) return VSLAM_OK;
    VS_ENTER(c);
    int rc;
    const int32_t nn = n;
    vslam_keypoint* d_k; float *d_d, *d_x; double* d_T; int32_t* d_n; uint8_t *d_v, *d_r;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_k = a.in(kps, n);
             d_d = a.in(disparity, (size_t)dstride * h);
             d_T = a.in(T_c_w, 7);
             d_n = a.in(&nn, 1);
             d_x = a.take<float>(3 * (size_t)n);
             d_v = a.take<uint8_t>(n);
             d_r = a.take<uint8_t>(n);
         }))) return rc;
    if ((rc = launch_find3d_disparity_batch(d_k, d_n, n, 1, d_d, w, h, dstride, (size_t)dstride * h, d_T, cam_of(c), d_x, d_v, d_r, c->stream))) return rc;
    VS_HIP(hipMemcpyAsync(xyz_w, d_x, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(valid, d_v, n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(reliable, d_r, n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    if (n_valid) { int k = 0; for (int i = 0; i < n; ++i) k += valid[i] != 0; *n_valid = k; }
    return VSLAM_OK;
}

int vslam_find_3d_disparity_dev(vslam_ctx* ctx, const vslam_keypoint* d_kps, const int32_t* d_n, int kp_capacity, int B, const float* d_disparity,
                                int w, int h, const double* d_T_c_w, float* d_xyz_w, uint8_t* d_valid, uint8_t* d_reliable) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_kps || !d_n || !d_disparity || !d_T_c_w || !d_xyz_w || !d_valid || !d_reliable || kp_capacity <= 0 || w <= 0 || h <= 0 || B < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_find3d_disparity_batch(d_kps, d_n, kp_capacity, B, d_disparity, w, h, w, (size_t)w * h, d_T_c_w, cam_of(c), d_xyz_w, d_valid, d_reliable, c->stream);
}

int vslam_triangulate_dev(vslam_ctx* ctx, const float* d_uvL, const float* d_uvR, const int32_t* d_n, int capacity, int B,
                          const double* d_T_c_w, float* d_xyz_w, uint8_t* d_valid, uint8_t* d_reliable) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_uvL || !d_uvR || !d_n || !d_T_c_w || !d_xyz_w || !d_valid || !d_reliable || capacity <= 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_triangulate(d_uvL, d_uvR, d_n, capacity, B, d_T_c_w, cam_of(c), d_xyz_w, d_valid, d_reliable, c->stream);
}

int vslam_triangulate(vslam_ctx* ctx, const float* uvL, const float* uvR, int n, const double T_c_w[7], float* xyz_w, uint8_t* valid,
                      uint8_t* reliable, int* n_valid) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n < 0 || !T_c_w || (n > 0 && (!uvL || !uvR || !xyz_w || !valid || !reliable))) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n_valid) *n_valid = 0;
    if (n == 0) return VSLAM_OK;
    VS_ENTER(c);
    int rc;
    const int32_t nn = n;
    float *d_l, *d_r, *d_x; double* d_T; int32_t* d_n; uint8_t *d_v, *d_rel;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_l = a.in(uvL, 2 * (size_t)n);
             d_r = a.in(uvR, 2 * (size_t)n);
             d_T = a.in(T_c_w, 7);
             d_n = a.in(&nn, 1);
             d_x = a.take<float>(3 * (size_t)n);
             d_v = a.take<uint8_t>(n);
             d_rel = a.take<uint8_t>(n);
         }))) return rc;
    if ((rc = launch_triangulate(d_l, d_r, d_n, n, 1, d_T, cam_of(c), d_x, d_v, d_rel, c->stream))) return rc;
    VS_HIP(hipMemcpyAsync(xyz_w, d_x, 12 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(valid, d_v, n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(reliable, d_rel, n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    if (n_valid) { int k = 0; for (int i = 0; i < n; ++i) k += valid[i] != 0; *n_valid = k; }
    return VSLAM_OK;
}

int vslam_gather_matched_uv_dev(vslam_ctx* ctx, const vslam_keypoint* d_kpsQ, const vslam_keypoint* d_kpsT, int kp_capacity,
                                const vslam_dmatch* d_matches, const int32_t* d_nmatch, int match_capacity, int B, float* d_uvQ, float* d_uvT) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_kpsQ || !d_kpsT || !d_matches || !d_nmatch || !d_uvQ || !d_uvT || kp_capacity <= 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_gather_uv(d_kpsQ, d_kpsT, kp_capacity, d_matches, d_nmatch, match_capacity, B, d_uvQ, d_uvT, c->stream);
}

int vslam_check_motion(int num_inliers, const double T_c_l[7], double frame_gap) {
    if (!T_c_l) return 0;
    return check_motion_rule(num_inliers, T_c_l, frame_gap) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- motion-only pose
int vslam_pnp_motion_only_dev(vslam_ctx* ctx, const float* d_xyz_w, const float* d_uv, const int32_t* d_n, int capacity, int B,
                              double* d_T_c_w, int iters, uint8_t* d_inlier, int32_t* d_n_inliers) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_xyz_w || !d_uv || !d_n || !d_T_c_w || capacity <= 0 || iters < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    PnpArgs p = pnp_args_of(c, d_xyz_w, d_uv, d_n, capacity, B, d_T_c_w, iters);
    p.inlier = d_inlier; p.n_inliers = d_n_inliers;
    return launch_pnp(p, &c->lm, c->stream);
}

int vslam_pnp_motion_only(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int iters, uint8_t* inlier,
                          int* n_inliers, vslam_lm_stats* stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !xyz_w || !uv || n <= 0 || !T_c_w || iters < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    int rc;
    const int32_t nn = n;
    float *d_x, *d_u; double* d_T; int32_t* d_n; uint8_t* d_in; vslam_lm_stats* d_st;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_x = a.in(xyz_w, 3 * (size_t)n);
             d_u = a.in(uv, 2 * (size_t)n);
             d_T = a.in(T_c_w, 7);
             d_n = a.take<int32_t>(2); // (point count in, inlier count out)
             d_in = a.take<uint8_t>(n);
             d_st = a.take<vslam_lm_stats>(1);
         }))) return rc;
    VS_HIP(hipMemcpyAsync(d_n, &nn, 4, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemsetAsync(d_st, 0, sizeof(vslam_lm_stats), c->stream));
    PnpArgs p = pnp_args_of(c, d_x, d_u, d_n, n, 1, d_T, iters);
    p.inlier = d_in; p.n_inliers = d_n + 1; p.stats = d_st; p.n_hint = n;
    if ((rc = launch_pnp(p, &c->lm, c->stream))) return rc;
    int32_t ni = 0;
    VS_HIP(hipMemcpyAsync(T_c_w, d_T, 56, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(&ni, d_n + 1, 4, hipMemcpyDeviceToHost, c->stream));
    if (inlier) VS_HIP(hipMemcpyAsync(inlier, d_in, n, hipMemcpyDeviceToHost, c->stream));
    if (stats) VS_HIP(hipMemcpyAsync(stats, d_st, sizeof(vslam_lm_stats), hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    if (n_inliers) *n_inliers = ni;
    return VSLAM_OK;
}

// Host-buffer RANSAC (include/vslam_hip.h): stages the caller's points and runs the batched launch at B = 1.  The subset draw, EPnP, the scoring
// and the acceptance replay are launch_pnp_ransac_batch's (pnp_kernels.hip); the only other restatement of that control flow is oracle/ransac.c
static int pnp_ransac_impl(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int max_iters, double reproj_err,
                           double confidence, int lm_iters, uint8_t* inlier, int* n_inliers, int* iters_run, double* models_Rt, int32_t* models_count) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !xyz_w || !uv || n < 0 || !T_c_w || max_iters < 0 || max_iters > 4096 || lm_iters < 0 || !(reproj_err > 0)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n_inliers) *n_inliers = 0;
    if (iters_run) *iters_run = 0;
    if (inlier && n > 0) memset(inlier, 0, (size_t)n);
    const int mp = 5;
    if (n < mp || max_iters == 0) return VSLAM_OK;
    VS_ENTER(c);
    int rc;
    const int32_t nn = n;
    float *d_x, *d_u, *d_ix, *d_iu; double* d_T; int32_t *d_n, *d_res; uint8_t* d_mask;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_x = a.in(xyz_w, 3 * (size_t)n); d_u = a.in(uv, 2 * (size_t)n);
             d_n = a.in(&nn, 1);
             d_T = a.take<double>(7); d_mask = a.take<uint8_t>(n);
             d_res = a.take<int32_t>(3); // inlier count and iterations run out; [2]: the refinement's point count in
             d_ix = a.take<float>(3 * (size_t)n); d_iu = a.take<float>(2 * (size_t)n);
         }))) return rc;
    double K[4];
    fill_K(c, K);
    RansacTables tab;
    if ((rc = launch_pnp_ransac_batch(d_x, d_u, d_n, n, 1, max_iters, K, reproj_err, confidence, c->ransac, d_T, d_mask, d_res, d_res + 1, c->stream, &tab))) return rc;
    const bool single = n == mp; // ptsetreg.cpp: count == modelPoints -> one model from all points, every point an inlier
    const int H = single ? 1 : max_iters;
    double T[7]; int32_t res[2];
    std::vector<uint8_t> mask(n);
    std::vector<int32_t> cnt(H), okv(H);
    VS_HIP(hipMemcpyAsync(T, d_T, 56, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(mask.data(), d_mask, n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipMemcpyAsync(res, d_res, 8, hipMemcpyDeviceToHost, c->stream));
    if (models_Rt) {
        VS_HIP(hipMemcpyAsync(models_Rt, tab.Rt, (size_t)H * 96, hipMemcpyDeviceToHost, c->stream));
        VS_HIP(hipMemcpyAsync(okv.data(), tab.ok, (size_t)H * 4, hipMemcpyDeviceToHost, c->stream));
        VS_HIP(hipMemcpyAsync(cnt.data(), tab.counts, (size_t)H * 4, hipMemcpyDeviceToHost, c->stream));
    }
    VS_HIP(hipStreamSynchronize(c->stream));
    if (models_count) for (int i = 0; i < H; ++i) models_count[i] = okv[i] ? (single ? n : cnt[i]) : -1;
    if (iters_run) *iters_run = res[1];
    const int max_good = res[0];
    if (max_good <= 0) return VSLAM_OK; // no model accepted: T_c_w stays as the caller left it
    // lm_iters > 0: refinement on the best model's inliers (solvePnP on the inliers; deviation R2 of oracle/ransac.c)
    std::vector<float> ix, iu;
    for (int i = 0; i < n; ++i) if (mask[i]) { ix.insert(ix.end(), xyz_w + 3 * (size_t)i, xyz_w + 3 * (size_t)i + 3); iu.insert(iu.end(), uv + 2 * (size_t)i, uv + 2 * (size_t)i + 2); }
    const int32_t m = (int32_t)(iu.size() / 2);
    if (m != max_good) { set_error("RANSAC inlier recount mismatch (%d vs %d)", m, max_good); return VSLAM_ERR_HIP; }
    if (lm_iters > 0) { // (0 = OpenCV 3.2.0: solvePnPRansac assigns _local_model, the best RANSAC model, to rvec / tvec; the refined pose is discarded)
        VS_HIP(hipMemcpyAsync(d_ix, ix.data(), ix.size() * 4, hipMemcpyHostToDevice, c->stream));
        VS_HIP(hipMemcpyAsync(d_iu, iu.data(), iu.size() * 4, hipMemcpyHostToDevice, c->stream));
        VS_HIP(hipMemcpyAsync(d_res + 2, &m, 4, hipMemcpyHostToDevice, c->stream));
        PnpArgs p = pnp_args_of(c, d_ix, d_iu, d_res + 2, m, 1, d_T, lm_iters); // (d_T holds the best model: the seed)
        p.huber_delta = 1e300; p.reproj_thr = reproj_err; p.n_hint = m;
        if ((rc = launch_pnp(p, &c->lm, c->stream))) return rc;
        VS_HIP(hipMemcpyAsync(T, d_T, 56, hipMemcpyDeviceToHost, c->stream));
        VS_HIP(hipStreamSynchronize(c->stream));
    }
    memcpy(T_c_w, T, 56);
    if (inlier) memcpy(inlier, mask.data(), n);
    if (n_inliers) *n_inliers = max_good;
    return VSLAM_OK;
}

int vslam_pnp_ransac(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int max_iters, double reproj_err,
                     double confidence, int lm_iters, uint8_t* inlier, int* n_inliers, int* iters_run) {
    return pnp_ransac_impl(ctx, xyz_w, uv, n, T_c_w, max_iters, reproj_err, confidence, lm_iters, inlier, n_inliers, iters_run, nullptr, nullptr);
}

int vslam_pnp_ransac_dev(vslam_ctx* ctx, const float* d_xyz_w, const float* d_uv, const int32_t* d_n, int capacity, int B, double* d_T_c_w, int max_iters,
                         double reproj_err, double confidence, uint8_t* d_inlier, int32_t* d_n_inliers, int32_t* d_iters_run) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_xyz_w || !d_uv || !d_n || !d_T_c_w || capacity <= 0 || B < 0 || max_iters <= 0 || max_iters > 4096 || !(reproj_err > 0)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    if (B == 0) return VSLAM_OK;
    double K[4];
    fill_K(c, K);
    return launch_pnp_ransac_batch(d_xyz_w, d_uv, d_n, capacity, B, max_iters, K, reproj_err, confidence, c->ransac, d_T_c_w, d_inlier, d_n_inliers, d_iters_run, c->stream);
}

// diagnostic form: additionally returns every hypothesis model ([R row-major | t], 12 doubles each) and its inlier count (-1: degenerate)
int vslam_pnp_ransac_models(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int max_iters, double reproj_err,
                            double confidence, int lm_iters, uint8_t* inlier, int* n_inliers, int* iters_run, double* models_Rt, int32_t* models_count) {
    if (!models_Rt || !models_count) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    return pnp_ransac_impl(ctx, xyz_w, uv, n, T_c_w, max_iters, reproj_err, confidence, lm_iters, inlier, n_inliers, iters_run, models_Rt, models_count);
}

// ---------------------------------------------------------------------------------------------- window optimisation
// the arrays every entry that optimises a vslam_ba_batch needs
static bool ba_batch_ok(const vslam_ba_batch* b) {
    return b && b->n_windows > 0 && b->d_lm_off && b->d_edge_off && b->d_T_c_w && b->d_xyz && b->d_lm_inlier && b->d_kf_idx && b->d_lm_idx && b->d_uv && b->total_lm > 0 &&
           b->total_edge > 0;
}
// the kernels' view of a batch: its arrays and totals, the context's intrinsics unless the batch brings its own K4, the context's Huber delta
static LmWindowArgs lm_args_of(const Ctx* c, const vslam_ba_batch& b) {
    LmWindowArgs a;
    memset(&a, 0, sizeof(a));
    a.n_windows = b.n_windows; a.n_kf = b.n_kf; a.n_kf_w = b.d_n_kf; a.lm_off = b.d_lm_off; a.edge_off = b.d_edge_off; a.T = b.d_T_c_w; a.xyz = b.d_xyz;
    a.reliable = b.d_reliable; a.lm_inlier = b.d_lm_inlier; a.kf_idx = b.d_kf_idx; a.lm_idx = b.d_lm_idx; a.uv = b.d_uv; a.chi2 = b.d_chi2; a.stats = b.d_stats;
    fill_K(c, a.K); a.huber_delta = c->p.huber_delta; a.total_lm = b.total_lm; a.total_edge = b.total_edge;
    if (b.K4) memcpy(a.K, b.K4, sizeof(a.K));
    return a;
}

// Shared host wrapper of optimize_map / optimize_pose_only: stable-sorts the caller's edges by landmark (the
// kernel's CSR contract), runs one pass on the GPU, un-permutes chi2 and applies the chi2 classification of
// optimization.cpp:224-266 on the host with the caller's flag_lm (quirk Q1 lives in the caller's edge list).
static int window_host(vslam_ctx* ctx, int mode, int n_kf, double* T_c_w, int n_lm, float* xyz, int n_edge, const int32_t* kf_idx,
                       const int32_t* lm_idx, const float* uv, const double* K4, const int32_t* flag_lm, int iters, int update_poses, int update_lms,
                       uint8_t* lm_inlier, double* chi2_out, double* thr_out, vslam_lm_stats* stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n_kf <= 0 || n_kf > VSLAM_MAX_KF || !T_c_w || n_lm <= 0 || !xyz || n_edge < 0 || (n_edge > 0 && (!kf_idx || !lm_idx || !uv)) || iters < 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (n_edge == 0) { // a graph without edges (every landmark of the window classified out): nothing to optimise and no flag to write; poses and landmarks stay
        if (stats) memset(stats, 0, sizeof(*stats));
        if (thr_out) { double th = c->p.huber_delta; for (int iteration = 0; iteration < 5; ++iteration) th *= 2; *thr_out = th; } // (:226-252: a ratio of 0 / 0 is never > 0.5)
        return VSLAM_OK;
    }
    for (int e = 0; e < n_edge; ++e)
        if (kf_idx[e] < 0 || kf_idx[e] >= n_kf || lm_idx[e] < 0 || lm_idx[e] >= n_lm || (flag_lm && (flag_lm[e] < -1 || flag_lm[e] >= n_lm))) { set_error("edge %d: index out of range", e); return VSLAM_ERR_ARG; }
    // counting sort by landmark (stable)
    std::vector<int32_t> ptr(n_lm + 1, 0), perm(n_edge), skf(n_edge), slm(n_edge);
    std::vector<float> suv(2 * (size_t)n_edge);
    for (int e = 0; e < n_edge; ++e) ptr[lm_idx[e] + 1]++;
    for (int l = 0; l < n_lm; ++l) ptr[l + 1] += ptr[l];
    { std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1); for (int e = 0; e < n_edge; ++e) perm[fill[lm_idx[e]]++] = e; }
    for (int j = 0; j < n_edge; ++j) { const int e = perm[j]; skf[j] = kf_idx[e]; slm[j] = lm_idx[e]; suv[2 * j] = uv[2 * e]; suv[2 * j + 1] = uv[2 * e + 1]; }
    VS_ENTER(c);
    int rc;
    double *d_T, *d_chi, *d_thr; float *d_xyz, *d_uv; uint8_t* d_inl; int32_t *d_kf, *d_lm, *d_off; vslam_lm_stats* d_st;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_T = a.in(T_c_w, 7 * (size_t)n_kf);
             d_xyz = a.in(xyz, 3 * (size_t)n_lm);
             d_inl = a.take<uint8_t>(n_lm);
             d_kf = a.take<int32_t>(n_edge);
             d_lm = a.take<int32_t>(n_edge);
             d_uv = a.take<float>(2 * (size_t)n_edge);
             d_chi = a.take<double>(n_edge);
             d_off = a.take<int32_t>(4);
             d_st = a.take<vslam_lm_stats>(1);
             d_thr = a.take<double>(1);
         }))) return rc;
    const int32_t off[4] = {0, n_lm, 0, n_edge};
    VS_HIP(hipMemsetAsync(d_inl, 1, n_lm, c->stream)); // the caller already filtered the graph (optimization.cpp:160 / :334)
    VS_HIP(hipMemcpyAsync(d_kf, skf.data(), 4 * (size_t)n_edge, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemcpyAsync(d_lm, slm.data(), 4 * (size_t)n_edge, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemcpyAsync(d_uv, suv.data(), 8 * (size_t)n_edge, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemcpyAsync(d_off, off, sizeof(off), hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipMemsetAsync(d_st, 0, sizeof(vslam_lm_stats), c->stream));
    VS_HIP(hipMemsetAsync(d_chi, 0, 8 * (size_t)n_edge, c->stream));
    const vslam_ba_batch b = {1, n_kf, d_off, d_off + 2, d_T, d_xyz, nullptr, d_inl, d_kf, d_lm, d_uv, d_chi, d_st, n_lm, n_edge, K4, nullptr}; // (K4: the caller's `const cv::Mat& K`, optimization.hpp:137-139)
    LmWindowArgs a = lm_args_of(c, b);
    a.chi2_thr = d_thr;
    if ((rc = launch_lm_windows(a, 0, mode, iters, update_poses, update_lms, &c->lm, c->stream))) return rc;
    int32_t status = 0;
    if ((rc = lm_fetch_status(&c->lm, 1, &status, c->stream))) return rc;
    if (status != VSLAM_OK) { set_error("window optimisation rejected the graph (duplicate (keyframe, landmark) edge or bad index)"); return status; }
    std::vector<double> chi(n_edge), chi_sorted(n_edge);
    VS_HIP(hipMemcpy(chi_sorted.data(), d_chi, 8 * (size_t)n_edge, hipMemcpyDeviceToHost));
    for (int j = 0; j < n_edge; ++j) chi[perm[j]] = chi_sorted[j];
    if (update_poses) VS_HIP(hipMemcpy(T_c_w, d_T, 56 * (size_t)n_kf, hipMemcpyDeviceToHost));
    if (mode == 0 && update_lms) VS_HIP(hipMemcpy(xyz, d_xyz, 12 * (size_t)n_lm, hipMemcpyDeviceToHost));
    if (stats) VS_HIP(hipMemcpy(stats, d_st, sizeof(vslam_lm_stats), hipMemcpyDeviceToHost));
    if (chi2_out) memcpy(chi2_out, chi.data(), 8 * (size_t)n_edge);
    // adaptive threshold + flags (optimization.cpp:224-266), caller's edge order
    double th = c->p.huber_delta; // optimization.cpp:154: one variable (chi2_th) is both the Huber delta and the initial chi2 threshold
    for (int iteration = 0; iteration < 5; ++iteration) {
        int out = 0, in = 0;
        for (int e = 0; e < n_edge; ++e) { if (chi[e] > th) ++out; else ++in; }
        if (in / double(in + out) > 0.5) break;
        th *= 2;
    }
    if (lm_inlier)
        for (int e = 0; e < n_edge; ++e) {
            const int l = flag_lm ? flag_lm[e] : lm_idx[e];
            if (l >= 0) lm_inlier[l] = !(chi[e] > th);
        }
    if (thr_out) *thr_out = th;
    return VSLAM_OK;
}

int vslam_local_ba(vslam_ctx* ctx, int n_kf, double* T_c_w, int n_lm, float* xyz, int n_edge, const int32_t* kf_idx, const int32_t* lm_idx,
                   const float* uv, const double* K4, const int32_t* flag_lm, int iters, int update_poses, int update_lms, uint8_t* lm_inlier, double* chi2_out,
                   double* chi2_threshold_out, vslam_lm_stats* stats) {
    return window_host(ctx, 0, n_kf, T_c_w, n_lm, xyz, n_edge, kf_idx, lm_idx, uv, K4, flag_lm, iters, update_poses, update_lms, lm_inlier, chi2_out,
                       chi2_threshold_out, stats);
}

int vslam_pose_only_window(vslam_ctx* ctx, int n_kf, double* T_c_w, int n_lm, const float* xyz, int n_edge, const int32_t* kf_idx,
                           const int32_t* lm_idx, const float* uv, const double* K4, const int32_t* flag_lm, int iters, int update_poses, uint8_t* lm_inlier,
                           double* chi2_out, double* chi2_threshold_out, vslam_lm_stats* stats) {
    return window_host(ctx, 1, n_kf, T_c_w, n_lm, const_cast<float*>(xyz), n_edge, kf_idx, lm_idx, uv, K4, flag_lm, iters, update_poses, 0, lm_inlier,
                       chi2_out, chi2_threshold_out, stats);
}

int vslam_ba_batch_dev(vslam_ctx* ctx, const vslam_ba_batch* b, int schedule, int mode, int iters, int update_poses, int update_lms) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !ba_batch_ok(b)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_lm_windows(lm_args_of(c, *b), schedule, mode, iters, update_poses, update_lms, &c->lm, c->stream);
}

// a table is in place: the call must cover exactly its frames, and a chunk of a longer sequence (sequence mode across ranks) stays single-sequence
static int seg_refuses(const Ctx* c, int n_frames, bool chunk) {
    if (!c->seg.first) return VSLAM_OK;
    if (n_frames != c->seg_frames) { set_error("the segment table covers %d frames, this call has %d (vslam_set_segments(ctx, 0, NULL) clears the table)", c->seg_frames, n_frames); return VSLAM_ERR_ARG; }
    if (chunk) { set_error("a segment table is set: chunk inputs (d_T_abs / d_carry_in / d_carry_out) are not available, sequence mode across ranks is single-sequence"); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

// ---- landmark identities out of the window builders, and the chained BA on them (the contract: include/vslam_hip.h)
int vslam_set_window_ids(vslam_ctx* ctx, int32_t* d_lm_id, int capacity) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("null context"); return VSLAM_ERR_ARG; }
    if (capacity < 0 || (capacity == 0) != (d_lm_id == nullptr)) { set_error("vslam_set_window_ids: a buffer with capacity >= 1, or NULL with 0 to clear it"); return VSLAM_ERR_ARG; }
    c->ids = d_lm_id; c->ids_cap = capacity;
    return VSLAM_OK;
}

int vslam_ba_chain_dev(vslam_ctx* ctx, const vslam_ba_batch* b, const int32_t* d_lm_id, const int32_t* d_kf_frame, int min_kf, int32_t* d_ran) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !ba_batch_ok(b)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (!d_lm_id) { set_error("vslam_ba_chain_dev: d_lm_id is required (the landmark ids a window builder wrote, vslam_set_window_ids)"); return VSLAM_ERR_ARG; }
    if (b->n_kf < 1 || b->n_kf > VSLAM_MAX_KF) { set_error("n_kf %d outside 1..%d", b->n_kf, VSLAM_MAX_KF); return VSLAM_ERR_ARG; }
    if (min_kf < 1 || min_kf > b->n_kf) { set_error("vslam_ba_chain_dev: min_kf %d outside 1..n_kf (%d)", min_kf, b->n_kf); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, b->n_windows, false)) return rc;
    VS_ENTER(c);
    // the sequences: the segment table, or the whole batch.  The host knows their lengths, so the loop below never waits for the device.
    const int n_win = b->n_windows, n_seg = c->seg.first ? c->seg.n_seg : 1;
    int n_steps = 0;
    std::vector<int> longer; // longer[j] = sequences with more than j frames = window slots of step j
    {
        std::vector<int> hist(n_win + 2, 0);
        for (int s = 0; s < n_seg; ++s) { const int len = c->seg.first ? c->seg_first_h[s + 1] - c->seg_first_h[s] : n_win; hist[len]++; n_steps = std::max(n_steps, len); }
        longer.assign(n_steps, 0);
        for (int j = n_steps - 1, acc = 0; j >= 0; --j) { acc += hist[j + 1]; longer[j] = acc; }
    }
    const int kp_cap = std::max(c->p.kp_capacity, c->ids_kp_cap);
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.n_windows = n_win; a.n_kf = b->n_kf; a.min_kf = min_kf; a.total_lm = b->total_lm; a.total_edge = b->total_edge;
    a.lm_off = b->d_lm_off; a.edge_off = b->d_edge_off; a.n_kf_w = b->d_n_kf; a.T = b->d_T_c_w; a.xyz = b->d_xyz; a.reliable = b->d_reliable;
    a.lm_inlier = b->d_lm_inlier; a.kf_idx = b->d_kf_idx; a.lm_idx = b->d_lm_idx; a.uv = b->d_uv; a.chi2 = b->d_chi2; a.stats = b->d_stats;
    a.lm_id = d_lm_id; a.kf_frame = d_kf_frame; a.ran = d_ran; a.first = c->seg.first; a.n_seg = n_seg;
    a.n_roots = (long long)n_win * kp_cap;
    const size_t tl = (size_t)b->total_lm, te = (size_t)b->total_edge;
    int32_t* head; size_t head_words = 0;
    if (int rc = carve(c->chain, c->stream, [&](Layout& L) {
            a.pose = L.take<double>((size_t)n_win * 7); a.pose_set = L.take<uint8_t>(n_win); a.bit = L.take<uint8_t>((size_t)a.n_roots); a.status = L.take<int32_t>(n_win);
            const size_t h0 = L.off;
            a.s_lm_off = L.take<int32_t>((size_t)n_seg + 1); a.s_edge_off = L.take<int32_t>((size_t)n_seg + 1); a.s_n_kf = L.take<int32_t>(n_seg); a.s_win = L.take<int32_t>(n_seg);
            head = a.s_lm_off; head_words = (L.off - h0) / sizeof(int32_t);
            a.s_T = L.take<double>((size_t)n_seg * b->n_kf * 7); a.s_xyz = L.take<float>(tl * 3); a.s_rel = L.take<uint8_t>(tl); a.s_inl = L.take<uint8_t>(tl);
            a.s_kf = L.take<int32_t>(te); a.s_lm = L.take<int32_t>(te); a.s_uv = L.take<float>(te * 2);
            a.s_chi2 = L.take<double>(b->d_chi2 ? te : 0); a.s_stats = L.take<vslam_lm_stats>(b->d_stats ? n_seg : 0);
        })) return rc;
    if (!b->d_reliable) a.s_rel = nullptr;
    if (!b->d_chi2) a.s_chi2 = nullptr;
    if (!b->d_stats) a.s_stats = nullptr;
    VS_HIP(hipMemsetAsync(a.pose_set, 0, n_win, c->stream));
    VS_HIP(hipMemsetAsync(a.bit, 1, (size_t)a.n_roots, c->stream)); // is_inlier = 1 until some window has written it
    VS_HIP(hipMemsetAsync(a.status, 0, sizeof(int32_t) * n_win, c->stream));
    VS_HIP(hipMemsetAsync(head, 0, sizeof(int32_t) * head_words, c->stream));
    const vslam_ba_batch staged = {0, b->n_kf, a.s_lm_off, a.s_edge_off, a.s_T, a.s_xyz, a.s_rel, a.s_inl, a.s_kf, a.s_lm, a.s_uv, a.s_chi2, a.s_stats, b->total_lm, b->total_edge,
                                   b->K4, a.s_n_kf}; // (n_windows: per step, below)
    LmWindowArgs w = lm_args_of(c, staged);
    for (int j = 0; j < n_steps; ++j) {
        const int n_slots = longer[j];
        w.n_windows = n_slots;
        if (int rc = launch_chain_stage(a, j, n_slots, c->stream)) return rc;
        if (int rc = launch_lm_windows(w, 1, 0, 10, 1, 0, &c->lm, c->stream)) return rc; // (the schedule of vslam_ba_batch_dev(schedule = 1))
        if (int rc = launch_chain_scatter(a, n_slots, c->lm.last.status, c->stream)) return rc;
    }
    // vslam_ba_status_dev: per window of the caller's batch, the status word of the step that ran it
    c->lm.last = LmLast::of_chain(a.status, n_win);
    return VSLAM_OK;
}

// ---- several independent sequences in one batch (the rules: include/vslam_hip.h)
int vslam_set_segments(vslam_ctx* ctx, int n_seg, const int32_t* first) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) { set_error("null context"); return VSLAM_ERR_ARG; }
    if (n_seg < 0 || (n_seg == 0) != (first == nullptr)) { set_error("vslam_set_segments: n_seg >= 1 with first (n_seg + 1 entries), or 0 with NULL to clear the table"); return VSLAM_ERR_ARG; }
    if (n_seg > 0) {
        if (first[0] != 0) { set_error("vslam_set_segments: first[0] = %d, must be 0", first[0]); return VSLAM_ERR_ARG; }
        for (int k = 0; k < n_seg; ++k)
            if (first[k + 1] <= first[k]) { set_error("vslam_set_segments: first[%d] = %d does not ascend past first[%d] = %d", k + 1, first[k + 1], k, first[k]); return VSLAM_ERR_ARG; }
    }
    VS_ENTER(c);
    VS_HIP(hipStreamSynchronize(c->stream)); // (launches in flight may still read the old table)
    if (n_seg == 0) { c->seg = SegView(); c->seg_frames = 0; c->seg_first_h.clear(); return VSLAM_OK; }
    const int n_frames = first[n_seg];
    int32_t *d_first, *d_start, *d_qitem;
    c->seg = SegView(); c->seg_frames = 0; c->seg_first_h.clear(); // (a failed upload leaves no half-written table in place)
    if (int rc = carve(c->segbuf, c->stream, [&](Layout& L) { d_first = L.take<int32_t>((size_t)n_seg + 1); d_start = L.take<int32_t>(n_frames); d_qitem = L.take<int32_t>(n_frames); })) return rc;
    VS_HIP(hipMemcpyAsync(d_first, first, sizeof(int32_t) * ((size_t)n_seg + 1), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_seg_expand(n_frames, n_seg, d_first, d_start, d_qitem, c->stream)) return rc;
    VS_HIP(hipStreamSynchronize(c->stream)); // (`first` is the caller's again on return)
    c->seg.first = d_first; c->seg.start = d_start; c->seg.qitem = d_qitem; c->seg.n_seg = n_seg; c->seg_frames = n_frames;
    c->seg_first_h.assign(first, first + n_seg + 1);
    return VSLAM_OK;
}

// what the builders' walk takes from the context (the default track_rule is resolved here)
static TrackParams track_params_of(const Ctx* c) {
    TrackParams tp;
    fill_K(c, tp.K4); tp.reproj_thr = c->p.pnp_reproj_thr; tp.track_rule = c->tune.track_rule >= 0 ? c->tune.track_rule : 1;
    return tp;
}

// a chunk of a longer sequence (sequence mode across ranks), and the refusal of the entries that need the whole history; who: "<the entry's mode> need(s)"
static bool is_chunk(const vslam_tracks_in* in) { return in->d_T_abs || in->d_carry_in || in->d_carry_out; }
static int chunk_refused(const char* who) {
    set_error("%s the whole history: not available on a chunk (d_T_abs / d_carry_in / d_carry_out set)", who); return VSLAM_ERR_ARG;
}

// the keyframe-policy arguments of the five entries that write the keyframe sets; policy0: the entry's own name for policy 0.  Every such entry checks
// in this order: its required pointers, what only it needs (d_num_inliers / d_pred / map_refuses), this, its chunk refusal, then build_windows' own
static int kf_policy_refuses(int policy, const char* policy0, int n_kf, double near_dist) {
    if (policy != 0 && policy != 1) { set_error("unknown keyframe policy %d (0 %s, 1 reference culling)", policy, policy0); return VSLAM_ERR_ARG; }
    if (n_kf < 1 || n_kf > VSLAM_MAX_KF) { set_error("n_kf %d outside 1..%d", n_kf, VSLAM_MAX_KF); return VSLAM_ERR_ARG; }
    if (!(near_dist >= 0.0)) { set_error("near_dist must be a number >= 0"); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

static int build_windows(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_status,
                         const KfPolicy& kp) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !in || !out || !d_status || in->n_frames <= 0 || n_kf <= 0 || n_kf > VSLAM_MAX_KF || lm_capacity <= 0 || edge_capacity <= 0 ||
        in->kp_capacity <= 0 || in->lr_capacity <= 0 || in->match_capacity <= 0 || in->pnp_capacity <= 0 || !in->d_kps || !in->d_lr || !in->d_nlr ||
        !in->d_xyz || !in->d_valid || !in->d_reliable || (in->n_frames > 1 && (!in->d_f2f || !in->d_nf2f || !in->d_pose_inlier || (!in->d_T_rel && !kp.G))) ||
        !out->d_lm_off || !out->d_edge_off || !out->d_T_c_w || !out->d_xyz || !out->d_reliable || !out->d_lm_inlier || !out->d_kf_idx || !out->d_lm_idx ||
        !out->d_uv || !out->d_n_kf) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if ((long long)in->n_frames * in->kp_capacity > 0x7FFFFFFFll) { set_error("n_frames x kp_capacity exceeds the 31-bit node keys"); return VSLAM_ERR_ARG; }
    if ((in->d_carry_out != nullptr) != (in->carry_out_frame > 0) || in->carry_out_frame < 0 || in->carry_out_frame >= in->n_frames + (in->n_frames == 1 ? 1 : 0)) {
        if (in->d_carry_out || in->carry_out_frame != 0) { set_error("carry_out_frame %d needs d_carry_out and 1 <= carry_out_frame < n_frames (%d)", in->carry_out_frame, in->n_frames); return VSLAM_ERR_ARG; }
    }
    if (in->kp_capacity > 65536) { set_error("kp_capacity %d exceeds 65536 (the window builder packs a keypoint index into 16 bits)", in->kp_capacity); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, in->n_frames, is_chunk(in))) return rc;
    KfPolicy kpi = kp;
    if (c->ids) { // vslam_set_window_ids: the builder also writes every landmark's root
        if (lm_capacity > c->ids_cap) { set_error("lm_capacity %d exceeds the window-id buffer's capacity %d (vslam_set_window_ids)", lm_capacity, c->ids_cap); return VSLAM_ERR_ARG; }
        if (is_chunk(in)) {
            set_error("window ids are set: chunk inputs (d_T_abs / d_carry_in / d_carry_out) are not available, a root from before the batch has no frame index"); return VSLAM_ERR_ARG;
        }
        kpi.lm_id = c->ids; c->ids_kp_cap = in->kp_capacity;
    }
    VS_ENTER(c);
    out->n_windows = in->n_frames; out->n_kf = n_kf; out->total_lm = lm_capacity; out->total_edge = edge_capacity;
    return launch_build_windows(*in, *out, d_status, track_params_of(c), kpi, c->track, c->stream, c->seg);
}

int vslam_build_windows_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_status) {
    const KfPolicy kp = {-1, 0.0, nullptr, nullptr};
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_build_windows_kf_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int policy, double near_dist, int lm_capacity, int edge_capacity,
                               vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status) {
    if (!ctx || !in || !d_kf_frame || !d_evicted) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = kf_policy_refuses(policy, "sliding", n_kf, near_dist)) return rc;
    if (policy == 1 && is_chunk(in)) return chunk_refused("keyframe culling needs");
    const KfPolicy kp = {policy, near_dist, d_kf_frame, d_evicted};
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_build_windows_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int policy, double near_dist, const int32_t* d_num_inliers,
                                  int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_frame_state,
                                  int32_t* d_status) {
    if (!ctx || !in || !d_kf_frame || !d_evicted || !d_frame_state) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (in->n_frames > 1 && !d_num_inliers) { set_error("the keyframe gate needs d_num_inliers (n_frames - 1 pose-stage inlier counts)"); return VSLAM_ERR_ARG; }
    if (int rc = kf_policy_refuses(policy, "oldest evicted", n_kf, near_dist)) return rc;
    if (is_chunk(in)) return chunk_refused("the keyframe gate needs");
    KfPolicy kp = {policy, near_dist, d_kf_frame, d_evicted};
    kp.gate = true; kp.num_inliers = d_num_inliers; kp.frame_state = d_frame_state;
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_chain_poses_dev(vslam_ctx* ctx, int n_frames, const double* d_T_rel, double* d_T_c_w) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n_frames <= 0 || !d_T_c_w || (n_frames > 1 && !d_T_rel)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, n_frames, false)) return rc;
    VS_ENTER(c);
    return launch_chain_poses(n_frames, d_T_rel, d_T_c_w, c->stream, c->seg);
}

// the refinement passes (vslam_build_map_pnp_inputs_dev, vslam_build_windows_map_dev): poses from the caller, so no chunk and no NULL pose table
static int map_refuses(const vslam_tracks_in* in, const double* d_T_c_w) {
    if (is_chunk(in) || in->carry_out_frame != 0) return chunk_refused("the map pose inputs need");
    if (!d_T_c_w) { set_error("d_T_c_w (n_frames x 7 absolute poses) is required"); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

int vslam_gate_states_dev(vslam_ctx* ctx, int n_frames, const double* d_T, int absolute, const int32_t* d_num_inliers, int32_t* d_frame_state) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n_frames <= 0 || !d_frame_state || (n_frames > 1 && (!d_T || !d_num_inliers))) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (absolute != 0 && absolute != 1) { set_error("absolute must be 0 (d_T = T_rel) or 1 (d_T = absolute T_c_w)"); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, n_frames, false)) return rc;
    VS_ENTER(c);
    return launch_gate_states(n_frames, d_T, absolute, d_num_inliers, d_frame_state, c->stream, c->seg);
}

int vslam_frame_pairs_dev(vslam_ctx* ctx, int n_frames, const int32_t* d_frame_state, int32_t* d_pred, double* d_gap) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n_frames <= 0 || !d_frame_state || !d_pred || (n_frames > 1 && !d_gap)) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, n_frames, false)) return rc;
    VS_ENTER(c);
    return launch_frame_pairs(n_frames, d_frame_state, d_pred, d_gap, c->stream, c->seg);
}

int vslam_gate_states_pairs_dev(vslam_ctx* ctx, int n_frames, const double* d_T_c_w, const int32_t* d_pred, const int32_t* d_num_inliers,
                                int32_t* d_frame_state) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n_frames <= 0 || !d_frame_state || !d_pred || (n_frames > 1 && (!d_T_c_w || !d_num_inliers))) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, n_frames, false)) return rc;
    VS_ENTER(c);
    return launch_gate_states_pairs(n_frames, d_T_c_w, d_pred, d_num_inliers, d_frame_state, c->track, c->stream, c->seg);
}

// d_frame_state: null for the ungated entry, required by the gated ones; rq: the re-match of the requery entry (its scratch is filled in here), else null;
// rv: the pairing of the recover entry (with rq), else null
static int map_pnp_inputs(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev, const int32_t* d_frame_state,
                          const MapInputsOut& out, MapRequery* rq, const MapRecover* rv) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !in) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = map_refuses(in, d_T_c_w)) return rc;
    if (out.capacity < 1 || !out.xyz || !out.uv || !out.n || !out.in_of_match || !out.status || in->n_frames <= 0 || in->kp_capacity <= 0 ||
        in->lr_capacity <= 0 || in->match_capacity <= 0 || in->pnp_capacity <= 0 || !in->d_kps || !in->d_lr || !in->d_nlr || !in->d_xyz || !in->d_valid ||
        !in->d_reliable || (in->n_frames > 1 && (!in->d_f2f || !in->d_nf2f || !in->d_pose_inlier))) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if ((long long)in->n_frames * in->kp_capacity > 0x7FFFFFFFll) { set_error("n_frames x kp_capacity exceeds the 31-bit node keys"); return VSLAM_ERR_ARG; }
    if (in->kp_capacity > 65536) { set_error("kp_capacity %d exceeds 65536 (the window builder packs a keypoint index into 16 bits)", in->kp_capacity); return VSLAM_ERR_ARG; }
    if (rq) {
        if (!rq->d_desc || !rq->d_feat || !rq->d_nfeat || !rq->d_f2f_out || !rq->d_nf2f_out || !in->d_nkps) {
            set_error("the re-match needs d_desc, d_feat, d_nfeat, d_f2f_out, d_nf2f_out and in->d_nkps"); return VSLAM_ERR_ARG;
        }
        if ((((uintptr_t)rq->d_desc | (uintptr_t)rq->desc_stride) & 15) != 0 || rq->desc_stride < (size_t)in->kp_capacity * 32) {
            set_error("d_desc and desc_stride_bytes must be multiples of 16 bytes, desc_stride_bytes >= kp_capacity x 32"); return VSLAM_ERR_ARG;
        }
        if (in->kp_capacity > kMaxRows) { set_error("kp_capacity %d exceeds the matcher's %d rows", in->kp_capacity, kMaxRows); return VSLAM_ERR_ARG; }
        if (in->n_frames - 1 > c->p.max_batch) { set_error("%d frame pairs exceed context max_batch %d", in->n_frames - 1, c->p.max_batch); return VSLAM_ERR_ARG; }
        if (in->n_frames > 1) { // the walk reads in->d_f2f while nothing orders it against the re-match's writes: the two tables must not overlap
            const size_t bytes = (size_t)(in->n_frames - 1) * in->match_capacity * sizeof(vslam_dmatch);
            const uintptr_t a = (uintptr_t)in->d_f2f, b = (uintptr_t)rq->d_f2f_out;
            if ((a < b + bytes && b < a + bytes) || in->d_nf2f == rq->d_nf2f_out) { set_error("d_f2f_out / d_nf2f_out must not alias in->d_f2f / in->d_nf2f"); return VSLAM_ERR_ARG; }
        }
        rq->ratio = c->p.match_ratio; rq->gap_thr = c->p.match_gap_thr; rq->d_train_best = c->match.d_train_best;
    }
    if (int rc = seg_refuses(c, in->n_frames, false)) return rc; // (map_refuses above turned every chunk away)
    VS_ENTER(c);
    return launch_map_pnp_inputs(*in, d_T_c_w, d_input_of_match_prev, d_frame_state, track_params_of(c), out, rq, rv, c->track, c->stream, c->seg);
}

int vslam_build_map_pnp_inputs_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev, float* d_xyz_w,
                                   float* d_uv, int32_t* d_n, int32_t* d_input_of_match, int out_capacity, int32_t* d_status) {
    return map_pnp_inputs(ctx, in, d_T_c_w, d_input_of_match_prev, nullptr, {d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status}, nullptr, nullptr);
}

int vslam_build_map_pnp_inputs_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                         const int32_t* d_frame_state, float* d_xyz_w, float* d_uv, int32_t* d_n, int32_t* d_input_of_match, int out_capacity,
                                         int32_t* d_status) {
    if (!d_frame_state) { set_error("the gated walk needs d_frame_state (n_frames states of the previous pass)"); return VSLAM_ERR_ARG; }
    return map_pnp_inputs(ctx, in, d_T_c_w, d_input_of_match_prev, d_frame_state, {d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status}, nullptr, nullptr);
}

int vslam_build_map_pnp_inputs_requery_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                           const int32_t* d_frame_state, const uint8_t* d_desc, size_t desc_stride_bytes, int32_t* d_feat, int32_t* d_nfeat,
                                           vslam_dmatch* d_f2f_out, int32_t* d_nf2f_out, float* d_xyz_w, float* d_uv, int32_t* d_n, int32_t* d_input_of_match,
                                           int out_capacity, int32_t* d_status) {
    if (!d_frame_state) { set_error("the gated walk needs d_frame_state (n_frames states of the previous pass)"); return VSLAM_ERR_ARG; }
    MapRequery rq = {d_desc, desc_stride_bytes, d_feat, d_nfeat, d_f2f_out, d_nf2f_out, 0.0, 0.0, nullptr};
    return map_pnp_inputs(ctx, in, d_T_c_w, d_input_of_match_prev, d_frame_state, {d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status}, &rq, nullptr);
}

int vslam_build_map_pnp_inputs_recover_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                           const int32_t* d_pred_prev, const int32_t* d_frame_state, const uint8_t* d_desc, size_t desc_stride_bytes,
                                           int32_t* d_feat, int32_t* d_nfeat, vslam_dmatch* d_f2f_out, int32_t* d_nf2f_out, float* d_xyz_w, float* d_uv, int32_t* d_n,
                                           int32_t* d_input_of_match, int out_capacity, int32_t* d_pred, double* d_gap, int32_t* d_status) {
    if (!d_frame_state) { set_error("the gated walk needs d_frame_state (n_frames states of the previous pass)"); return VSLAM_ERR_ARG; }
    if (!d_pred || !d_gap) { set_error("the recover entry writes the pairing: d_pred (n_frames) and d_gap (n_frames - 1) are required"); return VSLAM_ERR_ARG; }
    MapRequery rq = {d_desc, desc_stride_bytes, d_feat, d_nfeat, d_f2f_out, d_nf2f_out, 0.0, 0.0, nullptr};
    const MapRecover rv = {d_pred_prev, d_pred, d_gap};
    return map_pnp_inputs(ctx, in, d_T_c_w, d_input_of_match_prev, d_frame_state, {d_xyz_w, d_uv, d_n, d_input_of_match, out_capacity, d_status}, &rq, &rv);
}

int vslam_build_windows_map_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match, int n_kf, int policy,
                                double near_dist, int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted,
                                int32_t* d_status) {
    if (!ctx || !in || !d_kf_frame || !d_evicted) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = map_refuses(in, d_T_c_w)) return rc;
    if (int rc = kf_policy_refuses(policy, "sliding", n_kf, near_dist)) return rc;
    KfPolicy kp = {policy, near_dist, d_kf_frame, d_evicted};
    kp.G = d_T_c_w; kp.in_of_match = d_input_of_match;
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_build_windows_map_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match,
                                      const int32_t* d_frame_state, int n_kf, int policy, double near_dist, int lm_capacity, int edge_capacity,
                                      vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status) {
    if (!ctx || !in || !d_kf_frame || !d_evicted || !d_frame_state) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = map_refuses(in, d_T_c_w)) return rc;
    if (int rc = kf_policy_refuses(policy, "oldest evicted", n_kf, near_dist)) return rc;
    KfPolicy kp = {policy, near_dist, d_kf_frame, d_evicted};
    kp.G = d_T_c_w; kp.in_of_match = d_input_of_match; kp.gate = true; kp.state_in = d_frame_state;
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_build_windows_map_recover_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match,
                                        const int32_t* d_pred, const int32_t* d_frame_state, int n_kf, int policy, double near_dist, int lm_capacity,
                                        int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status) {
    if (!ctx || !in || !d_kf_frame || !d_evicted || !d_frame_state) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (!d_pred) { set_error("d_pred (n_frames: the pairing in->d_f2f was built on) is required"); return VSLAM_ERR_ARG; }
    if (int rc = map_refuses(in, d_T_c_w)) return rc;
    if (int rc = kf_policy_refuses(policy, "oldest evicted", n_kf, near_dist)) return rc;
    KfPolicy kp = {policy, near_dist, d_kf_frame, d_evicted};
    kp.G = d_T_c_w; kp.in_of_match = d_input_of_match; kp.gate = true; kp.state_in = d_frame_state; kp.recover = true; kp.pred_table = d_pred;
    return build_windows(ctx, in, n_kf, lm_capacity, edge_capacity, out, d_status, kp);
}

int vslam_edge_jacobians(vslam_ctx* ctx, int n, const float* xyz_w, const float* uv, const double T_c_w[7], const double* K4, double* err, double* J_pose,
                         double* J_point, double* chi2, double* huber_w) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || n <= 0 || !xyz_w || !uv || !T_c_w) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    int rc;
    float *d_xyz, *d_uv; double *d_T, *d_err, *d_Jp, *d_Jl, *d_chi, *d_hw;
    if ((rc = arena_stage(c, [&](Arena& a) {
             d_xyz = a.in(xyz_w, 3 * (size_t)n);
             d_uv = a.in(uv, 2 * (size_t)n);
             d_T = a.in(T_c_w, 7);
             d_err = a.take<double>(2 * (size_t)n);
             d_Jp = a.take<double>(12 * (size_t)n);
             d_Jl = a.take<double>(6 * (size_t)n);
             d_chi = a.take<double>(n);
             d_hw = a.take<double>(n);
         }))) return rc;
    double K[4];
    fill_K(c, K);
    if (K4) memcpy(K, K4, sizeof(K));
    if ((rc = launch_edge_jacobians(n, d_xyz, d_uv, d_T, K, c->p.huber_delta, d_err, d_Jp, d_Jl, d_chi, d_hw, c->stream))) return rc;
    if (err) VS_HIP(hipMemcpyAsync(err, d_err, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (J_pose) VS_HIP(hipMemcpyAsync(J_pose, d_Jp, 96 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (J_point) VS_HIP(hipMemcpyAsync(J_point, d_Jl, 48 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (chi2) VS_HIP(hipMemcpyAsync(chi2, d_chi, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (huber_w) VS_HIP(hipMemcpyAsync(huber_w, d_hw, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

int vslam_ba_status_dev(vslam_ctx* ctx, int n_windows, int32_t* h_status) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_status || n_windows <= 0) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    return lm_fetch_status(&c->lm, n_windows, h_status, c->stream);
}

int vslam_ba_schedule_passes_dev(vslam_ctx* ctx, int n_windows, int32_t* h_passes) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_passes || n_windows <= 0) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    return lm_fetch_passes(&c->lm, n_windows, h_passes, c->stream);
}

int vslam_ba_deferred_dev(vslam_ctx* ctx, int n_windows, int32_t* h_deferred) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !h_deferred || n_windows <= 0) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    return lm_fetch_deferred(&c->lm, n_windows, h_deferred, c->stream);
}

// ---------------------------------------------------------------------------------------------- profiling + glue
int vslam_profile_enable(vslam_ctx* ctx, int on) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return VSLAM_ERR_ARG;
    if (!c->prof) c->prof = new Prof();
    if (on) { // the common time origin of vslam_profile_intervals: recorded once per device, on the first context that profiles there
        if (c->device < 0 || c->device >= 16) { set_error("vslam_profile_enable: device %d beyond the profiler's table (16)", c->device); return VSLAM_ERR_ARG; }
        std::lock_guard<std::mutex> lock(g_prof_origin_mu);
        if (!g_prof_origin[c->device]) {
            hipEvent_t ev = nullptr;
            VS_HIP(hipSetDevice(c->device));
            VS_HIP(hipEventCreate(&ev));
            VS_HIP(hipEventRecord(ev, c->stream));
            VS_HIP(hipEventSynchronize(ev));
            g_prof_origin[c->device] = ev;
        }
    }
    c->prof->on = on != 0;
    prof_set_current(on ? c->prof : nullptr);
    return VSLAM_OK;
}

int vslam_profile_read(vslam_ctx* ctx, vslam_kernel_time* out, int cap, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out || !n_out || cap <= 0) return VSLAM_ERR_ARG;
    *n_out = 0;
    Prof* p = c->prof;
    if (!p) return VSLAM_OK;
    VS_ENTER(c);
    VS_HIP(hipStreamSynchronize(c->stream));
    int n = 0;
    for (const Prof::Rec& r : p->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = 0.f;
        int k = 0;
        for (; k < n; ++k) if (strncmp(out[k].name, r.name, sizeof(out[k].name) - 1) == 0) break;
        if (k == n) {
            if (n == cap) { p->pool.push_back(r.e0); p->pool.push_back(r.e1); continue; } // (events go back to the pool either way)
            memset(&out[n], 0, sizeof(out[n]));
            strncpy(out[n].name, r.name, sizeof(out[n].name) - 1);
            ++n;
        }
        out[k].total_ms += ms; out[k].launches += r.launches; out[k].calls += 1;
        p->pool.push_back(r.e0); p->pool.push_back(r.e1);
    }
    p->recs.clear();
    *n_out = n;
    return VSLAM_OK;
}

int vslam_profile_intervals(vslam_ctx* ctx, vslam_stage_interval* out, int cap, int* n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out || !n_out || cap <= 0) return VSLAM_ERR_ARG;
    *n_out = 0;
    Prof* p = c->prof;
    hipEvent_t origin = (c->device >= 0 && c->device < 16) ? g_prof_origin[c->device] : nullptr;
    if (!p || !origin) return VSLAM_OK;
    VS_ENTER(c);
    VS_HIP(hipStreamSynchronize(c->stream));
    int n = 0;
    for (const Prof::Rec& r : p->recs) {
        if (n < cap) {
            float a0 = 0.f, a1 = 0.f;
            if (hipEventElapsedTime(&a0, origin, r.e0) == hipSuccess && hipEventElapsedTime(&a1, origin, r.e1) == hipSuccess) {
                memset(&out[n], 0, sizeof(out[n]));
                strncpy(out[n].name, r.name, sizeof(out[n].name) - 1);
                out[n].t0_ms = a0; out[n].t1_ms = a1;
                ++n;
            }
        }
        p->pool.push_back(r.e0); p->pool.push_back(r.e1);
    }
    p->recs.clear();
    *n_out = n;
    return VSLAM_OK;
}

int vslam_build_pnp_inputs_dev(vslam_ctx* ctx, const vslam_dmatch* d_f2f, const int32_t* d_nf2f, int match_capacity,
                               const vslam_dmatch* d_lr, const int32_t* d_nlr, int lr_capacity, const float* d_xyz_lr,
                               const uint8_t* d_valid_lr, const vslam_keypoint* d_kps_cur, int kp_capacity, int B, int32_t* d_kp2lr,
                               float* d_xyz_out, float* d_uv_out, int32_t* d_nout, int out_capacity) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_f2f || !d_nf2f || !d_lr || !d_nlr || !d_xyz_lr || !d_valid_lr || !d_kps_cur || !d_kp2lr || !d_xyz_out || !d_uv_out || !d_nout ||
        match_capacity <= 0 || lr_capacity <= 0 || kp_capacity <= 0 || out_capacity <= 0) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    if (int rc = seg_refuses(c, B + 1, false)) return rc; // (B items = the pairs of B + 1 consecutive frames)
    VS_ENTER(c);
    return launch_build_pnp_inputs(d_f2f, d_nf2f, match_capacity, d_lr, d_nlr, lr_capacity, d_xyz_lr, d_valid_lr, d_kps_cur, kp_capacity, B,
                                   d_kp2lr, d_xyz_out, d_uv_out, d_nout, out_capacity, c->stream, c->seg.start);
}

// ---------------------------------------------------------------------------------------------- dense map
// Form of voxel_fuse_kernel: 0 = every point straight into the global table, 1 = tile sums in LDS first; Tuning::voxel_form overrides
// it (tests and tools/bench_voxel.py run both)
constexpr int kVoxelFormDefault = 1;
static int voxel_form(const Ctx* c) { return c->tune.voxel_form >= 0 ? c->tune.voxel_form : kVoxelFormDefault; }

// ---- the checks and steps the entries of the dense map, the surface map and the place database share
// a voxel size the kernels can use: positive and finite as a float, and so is its reciprocal
static int voxel_size_check(const char* who, double voxel_size) {
    const float vs = (float)voxel_size;
    if (!std::isfinite(voxel_size) || !(voxel_size > 0) || !std::isfinite(vs) || !(vs > 0.f) || !std::isfinite(1.0f / vs)) {
        set_error("%s: voxel_size %g is not a finite positive float", who, voxel_size); return VSLAM_ERR_ARG;
    }
    return VSLAM_OK;
}
// lo = 0: a map to write into; lo = -1: a map to read, or all of them
static int map_id_check(const char* who, int map_id, int lo) {
    if (map_id < lo || map_id > kVoxelMaxMap) { set_error("%s: map_id %d outside [%d, %d]", who, map_id, lo, kVoxelMaxMap); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}
// a counted list: the count is always written, rows only where a capacity gives them room (`have_out`: every output array is there; `null_out`: the
// message's words for one that is not)
static int counted_output_check(const char* who, const void* d_n_out, size_t capacity, bool have_out, const char* null_out) {
    if (!d_n_out || (capacity > 0 && !have_out)) { set_error("%s: null d_n_out, or %s with a capacity", who, null_out); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}
// the first n counter words of a map as they stand after everything queued before the call; synchronises
static int read_counters(const Ctx* c, const unsigned long long* d_counters, unsigned long long* host, int n) {
    VS_HIP(hipMemcpyAsync(host, d_counters, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

int vslam_voxel_create(vslam_ctx* ctx, double voxel_size, int log2_capacity, vslam_voxel_map** out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out) { set_error("vslam_voxel_create: null argument"); return VSLAM_ERR_ARG; }
    *out = nullptr;
    if (int rc = voxel_size_check("vslam_voxel_create", voxel_size)) return rc;
    if (log2_capacity < 10 || log2_capacity > 28) { set_error("vslam_voxel_create: log2_capacity %d outside [10, 28]", log2_capacity); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    VoxelMap* m = new VoxelMap();
    m->t.log2_capacity = log2_capacity; m->t.vs = (float)voxel_size; m->t.inv = 1.0f / m->t.vs;
    if (int rc = m->alloc(c, ((size_t)32 << log2_capacity) + sizeof(unsigned long long) * kVoxelCounters, "vslam_voxel_create")) { delete m; return rc; }
    m->t.slots = m->base;
    m->t.counters = reinterpret_cast<unsigned long long*>(m->t.slots + ((size_t)32 << log2_capacity));
    int rc = launch_voxel_clear(m->t, c->stream);
    if (rc == VSLAM_OK && hipStreamSynchronize(c->stream) != hipSuccess) { set_error("vslam_voxel_create: clearing the table failed"); rc = VSLAM_ERR_HIP; }
    if (rc) { vslam_voxel_destroy(reinterpret_cast<vslam_voxel_map*>(m)); return rc; }
    *out = reinterpret_cast<vslam_voxel_map*>(m);
    return VSLAM_OK;
}

void vslam_voxel_destroy(vslam_voxel_map* vm) {
    VoxelMap* m = reinterpret_cast<VoxelMap*>(vm);
    if (!m) return;
    m->free();
    delete m;
}

int vslam_voxel_clear(vslam_voxel_map* vm) {
    VoxelMap* m = reinterpret_cast<VoxelMap*>(vm);
    if (!m) { set_error("vslam_voxel_clear: null map"); return VSLAM_ERR_ARG; }
    VS_ENTER(m->ctx);
    return launch_voxel_clear(m->t, m->ctx->stream);
}

int vslam_voxel_stats(vslam_voxel_map* vm, struct vslam_voxel_stats* host) {
    VoxelMap* m = reinterpret_cast<VoxelMap*>(vm);
    if (!m || !host || host->struct_size != (int32_t)sizeof(struct vslam_voxel_stats)) { set_error("vslam_voxel_stats: null argument or struct_size mismatch"); return VSLAM_ERR_ARG; }
    VS_ENTER(m->ctx);
    unsigned long long w[kVoxelCounters];
    if (int rc = read_counters(m->ctx, m->t.counters, w, kVoxelCounters)) return rc;
    host->n_occupied = w[0]; host->n_points = w[1]; host->n_dropped_range = w[2]; host->n_dropped_full = w[3]; host->status = (uint32_t)w[4];
    return VSLAM_OK;
}

// the checks the image entries share; fills `a` from the context's camera
static int voxel_images(const Ctx* c, const char* who, const float* d_disparity, int w, int h, int B, const double* d_T_c_w, double z_min, double z_max, int step,
                        VoxelImages& a) {
    if (!d_disparity || !d_T_c_w) { set_error("%s: null pointer", who); return VSLAM_ERR_ARG; }
    if (B < 1 || B > c->p.max_batch || B > 65535) { set_error("%s: batch %d outside 1..max_batch %d", who, B, c->p.max_batch); return VSLAM_ERR_ARG; }
    if (w < 1 || h < 1 || step < 1) { set_error("%s: w %d, h %d and step %d must be >= 1", who, w, h, step); return VSLAM_ERR_ARG; }
    if (!std::isfinite(z_min) || !std::isfinite(z_max) || !(z_min < z_max)) { set_error("%s: the depth gate needs finite z_min < z_max (%g, %g)", who, z_min, z_max); return VSLAM_ERR_ARG; }
    if (((size_t)h + step - 1) / step / 16 + 1 > 65535) { set_error("%s: %d rows exceed the launch grid", who, h); return VSLAM_ERR_ARG; }
    a.disp = d_disparity; a.w = w; a.h = h; a.B = B; a.step = step; a.T = d_T_c_w; a.z_min = z_min; a.z_max = z_max;
    a.fx = c->p.cam[0]; a.fy = c->p.cam[1]; a.cx = c->p.cam[2]; a.cy = c->p.cam[3]; a.b = c->p.cam[4];
    return VSLAM_OK;
}

int vslam_reproject_dev(vslam_ctx* ctx, const float* d_disparity, int w, int h, int B, const double* d_T_c_w, double z_min, double z_max, int step,
                        float* d_xyz, uint8_t* d_valid) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !d_xyz || !d_valid) { set_error("vslam_reproject_dev: null argument"); return VSLAM_ERR_ARG; }
    VoxelImages a;
    if (int rc = voxel_images(c, "vslam_reproject_dev", d_disparity, w, h, B, d_T_c_w, z_min, z_max, step, a)) return rc;
    VS_ENTER(c);
    return launch_reproject(a, d_xyz, d_valid, c->stream);
}

// the front of the entries that fuse disparity maps, by their map ids and with optional gray images, into a map: the checks, and `a` filled
static int map_images(const Ctx* c, const char* who, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch, int w, int h, int B,
                      const double* d_T_c_w, const int32_t* d_map_id, double z_min, double z_max, int step, VoxelImages& a) {
    if (!d_map_id) { set_error("%s: null d_map_id", who); return VSLAM_ERR_ARG; }
    if (int rc = voxel_images(c, who, d_disparity, w, h, B, d_T_c_w, z_min, z_max, step, a)) return rc;
    if (d_gray && (pitch < w || img_bytes < (size_t)pitch * h)) {
        set_error("%s: pitch %d / img_bytes %zu do not hold a %d x %d image", who, pitch, img_bytes, w, h); return VSLAM_ERR_ARG;
    }
    return VSLAM_OK;
}

int vslam_voxel_insert_points_dev(vslam_ctx* ctx, vslam_voxel_map* vm, const float* d_xyz, const uint8_t* d_valid, const uint8_t* d_intensity, size_t n,
                                  int map_id) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    VoxelMap* m = owned_by<VoxelMap>(c, vm, "vslam_voxel_insert_points_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (n > 0 && !d_xyz) { set_error("vslam_voxel_insert_points_dev: null d_xyz"); return VSLAM_ERR_ARG; }
    if (int rc = map_id_check("vslam_voxel_insert_points_dev", map_id, 0)) return rc;
    VS_ENTER(c);
    return launch_voxel_insert_points(m->t, d_xyz, d_valid, d_intensity, n, map_id, c->stream);
}

int vslam_voxel_fuse_disparity_dev(vslam_ctx* ctx, vslam_voxel_map* vm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                                   int w, int h, int B, const double* d_T_c_w, const int32_t* d_map_id, double z_min, double z_max, int step) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    VoxelMap* m = owned_by<VoxelMap>(c, vm, "vslam_voxel_fuse_disparity_dev");
    if (!m) return VSLAM_ERR_ARG;
    VoxelImages a;
    if (int rc = map_images(c, "vslam_voxel_fuse_disparity_dev", d_disparity, d_gray, img_bytes, pitch, w, h, B, d_T_c_w, d_map_id, z_min, z_max, step, a)) return rc;
    VS_ENTER(c);
    return launch_voxel_fuse(m->t, a, d_gray, img_bytes, pitch, d_map_id, voxel_form(c), c->stream);
}

int vslam_voxel_extract_dev(vslam_ctx* ctx, vslam_voxel_map* vm, int map_id, int min_count, vslam_voxel* d_out, int32_t* d_map_out, size_t capacity,
                            uint64_t* d_n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    VoxelMap* m = owned_by<VoxelMap>(c, vm, "vslam_voxel_extract_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (int rc = counted_output_check("vslam_voxel_extract_dev", d_n_out, capacity, d_out, "null d_out")) return rc;
    if (int rc = map_id_check("vslam_voxel_extract_dev", map_id, -1)) return rc;
    VS_ENTER(c);
    return launch_voxel_extract(m->t, map_id, min_count, d_out, d_map_out, capacity, reinterpret_cast<unsigned long long*>(d_n_out), c->stream);
}

// ---------------------------------------------------------------------------------------------- surface map
// Form of the integration: 0 = every block walks all frames of the call, 1 = tsdf_cull_kernel writes a frame mask per block first;
// Tuning::tsdf_form overrides it (tests and tools/bench_tsdf.py run both)
constexpr int kTsdfFormDefault = 1;
static int tsdf_form(const Ctx* c) { return c->tune.tsdf_form >= 0 ? c->tune.tsdf_form : kTsdfFormDefault; }

int vslam_tsdf_create(vslam_ctx* ctx, double voxel_size, int trunc_voxels, int log2_blocks, vslam_tsdf_map** out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out) { set_error("vslam_tsdf_create: null argument"); return VSLAM_ERR_ARG; }
    *out = nullptr;
    if (int rc = voxel_size_check("vslam_tsdf_create", voxel_size)) return rc;
    if (trunc_voxels < 1 || trunc_voxels > 8) { set_error("vslam_tsdf_create: trunc_voxels %d outside [1, 8]", trunc_voxels); return VSLAM_ERR_ARG; }
    if (log2_blocks < 6 || log2_blocks > 22) { set_error("vslam_tsdf_create: log2_blocks %d outside [6, 22]", log2_blocks); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    TsdfMap* m = new TsdfMap(&c->dev_bytes);
    TsdfTable& t = m->t;
    const size_t n = (size_t)1 << log2_blocks, words = ((size_t)c->p.max_batch + 63) / 64;
    // one allocation: pool | keys | frame masks | frame table | counters | list (every part a multiple of 8 bytes, the pool 16-byte aligned)
    const size_t pool_b = n * 8192, keys_b = n * 8, pairs_b = n * words * 8, frames_b = (size_t)c->p.max_batch * kTsdfFrameDoubles * 8, cnt_b = 8 * kTsdfCounters;
    t.log2_blocks = log2_blocks; t.J = trunc_voxels; t.frame_words = (int)words; t.vs = (float)voxel_size; t.inv = 1.0f / t.vs;
    if (int rc = m->alloc(c, pool_b + keys_b + pairs_b + frames_b + cnt_b + n * 4, "vslam_tsdf_create")) { delete m; return rc; }
    uint8_t* p = m->base;
    t.pool = reinterpret_cast<uint4*>(p); p += pool_b;
    t.keys = reinterpret_cast<unsigned long long*>(p); p += keys_b;
    t.pairs = reinterpret_cast<unsigned long long*>(p); p += pairs_b;
    t.frames = reinterpret_cast<double*>(p); p += frames_b;
    t.counters = reinterpret_cast<unsigned long long*>(p); p += cnt_b;
    t.list = reinterpret_cast<uint32_t*>(p);
    int rc = launch_tsdf_clear(t, c->stream);
    if (rc == VSLAM_OK && hipStreamSynchronize(c->stream) != hipSuccess) { set_error("vslam_tsdf_create: clearing the pool failed"); rc = VSLAM_ERR_HIP; }
    if (rc) { vslam_tsdf_destroy(reinterpret_cast<vslam_tsdf_map*>(m)); return rc; }
    *out = reinterpret_cast<vslam_tsdf_map*>(m);
    return VSLAM_OK;
}

void vslam_tsdf_destroy(vslam_tsdf_map* tm) {
    TsdfMap* m = reinterpret_cast<TsdfMap*>(tm);
    if (!m) return;
    m->free();
    m->mesh.release();
    m->render.release();
    m->reint.release();
    m->dist.release();
    delete m;
}

int vslam_tsdf_clear(vslam_tsdf_map* tm) {
    TsdfMap* m = reinterpret_cast<TsdfMap*>(tm);
    if (!m) { set_error("vslam_tsdf_clear: null map"); return VSLAM_ERR_ARG; }
    VS_ENTER(m->ctx);
    m->epoch += 1;
    return launch_tsdf_clear(m->t, m->ctx->stream);
}

int vslam_tsdf_stats(vslam_tsdf_map* tm, struct vslam_tsdf_stats* host) {
    TsdfMap* m = reinterpret_cast<TsdfMap*>(tm);
    if (!m || !host || host->struct_size != (int32_t)sizeof(struct vslam_tsdf_stats)) { set_error("vslam_tsdf_stats: null argument or struct_size mismatch"); return VSLAM_ERR_ARG; }
    VS_ENTER(m->ctx);
    unsigned long long w[kTsdfCounters];
    if (int rc = read_counters(m->ctx, m->t.counters, w, kTsdfCounters)) return rc;
    host->n_blocks = w[0]; host->n_samples = w[1]; host->n_dropped_range = w[2]; host->n_dropped_full = w[3]; host->status = (uint32_t)w[4];
    host->n_frames_skipped = w[5]; host->n_pairs_visited = w[6]; host->n_pairs_kept = w[7];
    return VSLAM_OK;
}

int vslam_tsdf_integrate_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                             int w, int h, int B, const double* d_T_c_w, const int32_t* d_map_id, double z_min, double z_max, int step) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_integrate_dev");
    if (!m) return VSLAM_ERR_ARG;
    VoxelImages a;
    if (int rc = map_images(c, "vslam_tsdf_integrate_dev", d_disparity, d_gray, img_bytes, pitch, w, h, B, d_T_c_w, d_map_id, z_min, z_max, step, a)) return rc;
    VS_ENTER(c);
    m->epoch += 1;
    return launch_tsdf_integrate(m->t, a, d_gray, img_bytes, pitch, d_map_id, tsdf_form(c), c->stream);
}

int vslam_tsdf_reach_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, uint32_t* d_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_reach_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 4) { set_error("vslam_tsdf_reach_dev: d_out is null or not 4-byte aligned"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    // the block counter never exceeds 2^log2_blocks <= 2^22: its low word is the count
    VS_HIP(hipMemcpyAsync(d_out, m->t.counters, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return VSLAM_OK;
}

int vslam_tsdf_reintegrate_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                               int w, int h, int B, const double* d_T_old, const double* d_T_new, const int32_t* d_map_id,
                               const uint32_t* d_reach, double z_min, double z_max, int step) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_reintegrate_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (B == 0) return VSLAM_OK;
    if (!d_map_id || !d_T_old || !d_T_new || !d_reach) { set_error("vslam_tsdf_reintegrate_dev: null d_map_id, d_T_old, d_T_new or d_reach"); return VSLAM_ERR_ARG; }
    VoxelImages a;
    if (int rc = map_images(c, "vslam_tsdf_reintegrate_dev", d_disparity, d_gray, img_bytes, pitch, w, h, B, d_T_new, d_map_id, z_min, z_max, step, a)) return rc;
    VS_ENTER(c);
    m->epoch += 1;
    if (int rc = m->reint.reserve(tsdf_reint_table_bytes(m->t, c->p.max_batch), c->stream)) return rc;
    const TsdfReint r = tsdf_reint_tables(m->t, c->p.max_batch, m->reint.p, d_reach);
    return launch_tsdf_reintegrate(m->t, r, a, d_gray, img_bytes, pitch, d_T_old, d_map_id, tsdf_form(c), c->stream);
}

int vslam_tsdf_extract_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int min_weight, vslam_surfel* d_out, int32_t* d_map_out, size_t capacity,
                           uint64_t* d_n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_extract_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (int rc = counted_output_check("vslam_tsdf_extract_dev", d_n_out, capacity, d_out, "null d_out")) return rc;
    if (int rc = map_id_check("vslam_tsdf_extract_dev", map_id, -1)) return rc;
    VS_ENTER(c);
    return launch_tsdf_extract(m->t, map_id, min_weight, d_out, d_map_out, capacity, reinterpret_cast<unsigned long long*>(d_n_out), c->stream);
}

int vslam_tsdf_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int32_t* d_block_out, uint32_t* d_voxels_out, size_t capacity,
                          uint64_t* d_n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_blocks_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (int rc = counted_output_check("vslam_tsdf_blocks_dev", d_n_out, capacity, d_block_out && d_voxels_out, "a null output")) return rc;
    if (int rc = map_id_check("vslam_tsdf_blocks_dev", map_id, -1)) return rc;
    VS_ENTER(c);
    return launch_tsdf_blocks(m->t, map_id, d_block_out, d_voxels_out, capacity, reinterpret_cast<unsigned long long*>(d_n_out), c->stream);
}

int vslam_tsdf_mesh_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int min_weight, vslam_surfel* d_vertices, int32_t* d_vertex_map, size_t vertex_capacity,
                        vslam_triangle* d_triangles, size_t triangle_capacity, uint64_t* d_counts) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_mesh_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (!d_counts || (vertex_capacity > 0 && !d_vertices) || (triangle_capacity > 0 && !d_triangles)) {
        set_error("vslam_tsdf_mesh_dev: null d_counts, or a null output with a capacity"); return VSLAM_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d_vertices) % 16 || reinterpret_cast<uintptr_t>(d_vertex_map) % 4 || reinterpret_cast<uintptr_t>(d_triangles) % 4 ||
        reinterpret_cast<uintptr_t>(d_counts) % 8) {
        set_error("vslam_tsdf_mesh_dev: d_vertices must be 16-byte, d_counts 8-byte, d_vertex_map and d_triangles 4-byte aligned"); return VSLAM_ERR_ARG;
    }
    if (int rc = map_id_check("vslam_tsdf_mesh_dev", map_id, -1)) return rc;
    VS_ENTER(c);
    // the vertex-id table holds every block claimed so far: the count is read here, after everything queued before this call
    unsigned long long n_blocks = 0;
    if (int rc = read_counters(c, m->t.counters, &n_blocks, 1)) return rc;
    const size_t n_slots = (size_t)1 << m->t.log2_blocks, blocks = std::max<size_t>(std::min<size_t>((size_t)n_blocks, n_slots), 1);
    const size_t have = m->mesh.bytes >= n_slots * 4 ? (m->mesh.bytes - n_slots * 4) / (1536 * 4) : 0;
    if (have < blocks) {
        if (int rc = m->mesh.reserve((1536 * blocks + n_slots) * 4, c->stream)) return rc;
    }
    const size_t vid_blocks = (m->mesh.bytes - n_slots * 4) / (1536 * 4);
    uint32_t* pos_of_slot = reinterpret_cast<uint32_t*>(m->mesh.p);
    int32_t* vid = reinterpret_cast<int32_t*>(m->mesh.p + n_slots * 4);
    return launch_tsdf_mesh(m->t, vid, pos_of_slot, vid_blocks, map_id, min_weight, d_vertices, d_vertex_map, vertex_capacity, d_triangles, triangle_capacity,
                            reinterpret_cast<unsigned long long*>(d_counts), c->stream);
}

int vslam_tsdf_load_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const int32_t* d_block_ids, const uint32_t* d_voxels, size_t n) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_load_blocks_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (n > 0 && (!d_block_ids || !d_voxels)) { set_error("vslam_tsdf_load_blocks_dev: a null input with n > 0"); return VSLAM_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(d_block_ids) % 16 || reinterpret_cast<uintptr_t>(d_voxels) % 16) {
        set_error("vslam_tsdf_load_blocks_dev: d_block_ids and d_voxels must be 16-byte aligned"); return VSLAM_ERR_ARG;
    }
    VS_ENTER(c);
    m->epoch += 1;
    return launch_tsdf_load(m->t, d_block_ids, d_voxels, n, c->stream);
}

// Form of the render: 0 = every ray walks all K samples, 1 = tsdf_ray_range_kernel narrows each tile's sample range first;
// Tuning::tsdf_render_form overrides it (tests and tools/bench_tsdf.py run both)
constexpr int kTsdfRenderFormDefault = 1;
constexpr int kTsdfRenderMaxSamples = 8192;

int vslam_tsdf_render_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const struct vslam_tsdf_render_params* rp, int V, const double* d_T_c_w, const int32_t* d_map_id,
                          float* d_depth, float* d_attr, uint64_t* d_counts) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_render_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (!rp || rp->struct_size != (int32_t)sizeof(struct vslam_tsdf_render_params)) { set_error("vslam_tsdf_render_dev: null params or struct_size mismatch"); return VSLAM_ERR_ARG; }
    if (rp->w < 1 || rp->h < 1 || V < 0) { set_error("vslam_tsdf_render_dev: w %d, h %d below 1 or V %d below 0", rp->w, rp->h, V); return VSLAM_ERR_ARG; }
    if ((unsigned long long)V * (unsigned long long)rp->h * (unsigned long long)rp->w >= (1ull << 31)) {
        set_error("vslam_tsdf_render_dev: V * h * w = %d * %d * %d is not below 2^31", V, rp->h, rp->w); return VSLAM_ERR_ARG;
    }
    if (!std::isfinite(rp->fx) || !(rp->fx > 0) || !std::isfinite(rp->fy) || !(rp->fy > 0) || !std::isfinite(rp->cx) || !std::isfinite(rp->cy)) {
        set_error("vslam_tsdf_render_dev: camera (%g, %g, %g, %g) is not finite with positive focal lengths", rp->fx, rp->fy, rp->cx, rp->cy); return VSLAM_ERR_ARG;
    }
    if (!std::isfinite(rp->z_min) || !(rp->z_min > 0) || !std::isfinite(rp->z_max) || !(rp->z_max > rp->z_min)) {
        set_error("vslam_tsdf_render_dev: depth range (%g, %g) is not finite with 0 < z_min < z_max", rp->z_min, rp->z_max); return VSLAM_ERR_ARG;
    }
    if (!std::isfinite(rp->march) || !(rp->march >= 0.125 && rp->march <= 1.0)) { set_error("vslam_tsdf_render_dev: march %g outside [1/8, 1]", rp->march); return VSLAM_ERR_ARG; }
    // K: the smallest non-negative integer with z_min + (double)K * hs >= z_max
    const double hs = rp->march * (double)m->t.vs, guess = (rp->z_max - rp->z_min) / hs;
    long long K = guess < (double)(kTsdfRenderMaxSamples + 4) ? std::max<long long>((long long)std::floor(guess) - 2, 0) : kTsdfRenderMaxSamples + 1;
    while (K <= kTsdfRenderMaxSamples && !(rp->z_min + (double)K * hs >= rp->z_max)) ++K;
    if (K > kTsdfRenderMaxSamples) { set_error("vslam_tsdf_render_dev: (%g, %g) in steps of %g takes more than %d samples", rp->z_min, rp->z_max, hs, kTsdfRenderMaxSamples); return VSLAM_ERR_ARG; }
    if (V > 0 && (!d_T_c_w || !d_map_id || !d_depth)) { set_error("vslam_tsdf_render_dev: null d_T_c_w, d_map_id or d_depth with V > 0"); return VSLAM_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(d_attr) % 16 || reinterpret_cast<uintptr_t>(d_counts) % 8 || reinterpret_cast<uintptr_t>(d_depth) % 4) {
        set_error("vslam_tsdf_render_dev: d_attr must be 16-byte, d_counts 8-byte, d_depth 4-byte aligned"); return VSLAM_ERR_ARG;
    }
    if (V == 0) return VSLAM_OK;
    VS_ENTER(c);
    const int form = c->tune.tsdf_render_form >= 0 ? c->tune.tsdf_render_form : kTsdfRenderFormDefault;
    if (int rc = m->render.reserve(tsdf_render_table_bytes(V, rp->w, rp->h, form), c->stream)) return rc;
    TsdfRenderCall call;
    call.w = rp->w; call.h = rp->h; call.V = V; call.K = (int)K; call.min_weight = rp->min_weight;
    call.fx = rp->fx; call.fy = rp->fy; call.cx = rp->cx; call.cy = rp->cy; call.z_min = rp->z_min; call.hs = hs;
    call.d_T = d_T_c_w; call.d_map_id = d_map_id; call.d_depth = d_depth; call.d_attr = d_attr; call.d_counts = reinterpret_cast<unsigned long long*>(d_counts);
    return launch_tsdf_render(m->t, call, m->render.p, form, c->stream);
}

// Form of the distance layer's build: 0 = every voxel walks the site masks of the blocks around it, 1 = the separable transform in three passes
// (DESIGN.md 5.17); Tuning::tsdf_dist_form overrides it (tests and tools/bench_tsdf_distance.py run both)
constexpr int kTsdfDistFormDefault = 1;

int vslam_tsdf_distance_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const struct vslam_tsdf_distance_params* dp, uint64_t* d_counts) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_distance_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (!dp || dp->struct_size != (int32_t)sizeof(struct vslam_tsdf_distance_params)) { set_error("vslam_tsdf_distance_dev: null params or struct_size mismatch"); return VSLAM_ERR_ARG; }
    if (int rc = map_id_check("vslam_tsdf_distance_dev", dp->map_id, -1)) return rc;
    if (dp->radius_voxels < 1 || dp->radius_voxels > 16) { set_error("vslam_tsdf_distance_dev: radius_voxels %d outside [1, 16]", dp->radius_voxels); return VSLAM_ERR_ARG; }
    if (dp->log2_layer_blocks < 6 || dp->log2_layer_blocks > 24) { set_error("vslam_tsdf_distance_dev: log2_layer_blocks %d outside [6, 24]", dp->log2_layer_blocks); return VSLAM_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(d_counts) % 8) { set_error("vslam_tsdf_distance_dev: d_counts must be 8-byte aligned"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    m->dist_built = false; // (a build that fails below leaves no layer)
    if (int rc = m->dist.reserve(tsdf_dist_layer_bytes(dp->log2_layer_blocks), c->stream)) return rc;
    const TsdfLayer L = tsdf_dist_layer(m->dist.p, dp->log2_layer_blocks);
    const int form = c->tune.tsdf_dist_form >= 0 ? c->tune.tsdf_dist_form : kTsdfDistFormDefault;
    if (int rc = launch_tsdf_distance(m->t, L, dp->map_id, dp->min_weight, dp->radius_voxels, form, reinterpret_cast<unsigned long long*>(d_counts), c->stream)) return rc;
    m->dist_built = true; m->dist_epoch = m->epoch; m->dist_log2 = dp->log2_layer_blocks;
    return VSLAM_OK;
}

// the layer of a map for a reader, or a refusal when none was built or the map changed since
static int dist_layer_of(const TsdfMap* m, const char* who, TsdfLayer& L) {
    if (!m->dist_built || m->dist_epoch != m->epoch) { set_error("%s: distance layer not built or older than the map", who); return VSLAM_ERR_ARG; }
    L = tsdf_dist_layer(m->dist.p, m->dist_log2);
    return VSLAM_OK;
}

int vslam_tsdf_distance_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int32_t* d_block_out, uint16_t* d_cells_out, size_t capacity, uint64_t* d_n_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_distance_blocks_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (int rc = counted_output_check("vslam_tsdf_distance_blocks_dev", d_n_out, capacity, d_block_out && d_cells_out, "a null output")) return rc;
    if (int rc = map_id_check("vslam_tsdf_distance_blocks_dev", map_id, -1)) return rc;
    if (reinterpret_cast<uintptr_t>(d_block_out) % 16 || reinterpret_cast<uintptr_t>(d_cells_out) % 16 || reinterpret_cast<uintptr_t>(d_n_out) % 8) {
        set_error("vslam_tsdf_distance_blocks_dev: d_block_out and d_cells_out must be 16-byte, d_n_out 8-byte aligned"); return VSLAM_ERR_ARG;
    }
    TsdfLayer L;
    if (int rc = dist_layer_of(m, "vslam_tsdf_distance_blocks_dev", L)) return rc;
    VS_ENTER(c);
    return launch_tsdf_distance_blocks(L, map_id, d_block_out, d_cells_out, capacity, reinterpret_cast<unsigned long long*>(d_n_out), c->stream);
}

int vslam_tsdf_distance_query_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const double* d_xyz_w, const int32_t* d_map_id, size_t N, float* d_dist, uint8_t* d_class) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    TsdfMap* m = owned_by<TsdfMap>(c, tm, "vslam_tsdf_distance_query_dev");
    if (!m) return VSLAM_ERR_ARG;
    if (N > 0 && (!d_xyz_w || !d_map_id || !d_dist || !d_class)) { set_error("vslam_tsdf_distance_query_dev: a null pointer with N > 0"); return VSLAM_ERR_ARG; }
    if (reinterpret_cast<uintptr_t>(d_xyz_w) % 8 || reinterpret_cast<uintptr_t>(d_map_id) % 4 || reinterpret_cast<uintptr_t>(d_dist) % 4) {
        set_error("vslam_tsdf_distance_query_dev: d_xyz_w must be 8-byte, d_map_id and d_dist 4-byte aligned"); return VSLAM_ERR_ARG;
    }
    TsdfLayer L;
    if (int rc = dist_layer_of(m, "vslam_tsdf_distance_query_dev", L)) return rc;
    if (N == 0) return VSLAM_OK;
    VS_ENTER(c);
    return launch_tsdf_distance_query(m->t, L, d_xyz_w, d_map_id, N, d_dist, d_class, c->stream);
}

// ---------------------------------------------------------------------------------------------- place database
int vslam_place_create(vslam_ctx* ctx, int rows_per_entry, int capacity_entries, int with_geometry, vslam_place_db** out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !out) { set_error("vslam_place_create: null argument"); return VSLAM_ERR_ARG; }
    *out = nullptr;
    if (rows_per_entry < 1 || rows_per_entry > kMaxRows) { set_error("vslam_place_create: rows_per_entry %d outside 1..%d (the matcher's row limit)", rows_per_entry, kMaxRows); return VSLAM_ERR_ARG; }
    if (capacity_entries < 1) { set_error("vslam_place_create: capacity_entries %d must be >= 1", capacity_entries); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    PlaceDb* d = new PlaceDb(&c->dev_bytes);
    d->n_refused = 0;
    const size_t R = (size_t)rows_per_entry, Rs = (R + 31) & ~(size_t)31, cap = (size_t)capacity_entries;
    d->v = PlaceView{};
    d->v.rows = rows_per_entry; d->v.stride_rows = (int)Rs; d->v.capacity = capacity_entries; d->v.n_entries = 0;
    PlaceView& v = d->v;
    auto layout = [&](Layout& a) {
        v.desc = a.take<uint8_t>(cap * Rs * 32); v.n = a.take<int32_t>(cap); v.seq = a.take<int32_t>(cap); v.frame = a.take<int32_t>(cap);
        if (with_geometry) {
            v.xy = a.take<float2>(cap * R); v.xyz = a.take<float>(cap * R * 3); v.valid = a.take<uint8_t>(cap * R); v.qsel = a.take<int32_t>(cap * R);
            v.nqsel = a.take<int32_t>(cap);
        }
    };
    Layout m(nullptr);
    layout(m);
    if (int rc = d->alloc(c, m.off, "vslam_place_create")) { delete d; return rc; }
    Layout a(d->base);
    layout(a);
    *out = reinterpret_cast<vslam_place_db*>(d);
    return VSLAM_OK;
}

void vslam_place_destroy(vslam_place_db* db) {
    PlaceDb* d = reinterpret_cast<PlaceDb*>(db);
    if (!d) return;
    d->free();
    d->dst.release(); d->work.release();
    delete d;
}

int vslam_place_clear(vslam_place_db* db) {
    PlaceDb* d = reinterpret_cast<PlaceDb*>(db);
    if (!d) { set_error("vslam_place_clear: null database"); return VSLAM_ERR_ARG; }
    d->v.n_entries = 0; d->n_refused = 0;
    return VSLAM_OK;
}

int vslam_place_stats(vslam_place_db* db, struct vslam_place_stats* host) {
    PlaceDb* d = reinterpret_cast<PlaceDb*>(db);
    if (!d || !host || host->struct_size != (int32_t)sizeof(struct vslam_place_stats)) { set_error("vslam_place_stats: null argument or struct_size mismatch"); return VSLAM_ERR_ARG; }
    host->n_entries = d->v.n_entries; host->capacity = d->v.capacity; host->rows_per_entry = d->v.rows; host->with_geometry = d->v.xy ? 1 : 0;
    host->n_refused = d->n_refused;
    return VSLAM_OK;
}

int vslam_place_read_entry(vslam_place_db* db, int entry, int32_t* meta, uint8_t* desc, float* xy, float* xyz, uint8_t* valid, int32_t* qsel) {
    PlaceDb* d = reinterpret_cast<PlaceDb*>(db);
    if (!d || !meta) { set_error("vslam_place_read_entry: null database or meta"); return VSLAM_ERR_ARG; }
    if (entry < 0 || entry >= d->v.n_entries) { set_error("vslam_place_read_entry: entry %d is not among the %d entries held", entry, d->v.n_entries); return VSLAM_ERR_ARG; }
    Ctx* c = d->ctx;
    VS_ENTER(c);
    const PlaceView& v = d->v;
    const size_t e = (size_t)entry, R = (size_t)v.rows;
    hipStream_t st = c->stream;
    meta[3] = 0;
    VS_HIP(hipMemcpyAsync(&meta[0], v.n + e, 4, hipMemcpyDeviceToHost, st));
    VS_HIP(hipMemcpyAsync(&meta[1], v.seq + e, 4, hipMemcpyDeviceToHost, st));
    VS_HIP(hipMemcpyAsync(&meta[2], v.frame + e, 4, hipMemcpyDeviceToHost, st));
    if (desc) VS_HIP(hipMemcpyAsync(desc, v.desc + e * v.stride_rows * 32, R * 32, hipMemcpyDeviceToHost, st));
    if (v.xy) {
        VS_HIP(hipMemcpyAsync(&meta[3], v.nqsel + e, 4, hipMemcpyDeviceToHost, st));
        if (xy) VS_HIP(hipMemcpyAsync(xy, v.xy + e * R, R * 8, hipMemcpyDeviceToHost, st));
        if (xyz) VS_HIP(hipMemcpyAsync(xyz, v.xyz + e * R * 3, R * 12, hipMemcpyDeviceToHost, st));
        if (valid) VS_HIP(hipMemcpyAsync(valid, v.valid + e * R, R, hipMemcpyDeviceToHost, st));
        if (qsel) VS_HIP(hipMemcpyAsync(qsel, v.qsel + e * R, R * 4, hipMemcpyDeviceToHost, st));
    }
    VS_HIP(hipStreamSynchronize(st));
    return VSLAM_OK;
}

int vslam_place_read_meta(vslam_place_db* db, int first, int count, int32_t* n, int32_t* seq, int32_t* frame) {
    PlaceDb* d = reinterpret_cast<PlaceDb*>(db);
    if (!d) { set_error("vslam_place_read_meta: null database"); return VSLAM_ERR_ARG; }
    if (first < 0 || count < 0 || first > d->v.n_entries - count) { set_error("vslam_place_read_meta: entries [%d, %d + %d) are not among the %d held", first, first, count, d->v.n_entries); return VSLAM_ERR_ARG; }
    Ctx* c = d->ctx;
    VS_ENTER(c);
    if (count == 0) return VSLAM_OK;
    const size_t bytes = sizeof(int32_t) * (size_t)count;
    if (n) VS_HIP(hipMemcpyAsync(n, d->v.n + first, bytes, hipMemcpyDeviceToHost, c->stream));
    if (seq) VS_HIP(hipMemcpyAsync(seq, d->v.seq + first, bytes, hipMemcpyDeviceToHost, c->stream));
    if (frame) VS_HIP(hipMemcpyAsync(frame, d->v.frame + first, bytes, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}

// the query range of the score / select / verify entries
static int place_range(const PlaceDb* d, const char* who, int q0, int nq, int nq_max) {
    if (nq < 1 || nq > nq_max) { set_error("%s: nq %d outside 1..%d", who, nq, nq_max); return VSLAM_ERR_ARG; }
    if (q0 < 0 || q0 > d->v.n_entries - nq) { set_error("%s: queries [%d, %d + %d) are not among the %d entries held", who, q0, q0, nq, d->v.n_entries); return VSLAM_ERR_ARG; }
    return VSLAM_OK;
}

int vslam_place_add_dev(vslam_ctx* ctx, vslam_place_db* db, const uint8_t* d_desc, size_t desc_stride_bytes, const int32_t* d_n, const int32_t* d_add,
                        const int32_t* d_seq, const int32_t* d_frame, const vslam_keypoint* d_kps, const float* d_xyz, const uint8_t* d_valid, int kp_capacity,
                        int B, int* first_entry) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    PlaceDb* d = owned_by<PlaceDb>(c, db, "vslam_place_add_dev");
    if (!d) return VSLAM_ERR_ARG;
    if (!d_desc || !d_n || !d_seq || !d_frame) { set_error("vslam_place_add_dev: null d_desc, d_n, d_seq or d_frame"); return VSLAM_ERR_ARG; }
    if (B < 1) { set_error("vslam_place_add_dev: batch %d must be >= 1", B); return VSLAM_ERR_ARG; }
    if ((((uintptr_t)d_desc | (uintptr_t)desc_stride_bytes) & 15) != 0) { set_error("vslam_place_add_dev: d_desc and desc_stride_bytes must be multiples of 16 bytes"); return VSLAM_ERR_ARG; }
    if (d->v.xy && (!d_kps || !d_xyz || !d_valid || kp_capacity < 1)) { set_error("vslam_place_add_dev: a database with geometry needs d_kps, d_xyz, d_valid and kp_capacity >= 1"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    // which items are added, and where: decided on the host so that an add that does not fit adds nothing
    std::vector<int32_t> dst((size_t)B, 1);
    if (d_add) {
        VS_HIP(hipMemcpyAsync(dst.data(), d_add, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
        VS_HIP(hipStreamSynchronize(c->stream));
    }
    const int first = d->v.n_entries;
    long long n_add = 0;
    for (int b = 0; b < B; ++b) dst[b] = dst[b] != 0 ? first + (int)(n_add++) : -1;
    if (first_entry) *first_entry = first;
    if (n_add > (long long)d->v.capacity - first) {
        ++d->n_refused;
        set_error("vslam_place_add_dev: %lld entries do not fit (%d of %d held): nothing added", n_add, first, d->v.capacity);
        return VSLAM_ERR_CAPACITY;
    }
    if (n_add == 0) return VSLAM_OK;
    if (int rc = d->dst.reserve(sizeof(int32_t) * B, c->stream)) return rc;
    VS_HIP(hipMemcpyAsync(d->dst.p, dst.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));   // (dst is a local)
    if (int rc = launch_place_add(d->v, reinterpret_cast<const int32_t*>(d->dst.p), d_desc, desc_stride_bytes, d_n, d_seq, d_frame, d_kps, d_xyz, d_valid,
                                  kp_capacity, B, c->stream)) return rc;
    d->v.n_entries = first + (int)n_add;
    return VSLAM_OK;
}

int vslam_place_score_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, int tau, int min_gap, int32_t* d_score, int ld) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    PlaceDb* d = owned_by<PlaceDb>(c, db, "vslam_place_score_dev");
    if (!d) return VSLAM_ERR_ARG;
    if (!d_score) { set_error("vslam_place_score_dev: null d_score"); return VSLAM_ERR_ARG; }
    if (int rc = place_range(d, "vslam_place_score_dev", q0, nq, 65535)) return rc;
    if (tau < 0 || tau > 255) { set_error("vslam_place_score_dev: tau %d outside [0, 255]", tau); return VSLAM_ERR_ARG; }
    if (ld < d->v.n_entries) { set_error("vslam_place_score_dev: ld %d is below the %d entries held", ld, d->v.n_entries); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_place_score(d->v, q0, nq, tau, min_gap, d_score, ld, c->stream);
}

int vslam_place_select_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, const int32_t* d_score, int ld, int K, int min_score, int32_t* d_cand,
                           int32_t* d_cand_score) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    PlaceDb* d = owned_by<PlaceDb>(c, db, "vslam_place_select_dev");
    if (!d) return VSLAM_ERR_ARG;
    if (!d_score || !d_cand || !d_cand_score) { set_error("vslam_place_select_dev: null d_score, d_cand or d_cand_score"); return VSLAM_ERR_ARG; }
    if (int rc = place_range(d, "vslam_place_select_dev", q0, nq, 1 << 30)) return rc;
    if (K < 1 || K > 8) { set_error("vslam_place_select_dev: K %d outside 1..8", K); return VSLAM_ERR_ARG; }
    if (ld < d->v.n_entries) { set_error("vslam_place_select_dev: ld %d is below the %d entries held", ld, d->v.n_entries); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    return launch_place_select(d->v, nq, d_score, ld, K, min_score, d_cand, d_cand_score, c->stream);
}

int vslam_place_verify_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, const int32_t* d_cand, int K, int rank, int min_inliers, double* d_T_q_c,
                           int32_t* d_n_matches, int32_t* d_n_inliers) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    PlaceDb* d = owned_by<PlaceDb>(c, db, "vslam_place_verify_dev");
    if (!d) return VSLAM_ERR_ARG;
    if (!d_cand || !d_T_q_c || !d_n_matches || !d_n_inliers) { set_error("vslam_place_verify_dev: null d_cand, d_T_q_c, d_n_matches or d_n_inliers"); return VSLAM_ERR_ARG; }
    if (!d->v.xy) { set_error("vslam_place_verify_dev: the database was created without geometry"); return VSLAM_ERR_ARG; }
    if (int rc = place_range(d, "vslam_place_verify_dev", q0, nq, c->p.max_batch)) return rc;
    if (K < 1 || K > 8 || rank < 0 || rank >= K) { set_error("vslam_place_verify_dev: K %d outside 1..8 or rank %d outside [0, K)", K, rank); return VSLAM_ERR_ARG; }
    if (min_inliers < 0) { set_error("vslam_place_verify_dev: min_inliers %d must be >= 0", min_inliers); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    const PlaceView& v = d->v;
    const size_t R = (size_t)v.rows, n = (size_t)nq;
    int32_t *d_qitem, *d_nm, *d_np; double* d_gap; vslam_dmatch* d_m; float *d_xyz, *d_uv;
    if (int rc = carve(d->work, c->stream, [&](Layout& a) {
            d_qitem = a.take<int32_t>(n); d_nm = a.take<int32_t>(n); d_np = a.take<int32_t>(n); d_gap = a.take<double>(n);
            d_m = a.take<vslam_dmatch>(n * R); d_xyz = a.take<float>(n * R * 3); d_uv = a.take<float>(n * R * 2);
        })) return rc;
    if (int rc = launch_place_verify_prep(v, nq, d_cand, K, rank, d_qitem, d_gap, c->stream)) return rc;
    const size_t stride = (size_t)v.stride_rows * 32;
    if (int rc = vslam_feature_matching_pairs_dev(ctx, v.desc, stride, v.n, v.qsel, v.nqsel, v.rows, d_qitem, v.n_entries, v.desc + (size_t)q0 * stride, stride,
                                                  v.n + q0, d_gap, 1, nq, v.rows, d_m, v.rows, d_nm)) return rc;
    if (int rc = launch_place_gather(v, q0, nq, d_qitem, d_m, d_nm, min_inliers, d_xyz, d_uv, d_np, d_n_matches, c->stream)) return rc;
    return vslam_pnp_ransac_dev(ctx, d_xyz, d_uv, d_np, v.rows, nq, d_T_q_c, 100, c->p.pnp_reproj_thr, 0.99, nullptr, d_n_inliers, nullptr);
}

// ---------------------------------------------------------------------------------------------- pose graph
void vslam_pose_graph_default_params(vslam_pose_graph_params* p) { solver_default_params(p); }

// (the checks on the structs come before the one on the context: they need no device)
int vslam_pose_graph_dev(vslam_ctx* ctx, const vslam_pose_graph* graph, const vslam_pose_graph_params* params, double* d_T_out,
                         vslam_pose_graph_stats* d_stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!graph) { set_error("vslam_pose_graph_dev: null graph"); return VSLAM_ERR_ARG; }
    if (graph->struct_size != (int32_t)sizeof(vslam_pose_graph)) { set_error("vslam_pose_graph_dev: vslam_pose_graph struct_size %d, the library has %d", graph->struct_size, (int)sizeof(vslam_pose_graph)); return VSLAM_ERR_ARG; }
    vslam_pose_graph_params p;
    if (int rc = solver_params("vslam_pose_graph_dev", "vslam_pose_graph_params", params, p)) return rc;
    if (graph->n_graphs < 0 || graph->total_nodes < 0 || graph->total_edges < 0) { set_error("vslam_pose_graph_dev: negative count (n_graphs %d, total_nodes %d, total_edges %d)", graph->n_graphs, graph->total_nodes, graph->total_edges); return VSLAM_ERR_ARG; }
    if (!graph->d_node_off || !graph->d_edge_off) { set_error("vslam_pose_graph_dev: null d_node_off or d_edge_off"); return VSLAM_ERR_ARG; }
    if (graph->total_nodes > 0 && (!graph->d_T || !d_T_out)) { set_error("vslam_pose_graph_dev: null d_T or d_T_out"); return VSLAM_ERR_ARG; }
    if (graph->total_edges > 0 && (!graph->d_edge_i || !graph->d_edge_j || !graph->d_edge_Z || !graph->d_edge_w)) { set_error("vslam_pose_graph_dev: null d_edge_i, d_edge_j, d_edge_Z or d_edge_w"); return VSLAM_ERR_ARG; }
    if (!c) { set_error("vslam_pose_graph_dev: null context"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    if (int rc = launch_pose_graph(*graph, p, c->tune.pg_precond, d_T_out, d_stats, c->pgraph, c->stream)) return rc;
    c->pgraph_n = graph->n_graphs;
    return VSLAM_OK;
}

int vslam_pose_graph_status_dev(vslam_ctx* ctx, int n_graphs, int32_t* h_status) {
    return solver_status(reinterpret_cast<Ctx*>(ctx), "vslam_pose_graph_status_dev", "graphs", "vslam_pose_graph_dev", &Ctx::pgraph, &Ctx::pgraph_n, n_graphs, h_status);
}

// ---------------------------------------------------------------------------------------------- full bundle adjustment
void vslam_full_ba_default_params(vslam_full_ba_params* p) { solver_default_params(p); }

// (the checks on the structs come before the one on the context: they need no device)
int vslam_full_ba_dev(vslam_ctx* ctx, const vslam_full_ba* ba, const vslam_full_ba_params* params, double* d_T_out, double* d_xyz_out,
                      vslam_full_ba_stats* d_stats) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!ba) { set_error("vslam_full_ba_dev: null problem"); return VSLAM_ERR_ARG; }
    if (ba->struct_size != (int32_t)sizeof(vslam_full_ba)) { set_error("vslam_full_ba_dev: vslam_full_ba struct_size %d, the library has %d", ba->struct_size, (int)sizeof(vslam_full_ba)); return VSLAM_ERR_ARG; }
    vslam_full_ba_params p;
    if (int rc = solver_params("vslam_full_ba_dev", "vslam_full_ba_params", params, p)) return rc;
    const double big = 1.7976931348623157e308;
    if (!(ba->K4[0] > 0) || !(ba->K4[0] <= big) || !(ba->K4[1] > 0) || !(ba->K4[1] <= big) || !(fabs(ba->K4[2]) <= big) || !(fabs(ba->K4[3]) <= big) || !(ba->bf >= 0) ||
        !(ba->bf <= big) || !(ba->huber_delta >= 0) || !(ba->huber_delta <= big)) {
        set_error("vslam_full_ba_dev: camera out of range (fx, fy > 0, cx, cy finite, bf >= 0, huber_delta >= 0, all finite)");
        return VSLAM_ERR_ARG;
    }
    if (ba->n_problems < 0 || ba->total_kfs < 0 || ba->total_lms < 0 || ba->total_obs < 0 || ba->total_edges < 0) {
        set_error("vslam_full_ba_dev: negative count (n_problems %d, total_kfs %d, total_lms %d, total_obs %d, total_edges %d)", ba->n_problems, ba->total_kfs, ba->total_lms, ba->total_obs, ba->total_edges);
        return VSLAM_ERR_ARG;
    }
    if (!ba->d_kf_off || !ba->d_lm_off || !ba->d_obs_off || !ba->d_edge_off) { set_error("vslam_full_ba_dev: null d_kf_off, d_lm_off, d_obs_off or d_edge_off"); return VSLAM_ERR_ARG; }
    if (ba->total_kfs > 0 && (!ba->d_T || !d_T_out)) { set_error("vslam_full_ba_dev: null d_T or d_T_out"); return VSLAM_ERR_ARG; }
    if (ba->total_lms > 0 && (!ba->d_xyz || !d_xyz_out)) { set_error("vslam_full_ba_dev: null d_xyz or d_xyz_out"); return VSLAM_ERR_ARG; }
    if (ba->total_obs > 0 && (!ba->d_obs_kf || !ba->d_obs_lm || !ba->d_obs_uv)) { set_error("vslam_full_ba_dev: null d_obs_kf, d_obs_lm or d_obs_uv"); return VSLAM_ERR_ARG; }
    if (ba->total_edges > 0 && (!ba->d_edge_i || !ba->d_edge_j || !ba->d_edge_Z || !ba->d_edge_w)) { set_error("vslam_full_ba_dev: null d_edge_i, d_edge_j, d_edge_Z or d_edge_w"); return VSLAM_ERR_ARG; }
    if (!c) { set_error("vslam_full_ba_dev: null context"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    // the library's choice (profiles/full_ba.json): stored observations
    const int store = c->tune.fba_store >= 0 ? c->tune.fba_store : 1;
    if (int rc = launch_full_ba(*ba, p, store, d_T_out, d_xyz_out, d_stats, c->fullba, c->stream)) return rc;
    c->fullba_n = ba->n_problems;
    return VSLAM_OK;
}

int vslam_full_ba_status_dev(vslam_ctx* ctx, int n_problems, int32_t* h_status) {
    return solver_status(reinterpret_cast<Ctx*>(ctx), "vslam_full_ba_status_dev", "problems", "vslam_full_ba_dev", &Ctx::fullba, &Ctx::fullba_n, n_problems, h_status);
}

// ---------------------------------------------------------------------------------------------- match by projection
void vslam_project_match_default_params(vslam_project_match_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(vslam_project_match_params);
    p->radius_px = 15.f; p->tau = 50; p->ratio_pct = 80; p->z_min = 0.1; p->z_max = 1e4;
}

// (the checks on the structs come before the one on the context: they need no device)
int vslam_project_match_dev(vslam_ctx* ctx, const vslam_project_match* in, const vslam_project_match_params* params) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    const char* me = "vslam_project_match_dev";
    if (!in) { set_error("%s: null batch", me); return VSLAM_ERR_ARG; }
    if (in->struct_size != (int32_t)sizeof(vslam_project_match)) { set_error("%s: vslam_project_match struct_size %d, the library has %d", me, in->struct_size, (int)sizeof(vslam_project_match)); return VSLAM_ERR_ARG; }
    vslam_project_match_params p;
    vslam_project_match_default_params(&p);
    if (params) {
        if (params->struct_size != (int32_t)sizeof(vslam_project_match_params)) { set_error("%s: vslam_project_match_params struct_size %d, the library has %d", me, params->struct_size, (int)sizeof(vslam_project_match_params)); return VSLAM_ERR_ARG; }
        p = *params;
    }
    if (!(p.radius_px > 0.f) || !std::isfinite(p.radius_px)) { set_error("%s: radius_px %g is not positive and finite", me, (double)p.radius_px); return VSLAM_ERR_ARG; }
    if (p.tau < 0 || p.tau > 255) { set_error("%s: tau %d outside [0, 255]", me, p.tau); return VSLAM_ERR_ARG; }
    if (p.ratio_pct < 0 || p.ratio_pct > 100) { set_error("%s: ratio_pct %d outside [0, 100]", me, p.ratio_pct); return VSLAM_ERR_ARG; }
    if (p.z_min != p.z_min || p.z_max != p.z_max) { set_error("%s: a NaN depth gate", me); return VSLAM_ERR_ARG; }
    if (in->n_items < 1 || in->B < 1 || in->n_landmarks < 0 || in->n_src_rows < 0) {
        set_error("%s: counts out of range (n_items %d and B %d >= 1, n_landmarks %d and n_src_rows %d >= 0)", me, in->n_items, in->B, in->n_landmarks, in->n_src_rows);
        return VSLAM_ERR_ARG;
    }
    if (in->kp_capacity < 1 || in->kp_capacity > VSLAM_PROJECT_MATCH_MAX_KP) {
        set_error("%s: kp_capacity %d outside [1, %d] (the keypoint grid, pixels, lists and claims of an image live in LDS)", me, in->kp_capacity, VSLAM_PROJECT_MATCH_MAX_KP);
        return VSLAM_ERR_ARG;
    }
    if (!in->d_lm_off || !in->d_item_img || !in->d_item_T || !in->d_kps || !in->d_desc || !in->d_n) { set_error("%s: null d_lm_off, d_item_img, d_item_T, d_kps, d_desc or d_n", me); return VSLAM_ERR_ARG; }
    if (in->n_landmarks > 0 && (!in->d_lm_xyz || !in->d_lm_desc_row || !in->d_src_desc || !in->d_match || !in->d_dist || !in->d_status)) {
        set_error("%s: null d_lm_xyz, d_lm_desc_row, d_src_desc, d_match, d_dist or d_status", me);
        return VSLAM_ERR_ARG;
    }
    if (((uintptr_t)in->d_src_desc & 15) || ((uintptr_t)in->d_desc & 15)) { set_error("%s: d_src_desc and d_desc must be 16-byte aligned", me); return VSLAM_ERR_ARG; }
    if (in->desc_stride_bytes && ((in->desc_stride_bytes & 15) || in->desc_stride_bytes < (size_t)in->kp_capacity * 32)) {
        set_error("%s: desc_stride_bytes %zu is no multiple of 16 or below kp_capacity x 32 = %zu", me, in->desc_stride_bytes, (size_t)in->kp_capacity * 32);
        return VSLAM_ERR_ARG;
    }
    if (in->K4) {
        const double big = 1.7976931348623157e308;
        if (!(in->K4[0] > 0) || !(in->K4[0] <= big) || !(in->K4[1] > 0) || !(in->K4[1] <= big) || !(fabs(in->K4[2]) <= big) || !(fabs(in->K4[3]) <= big)) {
            set_error("%s: camera out of range (fx, fy > 0, all finite)", me);
            return VSLAM_ERR_ARG;
        }
    }
    if (!c) { set_error("%s: null context", me); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    double K[4];
    if (in->K4) memcpy(K, in->K4, sizeof(K)); else fill_K(c, K);
    const int stage = c->tune.pm_stage >= 0 ? c->tune.pm_stage : 0;
    return launch_project_match(*in, p, K, c->p.img_w, c->p.img_h, stage, c->stream);
}

// float4 streaming copy of `bytes` (src -> dst, both allocated here), `reps` timed launches after one warm-up, hipEvents on the
// context stream: *gbs_out = (bytes read + bytes written) / time.  The achievable-HBM figure bench.py reports next to the spec peak.
int vslam_hbm_copy_probe_variants(void) { return hbm_copy_probe_variants(); }

int vslam_hbm_copy_probe_variant(vslam_ctx* ctx, size_t bytes, int reps, int variant, double* gbs_out, char* name_out) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !gbs_out || bytes < (1u << 20) || reps <= 0 || variant < 0 || variant >= hbm_copy_probe_variants()) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    VS_ENTER(c);
    bytes &= ~(size_t)15;
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = VSLAM_OK;
    float ms = 0.f;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        set_error("copy probe: allocation failed"); rc = VSLAM_ERR_HIP;
    } else {
        (void)hipMemsetAsync(a, 1, bytes, c->stream);
        rc = launch_hbm_copy_probe(a, b, bytes, variant, c->stream);
        (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps && rc == VSLAM_OK; ++r) rc = launch_hbm_copy_probe(a, b, bytes, variant, c->stream);
        (void)hipEventRecord(e1, c->stream);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { set_error("copy probe: timing failed"); rc = VSLAM_ERR_HIP; }
    }
    if (rc == VSLAM_OK) *gbs_out = 2.0 * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;
    if (rc == VSLAM_OK && name_out) { strncpy(name_out, hbm_copy_probe_name(variant), 63); name_out[63] = 0; }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    return rc;
}

int vslam_hbm_copy_probe(vslam_ctx* ctx, size_t bytes, int reps, double* gbs_out) { // best of the variants
    if (!gbs_out) { set_error("bad argument"); return VSLAM_ERR_ARG; }
    double best = 0.0;
    for (int v = 0; v < hbm_copy_probe_variants(); ++v) {
        double g = 0.0;
        const int rc = vslam_hbm_copy_probe_variant(ctx, bytes, reps, v, &g, nullptr);
        if (rc != VSLAM_OK) return rc;
        if (g > best) best = g;
    }
    *gbs_out = best;
    return VSLAM_OK;
}

// ---------------------------------------------------------------------------------------------- raw device memory helpers
// (for hosts that do not bring their own allocator; bench.py uses torch tensors instead)
int vslam_dev_alloc(void** p, size_t bytes) { if (!p) return VSLAM_ERR_ARG; VS_HIP(hipMalloc(p, bytes)); return VSLAM_OK; }
int vslam_dev_free(void* p) { if (p) VS_HIP(hipFree(p)); return VSLAM_OK; }
int vslam_dev_upload(vslam_ctx* ctx, void* d, const void* h, size_t bytes) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    VS_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}
int vslam_dev_download(vslam_ctx* ctx, void* h, const void* d, size_t bytes) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    VS_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    VS_HIP(hipStreamSynchronize(c->stream));
    return VSLAM_OK;
}
int vslam_dev_memset(vslam_ctx* ctx, void* d, int value, size_t bytes) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return VSLAM_ERR_ARG;
    VS_ENTER(c);
    VS_HIP(hipMemsetAsync(d, value, bytes, c->stream));
    return VSLAM_OK;
}

} // extern "C"
