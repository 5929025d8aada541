/*
 * vslam_hip.h -- C-ABI of libvslam_hip.so: the MI355X (gfx950) build of the stereo-VO hot path of
 * shangzhouye/stereo-visual-slam (front-end ORB/ANMS/rBRIEF, cross-checked Hamming matching, stereo
 * triangulation, motion-only pose refinement, 10-keyframe local bundle adjustment).
 *
 * The reference has no FFI/plugin layer: its seam is the public C++ surface of visual_odometry.hpp,
 * optimization.hpp and map.hpp.  Each entry point below replaces the arithmetic behind
 * ONE reference method; `file:line` citations are into /root/reference.  The C++ host mirror that keeps the
 * reference's method names on top of this ABI lives in stereo-visual-slam_amd/host/ (see INTEGRATION.md for the
 * binding a maintainer of the reference would add).
 *
 * Conventions
 *   - plain pointers and sizes, POD structs, no C++/torch types; every call returns an int status
 *     (0 = ok, <0 = error, never throws, never reads out of bounds on bad indices -- quirk Q7);
 *   - `vslam_*`      : HOST buffers in/out, synchronous, one call per reference method (drop-in granularity);
 *   - `vslam_*_dev`  : DEVICE-resident, batched over B independent items (stereo pairs / frames / windows),
 *                      asynchronous on the context's stream -- the throughput path bench.py measures;
 *   - SE3 poses are 7 doubles: unit quaternion (x,y,z,w) then translation (Sophus::SE3d memory order);
 *   - camera = {fx, fy, cx, cy, baseline}; K4 = {fx, fy, cx, cy}.
 *   - a context is thread-compatible, not thread-safe; one context per GPU per thread.
 */
#ifndef VSLAM_HIP_H
#define VSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_OK 0
#define VSLAM_ERR_ARG (-1)       /* null pointer / bad size / index out of range */
#define VSLAM_ERR_HIP (-2)       /* a HIP runtime call failed; see vslam_last_error() */
#define VSLAM_ERR_CAPACITY (-3)  /* an internal or caller capacity was exceeded (results truncated) */
#define VSLAM_ERR_NO_DEVICE (-4) /* no gfx950-class GPU visible */

/* ABI revision of this header.  Bumped whenever a struct grows or a signature changes position-wise (revision 2 inserted K4 into
 * vslam_local_ba / vslam_pose_only_window; revision 3 added struct_size / abi_version to vslam_params and the alignment contract
 * of vslam_feature_matching_dev; revision 4 appended d_n_kf to vslam_ba_batch and added vslam_build_windows_dev, vslam_pnp_ransac_dev,
 * vslam_set_tuning, vslam_sgbm_status_dev).  vslam_create refuses a vslam_params whose struct_size / abi_version do not match the library's,
 * so a caller compiled against an older header fails with VSLAM_ERR_ARG instead of having its arguments reinterpreted. */
#define VSLAM_ABI_VERSION 5

#define VSLAM_ORB_NLEVELS 8
#define VSLAM_MAX_KF 12          /* keyframes per optimisation window (reference: Map::num_keyframes_ = 10, map.hpp:22) */
#define VSLAM_LM_MAX_ITERS 32

/* layout-compatible with cv::KeyPoint (28 B) -- types_def.hpp:23 `cv::KeyPoint keypoint_` */
typedef struct vslam_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} vslam_keypoint;

/* layout-compatible with cv::DMatch (16 B) -- visual_odometry.hpp:117 */
typedef struct vslam_dmatch {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} vslam_dmatch;

/* every hard-coded constant of the reference's hot path (SURVEY.md section 5 "Config / flags") */
typedef struct vslam_params {
    int32_t img_w, img_h;          /* 1241 x 376 (KITTI-00)                                         */
    int32_t max_batch;             /* largest B the context is sized for                            */
    int32_t orb_nfeatures;         /* 3000  visual_odometry.cpp:22                                  */
    int32_t anms_num;              /* 500   visual_odometry.cpp:82 (BASELINE config 2 uses 1500)    */
    int32_t fast_threshold;        /* 20    cv::ORB default                                         */
    int32_t kp_capacity;           /* per-image capacity of keypoint/descriptor outputs (>= 4096)   */
    double cam[5];                 /* fx fy cx cy b: 718.856 718.856 607.1928 185.2157 0.573  types_def.hpp:53-54 */
    double depth_min, depth_max;   /* 10, 400   visual_odometry.cpp:194                             */
    double depth_reliable;         /* 40        visual_odometry.cpp:201                             */
    double match_ratio;            /* 2.0       visual_odometry.cpp:242                             */
    double match_gap_thr;          /* 30.0      visual_odometry.cpp:242                             */
    double huber_delta;            /* 5.991     optimization.cpp:154,205                            */
    double pnp_reproj_thr;         /* 4.0 px    visual_odometry.cpp:277                             */
    double stereo_row_tol;         /* 2.0 px    epipolar gate of the L/R-match depth stage (vslam_triangulate*): a pair is kept
                                      only if |vL - vR| <= tol and uL > uR; < 0 = off.  No counterpart in the reference, whose
                                      depth is SGBM (row-constrained by construction, visual_odometry.cpp:159-174)         */
    int32_t struct_size;           /* sizeof(vslam_params) of the caller's header; set by vslam_default_params, checked by vslam_create */
    int32_t abi_version;           /* VSLAM_ABI_VERSION of the caller's header; likewise                                  */
} vslam_params;

typedef struct vslam_lm_stats {
    int32_t iterations, total_trials;
    double chi2_init, chi2_final, lambda_final;
    double chi2_iter[VSLAM_LM_MAX_ITERS];
    double lambda_iter[VSLAM_LM_MAX_ITERS];
    int32_t trials_iter[VSLAM_LM_MAX_ITERS];
} vslam_lm_stats;

typedef struct vslam_ctx vslam_ctx;

/* ------------------------------------------------------------------ context --------------------------- */
void vslam_default_params(vslam_params* p);
/* stream: a hipStream_t (as void*) to run on, or NULL to create a private one.  img_w, img_h in [64, 4095]; a context with a smaller image (each side
 * >= 2) serves the rectification stage and the entry points that take no context-sized image, and its ORB entry points return VSLAM_ERR_ARG. */
int vslam_create(const vslam_params* p, int device, void* stream, vslam_ctx** out);
void vslam_destroy(vslam_ctx* ctx);
const char* vslam_last_error(void);
const char* vslam_version(void);
int vslam_abi_version(void);       /* VSLAM_ABI_VERSION the library was built with */
int vslam_sync(vslam_ctx* ctx);
/* bytes of device memory the context holds */
size_t vslam_device_bytes(const vslam_ctx* ctx);
/* name of the GPU kernel families, for profiling cross-reference (NUL separated list not needed: static string) */
const char* vslam_kernel_names(void);

/* ------------------------------------------------------------------ rectification: raw pairs -> rectified pairs --- */
/* Every stage below assumes a rectified, undistorted stereo pair (SGBM searches along the row, the L/R matcher gates on |vL - vR|, vslam_triangulate
 * is the rectified-stereo DLT, find_3d is z = fx b / d).  The reference can assume it because KITTI odometry ships rectified images
 * and it reads them as they are; a rig that is not KITTI delivers raw images.  This stage has no counterpart in the
 * reference: it is the published arithmetic of OpenCV's initUndistortRectifyMap(K, D, R, P, size, CV_16SC2) followed by
 * remap(INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit gray images, restated -- PARITY UNPINNED like the rest of the tree (no OpenCV to compare with;
 * the tests' yardstick is the numpy restatement tests/rectify_ref.py).  Additive: vslam_params and the ABI version are unchanged.
 * Map, per camera and destination pixel (x, y), in double:
 *   P3 = [[fx', 0, cx'], [0, fy', cy'], [0, 0, 1]], M = (P3 R)^-1, (X, Y, W) = M (x, y, 1), xn = X / W, yn = Y / W, r2 = xn^2 + yn^2,
 *   kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
 *   xd = xn kr + 2 p1 xn yn + p2 (r2 + 2 xn^2), yd = yn kr + p1 (r2 + 2 yn^2) + 2 p2 xn yn, u = fx xd + cx, v = fy yd + cy,
 *   iu = rint(32 u), iv = rint(32 v) (half to even; clipped to +-2^40 first), sx = iu >> 5 (arithmetic), ax = iu & 31, likewise sy, ay;
 *   sx, sy saturate to int16; a non-finite u or v makes the entry "outside": sx = sy = -32768, ax = ay = 0.
 *   Stored as xy (h x w x 2 int16: sx, sy) and frac (h x w uint16: ay * 32 + ax) -- the CV_16SC2 + CV_16UC1 pair.
 * Remap: dst(x, y) = (w00 S(sx, sy) + w10 S(sx + 1, sy) + w01 S(sx, sy + 1) + w11 S(sx + 1, sy + 1) + 512) >> 10 with w00 = (32 - ax)(32 - ay),
 *   w10 = ax (32 - ay), w01 = (32 - ax) ay, w11 = ax ay; S reads 0 for any tap outside [0, src_w) x [0, src_h), per tap; integers throughout. */
typedef struct vslam_rectify_cam {
    double K[4];                   /* fx fy cx cy of the RAW camera                                                          */
    double D[8];                   /* k1 k2 p1 p2 k3 k4 k5 k6: OpenCV's order of the rational distortion model (zeros = none) */
    double R[9];                   /* rectifying rotation, row-major (cv::stereoRectify's R1 / R2); identity = undistort only */
    double P[4];                   /* fx' fy' cx' cy' of the RECTIFIED camera (the left 3 x 3 of P1 / P2)                     */
} vslam_rectify_cam;
typedef struct vslam_rectify_params {
    int32_t src_w, src_h;          /* raw image size, each in [2, 4096]                                                       */
    vslam_rectify_cam cam[2];      /* 0 = left, 1 = right                                                                     */
    int32_t struct_size;           /* sizeof(vslam_rectify_params) of the caller's header; set by vslam_default_rectify_params, checked */
} vslam_rectify_params;

/* the identity rig at the KITTI camera and 1241 x 376: D = 0, R = I, P = K = vslam_default_params' cam -- its map is the identity */
void vslam_default_rectify_params(vslam_rectify_params* p);

/* Is the rig admissible for dst_w x dst_h rectified images?  Host arithmetic only: no context, no GPU.  VSLAM_OK, or VSLAM_ERR_ARG with
 * vslam_last_error() naming the offending field: struct_size mismatch; src_w, src_h, dst_w or dst_h outside [2, 4096]; a non-finite entry
 * anywhere; fx, fy, fx' or fy' <= 0; R not a rotation (max |R R^T - I| > 1e-6 or det R <= 0). */
int vslam_rectify_params_check(const vslam_rectify_params* p, int dst_w, int dst_h);

/* The map of camera `cam` (0 | 1) for dst_w x dst_h rectified images, in host memory: xy dst_h x dst_w x 2 int16, frac dst_h x dst_w uint16, tightly
 * packed.  Host arithmetic in double, no context, no GPU; vslam_rectify_params_check runs first.  Once per rig: not a hot path. */
int vslam_rectify_build_maps(const vslam_rectify_params* p, int cam, int dst_w, int dst_h, int16_t* xy, uint16_t* frac);

/* Check, build both maps for the context's img_w x img_h and upload them.  The two maps are context state (8 bytes per destination pixel and
 * camera, counted by vslam_device_bytes, not part of the growable scratch).  A refused rig launches nothing and leaves maps already set in place.
 * Synchronises the context stream (a launch may still read the maps it replaces). */
int vslam_rectify_set(vslam_ctx* ctx, const vslam_rectify_params* p);

/* A caller's own maps for camera `cam` (e.g. cv::initUndistortRectifyMap's CV_16SC2 output for another lens model): xy img_h x img_w x 2 int16, frac
 * img_h x img_w uint16 (< 1024), host memory, for src_w x src_h raw images (each in [2, 4096]).  Any int16 coordinates are valid (taps outside the
 * source read 0).  Refused with VSLAM_ERR_ARG: cam outside 0 | 1, a null pointer, a source size out of range, a frac entry >= 1024. */
int vslam_rectify_set_maps(vslam_ctx* ctx, int cam, const int16_t* xy, const uint16_t* frac, int src_w, int src_h);

/* One raw image of camera `cam` (host, src_h rows of src_stride bytes) -> the rectified image (host, img_h rows of dst_stride bytes, img_w bytes
 * written per row).  Synchronous; the same kernel as the batched call.  VSLAM_ERR_ARG before that camera's map is set. */
int vslam_rectify(vslam_ctx* ctx, int cam, const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride);

/* Batched, device-resident: B raw pairs, image b of a side at d_src_* + b * src_img_bytes (src_h rows of src_pitch bytes), to B rectified pairs at
 * d_dst_* + b * dst_img_bytes (img_h rows of dst_pitch bytes; the padding bytes from img_w to dst_pitch are written as 0, so the output can go
 * straight into vslam_feature_detection_dev / vslam_disparity_map_dev).  Either side's pair of pointers may be NULL: that camera is skipped.
 * One launch for both sides; asynchronous on the context stream.  A lane applies its decoded map entries to a group of images of the batch, so
 * the cost per image falls with B up to a few groups per CU.  Destinations whose base, dst_pitch and dst_img_bytes are multiples of 4 are written
 * with dword stores, anything else byte by byte (same result, slower).
 * Refused with VSLAM_ERR_ARG: a side given before its map is set, both sides NULL, one pointer of a side NULL and the other not, B < 1 or
 * B > max_batch, src_pitch < src_w, dst_pitch < img_w, src_img_bytes < src_pitch x src_h (or >= 4 GiB), dst_img_bytes < dst_pitch x img_h. */
int vslam_rectify_dev(vslam_ctx* ctx, const uint8_t* d_src_left, const uint8_t* d_src_right, size_t src_img_bytes, int src_pitch, int B,
                      uint8_t* d_dst_left, uint8_t* d_dst_right, size_t dst_img_bytes, int dst_pitch);

/* ------------------------------------------------------------------ A1+A2+A3: VO::feature_detection --- */
/* Replaces the body of VO::feature_detection (visual_odometry.cpp:70-94) minus the GUI calls:
 * cv::ORB(3000)::detect (:80) -> VO::adaptive_non_maximal_suppresion(kps, anms_num) (:82, :96-157)
 * -> cv::ORB::compute (:85).  img: h rows of `stride` bytes (host).  kps/desc: caller buffers of `cap`
 * entries (desc: cap x 32 bytes).  *n_out = number of keypoints written. */
int vslam_feature_detection(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride,
                            vslam_keypoint* kps, uint8_t* desc, int cap, int* n_out);

/* The three stages individually, for parity tests (same citations). */
int vslam_orb_detect(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride, vslam_keypoint* kps, int cap, int* n_out);
int vslam_anms(vslam_ctx* ctx, vslam_keypoint* kps /*in/out*/, int n, int num, int* n_out);
int vslam_orb_compute(vslam_ctx* ctx, const uint8_t* img, int w, int h, int stride,
                      vslam_keypoint* kps /*in/out: filtered + regrouped by octave*/, int n, uint8_t* desc, int* n_out);

/* Batched, device-resident: d_imgs = B images, each h x pitch bytes, image b at d_imgs + b*img_bytes.
 * d_kps: B x kp_capacity keypoints; d_desc: B x kp_capacity x 32; d_count: B int32. */
int vslam_feature_detection_dev(vslam_ctx* ctx, const uint8_t* d_imgs, size_t img_bytes, int pitch, int B,
                                vslam_keypoint* d_kps, uint8_t* d_desc, int32_t* d_count);

/* ------------------------------------------------------------------ A5: VO::feature_matching ---------- */
/* Replaces VO::feature_matching (visual_odometry.cpp:219-251): BFMatcher(NORM_HAMMING, crossCheck=true)::match
 * (:225) + the distance gate d <= max(match_ratio*d_min, match_gap_thr*frame_gap) (:229-246).
 * q: nq x 32 (descriptors_1 = last frame), t: nt x 32 (descriptors_2 = current frame). out: >= nq entries.
 * gate = 0 returns the raw cross-check matches.  An empty match set yields *n_out = 0 (reference: UB, Q7). */
int vslam_feature_matching(vslam_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, double frame_gap,
                           int gate, vslam_dmatch* out, int* n_out);

/* Batched, device-resident: item b matches d_q + b*q_stride_bytes (d_nq[b] rows) against d_t + b*t_stride_bytes
 * (d_nt[b] rows); writes d_out + b*out_capacity (ascending queryIdx) and d_nout[b].  d_gap: per-item frame gap.
 * Alignment contract: d_q, d_t and both strides must be multiples of 16 bytes (the kernel reads descriptors with 16-byte
 * loads); anything else is VSLAM_ERR_ARG.  (The host-buffer call above stages into aligned memory itself.) */
int vslam_feature_matching_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq,
                               const uint8_t* d_t, size_t t_stride_bytes, const int32_t* d_nt,
                               const double* d_gap, int gate, int B, int max_rows,
                               vslam_dmatch* d_out, int out_capacity, int32_t* d_nout);

/* vslam_feature_matching_dev on a SUBSET of every item's query rows (additive: the ABI version is unchanged).  d_qsel (B x sel_capacity int32, device):
 * item b's selected query rows, d_qsel[b][0 .. d_nqsel[b]), ASCENDING original row indices; d_nqsel (B, device) their counts.
 * CONTRACT: the result equals vslam_feature_matching_dev run on the gathered rows Q[d_qsel[b][0 .. n)] with every queryIdx mapped back to the original
 * row index: trainIdx, distance, the output order (ascending original query index), the gate arithmetic (d_min over the subset's matches), the
 * out_capacity cut and d_nout are the unmasked entry's.  The first-minimum tie rules are unchanged (ascending selected row = ascending original row,
 * because the list ascends).  With d_qsel[b] = 0 .. d_nq[b] - 1 the output is vslam_feature_matching_dev's bit for bit; an empty selection gives
 * d_nout[b] = 0.  The unselected rows are never staged: the cost follows the selection's length, not d_nq.
 * PRECONDITION (not detected, like the one-to-one d_f2f of vslam_tracks_in): every index lies in [0, min(d_nq[b], max_rows)) and the list is strictly
 * ascending; otherwise the result is undefined (no access leaves the item's rows).  Refused with VSLAM_ERR_ARG: NULL d_qsel / d_nqsel,
 * sel_capacity < 1 or > 4096 (the matcher's row limit), and what vslam_feature_matching_dev refuses. */
int vslam_feature_matching_subset_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq, const int32_t* d_qsel,
                                      const int32_t* d_nqsel, int sel_capacity, const uint8_t* d_t, size_t t_stride_bytes, const int32_t* d_nt,
                                      const double* d_gap, int gate, int B, int max_rows, vslam_dmatch* d_out, int out_capacity, int32_t* d_nout);

/* vslam_feature_matching_subset_dev with the QUERY side of item b taken from another block (additive: the ABI version is unchanged).  d_qitem (B int32,
 * device): item b's query descriptor block (d_q + d_qitem[b] * q_stride_bytes), its d_nq entry, its d_qsel row and its d_nqsel entry are those of block
 * d_qitem[b]; the query side holds n_qitems blocks (d_nq / d_nqsel: n_qitems entries, d_qsel: n_qitems x sel_capacity).  The train side, d_gap[b] and
 * the outputs stay item b's.  d_qitem[b] outside [0, n_qitems) (-1 by convention: the item has no query frame) gives d_nout[b] = 0.  Several items
 * may name the same block.  This is how a frame is matched against its last ACCEPTED predecessor at the pair's real frame gap (VO::tracking after a
 * rejected frame, visual_odometry.cpp:630-637 and :239-242; vslam_build_map_pnp_inputs_recover_dev below).
 * CONTRACT: with d_qitem[b] = b (and n_qitems >= B) the output is vslam_feature_matching_subset_dev's bit for bit; in general item b equals that entry
 * run on the gathered blocks.  Same kernels: one index load ahead of the address arithmetic.  Refused with VSLAM_ERR_ARG: NULL d_qitem, n_qitems < 1,
 * and what vslam_feature_matching_subset_dev refuses (B counts items, so B <= max_batch; n_qitems is not bounded by it). */
int vslam_feature_matching_pairs_dev(vslam_ctx* ctx, const uint8_t* d_q, size_t q_stride_bytes, const int32_t* d_nq, const int32_t* d_qsel,
                                     const int32_t* d_nqsel, int sel_capacity, const int32_t* d_qitem, int n_qitems, const uint8_t* d_t, size_t t_stride_bytes,
                                     const int32_t* d_nt, const double* d_gap, int gate, int B, int max_rows, vslam_dmatch* d_out, int out_capacity,
                                     int32_t* d_nout);

/* ------------------------------------------------------------------ A6: dense stereo disparity --------- */
/* Replaces VO::disparity_map (visual_odometry.cpp:159-174): cv::StereoSGBM::create(0, 96, 9, 8*9*9, 32*9*9, 1, 63, 10,
 * 100, 32)->compute(left, right) followed by convertTo(CV_32F, 1/16).  left/right: h x w u8 (row stride in bytes);
 * disparity: h x w f32, tightly packed (invalid pixels = -1.0, like the reference).  Optional outputs (may be NULL):
 * disp_i16 = the CV_16S fixed-point map after median + speckle filtering, disp_raw_i16 = before them.
 * These two entries are vslam_disparity_map_ex[_dev] with the reference's set (vslam_default_sgbm_params): 96 disparities, a 9 x 9 window,
 * hence 100 < w <= 4096 and h > 9 (VSLAM_ERR_ARG otherwise; OpenCV 3.2's own output is undefined for w - 96 <= 4, where its
 * horizontal box sum reads past the pixel-cost row).  A rig with another baseline, lens or image size sets its own range, window
 * and matching constants through vslam_sgbm_params. */
int vslam_disparity_map(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                        float* disparity, int16_t* disp_i16, int16_t* disp_raw_i16);

/* Batched, device-resident: B stereo pairs at d_left/d_right + b*img_stride_bytes (row pitch in bytes); outputs
 * B x h x w, tightly packed.  The SGBM working set (about 250 MB per 1241x376 pair) is grown on demand and kept. */
int vslam_disparity_map_dev(vslam_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride_bytes,
                            int pitch, int w, int h, int B, float* d_disparity, int16_t* d_disp_i16, int16_t* d_disp_raw_i16);

/* The arguments of cv::StereoSGBM::create that a caller may set (additive: vslam_params and the ABI version are unchanged).  minDisparity is
 * 0 and the mode is MODE_SGBM (single pass, five directions): that is all the CPU oracle restates, so it is all this library computes.
 * Every accepted set gives OpenCV 3.2's map bit for bit; everything outside the accepted domain is VSLAM_ERR_ARG, never a different map. */
typedef struct vslam_sgbm_params {
    int32_t num_disparities;       /* 96    a multiple of 16 in [16, 256] (the winner key holds the disparity in 8 bits)            */
    int32_t block_size;            /* 9     odd, >= 1                                                                               */
    int32_t P1, P2;                /* 648, 2592 (8 / 32 * block^2)   0 < P1 < P2                                                     */
    int32_t disp12_max_diff;       /* 1     >= 0                                                                                    */
    int32_t pre_filter_cap;        /* 63    in [1, 63]; the Sobel channel is clipped to ftzero = max(cap, 15) | 1                    */
    int32_t uniqueness_ratio;      /* 10    in [0, 100]                                                                             */
    int32_t speckle_window_size;   /* 100   >= 0; 0 = no speckle filter                                                             */
    int32_t speckle_range;         /* 32    >= 0                                                                                    */
    int32_t struct_size;           /* sizeof(vslam_sgbm_params) of the caller's header; set by vslam_default_sgbm_params, checked  */
} vslam_sgbm_params;

/* the reference's set: (96, 9, 648, 2592, 1, 63, 10, 100, 32) and struct_size */
void vslam_default_sgbm_params(vslam_sgbm_params* p);

/* Is the set admissible for w x h images?  Host arithmetic only: no context, no GPU.  VSLAM_OK, or VSLAM_ERR_ARG with vslam_last_error()
 * naming the offending field.  Beyond the field ranges above:
 *   w - num_disparities > block_size / 2 (below that OpenCV 3.2 reads past its pixel-cost row), h > block_size, w <= 4096, and the
 *   16-bit range rule  3 * (block_size^2 * (2 * ftzero + 63) + P2) <= 65535:  a block cost is at most Cmax = block_size^2 * (2 * ftzero + 63)
 *   (Birchfield-Tomasi: 2 * ftzero on the clipped Sobel channel + 255 >> 2 on the raw one), a path value lies in [-P2, Cmax], and the running
 *   sum of three paths is kept as u16 with the offset 3 * P2.  The same bound keeps every 16-bit cost of OpenCV's own arithmetic from
 *   wrapping.  It holds P2 = 32 * block^2 up to block 9 at cap 63, and block 11 at cap 31; what lies beyond is refused. */
int vslam_sgbm_params_check(const vslam_sgbm_params* p, int w, int h);

/* vslam_disparity_map[_dev] with a caller's set (NULL = the reference's).  Same buffers and contracts; vslam_sgbm_params_check runs first, so
 * nothing is launched for a refused set.  The reference's set runs exactly the kernels of vslam_disparity_map[_dev]; any other set runs the
 * line-parallel kernels (one per path) at every batch size, on a cost volume of 16 * ceil-to-{2,4,6,8,12,16}(num_disparities / 16) int16 per pixel. */
int vslam_disparity_map_ex(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                           const vslam_sgbm_params* sgbm, float* disparity, int16_t* disp_i16, int16_t* disp_raw_i16);
int vslam_disparity_map_ex_dev(vslam_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride_bytes,
                               int pitch, int w, int h, int B, const vslam_sgbm_params* sgbm, float* d_disparity, int16_t* d_disp_i16,
                               int16_t* d_disp_raw_i16);

/* ------------------------------------------------------------------ A7: depth -> landmarks ------------ */
/* Replaces Frame::find_3d (types_def.cpp:9-18) + the gating of VO::set_ref_3d_position
 * (visual_odometry.cpp:176-217) for a disparity map (h x w f32, row stride in elements).  No compaction:
 * valid[i]/reliable[i] per keypoint, xyz_w[3i..] world point (f32, cv::Point3f).  *n_valid optional. */
int vslam_find_3d_disparity(vslam_ctx* ctx, const vslam_keypoint* kps, int n, const float* disparity, int w, int h,
                            int dstride, const double T_c_w[7], float* xyz_w, uint8_t* valid, uint8_t* reliable, int* n_valid);

/* north_star stage K8: the same contract from matched left/right pixels (uvL, uvR: n x 2 f32) through the
 * rectified-stereo inhomogeneous DLT instead of an SGBM disparity map. */
int vslam_triangulate(vslam_ctx* ctx, const float* uvL, const float* uvR, int n, const double T_c_w[7],
                      float* xyz_w, uint8_t* valid, uint8_t* reliable, int* n_valid);

/* Batched, device-resident form of the above: item b = d_n[b] keypoints at d_kps + b*kp_capacity, disparity map
 * d_disparity + b*h*w (tightly packed f32, e.g. the output of vslam_disparity_map_dev), pose d_T_c_w + 7*b. */
int vslam_find_3d_disparity_dev(vslam_ctx* ctx, const vslam_keypoint* d_kps, const int32_t* d_n, int kp_capacity, int B,
                                const float* d_disparity, int w, int h, const double* d_T_c_w, float* d_xyz_w,
                                uint8_t* d_valid, uint8_t* d_reliable);

/* Batched, device-resident: item b has d_n[b] pairs at offset b*capacity; pose d_T_c_w + 7*b. */
int vslam_triangulate_dev(vslam_ctx* ctx, const float* d_uvL, const float* d_uvR, const int32_t* d_n, int capacity, int B,
                          const double* d_T_c_w, float* d_xyz_w, uint8_t* d_valid, uint8_t* d_reliable);

/* Gather matched keypoint coordinates (device glue between matcher and triangulation / PnP):
 * uvQ[b][i] = kpsQ[b][match.queryIdx].pt, uvT[b][i] = kpsT[b][match.trainIdx].pt for i < min(d_nmatch[b], match_capacity); a count
 * <= 0 writes nothing, and rows at or past the count are left as they were.  An index outside [0, kp_capacity) is CLAMPED to that range (the
 * row is still written, with the pixel of keypoint 0 or kp_capacity - 1): the caller's tables decide what such a row means. */
int vslam_gather_matched_uv_dev(vslam_ctx* ctx, const vslam_keypoint* d_kpsQ, const vslam_keypoint* d_kpsT, int kp_capacity,
                                const vslam_dmatch* d_matches, const int32_t* d_nmatch, int match_capacity, int B,
                                float* d_uvQ, float* d_uvT);

/* ------------------------------------------------------------------ A8/A10: VO::motion_estimation ----- */
/* north_star stage K9, standing in for cv::solvePnPRansac (visual_odometry.cpp:277): motion-only LM on one
 * pose with PoseOnlyEdgeProjection's residual/Jacobian (optimization.cpp:75-101), g2o LM schedule, Huber
 * delta; inlier[i] = reprojection error <= pnp_reproj_thr at the estimate.  T_c_w in: guess, out: estimate. */
int vslam_pnp_motion_only(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int iters,
                          uint8_t* inlier, int* n_inliers, vslam_lm_stats* stats);

/* Batched, device-resident: problem b has d_n[b] points at offset b*capacity; poses d_T + 7*b (in/out). */
int vslam_pnp_motion_only_dev(vslam_ctx* ctx, const float* d_xyz_w, const float* d_uv, const int32_t* d_n, int capacity, int B,
                              double* d_T_c_w, int iters, uint8_t* d_inlier, int32_t* d_n_inliers);

/* The reference's own pose stage: cv::solvePnPRansac(pts3d, pts2d, K, Mat(), rvec, tvec, false, 100, 4.0, 0.99, inliers) at
 * visual_odometry.cpp:277 -- OpenCV's RNG (seed (uint64)-1, multiply-with-carry) and 5-point subset draw, EPnP on every subset
 * from scratch (no pose guess: useExtrinsicGuess = false), f32 squared reprojection errors against (float)(reproj_err^2), the
 * strict "more inliers than max(best, 4)" acceptance, RANSACUpdateNumIters, mask = RANSAC mask.
 * lm_iters = 0: T_c_w = the best RANSAC model itself -- what OpenCV 3.2.0 (the version the reference pins, README.md:72) returns: its
 * solvePnPRansac runs solvePnP on the inliers and then assigns `_local_model` to rvec / tvec (solvepnp.cpp), discarding the refined pose.
 * lm_iters > 0: T_c_w = the pose refined on the inliers of the best model (OpenCV 3.4.2+ behaviour).  All `max_iters` hypotheses are solved (one wave each) and scored in parallel on the device (they do not depend on
 * each other); the adaptive stopping rule is then replayed over the counts in order, so the result is that of the sequential loop.
 * Remaining deviations from OpenCV (the final refinement is this library's least-squares LM, not CvLevMarq; the eigen-solver's
 * basis for the null space of the 5-point system) are listed in oracle/ransac.c / epnp.c.  T_c_w: OUTPUT only (untouched on failure).
 * Returns VSLAM_OK; *n_inliers = 0 means RANSAC found no model (reference: solvePnPRansac returns false). */
int vslam_pnp_ransac(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int max_iters,
                     double reproj_err, double confidence, int lm_iters, uint8_t* inlier, int* n_inliers, int* iters_run);

/* The same call, additionally returning every hypothesis: models_Rt = max_iters x 12 doubles ([R row-major | t] of the EPnP model of
 * subset i), models_count = its inlier count over all points (-1: degenerate subset).  For diagnostics and the parity tests. */
int vslam_pnp_ransac_models(vslam_ctx* ctx, const float* xyz_w, const float* uv, int n, double T_c_w[7], int max_iters, double reproj_err,
                            double confidence, int lm_iters, uint8_t* inlier, int* n_inliers, int* iters_run, double* models_Rt,
                            int32_t* models_count);
/* The same call for B independent problems whose points are already on the device (throughput mode: the reference's own pose stage,
 * visual_odometry.cpp:277, batched): problem b owns d_n[b] points at [b * capacity, ...) of d_xyz_w (x 3) / d_uv (x 2).  All B x max_iters
 * hypotheses are solved and scored at once, the sequential acceptance rule with its adaptive stopping is replayed per problem.  Returns
 * what OpenCV 3.2.0 returns: the best RANSAC model itself (no refinement; the host-buffer call's lm_iters = 0), T = identity and 0 inliers
 * when no model was accepted or d_n[b] < 5.  d_inlier (B x capacity), d_n_inliers (B), d_iters_run (B) may be NULL.  Asynchronous. */
int vslam_pnp_ransac_dev(vslam_ctx* ctx, const float* d_xyz_w, const float* d_uv, const int32_t* d_n, int capacity, int B, double* d_T_c_w,
                         int max_iters, double reproj_err, double confidence, uint8_t* d_inlier, int32_t* d_n_inliers, int32_t* d_iters_run);

/* VO::check_motion_estimation (visual_odometry.cpp:316-346); host arithmetic (scalar). returns 1/0. */
int vslam_check_motion(int num_inliers, const double T_c_l[7], double frame_gap);

/* ------------------------------------------------------------------ A12: optimize_map ----------------- */
/* Replaces the optimiser of optimize_map (optimization.cpp:103-288) on the graph the caller built from the map
 * containers (:127-214): n_kf poses (none fixed), n_lm landmarks (f32 at rest, Q4), n_edge EdgeProjection
 * edges {kf_idx, lm_idx, uv}; any edge order.  g2o LM + Schur + Huber(huber_delta), `iters` iterations.
 * flag_lm[e]: landmark whose is_inlier flag edge e writes (reference: feat.landmark_id_, :258-264; quirk Q1),
 * or NULL for flag_lm = lm_idx.  lm_inlier: n_lm flags, in/out (:224-266, edges visited in ascending index).
 * update_poses / update_lms: if_update_map / if_update_landmark (:272-287).  chi2_out (n_edge) optional.
 * n_edge = 0 (a window whose landmarks were all classified out) is VSLAM_OK: poses, landmarks and flags stay, the statistics are zero.
 * K4 = {fx, fy, cx, cy}: the `const cv::Mat& K` argument of optimize_map / optimize_pose_only (optimization.hpp:137-139,
 * :150-152), passed per call; NULL = the context's intrinsics (vslam_params.cam). */
int vslam_local_ba(vslam_ctx* ctx, int n_kf, double* T_c_w, int n_lm, float* xyz, int n_edge,
                   const int32_t* kf_idx, const int32_t* lm_idx, const float* uv, const double* K4, const int32_t* flag_lm,
                   int iters, int update_poses, int update_lms, uint8_t* lm_inlier, double* chi2_out,
                   double* chi2_threshold_out, vslam_lm_stats* stats);

/* ------------------------------------------------------------------ A13: optimize_pose_only ----------- */
/* Replaces optimize_pose_only (optimization.cpp:290-436): unary PoseOnlyEdgeProjection edges, landmarks constant,
 * dense per-pose solve with one shared lambda, same chi2 classification, pose write-back (:429-435). */
int vslam_pose_only_window(vslam_ctx* ctx, int n_kf, double* T_c_w, int n_lm, const float* xyz, int n_edge,
                           const int32_t* kf_idx, const int32_t* lm_idx, const float* uv, const double* K4, const int32_t* flag_lm,
                           int iters, int update_poses, uint8_t* lm_inlier, double* chi2_out,
                           double* chi2_threshold_out, vslam_lm_stats* stats);

/* Batched, device-resident windows (throughput mode).  n_kf = keyframe slots per window (the stride of
 * d_T_c_w); window w uses the first d_n_kf[w] of them (NULL: all windows have n_kf keyframes).
 * Window w owns landmarks [lm_off[w], lm_off[w+1]) and edges [edge_off[w], edge_off[w+1]) of the concatenated
 * arrays; edges MUST be sorted by landmark inside a window (lm_idx ascending) with lm_idx/kf_idx window-local.
 * One call runs the reference's per-keyframe schedule (run_vslam.cpp:58-71) when schedule = 1:
 *   optimize_map(5 its, no write) x2, optimize_map(10 its, poses written), optimize_pose_only(10 its, written),
 * each followed by the chi2 classification that feeds the next pass's landmark filter; schedule = 0 runs a
 * single optimize_map(iters) (mode 0) or optimize_pose_only(iters) (mode 1) pass with update flags. */
typedef struct vslam_ba_batch {
    int32_t n_windows, n_kf;
    const int32_t* d_lm_off;      /* n_windows + 1 */
    const int32_t* d_edge_off;    /* n_windows + 1 */
    double* d_T_c_w;              /* n_windows x n_kf x 7, in/out */
    float* d_xyz;                 /* total_lm x 3, in/out (only with update_lms) */
    const uint8_t* d_reliable;    /* total_lm: Landmark::reliable_depth_ (optimize_map filter :160); NULL = all 1 */
    uint8_t* d_lm_inlier;         /* total_lm, in/out */
    const int32_t* d_kf_idx;      /* total_edge */
    const int32_t* d_lm_idx;      /* total_edge, window-local */
    const float* d_uv;            /* total_edge x 2 */
    double* d_chi2;               /* total_edge, out (last pass), caller's edge order; NULL = not wanted */
    vslam_lm_stats* d_stats;      /* n_windows (last pass) or NULL */
    int32_t total_lm, total_edge;
    const double* K4;             /* HOST pointer to {fx, fy, cx, cy} (the optimisers' `const cv::Mat& K`), NULL = context intrinsics */
    const int32_t* d_n_kf;        /* n_windows: keyframes of window w (1..n_kf), e.g. the growing map at the start of a sequence; NULL = n_kf */
} vslam_ba_batch;
int vslam_ba_batch_dev(vslam_ctx* ctx, const vslam_ba_batch* batch, int schedule, int mode, int iters,
                       int update_poses, int update_lms);

/* ------------------------------------------------------------------ graph construction on the device --
 * The BA half of a throughput-mode step built from the front-end's own output: replaces, for a batch of n_frames CONSECUTIVE
 * keyframes, the landmark / observation bookkeeping of VO::insert_key_frame (visual_odometry.cpp:363-424) and the graph build of
 * optimize_map / optimize_pose_only (optimization.cpp:127-214, :303-361).  Frame f = batch item f.  A frame's features are its
 * keypoints that the pose stage kept as inliers of a frame-to-frame match (they observe the landmark of the matched feature of
 * frame f - 1, :592-599) plus every other keypoint with a valid depth (it creates a landmark, :403-421); a landmark with an
 * unreliable depth takes the point of its first later observation with a reliable one (:391-401).  Window b = the map right after
 * keyframe b: keyframes [max(0, b - n_kf + 1), b], every landmark they observe (position and reliable flag as of frame b, world
 * = frame 0 through the chained relative poses), one edge per observation, edges landmark-major (landmarks ordered by their number
 * of observations inside the window, then by the first of them: frame, then keypoint index), lm_idx / kf_idx window-local, is_inlier = 1.
 * All pointers are device pointers. */
typedef struct vslam_tracks_in {
    int32_t n_frames;
    int32_t kp_capacity, lr_capacity, match_capacity, pnp_capacity; /* kp_capacity <= 65536 (the builder packs a keypoint index into 16 bits;
                                      larger values are refused with VSLAM_ERR_ARG) */
    const vslam_keypoint* d_kps;   /* n_frames x kp_capacity: left keypoints */
    const vslam_dmatch* d_lr;      /* n_frames x lr_capacity: depth association of frame f, queryIdx = left keypoint (L/R matches; the identity
                                      list when the depth comes from the disparity map) */
    const int32_t* d_nlr;          /* n_frames */
    const float* d_xyz;            /* n_frames x lr_capacity x 3: point of association m in the CAMERA frame of frame f (T_c_w = identity) */
    const uint8_t* d_valid;        /* n_frames x lr_capacity: the depth gates of set_ref_3d_position passed (:199) */
    const uint8_t* d_reliable;     /* n_frames x lr_capacity: reliable_depth_ (:201) */
    const vslam_dmatch* d_f2f;     /* (n_frames - 1) x match_capacity: item i = matches frame i (query) -> frame i + 1 (train).  PRECONDITION: one-to-one
                                      inside an item (no two matches share a queryIdx or a trainIdx) -- what the cross-checked matcher of
                                      vslam_feature_matching[_dev] (VO::feature_matching, visual_odometry.cpp:219-251) emits.  Matches that share a
                                      trainIdx (knn / ratio-test output) would make two tracks claim one keypoint: not supported, result undefined */
    const int32_t* d_nf2f;         /* n_frames - 1 */
    const uint8_t* d_pose_inlier;  /* (n_frames - 1) x pnp_capacity: inlier flag of input j of item i's pose problem, inputs in the order
                                      vslam_build_pnp_inputs_dev emitted them */
    const double* d_T_rel;         /* (n_frames - 1) x 7: T_{i+1,i}, the pose stage's estimate with frame i as the world */
    const int32_t* d_nkps;         /* n_frames: keypoints of frame f (no match refers to a keypoint index beyond it), or NULL: every slot up to
                                      kp_capacity is examined (slower, same result) */
    /* ---- ABI rev 5: a batch that is a CHUNK of a longer sequence (sequence mode, BASELINE config 5).  All four may be NULL / 0. */
    const double* d_T_abs;         /* n_frames x 7: T_{f,0} of every frame of the batch in the SEQUENCE's world (the gathered, chained relative poses);
                                      used instead of chaining d_T_rel from the batch's first frame */
    const float* d_carry_in;       /* kp_capacity x 4 floats, for the batch's FIRST frame: {x, y, z, flags} per keypoint slot -- flags (as float) 0: no
                                      track reaches this keypoint from before the batch; 1: one does, and (x, y, z) is its landmark's position so far
                                      (its creation point, no reliable depth seen yet); 3: likewise, position from a reliable depth.  What the rank that
                                      owns the frames before this chunk exports (d_carry_out): tracks and their landmark positions then continue across
                                      the chunk boundary exactly as in one unsharded batch */
    float* d_carry_out;            /* kp_capacity x 4 floats: the same record for frame `carry_out_frame` of THIS batch (the first frame of the next chunk) */
    int32_t carry_out_frame;       /* 1 .. n_frames - 1 (0: no carry-out) */
} vslam_tracks_in;
/* Fills the device arrays of `out` (caller-allocated: d_lm_off / d_edge_off n_frames + 1, d_T_c_w n_frames x n_kf x 7, d_xyz /
 * d_reliable / d_lm_inlier for lm_capacity landmarks, d_kf_idx / d_lm_idx / d_uv for edge_capacity edges, d_n_kf n_frames; the
 * const members are written through) and its scalar members (n_windows = n_frames, n_kf, total_lm = lm_capacity, total_edge =
 * edge_capacity: bounds).  d_status (1 int32): 0, or 1 when a capacity was too small -- the windows from the first one that did
 * not fit are then emitted empty.  Asynchronous on the context stream; `out` can go straight into vslam_ba_batch_dev.
 * Track continuation (round 6; vslam_set_tuning "track_rule", default 1): a frame-to-frame match gives the current keypoint the landmark of the
 * last-frame keypoint whenever that keypoint IS A FEATURE of the last frame -- created there (a valid depth) or tracked into it -- as VO::tracking
 * does (visual_odometry.cpp:568-599: the query set is frame_last_.features_).  If the last-frame keypoint owns a depth, it was input j of the pose
 * stage and d_pose_inlier decides (:306); if it does not, the pose stage's inlier rule (solvePnPRansac's 4 px, params.pnp_reproj_thr) is applied
 * to the landmark's MAP position (:260-270: pt_3d_, the creation point or the first reliable one) through the current frame's chained pose and
 * params.cam.  track_rule 0: only matches whose last-frame keypoint owns a depth continue a track (rounds 4-5). */
int vslam_build_windows_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int lm_capacity, int edge_capacity, vslam_ba_batch* out,
                            int32_t* d_status);

/* vslam_build_windows_dev with a choice of WHICH keyframes each window holds (additive: the ABI version is unchanged).
 * policy 0, sliding: S_b = [max(0, b - n_kf + 1), b]; the windows are vslam_build_windows_dev's bit for bit; evicted[b] = b - n_kf (-1 while < 0).
 * policy 1, reference culling (Map::remove_keyframe, map.cpp:48-130): S_0 = {0}; for b >= 1, S' = S_{b-1} + {b}, and when |S'| > n_kf
 *   d_k = |log(G_k o G_b^-1)|_2 for every k in S' \ {b}, G = the chained pose-stage poses the builder uses for the windows;
 *   far  = the first k (ascending frames) with d_k > far_d, starting from far_d = 0 (the largest distance, lowest frame on a tie);
 *   near = the first k (ascending frames) with d_k < near_d, starting from near_d = 1e6 (the smallest, lowest frame on a tie);
 *   near is evicted if near_d < near_dist (the reference: 0.2), otherwise far.
 *   Deviations from the reference: ties go to the lowest frame (the reference iterates an unordered_map); the distance is taken on the chained
 *   pose-stage poses, not on BA-refined ones (windows are independent); if no member qualifies (e.g. every distance is non-finite) the oldest
 *   member is evicted and bit 1 (value 2) of *d_status is set.  This entry point does not apply the keyframe gate of insert_key_frame
 *   (visual_odometry.cpp:353): every frame is a keyframe.  vslam_build_windows_gated_dev below applies it.
 * Window b holds the frames of S_b in ascending order in slots 0..|S_b|-1 (T_c_w slot k = G[S_b[k]], edges' kf_idx = slot); its landmarks are
 * those with at least one observation in a frame of S_b (what clean_map keeps), with position and reliable_depth_ as of frame b (a reliable
 * update in a culled frame counts), ordered as in vslam_build_windows_dev by observation count inside S_b, then by first observation inside S_b.
 * d_kf_frame (n_frames x n_kf, device): S_b ascending, -1 in unused slots; d_evicted (n_frames, device): the frame evicted at step b, -1 if none.
 * Status and capacity behaviour: vslam_build_windows_dev's (bit 0).  Refused with VSLAM_ERR_ARG: policy 1 on a chunk (d_T_abs, d_carry_in or
 * d_carry_out set: which keyframes survive depends on the whole history), near_dist NaN or negative, a policy other than 0 / 1, n_kf outside
 * 1..VSLAM_MAX_KF, NULL d_kf_frame / d_evicted. */
int vslam_build_windows_kf_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int policy, double near_dist, int lm_capacity,
                               int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status);

/* vslam_build_windows_kf_dev with insert_key_frame's keyframe gate (visual_odometry.cpp:348-424; additive: the ABI version is unchanged).
 * d_num_inliers (n_frames - 1, device): item i = the pose stage's inlier count (num_inliers_) of frame i + 1.  Per frame the state (d_frame_state,
 * n_frames, device): frame 0 is 2 (initialization); frame f >= 1 with n = d_num_inliers[f - 1], T = d_T_rel[f - 1] (T_c_l_):
 *   check = at least 10 inliers and |log T| <= 5 (check_motion_estimation :316-346, frame_gap 1; the arithmetic of vslam_check_motion);
 *   2 = keyframe: check && !(n >= 80 && angleY(T) < 0.03) (:353, angleY signed); 1 = tracked, not a keyframe; 0 = rejected (check false).
 * What a non-keyframe changes: its depth-valid keypoints that no track reaches create no landmark (they are not features: a match out of them
 * continues nothing), it records no observation, and a landmark with an unreliable depth does not take a reliable one from it (:391-401).
 * Tracked features pass through it, continued exactly as in vslam_build_windows_dev (d_pose_inlier, or track_rule 1's reprojection).
 * Keyframe sets: S_0 = {0}; at a keyframe step b, S_b = S_prev + {b}, and when that holds more than n_kf frames one member is evicted by the
 * policy -- 0: the oldest; 1: vslam_build_windows_kf_dev's Map::remove_keyframe rule (near_dist, ties, fallback and status bit 1 as there).  At
 * any other step S_b = S_{b-1} and d_evicted[b] = -1.  d_kf_frame[b] = S_b for every step (ascending, -1 padded).
 * Windows: at a keyframe step, window b is the map right after keyframe b is inserted -- vslam_build_windows_kf_dev's window on S_b (landmarks
 * with an observation in S_b, observations from keyframes only, position and reliable_depth_ as of frame b, the same order and capacity
 * behaviour).  At any other step the window is EMPTY: lm_off / edge_off do not advance, d_n_kf[b] = 0, T_c_w slot 0 = the frame's chained pose
 * (the BA reads defined numbers; nothing should read its result), the other slots untouched.
 * Deviations from the reference: a rejected frame (state 0) is never a keyframe but is otherwise treated like state 1 (tracks and the pose chain
 * pass through it; the reference re-matches the next frame against the last accepted one) and sets bit 2 (value 4) of *d_status; frame_gap is
 * always 1; the VO "Lost" state is not modelled; the pose stage's inputs are what the caller computed (after a non-keyframe they are not the
 * reference's; vslam_build_windows_map_gated_dev below runs the gate inside the map passes instead).  With every frame a keyframe, every output is
 * vslam_build_windows_kf_dev's with the same policy, bit for bit.
 * Refused with VSLAM_ERR_ARG: a chunk (d_T_abs, d_carry_in or d_carry_out set), NULL d_num_inliers when n_frames > 1, NULL d_kf_frame /
 * d_evicted / d_frame_state, a policy other than 0 / 1, near_dist NaN or negative, n_kf outside 1..VSLAM_MAX_KF. */
int vslam_build_windows_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, int n_kf, int policy, double near_dist, const int32_t* d_num_inliers,
                                  int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted,
                                  int32_t* d_frame_state, int32_t* d_status);

/* ---- Throughput mode, pose inputs against the MAP (additive: the ABI version and vslam_tracks_in are unchanged).
 * VO::motion_estimation (visual_odometry.cpp:260-277) hands solvePnPRansac every feature of the last frame that the current frame matched, at its
 * LANDMARK's map position (pt_3d_: the creation point or the first reliable one, :391-401), and erases the outliers from the frame (:306): tracking
 * is frame-to-map.  With every frame a keyframe, the sequential loop is, for f = 1 .. n_frames - 1:
 *   1. the query set is the features of frame f - 1 (the tracked inliers plus the landmarks created at f - 1);
 *   2. the inputs are every frame-to-frame match out of a feature, in match order: xyz_w = the landmark's position as of frame f - 1, uv = the
 *      current keypoint;
 *   3. the pose solver gives T_c_w(f) and an inlier mask; the inliers become features of f;
 *   4. insert_key_frame as in vslam_build_windows_dev: observations, reliable-depth upgrades, landmarks from f's own-depth keypoints that no track
 *      reaches, at T_c_w(f).
 * The batch stays parallel: it is computed in REFINEMENT PASSES, each parallel over all frames.  Pass 0 is the pose stage's own result:
 * G^0 = the chain of d_T_rel, links^0 = the d_pose_inlier flags of the own-depth inputs plus track_rule's judgement of depth-less features.
 * Pass k >= 1 starts from G^{k-1} (n_frames x 7 absolute T_c_w, frame 0 = the world = identity) and links^{k-1}: walk the tracks (a link holds
 * only if the previous pass said so; a link out of a slot that is no longer a feature continues nothing), emit every pair's inputs as in step 2
 * in the world of G^{k-1} (vslam_build_map_pnp_inputs_dev), run the caller's solver on every item at once (LM from the guess G^{k-1}_{i+1};
 * RANSAC takes no guess), and take G^k (row 0 = identity) and links^k = the inlier flags.  Failure rule: an item with 0 inliers gets
 * G^k_f = G^{k-1}_{f-1} and no links (stage A: a failed problem gives T_rel = identity).  Windows are built from G^K and links^K
 * (vslam_build_windows_map_dev).
 * CONTRACT: after k passes, frames 0..k are exactly the sequential loop's when the solver is a pure function of its inputs -- the inputs of pair
 * f - 1 -> f depend only on the links into frames <= f - 1 and the poses of frames <= f - 1 (induction on f).  With RANSAC this is exact, so
 * K >= n_frames - 1 passes reproduce the sequential loop; LM depends on its guess and converges rather than matching exactly.
 * These entries run without the keyframe gate (every frame a keyframe); the *_gated_dev entries below run the gate inside the passes. */

/* ---- Several independent sequences in one batch.  The entries of this section take "a batch of consecutive frames"; a context may instead declare
 * the batch as n_seg SEGMENTS laid back to back: segment k covers frames [first[k], first[k + 1]) and is a sequence of its own -- its first frame is an
 * initialisation frame and nothing crosses a boundary.  first: a HOST array of n_seg + 1 strictly ascending ints with first[0] = 0; n_seg = 0 with NULL
 * clears the table.  The table is context state like the rectification maps: uploaded once, expanded on the device to start(f) = the first frame of
 * f's segment, counted in vslam_device_bytes; the call synchronises the stream.
 * CONTRACT: for every segment, every output of every entry below is bit for bit what the same entry gives for a batch that holds that segment alone
 * (frame indices and offsets rebased).  Without a table every entry launches what it always launched, with the same bits.
 * A "boundary item" is item i of a per-pair array ((n_frames - 1) rows) whose frame i + 1 is a segment's first frame.  The rules:
 *   1. Boundary items are empty, whatever the caller's tables hold: no link, no pose input (d_n = 0, index map -1), no honoured match.  Tracks are
 *      paths over links, so no track crosses a boundary.  The *_requery_dev / *_recover_dev entries give such an item an empty re-matched table
 *      (d_nf2f_out = 0) without running the matcher on it.
 *   2. The pose chain restarts at every segment's first frame: G[start] = identity (vslam_chain_poses_dev and the builders' own chain, grouped per segment
 *      as for a batch that begins there), and a segment's landmark positions live in the world of its first frame.  The entries that take the
 *      caller's d_T_c_w expect row first[k] to be identity for every k; this is not checked.
 *   3. Frame states and pairings restart: state[start] = 2, pred[start] = -1, the boundary item's gap is 1.0, no pairing leaves a segment, and the
 *      Lost scan restarts -- a segment that ends Lost leaves the next one untouched.
 *   4. Keyframe sets and windows restart: the sliding window of frame b is [max(start(b), b - n_kf + 1), b] with d_n_kf[b] = min(b - start(b) + 1, n_kf);
 *      the culled and gated sets restart at S = {start}.
 *   5. Indices and status stay batch-wide: d_kf_frame / d_evicted / d_pred hold batch frame indices, offsets are those of the concatenated arrays, the
 *      status bits are ORs over the batch, and the capacity rule is unchanged (windows from the first one that does not fit, in batch order, are empty).
 * Honoured by vslam_build_windows_dev / _kf_dev / _gated_dev / _map_dev / _map_gated_dev / _map_recover_dev, vslam_build_map_pnp_inputs_dev / _gated_dev /
 * _requery_dev / _recover_dev, vslam_chain_poses_dev, vslam_gate_states_dev, vslam_gate_states_pairs_dev, vslam_frame_pairs_dev and
 * vslam_build_pnp_inputs_dev (B items = the pairs of B + 1 frames).
 * VSLAM_ERR_ARG, with vslam_last_error() naming the cause and nothing launched: a malformed table (the previous one stays in place); while a table
 * is set, one of those calls whose n_frames (or items + 1) differs from first[n_seg], or which carries a chunk input (d_T_abs, d_carry_in,
 * d_carry_out): a sequence sharded across ranks stays single-sequence. */
int vslam_set_segments(vslam_ctx* ctx, int n_seg, const int32_t* first);

/* G_0 = identity, G_f = T_rel[f - 1] o G_{f - 1} (n_frames x 7, device): the chain the window builders use, bit for bit.  Asynchronous. */
int vslam_chain_poses_dev(vslam_ctx* ctx, int n_frames, const double* d_T_rel, double* d_T_c_w);

/* One refinement pass's pose inputs.  d_T_c_w (n_frames x 7, device): G^{k-1}.  d_input_of_match_prev ((n_frames - 1) x match_capacity, device):
 * the previous pass's index map, with in->d_pose_inlier that pass's inlier flags ((n_frames - 1) x in->pnp_capacity, in->pnp_capacity = that pass's
 * out_capacity); NULL: pass-0 links (in->d_pose_inlier in own-depth order as in vslam_build_windows_dev, plus track_rule).  in->d_T_rel is not read.
 * Outputs per item i (frame pair i -> i + 1): d_xyz_w ((n_frames - 1) x out_capacity x 3 f32) the landmark's position as of frame i -- bit for bit the
 * position that landmark has in window i of vslam_build_windows_map_dev on the same poses and links; d_uv ((n_frames - 1) x out_capacity x 2) the
 * train keypoint (x, y); d_n (n_frames - 1) the input count; d_input_of_match ((n_frames - 1) x match_capacity) the input match k became, -1 for
 * none (entries from d_nf2f[i] on are -1).  *d_status: 0, or bit 0 when out_capacity cut an item's list (the inputs that fit are kept).  The
 * preconditions of vslam_tracks_in hold (one-to-one d_f2f, kp_capacity <= 65536).  Refused with VSLAM_ERR_ARG: a chunk (d_T_abs, d_carry_in,
 * d_carry_out or carry_out_frame set), NULL d_T_c_w, out_capacity < 1, a NULL output pointer.  Asynchronous on the context stream. */
int vslam_build_map_pnp_inputs_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                   float* d_xyz_w, float* d_uv, int32_t* d_n, int32_t* d_input_of_match, int out_capacity, int32_t* d_status);

/* vslam_build_windows_kf_dev on the poses d_T_c_w (n_frames x 7, G^K) and the links of d_input_of_match (index map of the pass that produced the flags
 * in in->d_pose_inlier; NULL: pass-0 links).  in->d_T_rel is not read.  Everything else -- policies 0 and 1, d_kf_frame / d_evicted, capacity and
 * status behaviour -- is vslam_build_windows_kf_dev's.  CONTRACT: with d_T_c_w = vslam_chain_poses_dev(d_T_rel) and d_input_of_match = NULL its output
 * equals vslam_build_windows_kf_dev's bit for bit.  Refused with VSLAM_ERR_ARG: a chunk, NULL d_T_c_w, and what vslam_build_windows_kf_dev refuses. */
int vslam_build_windows_map_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match, int n_kf,
                                int policy, double near_dist, int lm_capacity, int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame,
                                int32_t* d_evicted, int32_t* d_status);

/* ---- Throughput mode, the keyframe gate INSIDE the refinement passes (additive: the ABI version and vslam_tracks_in are unchanged).
 * insert_key_frame's gate (visual_odometry.cpp:353) joined with the map inputs.  The sequential loop, for f = 1 .. n_frames - 1:
 *   1. the query set is the features of frame f - 1: the tracked inliers into f - 1, plus -- if f - 1 is a keyframe (state 2; frame 0 always
 *      is) -- the landmarks created at f - 1;
 *   2. the inputs are every frame-to-frame match out of a feature, in match order: xyz_w = the landmark's position as of f - 1 (the creation point,
 *      or the first reliable one; reliable upgrades happen at keyframes only), uv = the current keypoint;
 *   3. the solver gives T_c_w(f), an inlier mask and num_inliers(f); with no inlier T_c_w(f) = T_c_w(f - 1) and there are no links;
 *   4. state(f) = keyframe_state(num_inliers(f), T_c_w(f) o T_c_w(f - 1)^-1) -- the rule of vslam_build_windows_gated_dev (check_motion_estimation,
 *      then the 80-inlier / angleY test; one definition, se3_device.h);
 *   5. at state 2 insert_key_frame runs (observations, reliable upgrades, new landmarks at T_c_w(f)) and the keyframe set is updated by the policy
 *      (0 oldest evicted, 1 culling); at states 0 and 1 the inliers pass through, nothing is recorded and the window is empty -- the rules of
 *      vslam_build_windows_gated_dev.
 * Deviations kept from vslam_build_windows_gated_dev: a rejected frame passes through (status bit 2), frame_gap is 1, no Lost state, BA results are
 * not fed back into tracking, windows are independent, the frame-to-frame matcher's query set is every keypoint of the last frame (this last one is
 * lifted by vslam_build_map_pnp_inputs_requery_dev below).
 * Passes: pass 0 is the pose stage (G^0 = the chain of d_T_rel, links^0 = its flags plus track_rule, states^0 = vslam_gate_states_dev(d_T_rel,
 * absolute = 0) on its inlier counts); pass k walks the tracks with states^{k-1} on (G^{k-1}, links^{k-1}) (vslam_build_map_pnp_inputs_gated_dev),
 * solves every item, takes G^k and links^k (the failure rule of step 3), then states^k = vslam_gate_states_dev(G^k, absolute = 1) on the pass's
 * inlier counts.  Windows: vslam_build_windows_map_gated_dev on (G^K, links^K, states^K).
 * CONTRACT: when the solver is a pure function of its inputs (RANSAC), after k passes the poses, inlier masks and states of frames 0..k and windows
 * 0..k equal the sequential loop's; K >= n_frames - 1 passes reproduce it.  LM depends on its guess and converges rather than matching exactly. */

/* d_frame_state (n_frames, device) = insert_key_frame's gate per frame: frame 0 is 2; frame f >= 1 gets keyframe_state(d_num_inliers[f - 1], T_c_l).
 * absolute = 0: d_T is T_rel ((n_frames - 1) x 7) and T_c_l = d_T[f - 1] -- bit for bit the d_frame_state vslam_build_windows_gated_dev writes;
 * absolute = 1: d_T is G (n_frames x 7 absolute T_c_w) and T_c_l = G_f o G_{f-1}^-1 (:615), computed on the device.  d_num_inliers: n_frames - 1,
 * item i = frame i + 1.  Refused with VSLAM_ERR_ARG: absolute outside 0 / 1, NULL d_frame_state, NULL d_T / d_num_inliers when n_frames > 1.
 * Asynchronous on the context stream. */
int vslam_gate_states_dev(vslam_ctx* ctx, int n_frames, const double* d_T, int absolute, const int32_t* d_num_inliers, int32_t* d_frame_state);

/* vslam_build_map_pnp_inputs_dev with the gated walk: d_frame_state (n_frames, device) = the previous pass's states; a node whose frame is not a
 * keyframe (state != 2) creates no landmark and gives no reliable depth, tracked features pass through it.  CONTRACT: with every state 2 the outputs
 * are vslam_build_map_pnp_inputs_dev's bit for bit.  Refused with VSLAM_ERR_ARG: NULL d_frame_state, and what vslam_build_map_pnp_inputs_dev refuses. */
int vslam_build_map_pnp_inputs_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                         const int32_t* d_frame_state, float* d_xyz_w, float* d_uv, int32_t* d_n, int32_t* d_input_of_match, int out_capacity,
                                         int32_t* d_status);

/* ---- The gated passes with the REFERENCE'S QUERY SET (additive: the ABI version and vslam_tracks_in are unchanged).  VO::tracking
 * (visual_odometry.cpp:568-575) builds descriptors_last from frame_last_.features_ only, and feature_matching runs its cross-check and the
 * max(match_ratio d_min, match_gap_thr frame_gap) gate on THAT subset.  In the gated sequential loop above, steps 1-2 then read:
 *   1. the query set is the features of frame f - 1 (as there); the frame-to-frame table of pair f - 1 -> f is the cross-checked, gated match of
 *      THOSE keypoints' descriptors (ascending keypoint index) against every keypoint of frame f;
 *   2. the inputs are every match of that table, in match order (every query is a feature by construction).
 * Frame 0's features are its depth-valid keypoints.  The deviation "the matcher's query set is every keypoint of the last frame" does not apply to
 * this mode; the others stay (a rejected frame passes through, frame_gap is 1, no Lost state, BA results are not fed back, windows are independent),
 * and the query order is ascending keypoint index where the reference's is feature order (ties and RANSAC's draw order only).
 * vslam_build_map_pnp_inputs_requery_dev = vslam_build_map_pnp_inputs_gated_dev, except that
 *   (a) the walk uses in->d_f2f / in->d_nf2f (the table the previous pass solved on) with that pass's index map and flags, and d_frame_state -- as there;
 *   (b) per frame f it writes the features of the walk -- d_feat (n_frames x in->kp_capacity int32): the ascending keypoint indices, d_nfeat (n_frames);
 *   (c) every pair i -> i + 1 is matched again by vslam_feature_matching_subset_dev's kernels: queries = the rows d_feat[i] of frame i's descriptors
 *       (frame f's block at d_desc + f * desc_stride_bytes, 32 bytes per keypoint), trains = every keypoint of frame i + 1 (in->d_nkps, required),
 *       frame_gap 1, gate on, the context's match_ratio / match_gap_thr; the table goes to d_f2f_out ((n_frames - 1) x in->match_capacity) /
 *       d_nf2f_out (n_frames - 1), which must not alias in->d_f2f / in->d_nf2f;
 *   (d) d_xyz_w, d_uv, d_n, d_input_of_match are emitted ON THE NEW TABLE (d_input_of_match indexes d_f2f_out).
 * The caller solves, and hands the next pass -- and vslam_build_windows_map_gated_dev -- in->d_f2f = this pass's d_f2f_out with this pass's index map
 * and flags.  Pass 1 takes the pose stage's all-keypoint table with d_input_of_match_prev = NULL.
 * CONTRACT: when the solver is a pure function of its inputs, after k passes the tables of pairs 0..k-1 and the poses, masks, states and windows of
 * frames 0..k equal the sequential loop's with steps 1-2 as above (the features of frame f after pass k are final for f <= k - 1: they depend on the
 * links into frames <= f and the tables of pairs <= f - 1, final after pass k - 1; pass 1 needs no links for frame 0).  With every keypoint of every
 * frame a feature the table is vslam_feature_matching_dev's and the inputs are vslam_build_map_pnp_inputs_gated_dev's on it, bit for bit.
 * n_frames = 1: d_nfeat[0] = 0 and nothing else is written.  Refused with VSLAM_ERR_ARG: what the gated entry refuses; NULL d_desc, d_feat, d_nfeat,
 * d_f2f_out, d_nf2f_out or in->d_nkps; d_desc / desc_stride_bytes not multiples of 16 or desc_stride_bytes < kp_capacity x 32; kp_capacity > 4096;
 * n_frames - 1 > max_batch; d_f2f_out overlapping in->d_f2f (or d_nf2f_out == in->d_nf2f). */
int vslam_build_map_pnp_inputs_requery_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                           const int32_t* d_frame_state, const uint8_t* d_desc, size_t desc_stride_bytes, int32_t* d_feat, int32_t* d_nfeat,
                                           vslam_dmatch* d_f2f_out, int32_t* d_nf2f_out, float* d_xyz_w, float* d_uv, int32_t* d_n, int32_t* d_input_of_match,
                                           int out_capacity, int32_t* d_status);

/* vslam_build_windows_map_dev with the frame states d_frame_state (n_frames, device) as an INPUT: the gated windows of vslam_build_windows_gated_dev --
 * the gated walk, keyframe sets updated at state 2 only (policy 0 oldest evicted, 1 culling), empty windows with d_n_kf[b] = 0 at states 0 and 1,
 * status bits 0-2 as there -- on the poses d_T_c_w and the links of d_input_of_match (NULL: pass-0 links).  in->d_T_rel is not read.
 * CONTRACTS, bit for bit: with every state 2 the outputs are vslam_build_windows_map_dev's with the same policy; with d_T_c_w = vslam_chain_poses_dev
 * (d_T_rel), d_input_of_match = NULL and d_frame_state = vslam_gate_states_dev(d_T_rel, absolute = 0) they are vslam_build_windows_gated_dev's
 * (windows, d_kf_frame, d_evicted, status).  Refused with VSLAM_ERR_ARG: NULL d_frame_state, and what vslam_build_windows_map_dev refuses. */
int vslam_build_windows_map_gated_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match,
                                      const int32_t* d_frame_state, int n_kf, int policy, double near_dist, int lm_capacity, int edge_capacity,
                                      vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status);

/* ---- The gated passes with the REFERENCE'S FAILURE HANDLING (additive: the ABI version, vslam_tracks_in and vslam_params are unchanged).  When
 * check_motion_estimation fails, VO::tracking does not call move_frame() (visual_odometry.cpp:630-637): the rejected frame and its features are dropped,
 * the next frame is matched against the features of the LAST ACCEPTED frame with frame_gap = the difference of their frame ids, which widens the
 * matcher's gate to max(match_ratio d_min, match_gap_thr frame_gap) (:239-242) and the motion check to 5 frame_gap (:328-329); after more than ten
 * consecutive rejections the state is Lost and the node loop ends (:673-693, run_vslam.cpp:78-81).  The sequential loop (conventions of
 * vslam_build_map_pnp_inputs_requery_dev unless stated; frame 0 is a keyframe, state 2), with last = 0 and lost_run = 0, for f = 1 .. n_frames - 1:
 *   1. if lost_run > 10 the VO is Lost: state(f) = 3, no table, no input, G_f = G_last, an empty window; Lost is absorbing (every later frame is 3);
 *   2. l = last, gap = f - l: the table of frame f is the cross-checked, gated match of the FEATURES OF FRAME l (ascending keypoint indices, as that
 *      frame was accepted) against every keypoint of frame f, with frame_gap = gap;
 *   3. every match of that table is an input, in match order: xyz_w = the landmark's map position as it stands after frame l (rejected frames change
 *      nothing in the map), uv = the keypoint of f;
 *   4. the solver gives T_c_w(f), a mask and num_inliers; with no inlier G_f = G_l and there are no links;
 *   5. T_c_l = G_f o G_l^-1; state(f) = 0 if !check_motion_rule(num_inliers, T_c_l, gap), else 1 if num_inliers >= 80 && angleY < 0.03, else 2;
 *   6. state 0: lost_run++, the frame's features are dropped (nothing is ever matched out of it), it records nothing, its window is empty, last stays;
 *   7. state 1 or 2: lost_run = 0, the inliers become the frame's features, at state 2 insert_key_frame runs and the keyframe set is updated by the
 *      policy exactly as in vslam_build_windows_map_gated_dev, last = f.
 * The remaining deviations of this mode from the reference: BA results are not fed back into tracking, and windows are independent (what sharding a
 * sequence into independent windows means); the query order is ascending keypoint index (ties and RANSAC's draw order only).
 * Passes: pass 0 is the pose stage on adjacent frames (states^0 = vslam_gate_states_dev(d_T_rel, absolute = 0), pred^{-1}(f) = f - 1).  Pass k >= 1
 * derives pred^{k-1} / gap from states^{k-1} (vslam_frame_pairs_dev's rule), walks the tracks on (G^{k-1}, table^{k-1}, links^{k-1}) -- table^{k-1}
 * was built on pred^{k-2} --, re-matches every frame f with pred^{k-1}(f) >= 0 from the features of pred^{k-1}(f) at gap f - pred^{k-1}(f), emits the
 * inputs on that table with positions as of frame pred^{k-1}(f) (vslam_build_map_pnp_inputs_recover_dev), solves every item (no inlier:
 * G^k_f = G^{k-1}_{pred(f)}; the LM guess stays G^{k-1}_f), and takes states^k = vslam_gate_states_pairs_dev(G^k, pred^{k-1}) on the pass's inlier
 * counts.  Windows: vslam_build_windows_map_recover_dev on (G^K, table^K, its pairing pred^{K-1}, links^K, states^K).
 * WALK RULE: only frames of state 1 or 2 (and frame 0) have features.  A link of item f - 1 holds only when the previous pass's mask kept it, its
 * query slot is a feature of pred_prev(f), frame f is accepted under the current states AND pred_prev(f) == pred(f): a table built on a pairing the
 * current states no longer give continues nothing this pass.  Frames of state 0 or 3 have an empty feature list.  The honoured links therefore join
 * consecutive accepted frames: tracks are disjoint paths, contiguous in accepted-frame rank, and every walk steps to the next accepted frame, which
 * lies strictly later, so it terminates on any input.
 * CONTRACT (A): with no state 0 (and so no 3) in any state vector involved, every output of vslam_build_map_pnp_inputs_recover_dev,
 * vslam_gate_states_pairs_dev and vslam_build_windows_map_recover_dev equals that of its sibling -- vslam_build_map_pnp_inputs_requery_dev,
 * vslam_gate_states_dev(absolute = 1), vslam_build_windows_map_gated_dev -- bit for bit (pred(f) = f - 1, every gap 1.0).
 * CONTRACT (B): with a solver that is a pure function of its inputs, after k passes everything that belongs to frames 0..k -- tables and feature lists,
 * inputs and masks, poses and states, pred / gap, windows -- equals the sequential loop above; K = n_frames - 1 reproduces it everywhere.  (Induction:
 * pred(f) read from states^{k-1} and from states^{k-2} agree for f <= k, so the links of final frames are always honoured.)
 * DEVICE SAFETY: every index read from a caller's array (d_pred_prev / d_pred of the windows entry, d_qitem, the states) is range-checked before it
 * addresses memory; an entry of d_pred_prev outside [-1, f) empties the item's links and sets bit 4 (value 16) of *d_status, as does a state outside
 * 0..3 (treated as rejected). */

/* The pairing: d_pred[f] (n_frames int32) = the last frame j < f with d_frame_state[j] in {1, 2} (frame 0 always counts); -1 for frame 0 and for a frame
 * that is Lost under these states -- a run of 11 or more frames of any other state ends directly before it, or an earlier frame is Lost.
 * d_gap[f - 1] (n_frames - 1 doubles) = f - d_pred[f], or 1.0 where d_pred[f] is -1.  One small scan kernel.  Refused with VSLAM_ERR_ARG: n_frames < 1,
 * NULL d_frame_state / d_pred, NULL d_gap when n_frames > 1.  Asynchronous on the context stream. */
int vslam_frame_pairs_dev(vslam_ctx* ctx, int n_frames, const int32_t* d_frame_state, int32_t* d_pred, double* d_gap);

/* vslam_gate_states_dev(absolute = 1) against the pairing d_pred (n_frames, the pairing the pass's items were built on): frame 0 is 2; frame f >= 1 with
 * p = d_pred[f] in [0, f) gets the gate on T_c_l = G_f o G_p^-1 with frame_gap = f - p in check_motion_rule; a frame with any other d_pred[f] had no
 * item in this pass and gets the raw state 0.  Then the Lost scan of vslam_frame_pairs_dev runs over the raw states in frame order and writes 3 from the
 * first Lost frame on.  CONTRACT: with d_pred[f] = f - 1 everywhere and no run of 11 zeros the output is vslam_gate_states_dev(absolute = 1)'s bit for
 * bit.  Refused with VSLAM_ERR_ARG: NULL d_pred / d_frame_state, NULL d_T_c_w / d_num_inliers when n_frames > 1, n_frames < 1. */
int vslam_gate_states_pairs_dev(vslam_ctx* ctx, int n_frames, const double* d_T_c_w, const int32_t* d_pred, const int32_t* d_num_inliers,
                                int32_t* d_frame_state);

/* vslam_build_map_pnp_inputs_requery_dev with the pairing.  d_pred_prev (n_frames, device): the pairing the table in in->d_f2f was built on; NULL means
 * f - 1 (the pose stage's table).  d_pred (n_frames) / d_gap (n_frames - 1): OUTPUTS, derived from d_frame_state as in vslam_frame_pairs_dev.  Item i is
 * frame i + 1, as everywhere.  The walk follows the WALK RULE above; d_feat / d_nfeat hold every frame's features (d_nfeat = 0 at states 0 and 3).  For
 * each f >= 1 with d_pred[f] >= 0 the feature list of frame d_pred[f] is matched against every keypoint of f at gap f - d_pred[f]
 * (vslam_feature_matching_pairs_dev's path), and the inputs are emitted on that table with positions as of frame d_pred[f].  A Lost frame gets
 * d_n = 0, d_nf2f_out = 0 and an index map of -1.  *d_status: bits 0-2 as in the sibling, bit 3 (value 8) when any frame is Lost, bit 4 (value 16) for
 * an out-of-range d_pred_prev entry or state.  n_frames = 1: d_pred[0] = -1, d_nfeat[0] = 0, nothing else is written.
 * Refused with VSLAM_ERR_ARG: what vslam_build_map_pnp_inputs_requery_dev refuses (a chunk included), NULL d_pred or d_gap. */
int vslam_build_map_pnp_inputs_recover_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match_prev,
                                           const int32_t* d_pred_prev, const int32_t* d_frame_state, const uint8_t* d_desc, size_t desc_stride_bytes,
                                           int32_t* d_feat, int32_t* d_nfeat, vslam_dmatch* d_f2f_out, int32_t* d_nf2f_out, float* d_xyz_w, float* d_uv, int32_t* d_n,
                                           int32_t* d_input_of_match, int out_capacity, int32_t* d_pred, double* d_gap, int32_t* d_status);

/* vslam_build_windows_map_gated_dev with the pairing d_pred (n_frames, device) of the table passed in in->d_f2f (a pass's d_pred output).  The walk
 * follows the WALK RULE above with the pairing of d_frame_state; observations, landmark creation and reliable upgrades happen at state 2 only; states
 * 0, 1 and 3 give empty windows; the keyframe sets are vslam_build_windows_map_gated_dev's.  *d_status: bits 0-2 as there, bit 3 when a frame is Lost,
 * bit 4 for an out-of-range d_pred entry or state.  Refused with VSLAM_ERR_ARG: NULL d_pred, and what vslam_build_windows_map_gated_dev refuses. */
int vslam_build_windows_map_recover_dev(vslam_ctx* ctx, const vslam_tracks_in* in, const double* d_T_c_w, const int32_t* d_input_of_match,
                                        const int32_t* d_pred, const int32_t* d_frame_state, int n_kf, int policy, double near_dist, int lm_capacity,
                                        int edge_capacity, vslam_ba_batch* out, int32_t* d_kf_frame, int32_t* d_evicted, int32_t* d_status);

/* ---- Throughput mode, CHAINED BA windows (additive: vslam_ba_batch, vslam_params and the ABI version are unchanged).  vslam_ba_batch_dev treats the
 * windows of a batch as independent: is_inlier is 1 on entry to every window, a keyframe enters window b at its pose-stage pose, and the BA runs from
 * the first keyframe.  The reference carries the is_inlier flags from one optimize_map to the next keyframe's graph (optimization.cpp:160), passes every
 * keyframe through up to ten successive schedules, each from the poses the one before wrote (:272-278), and starts at keyframes_.size() >= 10
 * (run_vslam.cpp:58).  optimize_map is only ever called with if_update_landmark = false and the new keyframe's pose comes from solvePnPRansac without
 * a guess (visual_odometry.cpp:268-290), so what one window hands to the next is (a) the poses of the keyframes they share and (b) one is_inlier flag per
 * landmark.  A keyframe's identity is its batch frame index; a landmark's is the root of its track, below.
 *
 * Landmark identities.  d_lm_id (capacity int32, device) is context state like the segment table; NULL / 0 clears it.  While it is set, every
 * vslam_build_windows*_dev entry also writes d_lm_id[l] for each landmark l of the concatenated landmark array: frame x kp_capacity + keypoint of the
 * keypoint that CREATED the landmark (batch frame index).  Two landmarks of a batch's windows are the same map landmark exactly when their ids are
 * equal; inside a window the ids are distinct.  With no buffer set every builder launches exactly what it launches without this entry.
 * Refused with VSLAM_ERR_ARG while a buffer is set: a builder call whose lm_capacity exceeds `capacity`; a chunk call (d_T_abs / d_carry_in /
 * d_carry_out), because a root from before the batch has no frame index.  The call itself refuses capacity < 0 and NULL with capacity != 0 (or the reverse). */
int vslam_set_window_ids(vslam_ctx* ctx, int32_t* d_lm_id, int capacity);

/* The chained BA.  `batch`: what a builder filled for the whole batch (n_windows = frames); d_lm_id: the ids that builder wrote (total_lm entries);
 * d_kf_frame: the builder's keyframe sets, or NULL for the sliding window [max(start(w), w - n_kf + 1), w].  The segment table says which windows form a
 * sequence; without one the batch is one sequence.  Step j = 0, 1, ... runs the schedule of vslam_ba_batch_dev(schedule = 1) -- same kernels, same
 * tuning keys -- on the j-th window of every sequence that has one, all of them in one launch.  Window w = first[s] + j at step j:
 *   1. entry state: slot k holds frame g = d_kf_frame[w][k]; for g == w the slot keeps the builder's pose, for g != w it takes the pose the chain holds
 *      for g (the latest value an earlier window of the sequence left for it; the builder's if there is none); lm_inlier[l] = the chain's flag of
 *      d_lm_id[l], 1 until some window has written it;
 *   2. the window is ACTIVE when d_n_kf[w] >= min_kf (min_kf = 10: the reference's keyframes_.size() >= 10; 1: every non-empty window); a window with
 *      d_n_kf[w] = 0 (the gate's non-keyframe steps) never is;
 *   3. an active window runs the schedule from that state; its poses, flags, chi2 and stats go to the caller's arrays at window w and into the chain
 *      state; d_ran[w] = 1;
 *   4. an inactive window with d_n_kf[w] > 0: the carried poses and flags of 1 are written to the caller's arrays at w, its own pose enters the chain
 *      state, d_ran[w] = 0 -- so the last window that held a frame always has that frame's final pose;
 *   5. an inactive window with d_n_kf[w] = 0 is left as built; d_ran[w] = 0.
 * COMPOSITION of step j (the result is bit for bit vslam_ba_batch_dev(schedule = 1) on this batch): one window slot per sequence with more than j
 * frames, ascending; n_kf, total_lm, total_edge and K4 the caller's; an active window's landmarks and edges packed in slot order; an inactive window
 * EMPTY (offsets do not advance, d_n_kf = 0, the builder's poses) -- the shape the gated builders emit.  Nothing between two steps waits for the device:
 * no synchronisation, no device-to-host copy.  State (a pose per frame, a byte per n_frames x kp_capacity root) and the staging batch (sized by the
 * caller's totals) live in a growable scratch of the context, counted by vslam_device_bytes.
 * Afterwards vslam_ba_status_dev(ctx, n_windows, h) returns, per window of the CALLER's batch, the status word of the step that ran it (0 for an
 * inactive window); vslam_ba_schedule_passes_dev / vslam_ba_deferred_dev describe single launches and return VSLAM_ERR_ARG until the next one.
 * d_chi2 / d_stats / d_reliable / d_n_kf of the batch and d_ran are optional.  Device safety: every offset, id and frame index read from the caller's
 * arrays is range-checked; a window whose offsets leave the arrays is treated as inactive.
 * Refused with VSLAM_ERR_ARG: NULL d_lm_id, min_kf outside 1..batch->n_kf, batch->n_windows different from the segment table's frame count when a
 * table is set, and what vslam_ba_batch_dev refuses.  Asynchronous on the context stream. */
int vslam_ba_chain_dev(vslam_ctx* ctx, const vslam_ba_batch* batch, const int32_t* d_lm_id, const int32_t* d_kf_frame, int min_kf, int32_t* d_ran);

/* per-window status of the most recent window launch on this process (VSLAM_OK or VSLAM_ERR_ARG per window) */
int vslam_ba_status_dev(vslam_ctx* ctx, int n_windows, int32_t* h_status);
/* optimize_map passes the most recent vslam_ba_batch_dev(schedule = 1) call EXECUTED per window: 3 = all of run_vslam.cpp:61-66; 1 or 2 = the
 * window's first / second pass flagged no new landmark, so the following passes would have repeated it bit for bit (all passes start from the same
 * poses and landmarks; only the flags carry over) and it was continued to the last pass's 10 iterations instead -- same result, 10 or 15 LM
 * iterations instead of 20.  vslam_set_tuning(ctx, "ba_adaptive", 0) runs every pass.  Synchronises the context stream. */
int vslam_ba_schedule_passes_dev(vslam_ctx* ctx, int n_windows, int32_t* h_passes);
/* Which kernel took each window of the most recent vslam_ba_batch_dev / vslam_local_ba call (optimization.cpp:103-288): h_deferred[w] = 0 when
 * ba_resident_kernel (landmark state in LDS) ran its optimize_map passes, 1 when it was left to lm_window_kernel (state in HBM: the window does not
 * fit half a CU's LDS, is denser than 2.2 observations per landmark, or the call did not involve the resident kernel).  Diagnostic for the
 * measurement tier (bench.py names the roofline kernel after what ran); synchronises the context stream. */
int vslam_ba_deferred_dev(vslam_ctx* ctx, int n_windows, int32_t* h_deferred);

/* Diagnostic (rows A10 / A11): the residual and the Jacobians of EdgeProjection (optimization.cpp:41-73) and PoseOnlyEdgeProjection
 * (:75-101) as THE DEVICE CODE OF THE LM KERNELS evaluates them -- the same device functions (normalised-coordinate factors At, Bt,
 * en, Huber weight), scaled back to pixels: err = z - K (T p) / Z (2), J_pose = d err / d xi for the left perturbation T <- exp(xi) T,
 * xi = [translation; rotation] (2 x 6, row-major), J_point = d err / d p_w (2 x 3), chi2 = |err|^2, w = Huber weight (delta =
 * params.huber_delta).  n observations of n world points through ONE pose; host buffers, synchronous; any output may be NULL. */
int vslam_edge_jacobians(vslam_ctx* ctx, int n, const float* xyz_w, const float* uv, const double T_c_w[7], const double* K4,
                         double* err, double* J_pose, double* J_point, double* chi2, double* huber_w);
/* Kernel-choice overrides of a context (tuning aid, and how the tests force every kernel path): name in {"orb_fuse_min", "orb_tiled" (0 | 1: the fused ORB kernel writes the levels that the orientation and descriptor kernels sample row-major | as 16 x 8 pixel tiles of one cache line each; default 1; same bits either way), "anms_cap" (pixels at which the ANMS radius walk stops early, 0 = never; same output either way, see vslam_orb_anms_path_dev), "sgbm_fuse_min",
 * "sgbm_fwd_min" (items per call from which the fused kernel is used), "sgbm_fw_rows" (32 | 64), "pose_only_window", "pose_only_waves" (0 = automatic | 12 | 4: waves per window of the schedule's pose-only kernel; default by the number of windows in the call; same bits either way), "pnp_window", "ba_adaptive" (0 | 1), "rectify_form" (0 | 1: source side of the rectification kernel, direct gathers | source boxes staged in LDS; same bytes), "voxel_form" (0 | 1: vslam_voxel_fuse_disparity_dev inserts every point directly | sums each image tile in LDS first; same table), "ba_lanes" (256 | 512: lanes per window of the
 * LDS-resident optimize_map kernel; default by the number of windows in the call; the results do not depend on it), "track_rule" (0 | 1: see
 * vslam_build_windows_dev; this one changes RESULTS, it is the before / after switch of round 6)};
 * value -1 = the library's batch-size rule.  vslam_create seeds them once from the environment variables VSLAM_<NAME> (an unparsable
 * or out-of-range value makes vslam_create fail with VSLAM_ERR_ARG); nothing reads the environment afterwards. */
int vslam_set_tuning(vslam_ctx* ctx, const char* name, int value);
/* status word of the most recent vslam_disparity_map_dev launch: synchronises the stream; *h_status = 0 and VSLAM_OK, or
 * *h_status != 0 and VSLAM_ERR_HIP when the chained forward sweep gave up waiting for a predecessor slab (its maps are void).
 * The host-buffer call vslam_disparity_map checks it itself. */
int vslam_sgbm_status_dev(vslam_ctx* ctx, int32_t* h_status);
/* per-image ORB capacity flags of the most recent ORB launch (0 = ok) */
int vslam_orb_status_dev(vslam_ctx* ctx, int B, int32_t* h_status);
/* Which way each image of the most recent ANMS launch (vslam_feature_detection[_dev], vslam_anms, vslam_orb_compute) went through orb_anms_kernel.
 * The kernel's suppression-radius walk stops once it has cleared "anms_cap" pixels (vslam_set_tuning; default one cell of its grid) and takes the
 * selection from such radii only when that is provably the selection of VO::adaptive_non_maximal_suppresion (visual_odometry.cpp:124-153);
 * otherwise it finishes the stopped walks and selects again.  The output never depends on it.  Synchronises the context stream. */
#define VSLAM_ANMS_PATH_NONE 0     /* no ANMS: anms_num <= 0 or fewer keypoints than anms_num (:100) */
#define VSLAM_ANMS_PATH_SHORTCUT 1 /* capped walk, selection accepted */
#define VSLAM_ANMS_PATH_FALLBACK 2 /* capped walk, check failed: stopped walks finished, selection redone */
#define VSLAM_ANMS_PATH_UNCAPPED 3 /* "anms_cap" = 0: every walk runs to its end */
int vslam_orb_anms_path_dev(vslam_ctx* ctx, int B, int32_t* h_path);
/* Diagnostic (rows A1 / A3): one level of the scale pyramid (blurred = 0: cv::resize INTER_LINEAR of the level above, what cv::ORB::detect runs
 * FAST / Harris / the IC angle on; level 0 is the caller's image and is not kept) or of the GaussianBlur 7x7 sigma 2 pyramid (blurred = 1: what
 * cv::ORB::compute samples) of image `item` of the most recent ORB launch of this context (vslam_feature_detection[_dev], vslam_orb_compute:
 * the calls that describe fill both; detect-only calls fill the unblurred pyramid), copied to host memory: *w x *h bytes, row stride out_stride.
 * Synchronises the stream.  visual_odometry.cpp:80,85 (inside cv::ORB). */
int vslam_orb_level(vslam_ctx* ctx, int item, int level, int blurred, uint8_t* out, int out_stride, int out_rows, int* w, int* h);

/* Device glue between the frame-to-frame matcher and the motion-only stage (the gather of
 * VO::motion_estimation, visual_odometry.cpp:260-270): for every frame-to-frame match (query = previous frame,
 * train = current frame) whose query keypoint owns a valid triangulated point (found through the previous frame's
 * L/R matches d_lr, whose queryIdx is the left keypoint), emit (xyz, current pixel), in match order.
 * d_kp2lr: B x kp_capacity int32 scratch.  Outputs: B x out_capacity.
 * The rule, as a sequential loop per item: d_kp2lr = -1; for i < min(d_nlr, lr_capacity) in order, an in-range queryIdx q sets d_kp2lr[q] = i, so
 * of two L/R matches with the same queryIdx the LAST one wins (the largest i, independent of the launch); the frame-to-frame matches
 * i < min(d_nf2f, match_capacity) are walked in order, one survives when both of its indices are inside [0, kp_capacity), d_kp2lr[queryIdx] >= 0
 * and d_valid_lr of that L/R match is non-zero (an out-of-range index drops the match; nothing is clamped here); survivor number s is written
 * only if s < out_capacity and d_nout = min(survivors, out_capacity).  Rows at or past d_nout are left as they were; a count <= 0 gives 0. */
int vslam_build_pnp_inputs_dev(vslam_ctx* ctx, const vslam_dmatch* d_f2f, const int32_t* d_nf2f, int match_capacity,
                               const vslam_dmatch* d_lr, const int32_t* d_nlr, int lr_capacity, const float* d_xyz_lr,
                               const uint8_t* d_valid_lr, const vslam_keypoint* d_kps_cur, int kp_capacity, int B,
                               int32_t* d_kp2lr, float* d_xyz_out, float* d_uv_out, int32_t* d_nout, int out_capacity);

/* ------------------------------------------------------------------ stage profiler --------------------- */
/* hipEvent brackets around every kernel family launched by this thread's calls on this context (the reference only
 * has a commented-out ros::Time stopwatch, visual_odometry.cpp:652,701-702).  vslam_profile_read synchronises the
 * stream, returns accumulated milliseconds per kernel family since the last read, and resets. */
typedef struct vslam_kernel_time {
    char name[48];
    double total_ms;
    int32_t launches; /* kernel launches covered */
    int32_t calls;    /* brackets recorded */
} vslam_kernel_time;
int vslam_profile_enable(vslam_ctx* ctx, int on);
int vslam_profile_read(vslam_ctx* ctx, vslam_kernel_time* out, int cap, int* n_out);
/* The same brackets as INTERVALS on one time axis PER DEVICE (milliseconds since the first vslam_profile_enable(.., 1) of any context of this
 * process on the context's device; contexts on different devices have different origins -- HIP events of two devices share no clock): with several contexts / streams in flight together this is what tells how much their kernel families overlap.  Synchronises
 * the stream, returns up to `cap` brackets recorded since the last read of either kind (in launch order) and resets, like vslam_profile_read. */
typedef struct vslam_stage_interval {
    char name[48];
    double t0_ms, t1_ms;
} vslam_stage_interval;
int vslam_profile_intervals(vslam_ctx* ctx, vslam_stage_interval* out, int cap, int* n_out);

/* Measurement aid: a float4 streaming copy of `bytes` (read + write), `reps` launches timed with hipEvents on the context
 * stream; *gbs_out = moved GB/s.  The achievable-bandwidth figure reported next to the 8 TB/s HBM spec. */
int vslam_hbm_copy_probe(vslam_ctx* ctx, size_t bytes, int reps, double* gbs_out);
/* One shape of that copy (unroll, non-temporal or not, workgroups per CU): variant = 0 .. vslam_hbm_copy_probe_variants() - 1;
 * name_out (>= 64 bytes, may be NULL) receives its description.  vslam_hbm_copy_probe reports the best of them. */
int vslam_hbm_copy_probe_variants(void);
int vslam_hbm_copy_probe_variant(vslam_ctx* ctx, size_t bytes, int reps, int variant, double* gbs_out, char* name_out);

/* ------------------------------------------------------------------ dense map: disparities fused into a voxel grid --- */
/* The SGBM stage computes a disparity for every pixel of every keyframe; this stage turns them, at the keyframes' poses, into a MAP: a sparse
 * voxel grid in a device hash table.  A point list is no product at batch size (1024 keyframes hold 4.8e8 pixels), a fused, bounded structure is.
 * Every voxel holds integers only -- a point count, the sums of the points' sub-voxel offsets (1/256 voxel) and of their 8-bit intensities -- so
 * the table is bit-reproducible under any arrival order.  The reference has no dense map (it publishes its landmark cloud, visualization.cpp:19-74).
 * Additive: vslam_params and the ABI version are unchanged; the host mirror (host/) does not call the stage.
 *
 * KEY of a point (x, y, z) in map `map_id`, with vs = (float)voxel_size and inv = 1.0f / vs, per axis in f32:
 *   t = x * inv (rounded to f32 before anything else uses it), c = floorf(t), i = (int)c, o = min((int)((t - c) * 256.0f), 255).
 * A point with a non-finite t, or an i outside [-2^17, 2^17), is dropped and counted (n_dropped_range).
 *   key = map_id << 54 | (ix + 2^17) << 36 | (iy + 2^17) << 18 | (iz + 2^17),  map_id in [0, 1022] (all-ones is the empty slot).
 * VOXEL: count, sum_ox, sum_oy, sum_oz, sum_intensity, all uint32: exact while count < 2^24 (255 * 2^24 < 2^32); an extraction that meets a larger
 * count sets status bit 1 and that voxel's sums are void.
 * TABLE: 2^log2_capacity slots of 32 bytes (key 8, the five sums 20, 4 unused), open addressing with linear probing over at most 128 slots.  A point
 * that finds no slot is dropped and counted (n_dropped_full, status bit 0); which points are lost then depends on the arrival order, but
 * sum of counts + n_dropped_full + n_dropped_range = valid points offered always holds.  Size the table for a load factor below one half. */
typedef struct vslam_voxel_map vslam_voxel_map;
struct vslam_voxel_stats {
    uint64_t n_occupied;       /* occupied slots                                   */
    uint64_t n_points;         /* points accumulated (the sum of the voxels' counts) */
    uint64_t n_dropped_range;  /* points dropped for range                         */
    uint64_t n_dropped_full;   /* points dropped because the table was full        */
    uint32_t status;           /* bit 0: table full; bit 1: a voxel count reached 2^24 */
    int32_t struct_size;       /* sizeof(struct vslam_voxel_stats) of the caller's header: set by the caller, checked */
};
typedef struct vslam_voxel {   /* one extracted voxel (32 bytes) */
    int32_t ix, iy, iz;        /* voxel index per axis */
    uint32_t count;
    float x, y, z;             /* centroid: ((double)ix + ((double)sum_ox / count + 0.5) / 256.0) * (double)vs, cast to float; y, z likewise */
    float intensity;           /* (float)((double)sum_intensity / count) */
} vslam_voxel;

/* A table of 2^log2_capacity slots (log2_capacity in [10, 28]) for voxels of voxel_size (finite, > 0), empty.  Its 32 << log2_capacity bytes are
 * counted in vslam_device_bytes while the handle lives.  A map belongs to its context and is destroyed before it.  Synchronous. */
int vslam_voxel_create(vslam_ctx* ctx, double voxel_size, int log2_capacity, vslam_voxel_map** out);
void vslam_voxel_destroy(vslam_voxel_map* vm);
/* empties the table and zeroes the counters and the status; asynchronous on the context stream */
int vslam_voxel_clear(vslam_voxel_map* vm);
/* the counters so far (host->struct_size set by the caller); synchronises the context stream */
int vslam_voxel_stats(vslam_voxel_map* vm, struct vslam_voxel_stats* host);

/* Every entry below is asynchronous on the context stream and refuses with VSLAM_ERR_ARG before it launches anything: a null pointer where one is
 * required, B < 1 or B > max_batch, step < 1, z_min >= z_max (or either not finite), a map_id outside [0, 1022] (extraction: [-1, 1022]),
 * w or h < 1, a pitch below w, a voxel map of another context.
 *
 * vslam_reproject_dev: every pixel (c, r) with c % step == 0 and r % step == 0 of B disparity maps (B x h x w f32, tightly packed) through
 * Frame::find_3d's arithmetic for a keypoint at ((float)c, (float)r) (types_def.cpp:9-18: f64 math, f32 at rest) and the inverse of the item's pose
 * d_T_c_w + 7 b, as vslam_find_3d_disparity_dev does; valid = z_min < Z < z_max.  Outputs B x ceil(h / step) x ceil(w / step): d_xyz f32 x 3,
 * d_valid uint8.  The fused entry below runs the same device function: same bits. */
int vslam_reproject_dev(vslam_ctx* ctx, const float* d_disparity, int w, int h, int B, const double* d_T_c_w, double z_min, double z_max, int step,
                        float* d_xyz, uint8_t* d_valid);
/* n f32 points into map map_id; d_valid (n uint8, NULL: all valid) masks points out, d_intensity (n uint8, NULL: 0) is summed per voxel.  Also the
 * way to map the landmarks of the BA windows (vslam_ba_batch positions). */
int vslam_voxel_insert_points_dev(vslam_ctx* ctx, vslam_voxel_map* vm, const float* d_xyz, const uint8_t* d_valid, const uint8_t* d_intensity, size_t n,
                                  int map_id);
/* Reprojection and insertion in one pass, no point ever written to memory: item b's valid points (vslam_reproject_dev's) go into map d_map_id[b]
 * (B int32; an item whose id is negative or above 1022 is skipped), their intensity the pixel of d_gray + b * img_bytes (rows of `pitch` bytes;
 * NULL: 0).  Two forms, same table (vslam_set_tuning "voxel_form"): 0 = every point straight into the table; 1 = a workgroup sums its image tile in
 * an LDS hash table first and adds each distinct voxel of the tile to the table once (in both, a lane first merges equal keys among its own four
 * adjacent pixels). */
int vslam_voxel_fuse_disparity_dev(vslam_ctx* ctx, vslam_voxel_map* vm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                                   int w, int h, int B, const double* d_T_c_w, const int32_t* d_map_id, double z_min, double z_max, int step);
/* The occupied slots with count >= min_count of map map_id (-1: every map), compacted into d_out (`capacity` vslam_voxel) and, when given, their
 * map ids into d_map_out (`capacity` int32); *d_n_out (uint64, device) = the full count even when it exceeds `capacity`.  The order is unspecified
 * (Map::landmarks_ is an unordered_map too): sort by (map, ix, iy, iz) to compare. */
int vslam_voxel_extract_dev(vslam_ctx* ctx, vslam_voxel_map* vm, int map_id, int min_count, vslam_voxel* d_out, int32_t* d_map_out, size_t capacity,
                            uint64_t* d_n_out);

/* ------------------------------------------------------------------ surface map: disparities fused into a TSDF, free space carved --- */
/* The dense map above counts the points that fell into a voxel.  This stage keeps, per voxel, the truncated signed distance to the observed surface
 * averaged over every view that sees the voxel (a TSDF): views that look THROUGH a voxel vote "free" and carve what a wrong disparity or a passing
 * car left there, and the surface is the field's zero crossing, read back as one oriented point (surfel) per crossing voxel edge.  Every sum is an
 * integer and every voxel is written by one lane, so the map is bit-reproducible whatever order frames and blocks arrive in.  The reference has no
 * such map.  Additive: vslam_params and the ABI version are unchanged; the host mirror (host/) does not call the stage.
 *
 * CONSTANTS: vs = (double)(float)voxel_size and inv = 1.0f / (float)voxel_size (the dense map's two numbers), J = trunc_voxels in [1, 8],
 * tau = (double)J * vs, kq = 1024.0 / tau.  All f64 arithmetic below runs in the written order, no contraction.
 * BLOCKS: 8 x 8 x 8 voxels; block coordinate per axis = i >> 3 (arithmetic) of the voxel index i in [-2^17, 2^17);
 *   key = map_id << 45 | (bx + 2^14) << 30 | (by + 2^14) << 15 | (bz + 2^14),  map_id in [0, 1022] (all-ones is the empty slot).
 * A block is 512 voxels of four uint32 (W, Sq, Wc, I), voxel (ix, iy, iz) at (iz & 7) << 6 | (iy & 7) << 3 | (ix & 7): 8 KiB.  The pool holds
 * 2^log2_blocks blocks and is its own hash table (slot s owns block s): open addressing, linear probing over at most 128 slots.
 * ALLOCATION.  A frame b takes part when d_map_id[b] is in 0 .. 1022 and its pose is finite (its seven numbers, the rotation matrix and the inverse
 * translation formed from them).  Of such a frame every pixel (c, r) with c % step == 0 and r % step == 0: depth = fx * b / (double)d, kept when
 * z_min < depth < z_max (vslam_reproject_dev's gate: NaN, 0 and negative disparities fail it); for j = -J .. J, Zj = depth + (double)j * vs, skipped
 * when Zj <= 0; the world point is vslam_reproject_dev's expression with Zj in place of the depth (X = x * Zj, Y = y * Zj, f32 at rest); its voxel
 * index per axis is the dense map's floorf(p * inv), an axis out of range drops the sample (n_dropped_range); the block that holds it is claimed,
 * all zero, if no slot holds it yet.  A sample that finds no slot is dropped (n_dropped_full, status bit 0); which blocks are lost then depends on
 * the arrival order, what the claimed ones hold does not.
 * INTEGRATION, after the call's allocation is complete: every claimed block whose map id equals d_map_id[b] -- blocks of earlier calls included,
 * that is what carves them; a block a LATER call claims does not receive this call's frames -- with every voxel (ix, iy, iz) of it, for every frame b
 * of the call that takes part:
 *   Xw = ((double)i + 0.5) * vs per axis;  P = R Xw + t with R = the rotation matrix of T_c_w[b] (P[a] = R[3a] X0 + R[3a+1] X1 + R[3a+2] X2 + t[a])
 *   skip unless P[2] > vs
 *   u = fx * (P[0] / P[2]) + cx;  v = fy * (P[1] / P[2]) + cy;  c = floor(u + 0.5), r = floor(v + 0.5);  skip unless 0 <= c < w and 0 <= r < h
 *   z = fx * b / (double)disparity[b][r][c];  skip unless z_min < z < z_max
 *   sdf = z - P[2];  skip if sdf < -tau   (behind the surface: no information)
 *   q = (int)rint(fmin(sdf, tau) * kq), in [-1024, 1024]
 *   W += 1;  Sq += q + 1024;  if (sdf <= tau) { Wc += 1;  I += gray[b][r * pitch + c]; }
 * `step` thins the allocation only.  The sums are exact while W < 2^20; an extraction that meets a larger W sets status bit 1 and skips the voxel.
 * RE-INTEGRATION (vslam_tsdf_reintegrate_dev): a frame taken out of the field at the pose it went in with and put in at a corrected one.  The sums above
 * are plain integer sums -- no running average, no clamp, no weight cap at integration time -- so taking a frame out is INTEGRATION's rule subtracted,
 * exactly.  A frame may only be subtracted from the blocks it was added to.  Blocks enter the block list in claim order, so the blocks a call's frames
 * reached are the list positions [0, n) with n the claimed-block count after that call's allocation: the frame's REACH (vslam_tsdf_reach_dev after the
 * integrate call).  A frame b takes part when d_map_id[b] is in 0 .. 1022; its OLD side takes part when T_old[b] is finite by ALLOCATION's test, its NEW
 * side when T_new[b] is.  An all-NaN old pose makes the frame a plain integration, an all-NaN new pose a removal; a pose that is not finite is how a side
 * is switched off: it does not count in n_frames_skipped and does not set status bit 2.  With n0 the claimed-block count before the call:
 *   Allocation: ALLOCATION's rule over the NEW sides only (same disparity, gates and step).
 *   Accumulation, for every claimed block of the frame's map -- those this call just claimed included -- and every voxel: add = the sum of INTEGRATION's
 *   four contributions over the NEW sides, operation for operation as INTEGRATION evaluates them, at T_new; sub = the same sum over the OLD sides at
 *   T_old, counting only frames with (list position of the block) < min(reach[b], n0).
 *   Update: if every one of the four stored sums is >= its component of sub, the voxel becomes stored + add - sub (one read-modify-write per voxel and
 *   call).  Otherwise the voxel keeps its stored value -- neither side is applied -- and status bit 3 is set: the call was given a disparity, pose,
 *   gate or reach that is not the one the frame went in with.
 * What follows: the caller passes the same disparity, gray image, z_min, z_max and old pose BYTES the frame was integrated with; `step` thins the
 * allocation only and need not match.  Blocks whose voxels all return to zero stay claimed (linear probing has no deletion here); no voxel of them is
 * good, so extraction, mesh and render do not see them.  After vslam_tsdf_load_blocks_dev the reach of frames integrated before the dump is not
 * recoverable (the loader's claim order is its own).  The 2^20 weight limit applies to the sums as stored after the update.
 * EXTRACTION: num(v) = (int64)Sq - 1024 * W, D(v) = (double)num / (double)W; good(v): v lies in a claimed block, max(min_weight, 1) <= W < 2^20 and
 * Wc >= 1.  For a good voxel a and each axis e, with b = a + e (in whichever block): the edge crosses when b is good and (num_a > 0) != (num_b > 0).
 *   t = D_a / (D_a - D_b);  position along e = ((double)i_a + 0.5 + t) * vs, the other two axes ((double)i + 0.5) * vs
 *   gradient: g_e = D_b - D_a;  for each other axis f, g_f = the mean over c in {a, b} (in this order, summed from 0) of (D(c + f) - D(c - f)) / 2
 *   over those c whose two f-neighbours are good, 0 if there are none;  normal = g / sqrt(gx * gx + gy * gy + gz * gz): it points into free space
 *   intensity = ((double)I_a + (double)I_b) / ((double)Wc_a + (double)Wc_b);  weight = min(W_a, W_b);  every float is f64 arithmetic cast once.
 * These are the vertices marching cubes places; vslam_tsdf_mesh_dev connects them:
 * MESH.  The cell of voxel c = (ix, iy, iz) has the corners c + (dx, dy, dz), numbered dx + 2 dy + 4 dz.  It is meshable when all eight corners are good
 * (the predicate above, with the call's min_weight); cube = the sum of 2^corner over the corners with num > 0.  A cell that is not meshable emits nothing.
 *   Cube edge k = 4 e + p + 2 q (e the axis, f = (e + 1) % 3, g = (e + 2) % 3) runs from corner p f^ + q g^ along e^.  It crosses when its two corners
 *   differ in sign; its vertex is then EXTRACTION's surfel (c + p f^ + q g^, axis e): no new arithmetic.
 *   Segments: on each of the six faces 0, 2 or 4 edges cross.  Two: one segment joins them.  Four (two positive corners on a diagonal): two segments,
 *   each joining the two face edges that meet at one positive corner -- the positive corners are cut apart, the negative ones stay joined.  A segment
 *   A -> B is directed so that n . ((m_B - m_A) x (P - m_A)) > 0, n the face's outward normal, m the edge midpoints, P a positive corner of the face on
 *   the segment's side (with two crossings any positive corner of the face, with four the one it cuts off).  The rule reads the face's own four signs
 *   only, so the two cells that share a face draw the same segments and the mesh has no cracks.
 *   Loops: every crossing edge now has one successor, so the crossing edges fall into loops.  A loop is rotated to start at its lowest-numbered member
 *   from which no fan diagonal joins two edges of one cube face (a triangle flat in a face would coincide with a neighbour's); loops are ordered by
 *   their smallest member; each is fanned (l0, l_i, l_i+1).  Triangles are counter-clockwise seen from free space: (v1 - v0) x (v2 - v0) points towards
 *   growing D, as the surfel normals do.  Degenerate triangles (a vertex at t = 0 or 1) are kept.  256 rows, at most 5 triangles each, 820 in all;
 *   row 1 is (0, 8, 4), row 254 is (0, 4, 8).  tools/gen_mc_table.py derives the table (csrc/mc_table.inc) from this paragraph. */
typedef struct vslam_tsdf_map vslam_tsdf_map;
struct vslam_tsdf_stats {
    uint64_t n_blocks;          /* claimed blocks                                                     */
    uint64_t n_samples;         /* allocation samples that found or claimed their block               */
    uint64_t n_dropped_range;   /* samples dropped for range                                          */
    uint64_t n_dropped_full;    /* samples dropped because no slot was left                           */
    uint64_t n_frames_skipped;  /* frames with a map id whose pose was not finite                     */
    uint64_t n_pairs_visited;   /* (block, frame) pairs of equal map id the integration has looked at */
    uint64_t n_pairs_kept;      /* ... of which the cull kept                                         */
    uint32_t status;            /* bit 0: pool full; bit 1: a weight reached 2^20; bit 2: a frame was skipped for its pose; bit 3: a re-integration met a sum below what it was to take out; bit 4: a distance layer found no slot for a block and is void */
    int32_t struct_size;        /* sizeof(struct vslam_tsdf_stats) of the caller's header: set by the caller, checked */
};
typedef struct vslam_surfel {   /* one zero-crossing voxel edge (48 bytes) */
    int32_t ix, iy, iz;         /* the edge's lower voxel a */
    uint32_t axis;              /* 0, 1, 2: the edge runs from a to a + 1 along x, y, z */
    uint32_t weight;
    float x, y, z, nx, ny, nz, intensity;
} vslam_surfel;

/* An empty map of 2^log2_blocks blocks (log2_blocks in [6, 22]) of voxels of voxel_size (finite, > 0), truncation trunc_voxels in [1, 8].  Its
 * bytes -- 8 KiB + 12 + 8 * ceil(max_batch / 64) per block, 128 per frame of max_batch -- are counted in vslam_device_bytes while the handle lives.
 * A map belongs to its context and is destroyed before it.  Synchronous. */
int vslam_tsdf_create(vslam_ctx* ctx, double voxel_size, int trunc_voxels, int log2_blocks, vslam_tsdf_map** out);
void vslam_tsdf_destroy(vslam_tsdf_map* tm);
/* every slot empty, every voxel and counter zero; asynchronous on the context stream */
int vslam_tsdf_clear(vslam_tsdf_map* tm);
/* the counters so far (host->struct_size set by the caller); synchronises the context stream */
int vslam_tsdf_stats(vslam_tsdf_map* tm, struct vslam_tsdf_stats* host);
/* Allocation and integration of B frames as above (the arguments and refusals of vslam_voxel_fuse_disparity_dev; d_gray NULL: I stays 0).
 * Two forms, same sums (vslam_set_tuning "tsdf_form"): 0 = every block walks all frames of the call; 1 = a cull kernel writes a frame mask per block
 * first.  Either skips a (block, frame) pair only when no voxel of the block can pass the rule. */
int vslam_tsdf_integrate_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                             int w, int h, int B, const double* d_T_c_w, const int32_t* d_map_id, double z_min, double z_max, int step);
/* The number of blocks claimed so far into *d_out (uint32, device, 4-byte aligned), asynchronously on the context stream: called after an integrate or
 * re-integrate call it yields that call's reach (RE-INTEGRATION) without a host round trip. */
int vslam_tsdf_reach_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, uint32_t* d_out);
/* RE-INTEGRATION of B frames: the arguments and refusals of vslam_tsdf_integrate_dev with two pose arrays (B x 7 each) and d_reach (B uint32: the reach
 * each frame went in with; a value above the list length counts as n0).  A null d_T_old, d_T_new or d_reach with B > 0 is refused; B == 0 is a no-op
 * that succeeds.  Both forms of "tsdf_form" give the same sums: 0 walks the old sides, then the new sides per block; 1 writes two frame masks per block
 * first, the old one with the reach test folded in.  n_pairs_visited / n_pairs_kept count both sides (an old side is visited where its reach admits the
 * block).  The first call on a map grows the old sides' tables -- 128 bytes per frame of max_batch and 8 * ceil(max_batch / 64) per block, counted in
 * vslam_device_bytes -- which synchronises the context stream; the kernels are asynchronous on it. */
int vslam_tsdf_reintegrate_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const float* d_disparity, const uint8_t* d_gray, size_t img_bytes, int pitch,
                               int w, int h, int B, const double* d_T_old, const double* d_T_new, const int32_t* d_map_id,
                               const uint32_t* d_reach, double z_min, double z_max, int step);
/* The crossing edges of map map_id (-1: every map) into d_out (`capacity` vslam_surfel, 16-byte aligned) and, when given, their map ids into
 * d_map_out; *d_n_out (uint64, device) = the full count even when it exceeds `capacity`.  The order is unspecified: sort by (map, ix, iy, iz, axis). */
int vslam_tsdf_extract_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int min_weight, vslam_surfel* d_out, int32_t* d_map_out, size_t capacity,
                           uint64_t* d_n_out);
/* The claimed blocks of map map_id (-1: every map), raw: (map, bx, by, bz) into d_block_out (`capacity` x 4 int32) and the block's 512 x 4 uint32 into
 * d_voxels_out (both 16-byte aligned); *d_n_out as above.  For tests and tools. */
int vslam_tsdf_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int32_t* d_block_out, uint32_t* d_voxels_out, size_t capacity,
                          uint64_t* d_n_out);
/* The mesh of map map_id (-1: every map) by the MESH rule.  The vertices are exactly the surfels vslam_tsdf_extract_dev returns for the same arguments
 * (same set, same bytes, order unspecified) into d_vertices (`vertex_capacity` vslam_surfel, 16-byte aligned) and, when given, their map ids into
 * d_vertex_map; the triangles into d_triangles (`triangle_capacity` x 3 int32 indices into this call's vertex array).  d_counts (two uint64, device) =
 * the full vertex and triangle counts even when they exceed the capacities; nothing is stored at or beyond a capacity; NULL buffers with capacity 0
 * make a counting call.  Triangle indices are meaningful when counts[0] <= vertex_capacity.  The first call on a map grows the map's vertex-id table
 * -- (1536 * claimed blocks + 2^log2_blocks) * 4 bytes, counted in vslam_device_bytes -- for which the call reads the block count (one synchronise of
 * the context stream); the kernels are asynchronous on the context stream.  A min_weight below 1 counts as 1, as in the extraction. */
typedef struct vslam_triangle { int32_t v[3]; } vslam_triangle;   /* 12 bytes: indices into the call's vertex array */
int vslam_tsdf_mesh_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int min_weight, vslam_surfel* d_vertices, int32_t* d_vertex_map,
                        size_t vertex_capacity, vslam_triangle* d_triangles, size_t triangle_capacity, uint64_t* d_counts);
/* The inverse of vslam_tsdf_blocks_dev: each of the n listed blocks (d_block_ids n x 4 int32 of (map, bx, by, bz), d_voxels n x 512 x 4 uint32, both
 * 16-byte aligned) is claimed if it is absent and its 512 voxels are replaced.  An id outside map 0 .. 1022 or coordinates [-2^14, 2^14) is refused
 * per block: it counts in n_dropped_range and nothing is written for it.  A block that finds no slot counts in n_dropped_full and sets status bit 0.
 * The ids of one call must be distinct (with duplicates, which copy stays is unspecified).  Asynchronous on the context stream. */
int vslam_tsdf_load_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const int32_t* d_block_ids, const uint32_t* d_voxels, size_t n);
/* RENDER.  What a camera at a given pose sees of the field: a depth image and, per pixel, the surface normal and intensity, ray-cast on the device.
 * All arithmetic is f64 in the written order, no contraction, and every float is cast once at the end.  The call carries a camera fx, fy, cx, cy and
 * an image size w, h of its own (not the context's: a caller renders at any scale), z_min < z_max, march and min_weight.  vs as above, hs = march * vs,
 * K = the smallest non-negative integer with z_min + (double)K * hs >= z_max (the host computes it with exactly that expression), sample k of 0 .. K-1
 * lies at Z_k = z_min + (double)k * hs.  A view v takes part when d_map_id[v] is in 0 .. 1022 and its pose is finite (ALLOCATION's test: the seven
 * numbers, the rotation matrix, the inverse translation); every pixel of a view that does not take part is a miss.
 *   The ray of pixel (c, r): x = ((double)c - cx) / fx, y = ((double)r - cy) / fy; like INTEGRATION's distance it is parametrised by the camera's z.
 *   The sample at depth Z: P = (x * Z, y * Z, Z); Xw[a] = Rinv[3a] * P0 + Rinv[3a+1] * P1 + Rinv[3a+2] * P2 + tinv[a] with Rinv = the transposed rotation
 *   matrix and tinv[a] = -(Rinv[3a] * t0 + Rinv[3a+1] * t1 + Rinv[3a+2] * t2) (vslam_reproject_dev's inverse pose); g[a] = Xw[a] / vs - 0.5,
 *   i[a] = floor(g[a]), f[a] = g[a] - (double)i[a].  The sample is UNKNOWN unless every axis has -2^17 <= i[a] and i[a] + 1 < 2^17 and all eight voxels
 *   i + (dx, dy, dz) of the view's map are good (EXTRACTION's predicate with the call's min_weight: a weight at 2^20 is not good, a min_weight below 1
 *   counts as 1).  Otherwise, with lerp(a, b, t) = a + t * (b - a) and D(dx, dy, dz) EXTRACTION's D of the corner:
 *     Dx[dy][dz] = lerp(D(0, dy, dz), D(1, dy, dz), f0);  Dy[dz] = lerp(Dx[0][dz], Dx[1][dz], f1);  D = lerp(Dy[0], Dy[1], f2)
 *     gradient, the analytic one of that interpolant -- the corner differences along an axis, lerped over the other two axes in the order x, y, z:
 *       gx = lerp(lerp(X00, X10, f1), lerp(X01, X11, f1), f2) with Xyz = D(1, y, z) - D(0, y, z)
 *       gy = lerp(lerp(Y00, Y10, f0), lerp(Y01, Y11, f0), f2) with Yxz = D(x, 1, z) - D(x, 0, z)
 *       gz = lerp(lerp(Z00, Z10, f0), lerp(Z01, Z11, f0), f1) with Zxy = D(x, y, 1) - D(x, y, 0)
 *     intensity: D's trilinear form over the corners' (double)I / (double)Wc.
 *   The march walks k = 0, 1, ... and keeps prev = "sample k-1 was known and had D > 0" with its D_prev.  An unknown sample clears prev; a known sample
 *   with D > 0 sets it; the first known sample with D <= 0 ends the ray (an exact zero counts as not positive, as in the mesh): a HIT if prev is set,
 *   otherwise a miss -- a back face, or a surface entered from unobserved space, is not rendered.  A ray that reaches K without ending is a miss.
 *   Hit: s = D_prev / (D_prev - D);  Z* = (z_min + (double)(k - 1) * hs) + s * hs;  depth = (float)Z*.  The attributes come from one more sample at Z*,
 *   or from sample k if that one is unknown: n = gradient / sqrt(gx * gx + gy * gy + gz * gz), in the world frame, pointing into free space as the surfel
 *   normals do, (0, 0, 0) if the norm is zero or not finite; the intensity of the same sample.  Stored: (float)nx, (float)ny, (float)nz, (float)intensity.
 *   Miss: the depth is 0.0f and the attributes are four 0.0f.
 * Two forms, same bytes (vslam_set_tuning "tsdf_render_form"): 0 = every ray walks all K samples; 1 = a range kernel first projects a sphere around every
 * claimed block onto the view's 16 x 16 pixel tiles and narrows each tile's walk to the samples that can be known.  d_counts, when given, receives the
 * rays that hit and the samples the march evaluated (the second depends on the form; attribute samples are not counted). */
struct vslam_tsdf_render_params {
    int32_t struct_size;   /* sizeof(struct vslam_tsdf_render_params) of the caller's header: set by the caller, checked */
    int32_t w, h;
    double fx, fy, cx, cy, z_min, z_max, march;
    int32_t min_weight, reserved;
};
/* V views of the map by the RENDER rule: d_T_c_w V x 7 poses, d_map_id V map ids (outside 0 .. 1022: the view is all misses), d_depth V x h x w floats,
 * d_attr V x h x w x 4 floats of (nx, ny, nz, intensity), 16-byte aligned, or NULL, d_counts NULL or two uint64 (8-byte aligned).  Every pixel of every
 * view is written, nothing beyond V * h * w (4 V h w) floats.  Asynchronous on the context stream; V == 0 is a no-op that succeeds; a call that needs
 * larger view / range tables than the map holds (128 bytes per view, with form 1 eight more per view and tile; counted in vslam_device_bytes) grows them
 * first, which synchronises the context stream.  VSLAM_ERR_ARG: a null map or a map of another context, a wrong struct_size, w or h below 1, V < 0,
 * V * h * w >= 2^31, fx or fy not finite or <= 0, cx or cy not finite, z_min not finite or <= 0, z_max not finite or <= z_min, march not finite or
 * outside [1/8, 1], K > 8192, a null d_T_c_w, d_map_id or d_depth with V > 0, a misaligned pointer. */
int vslam_tsdf_render_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const struct vslam_tsdf_render_params* params, int V, const double* d_T_c_w,
                          const int32_t* d_map_id, float* d_depth, float* d_attr, uint64_t* d_counts);
/* DISTANCE.  How far a point is from the nearest surface of the map: a layer of squared Euclidean distances over the field, built on the device, and
 * point queries against it.  All quantities are integers except the last step of a query, so the layer is exact, independent of the order the blocks
 * arrived in and reproducible to the byte.
 *   good(v) is EXTRACTION's predicate with the call's min_weight (below 1 counts as 1; a weight at 2^20 is not good), num(v) as there.
 *   CLASS of a voxel: 0 UNKNOWN (not good, or in no claimed block), 1 FREE (good and num > 0), 2 OCCUPIED (good and num <= 0: an exact zero is not
 *   positive, as in MESH and RENDER).
 *   SITE: an OCCUPIED voxel with at least one of its six face neighbours, in whichever block of the same map, FREE -- the non-positive end of every
 *   crossing edge of EXTRACTION, nothing else.
 *   d2(v), for any voxel index v in [-2^17, 2^17)^3: the minimum over the sites s of the same map of |v - s|^2, an integer in voxel units; FAR if that
 *   minimum exceeds R^2 or the map has no site.  R = radius_voxels in [1, 16], so d2 <= 256.  Sites of different maps never see each other.
 *   CELL WORD (uint16): bits 0-11 d2, 0xFFF = FAR; bits 12-13 the class; bits 14-15 zero.
 *   LAYER of a build call: every block with coordinates in [-2^14, 2^14) that (a) is claimed in the pool for a map the call covers, or (b) holds at
 *   least one voxel with d2 != FAR.  Blocks of kind (b) are in general NOT claimed in the pool; their voxels are UNKNOWN.  A block is 512 cell words
 *   in EXTRACTION's voxel order: 1 KiB.  A build with map_id >= 0 covers that map alone: no block of another map is in the layer.
 *   QUERY of a world point Xw (three f64) in map m: i[a] = floor(Xw[a] / vs) in f64, in the written order, no contraction.  Class 3 INVALID with
 *   dist = +INFINITY when m is outside 0 .. 1022, a coordinate is not finite or an index is outside [-2^17, 2^17).  Otherwise the cell word is the
 *   voxel's; a block outside the layer reads as FAR | UNKNOWN.  dist = (float)(sqrt((double)d2) * vs), negated when the class is OCCUPIED and d2 > 0;
 *   FAR gives +INFINITY, or -INFINITY when OCCUPIED.  The voxel is the NEAREST one: one sample per query, no interpolation, so the distance is that
 *   between voxel centres and moves in steps.
 * The layer lives in the map handle: a key table and cell pool of its own of 2^log2_layer_blocks blocks with the build's scratch, 2257 bytes per block
 * and 64 more, counted in vslam_device_bytes and released by vslam_tsdf_destroy.  It is grown by the first build or by a larger request, which
 * synchronises the context stream; the build itself is asynchronous on that stream and replaces any earlier layer of the handle.  The pool is not
 * written.  Before anything is computed the build claims, in the layer's table, every claimed block of the covered maps and every block within
 * ceil(R / 8) blocks per axis of a block that holds a site (coordinates outside [-2^14, 2^14) are dropped, never wrapped); one of these that finds no
 * slot -- the table is full, or for tables of 128 slots or more no free slot lies within 128 probes -- makes the whole layer VOID: status bit 4 of
 * vslam_tsdf_stats is set (it stays set until vslam_tsdf_clear), vslam_tsdf_distance_blocks_dev writes a count of 0, every valid query answers
 * FAR | UNKNOWN and the build's counts are (sites, 0, 0).  Nothing is half-served.
 * The layer is a snapshot: vslam_tsdf_integrate_dev, vslam_tsdf_reintegrate_dev (with B > 0), vslam_tsdf_load_blocks_dev and vslam_tsdf_clear make it
 * stale, and the two readers below refuse a map whose layer is missing or stale (VSLAM_ERR_ARG, "distance layer not built or older than the map").
 * Two forms, same bytes (vslam_set_tuning "tsdf_dist_form"): 0 = every voxel takes the minimum over the site masks of the blocks around it; 1 = the
 * separable exact transform, three passes along x, y and z. */
struct vslam_tsdf_distance_params {
    int32_t struct_size;         /* sizeof(struct vslam_tsdf_distance_params) of the caller's header: set by the caller, checked */
    int32_t map_id;              /* 0 .. 1022, or -1: every map */
    int32_t min_weight;
    int32_t radius_voxels;       /* [1, 16] */
    int32_t log2_layer_blocks;   /* [6, 24] */
    int32_t reserved;
};
/* Builds the layer by the DISTANCE rule.  d_counts: NULL, or three uint64 (device, 8-byte aligned): the sites, the layer's blocks, and those of them
 * that the pool does not hold for a covered map (kind (b) only).  An empty map succeeds with an empty layer.  VSLAM_ERR_ARG: a null map or a map of
 * another context, null params or a wrong struct_size, map_id outside [-1, 1022], radius_voxels outside [1, 16], log2_layer_blocks outside [6, 24], a
 * misaligned d_counts. */
int vslam_tsdf_distance_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const struct vslam_tsdf_distance_params* params, uint64_t* d_counts);
/* The layer's blocks of map map_id (-1: every map the build covered): (map, bx, by, bz) into d_block_out (`capacity` x 4 int32) and the block's 512 cell
 * words into d_cells_out (`capacity` x 512 uint16), both 16-byte aligned; *d_n_out (uint64, device) = the full count even when it exceeds `capacity`;
 * nothing is stored at or beyond it; the order is unspecified.  A block the build claimed that ended all FAR and is not claimed in the pool is not
 * emitted.  Asynchronous on the context stream.  VSLAM_ERR_ARG: a null or foreign map, a null d_n_out, a null output with a capacity, map_id outside
 * [-1, 1022], a misaligned pointer, a missing or stale layer. */
int vslam_tsdf_distance_blocks_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, int map_id, int32_t* d_block_out, uint16_t* d_cells_out, size_t capacity,
                                   uint64_t* d_n_out);
/* N point queries by the DISTANCE rule: d_xyz_w N x 3 f64 world points, d_map_id N map ids, d_dist N floats, d_class N bytes (0 .. 3).  Asynchronous on
 * the context stream; N == 0 succeeds.  VSLAM_ERR_ARG: a null or foreign map, a null pointer with N > 0, a misaligned pointer, a missing or stale layer. */
int vslam_tsdf_distance_query_dev(vslam_ctx* ctx, vslam_tsdf_map* tm, const double* d_xyz_w, const int32_t* d_map_id, size_t N, float* d_dist,
                                  uint8_t* d_class);

/* ------------------------------------------------------------------ place database: loop-closure candidates and verified edges --- */
/* Noticing that the camera is back at a place it has seen: keyframe descriptor blocks are kept in a database that outlives the steps (loops close
 * over thousands of frames, a batch holds max_batch), every query entry is scored against every earlier entry of its sequence by brute force over the
 * raw descriptors on the matrix cores -- no vocabulary, nothing trained -- and the best candidates are verified with the library's own matcher and
 * RANSAC pose stage, which also yields the relative pose the pose-graph stage below consumes.  The reference has no loop closure.  Additive: vslam_params and
 * the ABI version are unchanged; the host mirror (host/) does not call the stage.
 *
 * SCORE of query entry i (descriptor rows D_i, n_i of them) against entry j, all integer, hence exact and independent of arrival order:
 *   score(i, j) = #{ r < n_i : min_c hamming(D_i[r], D_j[c]) <= tau }      (asymmetric; 0 when n_j = 0)
 * The pair is ELIGIBLE when seq_j == seq_i and frame_j <= frame_i - min_gap; a pair that is not eligible scores -1 and costs no matrix work.
 * ENTRY: rows_per_entry R <= 4096 (the matcher's row limit); its first min(n, R) descriptor rows at a stride of R rounded up to 32 rows (every block
 * 16-byte aligned, the matcher's contract), seq, frame and, with geometry, per keypoint row the pixel (x, y of vslam_keypoint), the camera-frame point,
 * its valid flag, and the ascending list of the rows that own a valid point (the d_qsel / d_nqsel of vslam_feature_matching_pairs_dev).  Entry ids are
 * dense and ascending in the order of the adds. */
typedef struct vslam_place_db vslam_place_db;
struct vslam_place_stats {
    int32_t n_entries;         /* entries held                                      */
    int32_t capacity;          /* entries the database can hold                     */
    int32_t rows_per_entry;    /* R                                                 */
    int32_t with_geometry;     /* 1 when pixels / points / valid rows are kept      */
    uint64_t n_refused;        /* vslam_place_add_dev calls refused for lack of room */
    int32_t struct_size;       /* sizeof(struct vslam_place_stats) of the caller's header: set by the caller, checked */
};
/* An empty database of capacity_entries (>= 1) entries of rows_per_entry (1 .. 4096) rows.  Its bytes are counted in vslam_device_bytes while the
 * handle lives.  A database belongs to its context and is destroyed before it.  Synchronous. */
int vslam_place_create(vslam_ctx* ctx, int rows_per_entry, int capacity_entries, int with_geometry, vslam_place_db** out);
void vslam_place_destroy(vslam_place_db* db);
/* forgets every entry and zeroes the refusal counter (host bookkeeping only: nothing on the device is read before it is written again) */
int vslam_place_clear(vslam_place_db* db);
int vslam_place_stats(vslam_place_db* db, struct vslam_place_stats* host);
/* Entry `entry` as the database holds it, into host buffers (diagnostic, and the way to persist a database; synchronises the context stream):
 * meta[4] = {n, seq, frame, valid rows (0 without geometry)}; desc (R x 32 bytes; rows at or past n are zero); with geometry also xy (R x 2 f32),
 * xyz (R x 3 f32), valid (R uint8) and qsel (R int32, the first meta[3] defined).  Every buffer but meta may be NULL: not wanted. */
int vslam_place_read_entry(vslam_place_db* db, int entry, int32_t* meta, uint8_t* desc, float* xy, float* xyz, uint8_t* valid, int32_t* qsel);
/* n, seq and frame (count int32 each, host; any may be NULL) of entries [first, first + count); synchronises the context stream */
int vslam_place_read_meta(vslam_place_db* db, int first, int count, int32_t* n, int32_t* seq, int32_t* frame);

/* Every entry below refuses with VSLAM_ERR_ARG and a message before it launches anything: a null pointer where one is required, a range outside the
 * entries held, ld below the number of entries, a database of another context.
 *
 * vslam_place_add_dev: appends item b of a batch (B >= 1) when d_add[b] != 0 (d_add NULL: every item), in ascending b: the first min(d_n[b], R) rows of
 * d_desc + b * desc_stride_bytes (both multiples of 16 bytes), d_seq[b] and d_frame[b]; with geometry also d_kps / d_xyz (x 3) / d_valid at
 * [b * kp_capacity, ...), all required then (rows at or past kp_capacity own no point).  *first_entry (may be NULL) = the id of the first entry added
 * (the entry count when none was).  An add that does not fit adds NOTHING: VSLAM_ERR_CAPACITY, counted in n_refused.  The call reads d_add on the host
 * (it synchronises the context stream); the copies are asynchronous on it. */
int vslam_place_add_dev(vslam_ctx* ctx, vslam_place_db* db, const uint8_t* d_desc, size_t desc_stride_bytes, const int32_t* d_n, const int32_t* d_add,
                        const int32_t* d_seq, const int32_t* d_frame, const vslam_keypoint* d_kps, const float* d_xyz, const uint8_t* d_valid, int kp_capacity,
                        int B, int* first_entry);
/* d_score (nq x ld int32, ld >= the entry count; columns at or past the entry count are not touched): the score of query entries [q0, q0 + nq),
 * nq in 1 .. 65535, against every entry, tau in [0, 255].  Asynchronous; the same call twice writes the same bytes. */
int vslam_place_score_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, int tau, int min_gap, int32_t* d_score, int ld);
/* Per query of a score table the K (1 .. 8) eligible entries with the highest score that reach min_score, into d_cand / d_cand_score (nq x K int32):
 * descending score, ties to the smaller entry id; unused slots -1 / 0. */
int vslam_place_select_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, const int32_t* d_score, int ld, int K, int min_score, int32_t* d_cand,
                           int32_t* d_cand_score);
/* Geometric verification of query b's (entry q0 + b, nq <= max_batch) rank-`rank` candidate c = d_cand[b * K + rank] on a database with geometry:
 * (1) vslam_feature_matching_pairs_dev with entry c's block and its valid rows as the query side (d_qitem[b] = c), entry q0 + b's descriptors as the
 * train side, gate = 1 at gap 1.0; (2) a gather, in match order, of (point of c at queryIdx, pixel of entry q0 + b at trainIdx); (3)
 * vslam_pnp_ransac_dev with the context's pnp_reproj_thr, 100 iterations, confidence 0.99 (visual_odometry.cpp:277).  d_T_q_c (nq x 7) is that call's
 * T_c_w with "world" = candidate c's camera: the relative pose of a loop edge.  d_n_matches / d_n_inliers (nq int32).  An edge is ACCEPTED when
 * n_inliers >= min_inliers (>= 0; 10 is VO::check_motion_estimation's minimum, visual_odometry.cpp:319; its relative-motion limit does not apply to a
 * loop edge).  A query without a candidate (-1) gives identity / 0 / 0; one with fewer matches than min_inliers cannot be accepted and is not handed
 * to RANSAC: identity, its match count, 0 inliers.  Asynchronous; uses the context's matcher and RANSAC scratch. */
int vslam_place_verify_dev(vslam_ctx* ctx, vslam_place_db* db, int q0, int nq, const int32_t* d_cand, int K, int rank, int min_inliers, double* d_T_q_c,
                           int32_t* d_n_matches, int32_t* d_n_inliers);

/* ------------------------------------------------------------------ pose-graph optimisation: loop edges correct the trajectory --- */
/* What consumes the edges of the place database: a batch of n_graphs independent pose graphs, laid back to back (graph g owns nodes
 * [node_off[g], node_off[g+1]) and edges [edge_off[g], edge_off[g+1])), each optimised by one persistent workgroup through all its Levenberg-Marquardt
 * iterations.  The reference has no pose graph.  Additive: vslam_params and the ABI version are unchanged; the host mirror (host/) does not call it.
 *
 * PROBLEM.  Node k holds T_k = T_c_w (7 doubles, quaternion x, y, z, w then translation).  An edge is (i, j, Z, w[6]) with GRAPH-LOCAL node ids
 * i != j: Z measures T_i o T_j^-1 (p_i = Z p_j: the T_q_c of a loop edge with i = q, j = c), w is a diagonal information in tangent order
 * [upsilon; omega], finite and >= 0.  Residual r = log(Z^-1 o T_i o T_j^-1), cost = sum r' diag(w) r over the ACTIVE edges.  Update T <- exp(delta) o T.
 * With E = Z^-1 T_i T_j^-1 and A = I - ad(r)/2 + ad(r)^2/12:  dr/d delta_i = A Ad(Z^-1),  dr/d delta_j = -A Ad(E).
 * GAUGE.  d_fixed[k] != 0 holds node k; NULL holds node 0 of every graph.  A node without an active edge is held too (its block of H is zero).
 * LM.  (H + lambda diag(H)) delta = -g from lambda_init; a step is accepted when the cost falls, then lambda <- max(lambda / 10, 1e-12); a rejected
 * step gives lambda <- 10 lambda.  Stops at |delta| < step_tol, at lambda > 1e12, or at max_iters.  All arithmetic is f64.
 * SOLVER.  Preconditioned conjugate gradients, matrix-free over the edges, to |r| <= pcg_tol |b| or pcg_max_iters.  Two preconditioners
 * (vslam_set_tuning "pg_precond"): 0 = block-Jacobi (the 6 x 6 diagonal blocks); 1 = chain: the block-tridiagonal part of H + lambda diag(H), i.e. the
 * diagonal blocks and the blocks of the edges with |i - j| = 1, factorised and applied by a sequential block LDL' sweep; -1 = the library's rule
 * (DESIGN.md 5.10).  Nodes should therefore be numbered along the odometry chain.
 * DETERMINISM.  Node sums run over a per-node incidence list in ascending edge order, dot products in an order that depends on the graph's own node
 * and edge counts only, no floating-point atomics: the same call twice writes the same bytes, and a graph's output in a batch is bit for bit its
 * output alone.
 * SAFETY.  Every offset and node id is range-checked on the device.  A graph whose offsets are out of range or out of order is skipped entirely
 * (only its status word is written); one with a bad node id (outside [0, N) or i == j) or a non-finite pose, measurement or weight (or a negative
 * weight) has its poses copied through and its status bit set.  Degenerate graphs (0 or 1 node, no edges, every node held, a broken chain, a
 * component that reaches no held node) are results, not errors: finite output, status 0. */
#define VSLAM_PG_BAD_INDEX 1    /* an offset or node id out of range: graph skipped                              */
#define VSLAM_PG_NONFINITE 2    /* a non-finite pose / measurement / weight or a negative weight: graph skipped   */
#define VSLAM_PG_PCG_CAP 4      /* PCG reached pcg_max_iters in some step (the step is still a descent candidate) */
#define VSLAM_PG_LAMBDA 8       /* stopped because lambda exceeded 1e12                                           */
#define VSLAM_PG_SINGULAR 16    /* a diagonal block was not positive definite (zero weights): pivot replaced by 1 */
typedef struct vslam_pose_graph {
    int32_t struct_size;          /* sizeof(vslam_pose_graph): set by the caller, checked */
    int32_t n_graphs;
    int32_t total_nodes, total_edges;
    const int32_t* d_node_off;    /* n_graphs + 1 */
    const int32_t* d_edge_off;    /* n_graphs + 1 */
    const double* d_T;            /* total_nodes x 7, in */
    const uint8_t* d_fixed;       /* total_nodes, or NULL: node 0 of every graph */
    const int32_t* d_edge_i;      /* total_edges, graph-local */
    const int32_t* d_edge_j;      /* total_edges, graph-local */
    const double* d_edge_Z;       /* total_edges x 7 */
    const double* d_edge_w;       /* total_edges x 6 */
    const uint8_t* d_edge_active; /* total_edges, or NULL: all active */
    double* d_edge_chi2;          /* total_edges, out: r' diag(w) r of EVERY edge (inactive ones too) at the output poses; NULL = not wanted */
} vslam_pose_graph;
typedef struct vslam_pose_graph_params {
    int32_t struct_size;          /* sizeof(vslam_pose_graph_params) */
    int32_t max_iters;            /* LM iterations; 0 = evaluate only */
    int32_t pcg_max_iters;
    int32_t reserved;
    double pcg_tol;               /* relative residual */
    double step_tol;
    double lambda_init;
} vslam_pose_graph_params;
typedef struct vslam_pose_graph_stats {
    double chi2_init, chi2_final, lambda;
    int32_t lm_iters, pcg_iters, n_free, status;
} vslam_pose_graph_stats;
/* max_iters 50, pcg_max_iters 4000, pcg_tol 1e-10, step_tol 1e-9, lambda_init 1e-4 */
void vslam_pose_graph_default_params(vslam_pose_graph_params* p);
/* Optimises every graph of the batch: d_T_out (total_nodes x 7; may be d_T itself) and, when not NULL, d_stats (n_graphs) and graph->d_edge_chi2.
 * params NULL = the defaults.  max_iters = 0 evaluates only: chi2_init and the edge chi2 are written and the poses copied.  Refuses with
 * VSLAM_ERR_ARG and a message before it launches anything: a null where a pointer is required, negative counts, a wrong struct_size, parameters out
 * of range.  Asynchronous on the context stream; the state lives in a growable buffer of the context counted in vslam_device_bytes. */
int vslam_pose_graph_dev(vslam_ctx* ctx, const vslam_pose_graph* graph, const vslam_pose_graph_params* params, double* d_T_out,
                         vslam_pose_graph_stats* d_stats);
/* the status words of the n_graphs graphs of the most recent vslam_pose_graph_dev call, into h_status (host); synchronises the context stream */
int vslam_pose_graph_status_dev(vslam_ctx* ctx, int n_graphs, int32_t* h_status);

/* ------------------------------------------------------------------ full bundle adjustment: loop closing moves the map too -------- */
/* What follows the pose graph: all keyframes and all landmarks of a sequence over all their observations, with the loop edges as relative-pose
 * factors.  A batch of n_problems independent problems laid back to back (problem p owns keyframes [kf_off[p], kf_off[p+1]), landmarks
 * [lm_off[p], lm_off[p+1]), observations [obs_off[p], obs_off[p+1]) and edges [edge_off[p], edge_off[p+1])), each optimised by one persistent
 * workgroup through all its Levenberg-Marquardt iterations.  The reference has no such stage (its optimize_map sees ten keyframes).  Additive:
 * vslam_params and the ABI version are unchanged; the host mirror (host/) does not call it.
 *
 * PROBLEM.  Keyframe k holds T_k = T_c_w (7 doubles), landmark l holds X_l (3 doubles, world).  An observation is (kf, lm, uv, disp) with
 * PROBLEM-LOCAL ids, sorted by landmark inside a problem (non-decreasing lm: the rule of vslam_ba_batch).  With P = R_k X_l + t_k its residual is
 * e = [u - (fx Px / Pz + cx), v - (fy Py / Pz + cy)] (vo_projection_residual) and, when disp is valid, a third row d - bf / Pz.  disp is the stereo
 * disparity measured at that keypoint (fx b / Z of the keypoint's own stereo depth); a negative or NaN disp marks a left-image-only observation,
 * d_obs_disp NULL makes every observation one.  The stereo rows fix the scale: with them and one held keyframe the minimum is unique.
 * With A = de/dP = [[-fx/Pz, 0, fx Px/Pz^2], [0, -fy/Pz, fy Py/Pz^2], [0, 0, bf/Pz^2]]:  de/d delta_k = A [I, -P^],  de/dX_l = A R_k.
 * ROBUST KERNEL.  Huber on s = e'e of width huber_delta: rho = s for s <= delta^2, else 2 sqrt(s) delta - delta^2; the weight rho' multiplies
 * J'J and J'e (g2o's rule).  huber_delta = 0: none.
 * EDGES.  (i, j, Z, w[6]) between keyframes i != j: residual, Jacobians and meaning exactly those of vslam_pose_graph.  total_edges = 0 is allowed.
 * COST.  sum rho(e'e) over the ACTIVE observations + sum r' diag(w) r over the ACTIVE edges.  UPDATE.  T <- exp(delta) o T, X <- X + dX.
 * HELD.  d_fixed[k] != 0 holds keyframe k; NULL holds keyframe 0 of every problem.  A keyframe without an active observation and without an active
 * edge is held too.  A landmark without an active observation is copied through.
 * BEHIND THE CAMERA.  An active observation whose point has Pz <= 0 at the input state is inactive for this call and counted (n_obs_dropped,
 * VSLAM_FBA_DROPPED).  A trial state in which an active observation has Pz <= 0 costs infinity: the step is rejected.
 * LM.  The pose graph's rule: (H + lambda diag(H)) on the full system, before the elimination, from lambda_init; a step that lowers the cost is
 * accepted, then lambda <- max(lambda / 10, 1e-12); a rejected step gives lambda <- 10 lambda.  Stops at |delta| < step_tol (poses and points
 * together), at lambda > 1e12 or at max_iters.  All arithmetic is f64.
 * SOLVER.  The landmarks are eliminated (3 x 3 blocks V_l, closed-form inverse); the reduced camera system S = U + edges - W V^-1 W' is solved by
 * preconditioned conjugate gradients that never form it, to |r| <= pcg_tol |b| or pcg_max_iters; the preconditioner is block-Jacobi, the 6 x 6
 * blocks U_k + edges - sum_o W_o V^-1 W_o' (the diagonal blocks of S when no keyframe observes a landmark twice); then the landmarks are
 * back-substituted.  A damped V_l that is not positive definite holds that landmark for the iteration (VSLAM_FBA_SINGULAR); so does a diagonal
 * block of the preconditioner, whose pivot is replaced by 1.
 * DETERMINISM.  As the pose graph: keyframe sums walk a per-keyframe incidence list in ascending observation order, landmark sums their
 * observations in ascending order, dot products in an order that depends on the problem's own counts only, no floating-point atomics.  The same
 * call twice writes the same bytes, and a problem's output in a batch is bit for bit its output alone.
 * SAFETY.  Every offset is checked on the device for range, order and disjointness, every keyframe and landmark id for range, the landmark order
 * of the observations, and every pose, point, measurement and weight for finiteness (a +inf disp is non-finite; weights must be >= 0).  A problem
 * with a bad offset is skipped entirely (only its status word is written); one with a bad id, a broken landmark order or a non-finite value has
 * its poses and points copied through and its status bit set.  Its neighbours are untouched.  Degenerate problems (no observations, one keyframe,
 * every keyframe held, a keyframe without observations, a landmark seen once) are results: finite output. */
#define VSLAM_FBA_BAD_INDEX 1   /* an offset, a keyframe / landmark id out of range, or observations not sorted by landmark: problem skipped */
#define VSLAM_FBA_NONFINITE 2   /* a non-finite pose / point / measurement / weight or a negative weight: problem passed through              */
#define VSLAM_FBA_PCG_CAP 4     /* PCG reached pcg_max_iters in some step (the step is still a descent candidate)                             */
#define VSLAM_FBA_LAMBDA 8      /* stopped because lambda exceeded 1e12                                                                       */
#define VSLAM_FBA_SINGULAR 16   /* a damped landmark block or a preconditioner block was not positive definite in some iteration              */
#define VSLAM_FBA_DROPPED 32    /* observations behind the camera at the input state were left out (n_obs_dropped)                            */
typedef struct vslam_full_ba {
    int32_t struct_size;          /* sizeof(vslam_full_ba): set by the caller, checked */
    int32_t n_problems;
    int32_t total_kfs, total_lms, total_obs, total_edges;
    const int32_t* d_kf_off;      /* n_problems + 1 */
    const int32_t* d_lm_off;      /* n_problems + 1 */
    const int32_t* d_obs_off;     /* n_problems + 1 */
    const int32_t* d_edge_off;    /* n_problems + 1 */
    const double* d_T;            /* total_kfs x 7, in */
    const uint8_t* d_fixed;       /* total_kfs, or NULL: keyframe 0 of every problem */
    const double* d_xyz;          /* total_lms x 3, in */
    const int32_t* d_obs_kf;      /* total_obs, problem-local */
    const int32_t* d_obs_lm;      /* total_obs, problem-local, non-decreasing inside a problem */
    const float* d_obs_uv;        /* total_obs x 2 */
    const float* d_obs_disp;      /* total_obs, or NULL: all mono; negative or NaN = mono */
    const uint8_t* d_obs_active;  /* total_obs, or NULL: all active */
    double* d_obs_chi2;           /* total_obs, out: e'e of EVERY observation (inactive ones too) at the output state; NULL = not wanted */
    const int32_t* d_edge_i;      /* total_edges, problem-local */
    const int32_t* d_edge_j;      /* total_edges, problem-local */
    const double* d_edge_Z;       /* total_edges x 7 */
    const double* d_edge_w;       /* total_edges x 6 */
    const uint8_t* d_edge_active; /* total_edges, or NULL: all active */
    double K4[4];                 /* fx, fy, cx, cy */
    double bf;                    /* fx x baseline */
    double huber_delta;           /* 0 = no robust kernel */
} vslam_full_ba;
typedef struct vslam_full_ba_params {
    int32_t struct_size;          /* sizeof(vslam_full_ba_params) */
    int32_t max_iters;            /* LM iterations; 0 = evaluate only */
    int32_t pcg_max_iters;
    int32_t reserved;
    double pcg_tol;               /* relative residual */
    double step_tol;
    double lambda_init;
} vslam_full_ba_params;
typedef struct vslam_full_ba_stats {
    double chi2_init, chi2_final, lambda;
    int32_t lm_iters, pcg_iters, n_free, n_obs_dropped, status, reserved;
} vslam_full_ba_stats;
/* max_iters 50, pcg_max_iters 4000, pcg_tol 1e-10, step_tol 1e-9, lambda_init 1e-4 (the pose graph's; DESIGN.md 5.11 for the iteration counts) */
void vslam_full_ba_default_params(vslam_full_ba_params* p);
/* Optimises every problem of the batch: d_T_out (total_kfs x 7; may be d_T itself), d_xyz_out (total_lms x 3; may be d_xyz itself) and, when
 * not NULL, d_stats (n_problems) and ba->d_obs_chi2.  params NULL = the defaults.  max_iters = 0 evaluates only: chi2_init and the observation chi2
 * are written, poses and points copied.  Refuses with VSLAM_ERR_ARG and a message before it launches anything: a null where a pointer is
 * required, negative counts, a wrong struct_size, parameters or camera out of range.  Asynchronous on the context stream; the state lives in a
 * growable buffer of the context counted in vslam_device_bytes. */
int vslam_full_ba_dev(vslam_ctx* ctx, const vslam_full_ba* ba, const vslam_full_ba_params* params, double* d_T_out, double* d_xyz_out,
                      vslam_full_ba_stats* d_stats);
/* the status words of the n_problems problems of the most recent vslam_full_ba_dev call, into h_status (host); synchronises the context stream */
int vslam_full_ba_status_dev(vslam_ctx* ctx, int n_problems, int32_t* h_status);

/* ------------------------------------------------------------------ match by projection: re-observed and fused landmarks -------- */
/* Search by projection: the landmarks of neighbouring keyframes (or of the other end of a loop) are projected into a keyframe at its estimated
 * pose, and each looks for its descriptor among the keypoints inside a small pixel window round the projection.  Additive: vslam_params and the
 * ABI version are unchanged; the host mirror (host/) does not call it.
 *
 * ITEMS.  A batch of n_items items laid back to back: item m owns landmarks [lm_off[m], lm_off[m+1]), names a target image item_img[m] in [0, B)
 * and carries a pose item_T[m] (7 doubles qx qy qz qw tx ty tz, T_c_w).  The target image indexes d_kps and d_n at stride kp_capacity and d_desc at
 * desc_stride_bytes (0 = kp_capacity x 32): the layout vslam_place_add_dev takes.  Sort the items by image: neighbours then share the descriptors
 * in the cache.
 * LANDMARKS.  A world point lm_xyz (3 doubles) and a descriptor row lm_desc_row into d_src_desc (n_src_rows rows of 32 bytes; it may be d_desc
 * itself: a landmark's identity frame x kp_capacity + keypoint is then its row).
 * CAMERA.  K4 = fx fy cx cy, a HOST pointer read during the call, or NULL for the context's camera; w and h are the context's img_w and img_h.
 * THE RULE, per landmark, in f64 without contraction:
 *   1. R from the quaternion as it stands (no normalisation): R00 = 1 - 2 (yy + zz), R01 = 2 (xy - zw), R02 = 2 (xz + yw), R10 = 2 (xy + zw),
 *      R11 = 1 - 2 (xx + zz), R12 = 2 (yz - xw), R20 = 2 (xz - yw), R21 = 2 (yz + xw), R22 = 1 - 2 (xx + yy);  P = ((Ri0 X + Ri1 Y) + Ri2 Z) + ti.
 *      Not z_min <= Pz <= z_max: BEHIND.
 *   2. u = (fx Px) / Pz + cx, v = (fy Py) / Pz + cy.  Not (0 <= u <= w - 1 and 0 <= v <= h - 1): OUTSIDE.
 *   3. The candidates are the keypoints j < min(d_n[img], kp_capacity) with |(double)x_j - u| <= r and |(double)y_j - v| <= r, r = (double)radius_px.
 *      None: NO_CANDIDATE.
 *   4. d_j = hamming(descriptor of the landmark, descriptor of j).  The best candidate minimises (d_j, j); second = the smallest d over the other
 *      candidates.  d_best > tau: TOO_FAR.  ratio_pct > 0, a second candidate exists and 100 d_best > ratio_pct x second: AMBIGUOUS.
 *   5. Among the landmarks of ONE ITEM that passed 4 with the same keypoint j the one with the smallest (d_best, index inside the item) keeps it:
 *      MATCHED; the others: CONTESTED.  (Two items on one image do not contest each other.)
 * OUTPUTS, per landmark: d_match = the keypoint when MATCHED, else -1; d_dist = d_best whenever there was a candidate (TOO_FAR, AMBIGUOUS,
 * CONTESTED and MATCHED), else -1; d_n_cand (may be NULL) = the candidate count (0 before step 3); d_status = one of the codes below.
 * INVALID INPUT.  A non-finite point, a descriptor row outside [0, n_src_rows): that landmark is INVALID (-1, -1, 0).  A non-finite pose or an
 * image outside [0, B): every landmark of the item.  Offsets: with pm = max(0, lm_off[0..m-1]) item m WRITES exactly the landmarks
 * [max(lm_off[m], pm), min(lm_off[m+1], n_landmarks)) -- ranges that cannot overlap whatever lm_off holds -- and is sound when
 * pm <= lm_off[m] <= lm_off[m+1] <= n_landmarks; an item that is not writes INVALID there.  Nothing is read or written out of range.
 * DETERMINISM.  Every reduction is a minimum over integer keys or a count: the same call twice writes the same bytes, and an item's output in a
 * batch is its output alone.
 * LIMIT.  One workgroup holds an image's keypoint grid (32 x 32 px cells, img_w, img_h <= 4095: at most 128 x 128), pixel coordinates, cell lists and
 * claims in LDS: 4 bytes per cell and 18 per keypoint slot, so kp_capacity <= VSLAM_PROJECT_MATCH_MAX_KP.  (vslam_set_tuning "pm_stage" = 1 also
 * stages the image's descriptors there, 32 bytes per slot more, where two workgroups still fit a CU; the outputs are the same bytes.) */
#define VSLAM_PROJECT_MATCH_MAX_KP 4096
#define VSLAM_PM_MATCHED 0
#define VSLAM_PM_BEHIND 1
#define VSLAM_PM_OUTSIDE 2
#define VSLAM_PM_NO_CANDIDATE 3
#define VSLAM_PM_TOO_FAR 4
#define VSLAM_PM_AMBIGUOUS 5
#define VSLAM_PM_CONTESTED 6
#define VSLAM_PM_INVALID 7
typedef struct vslam_project_match {
    int32_t struct_size;            /* sizeof(vslam_project_match): set by the caller, checked */
    int32_t n_items, n_landmarks;
    int32_t B, kp_capacity, n_src_rows;
    const int32_t* d_lm_off;        /* n_items + 1 */
    const int32_t* d_item_img;      /* n_items */
    const double* d_item_T;         /* n_items x 7 */
    const double* d_lm_xyz;         /* n_landmarks x 3 */
    const int32_t* d_lm_desc_row;   /* n_landmarks */
    const uint8_t* d_src_desc;      /* n_src_rows x 32, 16-byte aligned */
    const vslam_keypoint* d_kps;    /* B x kp_capacity */
    const uint8_t* d_desc;          /* B x desc_stride_bytes, 16-byte aligned */
    size_t desc_stride_bytes;       /* a multiple of 16, >= kp_capacity x 32; 0 = kp_capacity x 32 */
    const int32_t* d_n;             /* B */
    const double* K4;               /* host, 4 doubles, or NULL: the context's camera */
    int32_t* d_match;               /* n_landmarks, out */
    int32_t* d_dist;                /* n_landmarks, out */
    int32_t* d_n_cand;              /* n_landmarks, out, or NULL */
    uint8_t* d_status;              /* n_landmarks, out */
} vslam_project_match;
typedef struct vslam_project_match_params {
    int32_t struct_size;            /* sizeof(vslam_project_match_params) */
    float radius_px;                /* > 0, finite */
    int32_t tau;                    /* 0 .. 255 */
    int32_t ratio_pct;              /* 0 .. 100; 0 = no ratio test */
    double z_min, z_max;            /* depth gate, neither NaN */
} vslam_project_match_params;
/* radius_px 15, tau 50, ratio_pct 80, z_min 0.1, z_max 1e4 */
void vslam_project_match_default_params(vslam_project_match_params* p);
/* One launch for the whole batch, asynchronous on the context stream.  p NULL = the defaults.  Refuses with VSLAM_ERR_ARG and a message before it
 * launches anything: a null where a pointer is required (the landmark and output arrays only when n_landmarks > 0), n_items or B < 1, n_landmarks
 * or n_src_rows < 0, a wrong struct_size, radius_px not positive and finite, tau or ratio_pct out of range, a NaN gate, a camera with fx or
 * fy <= 0 or a non-finite entry, kp_capacity outside [1, VSLAM_PROJECT_MATCH_MAX_KP], d_src_desc or d_desc not 16-byte aligned, a
 * desc_stride_bytes that is no multiple of 16 or below kp_capacity x 32. */
int vslam_project_match_dev(vslam_ctx* ctx, const vslam_project_match* in, const vslam_project_match_params* p);

/* ------------------------------------------------------------------ raw device memory helpers ---------- */
/* For hosts without their own device allocator (the C++ mirror in host/); bench.py passes torch tensors. */
int vslam_dev_alloc(void** p, size_t bytes);
int vslam_dev_free(void* p);
int vslam_dev_upload(vslam_ctx* ctx, void* d, const void* h, size_t bytes);
int vslam_dev_download(vslam_ctx* ctx, void* h, const void* d, size_t bytes);
int vslam_dev_memset(vslam_ctx* ctx, void* d, int value, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* VSLAM_HIP_H */
