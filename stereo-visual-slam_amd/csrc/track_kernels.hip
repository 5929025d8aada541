// track_kernels.hip -- device-side graph construction for the BA half of a throughput-mode step.
//
// What it replaces: the landmark / observation bookkeeping of VO::insert_key_frame
// (/root/reference/src/stereo_visual_slam_main/visual_odometry.cpp:363-424: a tracked feature adds an observation to the landmark of
// the feature it was matched to, every other keypoint with a valid depth creates a landmark, a landmark whose depth was unreliable
// takes the position of the first later observation with a reliable depth, :391-401) and the graph build of optimize_map /
// optimize_pose_only (optimization.cpp:127-214, :303-361: poses = the keyframes of the window, landmarks with >= 1 observation, one
// edge per observation) -- for a batch of B CONSECUTIVE keyframes whose front-end results are already in device memory.  Window b is the
// map right after keyframe b was inserted: keyframes [max(0, b - n_kf + 1), b] (Map::num_keyframes_ = 10, map.hpp:22), every landmark
// observed by one of them, positions and reliable_depth_ as of time b.  Poses: the pose stage's relative poses chained from frame 0.
//
// Throughput-mode simplifications (stated in DESIGN.md): every frame is a keyframe unless the gate of insert_key_frame is applied
// (vslam_build_windows_gated_dev: kf_gate_kernel, track_walk_kernel<true>, kf_set_kernel<true>), windows are independent (is_inlier = 1 on entry:
// the chi2 classification of window b - 1 does not feed window b).  Which keyframes window b holds is a policy: the sliding window
// [b - n_kf + 1, b] (vslam_build_windows_dev), or the distance-based culling of Map::remove_keyframe (map.cpp:48-130) evaluated on the
// chained poses (vslam_build_windows_kf_dev policy 1: kf_band_kernel + kf_set_kernel below; the window kernels are templated on it).
// Pose inputs against the map (vslam_build_map_pnp_inputs_dev / vslam_build_windows_map_dev): the poses come from the caller (a refinement pass's
// absolute G) and the links from an index map (track_link_kernel<true>); track_map_inputs_kernel emits every match out of a feature at its landmark's position.
// Gated inside the passes (the *_gated_dev map entries): the frame states come from the caller too (kf_gate_kernel<true> on a pass's G), and the
// walk and the keyframe sets are the gated ones (track_walk_kernel<true>, kf_set_kernel<true>).
// The reference's query set inside those passes (vslam_build_map_pnp_inputs_requery_dev): track_features_kernel lists every frame's features after the
// walk, the subset matcher (match_kernels.hip) re-matches every pair on them, and track_map_inputs_kernel emits on that table.
// The reference's failure handling inside those passes (the *_recover_dev entries): frame_pairs_kernel pairs every frame with its last ACCEPTED
// predecessor (state 1 or 2) and finds the Lost frames; the links of a pair are honoured only when the table was built on that pairing, so the
// tracks are paths through consecutive accepted frames and the walk / emit kernels step through `nxt` (the next accepted frame) instead of f + 1.
//
// gfx950 mapping: the reference walks std::unordered_map<id, Landmark> with per-landmark observation vectors; here a track is a chain
// of (frame, keypoint) nodes linked by two flat int32 tables pred / succ (B x kp_capacity) filled by one scatter pass per frame pair,
// every keypoint slot of the batch is a thread, and a window is one workgroup that ranks the chain HEADS inside its frames with ballots
// -- landmark-sorted, window-local edge lists come out directly, nothing is sorted.  Landmark order inside a window: by observation
// count, then by the head's (frame, keypoint).  The optimiser accepts any landmark order; THIS one makes the 64 consecutive landmarks a
// wave of its landmark-wise phases owns homogeneous (most landmarks of a real sequence are seen once, a few in all ten keyframes: in
// creation order every wave ran ten observation rounds for an average of 1.3 useful ones).
// All kernels are byte / index work on < 25 MB of tables per 256 frames: bound by launch latency, not by bandwidth.
#include "vslam_internal.h"

#include "se3_device.h"

namespace vslam {

// start / first / n_seg (vslam_set_segments; null, null, 0: the batch is one sequence): the batch holds n_seg independent sequences laid back to back,
// segment k = frames [first[k], first[k + 1]), start[f] = the first frame of f's segment.  Every kernel below that pairs frame f with f - 1, or treats
// frame 0 as THE initialisation, does so per segment; indices stay batch-wide.  A null test is all a one-sequence batch pays.
struct TrackDims { int B, kp_cap, lr_cap, match_cap, pnp_cap, n_kf; const int32_t* start = nullptr; const int32_t* first = nullptr; int n_seg = 0; };
__device__ inline int seg_start(const int32_t* __restrict__ start, int f) { return start ? start[f] : 0; }
// item `it` (the pair it -> it + 1) straddles two segments: it is empty whatever the caller's tables hold
__device__ inline bool seg_boundary_item(const int32_t* __restrict__ start, int it) { return start && start[it + 1] == it + 1; }
// the frames [lo, hi) workgroup blockIdx.x of a one-workgroup-per-segment kernel owns (first null: the whole batch)
__device__ inline void seg_slice(const int32_t* __restrict__ first, int B, int& lo, int& hi) {
    lo = first ? first[blockIdx.x] : 0; hi = first ? first[blockIdx.x + 1] : B;
}

// vslam_set_segments: start[f] by bisection of first, and the matcher's query block of every item (the item itself; -1 empties a boundary item)
__global__ __launch_bounds__(256) void seg_expand_kernel(int B, int n_seg, const int32_t* __restrict__ first, int32_t* __restrict__ start, int32_t* __restrict__ qitem) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= B) return;
    int lo = 0, hi = n_seg; // largest k with first[k] <= f
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first[mid] <= f) lo = mid; else hi = mid; }
    start[f] = first[lo];
    if (f > 0) qitem[f - 1] = first[lo] == f ? -1 : f - 1;
}

// ---- per frame: keypoint -> L/R match table; chain tables cleared
__global__ __launch_bounds__(256) void track_init_kernel(TrackDims d, const vslam_dmatch* __restrict__ d_lr, const int32_t* __restrict__ d_nlr,
                                                        int32_t* __restrict__ kp2lr, int32_t* __restrict__ pred, int32_t* __restrict__ succ, int32_t* __restrict__ cand) {
    const int f = blockIdx.x, tid = threadIdx.x;
    int32_t* k2 = kp2lr + (size_t)f * d.kp_cap;
    for (int i = tid; i < d.kp_cap; i += 256) { k2[i] = -1; pred[(size_t)f * d.kp_cap + i] = -1; succ[(size_t)f * d.kp_cap + i] = -1; cand[(size_t)f * d.kp_cap + i] = -1; }
    __syncthreads();
    const int nlr = min(max(d_nlr[f], 0), d.lr_cap);
    const vslam_dmatch* lr = d_lr + (size_t)f * d.lr_cap;
    for (int m = tid; m < nlr; m += 256) {
        const int q = lr[m].queryIdx;
        if (q >= 0 && q < d.kp_cap) k2[q] = m;
    }
}

// ---- global poses: G[0] = identity, G[f] = T_rel[f - 1] o G[f - 1]; inclusive scan of SE3 products (Hillis-Steele in LDS, chunks of 256
// frames chained through a carry).  SE3 composition is associative; the scan's grouping differs from a sequential chain only in rounding.
// Segments: one workgroup per segment runs the same chunk loop on its slice, so a segment's products are grouped as in a batch that begins at its
// first frame and G[first[k]] = identity.
__global__ __launch_bounds__(256) void track_pose_chain_kernel(int B_all, const double* __restrict__ T_rel, double* __restrict__ G, const int32_t* __restrict__ first) {
    __shared__ double buf[2][256][7];
    __shared__ double carry[7];
    const int tid = threadIdx.x;
    int f_lo, B;
    seg_slice(first, B_all, f_lo, B);
    if (tid == 0) { carry[0] = carry[1] = carry[2] = 0; carry[3] = 1; carry[4] = carry[5] = carry[6] = 0; }
    for (int base = f_lo; base < B; base += 256) {
        const int f = base + tid;
        double X[7] = {0, 0, 0, 1, 0, 0, 0};
        if (f > f_lo && f < B)
#pragma unroll
            for (int i = 0; i < 7; ++i) X[i] = T_rel[(size_t)(f - 1) * 7 + i];
        int cur = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) buf[0][tid][i] = X[i];
        __syncthreads();
        for (int dd = 1; dd < 256; dd <<= 1) {
            double Y[7];
            if (tid >= dd) se3::mul(buf[cur][tid], buf[cur][tid - dd], Y); // later frames on the left
            else
#pragma unroll
                for (int i = 0; i < 7; ++i) Y[i] = buf[cur][tid][i];
#pragma unroll
            for (int i = 0; i < 7; ++i) buf[cur ^ 1][tid][i] = Y[i];
            cur ^= 1;
            __syncthreads();
        }
        double Gf[7];
        se3::mul(buf[cur][tid], carry, Gf);
        if (f < B)
#pragma unroll
            for (int i = 0; i < 7; ++i) G[(size_t)f * 7 + i] = Gf[i];
        __syncthreads();
        if (tid == 255)
#pragma unroll
            for (int i = 0; i < 7; ++i) carry[i] = Gf[i];
        __syncthreads();
    }
}

// ---- per frame pair (i -> i + 1): every frame-to-frame match becomes a CANDIDATE link q -> t.  Input j of the pose stage is the j-th match
// whose query keypoint owns a valid depth (the compaction of build_pnp_inputs_kernel, geom_kernels.hip, repeated with the same ballot ranks):
// such a candidate carries the pose stage's inlier flag (the reference erases the outliers of motion_estimation from the frame, :306).  A
// candidate whose query keypoint has no depth of its own is decided by the walk below (track_rule 1) or never a link (track_rule 0).
// kMap (the refinement passes of vslam_build_map_pnp_inputs_dev / vslam_build_windows_map_dev): the pose problem's inputs are indexed by
// the map in_of_match (match k of item i -> input j, or -1), so every candidate is decided here: it holds when match k was input j and j an inlier.
constexpr int kCandDepth = 1 << 20, kCandInlier = 1 << 21; // cand word of slot t: q (low 16 bits) | flags (kp_capacity <= 65536), -1: no match reaches it
template <bool kMap>
__global__ __launch_bounds__(256) void track_link_kernel(TrackDims d, const vslam_dmatch* __restrict__ d_f2f, const int32_t* __restrict__ d_nf2f,
                                                        const uint8_t* __restrict__ d_valid, const uint8_t* __restrict__ d_inl,
                                                        const int32_t* __restrict__ kp2lr, int32_t* __restrict__ cand, int32_t* __restrict__ succ,
                                                        const int32_t* __restrict__ in_of_match, const int32_t* __restrict__ lfrm) {
    const int it = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_tot[4];
    // lfrm (the recover entries; null: adjacent frames): the query frame of item `it` when its links are honoured, -1 when they are not (uniform exit)
    const int l = lfrm ? lfrm[it] : it;
    if (l < 0 || seg_boundary_item(d.start, it)) return; // (no link crosses a segment boundary: the tracks are paths over these links)
    const int nm = min(max(d_nf2f[it], 0), d.match_cap);
    const vslam_dmatch* m = d_f2f + (size_t)it * d.match_cap;
    if (kMap) {
        for (int k = tid; k < nm; k += 256) {
            const int q = m[k].queryIdx, t = m[k].trainIdx;
            if (q < 0 || q >= d.kp_cap || t < 0 || t >= d.kp_cap) continue;
            const int j = in_of_match[(size_t)it * d.match_cap + k];
            const bool inl = j >= 0 && j < d.pnp_cap && d_inl[(size_t)it * d.pnp_cap + j] != 0;
            cand[(size_t)(it + 1) * d.kp_cap + t] = q | kCandDepth | (inl ? kCandInlier : 0);
            succ[(size_t)l * d.kp_cap + q] = t;
        }
        return;
    }
    const int32_t* k2 = kp2lr + (size_t)l * d.kp_cap;
    int written = 0;
    for (int base = 0; base < nm; base += 256) {
        const int k = base + tid;
        bool ok = false, in_range = false; int q = -1, t = -1;
        if (k < nm) {
            q = m[k].queryIdx; t = m[k].trainIdx;
            in_range = q >= 0 && q < d.kp_cap && t >= 0 && t < d.kp_cap;
            if (in_range) { const int li = k2[q]; ok = li >= 0 && d_valid[(size_t)l * d.lr_cap + li] != 0; }
        }
        const unsigned long long mask = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_tot[wave] = __popcll(mask);
        __syncthreads();
        int off = written;
        for (int w = 0; w < wave; ++w) off += s_tot[w];
        const int j = off + __popcll(mask & ((1ull << lane) - 1ull));
        if (in_range) { // (matches are one-to-one in query and train index: the matcher's cross-check)
            const bool inl = ok && j < d.pnp_cap && d_inl[(size_t)it * d.pnp_cap + j] != 0;
            cand[(size_t)(it + 1) * d.kp_cap + t] = q | (ok ? kCandDepth : 0) | (inl ? kCandInlier : 0);
            succ[(size_t)l * d.kp_cap + q] = t;
        }
        written += s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
    }
}

constexpr int kCarryCode = -2;
__device__ inline int carry_flags(const float* carry, int slot) { return carry ? (int)carry[4 * slot + 3] : 0; }

// the landmark position a chain node stands for: the point of node `src` (= first reliable node of the chain, else its root) in the world of G,
// or the carried position when the chain's source lies before the batch
__device__ inline void landmark_position(const TrackDims& d, int src, const int32_t* __restrict__ kp2lr, const float* __restrict__ d_xyz, const double* __restrict__ G,
                                         const float* __restrict__ carry, float out[3]) {
    if (src <= kCarryCode) { const int slot = kCarryCode - src; out[0] = carry[4 * slot]; out[1] = carry[4 * slot + 1]; out[2] = carry[4 * slot + 2]; return; }
    const int sf = src / d.kp_cap, si = src - sf * d.kp_cap;
    const int mm = kp2lr[(size_t)sf * d.kp_cap + si];
    const float* pc = d_xyz + 3 * ((size_t)sf * d.lr_cap + mm);
    double Gi[7], pw[3];
    const double p[3] = {(double)pc[0], (double)pc[1], (double)pc[2]};
    se3::inverse(G + (size_t)sf * 7, Gi);
    se3::act(Gi, p, pw);
    out[0] = (float)pw[0]; out[1] = (float)pw[1]; out[2] = (float)pw[2];
}

// PnPRansac's inlier test (visual_odometry.cpp:277, reprojection error <= 4 px; the contract of the pose stage's own flags) on a landmark's
// map position seen through the chained pose of the current frame
struct TrackCam { double fx, fy, cx, cy, thr2; int track_rule; };
__device__ inline bool reprojects_within(const float pos[3], const double* __restrict__ T, const vslam_keypoint* __restrict__ kp, const TrackCam& cam) {
    const double pw[3] = {(double)pos[0], (double)pos[1], (double)pos[2]};
    double pc[3];
    se3::act(T, pw, pc);
    const double du = (double)kp->x - (cam.fx * pc[0] / pc[2] + cam.cx), dv = (double)kp->y - (cam.fy * pc[1] / pc[2] + cam.cy);
    const double c = du * du + dv * dv;
    return isfinite(c) && c <= cam.thr2;
}

// ---- the tracks.  The candidate links form disjoint PATHS through the batch (a slot has at most one candidate in and one out); the thread of
// a path's first slot (no candidate reaches it, or it lies in the batch's first frame) walks the path forward in time, carrying the landmark the
// current slot stands for, and decides every candidate the way VO::tracking / motion_estimation would (visual_odometry.cpp:568-599, :260-306):
//   a slot with a valid depth of its own that no track reaches creates a landmark (:381-421: root = itself);
//   a candidate OUT of a slot that is a feature continues the track when the pose stage kept it (the slot owns a depth: it was an input), or -- [r6],
//   track_rule 1: the reference's query set is every feature of the last frame (:568-574), depth or not -- when the landmark's map position
//   (the creation point, or the first reliable one, :391-401, as of the last frame) reprojects within the pose stage's 4 px through the current frame's pose;
//   a candidate out of a slot that is no feature is nothing.
// Per slot it leaves: root (where the landmark was created), relsrc (the FIRST node of the chain, up to this one, with a reliable depth; -1: none yet),
// pred / succ (the links that hold).  A chunk of a longer sequence (carry: vslam_tracks_in::d_carry_in): a track may reach a keypoint of the batch's
// first frame from BEFORE the batch.  Such a slot is a feature whatever its own depth, and the chain's root -- and its first reliable node, if the
// carry says one was seen -- lie upstream: both tables then hold the code  kCarryCode - slot  (< -1), which resolves to the carried position.
// Sequential per path (its length: a few frames for most, the batch at worst), parallel over the ~B x 1200 paths.
// kGate (vslam_build_windows_gated_dev): a landmark is created, and takes its first reliable depth, only at a KEYFRAME node (state[f] == 2,
// insert_key_frame :353-424); a tracked feature passes through a non-keyframe exactly as above.
// nxt (the recover entries; null: f + 1): the frame a path continues in after frame f -- the next accepted frame, -1 for none.  nxt[f] > f, so the
// walk advances strictly in frame index and ends.
template <bool kGate>
__global__ __launch_bounds__(256) void track_walk_kernel(TrackDims d, TrackCam cam, const vslam_keypoint* __restrict__ d_kps, const float* __restrict__ d_xyz,
                                                        const uint8_t* __restrict__ d_valid, const uint8_t* __restrict__ d_rel, const int32_t* __restrict__ kp2lr,
                                                        const int32_t* __restrict__ cand, int32_t* __restrict__ pred, int32_t* __restrict__ succ,
                                                        const double* __restrict__ G, const float* __restrict__ carry, int32_t* __restrict__ root,
                                                        int32_t* __restrict__ relsrc, const int32_t* __restrict__ state, const int32_t* __restrict__ nxt) {
    const int f0 = blockIdx.y, i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= d.kp_cap) return;
    if (f0 > 0 && cand[(size_t)f0 * d.kp_cap + i0] >= 0) return; // some earlier slot's walk passes through here
    int cf = f0, ci = i0;
    bool feat = false;
    int r = -1, first = -1; // the landmark of the current slot: root and first reliable node (codes as in the tables)
    if (f0 == 0) {
        const int cfl = carry_flags(carry, i0);
        if (cfl & 1) { feat = true; r = kCarryCode - i0; if (cfl & 2) first = r; }
    }
    int pos_src = 0x7FFFFFFF; float pos[3] = {0.f, 0.f, 0.f}; // map position of the landmark, computed when a candidate needs it
    for (;;) {
        const size_t c = (size_t)cf * d.kp_cap + ci;
        const int node = cf * d.kp_cap + ci;
        const int mm = kp2lr[c];
        const bool own3d = mm >= 0 && d_valid[(size_t)cf * d.lr_cap + mm] != 0 && (!kGate || state[cf] == 2);
        if (!feat && own3d) { feat = true; r = node; first = -1; }                                        // :403-418 a landmark is created here
        if (feat && first == -1 && own3d && d_rel[(size_t)cf * d.lr_cap + mm] != 0) first = node;           // :391-401 (or created reliable)
        root[c] = feat ? r : -1; relsrc[c] = feat ? first : -1;
        const int nf = nxt ? nxt[cf] : cf + 1;
        if (nf <= cf || nf >= d.B) break;
        const int t = succ[c]; // (candidate)
        if (t < 0) break;
        const size_t cn = (size_t)nf * d.kp_cap + t;
        const int cd = cand[cn];
        bool holds = false;
        if (feat) {
            if (cd & kCandDepth) holds = (cd & kCandInlier) != 0;
            else if (cam.track_rule) {
                const int src = first != -1 ? first : r;
                if (src != pos_src) { landmark_position(d, src, kp2lr, d_xyz, G, carry, pos); pos_src = src; }
                holds = reprojects_within(pos, G + (size_t)nf * 7, d_kps + cn, cam);
            }
        }
        if (holds) pred[cn] = ci;
        else { succ[c] = -1; feat = false; r = -1; first = -1; }
        cf = nf; ci = t;
    }
}

// ---- per slot, after the walk: what a window needs to know about it without walking: node?, has a predecessor?, successors left in its chain
__global__ __launch_bounds__(256) void track_info_kernel(TrackDims d, const int32_t* __restrict__ pred, const int32_t* __restrict__ succ, const int32_t* __restrict__ root,
                                                        const float* __restrict__ carry, int32_t* __restrict__ info) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.kp_cap) return;
    const size_t at = (size_t)f * d.kp_cap + i;
    int p = pred[at];
    if (f == 0 && (carry_flags(carry, i) & 1)) p = 0; // (tracked from before the batch: a node with a predecessor; the index itself is never followed)
    const int r = root[at];
    int rem = 0;
    const bool node = r >= 0 || r <= kCarryCode;
    if (node) {
        int cf = f, ci = i;
        while (cf + 1 < d.B && rem < VSLAM_MAX_KF) {
            const int nx = succ[(size_t)cf * d.kp_cap + ci];
            if (nx < 0) break;
            ++cf; ci = nx; ++rem;
        }
    }
    info[at] = (node ? 1 : 0) | (p >= 0 ? 2 : 0) | (rem << 8);
}

// ---- culled windows only: per chain, its last frame and its first node with a reliable depth (-1: none), stored at the chain's ROOT node.  A chain
// is contiguous in frames from its root (no carry: policy 1 refuses chunks), so root / kp_cap is its first frame; the thread of the chain's last
// node is the only writer of the record.
__global__ __launch_bounds__(256) void track_ends_kernel(TrackDims d, const int32_t* __restrict__ succ, const int32_t* __restrict__ root,
                                                        const int32_t* __restrict__ relsrc, int2* __restrict__ ends) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.kp_cap) return;
    const size_t at = (size_t)f * d.kp_cap + i;
    const int r = root[at];
    if (r >= 0 && succ[at] < 0) ends[r] = make_int2(f, relsrc[at]);
}

// ---- the keyframe set of every window under the reference's culling (Map::remove_keyframe, map.cpp:48-130): S_0 = {0}; S_b = S_{b-1} + {b}, and
// when that holds more than n_kf frames the member k != b with d_k = |log(G_k o G_b^-1)| smallest is evicted if d_k < near_dist, else the one with
// d_k largest (ties: the lowest frame).  kf_distance is THE distance: the band pass and the chain's fallback both call it on the same G.
constexpr int kKfBand = 64;   // D[b][j - 1] = d(b - j, b), j = 1 .. kKfBand
constexpr int kKfRows = 32;   // band rows the serial chain stages in LDS at a time
__device__ inline double kf_distance(const double* __restrict__ Gk, const double Gb_inv[7]) {
    double T[7], xi[6];
    se3::mul(Gk, Gb_inv, T);
    se3::log(T, xi);
    return sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2] + xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
}

__global__ __launch_bounds__(256) void kf_band_kernel(int B, const double* __restrict__ G, double* __restrict__ D, const int32_t* __restrict__ start) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = t / kKfBand, j = t - b * kKfBand + 1;
    if (b >= B) return;
    double v = 0.0;
    if (b - j >= seg_start(start, b)) {
        double Gi[7];
        se3::inverse(G + (size_t)b * 7, Gi);
        v = kf_distance(G + (size_t)(b - j) * 7, Gi);
    }
    D[t] = v;
}

// LDS hand-off inside ONE wave: a wave's LDS operations complete in order, so only the compiler needs fencing -- __syncthreads()' workgroup-scope
// release would also wait for every global store in flight (the per-step outputs), about a microsecond per step of the chain below
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave, serial over the windows: lane k holds member k of S_{b-1} (ascending frames).  Per step: a band lookup per member (an LDS row, staged
// kKfRows steps at a time), the distance itself for members older than kKfBand, then every lane scans the <= VSLAM_MAX_KF (distance, frame) pairs
// from LDS in frame order -- the reference's loop, unrolled so that the reads issue together -- and the members shift down over the evicted one.
// kGate (vslam_build_windows_gated_dev): only a step whose frame state is 2 inserts its frame; any other step repeats S_{b-1}, evicts nothing and
// records 0 members in nmem (its window is empty); a rejected frame (state 0) sets bit 2 of the flags.  policy 0 evicts the oldest member (no band:
// D = nullptr), policy 1 as above.  nmem[b] = |S_b| at a keyframe step.
template <bool kGate>
__global__ __launch_bounds__(64) void kf_set_kernel(int B_all, int n_kf, double near_dist, const double* __restrict__ G, const double* __restrict__ D,
                                                    int32_t* __restrict__ kf_frame, int32_t* __restrict__ evicted, int32_t* __restrict__ flags,
                                                    const int32_t* __restrict__ state, int32_t* __restrict__ nmem, const int32_t* __restrict__ first) {
    __shared__ double rows[kKfRows][kKfBand];
    __shared__ double s_d[VSLAM_MAX_KF];
    __shared__ int s_m[VSLAM_MAX_KF];
    __shared__ int s_st[kKfRows];
    const int lane = threadIdx.x;
    const bool band = !kGate || D != nullptr;
    int f_lo, B; // (segments: one wave per segment, S restarts at {first[k]}; the chains are independent, the staging is relative to the slice)
    seg_slice(first, B_all, f_lo, B);
    int mem = lane == 0 ? f_lo : -1, n = 1, flag = 0;
    if (lane < n_kf) kf_frame[(size_t)f_lo * n_kf + lane] = mem;
    if (lane == 0) evicted[f_lo] = -1;
    if (kGate && lane == 0) nmem[f_lo] = 1; // (a segment's first frame is a keyframe: initialization)
    for (int base = f_lo + 1; base < B; base += kKfRows) {
        __syncthreads();
        if (band)
#pragma unroll
            for (int r = 0; r < kKfRows; ++r) rows[r][lane] = D[(size_t)min(base + r, B - 1) * kKfBand + lane]; // (clamped, not branched: the loads issue together)
        if (kGate && lane < kKfRows) s_st[lane] = state[min(base + lane, B - 1)];
        __syncthreads();
        for (int r = 0; r < kKfRows && base + r < B; ++r) {
            const int b = base + r;
            int ev = -1;
            const int st = kGate ? s_st[r] : 2;
            if (st != 2) {
                if (st == 0) flag |= 4;
            } else if (n < n_kf) {
                if (lane == n) mem = b;
                ++n;
            } else if (!band) { // policy 0: the oldest member goes
                ev = __shfl(mem, 0);
                const int moved = __shfl(mem, min(lane + 1, 63));
                if (lane < n - 1) mem = moved;
                if (lane == n - 1) mem = b;
            } else {
                const bool act = lane < n;
                const int j = b - mem;
                double dk = act && j <= kKfBand ? rows[r][j - 1] : 0.0;
                if (__any(act && j > kKfBand)) {
                    double Gi[7];
                    se3::inverse(G + (size_t)b * 7, Gi);
                    if (act && j > kKfBand) dk = kf_distance(G + (size_t)mem * 7, Gi);
                }
                const int moved = __shfl(mem, min(lane + 1, 63));
                if (act) { s_d[lane] = dk; s_m[lane] = mem; }
                wave_lds_sync();
                int far = -1, near = -1;
                double far_d = 0.0, near_d = 1e6; // (Map::remove_keyframe's starting values; NaN qualifies for neither)
#pragma unroll
                for (int k = 0; k < VSLAM_MAX_KF; ++k) {
                    const double x = s_d[k];
                    if (k < n && x > far_d) { far_d = x; far = k; }
                    if (k < n && x < near_d) { near_d = x; near = k; }
                }
                int e;
                if (near >= 0 && near_d < near_dist) e = near;
                else if (far >= 0) e = far;
                else { e = 0; flag |= 2; } // no member qualifies: the oldest goes, and the status says so
                ev = s_m[e];
                if (lane >= e && lane < n - 1) mem = moved;
                if (lane == n - 1) mem = b;
                wave_lds_sync();
            }
            if (lane < n_kf) kf_frame[(size_t)b * n_kf + lane] = lane < n ? mem : -1;
            if (lane == 0) evicted[b] = ev;
            if (kGate && lane == 0) nmem[b] = st == 2 ? n : 0;
        }
    }
    if (lane == 0) { if (first) { if (flag) atomicOr(flags, flag); } else *flags = flag; } // (segments: the launcher cleared the word)
}

// ---- insert_key_frame's gate, one thread per frame: frame 0 is a keyframe (initialization), frame f >= 1 gets keyframe_state(num_inliers_,
// T_c_l_) from the pose stage's outputs of item f - 1.  T: the relative poses T_rel (n_frames - 1 rows), or -- kAbs, a refinement pass's gate
// (vslam_gate_states_dev absolute = 1) -- the absolute poses G (n_frames rows), T_c_l_ = G_f o G_{f-1}^-1 as the reference takes it (:615)
template <bool kAbs>
__global__ __launch_bounds__(256) void kf_gate_kernel(int B, const int32_t* __restrict__ num_inliers, const double* __restrict__ T, int32_t* __restrict__ state,
                                                       const int32_t* __restrict__ start) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= B) return;
    const bool init = f == seg_start(start, f); // (a segment's first frame)
    if (!kAbs || init) { state[f] = init ? 2 : keyframe_state(num_inliers[f - 1], T + (size_t)(f - 1) * 7); return; }
    double Gi[7], T_c_l[7];
    se3::inverse(T + (size_t)(f - 1) * 7, Gi);
    se3::mul(T + (size_t)f * 7, Gi, T_c_l);
    state[f] = keyframe_state(num_inliers[f - 1], T_c_l);
}

// the same gate against the last ACCEPTED frame (vslam_gate_states_pairs_dev): T_c_l_ = G_f o G_pred(f)^-1 and frame_gap = f - pred(f) widens
// check_motion_estimation (visual_odometry.cpp:328-329).  A frame without a predecessor (pred outside [0, f)) had no item in the pass: raw state 0.
// With pred(f) = f - 1 the arithmetic is kf_gate_kernel<true>'s.
__global__ __launch_bounds__(256) void kf_gate_pairs_kernel(int B, const int32_t* __restrict__ num_inliers, const double* __restrict__ G,
                                                           const int32_t* __restrict__ pred, int32_t* __restrict__ state, const int32_t* __restrict__ start) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= B) return;
    const int f_lo = seg_start(start, f);
    if (f == f_lo) { state[f] = 2; return; }
    const int p = pred[f];
    if (p < f_lo || p >= f) { state[f] = 0; return; }
    double Gi[7], T_c_l[7];
    se3::inverse(G + (size_t)p * 7, Gi);
    se3::mul(G + (size_t)f * 7, Gi, T_c_l);
    state[f] = keyframe_state_gap(num_inliers[f - 1], T_c_l, (double)(f - p));
}

// ---- the pairing of VO::tracking's failure handling (visual_odometry.cpp:630-637, :673-693), one workgroup: pred[f] = the last frame j < f with state
// 1 or 2 (frame 0 always counts) as an exclusive max-scan in chunks of 256 frames; a frame is Lost when 11 or more rejected frames lie between it and
// that predecessor (f - pred > 11: lost_run > 10) or an earlier frame is Lost: pred = -1 from the first such frame on.  gap[f - 1] = f - pred[f] (1.0
// without a predecessor).  Optional outputs: state_out (may alias state; the EFFECTIVE states: 3 from the first Lost frame on, 0 for a state outside
// 0..3, else the state itself -- what the walk and the keyframe sets of the recover entries run on), nxt (the next accepted frame of
// every frame, -1 for none: nxt[pred[f]] = f for every accepted f, distinct predecessors), lfrm (item f - 1's query frame pred[f] when frame f is
// accepted and the table of pred_prev -- null: f - 1 -- was built on that same pairing, else -1), flags (bit 3: a Lost frame; bit 4: a state outside
// 0..3 or a pred_prev[f] outside [-1, f), whose item is emptied).  Thread tid owns the frames tid + 256 k in both phases.
constexpr int kLostGap = 11; // f - pred(f) above this: more than ten consecutive rejections (:673)
// Segments: one workgroup per segment on its slice [f_lo, B) -- the scan, the Lost frames and nxt restart there, a segment's first frame always counts
// and has pred -1; the boundary item before it gets gap 1.0 and lfrm -1; a pred_prev entry that points into an earlier segment is out of range.
__global__ __launch_bounds__(256) void frame_pairs_kernel(int B_all, const int32_t* state, int32_t* state_out, int32_t* __restrict__ pred, double* __restrict__ gap,
                                                         int32_t* __restrict__ nxt, const int32_t* __restrict__ pred_prev, int32_t* __restrict__ lfrm,
                                                         int32_t* __restrict__ flags, const int32_t* __restrict__ first) {
    __shared__ int s[256];
    __shared__ int carry, first_lost;
    const int tid = threadIdx.x;
    int f_lo, B;
    seg_slice(first, B_all, f_lo, B);
    if (tid == 0) { carry = -1; first_lost = B; }
    __syncthreads();
    int flag = 0;
    for (int base = f_lo; base < B; base += 256) {
        const int f = base + tid;
        const int st = f < B ? state[f] : 0;
        if (f > f_lo && f < B && (st < 0 || st > 3)) flag |= 16;
        s[tid] = f < B && (f == f_lo || st == 1 || st == 2) ? f : -1;
        __syncthreads();
        for (int dd = 1; dd < 256; dd <<= 1) {
            const int a = tid >= dd ? s[tid - dd] : -1;
            __syncthreads();
            s[tid] = max(s[tid], a);
            __syncthreads();
        }
        const int incl = max(carry, s[tid]), excl = max(carry, tid > 0 ? s[tid - 1] : -1);
        if (f < B) {
            pred[f] = f == f_lo ? -1 : excl;
            if (f > f_lo && f - excl > kLostGap) atomicMin(&first_lost, f);
        }
        __syncthreads();
        if (tid == 255) carry = incl;
        __syncthreads();
    }
    const int L = first_lost;
    if (nxt) {
        for (int f = f_lo + tid; f < B; f += 256) nxt[f] = -1;
        __syncthreads();
    }
    for (int f = f_lo + tid; f < B; f += 256) {
        const int st = state[f];
        const bool lost = f >= L;
        int p = pred[f];
        if (lost) { p = -1; pred[f] = -1; }
        if (state_out) state_out[f] = f == f_lo ? 2 : lost ? 3 : (st < 0 || st > 3) ? 0 : st;
        const bool acc = f > f_lo && !lost && (st == 1 || st == 2);
        if (f > 0) gap[f - 1] = p >= 0 ? (double)(f - p) : 1.0; // (p = -1 at a segment's first frame: the boundary item's gap is 1.0)
        if (nxt && acc) nxt[p] = f;
        if (lfrm && f > f_lo) {
            const int pp = pred_prev ? pred_prev[f] : f - 1;
            const bool bad = pp < -1 || pp >= f || (pp >= 0 && pp < f_lo);
            if (bad) flag |= 16;
            lfrm[f - 1] = acc && !bad && pp == p ? p : -1;
        } else if (lfrm && f > 0) lfrm[f - 1] = -1;
    }
    if (L < B) flag |= 8;
    if (flags && flag) atomicOr(flags, flag);
}

// the pairing's flags joined to a builder's status word (after window_scan_kernel wrote it)
__global__ void status_or_kernel(int32_t* __restrict__ status, const int32_t* __restrict__ flags) { *status |= *flags; }

// policy 0 through vslam_build_windows_kf_dev: the sliding window's sets written out
__global__ __launch_bounds__(256) void kf_sliding_kernel(int B, int n_kf, int32_t* __restrict__ kf_frame, int32_t* __restrict__ evicted, const int32_t* __restrict__ start) {
    const int t = blockIdx.x * 256 + threadIdx.x, b = t / n_kf, k = t - b * n_kf;
    if (b >= B) return;
    const int f_lo = seg_start(start, b), s = max(f_lo, b - n_kf + 1);
    kf_frame[t] = s + k <= b ? s + k : -1;
    if (k == 0) evicted[b] = b - f_lo >= n_kf ? b - n_kf : -1;
}

// ---- carry-out for the chunk that starts at frame c of this batch: per keypoint slot of frame c, does a track reach it from frame c - 1, and
// what is that track's landmark position / reliable flag AS OF ITS NODE IN FRAME c - 1 (the state the next chunk's chain walk would have found upstream)
__global__ __launch_bounds__(256) void track_carry_out_kernel(TrackDims d, int c, const int32_t* __restrict__ kp2lr, const int32_t* __restrict__ pred,
                                                             const int32_t* __restrict__ root, const int32_t* __restrict__ relsrc, const float* __restrict__ d_xyz,
                                                             const double* __restrict__ G, const float* __restrict__ carry_in, float* __restrict__ carry_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.kp_cap) return;
    float rec[4] = {0.f, 0.f, 0.f, 0.f};
    const int p = pred[(size_t)c * d.kp_cap + i];
    if (p >= 0) {
        const size_t pn = (size_t)(c - 1) * d.kp_cap + p;
        const int rs = relsrc[pn], src = (rs >= 0 || rs <= kCarryCode) ? rs : root[pn];
        landmark_position(d, src, kp2lr, d_xyz, G, carry_in, rec);
        rec[3] = (rs >= 0 || rs <= kCarryCode) ? 3.f : 1.f;
    }
    reinterpret_cast<float4*>(carry_out)[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// ---- per frame pair (i -> i + 1), after the walk: the pose problem of frame i + 1 against the MAP (VO::motion_estimation, visual_odometry.cpp:260-277):
// every match out of a feature of frame i (root != -1), in match order, with its landmark's position as of frame i -- the source rule of
// window_emit_kernel (the first reliable node, else the root), so the point is bit for bit the one window i holds -- and the current keypoint.
// Compacted with the ballot ranks of track_link_kernel; in_of_match[k] = the input match k became (-1: none, or cut by out_cap: status bit 0).
__global__ __launch_bounds__(256) void track_map_inputs_kernel(TrackDims d, const vslam_dmatch* __restrict__ d_f2f, const int32_t* __restrict__ d_nf2f,
                                                              const vslam_keypoint* __restrict__ d_kps, const float* __restrict__ d_xyz,
                                                              const int32_t* __restrict__ kp2lr, const int32_t* __restrict__ root,
                                                              const int32_t* __restrict__ relsrc, const double* __restrict__ G, int out_cap,
                                                              float* __restrict__ xyz_out, float* __restrict__ uv_out, int32_t* __restrict__ n_out,
                                                              int32_t* __restrict__ in_of_match, int32_t* __restrict__ status, const int32_t* __restrict__ qfrm) {
    const int it = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_tot[4];
    // qfrm (the recover entries; null: frame `it`): the frame the queries of item `it` live in, frame it + 1's last accepted predecessor (in [0, it]
    // by construction, frame_pairs_kernel); -1: the frame is Lost, no input and an index map of -1
    const int l = seg_boundary_item(d.start, it) ? -1 : qfrm ? qfrm[it] : it; // (a boundary item carries no pose input)
    const int nm = l < 0 ? 0 : min(max(d_nf2f[it], 0), d.match_cap);
    const vslam_dmatch* m = d_f2f + (size_t)it * d.match_cap;
    int32_t* map = in_of_match + (size_t)it * d.match_cap;
    int written = 0;
    for (int base = 0; base < nm; base += 256) {
        const int k = base + tid;
        bool ok = false; int q = -1, t = -1;
        if (k < nm) {
            q = m[k].queryIdx; t = m[k].trainIdx;
            ok = q >= 0 && q < d.kp_cap && t >= 0 && t < d.kp_cap && root[(size_t)l * d.kp_cap + q] != -1;
        }
        const unsigned long long mask = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_tot[wave] = __popcll(mask);
        __syncthreads();
        int off = written;
        for (int w = 0; w < wave; ++w) off += s_tot[w];
        const int j = off + __popcll(mask & ((1ull << lane) - 1ull));
        const bool keep = ok && j < out_cap;
        if (keep) {
            const size_t c = (size_t)l * d.kp_cap + q;
            const int rs = relsrc[c];
            float pos[3];
            landmark_position(d, rs != -1 ? rs : root[c], kp2lr, d_xyz, G, nullptr, pos);
            float* o = xyz_out + 3 * ((size_t)it * out_cap + j);
            o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2];
            const vslam_keypoint* kp = d_kps + (size_t)(it + 1) * d.kp_cap + t;
            reinterpret_cast<float2*>(uv_out)[(size_t)it * out_cap + j] = make_float2(kp->x, kp->y);
        }
        if (k < nm) map[k] = keep ? j : -1;
        written += s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
    }
    for (int k = nm + tid; k < d.match_cap; k += 256) map[k] = -1;
    if (tid == 0) {
        n_out[it] = min(written, out_cap);
        if (written > out_cap) atomicOr(status, 1);
    }
}

// ---- per frame, after the walk (vslam_build_map_pnp_inputs_requery_dev): the frame's FEATURES -- the slots with root != -1, the one definition the
// kernel above uses -- as an ascending list (the ballot ranks again) and their count: the query set VO::tracking hands feature_matching
// (visual_odometry.cpp:568-575, descriptors_last = frame_last_.features_).  Also the frame gap of the pair that starts here (1: adjacent frames).
__global__ __launch_bounds__(256) void track_features_kernel(TrackDims d, const int32_t* __restrict__ root, const int32_t* __restrict__ nkps,
                                                            int32_t* __restrict__ feat, int32_t* __restrict__ nfeat, double* __restrict__ gap) {
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_tot[4];
    // (a one-frame segment has no pair: like a one-frame batch, which runs no walk, it lists nothing)
    const bool lone = d.start && d.start[f] == f && (f + 1 >= d.B || d.start[f + 1] == f + 1);
    const int n = lone ? 0 : nkps ? min(max(nkps[f], 0), d.kp_cap) : d.kp_cap;
    int written = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const bool ok = i < n && root[(size_t)f * d.kp_cap + i] != -1;
        const unsigned long long mask = __ballot(ok);
        __syncthreads();
        if (lane == 0) s_tot[wave] = __popcll(mask);
        __syncthreads();
        int off = written;
        for (int w = 0; w < wave; ++w) off += s_tot[w];
        if (ok) feat[(size_t)f * d.kp_cap + off + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        written += s_tot[0] + s_tot[1] + s_tot[2] + s_tot[3];
    }
    if (tid == 0) { nfeat[f] = written; if (gap && f + 1 < d.B) gap[f] = 1.0; } // (gap null: the recover entry's pairing wrote the gaps)
}

// first frame of sliding window b: the window never reaches before its segment
__device__ inline int window_first(const TrackDims& d, int b) { return max(seg_start(d.start, b), b - d.n_kf + 1); }

// A chain HEAD of window [s, b]: a node in frame s, or a node without predecessor (a landmark created inside the window).  Every
// landmark observed in the window has exactly one.  Returns the observations it has inside the window (0: not a head) -- from the
// slot's info word alone (track_chain_kernel), no chain walk.
__device__ inline int window_head_len(int info, int s, int b, int f) {
    if (!(info & 1) || (f != s && (info & 2))) return 0;
    return min((info >> 8) + 1, b - f + 1);
}

// The same for a window whose keyframes are an arbitrary ascending set kf[0..n) (kf[n - 1] = b): a node in frame kf[k] is a head when its chain
// has no node in the previous member kf[k - 1] -- chains are contiguous in frames, so when the chain starts after it -- and it has one observation
// per member in [kf[k], min(last, b)].
__device__ inline int window_set_head_len(int r, const int2* __restrict__ ends, int kp_cap, const int* kf, int n, int k) {
    if (r < 0 || (k > 0 && r / kp_cap <= kf[k - 1])) return 0;
    const int last = ends[r].x;
    int len = 0;
    for (int j = k; j < n && kf[j] <= last; ++j) ++len;
    return len;
}

// A window's keyframes: the sliding window [s, b], or the culled set of kf_frame (kSet).  Loaded into the workgroup's LDS.  nmem (gated sets
// only, else nullptr): the member count of every window, 0 for the empty window of a non-keyframe step; without it every set holds
// min(b + 1, n_kf) frames.
struct WindowSet { const int32_t* kf_frame; const int2* ends; const int32_t* root; const int32_t* nmem; const int32_t* nxt = nullptr; // nxt: see track_walk_kernel
                   int32_t* lm_id = nullptr; }; // lm_id: vslam_set_window_ids (window_emit_kernel writes every landmark's root there)
template <bool kSet>
__device__ inline int window_frames(const TrackDims& d, const WindowSet& ws, int b, int* s_kf) {
    const int s = window_first(d, b), nk = kSet && ws.nmem ? ws.nmem[b] : b - s + 1;
    if (threadIdx.x < nk) s_kf[threadIdx.x] = kSet ? ws.kf_frame[(size_t)b * d.n_kf + threadIdx.x] : s + threadIdx.x;
    __syncthreads();
    return nk;
}

__device__ inline int block_sum_i32(int v, int* red /* 4 */) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---- per window: landmark and edge counts, and the landmarks per observation count (the bins of the emit pass)
constexpr int kHist = VSLAM_MAX_KF + 1;
template <bool kSet>
__global__ __launch_bounds__(256) void window_count_kernel(TrackDims d, const int32_t* __restrict__ info, const int32_t* __restrict__ nkps,
                                                          int32_t* __restrict__ counts, int32_t* __restrict__ hist, WindowSet ws) {
    const int b = blockIdx.x, tid = threadIdx.x, s = window_first(d, b);
    __shared__ int red[4];
    __shared__ int h[kHist];
    __shared__ int s_kf[VSLAM_MAX_KF];
    if (tid < kHist) h[tid] = 0;
    const int nk = kSet ? window_frames<true>(d, ws, b, s_kf) : 0;
    if (!kSet) __syncthreads();
    int nl = 0, ne = 0;
    for (int k = 0; k < (kSet ? nk : b - s + 1); ++k) {
        const int f = kSet ? s_kf[k] : s + k;
        const int nkp = nkps ? min(max(nkps[f], 0), d.kp_cap) : d.kp_cap; // (slots beyond the frame's keypoints are never nodes)
        for (int i = tid; i < nkp; i += 256) {
            const int len = kSet ? window_set_head_len(ws.root[(size_t)f * d.kp_cap + i], ws.ends, d.kp_cap, s_kf, nk, k)
                                 : window_head_len(info[(size_t)f * d.kp_cap + i], s, b, f);
            nl += len > 0; ne += len;
            if (len > 0) atomicAdd(&h[min(len, kHist - 1)], 1); // (integer: order-free)
        }
    }
    nl = block_sum_i32(nl, red);
    ne = block_sum_i32(ne, red);
    if (tid == 0) { counts[2 * b] = nl; counts[2 * b + 1] = ne; }
    if (tid < kHist) hist[(size_t)b * kHist + tid] = h[tid];
}

// ---- offsets of the concatenated arrays (exclusive scan over the windows; one workgroup).  A window that would run past a capacity, and
// every window after it, is emitted EMPTY and the status word is set: the caller sized its arrays too small.
template <bool kSet>
__global__ __launch_bounds__(256) void window_scan_kernel(TrackDims d, const int32_t* __restrict__ counts, int lm_capacity, int edge_capacity,
                                                         int32_t* __restrict__ lm_off, int32_t* __restrict__ edge_off, int32_t* __restrict__ n_kf_out,
                                                         int32_t* __restrict__ status, const int32_t* __restrict__ set_flags, const int32_t* __restrict__ nmem) {
    __shared__ int sl[256], se[256];
    __shared__ int carry_l, carry_e, cut;
    const int tid = threadIdx.x;
    if (tid == 0) { carry_l = 0; carry_e = 0; cut = 0; lm_off[0] = 0; edge_off[0] = 0; }
    __syncthreads();
    for (int base = 0; base < d.B; base += 256) {
        const int b = base + tid;
        const int cl = b < d.B ? counts[2 * b] : 0, ce = b < d.B ? counts[2 * b + 1] : 0;
        sl[tid] = cl; se[tid] = ce;
        __syncthreads();
        for (int dd = 1; dd < 256; dd <<= 1) {
            const int a = tid >= dd ? sl[tid - dd] : 0, e = tid >= dd ? se[tid - dd] : 0;
            __syncthreads();
            sl[tid] += a; se[tid] += e;
            __syncthreads();
        }
        const int il = carry_l + sl[tid], ie = carry_e + se[tid]; // inclusive
        const bool over = il > lm_capacity || ie > edge_capacity;
        if (b < d.B && over) atomicExch(&cut, 1);
        __syncthreads();
        if (b < d.B) {
            // (prefixes are monotone: once a window overflows all later ones do; an overflowing window repeats the last good offset)
            int ol = il, oe = ie;
            if (over) { ol = -1; oe = -1; }
            lm_off[b + 1] = ol; edge_off[b + 1] = oe;
            n_kf_out[b] = kSet && nmem ? nmem[b] : min(b - seg_start(d.start, b) + 1, d.n_kf);
        }
        __syncthreads();
        if (tid == 255) { carry_l = il; carry_e = ie; }
        __syncthreads();
    }
    // second pass: replace the -1 marks by the last good offset (windows from the first overflow on are empty)
    __syncthreads();
    if (tid == 0) {
        if (cut) {
            int gl = 0, ge = 0;
            for (int b = 0; b < d.B; ++b) {
                if (lm_off[b + 1] < 0) { lm_off[b + 1] = gl; edge_off[b + 1] = ge; }
                else { gl = lm_off[b + 1]; ge = edge_off[b + 1]; }
            }
        }
        *status = (cut ? 1 : 0) | (kSet ? *set_flags : 0);
    }
}

// ---- per window: poses, and the RANK of every chain head = its window-local landmark index (by observation count, then by (frame,
// keypoint)); the head's record goes to head_rec[global landmark index] for the emit pass.  No dependent loads here: one info word per
// slot, a ballot per count, three barriers per 1024 slots.
constexpr int kRankBlock = 1024, kRankWaves = kRankBlock / 64;
template <bool kSet>
__global__ __launch_bounds__(kRankBlock) void window_rank_kernel(TrackDims d, const double* __restrict__ G, const int32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ hist, const int32_t* __restrict__ info,
                                                                const int32_t* __restrict__ nkps, const int32_t* __restrict__ lm_off,
                                                                const int32_t* __restrict__ edge_off, double* __restrict__ T_out,
                                                                uint32_t* __restrict__ head_rec, WindowSet ws) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = window_first(d, b);
    __shared__ int s_c[kRankWaves][kHist];
    __shared__ int bin_l[kHist], s_run[kHist];
    __shared__ int s_kf[VSLAM_MAX_KF];
    const int nk = kSet ? window_frames<true>(d, ws, b, s_kf) : b - s + 1;
    if (kSet && nk == 0) { // the empty window of a non-keyframe step (gated sets): slot 0 = its own frame's pose, the other slots untouched
        if (tid < 7) T_out[(size_t)b * d.n_kf * 7 + tid] = G[(size_t)b * 7 + tid];
        return;
    }
    for (int i = tid; i < d.n_kf * 7; i += kRankBlock) { // poses of the window's keyframes (unused slots: identity)
        const int k = i / 7, c = i - 7 * k;
        T_out[(size_t)b * d.n_kf * 7 + i] = k < nk ? G[(size_t)((kSet ? s_kf[k] : s + k)) * 7 + c] : (c == 3 ? 1.0 : 0.0);
    }
    const int l0 = lm_off[b];
    if (lm_off[b + 1] - l0 != counts[2 * b] || edge_off[b + 1] - edge_off[b] != counts[2 * b + 1]) return; // truncated by the capacity check: empty window
    if (tid == 0) { int al = 0; for (int c = 1; c < kHist; ++c) { bin_l[c] = al; al += hist[(size_t)b * kHist + c]; } }
    if (tid < kHist) s_run[tid] = 0;
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
        const int f = kSet ? s_kf[k] : s + k;
        const int nkp = nkps ? min(max(nkps[f], 0), d.kp_cap) : d.kp_cap;
        for (int base = 0; base < nkp; base += kRankBlock) {
            const int i = base + tid;
            const int len = i >= nkp ? 0
                          : kSet ? min(window_set_head_len(ws.root[(size_t)f * d.kp_cap + i], ws.ends, d.kp_cap, s_kf, nk, k), kHist - 1)
                                 : min(window_head_len(info[(size_t)f * d.kp_cap + i], s, b, f), kHist - 1);
            int my_rank = 0, my_wave_cnt = 0;
#pragma unroll
            for (int c = 1; c < kHist; ++c) {
                const unsigned long long m = __ballot(len == c);
                if (len == c) my_rank = __popcll(m & ((1ull << lane) - 1ull));
                if (lane == c) my_wave_cnt = __popcll(m);
            }
            __syncthreads();
            if (lane < kHist) s_c[wave][lane] = my_wave_cnt;
            __syncthreads();
            if (len > 0) {
                int before = s_run[len];
                for (int w = 0; w < wave; ++w) before += s_c[w][len];
                head_rec[l0 + bin_l[len] + before + my_rank] = (uint32_t)k | ((uint32_t)i << 4) | ((uint32_t)len << 20); // (k: the head's slot)
            }
            __syncthreads();
            if (tid < kHist) { int t = 0; for (int w = 0; w < kRankWaves; ++w) t += s_c[w][tid]; s_run[tid] += t; }
        }
    }
}

// ---- one thread per landmark of the batch: its edges (chronological) and its position / reliable_depth_ as of its last observation inside
// the window.  Flat over the concatenated landmark array: the window is found by bisection of lm_off.  A culled window (kSet) walks the chain
// through the frames that are not members and emits at the members; its position is the chain's as of frame b (a reliable update in a culled
// frame counts), read from the chain's record instead of its node at min(last, b).
template <bool kSet>
__global__ __launch_bounds__(256) void window_emit_kernel(TrackDims d, const vslam_keypoint* __restrict__ d_kps, const float* __restrict__ d_xyz,
                                                         const int32_t* __restrict__ kp2lr, const int32_t* __restrict__ root,
                                                         const int32_t* __restrict__ relsrc, const int32_t* __restrict__ succ,
                                                         const double* __restrict__ G, const float* __restrict__ carry, const int32_t* __restrict__ hist,
                                                         const uint32_t* __restrict__ head_rec, const int32_t* __restrict__ lm_off,
                                                         const int32_t* __restrict__ edge_off, float* __restrict__ xyz_out,
                                                         uint8_t* __restrict__ rel_out, uint8_t* __restrict__ inl_out, int32_t* __restrict__ kf_out,
                                                         int32_t* __restrict__ lm_out, float* __restrict__ uv_out, WindowSet ws) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= lm_off[d.B]) return;
    int lo = 0, hi = d.B; // largest b with lm_off[b] <= g
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (lm_off[mid] <= g) lo = mid; else hi = mid; }
    const int b = lo, s = window_first(d, b), l = g - lm_off[b];
    const uint32_t rec = head_rec[g];
    const int32_t* kfs = ws.kf_frame + (size_t)b * d.n_kf;
    const int slot = (int)(rec & 15u), f = kSet ? kfs[slot] : s + slot, i = (int)((rec >> 4) & 0xFFFFu), len = (int)(rec >> 20);
    int bl = 0, be = 0; // first landmark / first edge of the landmarks with `len` observations
    for (int c = 1; c < len; ++c) { const int n = hist[(size_t)b * kHist + c]; bl += n; be += n * c; }
    int e = edge_off[b] + be + (l - bl) * len;
    int cf = f, ci = i;
    if (kSet) {
        for (int k = 0; k < len; ++k) {
            const int tf = kfs[slot + k];
            while (cf < tf) { // (a chain reaches tf: ends[]; it steps through the frames, or -- ws.nxt -- through the accepted ones)
                const int nx = succ[(size_t)cf * d.kp_cap + ci], nf = ws.nxt ? ws.nxt[cf] : cf + 1;
                if (nf <= cf || nf > tf) break;
                ci = nx < 0 ? ci : nx; cf = nf;
            }
            const vslam_keypoint* kp = d_kps + (size_t)cf * d.kp_cap + ci;
            kf_out[e] = slot + k; lm_out[e] = l;
            reinterpret_cast<float2*>(uv_out)[e] = make_float2(kp->x, kp->y);
            ++e;
        }
    } else {
        for (int k = 0; k < len; ++k) {
            const vslam_keypoint* kp = d_kps + (size_t)cf * d.kp_cap + ci;
            kf_out[e] = cf - s; lm_out[e] = l;
            reinterpret_cast<float2*>(uv_out)[e] = make_float2(kp->x, kp->y);
            ++e;
            if (k + 1 < len) { ci = succ[(size_t)cf * d.kp_cap + ci]; ++cf; }
        }
    }
    const size_t last = (size_t)cf * d.kp_cap + ci;
    bool has_rel;
    float pos[3];
    if (kSet) { // the chain's first reliable node, if it lies at or before b
        const int r = root[last], rs = ws.ends[r].y;
        has_rel = rs >= 0 && rs / d.kp_cap <= b;
        landmark_position(d, has_rel ? rs : r, kp2lr, d_xyz, G, carry, pos);
    } else {
        const int rs = relsrc[last];
        has_rel = rs >= 0 || rs <= kCarryCode;
        landmark_position(d, has_rel ? rs : root[last], kp2lr, d_xyz, G, carry, pos);
    }
    float* o = xyz_out + 3 * (size_t)g;
    o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2];
    rel_out[g] = has_rel; inl_out[g] = 1;
    if (ws.lm_id) ws.lm_id[g] = root[last]; // the landmark's identity across windows: its creating frame x kp_cap + its creating keypoint
}

struct WindowTables { double* G; int32_t *counts, *hist; uint32_t* head_rec; int2* ends = nullptr; double* D = nullptr; int32_t *set_flags = nullptr, *nmem = nullptr; }; // the window builder's own scratch

// ---- which keyframes every window holds: the gate's states (unless they are the caller's) and the sets on them, the culled sets, or the sliding sets
static void launch_kf_sets(int B, int n_kf, const vslam_tracks_in& in, const KfPolicy& kp, const WindowTables& w, const int32_t* state, int seg_grid, const SegView& seg, hipStream_t stream) {
    if (kp.gate) { // the states depend on the pose stage's outputs alone, the keyframe sets on the states and the poses
        if (!kp.state_in)
            hipLaunchKernelGGL(kf_gate_kernel<false>, dim3((B + 255) / 256), dim3(256), 0, stream, B, kp.num_inliers, in.d_T_rel, kp.frame_state, seg.start);
        if (kp.policy == 1) hipLaunchKernelGGL(kf_band_kernel, dim3((B * kKfBand + 255) / 256), dim3(256), 0, stream, B, w.G, w.D, seg.start);
        hipLaunchKernelGGL(kf_set_kernel<true>, dim3(seg_grid), dim3(64), 0, stream, B, n_kf, kp.near_dist, w.G, kp.policy == 1 ? w.D : nullptr, kp.kf_frame, kp.evicted, w.set_flags,
                           state, w.nmem, seg.first);
    } else if (kp.policy == 1) { // the keyframe sets depend on the poses alone
        hipLaunchKernelGGL(kf_band_kernel, dim3((B * kKfBand + 255) / 256), dim3(256), 0, stream, B, w.G, w.D, seg.start);
        hipLaunchKernelGGL(kf_set_kernel<false>, dim3(seg_grid), dim3(64), 0, stream, B, n_kf, kp.near_dist, w.G, w.D, kp.kf_frame, kp.evicted, w.set_flags, nullptr, nullptr, seg.first);
    } else if (kp.policy == 0)
        hipLaunchKernelGGL(kf_sliding_kernel, dim3((B * n_kf + 255) / 256), dim3(256), 0, stream, B, n_kf, kp.kf_frame, kp.evicted, seg.start);
}

// ---- the front half both builders share: the dims (with the segment table), the camera, the six n_frames x kp_capacity node tables, and the
// launches from the optional pairing to the walk.  A launcher carves its scratch ONCE (a second carve may grow the buffer and free the first
// one's memory), so the tables come out of the launcher's own layout: take().
struct TrackTables {
    TrackDims d; TrackCam cam;
    int32_t *kp2lr, *pred, *succ, *root, *relsrc, *cand;
    int32_t *nxt = nullptr, *lfrm = nullptr, *r_state = nullptr; // recover: the pairing's next accepted frame / link frame, the states with the Lost frames marked
    TrackTables(const vslam_tracks_in& in, int n_kf, const TrackParams& tp, const SegView& seg) {
        d.B = in.n_frames; d.kp_cap = in.kp_capacity; d.lr_cap = in.lr_capacity; d.match_cap = in.match_capacity; d.pnp_cap = in.pnp_capacity; d.n_kf = n_kf;
        d.start = seg.start; d.first = seg.first; d.n_seg = seg.n_seg;
        cam.fx = tp.K4[0]; cam.fy = tp.K4[1]; cam.cx = tp.K4[2]; cam.cy = tp.K4[3]; cam.thr2 = tp.reproj_thr * tp.reproj_thr; cam.track_rule = tp.track_rule;
    }
    size_t tab() const { return (size_t)d.B * d.kp_cap; }
    int seg_grid() const { return d.first ? d.n_seg : 1; } // the per-sequence kernels: one workgroup per segment
    void take(Layout& L, bool recover) {
        kp2lr = L.take<int32_t>(tab()); pred = L.take<int32_t>(tab()); succ = L.take<int32_t>(tab());
        root = L.take<int32_t>(tab()); relsrc = L.take<int32_t>(tab()); cand = L.take<int32_t>(tab());
        if (recover) { nxt = L.take<int32_t>(d.B); lfrm = L.take<int32_t>(d.B); r_state = L.take<int32_t>(d.B); }
    }
};

// the tables' initial state; before it, rv non-null (recover): the pairing of `state` (rv->d_pred / d_gap; rv->d_pred_prev: the one in.d_f2f was built on), flags ORed into *flags
static void launch_track_init(const TrackTables& t, const vslam_tracks_in& in, const MapRecover* rv, const int32_t* state, int32_t* flags, hipStream_t stream) {
    if (rv)
        hipLaunchKernelGGL(frame_pairs_kernel, dim3(t.seg_grid()), dim3(256), 0, stream, t.d.B, state, t.r_state, rv->d_pred, rv->d_gap, t.nxt, rv->d_pred_prev, t.lfrm, flags, t.d.first);
    hipLaunchKernelGGL(track_init_kernel, dim3(t.d.B), dim3(256), 0, stream, t.d, in.d_lr, in.d_nlr, t.kp2lr, t.pred, t.succ, t.cand);
}

// the links (through in_of_match when it is set, else by the pose stage's own-depth flags and track_rule) and the walk on the poses G; state non-null: the gated walk
static void launch_track_walk(const TrackTables& t, const vslam_tracks_in& in, const int32_t* in_of_match, const double* G, const float* carry_in, const int32_t* state,
                              hipStream_t stream) {
    const TrackDims& d = t.d;
    if (d.B > 1 && in_of_match)
        hipLaunchKernelGGL(track_link_kernel<true>, dim3(d.B - 1), dim3(256), 0, stream, d, in.d_f2f, in.d_nf2f, in.d_valid, in.d_pose_inlier, t.kp2lr, t.cand, t.succ, in_of_match, t.lfrm);
    else if (d.B > 1)
        hipLaunchKernelGGL(track_link_kernel<false>, dim3(d.B - 1), dim3(256), 0, stream, d, in.d_f2f, in.d_nf2f, in.d_valid, in.d_pose_inlier, t.kp2lr, t.cand, t.succ, nullptr, t.lfrm);
    const dim3 grid((d.kp_cap + 255) / 256, d.B);
    if (state)
        hipLaunchKernelGGL(track_walk_kernel<true>, grid, dim3(256), 0, stream, d, t.cam, in.d_kps, in.d_xyz, in.d_valid, in.d_reliable, t.kp2lr, t.cand, t.pred, t.succ, G, carry_in,
                           t.root, t.relsrc, state, t.nxt);
    else
        hipLaunchKernelGGL(track_walk_kernel<false>, grid, dim3(256), 0, stream, d, t.cam, in.d_kps, in.d_xyz, in.d_valid, in.d_reliable, t.kp2lr, t.cand, t.pred, t.succ, G, carry_in,
                           t.root, t.relsrc, nullptr, nullptr);
}

// ---- count / scan / rank / emit on the sliding windows (info words) or on the keyframe sets (kSet: chain records) into the caller's batch o, whose total_lm /
// total_edge are its capacities.  The builder WRITES the arrays that the optimiser's view of the struct declares const: the casts live here.
template <bool kSet>
static void launch_window_kernels(const TrackTables& t, const vslam_tracks_in& in, const WindowTables& w, const WindowSet& ws, const vslam_ba_batch& o, int32_t* d_status,
                                  hipStream_t stream) {
    const TrackDims& d = t.d;
    const int32_t* info = t.cand; // (the candidate words live in the info table until track_info_kernel writes it)
    hipLaunchKernelGGL(window_count_kernel<kSet>, dim3(d.B), dim3(256), 0, stream, d, info, in.d_nkps, w.counts, w.hist, ws);
    hipLaunchKernelGGL(window_scan_kernel<kSet>, dim3(1), dim3(256), 0, stream, d, w.counts, o.total_lm, o.total_edge, const_cast<int32_t*>(o.d_lm_off),
                       const_cast<int32_t*>(o.d_edge_off), const_cast<int32_t*>(o.d_n_kf), d_status, w.set_flags, w.nmem);
    hipLaunchKernelGGL(window_rank_kernel<kSet>, dim3(d.B), dim3(kRankBlock), 0, stream, d, w.G, w.counts, w.hist, info, in.d_nkps, o.d_lm_off, o.d_edge_off, o.d_T_c_w, w.head_rec, ws);
    hipLaunchKernelGGL(window_emit_kernel<kSet>, dim3((o.total_lm + 255) / 256), dim3(256), 0, stream, d, in.d_kps, in.d_xyz, t.kp2lr, t.root, t.relsrc, t.succ, w.G, in.d_carry_in, w.hist,
                       w.head_rec, o.d_lm_off, o.d_edge_off, o.d_xyz, const_cast<uint8_t*>(o.d_reliable), o.d_lm_inlier, const_cast<int32_t*>(o.d_kf_idx),
                       const_cast<int32_t*>(o.d_lm_idx), const_cast<float*>(o.d_uv), ws);
}

int launch_build_windows(const vslam_tracks_in& in, const vslam_ba_batch& out, int32_t* d_status, const TrackParams& tp, const KfPolicy& kp, DevBuf& scratch, hipStream_t stream,
                         const SegView& seg) {
    TrackTables t(in, out.n_kf, tp, seg);
    const TrackDims& d = t.d;
    const bool cull = kp.policy == 1 || kp.gate; // (cull: the set-templated window kernels)
    WindowTables w;
    MapRecover rv = {kp.pred_table, nullptr, nullptr}; int32_t* r_flags = nullptr; // (kp.recover: the pairing of the states, built on kp.pred_table)
    if (int rc = carve(scratch, stream, [&](Layout& L) {
            t.take(L, kp.recover);
            w.G = L.take<double>((size_t)d.B * 7);
            w.counts = L.take<int32_t>((size_t)d.B * 2);
            w.hist = L.take<int32_t>((size_t)d.B * (VSLAM_MAX_KF + 1));
            w.head_rec = L.take<uint32_t>(out.total_lm);
            if (cull) { // the chain records, the distance band, the set kernel's flags; the gate: also the member counts
                w.ends = L.take<int2>(t.tab());
                w.D = L.take<double>((size_t)d.B * kKfBand);
                w.set_flags = L.take<int32_t>(64);
                if (kp.gate) w.nmem = L.take<int32_t>(d.B);
            }
            if (kp.recover) { rv.d_pred = L.take<int32_t>(d.B); rv.d_gap = L.take<double>(d.B); r_flags = L.take<int32_t>(64); }
        })) return rc;
    WindowSet ws = {kp.kf_frame, w.ends, t.root, w.nmem};
    ws.nxt = t.nxt; ws.lm_id = kp.lm_id;
    ProfScope prof__(stream, "build_windows_kernels", 9);
    if (kp.recover) VS_HIP(hipMemsetAsync(r_flags, 0, sizeof(int32_t), stream)); // (the pairing's flags reach d_status at the end)
    launch_track_init(t, in, kp.recover ? &rv : nullptr, kp.state_in, r_flags, stream);
    if (kp.G) VS_HIP(hipMemcpyAsync(w.G, kp.G, sizeof(double) * 7 * (size_t)d.B, hipMemcpyDeviceToDevice, stream)); // (the map builder: the caller's poses)
    else if (in.d_T_abs) VS_HIP(hipMemcpyAsync(w.G, in.d_T_abs, sizeof(double) * 7 * (size_t)d.B, hipMemcpyDeviceToDevice, stream)); // (a chunk: poses in the sequence's world)
    else hipLaunchKernelGGL(track_pose_chain_kernel, dim3(t.seg_grid()), dim3(256), 0, stream, d.B, in.d_T_rel, w.G, seg.first);
    const int32_t* state = kp.recover ? t.r_state : kp.state_in ? kp.state_in : kp.frame_state; // (the map builder: the caller's states; recover: with the Lost frames marked)
    if (cull && seg.first) VS_HIP(hipMemsetAsync(w.set_flags, 0, sizeof(int32_t), stream)); // (the segments' waves OR their flags into the word)
    launch_kf_sets(d.B, out.n_kf, in, kp, w, state, t.seg_grid(), seg, stream);
    launch_track_walk(t, in, kp.in_of_match, w.G, in.d_carry_in, kp.gate ? state : nullptr, stream);
    const dim3 node_grid((d.kp_cap + 255) / 256, d.B);
    if (!kp.recover) // (the info words serve the sliding windows; the recovered windows are set windows, which read root / ends)
        hipLaunchKernelGGL(track_info_kernel, node_grid, dim3(256), 0, stream, d, t.pred, t.succ, t.root, in.d_carry_in, t.cand);
    if (in.d_carry_out && in.carry_out_frame > 0 && in.carry_out_frame < d.B)
        hipLaunchKernelGGL(track_carry_out_kernel, dim3((d.kp_cap + 255) / 256), dim3(256), 0, stream, d, in.carry_out_frame, t.kp2lr, t.pred, t.root, t.relsrc, in.d_xyz, w.G,
                           in.d_carry_in, in.d_carry_out);
    if (cull) {
        hipLaunchKernelGGL(track_ends_kernel, node_grid, dim3(256), 0, stream, d, t.succ, t.root, t.relsrc, w.ends);
        launch_window_kernels<true>(t, in, w, ws, out, d_status, stream);
        if (kp.recover) hipLaunchKernelGGL(status_or_kernel, dim3(1), dim3(1), 0, stream, d_status, r_flags);
    } else
        launch_window_kernels<false>(t, in, w, ws, out, d_status, stream);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

// ---- G[0] = identity, G[f] = T_rel[f - 1] o G[f - 1]: the builders' chain on its own (vslam_chain_poses_dev)
int launch_chain_poses(int n_frames, const double* d_T_rel, double* d_G, hipStream_t stream, const SegView& seg) {
    ProfScope prof__(stream, "track_pose_chain_kernel");
    hipLaunchKernelGGL(track_pose_chain_kernel, dim3(seg.first ? seg.n_seg : 1), dim3(256), 0, stream, n_frames, d_T_rel, d_G, seg.first);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

// ---- the keyframe gate on its own (vslam_gate_states_dev): on the relative poses (the gated builder's states, bit for bit) or on absolute ones
int launch_gate_states(int n_frames, const double* d_T, int absolute, const int32_t* d_num_inliers, int32_t* d_state, hipStream_t stream, const SegView& seg) {
    ProfScope prof__(stream, "kf_gate_kernel");
    if (absolute) hipLaunchKernelGGL(kf_gate_kernel<true>, dim3((n_frames + 255) / 256), dim3(256), 0, stream, n_frames, d_num_inliers, d_T, d_state, seg.start);
    else hipLaunchKernelGGL(kf_gate_kernel<false>, dim3((n_frames + 255) / 256), dim3(256), 0, stream, n_frames, d_num_inliers, d_T, d_state, seg.start);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

// ---- the pairing on its own (vslam_frame_pairs_dev) and the gate against it (vslam_gate_states_pairs_dev: raw states, then the Lost scan in place;
// the scan's pred / gap go to scratch)
int launch_frame_pairs(int n_frames, const int32_t* d_state, int32_t* d_pred, double* d_gap, hipStream_t stream, const SegView& seg) {
    ProfScope prof__(stream, "frame_pairs_kernel");
    hipLaunchKernelGGL(frame_pairs_kernel, dim3(seg.first ? seg.n_seg : 1), dim3(256), 0, stream, n_frames, d_state, (int32_t*)nullptr, d_pred, d_gap, (int32_t*)nullptr,
                       (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, seg.first);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_gate_states_pairs(int n_frames, const double* d_G, const int32_t* d_pred, const int32_t* d_num_inliers, int32_t* d_state, DevBuf& scratch,
                             hipStream_t stream, const SegView& seg) {
    int32_t* s_pred; double* s_gap;
    if (int rc = carve(scratch, stream, [&](Layout& L) { s_pred = L.take<int32_t>(n_frames); s_gap = L.take<double>(n_frames); })) return rc;
    ProfScope prof__(stream, "kf_gate_pairs_kernel", 2);
    hipLaunchKernelGGL(kf_gate_pairs_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, stream, n_frames, d_num_inliers, d_G, d_pred, d_state, seg.start);
    hipLaunchKernelGGL(frame_pairs_kernel, dim3(seg.first ? seg.n_seg : 1), dim3(256), 0, stream, n_frames, d_state, d_state, s_pred, s_gap, (int32_t*)nullptr, (const int32_t*)nullptr,
                       (int32_t*)nullptr, (int32_t*)nullptr, seg.first);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

int launch_seg_expand(int n_frames, int n_seg, const int32_t* d_first, int32_t* d_start, int32_t* d_qitem, hipStream_t stream) {
    hipLaunchKernelGGL(seg_expand_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, stream, n_frames, n_seg, d_first, d_start, d_qitem);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

// ---- one refinement pass's pose inputs (vslam_build_map_pnp_inputs_dev): the walk of the builders on the caller's poses G and the previous pass's
// links (in_of_match_prev, or the pose stage's own-depth flags and track_rule when it is null), then the map inputs of every frame pair.
// d_state (vslam_build_map_pnp_inputs_gated_dev; else null): the previous pass's frame states -- the gated walk, a non-keyframe creates nothing.
// rq (vslam_build_map_pnp_inputs_requery_dev; else null): between the walk and the emit every pair is RE-MATCHED with the features of its first frame
// as the query set (track_features_kernel + the subset matcher), and the inputs are emitted on that table instead of in.d_f2f
// rv (vslam_build_map_pnp_inputs_recover_dev, with rq; else null): d_state also gives the pairing -- every frame against its last accepted predecessor,
// Lost frames without one (frame_pairs_kernel: rv->d_pred, rv->d_gap) --, the walk honours a pair's links only when in.d_f2f was built on that pairing
// (rv->d_pred_prev) and steps through the accepted frames, and pair f - 1 is re-matched from the features of pred(f) at gap f - pred(f)
int launch_map_pnp_inputs(const vslam_tracks_in& in, const double* d_G, const int32_t* d_in_of_match_prev, const int32_t* d_state, const TrackParams& tp, const MapInputsOut& out,
                          const MapRequery* rq, const MapRecover* rv, DevBuf& scratch, hipStream_t stream, const SegView& seg) {
    TrackTables t(in, 1, tp, seg);
    const TrackDims& d = t.d;
    double* gap = nullptr;
    if (int rc = carve(scratch, stream, [&](Layout& L) {
            t.take(L, rv != nullptr);
            if (rq && !rv) gap = L.take<double>(d.B);
        })) return rc;
    ProfScope prof__(stream, "map_pnp_inputs_kernels", 4);
    VS_HIP(hipMemsetAsync(out.status, 0, sizeof(int32_t), stream));
    if (d.B < 2) {
        if (rq) VS_HIP(hipMemsetAsync(rq->d_nfeat, 0, sizeof(int32_t) * d.B, stream)); // (no pair: no walk, no list)
        if (rv) VS_HIP(hipMemsetAsync(rv->d_pred, 0xFF, sizeof(int32_t) * d.B, stream)); // (frame 0 has no predecessor; no gap entry)
        return VSLAM_OK;
    }
    launch_track_init(t, in, rv, d_state, out.status, stream); // (rv: the flags -- a Lost frame, an out-of-range state or d_pred_prev entry -- go straight into the status word)
    launch_track_walk(t, in, d_in_of_match_prev, d_G, nullptr, d_state && rv ? t.r_state : d_state, stream);
    const vslam_dmatch* f2f = in.d_f2f; const int32_t* nf2f = in.d_nf2f;
    if (rq) { // pair i: queries = the features of frame i, trains = every keypoint of frame i + 1, the gate of VO::feature_matching at frame_gap 1
        hipLaunchKernelGGL(track_features_kernel, dim3(d.B), dim3(256), 0, stream, d, t.root, in.d_nkps, rq->d_feat, rq->d_nfeat, gap);
        prof_end(stream); // (the matcher brackets its own kernels: this bracket closes before it ...
        // (rv: item i's query block is frame pred(i + 1) -- the d_qitem path, block indices = frame indices -- at the pairing's gaps; segments: the same
        // path with block i for item i and -1 for a boundary item, which the matcher leaves empty without running on it.  pred = -1 at a segment's first frame)
        if (int rc = launch_match(rq->d_desc, rq->desc_stride, in.d_nkps, rq->d_desc + rq->desc_stride, rq->desc_stride, in.d_nkps + 1, rv ? rv->d_gap : gap, 1,
                                  rq->ratio, rq->gap_thr, d.B - 1, d.kp_cap, rq->d_train_best, rq->d_f2f_out, d.match_cap, rq->d_nf2f_out, stream, rq->d_feat,
                                  d.kp_cap, rq->d_nfeat, rv ? rv->d_pred + 1 : seg.qitem, rv || seg.qitem ? d.B : 0)) return rc;
        prof_begin(stream, "track_map_inputs_kernel", 1); // ... and prof__ closes this one, around the emit)
        f2f = rq->d_f2f_out; nf2f = rq->d_nf2f_out;
    }
    hipLaunchKernelGGL(track_map_inputs_kernel, dim3(d.B - 1), dim3(256), 0, stream, d, f2f, nf2f, in.d_kps, in.d_xyz, t.kp2lr, t.root, t.relsrc, d_G,
                       out.capacity, out.xyz, out.uv, out.n, out.in_of_match, out.status, rv ? rv->d_pred + 1 : nullptr);
    VS_HIP(hipGetLastError());
    return VSLAM_OK;
}

} // namespace vslam
