"""Throughput-mode keyframe pipeline: B independent stereo keyframes per step, everything device-resident.

One step = the hot path BASELINE.json's metric names, over a batch of B stereo keyframes:
    ORB detect+ANMS+describe on the B left and B right images (one 2B-image launch set)
 -> L/R cross-checked Hamming match + gate          (stereo association, north_star)
 -> gather matched pixels -> rectified-stereo DLT triangulation (+ depth gates of set_ref_3d_position)
 -> frame-to-frame match: keyframe b-1 (query) vs keyframe b (train)      (VO::feature_matching, :575)
 -> 3D(prev, triangulated) - 2D(cur) gather -> motion-only LM pose (10 its) (VO::motion_estimation substitute)
 -> BA windows built ON THE DEVICE from the step's own tracks (ba_windows="tracks": window b = keyframes [b-9, b] of the batch, the
    landmarks / observations VO::insert_key_frame would have recorded, optimization.cpp:127-214) -- or B canned synthetic windows of the
    BASELINE config-4 shape (ba_windows="synthetic": 10 KF x ~3000 landmarks)
 -> local BA on the B windows: schedule 5+5+10 LM + 10 pose-only (run_vslam.cpp:58-71)
torch is used only for device memory and the stream; every stage is a C-ABI call into libvslam_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import BaBatch, DMATCH_DTYPE, KEYPOINT_DTYPE, LOOP_EDGE_DTYPE, TracksIn, VO, _sgbm_params, default_params, sgbm_params_check
from . import synth
from .dense import write_ply  # noqa: F401  (re-exported)
from .trajectory import assemble_trajectories, assemble_trajectory, sliding_keyframes, write_trajectory  # noqa: F401  (re-exported)


def _copy_struct(st):
    """a ctypes struct with the same field values (pointers included)"""
    return type(st).from_buffer_copy(st)


class KeyframePipeline:
    def __init__(self, B, device=0, anms_num=1500, n_lm=3000, n_kf=10, unique_frames=64, unique_windows=None, seed=0, verbose=False,
                 with_ba=True, depth="match", frame_range=None, render_workers=0, sequence=None, ba_windows="synthetic",
                 lm_per_window=None, edges_per_window=None, pose="lm", window_policy="sliding", near_dist=0.2,
                 keyframe_gate=False, pose_inputs="own_depth", pose_passes=1, f2f_queries="all", sgbm_params=None, rejected_frames="pass_through",
                 rectify=None, raw_images=None, segments=None, segment_sequences=None, ba_chain=False, ba_chain_min_kf=None, landmark_ids=False):
        """depth = "match": north_star stage (right-image ORB, L/R match, DLT); "sgbm": the reference's own depth path
        (VO::disparity_map + Frame::find_3d on the left keypoints; the right image is only consumed by SGBM).
        sgbm_params (depth="sgbm"): the StereoSGBM set of the batched disparity call -- an SgbmParams, a dict of its fields or a tuple
        (num_disparities, block_size[, P1, P2, ...]); None = the reference's (96, 9, 648, 2592, 1, 63, 10, 100, 32).
        Inputs: ONE rendered sequence of `unique_frames` consecutive stereo keyframes, laid over the batch as a ping-pong
        (0, 1, ..., n-1, n-2, ..., 1, 0, 1, ...), so that every item b >= 1 and its predecessor are adjacent frames of the same
        scene (driving the sequence backwards is as valid a frame-to-frame pair as driving it forwards); `unique_windows` BA
        windows (default: one per batch item).  frame_range = (first, last + 1, F): sequence mode -- the batch is the contiguous
        chunk [first, last] of an F-frame sequence (frame f shows ping-pong frame f of the SAME rendered scene on every rank).
        window_policy (ba_windows="tracks"): "sliding" -- window b = keyframes [b - n_kf + 1, b] (vslam_build_windows_dev); "reference" -- the
        keyframes Map::remove_keyframe's culling keeps (map.cpp:48-130; vslam_build_windows_kf_dev policy 1, nearest frame evicted when closer than
        near_dist, else the farthest).
        keyframe_gate (ba_windows="tracks"): insert_key_frame's gate (visual_odometry.cpp:353) on the pose stage's inlier counts and poses --
        only keyframes create landmarks, record observations and enter the windows' keyframe sets (vslam_build_windows_gated_dev; window_policy
        "sliding" evicts the oldest keyframe, "reference" culls); a non-keyframe step's window is empty.  Not available in sequence mode.
        pose_inputs (ba_windows="tracks"): "own_depth" -- the pose stage's inputs are the matches whose last-frame keypoint has a depth of its own, at
        that camera-frame point, poses relative and chained; "map" -- after that stage, `pose_passes` refinement passes solve every frame against the
        MAP, as VO::motion_estimation does (visual_odometry.cpp:260-277: every matched feature of the last frame at its landmark's position), each pass
        parallel over the batch (vslam_build_map_pnp_inputs_dev; after K passes frames 0..K are the sequential loop's), and the windows are built on
        the last pass's poses and links (vslam_build_windows_map_dev).  Not with keyframe_gate=True or in sequence mode.
        keyframe_gate="per_pass" (pose_inputs="map"): the gate inside the passes -- states^0 from stage A's inlier counts and relative poses, pass k walks
        the tracks with states^{k-1} (a non-keyframe creates no landmark and takes no reliable depth), solves, and takes states^k from its own inlier
        counts and poses (vslam_gate_states_dev); the windows are the gated ones on (G^K, links^K, states^K) (vslam_build_windows_map_gated_dev).  After
        K passes frames 0..K are the gated sequential loop's (include/vslam_hip.h).
        f2f_queries: "all" -- the frame-to-frame table is stage A's, every keypoint of the last frame a query; "features" (pose_inputs="map",
        keyframe_gate="per_pass") -- the reference's query set (visual_odometry.cpp:568-575): pass k re-matches every pair with the features of its
        first frame, as the walk of (table^{k-1}, links^{k-1}, states^{k-1}) finds them, against every keypoint of the second, and solves on that
        table (vslam_build_map_pnp_inputs_requery_dev); stage A's table stays untouched, the windows are built on the last pass's table.
        rejected_frames: "pass_through" -- a frame that check_motion_estimation rejects is treated like a tracked one (tracks run through it, every pair
        is matched at frame_gap 1); "recover" (pose_inputs="map", keyframe_gate="per_pass", f2f_queries="features") -- the reference's failure handling
        (visual_odometry.cpp:630-637, :673-693): a rejected frame and its features are dropped, the next frame is matched against the features of the last
        ACCEPTED frame at their real frame gap, more than ten rejections in a row end in the Lost state 3 (vslam_build_map_pnp_inputs_recover_dev,
        vslam_gate_states_pairs_dev, vslam_build_windows_map_recover_dev); download() adds the last pass's pairing map_pred / map_gap.
        rectify: a RectifyParams -- the rig delivers RAW images: they live in their own device buffer, and stage_rectify() (the first stage of step())
        fills the batch's images from them through the rig's two maps (vslam_rectify_set / vslam_rectify_dev) on the pipeline's stream.  raw_images:
        the (2B, src_h, src_w) uint8 raw images [left 0..B-1 | right 0..B-1]; absent, the rendered frames serve as the raw images (a rig whose
        source size equals the image size).  None: the images are the rendered frames, as before, and stage_rectify is never called.
        segments = [n_0, n_1, ...] (lengths >= 1 that sum to B; ba_windows="tracks", no frame_range): the batch holds that many INDEPENDENT sequences
        laid back to back (vslam_set_segments; the rules are in include/vslam_hip.h): every segment's first frame is an initialisation frame, and
        tracks, the pose chain, frame states and pairings, keyframe sets and windows all restart there, so every output of segment s is bit for bit
        that of KeyframePipeline(B=n_s, sequence=segment_sequences[s]) with the same options.  Segment s shows the frames that pipeline shows;
        segment_sequences = None renders them with seed + 7919 s (PipelineRing's convention).  pose_passes = K gives the sequential loop for frames
        0..K of EVERY segment, so K = max(n_s) - 1 is exact for the whole batch.  Frame indices in download() stay batch-wide; download() adds
        seg_first, trajectories() returns one trajectory per segment.
        ba_chain (ba_windows="tracks", no frame_range): the windows of a sequence run in order, each from the poses and is_inlier flags the previous one
        left (vslam_ba_chain_dev: the reference's carried flags, optimization.cpp:160, and successive schedules, :272-278); the segments run side by side.
        ba_chain_min_kf: the BA runs on windows with at least that many keyframes (None = n_kf: run_vslam.cpp:58's keyframes_.size() >= 10; 1 = every
        non-empty window); a smaller window passes the carried state through.  download() adds ba_lm_id (the landmarks' identities) and ba_ran.
        landmark_ids (ba_windows="tracks", no frame_range): the window builders also write every landmark's identity (vslam_set_window_ids), which
        full_ba() needs; ba_chain implies it.  False: no buffer is allocated and the builders launch what they always launched."""
        assert depth in ("match", "sgbm") and ba_windows in ("synthetic", "tracks") and pose in ("lm", "ransac")
        assert window_policy in ("sliding", "reference") and near_dist >= 0
        assert keyframe_gate in (False, True, "per_pass"), "keyframe_gate: False, True (on stage A's inputs) or 'per_pass' (inside the map passes)"
        per_pass = keyframe_gate == "per_pass"
        assert not keyframe_gate or (ba_windows == "tracks" and frame_range is None), "keyframe_gate needs ba_windows='tracks' and no frame_range"
        assert pose_inputs in ("own_depth", "map")
        assert not per_pass or pose_inputs == "map", "keyframe_gate='per_pass' needs pose_inputs='map'"
        if pose_inputs == "map":
            assert with_ba and ba_windows == "tracks" and int(pose_passes) >= 1, "pose_inputs='map' needs ba_windows='tracks' and pose_passes >= 1"
            assert (per_pass or not keyframe_gate) and frame_range is None, \
                "pose_inputs='map' is not available with keyframe_gate=True (keyframe_gate='per_pass' gates inside the passes) or frame_range"
        assert f2f_queries in ("all", "features")
        assert f2f_queries == "all" or (per_pass and pose_inputs == "map"), "f2f_queries='features' needs pose_inputs='map' and keyframe_gate='per_pass'"
        assert rejected_frames in ("pass_through", "recover")
        assert rejected_frames == "pass_through" or (per_pass and pose_inputs == "map" and f2f_queries == "features"), \
            "rejected_frames='recover' needs pose_inputs='map', keyframe_gate='per_pass' and f2f_queries='features'"
        self.seg_first = None
        if segments is not None:
            segments = [int(n_) for n_ in segments]
            assert len(segments) >= 1 and min(segments) >= 1 and sum(segments) == B, "segments: lengths >= 1 that sum to B"
            assert with_ba and ba_windows == "tracks" and frame_range is None, "segments need ba_windows='tracks' and no frame_range"
            assert sequence is None, "a segmented pipeline takes segment_sequences (one rendered sequence per segment), not sequence"
            assert segment_sequences is None or len(segment_sequences) == len(segments)
            self.seg_first = np.concatenate([[0], np.cumsum(segments)]).astype(np.int32)
        else:
            assert segment_sequences is None, "segment_sequences needs segments"
        self.ba_chain = bool(ba_chain)
        if self.ba_chain:
            assert with_ba and ba_windows == "tracks" and frame_range is None, "ba_chain needs ba_windows='tracks' and no frame_range"
            self.ba_chain_min_kf = n_kf if ba_chain_min_kf is None else int(ba_chain_min_kf)
            assert 1 <= self.ba_chain_min_kf <= n_kf, "ba_chain_min_kf: 1..n_kf"
        else:
            assert ba_chain_min_kf is None, "ba_chain_min_kf needs ba_chain"
        self.landmark_ids = bool(landmark_ids) or self.ba_chain
        assert not self.landmark_ids or (with_ba and ba_windows == "tracks" and frame_range is None), "landmark_ids needs ba_windows='tracks' and no frame_range"
        self.f2f_queries = f2f_queries
        self.rejected_frames = rejected_frames
        self.pose_inputs, self.pose_passes = pose_inputs, int(pose_passes)
        self.window_policy, self.near_dist = window_policy, float(near_dist)
        self.keyframe_gate = "per_pass" if per_pass else bool(keyframe_gate)
        self.depth = depth
        assert sgbm_params is None or depth == "sgbm", "sgbm_params needs depth='sgbm'"
        self.sgbm_params = _sgbm_params(sgbm_params)
        self.pose = pose   # "lm": north_star motion-only LM; "ransac": the reference's cv::solvePnPRansac(..., 100, 4.0, 0.99) (visual_odometry.cpp:277)
        self.ba_windows = ba_windows
        self.B = B
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        # One explicit stream for the library AND for the few torch ops between its calls (copies of initial guesses, the pose
        # gather): torch's default stream has handle 0, which the C-ABI reads as "create your own stream" -- the two would race.
        self.stream = torch.cuda.Stream(self.dev)
        self.with_ba = with_ba
        p = default_params(max_batch=2 * B, anms_num=anms_num)
        self.vo = VO(params=p, device=device, stream=self.stream.cuda_stream)
        self.cap = p.kp_capacity
        self.w, self.h = p.img_w, p.img_h
        self.pitch = (self.w + 63) // 64 * 64
        if self.sgbm_params is not None:
            sgbm_params_check(self.sgbm_params, self.w, self.h)  # (raises VslamError: a refused set never reaches the batched call)
        self.img_bytes = self.pitch * self.h
        d = self.dev
        # ---- inputs: 2B images [left 0..B-1 | right 0..B-1]; consecutive keyframes of `unique_scenes` short sequences
        imgs = np.zeros((2 * B, self.h, self.pitch), np.uint8)
        if self.seg_first is None:
            n_u = max(2, min(unique_frames, B if frame_range is None else int(frame_range[2]))) if (B > 1 or frame_range is not None) else 1
            # `sequence`: an already rendered synth.stereo_sequence(n_u, seed) (tests that build several pipelines over the same frames)
            seq = sequence if sequence is not None else synth.stereo_sequence(n_u, seed=seed, w=self.w, h=self.h, workers=render_workers)
            assert len(seq) == n_u, (len(seq), n_u)
            if verbose:
                print("rendered %d stereo keyframes" % n_u, flush=True)
            period = max(2 * (n_u - 1), 1)
            f0 = 0
            if frame_range is not None:
                f0 = int(frame_range[0])
                assert int(frame_range[1]) - f0 == B
            self.frame_of = [(t if t < n_u else period - t) for t in ((f0 + b) % period for b in range(B))]
            self.unique_frames = n_u
        else:   # every segment laid out as the pipeline of its length alone lays out its batch; frame_of indexes the sequences joined end to end
            self.h_seqs, self.frame_of, seq = [], [], []
            for s_, n_s in enumerate(segments):
                n_u = max(2, min(unique_frames, n_s)) if n_s > 1 else 1
                sq = segment_sequences[s_] if segment_sequences is not None else \
                    synth.stereo_sequence(n_u, seed=seed + 7919 * s_, w=self.w, h=self.h, workers=render_workers)
                assert len(sq) == n_u, (s_, len(sq), n_u)
                period = max(2 * (n_u - 1), 1)
                self.frame_of += [len(seq) + (t if t < n_u else period - t) for t in (b % period for b in range(n_s))]
                self.h_seqs.append(sq); seq = seq + list(sq)
            if verbose:
                print("rendered %d stereo keyframes in %d segments" % (len(seq), len(segments)), flush=True)
            self.unique_frames = unique_frames   # (the per-segment cap, as given: PipelineRing hands it to its other pipelines)
        for b in range(B):
            L, R, _, _ = seq[self.frame_of[b]]
            imgs[b, :, :self.w] = L
            imgs[B + b, :, :self.w] = R
        self.h_seq = seq   # (kept: a second pipeline over the same frames needs no second rendering)
        self.h_imgs = imgs
        self.h_imgs_unique_left = np.stack([np.pad(f[0], ((0, 0), (0, self.pitch - self.w))) for f in seq])
        self.h_imgs_unique_right = np.stack([np.pad(f[1], ((0, 0), (0, self.pitch - self.w))) for f in seq])
        self.rectify = rectify
        if rectify is None:
            assert raw_images is None, "raw_images needs rectify"
            self.d_imgs = torch.from_numpy(imgs).to(d)
        else:
            self.src_w, self.src_h = int(rectify.src_w), int(rectify.src_h)
            if raw_images is None:
                assert (self.src_w, self.src_h) == (self.w, self.h), "rendered frames as raw images need a rig whose source size is the image size"
                raw_images = imgs[:, :, :self.w]
            raw_images = np.asarray(raw_images, np.uint8)
            assert raw_images.shape == (2 * B, self.src_h, self.src_w), (raw_images.shape, (2 * B, self.src_h, self.src_w))
            self.src_pitch = (self.src_w + 63) // 64 * 64
            self.src_img_bytes = self.src_pitch * self.src_h
            raw = np.zeros((2 * B, self.src_h, self.src_pitch), np.uint8)
            raw[:, :, :self.src_w] = raw_images
            self.vo.rectify_set(rectify)   # (raises VslamError naming the field: a refused rig never reaches the batched call)
            self.d_raw = torch.from_numpy(raw).to(d)
            self.d_imgs = torch.zeros((2 * B, self.h, self.pitch), dtype=torch.uint8, device=d)   # filled by stage_rectify()
        # ---- ORB outputs
        self.d_kps = torch.zeros((2 * B, self.cap, 28), dtype=torch.uint8, device=d)
        self.d_desc = torch.zeros((2 * B, self.cap, 32), dtype=torch.uint8, device=d)
        self.d_cnt = torch.zeros(2 * B, dtype=torch.int32, device=d)
        # ---- matches (L/R and frame-to-frame)
        self.d_gap = torch.ones(B, dtype=torch.float64, device=d)
        self.d_lr = torch.zeros((B, self.cap, 16), dtype=torch.uint8, device=d)
        self.d_nlr = torch.zeros(B, dtype=torch.int32, device=d)
        self.d_f2f = torch.zeros((B, self.cap, 16), dtype=torch.uint8, device=d)
        self.d_nf2f = torch.zeros(B, dtype=torch.int32, device=d)
        # ---- triangulation
        self.d_uvL = torch.zeros((B, self.cap, 2), dtype=torch.float32, device=d)
        self.d_uvR = torch.zeros((B, self.cap, 2), dtype=torch.float32, device=d)
        ident = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (B, 1))
        self.d_Tident = torch.from_numpy(ident).to(d)
        self.d_xyz = torch.zeros((B, self.cap, 3), dtype=torch.float32, device=d)
        self.d_valid = torch.zeros((B, self.cap), dtype=torch.uint8, device=d)
        self.d_rel = torch.zeros((B, self.cap), dtype=torch.uint8, device=d)
        if depth == "sgbm":
            self.d_disp = torch.zeros((B, self.h, self.w), dtype=torch.float32, device=d)
            ident_lr = np.zeros((B, self.cap), DMATCH_DTYPE)
            ident_lr["queryIdx"] = np.arange(self.cap)[None, :]; ident_lr["trainIdx"] = np.arange(self.cap)[None, :]
            self.d_lr = torch.from_numpy(ident_lr.view(np.uint8).reshape(B, self.cap, 16)).to(d)  # keypoint i <-> landmark slot i
        # ---- PnP
        self.d_kp2lr = torch.zeros((B, self.cap), dtype=torch.int32, device=d)
        self.d_pxyz = torch.zeros((B, self.cap, 3), dtype=torch.float32, device=d)
        self.d_puv = torch.zeros((B, self.cap, 2), dtype=torch.float32, device=d)
        self.d_pn = torch.zeros(B, dtype=torch.int32, device=d)
        self.d_Tpnp = torch.from_numpy(ident.copy()).to(d)
        self.d_inl = torch.zeros((B, self.cap), dtype=torch.uint8, device=d)
        self.d_ninl = torch.zeros(B, dtype=torch.int32, device=d)
        # ---- local-BA windows built on the device from this step's tracks (vslam_build_windows_dev)
        if with_ba and ba_windows == "tracks":
            self.n_kf = n_kf
            # capacities of the concatenated window arrays: L/R match + DLT gives ~1/3 of the keypoints a depth, the disparity map nearly all
            if lm_per_window is None:
                lm_per_window = n_kf * anms_num if depth == "sgbm" else max(4 * n_kf * anms_num // 10, 1024)
            if edges_per_window is None:
                edges_per_window = lm_per_window + lm_per_window // 3
            self.lm_capacity, self.edge_capacity = B * lm_per_window, B * edges_per_window
            self.ba_T = torch.zeros((B, n_kf, 7), dtype=torch.float64, device=d)
            self.ba_xyz = torch.zeros((self.lm_capacity, 3), dtype=torch.float32, device=d)
            self.ba_rel = torch.zeros(self.lm_capacity, dtype=torch.uint8, device=d)
            self.ba_inl = torch.zeros(self.lm_capacity, dtype=torch.uint8, device=d)
            self.ba_kf = torch.zeros(self.edge_capacity, dtype=torch.int32, device=d)
            self.ba_lm = torch.zeros(self.edge_capacity, dtype=torch.int32, device=d)
            self.ba_uv = torch.zeros((self.edge_capacity, 2), dtype=torch.float32, device=d)
            self.ba_lm_off = torch.zeros(B + 1, dtype=torch.int32, device=d)
            self.ba_e_off = torch.zeros(B + 1, dtype=torch.int32, device=d)
            self.ba_nkf = torch.zeros(B, dtype=torch.int32, device=d)
            self.ba_build_status = torch.zeros(1, dtype=torch.int32, device=d)
            self.ba_chi2 = torch.zeros(1, dtype=torch.float64, device=d)
            if self._builder_writes_kf:
                self.ba_kf_frame = torch.zeros((B, n_kf), dtype=torch.int32, device=d)
                self.ba_evicted = torch.zeros(B, dtype=torch.int32, device=d)
            if keyframe_gate:   # (per_pass: the latest pass's states, updated in place pass by pass)
                self.ba_frame_state = torch.zeros(B, dtype=torch.int32, device=d)
            if self.landmark_ids:   # the landmarks' identities (written by the builder)
                self.ba_lm_id = torch.zeros(self.lm_capacity, dtype=torch.int32, device=d)
            if self.ba_chain:   # which windows the chain ran
                self.ba_ran = torch.zeros(B, dtype=torch.int32, device=d)
            tr = TracksIn()
            tr.n_frames = B; tr.kp_capacity = self.cap; tr.lr_capacity = self.cap; tr.match_capacity = self.cap; tr.pnp_capacity = self.cap
            tr.d_kps = self.d_kps.data_ptr(); tr.d_lr = self.d_lr.data_ptr(); tr.d_nlr = self.d_nlr.data_ptr(); tr.d_xyz = self.d_xyz.data_ptr()
            tr.d_valid = self.d_valid.data_ptr(); tr.d_reliable = self.d_rel.data_ptr(); tr.d_f2f = self.d_f2f.data_ptr()
            tr.d_nf2f = self.d_nf2f.data_ptr(); tr.d_pose_inlier = self.d_inl.data_ptr(); tr.d_T_rel = self.d_Tpnp.data_ptr()
            tr.d_nkps = self.d_cnt.data_ptr()   # (the first B counts: the left images)
            self.tracks = tr
            if pose_inputs == "map":
                # refinement passes: poses G^k (B x 7, double-buffered), the pass's inputs, its index map and inlier flags (double-buffered)
                self.map_G = [torch.zeros((B, 7), dtype=torch.float64, device=d) for _ in range(2)]
                self.map_T = torch.zeros((B, 7), dtype=torch.float64, device=d)
                self.map_xyz = torch.zeros((B, self.cap, 3), dtype=torch.float32, device=d)
                self.map_uv = torch.zeros((B, self.cap, 2), dtype=torch.float32, device=d)
                self.map_n = torch.zeros(B, dtype=torch.int32, device=d)
                self.map_index = [torch.full((B, self.cap), -1, dtype=torch.int32, device=d) for _ in range(2)]
                self.map_inl = [torch.zeros((B, self.cap), dtype=torch.uint8, device=d) for _ in range(2)]
                self.map_ninl = torch.zeros(B, dtype=torch.int32, device=d)
                self.map_status = torch.zeros(1, dtype=torch.int32, device=d)
                self.map_cur = 0
                if per_pass:    # (the states the last pass started from: what it changed is a report)
                    self.map_state_prev = torch.zeros(B, dtype=torch.int32, device=d)
                self.map_tracks = _copy_struct(tr)
                if f2f_queries == "features":   # table^k alternates between two buffers (table^0 = stage A's d_f2f); the last pass's feature lists
                    self.map_f2f = [torch.zeros((B, self.cap, 16), dtype=torch.uint8, device=d) for _ in range(2)]
                    self.map_nf2f = [torch.zeros(B, dtype=torch.int32, device=d) for _ in range(2)]
                    self.map_feat = torch.zeros((B, self.cap), dtype=torch.int32, device=d)
                    self.map_nfeat = torch.zeros(B, dtype=torch.int32, device=d)
                    self.map_table = None   # (index into map_f2f of the last pass's table)
                if rejected_frames == "recover":   # pred^k alternates like the tables (a pass reads the pairing its table was built on); the last pass's gaps
                    self.map_pred = [torch.full((B,), -1, dtype=torch.int32, device=d) for _ in range(2)]
                    self.map_gap = torch.ones(B, dtype=torch.float64, device=d)
            self.ba_batch = self._make_ba_batch(self.lm_capacity, self.edge_capacity, self.ba_rel, self.ba_nkf)
            self.unique_windows = B
            if self.landmark_ids:   # context state, like the segment table: every builder of this context writes the ids from here on
                self.vo.set_window_ids(self.ba_lm_id.data_ptr(), self.lm_capacity)
            if self.seg_first is not None:   # the table is context state: every consecutive-frame entry of this context honours it from here on
                self.vo.set_segments(self.seg_first)
                ft = torch.from_numpy(self.seg_first.astype(np.int64)).to(d)
                self.seg_starts = ft[:-1]            # the segments' first frames
                self.seg_boundary = ft[1:-1] - 1     # the items (pairs) that straddle two segments
                self.seg_start_of = torch.repeat_interleave(ft[:-1], ft[1:] - ft[:-1])   # start(f) per frame
        # ---- canned local-BA windows
        if with_ba and ba_windows == "synthetic":
            unique_windows = B if unique_windows is None else max(1, min(unique_windows, B))
            self.unique_windows = unique_windows
            self.window_seed0 = seed + 100
            wins = [synth.ba_window_fast(n_kf=n_kf, n_lm=n_lm, seed=self.window_seed0 + i) for i in range(unique_windows)]
            self.h_windows = wins
            lm_off, e_off = [0], [0]
            T0, xyz, kf, lm, uv = [], [], [], [], []
            for b in range(B):
                wn = wins[b % unique_windows]
                T0.append(wn["T0"]); xyz.append(wn["xyz"]); kf.append(wn["kf_idx"]); lm.append(wn["lm_idx"]); uv.append(wn["uv"])
                lm_off.append(lm_off[-1] + len(wn["xyz"])); e_off.append(e_off[-1] + len(wn["kf_idx"]))
            self.n_kf = n_kf
            self.ba_T0 = torch.from_numpy(np.stack(T0)).to(d)
            self.ba_T = self.ba_T0.clone()
            self.ba_xyz = torch.from_numpy(np.concatenate(xyz)).to(d)
            self.ba_kf = torch.from_numpy(np.concatenate(kf)).to(d)
            self.ba_lm = torch.from_numpy(np.concatenate(lm)).to(d)
            self.ba_uv = torch.from_numpy(np.concatenate(uv)).to(d)
            self.ba_lm_off = torch.tensor(lm_off, dtype=torch.int32, device=d)
            self.ba_e_off = torch.tensor(e_off, dtype=torch.int32, device=d)
            self.ba_inl = torch.ones(lm_off[-1], dtype=torch.uint8, device=d)
            self.ba_chi2 = torch.zeros(e_off[-1], dtype=torch.float64, device=d)
            self.total_lm, self.total_edge = lm_off[-1], e_off[-1]
            self.h_lm_off = np.array(lm_off, np.int64)
            self.edges_per_window = e_off[-1] / B
            self.lms_per_window = lm_off[-1] / B
            self.ba_batch = self._make_ba_batch(self.total_lm, self.total_edge)
        torch.cuda.synchronize(self.dev)

    def _make_ba_batch(self, total_lm, total_edge, rel=None, nkf=None):
        """the BaBatch over the pipeline's window tensors; rel / nkf: the reliable flags and per-window keyframe counts a builder writes (None: all
        reliable, n_kf keyframes each).  Per-edge chi2 is internal to optimize_map, not one of its outputs; the intrinsics are the context's."""
        bb = BaBatch()
        bb.n_windows = self.B; bb.n_kf = self.n_kf
        bb.d_lm_off = self.ba_lm_off.data_ptr(); bb.d_edge_off = self.ba_e_off.data_ptr(); bb.d_T_c_w = self.ba_T.data_ptr()
        bb.d_xyz = self.ba_xyz.data_ptr(); bb.d_reliable = None if rel is None else rel.data_ptr(); bb.d_lm_inlier = self.ba_inl.data_ptr()
        bb.d_kf_idx = self.ba_kf.data_ptr(); bb.d_lm_idx = self.ba_lm.data_ptr(); bb.d_uv = self.ba_uv.data_ptr()
        bb.d_chi2 = None; bb.d_stats = None; bb.K4 = None; bb.d_n_kf = None if nkf is None else nkf.data_ptr()
        bb.total_lm = total_lm; bb.total_edge = total_edge
        return bb

    # ------------------------------------------------------------------ which entries the options select (tools re-assign options on a live pipeline)
    @property
    def _map_flavour(self):
        """the refinement passes' entry: "recover" / "requery" / "gated" / "plain" (None: pose_inputs="own_depth")"""
        if self.pose_inputs != "map":
            return None
        return "recover" if self.rejected_frames == "recover" else "requery" if self.f2f_queries == "features" else \
            "gated" if self.keyframe_gate == "per_pass" else "plain"

    @property
    def _window_builder(self):
        """the window builder's entry: "map_recover" / "map_gated" / "map" on the passes' output, else "gated" / "kf" / "sliding" on stage A's"""
        if self.pose_inputs == "map":
            return "map_recover" if self.rejected_frames == "recover" else "map_gated" if self.keyframe_gate == "per_pass" else "map"
        return "gated" if self.keyframe_gate else "kf" if self.window_policy == "reference" else "sliding"

    @property
    def _builder_writes_kf(self):
        """the builder writes the keyframe sets ba_kf_frame / ba_evicted (every entry but the plain sliding one)"""
        return self._window_builder != "sliding"

    # ------------------------------------------------------------------ stages
    def stage_rectify(self):
        """raw pairs -> the batch's rectified images (rectify set): one launch for both cameras"""
        B = self.B
        self.vo.rectify_dev(self.d_raw.data_ptr(), self.d_raw.data_ptr() + B * self.src_img_bytes, self.src_img_bytes, self.src_pitch, B,
                            self.d_imgs.data_ptr(), self.d_imgs.data_ptr() + B * self.img_bytes, self.img_bytes, self.pitch)

    def stage_orb(self):
        n_img = self.B if self.depth == "sgbm" else 2 * self.B  # the reference never detects on the right image
        self.vo.feature_detection_dev(self.d_imgs.data_ptr(), self.img_bytes, self.pitch, n_img, self.d_kps.data_ptr(),
                                      self.d_desc.data_ptr(), self.d_cnt.data_ptr())

    def stage_stereo_match(self):
        B, cap = self.B, self.cap
        vo = self.vo
        if self.depth == "sgbm":
            # VO::disparity_map + Frame::find_3d / gates of set_ref_3d_position on every left keypoint (visual_odometry.cpp:159-217)
            vo.disparity_map_dev(self.d_imgs.data_ptr(), self.d_imgs.data_ptr() + B * self.img_bytes, self.img_bytes, self.pitch, self.w, self.h, B,
                                 self.d_disp.data_ptr(), sgbm=self.sgbm_params)
            vo.find_3d_disparity_dev(self.d_kps.data_ptr(), self.d_cnt.data_ptr(), cap, B, self.d_disp.data_ptr(), self.w, self.h,
                                     self.d_Tident.data_ptr(), self.d_xyz.data_ptr(), self.d_valid.data_ptr(), self.d_rel.data_ptr())
            with torch.cuda.stream(self.stream):
                self.d_nlr.copy_(self.d_cnt[:B])
            return
        # L/R: query = left descriptors of keyframe b, train = right descriptors of keyframe b
        vo.feature_matching_dev(self.d_desc.data_ptr(), cap * 32, self.d_cnt.data_ptr(), self.d_desc.data_ptr() + B * cap * 32, cap * 32,
                                self.d_cnt.data_ptr() + 4 * B, self.d_gap.data_ptr(), 1, B, cap, self.d_lr.data_ptr(), cap, self.d_nlr.data_ptr())
        vo.gather_matched_uv_dev(self.d_kps.data_ptr(), self.d_kps.data_ptr() + B * cap * 28, cap, self.d_lr.data_ptr(), self.d_nlr.data_ptr(),
                                 cap, B, self.d_uvL.data_ptr(), self.d_uvR.data_ptr())
        vo.triangulate_dev(self.d_uvL.data_ptr(), self.d_uvR.data_ptr(), self.d_nlr.data_ptr(), cap, B, self.d_Tident.data_ptr(),
                           self.d_xyz.data_ptr(), self.d_valid.data_ptr(), self.d_rel.data_ptr())

    def stage_track(self):
        """keyframe b-1 -> keyframe b for b = 1..B-1 (the first keyframe of the batch has no predecessor in the batch)"""
        B, cap = self.B, self.cap
        if B < 2:
            if self.pose_inputs == "map":   # one frame, no pair: the passes leave G = identity, state 2 and empty tables
                self._map_passes()
            return
        vo, n = self.vo, B - 1
        # query = left descriptors of keyframe b-1 (item i = b-1), train = left descriptors of keyframe b
        vo.feature_matching_dev(self.d_desc.data_ptr(), cap * 32, self.d_cnt.data_ptr(), self.d_desc.data_ptr() + cap * 32, cap * 32,
                                self.d_cnt.data_ptr() + 4, self.d_gap.data_ptr(), 1, n, cap, self.d_f2f.data_ptr(), cap, self.d_nf2f.data_ptr())
        if self.seg_first is not None and len(self.seg_boundary):   # the matcher pairs every frame with the next one: a pair across two segments is no pair
            with torch.cuda.stream(self.stream):
                self.d_nf2f[self.seg_boundary] = 0
        vo.build_pnp_inputs_dev(self.d_f2f.data_ptr(), self.d_nf2f.data_ptr(), cap, self.d_lr.data_ptr(), self.d_nlr.data_ptr(), cap,
                                self.d_xyz.data_ptr(), self.d_valid.data_ptr(), self.d_kps.data_ptr() + cap * 28, cap, n, self.d_kp2lr.data_ptr(),
                                self.d_pxyz.data_ptr(), self.d_puv.data_ptr(), self.d_pn.data_ptr(), cap)
        self._solve(self.d_pxyz, self.d_puv, self.d_pn, self.d_Tpnp, self.d_inl, self.d_ninl, self.d_Tident)
        if self.pose_inputs == "map":
            self._map_passes()

    def _solve(self, xyz, uv, n_in, T, inl, ninl, guess):
        """the pose stage on the B - 1 problems (xyz, uv, n_in): T (B x 7) and the inlier flags / counts"""
        cap, n = self.cap, self.B - 1
        if n == 0:
            return
        if self.pose == "ransac":   # no pose guess is consumed (useExtrinsicGuess = false)
            self.vo.pnp_ransac_dev(xyz.data_ptr(), uv.data_ptr(), n_in.data_ptr(), cap, n, T.data_ptr(), 100, 4.0, 0.99, inl.data_ptr(), ninl.data_ptr(), None)
            return
        with torch.cuda.stream(self.stream):
            T.copy_(guess)
        self.vo.motion_estimation_dev(xyz.data_ptr(), uv.data_ptr(), n_in.data_ptr(), cap, n, T.data_ptr(), 10, inl.data_ptr(), ninl.data_ptr())

    def _map_passes(self):
        """pose_inputs="map": G^0 = the chain of the stage's relative poses, links^0 its flags; pass k solves every frame f against the map of
        (G^{k-1}, links^{k-1}) -- LM from the guess G^{k-1}_f, RANSAC without one -- and an item with no inlier keeps G^k_f = G^{k-1}_{f-1}.
        keyframe_gate="per_pass": states^0 = the gate on stage A's counts and T_rel; pass k walks with states^{k-1}, then gates on its counts and G^k"""
        B, cap, n = self.B, self.cap, self.B - 1
        mt, cur = self.map_tracks, 0
        flavour = self._map_flavour
        gated, rematch, recover = flavour != "plain", flavour in ("requery", "recover"), flavour == "recover"
        self.vo.chain_poses_dev(B, self.d_Tpnp.data_ptr(), self.map_G[cur].data_ptr())
        if gated:
            self.vo.gate_states_dev(B, self.d_Tpnp.data_ptr(), 0, self.d_ninl.data_ptr(), self.ba_frame_state.data_ptr())
        state = self.ba_frame_state.data_ptr() if gated else None
        prev_index, prev_inl, pred_prev = None, self.d_inl, None   # (no pairing: stage A's table is on adjacent frames)
        mt.d_f2f = self.d_f2f.data_ptr(); mt.d_nf2f = self.d_nf2f.data_ptr()   # (table^0: stage A's)
        for k in range(self.pose_passes):
            nxt = cur ^ 1
            G, Gn = self.map_G[cur], self.map_G[nxt]
            mt.d_pose_inlier = prev_inl.data_ptr(); mt.pnp_capacity = cap
            head = (mt, G.data_ptr(), None if prev_index is None else prev_index.data_ptr())
            out = (self.map_xyz.data_ptr(), self.map_uv.data_ptr(), self.map_n.data_ptr(), self.map_index[nxt].data_ptr(), cap)
            status = self.map_status.data_ptr()
            if rematch:   # walk on table^{k-1}, re-match on its features into the other buffer, inputs on that table; the next pass walks on it
                t = k & 1
                rq = (self.d_desc.data_ptr(), cap * 32, self.map_feat.data_ptr(), self.map_nfeat.data_ptr(), self.map_f2f[t].data_ptr(), self.map_nf2f[t].data_ptr())
            if recover:   # ... with every frame matched from its last accepted predecessor; pred^k / gap are outputs, pred^{k-1} the pairing of table^{k-1}
                pred = self.map_pred[t]
                self.vo.build_map_pnp_inputs_recover_dev(*head, None if pred_prev is None else pred_prev.data_ptr(), state, *rq, *out, pred.data_ptr(),
                                                         self.map_gap.data_ptr(), status)
            elif rematch:
                self.vo.build_map_pnp_inputs_requery_dev(*head, state, *rq, *out, status)
            elif gated:
                self.vo.build_map_pnp_inputs_gated_dev(*head, state, *out, status)
            else:
                self.vo.build_map_pnp_inputs_dev(*head, *out, status)
            if rematch:
                mt.d_f2f = self.map_f2f[t].data_ptr(); mt.d_nf2f = self.map_nf2f[t].data_ptr()
                self.map_table = t
            with torch.cuda.stream(self.stream):
                guess = torch.cat([G[1:], G[:1]])   # (item i: frame i + 1; the last row is not read)
            self._solve(self.map_xyz, self.map_uv, self.map_n, self.map_T, self.map_inl[nxt], self.map_ninl, guess)
            with torch.cuda.stream(self.stream):
                Gn[0].copy_(self.d_Tident[0])
                if recover:   # no inlier: the pose of the frame matched against (a Lost frame: of the last accepted frame before the run)
                    keep = torch.cummax(pred, 0).values.clamp(min=0)
                    if self.seg_first is not None:   # (... of its own segment: never earlier than the segment's first frame)
                        keep = torch.maximum(keep, self.seg_start_of)
                    keep = keep[1:].long()
                    Gn[1:].copy_(torch.where((self.map_ninl[:n] > 0)[:, None], self.map_T[:n], G[keep]))
                else:
                    Gn[1:].copy_(torch.where((self.map_ninl[:n] > 0)[:, None], self.map_T[:n], G[:n]))
                if self.seg_first is not None:   # every segment's first frame is its world: the boundary items' solutions and fallbacks are dropped
                    Gn[self.seg_starts] = self.d_Tident[0]
                if gated and k == self.pose_passes - 1:
                    self.map_state_prev.copy_(self.ba_frame_state)
            if recover:   # the gate against the frame matched against, at the pair's gap, then the Lost scan
                self.vo.gate_states_pairs_dev(B, Gn.data_ptr(), pred.data_ptr(), self.map_ninl.data_ptr(), self.ba_frame_state.data_ptr())
                pred_prev = pred
            elif gated:   # (the inputs of this pass were built from the states before: same stream, so overwriting them here is ordered)
                self.vo.gate_states_dev(B, Gn.data_ptr(), 1, self.map_ninl.data_ptr(), self.ba_frame_state.data_ptr())
            prev_index, prev_inl, cur = self.map_index[nxt], self.map_inl[nxt], nxt
        self.map_cur = cur

    def stage_build_windows(self):
        """optimize_map's graph build (optimization.cpp:127-214) + insert_key_frame's bookkeeping (visual_odometry.cpp:363-424) on the device"""
        builder, status = self._window_builder, self.ba_build_status.data_ptr()
        if builder == "sliding":
            return self.vo.build_windows_dev(self.tracks, self.n_kf, self.lm_capacity, self.edge_capacity, self.ba_batch, status)
        policy = (self.n_kf, 1 if self.window_policy == "reference" else 0, self.near_dist)
        outs = (self.lm_capacity, self.edge_capacity, self.ba_batch, self.ba_kf_frame.data_ptr(), self.ba_evicted.data_ptr())
        if builder == "kf":
            self.vo.build_windows_kf_dev(self.tracks, *policy, *outs, status)
        elif builder == "gated":   # (d_ninl item i = the inlier count of frame i + 1)
            self.vo.build_windows_gated_dev(self.tracks, *policy, self.d_ninl.data_ptr(), *outs, self.ba_frame_state.data_ptr(), status)
        else:   # the last pass's poses and links
            c, mt = self.map_cur, self.map_tracks
            mt.d_pose_inlier = self.map_inl[c].data_ptr(); mt.pnp_capacity = self.cap
            head = (mt, self.map_G[c].data_ptr(), self.map_index[c].data_ptr())
            if builder == "map_recover":   # (map_table also names the pairing the last pass's table was built on)
                self.vo.build_windows_map_recover_dev(*head, self.map_pred[self.map_table].data_ptr(), self.ba_frame_state.data_ptr(), *policy, *outs, status)
            elif builder == "map_gated":
                self.vo.build_windows_map_gated_dev(*head, self.ba_frame_state.data_ptr(), *policy, *outs, status)
            else:
                self.vo.build_windows_map_dev(*head, *policy, *outs, status)

    def stage_build_windows_chunk(self, T_abs, carry_in=None, carry_out_frame=0):
        """sequence mode: this batch is the chunk [first, last] of a longer sequence.  T_abs (B, 7): the poses of its frames in the SEQUENCE's world (gathered
        relative poses, chained); carry_in (kp_capacity, 4) f32 or None: the tracks that reach the chunk's first frame from before it (the previous rank's
        carry-out); carry_out_frame > 0: also export that record for this local frame (returned tensor) -- the first frame of the next rank's chunk."""
        d = self.dev
        if not hasattr(self, "d_T_abs"):
            self.d_T_abs = torch.zeros((self.B, 7), dtype=torch.float64, device=d)
            self.d_carry_in = torch.zeros((self.cap, 4), dtype=torch.float32, device=d)
            self.d_carry_out = torch.zeros((self.cap, 4), dtype=torch.float32, device=d)
        with torch.cuda.stream(self.stream):
            self.d_T_abs.copy_(T_abs.to(d))
            if carry_in is not None:
                self.d_carry_in.copy_(carry_in.to(d))
        tr = self.tracks
        tr.d_T_abs = self.d_T_abs.data_ptr()
        tr.d_carry_in = self.d_carry_in.data_ptr() if carry_in is not None else None
        tr.d_carry_out = self.d_carry_out.data_ptr() if carry_out_frame > 0 else None
        tr.carry_out_frame = int(carry_out_frame)
        self.stage_build_windows()
        tr.d_T_abs = None; tr.d_carry_in = None; tr.d_carry_out = None; tr.carry_out_frame = 0
        return self.d_carry_out if carry_out_frame > 0 else None

    def ba_schedule_from(self, first):
        """the BA schedule on the built windows [first, B) only (sequence mode: the windows of the frames this rank OWNS; the ones before belong to its halo)"""
        b = _copy_struct(self.ba_batch)
        b.n_windows = self.B - first
        b.d_lm_off = self.ba_lm_off[first:].data_ptr(); b.d_edge_off = self.ba_e_off[first:].data_ptr()
        b.d_T_c_w = self.ba_T[first:].data_ptr(); b.d_n_kf = self.ba_nkf[first:].data_ptr()
        self._ba_view = b   # (kept alive until the next call)
        self.vo.ba_batch_dev(b, schedule=1)

    def stage_ba(self):
        if not self.with_ba:
            return
        if self.ba_windows == "tracks":
            self.stage_build_windows()
            if self.ba_chain:
                self.vo.ba_chain_dev(self.ba_batch, self.ba_lm_id.data_ptr(), self._chain_kf_frame(), self.ba_chain_min_kf, self.ba_ran.data_ptr())
            else:
                self.vo.ba_batch_dev(self.ba_batch, schedule=1)
            return
        with torch.cuda.stream(self.stream):
            self.ba_T.copy_(self.ba_T0)
            self.ba_inl.fill_(1)
        self.vo.ba_batch_dev(self.ba_batch, schedule=1)

    def _chain_kf_frame(self):
        """the keyframe sets the last builder call wrote (None: it was the plain sliding builder, which writes none)"""
        return self.ba_kf_frame.data_ptr() if self._builder_writes_kf else None

    def step(self):
        if self.rectify is not None:
            self.stage_rectify()
        self.stage_orb()
        self.stage_stereo_match()
        self.stage_track()
        self.stage_ba()

    # ------------------------------------------------------------------ host views (tests / reports)
    def download(self):
        self.vo.sync()
        torch.cuda.synchronize(self.dev)
        B, cap = self.B, self.cap
        out = dict(cnt=self.d_cnt.cpu().numpy(), nlr=self.d_nlr.cpu().numpy(), nf2f=self.d_nf2f.cpu().numpy(), pn=self.d_pn.cpu().numpy(),
                   ninl=self.d_ninl.cpu().numpy(), Tpnp=self.d_Tpnp.cpu().numpy())
        out["kps"] = self.d_kps.cpu().numpy().reshape(2 * B, -1).view(KEYPOINT_DTYPE).reshape(2 * B, cap)
        out["desc"] = self.d_desc.cpu().numpy()
        out["lr"] = self.d_lr.cpu().numpy().reshape(B, -1).view(DMATCH_DTYPE).reshape(B, cap)
        out["f2f"] = self.d_f2f.cpu().numpy().reshape(B, -1).view(DMATCH_DTYPE).reshape(B, cap)
        out["xyz"] = self.d_xyz.cpu().numpy(); out["valid"] = self.d_valid.cpu().numpy(); out["rel"] = self.d_rel.cpu().numpy()
        out["pxyz"] = self.d_pxyz.cpu().numpy(); out["puv"] = self.d_puv.cpu().numpy(); out["inl"] = self.d_inl.cpu().numpy()
        if self.with_ba:
            out["ba_T"] = self.ba_T.cpu().numpy(); out["ba_inl"] = self.ba_inl.cpu().numpy(); out["ba_chi2"] = self.ba_chi2.cpu().numpy()
        if self.with_ba and self.ba_windows == "tracks":
            for k, t in (("ba_lm_off", self.ba_lm_off), ("ba_e_off", self.ba_e_off), ("ba_nkf", self.ba_nkf), ("ba_xyz", self.ba_xyz), ("ba_rel", self.ba_rel),
                         ("ba_kf", self.ba_kf), ("ba_lm", self.ba_lm), ("ba_uv", self.ba_uv), ("ba_build_status", self.ba_build_status)):
                out[k] = t.cpu().numpy()
            out["ba_kf_frame"], out["ba_evicted"] = self._keyframe_sets()
            if self.seg_first is not None:
                out["seg_first"] = self.seg_first.copy()
            if self.landmark_ids:
                out["ba_lm_id"] = self.ba_lm_id.cpu().numpy()
            if self.ba_chain:
                out["ba_ran"] = self.ba_ran.cpu().numpy()
            if self.keyframe_gate:   # (per_pass: the last pass's states; frame_state_prev: the states that pass started from)
                out["frame_state"] = self.ba_frame_state.cpu().numpy()
                if self.keyframe_gate == "per_pass":
                    out["frame_state_prev"] = self.map_state_prev.cpu().numpy()
        if self.pose_inputs == "map":   # the last refinement pass (item i: frame i + 1); T_c_w = its poses G^K
            c = self.map_cur
            if self.f2f_queries == "features" and self.map_table is not None:   # the table that pass solved on and the feature lists it was matched from
                t = self.map_table
                out["map_f2f"] = self.map_f2f[t].cpu().numpy().reshape(B, -1).view(DMATCH_DTYPE).reshape(B, cap)
                out["map_nf2f"] = self.map_nf2f[t].cpu().numpy()
                out["map_feat"] = self.map_feat.cpu().numpy(); out["map_nfeat"] = self.map_nfeat.cpu().numpy()
                if self.rejected_frames == "recover":   # the pairing that table was built on (frame f against map_pred[f], -1: none) and its gaps
                    out["map_pred"] = self.map_pred[t].cpu().numpy(); out["map_gap"] = self.map_gap.cpu().numpy()
            out["map_n"] = self.map_n.cpu().numpy(); out["map_xyz"] = self.map_xyz.cpu().numpy(); out["map_uv"] = self.map_uv.cpu().numpy()
            out["map_index"] = self.map_index[c].cpu().numpy(); out["map_inl"] = self.map_inl[c].cpu().numpy(); out["map_ninl"] = self.map_ninl.cpu().numpy()
            out["T_c_w"] = self.map_G[c].cpu().numpy()
        return out

    def _keyframe_sets(self):
        """(kf_frame, evicted) of the built windows on the host.  Deliberate: pose_inputs="map" with a sliding, ungated window reports the host-side
        sliding sets, although its builder wrote the device arrays too"""
        if self.window_policy == "reference" or self.keyframe_gate:
            return self.ba_kf_frame.cpu().numpy(), self.ba_evicted.cpu().numpy()
        return self._sliding_keyframes()

    def _sliding_keyframes(self):
        """the sliding windows' sets on the host, per segment when the batch is segmented (batch frame indices)"""
        if self.seg_first is None:
            return sliding_keyframes(self.B, self.n_kf)
        parts = [sliding_keyframes(int(hi - lo), self.n_kf) for lo, hi in zip(self.seg_first[:-1], self.seg_first[1:])]
        kf = np.concatenate([np.where(k >= 0, k + lo, -1) for (k, _), lo in zip(parts, self.seg_first)]).astype(np.int32)
        ev = np.concatenate([np.where(e >= 0, e + lo, -1) for (_, e), lo in zip(parts, self.seg_first)]).astype(np.int32)
        return kf, ev

    def _trajectory_inputs(self):
        assert self.with_ba and self.ba_windows == "tracks"
        self.vo.sync()
        torch.cuda.synchronize(self.dev)
        kf_frame, evicted = self._keyframe_sets()
        valid = (self.ba_frame_state.cpu().numpy() == 2) if self.keyframe_gate else None
        return kf_frame, evicted, self.ba_T.cpu().numpy(), valid

    def trajectories(self):
        """a segmented pipeline's trajectories: one (frame_ids, T_c_w) per segment as trajectory() gives it for that segment's pipeline alone, the ids
        local to the segment.  An unsegmented pipeline has one segment."""
        kf_frame, evicted, ba_T, valid = self._trajectory_inputs()
        first = self.seg_first if self.seg_first is not None else np.array([0, self.B])
        return assemble_trajectories(kf_frame, evicted, ba_T, first, window_valid=valid)

    def trajectory(self):
        """(frame_ids, T_c_w): every frame's pose from the BA windows (ba_windows="tracks"), in the order the reference writes them -- a frame when it
        is evicted (from the last window that held it), the last window's frames at the end.  write_trajectory(path, *pipe.trajectory()) writes the
        file KITTI evaluation reads.  With keyframe_gate, only keyframes are written, each from the last keyframe window that held it.
        A segmented pipeline holds several trajectories: trajectories()."""
        assert self.seg_first is None, "a segmented pipeline has one trajectory per segment: use trajectories()"
        kf_frame, evicted, ba_T, valid = self._trajectory_inputs()
        return assemble_trajectory(kf_frame, evicted, ba_T, window_valid=valid)

    def dense_map_inputs(self, poses=None):
        """what dense_map() fuses: (T_c_w (B, 7) float64, map_id (B,) int32) -- every frame of trajectories() at its BA-refined pose with its segment's
        index (0 without a segment table) as map id; a frame outside the trajectories has map id -1 and the identity pose.  poses: one
        (frame_ids, T_c_w) per segment to use instead of trajectories(), e.g. what close_loops() returned"""
        trajs = self.trajectories() if poses is None else poses
        assert len(trajs) == (len(self.seg_first) - 1 if self.seg_first is not None else 1), "poses: one (frame_ids, T_c_w) per segment"
        assert len(trajs) <= 1023, "a voxel map holds at most 1023 maps (segments)"
        first = self.seg_first if self.seg_first is not None else np.array([0, self.B])
        T = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (self.B, 1))
        map_id = np.full(self.B, -1, np.int32)
        for s_, (ids, Ts) in enumerate(trajs):
            T[first[s_] + ids] = Ts
            map_id[first[s_] + ids] = s_
        return T, map_id

    def _map_inputs(self, poses, z_min=None, z_max=None, fuse=None, **given):
        """The front dense_map, surface_map, surface_views and surface_remap share -- which frames meet a map, at which poses, under which map ids,
        between which depth gates: (T_c_w (B, 7), map_id (B,), z_min, z_max) of dense_map_inputs(poses), a gate left None standing for the
        context's depth_min / depth_reliable.  given: the caller's voxel_map= or tsdf_map= argument, which, unless None, must be of this pipeline's
        context.  fuse: the name of a caller that fuses the step's SGBM maps; it needs depth="sgbm" and the BA windows' poses, and finds T and map_id
        on the device as self.dense_T / self.dense_map_id, uploaded on the pipeline's stream."""
        if fuse is not None:
            assert self.depth == "sgbm", "%s needs depth='sgbm': it fuses the SGBM disparity maps" % fuse
            assert self.with_ba and self.ba_windows == "tracks", "%s needs ba_windows='tracks': the poses are the BA windows'" % fuse
        for name, m in given.items():
            assert m is None or m.vo is self.vo, "%s belongs to another context" % name
        if poses is not None:
            self.vo.sync()
            torch.cuda.synchronize(self.dev)
        T, map_id = self.dense_map_inputs() if poses is None else self.dense_map_inputs(poses)   # (synchronises: the step is complete)
        p = self.vo.params
        z_min = p.depth_min if z_min is None else float(z_min)
        z_max = p.depth_reliable if z_max is None else float(z_max)
        if fuse is not None:
            with torch.cuda.stream(self.stream):
                self.dense_T = torch.from_numpy(T).to(self.dev)
                self.dense_map_id = torch.from_numpy(map_id).to(self.dev)
        return T, map_id, z_min, z_max

    def dense_map(self, voxel_size=0.2, log2_capacity=22, z_min=None, z_max=None, step=1, voxel_map=None, poses=None):
        """The dense map of the last step (depth="sgbm", ba_windows="tracks"): the SGBM disparity and the left image of every frame trajectories()
        returns, reprojected at that frame's BA-refined pose and fused into a VoxelMap (vslam_voxel_fuse_disparity_dev) -- map id = the segment index.
        z_min / z_max default to the context's depth_min / depth_reliable (the reference trusts stereo depth below 40 m only); every step-th pixel.
        voxel_map: a VoxelMap of this pipeline's context to accumulate into over several steps (voxel_size / log2_capacity then go unused); otherwise
        a new one.  poses: the corrected trajectories close_loops() returned, in place of the BA poses (None: the BA poses).
        Returns the map: .extract() / .stats() read it, write_ply(path, vm.extract()) writes it."""
        T, map_id, z_min, z_max = self._map_inputs(poses, z_min, z_max, fuse="dense_map", voxel_map=voxel_map)
        vm = voxel_map if voxel_map is not None else self.vo.voxel_map(voxel_size, log2_capacity)
        self.vo.voxel_fuse_disparity_dev(vm, self.d_disp.data_ptr(), self.d_imgs.data_ptr(), self.img_bytes, self.pitch, self.w, self.h, self.B,
                                         self.dense_T.data_ptr(), self.dense_map_id.data_ptr(), z_min, z_max, int(step))
        return vm

    def surface_map(self, voxel_size=0.2, trunc_voxels=4, log2_blocks=16, z_min=None, z_max=None, step=1, tsdf_map=None, poses=None):
        """The surface map of the last step (depth="sgbm", ba_windows="tracks"): what dense_map() fuses -- the SGBM disparity and the left image of every
        frame of dense_map_inputs(poses), same default gates depth_min .. depth_reliable -- integrated into a TsdfMap (vslam_tsdf_integrate_dev), map
        id = the segment index.  step thins the allocation only.  tsdf_map: a TsdfMap of this pipeline's context to accumulate into over several
        steps (a step's frames also carve the blocks earlier steps claimed; voxel_size / trunc_voxels / log2_blocks then go unused); otherwise a new
        one.  poses: what close_loops() or full_ba() returned, in place of the BA poses.
        Returns the map: .extract() reads the surfels, write_surfel_ply(path, tm.extract()) writes them; .mesh() connects them into triangles,
        write_mesh_ply(path, *tm.mesh()) writes the mesh.  self.surface_frames remembers what was integrated (poses, map ids, gates, the call's
        reach) for surface_remap()."""
        T, map_id, z_min, z_max = self._map_inputs(poses, z_min, z_max, fuse="surface_map", tsdf_map=tsdf_map)
        tm = tsdf_map if tsdf_map is not None else self.vo.tsdf_map(voxel_size, trunc_voxels, log2_blocks)
        tm.integrate_dev(self.d_disp.data_ptr(), self.d_imgs.data_ptr(), self.img_bytes, self.pitch, self.w, self.h, self.B,
                         self.dense_T.data_ptr(), self.dense_map_id.data_ptr(), z_min, z_max, int(step))
        self.last_surface_map = tm
        # what surface_remap() needs to take these frames out again: the poses and map ids they went in with, the gates, and the call's reach (the
        # block count after its allocation, read on the device: a 4-byte copy on the context stream -- the pipeline's own --, no kernel, no host round trip)
        with torch.cuda.stream(self.stream):
            reach = torch.zeros(1, dtype=torch.int32, device=self.dev)
        tm.reach_dev(reach.data_ptr())
        self.surface_frames = dict(tsdf_map=tm, T=T.copy(), map_id=map_id.copy(), z_min=z_min, z_max=z_max, step=int(step), reach=reach.expand(self.B))
        return tm

    def surface_remap(self, poses, tsdf_map=None, min_shift=0.0, min_turn=0.0):
        """The last step's frames taken out of the surface map at the poses surface_map() (or the last surface_remap()) put them in with and
        re-integrated at `poses` -- what close_loops() or full_ba() returned -- in one pass over the map (vslam_tsdf_reintegrate_dev), from the step's
        disparities and images still on the device.  Only frames whose camera centre moved more than min_shift metres or whose rotation changed by more
        than min_turn radians are re-integrated; the others stay as they are (map id -1 in the call).  A frame that left the trajectories is removed,
        one that entered them is added.  tsdf_map: the map surface_map() filled (None: that one).  The remembered poses and reach are updated, so
        a later surface_remap() starts from this one.  Returns (the map, the number of frames moved).
        Limits: the frames of the LAST surface_map() call only (the pipeline keeps one step's disparities); blocks that empty stay claimed."""
        st = getattr(self, "surface_frames", None)
        assert st is not None, "surface_remap needs a surface_map() call before it: it re-integrates that call's frames"
        tm = tsdf_map if tsdf_map is not None else st["tsdf_map"]
        assert tm is st["tsdf_map"] and getattr(tm, "h", None), "surface_remap: tsdf_map is not the (open) map the last surface_map() filled"
        T_new, id_new, _, _ = self._map_inputs(poses, tsdf_map=tm)
        T_old, id_old = st["T"], st["map_id"]
        was, now = id_old >= 0, id_new >= 0
        assert (id_old[was & now] == id_new[was & now]).all(), "surface_remap: a frame changed its segment"
        R = lambda T: np.stack([np.asarray(synth.R_from_quat(q)) for q in T[:, :4]])
        Ro, Rn = R(T_old), R(T_new)
        centre = lambda Rm, T: -np.einsum("bji,bj->bi", Rm, T[:, 4:])
        shift = np.linalg.norm(centre(Rn, T_new) - centre(Ro, T_old), axis=1)
        turn = np.arccos(np.clip((np.einsum("bij,bij->b", Ro, Rn) - 1.0) / 2.0, -1.0, 1.0))
        moved = (was != now) | (was & now & ((shift > float(min_shift)) | (turn > float(min_turn))))
        n_moved = int(moved.sum())
        if n_moved == 0:
            return tm, 0
        nan = np.full(7, np.nan)
        call_old = np.where((moved & was)[:, None], T_old, nan)
        call_new = np.where((moved & now)[:, None], T_new, nan)
        call_id = np.where(moved, np.where(now, id_new, id_old), -1).astype(np.int32)
        with torch.cuda.stream(self.stream):
            d_old, d_new = torch.from_numpy(call_old).to(self.dev), torch.from_numpy(call_new).to(self.dev)
            d_id, d_moved = torch.from_numpy(call_id).to(self.dev), torch.from_numpy(moved).to(self.dev)
            d_reach = st["reach"].contiguous()
            after = torch.zeros(1, dtype=torch.int32, device=self.dev)
        tm.reintegrate_dev(self.d_disp.data_ptr(), self.d_imgs.data_ptr(), self.img_bytes, self.pitch, self.w, self.h, self.B, d_old.data_ptr(), d_new.data_ptr(),
                           d_id.data_ptr(), d_reach.data_ptr(), st["z_min"], st["z_max"], st["step"])
        tm.reach_dev(after.data_ptr())
        with torch.cuda.stream(self.stream):
            st["reach"] = torch.where(d_moved, after.expand(self.B), d_reach)
        st["T"] = np.where(moved[:, None], np.where(now[:, None], T_new, T_old), T_old)
        st["map_id"] = np.where(moved, id_new, id_old).astype(np.int32)
        self.surface_remap_buffers = (d_old, d_new, d_id, d_reach)   # (alive until the stream has run the call)
        return tm, n_moved

    def surface_views(self, tsdf_map=None, poses=None, scale=1.0, march=0.5, min_weight=1, disparity=False):
        """What the surface map shows from every frame of dense_map_inputs(poses), each at its own pose and map id (TsdfMap.render): the carved,
        multi-view counterpart of the frames' single-view SGBM maps, or -- with poses= what close_loops() or full_ba() returned -- the map seen from
        where the corrected trajectory puts the cameras.  tsdf_map: a TsdfMap of this pipeline's context (None: the one the last surface_map()
        returned).  The context's camera and image size are multiplied by `scale`; the depth range is depth_min .. depth_reliable.
        Returns TsdfMap.render's dict (depth (B, h, w), normal, intensity, counts) with T_c_w and map_id added and, with disparity=True,
        disparity = fx * b / depth at the scaled fx (0 where the ray misses)."""
        tm = tsdf_map if tsdf_map is not None else getattr(self, "last_surface_map", None)
        assert tm is not None and getattr(tm, "h", None), "surface_views needs a TsdfMap: call surface_map() first or pass tsdf_map="
        assert scale > 0
        T, map_id, _, _ = self._map_inputs(poses, tsdf_map=tm)
        fx, fy, cx, cy, b = (float(v) for v in self.vo.params.cam)
        K4 = (fx * scale, fy * scale, cx * scale, cy * scale)
        size = (max(int(round(self.w * scale)), 1), max(int(round(self.h * scale)), 1))
        out = tm.render(T, map_id, K4=K4, size=size, march=march, min_weight=min_weight)
        out.update(T_c_w=T, map_id=map_id, K4=K4)
        if disparity:
            depth = out["depth"].astype(np.float64)
            with np.errstate(divide="ignore"):
                out["disparity"] = np.where(depth > 0, K4[0] * b / depth, 0.0).astype(np.float32)
        return out

    def surface_clearance(self, radius_m, tsdf_map=None, min_weight=1):
        """The clearance layer of the surface map (TsdfMap.distance, include/vslam_hip.h "DISTANCE") out to radius_m metres: per voxel the squared
        distance in voxels to the nearest surface voxel of its map and the voxel's class.  The radius in voxels is ceil(radius_m / voxel size) and
        must not exceed 16.  tsdf_map: a TsdfMap of this pipeline's context (None: the one the last surface_map() returned).  Returns
        TsdfMap.distance's dict (ids, cells, counts) with radius (voxels) and voxel_size added; tm.distance_query(points, map_id) then answers
        points until the map changes, and dense.clearance_slice(ids, cells, ...) flattens a height band into a costmap."""
        tm = tsdf_map if tsdf_map is not None else getattr(self, "last_surface_map", None)
        assert tm is not None and getattr(tm, "h", None), "surface_clearance needs a TsdfMap: call surface_map() first or pass tsdf_map="
        vs = float(np.float32(tm.voxel_size))
        radius = int(np.ceil(float(radius_m) / vs))
        assert 1 <= radius <= 16, "surface_clearance: radius_m %g is %d voxels of %g m, outside [1, 16]" % (radius_m, radius, vs)
        out = tm.distance(map_id=-1, min_weight=min_weight, radius=radius)
        out.update(radius=radius, voxel_size=vs)
        return out

    # ------------------------------------------------------------------ loop closure (nothing here runs unless loop_closures is called)
    def show_sequence(self, sequence):
        """lay another rendered sequence of the same length over the batch (an unsegmented pipeline without a rig): the next step() sees its frames.
        This is how one pipeline is driven over the successive chunks of a longer drive."""
        assert self.seg_first is None and self.rectify is None, "show_sequence: an unsegmented pipeline without rectify"
        assert len(sequence) == len(self.h_seq), (len(sequence), len(self.h_seq))
        B = self.B
        imgs = np.zeros((2 * B, self.h, self.pitch), np.uint8)
        for b in range(B):
            L, R, _, _ = sequence[self.frame_of[b]]
            imgs[b, :, :self.w] = L; imgs[B + b, :, :self.w] = R
        self.h_seq, self.h_imgs = sequence, imgs
        self.vo.sync()
        with torch.cuda.stream(self.stream):
            self.d_imgs.copy_(torch.from_numpy(imgs).to(self.dev))
        self.stream.synchronize()

    def _points_per_keypoint(self):
        """(xyz (B, cap, 3) f32, valid (B, cap) uint8) laid out per LEFT KEYPOINT: depth="sgbm" has them so; depth="match" holds them per L/R match and
        they are scattered through the L/R table (queryIdx = the left keypoint)"""
        if self.depth == "sgbm":
            return self.d_xyz, self.d_valid
        B, cap = self.B, self.cap
        with torch.cuda.stream(self.stream):
            kp = self.d_lr.view(torch.int32).reshape(B, cap, 4)[:, :, 0].long().clamp(0, cap - 1)
            live = torch.arange(cap, device=self.dev)[None, :] < self.d_nlr[:, None]
            # a dead slot is sent to a spare column that is cut off again
            tgt = torch.where(live, kp, torch.full_like(kp, cap))
            xyz = torch.zeros((B, cap + 1, 3), dtype=torch.float32, device=self.dev).scatter_(1, tgt[:, :, None].expand(B, cap, 3), self.d_xyz)
            valid = torch.zeros((B, cap + 1), dtype=torch.uint8, device=self.dev).scatter_(1, tgt, self.d_valid)
            xyz, valid = xyz[:, :cap].contiguous(), valid[:, :cap].contiguous()
        return xyz, valid

    def loop_closures(self, place_db=None, rows=None, tau=None, min_gap=None, K=3, min_score=None, min_inliers=10, frame_offset=0, seq_ids=None):
        """Loop-closure edges of the last step (include/vslam_hip.h "place database").  The step's frames -- all of them, or with keyframe_gate the
        keyframes (the frames trajectories() returns) -- are appended to `place_db` with seq = the segment index (seq_ids: a sequence id per segment
        instead) and frame = the batch-wide frame index + frame_offset (an int: what earlier steps of the same drive have consumed).  Each new entry
        is scored against every entry of its sequence at least min_gap frames older, the K best that reach min_score are verified with the matcher
        and the RANSAC pose stage, and one row per (query, candidate) comes back: a LOOP_EDGE_DTYPE array (entry_q, entry_c, seq, frame_q, frame_c,
        score, n_matches, n_inliers, accepted = n_inliers >= min_inliers, T_q_c = the pose of candidate c's camera frame in query q's: p_q = T_q_c p_c).
        place_db: a PlaceDB of this pipeline's context (vo.place_db(...)) kept by the caller -- handing the same one to every step finds loops into
        earlier batches, which is the point of it; None: a database of this pipeline's own, emptied first, so only loops inside the step are found.
        rows: descriptor rows kept per entry of a new database (None: anms_num).  tau: None = (int)match_gap_thr = 30, the distance the reference's
        matcher gate trusts at frame gap 1.  min_gap and min_score have no derivable default and must be given: on the project's renderer at 500
        keypoints and tau 30, a revisit within half a metre and 0.03 rad scored 83..148, the best other frame at most 54, a foreign scene at most 2
        (DESIGN.md 5.9); min_gap should exceed the frames over which consecutive views still overlap."""
        assert min_gap is not None and min_score is not None, "loop_closures: min_gap and min_score must be given (no derivable default; see the docstring)"
        assert 1 <= int(K) <= 8 and int(min_inliers) >= 0
        vo, B, cap = self.vo, self.B, self.cap
        tau = int(vo.params.match_gap_thr) if tau is None else int(tau)
        if place_db is None:
            if getattr(self, "_own_place_db", None) is None:
                self._own_place_db = vo.place_db(rows=rows, capacity=max(B, 1), with_geometry=True)
            place_db = self._own_place_db
            place_db.clear()
        assert place_db.vo is vo and place_db.with_geometry, "place_db: a PlaceDB with geometry of this pipeline's context"
        vo.sync()
        torch.cuda.synchronize(self.dev)
        first_of = self.seg_first if self.seg_first is not None else np.array([0, B])
        seg_of = np.repeat(np.arange(len(first_of) - 1), np.diff(first_of))
        seq = seg_of if seq_ids is None else np.asarray(seq_ids, np.int64)[seg_of]
        frame = np.arange(B) + int(frame_offset)
        xyz, valid = self._points_per_keypoint()
        with torch.cuda.stream(self.stream):
            d_seq = torch.from_numpy(seq.astype(np.int32)).to(self.dev); d_frame = torch.from_numpy(frame.astype(np.int32)).to(self.dev)
            d_add = (self.ba_frame_state == 2).to(torch.int32) if self.keyframe_gate else None
        self.stream.synchronize()
        q0 = vo.place_add_dev(place_db, self.d_desc.data_ptr(), cap * 32, self.d_cnt.data_ptr(), None if d_add is None else d_add.data_ptr(), d_seq.data_ptr(),
                              d_frame.data_ptr(), self.d_kps.data_ptr(), xyz.data_ptr(), valid.data_ptr(), cap, B)
        n_total = len(place_db)
        _, e_seq, e_frame = place_db.meta()
        rows_out = []
        chunk = int(vo.params.max_batch)
        for c0 in range(q0, n_total, chunk):
            nq = min(chunk, n_total - c0)
            d_score = place_db.score(c0, nq, tau, int(min_gap))
            d_cand, d_cs = place_db.select(c0, d_score, int(K), int(min_score))
            ver = [place_db.verify(c0, d_cand, r, int(min_inliers)) for r in range(int(K))]
            vo.sync()
            cand, cs = d_cand.cpu().numpy(), d_cs.cpu().numpy()
            for r, (dT, dnm, dni) in enumerate(ver):
                T, nm, ni = dT.cpu().numpy(), dnm.cpu().numpy(), dni.cpu().numpy()
                for b in np.flatnonzero(cand[:, r] >= 0):
                    e, c = c0 + int(b), int(cand[b, r])
                    rows_out.append((e, r, (e, c, e_seq[e], e_frame[e], e_frame[c], cs[b, r], nm[b], ni[b], bool(ni[b] >= min_inliers), T[b])))
        rows_out.sort(key=lambda t: (t[0], t[1]))
        out = np.zeros(len(rows_out), LOOP_EDGE_DTYPE)
        for i, (_, _, row) in enumerate(rows_out):
            out[i] = row
        return out

    def close_loops(self, edges, frame_offset=0, w_odo=(1.0, 1.0), w_loop=(1.0, 1.0), reject_chi2=None, params=None, motion_limit=5.0):
        """The last step's trajectories corrected by loop-closure edges (include/vslam_hip.h "pose-graph optimisation"): a PoseGraph with one graph
        per segment -- nodes = the frames trajectories() returns, odometry edges between consecutive ones from the BA poses, one loop edge per
        accepted row of `edges` (what loop_closures() returned, with the same frame_offset) -- optimised in one call, all segments side by side.
        A row belongs to the segment its frames lie in (its `seq` is not consulted: loop_closures may have given several segments one sequence id);
        rows that are not accepted, or whose frames are not both nodes of one segment -- frames of another step, of two segments, or ones the keyframe
        gate dropped -- are counted in .pose_graph.report, not dropped silently, and so are the odometry edges that exceed the motion limit
        (PoseGraph: a pose tracked across a cut in the recording is not a measurement).  w_odo, w_loop, motion_limit, reject_chi2, params: PoseGraph and
        PoseGraph.optimize (no measured default for the weights exists).  Returns what trajectories() returns, corrected; dense_map(poses=...) takes
        it.  The BA landmarks are not moved (full_ba() does that), and the frames of other steps are out of reach: each step starts a world of its own."""
        from .posegraph import PoseGraph
        first = np.asarray(self.seg_first if self.seg_first is not None else [0, self.B], np.int64)
        pg = PoseGraph(w_odo=w_odo, w_loop=w_loop, motion_limit=motion_limit)
        for s_, (ids, Ts) in enumerate(self.trajectories()):
            pg.add_trajectory(s_, np.asarray(ids, np.int64) + int(first[s_]) + int(frame_offset), Ts)
        rows = np.array(edges, copy=True)
        seg = np.searchsorted(first, rows["frame_q"].astype(np.int64) - int(frame_offset), side="right") - 1
        rows["seq"] = np.where((seg >= 0) & (seg < len(first) - 1), seg, -1)
        pg.add_loop_edges(rows)
        self.pose_graph = pg
        out = pg.optimize(self.vo, reject_chi2=reject_chi2, params=params)
        return [(ids - int(first[s_]) - int(frame_offset), Ts) for s_, (ids, Ts) in enumerate(out)]

    def window_landmark_ids(self):
        """the identities (creating frame x kp_capacity + creating keypoint) of the landmarks of the built windows, window after window (landmark_ids=True)"""
        assert self.landmark_ids, "window_landmark_ids needs landmark_ids=True (or ba_chain=True)"
        self.vo.sync()
        torch.cuda.synchronize(self.dev)
        return self.ba_lm_id.cpu().numpy()[:int(self.ba_lm_off.cpu().numpy()[-1])]

    def _window_observations(self):
        """the built windows on the host: (kf_frame, e_frame, e_id, ba_uv, lm_id, lm_xyz, win_of_e, win_of_lm) -- every observation as (batch frame,
        landmark id, uv) and every landmark as (id, world position), duplicates included, in window order"""
        kf_frame, _ = self._keyframe_sets()
        lm_off, e_off = self.ba_lm_off.cpu().numpy().astype(np.int64), self.ba_e_off.cpu().numpy().astype(np.int64)
        n_lm, n_e = int(lm_off[-1]), int(e_off[-1])
        ba_kf, ba_lm, ba_uv = self.ba_kf.cpu().numpy()[:n_e], self.ba_lm.cpu().numpy()[:n_e], self.ba_uv.cpu().numpy()[:n_e]
        lm_id, lm_xyz = self.ba_lm_id.cpu().numpy()[:n_lm].astype(np.int64), self.ba_xyz.cpu().numpy()[:n_lm].astype(np.float64)
        win_of_e = np.repeat(np.arange(self.B), np.diff(e_off)); win_of_lm = np.repeat(np.arange(self.B), np.diff(lm_off))
        e_frame = kf_frame[win_of_e, ba_kf].astype(np.int64)
        e_id = lm_id[lm_off[win_of_e] + ba_lm]
        return kf_frame, e_frame, e_id, ba_uv, lm_id, lm_xyz, win_of_e, win_of_lm

    def project_matcher(self, radius=15.0, tau=50, ratio_pct=80, z_min=0.1, z_max=1e4):
        """the callable reobserve() hands its batch to: one vslam_project_match_dev call on the step's resident left keypoints and descriptors (the
        landmarks' descriptor rows index the same array).  .project_match_batch keeps the last batch, .project_match_result its result, .project_match_ms the call's wall time."""
        import time
        from . import ProjectMatchBatch, default_project_match_params, PROJECT_MATCH_MAX_KP
        assert self.cap <= PROJECT_MATCH_MAX_KP, "kp_capacity %d exceeds vslam_project_match_dev's limit %d" % (self.cap, PROJECT_MATCH_MAX_KP)
        params = default_project_match_params(radius_px=float(radius), tau=int(tau), ratio_pct=int(ratio_pct), z_min=float(z_min), z_max=float(z_max))

        def matcher(b):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
            t = dict(off=up(b["lm_off"]), img=up(b["item_img"]), T=up(b["item_T"]), xyz=up(b["lm_xyz"]), row=up(b["lm_desc_row"]))
            batch = ProjectMatchBatch(n_items=len(b["item_img"]), n_landmarks=len(b["lm_desc_row"]), B=self.B, kp_capacity=self.cap, n_src_rows=self.B * self.cap,
                                      d_lm_off=t["off"].data_ptr(), d_item_img=t["img"].data_ptr(), d_item_T=t["T"].data_ptr(), d_lm_xyz=t["xyz"].data_ptr(),
                                      d_lm_desc_row=t["row"].data_ptr(), d_src_desc=self.d_desc.data_ptr(), d_kps=self.d_kps.data_ptr(), d_desc=self.d_desc.data_ptr(),
                                      desc_stride_bytes=self.cap * 32, d_n=self.d_cnt.data_ptr())
            torch.cuda.synchronize(self.dev)
            t0 = time.perf_counter()
            out = self.vo.project_match_dev(batch, params)
            self.vo.sync()
            self.project_match_ms = (time.perf_counter() - t0) * 1e3
            self.project_match_batch = b
            self.project_match_result = {k: v.cpu().numpy() for k, v in out.items()}
            return self.project_match_result
        return matcher

    def reobserve(self, edges=None, neighbours=10, loop_neighbours=2, radius=15.0, tau=50, ratio_pct=80, frame_offset=0, matcher=None):
        """Match by projection over the last step (include/vslam_hip.h "match by projection"; reobserve.py says how the items are formed and how the
        matches are applied): the landmarks of the neighbouring keyframes -- and, for the accepted rows of `edges` (what loop_closures() returned, with
        the same frame_offset), of the other end of the loop -- are projected into each keyframe at its estimated pose and looked for among its
        keypoints, all items in one device call.  Returns dict(observations (REOBS_DTYPE rows: frame, lm_id, kp, u, v, dist, kind local | loop),
        merge = (ids, canonical), report); full_ba(reobserved=...) takes it.  matcher: a callable in place of the device call (the yardstick in
        tests).  The depth gate is the context's depth_min .. depth_max, the one stereo points are created under, and merges pass reobserve.py's
        merge gate at the search radius.  Needs landmark_ids=True (or
        ba_chain=True).  Nothing is fed back into the BA windows or into tracking."""
        if not getattr(self, "landmark_ids", False):
            raise ValueError("reobserve needs the landmarks' identities: build the pipeline with landmark_ids=True (or ba_chain=True)")
        from .reobserve import reobserve
        trajs = self.trajectories()   # (synchronises: the step is complete)
        first = np.asarray(self.seg_first if self.seg_first is not None else [0, self.B], np.int64)
        _, e_frame, e_id, ba_uv, lm_id, lm_xyz, win_of_e, win_of_lm = self._window_observations()
        segs = []
        for s_, (ids, Ts) in enumerate(trajs):
            we = (win_of_e >= first[s_]) & (win_of_e < first[s_ + 1]); wl = (win_of_lm >= first[s_]) & (win_of_lm < first[s_ + 1])
            segs.append((first[s_], ids, Ts, e_frame[we], e_id[we], ba_uv[we], lm_id[wl], lm_xyz[wl]))
        kps = self.d_kps[:self.B].cpu().numpy().view(np.float32).reshape(self.B, self.cap, 7)[:, :, :2].copy()
        n = self.d_cnt.cpu().numpy()[:self.B]
        if matcher is None:
            # the depth gate is the one that creates landmarks: where no stereo point may be made, none is re-observed either (a landmark passing
            # beside the camera projects anywhere)
            matcher = self.project_matcher(radius=radius, tau=tau, ratio_pct=ratio_pct, z_min=self.vo.params.depth_min, z_max=self.vo.params.depth_max)
        cam = list(self.vo.params.cam)
        out = reobserve(segs, edges, self.cap, matcher, kps, n, neighbours=neighbours, loop_neighbours=loop_neighbours, frame_offset=frame_offset,
                        merge_gate=dict(K4=cam[:4], bf=cam[0] * cam[4], radius=radius))
        self.reobserve_result = out
        return out

    def full_ba(self, edges=None, poses=None, w_loop=(1.0, 1.0), huber_delta=None, params=None, frame_offset=0, reobserved=None):
        """Full bundle adjustment of the last step (include/vslam_hip.h "full bundle adjustment"): per segment all keyframes of trajectories() and all
        landmarks of the BA windows over all their observations, the accepted rows of `edges` (what loop_closures() returned, with the same
        frame_offset) as pose-pose factors of information w_loop, all segments in one call.  poses: the initial poses in place of trajectories(),
        e.g. what close_loops() returned -- the landmarks are then first carried along by their creating keyframe's correction.  huber_delta: None =
        the context's (the width the library's other BA passes use), 0 = no robust kernel.  params: a FullBAParams.  FullBA (fullba.py) says how the
        problem is formed and what is left out; that is counted in .full_ba_result["report"].  Returns what trajectories() returns, refined;
        dense_map(poses=...) takes it.  .full_ba_result keeps report and, per segment, dict(lm_id, xyz (every landmark of the windows at its new
        position, float64: vo.voxel_insert_points_dev takes them as float32), in_problem, problem, xyz_problem, stats, obs_chi2).
        reobserved: what reobserve() returned -- its observations are appended to the windows' and its merged landmark classes become one landmark
        each (FullBA.add_segment's merge); the report then counts observations_reobserved, landmarks_merged and observations_merged_duplicate.
        Needs landmark_ids=True (or ba_chain=True).  The result is not fed back into tracking, and frames of other steps are out of reach."""
        if not getattr(self, "landmark_ids", False):
            raise ValueError("full_ba needs the landmarks' identities: build the pipeline with landmark_ids=True (or ba_chain=True)")
        from .fullba import FullBA
        trajs = self.trajectories()   # (synchronises: the step is complete)
        if poses is not None:
            assert len(poses) == len(trajs), "poses: one (frame_ids, T_c_w) per segment"
        first = np.asarray(self.seg_first if self.seg_first is not None else [0, self.B], np.int64)
        cam = list(self.vo.params.cam)
        fb = FullBA(cam[:4], cam[0] * cam[4], self.cap, w_loop=w_loop, huber_delta=self.vo.params.huber_delta if huber_delta is None else huber_delta)
        _, e_frame, e_id, ba_uv, lm_id, lm_xyz, win_of_e, win_of_lm = self._window_observations()
        kp_xyz, kp_valid = self._points_per_keypoint()
        self.stream.synchronize()
        kp_xyz, kp_valid = kp_xyz.cpu().numpy(), kp_valid.cpu().numpy()
        for s_, (ids, Ts) in enumerate(trajs):
            T_new = None
            if poses is not None:
                ids_p, T_p = poses[s_]
                assert np.array_equal(np.asarray(ids_p), np.asarray(ids)), "poses: the frame ids of trajectories(), segment %d" % s_
                T_new = T_p
            we = (win_of_e >= first[s_]) & (win_of_e < first[s_ + 1]); wl = (win_of_lm >= first[s_]) & (win_of_lm < first[s_ + 1])
            if reobserved is None:
                fb.add_segment(first[s_], ids, Ts, e_frame[we], e_id[we], ba_uv[we], lm_id[wl], lm_xyz[wl], kp_xyz, kp_valid, T_new=T_new)
                continue
            ro = reobserved["observations"]
            mine = (ro["frame"] >= first[s_]) & (ro["frame"] < first[s_ + 1])
            fb.report["observations_reobserved"] = fb.report.get("observations_reobserved", 0) + int(mine.sum())
            fb.add_segment(first[s_], ids, Ts, np.concatenate([e_frame[we], ro["frame"][mine].astype(np.int64)]), np.concatenate([e_id[we], ro["lm_id"][mine]]),
                           np.concatenate([ba_uv[we].reshape(-1, 2), np.stack([ro["u"][mine], ro["v"][mine]], 1)]), lm_id[wl], lm_xyz[wl], kp_xyz, kp_valid,
                           T_new=T_new, merge=reobserved["merge"])
        if edges is not None:
            fb.add_loop_edges(edges, frame_offset=frame_offset)
        out = fb.optimize(self.vo, params=params)
        self.full_ba_result = dict(report=fb.report, segments=fb.last)
        return out

    def close(self):
        self.vo.close()


class PipelineRing:
    """P keyframe pipelines -- a context, a HIP stream and the device buffers of one batch each -- whose steps are in flight TOGETHER.

    Batches are independent (throughput mode), and a single step cannot keep the chip busy on its own: the BA kernel runs one window per
    CU for milliseconds (its last windows leave CUs empty, its SIMDs issue ~half the time), every ORB launch ends in a tail, the small
    bookkeeping kernels between them are latency.  With step k + 1 queued on a second stream the hardware scheduler fills those holes
    with the other batch's workgroups: 38.6 k -> 41.6 k keyframes/s at 2 x 512 keyframes in flight, results bit-identical to one pipeline
    stepping alone (tests/test_gpu_pipeline.py).  A third pipeline adds nothing (41.8 k at 3 x 256).
    step() hands the next batch to pipeline k mod P and returns without synchronising; sync() waits for all of them."""

    def __init__(self, P, B, distinct=False, sequences=None, **kw):
        """distinct: every pipeline renders (or is handed, `sequences[i]`) ITS OWN sequence of frames -- seed + 7919 i -- so that the batches in flight
        together are different data; otherwise all pipelines show the first one's frames (tests compare their results bit for bit)"""
        assert P >= 1
        kw0 = dict(kw)
        segmented = kw.get("segments") is not None   # (segments / segment_sequences pass through; `sequences[i]` is then pipeline i's segment_sequences)
        seq_key = "segment_sequences" if segmented else "sequence"
        if sequences is not None:
            kw0[seq_key] = sequences[0]
        first = KeyframePipeline(B, **kw0)
        self.pipes = [first]
        for i in range(1, P):
            kw2 = dict(kw)
            kw2["unique_frames"] = first.unique_frames
            kw2["verbose"] = False
            if sequences is not None and i < len(sequences):
                kw2[seq_key] = sequences[i]; kw2["render_workers"] = 0
            elif distinct:   # (a segmented pipeline uses seed + 7919 s for its segments: the next pipeline's seeds start after them)
                kw2["seed"] = kw.get("seed", 0) + 7919 * i * (len(kw["segments"]) if segmented else 1)
            else:
                kw2[seq_key] = first.h_seqs if segmented else first.h_seq   # the other pipelines show the same rendered frames: no second rendering
                kw2["render_workers"] = 0
            self.pipes.append(KeyframePipeline(B, **kw2))
        self.distinct = distinct or (sequences is not None and len(sequences) > 1)
        self.k = 0

    def __len__(self):
        return len(self.pipes)

    def next_pipe(self):
        return self.pipes[self.k % len(self.pipes)]

    def step(self):
        p = self.next_pipe()
        p.step()
        self.k += 1
        return p

    def sync(self):
        for p in self.pipes:
            p.vo.sync()

    def close(self):
        for p in self.pipes:
            if p.vo.h:
                p.close()
