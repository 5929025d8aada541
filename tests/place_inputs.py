"""Inputs of the loop-closure pipeline test: one rendered drive (pass A), the same places revisited at perturbed poses (pass B) and a foreign place.

  pass A: frames 0, 4, ..., 36 of synth._sequence_scene(40, 5) -- ten frames, about 4 m apart;
  pass B: the same ten poses, each perturbed in order with rng = default_rng(1): tx += U(-0.5, 0.5), tz += U(-0.5, 0.5), R <- rot_y(U(-0.03, 0.03)) R;
  foreign: frames 0, 4, ..., 16 of synth._sequence_scene(40, 77).

On the CPU oracle (oracle.feature_detection at anms_num = 500, the score restated in numpy, tau = 30) every B frame's twin scored 83..148, the best other
eligible A frame at most 54, the foreign scene at most 2 and frames 20 m apart at most 3: the conditions under which min_score = 60 separates them."""
import numpy as np

N_PASS, N_FOREIGN, STRIDE = 10, 5, 4


def _render(synth, sc, poses, w, h):
    out = []
    for T in poses:
        L, depth = sc.render(T, w, h)
        R, _ = sc.render(T, w, h, x_offset=synth.BASELINE)
        out.append((L, R, T, depth))
    return out


def loop_inputs(synth, w=None, h=None):
    """dict(A, B, foreign): lists of (left, right, T_c_w, depth) as synth.stereo_sequence returns them; the poses are the render poses (ground truth)"""
    w = synth.W_KITTI if w is None else w
    h = synth.H_KITTI if h is None else h
    traj, sc = synth._sequence_scene(40, 5)
    poses_a = [np.asarray(traj[i], np.float64).copy() for i in range(0, N_PASS * STRIDE, STRIDE)]
    rng = np.random.default_rng(1)
    poses_b = []
    for T in poses_a:
        T = T.copy()
        T[4] += rng.uniform(-0.5, 0.5)
        T[6] += rng.uniform(-0.5, 0.5)
        R = synth.rot_y(rng.uniform(-0.03, 0.03)) @ synth.R_from_quat(T[:4])
        poses_b.append(synth.se3_from_Rt(R, T[4:]))
    traj_f, sc_f = synth._sequence_scene(40, 77)
    poses_f = [traj_f[i] for i in range(0, N_FOREIGN * STRIDE, STRIDE)]
    return dict(A=_render(synth, sc, poses_a, w, h), B=_render(synth, sc, poses_b, w, h), foreign=_render(synth, sc_f, poses_f, w, h))
