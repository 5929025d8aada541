"""CPU: what the rule of match by projection is worth on rendered frames (tests/place_inputs.py): oracle ORB at anms_num = 500, landmarks = the source
frame's keypoints at their render-depth world points, projected into the target frame at its render pose moved by up to 0.2 m, the yardstick at radius
15, tau 50, ratio 80 %.  A match is correct when the two keypoints' render-depth world points agree within max(0.05 m, 2 % of depth).
Measured (printed by the test): see the assertion message; the floors are 40 matches per pair and 95 % of them correct."""
import numpy as np
import pytest

import place_inputs as PI
import project_match_ref as R
import project_match_truth as PT

PAIRS = (("A", 0, "A", 1), ("A", 0, "A", 2), ("A", 3, "B", 3), ("A", 3, "B", 4), ("A", 5, "B", 5))


@pytest.fixture(scope="module")
def frames(synth, oracle):
    inputs = PI.loop_inputs(synth)
    out = {}
    for name, i in sorted({(p[0], p[1]) for p in PAIRS} | {(p[2], p[3]) for p in PAIRS}):
        L, _, T, depth = inputs[name][i]
        kps, desc = oracle.feature_detection(L)
        out[(name, i)] = dict(xy=np.stack([kps["x"], kps["y"]], 1).astype(np.float32), desc=desc, T=np.asarray(T, np.float64), depth=depth)
    return out


def test_precision_of_the_rule_on_rendered_pairs(frames, synth):
    K4 = synth.CAM[:4]
    rng = np.random.default_rng(12)
    worst_n, worst_p = 10 ** 9, 1.0
    for a, i, b, j in PAIRS:
        src, dst = frames[(a, i)], frames[(b, j)]
        W, _ = PT.world_points(src["xy"], src["depth"], src["T"], K4, synth.R_from_quat)
        keep = np.flatnonzero(np.isfinite(W).all(1))
        noise = rng.normal(size=3); noise *= rng.uniform(0, 0.2) / np.linalg.norm(noise)
        T = dst["T"].copy(); T[4:] += noise
        got = R.project_match([0, len(keep)], [0], T[None], W[keep], keep.astype(np.int32), src["desc"], dst["xy"][None], dst["desc"][None], [len(dst["xy"])], K4,
                              synth.W_KITTI, synth.H_KITTI, radius_px=15.0, tau=50, ratio_pct=80)
        m = np.flatnonzero(got["status"] == R.MATCHED)
        Wd, zd = PT.world_points(dst["xy"][got["match"][m]], dst["depth"], dst["T"], K4, synth.R_from_quat)
        ok = PT.correct(W[keep][m], Wd, zd)
        prec = ok.sum() / max(len(m), 1)
        print("%s%d -> %s%d: %d matches, %d correct (%.3f); pose moved by %.3f m" % (a, i, b, j, len(m), ok.sum(), prec, np.linalg.norm(noise)))
        assert len(m) >= 40 and prec >= 0.95, (a, i, b, j, len(m), prec)
        worst_n, worst_p = min(worst_n, len(m)), min(worst_p, prec)
    print("fewest matches %d, lowest precision %.3f" % (worst_n, worst_p))
    assert worst_p >= PT.CPU_PRECISION
