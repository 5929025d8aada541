"""CPU: the render yardstick tests/tsdf_render_ref.py held to what a ray-cast of a TSDF must do -- a ray worked by hand, the back-face and
from-unknown rules on a field full of holes, views that take no part, the analytic sphere, and the integrated `scene` against the depth maps it was
fused from.  The device kernels are held to the yardstick bit for bit by tests/test_gpu_tsdf_render.py."""
import numpy as np

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_render_cases as RC
import tsdf_render_ref as RR

IDENT_AT = lambda eye: np.array([0, 0, 0, 1, -eye[0], -eye[1], -eye[2]], np.float64)   # R = I: t = -eye


def _two_block_field():
    """blocks (0, 0, 0, 0) and (0, 0, 0, 1) of 0.25 m voxels: q depends on iz only, q(iz) = 300 (8 - iz) + 120, seen (W = Wc = 1, I = 100) for iz in 6 .. 10"""
    ids = np.array([[0, 0, 0, 0], [0, 0, 0, 1]], np.int32)
    vox = np.zeros((2, 512, 4), np.uint32)
    for b in range(2):
        for l in range(512):
            iz = 8 * b + (l >> 6)
            if 6 <= iz <= 10:
                vox[b, l] = (1, 300 * (8 - iz) + 120 + 1024, 1, 100)
    return ids, vox


def test_a_ray_worked_by_hand():
    """The camera at (1, 1, 0) looks along +z: g = (3.5, 3.5, Z / 0.25 - 0.5), so a sample reads voxels iz = 3 + k and 4 + k half and half.
    k = 3: (720 + 420) / 2 = 570; k = 4: (420 + 120) / 2 = 270; k = 5: (120 - 180) / 2 = -30: the ray ends, s = 270 / 300 = 0.9,
    Z* = 2.0 + 0.9 * 0.25 = 2.225 -- where q crosses zero (iz + 0.5 = 8.9).  The gradient is (0, 0, -300): the normal looks back at the camera."""
    ids, vox = _two_block_field()
    out = RR.render(ids, vox, 0.25, IDENT_AT((1.0, 1.0, 0.0))[None], [0], (1.0, 1.0, 0.0, 0.0), (1, 1), 1.0, 3.0, march=1.0)
    assert out["K"] == 8 and out["hits"] == 1
    assert out["depth"][0, 0, 0] == np.float32(2.0 + 0.9 * 0.25)
    assert out["attr"][0, 0, 0].tolist() == [0.0, 0.0, -1.0, 100.0]
    assert out["margin_D"] == 30.0 and out["margin_g"] == 0.5
    # the same ray from behind the surface meets a negative sample first: a back face is not rendered
    back = RR.look_at((1.0, 1.0, 4.0), (1.0, 1.0, 0.0))
    out = RR.render(ids, vox, 0.25, back[None], [0], (1.0, 1.0, 0.0, 0.0), (1, 1), 1.0, 3.5, march=1.0)
    assert out["hits"] == 0 and not out["depth"].any() and not out["attr"].any()
    # min_weight 2 leaves nothing known
    out = RR.render(ids, vox, 0.25, IDENT_AT((1.0, 1.0, 0.0))[None], [0], (1.0, 1.0, 0.0, 0.0), (1, 1), 1.0, 3.0, march=1.0, min_weight=2)
    assert out["hits"] == 0 and out["margin_D"] == np.inf


def test_samples_of():
    assert RR.samples_of(1.0, 3.0, 0.25) == 8 and RR.samples_of(1.0, 3.0001, 0.25) == 9 and RR.samples_of(0.5, 0.6, 1.0) == 1
    for z0, z1, hs in ((0.3, 8.0, 0.075), (2.0, 25.0, 0.1), (0.25, 9.0, 0.025)):
        K = RR.samples_of(z0, z1, hs)
        assert z0 + np.float64(K) * hs >= z1 and not (z0 + np.float64(K - 1) * hs >= z1)


def test_views_that_take_no_part_are_all_misses():
    ids, vox = _two_block_field()
    T = IDENT_AT((1.0, 1.0, 0.0))
    nan, inf = T.copy(), T.copy()
    nan[1] = np.nan
    inf[6] = np.inf
    poses = np.stack([T, T, T, T, nan, inf])
    out = RR.render(ids, vox, 0.25, poses, [0, -1, 1023, 3, 0, 0], (1.0, 1.0, 0.0, 0.0), (1, 1), 1.0, 3.0, march=1.0)
    assert out["hits"] == 1 and out["depth"][0, 0, 0] > 0
    assert not out["depth"][1:].any() and not out["attr"][1:].any()


def test_back_faces_and_surfaces_entered_from_unknown_space_are_not_rendered():
    """noise_holes, marched again by a plain state machine per ray over samples computed for every k: the yardstick's hits are exactly the rays whose
    first known non-positive sample follows a known positive one; endings that are refused (the sample before was unknown, or there was none) occur"""
    c = MC.cases()["noise_holes"]
    cam, (w, h), (z0, z1), march = (14.0, 14.0, 9.3, 6.7), (20, 14), RC.NOISE_Z, 0.5
    T = RC.noise_views()
    got = RR.render(c["ids"], c["voxels"], c["voxel_size"], T, np.zeros(len(T), np.int32), cam, (w, h), z0, z1, march)
    vs = np.float64(np.float32(c["voxel_size"]))
    tab = RR.tables_of(c["ids"], c["voxels"])[0]
    cc, rr = np.meshgrid(np.arange(w), np.arange(h))
    x, y = (cc.ravel() - np.float64(cam[2])) / cam[0], (rr.ravel() - np.float64(cam[3])) / cam[1]
    kinds = {"hit": 0, "refused": 0, "none": 0}
    for v in range(len(T)):
        _, _, Rinv, tinv, _ = RR.TR.frame_of(T[v])
        known, D = [], []
        for k in range(got["K"]):
            kn, Dk, _, _, _ = RR.sample(tab, Rinv, tinv, x, y, np.float64(z0) + np.float64(k) * (march * vs), vs, 1)
            known.append(kn); D.append(Dk)
        known, D = np.array(known), np.array(D)
        for p in range(w * h):
            kind, after_positive = "none", False
            for k in range(got["K"]):
                if known[k, p] and not D[k, p] > 0:   # the first known sample that is not positive ends the ray
                    kind = "hit" if after_positive else "refused"
                    break
                after_positive = bool(known[k, p])
            kinds[kind] += 1
            assert (got["depth"][v].ravel()[p] > 0) == (kind == "hit"), (v, p, kind)
            if kind != "hit":
                assert not got["attr"][v].reshape(-1, 4)[p].any()
    assert kinds["hit"] > 50 and kinds["refused"] > 20 and kinds["none"] > 0, kinds
    assert got["hits"] == kinds["hit"]


def test_the_analytic_sphere():
    """four views from outside at march 0.5: no hit off the sphere, at least 99 % of the rays that meet it hit, every hit within one voxel of the
    analytic intersection along the ray, the median within a tenth"""
    c = MC.cases()["sphere"]
    ref = RC.reference_of("sphere", 0.5)
    fx, fy, cx, cy = RC.SPHERE_CAM
    w, h = RC.SPHERE_SIZE
    cc, rr = np.meshgrid(np.arange(w), np.arange(h))
    x, y = (cc - cx) / fx, (rr - cy) / fy
    errs = []
    for v, eye in enumerate(RC.SPHERE_EYES):
        R = RR.TR.frame_of(ref["T"][v])[2].reshape(3, 3)           # Rinv: camera -> world
        d = np.stack([R[a, 0] * x + R[a, 1] * y + R[a, 2] for a in range(3)], -1)   # the ray per unit of camera z
        o = np.asarray(eye) - c["centre"]
        A, B, Cq = (d * d).sum(-1), 2 * (d * o).sum(-1), (o * o).sum() - RC.SPHERE_RADIUS ** 2
        disc = B * B - 4 * A * Cq
        meets = disc > 0
        Zt = np.where(meets, (-B - np.sqrt(np.where(meets, disc, 0))) / (2 * A), 0)
        hit = ref["depth"][v] > 0
        assert not (hit & ~meets).any(), "a hit on a ray that misses the sphere"
        assert (hit & meets).sum() >= 0.99 * meets.sum(), ((hit & meets).sum(), meets.sum())
        errs.append((np.abs(ref["depth"][v] - Zt) * np.sqrt(A))[hit] / c["voxel_size"])
        n = ref["attr"][v][hit][:, :3].astype(np.float64)
        radial = ((eye + d * ref["depth"][v][..., None].astype(np.float64)) - c["centre"])[hit]
        radial /= np.sqrt((radial * radial).sum(-1, keepdims=True))
        assert np.median((n * radial).sum(-1)) > 0.99, "the normals point out of the sphere, into free space"
        assert np.allclose(ref["attr"][v][hit][:, 3], 100.0)
    errs = np.concatenate(errs)
    print("sphere: %d hits, median %.4f voxel, max %.4f voxel" % (len(errs), np.median(errs), errs.max()))
    assert errs.max() <= 1.0 and np.median(errs) <= 0.1, (errs.max(), np.median(errs))


SCENE_MEDIAN, SCENE_P95 = 0.05, 0.05   # voxels: the yardstick's own 0.0006 and 0.0024, each rounded up to the next 0.05


def test_the_scene_rendered_at_its_integrating_poses_returns_the_depth_it_was_fused_from():
    case = TC.cases()["scene"]
    ref = RC.reference_of("scene", 0.5)
    with np.errstate(divide="ignore"):
        z_in = case["cam"][0] * case["cam"][4] / case["disp"].astype(np.float64)
    both = (ref["depth"] > 0) & (z_in > case["z_min"]) & (z_in < case["z_max"])
    err = np.abs(ref["depth"].astype(np.float64) - z_in)[both] / case["voxel_size"]
    print("scene: %d of %d pixels compared, median %.4f voxel, p95 %.4f voxel, margins D %.3g g %.3g"
          % (both.sum(), both.size, np.median(err), np.percentile(err, 95), ref["margin_D"], ref["margin_g"]))
    assert both.sum() > 0.5 * both.size
    assert np.median(err) <= SCENE_MEDIAN and np.percentile(err, 95) <= SCENE_P95
