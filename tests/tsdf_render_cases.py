"""Views of the render tests (tests/test_tsdf_render_ref.py on the CPU, tests/test_gpu_tsdf_render.py on the device) over the fields of
tests/tsdf_mesh_cases.py, and the yardstick's answer for each, computed once and shared: do not change it."""
import functools

import numpy as np

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_render_ref as RR

SPHERE_EYES = ((1.8, 1.8, -1.6), (5.0, 4.2, 0.3), (-1.0, 1.0, 4.5), (1.9, 5.2, 1.7))
SPHERE_CAM, SPHERE_SIZE, SPHERE_Z = (50.0, 50.0, 31.37, 23.61), (64, 48), (0.3, 8.0)
SPHERE_RADIUS = 1.31

# the noise fields fill [-3.2, 1.6)^3: two cameras outside looking in, one inside the field (in the absent centre block of noise_holes)
NOISE_CAM, NOISE_SIZE, NOISE_Z = (40.0, 40.0, 33.41, 22.63), (67, 45), (0.25, 9.0)
NOISE_EYES = (((-6.1, -0.9, -0.7), (-0.8, -0.8, -0.8)), ((0.3, 3.9, -5.2), (-0.8, -0.8, -0.8)), ((-0.83, -0.77, -0.81), (1.0, 0.4, 2.0)))


def sphere_views():
    centre = MC.cases()["sphere"]["centre"]
    return np.stack([RR.look_at(e, centre) for e in SPHERE_EYES])


def noise_views():
    return np.stack([RR.look_at(e, t) for e, t in NOISE_EYES])


def two_maps_views():
    """views of map 0 and of map 5, of a map without blocks, of map id -1 and with a NaN pose: (T (5, 7), map_id (5,))"""
    a = RR.look_at((-3.4, -0.6, -0.3), (0.0, 0.0, 0.0))
    b = RR.look_at((0.4, 0.2, -3.9), (0.0, 0.0, 0.0))
    nan = a.copy()
    nan[5] = np.nan
    return np.stack([a, b, a, b, nan]), np.array([0, 5, 7, -1, 0], np.int32)


def scene_call():
    """the `scene` case of tsdf_cases at its four integrating poses with its own camera and gates"""
    case = TC.cases()["scene"]
    n, h, w = case["disp"].shape
    return dict(T=case["T"], map_id=case["map_id"], cam=case["cam"][:4], size=(w, h), z_min=case["z_min"], z_max=case["z_max"])


@functools.lru_cache(maxsize=None)
def reference_of(name, march=0.5, min_weight=1):
    """the yardstick's render of a case's standard views"""
    c = MC.cases()[name]
    if name == "sphere":
        T, ids, cam, size, (z0, z1) = sphere_views(), np.zeros(4, np.int32), SPHERE_CAM, SPHERE_SIZE, SPHERE_Z
    elif name == "two_maps":
        (T, ids), cam, size, (z0, z1) = two_maps_views(), NOISE_CAM, NOISE_SIZE, NOISE_Z
    elif name == "scene":
        s = scene_call()
        T, ids, cam, size, z0, z1 = s["T"], s["map_id"], s["cam"], s["size"], s["z_min"], s["z_max"]
    else:
        T, ids, cam, size, (z0, z1) = noise_views(), np.zeros(3, np.int32), NOISE_CAM, NOISE_SIZE, NOISE_Z
    out = RR.render(c["ids"], c["voxels"], c["voxel_size"], T, ids, cam, size, z0, z1, march, min_weight)
    out.update(T=T, map_id=ids, cam=cam, size=size, z_min=z0, z_max=z1, march=march, min_weight=min_weight)
    for k in ("depth", "attr"):
        out[k].setflags(write=False)
    return out
