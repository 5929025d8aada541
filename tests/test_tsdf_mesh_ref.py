"""CPU: the mesh rule (include/vslam_hip.h "MESH").  The committed table csrc/mc_table.inc, parsed as data, against the yardstick's own derivation
(tests/tsdf_mesh_ref.py); the figures the rule must give; and the properties of the meshes the yardstick builds from the cases of
tests/tsdf_mesh_cases.py -- every configuration present, no directed edge twice, open edges only against cells that are not meshable, a closed
outward-facing sphere -- so that the device test compares against a yardstick that has itself been held to the rule."""
import os
import re

import numpy as np
import pytest

import tsdf_mesh_cases as MC
import tsdf_mesh_ref as MR
import voxel_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "stereo-visual-slam_amd", "csrc", "mc_table.inc")
WEIGHTS = (1, 2)


def _committed_rows():
    with open(TABLE) as f:
        words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]{16})ull", f.read())]
    assert len(words) == 256
    count = np.array([w >> 60 for w in words])
    edges = np.full((256, 5, 3), -1, np.int64)
    for i, w in enumerate(words):
        for j in range(count[i]):
            edges[i, j] = [(w >> (12 * j + 4 * c)) & 15 for c in range(3)]
        assert w & ((1 << 60) - 1) >> (12 * count[i]) << (12 * count[i]) == 0, "bits beyond the row's triangles"
    return count, edges


def test_the_committed_table_equals_the_rule():
    count, edges, _ = MR.mc_rows()
    got_count, got_edges = _committed_rows()
    assert np.array_equal(got_count, count)
    assert np.array_equal(got_edges, edges)


def test_the_rule_gives_the_figures_of_the_header():
    count, edges, longest = MR.mc_rows()
    assert count.max() == 5 and count.sum() == 820 and longest == 7
    assert {int(k): int((count == k).sum()) for k in range(6)} == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}
    assert edges[1, 0].tolist() == [0, 8, 4] and edges[254, 0].tolist() == [0, 4, 8]
    assert count[0] == 0 and count[255] == 0
    # (a row and its complement differ where a face is ambiguous: the positive corners are the ones cut apart)
    assert count[0b01000001] == 2 and count[255 - 0b01000001] == 4


def test_one_positive_corner_gives_one_triangle():
    """every voxel of one block at D < 0 except (3, 4, 5): the cell whose corner 0 it is has cube = 1 and emits (edge 0, edge 8, edge 4) = the
    voxel's own x, z and y edges, counter-clockwise seen from the positive voxel; the eight cells around the voxel give an octahedron"""
    vox = np.zeros((1, 512, 4), np.uint32)
    vox[..., 0] = 1; vox[..., 1] = 1024 - 512; vox[..., 2] = 1
    c = (3, 4, 5)
    vox[0, c[2] << 6 | c[1] << 3 | c[0], 1] = 1024 + 256
    ids = np.array([[0, -1, 2, 0]], np.int32)
    base = [-8 + c[0], 16 + c[1], c[2]]
    tk = MR.triangle_keys(ids, vox)
    assert len(tk) == 8
    mine = tk[(tk[:, :, :3] == base).all((1, 2))]
    assert mine.tolist() == [[base + [0], base + [2], base + [1]]]
    verts, tris = MR.mesh(ids, vox, 0.2)
    assert len(verts) == 6 and len(tris) == 8
    p = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    centre = (np.array(base) + 0.5) * np.float64(np.float32(0.2))
    n = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])
    assert (np.einsum("ij,ij->i", n, centre - p[tris].mean(1)) > 0).all(), "the normals point towards growing D: here into the octahedron"


@pytest.mark.parametrize("name", ["noise_full", "noise_holes"])
def test_every_configuration_occurs(name):
    c = MC.cases()[name]
    _, _, _, meshable, cube = MR.cells_of(c["ids"], c["voxels"], 1)
    n = np.bincount(cube[meshable], minlength=256)
    assert n.min() >= 3, (int(n.argmin()), int(n.min()))
    assert (n.mean() > 40) if name == "noise_full" else (12 < n.mean() < 40), n.mean()


def _directed_edges(tris):
    return np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).astype(np.int64)


def _open_edges(tris, n_vertices):
    e = _directed_edges(tris)
    code = e[:, 0] * n_vertices + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    return e[~np.isin(code, e[:, 1] * n_vertices + e[:, 0])]


@pytest.mark.parametrize("min_weight", WEIGHTS)
@pytest.mark.parametrize("name", ["noise_full", "noise_holes", "two_maps", "sphere", "scene"])
def test_edges_are_paired_except_against_cells_that_are_not_meshable(name, min_weight):
    c = MC.cases()[name]
    verts, tris = MC.reference_of(name, min_weight)
    if name == "sphere" and min_weight == 2:   # (every seen voxel of the sphere has W = 1)
        assert len(verts) == 0 and len(tris) == 0
        return
    assert len(tris) > 0 and tris.min() >= 0 and tris.max() < len(verts)
    opened = _open_edges(tris, len(verts))
    if name == "sphere":
        assert len(opened) == 0
        return
    for m in sorted(set(c["ids"][:, 0].tolist())):
        sel = c["ids"][:, 0] == m
        ix, iy, iz, meshable, _ = MR.cells_of(c["ids"][sel], c["voxels"][sel], min_weight)
        cells = np.sort(MR._pack(ix[meshable], iy[meshable], iz[meshable]))
        ev = verts[opened[verts["map"][opened[:, 0]] == m]]          # (n, 2) vertices
        a = np.stack([ev["ix"], ev["iy"], ev["iz"]], -1).astype(np.int64)   # (n, 2, 3) lower voxels
        b = a + (ev["axis"][..., None] == np.arange(3)).astype(np.int64)
        pts = np.concatenate([a, b], 1)                                 # (n, 4, 3): the lattice points of the two voxel edges
        flat = (pts == pts[:, :1]).all(1)                               # (n, 3): the axis across which they all agree
        assert (flat.sum(1) == 1).all(), "an open edge that lies in no cell face"
        upper = pts.min(1)
        lower = upper - flat
        has = lambda cell: np.isin(MR._pack(cell[:, 0], cell[:, 1], cell[:, 2]), cells)
        hu, hl = has(upper), has(lower)
        assert (hu != hl).all(), "an open edge needs exactly one meshable cell at its face"
        if name == "noise_full" and min_weight == 1:
            out = np.where(hu[:, None], lower, upper)
            assert ((out < -16) | (out > 6)).any(1).all(), "noise_full is open at the outer boundary only"
    assert len(opened) > 0


def test_the_sphere_is_closed_and_faces_outwards():
    c = MC.cases()["sphere"]
    verts, tris = MC.reference_of("sphere")
    assert len(_open_edges(tris, len(verts))) == 0
    V, E, F = len(np.unique(tris)), len(_directed_edges(tris)) // 2, len(tris)
    assert V == len(verts) and V - E + F == 2, (V, E, F)
    p = np.stack([verts["x"], verts["y"], verts["z"]], 1).astype(np.float64)
    n = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])
    area = np.linalg.norm(n, axis=1)
    inward = np.einsum("ij,ij->i", n, p[tris].mean(1) - c["centre"]) < 0
    assert F > 1000 and not (inward & (area > 0)).any(), int((inward & (area > 0)).sum())
    # ... and the surfel normals agree with the triangles they belong to
    vn = np.stack([verts["nx"], verts["ny"], verts["nz"]], 1).astype(np.float64)
    assert (np.einsum("ij,ij->i", n[area > 0], vn[tris[area > 0, 0]]) > 0).all()


@pytest.mark.parametrize("min_weight", WEIGHTS)
def test_two_maps_equal_the_two_maps_alone(min_weight):
    both_v, both_t = MC.reference_of("two_maps", min_weight)
    v0, t0 = MC.reference_of("two_maps", min_weight, 0)
    v5, t5 = MC.reference_of("two_maps", min_weight, 5)
    assert len(v0) and len(v5) and v0.tobytes() != v5.tobytes()
    assert np.concatenate([v0, v5]).tobytes() == both_v.tobytes()
    assert np.array_equal(np.concatenate([t0, t5 + len(v0)]), both_t)
    c = MC.cases()["two_maps"]
    sel = c["ids"][:, 0] == 5
    alone_v, alone_t = MR.mesh(c["ids"][sel], c["voxels"][sel], c["voxel_size"], min_weight)
    assert alone_v.tobytes() == v5.tobytes() and np.array_equal(alone_t, t5)


def test_min_weight_changes_the_holes_case():
    assert len(MC.reference_of("noise_holes", 1)[1]) > len(MC.reference_of("noise_holes", 2)[1]) > 0


def test_mesh_ply_round_trip(tmp_path):
    from stereo_visual_slam_amd.dense import read_mesh_ply, write_mesh_ply
    verts, tris = MC.reference_of("two_maps")
    path = str(tmp_path / "mesh.ply")
    write_mesh_ply(path, verts, tris)
    with open(path, "rb") as f:
        head = f.read(600).split(b"end_header\n")[0].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(verts)]
    assert head[-3:-1] == ["element face %d" % len(tris), "property list uchar int vertex_indices"]
    v, t = read_mesh_ply(path)
    assert np.array_equal(t, tris) and t.dtype == np.int32
    for name in v.dtype.names:
        assert np.array_equal(v[name].view(np.uint32), verts[name].view(np.uint32)), name
    with pytest.raises(AssertionError):
        write_mesh_ply(path, verts[:3], tris)
