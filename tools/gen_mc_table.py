#!/usr/bin/env python3
"""Derive the marching-cubes table of the surface map's mesh (include/vslam_hip.h "MESH") from its rule and write csrc/mc_table.inc.

Nothing is copied from a published table: the corner and edge numbering is the header's own (corner dx + 2 dy + 4 dz; edge 4 e + p + 2 q runs from
corner p f^ + q g^ along e^, f = (e + 1) % 3, g = (e + 2) % 3) and every row follows from the face rule -- segments on each of the six faces read
from that face's four signs alone, directed with the positive side on their left seen from outside, chained into loops, each loop fanned from its
lowest-numbered member whose fan diagonals never join two edges of one face.  All arithmetic is in doubled integer coordinates.

    python tools/gen_mc_table.py            # writes stereo-visual-slam_amd/csrc/mc_table.inc and prints the table's figures

A row is one uint64: triangle j's three cube edges in bits 12 j .. 12 j + 11 (4 bits each, first corner lowest), the triangle count in bits 60 .. 63."""
import os
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "stereo-visual-slam_amd", "csrc", "mc_table.inc")


def corner_xyz(i):
    return (i & 1, (i >> 1) & 1, (i >> 2) & 1)


def corner_id(c):
    return c[0] + 2 * c[1] + 4 * c[2]


def edge_corners(k):
    e, p, q = k >> 2, k & 1, (k >> 1) & 1
    a = [0, 0, 0]
    a[(e + 1) % 3] = p
    a[(e + 2) % 3] = q
    b = list(a)
    b[e] = 1
    return corner_id(a), corner_id(b)


EDGES = [edge_corners(k) for k in range(12)]
# doubled coordinates: a corner is (0 | 2, ...), an edge midpoint has one odd coordinate
MID2 = [tuple(x + y for x, y in zip(corner_xyz(a), corner_xyz(b))) for a, b in EDGES]
# a face is (axis d, side s): its outward normal is -d^ (s = 0) or +d^ (s = 1)
FACES = [(d, s) for d in range(3) for s in (0, 1)]
FACE_EDGES = {fc: [k for k in range(12) if all(corner_xyz(c)[fc[0]] == fc[1] for c in EDGES[k])] for fc in FACES}
FACE_CORNERS = {fc: [c for c in range(8) if corner_xyz(c)[fc[0]] == fc[1]] for fc in FACES}


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def directed(fc, ka, kb, pos_corner):
    """the segment between face edges ka and kb, directed so that n . ((m_B - m_A) x (P - m_A)) > 0"""
    d, s = fc
    ma, mb = MID2[ka], MID2[kb]
    P2 = tuple(2 * x for x in corner_xyz(pos_corner))
    w = cross(tuple(b - a for a, b in zip(ma, mb)), tuple(p - a for a, p in zip(ma, P2)))[d] * (1 if s else -1)
    assert w != 0
    return (ka, kb) if w > 0 else (kb, ka)


def segments(cube):
    sign = [(cube >> c) & 1 for c in range(8)]
    segs = []
    for fc in FACES:
        crossing = [k for k in FACE_EDGES[fc] if sign[EDGES[k][0]] != sign[EDGES[k][1]]]
        pos = [c for c in FACE_CORNERS[fc] if sign[c]]
        if len(crossing) == 2:
            segs.append(directed(fc, crossing[0], crossing[1], pos[0]))
        elif len(crossing) == 4:   # two positive corners on a diagonal: each is cut off by a segment of its own
            assert len(pos) == 2
            for c in pos:
                ka, kb = [k for k in crossing if c in EDGES[k]]
                segs.append(directed(fc, ka, kb, c))
        else:
            assert not crossing
    return segs


def share_face(ka, kb):
    return any(ka in ks and kb in ks for ks in FACE_EDGES.values())


def row(cube):
    """the triangles of one configuration as tuples of three cube edges"""
    segs = segments(cube)
    succ = dict(segs)
    assert len(succ) == len(segs) and sorted(succ) == sorted(succ.values()), "every crossing edge has one successor and one predecessor"
    loops, seen = [], set()
    for k in sorted(succ):
        if k in seen:
            continue
        loop = [k]
        while succ[loop[-1]] != k:
            loop.append(succ[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    tris = []
    for loop in loops:   # (found in the order of their smallest member)
        n = len(loop)
        starts = [i for i in range(n) if not any(share_face(loop[i], loop[(i + j) % n]) for j in range(2, n - 1))]
        assert starts, "no fan start without a diagonal inside a face"
        i0 = min(starts, key=lambda i: loop[i])
        l = loop[i0:] + loop[:i0]
        tris += [(l[0], l[i], l[i + 1]) for i in range(1, n - 1)]
    return tris, max((len(l) for l in loops), default=0)


def table():
    rows, longest = [], 0
    for cube in range(256):
        tris, ln = row(cube)
        rows.append(tris)
        longest = max(longest, ln)
    return rows, longest


def pack(tris):
    w = len(tris) << 60
    for j, t in enumerate(tris):
        for c, k in enumerate(t):
            w |= k << (12 * j + 4 * c)
    return w


def main():
    rows, longest = table()
    hist = Counter(len(r) for r in rows)
    assert max(hist) <= 5 and rows[1] == [(0, 8, 4)] and rows[254] == [(0, 4, 8)]
    print("triangles %d, rows by count %s, longest loop %d" % (sum(len(r) for r in rows), dict(sorted(hist.items())), longest))
    with open(OUT, "w") as f:
        f.write("/* GENERATED by tools/gen_mc_table.py from the MESH rule of include/vslam_hip.h -- 256 rows, one uint64 each: triangle j's three cube edges in\n"
                " * bits 12 j .. 12 j + 11 (4 bits each), the triangle count in bits 60 .. 63.  Data only. */\n")
        f.write("__constant__ unsigned long long k_mc_table[256] = {\n")
        for i in range(0, 256, 4):
            f.write("  " + ", ".join("0x%016xull" % pack(r) for r in rows[i:i + 4]) + ",\n")
        f.write("};\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
