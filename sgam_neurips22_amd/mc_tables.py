"""Marching-cubes tables derived from first principles (no table is typed in): `python -m sgam_neurips22_amd.mc_tables`
rewrites csrc/mc_tables.h, and tests/test_mesh_cpu.py regenerates it and compares bytes.

Cube conventions (the kernels' and tests/mc_oracle.py's):
  corner c = (c & 1, (c >> 1) & 1, c >> 2) as (x, y, z) offsets from the cell's low lattice point; case bit c = (f(c) < 0);
  edge e: axis a = e // 4, low end at the corner whose two other coordinates are the bits of j = e % 4, lower axis first
          (a = 0: (0, j & 1, j >> 1); a = 1: (j & 1, 0, j >> 1); a = 2: (j & 1, j >> 1, 0)).
Construction per sign configuration:
  1. every edge whose ends differ in sign carries a vertex;
  2. on each of the six faces the intersected edges are joined into segments; an ambiguous face (diagonal corners of equal
     sign, four intersected edges) cuts off each NEGATIVE corner on its own — a rule that depends on the face's four signs
     only, so the two cells sharing a face always draw the same segments (watertight by construction);
  3. each segment is directed so that, seen from outside the cube, the negative side lies to its right
     ((outward normal x direction) points to the positive side); the segments then chain into closed loops;
  4. each loop is fan-triangulated, (v0, v1, v2), (v0, v2, v3), ..., from the first vertex (in loop order) none of whose
     diagonals joins two vertices of one cube face (such a diagonal lies in the face, where the neighbour cell may draw it too:
     an edge of four triangles) — the winding puts every normal (v1 - v0) x (v2 - v0) on the side of positive TSDF (free
     space, the side the cameras see).
This is NOT Open3D's (Bourke / Bloyd) table: on non-ambiguous faces it triangulates the same surface; on ambiguous faces
Open3D's choice is unpinned."""
import os

CORNERS = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]


def _edge(e):
    a, j = e // 4, e % 4
    lo = [0, 0, 0]
    others = [r for r in range(3) if r != a]
    lo[others[0]], lo[others[1]] = j & 1, j >> 1
    hi = list(lo)
    hi[a] = 1
    return a, CORNERS.index(tuple(lo)), CORNERS.index(tuple(hi))


EDGES = [_edge(e) for e in range(12)]                 # (axis, low corner, high corner)


def _faces():
    """(outward normal, the face's four corners in cyclic order, its four edges)"""
    out = []
    for a in range(3):
        for s in (0, 1):
            u, v = [r for r in range(3) if r != a]
            cyc = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[a], p[u], p[v] = s, du, dv
                cyc.append(CORNERS.index(tuple(p)))
            edges = [e for e in range(12) if {EDGES[e][1], EDGES[e][2]} <= set(cyc)]
            n = [0, 0, 0]
            n[a] = 1 if s else -1
            out.append((tuple(n), cyc, edges))
    return out


FACES = _faces()


def _mid(e):
    a, c0, _ = EDGES[e]
    p = [float(x) for x in CORNERS[c0]]
    p[a] += 0.5
    return p


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def face_segments(case, face):
    """the directed segments (edge, edge) that `case` draws on face `face` (index into FACES)"""
    n, cyc, _ = FACES[face]
    neg = [bool((case >> c) & 1) for c in cyc]
    cut = [e for e in FACES[face][2] if ((case >> EDGES[e][1]) & 1) != ((case >> EDGES[e][2]) & 1)]
    if not cut:
        return []

    def edge_of(c0, c1):
        return next(e for e in FACES[face][2] if {EDGES[e][1], EDGES[e][2]} == {c0, c1})

    pairs = []
    if len(cut) == 2:
        pairs.append(tuple(cut))
    else:                                             # ambiguous: cut off each negative corner
        assert len(cut) == 4 and neg[0] == neg[2] and neg[1] == neg[3] and neg[0] != neg[1]
        for k in range(4):
            if neg[k]:
                pairs.append((edge_of(cyc[k], cyc[k - 1]), edge_of(cyc[k], cyc[(k + 1) % 4])))
    segs = []
    for ea, eb in pairs:
        ma, mb = _mid(ea), _mid(eb)
        d = [mb[r] - ma[r] for r in range(3)]
        side = _cross(n, d)
        c_neg = next(c for k, c in enumerate(cyc) if neg[k])
        # which side of the segment's line the negative corners of this pair's region lie on
        s = sum(side[r] * (CORNERS[c_neg][r] - ma[r]) for r in range(3))
        if len(pairs) == 2:                           # (ambiguous face: measure against the corner this segment cuts off)
            c_cut = next(c for k, c in enumerate(cyc) if neg[k] and ea in _corner_edges(c, face) and eb in _corner_edges(c, face))
            s = sum(side[r] * (CORNERS[c_cut][r] - ma[r]) for r in range(3))
        assert s != 0
        segs.append((ea, eb) if s < 0 else (eb, ea))
    return segs


def _corner_edges(c, face):
    return [e for e in FACES[face][2] if c in (EDGES[e][1], EDGES[e][2])]


def case_loops(case):
    """closed loops of edges (directed) of one sign configuration"""
    nxt = {}
    for f in range(6):
        for a, b in face_segments(case, f):
            assert a not in nxt
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def _share_face(ea, eb):
    return any(ea in f[2] and eb in f[2] for f in FACES)


def _triangulate(loop):
    """fan of the loop from the first apex whose diagonals join no two vertices of one cube face: such a diagonal would lie
    in the face, where the neighbour cell may draw the same one (an edge of four triangles).  Apexes are tried in loop order."""
    n = len(loop)
    for r in range(n):
        lp = loop[r:] + loop[:r]
        if all(not _share_face(lp[0], lp[k]) for k in range(2, n - 1)):
            return [(lp[0], lp[k], lp[k + 1]) for k in range(1, n - 1)]
    raise AssertionError(f"no admissible fan for loop {loop}")


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        tris += _triangulate(loop)
    return tris


def tables():
    """(edge mask per case, triangle list per case, max triangles per case)"""
    masks, tris = [], []
    for case in range(256):
        masks.append(sum(1 << e for e in range(12) if ((case >> EDGES[e][1]) & 1) != ((case >> EDGES[e][2]) & 1)))
        tris.append(case_triangles(case))
    return masks, tris, max(len(t) for t in tris)


def header_text():
    masks, tris, mt = tables()
    lines = ["// mc_tables.h — GENERATED by sgam_neurips22_amd/mc_tables.py (do not edit; tests/test_mesh_cpu.py regenerates and compares).",
             "// Marching-cubes tables derived by walking the cube's faces (see that module's docstring for the corner / edge numbering",
             "// and the ambiguous-face rule); not Open3D's table.",
             "#pragma once",
             "",
             f"#define SGAM_MC_MAX_TRIS {mt}",
             "",
             "// edge e: axis, low-end corner offset (x, y, z)",
             "__constant__ const signed char MC_EDGE[12][4] = {"]
    for e in range(12):
        a, c0, _ = EDGES[e]
        lines.append("    {%d, %d, %d, %d}," % ((a,) + CORNERS[c0]))
    lines += ["};", "", "// bit e set: edge e carries a vertex", "__constant__ const unsigned short MC_EDGE_MASK[256] = {"]
    for r in range(0, 256, 8):
        lines.append("    " + " ".join("0x%03x," % m for m in masks[r:r + 8]))
    lines += ["};", "", "// triangles per case", "__constant__ const unsigned char MC_NTRI[256] = {"]
    for r in range(0, 256, 16):
        lines.append("    " + " ".join("%d," % len(t) for t in tris[r:r + 16]))
    lines += ["};", "", f"// edge triples per case, in table order, padded with -1", f"__constant__ const signed char MC_TRI[256][{3 * mt}] = {{"]
    for case in range(256):
        flat = [e for t in tris[case] for e in t] + [-1] * (3 * (mt - len(tris[case])))
        lines.append("    {" + ", ".join(str(v) for v in flat) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_tables.h")


def table_arrays():
    """numpy form of the tables: (edge mask [256] int, ntri [256] int, tri [256][3 * max] int (-1 padded), edge [12][4] int)"""
    import numpy as np
    masks, tris, mt = tables()
    tri = np.full((256, 3 * mt), -1, dtype=np.int64)
    for c in range(256):
        flat = [e for t in tris[c] for e in t]
        tri[c, :len(flat)] = flat
    edge = np.array([(EDGES[e][0],) + CORNERS[EDGES[e][1]] for e in range(12)], dtype=np.int64)
    return np.array(masks), np.array([len(t) for t in tris]), tri, edge


if __name__ == "__main__":
    _, _, mt = tables()
    with open(HEADER, "w") as f:
        f.write(header_text())
    print(f"wrote {HEADER}: at most {mt} triangles per case")
