"""Clean-up of a marching-cubes mesh on the device (csrc/mesh_ops.hip): connected components, removal of small
components, vertex / triangle incidence, vertex normals, Taubin smoothing, vertex clustering — and `clean`, which chains them.

Input: a `tsdf.DeviceMesh` (vertices (cap,3) fp32, vertex_colors (cap,3) fp32 or None, triangles (cap,3) int32, n_vertices /
n_triangles; rows beyond the sizes are never read).  Output meshes are new, exactly sized DeviceMesh objects with counts =
[nv, nt, 0, 0], which `tsdf.render_mesh_rgbd` takes unchanged.  An empty input gives an empty result without a launch.

Integer scans and compaction (`cumsum`, `nonzero`, row gathers by the compacted indices) are torch plumbing, as in
geometry.voxel_sample; everything else is a kernel.  Integer atomics only: results are bit-identical run to run; tests/meshops_oracle.py
restates every rule in numpy.  The rules follow Open3D's documented behaviour as recalled and are unpinned against Open3D.

Queries against a mesh (csrc/mesh_query.hip): `point_mesh_distance` / `TriangleGrid` (the exact distance from points
to the surface, brute force or a uniform grid of triangles, the same bits either way), `triangle_areas`, `sample_points` (points
drawn uniformly by area, a pure function of (mesh, seed, i)) and `surface_metrics` (geometry.cloud_metrics' numbers with a mesh on
either side); tests/meshquery_oracle.py restates them.

Rays against a mesh (csrc/mesh_ray.hip): `cast_rays` (the nearest hit), `test_occlusions` (any hit),
`create_rays_pinhole` and `visible_points` (which points a set of pinhole cameras sees, the mesh as the occluder), by brute force or
through the same `TriangleGrid`, the same bits either way; tests/raycast_oracle.py restates them.  Open3D's `RaycastingScene`
semantics (`cast_rays`, `test_occlusions`, `create_rays_pinhole`) are recalled, not pinned: Open3D is not available here.

`TriangleBVH` (csrc/mesh_bvh.hip) serves the same three queries through a bounding-volume hierarchy built on the
device, for meshes whose triangles are not near one scale; it is chosen explicitly (`accel=`, `accelerator="bvh"`), gives the same
bits, and tests/bvh_oracle.py restates it.

`simplify_quadric_decimation` (csrc/mesh_simplify.hip): quadric-error edge collapses in parallel rounds — fp64
vertex quadrics, a per-round cost threshold, an independent set of edges by two minimum passes over a scrambled edge id, flip and
link tests — without atomics, the same bits run to run; tests/decimation_oracle.py restates it.

There is no CPU fallback: a mesh that is not on the device raises `SgamHipError`."""
import math
import time

import numpy as np
import torch

from . import _lib, geometry
from .ops import SgamHipError, _need_cuda, _p, _stream, check
from .tsdf import DeviceMesh

KINDS = {"triangles": 0, "vertices": 1}


def make_mesh(vertices, triangles, vertex_colors=None):
    """an exactly-sized DeviceMesh of device tensors: vertices (nv,3) fp32, triangles (nt,3) int32, vertex_colors (nv,3) fp32 or None"""
    _need_cuda(vertices, triangles, vertex_colors)
    nv, nt = int(vertices.shape[0]), int(triangles.shape[0])
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or triangles.dim() != 2 or triangles.shape[1] != 3 or \
            triangles.dtype != torch.int32 or (vertex_colors is not None and (tuple(vertex_colors.shape) != (nv, 3) or vertex_colors.dtype != torch.float32)):
        raise ValueError("make_mesh: vertices (nv,3) fp32, triangles (nt,3) int32, vertex_colors (nv,3) fp32 or None")
    counts = torch.tensor([nv, nt, 0, 0], dtype=torch.int32, device=vertices.device)
    return DeviceMesh(vertices.contiguous(), None if vertex_colors is None else vertex_colors.contiguous(), triangles.contiguous(), counts, nv, nt)


def _sizes(mesh, what):
    _need_cuda(mesh.vertices, mesh.triangles, mesh.vertex_colors)
    nv, nt = int(mesh.n_vertices), int(mesh.n_triangles)
    v, t, c = mesh.vertices, mesh.triangles, mesh.vertex_colors
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype != torch.float32 or not v.is_contiguous() or t.dim() != 2 or t.shape[1] != 3 or \
            t.dtype != torch.int32 or not t.is_contiguous() or not 0 <= nv <= v.shape[0] or not 0 <= nt <= t.shape[0] or \
            (c is not None and (c.shape != v.shape or c.dtype != torch.float32 or not c.is_contiguous())):
        raise ValueError(f"{what}: a DeviceMesh of contiguous (cap,3) fp32 vertices [and colours] and (cap,3) int32 triangles, sizes within them")
    if nt and not nv:
        raise ValueError(f"{what}: {nt} triangles without a vertex")
    return nv, nt


def _flag(device):
    return torch.zeros((1,), dtype=torch.int32, device=device)


def _check_flag(flag, what):
    f = int(flag.item())
    if f & 2:
        raise SgamHipError(f"{what}: a triangle names a vertex outside the mesh")
    if f:
        raise SgamHipError(f"{what}: a loop ran into its bound (the workspace or the inputs changed under the kernel)")


def _i32(n, device):
    return torch.empty((n,), dtype=torch.int32, device=device)


def _scan(count):
    """(n,) int32 counts -> ((n+1,) int32 exclusive offsets, total): integer plumbing; synchronises"""
    off = torch.zeros((count.numel() + 1,), dtype=torch.int64, device=count.device)
    off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    total = int(off[-1].item())
    if total >= 2 ** 31:
        raise SgamHipError(f"mesh incidence: {total} entries do not fit int32 offsets")
    return off.to(torch.int32), total


def _part(mesh, vertex_index, triangles):
    """the exactly-sized mesh of the vertices at vertex_index (int64, ascending) with the given new triangles"""
    col = None if mesh.vertex_colors is None else mesh.vertex_colors[vertex_index]
    return make_mesh(mesh.vertices[vertex_index], triangles, col)


def components(mesh):
    """Connected components: two vertices are connected when a triangle uses both.  -> {"vertex_label" (nv,) int32: the least
    vertex index of the vertex's component (an unreferenced vertex: its own index), "triangle_label" (nt,) int32: the label of
    corner 0, "labels" (C,) int32 ascending: the components with at least one triangle, "n_triangles" (C,) int32}.  A lock-free
    union-find, one lane per triangle (sgam_mesh_components_i32)."""
    nv, nt = _sizes(mesh, "components")
    dev = mesh.vertices.device
    if nt == 0:
        e = _i32(0, dev)
        return {"vertex_label": torch.arange(nv, dtype=torch.int32, device=dev), "triangle_label": e, "labels": e.clone(), "n_triangles": e.clone()}
    ws, nbytes = geometry.workspace("sgam_mesh_components_workspace_bytes", dev, nv)
    vl, tl, cnt, flag = _i32(nv, dev), _i32(nt, dev), _i32(nv, dev), _flag(dev)
    check(_lib.load().sgam_mesh_components_i32(_p(mesh.triangles), nt, nv, _p(ws), nbytes, _p(vl), _p(tl), _p(cnt), _p(flag), _stream()),
          "sgam_mesh_components_i32")
    labels = torch.nonzero(cnt).reshape(-1)                                # compaction: plumbing (ascending); synchronises
    _check_flag(flag, "sgam_mesh_components_i32")
    return {"vertex_label": vl, "triangle_label": tl, "labels": labels.to(torch.int32), "n_triangles": cnt[labels]}


def select_triangles(mesh, keep):
    """The triangles with keep[t] ((nt,) bool on the device), in their order, and the vertices they use, in their order; indices
    remapped, colours carried.  -> {"mesh": DeviceMesh, "vertex_index" (new -> old) int32}"""
    nv, nt = _sizes(mesh, "select_triangles")
    dev = mesh.vertices.device
    _need_cuda(keep)
    if tuple(keep.shape) != (nt,) or keep.dtype != torch.bool:
        raise ValueError(f"select_triangles: keep is ({nt},) bool, not {tuple(keep.shape)} {keep.dtype}")
    tri_index = torch.nonzero(keep).reshape(-1) if nt else torch.empty((0,), dtype=torch.int64, device=dev)
    m = int(tri_index.numel())
    if m == 0:
        empty = torch.empty((0,), dtype=torch.int64, device=dev)
        return {"mesh": _part(mesh, empty, torch.empty((0, 3), dtype=torch.int32, device=dev)), "vertex_index": _i32(0, dev)}
    lib = _lib.load()
    used, flag = _i32(nv, dev), _flag(dev)
    check(lib.sgam_mesh_mark_vertices_i32(_p(mesh.triangles), nt, nv, _p(keep.contiguous().view(torch.uint8)), _p(used), _p(flag), _stream()),
          "sgam_mesh_mark_vertices_i32")
    vertex_index = torch.nonzero(used).reshape(-1)
    vertex_map = (torch.cumsum(used, 0) - 1).to(torch.int32)
    out = torch.empty((m, 3), dtype=torch.int32, device=dev)
    check(lib.sgam_mesh_remap_triangles_i32(_p(mesh.triangles), nt, _p(tri_index.to(torch.int32)), m, _p(vertex_map), nv, _p(out), _p(flag),
                                            _stream()), "sgam_mesh_remap_triangles_i32")
    _check_flag(flag, "select_triangles")
    return {"mesh": _part(mesh, vertex_index, out), "vertex_index": vertex_index.to(torch.int32)}


def _count_arg(v, name):
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f"{name} is a non-negative integer or None, not {v!r}")
    return int(v)


def remove_small_components(mesh, min_triangles=None, keep_largest=None):
    """Keeps the components with n_triangles >= min_triangles and / or the keep_largest components with the most triangles (ties
    go to the lower label); both given: the intersection.  -> select_triangles' dict"""
    min_triangles, keep_largest = _count_arg(min_triangles, "min_triangles"), _count_arg(keep_largest, "keep_largest")
    nv, nt = _sizes(mesh, "remove_small_components")
    dev = mesh.vertices.device
    if nt == 0:
        return select_triangles(mesh, torch.zeros((0,), dtype=torch.bool, device=dev))
    comp = components(mesh)
    labels, n = comp["labels"].long(), comp["n_triangles"]
    ok = torch.ones_like(n, dtype=torch.bool)
    if min_triangles is not None:
        ok &= n >= min_triangles
    if keep_largest is not None:
        order = torch.sort(n, descending=True, stable=True).indices[:keep_largest]       # labels ascend: a tie goes to the lower one
        top = torch.zeros_like(ok)
        top[order] = True
        ok &= top
    kept = torch.zeros((nv,), dtype=torch.bool, device=dev)
    kept[labels[ok]] = True
    return select_triangles(mesh, kept[comp["triangle_label"].long()])


def incidence(mesh, kind):
    """CSR {"offsets" (nv+1,) int32, "items" int32}: kind "triangles": the ids of the triangles using each vertex, ascending, each
    once; "vertices": the distinct other vertices sharing a triangle with it, ascending.  No cap on the degree: count, scan, fill
    through an atomic cursor, then one lane per vertex sorts its own segment (sgam_mesh_incidence_count_i32 / _fill_i32)."""
    if kind not in KINDS:
        raise ValueError(f"incidence: kind 'triangles' or 'vertices', not {kind!r}")
    nv, nt = _sizes(mesh, "incidence")
    dev = mesh.vertices.device
    zero = {"offsets": torch.zeros((nv + 1,), dtype=torch.int32, device=dev), "items": _i32(0, dev)}
    if nt == 0:
        return zero
    lib = _lib.load()
    count, flag = _i32(nv, dev), _flag(dev)
    check(lib.sgam_mesh_incidence_count_i32(_p(mesh.triangles), nt, nv, KINDS[kind], _p(count), _p(flag), _stream()),
          "sgam_mesh_incidence_count_i32")
    raw_offsets, n_raw = _scan(count)
    _check_flag(flag, "sgam_mesh_incidence_count_i32")
    if n_raw == 0:
        return zero
    items, degree = _i32(n_raw, dev), _i32(nv, dev)
    check(lib.sgam_mesh_incidence_fill_i32(_p(mesh.triangles), nt, nv, KINDS[kind], _p(raw_offsets), n_raw, _p(items), _p(degree), _p(flag),
                                           _stream()), "sgam_mesh_incidence_fill_i32")
    if kind == "triangles":                                                # nothing repeats: the raw CSR is the result
        _check_flag(flag, "sgam_mesh_incidence_fill_i32")
        return {"offsets": raw_offsets, "items": items}
    offsets, _ = _scan(degree)
    _check_flag(flag, "sgam_mesh_incidence_fill_i32")
    return {"offsets": offsets, "items": items[items >= 0]}                # compaction: plumbing (keeps the order)


def _csr_args(csr):
    items = csr["items"]
    n = int(items.numel())
    return _p(csr["offsets"]), _p(items if n else _i32(1, items.device)), n


def vertex_normals(mesh):
    """(nv,3) fp32: per vertex the float64 sum, in ascending triangle id, of the unnormalised (v1 - v0) x (v2 - v0) of its triangles,
    normalised in float64 (a zero sum: the zero vector), rounded to fp32 once — tsdf.vertex_normals' rule with the order pinned"""
    nv, nt = _sizes(mesh, "vertex_normals")
    dev = mesh.vertices.device
    if nv == 0 or nt == 0:
        return torch.zeros((nv, 3), dtype=torch.float32, device=dev)
    csr = incidence(mesh, "triangles")
    out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    check(_lib.load().sgam_mesh_vertex_normals_f32(_p(mesh.vertices), nv, _p(mesh.triangles), nt, *_csr_args(csr), _p(out), _stream()),
          "sgam_mesh_vertex_normals_f32")
    return out


def smooth_taubin(mesh, iterations=10, lambda_filter=0.5, mu=-0.53):
    """Taubin smoothing: each iteration a step with weight lambda_filter, then one with weight mu; a step is p' = fp32(p + w (mean -
    p)) in float64 from the previous step's fp32 positions, mean over the vertex's neighbours (incidence "vertices", ascending); a
    vertex without neighbours stays.  Triangles and colours are unchanged.  -> DeviceMesh"""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError(f"smooth_taubin: iterations is a non-negative integer, not {iterations!r}")
    lam, mu = float(lambda_filter), float(mu)
    if not (np.isfinite(lam) and np.isfinite(mu)):
        raise ValueError("smooth_taubin: lambda_filter and mu are finite")
    nv, nt = _sizes(mesh, "smooth_taubin")
    a = mesh.vertices[:nv].clone()
    col = None if mesh.vertex_colors is None else mesh.vertex_colors[:nv].clone()
    tri = mesh.triangles[:nt].clone()
    if nt and iterations:
        csr = incidence(mesh, "vertices")
        args = _csr_args(csr)
        b = torch.empty_like(a)
        lib = _lib.load()
        for _ in range(int(iterations)):
            check(lib.sgam_mesh_smooth_step_f32(_p(a), _p(b), nv, *args, lam, _stream()), "sgam_mesh_smooth_step_f32")
            check(lib.sgam_mesh_smooth_step_f32(_p(b), _p(a), nv, *args, mu, _stream()), "sgam_mesh_smooth_step_f32")
    return make_mesh(a, tri, col)


def simplify_vertex_clustering(mesh, voxel_size, origin=None):
    """Vertex clustering on geometry.voxel_sample's voxel grid (origin: 3 floats, default the fp32 minimum corner of the vertices;
    voxel_grid_for's limits).  Contraction rule: a cluster's new vertex is its representative under that rule — the member of least
    (d2 to the voxel centre as bits, index), a real vertex with its colour, not an average.  New vertices are numbered in ascending
    old index.  A triangle with two corners in one cluster is dropped; of the triangles whose new triples are equal after rotating
    the least index to the front (orientation kept) the one with the lowest old index survives; survivors stay in old order.
    -> {"mesh": DeviceMesh, "vertex_index" (new -> old) int32}"""
    nv, nt = _sizes(mesh, "simplify_vertex_clustering")
    dev = mesh.vertices.device
    geometry.positive_edge("voxel_size", voxel_size)
    empty_t = torch.empty((0, 3), dtype=torch.int32, device=dev)
    if nv == 0:
        return {"mesh": _part(mesh, torch.empty((0,), dtype=torch.int64, device=dev), empty_t), "vertex_index": _i32(0, dev)}
    pts = mesh.vertices[:nv]
    box, n_valid = geometry.valid_box(pts)
    if n_valid == 0:
        return {"mesh": _part(mesh, torch.empty((0,), dtype=torch.int64, device=dev), empty_t), "vertex_index": _i32(0, dev)}
    o, h = geometry.voxel_grid_for(box[0], box[1], voxel_size, origin)
    lib = _lib.load()
    ws, nbytes = geometry.workspace("sgam_points_voxel_workspace_bytes", dev, nv)
    keep = torch.empty((nv,), dtype=torch.uint8, device=dev)
    count, rep, flag = _i32(nv, dev), _i32(nv, dev), _flag(dev)
    check(lib.sgam_points_voxel_assign_f32(_p(pts), nv, float(o[0]), float(o[1]), float(o[2]), h, _p(ws), nbytes, _p(keep), _p(count), _p(rep),
                                           _p(flag), _stream()), "sgam_points_voxel_assign_f32")
    vertex_index = torch.nonzero(keep).reshape(-1)                         # the representatives, ascending
    new_of_old = torch.cumsum(keep, 0, dtype=torch.int64) - 1
    cluster_of = torch.where(rep >= 0, new_of_old[rep.clamp(min=0).long()], torch.full_like(new_of_old, -1)).to(torch.int32)
    geometry.check_voxel_overflow(flag, "sgam_points_voxel_assign_f32")
    tri = empty_t
    if nt:
        ws, nbytes = geometry.workspace("sgam_mesh_dedup_workspace_bytes", dev, nt)
        tri_new = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        tkeep = torch.empty((nt,), dtype=torch.uint8, device=dev)
        check(lib.sgam_mesh_cluster_triangles_i32(_p(mesh.triangles), nt, _p(cluster_of), nv, _p(ws), nbytes, _p(tri_new), _p(tkeep), _p(flag),
                                                  _stream()), "sgam_mesh_cluster_triangles_i32")
        tri = tri_new[torch.nonzero(tkeep).reshape(-1)]
        _check_flag(flag, "sgam_mesh_cluster_triangles_i32")
    return {"mesh": _part(mesh, vertex_index, tri), "vertex_index": vertex_index.to(torch.int32)}


SIMPLIFY_KEYS = ("target_triangles", "target_ratio", "max_error", "boundary_weight", "oversample", "max_rounds")


def _f32_at_most(x):
    """the largest fp32 <= x (x >= 0; +inf: the largest finite one)"""
    top = float(np.finfo(np.float32).max)
    c = np.float32(min(float(x), top))
    return float(c if float(c) <= float(x) else np.nextafter(c, np.float32(-np.inf)))


# scripts/mesh_decimation_time.py sets this to a dict: seconds per phase of simplify_quadric_decimation's rounds, each phase closed
# by a synchronisation (None: no synchronisation is added)
ROUND_SECONDS = None


def _lap(name, since):
    if ROUND_SECONDS is None:
        return since
    torch.cuda.synchronize()
    now = time.perf_counter()
    ROUND_SECONDS[name] = ROUND_SECONDS.get(name, 0.0) + now - since
    return now


def _number(v, name):
    """a real number as a float (NaN included: every range test fails on it)"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"simplify_quadric_decimation: {name} is a number, not {v!r}")
    return float(v)


def _copy_of(mesh, nv, nt):
    return make_mesh(mesh.vertices[:nv].clone(), mesh.triangles[:nt].clone(), None if mesh.vertex_colors is None else mesh.vertex_colors[:nv].clone())


def simplify_quadric_decimation(mesh, target_triangles=None, target_ratio=None, max_error=math.inf, boundary_weight=1.0, oversample=2.0,
                                max_rounds=256):
    """Quadric-error decimation (Garland-Heckbert, Open3D's simplify_quadric_decimation as recalled, unpinned) by edge collapses in
    parallel rounds (csrc/mesh_simplify.hip; the rules in full: include/sgam_hip.h; tests/decimation_oracle.py
    restates them).  Exactly one of target_triangles (an integer >= 0) and target_ratio (0 < r <= 1: target = floor(r nt)).
    -> {"mesh": DeviceMesh, "vertex_index" (nv',) int32: the input vertex whose slot the output vertex descends from, "rounds",
    "max_cost": the largest fp32 cost applied, "stopped": "target" | "no_candidates" | "max_rounds"}.  All arithmetic is fp64 from
    the widened fp32 inputs in a fixed order, a position is rounded to fp32 once; equal bits run to run.
    1. Vertex quadrics, once: per vertex, in ascending triangle id, A [n; d][n; d]^T of its triangles with area (unit normal n, d =
       -n.v0, area A), then boundary_weight A times the plane through every edge of it that exactly one triangle uses,
       perpendicular to that triangle.  They are summed along the collapses.
    2. A round works on the current compacted mesh and its rebuilt incidence; an edge is a "vertices" entry with item > owner, its
       id the rank among those.
    3. Per edge (lo, hi), Q = Q_lo + Q_hi: when |det A| > 1e-8 (tr A / 3)^3 (a RELATIVE test, unlike Open3D's) the target is
       -A^-1 b by Cramer's rule, kept when |target - mid|^2 <= 4 |hi - lo|^2; else whichever of lo, hi, mid costs least (ties in
       that order).  cost = fp32(max(v^T Q v, 0)); the new colour is interpolated at the clamped projection onto the segment.
    4. Legal: every triangle with exactly one of the ends keeps dot(n_before, n_after) > 0 (so a triangle without area next to the
       edge refuses it); lo and hi have as many common neighbours as triangles on the edge, and no triangle of lo turns, with hi in
       lo's place, into the corner set of a triangle of hi, and an edge inside the surface does not join two vertices of its
       border (the link condition; Open3D does not test it).
    5. tau = the ceil(oversample need)-th smallest legal cost, need = ceil((nt - target) / 2), capped by max_error; candidates are
       the legal edges with cost <= tau.
    6. priority = a 32-bit bijective scramble of the edge id; p1[v] = the least priority of v's candidate edges, p2[v] = the least
       p1 of v and its neighbours; an edge is selected iff its priority = p2[lo] = p2[hi]: no vertex of a selected edge neighbours
       a vertex of another.
    7. When every selected edge would take nt below the target they are applied in ascending (cost bits, priority) while the
       running count is > target.
    8. lo survives with the target position, colour and Q; hi and the triangles with both ends go; the order is kept.
    An empty mesh or a target >= nt returns a copy without a launch."""
    if (target_triangles is None) == (target_ratio is None):
        raise ValueError("simplify_quadric_decimation: exactly one of target_triangles and target_ratio")
    if target_triangles is not None:
        target_triangles = _count_arg(target_triangles, "simplify_quadric_decimation: target_triangles")
    elif not 0 < _number(target_ratio, "target_ratio") <= 1:
        raise ValueError(f"simplify_quadric_decimation: 0 < target_ratio <= 1, not {target_ratio!r}")
    if not _number(max_error, "max_error") >= 0:
        raise ValueError(f"simplify_quadric_decimation: max_error >= 0 (+inf: no cap), not {max_error!r}")
    if not 0 <= _number(boundary_weight, "boundary_weight") < math.inf:
        raise ValueError(f"simplify_quadric_decimation: boundary_weight is finite and >= 0, not {boundary_weight!r}")
    if not 0 < _number(oversample, "oversample") < math.inf:
        raise ValueError(f"simplify_quadric_decimation: oversample is finite and > 0, not {oversample!r}")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1:
        raise ValueError(f"simplify_quadric_decimation: max_rounds is a positive integer, not {max_rounds!r}")
    nv, nt = _sizes(mesh, "simplify_quadric_decimation")
    dev = mesh.vertices.device
    target = target_triangles if target_triangles is not None else int(math.floor(float(target_ratio) * nt))
    cur = _copy_of(mesh, nv, nt)
    index = torch.arange(nv, dtype=torch.int32, device=dev)
    out = {"mesh": cur, "vertex_index": index, "rounds": 0, "max_cost": 0.0, "stopped": "target"}
    if nt <= target:
        return out
    lib = _lib.load()
    cap, flag = _f32_at_most(max_error), _flag(dev)
    quadrics = torch.empty((nv, 10), dtype=torch.float64, device=dev)
    check(lib.sgam_mesh_quadric_init_f64(_p(cur.vertices), nv, _p(cur.triangles), nt, *_csr_args(incidence(cur, "triangles")), float(boundary_weight),
                                         _p(quadrics), _p(flag), _stream()), "sgam_mesh_quadric_init_f64")
    rounds, max_cost = 0, 0.0
    while True:
        nv, nt = cur.n_vertices, cur.n_triangles
        if nt <= target or rounds == max_rounds:
            stopped = "target" if nt <= target else "max_rounds"
            break
        lap = _lap("other", time.perf_counter())
        by_tri, by_vert = incidence(cur, "triangles"), incidence(cur, "vertices")
        lap = _lap("incidence", lap)
        degree = (by_vert["offsets"][1:] - by_vert["offsets"][:-1]).long()
        owner = torch.repeat_interleave(torch.arange(nv, dtype=torch.int32, device=dev), degree)   # edges: integer plumbing, like the scans
        up = by_vert["items"] > owner
        edge_of_entry = torch.where(up, torch.cumsum(up, 0) - 1, -1).to(torch.int32)
        edges = torch.stack([owner[up], by_vert["items"][up]], 1).contiguous()
        ne = int(edges.shape[0])
        lap = _lap("edge list", lap)
        if ne == 0:
            stopped = "no_candidates"
            break
        col = cur.vertex_colors
        cost, removed = torch.empty((ne,), dtype=torch.float32, device=dev), _i32(ne, dev)
        position = torch.empty((ne, 3), dtype=torch.float32, device=dev)
        color = None if col is None else torch.empty((ne, 3), dtype=torch.float32, device=dev)
        check(lib.sgam_mesh_collapse_evaluate_f64(_p(cur.vertices), _p(col), nv, _p(cur.triangles), nt, _p(quadrics), *_csr_args(by_tri),
                                                  *_csr_args(by_vert), _p(edges), ne, _p(cost), _p(removed), _p(position), _p(color), _p(flag),
                                                  _stream()), "sgam_mesh_collapse_evaluate_f64")
        lap = _lap("edge kernel", lap)
        legal = torch.sort(cost[cost <= np.finfo(np.float32).max]).values                     # the k-th value: plumbing; synchronises
        if legal.numel() == 0:
            stopped = "no_candidates"
            break
        k = max(int(math.ceil(float(oversample) * ((nt - target + 1) // 2))), 1)
        tau = min(float(legal[min(k, int(legal.numel())) - 1].item()), cap)
        lap = _lap("threshold", lap)
        ws, nbytes = geometry.workspace("sgam_mesh_collapse_workspace_bytes", dev, nv)
        key = torch.empty((ne,), dtype=torch.int64, device=dev)
        check(lib.sgam_mesh_collapse_select_i32(nv, *_csr_args(by_vert), _p(edge_of_entry), _p(edges), _p(cost), ne, tau, _p(ws), nbytes, _p(key),
                                                _p(flag), _stream()), "sgam_mesh_collapse_select_i32")
        chosen = torch.nonzero(key >= 0).reshape(-1)
        if chosen.numel() == 0:
            stopped = "no_candidates"
            break
        taken = removed[chosen].long()
        if nt - int(taken.sum().item()) < target:                              # the budget prefix in ascending (cost bits, priority)
            order = torch.sort(key[chosen]).indices
            before = nt - (torch.cumsum(taken[order], 0) - taken[order])
            chosen = torch.sort(chosen[order[before > target]]).values
        m, chosen32 = int(chosen.numel()), chosen.to(torch.int32)
        lap = _lap("selection and budget", lap)
        merge = torch.arange(nv, dtype=torch.int32, device=dev)
        vertex_keep, triangle_keep = torch.ones((nv,), dtype=torch.int32, device=dev), torch.ones((nt,), dtype=torch.int32, device=dev)
        check(lib.sgam_mesh_collapse_apply_f64(_p(cur.vertices), _p(col), _p(quadrics), nv, _p(cur.triangles), nt, *_csr_args(by_tri), _p(edges),
                                               _p(position), _p(color), ne, _p(chosen32), m, _p(merge), _p(vertex_keep),
                                               _p(triangle_keep), _p(flag), _stream()), "sgam_mesh_collapse_apply_f64")
        rounds += 1
        max_cost = max(max_cost, float(cost[chosen].max().item()))
        kept = torch.nonzero(vertex_keep).reshape(-1)                          # compaction: plumbing (keeps the order)
        vertex_map = (torch.cumsum(vertex_keep, 0) - 1)[merge.long()].to(torch.int32)
        tri_index = torch.nonzero(triangle_keep).reshape(-1)
        n_left = int(tri_index.numel())
        tri = torch.empty((n_left, 3), dtype=torch.int32, device=dev)
        tri_index = tri_index.to(torch.int32)
        if n_left:
            check(lib.sgam_mesh_remap_triangles_i32(_p(cur.triangles), nt, _p(tri_index), n_left, _p(vertex_map), nv, _p(tri),
                                                    _p(flag), _stream()), "sgam_mesh_remap_triangles_i32")
        _check_flag(flag, "simplify_quadric_decimation")
        cur, quadrics, index = _part(cur, kept, tri), quadrics[kept].contiguous(), index[kept]
        _lap("apply and compaction", lap)
    _check_flag(flag, "simplify_quadric_decimation")
    return {"mesh": cur, "vertex_index": index, "rounds": rounds, "max_cost": max_cost, "stopped": stopped}


CLEAN_KEYS = ("min_triangles", "keep_largest", "smooth_iterations", "voxel_size", "normals")


def clean(mesh, min_triangles=None, keep_largest=None, smooth_iterations=0, voxel_size=None, normals=True):
    """remove_small_components (when min_triangles or keep_largest is given) -> smooth_taubin(smooth_iterations) ->
    simplify_vertex_clustering(voxel_size) (when given) -> vertex_normals (when asked).  -> {"mesh": DeviceMesh, "vertex_normals":
    (nv,3) fp32 or None, "vertex_index": (nv,) int32 into the input's vertices}"""
    nv, nt = _sizes(mesh, "clean")
    dev = mesh.vertices.device
    index = torch.arange(nv, dtype=torch.int32, device=dev)
    given = mesh
    if (min_triangles is not None or keep_largest is not None) and nt:
        r = remove_small_components(mesh, min_triangles, keep_largest)
        mesh, index = r["mesh"], index[r["vertex_index"].long()]
    if smooth_iterations and mesh.n_triangles:
        mesh = smooth_taubin(mesh, smooth_iterations)
    if voxel_size is not None and mesh.n_vertices:
        r = simplify_vertex_clustering(mesh, voxel_size)
        mesh, index = r["mesh"], index[r["vertex_index"].long()]
    if mesh is given:                                                      # nothing ran: still a new, exactly sized mesh
        mesh = make_mesh(mesh.vertices[:nv].clone(), mesh.triangles[:nt].clone(),
                         None if mesh.vertex_colors is None else mesh.vertex_colors[:nv].clone())
    return {"mesh": mesh, "vertex_normals": vertex_normals(mesh) if normals else None, "vertex_index": index}


# ---------------------------------------------------------------- queries against a mesh (csrc/mesh_query.hip)
# triangle count from which point_mesh_distance(method="auto") builds a grid: the measured crossover of the two kernels with as
# many queries as triangles (scripts/mesh_distance_time.py, table in DESIGN §4.4.8: brute force wins up to 210 triangles, the two
# tie at 384, the grid, build included, wins from 484 on)
AUTO_GRID_MIN_TRIANGLES = 512
# the cell edge grows while a candidate triangle is entered into more cells than this on average: at the default edge (at least
# the mean longest bounding-box edge) a typical triangle touches at most 8 cells, so 16 is only reached by a caller's small cell_size
GRID_MAX_ENTRIES_PER_TRIANGLE = 16.0


def _area2(mesh, nv, nt, what):
    """(nt,) fp32 twice-the-areas (0: not a triangle); raises on a vertex index outside the mesh; synchronises"""
    a2, flag = torch.empty((nt,), dtype=torch.float32, device=mesh.vertices.device), _flag(mesh.vertices.device)
    check(_lib.load().sgam_mesh_triangle_area2_f32(_p(mesh.vertices), nv, _p(mesh.triangles), nt, _p(a2), _p(flag), _stream()),
          "sgam_mesh_triangle_area2_f32")
    _check_flag(flag, what)
    return a2


def triangle_areas(mesh):
    """(nt,) fp32: the area of every triangle, half of A2 = sqrt((nx * nx + ny * ny) + nz * nz) in fp32, n = ab x ac; 0 for a
    triangle that is not one (a vertex that is not finite, no area)"""
    nv, nt = _sizes(mesh, "triangle_areas")
    if nt == 0:
        return torch.empty((0,), dtype=torch.float32, device=mesh.vertices.device)
    return _area2(mesh, nv, nt, "triangle_areas") * 0.5


def sample_points(mesh, n, seed=0, colors=True, normals=False):
    """n points drawn uniformly by area from the mesh's surface (sgam_mesh_sample_f32) -> {"points" (n,3) fp32, "triangle" (n,) int32,
    "colors" (n,3) fp32 (None without vertex colours or with colors=False), "normals" (n,3) fp32: the triangle's unit normal, only
    with normals=True}.  Integer weights w[t] = floor(double(A2[t]) / double(max A2) * 2^32), their inclusive int64 sums (torch
    plumbing) and one Philox4x32-10 draw per sample: sample i is a pure function of (mesh, seed, i) — equal run to run, and the
    first n samples are a prefix of any longer draw.  A mesh without area raises ValueError when n > 0."""
    nv, nt = _sizes(mesh, "sample_points")
    n = _count_arg(n, "sample_points: n")
    if n is None or n >= 2 ** 31:
        raise ValueError(f"sample_points: n is an integer in 0..2^31-1, not {n!r}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    dev = mesh.vertices.device
    col = mesh.vertex_colors if colors else None
    out = {"points": torch.empty((n, 3), dtype=torch.float32, device=dev), "triangle": _i32(n, dev),
           "colors": None if col is None else torch.empty((n, 3), dtype=torch.float32, device=dev)}
    if normals:
        out["normals"] = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if nt == 0:
        raise ValueError("sample_points: the mesh has no triangles")
    a2 = _area2(mesh, nv, nt, "sample_points").double()
    top = float(a2.max().item())
    if not (top > 0 and math.isfinite(top)):
        raise ValueError("sample_points: the mesh has no area" if top == 0 else "sample_points: a triangle's area overflows fp32")
    cdf = torch.cumsum(torch.floor(a2 / top * 4294967296.0).to(torch.int64), 0)
    flag = _flag(dev)
    check(_lib.load().sgam_mesh_sample_f32(_p(mesh.vertices), _p(col), nv, _p(mesh.triangles), nt, _p(cdf), seed, n, _p(out["points"]),
                                           _p(out["triangle"]), _p(out["colors"]), _p(out.get("normals")), _p(flag), _stream()),
          "sgam_mesh_sample_f32")
    _check_flag(flag, "sgam_mesh_sample_f32")
    return out


def _queries(points, mesh, what):
    _need_cuda(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{what}: the queries are an (N,3) fp32 cloud, not {tuple(points.shape)} {points.dtype}")
    if points.device != mesh.vertices.device:
        raise ValueError(f"{what}: the queries and the mesh live on one device")
    return points.contiguous()


def _no_answers(out):
    out["d2"].fill_(math.inf)
    out["triangle"].fill_(-1)
    if "closest" in out:
        out["closest"].fill_(math.nan)
    return out


class TriangleGrid:
    """the candidate triangles of one mesh entered into a uniform grid (sgam_mesh_grid_count + sgam_mesh_grid_build); query() as
    often as needed.  cell_size defaults to the larger of geometry.default_cell_size(box of the candidates' vertices, candidates)
    and the mean longest bounding-box edge of the candidates, so a typical triangle touches at most eight cells; whatever it is,
    it grows by a quarter while the entries exceed int32 offsets or max_entries_per_triangle entries per candidate on average
    (geometry.grid_for's loop).  The result never depends on it."""

    def __init__(self, mesh, cell_size=None, max_entries_per_triangle=GRID_MAX_ENTRIES_PER_TRIANGLE):
        self.nv, self.nt = _sizes(mesh, "TriangleGrid")
        if not float(max_entries_per_triangle) >= 1:
            raise ValueError(f"TriangleGrid: max_entries_per_triangle is at least 1, not {max_entries_per_triangle!r}")
        if cell_size is not None:
            geometry.positive_edge("cell_size", cell_size)
        self.mesh, self.device = mesh, mesh.vertices.device
        self.n_entries = self.n_candidates = 0
        self.guard = 0.0
        self._flag = None
        if self.nt == 0:
            return
        cand = torch.nonzero(_area2(mesh, self.nv, self.nt, "TriangleGrid") > 0).reshape(-1)
        if cand.numel() == 0:
            return
        corners = mesh.vertices[mesh.triangles[cand].long()]                # (n,3,3): torch plumbing, like geometry.valid_box
        self.guard = _guard_of(corners)
        lo, hi = corners.amin(1), corners.amax(1)
        box = torch.stack([lo.amin(0), hi.amax(0)]).cpu().numpy()
        longest = float((hi - lo).amax(1).double().mean().item())
        h = max(geometry.default_cell_size(box[0], box[1], int(cand.numel())), longest) if cell_size is None else cell_size
        lib = _lib.load()
        triangles = (_p(mesh.vertices), self.nv, _p(mesh.triangles), self.nt)
        totals, flag = torch.zeros((2,), dtype=torch.int64, device=self.device), _flag(self.device)
        while True:
            self.origin, self.cell_size, self.dims = geometry.grid_for(box[0], box[1], int(cand.numel()), h)
            self._grid = (*(float(o) for o in self.origin), self.cell_size, *self.dims)     # the library's grid arguments
            check(lib.sgam_mesh_grid_count(*triangles, *self._grid, _p(totals), _p(flag), _stream()), "sgam_mesh_grid_count")
            entries, candidates = (int(v) for v in totals.cpu().tolist())   # one synchronisation, like _scan
            if entries < 2 ** 31 and entries <= float(max_entries_per_triangle) * candidates:
                break
            h = float(np.float32(self.cell_size * 1.25))
        _check_flag(flag, "sgam_mesh_grid_count")
        if entries == 0:
            return
        self.workspace, self.bytes = geometry.workspace("sgam_mesh_grid_workspace_bytes", self.device, entries, *self.dims)
        self._tables = (_p(self.workspace), self.bytes)
        check(lib.sgam_mesh_grid_build(*triangles, *self._grid, entries, *self._tables, _p(flag), _stream()), "sgam_mesh_grid_build")
        self.n_entries, self.n_candidates, self._flag = entries, candidates, flag

    def query(self, points, max_distance=None, closest=False):
        """points (Nq,3) fp32 on the grid's device -> point_mesh_distance's dict (sgam_mesh_distance_grid_f32)"""
        q = _queries(points, self.mesh, "TriangleGrid.query")
        m2 = geometry.max_d2_of(max_distance)
        nq = int(q.shape[0])
        out = geometry.answers((nq,), self.device, "triangle", closest)
        if nq == 0 or self.n_entries == 0:
            return _no_answers(out)
        if self._flag is not None:                                          # the build's flag, read once (the first query synchronises)
            _check_flag(self._flag, "sgam_mesh_grid_build")
            self._flag = None
        check(_lib.load().sgam_mesh_distance_grid_f32(_p(q), nq, self.n_entries, *self._grid, *self._tables, m2, _p(out["d2"]),
                                                      _p(out["triangle"]), _p(out.get("closest")), _stream()), "sgam_mesh_distance_grid_f32")
        return out

    def _ready(self):
        if self._flag is not None:                                          # the build's flag, read once (the first query synchronises)
            _check_flag(self._flag, "sgam_mesh_grid_build")
            self._flag = None

    def _cast(self, rays, mode, tnear, tfar, uv, normals, what):
        r, shape = _rays(rays, self.mesh, what)
        tnear, tfar = _window(tnear, tfar, what)
        n = int(r.shape[0])
        out = _ray_answers(n, self.device, mode, uv, normals)
        if n == 0 or self.n_entries == 0:
            return _shaped(_no_hits(out), shape)
        self._ready()
        flag = _flag(self.device)
        check(_lib.load().sgam_mesh_raycast_grid_f32(_p(r), n, self.n_entries, *self._grid, *self._tables, mode, tnear, tfar, self.guard,
                                                     _p(out.get("t")), _p(out.get("triangle")), _p(out.get("uv")), _p(out.get("normal")),
                                                     _p(out.get("hit")), _p(flag), _stream()), "sgam_mesh_raycast_grid_f32")
        _check_flag(flag, "sgam_mesh_raycast_grid_f32")
        return _shaped(out, shape)

    def cast_rays(self, rays, tnear=0.0, tfar=math.inf, uv=False, normals=False):
        """rays (...,6) fp32 on the grid's device -> cast_rays' dict (sgam_mesh_raycast_grid_f32)"""
        return self._cast(rays, RAY_NEAREST, tnear, tfar, uv, normals, "TriangleGrid.cast_rays")

    def test_occlusions(self, rays, tnear=0.0, tfar=math.inf):
        """rays (...,6) fp32 -> (...) bool: some triangle is hit inside [tnear, tfar]"""
        return self._cast(rays, RAY_ANY, tnear, tfar, False, False, "TriangleGrid.test_occlusions")["hit"].bool()

    def visible_points(self, points, poses_w2c, K, H, W, z_near, z_far, tolerance=1e-3):
        """visible_points' dict through this grid (sgam_mesh_visibility_grid_f32)"""
        q, poses, cam = _visibility_args(points, self.mesh, poses_w2c, K, H, W, z_near, z_far, tolerance, "TriangleGrid.visible_points")
        n = int(q.shape[0])
        count = torch.zeros((n,), dtype=torch.int32, device=self.device)
        if n and self.n_entries == 0:                                       # nothing occludes: the frustum alone decides
            return visible_points(q, self.mesh, poses, K, H, W, z_near, z_far, tolerance, method="brute")
        if n:
            self._ready()
            flag = _flag(self.device)
            check(_lib.load().sgam_mesh_visibility_grid_f32(_p(q), n, _p(poses), int(poses.shape[0]), *cam, self.guard, self.n_entries, *self._grid,
                                                            *self._tables, _p(count), _p(flag), _stream()), "sgam_mesh_visibility_grid_f32")
            _check_flag(flag, "sgam_mesh_visibility_grid_f32")
        return {"visible": count > 0, "count": count}


class TriangleBVH:
    """the candidate triangles of one mesh in a bounding-volume hierarchy built on the device (sgam_mesh_bvh_keys, torch.sort of the
    keys, sgam_mesh_bvh_build; csrc/mesh_bvh.hip): TriangleGrid's methods with the same arguments and dicts, and
    the same bits as brute force for every input.  A triangle is one leaf whatever its size, so the cost does not depend on the
    triangles being near one scale; there is no tuning argument.  n_candidates, n_nodes (2 n - 1), guard, bytes; `height` costs one
    read-back."""

    def __init__(self, mesh):
        self.nv, self.nt = _sizes(mesh, "TriangleBVH")
        self.mesh, self.device = mesh, mesh.vertices.device
        self.n_candidates = self.n_nodes = self.bytes = 0
        self.guard = 0.0
        self._flag = None
        if self.nt == 0:
            return
        cand = torch.nonzero(_area2(mesh, self.nv, self.nt, "TriangleBVH") > 0).reshape(-1)
        if cand.numel() == 0:
            return
        corners = mesh.vertices[mesh.triangles[cand].long()]                # (n,3,3): torch plumbing, as in TriangleGrid
        self.guard = _guard_of(corners)
        self._box = tuple(float(v) for v in torch.cat([corners.amin((0, 1)), corners.amax((0, 1))]).cpu().tolist())
        lib = _lib.load()
        triangles = (_p(mesh.vertices), self.nv, _p(mesh.triangles), self.nt)
        keys = torch.empty((self.nt,), dtype=torch.int64, device=self.device)
        count, flag = torch.zeros((1,), dtype=torch.int64, device=self.device), _flag(self.device)
        check(lib.sgam_mesh_bvh_keys(*triangles, *self._box, _p(keys), _p(count), _p(flag), _stream()), "sgam_mesh_bvh_keys")
        keys = torch.sort(keys).values                                      # unique keys: the order is a pure function of them
        n = int(count.item())
        _check_flag(flag, "sgam_mesh_bvh_keys")
        if n == 0:
            return
        self.workspace, self.bytes = geometry.workspace("sgam_mesh_bvh_workspace_bytes", self.device, n)
        self._tables = (n, _p(self.workspace), self.bytes)
        check(lib.sgam_mesh_bvh_build(*triangles, _p(keys), *self._tables, _p(flag), _stream()), "sgam_mesh_bvh_build")
        self.n_candidates, self.n_nodes, self._flag = n, 2 * n - 1, flag

    def _ready(self):
        if self._flag is not None:                                          # the build's flag, read once (the first query synchronises)
            _check_flag(self._flag, "sgam_mesh_bvh_build")
            self._flag = None

    def tables(self):
        """the built tables as views of the workspace: {"records" (n,12) fp32 — nine coordinates and, as bits, the id at [3] —
        "boxes" (2n-1,6) fp32, "children" (n-1,2) int32, "height" (n-1,) int32}: the layout of include/sgam_hip.h"""
        n = self.n_candidates
        if n == 0:
            return None
        self._ready()
        raw = self.workspace.reshape(-1).view(torch.uint8)
        r16 = lambda v: (v + 15) & ~15                                      # noqa: E731
        o1 = 48 * n
        o2 = o1 + r16(24 * (2 * n - 1))
        o3 = o2 + r16(8 * max(n - 1, 1))
        return {"records": raw[:o1].view(torch.float32).reshape(n, 12), "boxes": raw[o1:o1 + 24 * (2 * n - 1)].view(torch.float32).reshape(2 * n - 1, 6),
                "children": raw[o2:o2 + 8 * (n - 1)].view(torch.int32).reshape(n - 1, 2), "height": raw[o3:o3 + 4 * (n - 1)].view(torch.int32)}

    @property
    def height(self):
        """the longest path from the root to a leaf, in edges (0: a single leaf or no tree); one read-back"""
        if self.n_candidates < 2:
            return 0
        return int(self.tables()["height"][0].item())

    def query(self, points, max_distance=None, closest=False):
        """points (Nq,3) fp32 on the tree's device -> point_mesh_distance's dict (sgam_mesh_distance_bvh_f32)"""
        q = _queries(points, self.mesh, "TriangleBVH.query")
        m2 = geometry.max_d2_of(max_distance)
        nq = int(q.shape[0])
        out = geometry.answers((nq,), self.device, "triangle", closest)
        if nq == 0 or self.n_candidates == 0:
            return _no_answers(out)
        self._ready()
        flag = _flag(self.device)
        check(_lib.load().sgam_mesh_distance_bvh_f32(_p(q), nq, self._tables[0], *self._box, *self._tables[1:], m2, _p(out["d2"]), _p(out["triangle"]),
                                                     _p(out.get("closest")), _p(flag), _stream()), "sgam_mesh_distance_bvh_f32")
        _check_flag(flag, "sgam_mesh_distance_bvh_f32")
        return out

    def _cast(self, rays, mode, tnear, tfar, uv, normals, what):
        r, shape = _rays(rays, self.mesh, what)
        tnear, tfar = _window(tnear, tfar, what)
        n = int(r.shape[0])
        out = _ray_answers(n, self.device, mode, uv, normals)
        if n == 0 or self.n_candidates == 0:
            return _shaped(_no_hits(out), shape)
        self._ready()
        flag = _flag(self.device)
        check(_lib.load().sgam_mesh_raycast_bvh_f32(_p(r), n, *self._tables, mode, tnear, tfar, self.guard, _p(out.get("t")), _p(out.get("triangle")),
                                                    _p(out.get("uv")), _p(out.get("normal")), _p(out.get("hit")), _p(flag), _stream()),
              "sgam_mesh_raycast_bvh_f32")
        _check_flag(flag, "sgam_mesh_raycast_bvh_f32")
        return _shaped(out, shape)

    def cast_rays(self, rays, tnear=0.0, tfar=math.inf, uv=False, normals=False):
        """rays (...,6) fp32 on the tree's device -> cast_rays' dict (sgam_mesh_raycast_bvh_f32)"""
        return self._cast(rays, RAY_NEAREST, tnear, tfar, uv, normals, "TriangleBVH.cast_rays")

    def test_occlusions(self, rays, tnear=0.0, tfar=math.inf):
        """rays (...,6) fp32 -> (...) bool: some triangle is hit inside [tnear, tfar]"""
        return self._cast(rays, RAY_ANY, tnear, tfar, False, False, "TriangleBVH.test_occlusions")["hit"].bool()

    def visible_points(self, points, poses_w2c, K, H, W, z_near, z_far, tolerance=1e-3):
        """visible_points' dict through this tree (sgam_mesh_visibility_bvh_f32)"""
        q, poses, cam = _visibility_args(points, self.mesh, poses_w2c, K, H, W, z_near, z_far, tolerance, "TriangleBVH.visible_points")
        n = int(q.shape[0])
        count = torch.zeros((n,), dtype=torch.int32, device=self.device)
        if n and self.n_candidates == 0:                                    # nothing occludes: the frustum alone decides
            return visible_points(q, self.mesh, poses, K, H, W, z_near, z_far, tolerance, method="brute")
        if n:
            self._ready()
            flag = _flag(self.device)
            check(_lib.load().sgam_mesh_visibility_bvh_f32(_p(q), n, _p(poses), int(poses.shape[0]), *cam, self.guard, *self._tables, _p(count),
                                                           _p(flag), _stream()), "sgam_mesh_visibility_bvh_f32")
            _check_flag(flag, "sgam_mesh_visibility_bvh_f32")
        return {"visible": count > 0, "count": count}


ACCELERATORS = {"grid": TriangleGrid, "bvh": TriangleBVH}


def _accelerator(name, what):
    """the class behind method="grid" (and behind "auto" above its threshold): "grid" or "bvh" """
    if name not in ACCELERATORS:
        raise ValueError(f"{what}: accelerator 'grid' or 'bvh', not {name!r}")
    return ACCELERATORS[name]


def _accel_of(accel, mesh, method, cell_size, what):
    """a prebuilt TriangleGrid / TriangleBVH of this same mesh, given as accel="""
    if not isinstance(accel, (TriangleGrid, TriangleBVH)) or accel.mesh is not mesh:
        raise ValueError(f"{what}: accel is a TriangleGrid or TriangleBVH built for this same mesh")
    geometry.check_method(method, what)
    if cell_size is not None:
        raise ValueError(f"{what}: cell_size belongs to the grid that is built, not to a prebuilt accel")
    return accel


def point_mesh_distance(points, mesh, method="auto", max_distance=None, cell_size=None, closest=False, accel=None):
    """The exact distance from every point to the surface of the mesh.  points (Nq,3) fp32 on the mesh's device -> {"d2" (Nq,) fp32:
    the squared distance, "triangle" (Nq,) int32: the nearest triangle, "closest" (Nq,3) fp32: the nearest point of it, with
    closest=True}.  The closest point on a triangle by its seven Voronoi regions in fp32, one IEEE operation at a time
    (include/sgam_hip.h); the winner is the triangle of least (d2 bits, index), so a query that is nearest a shared edge or vertex
    gets the lower index; a triangle with a vertex that is not finite or without area is not a triangle.  No winner — an empty
    mesh, a query that is not a point, or nothing within max_distance (d2 > fp32(max_distance)^2) — gives triangle -1, d2 +inf,
    closest NaN.  method "brute" (sgam_mesh_distance_brute_f32) / "grid" (TriangleGrid) / "auto": the grid from
    AUTO_GRID_MIN_TRIANGLES triangles on; the two give the same bits, and cell_size (grid only) changes the speed, not the result.
    A triangle that names a vertex outside the mesh raises SgamHipError.  accel: a TriangleGrid or TriangleBVH of this same mesh
    built before; it answers, whatever the method (the same bits)."""
    if accel is not None:
        return _accel_of(accel, mesh, method, cell_size, "point_mesh_distance").query(points, max_distance, closest)
    method = geometry.search_method(method, cell_size, int(mesh.n_triangles), AUTO_GRID_MIN_TRIANGLES, "point_mesh_distance")
    nv, nt = _sizes(mesh, "point_mesh_distance")
    q = _queries(points, mesh, "point_mesh_distance")
    m2 = geometry.max_d2_of(max_distance)
    nq = int(q.shape[0])
    if nq == 0 or nt == 0:
        return _no_answers(geometry.answers((nq,), q.device, "triangle", closest))
    if method == "grid":
        return TriangleGrid(mesh, cell_size).query(q, max_distance, closest)
    out, flag = geometry.answers((nq,), q.device, "triangle", closest), _flag(q.device)
    check(_lib.load().sgam_mesh_distance_brute_f32(_p(mesh.vertices), nv, _p(mesh.triangles), nt, _p(q), nq, m2, _p(out["d2"]),
                                                   _p(out["triangle"]), _p(out.get("closest")), _p(flag), _stream()),
          "sgam_mesh_distance_brute_f32")
    _check_flag(flag, "sgam_mesh_distance_brute_f32")
    return out


def _is_mesh(g, what):
    if isinstance(g, DeviceMesh):
        return True
    if isinstance(g, torch.Tensor) and g.dim() == 2 and g.shape[1] == 3 and g.dtype == torch.float32:
        return False
    raise ValueError(f"{what}: a DeviceMesh or an (N,3) fp32 cloud")


def surface_metrics(pred, ref, threshold, n_samples=None, seed=0, max_distance=None, method="auto", cull=None, accelerator="grid"):
    """geometry.cloud_metrics' numbers — the same keys — where either side may be a surface: pred and ref are each a DeviceMesh or
    an (N,3) fp32 device cloud.  accuracy / precision: the distance FROM the points of pred TO ref; completeness / recall: from the
    points of ref to pred.  A mesh on the `from` side is represented by n_samples area-uniform samples (sample_points with
    `seed`; required when either argument is a mesh), a mesh on the `to` side is its surface (point_mesh_distance), a cloud on
    the `to` side geometry.nearest_neighbors.  The sums go through geometry.reduce_d2; n_pred / n_ref count the `from` points that
    are points.  Two clouds give cloud_metrics' own numbers.  cull (a reference that is a mesh only): a callable that takes the
    reference's samples (n,3) and returns the (n,) bool mask of those to keep — e.g. visible_points' "visible" — so completeness /
    recall run over the kept samples only; n_ref counts them and the dict gains "n_ref_culled", the samples dropped.
    accelerator "grid" | "bvh": the structure behind method="grid" and behind "auto" above its threshold for a mesh on the `to`
    side (TriangleGrid or TriangleBVH); the numbers do not depend on it."""
    tree = _accelerator(accelerator, "surface_metrics")
    mp, mr = _is_mesh(pred, "surface_metrics"), _is_mesh(ref, "surface_metrics")
    if cull is not None and not mr:
        raise ValueError("surface_metrics: cull needs a reference that is a mesh (its samples are what is culled)")
    if not mp and not mr:
        return geometry.cloud_metrics(pred, ref, threshold, max_distance=max_distance, method=method)
    n = _count_arg(n_samples, "surface_metrics: n_samples")
    if not n:
        raise ValueError("surface_metrics: n_samples (a positive integer) is required when either argument is a mesh")
    geometry.check_method(method, "surface_metrics")

    def points_of(g, is_mesh):
        if not is_mesh:
            _need_cuda(g)
            return g.contiguous()
        if not g.n_triangles:
            raise ValueError("surface_metrics: a mesh without triangles has no surface")
        return sample_points(g, n, seed, colors=False)["points"]

    def distance(p, g, is_mesh):
        if is_mesh:
            if tree is TriangleBVH and g.n_triangles and p.shape[0] and \
                    geometry.search_method(method, None, int(g.n_triangles), AUTO_GRID_MIN_TRIANGLES, "surface_metrics") == "grid":
                return point_mesh_distance(p, g, method, max_distance, accel=TriangleBVH(g))["d2"]
            return point_mesh_distance(p, g, method, max_distance)["d2"]
        return geometry.nearest_neighbors(p, g, method, max_distance)["d2"]

    pp, rp = points_of(pred, mp), points_of(ref, mr)
    culled = None
    if cull is not None:
        keep = cull(rp)
        if tuple(keep.shape) != (rp.shape[0],) or keep.dtype != torch.bool:
            raise ValueError("surface_metrics: cull returns an (n,) bool mask of the reference's samples")
        culled = int(rp.shape[0]) - int(keep.sum().item())
        rp = rp[keep].contiguous()
    if pp.shape[0] < 1 or rp.shape[0] < 1:
        raise ValueError("surface_metrics: both sides need at least one point" + (" (cull kept none of the reference's samples)" if culled else ""))
    out = geometry.metrics_from_sums(geometry.reduce_d2(distance(pp, ref, mr), threshold), geometry.reduce_d2(distance(rp, pred, mp), threshold),
                                     int(torch.isfinite(pp).all(dim=1).sum().item()), int(torch.isfinite(rp).all(dim=1).sum().item()))
    if culled is not None:
        out["n_ref_culled"] = culled
    return out


# ---------------------------------------------------------------- rays against a mesh (csrc/mesh_ray.hip)
RAY_NEAREST, RAY_ANY = 0, 1
# triangle count from which cast_rays / test_occlusions / visible_points(method="auto") build a grid: the measured crossover of the
# two kernels on 4 x 256 x 256 primary rays, grid build included (scripts/mesh_raycast_time.py, table in DESIGN §4.4.9: brute force
# wins at 142 triangles, the two tie at 292, the grid wins from 484 on; visibility ties at 712 and the grid wins from 1 940 on)
AUTO_GRID_MIN_TRIANGLES_RAYS = 512


def _guard_of(corners):
    """the guard of the intersection rule: 2^-15 of the largest |coordinate| of the candidates' corners ((n,3,3) fp32), an exact
    fp32 product; synchronises"""
    return float(np.float32(corners.abs().amax().item()) * np.float32(2.0 ** -15))


def _ray_guard(mesh, nv, nt, what):
    """the guard for a mesh without a grid; None: no candidate triangle"""
    cand = torch.nonzero(_area2(mesh, nv, nt, what) > 0).reshape(-1)
    if cand.numel() == 0:
        return None
    return _guard_of(mesh.vertices[mesh.triangles[cand].long()])


def _rays(rays, mesh, what):
    _need_cuda(rays)
    if rays.dim() < 1 or rays.shape[-1] != 6 or rays.dtype != torch.float32:
        raise ValueError(f"{what}: the rays are (...,6) fp32 (origin, direction), not {tuple(rays.shape)} {rays.dtype}")
    if rays.device != mesh.vertices.device:
        raise ValueError(f"{what}: the rays and the mesh live on one device")
    if rays.numel() // 6 >= 2 ** 31:
        raise ValueError(f"{what}: at most 2^31 - 1 rays in one call")
    return rays.contiguous().reshape(-1, 6), tuple(rays.shape[:-1])


def _window(tnear, tfar, what):
    tnear, tfar = float(np.float32(tnear)), float(np.float32(tfar))
    if not (0.0 <= tnear < math.inf and tfar >= tnear):
        raise ValueError(f"{what}: 0 <= tnear <= tfar, tnear finite, not [{tnear}, {tfar}]")
    return tnear, tfar


def _ray_answers(n, device, mode, uv, normals):
    if mode == RAY_ANY:
        return {"hit": torch.empty((n,), dtype=torch.uint8, device=device)}
    out = {"t": torch.empty((n,), dtype=torch.float32, device=device), "triangle": _i32(n, device)}
    if uv:
        out["uv"] = torch.empty((n, 2), dtype=torch.float32, device=device)
    if normals:
        out["normal"] = torch.empty((n, 3), dtype=torch.float32, device=device)
    return out


def _no_hits(out):
    for k, v in out.items():
        v.fill_({"t": math.inf, "triangle": -1, "hit": 0}.get(k, math.nan))
    return out


def _shaped(out, shape):
    return {k: v.reshape(*shape, *v.shape[1:]) for k, v in out.items()}


def _cast(rays, mesh, mode, method, tnear, tfar, cell_size, uv, normals, what, accel=None):
    if accel is not None:
        return _accel_of(accel, mesh, method, cell_size, what)._cast(rays, mode, tnear, tfar, uv, normals, what)
    method = geometry.search_method(method, cell_size, int(mesh.n_triangles), AUTO_GRID_MIN_TRIANGLES_RAYS, what)
    nv, nt = _sizes(mesh, what)
    r, shape = _rays(rays, mesh, what)
    tnear, tfar = _window(tnear, tfar, what)
    n = int(r.shape[0])
    if n == 0 or nt == 0:
        return _shaped(_no_hits(_ray_answers(n, r.device, mode, uv, normals)), shape)
    if method == "grid":
        return TriangleGrid(mesh, cell_size)._cast(r.reshape(*shape, 6), mode, tnear, tfar, uv, normals, what)
    out = _ray_answers(n, r.device, mode, uv, normals)
    guard = _ray_guard(mesh, nv, nt, what)
    if guard is None:
        return _shaped(_no_hits(out), shape)
    flag = _flag(r.device)
    check(_lib.load().sgam_mesh_raycast_brute_f32(_p(mesh.vertices), nv, _p(mesh.triangles), nt, _p(r), n, mode, tnear, tfar, guard, _p(out.get("t")),
                                                  _p(out.get("triangle")), _p(out.get("uv")), _p(out.get("normal")), _p(out.get("hit")),
                                                  _p(flag), _stream()), "sgam_mesh_raycast_brute_f32")
    _check_flag(flag, "sgam_mesh_raycast_brute_f32")
    return _shaped(out, shape)


def cast_rays(rays, mesh, method="auto", tnear=0.0, tfar=math.inf, cell_size=None, uv=False, normals=False, accel=None):
    """The nearest hit of every ray with the mesh.  rays (...,6) fp32 on the mesh's device, (origin, direction); the direction is
    not normalised, so t is in units of its length -> {"t" (...) fp32: +inf without a hit, "triangle" (...) int32: -1 without a
    hit, "uv" (...,2) fp32 with uv=True: the hit's barycentric (u, v) (the point is (1 - u - v) a + u b + v c), "normal" (...,3)
    fp32 with normals=True: the hit triangle's unit normal (ab x ac, not turned towards the ray)}; NaN without a hit.  Two-sided
    Moeller-Trumbore in fp32, one IEEE operation at a time, with a bounding-box guard of 2^-15 of the mesh's coordinate scale
    (include/sgam_hip.h); hits inside [tnear, tfar] count, 0 <= tnear; the winner is the hit of least (t bits, triangle index).
    A ray with a component that is not finite or without a direction hits nothing.  method "brute" / "grid" (TriangleGrid) /
    "auto": the grid from AUTO_GRID_MIN_TRIANGLES_RAYS triangles on; the two give the same bits and cell_size (grid only) changes
    the speed, not the result.  A triangle that names a vertex outside the mesh raises SgamHipError.  accel: a TriangleGrid or
    TriangleBVH of this same mesh built before; it answers, whatever the method (the same bits)."""
    return _cast(rays, mesh, RAY_NEAREST, method, tnear, tfar, cell_size, uv, normals, "cast_rays", accel)


def test_occlusions(rays, mesh, method="auto", tnear=0.0, tfar=math.inf, cell_size=None, accel=None):
    """(...) bool: the ray hits some triangle inside [tnear, tfar] — cast_rays' rule, left at the first hit"""
    return _cast(rays, mesh, RAY_ANY, method, tnear, tfar, cell_size, False, False, "test_occlusions", accel)["hit"].bool()


test_occlusions.__test__ = False                                           # (a public name, not a test for pytest to collect)


def _intrinsics(K, what):
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{what}: K is a 3 x 3 intrinsics matrix, not {K.shape}")
    return tuple(float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def _poses(poses_w2c, device, what):
    poses = poses_w2c if isinstance(poses_w2c, torch.Tensor) else torch.as_tensor(np.asarray(poses_w2c, dtype=np.float32))
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] < 1:
        raise ValueError(f"{what}: poses_w2c is (P,4,4) world -> camera with P >= 1, not {tuple(poses.shape)}")
    return poses.to(device=device, dtype=torch.float32).contiguous()


def create_rays_pinhole(poses_w2c, K, H, W, device="cuda"):
    """(P,H,W,6) fp32 rays of P pinhole images (sgam_rays_pinhole_f32): poses_w2c (P,4,4) world -> camera, K 3 x 3.  The origin is
    the camera centre, the direction the ray through the centre of pixel (row i, column j) in world coordinates with camera z = 1
    (not normalised), so the t of a hit is its view-space depth."""
    fx, fy, cx, cy = _intrinsics(K, "create_rays_pinhole")
    poses = _poses(poses_w2c, poses_w2c.device if isinstance(poses_w2c, torch.Tensor) else device, "create_rays_pinhole")
    _need_cuda(poses)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or poses.shape[0] * H * W >= 2 ** 31:
        raise ValueError(f"create_rays_pinhole: H, W >= 1 and P * H * W < 2^31, not {poses.shape[0]} x {H} x {W}")
    out = torch.empty((poses.shape[0], H, W, 6), dtype=torch.float32, device=poses.device)
    check(_lib.load().sgam_rays_pinhole_f32(_p(poses), int(poses.shape[0]), fx, fy, cx, cy, H, W, _p(out), _stream()), "sgam_rays_pinhole_f32")
    return out


def _visibility_args(points, mesh, poses_w2c, K, H, W, z_near, z_far, tolerance, what):
    q = _queries(points, mesh, what)
    poses = _poses(poses_w2c, q.device, what)
    fx, fy, cx, cy = _intrinsics(K, what)
    zn, zf, tol = float(np.float32(z_near)), float(np.float32(z_far)), float(np.float32(tolerance))
    if not (0 < zn <= zf < math.inf) or not 0 <= tol <= 1 or int(H) < 1 or int(W) < 1:
        raise ValueError(f"{what}: 0 < z_near <= z_far, 0 <= tolerance <= 1, H, W >= 1")
    return q, poses, (fx, fy, cx, cy, int(H), int(W), zn, zf, tol)


def visible_points(points, mesh, poses_w2c, K, H, W, z_near, z_far, tolerance=1e-3, method="auto", grid=None):
    """Which points the pinhole cameras see, with the mesh as the occluder.  points (N,3) fp32 on the mesh's device, poses_w2c
    (P,4,4) world -> camera, K 3 x 3, an H x W image -> {"visible" (N,) bool, "count" (N,) int32: the poses that see the point}.
    A pose sees a point when it lies in the frustum (z_near <= camera z <= z_far, its pixel by the point-splat view's rule inside
    the image) and the ray from the camera centre to the point hits nothing in [0, 1 - tolerance] (t = 1 is the point itself;
    the tolerance keeps a sample of the occluder's own surface from hiding itself).  The N x P rays are formed inside the kernel.
    grid: a TriangleGrid or a TriangleBVH of the mesh built before (it answers, whatever the method)."""
    if grid is not None:
        if grid.mesh is not mesh:
            raise ValueError("visible_points: the grid was built for another mesh")
        return grid.visible_points(points, poses_w2c, K, H, W, z_near, z_far, tolerance)
    method = geometry.search_method(method, None, int(mesh.n_triangles), AUTO_GRID_MIN_TRIANGLES_RAYS, "visible_points")
    nv, nt = _sizes(mesh, "visible_points")
    if method == "grid" and nt:
        return TriangleGrid(mesh).visible_points(points, poses_w2c, K, H, W, z_near, z_far, tolerance)
    q, poses, cam = _visibility_args(points, mesh, poses_w2c, K, H, W, z_near, z_far, tolerance, "visible_points")
    n = int(q.shape[0])
    count = torch.zeros((n,), dtype=torch.int32, device=q.device)
    if n:
        lib, flag = _lib.load(), _flag(q.device)
        guard = _ray_guard(mesh, nv, nt, "visible_points") if nt else None
        if guard is None:                                                   # nothing occludes: one triangle without area carries the frustum test
            v, t, nv, nt, guard = torch.zeros((1, 3), dtype=torch.float32, device=q.device), torch.zeros((1, 3), dtype=torch.int32, device=q.device), 1, 1, 0.0
        else:
            v, t = mesh.vertices, mesh.triangles
        check(lib.sgam_mesh_visibility_brute_f32(_p(v), nv, _p(t), nt, _p(q), n, _p(poses), int(poses.shape[0]), *cam, guard, _p(count), _p(flag),
                                                 _stream()), "sgam_mesh_visibility_brute_f32")
        _check_flag(flag, "sgam_mesh_visibility_brute_f32")
    return {"visible": count > 0, "count": count}
