"""CPU: the mesh clean-up kernels' numpy twin (tests/meshops_oracle.py) against outside truth — scipy's connected components, a
set-based restatement of the incidence, the analytic sphere, the host tsdf.vertex_normals, topology and area / volume through
tests/mc_oracle.py — on marching-cubes meshes and hand meshes, and the argument checks of the new entry points through ctypes.
The meshes are built here; tests/test_gpu_meshops.py runs the kernels on the same ones against the twin bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from sgam_neurips22_amd import _lib, tsdf

sys.path.insert(0, os.path.dirname(__file__))
import mc_oracle  # noqa: E402
import meshops_oracle as MO  # noqa: E402

f32 = np.float32
THREE_SPHERES = (((14.2, 15.1, 19.6), 9.3), ((31.3, 30.2, 28.9), 4.1), ((6.2, 33.3, 7.7), 2.2))
SPHERE = (((19.2, 18.7, 19.6), 14.3),)
_CACHE = {}


# ---------------------------------------------------------------- the meshes (shared with the GPU tests; never modified)
def field(n, spheres):
    """clip(min_i(|x - c_i| - r_i) / 4, -1, 1) on an n^3 lattice"""
    x = np.arange(n, dtype=np.float64)
    zz, yy, xx = np.meshgrid(x, x, x, indexing="ij")
    d = np.min([np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - r for c, r in spheres], axis=0)
    return np.clip(d / 4.0, -1.0, 1.0).astype(f32)


def mesh(name):
    """"three" (three spheres, voxel 0.1), "noise" (uniform noise, voxel 1), "sphere" (one sphere, voxel 0.1): dict(vertices,
    triangles, colors: a made-up fp32 colour per vertex, so that carrying colours is tested)"""
    if name not in _CACHE:
        if name == "three":
            m = mc_oracle.marching_cubes(field(40, THREE_SPHERES), 0.1)
        elif name == "noise":
            m = mc_oracle.marching_cubes(np.random.RandomState(5).uniform(-1, 1, (20, 20, 20)).astype(f32), 1.0)
        elif name == "sphere":
            m = mc_oracle.marching_cubes(field(40, SPHERE), 0.1)
        else:
            raise KeyError(name)
        v = m["vertices"]
        col = np.stack([np.arange(len(v)) % 256, (np.arange(len(v)) // 7) % 256, (v[:, 0] * 10) % 256], 1).astype(f32)
        for a in (v, m["triangles"], col):
            a.setflags(write=False)
        _CACHE[name] = dict(vertices=v, triangles=m["triangles"], colors=col)
    return _CACHE[name]


def noisy_sphere():
    """the sphere's float64 vertices moved radially by N(0, 0.02), cast to fp32; -> (vertices, centre, radius)"""
    m = mesh("sphere")
    c = (np.array(SPHERE[0][0]) + 0.5) * 0.1
    v = m["vertices"].astype(np.float64)
    d = v - c
    r = np.linalg.norm(d, axis=1, keepdims=True)
    v = c + d / r * (r + np.random.RandomState(1).normal(0, 0.02, (len(v), 1)))
    return v.astype(f32), c, SPHERE[0][1] * 0.1


def strip(n_tri, seed=None):
    """a strip of n_tri triangles whose vertex ids DESCEND along the strip (triangle t = (n - t, n - t - 1, n - t - 2) + 1 ...), or
    the same strip with the ids permuted by `seed`; -> (vertices, triangles)"""
    nv = n_tri + 2
    ids = np.arange(nv)[::-1].copy()
    if seed is not None:
        ids = np.random.RandomState(seed).permutation(nv)
    k = np.arange(n_tri)
    tri = np.stack([ids[k], ids[k + 1], ids[k + 2]], 1).astype(np.int32)
    pos = np.zeros((nv, 3), dtype=f32)
    pos[ids, 0] = (np.arange(nv) // 2).astype(f32) * f32(0.5)
    pos[ids, 1] = (np.arange(nv) % 2).astype(f32)
    pos[ids, 2] = np.sin(np.arange(nv) / 9.0).astype(f32)
    return pos, tri


def fan(n_tri=700):
    """n_tri triangles round one hub (vertex 3; vertices 0..2 unreferenced): the hub's raw neighbour segment has 2 n_tri entries"""
    a = np.arange(n_tri) * (2 * np.pi / n_tri)
    rim = np.stack([np.cos(a) * (1 + 0.1 * np.sin(5 * a)), np.sin(a), 0.2 * np.cos(3 * a)], 1)
    v = np.concatenate([[[9, 9, 9], [8, 8, 8], [7, 7, 7], [0.01, -0.02, 0.3]], rim]).astype(f32)
    k = np.arange(n_tri)
    tri = np.stack([np.full(n_tri, 3), 4 + k, 4 + (k + 1) % n_tri], 1).astype(np.int32)
    return v, tri[np.random.RandomState(2).permutation(n_tri)]


V6 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [2, 2, 2]], dtype=f32)
HAND = {
    "one": (V6[:3], np.array([[0, 1, 2]], dtype=np.int32)),
    "shared_vertex": (V6[:5], np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int32)),
    "disjoint": (V6[:6], np.array([[3, 4, 5], [0, 1, 2]], dtype=np.int32)),
    "aab": (V6[:4], np.array([[1, 1, 3], [0, 2, 2]], dtype=np.int32)),
    "unreferenced": (V6, np.array([[5, 1, 2], [2, 1, 4]], dtype=np.int32)),
}


def cluster_hand():
    """vertices 3, 4, 5 fall voxel by voxel onto 0, 1, 2 (voxel 1, origin 0; 0..2 sit nearer their voxel centres); 6, 7 share a
    voxel of their own.  Triangles: 0 = (0,1,2); 1 = (3,4,5), the same after clustering; 2 = (5,3,4), the same, rotated; 3 =
    (2,1,0), the reversed copy: kept; 4 = (0,6,7): two corners in one voxel"""
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.2, 0.6, 0.4], [1.7, 0.5, 0.6], [0.5, 1.9, 0.5],
                  [3.5, 3.5, 3.5], [3.6, 3.4, 3.5]], dtype=f32)
    t = np.array([[0, 1, 2], [3, 4, 5], [5, 3, 4], [2, 1, 0], [0, 6, 7]], dtype=np.int32)
    return v, t


# ---------------------------------------------------------------- helpers
def scipy_labels(tri, nv):
    t = np.asarray(tri, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv))
    _, lab = connected_components(g, directed=False)
    least = np.full(lab.max() + 1, nv, dtype=np.int64)
    np.minimum.at(least, lab, np.arange(nv))
    return least[lab]


def check_components(tri, nv):
    c = MO.components(tri, nv)
    want = scipy_labels(tri, nv)
    assert np.array_equal(c["vertex_label"], want)
    assert np.array_equal(c["triangle_label"], want[np.asarray(tri)[:, 0]])
    labels, counts = np.unique(want[np.asarray(tri)[:, 0]], return_counts=True)
    assert np.array_equal(c["labels"], labels) and np.array_equal(c["n_triangles"], counts)
    assert c["vertex_label"].dtype == c["triangle_label"].dtype == c["labels"].dtype == c["n_triangles"].dtype == np.int32
    return c


def check_incidence(tri, nv):
    tri = np.asarray(tri)
    tris_of, verts_of = [set() for _ in range(nv)], [set() for _ in range(nv)]
    for t, (a, b, c) in enumerate(tri.tolist()):
        for x in (a, b, c):
            tris_of[x].add(t)
            verts_of[x].update(y for y in (a, b, c) if y != x)
    for kind, sets in (("triangles", tris_of), ("vertices", verts_of)):
        off, items = MO.incidence(tri, nv, kind)
        assert off.dtype == items.dtype == np.int32 and off[0] == 0 and off[-1] == len(items) and len(off) == nv + 1
        assert [items[off[i]:off[i + 1]].tolist() for i in range(nv)] == [sorted(s) for s in sets]
    return np.diff(MO.incidence(tri, nv, "vertices")[0])


# ---------------------------------------------------------------- components, selection, removal
def test_three_spheres_components_and_removal():
    m = mesh("three")
    v, t = m["vertices"], m["triangles"]
    assert (len(v), len(t)) == (2026, 4040)
    c = check_components(t, len(v))
    assert sorted(c["n_triangles"].tolist(), reverse=True) == [3256, 616, 168]
    two = MO.remove_small_components(v, t, m["colors"], min_triangles=200)
    assert len(MO.components(two["triangles"], len(two["vertices"]))["labels"]) == 2 and len(two["triangles"]) == 3256 + 616
    big = MO.remove_small_components(v, t, m["colors"], keep_largest=1)
    assert len(big["triangles"]) == 3256 and mc_oracle.euler_and_edges(big["triangles"])[0] == 2
    assert np.array_equal(big["vertices"], v[big["vertex_index"]]) and np.array_equal(big["colors"], m["colors"][big["vertex_index"]])
    assert (np.diff(big["vertex_index"]) > 0).all()
    # both: the intersection; ties of keep_largest go to the lower label
    both = MO.remove_small_components(v, t, None, min_triangles=700, keep_largest=2)
    assert len(both["triangles"]) == 3256
    comp = dict(labels=np.array([2, 5, 9], np.int32), n_triangles=np.array([4, 7, 4], np.int32))
    assert MO.kept_components(comp, keep_largest=2).tolist() == [2, 5]
    assert MO.kept_components(comp, keep_largest=0).tolist() == [] and MO.kept_components(comp, min_triangles=5).tolist() == [5]


def test_noise_field_components_and_incidence():
    m = mesh("noise")
    v, t = m["vertices"], m["triangles"]
    assert (len(v), len(t)) == (11264, 21844)
    c = check_components(t, len(v))
    assert len(c["labels"]) == 79
    assert check_incidence(t, len(v)).max() == 18


def test_strips_and_fan():
    for seed in (None, 7):
        v, t = strip(3000, seed)
        c = check_components(t, len(v))
        assert len(c["labels"]) == 1 and c["labels"][0] == 0 and c["n_triangles"][0] == 3000
    v, t = fan()
    c = check_components(t, len(v))
    assert c["labels"].tolist() == [3] and c["vertex_label"][:3].tolist() == [0, 1, 2]
    deg = check_incidence(t, len(v))
    assert deg[3] == 700 and deg[:3].tolist() == [0, 0, 0] and (deg[4:] == 3).all()


# ---------------------------------------------------------------- normals
def test_normals_on_the_sphere_and_against_the_host_rule():
    m = mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    assert (len(v), len(t)) == (3844, 7684)
    deg = np.diff(MO.incidence(t, len(v), "triangles")[0])
    assert (deg.min(), deg.max()) == (4, 9)
    n = MO.vertex_normals(v, t)
    assert n.dtype == f32
    c = (np.array(SPHERE[0][0]) + 0.5) * 0.1
    radial = v.astype(np.float64) - c
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    dots = (n.astype(np.float64) * radial).sum(1)
    print(f"sphere normals: least dot product with the radial direction {dots.min():.4f}")
    assert dots.min() >= 0.99
    for name in ("sphere", "noise"):
        m = mesh(name)
        v, t = m["vertices"], m["triangles"]
        got, want = MO.vertex_normals(v, t).astype(np.float64), tsdf.vertex_normals(v, t)
        v64 = v.astype(np.float64)
        fn = np.cross(v64[t[:, 1]] - v64[t[:, 0]], v64[t[:, 2]] - v64[t[:, 0]])
        total, terms = np.zeros_like(v64), np.zeros(len(v))
        for k in range(3):
            np.add.at(total, t[:, k], fn)
            np.add.at(terms, t[:, k], np.linalg.norm(fn, axis=1))
        firm = np.linalg.norm(total, axis=1) > 1e-6 * terms
        err = np.abs(got - want.astype(f32))[firm].max()
        print(f"{name}: vertex normals against tsdf.vertex_normals on {firm.sum()} of {len(v)} vertices: max |diff| {err:.2e}")
        assert firm.mean() > 0.99 and err <= 1e-6


# ---------------------------------------------------------------- Taubin smoothing
def test_taubin_removes_noise_and_keeps_the_size():
    m = mesh("sphere")
    v, c, R = noisy_sphere()
    r0 = np.linalg.norm(v.astype(np.float64) - c, axis=1)
    out = MO.smooth_taubin(v, m["triangles"], 10)
    r1 = np.linalg.norm(out.astype(np.float64) - c, axis=1)
    print(f"taubin: radial std {r0.std():.4f} -> {r1.std():.4f}, mean radius {r0.mean():.4f} -> {r1.mean():.4f} (R = {R})")
    assert out.dtype == f32 and r1.std() <= 0.5 * r0.std() and abs(r1.mean() - r0.mean()) <= 0.002
    same = MO.smooth_taubin(v, m["triangles"], 0)
    assert np.array_equal(same.view(np.uint32), v.view(np.uint32))
    # a vertex without neighbours stays where it is
    fv, ft = fan()
    assert np.array_equal(MO.smooth_taubin(fv, ft, 2)[:3], fv[:3])


# ---------------------------------------------------------------- vertex clustering
def test_clustering_the_sphere():
    m = mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    s = MO.simplify_vertex_clustering(v, t, 0.25, m["colors"])
    sv, st = s["vertices"], s["triangles"]
    assert (len(sv), len(st)) == (516, 1028)
    assert (st[:, 0] != st[:, 1]).all() and (st[:, 1] != st[:, 2]).all() and (st[:, 0] != st[:, 2]).all()
    rot = np.stack([np.roll(r, -int(np.argmin(r))) for r in st])
    assert len(np.unique(rot, axis=0)) == len(st)
    chi, (_, ucount), (_, dcount) = mc_oracle.euler_and_edges(st)
    assert chi == 2 and (ucount == 2).all() and (dcount == 1).all()
    a0, v0 = mc_oracle.area_and_volume(v, t)
    a1, v1 = mc_oracle.area_and_volume(sv, st)
    print(f"clustering: area ratio {a1 / a0:.3f}, volume ratio {v1 / v0:.3f}")
    assert abs(a1 / a0 - 1) <= 0.01 and abs(v1 / v0 - 1) <= 0.02
    assert (np.diff(s["vertex_index"]) > 0).all()
    assert np.array_equal(sv, v[s["vertex_index"]]) and np.array_equal(s["colors"], m["colors"][s["vertex_index"]])    # real vertices


def test_clustering_hand_mesh():
    v, t = cluster_hand()
    s = MO.simplify_vertex_clustering(v, t, 1.0, origin=(0, 0, 0))
    assert s["vertex_index"].tolist() == [0, 1, 2, 6]
    assert s["triangles"].tolist() == [[0, 1, 2], [2, 1, 0]]
    only = MO.simplify_vertex_clustering(v, t[[1, 2, 4]], 1.0, origin=(0, 0, 0))
    assert only["triangles"].tolist() == [[0, 1, 2]]                        # (3,4,5) lands on the new (0,1,2); its rotation is a duplicate
    rep = MO.voxel_assign(v, 1.0, (0, 0, 0))
    assert rep.tolist() == [0, 1, 2, 0, 1, 2, 6, 6]


# ---------------------------------------------------------------- hand meshes for every rule
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_meshes(name):
    v, t = HAND[name]
    nv = len(v)
    c = check_components(t, nv)
    check_incidence(t, nv)
    want = {"one": [0, 0, 0], "shared_vertex": [0] * 5, "disjoint": [0, 0, 0, 3, 3, 3], "aab": [0, 1, 0, 1],
            "unreferenced": [0, 1, 1, 3, 1, 1, 6]}[name]
    assert c["vertex_label"].tolist() == want
    if name == "aab":
        assert c["labels"].tolist() == [0, 1] and c["n_triangles"].tolist() == [1, 1]
        assert MO.incidence(t, nv, "vertices")[1].tolist() == [2, 3, 0, 1]
    none = MO.select_triangles(v, t, np.zeros(len(t), bool))
    assert none["vertices"].shape == (0, 3) and none["triangles"].shape == (0, 3) and len(none["vertex_index"]) == 0
    every = MO.select_triangles(v, t, np.ones(len(t), bool))
    used = np.unique(t)
    assert np.array_equal(every["vertex_index"], used) and np.array_equal(every["vertices"], v[used])
    if len(used) == nv:
        assert np.array_equal(every["triangles"], t)
    n = MO.vertex_normals(v, t)
    ref = tsdf.vertex_normals(v, t)
    assert np.abs(n - ref).max() <= 1e-6
    sm = MO.smooth_taubin(v, t, 1)
    unref = np.setdiff1d(np.arange(nv), used)
    assert np.array_equal(sm[unref], v[unref])
    out = MO.clean(v, t, None, keep_largest=1, smooth_iterations=1, voxel_size=0.5)
    assert len(out["vertex_normals"]) == len(out["vertices"]) == len(out["vertex_index"])


# ---------------------------------------------------------------- the Python layer's checks
def test_meshops_refuses_host_tensors_and_bad_arguments():
    import torch

    from sgam_neurips22_amd import meshops
    v, t = HAND["one"]
    host = tsdf.DeviceMesh(torch.from_numpy(v.copy()), None, torch.from_numpy(t.copy()), torch.tensor([3, 1, 0, 0], dtype=torch.int32), 3, 1)
    for call in (meshops.components, meshops.vertex_normals, meshops.smooth_taubin, meshops.clean, lambda m: meshops.incidence(m, "vertices"),
                 lambda m: meshops.simplify_vertex_clustering(m, 0.5), lambda m: meshops.remove_small_components(m, keep_largest=1)):
        with pytest.raises(_lib.SgamHipError, match="no CPU fallback"):
            call(host)
    for call in (lambda: meshops.incidence(host, "edges"), lambda: meshops.smooth_taubin(host, -1), lambda: meshops.smooth_taubin(host, 1, float("nan")),
                 lambda: meshops.remove_small_components(host, min_triangles=-2), lambda: meshops.remove_small_components(host, keep_largest=1.5)):
        with pytest.raises(ValueError):
            call()
    assert set(meshops.CLEAN_KEYS) == {"min_triangles", "keep_largest", "smooth_iterations", "voxel_size", "normals"}


# ---------------------------------------------------------------- the C entry points
def test_mesh_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == 10                                 # additive: the ABI version stays
    for name in ("sgam_mesh_components_workspace_bytes", "sgam_mesh_components_i32", "sgam_mesh_mark_vertices_i32",
                 "sgam_mesh_remap_triangles_i32", "sgam_mesh_incidence_count_i32", "sgam_mesh_incidence_fill_i32",
                 "sgam_mesh_vertex_normals_f32", "sgam_mesh_smooth_step_f32", "sgam_points_voxel_assign_f32",
                 "sgam_mesh_dedup_workspace_bytes", "sgam_mesh_cluster_triangles_i32"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    p, q = ctypes.c_void_p(256), ctypes.c_void_p(512)                   # never dereferenced: every check comes before a launch
    odd = ctypes.c_void_p(264)

    size = lib.sgam_mesh_components_workspace_bytes
    assert size(1) == 16 and size(4) == 16 and size(5) == 32 and size(0) == size(-3) == -1

    def comp(tri=p, nt=10, nv=8, w=p, wb=size(8), vl=p, tl=p, tc=p, flag=p):
        return lib.sgam_mesh_components_i32(tri, nt, nv, w, wb, vl, tl, tc, flag, None)

    for kw in (dict(tri=None), dict(vl=None), dict(tl=None), dict(tc=None), dict(flag=None), dict(nt=0), dict(nt=-1), dict(nv=0), dict(w=None),
               dict(wb=size(8) - 1), dict(w=odd), dict(nt=(1 << 28) + 1)):
        assert comp(**kw) == -1, kw

    for args in ((None, 10, 8, None, p, p), (p, 10, 8, None, None, p), (p, 10, 8, None, p, None), (p, 0, 8, None, p, p), (p, 10, 0, None, p, p)):
        assert lib.sgam_mesh_mark_vertices_i32(*args, None) == -1, args

    def remap(tri=p, nt=10, idx=p, m=4, vmap=p, nv=8, out=p, flag=p):
        return lib.sgam_mesh_remap_triangles_i32(tri, nt, idx, m, vmap, nv, out, flag, None)

    for kw in (dict(tri=None), dict(idx=None), dict(vmap=None), dict(out=None), dict(flag=None), dict(nt=0), dict(m=0), dict(m=11), dict(nv=0)):
        assert remap(**kw) == -1, kw

    for args in ((None, 10, 8, 0, p, p), (p, 10, 8, 0, None, p), (p, 10, 8, 0, p, None), (p, 0, 8, 0, p, p), (p, 10, -2, 1, p, p),
                 (p, 10, 8, 2, p, p), (p, 10, 8, -1, p, p)):
        assert lib.sgam_mesh_incidence_count_i32(*args, None) == -1, args

    def fill(tri=p, nt=10, nv=8, kind=1, off=p, n_raw=60, items=p, deg=p, flag=p):
        return lib.sgam_mesh_incidence_fill_i32(tri, nt, nv, kind, off, n_raw, items, deg, flag, None)

    for kw in (dict(tri=None), dict(off=None), dict(items=None), dict(deg=None), dict(flag=None), dict(nt=0), dict(nv=0), dict(kind=2),
               dict(kind=-1), dict(n_raw=0), dict(n_raw=61)):
        assert fill(**kw) == -1, kw

    def normals(v=p, nv=8, tri=p, nt=10, off=p, items=p, n=30, out=p):
        return lib.sgam_mesh_vertex_normals_f32(v, nv, tri, nt, off, items, n, out, None)

    for kw in (dict(v=None), dict(tri=None), dict(off=None), dict(items=None), dict(out=None), dict(nv=0), dict(nt=0), dict(n=-1)):
        assert normals(**kw) == -1, kw

    def smooth(src=p, dst=q, nv=8, off=p, items=p, n=30, w=0.5):
        return lib.sgam_mesh_smooth_step_f32(src, dst, nv, off, items, n, w, None)

    for kw in (dict(src=None), dict(dst=None), dict(dst=p), dict(off=None), dict(items=None), dict(nv=0), dict(n=-1), dict(w=float("nan")),
               dict(w=float("inf"))):
        assert smooth(**kw) == -1, kw

    vsize = lib.sgam_points_voxel_workspace_bytes

    def assign(pts=p, N=100, o=(0.0, 0.0, 0.0), h=0.5, w=p, wb=vsize(100), keep=p, count=p, rep=p, flag=p):
        return lib.sgam_points_voxel_assign_f32(pts, N, *o, h, w, wb, keep, count, rep, flag, None)

    for kw in (dict(pts=None), dict(keep=None), dict(count=None), dict(rep=None), dict(flag=None), dict(N=0), dict(N=-1), dict(h=0.0),
               dict(h=-1.0), dict(h=float("nan")), dict(h=float("inf")), dict(o=(0.0, float("nan"), 0.0)), dict(w=None),
               dict(wb=vsize(100) - 1), dict(w=odd), dict(N=200)):
        assert assign(**kw) == -1, kw

    dsize = lib.sgam_mesh_dedup_workspace_bytes
    assert dsize(1) == 4 * 256 + 16 and dsize(128) == 4 * 256 + 512 and dsize(129) == 4 * 512 + 528 and dsize(0) == dsize(-1) == -1
    assert dsize((1 << 28) + 1) == -1

    def cluster(tri=p, nt=100, cl=p, nv=80, w=p, wb=dsize(100), out=p, keep=p, flag=p):
        return lib.sgam_mesh_cluster_triangles_i32(tri, nt, cl, nv, w, wb, out, keep, flag, None)

    for kw in (dict(tri=None), dict(cl=None), dict(out=None), dict(keep=None), dict(flag=None), dict(nt=0), dict(nv=0), dict(w=None),
               dict(wb=dsize(100) - 1), dict(w=odd), dict(nt=200)):
        assert cluster(**kw) == -1, kw
