"""CPU: the BVH's numpy twin (tests/bvh_oracle.py) — the structure it builds, the SOUNDNESS of its two pruning rules tested
directly (no node on the path to a brute-force winner, or to a tie with it, is ever skipped), its traversal against the brute
force of tests/meshquery_oracle.py and tests/raycast_oracle.py bit for bit, and the argument checks of the new entry points through
ctypes.  tests/test_gpu_bvh.py runs the kernels against the twin and the brute-force truths and shares the meshes and rays
defined here."""
import ctypes
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import bvh_oracle as B  # noqa: E402
import meshquery_oracle as Q  # noqa: E402
import raycast_oracle as R  # noqa: E402
import test_meshops_cpu as C  # noqa: E402
import test_raycast_cpu as RC  # noqa: E402
from test_gpu_meshquery import spanning_mesh  # noqa: E402

f32 = np.float32


# ---------------------------------------------------------------- meshes, rays and queries shared with the GPU tests (never modified)
def mixed_mesh():
    """the marching-cubes sphere and the twelve triangles of a surrounding box 100 times its size: the mesh a grid cannot serve"""
    m = C.mesh("sphere")
    v, t = m["vertices"], m["triangles"]
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo).max() * 50
    corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], dtype=np.float64) * half + mid
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], dtype=np.int32) + len(v)
    return np.concatenate([v, corners.astype(f32)]), np.concatenate([t[:300], box, t[300:]])


def one_code_mesh(copies=37):
    """exact copies of one triangle: every Morton code is equal, so order and ties go by the index alone"""
    v = np.array([[0, 0, 0.5], [1, 0, 0.25], [0, 1, 0.75]], dtype=f32)
    return v, np.tile(np.array([[0, 1, 2]], dtype=np.int32), (copies, 1))


MESHES = {"lattice": RC.lattice_mesh, "spanning": spanning_mesh, "mixed": mixed_mesh}
_TREES = {}


def tree(name):
    if name not in _TREES:
        _TREES[name] = B.Tree(*MESHES[name]())
    return _TREES[name]


def random_rays(v, n, seed):
    """n seeded rays from around the mesh's box towards it: a third aimed at vertices (t = 1 there), directions with exact 0 and
    -0 components, some normalised"""
    rs = np.random.RandomState(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    size = (hi - lo).max()
    o = rs.uniform(lo - 0.3 * size, hi + 0.3 * size, (n, 3))
    target = np.where(rs.uniform(size=(n, 1)) < 0.33, v[rs.randint(0, len(v), n)], rs.uniform(lo, hi, (n, 3)))
    d = target - o
    d[::7, 0], d[3::11, 1], d[5::13, 2] = 0.0, -0.0, 0.0
    d[1::9] /= np.maximum(np.linalg.norm(d[1::9], axis=1, keepdims=True), 1e-9)
    return np.concatenate([o, d], 1).astype(f32)


def far_rays(v, n=60, seed=6):
    """rays whose origins lie 2^4, 2^10 and 2^16 coordinate scales away, aimed at the mesh's vertices"""
    rs = np.random.RandomState(seed)
    scale = float(np.abs(v).max())
    out = []
    for k in (4, 10, 16):
        u = rs.normal(0, 1, (n, 3))
        o = (u / np.linalg.norm(u, axis=1, keepdims=True)) * scale * 2.0 ** k
        target = v[rs.randint(0, len(v), n)].astype(np.float64)
        d = target - o
        d[::2] /= 2.0 ** k                                                    # half of them with t = 2^k at the mesh
        out.append(np.concatenate([o, d], 1))
    return np.concatenate(out).astype(f32)


def face_rays(tr, n_nodes=24, seed=9):
    """rays lying IN a face of a node's box (the origin's coordinate is the face's, the direction's component there an exact 0 or
    -0), through the corner of the triangle that defines that face, and the same rays moved off the face by one ulp either way"""
    rs = np.random.RandomState(seed)
    nodes = rs.randint(0, max(tr.n - 1, 1), n_nodes)
    out = []
    for c in nodes:
        box = tr.boxes[c]
        for axis in range(3):
            for side in (0, 3):
                plane = box[side + axis]
                first, last = (tr.span[c] if tr.n > 1 else (0, 0))
                pts = tr.records[first:last + 1].reshape(-1, 3)
                p = pts[np.flatnonzero(pts[:, axis] == plane)[0]].astype(np.float64)
                step = rs.uniform(0.2, 1.0, 3) * rs.choice([-1, 1], 3)
                step[axis] = 0.0
                for zero in (0.0, -0.0):
                    for nudge in (0, 1, -1):
                        o = p - step
                        d = step.copy()
                        d[axis] = zero
                        o[axis] = plane if nudge == 0 else np.nextafter(plane, f32(np.inf * nudge))
                        out.append(np.concatenate([o, d]))
    return np.array(out, dtype=f32)


def random_queries(v, n, seed):
    """n seeded queries: around the box, on the mesh's vertices and edge midpoints (ties between the triangles that share them),
    far away, and rows that are not points"""
    rs = np.random.RandomState(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    size = (hi - lo).max()
    q = rs.uniform(lo - 0.5 * size, hi + 0.5 * size, (n, 3))
    q[::5] = v[rs.randint(0, len(v), len(q[::5]))]
    q[1::17] *= 1000.0
    q = q.astype(f32)
    if n > 8:
        q[n // 3, 1], q[n // 2, 0], q[n - 2] = np.nan, np.inf, -np.inf
    return q


def shared_edge_queries(v, t, n=40, seed=2):
    """queries exactly on vertices and on midpoints of edges that two triangles share: the lower index wins"""
    rs = np.random.RandomState(seed)
    tri = t[rs.randint(0, len(t), n)]
    return np.concatenate([v[tri[:, 0]], ((v[tri[:, 0]].astype(np.float64) + v[tri[:, 1]]) / 2)]).astype(f32)


# ---------------------------------------------------------------- structure
def check_structure(tr):
    n = tr.n
    assert len(tr.ids) == n == len(set(tr.ids.tolist())) and (np.diff(tr.sorted) > 0).all()
    if n == 0:
        return
    a, b, c, _ = Q.corners(tr.vertices, tr.triangles)
    assert sorted(tr.ids.tolist()) == np.flatnonzero(Q.candidates(a, b, c)).tolist()           # every candidate is exactly one leaf
    if n == 1:
        assert tr.children.shape == (0, 2) and tr.boxes.shape == (1, 6)
        return
    seen = np.zeros(2 * n - 1, dtype=int)
    for i in range(n - 1):
        first, last = tr.span[i]
        parts = []
        for ch in tr.children[i]:
            seen[ch] += 1
            parts.append((ch - (n - 1),) * 2 if ch >= n - 1 else tuple(tr.span[ch]))
        assert parts[0][0] == first and parts[0][1] + 1 == parts[1][0] and parts[1][1] == last, i    # the children partition the parent
        pts = tr.records[first:last + 1].reshape(-1, 3)
        assert np.array_equal(tr.boxes[i, :3], pts.min(0)) and np.array_equal(tr.boxes[i, 3:], pts.max(0)), i
        assert tr.height[i] == 1 + max(0 if ch >= n - 1 else tr.height[ch] for ch in tr.children[i])
    assert seen[0] == 0 and (seen[1:] == 1).all() and tuple(tr.span[0]) == (0, n - 1)
    assert 1 <= tr.height[0] <= B.KEY_BITS and tr.height.min() >= 1


@pytest.mark.parametrize("name", sorted(MESHES))
def test_structure_of_the_shared_meshes(name):
    tr = tree(name)
    check_structure(tr)
    assert tr.height[0] <= 2 * int(np.ceil(np.log2(tr.n))) + 8                  # (these meshes are far from the adversarial bound)


def test_structure_of_zero_to_three_candidates_one_code_and_non_candidates():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [0.2, 0.3, 1], [2, 2, 2], [np.nan, 0, 0]], dtype=f32)
    tris = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 4, 5]], dtype=np.int32)
    for n in range(4):
        tr = B.Tree(v, tris[:n])
        assert tr.n == n
        check_structure(tr)
    assert B.Tree(v, tris[:2]).children.tolist() == [[1, 2]] and B.Tree(v, tris[:3]).height[0] == 2
    empty = B.Tree(v, tris[:0])
    assert B.cast(empty, [0.2, 0.2, 1, 0, 0, -1])[:3] == (B.INF, -1, False) and B.distance(empty, [0, 0, 0])[1] == -1
    one = B.Tree(*one_code_mesh())
    check_structure(one)
    assert len(set((one.sorted >> B.ID_BITS).tolist())) == 1 and one.ids.tolist() == list(range(37))     # one code: the order is the index
    assert one.height[0] <= 6                                                   # the index bits alone make a balanced tree
    # what is not a candidate: a NaN corner, no area, an index outside the mesh — never a leaf; their keys sort last
    mixed = np.array([[0, 1, 2], [0, 1, 6], [1, 1, 2], [1, 3, 2], [0, 1, 9], [2, 3, 4], [-1, 0, 1]], dtype=np.int32)
    tr = B.Tree(v, mixed)
    check_structure(tr)
    k, n = B.keys(v, mixed)
    assert n == 3 and sorted(tr.ids.tolist()) == [0, 3, 5] and (k[[1, 2, 4, 6]] == B.NO_KEY).all() and (k[[0, 3, 5]] >= 0).all()
    assert (k[[0, 3, 5]] < (1 << B.KEY_BITS)).all()


def test_keys_by_hand():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [4, 4, 4], [3, 4, 4], [4, 3, 4], [4, 4, 3]], dtype=f32)
    t = np.array([[0, 1, 2], [3, 4, 5], [3, 5, 6]], dtype=np.int32)
    k, n = B.keys(v, t)
    # box [0, 4]^3; centres (0.5, 0.5, 0), (3.5, 3.5, 4), (4, 3.5, 3.5): q = floor(c / 4 * 2048), capped at 2047
    q = [(256, 256, 0), (1792, 1792, 2047), (2047, 1792, 1792)]
    for i, (x, y, z) in enumerate(q):
        code = sum((((x >> b) & 1) << (3 * b + 2)) | (((y >> b) & 1) << (3 * b + 1)) | (((z >> b) & 1) << (3 * b)) for b in range(11))
        assert int(k[i]) == (code << 28) | i
    assert n == 3
    flat, _ = B.keys(v[:3], t[:1])                                              # a box without extent on an axis: that axis gives 0
    assert int(flat[0]) & ((1 << 28) - 1) == 0 and (int(flat[0]) >> 28) & int("001" * 11, 2) == 0


# ---------------------------------------------------------------- soundness of the two pruning rules
def ray_sets(name):
    v, _ = MESHES[name]()
    sets = [(random_rays(v, 1500 if name != "lattice" else 700, 11), ((0.0, np.inf), (0.25, 1.0))), (far_rays(v), ((0.0, np.inf),)),
            (face_rays(tree(name)), ((0.0, np.inf), (0.0, 1.0)))]
    if name == "lattice":
        sets.append((RC.adversarial_rays(), RC.WINDOWS))
    return sets


@pytest.mark.parametrize("name", sorted(MESHES))
def test_no_node_that_holds_a_hit_fails_the_ray_test(name):
    """for EVERY hit of every ray (so also every tie with the winner), the hit's leaf and all its ancestors pass with [tnear, t_hit]"""
    tr = tree(name)
    paths = tr.paths()
    a, b, c = tr.records[:, 0], tr.records[:, 1], tr.records[:, 2]
    pairs = 0
    for rays, windows in ray_sets(name):
        real = R.is_ray(rays)
        for tnear, tfar in windows:
            for s in range(0, len(rays), 128):
                rs = rays[s:s + 128]
                hit, t, _, _ = R.ray_triangle(a[None], b[None], c[None], rs[:, None, :3], rs[:, None, 3:], tnear, tfar, tr.guard)
                i, k = np.nonzero(hit & real[s:s + 128, None])
                ok, enter = B.ray_node(tr.boxes[paths[k]], rs[i][:, None], tr.guard, tnear, t[i, k][:, None])
                assert ok.all(), (name, tnear, tfar, rs[i][~ok.all(1)][:3])
                assert (enter <= t[i, k][:, None]).all()                        # and the pop's second look (near <= best) passes too
                pairs += len(i)
    assert pairs > 1000


@pytest.mark.parametrize("name", sorted(MESHES))
def test_no_ancestor_of_a_winner_or_a_tie_fails_the_distance_test(name):
    tr = tree(name)
    paths = tr.paths()
    v, t = MESHES[name]()
    q = np.concatenate([random_queries(v, 1200, 4), shared_edge_queries(v, t)])
    q = q[np.isfinite(q).all(1)]
    a, b, c = tr.records[:, 0], tr.records[:, 1], tr.records[:, 2]
    ties = 0
    for s in range(0, len(q), 128):
        qs = q[s:s + 128]
        d2, _, _ = Q.point_triangle(a[None], b[None], c[None], qs[:, None])
        best = np.where(np.isfinite(d2), d2, np.inf).min(1).astype(f32)
        i, k = np.nonzero(d2 == best[:, None])                                  # the winner and every exact tie with it
        ties += len(i) - len(qs)
        for max_d2 in (np.inf, best[i][:, None]):                               # unbounded, and bounded exactly at the winner
            ok, lb = B.distance_node(tr.boxes[paths[k]], qs[i][:, None], tr.margin, max_d2, best[i][:, None])
            assert ok.all(), (name, qs[i][~ok.all(1)][:3])
            assert not (best[i][:, None] < lb).any()
    assert ties > 20 or name == "spanning"                                      # (its triangles share no vertex: nothing ties there)


# ---------------------------------------------------------------- the twin's traversal equals the twin's brute force
@pytest.mark.parametrize("name", sorted(MESHES))
def test_traversal_equals_brute_force_for_rays(name):
    tr = tree(name)
    v, t = MESHES[name]()
    popped = []
    for rays, windows in ray_sets(name):
        rays = rays[::max(1, len(rays) // (15 if name == "mixed" else 90))]      # (a numpy walk takes milliseconds per ray)
        for window in windows[:3]:
            want = R.cast_rays(v, t, rays, *window)
            for i in range(len(rays)):
                best, tri, hit, pops, deepest = B.cast(tr, rays[i], *window)
                assert (tri, f32(best).view(np.uint32)) == (want["triangle"][i], want["t"][i:i + 1].view(np.uint32)[0]), (name, window, i, rays[i])
                assert B.cast(tr, rays[i], *window, any_hit=True)[2] == want["hit"][i] == hit
                assert deepest <= tr.height[0] + 1
                popped.append(pops)
    assert np.mean(popped) < 0.25 * (2 * tr.n - 1)                              # it prunes: far fewer nodes than the tree has


@pytest.mark.parametrize("name", sorted(MESHES))
def test_traversal_equals_brute_force_for_distance(name):
    tr = tree(name)
    v, t = MESHES[name]()
    q = np.concatenate([random_queries(v, 150, 4), shared_edge_queries(v, t, 15)])
    size = float((v.max(0) - v.min(0)).max())
    popped = []
    for max_distance in (None, 0.05 * size):
        m2 = np.inf if max_distance is None else f32(max_distance) * f32(max_distance)
        want = Q.mesh_distance(v, t, q, m2)
        for i in range(len(q)):
            d2, tri, x, pops = B.distance(tr, q[i], m2)
            assert (tri, f32(d2).view(np.uint32)) == (want["triangle"][i], want["d2"][i:i + 1].view(np.uint32)[0]), (name, max_distance, i, q[i])
            assert np.array_equal(np.asarray(x, f32).view(np.uint32), want["closest"][i].view(np.uint32))
            popped.append(pops)
    assert (want["triangle"] == -1).sum() > 3 and np.mean(popped) < 0.25 * (2 * tr.n - 1)


def test_traversal_equals_brute_force_for_visibility():
    v, t = RC.two_quads()
    tr = B.Tree(v, t)
    pts = np.array([[0.05, 0.02, 2.0], [0.3, 0.3, 2.0], [0.9, 0.0, 1.9], [0.1, 0.1, 1.0005], [0.0, 0.0, 5.0], [5.0, 0.0, 2.0], [0, 0, -2.0], [np.nan, 0, 1]], dtype=f32)
    cam = dict(fx=20.0, fy=20.0, cx=31.5, cy=31.5, H=64, W=64, z_near=0.1, z_far=4.0)
    poses = np.stack([np.eye(4), [[1, 0, 0, -0.8], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]]).astype(f32)
    for tol in (1e-3, 0.0):
        assert B.visibility(tr, pts, poses, tolerance=tol, **cam).tolist() == R.visibility(pts, v, t, poses, tolerance=tol, **cam).tolist()
    assert B.visibility(tr, pts, poses[:1], **cam).tolist() == [0, 0, 1, 1, 0, 0, 0, 0]
    v, t = mixed_mesh()
    rs = np.random.RandomState(1)
    pts = np.concatenate([v[rs.randint(0, len(v) - 8, 40)], rs.uniform(v[:-8].min(0), v[:-8].max(0), (20, 3))]).astype(f32)
    pose = np.eye(4, dtype=f32)[None].copy()
    pose[0, :3, 3] = -(v[:-8].mean(0) - np.array([0, 0, 6.0], dtype=f32))          # a camera 6 in front of the sphere, inside the big box
    want = R.visibility(pts, v, t, pose, **{**cam, "z_far": 20.0})
    assert B.visibility(tree("mixed"), pts, pose, **{**cam, "z_far": 20.0}).tolist() == want.tolist() and 0 < want.sum() < len(pts)


# ---------------------------------------------------------------- the entry points without a GPU
def test_bvh_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == _lib.ABI_VERSION == 10                     # additions only
    one, inf, nan = ctypes.c_void_p(16), float("inf"), float("nan")
    r16 = lambda n: (n + 15) & ~15                                              # noqa: E731
    for n in (1, 2, 3, 1000):
        assert lib.sgam_mesh_bvh_workspace_bytes(n) == 48 * n + r16(24 * (2 * n - 1)) + r16(8 * max(n - 1, 1)) + r16(4 * max(n - 1, 1))
    assert lib.sgam_mesh_bvh_workspace_bytes(0) == -1 and lib.sgam_mesh_bvh_workspace_bytes((1 << 28) + 1) == -1
    mesh, box = (one, 3, one, 1), (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)

    def keys(mesh=mesh, box=box, out=one, count=one, flag=one):
        return lib.sgam_mesh_bvh_keys(*mesh, *box, out, count, flag, None)

    for bad in (dict(mesh=(None, 3, one, 1)), dict(mesh=(one, 0, one, 1)), dict(mesh=(one, 3, None, 1)), dict(mesh=(one, 3, one, 0)),
                dict(mesh=(one, 3, one, (1 << 28) + 1)), dict(out=None), dict(count=None), dict(flag=None), dict(box=(0.0, 0.0, 0.0, 1.0, -1.0, 1.0)),
                dict(box=(nan, 0.0, 0.0, 1.0, 1.0, 1.0)), dict(box=(0.0, 0.0, 0.0, inf, 1.0, 1.0))):
        assert keys(**bad) == -1, bad

    def build(mesh=(one, 3, one, 4), keys=one, n=4, ws=one, nbytes=1 << 20, flag=one):
        return lib.sgam_mesh_bvh_build(*mesh, keys, n, ws, nbytes, flag, None)

    for bad in (dict(mesh=(None, 3, one, 4)), dict(keys=None), dict(n=0), dict(n=5), dict(ws=None), dict(nbytes=64), dict(ws=ctypes.c_void_p(24)),
                dict(flag=None)):
        assert build(**bad) == -1, bad
    tables = dict(n=4, ws=one, nbytes=1 << 20)

    def distance(q=one, nq=1, box=box, m2=inf, d2=one, tri=one, flag=one, **kw):
        a = {**tables, **kw}
        return lib.sgam_mesh_distance_bvh_f32(q, nq, a["n"], *box, a["ws"], a["nbytes"], m2, d2, tri, None, flag, None)

    ok = dict(rays=one, nr=1, mode=0, tnear=0.0, tfar=inf, guard=0.0, t=one, tri=one, hit=None, flag=one)

    def cast(**kw):
        a = {**ok, **tables, **kw}
        return lib.sgam_mesh_raycast_bvh_f32(a["rays"], a["nr"], a["n"], a["ws"], a["nbytes"], a["mode"], a["tnear"], a["tfar"], a["guard"], a["t"],
                                             a["tri"], None, None, a["hit"], a["flag"], None)

    cam = (10.0, 10.0, 4.0, 4.0, 8, 8, 0.1, 4.0, 1e-3, 0.0)

    def visible(points=one, np_=1, poses=one, p=1, cam=cam, count=one, flag=one, **kw):
        a = {**tables, **kw}
        return lib.sgam_mesh_visibility_bvh_f32(points, np_, poses, p, *cam, a["n"], a["ws"], a["nbytes"], count, flag, None)

    for call in (distance, cast, visible):
        for bad in (dict(n=0), dict(n=(1 << 28) + 1), dict(ws=None), dict(nbytes=64), dict(ws=ctypes.c_void_p(24)), dict(flag=None)):
            assert call(**bad) == -1, (call.__name__, bad)
    for bad in (dict(q=None), dict(nq=0), dict(m2=-1.0), dict(m2=nan), dict(d2=None), dict(tri=None), dict(box=(0.0, 0.0, 1.0, 1.0, 1.0, 0.0))):
        assert distance(**bad) == -1, bad
    for bad in (dict(rays=None), dict(nr=0), dict(mode=2), dict(mode=-1), dict(mode=1), dict(tnear=-1.0), dict(tnear=nan), dict(tnear=inf), dict(tfar=nan),
                dict(tnear=2.0, tfar=1.0), dict(guard=-1.0), dict(guard=nan), dict(guard=inf), dict(t=None), dict(tri=None)):
        assert cast(**bad) == -1, bad
    for bad in (dict(points=None), dict(np_=0), dict(poses=None), dict(p=0), dict(count=None), dict(cam=(0.0,) + cam[1:]), dict(cam=cam[:6] + (0.0,) + cam[7:]),
                dict(cam=cam[:8] + (1.5, 0.0)), dict(cam=cam[:9] + (-1.0,))):
        assert visible(**bad) == -1, bad


def test_python_api_refuses_host_tensors_another_mesh_and_bad_arguments():
    import torch
    from sgam_neurips22_amd import meshops
    from sgam_neurips22_amd.ops import SgamHipError
    from sgam_neurips22_amd.tsdf import DeviceMesh

    def host_mesh():
        return DeviceMesh(torch.from_numpy(RC.SQUARE.copy()), None, torch.from_numpy(RC.SQUARE_T.copy()), torch.tensor([4, 2, 0, 0], dtype=torch.int32), 4, 2)

    mesh, rays = host_mesh(), torch.zeros((3, 6))
    with pytest.raises(SgamHipError):
        meshops.TriangleBVH(mesh)
    other = object.__new__(meshops.TriangleBVH)                                 # a tree that claims another mesh (nothing was built)
    other.mesh = host_mesh()
    for call in (lambda: meshops.cast_rays(rays, mesh, accel=other), lambda: meshops.test_occlusions(rays, mesh, accel=other),
                 lambda: meshops.point_mesh_distance(rays[:, :3], mesh, accel=other), lambda: meshops.cast_rays(rays, mesh, accel="bvh"),
                 lambda: meshops.visible_points(rays[:, :3], mesh, np.eye(4)[None], np.eye(3), 4, 4, 0.1, 1.0, grid=other)):
        with pytest.raises(ValueError):
            call()
    other.mesh = mesh
    with pytest.raises(ValueError):
        meshops.cast_rays(rays, mesh, accel=other, cell_size=0.1)               # cell_size belongs to a grid that is built
    with pytest.raises(ValueError):
        meshops.cast_rays(rays, mesh, accel=other, method="bvh")                # the method strings did not change
    with pytest.raises(ValueError):
        meshops.surface_metrics(mesh, mesh, 0.1, n_samples=8, accelerator="tree")
    for method in ("bvh", "tree"):
        with pytest.raises(ValueError):
            meshops.point_mesh_distance(rays[:, :3], mesh, method=method)
