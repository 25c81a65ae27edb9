"""CPU: the ray kernels' numpy twin (tests/raycast_oracle.py) against hand truths, its reference grid walk against its own brute
force on rays chosen to trouble the walk, the twin against a float64 Moeller-Trumbore on the marching-cubes meshes of
tests/test_meshops_cpu.py, and the argument checks of the new entry points through ctypes.  tests/test_gpu_raycast.py runs the
kernels against the twin bit for bit and shares the meshes and rays defined here."""
import ctypes
import os
import sys

import numpy as np
import pytest

from sgam_neurips22_amd import _lib

sys.path.insert(0, os.path.dirname(__file__))
import raycast_oracle as R  # noqa: E402
import test_meshops_cpu as C  # noqa: E402

f32 = np.float32
ULP = 2.0 ** -23
# test_twin_against_float64, measured on the CPU over both meshes, and the factor allowed on top:
#   MEASURED_K: the largest |t - t64| |d| / (2^-23 (t |d| + coordinate scale) / |cos|) over the triangles both hit, cos the angle
#   between the ray and the triangle's normal (a grazing ray turns a rounding of the coordinates into a long way along the ray);
#   MEASURED_BAND: where the two disagree on hit / miss, how far the hit that only one of them has lies from its triangle's
#   nearest edge, in float64 barycentric units (grazing rays at triangles of 1 / 40 of the coordinate scale included)
MEASURED_K, MEASURED_BAND, FACTOR = 1.76, 3.4e-3, 4.0

SQUARE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=f32)
SQUARE_T = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)


# ---------------------------------------------------------------- meshes and rays shared with the GPU tests (never modified)
def lattice_mesh(n=8):
    """two tessellated planes z = 1/4 and z = 3/4 over the unit square (n x n quads of two triangles) and a wall x = 1/2 over
    y, z in [0, 1]: every coordinate a multiple of 1 / n, so cell faces of a grid of edge 1 / n pass through vertices and edges"""
    k = np.arange(n + 1, dtype=np.float64) / n
    a, b = np.meshgrid(k, k, indexing="ij")
    sheets = [np.stack([a, b, np.full_like(a, 0.25)], -1), np.stack([a, b, np.full_like(a, 0.75)], -1), np.stack([np.full_like(a, 0.5), a, b], -1)]
    v = np.concatenate([s.reshape(-1, 3) for s in sheets]).astype(f32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    q = (i * (n + 1) + j).reshape(-1)
    quad = np.concatenate([np.stack([q, q + n + 1, q + 1], 1), np.stack([q + n + 1, q + n + 2, q + 1], 1)])
    t = np.concatenate([quad + s * (n + 1) ** 2 for s in range(3)]).astype(np.int32)
    return v, t


def adversarial_rays(n=8):
    """rays that trouble a walk through a grid of edge 1 / n over the unit box (lattice_mesh): origins on cell faces, edges and
    corners with axis-parallel and exactly diagonal directions, origins inside / outside / pointing away, rays along the grid's
    border, one and two zero direction components, hits exactly on shared edges and vertices, a far origin, rows that are not rays"""
    h = 1.0 / n
    rays = []
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    diagonals = [(1, 1, 0), (-1, 1, 0), (1, 0, -1), (0, -1, 1), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)]
    for o in [(3 * h, 2 * h, 5 * h), (3 * h, 2.5 * h, 5.5 * h), (3 * h, 2 * h, 5.5 * h), (0, 0, 0), (1, 1, 1), (0.5, 0.5, 0.5), (h, 0.5, 1)]:
        rays += [(*o, *d) for d in axes + diagonals]                        # corners, faces, edges of cells; the grid's own corners
    for o in [(0.3, 0.4, 0.5), (0.77, 0.12, 0.9), (-1, 0.4, 0.6), (2, 2, 2), (0.4, -3, 0.3), (0.45, 0.55, 4)]:
        rays += [(*o, *d) for d in axes + diagonals]                        # inside, outside, towards and away
    for y in (0.0, 1.0, -2.0 ** -20, 1 + 2.0 ** -20, 2.0 ** -12, 1 + 2.0 ** -12):
        rays += [(-1, y, 0.3, 1, 0, 0), (2, y, 0.8, -1, 0, 0), (y, -1, 0.3, 0, 1, 0), (0.2, y, 3, 0, 0, -1), (-1, y, -1, 1, 0, 1)]       # along the border
    rays += [(0.1, 0.2, 1.5, 0.3, 0, -1), (0.1, 0.2, 1.5, 0, 0.3, -1), (-0.5, 0.3, 0.1, 1, 0.01, 0), (0.9, 0.9, -1, 0, -0.001, 1)]   # zero components
    for x, y in [(0.25, 0.25), (0.5, 0.5), (0.3125, 0.25), (0.25, 0.3125), (0.3125, 0.3125), (0.125, 0.875), (0, 0), (1, 1), (0.5, 0.25)]:
        rays += [(x, y, 1.5, 0, 0, -1), (x, y, -1, 0, 0, 2), (x, y, 0.5, 0, 0, 1)]     # shared vertices, edges, diagonals; the wall's top edge
    rays += [(2, 0.25, 0.5, -1, 0, 0), (2, 0.3125, 0.3125, -2, 0, 0), (1.5, 0.5, 0.5, -1, 0, 0)]       # onto the wall: vertex, diagonal
    rays += [(300, 0.4, 0.6, -1, 0, 0), (0.4, 0.6, -5000, 0, 0, 1), (1e6, 1e6, 1e6, -1, -1, -1)]       # far origins
    rs = np.random.RandomState(12)
    o = rs.uniform(-0.5, 1.5, (60, 3))
    rays += [(*a, *b) for a, b in zip(o, rs.uniform(0, 1, (60, 3)) - o)]
    rays = np.array(rays, dtype=f32)
    bad = np.array([[np.nan, 0, 0, 1, 0, 0], [0, 0, 0, np.inf, 0, 0], [0.5, 0.5, 1, 0, 0, 0], [0, -np.inf, 0, 0, 0, 1], [0.5, 0.5, 1, 0, np.nan, -1]], dtype=f32)
    return np.concatenate([rays, bad])


WINDOWS = ((0.0, np.inf), (0.0, 0.7), (0.9, np.inf), (0.25, 0.25), (0.75, 1.25))


def hand_rays(n, seed=0):
    """n rays around the unit box, rows that are not rays among them (row 0 stays a ray)"""
    rs = np.random.RandomState(seed)
    o = rs.uniform(-1, 2, (n, 3))
    r = np.concatenate([o, rs.uniform(0, 1, (n, 3)) - o], 1).astype(f32)
    r[0] = [0.25, 0.25, 1, 0, 0, -1]
    if n > 4:
        r[n // 3, 1] = np.nan
        r[n // 2, 3] = np.inf
        r[n - 2, 3:] = 0
    return r


def mesh_rays(v, n=600, seed=3):
    """n rays at a mesh: from around and inside its box towards points near its vertices, and some that miss"""
    rs = np.random.RandomState(seed)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    size = (hi - lo).max()
    o = rs.uniform(lo - 0.5 * size, hi + 0.5 * size, (n, 3))
    target = v[rs.randint(0, len(v), n)] + rs.normal(0, 0.02 * size, (n, 3))
    d = target - o
    d[: n // 3] /= np.linalg.norm(d[: n // 3], axis=1, keepdims=True)       # a third normalised, the rest with t = 1 near the target
    d[-n // 10:] = rs.normal(0, 1, (n // 10, 3))
    return np.concatenate([o, d], 1).astype(f32)


# ---------------------------------------------------------------- hand truths
@pytest.mark.parametrize("order", [0, 1])
def test_unit_square_both_triangles_hit_and_the_lower_index_wins(order):
    t = SQUARE_T[::-1].copy() if order else SQUARE_T
    ray = np.array([[0.5, 0.5, 1, 0, 0, -1]], dtype=f32)
    for k in range(2):
        hit, tt, u, v = R.ray_triangle(*(SQUARE[t[k, c]] for c in range(3)), ray[0, :3], ray[0, 3:], 0, np.inf, 0)
        assert hit and tt == 1.0
    out = R.cast_rays(SQUARE, t, ray)
    assert out["t"].tolist() == [1.0] and out["triangle"].tolist() == [0] and out["hit"].tolist() == [True]
    (u, v), (a, b, c) = out["uv"][0], SQUARE[t[0]]
    assert np.abs(out["normal"][0]).tolist() == [0.0, 0.0, 1.0] and ((1 - u - v) * a + u * b + v * c).tolist() == [0.5, 0.5, 0.0]


def test_windows_scaling_planes_and_rows_that_are_not_rays():
    ray = np.array([[0.25, 0.25, 1, 0, 0, -1]], dtype=f32)
    assert R.cast_rays(SQUARE, SQUARE_T, ray, 0.0, 1.0)["t"][0] == 1.0                 # the window is closed at both ends
    assert R.cast_rays(SQUARE, SQUARE_T, ray, 1.0, 1.0)["triangle"][0] == 0
    assert R.cast_rays(SQUARE, SQUARE_T, ray, 0.0, 0.999)["triangle"][0] == -1
    assert R.cast_rays(SQUARE, SQUARE_T, ray, 1.001, np.inf)["t"][0] == np.inf
    for s in (0.5, 2.0, 4.0):                                                           # t is in units of |d|
        scaled = ray.copy()
        scaled[0, 3:] *= f32(s)
        assert R.cast_rays(SQUARE, SQUARE_T, scaled)["t"][0] == f32(1.0 / s)
    back = np.array([[0.25, 0.25, 1, 0, 0, 1], [0.25, 0.25, -1, 0, 0, 1]], dtype=f32)  # behind the origin: t < 0 is no hit; two-sided
    assert R.cast_rays(SQUARE, SQUARE_T, back)["triangle"].tolist() == [-1, 0]
    in_plane = np.array([[-1, 0.25, 0, 1, 0, 0], [0.25, 0.25, 0, 1, 1, 0]], dtype=f32)  # det = 0
    assert R.cast_rays(SQUARE, SQUARE_T, in_plane)["triangle"].tolist() == [-1, -1]
    bad = adversarial_rays()[-5:]
    assert not R.is_ray(bad).any()
    out = R.cast_rays(SQUARE, SQUARE_T, bad)
    assert (out["triangle"] == -1).all() and np.isinf(out["t"]).all() and np.isnan(out["uv"]).all() and not out["hit"].any()
    neg_zero = np.array([[0.25, 0.25, 0, 0, 0, -1]], dtype=f32)                         # t = -0 is canonicalised to +0 and counts
    out = R.cast_rays(SQUARE, SQUARE_T, neg_zero)
    assert out["triangle"][0] == 0 and out["t"].view(np.uint32)[0] == 0
    nothing = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [np.nan, 0, 0]], dtype=f32)    # no area, not finite: never hit
    assert R.cast_rays(nothing, np.array([[0, 1, 2], [0, 1, 3]], np.int32), ray)["triangle"][0] == -1
    assert R.guard_of(nothing, np.array([[0, 1, 2]], np.int32)) is None and R.guard_of(SQUARE, SQUARE_T) == f32(2.0 ** -15)


def test_pinhole_rays_and_visibility_by_hand():
    pose = np.eye(4, dtype=f32)[None]
    rays = R.rays_pinhole(pose, 10.0, 10.0, 3.5, 2.5, 6, 8)
    assert rays.shape == (1, 6, 8, 6) and (rays[..., :3] == 0).all() and (rays[..., 5] == 1).all()
    assert rays[0, 2, 3, 3] == f32(-0.05) and rays[0, 5, 7, 4] == f32(0.25)
    moved = pose.copy()
    moved[0, :3, 3] = [0, 0, 2]                                            # the camera at z = -2 looking along +z
    assert R.rays_pinhole(moved, 10.0, 10.0, 3.5, 2.5, 6, 8)[0, 0, 0, :3].tolist() == [0, 0, -2]
    # two quads: the near one z = 1 covers x, y in [-0.2, 0.2], the far one z = 2 covers [-1, 1]; camera at the origin
    v, t = two_quads()
    pts = np.array([[0.05, 0.02, 2.0], [0.3, 0.3, 2.0], [0.9, 0.0, 1.9], [0.1, 0.1, 1.0005], [0.0, 0.0, 5.0], [5.0, 0.0, 2.0], [0, 0, -2.0]], dtype=f32)
    cam = dict(fx=20.0, fy=20.0, cx=31.5, cy=31.5, H=64, W=64, z_near=0.1, z_far=4.0)
    count = R.visibility(pts, v, t, pose, tolerance=1e-3, **cam)
    #   two in the near quad's shadow (|x|, |y| <= 0.4 at z = 2) | lit | just behind the near quad | beyond z_far | outside the image | behind
    assert count.tolist() == [0, 0, 1, 1, 0, 0, 0]
    assert R.visibility(pts, v, t, pose, tolerance=0.0, **cam).tolist() == [0, 0, 1, 0, 0, 0, 0]      # without it a surface hides what lies on it
    side = np.array([[[1, 0, 0, -0.8], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=f32)         # a camera at x = 0.8
    assert R.visibility(pts, v, t, np.concatenate([pose, side]), tolerance=1e-3, **cam).tolist() == [1, 1, 2, 2, 0, 0, 0]


def two_quads():
    def quad(s, z):
        return [[-s, -s, z], [s, -s, z], [-s, s, z], [s, s, z]]
    v = np.array(quad(0.2, 1.0) + quad(1.0, 2.0), dtype=f32)
    return v, np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6], [5, 7, 6]], dtype=np.int32)


# ---------------------------------------------------------------- the walk
_BRUTE = {}


def lattice_truth(window):
    if window not in _BRUTE:
        v, t = lattice_mesh()
        _BRUTE[window] = R.cast_rays(v, t, adversarial_rays(), *window)
    return _BRUTE[window]


@pytest.mark.parametrize("cell", [0.125, 0.3, 2.5])
def test_the_twins_walk_equals_its_brute_force_on_adversarial_rays(cell):
    v, t = lattice_mesh()
    G, guard = R.grid_for(v, t, cell), R.guard_of(v, t)
    assert 2 * float(guard) <= float(G.margin) and G.dims == ((9, 9, 9) if cell == 0.125 else (4, 4, 4) if cell == 0.3 else (1, 1, 1))
    rays = adversarial_rays()
    cells = 0
    for w, window in enumerate(WINDOWS):
        want = lattice_truth(window)
        for i in range(0, len(rays), (1 if w == 0 else 3) * (1 if cell == 0.125 else 4)):        # (a cell of many triangles is slow in numpy)
            best, tri, hit, visited, steps = R.walk(G, rays[i], *window, guard)
            assert (tri, f32(best).view(np.uint32)) == (want["triangle"][i], want["t"][i:i + 1].view(np.uint32)[0]), (window, i, rays[i])
            assert R.walk(G, rays[i], *window, guard, any_hit=True)[2] == want["hit"][i] == hit
            assert steps <= max(G.dims) + 1
            cells += len(visited) if w == 0 else 0
    full = lattice_truth(WINDOWS[0])
    assert (full["triangle"] >= 0).sum() > 100 and (full["triangle"] == -1).sum() > 40
    if cell == 0.125:                                                       # the walk stops: 9.6 of the grid's 729 cells per ray of the open window
        assert cells / len(rays) < 20


def test_exact_ties_on_shared_edges_go_to_the_lower_index_in_both_orders():
    v, t = lattice_mesh()
    rays = np.array([[0.25, 0.25, 1.5, 0, 0, -1], [0.3125, 0.3125, 1.5, 0, 0, -1], [2, 0.25, 0.5, -1, 0, 0]], dtype=f32)
    for tri in (t, t[::-1].copy()):
        out = R.cast_rays(v, tri, rays)
        assert out["t"].tolist() == [0.75, 0.75, 1.5]
        G = R.grid_for(v, tri, 0.125)
        for i, ray in enumerate(rays):
            a, b, c, _ = R.Q.corners(v, tri)
            hits = [k for k in range(len(tri)) if R.ray_triangle(a[k], b[k], c[k], ray[:3], ray[3:], 0, np.inf, R.guard_of(v, tri))[0]
                    and R.ray_triangle(a[k], b[k], c[k], ray[:3], ray[3:], 0, np.inf, 0)[1] == out["t"][i]]
            assert len(hits) >= 2 and out["triangle"][i] == min(hits)
            assert R.walk(G, ray, 0, np.inf, R.guard_of(v, tri))[1] == min(hits)


# ---------------------------------------------------------------- the twin against float64
def _bary_f64(a, b, c, o, d):
    a, b, c, o, d = (np.asarray(x, dtype=np.float64) for x in (a, b, c, o, d))
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    s = o - a
    u = (s * p).sum(-1) / det
    v = (d * np.cross(s, e1)).sum(-1) / det
    return np.minimum(np.minimum(u, v), 1 - u - v)


def edge_rays(v, t, n=150, seed=4):
    """rays from outside the mesh aimed exactly at n of its vertices and at n of its edges' midpoints"""
    rs = np.random.RandomState(seed)
    tri = t[rs.randint(0, len(t), n)]
    target = np.concatenate([v[tri[:, 0]], (v[tri[:, 0]].astype(np.float64) + v[tri[:, 1]]) / 2])
    o = v.max(0) * 1.5 + rs.uniform(0, 1, (2 * n, 3))
    return np.concatenate([o, target - o], 1).astype(f32)


def float64_figures(name):
    """-> (K, band, n both hit the same triangle, n disagreements) of the twin against float64 on mesh `name`"""
    m = C.mesh(name)
    v, t = m["vertices"], m["triangles"]
    rays = np.concatenate([mesh_rays(v), edge_rays(v, t)])
    twin, ref = R.cast_rays(v, t, rays), R.cast_rays_f64(v, t, rays)
    guard = R.guard_of(v, t)
    scale = float(np.abs(v).max())
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    norm = np.linalg.norm(d, axis=1)

    def bound(i, tri):
        """2^-23 (t |d| + scale) / |cos| of ray i on triangle tri: the length a rounding of the coordinates moves the hit along the ray"""
        a, b, c = (v[t[tri, k]].astype(np.float64) for k in range(3))
        n = np.cross(b - a, c - a)
        cos = abs((n * d[i]).sum()) / (np.linalg.norm(n) * norm[i])
        return ULP * (ref["t"][i] * norm[i] + scale) / cos

    K = band = 0.0
    same = np.flatnonzero((twin["triangle"] == ref["triangle"]) & (twin["triangle"] >= 0))
    for i in same:
        K = max(K, abs(float(twin["t"][i]) - ref["t"][i]) * norm[i] / bound(i, twin["triangle"][i]))
    differ = np.flatnonzero(twin["triangle"] != ref["triangle"])
    for i in differ:
        mine, theirs = int(twin["triangle"][i]), int(ref["triangle"][i])
        if mine >= 0:                                                       # float64 misses the twin's triangle: by how much
            band = max(band, max(0.0, -float(_bary_f64(v[t[mine, 0]], v[t[mine, 1]], v[t[mine, 2]], o[i], d[i]))))
        if theirs >= 0:
            a, b, c = (v[t[theirs, k]] for k in range(3))
            hit, tt, _, _ = R.ray_triangle(a, b, c, rays[i, :3], rays[i, 3:], 0, np.inf, guard)
            if not hit:                                                     # the twin misses float64's triangle: how far inside the hit was
                band = max(band, float(_bary_f64(a, b, c, o[i], d[i])))
            else:                                                           # both hit both: the two t differ by rounding only
                K = max(K, abs(float(tt) - ref["t"][i]) * norm[i] / bound(i, theirs))
    return K, band, len(same), len(differ)


def test_twin_against_float64():
    """hit / miss and the triangle agree except within MEASURED_BAND of an edge, and |t - t64| |d| <= K 2^-23 (t |d| + scale) / |cos|,
    cos the angle of the ray with the triangle's normal"""
    worst_k = worst_band = 0.0
    for name in ("sphere", "noise"):
        K, band, n_same, n_differ = float64_figures(name)
        print(f"{name}: K = {K:.3f}, band = {band:.3e}, {n_same} rays hit the same triangle, {n_differ} differ")
        assert n_same > 300 and n_differ <= 150                              # (300 of the rays are aimed at edges and vertices)
        worst_k, worst_band = max(worst_k, K), max(worst_band, band)
    assert worst_k <= MEASURED_K * FACTOR and worst_band <= MEASURED_BAND * FACTOR


# ---------------------------------------------------------------- the entry points without a GPU
def test_ray_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == _lib.ABI_VERSION == 10                 # additions only
    one, inf, nan = ctypes.c_void_p(16), float("inf"), float("nan")
    mesh = (one, 3, one, 1)
    ok = dict(rays=one, n=1, mode=0, tnear=0.0, tfar=inf, guard=0.0, t=one, tri=one, uv=None, normal=None, hit=None, flag=one)

    def brute(**kw):
        a = {**ok, **kw}
        return lib.sgam_mesh_raycast_brute_f32(*a.get("mesh", mesh), a["rays"], a["n"], a["mode"], a["tnear"], a["tfar"], a["guard"], a["t"], a["tri"],
                                               a["uv"], a["normal"], a["hit"], a["flag"], None)

    grid_args = dict(entries=4, grid=(0.0, 0.0, 0.0, 1.0, 2, 2, 2), ws=one, bytes=1 << 20)

    def grid(**kw):
        a = {**ok, **grid_args, **kw}
        return lib.sgam_mesh_raycast_grid_f32(a["rays"], a["n"], a["entries"], *a["grid"], a["ws"], a["bytes"], a["mode"], a["tnear"], a["tfar"],
                                              a["guard"], a["t"], a["tri"], a["uv"], a["normal"], a["hit"], a["flag"], None)

    for call in (brute, grid):
        for bad in (dict(rays=None), dict(n=0), dict(mode=2), dict(mode=-1), dict(tnear=-1.0), dict(tnear=nan), dict(tnear=inf), dict(tfar=nan),
                    dict(tnear=2.0, tfar=1.0), dict(guard=-1.0), dict(guard=nan), dict(guard=inf), dict(t=None), dict(tri=None), dict(flag=None),
                    dict(mode=1)):                                          # mode 1 without hit_out
            assert call(**bad) == -1, (call.__name__, bad)
    assert brute(mesh=(None, 3, one, 1)) == -1 and brute(mesh=(one, 3, one, 0)) == -1 and brute(mesh=(one, 0, one, 1)) == -1
    assert brute(mesh=(one, 3, one, (1 << 28) + 1)) == -1
    # the grid: sizes, workspace, and a guard above half the margin (2^-14 * (2 + 2) here)
    for bad in (dict(grid=(0.0, 0.0, 0.0, 0.0, 2, 2, 2)), dict(grid=(0.0, 0.0, 0.0, 1.0, 0, 2, 2)), dict(ws=None), dict(bytes=8), dict(ws=ctypes.c_void_p(24)),
                dict(entries=0), dict(guard=2.0 ** -14 * 4)):
        assert grid(**bad) == -1, bad
    cam = (10.0, 10.0, 4.0, 4.0, 8, 8, 0.1, 4.0, 1e-3, 0.0)

    def vis_brute(points=one, n=1, poses=one, p=1, cam=cam, count=one, flag=one, mesh=mesh):
        return lib.sgam_mesh_visibility_brute_f32(*mesh, points, n, poses, p, *cam, count, flag, None)

    def vis_grid(points=one, n=1, poses=one, p=1, cam=cam, count=one, flag=one, entries=4, grid=(0.0, 0.0, 0.0, 1.0, 2, 2, 2), ws=one, nbytes=1 << 20):
        return lib.sgam_mesh_visibility_grid_f32(points, n, poses, p, *cam, entries, *grid, ws, nbytes, count, flag, None)

    def with_cam(k, value):
        return cam[:k] + (value,) + cam[k + 1:]

    for call in (vis_brute, vis_grid):
        for bad in (dict(points=None), dict(n=0), dict(poses=None), dict(p=0), dict(count=None), dict(flag=None), dict(cam=with_cam(0, 0.0)),
                    dict(cam=with_cam(1, nan)), dict(cam=with_cam(2, inf)), dict(cam=with_cam(4, 0)), dict(cam=with_cam(5, -1)), dict(cam=with_cam(6, 0.0)),
                    dict(cam=with_cam(7, 0.05)), dict(cam=with_cam(7, inf)), dict(cam=with_cam(8, -0.1)), dict(cam=with_cam(8, 1.5)), dict(cam=with_cam(8, nan)),
                    dict(cam=with_cam(9, -1.0))):
            assert call(**bad) == -1, (call.__name__, bad)
    assert vis_brute(mesh=(one, 3, None, 1)) == -1 and vis_grid(ws=None) == -1 and vis_grid(nbytes=8) == -1 and vis_grid(cam=with_cam(9, 1.0)) == -1
    assert lib.sgam_rays_pinhole_f32(None, 1, 10.0, 10.0, 4.0, 4.0, 8, 8, one, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 1, 10.0, 10.0, 4.0, 4.0, 8, 8, None, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 0, 10.0, 10.0, 4.0, 4.0, 8, 8, one, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 1, 0.0, 10.0, 4.0, 4.0, 8, 8, one, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 1, 10.0, 10.0, nan, 4.0, 8, 8, one, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 1, 10.0, 10.0, 4.0, 4.0, 0, 8, one, None) == -1
    assert lib.sgam_rays_pinhole_f32(one, 1 << 12, 10.0, 10.0, 4.0, 4.0, 1 << 10, 1 << 10, one, None) == -1        # P * H * W = 2^32


def test_python_api_refuses_host_tensors_and_bad_arguments():
    import torch
    from sgam_neurips22_amd import meshops
    from sgam_neurips22_amd.ops import SgamHipError
    from sgam_neurips22_amd.tsdf import DeviceMesh
    v, t = torch.from_numpy(SQUARE), torch.from_numpy(SQUARE_T)
    mesh = DeviceMesh(v, None, t, torch.tensor([4, 2, 0, 0], dtype=torch.int32), 4, 2)
    rays = torch.zeros((3, 6))
    for call in (lambda: meshops.cast_rays(rays, mesh), lambda: meshops.test_occlusions(rays, mesh, method="brute"),
                 lambda: meshops.visible_points(rays[:, :3], mesh, np.eye(4)[None], np.eye(3), 4, 4, 0.1, 1.0)):
        with pytest.raises(SgamHipError):
            call()
    with pytest.raises(ValueError):
        meshops.cast_rays(rays, mesh, method="bvh")
    with pytest.raises(ValueError):
        meshops.cast_rays(rays, mesh, method="brute", cell_size=0.1)
    assert getattr(meshops.test_occlusions, "__test__") is False
