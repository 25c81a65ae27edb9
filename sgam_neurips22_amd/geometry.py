"""Geometry metrics between point clouds on the device (csrc/point_nn.hip): exact nearest neighbours — brute force or a uniform
grid, the same bits either way — chamfer distance, accuracy / completeness, precision / recall / F-score at a distance threshold,
and the frame store unprojected into one cloud.  Device tensors in, device tensors (or plain floats) out; nothing is pulled to the
host but a bounding box (six floats) and the per-block sums.  `InfiniteSceneGeneration.merged_point_cloud()` /
`.geometry_metrics()` are the scene-level callers.  On top of the same search: the k nearest neighbours (`knn`, k <= 32), uniform
voxel sampling (`voxel_sample`), the statistical outlier rule (`statistical_outliers`) and normals (`estimate_normals`) — the
clean-up `merged_point_cloud(voxel_size=..., nb_neighbors=..., normals=True)` runs (csrc/point_cloud.hip), in the
one order `prepare_cloud` gives every cloud that is cleaned or registered.  And the
rigid registration of two clouds on the search and the normals: `register_icp`, `evaluate_registration`, `transform_points`
(csrc/point_icp.hip), which `geometry_metrics(align=...)` and `frame_drift()` run — with estimation "colored"
(`color_gradients`) also on the clouds' colours, where a plane leaves the geometry's pose free, and coarse to fine
(`register_icp_multiscale`).  ICP needs a pose to start from; for two clouds that share no frame of reference
`register_global` finds one: FPFH features (`fpfh`), their nearest neighbours (`match_features`) and RANSAC over the feature
correspondences (`register_ransac`), csrc/point_global.hip, which `geometry_metrics(align={"init": "global", ...})` runs.
Many clouds at once: `multiway_registration` registers them pair by pair into a `PoseGraph`, and `optimize_pose_graph` solves for
one consistent pose per cloud on the device (csrc/pose_graph.hip), which `scene.optimize_poses()` runs.
Agreement in the image rather than between clouds: `view_consistency` puts the pixels of one frame into the camera of another
and classifies them against what that frame holds (csrc/view_consistency.hip); `consistency_summary` reads it.
And the step that minimises that image error: `rgbd_odometry` refines the poses of many frame pairs in lock step on an image
pyramid (`rgbd_pyramid`), and `multiway_rgbd` builds the pose graph from one batched call (csrc/rgbd_odometry.hip).
What is IN a cloud: `radius_count`, `cluster_dbscan`, `segment_plane` / `segment_planes`, `cluster_boxes` and `segment_cloud`, which
`scene.segment()` runs (csrc/point_segment.hip).

A point with a coordinate that is not finite (NaN: what `unproject_frames` writes for an invalid depth) is "not a point": it is
never a neighbour, has none itself, and is left out of every mean and count.  No gradients.

There is no CPU fallback: an input that is not on the device raises `SgamHipError`."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .ops import SgamHipError, _need_cuda, _p, _stream, check

GRID_OCCUPANCY = 2.0             # target mean number of reference points per cell of the default grid
GRID_MAX_CELLS = 1 << 24         # the library's cell cap: 2 x 64 MB of cell tables next to 16 B per reference point
# reference-set size from which method="auto" builds a grid: the measured crossover of the two kernels with as many queries as
# reference points (scripts/geometry_time.py, table in DESIGN §4.4.4: brute force wins at 4096, the grid from 16384 on)
AUTO_GRID_MIN_REF = 16384
KNN_MAX_K = 32                   # the k-NN kernels keep a lane's list of k (d2, index) keys in LDS: compiled for 8 / 16 / 32 slots
# reference-set size from which knn(method="auto") builds a grid: the measured crossover of the two k-NN kernels with the cloud as
# its own query set (scripts/cloud_time.py, table in DESIGN §4.4.5: at 512 points brute force still wins at k = 8 and loses at
# k = 16 / 32; from 1024 on the grid, build included, wins at every k measured).  Lower than AUTO_GRID_MIN_REF: the insertions
# make every pair of the brute-force search dearer, and the grid visits few pairs.
AUTO_KNN_GRID_MIN_REF = 1024
VOXEL_MAX_EXTENT = 1 << 20       # voxels along an axis, either side of the origin: the voxel key packs 3 x 21 bits biased by 2^20


def _f32(v):
    return float(np.float32(v))


def max_d2_of(max_distance):
    """the fp32 number the kernels compare d2 with: fp32(max_distance) squared in fp32; None -> +inf"""
    if max_distance is None:
        return math.inf
    m = np.float32(max_distance)
    if not m >= 0:
        raise ValueError(f"max_distance must be >= 0, not {max_distance!r}")
    return float(m * m)


def default_cell_size(lo, hi, n):
    """cell edge of the default grid over the box [lo, hi] of n valid points: the cube root of (box volume * GRID_OCCUPANCY / n),
    an axis thinner than 1/1000 of the longest counted as that (a planar or collinear cloud still gets cells of a useful size),
    and never below 2^-10 of the coordinate scale (the stop rule's safety margin is 2^-16 of it).  A box without extent: 1."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    e = hi - lo
    emax = float(e.max())
    if not emax > 0:
        return 1.0
    scale = max(float(np.abs(lo).max()), float(np.abs(hi).max()), emax)
    h = (float(np.prod(np.maximum(e, emax * 1e-3))) * GRID_OCCUPANCY / max(int(n), 1)) ** (1.0 / 3.0)
    return max(h, scale * 2.0 ** -10)


def positive_edge(name, given, default=None):
    """the cell or voxel edge `given` (`default` where it is None) as a float of fp32 precision; ValueError unless it is positive
    and finite in fp32"""
    h = np.float32(default if given is None else given)
    if not (h > 0 and np.isfinite(h)):
        raise ValueError(f"{name} must be positive and finite, not {given!r}")
    return float(h)


def grid_for(lo, hi, n, cell_size=None):
    """(origin fp32[3], cell edge fp32, (gx, gy, gz)) of the grid over the box [lo, hi]: g = floor(extent / h) + 1 per axis, the
    edge grown by a quarter until the grid fits GRID_MAX_CELLS cells"""
    lo32, hi32 = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
    h = positive_edge("cell_size", cell_size, default_cell_size(lo, hi, n) if cell_size is None else None)
    while True:
        g = np.floor((hi - lo) / h) + 1.0
        if float(np.prod(g)) <= GRID_MAX_CELLS:
            return lo32, float(np.float32(h)), tuple(int(v) for v in g)
        h = float(np.float32(h * 1.25))


def _clouds(query, ref):
    _need_cuda(query, ref)
    if query.dim() not in (2, 3) or query.dim() != ref.dim() or query.shape[-1] != 3 or ref.shape[-1] != 3:
        raise ValueError(f"point clouds are (N,3) or (B,N,3): got {tuple(query.shape)} and {tuple(ref.shape)}")
    if query.dtype != torch.float32 or ref.dtype != torch.float32:
        raise ValueError("point clouds are fp32")
    q = query.contiguous().reshape(-1, query.shape[-2], 3) if query.dim() == 3 else query.contiguous()[None]
    r = ref.contiguous().reshape(-1, ref.shape[-2], 3) if ref.dim() == 3 else ref.contiguous()[None]
    if q.shape[0] != r.shape[0] or q.shape[1] < 1 or r.shape[1] < 1 or q.shape[0] < 1:
        raise ValueError(f"point clouds need the same batch size and at least one point each: {tuple(query.shape)}, {tuple(ref.shape)}")
    _one_device(q, r)
    return q, r


def _one_device(*tensors, text="point clouds live on one device"):
    """the tensors (None: skipped) are on the GPU, all of them on one device"""
    _need_cuda(*tensors)
    devices = {t.device for t in tensors if t is not None}
    if len(devices) > 1:
        raise ValueError(text)


_DTYPES = {torch.float32: "fp32", torch.float64: "fp64", torch.int32: "int32", torch.uint8: "uint8"}


def _tensor_of(t, shape, dtype, what, name, verb="are"):
    """`t` contiguous if it is a tensor of `shape` and `dtype`, ValueError "what: name are (shape) dtype, not <what it is>" if not.  An
    entry of `shape` that is a letter stands for any size from 1 on."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != len(shape) or \
            any(g < 1 if isinstance(s, str) else g != s for s, g in zip(shape, t.shape)):
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
        want = ",".join(str(s) for s in shape) + ("," if len(shape) == 1 else "")
        raise ValueError(f"{what}: {name} {verb} ({want}) {_DTYPES[dtype]}, not {got}")
    return t.contiguous()


def _integer(name, v, lo, hi, what=None, rule=None):
    """v as an int; ValueError unless it is an integer (no bool) in lo..hi"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what + ': ' if what else ''}{name} is {rule or f'an integer in {lo}..{hi}'}, not {v!r}")
    return int(v)


def valid_box(points):
    """(box (2,3) fp32 numpy: minimum and maximum corner of the valid points, number of valid points): torch reductions as
    plumbing, six floats to the host"""
    valid = torch.isfinite(points).all(dim=1, keepdim=True)
    inf = torch.tensor(math.inf, device=points.device)
    box = torch.stack([torch.where(valid, points, inf).amin(0), torch.where(valid, points, -inf).amax(0)]).cpu().numpy()
    return box, int(valid.sum().item())


def workspace(fn, device, *args):
    """(uninitialised device memory, 16-byte aligned, for a library call that carves its tables out of it, its bytes = fn(*args))"""
    nbytes = int(getattr(_lib.load(), fn)(*args))
    if nbytes < 0:
        check(nbytes, fn)
    return torch.empty(((nbytes + 15) // 16, 2), dtype=torch.int64, device=device), nbytes


def _block_sums(fn, C, x, *args):
    """the library's chunk reduction `fn` (C sums per block) on a flat device tensor -> (C,) numpy: per-block fp64 partials on the
    device, folded on the host like the loss partials of the training step"""
    lib = _lib.load()
    n = int(x.numel())
    part = torch.empty((int(getattr(lib, fn + "_partials")(n)) // C, C), dtype=torch.float64, device=x.device)
    check(getattr(lib, fn)(_p(x), n, *args, _p(part), _stream()), fn)
    return part.cpu().numpy().sum(axis=0)


def check_method(method, what):
    if method not in ("auto", "brute", "grid"):
        raise ValueError(f"{what}: method 'auto', 'brute' or 'grid', not {method!r}")


def search_method(method, cell_size, n, auto_grid_min, what):
    """"brute" or "grid" for a search over n reference items: "auto" is the grid from auto_grid_min items on (the caller's measured
    crossover); cell_size belongs to the grid"""
    check_method(method, what)
    if method == "auto":
        method = "grid" if n >= auto_grid_min else "brute"
    if method == "brute" and cell_size is not None:
        raise ValueError(f"{what}: cell_size belongs to method='grid'")
    return method


def answers(shape, device, index="index", closest=False):
    """the buffers a search writes: {"d2" fp32, `index` int32 [, "closest" fp32 (..., 3)]}, uninitialised"""
    out = {"d2": torch.empty(shape, dtype=torch.float32, device=device), index: torch.empty(shape, dtype=torch.int32, device=device)}
    if closest:
        out["closest"] = torch.empty((*shape, 3), dtype=torch.float32, device=device)
    return out


def check_voxel_overflow(flag, fn):
    """the voxel table's int32 overflow flag after `fn`; synchronises"""
    if int(flag.item()):
        raise SgamHipError(f"{fn}: the voxel table overflowed (a point found no slot)")


class PointGrid:
    """the reference set of one cloud sorted into a uniform grid (sgam_points_grid_build); query() as often as needed"""

    def __init__(self, ref, cell_size=None):
        _need_cuda(ref)
        if ref.dim() != 2 or ref.shape[1] != 3 or ref.dtype != torch.float32 or ref.shape[0] < 1:
            raise ValueError(f"PointGrid: an (N,3) fp32 cloud, not {tuple(ref.shape)} {ref.dtype}")
        self.ref = ref.contiguous()
        self.n = int(ref.shape[0])
        box, n_valid = valid_box(self.ref)
        if n_valid == 0:                          # nothing to find: one empty cell, the query kernel answers -1 / +inf
            box = np.zeros((2, 3), dtype=np.float32)
        self.n_valid = n_valid
        self.origin, self.cell_size, self.dims = grid_for(box[0], box[1], max(n_valid, 1), cell_size)
        self.workspace, self.bytes = workspace("sgam_points_grid_workspace_bytes", ref.device, self.n, *self.dims)
        # what the build and every query pass the library: the reference count, the grid, its tables
        self._args = (self.n, *(float(o) for o in self.origin), self.cell_size, *self.dims, _p(self.workspace), self.bytes)
        check(_lib.load().sgam_points_grid_build(_p(self.ref), *self._args, _stream()), "sgam_points_grid_build")

    def query(self, query, max_distance=None, out=None):
        """query (Nq,3) fp32 on the grid's device -> {"d2" (Nq,) fp32, "index" (Nq,) int32}"""
        q = query.contiguous()
        nq = int(q.shape[0])
        out = answers((nq,), q.device) if out is None else out
        check(_lib.load().sgam_points_nn_grid_f32(_p(q), nq, *self._args, max_d2_of(max_distance), _p(out["d2"]), _p(out["index"]),
                                                  _stream()), "sgam_points_nn_grid_f32")
        return {"d2": out["d2"], "index": out["index"]}

    def query_knn(self, query, k, max_distance=None, exclude_self=False, out=None):
        """query (Nq,3) fp32 on the grid's device -> {"d2" (Nq,k) fp32, "index" (Nq,k) int32}: knn()'s rows (sgam_points_knn_grid_f32)"""
        k = _check_k(k)
        q = query.contiguous()
        nq = int(q.shape[0])
        if exclude_self and nq != self.n:
            raise ValueError(f"query_knn: exclude_self needs the grid's own cloud as the query ({nq} queries, {self.n} reference points)")
        out = answers((nq, k), q.device) if out is None else out
        check(_lib.load().sgam_points_knn_grid_f32(_p(q), nq, *self._args, k, max_d2_of(max_distance), int(bool(exclude_self)),
                                                   _p(out["d2"]), _p(out["index"]), _stream()), "sgam_points_knn_grid_f32")
        return {"d2": out["d2"], "index": out["index"]}


def nearest_neighbors(query, ref, method="auto", max_distance=None, cell_size=None):
    """For every query point the nearest reference point.  query (Nq,3) / ref (Nr,3), or (B,Nq,3) / (B,Nr,3) independent clouds;
    fp32 device tensors.  Returns {"d2": squared distance, fp32, "index": int32}, shaped (Nq,) or (B,Nq).
        d2 = (dx * dx + dy * dy) + dz * dz in fp32; an exact tie goes to the lower reference index
        a query that is not a point, or a cloud without a valid reference point: index -1, d2 +inf
        max_distance: reference points farther than it (d2 > fp32(max_distance)^2) count as no neighbour
    method "brute": every pair (sgam_points_nn_brute_f32, batched in one launch); "grid": a uniform grid over the reference box,
    searched in growing shells (sgam_points_grid_build + sgam_points_nn_grid_f32, one batch item at a time); "auto": the grid from
    AUTO_GRID_MIN_REF reference points on.  The two give the same bits; cell_size (grid only) changes the speed, not the result."""
    q, r = _clouds(query, ref)
    B, nq, nr = int(q.shape[0]), int(q.shape[1]), int(r.shape[1])
    method = search_method(method, cell_size, nr, AUTO_GRID_MIN_REF, "nearest_neighbors")
    d2, idx = answers((B, nq), q.device).values()
    if method == "brute":
        for b0 in range(0, B, 65535):
            _nn_brute(q[b0:], r[b0:], min(65535, B - b0), max_d2_of(max_distance), d2[b0:], idx[b0:])
    else:
        for b in range(B):
            PointGrid(r[b], cell_size).query(q[b], max_distance, out={"d2": d2[b], "index": idx[b]})
    if query.dim() == 2:
        return {"d2": d2[0], "index": idx[0]}
    return {"d2": d2.reshape(query.shape[:-1]), "index": idx.reshape(query.shape[:-1])}


def _nn_brute(q, r, B, max_d2, d2, index):
    """one launch of the brute-force search over B clouds of q (.., Nq, 3) against r (.., Nr, 3), contiguous from their first item on"""
    check(_lib.load().sgam_points_nn_brute_f32(_p(q), _p(r), B, int(q.shape[-2]), int(r.shape[-2]), max_d2, _p(d2), _p(index), _stream()),
          "sgam_points_nn_brute_f32")


class BruteForce:
    """PointGrid's counterpart without a structure: the reference set as it is, every pair looked at; the same answers"""

    def __init__(self, ref):
        _need_cuda(ref)
        self.ref, self.n = ref.contiguous(), int(ref.shape[0])

    def query(self, query, max_distance=None, out=None):
        q = query.contiguous()
        out = answers((int(q.shape[0]),), q.device) if out is None else out
        _nn_brute(q, self.ref, 1, max_d2_of(max_distance), out["d2"], out["index"])
        return {"d2": out["d2"], "index": out["index"]}

    def query_knn(self, query, k, max_distance=None, exclude_self=False, out=None):
        k = _check_k(k)
        q = query.contiguous()
        nq = int(q.shape[0])
        out = answers((nq, k), q.device) if out is None else out
        check(_lib.load().sgam_points_knn_brute_f32(_p(q), _p(self.ref), nq, self.n, k, max_d2_of(max_distance), int(bool(exclude_self)),
                                                    _p(out["d2"]), _p(out["index"]), _stream()), "sgam_points_knn_brute_f32")
        return {"d2": out["d2"], "index": out["index"]}


def search_structure(ref, method, cell_size, auto_grid_min, what):
    """the object that answers query() / query_knn() over the cloud ref: a PointGrid or BruteForce, by search_method's rule"""
    method = search_method(method, cell_size, int(ref.shape[0]), auto_grid_min, what)
    return PointGrid(ref, cell_size) if method == "grid" else BruteForce(ref)


def _check_k(k):
    return _integer("k", k, 1, KNN_MAX_K)


def _one_cloud(points, what):
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or points.shape[0] < 1:
        raise ValueError(f"{what}: an (N,3) fp32 cloud with at least one point, not {tuple(points.shape)} {points.dtype}")
    return int(points.shape[0])


def knn(query, ref, k, method="auto", max_distance=None, exclude_self=False, cell_size=None):
    """For every query point its k nearest reference points.  query (Nq,3), ref (Nr,3) fp32 device tensors, 1 <= k <= KNN_MAX_K.
    Returns {"d2" (Nq,k) fp32, "index" (Nq,k) int32}: distance, candidates and order are nearest_neighbors' — a row is ascending in
    (d2 bits, index); candidates with d2 > fp32(max_distance)^2, NaN or +inf never enter; a row with fewer than k candidates ends
    in index -1 / d2 +inf (a query that is not a point: the whole row).  exclude_self: query and ref are the same cloud and the
    candidate whose index is the query's is skipped.  k = 1 gives nearest_neighbors' bits.  method "brute"
    (sgam_points_knn_brute_f32) / "grid" (PointGrid.query_knn) / "auto": the grid from AUTO_KNN_GRID_MIN_REF reference points on;
    the two give the same bits."""
    k = _check_k(k)
    nq, nr = _one_cloud(query, "knn"), _one_cloud(ref, "knn")
    if exclude_self and nq != nr:
        raise ValueError(f"knn: exclude_self needs query and ref to be the same cloud ({nq} queries, {nr} reference points)")
    method = search_method(method, cell_size, nr, AUTO_KNN_GRID_MIN_REF, "knn")
    max_d2_of(max_distance)
    _one_device(query, ref)
    return search_structure(ref, method, cell_size, AUTO_KNN_GRID_MIN_REF, "knn").query_knn(query, k, max_distance, exclude_self)


def voxel_grid_for(lo, hi, voxel_size, origin=None):
    """(origin fp32[3], voxel edge as a float of fp32 precision) of voxel_sample over the box [lo, hi] of the valid points: the
    origin defaults to the box's fp32 minimum corner.  ValueError where the box reaches VOXEL_MAX_EXTENT voxels or more from the
    origin along an axis (the voxel key has 21 bits per axis, biased by 2^20 so that a given origin may lie inside the box)."""
    h64 = positive_edge("voxel_size", voxel_size)
    lo32, hi32 = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
    o32 = lo32.copy() if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    if not np.isfinite(o32).all():
        raise ValueError(f"voxel_sample: the origin must be finite, not {origin!r}")
    o = o32.astype(np.float64)
    reach = max(float(np.abs(lo32.astype(np.float64) - o).max()), float(np.abs(hi32.astype(np.float64) - o).max()),
                float((hi32.astype(np.float64) - lo32.astype(np.float64)).max()))
    if not reach / h64 < VOXEL_MAX_EXTENT:
        raise ValueError(f"voxel_sample: the cloud spans {reach / h64:.3g} voxels of {h64:g} along an axis, the limit is 2^20")
    return o32, h64


def voxel_sample(points, voxel_size, origin=None):
    """Uniform voxel sampling (PCL's UniformSampling rule, not a mean): every occupied voxel of edge `voxel_size` keeps ONE of its
    points.  points (N,3) fp32 on the device -> {"index" (M,) int32 ascending: the kept points, "count" (M,) int32: the members
    of each kept point's voxel}.  Per axis in fp32: v = floorf((p - o) / voxel_size), centre c = o + (v + 0.5f) * voxel_size; kept:
    the member of least (d2(p, c) bits, index), so an exact tie goes to the lower index.  `origin` (3 floats) defaults to the fp32
    minimum corner of the valid points.  Points that are not points belong to no voxel.  (sgam_points_voxel_sample_f32: a hash
    table of voxel keys with integer atomics only; the result does not depend on the order of arrival.)"""
    n = _one_cloud(points, "voxel_sample")
    _need_cuda(points)
    p = points.contiguous()
    box, n_valid = valid_box(p)
    if n_valid == 0:
        positive_edge("voxel_size", voxel_size)
        empty =torch.empty((0,), dtype=torch.int32, device=p.device)
        return {"index": empty, "count": empty.clone()}
    o, h = voxel_grid_for(box[0], box[1], voxel_size, origin)
    ws, nbytes = workspace("sgam_points_voxel_workspace_bytes", p.device, n)
    keep = torch.empty((n,), dtype=torch.uint8, device=p.device)
    count = torch.empty((n,), dtype=torch.int32, device=p.device)
    flag = torch.zeros((1,), dtype=torch.int32, device=p.device)
    check(_lib.load().sgam_points_voxel_sample_f32(_p(p), n, float(o[0]), float(o[1]), float(o[2]), h, _p(ws), nbytes, _p(keep),
                                                   _p(count), _p(flag), _stream()), "sgam_points_voxel_sample_f32")
    index = torch.nonzero(keep).reshape(-1)                               # compaction: plumbing (ascending); synchronises
    check_voxel_overflow(flag, "sgam_points_voxel_sample_f32")
    return {"index": index.to(torch.int32), "count": count[index]}


def _md_sum(md, shift, squared):
    s = _block_sums("sgam_points_md_reduce", 2, md, float(shift), int(squared))
    return float(s[0]), int(s[1])


def statistical_outliers(points, nb_neighbors=20, std_ratio=2.0, method="auto"):
    """Open3D's `remove_statistical_outlier` rule as its documentation states it (unpinned against Open3D: DESIGN §4.4.5).
    points (N,3) fp32 on the device -> {"keep" (N,) bool, "mean_distance" (N,) fp64 (device tensors), "mean", "std", "threshold"
    (floats)}.  mean_distance_i = the mean of sqrt((double)d2) over the valid entries of row i of knn(points, points,
    nb_neighbors) — the point itself is among its neighbours — summed in ascending column order; mean and std over the points
    that are points, in two passes (sum md; sum (md - mean)^2, divisor n - 1; fewer than two points: std 0);
    threshold = mean + std_ratio * std; keep_i = mean_distance_i <= threshold.  A point that is not a point has mean distance NaN
    and is never kept."""
    n = _one_cloud(points, "statistical_outliers")
    k = _check_k(nb_neighbors)
    std_ratio = float(std_ratio)
    if not math.isfinite(std_ratio):
        raise ValueError(f"std_ratio must be finite, not {std_ratio!r}")
    p = points.contiguous()
    nn = knn(p, p, k, method=method)
    md = torch.empty((n,), dtype=torch.float64, device=p.device)
    check(_lib.load().sgam_points_knn_mean_distance(_p(nn["d2"]), _p(nn["index"]), n, k, _p(md), _stream()), "sgam_points_knn_mean_distance")
    total, count = _md_sum(md, 0.0, 0)
    mean = total / count if count else float("nan")
    std = 0.0
    if count > 1:
        ss, _ = _md_sum(md, mean, 1)
        std = math.sqrt(ss / (count - 1))
    threshold = mean + std_ratio * std
    return {"keep": md <= threshold, "mean_distance": md, "mean": mean, "std": std, "threshold": threshold}


def estimate_normals(points, k=16, viewpoints=None, view_of=None, method="auto"):
    """Normals of a cloud from the covariance of every point's k nearest neighbours (itself included).  points (N,3) fp32 on the
    device -> (N,3) fp32.  Centroid and 3x3 covariance in fp64 from the fp32 coordinates in ascending column order of the point's
    knn row, diagonalised by a cyclic Jacobi iteration with a fixed number of sweeps; the normal is the unit eigenvector of the
    least eigenvalue, rounded to fp32 once.  Fewer than 3 valid neighbours (and a point that is not a point): NaN.  Orientation:
    with viewpoints (V,3) fp32 and view_of (N,) int32 on the device, flipped so that n . (viewpoints[view_of] - p) >= 0;
    without, the component of largest magnitude is made positive (the lowest axis on a tie)."""
    n = _one_cloud(points, "estimate_normals")
    k = _check_k(k)
    if (viewpoints is None) != (view_of is None):
        raise ValueError("estimate_normals: viewpoints and view_of are given together")
    V = 0
    if viewpoints is not None:
        viewpoints = _tensor_of(viewpoints, ("V", 3), torch.float32, "estimate_normals", "viewpoints")
        view_of = _tensor_of(view_of, (n,), torch.int32, "estimate_normals", "view_of", "is")
        _need_cuda(viewpoints, view_of)
        V = int(viewpoints.shape[0])
    p = points.contiguous()
    nn = knn(p, p, k, method=method)
    out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    check(_lib.load().sgam_points_normals_f32(_p(p), n, _p(nn["index"]), k, _p(viewpoints), V, _p(view_of), _p(out), _stream()),
          "sgam_points_normals_f32")
    return out


def prepare_cloud(points, what, voxel_size=None, outliers=None, normal_k=None, viewpoints=None, view_of=None):
    """The preparation every registration (and merged_point_cloud's clean-up) gives a cloud, each step where its argument is given,
    in this order: the rows that are points; voxel_sample(voxel_size); statistical_outliers(*outliers): (nb_neighbors, std_ratio);
    estimate_normals(normal_k), towards viewpoints (V,3) fp32 where given with view_of (N,) int32 per row of the cloud AS GIVEN.
    points (N,3) fp32 on the device -> (points (M,3), index (M,) int64: the kept rows of the cloud as given, ascending — what
    a caller gathers its colours and per-point data through —, normals (M,3) or None; the outlier rule may leave M = 0)."""
    index = torch.nonzero(torch.isfinite(points).all(dim=1)).reshape(-1)
    if index.numel() < 1:
        raise ValueError(f"{what}: a cloud without a valid point cannot be registered")
    p = points[index].contiguous()
    if voxel_size is not None:
        pick = voxel_sample(p, voxel_size)["index"].long()
        p, index = p[pick].contiguous(), index[pick]
    if outliers is not None:
        keep = statistical_outliers(p, *outliers)["keep"]
        p, index = p[keep].contiguous(), index[keep]
    if normal_k is None:
        return p, index, None
    if not index.numel():
        return p, index, torch.empty((0, 3), dtype=torch.float32, device=p.device)
    if viewpoints is None:
        return p, index, estimate_normals(p, normal_k)
    view_of = _tensor_of(view_of, (int(points.shape[0]),), torch.int32, what, "view_of", "is")
    return p, index, estimate_normals(p, normal_k, viewpoints.contiguous(), view_of[index].contiguous())


# ---------------------------------------------------------------- rigid registration (csrc/point_icp.hip)
ICP_STATE, ICP_ROW, ICP_SLOTS = 24, 8, 32        # doubles of the device state, of a history row, of a chunk's sums (include/sgam_hip.h)
ICP_ESTIMATIONS = ("point_to_plane", "point_to_point", "colored")
LAMBDA_GEOMETRIC = 0.968         # Open3D's default weight of the geometric term of coloured ICP


def _pose(T, device, what):
    """a 4x4 pose as 16 fp64 on the device: numpy (or nested lists), or a device tensor; None -> the identity"""
    if T is None:
        return torch.eye(4, dtype=torch.float64, device=device)
    if isinstance(T, torch.Tensor):
        if tuple(T.shape) != (4, 4) or T.dtype != torch.float64:
            raise ValueError(f"{what}: a pose given as a tensor is (4,4) fp64, not {tuple(T.shape)} {T.dtype}")
        _need_cuda(T)
        return T.contiguous()
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{what}: a pose is 4x4, not {T.shape}")
    return torch.from_numpy(np.ascontiguousarray(T)).to(device)


def transform_points(points, T, out=None):
    """points (N,3) fp32 on the device moved by the 4x4 pose T (numpy, or a (4,4) fp64 device tensor: no host round trip) ->
    (N,3) fp32.  T[0..11] are rounded to fp32 once, then X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3] in fp32, the
    unprojection's expression; a point that is not a point stays NaN.  (sgam_points_transform_f32)"""
    n = _one_cloud(points, "transform_points")
    _need_cuda(points)
    p = points.contiguous()
    T = _pose(T, p.device, "transform_points")
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    check(_lib.load().sgam_points_transform_f32(_p(p), n, _p(T), _p(out), _stream()), "sgam_points_transform_f32")
    return out


def check_estimation(estimation, what):
    if estimation not in ICP_ESTIMATIONS:
        raise ValueError(f"{what}: estimation is one of {ICP_ESTIMATIONS}, not {estimation!r}")


def icp_state(init, device, what):
    """the 24 fp64 of the update kernel's device state, its pose [0..16) the pose `init` (_pose's forms; None: the identity)"""
    state = torch.zeros((ICP_STATE,), dtype=torch.float64, device=device)
    state[:16] = _pose(init, device, what).reshape(16)
    return state


def icp_partials(n, device, partials, what):
    """the (chunks, ICP_SLOTS) fp64 sums of n source points: a new buffer, or the caller's when it holds that many"""
    blocks = int(_lib.load().sgam_points_icp_partials(n)) // ICP_SLOTS
    if partials is None:
        return torch.empty((blocks, ICP_SLOTS), dtype=torch.float64, device=device)
    if partials.dtype != torch.float64 or partials.numel() != blocks * ICP_SLOTS or not partials.is_contiguous():
        raise ValueError(f"{what}: partials hold {blocks} x {ICP_SLOTS} fp64 for {n} points, not {tuple(partials.shape)} {partials.dtype}")
    return partials


def _colors_of(colors, n, what, name):
    """the uint8 (n,3) colours of a cloud of n points, contiguous"""
    if colors is None:
        raise ValueError(f"{what}: estimation 'colored' needs {name} (uint8, one colour per point)")
    return _tensor_of(colors, (n, 3), torch.uint8, what, name)


def _lambda_of(lambda_geometric, what):
    lam = float(lambda_geometric)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{what}: lambda_geometric is in [0, 1], not {lambda_geometric!r}")
    return lam


def _accumulate(what, moved, target, target_normals, index, d2, partials, colored=None):
    """the one body of icp_accumulate and, with colored = (source colours, target colours, target gradients, lambda_geometric), of
    icp_accumulate_colored"""
    n, nr = _one_cloud(moved, what), _one_cloud(target, what)
    if target_normals is not None or colored is not None:
        target_normals = _tensor_of(target_normals, (nr, 3), torch.float32, what, "target_normals")
    if colored is not None:
        gradients = _tensor_of(colored[2], (nr, 3), torch.float32, what, "target_gradients")
        sc, tc = _colors_of(colored[0], n, what, "source_colors"), _colors_of(colored[1], nr, what, "target_colors")
        lam = _lambda_of(colored[3], what)
    index, d2 = _tensor_of(index, (n,), torch.int32, what, "index", "is"), _tensor_of(d2, (n,), torch.float32, what, "d2", "is")
    partials = icp_partials(n, moved.device, partials, what)
    m, t = moved.contiguous(), target.contiguous()
    if colored is None:
        _need_cuda(m, t, target_normals, index, d2, partials)
        check(_lib.load().sgam_points_icp_accumulate(_p(m), _p(t), _p(target_normals), _p(index), _p(d2), n, nr, _p(partials), _stream()),
              "sgam_points_icp_accumulate")
    else:
        _need_cuda(m, sc, t, target_normals, tc, gradients, index, d2, partials)
        check(_lib.load().sgam_points_icp_accumulate_colored(_p(m), _p(sc), _p(t), _p(target_normals), _p(tc), _p(gradients), _p(index), _p(d2),
                                                             n, nr, lam, _p(partials), _stream()), "sgam_points_icp_accumulate_colored")
    return partials


def icp_accumulate(moved, target, target_normals, index, d2, partials=None):
    """sgam_points_icp_accumulate: the sums of one Gauss-Newton step over the correspondences (index, d2: the search's result for
    `moved` against `target`) -> partials (ceil(N / 4096), 32) fp64 on the device.  target_normals None: point-to-point."""
    return _accumulate("icp_accumulate", moved, target, target_normals, index, d2, partials)


def color_gradients(points, normals, colors, k=16, method="auto", knn_index=None):
    """The gradient of the colour intensity over a cloud's surface, what coloured ICP reads of its target (Park, Zhou, Koltun 2017;
    Open3D's registration_colored_icp as documented).  points (N,3) fp32, normals (N,3) fp32, colors (N,3) uint8 on the device ->
    (N,3) fp32.  Intensity I = (r + g + b) / 765.  Per point, over the valid entries of its row of knn(points, points, k,
    exclude_self=True) in ascending column order and in fp64: the neighbour projected into the tangent plane, u = e - (e . n) n
    with e = p_j - p; the least-squares fit of u . g = I_j - I_p together with the constraint m (n . g) = 0 (m neighbours), solved
    by a 3x3 Cholesky with the update kernel's pivot rule.  NaN where the point is not a point, its normal is not finite, it has
    fewer than 3 neighbours or they leave the gradient free (a collinear neighbourhood).  knn_index (N,k) int32 on the device:
    the rows to use in place of the search's (an entry outside [0, N) is skipped).  (sgam_points_color_gradient_f32)"""
    what = "color_gradients"
    n = _one_cloud(points, what)
    k = _check_k(k)
    nrm = _tensor_of(normals, (n, 3), torch.float32, what, "normals")
    colors = _colors_of(colors, n, what, "colors")
    check_method(method, what)
    if knn_index is not None:
        knn_index = _tensor_of(knn_index, (n, k), torch.int32, what, "knn_index", "is")
    p = points.contiguous()
    rows = knn(p, p, k, method=method, exclude_self=True)["index"] if knn_index is None else knn_index
    _need_cuda(p, nrm, colors, rows)
    out = torch.empty((n, 3), dtype=torch.float32, device=p.device)
    check(_lib.load().sgam_points_color_gradient_f32(_p(p), _p(nrm), _p(colors), n, _p(rows), k, _p(out), _stream()),
          "sgam_points_color_gradient_f32")
    return out


def icp_accumulate_colored(moved, source_colors, target, target_normals, target_colors, target_gradients, index, d2, lambda_geometric,
                           partials=None):
    """sgam_points_icp_accumulate_colored: icp_accumulate's sums with the geometric row scaled by sqrt(lambda_geometric) and the
    photometric row (scaled by sqrt(1 - lambda_geometric)) added to the same 32 slots -> partials (ceil(N / 4096), 32) fp64"""
    return _accumulate("icp_accumulate_colored", moved, target, target_normals, index, d2, partials,
                       (source_colors, target_colors, target_gradients, lambda_geometric))


def icp_update(partials, iteration, relative_fitness, relative_rmse, state, history):
    """sgam_points_icp_update: one Gauss-Newton step from the chunk sums, on the device state (24 fp64) and into history[iteration]"""
    if partials.dtype != torch.float64 or partials.dim() != 2 or partials.shape[1] != ICP_SLOTS or partials.shape[0] < 1 or \
            not partials.is_contiguous():
        raise ValueError(f"icp_update: partials are (blocks, {ICP_SLOTS}) fp64, not {tuple(partials.shape)} {partials.dtype}")
    if state.dtype != torch.float64 or state.numel() != ICP_STATE or not state.is_contiguous():
        raise ValueError(f"icp_update: the state is {ICP_STATE} fp64")
    if history.dtype != torch.float64 or history.dim() != 2 or history.shape[1] != ICP_ROW or not history.is_contiguous() or \
            not 0 <= int(iteration) < history.shape[0]:
        raise ValueError(f"icp_update: history is (rows, {ICP_ROW}) fp64 with rows > iteration = {iteration}")
    _need_cuda(partials, state, history)
    check(_lib.load().sgam_points_icp_update(_p(partials), int(partials.shape[0]), int(iteration), float(relative_fitness),
                                             float(relative_rmse), _p(state), _p(history), _stream()), "sgam_points_icp_update")


class _Correspondences:
    """the target's search structure, built ONCE, and the buffers an iteration writes: moved source, (d2, index), chunk sums"""

    def __init__(self, source, target, max_correspondence_distance, method, cell_size, what):
        self.n, self.nr = _one_cloud(source, what), _one_cloud(target, what)
        method = search_method(method, cell_size, self.nr, AUTO_GRID_MIN_REF, what)
        if max_correspondence_distance is None or not float(max_correspondence_distance) > 0:
            raise ValueError(f"{what}: max_correspondence_distance must be positive, not {max_correspondence_distance!r}")
        _one_device(source, target)
        self.max_distance = float(max_correspondence_distance)
        self.source, self.target = source.contiguous(), target.contiguous()
        self.search = search_structure(self.target, method, cell_size, AUTO_GRID_MIN_REF, what)
        dev = self.source.device
        self.moved = torch.empty((self.n, 3), dtype=torch.float32, device=dev)
        self.nn = answers((self.n,), dev)
        self.partials = icp_partials(self.n, dev, None, what)

    def step(self, T, normals, colored=None, index=None, d2=None):
        """transform, search, accumulate: three launches, nothing read back.  colored: (source colours, target colours, target
        gradients, lambda_geometric) for the coloured sums.  index, d2 (n,): fixed correspondences in place of the search's, which
        is then not run: two launches"""
        transform_points(self.source, T, out=self.moved)
        if index is None:
            self.search.query(self.moved, self.max_distance, out=self.nn)
            index, d2 = self.nn["index"], self.nn["d2"]
        return _accumulate("icp_accumulate" if colored is None else "icp_accumulate_colored", self.moved, self.target, normals, index, d2,
                           self.partials, colored)

    def evaluate(self, T):
        """(fitness, inlier_rmse, correspondences) of the pose T: the chunks folded on the host in ascending order"""
        s = np.zeros(ICP_SLOTS)
        for row in self.step(T, None).cpu().numpy():
            s = s + row
        count, points = int(s[29]), int(s[30])
        return (count / points if points else float("nan")), (math.sqrt(s[28] / count) if count else float("nan")), count


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, method="auto"):
    """Open3D's `evaluate_registration` as its documentation states it: source (N,3) moved by `transformation` (4x4, the identity
    by default) against target (M,3), fp32 device tensors -> {"fitness": correspondences / source points that are points,
    "inlier_rmse": sqrt(mean squared distance over the correspondences), "correspondences"}.  A correspondence: a source point
    whose nearest target point lies within max_correspondence_distance.  One transform + search + accumulate, no update."""
    c = _Correspondences(source, target, max_correspondence_distance, method, None, "evaluate_registration")
    fitness, rmse, count = c.evaluate(_pose(transformation, c.source.device, "evaluate_registration"))
    return {"fitness": fitness, "inlier_rmse": rmse, "correspondences": count}


def register_icp(source, target, max_correspondence_distance, init=None, estimation="point_to_plane", target_normals=None, max_iterations=30,
                 relative_fitness=1e-6, relative_rmse=1e-6, method="auto", cell_size=None, check_every=8, source_colors=None,
                 target_colors=None, target_gradients=None, lambda_geometric=LAMBDA_GEOMETRIC, gradient_k=16):
    """ICP of source (N,3) onto target (M,3), fp32 device tensors, by Gauss-Newton steps on the device (Open3D's
    `registration_icp` as documented, its three criteria as defaults; unpinned against Open3D).  estimation "point_to_plane"
    needs target_normals (M,3) fp32 (geometry.estimate_normals; a NaN normal leaves its point out), "point_to_point" takes none.
    init: 4x4 numpy or fp64 device tensor, the identity by default.  The target's search structure is built once (`method`,
    `cell_size` as in nearest_neighbors); an iteration is four launches — transform, search, accumulate, update — and reads
    nothing back: the update kernel applies the stop rules and freezes the state.  check_every=n reads the 8-byte status every n
    iterations and stops issuing launches once it is not 0; None never looks; the result does not depend on it.  Returns
        transformation (4,4) fp64 device tensor, source -> target      iterations: updates applied
        status 0 (max_iterations reached) / 1 (converged: fitness and RMSE both moved less than the criteria) / 2 (degenerate: fewer
        than 6 correspondences, or a direction of the pose the correspondences leave free)      converged: status == 1
        history (rows, 8) fp64 numpy, a row per iteration evaluated: fitness, RMSE, correspondences, sum r^2, |omega|, |v|, status, 0
        fitness, inlier_rmse: evaluate_registration's numbers at the returned transformation.
    estimation "colored" (coloured ICP: Park, Zhou, Koltun 2017; Open3D's `registration_colored_icp` as documented, unpinned): for
    clouds whose geometry leaves the pose free — a plane slides along itself under point-to-plane — and whose colours do not.  It
    needs target_normals, source_colors (N,3) and target_colors (M,3) uint8 device tensors; target_gradients (M,3) fp32 are
    color_gradients(target, target_normals, target_colors, k=gradient_k) when not given.  Every correspondence adds the
    point-to-plane row scaled by sqrt(lambda_geometric) and a photometric row scaled by sqrt(1 - lambda_geometric): the source
    point's intensity against the target's intensity carried along its gradient to the source point's foot in the tangent plane
    (sgam_points_icp_accumulate_colored).  A target point whose gradient is NaN is left out.  History column 3 is then the sum of
    both squared residuals; everything else, the four launches per iteration included, is as above."""
    what = "register_icp"
    check_estimation(estimation, what)
    if estimation in ("point_to_plane", "colored") and target_normals is None:
        raise ValueError(f"{what}: {estimation} needs target_normals (geometry.estimate_normals)")
    if estimation != "colored" and (source_colors is not None or target_colors is not None or target_gradients is not None):
        raise ValueError(f"{what}: colours and gradients belong to estimation='colored'")
    if estimation == "point_to_point" and target_normals is not None:
        raise ValueError(f"{what}: point_to_point takes no target_normals")
    max_iterations = _integer("max_iterations", max_iterations, 1, math.inf, what, "a positive integer")
    if check_every is not None:
        _integer("check_every", check_every, 1, math.inf, what, "a positive integer or None")
    if not (float(relative_fitness) >= 0 and float(relative_rmse) >= 0):
        raise ValueError(f"{what}: relative_fitness and relative_rmse are >= 0")
    if estimation == "colored":                   # (what can be refused without the device is refused before it is asked for)
        lam = _lambda_of(lambda_geometric, what)
        gradient_k = _check_k(gradient_k)
        n, nr = _one_cloud(source, what), _one_cloud(target, what)
        source_colors, target_colors = _colors_of(source_colors, n, what, "source_colors"), _colors_of(target_colors, nr, what, "target_colors")
        if target_gradients is not None:
            target_gradients = _tensor_of(target_gradients, (nr, 3), torch.float32, what, "target_gradients")
    c = _Correspondences(source, target, max_correspondence_distance, method, cell_size, what)
    if target_normals is not None:
        _need_cuda(target_normals)
        target_normals = _tensor_of(target_normals, (c.nr, 3), torch.float32, what, "target_normals")
    colored = None
    if estimation == "colored":
        if target_gradients is None:
            target_gradients = color_gradients(c.target, target_normals, target_colors, k=gradient_k)
        _need_cuda(source_colors, target_colors, target_gradients)
        colored = (source_colors, target_colors, target_gradients, lam)
    dev = c.source.device
    state = icp_state(init, dev, what)
    history = torch.zeros((max_iterations, ICP_ROW), dtype=torch.float64, device=dev)
    T = state[:16].view(4, 4)                 # the pose where the update kernel writes it: no host round trip
    for it in range(max_iterations):
        icp_update(c.step(T, target_normals, colored), it, relative_fitness, relative_rmse, state, history)
        if check_every is not None and (it + 1) % check_every == 0 and float(state[18].item()) != 0.0:
            break
    final = state.cpu().numpy()
    rows = history.cpu().numpy()[:it + 1]
    stopped = np.flatnonzero(rows[:, 6] != 0.0)
    if len(stopped):
        rows = rows[:stopped[0] + 1]
    transformation = state[:16].clone().reshape(4, 4)
    fitness, rmse, _ = c.evaluate(transformation)
    return {"transformation": transformation, "fitness": fitness, "inlier_rmse": rmse, "iterations": int(final[19]),
            "converged": int(final[18]) == 1, "status": int(final[18]), "history": rows}


def register_icp_multiscale(source, target, voxel_sizes, max_correspondence_distances, max_iterations, init=None, estimation="point_to_plane",
                            source_colors=None, target_colors=None, lambda_geometric=LAMBDA_GEOMETRIC, normal_k=16, gradient_k=16,
                            relative_fitness=1e-6, relative_rmse=1e-6, method="auto", check_every=8):
    """register_icp coarse to fine (Open3D's multi-scale recipe): one level per entry of voxel_sizes, with its entry of
    max_correspondence_distances and of max_iterations (a list as long, or one integer for every level).  Per level both clouds
    are voxel-sampled at the level's voxel size (voxel_sample: real points, so the colours go along; None: the clouds as they
    are), the sampled target's normals are estimate_normals(k=normal_k) for "point_to_plane" and "colored", for "colored" its
    gradients are color_gradients(k=gradient_k), and register_icp starts from the previous level's pose, which stays on the
    device.  No kernel of its own.  Returns the last level's dict plus "levels": the list of every level's dict, each with its
    "voxel_size", "max_correspondence_distance", "n_source" and "n_target"."""
    what = "register_icp_multiscale"
    check_estimation(estimation, what)
    voxel_sizes, distances = list(voxel_sizes), list(max_correspondence_distances)
    iterations = [max_iterations] * len(voxel_sizes) if isinstance(max_iterations, (int, np.integer)) else list(max_iterations)
    if not voxel_sizes or len(distances) != len(voxel_sizes) or len(iterations) != len(voxel_sizes):
        raise ValueError(f"{what}: voxel_sizes, max_correspondence_distances and max_iterations name the same levels, at least one "
                         f"({len(voxel_sizes)}, {len(distances)}, {len(iterations)})")
    n, nr = _one_cloud(source, what), _one_cloud(target, what)
    colored = estimation == "colored"
    if colored:
        _lambda_of(lambda_geometric, what)
        source_colors, target_colors = _colors_of(source_colors, n, what, "source_colors"), _colors_of(target_colors, nr, what, "target_colors")
    elif source_colors is not None or target_colors is not None:
        raise ValueError(f"{what}: colours belong to estimation='colored'")
    _need_cuda(source, target)
    pose, levels, k = init, [], None if estimation == "point_to_point" else normal_k
    for h, distance, its in zip(voxel_sizes, distances, iterations):
        if h is None:                             # the clouds as they are, the rows that are not points included
            src, tgt, sc, tc = source.contiguous(), target.contiguous(), source_colors, target_colors
            normals = None if k is None else estimate_normals(tgt, k)
        else:
            (src, si, _), (tgt, ti, normals) = prepare_cloud(source, what, h), prepare_cloud(target, what, h, normal_k=k)
            if colored:
                sc, tc = source_colors[si].contiguous(), target_colors[ti].contiguous()
        extra = dict(source_colors=sc, target_colors=tc, lambda_geometric=lambda_geometric, gradient_k=gradient_k) if colored else {}
        reg = register_icp(src, tgt, distance, init=pose, estimation=estimation, target_normals=normals, max_iterations=its,
                           relative_fitness=relative_fitness, relative_rmse=relative_rmse, method=method, check_every=check_every, **extra)
        reg.update(voxel_size=h, max_correspondence_distance=distance, n_source=int(src.shape[0]), n_target=int(tgt.shape[0]))
        levels.append(reg)
        pose = reg["transformation"]
    return dict(levels[-1], levels=levels)


# ---------------------------------------------------------------- multiway registration (csrc/pose_graph.hip)
PG_STATE, PG_ROW = 16, 8         # doubles of the optimiser's device state and of a history row (include/sgam_hip.h)
PG_MAX_NODES, PG_MAX_EDGES, SPD_MAX_N = 1024, 65536, 6144
PG_STATUS, PG_MU = 3, 11         # state slots the host side touches: the status word the solve shares, and mu
_TRI6 = [[(min(a, b) * 6 - min(a, b) * (min(a, b) - 1) // 2 + abs(a - b)) for b in range(6)] for a in range(6)]


def spd_solve(A, b, damping=None, status=None, n=None):
    """(A + damping I) x = b for a symmetric positive definite A by the device Cholesky of csrc/pose_graph.hip
    (sgam_spd_solve_f64).  A (rows >= n, ld >= n) fp64 device tensor whose leading n x n lower triangle is read (n: b's length by
    default), b (n,) fp64; damping None, a float, or a one-element fp64 device tensor (no host round trip).  status: a one-element
    fp64 device tensor (a new zero by default): the solve does nothing when it is not 0 and sets it to 2 at a pivot that is not
    finite or <= 1e-12 of the damped diagonal entry it started from; x is then not written.  -> (x (n,) fp64, status tensor)."""
    what = "spd_solve"
    if not isinstance(A, torch.Tensor) or A.dtype != torch.float64 or A.dim() != 2 or A.stride(1) != 1:
        raise ValueError(f"{what}: A is a 2-D fp64 tensor with unit column stride")
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64 or b.dim() != 1:
        raise ValueError(f"{what}: b is (n,) fp64")
    n = int(b.shape[0]) if n is None else int(n)
    ld = int(A.stride(0)) if A.shape[0] > 1 else int(A.shape[1])
    if not 1 <= n <= SPD_MAX_N or A.shape[0] < n or A.shape[1] < n or b.shape[0] < n or ld < n:
        raise ValueError(f"{what}: n is in 1..{SPD_MAX_N} and A at least n x n, not n = {n}, A {tuple(A.shape)}")
    dev = A.device
    if isinstance(damping, torch.Tensor):
        if damping.dtype != torch.float64 or damping.numel() != 1:
            raise ValueError(f"{what}: damping given as a tensor is one fp64 value")
    elif damping is not None:
        damping = torch.full((1,), float(damping), dtype=torch.float64, device=dev)
    if status is None:
        status = torch.zeros((1,), dtype=torch.float64, device=dev)
    elif status.dtype != torch.float64 or status.numel() != 1:
        raise ValueError(f"{what}: status is one fp64 value")
    b = b.contiguous()
    _one_device(A, b, damping, status, text=f"{what}: the operands live on one device")
    lib = _lib.load()
    need = int(lib.sgam_spd_solve_workspace_doubles(n))
    work = torch.empty((need,), dtype=torch.float64, device=dev)
    x = torch.zeros((n,), dtype=torch.float64, device=dev)
    check(lib.sgam_spd_solve_f64(_p(A), n, ld, _p(damping), _p(b), _p(work), need, _p(x), _p(status), _stream()), "sgam_spd_solve_f64")
    return x, status


class PoseGraph:
    """The pose graph of multiway registration: n_nodes clouds and edges (s, t, T_st, Lambda, uncertain), T_st the registration of
    cloud s onto cloud t (4x4), Lambda its 6x6 information matrix in the (omega, v) order of the ICP update
    (`registration_information`), uncertain = a loop closure the line process may switch off (an odometry edge is certain).
    Plain device tensors underneath: `add_edge` appends, `PoseGraph.from_tensors` takes finished ones."""

    def __init__(self, n_nodes, device="cuda"):
        self.n_nodes = _integer("n_nodes", n_nodes, 1, PG_MAX_NODES, "PoseGraph")
        self.device = torch.device(device)
        self.source, self.target, self.uncertain = [], [], []
        self._T, self._info, self._stacked = [], [], None

    def __len__(self):
        return len(self.source)

    def add_edge(self, s, t, transformation, information, uncertain=False):
        what = "PoseGraph.add_edge"
        s, t = _integer("s", s, 0, self.n_nodes - 1, what), _integer("t", t, 0, self.n_nodes - 1, what)
        if s == t:
            raise ValueError(f"{what}: an edge joins two different nodes, not {s} and {t}")
        if len(self.source) >= PG_MAX_EDGES:
            raise ValueError(f"{what}: a graph holds at most {PG_MAX_EDGES} edges")
        T = _pose(transformation, self.device, what)
        if isinstance(information, torch.Tensor):
            if tuple(information.shape) != (6, 6) or information.dtype != torch.float64:
                raise ValueError(f"{what}: information given as a tensor is (6,6) fp64, not {tuple(information.shape)} {information.dtype}")
            _need_cuda(information)
            info = information.contiguous()
        else:
            info = np.asarray(information, dtype=np.float64)
            if info.shape != (6, 6):
                raise ValueError(f"{what}: information is 6x6, not {info.shape}")
            info = torch.from_numpy(np.ascontiguousarray(info)).to(self.device)
        self.source.append(s), self.target.append(t), self.uncertain.append(bool(uncertain))
        self._T.append(T), self._info.append(info)
        self._stacked = None
        return self

    @classmethod
    def from_tensors(cls, n_nodes, source, target, transformations, information, uncertain):
        """source, target (E,) integer, transformations (E,4,4) fp64, information (E,6,6) fp64, uncertain (E,) bool: device tensors
        (the two index vectors are copied to the host once, for the checks)"""
        what = "PoseGraph.from_tensors"
        E = int(source.numel())
        T = _tensor_of(transformations, (E, 4, 4), torch.float64, what, "transformations") if E else transformations
        info = _tensor_of(information, (E, 6, 6), torch.float64, what, "information") if E else information
        if E > PG_MAX_EDGES or int(target.numel()) != E or int(uncertain.numel()) != E:
            raise ValueError(f"{what}: source, target and uncertain name the same E <= {PG_MAX_EDGES} edges")
        _one_device(source, target, T, info, uncertain, text=f"{what}: the tensors live on one device")
        g = cls(n_nodes, T.device)
        g.source, g.target = [int(v) for v in source.cpu().tolist()], [int(v) for v in target.cpu().tolist()]
        g.uncertain = [bool(v) for v in uncertain.cpu().tolist()]
        for s, t in zip(g.source, g.target):
            if not (0 <= s < g.n_nodes and 0 <= t < g.n_nodes) or s == t:
                raise ValueError(f"{what}: an edge joins two different nodes of 0..{g.n_nodes - 1}, not {s} and {t}")
        g._stacked = (T, info)
        return g

    def tensors(self):
        """(source (E,) int32, target (E,) int32, transformations (E,4,4), information (E,6,6), uncertain (E,) uint8) on the device"""
        if self._stacked is None:
            self._stacked = (torch.stack(self._T), torch.stack(self._info)) if self._T else (
                torch.zeros((0, 4, 4), dtype=torch.float64, device=self.device), torch.zeros((0, 6, 6), dtype=torch.float64, device=self.device))
        dev = self._stacked[0].device
        return (torch.tensor(self.source, dtype=torch.int32, device=dev), torch.tensor(self.target, dtype=torch.int32, device=dev),
                self._stacked[0], self._stacked[1], torch.tensor(self.uncertain, dtype=torch.uint8, device=dev))


def _pg_check(source, target, n_nodes, fixed, what):
    """sgam_pose_graph_check on the host copies of the index vectors: the kernels trust them"""
    s, t = np.ascontiguousarray(source, dtype=np.int32), np.ascontiguousarray(target, dtype=np.int32)
    rc = _lib.load().sgam_pose_graph_check(ctypes.c_void_p(s.ctypes.data), ctypes.c_void_p(t.ctypes.data), len(s), int(n_nodes), int(fixed))
    if rc != 0:
        raise ValueError(f"{what}: 1..{PG_MAX_NODES} nodes, at most {PG_MAX_EDGES} edges between two different nodes of the graph, and a "
                         f"fixed node of the graph (nodes {n_nodes}, edges {len(s)}, fixed {fixed})")


class _PoseGraphRun:
    """One Levenberg-Marquardt run on the device: the static incidence lists (torch plumbing, built once), every buffer, the
    prologue and the launches of one attempt.  src, dst (E,) int32, T (E,4,4), info (E,6,6) fp64, unc (E,) uint8, all on the device
    and checked; mu a float or a one-element fp64 device tensor; poses (N,4,4) fp64 device (copied)."""

    def __init__(self, n_nodes, src, dst, T, info, unc, mu, fixed, poses):
        self.N, self.E, self.fixed = int(n_nodes), int(src.numel()), int(fixed)
        self.n = 6 * self.N
        dev, f64 = T.device, torch.float64
        self.src, self.dst, self.T, self.info, self.unc = src.contiguous(), dst.contiguous(), T.contiguous(), info.contiguous(), unc.contiguous()
        N, E = self.N, self.E
        s64, d64, e = src.long(), dst.long(), torch.arange(E, device=dev)
        # a node's edges, and a node pair's, in ascending edge index (the keys are distinct: one sort each)
        node = torch.cat([s64, d64])
        order = torch.argsort(node * E + torch.cat([e, e]))
        diag_entry = torch.cat([2 * e, 2 * e + 1])[order]
        pair = torch.minimum(s64, d64) * N + torch.maximum(s64, d64)
        order = torch.argsort(pair * E + e)
        pairs, counts = torch.unique_consecutive(pair[order], return_counts=True)
        nodes = torch.arange(N, device=dev)
        self.block_row = torch.cat([nodes, pairs // N]).int()
        self.block_col = torch.cat([nodes, pairs % N]).int()
        sizes = torch.cat([torch.bincount(node, minlength=N), counts])
        self.block_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(sizes, 0)]).int()
        self.block_entry = torch.cat([diag_entry, (2 * e + (s64 > d64).long())[order]]).int()
        self.blocks = int(self.block_row.numel())
        self.state = torch.zeros((PG_STATE,), dtype=f64, device=dev)
        self.state[PG_MU] = mu if not isinstance(mu, torch.Tensor) else mu.reshape(())
        self.poses = poses.reshape(N, 16).clone()
        self.trial = torch.empty_like(self.poses)
        z = lambda *shape: torch.zeros(shape, dtype=f64, device=dev)  # noqa: E731
        self.lin = {"r": z(E, 6), "J": z(E, 6, 6), "q": z(E), "l": z(E), "cost": z(E), "K": z(E, 6, 6), "g": z(E, 6)}
        self.l = z(E)
        self.H, self.b, self.delta = z(self.n, self.n), z(self.n), z(self.n)
        self.work_doubles = int(_lib.load().sgam_spd_solve_workspace_doubles(self.n))
        self.work = None
        self.lib = _lib.load()

    def linearize(self, poses):
        o = self.lin
        check(self.lib.sgam_pose_graph_linearize(_p(poses), self.N, _p(self.src), _p(self.dst), _p(self.T), _p(self.info), _p(self.unc), self.E,
                                                 _p(self.state), _p(o["r"]), _p(o["J"]), _p(o["q"]), _p(o["l"]), _p(o["cost"]), _p(o["K"]),
                                                 _p(o["g"]), _stream()), "sgam_pose_graph_linearize")

    def fold(self, step):
        check(self.lib.sgam_pose_graph_fold(_p(self.lin["cost"]), self.E, _p(self.delta) if step else None, _p(self.b), self.n, _p(self.state),
                                            _stream()), "sgam_pose_graph_fold")

    def assemble(self, gated):
        check(self.lib.sgam_pose_graph_assemble(_p(self.lin["K"]), _p(self.lin["g"]), self.N, self.fixed, _p(self.block_row), _p(self.block_col),
                                                _p(self.block_ptr), _p(self.block_entry), self.blocks, _p(self.state), int(gated), _p(self.H),
                                                _p(self.b), _stream()), "sgam_pose_graph_assemble")

    def decide(self, mode, attempt, relative_cost, history):
        check(self.lib.sgam_pose_graph_decide(mode, attempt, _p(self.H), self.N, self.fixed, float(relative_cost), _p(self.poses), _p(self.trial),
                                              _p(self.l), _p(self.lin["l"]), self.E, _p(self.state), _p(history), _stream()),
              "sgam_pose_graph_decide")

    def prologue(self):
        """l, F, H, b, lambda and nu at the initial poses"""
        self.linearize(self.poses)
        self.fold(False)
        self.assemble(False)
        self.decide(0, 0, 0.0, None)

    def attempt(self, k, gradient_tolerance, relative_cost, history):
        """the launches of attempt k; nothing is read back"""
        if self.work is None:
            self.work = torch.empty((self.work_doubles,), dtype=torch.float64, device=self.H.device)
        lib, st = self.lib, self.state
        check(lib.sgam_pose_graph_gate(_p(self.b), self.n, k, float(gradient_tolerance), _p(st), _p(history), _stream()), "sgam_pose_graph_gate")
        check(lib.sgam_spd_solve_f64(_p(self.H), self.n, self.n, _p(st), _p(self.b), _p(self.work), self.work_doubles, _p(self.delta),
                                     _p(st[PG_STATUS:]), _stream()), "sgam_spd_solve_f64")
        check(lib.sgam_pose_graph_trial(_p(self.poses), _p(self.delta), self.N, _p(st), _p(self.trial), _stream()), "sgam_pose_graph_trial")
        self.linearize(self.trial)
        self.fold(True)
        self.decide(1, k, relative_cost, history)
        self.assemble(True)

    def run(self, max_iterations, gradient_tolerance, relative_cost):
        history = torch.zeros((max_iterations, PG_ROW), dtype=torch.float64, device=self.H.device)
        self.prologue()
        for k in range(max_iterations):
            self.attempt(k, gradient_tolerance, relative_cost, history)
        return history


def pose_graph_linearize(graph, poses, line_process_weight, fixed=0):
    """The optimiser's prologue on its own (a diagnostic, and what the tests compare with the numpy twin bit for bit): graph (a
    PoseGraph with at least one edge) at poses (N,4,4) fp64 on the device, mu = line_process_weight -> per edge r (E,6), J (E,6,6),
    q, l, cost (E,), K (E,6,6), g (E,6); the normal equations H (6N,6N), b (6N,) with node `fixed` pinned; "F" (the folded cost)
    and "lambda" (1e-5 * the largest free diagonal entry of H) as one-element device tensors."""
    what = "pose_graph_linearize"
    if not isinstance(graph, PoseGraph) or len(graph) < 1:
        raise ValueError(f"{what}: graph is a geometry.PoseGraph with at least one edge")
    fixed = _integer("fixed", fixed, 0, graph.n_nodes - 1, what)
    _pg_check(graph.source, graph.target, graph.n_nodes, fixed, what)
    src, dst, T, info, unc = graph.tensors()
    P = _tensor_of(poses, (graph.n_nodes, 4, 4), torch.float64, what, "poses")
    _one_device(P, T, text=f"{what}: poses and graph live on one device")
    run = _PoseGraphRun(graph.n_nodes, src, dst, T, info, unc, float(line_process_weight), fixed, P)
    run.prologue()
    return dict(run.lin, H=run.H, b=run.b, F=run.state[2:3], **{"lambda": run.state[0:1]})


def _pg_mu(info, unc, max_correspondence_distance, preference_loop_closure, line_process_weight, what):
    """mu of the line process: the caller's, or Open3D's rule (recalled, unpinned against Open3D): preference_loop_closure *
    max_correspondence_distance^2 * the mean of Lambda[5][5] over the uncertain edges — under this project's (omega, v) order
    Lambda[5][5] of registration_information is the number of correspondences.  A device scalar: nothing is read back."""
    if line_process_weight is not None:
        mu = float(line_process_weight)
        if not (mu > 0 and math.isfinite(mu)):
            raise ValueError(f"{what}: line_process_weight is positive and finite, not {line_process_weight!r}")
        return mu
    if not bool(unc.any().item()):
        return 1.0                                # (no uncertain edge reads it)
    if max_correspondence_distance is None or not float(max_correspondence_distance) > 0 or not float(preference_loop_closure) > 0:
        raise ValueError(f"{what}: a graph with uncertain edges needs line_process_weight, or a positive max_correspondence_distance "
                         "and preference_loop_closure for the default")
    return float(preference_loop_closure) * float(max_correspondence_distance) ** 2 * info[unc.bool(), 5, 5].mean()


def optimize_pose_graph(graph, max_correspondence_distance=None, preference_loop_closure=2.0, line_process_weight=None,
                        edge_prune_threshold=0.25, max_iterations=100, fixed=0, reoptimize=True, poses=None, gradient_tolerance=1e-6,
                        relative_cost=1e-12):
    """Multiway registration's last stage (Choi, Zhou, Koltun 2015 and the structure of Open3D's
    `global_optimization` with GlobalOptimizationLevenbergMarquardt, recalled and unpinned): one consistent set of poses P_i from the
    pairwise registrations of `graph` (a PoseGraph).  P_i moves cloud i into the common frame; node `fixed` keeps its pose; `poses`
    (N,4,4) fp64 numpy or device tensor is the start, the identity by default.  Minimised: F = sum_e l_e r_e^T Lambda_e r_e +
    sum_uncertain mu (sqrt(l_e) - 1)^2 with r_e = vee(P_t^-1 P_s T_st^-1) and, on the uncertain edges, the line process
    l_e = (mu / (mu + r^T Lambda r))^2, which switches a wrong loop closure off.  mu = line_process_weight, by default
    preference_loop_closure * max_correspondence_distance^2 * the mean Lambda[5][5] (the correspondence count) over the uncertain edges.
    Levenberg-Marquardt (Madsen-Nielsen damping, tau = 1e-5) runs on the device: the dense normal equations are assembled by a gather
    and solved by a blocked fp64 Cholesky on the matrix cores; poses, state and history stay in device memory and the host loop
    issues max_iterations attempts without looking.  Afterwards the uncertain edges with l < edge_prune_threshold are pruned and,
    with reoptimize, a second run on the kept edges from the first run's poses removes the bias (of order l r) they left.  Returns
        poses (N,4,4) fp64 device      line_weights (E,) fp64 device: l after the first run      kept (E,) bool device
        history, history_second (attempts, 8) fp64 numpy: F, lambda, rho, max|b|, accepted, F', status, nu (None: no second run)
        status 0 (max_iterations reached) / 1 (converged: max|b| < gradient_tolerance, or a trial's F within relative_cost F) / 2 (degenerate:
        a failed pivot or a damping that is not finite) of the last run      iterations: accepted steps of both runs      cost: F
        converged: status == 1.
    A graph without edges is returned as it came, converged."""
    what = "optimize_pose_graph"
    if not isinstance(graph, PoseGraph):
        raise ValueError(f"{what}: graph is a geometry.PoseGraph, not {type(graph).__name__}")
    N = graph.n_nodes
    fixed = _integer("fixed", fixed, 0, N - 1, what)
    max_iterations = _integer("max_iterations", max_iterations, 1, math.inf, what, "a positive integer")
    thr = float(edge_prune_threshold)
    if not 0.0 <= thr <= 1.0:
        raise ValueError(f"{what}: edge_prune_threshold is in [0, 1], not {edge_prune_threshold!r}")
    if not (float(gradient_tolerance) >= 0 and float(relative_cost) >= 0):
        raise ValueError(f"{what}: gradient_tolerance and relative_cost are >= 0")
    _pg_check(graph.source, graph.target, N, fixed, what)
    src, dst, T, info, unc = graph.tensors()
    dev = T.device
    _need_cuda(T)
    if poses is None:
        P = torch.eye(4, dtype=torch.float64, device=dev).repeat(N, 1, 1)
    elif isinstance(poses, torch.Tensor):
        P = _tensor_of(poses, (N, 4, 4), torch.float64, what, "poses")
        _one_device(P, T, text=f"{what}: poses and graph live on one device")
    else:
        P = np.asarray(poses, dtype=np.float64)
        if P.shape != (N, 4, 4):
            raise ValueError(f"{what}: poses are ({N},4,4), not {P.shape}")
        P = torch.from_numpy(np.ascontiguousarray(P)).to(dev)
    E = len(graph)
    if E == 0:
        return {"poses": P.clone(), "line_weights": torch.zeros((0,), dtype=torch.float64, device=dev),
                "kept": torch.zeros((0,), dtype=torch.bool, device=dev), "history": np.zeros((0, PG_ROW)), "history_second": None,
                "status": 1, "iterations": 0, "cost": 0.0, "converged": True}
    mu = _pg_mu(info, unc, max_correspondence_distance, preference_loop_closure, line_process_weight, what)
    first = _PoseGraphRun(N, src, dst, T, info, unc, mu, fixed, P)
    history = first.run(max_iterations, gradient_tolerance, relative_cost)
    kept = ~(unc.bool() & (first.l < thr))
    last, history_second = first, None
    n_kept = int(kept.sum().item())
    if reoptimize and 0 < n_kept < E:
        second = _PoseGraphRun(N, src[kept], dst[kept], T[kept], info[kept], unc[kept], first.state[PG_MU].clone(), fixed, first.poses)
        history_second = second.run(max_iterations, gradient_tolerance, relative_cost).cpu().numpy()
        last = second
    st = last.state.cpu().numpy()
    iterations = int(first.state[4].item()) + (int(st[4]) if last is not first else 0)
    return {"poses": last.poses.reshape(N, 4, 4).clone(), "line_weights": first.l, "kept": kept, "history": history.cpu().numpy(),
            "history_second": history_second, "status": int(st[PG_STATUS]), "iterations": iterations, "cost": float(st[2]),
            "converged": int(st[PG_STATUS]) == 1}


def registration_information(source, target, max_correspondence_distance, transformation=None, method="auto"):
    """The 6x6 information matrix of a pairwise registration, what a pose-graph edge weighs its residual with: source (N,3) moved
    by `transformation` (4x4) against target (M,3), fp32 device tensors -> Lambda (6,6) fp64 on the device, (omega, v) order.
    Lambda = sum over the correspondences (source points with a target point within max_correspondence_distance) of G^T G with
    G = [-[p]x | I] and p the MOVED SOURCE point: slots 0..20 of the existing sgam_points_icp_accumulate in its point-to-point form,
    the chunks added in ascending order, mirrored to the full matrix; Lambda[5][5] is the number of correspondences.  Open3D's
    `get_information_matrix_from_point_clouds` builds the same sum on the PARTNER (target) point where this one uses the moved
    source point; the two points are within the correspondence distance of each other.  No kernel of its own."""
    what = "registration_information"
    c = _Correspondences(source, target, max_correspondence_distance, method, None, what)
    partials = c.step(_pose(transformation, c.source.device, what), None)
    total = partials[0].clone()
    for row in partials[1:]:
        total = total + row
    return total[torch.tensor(_TRI6, dtype=torch.long, device=total.device)]


def multiway_registration(clouds, max_correspondence_distance, estimation="point_to_plane", min_fitness=0.3, loop_closure_stride=1,
                          normals=None, colors=None, normal_k=16, registrations=None, max_icp_iterations=30, method="auto", **options):
    """Open3D's multiway registration recipe on the device: the clouds (a list of (N_i,3) fp32 device tensors that share one nominal
    frame, in sequence order) are registered pair by pair and one correction P_i per cloud is solved for, such that the clouds
    P_i * cloud_i agree (`optimize_pose_graph`; cloud `fixed`, 0 by default, keeps the identity).
      - consecutive clouds (i, i + 1): register_icp(cloud_i onto cloud_{i+1}) from the identity -> a CERTAIN edge (odometry);
      - a pair (i, j), j - i >= 2 and (j - i) % loop_closure_stride == 0, is a candidate when evaluate_registration at the identity
        gives fitness >= min_fitness; it is then registered the same way -> an UNCERTAIN edge (loop closure);
      - `registrations` {(i, j): 4x4}: the pose of a pair known from elsewhere (register_global, say), taken in place of ICP's;
        such a pair (j > i + 1) is a candidate whatever its fitness;
      - a registration that ends degenerate (status 2) adds no edge; a consecutive pair without an edge is listed in
        "missing_odometry" (its clouds are then held together by loop closures only, or not at all);
      - every edge's information matrix is registration_information at the registered pose.
    estimation as in register_icp: "point_to_plane" and "colored" use `normals` (a list, estimate_normals(k=normal_k) where None),
    "colored" also `colors` (a list of (N_i,3) uint8).  options: optimize_pose_graph's (preference_loop_closure,
    line_process_weight, edge_prune_threshold, max_iterations, fixed, reoptimize, ...).  Returns optimize_pose_graph's dict plus
    "graph", "edges" [(s, t, uncertain)], "registrations" [register_icp's dict or None per edge], "missing_odometry" [(i, i + 1)]."""
    what = "multiway_registration"
    check_estimation(estimation, what)
    clouds = list(clouds)
    n = len(clouds)
    if not 1 <= n <= PG_MAX_NODES:
        raise ValueError(f"{what}: 1..{PG_MAX_NODES} clouds, not {n}")
    stride = _integer("loop_closure_stride", loop_closure_stride, 1, math.inf, what, "a positive integer")
    if not 0.0 <= float(min_fitness) <= 1.0:
        raise ValueError(f"{what}: min_fitness is in [0, 1], not {min_fitness!r}")
    if max_correspondence_distance is None or not float(max_correspondence_distance) > 0:
        raise ValueError(f"{what}: max_correspondence_distance must be positive, not {max_correspondence_distance!r}")
    for c in clouds:
        _one_cloud(c, what)
    _one_device(*clouds)
    registrations = dict(registrations or {})
    for key in registrations:
        if not (isinstance(key, tuple) and len(key) == 2 and 0 <= key[0] < key[1] < n):
            raise ValueError(f"{what}: registrations are keyed by pairs (i, j) with 0 <= i < j < {n}, not {key!r}")
    if estimation == "colored":
        if colors is None or len(colors) != n:
            raise ValueError(f"{what}: estimation 'colored' needs colors, one (N_i,3) uint8 tensor per cloud")
    elif colors is not None:
        raise ValueError(f"{what}: colors belong to estimation='colored'")
    if normals is not None and len(normals) != n:
        raise ValueError(f"{what}: normals are a list with one entry per cloud")
    dev = clouds[0].device
    clouds = [c.contiguous() for c in clouds]
    if estimation == "point_to_point":
        if normals is not None:
            raise ValueError(f"{what}: point_to_point takes no normals")
        normals = [None] * n
    else:
        normals = [None] * n if normals is None else list(normals)
        # (cloud 0 is never a target: pairs are registered from the lower onto the higher index)
        normals = [nr if nr is not None or i == 0 else estimate_normals(clouds[i], normal_k) for i, nr in enumerate(normals)]
    gradients = {}
    graph, edges, regs, missing = PoseGraph(n, dev), [], [], []
    for i in range(n):
        for j in range(i + 1, n):
            odometry = j == i + 1
            given = registrations.get((i, j))
            if not odometry and given is None:
                if (j - i) % stride:
                    continue
                if evaluate_registration(clouds[i], clouds[j], max_correspondence_distance, method=method)["fitness"] < float(min_fitness):
                    continue
            reg = None
            if given is None:
                extra = {}
                if estimation == "colored":
                    if j not in gradients:
                        gradients[j] = color_gradients(clouds[j], normals[j], colors[j])
                    extra = dict(source_colors=colors[i], target_colors=colors[j], target_gradients=gradients[j])
                reg = register_icp(clouds[i], clouds[j], max_correspondence_distance, estimation=estimation, target_normals=normals[j],
                                   max_iterations=max_icp_iterations, method=method, **extra)
                if reg["status"] == 2:
                    if odometry:
                        missing.append((i, j))
                    continue
                T = reg["transformation"]
            else:
                T = _pose(given, dev, what)
            info = registration_information(clouds[i], clouds[j], max_correspondence_distance, T, method=method)
            graph.add_edge(i, j, T, info, uncertain=not odometry)
            edges.append((i, j, not odometry))
            regs.append(reg)
    out = optimize_pose_graph(graph, max_correspondence_distance=max_correspondence_distance, **options)
    out.update(graph=graph, edges=edges, registrations=regs, missing_odometry=missing)
    return out


# ---------------------------------------------------------------- global registration (csrc/point_global.hip)
FPFH_DIM, FPFH_ROW = 33, 34      # values of a feature; int32 of a row of fpfh_counts: the 33 counts and the number of pairs counted
RANSAC_MAX_DRAWS = 16            # Philox draws a hypothesis may use for its distinct picks (include/sgam_hip.h)
GLOBAL_REFINE = ("point_to_plane", "point_to_point", None)


def fpfh_counts(points, normals, knn_index):
    """sgam_points_fpfh_counts: the SPFH of every point, stored exactly -> (N, 34) int32 on the device: 11 counts each of theta,
    f1 and f2 (Open3D's order) and, in column 33, the number m of neighbour pairs counted.  knn_index (N,k) int32: row i of
    knn(points, points, k), the point itself among its neighbours."""
    what = "fpfh_counts"
    n = _one_cloud(points, what)
    normals = _tensor_of(normals, (n, 3), torch.float32, what, "normals")
    rows = _tensor_of(knn_index, (n, "k"), torch.int32, what, "knn_index", "is")
    k = _check_k(int(rows.shape[1]))
    p = points.contiguous()
    _need_cuda(p, normals, rows)
    counts = torch.empty((n, FPFH_ROW), dtype=torch.int32, device=p.device)
    check(_lib.load().sgam_points_fpfh_counts(_p(p), _p(normals), n, _p(rows), k, _p(counts), _stream()), "sgam_points_fpfh_counts")
    return counts


def fpfh(points, normals, k=32, radius=None, method="auto"):
    """Fast point feature histograms (Rusu, Blodow, Beetz 2009; Open3D's `compute_fpfh_feature` as documented, unpinned against
    Open3D: DESIGN §4.4.6).  points (N,3), normals (N,3) fp32 on the device -> (N,33) fp32: 11 bins each of theta, f1, f2.
    Neighbourhood: row i of knn(points, points, k, max_distance=radius) — Open3D's hybrid search, a radius and max_nn, the point
    itself among its neighbours; k <= KNN_MAX_K.  The pair features of a point and each neighbour are computed in fp64 from the
    fp32 inputs; no transcendental decides a bin (the bin of theta = atan2(y, x) is counted from half-plane tests against the ten
    bin-edge directions).  SPFH = count * (100 / m) over the m pairs counted; FPFH block = 100 * A / sum(A) + SPFH with
    A = sum over the neighbours (columns >= 1 with d2 > 0) of SPFH(neighbour) / d2, in fp64, rounded to fp32 once: each block of a
    regular row sums to 200.  A point that is not a point or has no finite normal gets a NaN row and counts for no neighbour.
    The features describe the surface only where the normals are CONSISTENTLY oriented (estimate_normals with viewpoints).
    Brute force and grid search give the same bits.  (sgam_points_fpfh_counts, sgam_points_fpfh_combine_f32)"""
    what = "fpfh"
    n = _one_cloud(points, what)
    k = _check_k(k)
    normals = _tensor_of(normals, (n, 3), torch.float32, what, "normals")
    check_method(method, what)
    if radius is not None and not float(radius) > 0:
        raise ValueError(f"{what}: radius must be positive or None, not {radius!r}")
    p = points.contiguous()
    nn = knn(p, p, k, method=method, max_distance=radius)
    counts = fpfh_counts(p, normals, nn["index"])
    out = torch.empty((n, FPFH_DIM), dtype=torch.float32, device=p.device)
    check(_lib.load().sgam_points_fpfh_combine_f32(_p(counts), _p(p), _p(normals), n, _p(nn["index"]), _p(nn["d2"]), k, _p(out), _stream()),
          "sgam_points_fpfh_combine_f32")
    return out


def match_features(source_features, target_features, mutual=False):
    """For every source row the nearest target row in feature space.  (Ns,33), (Nt,33) fp32 on the device -> {"index" (Ns,)
    int32, "d2" (Ns,) fp32}: the target row of least (d2 bits, index), d2 = the fp32 sum of (a_j - b_j)^2 over j = 0..32 in
    ascending j; a NaN row never matches and is never matched: index -1, d2 +inf.  Brute force, the target rows staged through
    LDS (sgam_features_match_f32).  mutual=True keeps (i, j) only where j's nearest source row is i (a second search with the
    roles swapped and a gather); the other rows get -1 / +inf."""
    what = "match_features"
    s = _tensor_of(source_features, ("N", FPFH_DIM), torch.float32, what, "source_features")
    t = _tensor_of(target_features, ("N", FPFH_DIM), torch.float32, what, "target_features")
    _one_device(s, t, text=f"{what}: the features live on one device")

    def search(a, b):
        out = answers((int(a.shape[0]),), a.device)
        check(_lib.load().sgam_features_match_f32(_p(a), int(a.shape[0]), _p(b), int(b.shape[0]), FPFH_DIM, _p(out["d2"]), _p(out["index"]),
                                                  _stream()), "sgam_features_match_f32")
        return out

    out = search(s, t)
    if mutual:
        back = search(t, s)["index"]
        rows = torch.arange(s.shape[0], dtype=torch.int32, device=s.device)
        keep = (out["index"] >= 0) & (back[out["index"].clamp(min=0).long()] == rows)
        out = {"index": torch.where(keep, out["index"], torch.full_like(out["index"], -1)),
               "d2": torch.where(keep, out["d2"], torch.full_like(out["d2"], math.inf))}
    return {"index": out["index"], "d2": out["d2"]}


def correspondences_of(match):
    """(C,2) int32 (source row, target row) of the matched rows of a match_features result, ascending in the source row; synchronises"""
    rows = torch.nonzero(match["index"] >= 0).reshape(-1)
    return torch.stack([rows.to(torch.int32), match["index"][rows]], dim=1).contiguous()


def _ransac_inputs(source, target, correspondences, what):
    ns, nt = _one_cloud(source, what), _one_cloud(target, what)
    c = _tensor_of(correspondences, ("C", 2), torch.int32, what, "correspondences")
    _one_device(source, target, c, text=f"{what}: clouds and correspondences live on one device")
    return source.contiguous(), target.contiguous(), c, ns, nt, int(c.shape[0])


def ransac_hypotheses(source, target, correspondences, max_correspondence_distance, hypotheses, ransac_n=3, edge_length_similarity=0.9,
                      seed=0):
    """sgam_points_ransac_hypotheses: hypothesis h = 0 .. hypotheses - 1 draws ransac_n distinct rows of `correspondences` from
    Philox4x32-10 keyed by `seed` at counter (h, draw, 0, 0), checks the edge lengths of the two sides against each other,
    estimates the pose by Horn's closed form and checks that every sample lands within the distance; all in fp64 -> {"samples"
    (H,4) int32, "valid" (H,) int32, "poses" (H,12) fp64: row-major 3 x 4, zeros where not valid}, device tensors."""
    what = "ransac_hypotheses"
    H = _integer("hypotheses", hypotheses, 1, 2 ** 31 - 1, what)
    if ransac_n not in (3, 4) or isinstance(ransac_n, bool):
        raise ValueError(f"{what}: ransac_n is 3 or 4, not {ransac_n!r}")
    sim, dist = float(edge_length_similarity), float(max_correspondence_distance)
    if not 0.0 <= sim <= 1.0:
        raise ValueError(f"{what}: edge_length_similarity is in [0, 1], not {edge_length_similarity!r}")
    if not (dist > 0 and math.isfinite(dist)):
        raise ValueError(f"{what}: max_correspondence_distance must be positive and finite, not {max_correspondence_distance!r}")
    seed = _integer("seed", seed, 0, 2 ** 64 - 1, what)
    s, t, c, ns, nt, C = _ransac_inputs(source, target, correspondences, what)
    out = {"samples": torch.empty((H, 4), dtype=torch.int32, device=s.device), "valid": torch.empty((H,), dtype=torch.int32, device=s.device),
           "poses": torch.empty((H, 12), dtype=torch.float64, device=s.device)}
    check(_lib.load().sgam_points_ransac_hypotheses(_p(s), ns, _p(t), nt, _p(c), C, H, int(ransac_n), sim, dist, seed, _p(out["samples"]),
                                                    _p(out["valid"]), _p(out["poses"]), _stream()), "sgam_points_ransac_hypotheses")
    return out


def ransac_score(source, target, correspondences, poses, valid, max_correspondence_distance, compact=True):
    """sgam_points_ransac_score: the inlier count of every valid hypothesis — the correspondences whose source point, moved by the
    pose rounded to fp32 (transform_points' expression), lies within fp32(distance)^2 of its target point in the search's fp32 d2
    — and the best of them -> {"counts" (H,) int32 (-1: not valid), "best" (1,) int64 on the device: (count << 32) | (2^32 - 1 - h)
    of the largest count, the lowest h on a tie; 0: no valid hypothesis}.  compact: gather the valid hypotheses first (the same
    outputs; faster where few are valid)."""
    what = "ransac_score"
    s, t, c, ns, nt, C = _ransac_inputs(source, target, correspondences, what)
    poses = _tensor_of(poses, ("H", 12), torch.float64, what, "poses")
    H = int(poses.shape[0])
    valid = _tensor_of(valid, (H,), torch.int32, what, "valid", "is")
    if max_correspondence_distance is None:
        raise ValueError(f"{what}: max_correspondence_distance must be given")
    m2 = max_d2_of(max_correspondence_distance)
    _need_cuda(poses, valid)
    ws, nbytes = workspace("sgam_points_ransac_score_workspace_bytes", s.device, H)
    out = {"counts": torch.empty((H,), dtype=torch.int32, device=s.device), "best": torch.empty((1,), dtype=torch.int64, device=s.device)}
    check(_lib.load().sgam_points_ransac_score(_p(s), ns, _p(t), nt, _p(c), C, _p(poses), _p(valid), H, m2, int(bool(compact)), _p(ws), nbytes,
                                               _p(out["counts"]), _p(out["best"]), _stream()), "sgam_points_ransac_score")
    return out


def ransac_inliers(source, target, correspondences, poses, best, max_correspondence_distance, state=None):
    """sgam_points_ransac_inliers: the winner of ransac_score unpacked on the device -> {"mask" (C,) uint8: the inliers of the best
    pose, "index" (Ns,) int32: per source point the target row of its inlier correspondence (the largest, should several name
    it), -1 elsewhere, "state" (24,) fp64: an ICP state whose pose [0..16) is the best hypothesis's — left as it was (the
    identity when not given) without a valid hypothesis — "info" (2,) int32: the hypothesis (-1: none) and its count}."""
    what = "ransac_inliers"
    s, t, c, ns, nt, C = _ransac_inputs(source, target, correspondences, what)
    poses = _tensor_of(poses, ("H", 12), torch.float64, what, "poses")
    if not isinstance(best, torch.Tensor) or best.numel() != 1 or best.dtype != torch.int64:
        raise ValueError(f"{what}: best is one int64")
    if state is None:
        state = icp_state(None, s.device, what)
    elif state.dtype != torch.float64 or state.numel() != ICP_STATE or not state.is_contiguous():
        raise ValueError(f"{what}: the state is {ICP_STATE} fp64")
    m2 = max_d2_of(max_correspondence_distance)
    _need_cuda(poses, best, state)
    out = {"mask": torch.empty((C,), dtype=torch.uint8, device=s.device), "index": torch.empty((ns,), dtype=torch.int32, device=s.device),
           "state": state, "info": torch.empty((2,), dtype=torch.int32, device=s.device)}
    check(_lib.load().sgam_points_ransac_inliers(_p(s), ns, _p(t), nt, _p(c), C, _p(poses), int(poses.shape[0]), _p(best), m2, _p(out["mask"]),
                                                 _p(out["index"]), _p(state), _p(out["info"]), _stream()), "sgam_points_ransac_inliers")
    return out


def register_ransac(source, target, correspondences, max_correspondence_distance, max_iterations=100_000, ransac_n=3,
                    edge_length_similarity=0.9, seed=0, refit_iterations=4):
    """Open3D's `registration_ransac_based_on_feature_matching` as documented (unpinned: DESIGN §4.4.6), on the device: the pose
    of source (N,3) onto target (M,3), fp32 device tensors, from `correspondences` (C,2) int32 (source row, target row: what
    correspondences_of(match_features(...)) gives) of which most may be wrong.  max_iterations hypotheses, each one lane: ransac_n
    (3 or 4) distinct correspondences drawn from Philox4x32-10 keyed by `seed`; the edge-length check (every pair of samples:
    la >= s lb and lb >= s la with s = edge_length_similarity), Horn's closed-form pose in fp64, the distance check of the
    samples (ransac_hypotheses); then the inlier count of every valid hypothesis over all C correspondences and the best of them,
    the lowest hypothesis on a tie (ransac_score).  There is NO early exit on a `confidence`: the GPU evaluates the fixed number
    of hypotheses, all of them independent, and the result is a function of the inputs and the seed only, run to run identical.
    The best pose is then refitted on its inliers as fixed correspondences by refit_iterations point-to-point Gauss-Newton
    steps (icp_accumulate / icp_update; fewer than 6 inliers leave the hypothesis's pose).  Nothing is read back before the end.
    Returns transformation (4,4) fp64 device tensor; fitness, inlier_rmse: evaluate_registration's numbers on the full clouds;
    hypothesis (-1: none was valid); inliers {"count", "mask" (C,) bool device tensor} of the best hypothesis's pose;
    valid_hypotheses; status 0, or 2 (degenerate) when no hypothesis was valid: the transformation is then the identity."""
    what = "register_ransac"
    H = _integer("max_iterations", max_iterations, 1, 2 ** 31 - 1, what)
    refits = _integer("refit_iterations", refit_iterations, 0, 1 << 20, what)
    hyp = ransac_hypotheses(source, target, correspondences, max_correspondence_distance, H, ransac_n, edge_length_similarity, seed)
    s, t, c, ns, nt, C = _ransac_inputs(source, target, correspondences, what)
    score = ransac_score(s, t, c, hyp["poses"], hyp["valid"], max_correspondence_distance)
    win = ransac_inliers(s, t, c, hyp["poses"], score["best"], max_correspondence_distance)
    state, T = win["state"], win["state"][:16].view(4, 4)
    corr = _Correspondences(s, t, max_correspondence_distance, "auto", None, what)     # (its search serves the evaluation at the end)
    if refits:
        zeros = torch.zeros((ns,), dtype=torch.float32, device=s.device)          # (the refit has no stop rule: no RMSE is needed)
        history = torch.zeros((refits, ICP_ROW), dtype=torch.float64, device=s.device)
        for it in range(refits):
            icp_update(corr.step(T, None, index=win["index"], d2=zeros), it, 0.0, 0.0, state, history)
    transformation = state[:16].clone().reshape(4, 4)
    info = win["info"].cpu().numpy()
    fitness, rmse, _ = corr.evaluate(transformation)
    return {"transformation": transformation, "fitness": fitness, "inlier_rmse": rmse, "hypothesis": int(info[0]),
            "inliers": {"count": int(info[1]), "mask": win["mask"].bool()}, "valid_hypotheses": int(hyp["valid"].sum().item()),
            "status": 0 if int(info[0]) >= 0 else 2}


def _global_side(points, viewpoints, voxel_size, normal_k, what):
    """one cloud of register_global: the rows that are points, voxel-sampled, with normals -> (points, normals).  viewpoints: None,
    one (3,) viewpoint of the whole cloud, or (viewpoints (V,3), view_of (N,)); estimate_normals checks what they hold"""
    n = _one_cloud(points, what)
    view_of = None
    if isinstance(viewpoints, (tuple, list)):
        viewpoints, view_of = viewpoints
    elif viewpoints is not None:
        view_of = torch.zeros((n,), dtype=torch.int32, device=points.device)
    if isinstance(viewpoints, torch.Tensor) and viewpoints.dim() == 1:
        viewpoints = viewpoints[None]
    p, _, normals = prepare_cloud(points, what, voxel_size, normal_k=normal_k, viewpoints=viewpoints, view_of=view_of)
    return p, normals


def register_global(source, target, voxel_size, source_viewpoints=None, target_viewpoints=None, normal_k=16, feature_k=32,
                    feature_radius=None, max_correspondence_distance=None, mutual=False, refine="point_to_plane", **ransac):
    """The pose of source (N,3) onto target (M,3), fp32 device tensors, WITHOUT a starting pose: Open3D's global registration
    recipe on the device.  The rows that are not points are dropped, then: 1. voxel_sample of both clouds at
    voxel_size; 2. estimate_normals(k=normal_k); 3. fpfh(k=feature_k, radius=feature_radius, default 5 voxel_size); 4.
    match_features(mutual=mutual) of the source's features in the target's; 5. register_ransac(**ransac) at
    max_correspondence_distance (default 1.5 voxel_size; the ratios of Open3D's tutorial); 6. register_icp(estimation=refine)
    from RANSAC's pose on the sampled clouds at the same distance; refine=None stops after RANSAC.
    FPFH needs consistently oriented normals.  Without viewpoints estimate_normals makes the component of largest magnitude
    positive, a rule that is NOT rotation-invariant: the two clouds' normals then disagree where the rotation between them is
    large, and so do their features.  Scenes should pass their camera centres, as merged_point_cloud does: source_viewpoints /
    target_viewpoints is one (3,) fp32 viewpoint of the whole cloud, or (viewpoints (V,3) fp32, view_of (N,) int32 per point
    of the cloud as given).  Returns transformation (4,4) fp64 device tensor, fitness, inlier_rmse (the last stage's, on the
    sampled clouds), "ransac": register_ransac's dict, "icp": register_icp's (None without refine), correspondences, n_source,
    n_target (sampled points)."""
    what = "register_global"
    if refine not in GLOBAL_REFINE:
        raise ValueError(f"{what}: refine is one of {GLOBAL_REFINE}, not {refine!r}")
    h = positive_edge("voxel_size", voxel_size)
    radius = 5.0 * h if feature_radius is None else float(feature_radius)
    distance = 1.5 * h if max_correspondence_distance is None else float(max_correspondence_distance)
    if not (radius > 0 and distance > 0):
        raise ValueError(f"{what}: feature_radius and max_correspondence_distance must be positive")
    _check_k(normal_k), _check_k(feature_k)
    _need_cuda(source, target)
    src, src_n = _global_side(source, source_viewpoints, h, normal_k, what)
    tgt, tgt_n = _global_side(target, target_viewpoints, h, normal_k, what)
    corr = correspondences_of(match_features(fpfh(src, src_n, feature_k, radius), fpfh(tgt, tgt_n, feature_k, radius), mutual=mutual))
    if corr.shape[0] < 1:
        raise ValueError(f"{what}: no feature of the source matches one of the target")
    coarse = register_ransac(src, tgt, corr, distance, **ransac)
    out = {"ransac": coarse, "icp": None, "correspondences": int(corr.shape[0]), "n_source": int(src.shape[0]), "n_target": int(tgt.shape[0])}
    last = coarse
    if refine is not None:
        last = out["icp"] = register_icp(src, tgt, distance, init=coarse["transformation"], estimation=refine,
                                         target_normals=tgt_n if refine == "point_to_plane" else None)
    out.update(transformation=last["transformation"], fitness=last["fitness"], inlier_rmse=last["inlier_rmse"])
    return out


def reduce_d2(d2, threshold=0.0):
    """sgam_points_nn_reduce on a flat fp32 device tensor -> (sum d2, sum sqrt(d2), number of finite entries, number of those with
    sqrt(d2) <= threshold)"""
    _need_cuda(d2)
    s = _block_sums("sgam_points_nn_reduce", 4, d2.contiguous().reshape(-1), _f32(threshold))
    return float(s[0]), float(s[1]), int(s[2]), int(s[3])


def _mean(total, count):
    return total / count if count else float("nan")


def metrics_from_sums(fwd, bwd, n_pred, n_ref):
    """cloud_metrics' dict from reduce_d2's tuples of the two directions (fwd: pred -> ref, bwd: ref -> pred) and the valid points
    of the two sides"""
    (s2p, s1p, mp, hp), (s2r, s1r, mr, hr) = fwd, bwd
    precision, recall = _mean(hp, n_pred), _mean(hr, n_ref)
    both = precision + recall
    fscore = 2.0 * precision * recall / both if both > 0 else (0.0 if both == 0 else float("nan"))      # (NaN: an empty cloud)
    return {"chamfer": _mean(s2p, mp) + _mean(s2r, mr), "accuracy": _mean(s1p, mp), "completeness": _mean(s1r, mr),
            "precision": precision, "recall": recall, "fscore": fscore, "n_pred": n_pred, "n_ref": n_ref}


def chamfer_distance(x, y, method="auto"):
    """pytorch3d's `chamfer_distance(x, y)` with its defaults, the loss the reference imports: squared L2 distance from every
    point to its nearest neighbour in the other cloud, the MEAN over the points of each direction, the two directions SUMMED, the
    MEAN over the batch:  mean_b [ mean_i min_j |x_bi - y_bj|^2 + mean_j min_i |x_bi - y_bj|^2 ].  x (N,3) / (B,N,3), y (M,3) /
    (B,M,3) fp32 on the device -> float.  Points that are not points are left out of the means.  No gradients (the reference's
    `ChamferLoss` module, which needs a backward pass, is not built)."""
    qx, qy = _clouds(x, y)
    fwd = nearest_neighbors(qx, qy, method)["d2"]
    bwd = nearest_neighbors(qy, qx, method)["d2"]
    total = 0.0
    for b in range(qx.shape[0]):
        sx, _, nx, _ = reduce_d2(fwd[b])
        sy, _, ny, _ = reduce_d2(bwd[b])
        total += _mean(sx, nx) + _mean(sy, ny)
    return total / qx.shape[0]


def resample_pair(pred, ref, voxel_size):
    """both clouds through voxel_sample on ONE voxel grid: origin = the fp32 minimum corner over the valid points of both"""
    (box_p, n_p), (box_r, n_r) = valid_box(pred), valid_box(ref)
    origin = np.minimum(box_p[0], box_r[0]) if n_p and n_r else (box_p[0] if n_p else box_r[0])
    out = []
    for pts, n in ((pred, n_p), (ref, n_r)):
        out.append(pts[voxel_sample(pts, voxel_size, origin)["index"].long()].contiguous() if n else pts)
    return out


def cloud_metrics(pred, ref, threshold, max_distance=None, method="auto", voxel_size=None):
    """The standard numbers of a predicted cloud (N,3) against a reference cloud (M,3), fp32 device tensors -> dict of floats:
        chamfer       mean squared distance pred -> ref + mean squared distance ref -> pred (chamfer_distance's definition)
        accuracy      mean distance pred -> ref          completeness  mean distance ref -> pred
        precision     share of the valid pred points within `threshold` of ref          recall: the same for ref against pred
        fscore        2 precision recall / (precision + recall), 0 when both are 0
        n_pred, n_ref the valid points of each cloud
    max_distance: a neighbour farther than it counts as none — such points stay out of the means and count as misses.
    voxel_size: both clouds are first resampled by voxel_sample on one shared voxel grid (resample_pair), which makes the numbers
    comparable between clouds of different density; n_pred / n_ref then count the kept points."""
    if pred.dim() != 2 or ref.dim() != 2:
        raise ValueError("cloud_metrics: two (N,3) clouds")
    if voxel_size is not None:
        _need_cuda(pred, ref)
        pred, ref = resample_pair(pred.contiguous(), ref.contiguous(), voxel_size)
        if pred.shape[0] < 1 or ref.shape[0] < 1:
            raise ValueError("cloud_metrics: a cloud without a valid point cannot be resampled")
    fwd = nearest_neighbors(pred, ref, method, max_distance)["d2"]
    bwd = nearest_neighbors(ref, pred, method, max_distance)["d2"]
    return metrics_from_sums(reduce_d2(fwd, threshold), reduce_d2(bwd, threshold), int(torch.isfinite(pred).all(dim=1).sum().item()),
                             int(torch.isfinite(ref).all(dim=1).sum().item()))


def inverse_intrinsics(K):
    """fp32[9]: inv(K) in float64, rounded once (the point-splat render's Kinv)"""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(K, dtype=np.float64)).astype(np.float32).reshape(9))


def camera_to_world(Ts_w2c):
    """(F,3,4) fp32: inv(T) of every world -> camera 4x4 in float64, rounded once"""
    Ts = np.asarray(Ts_w2c, dtype=np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.stack([np.linalg.inv(T)[:3] for T in Ts]).astype(np.float32))


def frame_store(depths, rgbs_u8, what, rgb_optional=False):
    """The frames a kernel reads where the store keeps them: F device tensors (Hs,Ws) fp32 and as many (Hs,Ws,3) uint8 (None with
    rgb_optional), each contiguous, on one device -> (F, Hs, Ws, device, ptrs).  ptrs: int64 on the device, the depth addresses then
    the colour addresses, ONE pinned upload (DEVICE tables: hundreds of frames do not fit a kernel's arguments)."""
    F = len(depths)
    rgbs = [] if rgbs_u8 is None and rgb_optional else rgbs_u8
    if F == 0 or len(rgbs) != (0 if rgbs_u8 is None else F):
        raise SgamHipError(f"{what}: needs as many colour frames as depth frames, and at least one")
    _need_cuda(*depths, *rgbs)
    dev = depths[0].device
    Hs, Ws = (int(n) for n in depths[0].shape)
    for d in depths:
        if tuple(d.shape) != (Hs, Ws) or d.dtype != torch.float32 or not d.is_contiguous() or d.device != dev:
            raise SgamHipError(f"{what}: every depth is a contiguous ({Hs},{Ws}) fp32 tensor on one device")
    for c in rgbs:
        if tuple(c.shape) != (Hs, Ws, 3) or c.dtype != torch.uint8 or not c.is_contiguous() or c.device != dev:
            raise SgamHipError(f"{what}: every colour is a contiguous ({Hs},{Ws},3) uint8 tensor on that device")
    table = np.array([t.data_ptr() for t in depths] + [t.data_ptr() for t in rgbs], dtype=np.int64)
    return F, Hs, Ws, dev, torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)


def unproject_frames(depths, rgbs_u8, K, Ts_w2c, z_near, z_far):
    """F frames as ONE coloured cloud in world coordinates, in one launch (sgam_points_unproject_f32).  depths: F device tensors
    (Hs,Ws) fp32, rgbs_u8: F device tensors (Hs,Ws,3) uint8 or None (geometry only) — each contiguous, read where it lives through
    device address tables; K 3x3; Ts_w2c (F,4,4) world -> camera.  Returns {"points" (F*Hs*Ws,3) fp32, "colors" (F*Hs*Ws,3) uint8
    (absent without rgbs_u8)}, frame-major then row-major pixels — export_point_clouds' order.  The arithmetic is the point-splat
    render's in fp32; a pixel whose depth is not finite or outside [z_near, z_far] becomes a NaN point (its colour
    is still copied): nothing is compacted, indices stay f * Hs * Ws + i * Ws + j."""
    F, Hs, Ws, dev, ptrs = frame_store(depths, rgbs_u8, "unproject_frames", rgb_optional=True)
    T = camera_to_world(Ts_w2c)
    if T.shape[0] != F:
        raise SgamHipError(f"unproject_frames: {F} frames but {T.shape[0]} poses")
    Kinv = inverse_intrinsics(K)
    T_dev = torch.from_numpy(T.reshape(F, 12)).pin_memory().to(dev, non_blocking=True)
    out = {"points": torch.empty((F * Hs * Ws, 3), dtype=torch.float32, device=dev)}
    if rgbs_u8 is not None:
        out["colors"] = torch.empty((F * Hs * Ws, 3), dtype=torch.uint8, device=dev)
    check(_lib.load().sgam_points_unproject_f32(_p(ptrs[:F]), _p(ptrs[F:]) if rgbs_u8 is not None else None, F, Hs, Ws,
                                                ctypes.c_void_p(Kinv.ctypes.data), _p(T_dev), _f32(z_near), _f32(z_far), _p(out["points"]),
                                                _p(out.get("colors")), _stream()), "sgam_points_unproject_f32")
    return out


# ---------------------------------------------------------------- reprojection view consistency (csrc/view_consistency.hip)
CONSISTENCY_CLASSES = ("invalid", "out_of_view", "target_hole", "occluded", "violation", "edge", "covisible")
CONSISTENCY_MAX_PAIRS = 16384            # pairs per kernel call
CONSISTENCY_WORKSPACE_BYTES = 256 << 20  # and not more than this many bytes of per-workgroup sums (96 B per workgroup and pair)


def relative_poses(Ts_w2c, pairs):
    """(P,12) fp32: the top 3 x 4 of T_t T_s^-1 for every (s, t) of `pairs`, formed in float64 and rounded once"""
    Ts = np.asarray(Ts_w2c, dtype=np.float64).reshape(-1, 4, 4)
    inv = {}
    out = np.empty((len(pairs), 12), dtype=np.float32)
    for k, (s, t) in enumerate(pairs):
        if s not in inv:
            inv[s] = np.linalg.inv(Ts[s])
        out[k] = (Ts[t] @ inv[s])[:3].reshape(12).astype(np.float32)
    return out


def view_consistency(depths, rgbs_u8, K, Ts_w2c, z_near, z_far, depth_tolerance, pairs=None, maps=False, _max_pairs=None):
    """Reprojection (warping) error between frames (sgam_view_consistency_f32): for every ordered pair (s, t) the
    pixels of frame s are put into camera t with their own depth and classified against what frame t holds there — 0 invalid, 1
    out of view, 2 target hole, 3 occluded (behind what t sees: harmless), 4 violation (t sees through the point: a real
    inconsistency), 5 edge, 6 covisible — and the covisible ones give a colour error (|r| + |g| + |b| in units of 0..255, against the
    bilinear colour of t) and a depth error (Z minus the bilinear depth of t).  depths: F device tensors (H,W) fp32, rgbs_u8: F device
    tensors (H,W,3) uint8, each contiguous, read where they live; K 3x3, shared; Ts_w2c (F,4,4) world -> camera; depth_tolerance:
    tau of the rule, in depth units.  pairs: a list of (s, t) positions; None: every ordered pair with s != t.

    Returns {"pairs": the list, "sums": (P,12) fp64 on the device — the seven class counts, then over the covisible pixels the sums
    of the colour error, its squares per channel, |depth error|, its square, and |depth error| / Z (consistency_summary turns a row
    into rates and means)}; with maps=True also "class_map" (P,H,W) uint8, "color_error" and "depth_error" (P,H,W) fp32, 0 where
    the pixel is not covisible.  No atomics: the same call gives the same bits.  Pairs go to the kernel in chunks."""
    what = "view_consistency"
    F = len(depths)
    tau, zn, zf = np.float32(depth_tolerance), np.float32(z_near), np.float32(z_far)
    if not tau >= 0:
        raise ValueError(f"{what}: depth_tolerance must be >= 0, not {depth_tolerance!r}")
    if not zn <= zf:
        raise ValueError(f"{what}: needs z_near <= z_far, not {z_near!r} and {z_far!r}")
    Ts = np.asarray(Ts_w2c, dtype=np.float64)
    if Ts.shape != (F, 4, 4) or not np.isfinite(Ts).all():
        raise ValueError(f"{what}: Ts_w2c is one finite 4x4 per frame ({F},4,4), not {Ts.shape}")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{what}: K is 3x3, not {K.shape}")
    if pairs is None:
        pairs = [(s, t) for s in range(F) for t in range(F) if s != t]
    else:
        pairs = list(pairs)
        for pr in pairs:
            if not isinstance(pr, (tuple, list)) or len(pr) != 2:
                raise ValueError(f"{what}: pairs are (s, t) positions, not {pr!r}")
        pairs = [(_integer("a pair's source", s, 0, F - 1, what), _integer("a pair's target", t, 0, F - 1, what)) for s, t in pairs]
    if not pairs:
        raise ValueError(f"{what}: no pairs")
    step = _integer("_max_pairs", CONSISTENCY_MAX_PAIRS if _max_pairs is None else _max_pairs, 1, CONSISTENCY_MAX_PAIRS, what)
    F, H, W, dev, ptrs = frame_store(depths, rgbs_u8, what)
    if H < 2 or W < 2:
        raise ValueError(f"{what}: frames of at least 2 x 2 pixels, not {H} x {W}")
    lib = _lib.load()
    step = max(1, min(step, CONSISTENCY_WORKSPACE_BYTES // (96 * ((H * W + 255) // 256))))
    P = len(pairs)
    kinv = inverse_intrinsics(K)
    fx, fy, cx, cy = (_f32(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    host = torch.from_numpy(np.concatenate([np.asarray(pairs, dtype=np.int32).reshape(-1), relative_poses(Ts, pairs).reshape(-1).view(np.int32)]))
    table = host.pin_memory().to(dev, non_blocking=True)                    # ONE upload: the pairs, then the poses' bits
    pairs_dev, T_dev = table[:2 * P].view(P, 2), table[2 * P:].view(torch.float32).view(P, 12)
    out = {"pairs": pairs, "sums": torch.empty((P, 12), dtype=torch.float64, device=dev)}
    if maps:
        out["class_map"] = torch.empty((P, H, W), dtype=torch.uint8, device=dev)
        out["color_error"] = torch.empty((P, H, W), dtype=torch.float32, device=dev)
        out["depth_error"] = torch.empty((P, H, W), dtype=torch.float32, device=dev)
    ws, nbytes = workspace("sgam_view_consistency_workspace_bytes", dev, H, W, min(step, P))
    for p0 in range(0, P, step):
        n = min(step, P - p0)
        part = [_p(out[k][p0:p0 + n]) if maps else None for k in ("class_map", "color_error", "depth_error")]
        check(lib.sgam_view_consistency_f32(_p(ptrs[:F]), _p(ptrs[F:]), F, H, W, ctypes.c_void_p(kinv.ctypes.data), fx, fy, cx, cy,
                                            float(zn), float(zf), float(tau), _p(pairs_dev[p0:p0 + n]), _p(T_dev[p0:p0 + n]), n,
                                            _p(out["sums"][p0:p0 + n]), *part, _p(ws), nbytes, _stream()), "sgam_view_consistency_f32")
    return out


def _ratio(a, b):
    return a / b if b > 0 else math.nan


def consistency_summary(sums):
    """A row (12,) of view_consistency's sums — or several rows (P,12), added first — as plain floats (one host read): the seven
    class counts by name (CONSISTENCY_CLASSES), n_valid = every pixel but the invalid ones, covisibility = covisible / n_valid,
    violation_rate = violation / (occluded + violation + edge + covisible), and over the covisible pixels color_mae (per channel,
    units of 0..255), psnr (dB, peak 255; inf where the colours agree exactly), depth_mae, depth_rmse, depth_rel (mean of |depth
    error| / Z).  A value whose denominator is 0 is NaN."""
    rows = sums.detach().cpu().numpy() if isinstance(sums, torch.Tensor) else np.asarray(sums)
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim not in (1, 2) or rows.shape[-1] != 12:
        raise ValueError(f"consistency_summary: a (12,) row or (P,12) rows of view_consistency's sums, not {rows.shape}")
    r = [float(v) for v in (rows.sum(axis=0) if rows.ndim == 2 else rows)]
    out = {name: int(r[k]) for k, name in enumerate(CONSISTENCY_CLASSES)}
    n_cov = r[6]
    s1, s2, s3, s4, s5 = r[7:12]
    out["n_valid"] = int(sum(r[1:7]))
    out["covisibility"] = _ratio(n_cov, sum(r[1:7]))
    out["violation_rate"] = _ratio(r[4], r[3] + r[4] + r[5] + r[6])
    out["color_mae"] = _ratio(s1, 3.0 * n_cov)
    out["psnr"] = math.nan if not n_cov > 0 else math.inf if s2 == 0 else 10.0 * math.log10(255.0 ** 2 * 3.0 * n_cov / s2)
    out["depth_mae"] = _ratio(s3, n_cov)
    out["depth_rmse"] = math.sqrt(s4 / n_cov) if n_cov > 0 else math.nan
    out["depth_rel"] = _ratio(s5, n_cov)
    return out


# ---------------------------------------------------------------- direct RGB-D odometry (csrc/rgbd_odometry.hip)
ODOMETRY_MAX_LEVELS = 4
ODOMETRY_CHUNK = 1024                    # source pixels per workgroup of the accumulation (include/sgam_hip.h)
ODOMETRY_WORKSPACE_BYTES = 256 << 20     # not more than this many bytes of per-workgroup sums (256 B per workgroup and pair)


def level_intrinsics(K, level):
    """K of pyramid level `level`: diag(2^-l, 2^-l, 1) K in float64 (fx, fy, cx, cy halved per level, exact)"""
    K = np.array(K, dtype=np.float64)
    K[:2] *= 0.5 ** level
    return K


def _odometry_levels(H, W, levels, what):
    """[(H_l, W_l)] of `levels` pyramid levels; ValueError for levels outside 1..4 or a level smaller than 2 x 2"""
    levels = _integer("levels", levels, 1, ODOMETRY_MAX_LEVELS, what)
    sizes = [(H, W)]
    for _ in range(1, levels):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    if min(sizes[-1]) < 2:
        raise ValueError(f"{what}: {levels} levels of {H} x {W} frames end smaller than 2 x 2 ({sizes[-1][0]} x {sizes[-1][1]})")
    return sizes


def rgbd_pyramid(depths, rgbs_u8, K, levels):
    """The image pyramid direct odometry reads (sgam_rgbd_pyramid_f32) of a frame store — depths: F device tensors
    (H,W) fp32, rgbs_u8: F device tensors (H,W,3) uint8, as in view_consistency.  Level 0: intensity (r + g + b) / 765 and the depth;
    level l+1: the 3 x 3 binomial filter of the intensity at (2i, 2j) with clamped borders, the depth at (2i, 2j) unfiltered (validity
    is never averaged); sizes (H+1)//2, (W+1)//2; intrinsics halved.  One launch per level, all frames.  Returns {"levels", "frames"
    F, "sizes" [(H_l, W_l)], "K" [3x3 float64 per level], "intensity", "depth": per level a (F,H_l,W_l) fp32 device tensor}."""
    what = "rgbd_pyramid"
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{what}: K is 3x3, not {K.shape}")
    if len(depths) and isinstance(depths[0], torch.Tensor) and depths[0].dim() == 2:
        sizes = _odometry_levels(int(depths[0].shape[0]), int(depths[0].shape[1]), levels, what)   # (refused before the device is asked for)
    else:
        _integer("levels", levels, 1, ODOMETRY_MAX_LEVELS, what)
    F, H, W, dev, ptrs = frame_store(depths, rgbs_u8, what)
    if H < 2 or W < 2:
        raise ValueError(f"{what}: frames of at least 2 x 2 pixels, not {H} x {W}")
    sizes = _odometry_levels(H, W, levels, what)
    total = F * sum(h * w for h, w in sizes)
    inten, depth = (torch.empty((total,), dtype=torch.float32, device=dev) for _ in range(2))
    check(_lib.load().sgam_rgbd_pyramid_f32(_p(ptrs[:F]), _p(ptrs[F:]), F, H, W, len(sizes), _p(inten), _p(depth), _stream()),
          "sgam_rgbd_pyramid_f32")
    out = {"levels": len(sizes), "frames": F, "sizes": sizes, "K": [level_intrinsics(K, l) for l in range(len(sizes))], "intensity": [],
           "depth": []}
    off = 0
    for h, w in sizes:
        out["intensity"].append(inten[off:off + F * h * w].view(F, h, w))
        out["depth"].append(depth[off:off + F * h * w].view(F, h, w))
        off += F * h * w
    return out


class _RgbdOdometry:
    """The device side of rgbd_odometry: ONE pinned upload (the plane address tables of every level, the pairs, the initial states,
    the information frames), and the two launches of an iteration for a range of pairs.  pairs are not checked here: a pair with an
    index outside [0, F) reads nothing (the kernels' rule), which the tests use."""

    def __init__(self, pyramid, pairs, init, z_near, z_far, max_depth_diff, lambda_geometric, frames=None, rows=1):
        self.pyr, self.P, self.rows = pyramid, len(pairs), int(rows)
        F, P, L = pyramid["frames"], self.P, pyramid["levels"]
        dev = pyramid["depth"][0].device
        self.zn, self.zf, self.tau, self.lam = _f32(z_near), _f32(z_far), _f32(max_depth_diff), float(lambda_geometric)
        addr = []
        for l, (h, w) in enumerate(pyramid["sizes"]):
            for plane in (pyramid["depth"][l], pyramid["intensity"][l]):
                addr.append(plane.data_ptr() + 4 * h * w * np.arange(F, dtype=np.int64))
        state = np.zeros((P, ICP_STATE), dtype=np.float64)
        state[:, :16] = np.eye(4).reshape(16) if init is None else np.asarray(init, dtype=np.float64).reshape(P, 16)
        words = [np.concatenate(addr), np.asarray(pairs, dtype=np.int32).reshape(-1).view(np.int64),
                 state.reshape(-1).view(np.int64)]
        if frames is not None:
            words.append(np.ascontiguousarray(np.asarray(frames, dtype=np.float64).reshape(P, 4, 4)[:, :3].reshape(-1).astype(np.float32))
                         .view(np.int64))
        table = torch.from_numpy(np.concatenate(words)).pin_memory().to(dev, non_blocking=True)           # the one upload
        o = 2 * L * F
        self.addr = table[:o].view(L, 2, F)
        self.pairs = table[o:o + P].view(torch.int32).view(P, 2)
        self.state = table[o + P:o + P + ICP_STATE * P].view(torch.float64).view(P, ICP_STATE)
        self.frames = table[o + P + ICP_STATE * P:].view(torch.float32).view(P, 12) if frames is not None else None
        self.history = torch.zeros((P, self.rows, ICP_ROW), dtype=torch.float64, device=dev)
        self.kinv = [inverse_intrinsics(Kl) for Kl in pyramid["K"]]
        self.lib = _lib.load()
        self.ws = self.nbytes = None
        self.F, self.dev = F, dev

    def workspace_for(self, n):
        """the per-workgroup sums of n pairs on level 0, the largest level (every level's launches carve theirs from it)"""
        H, W = self.pyr["sizes"][0]
        self.ws, self.nbytes = workspace("sgam_rgbd_odometry_workspace_bytes", self.dev, H, W, n)

    def accumulate(self, level, p0, n, level_first, information=False):
        (H, W), K, kinv = self.pyr["sizes"][level], self.pyr["K"][level], self.kinv[level]
        fr = self.frames[p0:p0 + n] if information and self.frames is not None else None
        check(self.lib.sgam_rgbd_odometry_accumulate_f32(
            _p(self.addr[level, 0]), _p(self.addr[level, 1]), self.F, H, W, ctypes.c_void_p(kinv.ctypes.data), _f32(K[0, 0]), _f32(K[1, 1]),
            _f32(K[0, 2]), _f32(K[1, 2]), self.zn, self.zf, self.tau, self.lam, _p(self.pairs[p0:p0 + n]), _p(self.state[p0:p0 + n]), n,
            int(bool(level_first)), int(bool(information)), _p(fr), _p(self.ws), self.nbytes, _stream()), "sgam_rgbd_odometry_accumulate_f32")

    def update(self, level, p0, n, row, level_first, relative_fitness, relative_rmse, sums=None):
        H, W = self.pyr["sizes"][level]
        check(self.lib.sgam_rgbd_odometry_update(_p(self.ws), self.nbytes, H, W, n, int(row), self.rows, int(bool(level_first)),
                                                 float(relative_fitness), float(relative_rmse), _p(self.state[p0:p0 + n]),
                                                 _p(self.history[p0:p0 + n]), _p(sums), _stream()), "sgam_rgbd_odometry_update")

    def fold(self, level, p0, n, sums):
        """the pairs' folded sums alone, into sums (n,32) fp64"""
        H, W = self.pyr["sizes"][level]
        check(self.lib.sgam_rgbd_odometry_update(_p(self.ws), self.nbytes, H, W, n, -1, self.rows, 0, 0.0, 0.0, None, None, _p(sums), _stream()),
              "sgam_rgbd_odometry_update")


def _odometry_arguments(what, K, z_near, z_far, max_depth_diff, iterations, lambda_geometric, relative_fitness, relative_rmse):
    """the host-side checks rgbd_odometry makes before the device is asked for -> (K float64, iterations tuple, lambda)"""
    tau, zn, zf = np.float32(max_depth_diff), np.float32(z_near), np.float32(z_far)
    if not tau >= 0:
        raise ValueError(f"{what}: max_depth_diff must be >= 0, not {max_depth_diff!r}")
    if not zn <= zf:
        raise ValueError(f"{what}: needs z_near <= z_far, not {z_near!r} and {z_far!r}")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"{what}: K is 3x3, not {K.shape}")
    if isinstance(iterations, (int, np.integer)) or not 1 <= len(iterations) <= ODOMETRY_MAX_LEVELS:
        raise ValueError(f"{what}: iterations is a sequence of 1..{ODOMETRY_MAX_LEVELS} counts, coarse to fine, not {iterations!r}")
    iterations = tuple(_integer("an entry of iterations", n, 1, 1 << 20, what) for n in iterations)
    lam = _lambda_of(lambda_geometric, what)
    if not (float(relative_fitness) >= 0 and float(relative_rmse) >= 0):
        raise ValueError(f"{what}: relative_fitness and relative_rmse are >= 0")
    return K, iterations, lam


def rgbd_odometry(depths, rgbs_u8, K, pairs, z_near, z_far, max_depth_diff, init=None, iterations=(20, 10, 5),
                  lambda_geometric=LAMBDA_GEOMETRIC, relative_fitness=1e-6, relative_rmse=1e-6, information=True, information_frames=None,
                  pyramid=None, _max_pairs=None):
    """Direct RGB-D odometry of P frame pairs in lock step (csrc/rgbd_odometry.hip; Open3D's compute_rgbd_odometry
    with the hybrid term as recalled, unpinned — with view_consistency's covisible class and bilinear reads as correspondences and
    the exact derivatives of that interpolant as image gradients).  For every pair (s, t) of `pairs` the pose M (camera s -> camera
    t) that minimises, over the pixels both frames see, (1 - lambda_geometric) (I_s - I_t(proj))^2 + lambda_geometric (Z -
    D_t(proj))^2, by Gauss-Newton steps coarse to fine over rgbd_pyramid(depths, rgbs_u8, K, len(iterations)) (or the `pyramid`
    given: the same frames, at least that many levels).  depths, rgbs_u8, K, z_near, z_far as in view_consistency; max_depth_diff is
    its depth tolerance.  init (P,4,4): the poses to start from, None: the identity.  iterations: the steps per level, coarse ->
    fine; every iteration of every level is issued for all pairs — two launches — and nothing is read back: each pair stops by
    register_icp's rules (relative_fitness, relative_rmse; a level's first step is always taken) and freezes on the device.
    Returns, on the device: "transformation" (P,4,4) fp64, "status" (P,) fp64 0 / 1 / 2 as register_icp's (2: fewer than 6 covisible
    pixels or a direction of the pose they leave free: final at every level), "fitness" (covisible / valid source pixels), "rmse"
    (depth RMSE over the covisible pixels), "iterations" (steps applied), "history" (P, sum(iterations), 8) (register_icp's row per
    iteration, levels coarse to fine); with information also "information" (P,6,6): sum of G^T G, G = [-[q]x | I], over the
    covisible pixels at the final pose at level 0, q = the moved source point, taken into the frame information_frames[p] (4x4, P
    of them) when given — registration_information's matrix for a pose-graph edge; [5][5] is the covisible count.  Plus "pairs".
    One pinned upload; pairs go to the kernels in chunks."""
    what = "rgbd_odometry"
    K, iterations, lam = _odometry_arguments(what, K, z_near, z_far, max_depth_diff, iterations, lambda_geometric, relative_fitness,
                                             relative_rmse)
    levels = len(iterations)
    F = len(depths) if pyramid is None else pyramid["frames"]
    pairs = list(pairs)
    for pr in pairs:
        if not isinstance(pr, (tuple, list)) or len(pr) != 2:
            raise ValueError(f"{what}: pairs are (s, t) positions, not {pr!r}")
    pairs = [(_integer("a pair's source", s, 0, F - 1, what), _integer("a pair's target", t, 0, F - 1, what)) for s, t in pairs]
    if not pairs:
        raise ValueError(f"{what}: no pairs")
    P = len(pairs)
    for name, v in (("init", init), ("information_frames", information_frames)):
        if v is not None:
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (P, 4, 4) or not np.isfinite(v).all():
                raise ValueError(f"{what}: {name} is one finite 4x4 per pair ({P},4,4), not {v.shape}")
    if information_frames is not None and not information:
        raise ValueError(f"{what}: information_frames belongs to information=True")
    step = _integer("_max_pairs", CONSISTENCY_MAX_PAIRS if _max_pairs is None else _max_pairs, 1, CONSISTENCY_MAX_PAIRS, what)
    if pyramid is None:
        pyramid = rgbd_pyramid(depths, rgbs_u8, K, levels)
    elif pyramid["levels"] < levels:
        raise ValueError(f"{what}: the pyramid has {pyramid['levels']} levels, iterations asks for {levels}")
    H, W = pyramid["sizes"][0]
    step = max(1, min(step, P, ODOMETRY_WORKSPACE_BYTES // (256 * ((H * W + ODOMETRY_CHUNK - 1) // ODOMETRY_CHUNK))))
    run = _RgbdOdometry(pyramid, pairs, init, z_near, z_far, max_depth_diff, lam, information_frames, rows=sum(iterations))
    run.workspace_for(step)
    sums = torch.zeros((P, ICP_SLOTS), dtype=torch.float64, device=run.dev) if information else None
    for p0 in range(0, P, step):
        n = min(step, P - p0)
        row = 0
        for k, count in enumerate(iterations):
            level = levels - 1 - k
            for it in range(count):
                run.accumulate(level, p0, n, it == 0)
                run.update(level, p0, n, row, it == 0, relative_fitness, relative_rmse)
                row += 1
        if information:
            run.accumulate(0, p0, n, False, information=True)
            run.fold(0, p0, n, sums[p0:p0 + n])
    st = run.state
    out = {"pairs": pairs, "transformation": st[:, :16].reshape(P, 4, 4).clone(), "status": st[:, 18].clone(), "fitness": st[:, 16].clone(),
           "rmse": st[:, 17].clone(), "iterations": st[:, 19].clone(), "history": run.history}
    if information:
        out["information"] = sums[:, torch.tensor(_TRI6, dtype=torch.long, device=run.dev)]
    return out


def multiway_rgbd(depths, rgbs_u8, K, Ts_w2c, z_near, z_far, max_depth_diff, min_covisibility=0.3, loop_closure_stride=1, iterations=(20, 10, 5),
                  lambda_geometric=LAMBDA_GEOMETRIC, relative_fitness=1e-6, relative_rmse=1e-6, **options):
    """multiway_registration's recipe with direct RGB-D odometry in place of one ICP per pair: the frames (depths,
    rgbs_u8, K as in view_consistency, Ts_w2c (F,4,4) the nominal world -> camera poses, in sequence order) give candidate pairs
    (i, j), i < j — consecutive frames always, as CERTAIN edges; every other pair with (j - i) % loop_closure_stride == 0 whose
    covisibility at the nominal poses, sums[6] / (H W - sums[0]) of ONE view_consistency call, is >= min_covisibility, as UNCERTAIN
    edges (loop closures) — and ONE batched rgbd_odometry registers all of them from init = T_j T_i^-1.  One host read brings the
    statuses and poses: a pair that ends degenerate (status 2) adds no edge, a consecutive one is listed in "missing_odometry".
    The edge of (i, j) in the pose graph's world frame is T_j^-1 M_ij T_i (float64 on the host), its information matrix
    rgbd_odometry's with information_frames = T_j^-1.  Then optimize_pose_graph(graph, max_correspondence_distance=max_depth_diff,
    **options) — its default line-process weight reads max_depth_diff as the distance.  Returns optimize_pose_graph's dict (poses:
    one world-frame correction per frame) plus "graph", "edges" [(i, j, uncertain)], "registrations" [{"pair", "transformation"
    (device 4x4, camera i -> camera j), "status", "iterations"} per edge], "missing_odometry" [(i, i + 1)], "odometry" (rgbd_odometry's
    dict over all candidates)."""
    what = "multiway_rgbd"
    n = len(depths)
    if not 1 <= n <= PG_MAX_NODES:
        raise ValueError(f"{what}: 1..{PG_MAX_NODES} frames, not {n}")
    stride = _integer("loop_closure_stride", loop_closure_stride, 1, math.inf, what, "a positive integer")
    if not 0.0 <= float(min_covisibility) <= 1.0:
        raise ValueError(f"{what}: min_covisibility is in [0, 1], not {min_covisibility!r}")
    if not float(max_depth_diff) > 0:
        raise ValueError(f"{what}: max_depth_diff must be positive, not {max_depth_diff!r}")
    K, iterations, lam = _odometry_arguments(what, K, z_near, z_far, max_depth_diff, iterations, lambda_geometric, relative_fitness,
                                             relative_rmse)
    Ts = np.asarray(Ts_w2c, dtype=np.float64)
    if Ts.shape != (n, 4, 4) or not np.isfinite(Ts).all():
        raise ValueError(f"{what}: Ts_w2c is one finite 4x4 per frame ({n},4,4), not {Ts.shape}")
    F, H, W, dev, _ = frame_store(depths, rgbs_u8, what)
    cand = [(i, i + 1) for i in range(n - 1)]
    loops = [(i, j) for i in range(n) for j in range(i + 2, n) if (j - i) % stride == 0]
    if loops:
        rows = view_consistency(depths, rgbs_u8, K, Ts, z_near, z_far, max_depth_diff, pairs=loops)["sums"].cpu().numpy()
        cand += [pr for pr, r in zip(loops, rows) if H * W - r[0] > 0 and r[6] / (H * W - r[0]) >= float(min_covisibility)]
    graph, edges, regs, missing = PoseGraph(n, dev), [], [], []
    odo = None
    if cand:
        inv = [np.linalg.inv(T) for T in Ts]
        odo = rgbd_odometry(depths, rgbs_u8, K, cand, z_near, z_far, max_depth_diff, init=np.stack([Ts[j] @ inv[i] for i, j in cand]),
                            iterations=iterations, lambda_geometric=lam, relative_fitness=relative_fitness, relative_rmse=relative_rmse,
                            information=True, information_frames=np.stack([inv[j] for _, j in cand]))
        P = len(cand)
        host = torch.cat([odo["transformation"].reshape(P, 16), odo["status"][:, None], odo["iterations"][:, None]], dim=1).cpu().numpy()
        keep = [k for k in range(P) if host[k, 16] != 2.0]
        missing = [cand[k] for k in range(P) if host[k, 16] == 2.0 and cand[k][1] == cand[k][0] + 1]
        if keep:
            world = np.stack([inv[cand[k][1]] @ host[k, :16].reshape(4, 4) @ Ts[cand[k][0]] for k in keep])
            index = torch.tensor(keep, dtype=torch.long, device=dev)
            graph = PoseGraph.from_tensors(n, torch.tensor([cand[k][0] for k in keep], dtype=torch.int32, device=dev),
                                           torch.tensor([cand[k][1] for k in keep], dtype=torch.int32, device=dev),
                                           torch.from_numpy(world).to(dev), odo["information"][index].contiguous(),
                                           torch.tensor([cand[k][1] != cand[k][0] + 1 for k in keep], dtype=torch.bool, device=dev))
            edges = [(cand[k][0], cand[k][1], cand[k][1] != cand[k][0] + 1) for k in keep]
            regs = [{"pair": cand[k], "transformation": odo["transformation"][k], "status": int(host[k, 16]), "iterations": int(host[k, 17])}
                    for k in keep]
    out = optimize_pose_graph(graph, max_correspondence_distance=max_depth_diff, **options)
    out.update(graph=graph, edges=edges, registrations=regs, missing_odometry=missing, odometry=odo)
    return out


# ---------------------------------------------------------------- segmentation (csrc/point_segment.hip)
# cloud sizes from which method="auto" builds a grid, measured with about 20 neighbours per point (scripts/segmentation_time.py,
# profiles/segmentation_time.json, table in DESIGN §4.4.14).  cluster_dbscan, grid build included: the grid wins at every size
# measured, 0.73 against 1.10 ms at 1024 points and 1.35 against 15.7 ms at 65536 (its link walk unites only real neighbours);
# smaller clouds were not measured and stay with brute force.  radius_count alone: brute force wins at 4096 (0.12 against 0.25 ms,
# the grid's build and its box read being the fixed cost) and loses at 16384 (0.47 against 0.28 ms).
AUTO_RADIUS_GRID_MIN = 1024
AUTO_RADIUS_COUNT_GRID_MIN = 16384
PLANE_MAX_HYPOTHESES = 1 << 24   # hypotheses per round the library takes
SEGMENT_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                   (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200),
                   (128, 0, 0), (170, 255, 195))        # cluster c is drawn in SEGMENT_PALETTE[c % 16]; planes grey, noise black
SEGMENT_PLANE_GREYS = (160, 120, 200, 90)               # plane r is drawn in the grey SEGMENT_PLANE_GREYS[r % 4]


def _masked(points, mask, what):
    """the cloud with the points where mask is False made "not a point" (NaN): torch.where as plumbing"""
    n = _one_cloud(points, what)
    _need_cuda(points)
    p = points.contiguous()
    if mask is None:
        return p, n
    m = _tensor_of(mask, (n,), torch.bool, what, "mask", verb="is")
    _one_device(p, m)
    return torch.where(m[:, None], p, torch.full((), math.nan, dtype=torch.float32, device=p.device)).contiguous(), n


def _radius_grid(p, n, radius, method, cell_size, what, auto_grid_min=AUTO_RADIUS_GRID_MIN):
    """None (brute force) or the PointGrid of the cloud over itself with cells of the radius (grid_for grows them if needed)"""
    method = search_method(method, cell_size, n, auto_grid_min, what)
    if method == "brute":
        return None
    if cell_size is None and _f32(radius) > 0 and math.isfinite(_f32(radius)):
        cell_size = _f32(radius)
    return PointGrid(p, cell_size)


def radius_count(points, radius, method="auto", cell_size=None):
    """For every point of the cloud (N,3) fp32 the number of points within `radius` of it, itself included -> (N,) int32; 0 for a
    point that is not a point.  j counts for i iff d2 = (dx * dx + dy * dy) + dz * dz <= fp32(radius)^2 in fp32 (max_d2_of).
    method "brute" (sgam_points_radius_count_brute_f32) / "grid" (the PointGrid of the cloud, cells of `cell_size`, default the radius;
    sgam_points_radius_count_grid_f32) / "auto": the grid from AUTO_RADIUS_COUNT_GRID_MIN points on.  The same bits either way and
    for every cell size."""
    p, n = _masked(points, None, "radius_count")
    max_d2 = max_d2_of(radius)
    if radius is None:
        raise ValueError("radius_count: radius must be >= 0, not None")
    grid = _radius_grid(p, n, radius, method, cell_size, "radius_count", AUTO_RADIUS_COUNT_GRID_MIN)
    count = torch.empty((n,), dtype=torch.int32, device=p.device)
    if grid is None:
        check(_lib.load().sgam_points_radius_count_brute_f32(_p(p), n, max_d2, _p(count), _stream()), "sgam_points_radius_count_brute_f32")
    else:
        check(_lib.load().sgam_points_radius_count_grid_f32(_p(p), *grid._args, max_d2, _p(count), _stream()),
              "sgam_points_radius_count_grid_f32")
    return count


def cluster_dbscan(points, eps, min_points, method="auto", cell_size=None, mask=None):
    """DBSCAN (Open3D's PointCloud.cluster_dbscan, sklearn's DBSCAN) of the cloud (N,3) fp32 on the device -> {"labels" (N,) int32:
    the cluster, -1 for noise, "core" (N,) bool, "count" (N,) int32: radius_count's, "n_clusters" () int32, "sizes" (N,) int32:
    the members of cluster l at [l], "flag" (1,) int32: 0 unless a loop of the union-find reached its bound}, all device tensors
    sized by N: nothing synchronises.  core: count >= min_points; a cluster is a connected component of the core points under the
    neighbour relation, numbered in ascending order of its least core index (the order in which Open3D and sklearn discover
    them); a point that is not core joins the cluster of its core neighbour of least (d2 bits, index) — deterministic, where
    Open3D's rule is first come, first served —, without one it is noise, like every point that is not a point.  mask (N,) bool:
    points where it is False are treated as not a point.  method / cell_size as for radius_count ("auto": the grid from
    AUTO_RADIUS_GRID_MIN points on); the same bits either way."""
    p, n = _masked(points, mask, "cluster_dbscan")
    if eps is None:
        raise ValueError("cluster_dbscan: eps must be >= 0, not None")
    max_d2 = max_d2_of(eps)
    min_points = _integer("min_points", min_points, 1, 0x7fffffff, "cluster_dbscan")
    grid = _radius_grid(p, n, eps, method, cell_size, "cluster_dbscan")
    dev = p.device
    ws, nbytes = workspace("sgam_points_dbscan_workspace_bytes", dev, n)
    out = {"labels": torch.empty((n,), dtype=torch.int32, device=dev), "core": torch.empty((n,), dtype=torch.uint8, device=dev),
           "count": torch.empty((n,), dtype=torch.int32, device=dev), "n_clusters": torch.empty((), dtype=torch.int32, device=dev),
           "sizes": torch.empty((n,), dtype=torch.int32, device=dev), "flag": torch.zeros((1,), dtype=torch.int32, device=dev)}
    tail = (max_d2, min_points, _p(ws), nbytes, _p(out["count"]), _p(out["core"]), _p(out["labels"]), _p(out["sizes"]),
            _p(out["n_clusters"]), _p(out["flag"]), _stream())
    if grid is None:
        check(_lib.load().sgam_points_dbscan_brute_f32(_p(p), n, *tail), "sgam_points_dbscan_brute_f32")
    else:
        check(_lib.load().sgam_points_dbscan_grid_f32(_p(p), *grid._args, *tail), "sgam_points_dbscan_grid_f32")
    out["core"] = out["core"].view(torch.bool)
    return out


def _plane_arguments(what, distance_threshold, num_iterations, seed):
    thr = np.float32(distance_threshold)
    if not (thr >= 0 and np.isfinite(thr)):
        raise ValueError(f"{what}: distance_threshold must be >= 0 and finite, not {distance_threshold!r}")
    H = _integer("num_iterations", num_iterations, 1, PLANE_MAX_HYPOTHESES, what)
    return float(thr), H, _integer("seed", seed, 0, (1 << 64) - 1, what)


def segment_planes(points, distance_threshold, max_planes, min_inliers=3, num_iterations=1000, seed=0, mask=None):
    """Up to max_planes planes of the cloud (N,3) fp32 by RANSAC, each over the points the earlier ones left (Open3D's
    PointCloud.segment_plane, peeled) -> {"labels" (N,) int32: the plane that took the point, else -1, "planes" (max_planes,4) fp32:
    the least-squares plane (a, b, c, d) through each plane's inliers, "ransac_planes" (max_planes,4): the winning hypotheses, whose
    inliers the labels are, "counts" (max_planes,) int32}, device tensors; one launch sequence, nothing read back.  Per round
    num_iterations hypotheses, ALL scored (no early exit on a probability); the greatest inlier count wins, a tie to the lowest
    hypothesis (no RMSE tie-break): integers only, the same bits run to run.  A round whose best count is below
    max(min_inliers, 3): NaN planes, count 0.  Inlier: |a x + b y + c z + d| <= fp32(distance_threshold) in fp32."""
    p, n = _masked(points, mask, "segment_planes")
    thr, H, seed = _plane_arguments("segment_planes", distance_threshold, num_iterations, seed)
    max_planes = _integer("max_planes", max_planes, 1, 65536, "segment_planes")
    min_inliers = _integer("min_inliers", min_inliers, 0, 0x7fffffff, "segment_planes")
    dev = p.device
    ws, nbytes = workspace("sgam_points_planes_workspace_bytes", dev, n, H)
    out = {"labels": torch.empty((n,), dtype=torch.int32, device=dev), "planes": torch.empty((max_planes, 4), dtype=torch.float32, device=dev),
           "ransac_planes": torch.empty((max_planes, 4), dtype=torch.float32, device=dev),
           "counts": torch.empty((max_planes,), dtype=torch.int32, device=dev)}
    check(_lib.load().sgam_points_segment_planes_f32(_p(p), n, H, max_planes, thr, min_inliers, seed, _p(ws), nbytes, _p(out["labels"]),
                                                     _p(out["planes"]), _p(out["ransac_planes"]), _p(out["counts"]), _stream()),
          "sgam_points_segment_planes_f32")
    return out


def segment_plane(points, distance_threshold, num_iterations=1000, seed=0, mask=None):
    """The dominant plane of the cloud: segment_planes' max_planes = 1 case -> {"plane" (4,) fp32: the least-squares plane through
    the inliers, "ransac_plane" (4,): the winning hypothesis, "inliers" (N,) bool: within the threshold of ransac_plane, "count" ()
    int32}."""
    out = segment_planes(points, distance_threshold, 1, 3, num_iterations, seed, mask)
    return {"plane": out["planes"][0], "ransac_plane": out["ransac_planes"][0], "inliers": out["labels"] == 0, "count": out["counts"][0]}


def plane_score(points, planes, distance_threshold, labels=None, hypotheses_per_lane=0):
    """sgam_points_plane_score_f32, the RANSAC's hot kernel alone: planes (H,4) fp32 against the cloud (N,3) -> (H,) int32 inlier
    counts over the points whose `labels` entry is negative (None: all).  hypotheses_per_lane 1, 2 or 4 (0: the library's choice)
    changes the kernel's layout, never the counts."""
    p, n = _masked(points, None, "plane_score")
    thr = _plane_arguments("plane_score", distance_threshold, 1, 0)[0]
    pl = _tensor_of(planes, ("H", 4), torch.float32, "plane_score", "planes")
    lab = None if labels is None else _tensor_of(labels, (n,), torch.int32, "plane_score", "labels")
    _one_device(p, pl, lab)
    if hypotheses_per_lane not in (0, 1, 2, 4):
        raise ValueError(f"plane_score: hypotheses_per_lane is 0, 1, 2 or 4, not {hypotheses_per_lane!r}")
    H = int(pl.shape[0])
    counts = torch.empty((H,), dtype=torch.int32, device=p.device)
    check(_lib.load().sgam_points_plane_score_f32(_p(p), None if lab is None else _p(lab), n, _p(pl), H, thr, int(hypotheses_per_lane),
                                                  _p(counts), _stream()), "sgam_points_plane_score_f32")
    return counts


def cluster_boxes(points, labels, n_clusters):
    """Per label 0 .. n_clusters - 1 (an int) the number of its points and their axis-aligned box -> {"count" (n,) int32, "lo" (n,3),
    "hi" (n,3) fp32}, device tensors.  Integer atomics on order-preserving keys of the coordinates: exact and independent of the
    order.  A label without a point: lo +inf, hi -inf.  No centroid: an atomic floating-point sum would not be reproducible."""
    n = _one_cloud(points, "cluster_boxes")
    _need_cuda(points)
    p = points.contiguous()
    lab = _tensor_of(labels, (n,), torch.int32, "cluster_boxes", "labels")
    _one_device(p, lab)
    k = _integer("n_clusters", n_clusters, 0, 0x7fffffff, "cluster_boxes")
    out = {"count": torch.empty((k,), dtype=torch.int32, device=p.device), "lo": torch.empty((k, 3), dtype=torch.float32, device=p.device),
           "hi": torch.empty((k, 3), dtype=torch.float32, device=p.device)}
    if k:
        check(_lib.load().sgam_points_cluster_boxes_f32(_p(p), _p(lab), n, k, _p(out["count"]), _p(out["lo"]), _p(out["hi"]), _stream()),
              "sgam_points_cluster_boxes_f32")
    return out


def segment_cloud(points, plane_threshold, eps, min_points, max_planes=1, min_plane_inliers=3, num_iterations=1000, seed=0, method="auto"):
    """Planes first, then DBSCAN over what no plane took: segment_planes' result under "plane_labels", "planes", "ransac_planes",
    "plane_counts", and cluster_dbscan's (mask = plane_labels < 0) under "cluster_labels", "core", "count", "n_clusters", "sizes",
    "flag".  Device tensors; nothing synchronises."""
    planes = segment_planes(points, plane_threshold, max_planes, min_plane_inliers, num_iterations, seed)
    clusters = cluster_dbscan(points, eps, min_points, method=method, mask=planes["labels"] < 0)
    return {"plane_labels": planes["labels"], "planes": planes["planes"], "ransac_planes": planes["ransac_planes"],
            "plane_counts": planes["counts"], "cluster_labels": clusters["labels"], "core": clusters["core"], "count": clusters["count"],
            "n_clusters": clusters["n_clusters"], "sizes": clusters["sizes"], "flag": clusters["flag"]}


def segment_colors(plane_labels, cluster_labels):
    """(N,3) uint8 on the device: the fixed palette of a segmented cloud — a point on plane r in the grey SEGMENT_PLANE_GREYS[r % 4],
    a point of cluster c in SEGMENT_PALETTE[c % 16], noise black (torch indexing as plumbing)"""
    dev = plane_labels.device
    greys = torch.tensor([(g, g, g) for g in SEGMENT_PLANE_GREYS], dtype=torch.uint8, device=dev)
    palette = torch.tensor(SEGMENT_PALETTE, dtype=torch.uint8, device=dev)
    pl, cl = plane_labels.long(), cluster_labels.long()
    out = torch.zeros((pl.shape[0], 3), dtype=torch.uint8, device=dev)
    out = torch.where((cl >= 0)[:, None], palette[cl.clamp(min=0) % len(SEGMENT_PALETTE)], out)
    return torch.where((pl >= 0)[:, None], greys[pl.clamp(min=0) % len(SEGMENT_PLANE_GREYS)], out)
