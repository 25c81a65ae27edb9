"""k-means on the HIP backend (csrc/kmeans.hip; include/sgam_hip.h "Device-resident online k-means codebook refresh").

`kmeans2` is `scipy.cluster.vq.kmeans2(data, k, iter, minit, missing='warn')` on device tensors: a fixed number of Lloyd iterations
(no convergence test — scipy has none on this path), arg-min with the first index among ties, an empty cluster keeps its previous
centre.  The only difference from scipy is the generator of `minit='points'` (a Philox-keyed permutation instead of numpy's
`rng.choice`).  The iterations are host-sequenced launches on the current stream; nothing here synchronises.

Besides the training step's refresh (`training.DeviceCodebookRefresh`) this is the tool that writes a `kmean_init_codebook_path`
file from buffered features: `np.save(path, kmeans2(features, n_embed, seed=s)[0].cpu().numpy())`.
"""
import torch

from . import _lib
from ._lib import SgamHipError, check
from ._opscore import _need_cuda, _p, _stream


def _points(x, what="data"):
    _need_cuda(x)
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise SgamHipError(f"kmeans: {what} must be a contiguous fp32 (rows, D) device tensor, not {x.dtype} {tuple(x.shape)}")
    return x


def default_chunk(N, D, k):
    c = _lib.load().sgam_kmeans_chunk_points(N, D, k)
    if c < 0:
        raise SgamHipError(f"kmeans: unsupported shape N={N} D={D} k={k} (D must be a multiple of 32)")
    return c


def assign(x, centres, chunk=None, out=None, workspace=None):
    """labels (N,) int32 of the points x (N, D) against centres (k, D); `chunk` points per distance tile (default: the library's)"""
    x, centres = _points(x), _points(centres, "centres")
    N, D = x.shape
    k = centres.shape[0]
    if centres.shape[1] != D:
        raise SgamHipError(f"kmeans: centres are {tuple(centres.shape)}, data {tuple(x.shape)}")
    lib = _lib.load()
    chunk = int(chunk) if chunk else default_chunk(N, D, k)
    need = lib.sgam_kmeans_assign_workspace_bytes(N, D, k, chunk)
    if need < 0:
        raise SgamHipError(f"kmeans: unsupported shape N={N} D={D} k={k} chunk={chunk}")
    ws = workspace if workspace is not None and workspace.numel() >= need else torch.empty((need,), device=x.device, dtype=torch.uint8)
    labels = out if out is not None else torch.empty((N,), device=x.device, dtype=torch.int32)
    check(lib.sgam_kmeans_assign_f32(_p(x), _p(centres), _p(labels), N, D, k, chunk, _p(ws), ws.numel(), _stream()),
          "sgam_kmeans_assign_f32")
    return labels


def update(x, labels, centres, block_points=0, workspace=None):
    """centres (k, D) rewritten IN PLACE with the means of their members (empty clusters untouched); returns count (k,) int32"""
    x, centres = _points(x), _points(centres, "centres")
    _need_cuda(labels)
    N, D = x.shape
    k = centres.shape[0]
    if labels.dtype != torch.int32 or labels.numel() != N or not labels.is_contiguous():
        raise SgamHipError("kmeans: labels must be a contiguous int32 tensor with one entry per point")
    lib = _lib.load()
    need = lib.sgam_kmeans_update_workspace_bytes(N, k, int(block_points))
    if need < 0:
        raise SgamHipError(f"kmeans: unsupported update shape N={N} k={k} block_points={block_points}")
    ws = workspace if workspace is not None and workspace.numel() >= need else torch.empty((need,), device=x.device, dtype=torch.uint8)
    count = torch.empty((k,), device=x.device, dtype=torch.int32)
    check(lib.sgam_kmeans_update_f32(_p(x), _p(labels), _p(centres), _p(count), N, D, k, int(block_points), _p(ws), ws.numel(),
                                     _stream()), "sgam_kmeans_update_f32")
    return count


def init_points(x, k, seed=0, refresh=0):
    """minit='points': (centres (k, D) = k distinct rows of x, picks (k,) int32) by the header's Philox-keyed permutation"""
    x = _points(x)
    N, D = x.shape
    if not 0 < k <= N:
        raise SgamHipError(f"kmeans: cannot pick {k} distinct rows out of {N}")
    centres = torch.empty((k, D), device=x.device, dtype=torch.float32)
    picks = torch.empty((k,), device=x.device, dtype=torch.int32)
    check(_lib.load().sgam_kmeans_init_points_f32(_p(x), _p(centres), _p(picks), N, D, k, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                  int(refresh) & 0xFFFFFFFFFFFFFFFF, _stream()), "sgam_kmeans_init_points_f32")
    return centres, picks


def kmeans2(data, k_or_centres, iter=10, minit="points", seed=0, refresh=0, chunk=None):      # noqa: A002 (scipy's argument name)
    """-> (centres (k, D) fp32, labels (N,) int32), like scipy's kmeans2: the labels are those of the LAST assignment, the centres
    the means computed from it.  minit='points': k_or_centres is k; minit='matrix': the (k, D) initial centres (not modified)."""
    data = _points(data)
    if minit == "points":
        centres, _ = init_points(data, int(k_or_centres), seed, refresh)
    elif minit == "matrix":
        centres = _points(k_or_centres, "initial centres").clone()
    else:
        raise NotImplementedError(f"minit={minit!r} (scipy's 'random' / '++' are not built)")
    if iter < 1:
        raise ValueError("kmeans2: iter must be at least 1")
    N, D = data.shape
    k = centres.shape[0]
    lib = _lib.load()
    chunk = int(chunk) if chunk else default_chunk(N, D, k)
    need = max(lib.sgam_kmeans_assign_workspace_bytes(N, D, k, chunk), lib.sgam_kmeans_update_workspace_bytes(N, k, 0))
    ws = torch.empty((max(need, 1),), device=data.device, dtype=torch.uint8)      # one workspace: the launches are stream-ordered
    labels = torch.empty((N,), device=data.device, dtype=torch.int32)
    for _ in range(int(iter)):
        assign(data, centres, chunk=chunk, out=labels, workspace=ws)
        update(data, labels, centres, workspace=ws)
    return centres, labels


def codebook_countdown(indices, countdown, timeout, n_dead, dead):
    """train_codebook_map bookkeeping in one launch (sgam_codebook_countdown_i32); all arguments are device tensors"""
    _need_cuda(indices, countdown, n_dead, dead)
    idx = indices.reshape(-1)
    if idx.dtype != torch.int64 or not idx.is_contiguous():
        idx = idx.to(torch.int64).contiguous()
    n = countdown.numel()
    if countdown.dtype != torch.int32 or dead.dtype != torch.int32 or n_dead.dtype != torch.int32 or dead.numel() < n:
        raise SgamHipError("codebook_countdown: countdown / dead (n_embed,) and n_dead (1,) must be int32 device tensors")
    check(_lib.load().sgam_codebook_countdown_i32(_p(idx), idx.numel(), _p(countdown), n, int(timeout), _p(n_dead), _p(dead),
                                                  _stream()), "sgam_codebook_countdown_i32")


def scatter_rows(codebook, centres, dead, n_rows, countdown=None, timeout=0):
    """codebook[dead[i]] = centres[i] for i < n_rows, in place (and the countdown reset of those words when given)"""
    codebook, centres = _points(codebook, "codebook"), _points(centres, "centres")
    _need_cuda(dead, countdown)
    if dead.dtype != torch.int32 or centres.shape[0] < n_rows or dead.numel() < n_rows or centres.shape[1] != codebook.shape[1]:
        raise SgamHipError("scatter_rows: dead must be int32 with at least n_rows entries, centres (>= n_rows, D)")
    check(_lib.load().sgam_codebook_scatter_rows_f32(_p(codebook), _p(centres), _p(dead), int(n_rows), codebook.shape[1],
                                                     codebook.shape[0], _p(countdown), int(timeout), _stream()),
          "sgam_codebook_scatter_rows_f32")
