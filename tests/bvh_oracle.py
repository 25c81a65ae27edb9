"""CPU restatement of csrc/mesh_bvh.hip (include/sgam_hip.h, "A bounding-volume hierarchy over a mesh's candidate triangles"): the
Morton key, the sort order, Karras's hierarchy, the boxes with the round each is computed in, the two node tests (the pruning
rules) in np.float32, one IEEE operation at a time and in the kernel's order, and a reference traversal with the kernel's stack
discipline.  The per-triangle arithmetic and the brute-force truths are meshquery_oracle's and raycast_oracle's.  Test
infrastructure only — the product path never imports it."""
import numpy as np

import meshquery_oracle as Q
import raycast_oracle as R

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
KEY_BITS, ID_BITS, STACK = 61, 28, 64
NO_KEY = np.iinfo(np.int64).max
REL, ABS = f32(2.0 ** -21), f32(2.0 ** -100)
SHRINK = f32(1.0 - 2.0 ** -14)
_quiet = Q._quiet


# ---------------------------------------------------------------- keys
def candidate_box(vertices, triangles):
    """(lo (3,), hi (3,)) float32 of the candidates' corners; None without a candidate"""
    a, b, c, _ = Q.corners(vertices, triangles)
    cand = Q.candidates(a, b, c)
    if not cand.any():
        return None
    pts = np.concatenate([a[cand], b[cand], c[cand]])
    return pts.min(0).astype(f32), pts.max(0).astype(f32)


@_quiet
def keys(vertices, triangles, box=None):
    """sgam_mesh_bvh_keys: -> (keys (nt,) int64, the candidates' count)"""
    a, b, c, _ = Q.corners(vertices, triangles)
    cand = Q.candidates(a, b, c)
    out = np.full(len(a), NO_KEY, dtype=np.int64)
    if not cand.any():
        return out, 0
    lo, hi = candidate_box(vertices, triangles) if box is None else (np.asarray(box[0], f32), np.asarray(box[1], f32))
    mn, mx = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    centre = (f32(0.5) * mn + f32(0.5) * mx).astype(f32)
    s = ((centre - lo) / (hi - lo)).astype(f32)
    q = np.where(s >= 0, np.minimum(np.floor((s * f32(2048)).astype(f32)), f32(2047)), f32(0))
    q = np.where(cand[:, None], q, 0).astype(np.int64)
    code = np.zeros(len(a), dtype=np.int64)
    for i in range(11):
        code |= (((q[:, 0] >> i) & 1) << (3 * i + 2)) | (((q[:, 1] >> i) & 1) << (3 * i + 1)) | (((q[:, 2] >> i) & 1) << (3 * i))
    out[cand] = ((code << ID_BITS) | np.arange(len(a), dtype=np.int64))[cand]
    return out, int(cand.sum())


def margin_of(lo, hi):
    """the distance rule's margin: 2^-14 * (largest |coordinate| of the box + its longest edge), float64, rounded to fp32 once"""
    lo, hi = np.asarray(lo, f32).astype(np.float64), np.asarray(hi, f32).astype(np.float64)
    return f32((max(np.abs(lo).max(), np.abs(hi).max()) + (hi - lo).max()) / 16384.0)


# ---------------------------------------------------------------- the tree
class Tree:
    """sgam_mesh_bvh_build restated.  n candidates; nodes in one space: internal i is i (0 the root), leaf k is n - 1 + k.
    ids (n,) the triangle of each leaf; records (n,3,3) float32 its corners; children (n-1,2); boxes (2n-1,6) (lo, hi);
    height (n-1,): the round an internal node's box is computed in; parent (2n-1,), -1 for the root; span (n-1,2): the first and
    last leaf of an internal node"""

    def __init__(self, vertices, triangles):
        self.vertices, self.triangles = np.asarray(vertices, f32).reshape(-1, 3), np.asarray(triangles).reshape(-1, 3)
        box = candidate_box(vertices, triangles)
        k, self.n = keys(vertices, triangles)
        n = self.n
        self.sorted = np.sort(k)[:n]
        self.ids = (self.sorted & ((1 << ID_BITS) - 1)).astype(np.int32)
        self.guard = R.guard_of(vertices, triangles)
        if n == 0:
            return
        self.lo, self.hi = box
        self.margin = margin_of(*box)
        a, b, c, _ = Q.corners(vertices, triangles)
        self.records = np.stack([a[self.ids], b[self.ids], c[self.ids]], 1)
        self.children = np.zeros((n - 1, 2), dtype=np.int32)
        self.span = np.zeros((n - 1, 2), dtype=np.int64)
        self.parent = np.full(2 * n - 1, -1, dtype=np.int64)
        ks = [int(x) for x in self.sorted]

        def delta(i, j):
            return 64 - (ks[i] ^ ks[j]).bit_length() if 0 <= j < n else -1

        for i in range(n - 1):
            d = 1 if delta(i, i + 1) > delta(i, i - 1) else -1
            dmin = delta(i, i - d)
            lmax = 2
            while delta(i, i + lmax * d) > dmin:
                lmax *= 2
            length, t = 0, lmax // 2
            while t >= 1:
                if delta(i, i + (length + t) * d) > dmin:
                    length += t
                t //= 2
            j = i + length * d
            dnode = delta(i, j)
            s, t = 0, length
            while True:
                t = (t + 1) // 2
                if delta(i, i + (s + t) * d) > dnode:
                    s += t
                if t <= 1:
                    break
            g = i + s * d + min(d, 0)
            first, last = min(i, j), max(i, j)
            self.children[i] = (n - 1 + g if first == g else g, n - 1 + g + 1 if last == g + 1 else g + 1)
            self.span[i] = (first, last)
            self.parent[self.children[i]] = i
        self.boxes = np.zeros((2 * n - 1, 6), dtype=f32)
        self.boxes[n - 1:, :3], self.boxes[n - 1:, 3:] = self.records.min(1), self.records.max(1)
        self.height = np.zeros(n - 1, dtype=np.int32)
        for r in range(1, min(KEY_BITS, n - 1) + 1):                         # one launch per round
            before = self.height.copy()
            for i in np.flatnonzero(before == 0):
                l, rr = self.children[i]
                if all(c >= n - 1 or 0 < before[c] < r for c in (l, rr)):
                    self.boxes[i, :3] = np.minimum(self.boxes[l, :3], self.boxes[rr, :3])
                    self.boxes[i, 3:] = np.maximum(self.boxes[l, 3:], self.boxes[rr, 3:])
                    self.height[i] = r

    def device_records(self):
        """records as the workspace holds them: (n,12) float32, the id's bits at [3], zeros at [7] and [11]"""
        out = np.zeros((self.n, 12), dtype=f32)
        out[:, 0:3], out[:, 4:7], out[:, 8:11] = self.records[:, 0], self.records[:, 1], self.records[:, 2]
        out[:, 3] = self.ids.view(f32)
        return out

    def ancestors(self, leaf):
        """the nodes from leaf k's parent up to the root"""
        out, c = [], self.parent[self.n - 1 + leaf]
        while c >= 0:
            out.append(int(c))
            c = self.parent[c]
        return out

    def leaf_of(self):
        """triangle index -> leaf (-1: not a candidate)"""
        out = np.full(len(self.triangles), -1, dtype=np.int64)
        out[self.ids] = np.arange(self.n)
        return out

    def paths(self):
        """(n, D) the leaf's own node and its ancestors, padded with the root: every node whose skipping would lose the leaf"""
        rows = [[self.n - 1 + k] + self.ancestors(k) for k in range(self.n)]
        depth = max(len(r) for r in rows)
        return np.array([r + [0] * (depth - len(r)) for r in rows], dtype=np.int64)


# ---------------------------------------------------------------- the two node tests (arrays broadcast against each other)
@_quiet
def distance_node(box, q, margin, max_d2, best):
    """the distance rule: box (...,6), q (...,3) -> (visit (...) bool, lb (...) float32)"""
    box, q = np.asarray(box, f32), np.asarray(q, f32)
    e = np.maximum(np.maximum(box[..., :3] - q, q - box[..., 3:]), f32(0))
    m = np.sqrt(Q.dot3(e, e).astype(f32)).astype(f32)
    ms = ((m - f32(margin)) * SHRINK).astype(f32)
    lb = np.where(ms > 0, (ms * ms).astype(f32), f32(0)).astype(f32)
    return ~((ms > 0) & ((np.asarray(best, f32) < lb) | (lb > f32(max_d2)))), lb


@_quiet
def ray_node(box, ray, guard, tnear, tend):
    """the ray rule against the window [tnear, tend]: box (...,6), ray (...,6) -> (visit (...) bool, enter (...) float32)"""
    box, ray = np.asarray(box, f32), np.asarray(ray, f32)
    o, d = ray[..., :3], ray[..., 3:]
    L, H = (box[..., :3] - f32(guard)).astype(f32), (box[..., 3:] + f32(guard)).astype(f32)
    M = np.maximum(np.abs(L), np.abs(H))
    E = (((np.abs(o) + M).astype(f32) * REL).astype(f32) + ABS).astype(f32)
    A, B = (L - E).astype(f32), (H + E).astype(f32)
    flat = d == 0
    s1, s2 = ((A - o).astype(f32) / d).astype(f32), ((B - o).astype(f32) / d).astype(f32)
    a, b = np.fmin(s1, s2), np.fmax(s1, s2)
    a = (a - ((np.abs(a) * REL).astype(f32) + ABS).astype(f32)).astype(f32)
    b = (b + ((np.abs(b) * REL).astype(f32) + ABS).astype(f32)).astype(f32)
    a, b = np.where(flat, NAN, a), np.where(flat, NAN, b)                    # an axis with d = 0 sets no slab (fmax / fmin drop NaN)
    enter, leave = np.asarray(tnear, f32), np.asarray(tend, f32)
    for j in range(3):
        enter, leave = np.fmax(enter, a[..., j]), np.fmin(leave, b[..., j])
    ok = (~flat | ((o >= A) & (o <= B))).all(-1)
    return ok & ~(enter > leave), np.broadcast_to(enter, ok.shape).astype(f32)


# ---------------------------------------------------------------- the reference traversal (the kernel's stack discipline)
def _walk(tree, test, still, leaf):
    """-> (nodes popped, the deepest the stack got); test(node) -> (visit, near); still(near) -> bool; leaf(k) -> True to leave"""
    n = tree.n
    stack, deepest, pops = [], 0, 0
    ok, near = test(0)
    if ok:
        stack.append((0, near))
    while stack:
        pops += 1
        assert pops <= 2 * n - 1
        c, near = stack.pop()
        if not still(near):
            continue
        if c >= n - 1:
            if leaf(c - (n - 1)):
                break
            continue
        l, r = (int(x) for x in tree.children[c])
        (pl, nl), (pr, nr) = test(l), test(r)
        if pl and pr:
            stack += [(l, nl), (r, nr)] if nr < nl else [(r, nr), (l, nl)]      # the nearer child on top; equal: the left one
        elif pl or pr:
            stack.append((l, nl) if pl else (r, nr))
        deepest = max(deepest, len(stack))
        assert len(stack) <= STACK
    return pops, deepest


@_quiet
def distance(tree, query, max_d2=np.inf):
    """sgam_mesh_distance_bvh_f32 for ONE query -> (d2, triangle, closest (3,), nodes popped)"""
    q = np.asarray(query, f32)
    best, bi, x = [INF], [-1], [np.full(3, NAN, f32)]
    if tree.n == 0 or not np.isfinite(q).all():
        return best[0], bi[0], x[0], 0
    max_d2 = f32(max_d2)

    def test(c):
        ok, lb = distance_node(tree.boxes[c], q, tree.margin, max_d2, best[0])
        return bool(ok), f32(lb)

    def leaf(k):
        d2, cp, _ = Q.point_triangle(tree.records[k, 0], tree.records[k, 1], tree.records[k, 2], q)
        if d2 <= max_d2 and (d2 < best[0] or (d2 == best[0] and tree.ids[k] < bi[0])):
            best[0], bi[0], x[0] = f32(d2), int(tree.ids[k]), cp
        return False

    pops, _ = _walk(tree, test, lambda near: not best[0] < near, leaf)
    return best[0], bi[0], x[0], pops


@_quiet
def cast(tree, ray, tnear=0.0, tfar=np.inf, any_hit=False):
    """sgam_mesh_raycast_bvh_f32 for ONE ray -> (t, triangle, hit, nodes popped, deepest stack)"""
    r = np.asarray(ray, f32)
    best, bi = [INF], [-1]
    if tree.n == 0 or not R.is_ray(r)[0]:
        return best[0], bi[0], False, 0, 0
    tnear, tfar = f32(tnear), f32(tfar)

    def end():
        return tfar if any_hit else min(tfar, best[0])

    def test(c):
        ok, enter = ray_node(tree.boxes[c], r, tree.guard, tnear, end())
        return bool(ok), f32(enter)

    def leaf(k):
        hit, t, _, _ = R.ray_triangle(tree.records[k, 0], tree.records[k, 1], tree.records[k, 2], r[:3], r[3:], tnear, tfar, tree.guard)
        if hit and (t < best[0] or (t == best[0] and tree.ids[k] < bi[0])):
            best[0], bi[0] = f32(t), int(tree.ids[k])
        return any_hit and bi[0] >= 0

    pops, deepest = _walk(tree, test, lambda near: not near > end(), leaf)
    return best[0], bi[0], bi[0] >= 0, pops, deepest


def visibility(tree, points, poses_w2c, fx, fy, cx, cy, H, W, z_near, z_far, tolerance=1e-3):
    """sgam_mesh_visibility_bvh_f32 -> count (N,) int32"""
    rays, inside = R.visibility_rays(points, poses_w2c, fx, fy, cx, cy, H, W, z_near, z_far)
    tfar = f32(1) - f32(tolerance)
    real = R.is_ray(rays.reshape(-1, 6)).reshape(inside.shape)
    count = np.zeros(inside.shape[1], dtype=np.int32)
    for p in range(inside.shape[0]):
        for i in np.flatnonzero(inside[p] & real[p]):
            count[i] += 0 if cast(tree, rays[p, i], 0.0, tfar, any_hit=True)[2] else 1
    return count
