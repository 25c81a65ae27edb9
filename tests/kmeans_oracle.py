"""CPU restatement of the device k-means codebook refresh (include/sgam_hip.h, "Device-resident online k-means codebook refresh"):
fp64 Lloyd iterations with first-of-ties arg-min and empty-keeps-previous, the Philox-keyed permutation of minit='points', the
countdown rule of model.py:313-323, and the generator of margin-guarded fixtures.  Test infrastructure only — the product path
never imports it."""
import numpy as np

from sampler_oracle import philox4x32_10

ITER = 10                 # scipy.cluster.vq.kmeans2's default
MARGIN = 1e-4             # the project's codebook convention: relative top-2 margin of every arg-min the GPU is held to bit-equal


def distances(x, c):
    """[N][k] squared distances in fp64"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return (x * x).sum(1)[:, None] - 2.0 * (x @ c.T) + (c * c).sum(1)[None]


def assign(x, c):
    """labels (first index among ties: np.argmin) and the relative top-2 margin (d2 - d1) / d2 of every point"""
    d = distances(x, c)
    lab = d.argmin(1).astype(np.int32)
    if d.shape[1] == 1:
        return lab, np.full(len(lab), np.inf)
    two = np.partition(d, 1, axis=1)[:, :2]
    return lab, (two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)


def update(x, labels, c):
    """new centres in fp64 (mean of the members; a centre without members keeps its value) and the member counts"""
    x = np.asarray(x, np.float64)
    new = np.asarray(c, np.float64).copy()
    k = len(new)
    count = np.bincount(labels, minlength=k).astype(np.int32)
    order = np.argsort(labels, kind="stable")
    starts = np.concatenate([[0], np.cumsum(count)])
    for j in np.nonzero(count)[0]:
        new[j] = x[order[starts[j]:starts[j + 1]]].sum(0) / count[j]
    return new, count


def lloyd(x, init, iters=ITER):
    """-> (centres fp64, labels of the LAST assignment (what kmeans2 returns), min relative margin over all iterations per point)"""
    c = np.asarray(init, np.float64).copy()
    margin = np.full(len(x), np.inf)
    lab = None
    for _ in range(iters):
        lab, m = assign(x, c)
        margin = np.minimum(margin, m)
        c, _ = update(x, lab, c)
    return c, lab, margin


# ---- minit='points': the first k values of a Philox-keyed Feistel permutation of [0, N), cycle-walked ----
def half_bits(N):
    h = 1
    while h < 16 and 4 ** h < N:
        h += 1
    return h


def permute(v, h, seed, refresh):
    seed, refresh = int(seed) & 0xFFFFFFFFFFFFFFFF, int(refresh) & 0xFFFFFFFFFFFFFFFF
    mask = np.uint64((1 << h) - 1)
    v = np.asarray(v, dtype=np.uint64)
    L, R = v >> np.uint64(h), v & mask
    for r in range(4):
        f = philox4x32_10((R, r, refresh & 0xFFFFFFFF, refresh >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0] & mask
        L, R = R, L ^ f
    return (L << np.uint64(h)) | R


def pick_points(N, k, seed, refresh):
    """k distinct indices in [0, N), int32 — bit for bit what sgam_kmeans_init_points_f32 writes to `picks`"""
    assert 0 < k <= N
    h = half_bits(N)
    v = permute(np.arange(k, dtype=np.uint64), h, seed, refresh)
    while True:
        out = v >= np.uint64(N)
        if not out.any():
            return v.astype(np.int32)
        v[out] = permute(v[out], h, seed, refresh)


# ---- the countdown rule (model.py:313-323 after the forward, :274-295 before it) ----
class Countdown:
    """host restatement of what DeviceCodebookRefresh keeps on the GPU: int32 countdowns, the dead count / ascending dead list as
    of the end of the last after_forward, a buffer that holds the last min(stored, buffer_size + 1) maps"""

    def __init__(self, n, cfg):
        self.cfg, self.n = dict(cfg), n
        self.timeout = int(cfg.get("online_kmeans_word_timeout", 10))
        self.countdown = np.full(n, self.timeout, np.int32)
        self.dead = np.arange(n, dtype=np.int32)[:n if self.timeout <= 0 else 0]
        self.stored = 0

    def started(self, step):
        return step >= self.cfg.get("start_global_step", 0)

    def before_step(self, step):
        """-> the dead list the refresh replaces at this step ([] when it does not fire)"""
        if not self.started(step):
            return []
        buffered = min(self.stored, self.cfg["train_feature_buffer_size"] + 1)
        if not (step % self.cfg["frequency"] == 0 and buffered >= self.cfg["train_feature_buffer_size"]):
            return []
        if not len(self.dead) / self.n > self.cfg["inactive_threshold"]:
            return []
        dead = [int(j) for j in self.dead]
        self.countdown[self.dead] = self.timeout          # sgam_codebook_scatter_rows_f32 with a countdown
        self.dead = self.dead[:0]
        return dead

    def after_forward(self, step, first_image_indices):
        if not self.started(step):
            return
        self.countdown[np.asarray(first_image_indices).reshape(-1)] = self.timeout     # sgam_codebook_countdown_i32
        self.countdown -= 1
        self.dead = np.nonzero(self.countdown <= 0)[0].astype(np.int32)
        self.stored += 1


# ---- fixtures ----
def mixture(N, D, k, sep, seed):
    """N points around k Gaussian centres of scale `sep` with unit noise, fp32; init = k distinct points"""
    rng = np.random.default_rng(seed)
    cent = (rng.standard_normal((k, D)) * sep).astype(np.float32)
    x = (cent[rng.integers(0, k, N)] + rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    init = x[rng.choice(N, k, replace=False)].copy()
    return x, init


def guarded(x, init, iters=ITER, margin=MARGIN, max_drop=0.02, max_rounds=5):
    """drop every point whose relative top-2 margin falls below `margin` at any of the `iters` iterations of the fp64 oracle, and
    repeat (removing points moves the centres) until none is dropped.  The init rows are kept as they are (they need not be data
    rows).  Asserts the caps: at most `max_drop` of the points, at most `max_rounds` rounds.  -> (x, centres, labels, rounds)"""
    n0 = len(x)
    for rnd in range(1, max_rounds + 1):
        c, lab, m = lloyd(x, init, iters)
        bad = m < margin
        if not bad.any():
            assert n0 - len(x) <= max_drop * n0, f"margin guard dropped {n0 - len(x)} of {n0} points"
            return x, c, lab, rnd
        x = np.ascontiguousarray(x[~bad])
        assert n0 - len(x) <= max_drop * n0, f"margin guard dropped {n0 - len(x)} of {n0} points"
    raise AssertionError(f"margin guard did not settle in {max_rounds} rounds")
