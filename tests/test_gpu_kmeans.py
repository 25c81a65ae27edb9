"""GPU: the device-resident k-means codebook refresh (csrc/kmeans.hip, sgam_neurips22_amd/kmeans.py,
training.DeviceCodebookRefresh) against the fp64 host restatement of tests/kmeans_oracle.py (pinned to scipy's kmeans2 in
tests/test_kmeans_cpu.py), against scipy itself, and against the host refresh inside the training step.

Bit-equal labels are asked on margin-guarded inputs only: the generator (kmeans_oracle.guarded) drops every point whose relative
top-2 margin is below 1e-4 at any iteration of the fp64 oracle and asserts that this costs at most 2 % of the points in at most
5 rounds.  The no-sync property is checked by capturing a non-firing step's refresh calls into a HIP graph on a side stream
(capture fails on any synchronisation) and by counting Tensor.item calls on steps that may fire."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import kmeans, testing, training
from sgam_neurips22_amd.config import default_params
from sgam_neurips22_amd.generative_sensing_module.model import VQModel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_oracle as KO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CENTRE_TOL = 2e-5            # tests/test_kmeans_cpu.py: 4 x the measured scipy-float32 vs fp64 difference on unit-noise data


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_FIX = {}


def _fixture(name):
    """margin-guarded inputs, generated once per session: (x, init, centres fp64 after 10 iterations, labels, iterations guarded)"""
    if name not in _FIX:
        if name == "k96":
            x, init = KO.mixture(4096, 256, 96, 4.0, 1)
            init[5] = init[4]                      # duplicate row (exact tie -> lower index) and a row that never gets members
            init[9] = 50.0
            iters = KO.ITER
        elif name == "k64":
            x, init = KO.mixture(8192, 256, 64, 4.0, 0)
            iters = KO.ITER
        else:                                      # k = 1639 (the CLEVR config's 0.1 * 16 384 + 1): the assignment alone
            x, init = KO.mixture(12288, 256, 1639, 4.0, 2)
            iters = 1
        n0 = len(x)
        gx, c, lab, rounds = KO.guarded(x, init, iters)
        print(f"fixture {name}: {n0 - len(gx)} of {n0} points dropped by the margin guard in {rounds} round(s)")
        _FIX[name] = (gx, init, c, lab, iters)
    return _FIX[name]


# ------------------------------------------------------------------------------------------------------------------ assign
@pytest.mark.parametrize("name", ["k96", "k64", "k1639"])
def test_assign_labels_are_bit_equal_to_the_oracle(name):
    x, init, c, lab, iters = _fixture(name)
    N = len(x)
    xd = _dev(x)
    want0, m0 = KO.assign(x, init)
    assert m0.min() >= KO.MARGIN or name == "k96"          # (k96: the duplicated row is an EXACT tie, margin 0, first index wins)
    runs = {}
    for chunk in (None, 1000, 128, N + 5):                 # default, N not a multiple of the chunk, small tiles, unchunked
        got = kmeans.assign(xd, _dev(init), chunk=chunk).cpu().numpy()
        runs[chunk] = got
        print(f"assign {name} chunk {chunk}: {(got != want0).sum()} of {N} labels differ from the oracle")
    for chunk, got in runs.items():
        assert got.dtype == np.int32 and np.array_equal(got, want0), chunk
    if iters == KO.ITER:                                   # the last iteration's centres as well (fp64 centres rounded to fp32)
        c32 = c.astype(np.float32)
        want, m = KO.assign(x, c32)
        keep = m >= KO.MARGIN                              # rounding the centres to fp32 moves the margins a little: compare inside them
        got = kmeans.assign(xd, _dev(c32)).cpu().numpy()
        assert keep.mean() > 0.98 and np.array_equal(got[keep], want[keep])


def test_assign_ignores_the_padding_rows():
    """k = 1 .. 130: tables padded to 128 / 256 rows; a padded row (|c|^2 = +inf) never wins, even for points far from every centre"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((300, 32)) * 100).astype(np.float32)
    for k in (1, 3, 127, 129, 130):
        c = rng.standard_normal((k, 32)).astype(np.float32)
        if k >= 3:
            c[k - 1] = c[0]                                    # an exact tie: the first index wins, the duplicate never does
        got = kmeans.assign(_dev(x), _dev(c)).cpu().numpy()
        want, m = KO.assign(x, c)
        assert got.min() >= 0 and got.max() < k
        if k >= 3:
            assert (got != k - 1).all() and (got == 0).any() == (want == 0).any()
        assert np.array_equal(got[m >= KO.MARGIN], want[m >= KO.MARGIN])


# ------------------------------------------------------------------------------------------------------------------ update
def _within_one_ulp(got, want64):
    w = want64.astype(np.float32)
    return (got == w) | (got == np.nextafter(w, np.float32(np.inf))) | (got == np.nextafter(w, np.float32(-np.inf)))


@pytest.mark.parametrize("labels_kind", ["oracle", "skewed"])
def test_update_means_counts_empty_centres_and_determinism(labels_kind):
    x, init, c, lab, _ = _fixture("k96")
    N, k = len(x), len(init)
    if labels_kind == "skewed":                            # one cluster holds most of the points, several hold none, some are out of range
        rng = np.random.default_rng(5)
        lab = np.where(rng.uniform(size=N) < 0.7, 17, rng.integers(0, k // 2, N)).astype(np.int32)
    prev = init.copy()
    want, count = KO.update(x, lab, prev)
    xd, ld = _dev(x), _dev(lab.astype(np.int32))
    runs = []
    for bp in (0, 0, 256, 4096):
        cd = _dev(prev)
        cnt = kmeans.update(xd, ld, cd, block_points=bp)
        runs.append((cd.cpu().numpy(), cnt.cpu().numpy()))
    got, gcount = runs[0]
    assert np.array_equal(gcount, count)
    ok = _within_one_ulp(got, want)
    print(f"update {labels_kind}: {(~ok).sum()} of {ok.size} centre values beyond 1 ulp of fp32(fp64 mean); "
          f"{(got != want.astype(np.float32)).sum()} not equal to it; empty clusters {(count == 0).sum()}")
    assert ok.all()
    empty = count == 0
    assert empty.any() and np.array_equal(got[empty].view(np.uint32), prev[empty].view(np.uint32))      # bit-equal to the previous value
    for other, ocount in runs[1:]:                         # run to run, and under other block sizes: bit-identical
        assert np.array_equal(other.view(np.uint32), got.view(np.uint32)) and np.array_equal(ocount, gcount)


def test_update_ignores_labels_out_of_range():
    x = np.arange(8 * 32, dtype=np.float32).reshape(8, 32)
    prev = np.full((3, 32), -1.0, np.float32)
    cd = _dev(prev)
    cnt = kmeans.update(_dev(x), _dev(np.array([0, 5, -1, 0, 2, 2, 2, 99], np.int32)), cd)
    assert cnt.cpu().tolist() == [2, 0, 3]
    got = cd.cpu().numpy()
    assert np.array_equal(got[0], x[[0, 3]].mean(0)) and np.array_equal(got[1], prev[1]) and np.array_equal(got[2], x[[4, 5, 6]].mean(0))


# ------------------------------------------------------------------------------------------------------------------ kmeans2
@pytest.mark.parametrize("name", ["k96", "k64"])
def test_kmeans2_matrix_matches_scipy(name):
    from scipy.cluster.vq import kmeans2 as scipy_kmeans2
    x, init, c64, lab64, _ = _fixture(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c_s, l_s = scipy_kmeans2(x, init.copy(), iter=10, minit="matrix", missing="warn")
    init_d = _dev(init)
    c_d, l_d = kmeans.kmeans2(_dev(x), init_d, iter=10, minit="matrix")
    c_d, l_d = c_d.cpu().numpy(), l_d.cpu().numpy()
    err_s, err_o = np.abs(c_d - c_s).max(), np.abs(c_d.astype(np.float64) - c64).max()
    print(f"kmeans2 {name}: labels vs scipy {(l_d != l_s).sum()} differ, vs oracle {(l_d != lab64).sum()}; "
          f"max|dcentre| vs scipy {err_s:.2e}, vs oracle {err_o:.2e}")
    assert np.array_equal(l_d, l_s) and np.array_equal(l_d, lab64)
    assert err_s <= CENTRE_TOL and err_o <= CENTRE_TOL
    assert np.array_equal(init_d.cpu().numpy(), init)       # the initial matrix is not modified
    # a different chunk size: the same bits
    c2, l2 = kmeans.kmeans2(_dev(x), init_d, iter=10, minit="matrix", chunk=512)
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), c_d.view(np.uint32)) and np.array_equal(l2.cpu().numpy(), l_d)


@pytest.mark.parametrize("N,k", [(4096, 96), (5000, 1639), (17, 17), (100000, 64)])
def test_init_points_equal_the_oracle_picks(N, k):
    rng = np.random.default_rng(N)
    x = rng.standard_normal((N, 32)).astype(np.float32)
    xd = _dev(x)
    for seed, refresh in ((0, 0), (7, 3), (2 ** 40 + 5, 2 ** 33 + 1)):
        c, picks = kmeans.init_points(xd, k, seed=seed, refresh=refresh)
        want = KO.pick_points(N, k, seed, refresh)
        assert np.array_equal(picks.cpu().numpy(), want)
        assert np.array_equal(c.cpu().numpy().view(np.uint32), x[want].view(np.uint32))
    # kmeans2(minit='points') starts from exactly those rows: one iteration equals the matrix form given them
    a = kmeans.kmeans2(xd, k, iter=1, minit="points", seed=7, refresh=3)
    b = kmeans.kmeans2(xd, _dev(x[KO.pick_points(N, k, 7, 3)]), iter=1, minit="matrix")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# --------------------------------------------------------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize("n,T", [(64, 16), (100, 7), (16384, 256), (5000, 3000)])
def test_countdown_and_scatter_kernels_follow_the_rule(n, T):
    cfg = {"online_kmeans_word_timeout": 3, "train_feature_buffer_size": 0, "frequency": 1, "inactive_threshold": -1.0}
    host = KO.Countdown(n, cfg)
    cd = torch.full((n,), 3, device=DEV, dtype=torch.int32)
    n_dead = torch.zeros((1,), device=DEV, dtype=torch.int32)
    dead = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    rng = np.random.default_rng(n)
    D = 8
    book = rng.standard_normal((n, D)).astype(np.float32)
    book_d = _dev(book)
    for step in range(9):
        idx = rng.integers(0, max(n // 3, 1), T) + (step // 3) * (n // 3)
        kmeans.codebook_countdown(_dev(idx.astype(np.int64)), cd, 3, n_dead, dead)
        host.after_forward(step, idx)
        nd = int(n_dead.item())
        assert nd == len(host.dead) and np.array_equal(dead[:nd].cpu().numpy(), host.dead)
        assert np.array_equal(cd.cpu().numpy(), host.countdown)
        if step % 4 == 3 and nd:                           # a refresh: rows scattered, their countdowns reset
            centres = rng.standard_normal((nd, D)).astype(np.float32)
            kmeans.scatter_rows(book_d, _dev(centres), dead, nd, countdown=cd, timeout=3)
            book[host.dead] = centres
            assert host.before_step(step) == dead[:nd].cpu().tolist()
            assert np.array_equal(book_d.cpu().numpy().view(np.uint32), book.view(np.uint32))
            assert np.array_equal(cd.cpu().numpy(), host.countdown)


class _Quant(torch.nn.Module):
    def __init__(self, n, D):
        super().__init__()
        self.embedding = torch.nn.Embedding(n, D)


class _Stub(torch.nn.Module):
    def __init__(self, n=64, D=32):
        super().__init__()
        self.quantize = _Quant(n, D)


def test_non_firing_step_does_not_synchronise(monkeypatch):
    """chosen check: the refresh calls of a non-firing step are captured into a HIP graph on a side stream — any device-to-host copy
    or synchronisation would fail the capture — and the replayed graph does the bookkeeping.  On a step that may fire exactly one
    Tensor.item (the 4-byte dead count) happens, counted at the Python level."""
    n, D, T = 64, 32, 16
    cfg = {"do_online_kmeans_clustering": True, "online_kmeans_word_timeout": 2, "inactive_threshold": 0.9,
           "train_feature_buffer_size": 2, "frequency": 4, "start_global_step": 0}
    r = training.DeviceCodebookRefresh(_Stub(n, D).to(DEV), cfg, seed=1)
    host = KO.Countdown(n, cfg)
    idx = torch.arange(2 * T, device=DEV, dtype=torch.int64).reshape(2, 4, 4) % 8
    z = torch.randn((1, 4, 4, D), device=DEV)
    for step in (1, 2, 3):                                   # warm-up outside the capture: the ring exists, the ring has wrapped
        assert r.before_step(step) == 0
        r.after_forward(step, idx, z)
        host.after_forward(step, idx[0].cpu().numpy())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                # captures on a side stream
        assert r.before_step(5) == 0                         # 5 % 4 != 0: decided on the host
        r.after_forward(5, idx, z * 2)
    g.replay()
    torch.cuda.synchronize()
    host.after_forward(5, idx[0].cpu().numpy())
    assert np.array_equal(r.countdown.cpu().numpy(), host.countdown)
    assert int(r.n_dead.item()) == len(host.dead) and np.array_equal(r.dead[:len(host.dead)].cpu().numpy(), host.dead)
    assert torch.equal(r.ring[3 % 3], (z * 2).reshape(T, D)) and r.stored == 4
    # Python-level count of host reads
    calls = []
    real_item = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (calls.append(1), real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError(".cpu() inside the refresh")))
    assert r.before_step(6) == 0 and r.before_step(7) == 0
    r.after_forward(7, idx, z)
    assert calls == []
    assert r.before_step(8) == 0                             # may fire: the dead count is read (56 / 64 is not above 0.9)
    assert calls == [1]


# --------------------------------------------------------------------------------------------------------------- end to end
def _trainer(backend, golden):
    g0 = golden("train_step_small.npz")
    p = testing.small_train_params(default_params("google_earth"))
    p["phase"] = "codebook"
    p["online_kmeans_config"] = {"do_online_kmeans_clustering": True, "online_kmeans_word_timeout": 2, "inactive_threshold": 0.3,
                                 "train_feature_buffer_size": 2, "frequency": 3, "start_global_step": 1,
                                 "kmean_init_codebook_path": None}
    if backend is not None:
        p["online_kmeans_config"].update(backend=backend, seed=5)
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=11)
    cb = testing.codebook_from_stats(float(g0["zmean"]), float(g0["zstd"]), 64, 32, int(g0["cb_seed"]))
    cb[32:] += 100.0                                         # half of the words are out of reach: they die and are refreshed
    sd["quantize.embedding.weight"] = cb
    m.load_state_dict(sd)
    m = m.to(DEV)
    return m, training.AutoencoderTrainer(m, phase="codebook", lr=1e-4)


def _run(tr, m, steps):
    """-> [(step, dead list, codebook right after the refresh, the quantiser's cached copy right after it)]"""
    x, mask, x_dst = (t.to(DEV) for t in testing.train_batch())
    fires = []
    inner = tr.refresh.before_step

    def before_step(step):
        old = m.quantize.embedding.weight.data.clone()
        n = inner(step)
        if n:
            new = m.quantize.embedding.weight.data.clone()
            changed = torch.nonzero((new != old).any(1)).reshape(-1).cpu().tolist()
            fires.append({"step": step, "n": n, "changed": changed, "old": old.cpu().numpy(), "new": new.cpu().numpy(),
                          "cached": m.quantize._codebook()[0].clone().cpu().numpy()})
        return n
    tr.refresh.before_step = before_step
    for _ in range(steps):
        tr.step(x, x_dst, mask)
    return fires


def test_device_refresh_matches_the_host_refresh_in_the_training_step(golden, monkeypatch):
    import scipy.cluster.vq
    real_kmeans2 = scipy.cluster.vq.kmeans2
    md, trd = _trainer("device", golden)
    assert isinstance(trd.refresh, training.DeviceCodebookRefresh) and trd.refresh.seed == 5
    dev_fires, dev_meta = [], []
    inner = trd.refresh.before_step

    def dev_before(step):
        n = inner(step)
        if n:
            dev_meta.append((dict(trd.refresh.last_fire), trd.refresh.dead[:n].cpu().tolist()))
        return n
    trd.refresh.before_step = dev_before
    dev_fires = _run(trd, md, 8)
    assert dev_fires and dev_fires[0]["step"] == 3, [f["step"] for f in dev_fires]

    mh, trh = _trainer(None, golden)                         # no "backend" key: the host refresh, as with the shipped YAMLs
    assert type(trh.refresh) is training.OnlineCodebookRefresh
    host_dead = []

    def kmeans2_with_the_device_picks(data, k, minit="points"):
        """the host refresh, its random init replaced by the rows the device picked (minit='matrix'): the ring's storage order is
        the host buffer's oldest-first order rotated by whole maps"""
        meta, _ = dev_meta[len(host_dead)]
        maps = meta["maps"]
        ring = np.roll(np.asarray(data).reshape(maps, -1, data.shape[1]), meta["oldest_slot"], axis=0).reshape(-1, data.shape[1])
        picks = KO.pick_points(len(ring), k, 5, meta["refresh"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return real_kmeans2(data, ring[picks].copy(), iter=10, minit="matrix", missing="warn")
    monkeypatch.setattr(scipy.cluster.vq, "kmeans2", kmeans2_with_the_device_picks)
    real_update = mh.quantize.update_codebook

    def update_codebook(features, idx):
        real_update(features, idx)
        host_dead.append(list(idx))
    mh.quantize.update_codebook = update_codebook
    host_fires = _run(trh, mh, 8)

    print("fire steps device", [f["step"] for f in dev_fires], "host", [f["step"] for f in host_fires],
          "dead counts", [f["n"] for f in dev_fires])
    assert [f["step"] for f in dev_fires] == [f["step"] for f in host_fires]
    assert [d for _, d in dev_meta] == host_dead
    assert dev_meta[0][1][-32:] == list(range(32, 64))       # the unreachable half is among the first refresh's dead words
    # the first refresh (identical state on both sides up to it): rows
    fd, fh = dev_fires[0], host_fires[0]
    dead = dev_meta[0][1]
    alive = [j for j in range(64) if j not in dead]
    assert np.array_equal(fd["old"].view(np.uint32), fh["old"].view(np.uint32))
    err = np.abs(fd["new"][dead] - fh["new"][dead]).max()
    print(f"first refresh: {len(dead)} rows replaced, max|device - host| {err:.2e}")
    assert err <= CENTRE_TOL
    assert np.array_equal(fd["new"][alive].view(np.uint32), fd["old"][alive].view(np.uint32))           # untouched rows bit-equal
    assert set(fd["changed"]) <= set(dead) and len(fd["changed"]) >= 32
    # packs invalidated: what the quantiser's next forward reads is the refreshed codebook
    assert np.array_equal(fd["cached"].view(np.uint32), fd["new"].view(np.uint32))
    assert np.abs(fd["new"][32:]).max() < 50.0               # the unreachable rows are back among the features
    # the refreshed words' countdowns were reset on the device as on the host
    assert all(trh.refresh.countdown[j] <= 2 for j in range(64)) and int(trd.refresh.countdown.max()) <= 2


def test_unknown_backend_is_refused(golden):
    p = testing.small_train_params(default_params("google_earth"))
    p["phase"] = "codebook"
    p["online_kmeans_config"] = {"do_online_kmeans_clustering": True, "backend": "fpga", "kmean_init_codebook_path": None}
    with pytest.raises(ValueError, match="backend"):
        training.AutoencoderTrainer(VQModel(**p).to(DEV), phase="codebook")
