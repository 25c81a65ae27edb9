"""Record what the registration stack computes into tests/golden/registration_hashes.json.

The registration code of sgam_neurips22_amd/geometry.py and its kernels (csrc/point_icp.hip, csrc/point_global.hip) may be
rearranged, never change a bit: per case of `cases()` the file holds the sha256 of the raw bytes of every output tensor, every
float of a result dict as the sha256 of its fp64 bits, and the integers, booleans and texts of the dict as they are.
tests/test_gpu_registration_hashes.py replays the cases against the file.  Only public names of `geometry` are called.

The file is recorded from a build of the commit BEFORE a change to that code and names that build (`recorded_from`, `lib_digest`:
sgam_build_commit / sgam_build_digest of the library that ran).  It is never re-recorded from the code under test:

    python -m sgam_neurips22_amd.build                          # in a checkout of the earlier commit
    python scripts/record_registration_hashes.py                (needs the GPU; this file copied into that checkout)

Cases: transform_points (257 points, a NaN row, the pose as numpy and as a device tensor); icp_accumulate (point-to-point,
point-to-plane) and icp_accumulate_colored (lambda 0.968, 1, 0) at 255 and 4097 source points against 300 target points with a NaN
source row, an index of -1, an index past the target, NaN target normals and gradients, once into a fresh and once into a given
buffer; icp_update on every path (a step, the small-angle branch, converged, fewer than 6 correspondences, a pivot refusal, a frozen
state); color_gradients at (300, k = 8) and (70, k = 32) with NaN normals and points, a collinear cluster, and rows given by the
caller with holes, entries out of range and rows cut to two neighbours; evaluate_registration / register_icp on 500 against 600
points (a given init, the three estimations, brute force and grid, check_every 1 / 8 / None, NaN rows); register_icp_multiscale
over two levels, one of them not sampled, with NaN rows; the RANSAC pieces and register_ransac on 300 against 300 points with 200
correspondences of which half are wrong (ransac_n 3 / 4, refits 0 / 4, and a distance no hypothesis meets); register_global on
about 1500 points per side from the 140 degree motion (viewpoints in both forms, NaN rows, refine point_to_plane / None).
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import colored_icp_oracle as CIO  # noqa: E402
import global_registration_oracle as GR  # noqa: E402
import icp_oracle as IO  # noqa: E402
from sgam_neurips22_amd import _lib, geometry, testing  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "registration_hashes.json")
DEV = "cuda"
f32 = np.float32
DISTANCE = 0.5                    # the correspondence distance of the surface cases (tests/test_icp_cpu.py: MAX_DISTANCE)
ESTIMATIONS = ("point_to_plane", "point_to_point", "colored")
LINE = 40                         # points of the collinear cluster of the gradient cases: more than the largest k


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pose32(T):
    """a pose whose entries are fp32 numbers (held in fp64): the same bits whatever the host's sin and cos round to"""
    return np.asarray(T, dtype=np.float64).astype(f32).astype(np.float64)


def _hashes(v):
    """the recorded form of a result: tensors and arrays -> sha256 of their bytes, floats -> sha256 of their fp64 bits, dicts and
    lists element by element, integers / booleans / texts / None as they are"""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return testing.sha256(v).hex()
    if isinstance(v, dict):
        return {str(k): _hashes(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_hashes(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return "f64:" + testing.sha256(np.array([v], dtype=np.float64)).hex()
    assert v is None or isinstance(v, str), type(v)
    return v


def _with_nan_rows(arrays, n_out, seed):
    """the rows of every array of `arrays` (one length) spread in order over n_out rows; the rows between are NaN (0 where the array
    is uint8).  -> the list of the longer arrays"""
    n = len(arrays[0])
    rows = np.sort(np.random.RandomState(seed).choice(n_out, n, replace=False))
    out = []
    for a in arrays:
        b = np.zeros((n_out,) + a.shape[1:], dtype=a.dtype) if a.dtype == np.uint8 else np.full((n_out,) + a.shape[1:], np.nan, dtype=a.dtype)
        b[rows] = a
        out.append(b)
    return out


# ---------------------------------------------------------------- transform
def _run_transform(case):
    p = IO.surface(257, 357)[0]
    p[100] = np.nan
    T = IO.perturbation()
    return {"numpy": geometry.transform_points(_t(p), T), "tensor": geometry.transform_points(_t(p), _t(T))}


# ---------------------------------------------------------------- accumulate
def _accumulate_inputs(n):
    nr = 300
    tgt, nrm, tc = CIO.textured_surface(nr, 7, -0.3, 4.3)
    grad = CIO.color_gradient(tgt, nrm, tc, CIO.knn_rows(tgt, 16))
    src, _, sc = CIO.textured_surface(n, 200 + n)
    moved = IO.transform(src, IO.rigid(1.0, [0.3, 1.0, -0.2], [0.01, 0.02, -0.01]))
    moved[np.arange(n) % 11 == 5] = np.nan                              # source rows that are not points
    nn = geometry.nearest_neighbors(_t(moved), _t(tgt), max_distance=DISTANCE)
    index, d2 = nn["index"].cpu().numpy().copy(), nn["d2"].cpu().numpy().copy()
    erased = np.arange(n) % 7 == 3
    index[erased], d2[erased] = -1, np.inf
    index[np.arange(n) % 19 == 4] = nr                                  # an index equal to Nr: refused, not read
    nrm, grad = nrm.copy(), grad.copy()
    nrm[::13] = np.nan
    grad[::17] = np.nan
    return dict(moved=_t(moved), sc=_t(sc), tgt=_t(tgt), nrm=_t(nrm), tc=_t(tc), grad=_t(grad), index=_t(index), d2=_t(d2))


def _run_accumulate(case):
    a = _accumulate_inputs(case["n"])
    blocks = (case["n"] + 4095) // 4096

    def call(partials=None):
        if case["kind"] == "colored":
            return geometry.icp_accumulate_colored(a["moved"], a["sc"], a["tgt"], a["nrm"], a["tc"], a["grad"], a["index"], a["d2"], case["lam"],
                                                   partials=partials)
        return geometry.icp_accumulate(a["moved"], a["tgt"], a["nrm"] if case["kind"] == "point_to_plane" else None, a["index"], a["d2"],
                                       partials=partials)

    fresh = call()
    given = torch.full((blocks, 32), -7.0, dtype=torch.float64, device=DEV)
    back = call(given)
    assert back.data_ptr() == given.data_ptr() and tuple(fresh.shape) == (blocks, 32)
    return {"partials": fresh, "given": given, "correspondences": int(fresh[:, 29].sum().item())}


# ---------------------------------------------------------------- update
def _exact_copy(n, seed=5):
    """tests/test_icp_cpu.py's exact_copy: (source, the source moved by the perturbation, the moved normals)"""
    src, nrm = IO.surface(n, seed)
    T = IO.perturbation()
    return src, IO.transform(src, T), (nrm.astype(np.float64) @ T[:3, :3].T).astype(f32)


def _sums(src, tgt, nrm, init, rows=None):
    """the device's own chunk sums of `src` moved by `init` against `tgt` (point-to-plane)"""
    moved = geometry.transform_points(_t(src), init)
    nn = geometry.nearest_neighbors(moved, _t(tgt), max_distance=DISTANCE)
    if rows is not None:
        moved, nn = moved[:rows].contiguous(), {k: v[:rows].contiguous() for k, v in nn.items()}
    return geometry.icp_accumulate(moved, _t(tgt), _t(nrm), nn["index"], nn["d2"])


def _update(partials, iteration, state):
    s, h = _t(np.asarray(state, dtype=np.float64)), torch.full((4, 8), -7.0, dtype=torch.float64, device=DEV)
    geometry.icp_update(partials, iteration, 1e-6, 1e-6, s, h)
    return s, h


def _run_update(case):
    src, tgt, nrm = _exact_copy(1000)
    init = _pose32(IO.rigid(0.5, [0, 1, 0], [0.01, 0.0, -0.01]))
    partials = _sums(src, tgt, nrm, init)
    partials = torch.cat([partials * 0.25, partials * 0.5, partials * 0.25]).contiguous()     # three chunks to fold (exact scalings)
    out = {}
    step_s, step_h = _update(partials, 0, IO.new_state(init))
    out["step"] = {"state": step_s, "history": step_h}
    assert float(step_s[18]) == 0 and float(step_s[19]) == 1
    # the small-angle branch: a cloud against itself from the identity
    same = _sums(tgt, tgt, nrm, np.eye(4))
    small_s, small_h = _update(same, 0, IO.new_state())
    out["small_angle"] = {"state": small_s, "history": small_h}
    assert float(small_s[18]) == 0 and float(small_s[19]) == 1
    # converged: the same sums at iteration 3 with the current fitness and RMSE as the previous ones
    moving = step_s.cpu().numpy().copy()
    moving[:16], moving[19] = IO.new_state(init)[:16], 0.0
    conv_s, conv_h = _update(partials, 3, moving)
    out["converged"] = {"state": conv_s, "history": conv_h}
    assert float(conv_s[18]) == 1
    # fewer than six correspondences
    few_s, few_h = _update(_sums(src, tgt, nrm, init, rows=5), 0, IO.new_state(init))
    out["few"] = {"state": few_s, "history": few_h}
    assert float(few_s[18]) == 2 and float(few_s[20]) == 5
    # a pivot refusal: tests/test_icp_cpu.py's plane_case, which slides along itself
    rs = np.random.RandomState(9)
    p = np.stack([rs.uniform(0, 4, 500), rs.uniform(0, 4, 500), np.zeros(500)], 1).astype(f32)
    slide = _pose32(IO.rigid(1.0, [0, 0, 1], [0.01, 0.0, 0.0]))
    plane_s, plane_h = _update(_sums(p, p.copy(), np.tile(np.array([0, 0, 1], dtype=f32), (500, 1)), slide), 0, IO.new_state(slide))
    out["pivot"] = {"state": plane_s, "history": plane_h}
    assert float(plane_s[18]) == 2 and float(plane_s[20]) == 500
    # a call on a frozen state
    for name, frozen in (("frozen_converged", conv_s), ("frozen_degenerate", few_s)):
        s, h = _update(partials, 2, frozen.cpu().numpy())
        out[name] = {"state": s, "history": h}
        assert torch.equal(s.view(torch.int64), frozen.view(torch.int64))
    return out


# ---------------------------------------------------------------- gradients
def _run_gradients(case):
    n, k = case["n"], case["k"]
    p, nrm, col = CIO.textured_surface(n, 300 + n)
    first = 10 if n < 257 else 100
    line = np.arange(first, first + LINE)
    p[line] = np.stack([10.0 + 0.01 * np.arange(LINE), np.full(LINE, 10.0), np.full(LINE, 1.0)], 1).astype(f32)
    rs = np.random.RandomState(n)
    bad = rs.uniform(size=n) < 0.2
    bad[line] = False
    p[bad] = np.nan
    nrm[rs.uniform(size=n) < 0.1] = np.nan
    nrm[line] = np.array([0.0, 0.6, 0.8], dtype=f32)
    P, N, C = _t(p), _t(nrm), _t(col)
    out = {m: geometry.color_gradients(P, N, C, k=k, method=m) for m in ("brute", "grid")}
    assert bool(torch.isnan(out["brute"][torch.from_numpy(line).to(DEV)]).all()) and bool(torch.isfinite(out["brute"]).any())
    # rows given by the caller: holes in the middle of a row, entries past the cloud, rows cut to two neighbours
    rows = geometry.knn(P, P, k, exclude_self=True)["index"].cpu().numpy().copy()
    rows[::3, k // 2] = -1
    rows[1::5, 0] = n + 7
    rows[2::7, 2:] = -1
    out["rows"] = geometry.color_gradients(P, N, C, k=k, knn_index=_t(rows))
    assert bool(torch.isnan(out["rows"][2::7]).all())
    return out


# ---------------------------------------------------------------- the loop
def _icp_inputs(nan_rows):
    """500 source points of the textured surface against 600 other samples of it moved by the perturbation, from a pose 1 degree
    and 0.03 off the truth"""
    src, _, sc = CIO.textured_surface(500, 5, 0.3, 3.7)
    other, nrm, oc = CIO.textured_surface(600, 6)
    T = IO.perturbation()
    tgt, tn, tc = CIO.moved_target(other, nrm, oc, T)
    if nan_rows:
        src, sc = _with_nan_rows([src, sc], 560, 12)
        tgt, tn, tc = _with_nan_rows([tgt, tn, tc], 650, 13)
        tn[::29] = np.nan
    init = _pose32(IO.rigid(1.0, [0.2, 1.0, 0.3], [0.02, -0.01, 0.02]) @ T)
    return _t(src), _t(sc), _t(tgt), _t(tn), _t(tc), init


def _icp_kw(estimation, tn, sc, tc):
    kw = dict(estimation=estimation, target_normals=None if estimation == "point_to_point" else tn)
    if estimation == "colored":
        kw.update(source_colors=sc, target_colors=tc)
    return kw


def _run_icp(case):
    src, sc, tgt, tn, tc, init = _icp_inputs(case["nan_rows"])
    kw = _icp_kw(case["estimation"], tn, sc, tc)
    out = {"evaluate": geometry.evaluate_registration(src, tgt, DISTANCE, transformation=init, method=case["method"]),
           "evaluate_identity": geometry.evaluate_registration(src, tgt, DISTANCE, method=case["method"])}
    for ce in (1, 8, None):
        out[f"check_every_{ce}"] = geometry.register_icp(src, tgt, DISTANCE, init=init, max_iterations=12, method=case["method"], check_every=ce, **kw)
    out["init_tensor"] = geometry.register_icp(src, tgt, DISTANCE, init=_t(init), max_iterations=12, method=case["method"], **kw)
    assert out["check_every_8"]["history"].shape[0] >= 2
    return out


def _run_multiscale(case):
    p, nrm, col = CIO.textured_surface(1500, 5)
    C = np.eye(4)
    C[:3, 3] = [2.0, 2.0, 0.5]
    T = C @ IO.rigid(5.0, [1.0, -2.0, 1.5], [0.1, -0.1, 0.5]) @ np.linalg.inv(C)
    tgt, _, tc = CIO.moved_target(p, nrm, col, T)
    src, sc = _with_nan_rows([p, col], 1600, 21)
    tgt, tc = _with_nan_rows([tgt, tc], 1650, 22)
    colours = dict(source_colors=_t(sc), target_colors=_t(tc)) if case["estimation"] == "colored" else {}
    out = geometry.register_icp_multiscale(_t(src), _t(tgt), [0.3, None], [0.9, 0.2], [12, 6], estimation=case["estimation"], **colours)
    assert out["levels"][0]["n_source"] < 1500 and (out["levels"][1]["n_source"], out["levels"][1]["n_target"]) == (1600, 1650)
    return out


# ---------------------------------------------------------------- RANSAC
def _run_ransac(case):
    src = IO.surface(300, 60)[0]
    tgt = IO.transform(src, GR.far_motion())
    rs = np.random.RandomState(4)
    corr = np.stack([np.arange(200), np.arange(200)], axis=1).astype(np.int32)
    wrong = np.arange(200) % 2 == 1
    corr[wrong, 1] = rs.randint(0, 300, wrong.sum())
    src[7] = np.nan
    corr[12] = (305, 2)
    corr[14] = (3, -1)
    s, t, c = _t(src), _t(tgt), _t(corr)
    distance, n = case["distance"], case["ransac_n"]
    hyp = geometry.ransac_hypotheses(s, t, c, distance, 1024, n, 0.9, 17)
    out = {"hypotheses": hyp}
    for compact in (True, False):
        out[f"score_compact_{compact}"] = score = geometry.ransac_score(s, t, c, hyp["poses"], hyp["valid"], distance, compact=compact)
    out["inliers"] = geometry.ransac_inliers(s, t, c, hyp["poses"], score["best"], distance)
    out["inliers_given_state"] = geometry.ransac_inliers(s, t, c, hyp["poses"], score["best"], distance,
                                                         state=torch.arange(24, dtype=torch.float64, device=DEV))
    for refits in (0, 4):
        out[f"register_refit_{refits}"] = geometry.register_ransac(s, t, c, distance, max_iterations=1024, ransac_n=n, seed=17, refit_iterations=refits)
    assert (out["register_refit_4"]["status"] == 2) == case["void"] and (int(hyp["valid"].sum().item()) == 0) == case["void"]
    return out


# ---------------------------------------------------------------- global registration
def _run_global(case):
    T = GR.far_motion()
    tgt0 = IO.surface(1600, 10)[0]
    src0 = tgt0[np.random.RandomState(0).permutation(1600)[:1550]]
    src, = _with_nan_rows([src0], 1650, 31)
    tgt, = _with_nan_rows([IO.transform(tgt0, T)], 1700, 32)
    view = np.array([2.0, 2.0, 50.0])
    moved_view = T[:3, :3] @ view + T[:3, 3]
    if case["views"] == "one":
        sv, tv = _t(view.astype(f32)), _t(moved_view.astype(f32))
    else:                                       # two camera centres, the points dealt to them in turn
        off = np.array([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0]])
        sv = (_t((view + off).astype(f32)), _t((np.arange(1650) % 2).astype(np.int32)))
        tv = (_t(((view + off) @ T[:3, :3].T + T[:3, 3]).astype(f32)), _t((np.arange(1700) % 2).astype(np.int32)))
    out = geometry.register_global(_t(src), _t(tgt), 0.05, source_viewpoints=sv, target_viewpoints=tv, feature_k=24, feature_radius=0.5,
                                   max_correspondence_distance=0.15, refine=case["refine"], max_iterations=3000, seed=0)
    assert 1200 <= out["n_source"] < 1550 and 1200 <= out["n_target"] < 1600 and out["ransac"]["status"] == 0
    return out


RUN = {"transform": _run_transform, "accumulate": _run_accumulate, "update": _run_update, "gradients": _run_gradients, "icp": _run_icp,
       "multiscale": _run_multiscale, "ransac": _run_ransac, "global": _run_global}


def cases():
    out = [dict(id="transform", kind_of="transform"), dict(id="update", kind_of="update")]
    for n in (255, 4097):
        out += [dict(id=f"accumulate-{kind}-n{n}", kind_of="accumulate", kind=kind, n=n, lam=None) for kind in ("point_to_point", "point_to_plane")]
        out += [dict(id=f"accumulate-colored-lambda{lam}-n{n}", kind_of="accumulate", kind="colored", n=n, lam=lam) for lam in (0.968, 1.0, 0.0)]
    out += [dict(id=f"gradients-n{n}-k{k}", kind_of="gradients", n=n, k=k) for n, k in ((300, 8), (70, 32))]
    for estimation in ESTIMATIONS:
        out += [dict(id=f"icp-{estimation}-{method}", kind_of="icp", estimation=estimation, method=method, nan_rows=False) for method in ("brute", "grid")]
        out.append(dict(id=f"icp-{estimation}-nan_rows", kind_of="icp", estimation=estimation, method="auto", nan_rows=True))
    out += [dict(id=f"multiscale-{estimation}", kind_of="multiscale", estimation=estimation) for estimation in ("point_to_plane", "colored")]
    out += [dict(id=f"ransac-n{n}", kind_of="ransac", ransac_n=n, distance=0.05, void=False) for n in (3, 4)]
    out.append(dict(id="ransac-no_valid_hypothesis", kind_of="ransac", ransac_n=3, distance=1e-9, void=True))
    out += [dict(id=f"global-views_{views}-refine_{refine}", kind_of="global", views=views, refine=refine)
            for views in ("one", "per_point") for refine in ("point_to_plane", None)]
    return out


def run_case(case):
    """-> the nested dict of hashes and plain values of one case on the GPU"""
    with torch.no_grad():
        return _hashes(RUN[case["kind_of"]](case))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    lib = _lib.load()
    doc = {"recorded_from": lib.sgam_build_commit().decode(), "lib_digest": lib.sgam_build_digest().decode(), "cases": {}}
    for case in cases():
        first, rec = run_case(case), run_case(case)
        assert first == rec, f"{case['id']}: two runs differ: {first} {rec}"
        doc["cases"][case["id"]] = rec
        print(case["id"], "recorded", flush=True)
    with open(args.out, "w") as f:
        rows = ",\n".join(f"{json.dumps(cid)}: {json.dumps(rec)}" for cid, rec in doc["cases"].items())
        f.write('{"recorded_from": %s, "lib_digest": %s,\n"cases": {\n%s\n}}\n'
                % (json.dumps(doc["recorded_from"]), json.dumps(doc["lib_digest"]), rows))
    print("wrote", args.out, "from", doc["recorded_from"], doc["lib_digest"])


if __name__ == "__main__":
    main()
