"""Times of the pose-graph optimiser and of its dense solve (csrc/pose_graph.hip) — the numbers of DESIGN.md §4.4.11.

    python scripts/pose_graph_time.py [--json profiles/pose_graph_time.json] [--twin-max-nodes 512] [--no-host]

On one MI355X.  The solve alone at n = 192, 768, 3072 and 6144 on a seeded SPD matrix (device events around back-to-back calls of
sgam_spd_solve_f64 with its workspace allocated once; FLOP counted as n^3 / 3 + 2 n^2 against the fp64 peak), beside
numpy.linalg.solve of the same system on the host, with the residual of both.  The optimiser at N = 32, 128, 512 and 1024 nodes on
a noisy ring with stride-8 loop closures from a perturbed start (a host clock around geometry.optimize_pose_graph with a fixed
number of attempts, which ends in the download of state and history), beside the numpy twin (tests/posegraph_oracle.py) up to
--twin-max-nodes.  No threshold was set in advance: recorded numbers, not gates."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sgam_neurips22_amd import _lib, geometry  # noqa: E402
from sgam_neurips22_amd._opscore import _p, _stream  # noqa: E402

import posegraph_oracle as PO  # noqa: E402

FP64_PEAK = 78.6e12          # scripts/feature_metrics_time.py: one v_mfma_f64_16x16x4_f64 per 64 cycles and SIMD
DEV = "cuda"
ATTEMPTS = 20


def device_ms(fn, window_s=0.3, most=200):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = int(max(3, min(most, window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def time_solve(n, host):
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(n)
    G = torch.randn((n, n), dtype=torch.float64, generator=g).to(DEV)
    A = G @ G.T / n + torch.eye(n, dtype=torch.float64, device=DEV)            # (test data by torch; the solve below is the library's)
    b = torch.randn((n,), dtype=torch.float64, generator=g).to(DEV)
    need = int(lib.sgam_spd_solve_workspace_doubles(n))
    work = torch.empty((need,), dtype=torch.float64, device=DEV)
    x, status = torch.zeros((n,), dtype=torch.float64, device=DEV), torch.zeros((1,), dtype=torch.float64, device=DEV)
    call = lambda: _lib.check(lib.sgam_spd_solve_f64(_p(A), n, n, None, _p(b), _p(work), need, _p(x), _p(status), _stream()),  # noqa: E731
                              "sgam_spd_solve_f64")
    ms, reps = device_ms(call)
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    one_call_host_ms = 1e3 * (time.perf_counter() - t)
    flop = n ** 3 / 3.0 + 2.0 * n * n
    An, bn, xn = A.cpu().numpy(), b.cpu().numpy(), x.cpu().numpy()
    scale = np.linalg.norm(An, 2) * np.linalg.norm(xn)
    rec = {"n": n, "launches": 1 + 3 * ((n + 63) // 64) - 2 + 2 * ((n + 63) // 64), "ms": ms, "reps": reps, "one_call_host_clock_ms": one_call_host_ms,
           "gflop": flop / 1e9, "tflops": flop / (ms * 1e-3) / 1e12, "fraction_of_fp64_peak": flop / (ms * 1e-3) / FP64_PEAK,
           "status": float(status.item()), "residual_over_norms": float(np.linalg.norm(An @ xn - bn) / scale)}
    if host:
        t = time.perf_counter()
        ref = np.linalg.solve(An, bn)
        rec["numpy_solve_ms"] = 1e3 * (time.perf_counter() - t)
        rec["numpy_residual_over_norms"] = float(np.linalg.norm(An @ ref - bn) / scale)
        rec["difference_to_numpy"] = float(np.linalg.norm(xn - ref) / np.linalg.norm(ref))
    print(f"solve n = {n:5d}: {ms:9.3f} ms ({rec['launches']} launches, {reps} calls)  {rec['tflops']:6.3f} TFLOP/s = "
          f"{100 * rec['fraction_of_fp64_peak']:5.2f} % of the fp64 peak, residual {rec['residual_over_norms']:.2e}"
          + (f"   numpy.linalg.solve {rec['numpy_solve_ms']:.1f} ms" if host else ""))
    return rec


def time_optimiser(n_nodes, twin):
    truth, src, dst, T, info, unc = PO.ring(n_nodes, 7, stride=8, noise=0.005)
    init = PO.perturbed(truth, 8, 0.05, 0.1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    graph = geometry.PoseGraph.from_tensors(n_nodes, t(src), t(dst), t(T), t(info), t(unc))
    start = t(init)
    run = lambda: geometry.optimize_pose_graph(graph, line_process_weight=5.0, poses=start, max_iterations=ATTEMPTS, reoptimize=False)  # noqa: E731
    out = run()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        s = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - s)
    h = out["history"]
    live = int((h[:, 2] != 0).sum() + 0)                                       # attempts that reached the decision with a step
    rec = {"nodes": n_nodes, "unknowns": 6 * n_nodes, "edges": int(len(src)), "attempts_issued": ATTEMPTS, "attempts_live": live,
           "iterations": out["iterations"], "status": out["status"], "cost": out["cost"], "end_to_end_ms": 1e3 * best,
           "largest_pose_entry_off_the_noise_free_truth": float(np.abs(out["poses"].cpu().numpy() - truth).max())}
    if twin:
        s = time.perf_counter()
        want = PO.run(init, src, dst, T, info, unc, 5.0, max_iterations=ATTEMPTS)
        rec["numpy_twin_ms"] = 1e3 * (time.perf_counter() - s)
        rec["largest_pose_entry_off_the_twin"] = float(np.abs(out["poses"].cpu().numpy() - want["poses"]).max())
        rec["twin_status"] = int(want["state"][PO.S_STATUS])
    print(f"optimiser N = {n_nodes:5d} ({len(src)} edges): {rec['end_to_end_ms']:9.2f} ms for {ATTEMPTS} attempts ({live} live, "
          f"{out['iterations']} accepted, status {out['status']})" + (f"   numpy twin {rec['numpy_twin_ms']:.0f} ms, poses off the twin "
                                                                        f"{rec['largest_pose_entry_off_the_twin']:.1e}" if twin else ""))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--twin-max-nodes", type=int, default=512)
    ap.add_argument("--no-host", action="store_true", help="skip numpy.linalg.solve and the twin")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pose_graph_time.py measures on the GPU"
    lib = _lib.load()
    out = {"script": "pose_graph_time", "device": torch.cuda.get_device_name(0), "build": lib.sgam_build_commit().decode(),
           "fp64_peak_tflops": FP64_PEAK / 1e12, "unit": "ms", "solve": [], "optimiser": []}
    for n in (192, 768, 3072, 6144):
        out["solve"].append(time_solve(n, not a.no_host))
    for n_nodes in (32, 128, 512, 1024):
        out["optimiser"].append(time_optimiser(n_nodes, not a.no_host and n_nodes <= a.twin_max_nodes))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
