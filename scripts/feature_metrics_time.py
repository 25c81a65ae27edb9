"""Rates of the feature-set metrics (sgam_neurips22_amd/feature_metrics.py) — the numbers of DESIGN.md §4.7.2.

    python scripts/feature_metrics_time.py [--json profiles/feature_metrics_time.json] [--no-twin]

On one MI355X, seeded |N(0, 1)| features: the fp64 Gram at N = 256 / 1024 / 4096 rows of d = 2048 and N = 4096 of d = 64 (device
events around enough back-to-back launches for a window of about 0.2 s, after a warm-up; GFLOP counted after symmetry,
2 d N (N + 1) / 2, against the fp64 peak); KID at 2048 + 2048 rows with 100 subsets of 1000 and precision / recall / density /
coverage at 2048 + 2048 rows, k = 3, each end to end (a host clock around the call, which ends in the download of its scalars)
and by launch group.  The numpy twin (tests/featmetrics_oracle.py) on the same inputs is timed beside each as context, and the
results of the two are compared.  There is no earlier path to compare with: recorded numbers, not gates."""
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

from sgam_neurips22_amd import _lib  # noqa: E402
from sgam_neurips22_amd import feature_metrics as FM  # noqa: E402
from sgam_neurips22_amd._opscore import _p, _stream  # noqa: E402

import featmetrics_oracle as FO  # noqa: E402

# fp64 peak of the MI355X, vector and matrix path alike: half of the 157.3 TFLOP/s fp32 rate of MI355X_MICROARCH.md (32 fp64
# FLOP per clock and SIMD: one v_mfma_f64_16x16x4_f64 of 2048 FLOP per 64 cycles, on 1024 SIMDs at 2.4 GHz)
FP64_PEAK = 78.6e12
DEV = "cuda"


def device_ms(fn, window_s=0.2):
    """ms per call from device events: warm-up, a probe to size the loop, then one timed window of back-to-back calls"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = int(max(3, min(2000, window_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def host_s(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def features(n, d, seed, scale=1.0, shift=0.0):
    return (np.abs(np.random.default_rng(seed).standard_normal((n, d))) * scale + shift).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-twin", action="store_true", help="skip the numpy timings")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "feature_metrics_time.py measures on the GPU"
    out = {"fp64_peak_tflops": FP64_PEAK / 1e12, "gram": []}
    lib = _lib.load()
    for n, d in ((256, 2048), (1024, 2048), (4096, 2048), (4096, 64)):
        z = features(n, d, n + d)
        zd = torch.from_numpy(z).to(DEV)
        G = torch.empty((n, n), device=DEV, dtype=torch.float64)
        ms, reps = device_ms(lambda: _lib.check(lib.sgam_feature_gram_f64(_p(zd), n, d, d, _p(G), _stream()), "sgam_feature_gram_f64"))
        flop = 2.0 * d * n * (n + 1) / 2.0
        bytes_ = 4.0 * n * d + 8.0 * n * n
        rec = {"n": n, "d": d, "ms": ms, "reps": reps, "gflop": flop / 1e9, "tflops": flop / (ms * 1e-3) / 1e12,
               "fraction_of_fp64_peak": flop / (ms * 1e-3) / FP64_PEAK, "output_gb_per_s": bytes_ / (ms * 1e-3) / 1e9}
        if not a.no_twin:
            t = time.perf_counter()
            want = FO.gram(z)
            rec["numpy_ms"] = 1e3 * (time.perf_counter() - t)
            rec["max_err_over_bound"] = float((np.abs(G.cpu().numpy() - want) / (d * 2.0 ** -53 * FO.gram_majorant(z))).max())
        out["gram"].append(rec)
        print(f"gram N = {n:5d} d = {d:5d}: {ms:8.3f} ms ({reps} launches)  {rec['gflop']:8.2f} GFLOP  {rec['tflops']:6.2f} TFLOP/s = "
              f"{100 * rec['fraction_of_fp64_peak']:5.1f} % of the fp64 peak" + (f"   numpy {rec['numpy_ms']:.1f} ms" if "numpy_ms" in rec else ""))
    # KID at 2048 + 2048 rows, 100 subsets of 1000
    n1 = n2 = 2048
    d, S, m = 2048, 100, 1000
    f1, f2 = features(n1, d, 1), features(n2, d, 2, 1.1, 0.05)
    d1, d2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    kid = FM.kid_from_features(d1, d2, subsets=S, subset_size=m, seed=0)
    z = torch.cat([d1, d2])
    G = FM.feature_gram(z)
    idx = FM.kid_subsets(n1, n2, m, S, 0, DEV)
    rec = {"n1": n1, "n2": n2, "d": d, "subsets": S, "subset_size": m, "kid": kid["kid"], "kid_std": kid["kid_std"],
           "end_to_end_ms": 1e3 * host_s(lambda: FM.kid_from_features(d1, d2, subsets=S, subset_size=m, seed=0)),
           "gram_ms": device_ms(lambda: FM.feature_gram(z))[0],
           "subsets_ms": device_ms(lambda: FM.kid_subsets(n1, n2, m, S, 0, DEV))[0]}
    values = torch.empty((S,), device=DEV, dtype=torch.float64)
    ws = torch.empty((3 * S * m,), device=DEV, dtype=torch.float64)
    rec["mmd_ms"] = device_ms(lambda: _lib.check(lib.sgam_kid_mmd_f64(_p(G), n1, n2, _p(idx), m, S, 1.0 / d, 1.0, _p(ws), 24 * S * m,
                                                                      _p(values), _stream()), "sgam_kid_mmd_f64"))[0]
    if not a.no_twin:
        t = time.perf_counter()
        want = FO.kid(f1, f2, subsets=S, subset_size=m, seed=0)
        rec["numpy_ms"] = 1e3 * (time.perf_counter() - t)
        scale = FO.kid_values(FO.gram_majorant(np.concatenate([f1, f2])), n1, want["idx"], 1.0 / d, 1.0, majorant=True)
        rec["numpy_kid"] = want["kid"]
        rec["max_diff_over_tol"] = float((np.abs(kid["values"].cpu().numpy() - want["values"]) / ((3 * d + 2 * m + 16) * 2.0 ** -53 * scale)).max())
    out["kid"] = rec
    print(f"KID {n1} + {n2} rows, {S} subsets of {m}: {rec['kid']:.6f} +- {rec['kid_std']:.6f}; end to end {rec['end_to_end_ms']:.2f} ms "
          f"(Gram {rec['gram_ms']:.3f}, subsets {rec['subsets_ms']:.3f}, MMD sums {rec['mmd_ms']:.3f})"
          + (f"   numpy {rec['numpy_ms']:.0f} ms, max|diff| / tol {rec['max_diff_over_tol']:.4f}" if "numpy_ms" in rec else ""))
    # precision / recall / density / coverage at 2048 + 2048 rows, k = 3: half of the scene's rows next to reference rows
    k = 3
    ref, gen = f1, f2.copy()
    gen[:n2 // 2] = ref[:n2 // 2] + np.float32(1e-2) * np.random.default_rng(3).standard_normal((n2 // 2, d)).astype(np.float32)
    dr, dg = torch.from_numpy(ref).to(DEV), torch.from_numpy(gen).to(DEV)
    got = FM.prdc_from_features(dr, dg, k=k)
    G = FM.feature_gram(torch.cat([dr, dg]))
    rec = {"n_reference": n1, "n_generated": n2, "d": d, "k": k, **got,
           "end_to_end_ms": 1e3 * host_s(lambda: FM.prdc_from_features(dr, dg, k=k)),
           "radii_and_counts_ms": device_ms(lambda: FM.prdc_counts(G, n1, n2, k))[0]}
    if not a.no_twin:
        t = time.perf_counter()
        twin = FO.prdc(FO.gram(np.concatenate([ref, gen])), n1, n2, k)
        rec["numpy_ms"] = 1e3 * (time.perf_counter() - t)
        rec["counts_equal_numpy"] = bool(FO.prdc_values(twin["counts"], n1, n2, k) == {key: got[key] for key in ("precision", "recall", "density", "coverage")})
        rec["numpy_margin"] = twin["margin"]
    out["prdc"] = rec
    print(f"PRDC {n1} + {n2} rows, k = {k}: precision {got['precision']:.4f} recall {got['recall']:.4f} density {got['density']:.4f} coverage "
          f"{got['coverage']:.4f}; end to end {rec['end_to_end_ms']:.2f} ms (radii + counts {rec['radii_and_counts_ms']:.3f})"
          + (f"   numpy {rec['numpy_ms']:.0f} ms, counts equal: {rec['counts_equal_numpy']}" if "numpy_ms" in rec else ""))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
