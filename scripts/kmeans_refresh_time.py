"""What the online k-means codebook refresh costs (DESIGN §4.6 "Device refresh").

    python scripts/kmeans_refresh_time.py step            # bookkeeping per `codebook`-phase update: refresh off / host / device
    python scripts/kmeans_refresh_time.py refresh [K..]   # one refresh at the CLEVR config's size on the device (default K: 1639 16384)
    python scripts/kmeans_refresh_time.py host [K] [ITER] # scipy's kmeans2 on the same data on the host's CPUs (default 1639, iter 1)

Each mode is one process and prints one JSON line; per `measuring-on-mi355x`: warm-up, REPEATS (default 5) repeats, median and
spread.  N / D from the environment (default 262144 / 256: train_feature_buffer_size 1024 x 16 x 16 latents)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D = int(os.environ.get("N", 262144)), int(os.environ.get("D", 256))
REPEATS = int(os.environ.get("REPEATS", 5))
SPLIT_ROOF_TFLOPS = 833.0          # the split-fp32 roof bench.py uses


def _spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": len(ms)}


def _data(torch, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn((4096, D), device=dev, generator=g) * 2.0
    return (centres[torch.randint(0, 4096, (N,), device=dev, generator=g)] + torch.randn((N, D), device=dev, generator=g)).contiguous()


def refresh(ks):
    import torch
    from sgam_neurips22_amd import kmeans, ops
    dev = torch.device("cuda", 0)
    x = _data(torch, dev)
    out = {"mode": "refresh", "N": N, "D": D, "iter": 10}
    for k in ks:
        kmeans.kmeans2(x, k, iter=1, seed=0)                      # warm-up (allocator, code objects)
        torch.cuda.synchronize()
        ms = []
        for r in range(REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            kmeans.kmeans2(x, k, iter=10, seed=0, refresh=r)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        # kernel shares of ONE iteration from the library's own timeline
        recs, bracket = ops.kernel_timeline(lambda: kmeans.kmeans2(x, k, iter=1, seed=0))
        per = {}
        for name, t, *_ in recs:
            key = name.split("<")[0]
            per[key] = per.get(key, 0.0) + max(t - bracket, 0.0)
        gemm = sum(v for n, v in per.items() if "conv_gemm" in n)
        total = sum(per.values())
        kpad = (k + 127) // 128 * 128
        out[f"k{k}"] = dict(_spread(ms), iteration_ms=round(total, 3), gemm_ms=round(gemm, 3), gemm_share=round(gemm / total, 3),
                            gemm_tflops=round(2.0 * N * kpad * D / (gemm * 1e-3) / 1e12, 1),
                            gemm_fraction_of_split_roof=round(2.0 * N * kpad * D / (gemm * 1e-3) / 1e12 / SPLIT_ROOF_TFLOPS, 4),
                            kernels_ms={n: round(v, 3) for n, v in sorted(per.items(), key=lambda kv: -kv[1])})
    print(json.dumps(out), flush=True)


def host(k, iters):
    import warnings
    import numpy as np
    from scipy.cluster.vq import kmeans2
    rng = np.random.default_rng(0)
    centres = (rng.standard_normal((4096, D)) * 2.0).astype(np.float32)
    x = centres[rng.integers(0, 4096, N)] + rng.standard_normal((N, D), dtype=np.float32)
    t = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kmeans2(x, k, iter=iters, minit="points")
    print(json.dumps({"mode": "host", "N": N, "D": D, "k": k, "iter": iters, "seconds": round(time.perf_counter() - t, 2),
                      "cpus": len(os.sched_getaffinity(0))}), flush=True)


def step():
    """`codebook`-phase AutoencoderTrainer updates of the bench's 256 x 256 model, refresh off / host / device with a frequency that
    never fires: what is timed is the per-step bookkeeping alone"""
    import torch
    from bench import build_model
    from sgam_neurips22_amd import testing, training
    dev = torch.device("cuda", 0)
    xt, mk = testing.rect_hole_input(1, 256, 256, seed=9)
    xd = testing.seeded_tensor("bench.train.dst", (1, 4, 256, 256), scale=0.5).clamp(-1, 1).to(dev)
    xt, mk = xt.to(dev), mk.to(dev)
    out = {"mode": "step"}
    for backend in ("off", "host", "device", "off", "host", "device"):
        m = build_model(dev)[0]
        m.online_kmeans_config = {"do_online_kmeans_clustering": backend != "off", "backend": backend if backend != "off" else "host",
                                  "online_kmeans_word_timeout": 10, "inactive_threshold": 0.1, "train_feature_buffer_size": 16,
                                  "frequency": 10 ** 9, "start_global_step": 0}
        tr = training.AutoencoderTrainer(m, phase="codebook", lr=4.5e-6)
        for _ in range(2):
            tr.step(xt, xd, mk)
        ms = []
        for _ in range(max(REPEATS, 8)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            tr.step(xt, xd, mk)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t))
        out.setdefault(backend, []).append(_spread(ms))
        del tr, m
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "refresh"
    if mode == "refresh":
        refresh([int(v) for v in sys.argv[2:]] or [1639, 16384])
    elif mode == "host":
        host(int(sys.argv[2]) if len(sys.argv) > 2 else 1639, int(sys.argv[3]) if len(sys.argv) > 3 else 1)
    elif mode == "step":
        step()
    else:
        raise SystemExit(__doc__)
