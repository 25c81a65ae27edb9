#!/usr/bin/env python
"""What a node of the fp32 frame's own launch pairs costs in a captured chain, for one build of the library.

graph_gap.py prices a boundary between trivial kernels; this one prices it behind the frame's big writers.  Each chain is ~40
dependent launches of a pair the frame runs, captured once and replayed:

    gn256    256^2 128->128 GroupNorm conv (halo2 128-row tile, 33.5 MB out) + gn_finalize_stats
    splitk16 16^2 512->512 GroupNorm conv as split-K partial tiles (8.4 MB of workspace) + group-major combine
    attn64   AttnBlock at 64^2 x 256: gn_finalize_stats + attn_qkv_gn (12 MB) + attn_flash (32 MB of partial O) + combine_proj

Per chain it prints the kernels of one step, their eager kernel time (ops.kernel_timeline), the replayed time per node and the
difference: what a node costs beyond its kernel, i.e. the boundary.  A / B = the same script on two libraries (SGAM_HIP_LIB),
alternated in one session; the parent twice gives the parent-to-parent spread every difference is read against.

`frame` as a chain name measures the frame itself: GPU time of the replayed 256^2 forward minus the sum of its kernels' eager
times (best of three timelines), with the kernel time by family.

    python scripts/store_policy_gap.py [--chains gn256,splitk16,attn64,frame] [--reps 9] [--json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402

from sgam_neurips22_amd import _lib, ops, testing  # noqa: E402

DEV = "cuda"


def _conv_chain(tag, H, C, steps):
    """x -> conv3x3(swish(GroupNorm(x))) repeated: every conv reads the statistics its predecessor's epilogue / combine left"""
    x0 = testing.seeded_tensor(tag + ".x", (1, H, H, C), 1.0, 0.2).to(DEV)
    w = ops.pack_conv_weight(testing.seeded_tensor(tag + ".w", (C, C, 3, 3), scale=(1.0 / (C * 9)) ** 0.5).to(DEV), dtype="f32x")
    b = testing.seeded_tensor(tag + ".b", (C,), scale=0.1).to(DEV)
    g, bt = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)

    def conv(x):
        return ops.conv2d_nhwc(x, w, b, cout=C, kh=3, kw=3, pad_t=1, pad_l=1, norm=(g, bt, True, 32, 1e-6))
    first = ops.conv2d_nhwc(x0, w, b, cout=C, kh=3, kw=3, pad_t=1, pad_l=1)        # carries statistics like every frame tensor

    def run():
        x = first
        for _ in range(steps):
            x = conv(x)
        return x
    return run, lambda: conv(first), steps


def _attn_chain(steps):
    from sgam_neurips22_amd.generative_sensing_module.modules.diffusionmodules import model as dm
    mod = dm.AttnBlock(256)
    mod.load_state_dict(testing.synthetic_state_dict(mod.state_dict(), seed=11))
    mod = mod.to(DEV).eval()
    w = ops.pack_conv_weight(testing.seeded_tensor("spg.attn.w", (256, 256, 3, 3), scale=(1.0 / (256 * 9)) ** 0.5).to(DEV), dtype="f32x")
    x0 = testing.seeded_tensor("spg.attn.x", (1, 64, 64, 256), 1.0, 0.3).to(DEV)
    first = ops.conv2d_nhwc(x0, w, None, cout=256, kh=3, kw=3, pad_t=1, pad_l=1)

    def run():
        x = first
        for _ in range(steps):
            x = mod.forward_nhwc(x)
        return x
    return run, lambda: mod.forward_nhwc(first), steps


CHAINS = {"gn256": lambda: _conv_chain("spg.gn256", 256, 128, 20), "splitk16": lambda: _conv_chain("spg.sk16", 16, 512, 20),
          "attn64": lambda: _attn_chain(10)}


def measure(name, reps):
    run, step, steps = CHAINS[name]()          # the whole chain, one step of it, steps in the chain
    with torch.no_grad():
        run()                                   # packs weights, fills the allocator
        recs, bracket = ops.kernel_timeline(step)
        again, _ = ops.kernel_timeline(step)
        kern_ms = [min(a[1], b[1]) - bracket for a, b in zip(recs, again)]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run()
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(reps):
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
    assert torch.isfinite(out).all()
    times.sort()
    nodes = steps * len(recs)
    node_us = times[len(times) // 2] * 1e3 / nodes
    k_us = sum(kern_ms) * 1e3 / len(recs)
    return dict(chain=name, kernels=[r[0].split("(")[0] for r in recs], kernel_us=[round(k * 1e3, 2) for k in kern_ms], nodes=nodes,
                node_us=round(node_us, 3), node_us_min=round(times[0] * 1e3 / nodes, 3), kernel_us_per_node=round(k_us, 3),
                boundary_us=round(node_us - k_us, 3))


FAMILIES = (("halo2_kernel<128", "128-row tiles"), ("halo2_kernel<64", "64-row tiles"), ("conv_gemm_f32x", "generic tiles"),
            ("splitk_reduce", "combines"), ("attn_qkv_gn", "attention front end"), ("attn_flash", "flash partials"),
            ("attn_combine", "attention merge"), ("gemm_gn_f32x", "panel GEMMs"))


def measure_frame(reps):
    """the frame itself: GPU time of the replayed forward against the sum of its kernels' eager times (the rest is boundaries)"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    p = default_params("google_earth")
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(0.0, 0.5, p["n_embed"], 256, 1)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    x, em = testing.rect_hole_input(1, 256, 256, seed=40)
    x, em = x.to(DEV), em.to(DEV)

    def eager():
        with torch.no_grad(), m.eager():
            m(x, extrapolation_mask=em)
    eager()
    eager()
    runs = [ops.kernel_timeline(eager) for _ in range(3)]
    n = len(runs[0][0])
    assert all(len(r[0]) == n for r in runs)
    per = [min(max(r[0][i][1] - r[1], 0.0) for r in runs) for i in range(n)]          # best of three per launch, net of the bracket
    fam = {}
    for i, rec in enumerate(runs[0][0]):
        label = next((lab for key, lab in FAMILIES if key in rec[0]), "other")
        a = fam.setdefault(label, [0, 0.0])
        a[0] += 1
        a[1] += per[i]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                   # the same launches, captured the way the model captures them
        eager()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    return dict(chain="frame", nodes=n, replay_ms=round(med, 4), replay_ms_min=round(times[0], 4), kernel_ms=round(sum(per), 4),
                boundary_ms=round(med - sum(per), 4), boundary_us_per_node=round((med - sum(per)) * 1e3 / n, 3),
                families={k: [v[0], round(v[1] * 1e3, 1)] for k, v in fam.items()},
                launches=[[rec[0], round(per[i] * 1e3, 2)] for i, rec in enumerate(runs[0][0])])      # in order (--json only)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chains", default="gn256,splitk16,attn64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", action="store_true", help="one JSON line per chain instead of the table")
    a = ap.parse_args()
    lib = _lib.load()
    stamp = f"{lib.sgam_build_commit().decode()} {lib.sgam_build_digest().decode()}"
    for name in [c for c in a.chains.split(",") if c]:
        r = measure_frame(max(a.reps, 30)) if name == "frame" else measure(name, a.reps)
        r["lib"] = stamp
        if a.json:
            print(json.dumps(r), flush=True)
        elif name == "frame":
            print(f"frame     {r['nodes']:3d} nodes  replay {r['replay_ms']:.4f} ms (min {r['replay_ms_min']:.4f})  kernels {r['kernel_ms']:.4f} ms"
                  f"  beyond the kernels {r['boundary_ms']:.4f} ms = {r['boundary_us_per_node']:.2f} us/node   [{stamp}]", flush=True)
            for lab, (calls, us) in r["families"].items():
                print(f"            {calls:3d} x  {us:8.1f} us  {lab}", flush=True)
        else:
            print(f"{name:9s} {r['nodes']:3d} nodes  {r['node_us']:7.2f} us/node (min {r['node_us_min']:.2f})  kernels {r['kernel_us_per_node']:7.2f}"
                  f"  beyond the kernel {r['boundary_us']:6.2f}   [{stamp}]", flush=True)
            for k, us in zip(r["kernels"], r["kernel_us"]):
                print(f"            {us:8.2f} us  {k}", flush=True)


if __name__ == "__main__":
    main()
