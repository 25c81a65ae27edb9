"""What a view of the finished scene costs (DESIGN §4.4 "Coloured views"): the batched coloured mesh render
(tsdf.render_mesh_rgbd: rgb + depth of P poses in one call) beside the two ways the same pictures were made before it —
P calls of sgam_mesh_render_depth_f32 (depth only) and P calls of TsdfVolume.render_depth(want_color=True) (the ray cast's
nearest-voxel colour).

    python scripts/flythrough_time.py [--frames 6] [--poses 1 16 64] [--repeats 5]

The mesh is that of a GoogleEarth rgbd_integration run (synthetic weights, 256 x 256, `--frames` frames), the poses its
fly-through.  Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device events,
the three variants alternated within a repeat, median and spread.  One process, one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _scene(frames):
    import torch
    from sgam_neurips22_amd import testing
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    p = default_params("google_earth")
    m = VQModel(**p)
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(0.0, 0.5, p["n_embed"], 256, 1)
    m.load_state_dict(sd)
    m = m.to(torch.device("cuda", 0)).eval()
    scene = InfiniteSceneGeneration(m, "google_earth", output_dim=(frames, 1), seed_frame=synthetic_seed_frame("google_earth", 0, 256),
                                    use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30)
    scene.scene_expansion()
    return scene


def _timed(torch, fn, min_ms=200.0):
    """ms per call of fn over a window of at least min_ms"""
    n, total = 0, 0.0
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = 1
    while total < min_ms:
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b)
        total, n = total + t, n + calls
        calls = max(1, min(1024, int(calls * min_ms / max(t, 1e-3))))
    return total / n


def _spread(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, ops, tsdf
    if not torch.cuda.is_available():
        raise SystemExit("flythrough_time.py measures on the GPU: no device found")
    scene = _scene(args.frames)
    H, W = scene.image_resolution
    z0, z1 = scene._Z_RANGE[scene.data]
    vol = scene.colour_volume(max_bricks=max(1, scene.volume.stats()[0]))
    vol.check()
    mesh = vol.extract_mesh_device()
    n_between = -(-max(args.poses) // max(1, args.frames - 1))
    all_poses = scene.flythrough_poses(n_between=n_between)
    assert len(all_poses) >= max(args.poses)
    fx, fy, cx, cy = vol._k4(scene.K)
    lib = _lib.load()
    depth1 = torch.empty((H, W), dtype=torch.float32, device=scene.device)
    out = {"script": "flythrough_time", "frames": args.frames, "H": H, "W": W, "vertices": mesh.n_vertices, "triangles": mesh.n_triangles,
           "bricks": vol.stats()[0], "repeats": args.repeats, "build": lib.sgam_build_commit().decode(), "unit": "ms per view"}
    for P in args.poses:
        poses = all_poses[:P]
        poses32 = [np.ascontiguousarray(T, dtype=np.float32) for T in poses]
        bufs = {"depth": torch.empty((P, H, W), dtype=torch.float32, device=scene.device),
                "rgb": torch.empty((P, H, W, 3), dtype=torch.float32, device=scene.device)}

        def batched():
            tsdf.render_mesh_rgbd(mesh, scene.K, poses, H, W, z0, z1, out=bufs)

        def depth_calls():
            for T in poses32:
                _lib.check(lib.sgam_mesh_render_depth_f32(
                    ops._p(mesh.vertices), mesh.vertices.shape[0], ops._p(mesh.triangles), mesh.triangles.shape[0], ops._p(mesh.counts),
                    H, W, fx, fy, cx, cy, ctypes.c_void_p(T.ctypes.data), z0, z1, ops._p(depth1), ops._stream()), "sgam_mesh_render_depth_f32")

        def ray_casts():
            for T in poses:
                vol.render_depth(scene.K, T, H, W, z0, z1, want_color=True, out=depth1)

        variants = {"mesh_rgbd_batched": batched, "mesh_depth_calls": depth_calls, "raycast_colour_calls": ray_casts}
        for fn in variants.values():            # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                ms[k].append(_timed(torch, fn) / P)
        res = {k: _spread(v) for k, v in ms.items()}
        yard = res["mesh_depth_calls"]["median"] + res["raycast_colour_calls"]["median"]
        res["batched_over_depth_calls"] = round(res["mesh_rgbd_batched"]["median"] / res["mesh_depth_calls"]["median"], 3)
        res["batched_over_raycast_calls"] = round(res["mesh_rgbd_batched"]["median"] / res["raycast_colour_calls"]["median"], 3)
        res["batched_over_depth_plus_raycast"] = round(res["mesh_rgbd_batched"]["median"] / yard, 3)
        res["hit_fraction"] = round(float((bufs["depth"] > 0).float().mean()), 3)
        out[f"P{P}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
