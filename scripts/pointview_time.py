"""What a point-splat view of the finished scene costs: pointview.render_points_rgbd — every stored frame of a
forward-splat-branch scene splatted with a z-test at P poses in one call — for radius 0 / 1 / 2, with and without the 3x3 fill,
in ms per view.

    python scripts/pointview_time.py [--frames 32] [--poses 64] [--size 256] [--repeats 5] [--mesh [--tsdf-budget-gb 4]] [--ab-lib OTHER.so]

The scene is a GoogleEarth run on the splat branch (synthetic weights, 256 x 256, `--frames` frames), the poses its fly-through.
--mesh: the coloured mesh render (tsdf.render_mesh_rgbd) of an rgbd_integration run of the same grid — the same poses — beside it.
--ab-lib: a second build of the library; its sgam_points_render_rgbd_f32 is alternated three times with the in-tree build's on the
same buffers (the kernel calls alone: tables uploaded once), and the outputs are compared.
Per `measuring-on-mi355x`: every shape warmed up, each repeat a window of >= 0.2 s of calls between device events, the variants
alternated within a repeat, median and spread.  One process, one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flythrough_time import _spread, _timed  # noqa: E402


def _scene(frames, rgbd, budget=1 << 30):
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
    kw = dict(use_rgbd_integration=True, tsdf_memory_budget_bytes=budget) if rgbd else {}
    scene = InfiniteSceneGeneration(m, "google_earth", output_dim=(frames, 1), seed_frame=synthetic_seed_frame("google_earth", 0, 256), **kw)
    scene.scene_expansion()
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mesh", action="store_true")
    ap.add_argument("--tsdf-budget-gb", type=int, default=4)
    ap.add_argument("--ab-lib", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sgam_neurips22_amd import _lib, ops, pointview, tsdf
    if not torch.cuda.is_available():
        raise SystemExit("pointview_time.py measures on the GPU: no device found")
    scene = _scene(args.frames, rgbd=False)
    dev = scene.device
    H = W = args.size
    P = args.poses
    z0, z1 = scene._Z_RANGE[scene.data]
    n_between = -(-P // max(1, args.frames - 1))
    poses = scene.flythrough_poses(n_between=n_between)[:P]
    assert len(poses) == P
    K = scene.K if (H, W) == tuple(scene.image_resolution) else \
        np.diag([W / scene.image_resolution[1], H / scene.image_resolution[0], 1.0]) @ scene.K
    coords = [c for c, _ in sorted(scene.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
    depths = [scene.frames[c]["depth"] for c in coords]
    rgbs = [scene.frames[c]["rgb_u8"] for c in coords]
    Ts_src = [scene.transform_grid[c[0]][c[1]]["T"] for c in coords]
    T_rel = pointview.relative_transforms(poses, Ts_src)
    bufs = {"depth": torch.empty((P, H, W), dtype=torch.float32, device=dev), "rgb": torch.empty((P, H, W, 3), dtype=torch.float32, device=dev),
            "rgb_u8": torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)}
    lib = _lib.load()
    out = {"script": "pointview_time", "frames": len(coords), "poses": P, "H": H, "W": W, "repeats": args.repeats,
           "points_per_view": len(coords) * depths[0].numel(), "build": lib.sgam_build_commit().decode(), "unit": "ms per view"}

    variants = {}
    for radius in (0, 1, 2):
        for fill in (False, True):
            def call(radius=radius, fill=fill):
                pointview.render_points_rgbd(depths, rgbs, scene.K, Ts_src, K, poses, H, W, z0, z1, radius=radius, hole_fill=fill, T_rel=T_rel,
                                             out=bufs)
            variants[f"points_r{radius}_{'fill' if fill else 'raw'}"] = call
    hit = {}
    for k, fn in variants.items():               # warm-up: code objects, allocator; and what each variant covers
        fn()
        hit[k] = round(float((bufs["depth"] > 0).float().mean()), 3)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            ms[k].append(_timed(torch, fn) / P)
    out["points"] = {k: dict(_spread(v), hit_fraction=hit[k]) for k, v in ms.items()}

    if args.ab_lib:
        other = ctypes.CDLL(args.ab_lib)
        res, argt = _lib.PROTOTYPES["sgam_points_render_rgbd_f32"]
        other.sgam_points_render_rgbd_f32.restype, other.sgam_points_render_rgbd_f32.argtypes = res, argt
        F, (Hs, Ws) = len(coords), depths[0].shape
        table = torch.tensor([t.data_ptr() for t in depths] + [t.data_ptr() for t in rgbs], dtype=torch.int64).to(dev)
        rel = torch.from_numpy(T_rel.reshape(P, F * 12)).to(dev)
        Kinv = np.ascontiguousarray(np.linalg.inv(scene.K).astype(np.float32).reshape(9))
        ws = torch.empty((P * H * W,), dtype=torch.int64, device=dev)
        ab = {}
        for radius in (0, 1, 2):
            def raw(which, radius=radius):
                _lib.check(which.sgam_points_render_rgbd_f32(
                    ops._p(table[:F]), ops._p(table[F:]), F, Hs, Ws, ctypes.c_void_p(Kinv.ctypes.data), ops._p(rel), P, H, W, float(K[0, 0]),
                    float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), z0, z1, radius, 1, ops._p(bufs["depth"]), ops._p(bufs["rgb"]),
                    ops._p(bufs["rgb_u8"]), None, ops._p(ws), ws.numel() * 8, ops._stream()), "sgam_points_render_rgbd_f32")
            raw(lib)
            ref = {k: v.clone() for k, v in bufs.items()}
            raw(other)
            same = all(torch.equal(ref[k], bufs[k]) for k in ref)
            t = {"in_tree": [], "other": []}
            for _ in range(3):
                t["in_tree"].append(_timed(torch, lambda: raw(lib)) / P)
                t["other"].append(_timed(torch, lambda: raw(other)) / P)
            ab[f"r{radius}_fill"] = {"in_tree": [round(x, 4) for x in t["in_tree"]], "other": [round(x, 4) for x in t["other"]],
                                     "in_tree_over_other": round(statistics.median(t["in_tree"]) / statistics.median(t["other"]), 3),
                                     "outputs_equal": same}
        out["ab"] = dict(ab, other=os.path.basename(args.ab_lib))

    if args.mesh:
        del scene
        torch.cuda.empty_cache()
        rscene = _scene(args.frames, rgbd=True, budget=args.tsdf_budget_gb << 30)
        rposes = rscene.flythrough_poses(n_between=n_between)[:P]
        assert np.array_equal(rposes, poses)             # the same grid: the same fly-through
        vol = rscene.colour_volume(max_bricks=max(1, rscene.volume.stats()[0]))
        vol.check()
        mesh = vol.extract_mesh_device()

        def mesh_call():
            tsdf.render_mesh_rgbd(mesh, K, rposes, H, W, z0, z1, u8=True, out=bufs)

        mesh_call()
        torch.cuda.synchronize()
        out["mesh_rgbd_batched"] = dict(_spread([_timed(torch, mesh_call) / P for _ in range(args.repeats)]), triangles=mesh.n_triangles,
                                        hit_fraction=round(float((bufs["depth"] > 0).float().mean()), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
