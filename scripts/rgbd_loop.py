"""the rgbd_integration branch of the scene loop alone (BASELINE configs[2] with --use_rgbd_integration): STEPS frames after WARMUP,
wall clock per frame; run under rocprofv3 --kernel-trace --stats for the per-kernel record (scripts/prof_rgbd.sh).
`--lockstep S`: after the solo loop (the same-process baseline), S scenes (seeds 0 .. S-1) in lock step on the same branch
(distributed.LockstepScenes: scene-batched TSDF kernels, one forward at B = S): frames/s aggregate and per scene."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import build_model, DATASET
from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
ap = argparse.ArgumentParser()
ap.add_argument("--lockstep", type=int, default=0, metavar="S")
args = ap.parse_args()
steps, warmup = int(os.environ.get("STEPS", 31)), int(os.environ.get("WARMUP", 3))
dev = torch.device("cuda", 0)
model, sd, p = build_model(dev)
model.enable_hip_graph(os.environ.get("NO_GRAPH", "0") != "1")
if os.environ.get("SPLAT_TOO", "1") == "1":      # the forward-splat branch on the same box, for the difference
    s0 = InfiniteSceneGeneration(model, DATASET, seed_index=0, output_dim=(steps + warmup + 4, 1), seed_frame=synthetic_seed_frame(DATASET, 0))
    for _ in range(warmup):
        s0.one_step_prediction(s0.next_pose(s0.curr)); s0.curr += 1
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        s0.one_step_prediction(s0.next_pose(s0.curr)); s0.curr += 1
    torch.cuda.synchronize()
    dt0 = time.perf_counter() - t
    print(f"splat loop: {steps / dt0:.1f} frames/s, {1e3 * dt0 / steps:.3f} ms/frame")
    del s0
sc = InfiniteSceneGeneration(model, DATASET, seed_index=0, output_dim=(steps + warmup + 4, 1), seed_frame=synthetic_seed_frame(DATASET, 0),
                             use_rgbd_integration=True)
for _ in range(warmup):
    sc.one_step_prediction(sc.next_pose(sc.curr)); sc.curr += 1
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(steps):
    sc.one_step_prediction(sc.next_pose(sc.curr)); sc.curr += 1
torch.cuda.synchronize()
dt = time.perf_counter() - t
print(f"rgbd loop: {steps / dt:.1f} frames/s, {1e3 * dt / steps:.3f} ms/frame, tsdf stats {sc.volume.stats()}")
if args.lockstep > 0:
    from sgam_neurips22_amd.distributed import LockstepScenes
    del sc
    S = args.lockstep
    L = LockstepScenes(model, DATASET, [synthetic_seed_frame(DATASET, i) for i in range(S)], output_dim=(steps + warmup + 4, 1),
                       use_rgbd_integration=True)
    for _ in range(warmup):
        L.step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        L.step()
    torch.cuda.synchronize()
    dtL = time.perf_counter() - t
    print(f"rgbd lockstep S={S}: {S * steps / dtL:.1f} frames/s aggregate, {steps / dtL:.1f} per scene, {1e3 * dtL / steps:.3f} ms/step, "
          f"solo rgbd loop in this process {steps / dt:.1f} frames/s, tsdf stats {[sc.volume.stats() for sc in L.scenes]}")
