"""What top-k infill sampling costs in the scene loop: the 32-frame GoogleEarth loop (bench.py's model and scene) at topk = 4,
sample_number = 1, HIP graphs enabled, with (a) the host sampler (the reference's CPU draws; eager forwards), (b) the device
sampler (VQModel.set_infill_sampler("device"); captured forwards) and (c) topk = 1 (the arg-min loop) — alternated a-b-c
ROUNDS times, every measurement in a process of its own, and the same for LockstepScenes with SCENES scenes.

    python scripts/sampler_loop.py                      # driver: prints one line per measurement and a summary
    python scripts/sampler_loop.py --worker host|device|topk1 [--lockstep N]

BASE_TREE=<checkout of another commit, built> runs variant (a) from that tree as well ("host@base": the baseline the device
sampler has to beat is the host sampler of the commit before it).  STEPS / WARMUP / ROUNDS / SCENES from the environment."""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("SGAM_TREE") or os.path.dirname(HERE)
STEPS, WARMUP = int(os.environ.get("STEPS", 32)), int(os.environ.get("WARMUP", 4))
ROUNDS, SCENES = int(os.environ.get("ROUNDS", 2)), int(os.environ.get("SCENES", 8))


def worker(variant, lockstep):
    sys.path.insert(0, ROOT)
    import torch
    from bench import DATASET, build_model
    from sgam_neurips22_amd import ops
    from sgam_neurips22_amd.distributed import LockstepScenes
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    dev = torch.device("cuda", 0)
    model, _, _ = build_model(dev)
    model.enable_hip_graph(True)
    kw = {"topk": 1 if variant == "topk1" else 4}
    if variant == "device":
        kw.update(infill_sampler="device", infill_seed=0)
    total = (STEPS + WARMUP + 2, 1)
    if lockstep:
        L = LockstepScenes(model, DATASET, [synthetic_seed_frame(DATASET, i) for i in range(lockstep)], output_dim=total, **kw)
        step, per_step = L.step, lockstep
    else:
        sc = InfiniteSceneGeneration(model, DATASET, seed_index=0, output_dim=total, seed_frame=synthetic_seed_frame(DATASET, 0), **kw)

        def step():
            sc.one_step_prediction(sc.next_pose(sc.curr))
            sc.curr += 1
        per_step = 1
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    # launches of this library per step, counted on one eager step after the timed window (the timeline brackets every launch)
    with model.eager():
        recs, _ = ops.kernel_timeline(step)
    torch.cuda.synchronize()
    print(json.dumps({"variant": variant, "lockstep": lockstep, "frames_per_s": STEPS * per_step / dt,
                      "ms_per_step": 1e3 * dt / STEPS, "sgam_launches_per_step": len(recs), "graphs": len(model._graphs),
                      "tree": ROOT}), flush=True)


def driver():
    base = os.environ.get("BASE_TREE")
    variants = [("host", ROOT), ("device", ROOT), ("topk1", ROOT)] + ([("host@base", base)] if base else [])
    rows = []
    for lockstep in (0, SCENES):
        for _ in range(ROUNDS):
            for name, tree in variants:
                env = dict(os.environ, SGAM_TREE=tree)
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", name.split("@")[0]] + (["--lockstep", str(lockstep)] if lockstep else [])
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=tree)
                if r.returncode != 0:          # a failed measurement ends the run: nothing more is started on the GPU
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"{name} (lockstep {lockstep}) exited with {r.returncode}")
                row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                row["variant"] = name
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("summary (frames/s per round; sgam launches per step):")
    for lockstep in (0, SCENES):
        for name, _ in variants:
            sel = [r for r in rows if r["variant"] == name and r["lockstep"] == lockstep]
            print(f"  {'lockstep x' + str(lockstep) if lockstep else 'single scene':>14} {name:>10}: "
                  + ", ".join(f"{r['frames_per_s']:.1f}" for r in sel) + f"  ({sel[0]['sgam_launches_per_step']} launches, {sel[0]['graphs']} graphs)")


if __name__ == "__main__":
    if "--worker" in sys.argv:
        ls = int(sys.argv[sys.argv.index("--lockstep") + 1]) if "--lockstep" in sys.argv else 0
        worker(sys.argv[sys.argv.index("--worker") + 1], ls)
    else:
        driver()
