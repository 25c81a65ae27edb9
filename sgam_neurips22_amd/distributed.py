"""Scene-parallel multi-GPU support: independent trajectories shard across ranks, one process
per GPU, weights replicated, NO data-path collective.  The only communication is one tiny all-gather of the
per-rank (frames, seconds, checksum) record at the end — RCCL over xGMI on the GPU box (backend "nccl"),
gloo in the CPU tests."""
import os

# HIP streams are dealt onto hardware queues (4 by default): with fewer queues than concurrent scenes — or an unlucky
# deal — two scenes share a queue and run back to back instead of side by side (measured on one box: two scenes 319
# frames/s with the default, 447 with 8 queues; three scenes 392 vs 503).  Must be in the environment before the HIP
# runtime starts, i.e. before the first CUDA call of the process.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# dmabuf IPC only on this host driver: without it RCCL's peer set-up fails with `hipIpcGetMemHandle: invalid argument`
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def env_world():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))


def launched_by_torchrun():
    """a rendezvous is in the environment (torch.distributed.run exports these for every rank, world size 1 included)"""
    return "RANK" in os.environ and "WORLD_SIZE" in os.environ and "MASTER_PORT" in os.environ


def collectives_active(group=None):
    """True when the (tiny) collectives of this package must actually be issued: a process group exists and either has
    more than one rank or the run is a world-1 rehearsal of the multi-GPU path (`torch.distributed.run --nproc-per-node 1`,
    or SGAM_DIST_WORLD1=1) — the one-GPU way to take RCCL initialisation, the all-gather / all-reduce / broadcast on device
    tensors and the teardown through the exact code an N-GPU run executes (tests/test_gpu_distributed.py)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or launched_by_torchrun() or os.environ.get("SGAM_DIST_WORLD1") == "1"


def init(backend=None):
    """Initialise torch.distributed from the torchrun environment (any world size, 1 included: the launcher path is the
    same code at every N); no-op for a plain single process."""
    rank, local_rank, world = env_world()
    if (world > 1 or launched_by_torchrun()) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            # RCCL's own version line (NCCL_DEBUG=VERSION), into a per-rank file instead of stdout — rank 0 prints ONE JSON line
            # there; gather_metrics() reads rank 0's file back into the record, so a failing first multi-GPU run can be
            # diagnosed from bench_extra.json alone
            os.environ.setdefault("NCCL_DEBUG", "VERSION")
            os.environ.setdefault("NCCL_DEBUG_FILE", os.path.join(os.environ.get("TMPDIR", "/tmp"), f"sgam_rccl_{os.getpid()}_r{rank}.log"))
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


def self_launch(script, argv, n):
    """`python bench.py --gpus N` without a launcher: re-run `script argv` as N ranks of one node through
    torch.distributed.run (the same command line the driver uses), rendezvous on 127.0.0.1 and a free port.  Returns the
    launcher's exit code."""
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), script] + list(argv)
    return subprocess.call(cmd, env=env)


def pin_to_gpu_numa_node(local_rank):
    """Bind this rank's host threads to the CPUs of the NUMA node its GPU hangs off (PCI bus id -> sysfs numa_node ->
    cpulist), so that the pinned staging buffer and the launch thread are local to the GPU.  Best effort: returns the
    node number, or None when the topology cannot be read (containers without sysfs, single-node hosts)."""
    try:
        prop = torch.cuda.get_device_properties(local_rank)
        bdf = f"{getattr(prop, 'pci_domain_id', 0):04x}:{prop.pci_bus_id:02x}:{prop.pci_device_id:02x}.0"
        with open(f"/sys/bus/pci/devices/{bdf}/numa_node") as f:
            node = int(f.read().strip())
        if node < 0:
            return None
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            cpus = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        if cpus:
            os.sched_setaffinity(0, cpus & os.sched_getaffinity(0) or cpus)
        return node
    except Exception:
        return None


def shard_scenes(num_scenes, rank, world):
    """rank r owns scenes {s : s mod world == r} (round-robin)."""
    return [s for s in range(num_scenes) if s % world == rank]


def barrier():
    if dist.is_available() and dist.is_initialized():
        dist.barrier()


def rccl_info():
    """what this process knows about its RCCL: the library version torch was built against / loaded, the environment that
    shapes the multi-process path, and (once a communicator exists) RCCL's own NCCL_DEBUG=VERSION line(s)"""
    info = {"backend": dist.get_backend() if dist.is_available() and dist.is_initialized() else None,
            "env": {k: os.environ.get(k) for k in ("HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG", "GPU_MAX_HW_QUEUES", "WORLD_SIZE",
                                                   "LOCAL_WORLD_SIZE", "MASTER_ADDR")}}
    try:
        info["version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
    except Exception as e:                      # CPU-only torch / gloo runs
        info["version"] = None
        info["version_error"] = type(e).__name__
    path = os.environ.get("NCCL_DEBUG_FILE")
    if path and os.path.exists(path):
        try:
            with open(path) as f:
                info["debug_log"] = [ln.rstrip() for ln in f.readlines()[:8]]
        except OSError:
            pass
    return info


def gather_metrics(frames, seconds, checksum, device, numa_node=None):
    """All-gather one (frames, seconds, checksum, numa node, local rank) record per rank.  Returns dict(total_frames,
    max_seconds, frames_per_s, per_rank=[(frames, seconds, checksum)], per_rank_records=[{...}], rccl={...}) on every rank.
    40 bytes per rank: latency-bound, no bandwidth tuning."""
    rank, local_rank, _ = env_world()
    rec = torch.tensor([float(frames), float(seconds), float(checksum), -1.0 if numa_node is None else float(numa_node),
                        float(local_rank)], dtype=torch.float64, device=device)
    if collectives_active():
        out = [torch.zeros_like(rec) for _ in range(dist.get_world_size())]
        dist.all_gather(out, rec)
    else:
        out = [rec]
    rows = [t.tolist() for t in out]
    per_rank = [tuple(r[:3]) for r in rows]
    total = sum(r[0] for r in per_rank)
    tmax = max(r[1] for r in per_rank)
    records = [{"rank": i, "frames": r[0], "seconds": round(r[1], 6), "checksum": r[2], "numa_node": None if r[3] < 0 else int(r[3]),
                "local_rank": int(r[4])} for i, r in enumerate(rows)]
    return {"total_frames": total, "max_seconds": tmax, "frames_per_s": total / tmax if tmax > 0 else 0.0,
            "per_rank": per_rank, "per_rank_records": records, "rccl": rccl_info()}


class ConcurrentScenes:
    """Several independent trajectories on ONE GPU, each on its own HIP stream with its own model instance (captured
    graphs own static buffers, so scenes cannot share one).  A single scene is latency-bound between its ~170 dependent
    kernel launches per frame (the 16^2 / 32^2 layers fill a fraction of the chip); kernels of other scenes fill those
    gaps: aggregate frames/s rises ~1.45x with two scenes and ~1.6x with three on an MI355X, every scene still producing
    exactly the frames it produces alone (tests/test_gpu_vqgan.py).  Scenes are the path's shardable unit:
    this is the same sharding below GPU granularity; no collective, no data shared between scenes."""

    def __init__(self, make_scene, n):
        """make_scene(i) -> InfiniteSceneGeneration bound to its OWN VQModel instance (called inside stream i)."""
        self.streams = [torch.cuda.Stream() for _ in range(n)]
        self.scenes = []
        for i, s in enumerate(self.streams):
            with torch.cuda.stream(s):
                self.scenes.append(make_scene(i))

    def step(self):
        """one generated frame per scene; the host enqueues the scenes round-robin, the GPU overlaps them"""
        for sc, s in zip(self.scenes, self.streams):
            with torch.cuda.stream(s):
                sc.one_step_prediction(sc.next_pose(sc.curr))
                sc.curr += 1

    def synchronize(self):
        for s in self.streams:
            s.synchronize()


class LockstepScenes:
    """S independent trajectories on ONE GPU advanced in LOCK STEP through ONE launch sequence at batch S (VERDICT r2 next
    #4): the scenes of a rank share the weights, the pose grid and the visiting order, so step t of every scene is the same
    computation on different frames — one forward splat with a pointer table of S x N source frames, one VQGAN forward at
    B = S (one captured graph), one feedback codec launch.  Where `ConcurrentScenes` hides a single trajectory's launch
    latency behind other streams, this feeds the kernels themselves: the 16^2 ... 64^2 layers run M = S x pixels rows
    against the same weights (fewer split-K plans, S x the work per weight byte streamed).  Each scene keeps its own frame
    store and bookkeeping (an `InfiniteSceneGeneration` per scene); no data is shared between scenes, and a scene's frames
    match its solo run up to the summation order a different tile plan implies (same codebook indices away from near-ties,
    RGB-D within 5e-5: tests/test_gpu_lockstep.py).

    `use_rgbd_integration=True`: each scene keeps its own geometry-only fused volume (and its own `_tsdf_log`: the run's tail —
    export_point_clouds, export_triangle_mesh, colour_volume — works per scene); the S volumes share the pose grid, hence the box
    of units, and advance through the scene-batched TSDF kernels: one integration and one ray cast per step whatever S
    (tsdf.integrate_many_scenes / render_depth_scenes), then one inverse warp and one depth normalisation at B = S
    (tests/test_gpu_lockstep_rgbd.py)."""

    MAX_SPLAT_SOURCES = 64      # SGAM_MAX_SRCS of csrc/warp.hip: entries of the by-value pointer table of one splat launch
    MAX_TSDF_SOURCES = 8        # MAX_SRC of csrc/tsdf.hip: source frames of one integration step

    def __init__(self, model, data, seed_frames, seed_indices=None, output_dim=None, **scene_kw):
        from .inference_pipeline import InfiniteSceneGeneration
        self.rgbd = bool(scene_kw.get("use_rgbd_integration"))
        if self.rgbd:
            if scene_kw.get("rgbd_depth_render", "raycast") == "mesh":
                raise ValueError("LockstepScenes: rgbd_depth_render='mesh' extracts and rasterises one mesh per scene and step; "
                                 "use rgbd_depth_render='raycast' in lock step, or ConcurrentScenes for the mesh render")
            if scene_kw.get("tgt_depth_provider") is not None:
                raise ValueError("LockstepScenes: a tgt_depth_provider is called per scene and step; run such scenes solo "
                                 "(InfiniteSceneGeneration) or under ConcurrentScenes")
            if (scene_kw.get("num_src") or 0) > self.MAX_TSDF_SOURCES:
                raise ValueError(f"LockstepScenes: num_src={scene_kw['num_src']} source frames per scene; one TSDF integration step "
                                 f"takes at most {self.MAX_TSDF_SOURCES} — use num_src <= {self.MAX_TSDF_SOURCES} on the "
                                 "rgbd_integration branch")
            if scene_kw.get("tsdf_memory_budget_bytes") is None:
                # S pools of the solo default (a quarter of the free memory EACH) would exhaust the card: share one out
                free = torch.cuda.mem_get_info(model.device)[0]
                scene_kw["tsdf_memory_budget_bytes"] = min(48 << 30, free // 4) // len(seed_frames)
        self.model, self.data = model, data
        seed_indices = list(range(len(seed_frames))) if seed_indices is None else list(seed_indices)
        self.scenes = [InfiniteSceneGeneration(model, data, seed_index=si, output_dim=output_dim, seed_frame=sf, **scene_kw)
                       for si, sf in zip(seed_indices, seed_frames)]
        sc0 = self.scenes[0]
        if len(self.scenes) * sc0.num_src > self.MAX_SPLAT_SOURCES:
            # refuse at construction, not by a bare assert in mid-trajectory after some scenes' bookkeeping has advanced
            raise ValueError(f"LockstepScenes: {len(self.scenes)} scenes x {sc0.num_src} source frames = {len(self.scenes) * sc0.num_src} "
                             f"sources per splat launch; the kernel's pointer table holds {self.MAX_SPLAT_SOURCES} (SGAM_MAX_SRCS, "
                             f"csrc/warp.hip) — use at most {self.MAX_SPLAT_SOURCES // sc0.num_src} scenes per LockstepScenes")
        S, (H, W), dev = len(self.scenes), sc0.image_resolution, sc0.device
        self.S = S
        # the batch's persistent model input: the warp writes it, the captured graph reads it by address
        self._warp_out = {"x": torch.empty((S, 4, H, W), device=dev), "extrap": torch.empty((S, 1, H, W), device=dev, dtype=torch.bool),
                          "winner": torch.empty((S, H * W), device=dev, dtype=torch.int32)}
        self._warp_out["x"]._sgam_persistent = self._warp_out["extrap"]._sgam_persistent = True
        self._K_S = sc0._K_dev.expand(S, 3, 3).contiguous()
        self._Kinv_Sn = {}
        if self.rgbd:
            # the rgbd conditioning's persistent buffers.  The warp and the normalisation write contiguous planes; the planes of
            # an (S,4,H,W) tensor are not (S > 1), so one cat per step assembles the model input
            self._tgt_depth = torch.empty((S, H, W), device=dev)
            self._warped = torch.empty((S, 3, H, W), device=dev)
            self._norm_depth = torch.empty((S, 1, H, W), device=dev)
            self._Kinv_S = sc0._Kinv_dev.expand(S, 3, 3).contiguous()
            self._K_Sn = {}

    @property
    def curr(self):
        return self.scenes[0].curr

    @torch.no_grad()
    def step(self, keep_results=False):
        """one generated frame per scene.  Returns the step's batched tensors (views of persistent / graph-static buffers,
        like one_step_prediction: cloned with keep_results)."""
        import numpy as np
        from . import ops
        sc0 = self.scenes[0]
        tgt = sc0.next_pose(sc0.curr)
        if self.rgbd:
            x, mask, srcs_all = self._rgbd_conditioning(tgt)
            return self._forward_and_feedback(tgt, srcs_all, x, mask, keep_results, tgt_depth=self._tgt_depth)
        feats, depths, Ts, srcs_all = [], [], [], []
        for sc in self.scenes:
            if sc.curr != sc0.curr:
                raise RuntimeError("LockstepScenes: the scenes left lock step")
            srcs, _ = sc.get_src_grid_coords(tgt)
            tgt_meta = sc.transform_grid[tgt[0]][tgt[1]]
            R, t, _ = sc.relative_poses(tgt_meta, [sc.transform_grid[c[0]][c[1]] for c in srcs])
            T = np.zeros((len(srcs), 4, 4), dtype=np.float32)
            T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R, t, 1.0
            Ts.append(T)
            feats += [sc.frames[c]["rgb_f"] for c in srcs]
            depths += [sc._src_depth(c) for c in srcs]
            srcs_all.append(srcs)
        n = len(srcs_all[0])
        if any(len(s) != n for s in srcs_all):
            raise RuntimeError("LockstepScenes: scenes disagree on the number of source frames")
        (T_dev,) = sc0._upload(np.concatenate(Ts))
        if n not in self._Kinv_Sn:
            self._Kinv_Sn[n] = sc0._Kinv_dev.expand(self.S * n, 3, 3).contiguous()
        o = ops.forward_splat_srcs(feats, depths, self._K_S, self._Kinv_Sn[n], T_dev.reshape(self.S * n, 4, 4), B=self.S,
                                   dataset=self.data, want=("x", "extrap"), extrap_bool=True, out=self._warp_out)
        return self._forward_and_feedback(tgt, srcs_all, o["x"], o["extrap"], keep_results)

    def _rgbd_conditioning(self, tgt):
        """the rgbd_integration branch's model input for S scenes (InfiniteSceneGeneration.rgbd_integration + prepare_batch_data
        + get_x, per scene the same values): fuse every scene's sources into its volume, ray-cast the S target depths, inverse-warp
        the sources into them, normalise.  Returns x (S,4,H,W), the hole mask (S,1,H,W) and the scenes' source coordinates."""
        import numpy as np
        from . import ops, tsdf
        sc0 = self.scenes[0]
        feats, depths, T_t2s, srcs_all, w2c, c2w = [], [], [], [], [], []
        for sc in self.scenes:
            if sc.curr != sc0.curr:
                raise RuntimeError("LockstepScenes: the scenes left lock step")
            srcs, _ = sc.get_src_grid_coords(tgt)
            nodes = [sc.transform_grid[c[0]][c[1]] for c in srcs]
            T_t2s.append(sc.relative_poses(sc.transform_grid[tgt[0]][tgt[1]], nodes)[2])
            feats += [sc.frames[c]["rgb_f"] for c in srcs]
            depths.append([sc.frames[c]["depth"] for c in srcs])       # as loaded (reference :570-580), not the splat's re-converted map
            w2c.append([nd["T"] for nd in nodes])
            c2w.append([nd["T_inv"] for nd in nodes])
            srcs_all.append(srcs)
        n = len(srcs_all[0])
        if n == 0 or any(len(s) != n for s in srcs_all):
            raise RuntimeError("LockstepScenes: scenes disagree on the number of source frames")
        S, (H, W) = self.S, sc0.image_resolution
        volumes = [sc.volume for sc in self.scenes]
        tsdf.integrate_many_scenes(volumes, depths, sc0.K, w2c, Ts_c2w_per_scene=c2w)
        for sc, srcs in zip(self.scenes, srcs_all):
            sc._tsdf_log.append(srcs)
        z0, z1 = sc0._Z_RANGE[self.data]
        tgt_node = sc0.transform_grid[tgt[0]][tgt[1]]                  # (the scenes share the pose grid)
        tsdf.render_depth_scenes(volumes, sc0.K, [tgt_node["T"]] * S, H, W, z0, z1, Ts_c2w=[tgt_node["T_inv"]] * S, out=self._tgt_depth)
        (T_dev,) = sc0._upload(np.concatenate(T_t2s))
        if n not in self._K_Sn:
            self._K_Sn[n] = sc0._K_dev.expand(S * n, 3, 3).contiguous()
        ops.inverse_warp_srcs(feats, [d for ds in depths for d in ds], self._tgt_depth, self._K_Sn[n], self._Kinv_S,
                              T_dev.reshape(S * n, 4, 4), B=S, out=self._warped)
        x, mask = self._warp_out["x"], self._warp_out["extrap"]
        ops.depth_normalise(self._tgt_depth[:, None], self.data, compute_mask=True, mask_bool=True, out=self._norm_depth, out_mask=mask)
        torch.cat((self._warped, self._norm_depth), 1, out=x)
        return x, mask, srcs_all

    def _forward_and_feedback(self, tgt, srcs_all, x, mask, keep_results, **extra):
        from . import ops
        sc0 = self.scenes[0]
        if sc0.infill_sampler == "device":       # every scene draws from its own stream, at the frame index: what it draws alone
            self.model.infill_call = sc0.curr
            self.model.infill_streams = [sc.seed_index for sc in self.scenes]
        decs, _, idx, pre_q = self.model(x, topk=sc0.topk, extrapolation_mask=mask, sample_number=1, get_codebook_count=True,
                                        get_pre_quantized_feature=True)
        dec = decs[0][0]                                             # (S,4,H,W); sample number is 1
        rgb_f, depth, rgb_u8 = ops.frame_feedback(dec, self.data, want_u8=True)
        for s, sc in enumerate(self.scenes):
            sc.save_to_store(tgt, rgb_u8[s], rgb_f[s], depth[s])
            sc.curr += 1
        own = (lambda t: t.clone()) if keep_results else (lambda t: t)
        return {"tgt": tgt, "src_coords": srcs_all, "x": own(x), "extrapolation_mask": own(mask), "rgbd": own(dec),
                "indices": own(idx), "pre_quantized_features": own(pre_q), **{k: own(v) for k, v in extra.items()}}

    def expand(self, steps=None, range_check_every=8):
        """`steps` lock-stepped frames per scene (default: to the end of the grid), with the split-fp32 range guard checked
        every `range_check_every` frames like InfiniteSceneGeneration.scene_expansion (on a trip: mode 'mfma', the frames
        since the last verified one are regenerated)."""
        from . import ops
        sc0 = self.scenes[0]
        total = sc0.output_dim[0] * sc0.output_dim[1]
        end = total if steps is None else min(total, sc0.curr + steps)
        ops.range_flag(sc0.device)
        verified = sc0.curr
        while sc0.curr < end:
            self.step()
            if sc0.curr == end or (sc0.curr - verified) >= range_check_every:
                if ops.F32_MODE == "split" and ops.f32x_range_tripped():
                    import warnings
                    warnings.warn(f"sgam split-fp32 path: an activation left fp16's range; regenerating frames {verified}.."
                                  f"{sc0.curr - 1} of every lock-stepped scene on the fp32-in MFMA path", RuntimeWarning)
                    ops.set_f32_mode("mfma")
                    self.model._graphs = {}
                    for sc in self.scenes:      # the flag is per GPU, not per scene: every scene rewinds together
                        sc.curr = sc._rewind_to(verified)      # (restarts the scene's volume: new objects, a new scene table)
                verified = sc0.curr
        for sc in self.scenes:
            if sc.volume is not None:
                sc.volume.check()               # pool overflow / samples outside the box: do not lose geometry silently
        return [sc.frames for sc in self.scenes]
