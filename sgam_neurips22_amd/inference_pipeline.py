"""InfiniteSceneGeneration — the frame-autoregressive scene-expansion loop on the HIP backend.

Counterpart of the reference harness ``sgam/inference_pipeline.py`` (constructor :23-142, prepare_grid
:157-204, zig_zag_order :452-474, get_src_grid_coords :507-531, prepare_batch_data :533-609,
inverse_warping :662-743, one_step_prediction :860-926, save_to_disk :928-959), rebuilt around an
IN-MEMORY frame store: generated frames never leave HBM between steps.  What the reference does through
its PNG / NPY round trip is reproduced bit-for-bit on the GPU by ``ops.frame_feedback``:
RGB is quantised to uint8 by truncation and re-expanded as float32(u/127.5-1), depth is de-normalised in
the reference's fp32 expression order.  Files are written only by ``export_to_disk`` after the run.

Pose grid, zig-zag order, source selection (radius 0.3 / 1.0, nearest ``num_src``) and
``T_rel = T_tgt @ inv(T_src)`` are the reference's float64 numpy formulas (host logic, a few 4x4s per
step).  ``use_rgbd_integration=True`` (reference :745-838: Open3D TSDF fusion of the source frames, mesh
extraction and an off-screen depth render at the target pose) runs on the device: ``tsdf.TsdfVolume``
integrates the source depth maps with Open3D's published rule and ray-casts the fused surface
(csrc/tsdf.hip; SURVEY §8 f1 — parity pinned to oracle/tsdf.py and analytic scenes, not to Open3D itself);
a ``tgt_depth_provider`` callback can still replace it.  ``inverse_warping`` is a HIP kernel.
"""
import os
from pathlib import Path

import numpy as np
import torch

from . import ops
from .generative_sensing_module.model import VQModel

_GL2CV = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], dtype=np.float64)

_START = {
    "google_earth": (np.array([[1., 0., 0., -3.], [0., 0.86602527, -0.50000024, -6.],
                               [0., 0.50000024, 0.86602527, 2.], [0., 0., 0., 1.]]),
                     np.array([0., 0.11878788, 0.]), np.array([0.12, 0, 0.])),
    "clevr-infinite": (np.array([[1., 0., 0., -20.], [0., 0.95533651, -0.29552022, -20.],
                                 [0., 0.29552022, 0.95533651, 0.], [0., 0., 0., 1.]]),
                       np.array([0, 0.81632614, 0.]), np.array([0.81632614, 0, 0.])),
}


def intrinsics(data, image_resolution=(256, 256)):
    """reference :61-65 (CLEVR) and :83-89 (GoogleEarth, rows scaled by res/512)."""
    if data == "clevr-infinite":
        return np.array([[355.5555, 0, 128], [0, 355.5555, 128], [0, 0, 1]], dtype=np.float64)
    if data == "google_earth":
        K = np.array([[497.77774, 0, 256], [0, 497.77774, 256], [0, 0, 1]], dtype=np.float64)
        K[0] = K[0] * image_resolution[1] / 512
        K[1] = K[1] * image_resolution[0] / 512
        return K
    raise NotImplementedError(data)


def ray_to_z_depth(depth, K):
    """CLEVR ray-length -> z-depth conversion (reference :71-79 / :582-590), float64 numpy."""
    h, w = depth.shape[:2]
    xs, ys = np.meshgrid(np.linspace(0, w - 1, w), np.linspace(0, h - 1, h))
    return depth * K[0][0] / np.sqrt(K[0][0] ** 2 + (K[0][2] - ys - 0.5) ** 2 + (K[1][2] - xs - 0.5) ** 2)


def synthetic_seed_frame(data, seed_index=0, res=256):
    """Seeded smooth RGB-D seed frame for boxes without the reference's templates/ (bench, GPU tests):
    RGB uint8, depth fp32 in the template range ([1.4,3.4] GoogleEarth, [10.3,15.5] CLEVR)."""
    rs = np.random.RandomState(1000 + int(seed_index))        # main_scene_generation passes seed_index through argparse
    yy, xx = np.meshgrid(np.linspace(0, 1, res), np.linspace(0, 1, res), indexing="ij")
    acc = np.zeros((res, res, 4))
    for _ in range(12):
        fx, fy = rs.uniform(0.5, 6, 2)
        ph = rs.uniform(0, 2 * np.pi, 4)
        amp = rs.uniform(0.2, 1.0, 4)
        acc += amp * np.sin(2 * np.pi * (fx * xx + fy * yy)[..., None] + ph)
    acc = (acc - acc.min((0, 1))) / (acc.max((0, 1)) - acc.min((0, 1)))
    rgb = (acc[..., :3] * 255).astype(np.uint8)
    lo, hi = (1.4, 3.4) if data == "google_earth" else (10.3, 15.5)
    depth = (lo + (hi - lo) * acc[..., 3]).astype(np.float32)
    return rgb, depth


def load_template_seed(data, seed_index, image_resolution, templates_root="templates"):
    """The reference's seed frame exactly as prepare_batch_data reads it (:534-537): PIL LANCZOS resize of the
    PNG, nearest resize of the depth map.  Host codec boundary."""
    from PIL import Image
    import torch.nn.functional as F
    if data == "google_earth":
        d = Path(templates_root) / "google_earth" / f"seed{seed_index}"
        img_fn = sorted(d.glob("im*"))[0]
        dm_fn = Path(str(img_fn).replace("im", "dm").replace(".png", ".npy"))
    else:
        d = Path(templates_root) / "clevr-infinite"
        img_fn, dm_fn = d / "im_00000_00_00.png", d / "dm_00000_00_00.npy"
    rgb = np.array(Image.open(img_fn).convert("RGB").resize((image_resolution[1], image_resolution[0]),
                                                            resample=Image.LANCZOS))
    depth = np.load(dm_fn)
    if data == "clevr-infinite":  # the reference rewrites the template depth at construction (:71-79), in float64
        depth = ray_to_z_depth(depth, intrinsics(data))
    depth = F.interpolate(torch.from_numpy(depth[None, None]), size=image_resolution)[0][0].numpy().squeeze()
    # CLEVR: stays float64 — the reference keeps the seed depth in float64 through BOTH ray->z conversions (the .npy it
    # rewrites at construction, :79, and the per-load re-conversion, :582-590) and rounds to fp32 once (:607)
    return rgb, (depth if data == "clevr-infinite" else depth.astype(np.float32))


class _Lazy(dict):
    """dict whose listed keys are built on first access: the reference's batch / result dictionaries carry stacked
    copies of the source frames (`src_imgs`, `src_depths`, ...) that the device path itself never reads — they are
    materialised only for a caller that asks for them"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._makers = {}

    def lazy(self, key, fn):
        self._makers[key] = fn
        return self

    def __missing__(self, key):
        if key in self._makers:
            self[key] = v = self._makers.pop(key)()
            return v
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._makers


class InfiniteSceneGeneration:
    def __init__(self, dynamic_model, data, topk=1, step_size_denom=2, use_rgbd_integration=False,
                 use_discriminator_loss=False, discriminator_loss_weight=0, recon_on_visible=False,
                 offscreen_rendering=True, output_dim=None, seed_index=0, num_src=None, seed_frame=None,
                 templates_root="templates", tgt_depth_provider=None, image_resolution=(256, 256),
                 trajectory_shape="grid", grid_transform_path=None, rgbd_depth_render="raycast",
                 infill_sampler="host", infill_seed=0, infill_per_token=False, tsdf_memory_budget_bytes=None):
        """`trajectory_shape` / `grid_transform_path` are this backend's spelling of what the reference hard-codes: its
        constructor sets trajectory_shape = 'grid' (:67, :82) and fills `grid_res/<data>_seed<k>` with the seed frame, so its
        'spiral' / 'cylinder' / 'trajectory' pose sets (:206-421) and the known-frame map (:144-155) are reachable only by
        editing it.  Here they are arguments: the shape selects the pose set, and a `grid_transform_path` folder holding
        `dm_<frame>_<ii>_<jj>.npy` + `im_<frame>_<ii>_<jj>.png` pairs (the layout export_to_disk writes) marks those poses
        visited and loads them into the frame store as KNOWN frames: a 'trajectory' run (which also reads `cam0_to_world.txt`
        there) warps from them; the grid / spiral / cylinder loops regenerate every pose from index 1, like the reference's —
        known frames there only seed `anchor_poses`, nothing is resumed.

        `infill_sampler` picks who draws the `topk > 1` infill codes: "host" = the reference's CPU-generator draws (eager
        forwards), "device" = the counter-based sampler on the GPU (VQModel.set_infill_sampler): frame `i` of this scene
        draws from (infill_seed, stream id = seed_index, call number = i) whatever ran before it — a rewind regenerates the
        same frames and a lock-stepped scene draws what it draws alone — and the forward replays as a captured graph.
        `infill_per_token=True`: every token from its own distribution rather than the reference's token-0 one.

        `tsdf_memory_budget_bytes`: the brick pool of this scene's fused volume (TsdfVolume(memory_budget_bytes=...)); None = its
        default, a quarter of the memory free when the volume is made."""
        if infill_sampler not in ("host", "device"):
            raise ValueError(f"infill_sampler: 'host' or 'device', not {infill_sampler!r}")
        if data not in _START:
            raise NotImplementedError(data)
        if rgbd_depth_render not in ("raycast", "mesh"):
            raise ValueError(f"rgbd_depth_render: 'raycast' or 'mesh', not {rgbd_depth_render!r}")
        # the depth rgbd_integration conditions on: "raycast" = the direct ray cast of the fused TSDF (default), "mesh" = the
        # reference's per-step structure, marching-cubes mesh of the volume + depth render of that mesh (:777-826)
        self.rgbd_depth_render = rgbd_depth_render
        if trajectory_shape not in ("grid", "spiral", "cylinder", "trajectory"):
            raise NotImplementedError(trajectory_shape)
        self.dynamic_model, self.data, self.topk = dynamic_model, data, topk
        self.seed_index, self.step_size_denom = seed_index, step_size_denom
        self.use_rgbd_integration = use_rgbd_integration
        self.tgt_depth_provider = tgt_depth_provider
        self.tsdf_memory_budget_bytes = tsdf_memory_budget_bytes
        self.image_resolution = tuple(image_resolution)
        self.output_dim = output_dim if output_dim is not None else ((20, 20) if data == "clevr-infinite" else (100, 1))
        self.K = intrinsics(data, self.image_resolution)
        self.K_inv = np.linalg.inv(self.K)
        is_vq = isinstance(dynamic_model, VQModel)
        self.infill_sampler = infill_sampler if is_vq else "host"
        if is_vq and (infill_sampler == "device" or dynamic_model.quantize.device_sampler is not None):
            dynamic_model.set_infill_sampler(infill_sampler, seed=infill_seed, per_token=infill_per_token)
        default_src = 5 if data == "clevr-infinite" else 3
        self.num_src = (default_src if num_src is None else num_src) if is_vq else 1
        self.curr = 1
        self.trajectory_shape = trajectory_shape
        self.grid_transform_path = None if grid_transform_path is None else Path(grid_transform_path)
        self.anchor_poses = {}
        self.device = dynamic_model.device
        if seed_frame is None:
            if os.path.isdir(os.path.join(templates_root, data)):
                seed_frame = load_template_seed(data, seed_index, self.image_resolution, templates_root)
            else:
                import warnings
                warnings.warn(f"{templates_root}/{data} not found: starting from a SYNTHETIC seed frame, not the reference's "
                              "template", RuntimeWarning)
                seed_frame = synthetic_seed_frame(data, seed_index, self.image_resolution[0])
        self.frames = {}        # grid coord -> dict(rgb_f (H,W,3) fp32, depth (H,W) fp32, rgb_u8, index)
        known_map = self.get_known_map()
        if trajectory_shape == "grid":                      # reference :104-116
            self.prepare_grid(self.output_dim, known_map)
            self._ordered_grid_coords = self.zig_zag_order()
        elif trajectory_shape == "spiral":
            self.prepare_spiral(self.output_dim, known_map)
            self._ordered_grid_coords = self.zig_zag_order()
        elif trajectory_shape == "cylinder":
            self.prepare_ring(self.output_dim, known_map, horizontal_offset=0.002)
            self._ordered_grid_coords = self.zig_zag_order()
        else:
            if self.grid_transform_path is None:
                raise ValueError("trajectory_shape='trajectory' reads <grid_transform_path>/cam0_to_world.txt")
            self._ordered_grid_coords = self.prepare_trajectory(self.output_dim[0], known_map,
                                                                pose_path=self.grid_transform_path / "cam0_to_world.txt")
        self._store_seed(seed_frame)
        self._load_known_frames(known_map)
        self.dynamic_model.use_rgbd_integration = use_rgbd_integration
        self.volume = None
        self._tsdf_log = []      # the source coordinates of every integration step, in order (colour_volume replays them)
        self._tsdf_log_stale = []   # logged source coordinates whose frame was overwritten since (the replay would fuse the new one)
        if use_rgbd_integration and tgt_depth_provider is None:
            self.volume = self._make_volume()
        K32 = torch.from_numpy(self.K.astype(np.float32))
        # host-side fp32 inverse like the reference (warp.py:210 / inference_pipeline.py:694), done once
        self._K_dev = K32.to(self.device)
        self._Kinv_dev = torch.inverse(K32).to(self.device)
        self._Kinv_n = {}        # n sources -> (n,3,3) contiguous copy of the inverse intrinsics
        self._K_n = {}           # n sources -> (n,3,3) contiguous copy of the intrinsics
        # pinned staging ring for the per-step pose upload (see _upload)
        self._stage = [torch.empty(4096, dtype=torch.float32).pin_memory() for _ in range(8)] \
            if self.device.type == "cuda" else None
        self._stage_done = [None] * 8
        self._stage_i = 0
        H, W = self.image_resolution
        # the target view is unknown at inference: the reference feeds zeros (:560-561); constant, so made once
        self._dst_img = torch.zeros((1, H, W, 3), device=self.device)
        self._dst_depth = torch.zeros((1, H, W), device=self.device)
        self._x_dst = None       # get_x's x_dst of that constant target, kept after the first step
        # persistent outputs of the conditioning warp = the model's graph inputs (captured by address: no copy per step)
        self._warp_out = {"x": torch.empty((1, 4, H, W), device=self.device),
                          "extrap": torch.empty((1, 1, H, W), device=self.device, dtype=torch.bool),
                          "winner": torch.empty((1, H * W), device=self.device, dtype=torch.int32)} \
            if self.device.type == "cuda" else None
        if self._warp_out is not None:
            self._warp_out["x"]._sgam_persistent = self._warp_out["extrap"]._sgam_persistent = True

    # ---------------------------------------------------------------- TSDF fusion (reference :119-133, 745-838)
    # view-space z range of valid depths per dataset: the inverse-depth codec's bounds (model.py:210-229)
    _Z_RANGE = {"google_earth": (0.05, 4.8), "clevr-infinite": (1.0, 16.5)}

    def _make_volume(self, color=False, max_bricks=None):
        from .tsdf import VOLUME_PARAMS, TsdfVolume, frustum_bounds, UNIT
        voxel, trunc = VOLUME_PARAMS[self.data]
        poses = [node["T"] for row in self.transform_grid for node in row]
        H, W = self.image_resolution
        lo, hi = frustum_bounds(self.K, poses, H, W, self._Z_RANGE[self.data][1], margin=trunc + voxel * UNIT)
        # The loop's volume fuses GEOMETRY only: the conditioning path consumes nothing but the rendered depth, and colour
        # is 60 % of a voxel's bytes.  The reference's RGB8 colour (:123-131) is fused when the run's tail asks for it:
        # export_point_clouds replays the logged integrations into a colour volume (same kernels, same order).
        return TsdfVolume(voxel, trunc, lo, hi, self.device, color=color, memory_budget_bytes=self.tsdf_memory_budget_bytes,
                          max_bricks=max_bricks)

    def rgbd_integration(self, src_nodes, tgt_node):
        """reference :745-838: integrate every source frame of this step (again — the volume is cumulative, like the
        reference's self.volume), then render the fused surface's depth at the target pose.  (H,W) device fp32.
        One pass over the union of the units the sources open (TsdfVolume.integrate_many); poses are the nodes' own 4x4s."""
        # the reference fuses the depth as loaded (:570-574) — for the CLEVR seed that is the ONCE-converted map;
        # its second ray->z conversion (:582-590) only touches batch['src_depths'], after the fusion
        coords = [s["grid_coord"] for s in src_nodes]
        self.volume.integrate_many([self.frames[c]["depth"] for c in coords], self.K, [s["T"] for s in src_nodes],
                                   Ts_c2w=[s["T_inv"] for s in src_nodes])
        self._tsdf_log.append(coords)
        H, W = self.image_resolution
        z0, z1 = self._Z_RANGE[self.data]
        if self.rgbd_depth_render == "mesh":
            return self.volume.render_mesh_depth(self.K, tgt_node["T"], H, W, z0, z1)
        return self.volume.render_depth(self.K, tgt_node["T"], H, W, z0, z1, T_c2w=tgt_node["T_inv"])

    def colour_volume(self, max_bricks=None):
        """The fused volume WITH the reference's RGB8 colour (:123-131, 777-790): the logged integrations of the run replayed
        in order — every source frame is still in the frame store — through the colour-fusing form of the same kernels.
        max_bricks: the colour pool's size (default: TsdfVolume's, from the memory budget)."""
        vol = self._make_volume(color=True, max_bricks=max_bricks)
        for coords in self._tsdf_log:
            nodes = [self.transform_grid[c[0]][c[1]] for c in coords]
            vol.integrate_many([self.frames[c]["depth"] for c in coords], self.K, [n["T"] for n in nodes],
                               rgbs_u8=[self.frames[c]["rgb_u8"] for c in coords], Ts_c2w=[n["T_inv"] for n in nodes])
        return vol

    # ---------------------------------------------------------------- grid / order / source choice
    def get_known_map(self):
        """reference :144-155: the frames a result folder already holds, keyed by grid coordinate — file names
        `dm_<frame index>_<ii>_<jj>.npy` (+ the `im_*.png` beside each).  No folder: nothing is known but the seed."""
        known = {}
        if self.grid_transform_path is None:
            return known
        for f in Path(self.grid_transform_path).glob("dm*"):
            idx, gi, gj = (int(v) for v in f.name[3:-4].split("_")[:3])
            # (the sibling file by NAME: the reference's str.replace("dm", "im") rewrites those letters anywhere in the path)
            known[(gi, gj)] = {"rgb_path": str(f.with_name("im" + f.name[2:-3] + "png")), "depth_path": str(f),
                               "orig_frame_idx": idx}
        return known

    def _node(self, R, t, coord, known_map):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        # "T" = [R | t] world -> camera and its inverse, made once per pose (the step assembles nothing)
        node = {"R": R, "t": t, "K": self.K, "position": -R.T @ t, "visited": coord in known_map, "grid_coord": coord,
                "T": T, "T_inv": np.linalg.inv(T)}
        if coord in known_map:
            node["rgb_path"], node["depth_path"] = known_map[coord]["rgb_path"], known_map[coord]["depth_path"]
            self.anchor_poses[coord] = node
        return node

    def _load_known_frames(self, known_map):
        """the known frames of the folder enter the frame store exactly as the reference reads them back in
        prepare_batch_data (:534-537, 570-574): PIL LANCZOS resize of the PNG, nearest resize of the depth map, RGB through
        the uint8 codec.  The seed pose keeps the seed frame handed to the constructor."""
        if not known_map:
            return
        from PIL import Image
        import torch.nn.functional as F
        H, W = self.image_resolution
        for coord in sorted(known_map, key=lambda c: known_map[c]["orig_frame_idx"]):
            if coord == self._ordered_grid_coords[0] and coord in self.frames:
                continue
            if coord[0] >= len(self.transform_grid) or coord[1] >= len(self.transform_grid[coord[0]]):
                continue                                     # a frame outside this run's pose set
            rgb = np.array(Image.open(known_map[coord]["rgb_path"]).convert("RGB").resize((W, H), resample=Image.LANCZOS))
            depth = np.load(known_map[coord]["depth_path"])
            depth = F.interpolate(torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)[None, None]), size=(H, W))[0][0]
            u8 = torch.from_numpy(np.ascontiguousarray(rgb)).to(self.device)
            self.frames[coord] = {"rgb_u8": u8, "rgb_f": ops.rgb_u8_to_f32(u8), "depth": depth.contiguous().to(self.device),
                                  "index": known_map[coord]["orig_frame_idx"]}
            self.transform_grid[coord[0]][coord[1]]["visited"] = True

    def prepare_grid(self, grid_size, known_map=None):
        known_map = known_map or {}
        start, step_i, step_j = _START[self.data]
        step_i, step_j = step_i / self.step_size_denom, step_j / self.step_size_denom
        self.transform_grid = []
        self.anchor_poses = {}
        for i in range(grid_size[0]):
            row = []
            for j in range(grid_size[1]):
                c2w = np.eye(4)
                c2w[:3, :3] = start[:3, :3]
                c2w[:3, 3] = start[:3, 3] + step_unit(step_j, j) + step_unit(step_i, i)
                w2c = np.linalg.inv(c2w @ _GL2CV)
                row.append(self._node(w2c[:3, :3], w2c[:3, 3], (i, j), known_map))
            self.transform_grid.append(row)

    def prepare_spiral(self, grid_size, known_map=None):
        """reference :206-288: an Archimedean spiral of grid_size[0] poses in the seed camera's plane (arc 1, separation 1,
        positions theta (cos theta, sin theta) / 10 from the seed position), each camera turned about z by the reference's
        `90 - theta` — radians, as written there — one pose per row of the grid."""
        known_map = known_map or {}
        start = _START[self.data][0]
        self.transform_grid, self.anchor_poses = [], {}
        w2c = np.linalg.inv(start @ _GL2CV)
        R, t = w2c[:3, :3], w2c[:3, 3]
        origin = -R.T @ t
        arc, separation = 1, 1
        r = arc
        b = separation / (2 * np.pi)
        theta = float(r) / b
        for i in range(grid_size[0]):
            a = 90 - theta
            c2w = np.eye(4)
            c2w[:3, 3] = origin
            c2w[0, 3] += theta * np.cos(theta) / 10
            c2w[1, 3] += theta * np.sin(theta) / 10
            c2w[:3, :3] = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]])
            w2c = np.linalg.inv(c2w)
            theta += float(arc) / r
            r = b * theta
            self.transform_grid.append([self._node(w2c[:3, :3], w2c[:3, 3], (i, 0), known_map)])

    def prepare_ring(self, grid_size, known_map=None, horizontal_offset=0):
        """reference :290-360 (the 'cylinder' shape): every pose is the previous one turned by pi / 80 about the camera's x
        axis and moved by -step_i (x component replaced by `horizontal_offset`) in ITS OWN frame — a ring that closes after
        160 poses.  The reference appends every pose to ONE row while naming them (i, 0), so its own loop could not index
        them (transform_grid[i][0]); here pose i is row i, like the spiral — same poses, steppable."""
        known_map = known_map or {}
        start, step_i, _ = _START[self.data]
        step_i = step_i / self.step_size_denom
        if self.data != "google_earth":
            step_i = -step_i                                  # the reference's CLEVR branch of this shape negates it (:309)
        self.transform_grid, self.anchor_poses = [], {}
        curr = start @ _GL2CV
        theta = np.pi / 80
        rot = np.eye(4)
        rot[:3, :3] = np.array([[1, 0, 0], [0, np.cos(theta), np.sin(theta)], [0, -np.sin(theta), np.cos(theta)]])
        for i in range(grid_size[0]):
            T = np.eye(4)
            T[:3, 3] = -step_i
            T[0, 3] = horizontal_offset
            w2c = T @ rot @ np.linalg.inv(curr)
            curr = np.linalg.inv(w2c)
            self.transform_grid.append([self._node(w2c[:3, :3], w2c[:3, 3], (i, 0), known_map)])

    @staticmethod
    def load_poses(pose_file):
        """reference :362-368: one pose per line — frame index, then the row-major 4 x 4 camera-to-world matrix"""
        poses = np.loadtxt(pose_file)
        frames = poses[:, 0].astype(int)
        mats = np.reshape(poses[:, 1:], (-1, 4, 4))
        return {int(k): {"frame_idx": int(k), "pose": v} for k, v in zip(frames, mats)}

    def prepare_trajectory(self, trajectory_length, known_map, pose_path):
        """reference :370-421: `trajectory_length` consecutive poses of the file, starting at the frame index of the first
        known frame; returns the visiting order (i, 0)."""
        self.transform_grid, self.anchor_poses = [], {}
        poses = self.load_poses(pose_path)
        if not known_map:
            raise ValueError("a 'trajectory' run starts from a known frame: none found in " + str(self.grid_transform_path))
        start_idx = known_map[sorted(known_map.keys())[0]]["orig_frame_idx"]
        assert start_idx in poses
        order_idx = sorted(poses.keys())
        ptr = order_idx.index(start_idx)
        assert ptr + trajectory_length < len(order_idx)
        ordered = []
        for i in range(trajectory_length):
            w2c = np.linalg.inv(poses[order_idx[ptr + i]]["pose"])
            self.transform_grid.append([self._node(w2c[:3, :3], w2c[:3, 3], (i, 0), known_map)])
            ordered.append((i, 0))
        return ordered

    def get_closest_anchor(self, curr_node):
        """reference :423-431: the known pose nearest to a node"""
        best, res = 99999999, None
        for k in self.anchor_poses:
            d = np.linalg.norm(self.anchor_poses[k]["position"] - curr_node["position"])
            if d < best:
                best, res = d, self.anchor_poses[k]
        return res

    def zig_zag_order(self):
        rows, cols = self.output_dim
        diag = [[] for _ in range(rows + cols - 1)]
        for i in range(rows):
            for j in range(cols):
                if (i + j) % 2 == 0:
                    diag[i + j].insert(0, (i, j))
                else:
                    diag[i + j].append((i, j))
        order = [c for d in diag for c in d]
        self.transform_grid[order[0][0]][order[0][1]]["visited"] = True
        return order

    def row_major_order(self):
        """reference :477-488: boustrophedon over the rows"""
        rows, cols = self.output_dim
        order = [(i, j if i % 2 == 0 else cols - j - 1) for i in range(rows) for j in range(cols)]
        self.transform_grid[order[0][0]][order[0][1]]["visited"] = True
        return order

    def column_major_order(self):
        """reference :490-501: boustrophedon over the columns"""
        rows, cols = self.output_dim
        order = [(i if j % 2 == 0 else rows - i - 1, j) for j in range(cols) for i in range(rows)]
        self.transform_grid[order[0][0]][order[0][1]]["visited"] = True
        return order

    def next_pose(self, curr):
        return self._ordered_grid_coords[curr]

    def get_src_grid_coords(self, tgt_grid_coord):
        if getattr(self, "trajectory_shape", "grid") == "trajectory":           # reference :531: the num_src poses just behind the target
            # (the reference indexes tgt - i - 1 unchecked: close to the start that wraps to the END of the trajectory; here the
            # sources are the poses that exist behind the target — one_step_prediction checks that they hold a frame)
            return [(tgt_grid_coord[0] - i - 1, 0) for i in range(self.num_src) if tgt_grid_coord[0] - i - 1 >= 0], None
        tgt = self.transform_grid[tgt_grid_coord[0]][tgt_grid_coord[1]]
        radius = 0.3 if self.data != "clevr-infinite" else 1
        found = []
        for i in range(self.curr):
            cc = self._ordered_grid_coords[i]
            cand = self.transform_grid[cc[0]][cc[1]]
            dist = np.linalg.norm(cand["position"] - tgt["position"])
            if cand["visited"] and dist <= radius:
                found.append((cc, dist))
        found = sorted(found, key=lambda x: x[1])[: self.num_src]
        return [c for c, _ in found], None

    # ---------------------------------------------------------------- frame store
    def _store_seed(self, seed_frame):
        rgb_u8, depth = seed_frame
        u8 = torch.from_numpy(np.ascontiguousarray(rgb_u8)).to(self.device)
        fr = {"rgb_u8": u8, "rgb_f": ops.rgb_u8_to_f32(u8),  # table lookup = the PNG re-read
              "depth": torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(self.device), "index": 0}
        if self.data == "clevr-infinite":
            # the reference converts the seed's ray depth to z AGAIN on every load (:582-590), still in float64 (the
            # once-converted map was saved as float64, :79) and rounds to fp32 only at :607.  Both fp32 maps are derived
            # from the float64 once-converted depth: `depth` feeds rgbd_integration / inverse_warping (:570-580),
            # `depth_reconv` the forward splat (batch['src_depths']).
            d64 = np.asarray(depth, dtype=np.float64)
            fr["depth_reconv"] = torch.from_numpy(ray_to_z_depth(d64, self.K).astype(np.float32)).to(self.device)
        self.frames[(0, 0)] = fr
        self.transform_grid[0][0]["visited"] = True

    def _src_depth(self, coord):
        """the depth map prepare_batch_data puts into batch['src_depths'] (the forward splat's source depth)"""
        fr = self.frames[coord]
        return fr.get("depth_reconv", fr["depth"])

    # ---------------------------------------------------------------- batch assembly
    def relative_poses(self, tgt_node, src_nodes):
        T_tgt = tgt_node["T"]
        R_rels, t_rels, T_tgt2srcs = [], [], []
        for s in src_nodes:
            T_rel = T_tgt @ np.linalg.inv(s["T"])
            T_tgt2srcs.append(np.linalg.inv(T_rel))
            R_rels.append(T_rel[:3, :3])
            t_rels.append(T_rel[:3, 3])
        return np.stack(R_rels), np.stack(t_rels), np.stack(T_tgt2srcs)

    def _upload(self, *arrays):
        """Host fp32 arrays -> device tensors through ONE asynchronous copy out of a pinned staging slot.  A pageable
        `.to(device)` makes the host wait for everything queued on the stream — i.e. for the previous frame — and the
        GPU then idles while the host enqueues the next frame's conditioning launches."""
        flat = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in arrays])
        if self._stage is None or flat.size > self._stage[0].numel():
            devt = torch.from_numpy(flat).to(self.device)
        else:
            i = self._stage_i
            self._stage_i = (i + 1) % len(self._stage)
            if self._stage_done[i] is not None:
                self._stage_done[i].synchronize()        # only ever waits when the host is a whole ring ahead
            self._stage[i][:flat.size].copy_(torch.from_numpy(flat))
            devt = torch.empty(flat.size, dtype=torch.float32, device=self.device)
            devt.copy_(self._stage[i][:flat.size], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._stage_done[i] = ev
        outs, o = [], 0
        for a in arrays:
            outs.append(devt[o:o + a.size].view(a.shape))
            o += a.size
        return outs

    def prepare_batch_data(self, tgt_node, src_nodes, num_src):
        coords = [s["grid_coord"] for s in src_nodes]
        n = len(coords)
        R_rels, t_rels, T_tgt2srcs = self.relative_poses(tgt_node, src_nodes)
        # the sources stay where the frame store holds them: the warps read them through a pointer table
        feats = [self.frames[c]["rgb_f"] for c in coords]                                  # N x (H,W,3)
        depths = [self._src_depth(c) for c in coords]                                      # N x (H,W)
        # T_src2tgt = [R | t; 0 0 0 1] (model.py:190-194): the same fp32 values the device-side assembly would hold
        T = np.zeros((n, 4, 4), dtype=np.float32)
        T[:, :3, :3], T[:, :3, 3], T[:, 3, 3] = R_rels, t_rels, 1.0
        T_dev, T_t2s_dev, R_dev, t_dev = self._upload(T, T_tgt2srcs, R_rels, t_rels)
        if n not in self._Kinv_n:
            self._Kinv_n[n] = self._Kinv_dev.expand(n, 3, 3).contiguous()
        batch = _Lazy({
            "Ks": self._K_dev.expand(1, n, 3, 3),
            "_src_Kinv": self._Kinv_n[n], "_T_src2tgt": T_dev,
            "R_rels": R_dev[None], "t_rels": t_dev[None],
            "dst_img": self._dst_img, "dst_depth": self._dst_depth,
            "_src_list": (feats, depths), "_warp_out": self._warp_out,
        })
        batch.lazy("src_imgs", lambda: torch.stack(feats)[None])                           # (1,N,H,W,3)
        batch.lazy("src_depths", lambda: torch.stack(depths)[None])                        # (1,N,H,W)
        if self.use_rgbd_integration:
            if self.tgt_depth_provider is not None:
                tgt_depth = self.tgt_depth_provider(self, tgt_node, src_nodes, batch)      # (H,W) device fp32
            else:
                tgt_depth = self.rgbd_integration(src_nodes, tgt_node)
            # inverse_warping sees the depths as loaded (:575-580) — for the CLEVR seed the once-converted map
            if n not in self._K_n:
                self._K_n[n] = self._K_dev.expand(n, 3, 3).contiguous()
            # written straight into the rgb planes of the persistent model input (B = 1: a contiguous view)
            dst = self._warp_out["x"][:, :3] if self._warp_out is not None else None
            warped = ops.inverse_warp_srcs(feats, [self.frames[c]["depth"] for c in coords], tgt_depth[None],
                                           self._K_n[n], self._Kinv_dev[None], T_t2s_dev, out=dst)
            batch["warped_tgt_features"] = warped
            batch["warped_tgt_depth"] = tgt_depth[None]
        return batch

    def inverse_warping(self, src_imgs, src_depths, tgt_depth, src_intrinsics, tgt_intrinsic, T_tgt2srcs,
                        padding_mode='zeros', depth_threshold=100, as_numpy=True, tgt_Kinv=None):
        """reference :662-743; returns item 0 of the (B,3,H,W) result ((3,H,W) numpy like the reference, or a
        device tensor with as_numpy=False)."""
        B, N = src_imgs.shape[:2]
        dev = src_imgs.device
        # fp32 inverse on the host like the reference (:694); callers that hold it already (the scene loop: one fixed K)
        # pass tgt_Kinv and skip the device->host round trip, which would otherwise serialise host and GPU every step
        Kinv = tgt_Kinv if tgt_Kinv is not None else \
            torch.inverse(tgt_intrinsic.detach().to("cpu", torch.float32).reshape(B, 3, 3)).to(dev)
        out = ops.inverse_warp(src_imgs, src_depths, tgt_depth, src_intrinsics.reshape(B * N, 3, 3), Kinv,
                               T_tgt2srcs.reshape(B * N, 4, 4))
        return out.cpu().numpy()[0] if as_numpy else out[0]

    # ---------------------------------------------------------------- the step
    @torch.no_grad()
    def one_step_prediction(self, tgt_pose_grid_coord, save_res_to_disk=True, keep_results=False):
        """reference :860-926.  ALIASING (differs from the reference, which returns fresh tensors): `x`,
        `extrapolation_mask`, `warped_depth` are views of this scene's persistent model-input buffers and `rgbd` /
        `feature` / `pre_quantized_features` are the static outputs of the captured HIP graph — the NEXT step overwrites
        them in place.  The frame store (`self.frames`) always holds its own tensors.  A caller that keeps a result
        dictionary across steps passes keep_results=True (six device copies per step) or clones what it keeps."""
        src_coords, _ = self.get_src_grid_coords(tgt_pose_grid_coord)
        if not src_coords:       # the reference dies in np.stack([]) here (:596); e.g. the GoogleEarth spiral: poses 0.7 apart, radius 0.3
            raise ValueError(f"no visited pose within the source radius of {tuple(tgt_pose_grid_coord)}: nothing to warp from")
        missing = [c for c in src_coords if c not in self.frames]
        if missing:          # (a 'trajectory' run started without the frame of the pose behind its first target)
            raise ValueError(f"source pose(s) {missing} of target {tuple(tgt_pose_grid_coord)} hold no frame: nothing to warp from")
        tgt_meta = self.transform_grid[tgt_pose_grid_coord[0]][tgt_pose_grid_coord[1]]
        src_metas = [self.transform_grid[c[0]][c[1]] for c in src_coords]
        batch = self.prepare_batch_data(tgt_meta, src_metas, self.num_src)
        depths = batch["_src_list"][1]
        batch.lazy("src_depths", lambda: torch.stack(depths)[None][..., None])             # (1,N,H,W,1) like :868
        if self._x_dst is not None:
            batch["_x_dst"] = self._x_dst
        x, x_dst, extrapolation_mask, warped_depth = self.dynamic_model.get_x(
            batch, self.data, return_extrapolation_mask=True, no_depth_range=True, parallel=True)
        self._x_dst = x_dst
        if self.infill_sampler == "device":      # this frame's draws: a function of (infill_seed, seed_index, frame index)
            self.dynamic_model.infill_call = self.curr
            self.dynamic_model.infill_streams = (self.seed_index,)
        x_sample_dets, _, pre_q, quant = self.dynamic_model(
            x, topk=self.topk, extrapolation_mask=extrapolation_mask, get_pre_quantized_feature=True,
            get_quantized_feature=True, sample_number=1)
        x_sample_det = x_sample_dets[0][0]                      # (B,4,H,W); sample number is 1
        rgb_f, depth, rgb_u8 = ops.frame_feedback(x_sample_det, self.data, want_u8=True)
        if save_res_to_disk:  # name kept from the reference; here "disk" is the in-HBM frame store
            self.save_to_store(tgt_pose_grid_coord, rgb_u8[0], rgb_f[0], depth[0])
        own = (lambda t: t.clone()) if keep_results else (lambda t: t)
        res = _Lazy({
            "rgbd": own(x_sample_dets[0].squeeze().detach()), "feature": own(quant.squeeze().detach()),
            "pre_quantized_features": own(pre_q.squeeze().detach()), "fixed": False, "x": own(x.detach()),
            "batch_R_rels": batch['R_rels'], "batch_t_rels": batch['t_rels'], "warped_depth": own(warped_depth),
            "extrapolation_mask": own(extrapolation_mask), "src_coords": src_coords,
        })
        res.lazy("batch_src_imgs", lambda: batch['src_imgs'])          # stacked copies only if the caller reads them
        res.lazy("batch_src_depths", lambda: batch['src_depths'])
        return res

    def save_to_store(self, coord, rgb_u8, rgb_f, depth):
        if coord in self.frames and any(coord in coords for coords in getattr(self, "_tsdf_log", ())):
            self.__dict__.setdefault("_tsdf_log_stale", []).append(coord)      # a fused source is overwritten: see render_views
        self.frames[coord] = {"rgb_u8": rgb_u8, "rgb_f": rgb_f, "depth": depth, "index": self.curr}
        self.transform_grid[coord[0]][coord[1]]["visited"] = True

    def _range_checkpoint(self, verified_curr):
        """split-fp32 range guard at a synchronisation point of the loop: when a kernel reported a non-finite output since
        the last checkpoint, the frames generated since then are dropped, the process switches to the fp32-in MFMA path
        (no range precondition) and the loop resumes from the last verified frame.  Returns the new `curr`."""
        if not (self.device.type == "cuda" and ops.F32_MODE == "split" and ops.f32x_range_tripped()):
            return self.curr
        import warnings
        warnings.warn(f"sgam split-fp32 path: an activation left fp16's range; regenerating frames {verified_curr}.."
                      f"{self.curr - 1} on the fp32-in MFMA path (SGAM_F32_MODE -> 'mfma')", RuntimeWarning)
        ops.set_f32_mode("mfma")
        self.dynamic_model._graphs = {}
        return self._rewind_to(verified_curr)

    def _rewind_to(self, verified_curr):
        """drop the frames generated since `verified_curr` (they may hold non-finite values); returns the new `curr`"""
        for c in self._ordered_grid_coords[verified_curr:self.curr]:
            self.frames.pop(c, None)
            self.transform_grid[c[0]][c[1]]["visited"] = False
        if self.volume is not None:            # the fused volume saw the invalid frames: start it again (every step
            self.volume = self._make_volume()  # re-integrates its own sources, :757-790)
            self._tsdf_log = []
            self._tsdf_log_stale = []
        return verified_curr

    def scene_expansion(self, return_hs=False, range_check_every=8):
        total = self.output_dim[0] * self.output_dim[1]
        if self.device.type == "cuda":
            ops.range_flag(self.device)
        verified = self.curr
        while self.curr < total:
            self.one_step_prediction(self.next_pose(self.curr))
            self.curr += 1
            if self.curr == total or (self.curr - verified) >= range_check_every:
                self.curr = self._range_checkpoint(verified)
                verified = self.curr
                if self.volume is not None:
                    self.volume.check()            # pool overflow / samples outside the box: do not lose geometry silently
        return self.frames

    # ---------------------------------------------------------------- export (after the run)
    def export_to_disk(self, out_dir):
        """Write im_XXXXX_ii_jj.png / dm_*.npy / R_*.npy / t_*.npy like the reference's save_to_disk (:928-942)."""
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
        for (i, j), fr in self.frames.items():
            suffix = f"_{i:02d}_{j:02d}"
            node = self.transform_grid[i][j]
            np.save(os.path.join(out_dir, f"R_{fr['index']:05d}{suffix}.npy"), node["R"])
            np.save(os.path.join(out_dir, f"t_{fr['index']:05d}{suffix}.npy"), node["t"])
            np.save(os.path.join(out_dir, f"dm_{fr['index']:05d}{suffix}.npy"), fr["depth"].cpu().numpy())
            Image.fromarray(fr["rgb_u8"].cpu().numpy()).save(os.path.join(out_dir, f"im_{fr['index']:05d}{suffix}.png"))
        return self.export_point_clouds(out_dir)


    def export_point_clouds(self, out_dir, clean=None, segment=None):
        """the two artefacts the reference's scene_expansion leaves behind the frames (inference_pipeline.py:441-450):
        `merged_pcds.ply` — every stored frame unprojected with its own depth, colour and pose, merged in the order of the
        frame index (the reference globs its R_<index>_*.npy files sorted: the same order) — and, on the rgbd_integration
        branch, `rgbd_integrated_mesh.ply` — the zero-crossing points of the fused volume (extracted on the device).  `clean`: a
        dict of merged_point_cloud's clean-up arguments (voxel_size, nb_neighbors, std_ratio, normals, normal_k); when given,
        `merged_pcds_clean.ply` — the device cloud after that clean-up, with normals when asked — is written as well
        (`merged_pcds.ply` keeps its host path and its bytes).  `segment`: a dict of segment()'s arguments; when given,
        `merged_pcds_segmented.ply` — segment()'s points coloured by label from geometry.SEGMENT_PALETTE, planes grey, noise
        black — is written as well.  Returns {file name: number of points}."""
        from . import pointcloud
        os.makedirs(out_dir, exist_ok=True)
        pts, cols = [], []
        for (i, j), fr in sorted(self.frames.items(), key=lambda kv: (kv[1]["index"], kv[0])):
            node = self.transform_grid[i][j]
            Rt = np.eye(4)
            Rt[:3, :3], Rt[:3, 3] = node["R"], np.asarray(node["t"]).reshape(3)
            p, c = pointcloud.unproject_frame(fr["depth"].cpu().numpy(), fr["rgb_u8"].cpu().numpy(), self.K, Rt)
            pts.append(p)
            cols.append(c)
        out = {"merged_pcds.ply": pointcloud.write_ply(os.path.join(out_dir, "merged_pcds.ply"), np.concatenate(pts), np.concatenate(cols))}
        if clean is not None:
            unknown = sorted(set(clean) - {"voxel_size", "nb_neighbors", "std_ratio", "normals", "normal_k"})
            if unknown:
                raise ValueError(f"export_point_clouds: clean does not take {unknown}")
            pc = self.merged_point_cloud(**clean)
            valid = torch.isfinite(pc["points"]).all(dim=1)              # (an empty `clean`: the raw cloud, NaN points left out)
            nrm = pc["normals"][valid].cpu().numpy() if "normals" in pc else None
            out["merged_pcds_clean.ply"] = pointcloud.write_ply(os.path.join(out_dir, "merged_pcds_clean.ply"), pc["points"][valid].cpu().numpy(),
                                                                pc["colors"][valid].cpu().numpy().astype(np.float64) / 255.0, nrm)
        if segment is not None:
            from . import geometry
            seg = self.segment(**segment)
            valid = torch.isfinite(seg["points"]).all(dim=1)
            paint = geometry.segment_colors(seg["plane_labels"], seg["cluster_labels"])
            out["merged_pcds_segmented.ply"] = pointcloud.write_ply(os.path.join(out_dir, "merged_pcds_segmented.ply"),
                                                                    seg["points"][valid].cpu().numpy(),
                                                                    paint[valid].cpu().numpy().astype(np.float64) / 255.0)
        if self.use_rgbd_integration and self.volume is not None:
            pc = self.colour_volume().extract_point_cloud()
            out["rgbd_integrated_mesh.ply"] = pointcloud.write_ply(os.path.join(out_dir, "rgbd_integrated_mesh.ply"), pc["points"],
                                                                   pc.get("colors"), pc["normals"])
        return out

    def _clean_arguments(self, clean, what):
        from . import meshops
        unknown = sorted(set(clean) - set(meshops.CLEAN_KEYS))
        if unknown:
            raise ValueError(f"{what}: clean does not take {unknown}")
        return dict(clean)

    def clean_triangle_mesh(self, volume=None, **clean):
        """meshops.clean (small components removed, Taubin smoothing, vertex clustering, normals — min_triangles,
        keep_largest, smooth_iterations, voxel_size, normals) of the marching-cubes mesh of the run's colour volume, on the device.
        volume: a colour_volume() the caller holds already.  Returns {"mesh": tsdf.DeviceMesh (colours 0..255), "vertex_normals"
        (nv,3) fp32 or None, "vertex_index" (nv,) int32 into the extracted mesh's vertices}.  rgbd_integration branch only."""
        from . import meshops
        if not (self.use_rgbd_integration and self.volume is not None):
            raise ValueError("clean_triangle_mesh: the scene was not run on the rgbd_integration branch")
        clean = self._clean_arguments(clean, "clean_triangle_mesh")
        vol = self.colour_volume() if volume is None else volume
        return meshops.clean(vol.extract_mesh_device(), **clean)

    def _simplify_arguments(self, simplify, what):
        from . import meshops
        unknown = sorted(set(simplify) - set(meshops.SIMPLIFY_KEYS))
        if unknown:
            raise ValueError(f"{what}: simplify does not take {unknown}")
        return dict(simplify)

    def simplify_triangle_mesh(self, volume=None, clean=None, **simplify):
        """meshops.simplify_quadric_decimation (quadric-error edge collapses — target_triangles or target_ratio,
        max_error, boundary_weight, oversample, max_rounds) of the marching-cubes mesh of the run's colour volume, on the device,
        after clean_triangle_mesh's clean-up when `clean` (a dict of its arguments) is given.  Returns the decimation's dict
        with "vertex_normals" (nv,3) fp32 (meshops.vertex_normals of the result) and "vertex_index" into the extracted mesh's
        vertices.  rgbd_integration branch only."""
        from . import meshops
        if not (self.use_rgbd_integration and self.volume is not None):
            raise ValueError("simplify_triangle_mesh: the scene was not run on the rgbd_integration branch")
        simplify = self._simplify_arguments(simplify, "simplify_triangle_mesh")
        if clean is not None:
            clean = self._clean_arguments(clean, "simplify_triangle_mesh")
        vol = self.colour_volume() if volume is None else volume
        return self._simplified(vol.extract_mesh_device(), clean, simplify)

    @staticmethod
    def _simplified(mesh, clean, simplify):
        """the mesh cleaned (when asked) and decimated: simplify_quadric_decimation's dict with the result's normals"""
        from . import meshops
        index = None
        if clean is not None:
            c = meshops.clean(mesh, **dict(clean, normals=False))
            mesh, index = c["mesh"], c["vertex_index"]
        out = meshops.simplify_quadric_decimation(mesh, **simplify)
        if index is not None:
            out["vertex_index"] = index[out["vertex_index"].long()]
        out["vertex_normals"] = meshops.vertex_normals(out["mesh"])
        return out

    @staticmethod
    def _write_device_mesh(path, mesh, normals):
        from . import pointcloud
        col = None if mesh.vertex_colors is None else (mesh.vertex_colors / 255.0).cpu().numpy()
        return pointcloud.write_triangle_mesh(path, mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), col,
                                              None if normals is None else normals.cpu().numpy())

    def export_triangle_mesh(self, out_dir, clean=None, simplify=None):
        """`rgbd_integrated_triangle_mesh.ply`: the marching-cubes mesh of the run's colour volume (colour_volume(): the logged
        integrations replayed with RGB8 colour) with vertex colours and normals, in Open3D's binary mesh PLY layout.  Returns the
        number of triangles.  `clean`: a dict of clean_triangle_mesh's arguments; when given,
        `rgbd_integrated_triangle_mesh_clean.ply` — that mesh after the device clean-up — is written as well (the first file keeps
        its bytes) and {file name: number of triangles} is returned.  `simplify`: a dict of simplify_triangle_mesh's arguments;
        when given, `rgbd_integrated_triangle_mesh_simplified.ply` — the (cleaned, when `clean` is given too) mesh after
        quadric-error decimation, with its own normals — is written as well, and the dict is returned."""
        from . import pointcloud
        if not (self.use_rgbd_integration and self.volume is not None):
            raise ValueError("export_triangle_mesh: the scene was not run on the rgbd_integration branch")
        if clean is not None:
            clean = self._clean_arguments(clean, "export_triangle_mesh")
        if simplify is not None:
            simplify = self._simplify_arguments(simplify, "export_triangle_mesh")
        os.makedirs(out_dir, exist_ok=True)
        vol = self.colour_volume()
        mesh = vol.extract_triangle_mesh()
        n = pointcloud.write_triangle_mesh(os.path.join(out_dir, "rgbd_integrated_triangle_mesh.ply"), mesh["vertices"],
                                           mesh["triangles"], mesh.get("vertex_colors"), mesh["vertex_normals"])
        if clean is None and simplify is None:
            return n
        out = {"rgbd_integrated_triangle_mesh.ply": n}
        if clean is not None:
            c = self.clean_triangle_mesh(volume=vol, **clean)
            name = "rgbd_integrated_triangle_mesh_clean.ply"
            out[name] = self._write_device_mesh(os.path.join(out_dir, name), c["mesh"], c["vertex_normals"])
        if simplify is not None:
            d = self.simplify_triangle_mesh(volume=vol, clean=clean, **simplify)
            name = "rgbd_integrated_triangle_mesh_simplified.ply"
            out[name] = self._write_device_mesh(os.path.join(out_dir, name), d["mesh"], d["vertex_normals"])
        return out


    # ---------------------------------------------------------------- views of the finished scene
    def flythrough_poses(self, n_between=4, order=None):
        """World -> camera 4x4s (float64, (P,4,4)) along the run's visiting order (or along `order`, a list of grid
        coordinates): every node's own T, and between consecutive nodes n_between interpolated poses — the camera centre linear,
        the rotation by quaternion slerp.  P = (nodes - 1) * (n_between + 1) + 1.  Pure numpy."""
        if order is None:
            order = [c for c in self._ordered_grid_coords if self.transform_grid[c[0]][c[1]]["visited"]]
        nodes = [self.transform_grid[c[0]][c[1]] for c in order]
        if not nodes:
            raise ValueError("flythrough_poses: no poses to visit")
        poses = [nodes[0]["T"].copy()]
        for a, b in zip(nodes[:-1], nodes[1:]):
            qa, qb = _quat_from_rot(a["T"][:3, :3]), _quat_from_rot(b["T"][:3, :3])
            ca, cb = -a["T"][:3, :3].T @ a["T"][:3, 3], -b["T"][:3, :3].T @ b["T"][:3, 3]
            for k in range(1, n_between + 1):
                s = k / (n_between + 1)
                R = _rot_from_quat(_slerp(qa, qb, s))
                T = np.eye(4)
                T[:3, :3], T[:3, 3] = R, -R @ ((1 - s) * ca + s * cb)
                poses.append(T)
            poses.append(b["T"].copy())
        return np.stack(poses)

    def render_views(self, poses, source="mesh", out_dir=None, H=None, W=None, point_radius=0, hole_fill=True, frames=None, mesh_clean=None,
                     mesh_simplify=None):
        """RGB-D views of the finished scene at `poses` (P world -> camera 4x4s, e.g. flythrough_poses()): the run's colour volume
        (colour_volume(): the logged integrations replayed with RGB8 colour, its pool sized to the loop volume's brick count,
        checked after the replay), its marching-cubes mesh extracted once, all poses in one coloured mesh render
        (tsdf.render_mesh_rgbd).  source="raycast": the same poses through the ray cast's nearest-voxel colour, one pose per
        call — a comparison path.  Both need the rgbd_integration branch and its log.  source="points" needs neither and works
        on either branch: the frame store itself, every stored frame unprojected, moved into the view camera and splatted with
        a z-test at all poses in one call (pointview.render_points_rgbd) — frames in export_point_clouds' order (frame index, then
        coordinate: an exact z tie goes to the earlier frame), or only those at the grid coordinates `frames`; point_radius 0..2:
        a (2 r + 1)^2 footprint per point; hole_fill: the conditioning's 3x3 median fill of the samples nothing landed on.
        mesh_clean (source="mesh" only): a dict of clean_triangle_mesh's arguments — the mesh is cleaned on the device (DESIGN
        §4.4.7) before it is rendered.  mesh_simplify (source="mesh" only): a dict of simplify_triangle_mesh's arguments — the
        (cleaned) mesh is decimated on the device before it is rendered.
        Returns device tensors {"rgb" (P,H,W,3) fp32 0..255, "depth" (P,H,W) fp32, "rgb_u8" (P,H,W,3) uint8}; with out_dir also
        view_%04d.png (RGB8) and view_depth_%04d.npy per pose."""
        from . import tsdf
        if source not in ("mesh", "raycast", "points"):
            raise ValueError(f"render_views: source 'mesh', 'raycast' or 'points', not {source!r}")
        if mesh_clean is not None:
            if source != "mesh":
                raise ValueError("render_views: mesh_clean belongs to source='mesh'")
            mesh_clean = self._clean_arguments(mesh_clean, "render_views")
        if mesh_simplify is not None:
            if source != "mesh":
                raise ValueError("render_views: mesh_simplify belongs to source='mesh'")
            mesh_simplify = self._simplify_arguments(mesh_simplify, "render_views")
        if source != "points":
            if not (self.use_rgbd_integration and self.volume is not None):
                raise ValueError("render_views: the scene was not run on the rgbd_integration branch")
            stale = getattr(self, "_tsdf_log_stale", None)
            if stale:
                raise ValueError(f"render_views: the frames at {sorted(set(stale))} were fused as sources and overwritten "
                                 "later; replaying the logged integrations would fuse the new frames, not the ones the run fused")
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        H = self.image_resolution[0] if H is None else int(H)
        W = self.image_resolution[1] if W is None else int(W)
        K = self.K
        if (H, W) != tuple(self.image_resolution):                  # the same field of view at another size
            K = np.diag([W / self.image_resolution[1], H / self.image_resolution[0], 1.0]) @ self.K
        z0, z1 = self._Z_RANGE[self.data]
        if source == "points":
            from . import pointview
            coords = [c for c, _ in sorted(self.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
            if frames is not None:
                keep = {tuple(c) for c in frames}
                missing = sorted(keep - set(coords))
                if missing:
                    raise ValueError(f"render_views: no stored frame at {missing}")
                coords = [c for c in coords if c in keep]
            if not coords:
                raise ValueError("render_views: no stored frames to render")
            out = pointview.render_points_rgbd(
                [self.frames[c]["depth"] for c in coords], [self.frames[c]["rgb_u8"] for c in coords], self.K,
                [self.transform_grid[c[0]][c[1]]["T"] for c in coords], K, poses, H, W, z0, z1, radius=point_radius, hole_fill=hole_fill)
        else:
            vol = self.colour_volume(max_bricks=max(1, self.volume.stats()[0]))
            vol.check()
        if source == "mesh":
            mesh = vol.extract_mesh_device()
            if mesh_clean is not None:
                from . import meshops
                mesh = meshops.clean(mesh, **dict(mesh_clean, normals=False))["mesh"]
                if mesh.n_triangles == 0:
                    raise ValueError("render_views: mesh_clean left no triangle to render")
            if mesh_simplify is not None:
                from . import meshops
                mesh = meshops.simplify_quadric_decimation(mesh, **mesh_simplify)["mesh"]
                if mesh.n_triangles == 0:
                    raise ValueError("render_views: mesh_simplify left no triangle to render")
            out = tsdf.render_mesh_rgbd(mesh, K, poses, H, W, z0, z1, u8=True)
        elif source == "raycast":
            out = {"depth": torch.empty((len(poses), H, W), dtype=torch.float32, device=self.device),
                   "rgb": torch.empty((len(poses), H, W, 3), dtype=torch.float32, device=self.device)}
            for p, T in enumerate(poses):
                out["rgb"][p] = vol.render_depth(K, T, H, W, z0, z1, want_color=True, out=out["depth"][p])[1]
            out["rgb_u8"] = out["rgb"].clamp(0, 255).to(torch.uint8)
        if out_dir is not None:
            from PIL import Image
            os.makedirs(out_dir, exist_ok=True)
            u8, depth = out["rgb_u8"].cpu().numpy(), out["depth"].cpu().numpy()
            for p in range(len(poses)):
                Image.fromarray(u8[p]).save(os.path.join(out_dir, f"view_{p:04d}.png"))
                np.save(os.path.join(out_dir, f"view_depth_{p:04d}.npy"), depth[p])
        return out

    # ---------------------------------------------------------------- geometry of the finished scene
    def _stored_coords(self, frames, what):
        """grid coordinates of the stored frames in export_point_clouds' order (frame index, then coordinate), or those of `frames`"""
        coords = [c for c, _ in sorted(self.frames.items(), key=lambda kv: (kv[1]["index"], kv[0]))]
        if frames is not None:
            keep = {tuple(c) for c in frames}
            missing = sorted(keep - set(coords))
            if missing:
                raise ValueError(f"{what}: no stored frame at {missing}")
            coords = [c for c in coords if c in keep]
        if not coords:
            raise ValueError(f"{what}: no stored frames")
        return coords

    def _corrected_poses(self, coords, pose_corrections, what):
        """the world -> camera poses of the stored frames at `coords`; with pose_corrections — optimize_poses' result, or a dict
        {coord: 4x4 world-frame correction C} — the frames it names get T C^-1 (float64): their points come out moved by C"""
        Ts = [self.transform_grid[c[0]][c[1]]["T"] for c in coords]
        if pose_corrections is None:
            return Ts
        if not isinstance(pose_corrections, dict):
            raise ValueError(f"{what}: pose_corrections is optimize_poses' result or a dict {{coord: 4x4}}, not {type(pose_corrections).__name__}")
        if "corrections" in pose_corrections and "coords" in pose_corrections:
            C = pose_corrections["corrections"]
            C = np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
            pose_corrections = {tuple(c): C[i] for i, c in enumerate(pose_corrections["coords"])}
        fixes = {}
        for c, C in pose_corrections.items():
            C = np.asarray(C.detach().cpu() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
            if C.shape != (4, 4) or not np.isfinite(C).all():
                raise ValueError(f"{what}: the pose correction of frame {c} is a finite 4x4")
            fixes[tuple(c)] = C
        return [np.asarray(T, dtype=np.float64) @ np.linalg.inv(fixes[c]) if c in fixes else T for c, T in zip(coords, Ts)]

    def merged_point_cloud(self, frames=None, voxel_size=None, nb_neighbors=None, std_ratio=2.0, normals=False, normal_k=16,
                           pose_corrections=None):
        """The frame store as ONE coloured cloud on the device (geometry.unproject_frames: one launch, the frames read where the
        store keeps them): {"points" (F*H*W,3) fp32 world coordinates, "colors" (F*H*W,3) uint8}, the frames in
        export_point_clouds' order (frame index, then coordinate) or only those at the grid coordinates `frames`; works on either
        warp branch.  A pixel whose depth is not finite or outside the dataset's z range is a NaN point (nothing is compacted).
        `merged_pcds.ply` itself stays the host export's float64 bytes (export_point_clouds).

        With voxel_size, nb_neighbors or normals the cloud is cleaned on the device, in this order: the NaN points
        are dropped; geometry.voxel_sample keeps one real point per voxel of edge voxel_size; geometry.statistical_outliers
        (nb_neighbors, std_ratio) drops the outliers of what is left; geometry.estimate_normals (normal_k neighbours) gives what is
        left normals oriented towards the camera centre of the frame each point came from.  Returns {"points" (M,3), "colors" (M,3)
        uint8, "index" (M,) int32 into the uncompacted order above, "normals" (M,3) fp32 if asked}.

        pose_corrections: optimize_poses' result, or a dict {coord: 4x4}: the frames it names are unprojected with the corrected
        pose T C^-1, so their points come out moved by the world-frame correction C (the drift between the scene's own frames taken
        out); the store is not touched.  None: the stored poses."""
        from . import geometry
        coords = self._stored_coords(frames, "merged_point_cloud")
        z0, z1 = self._Z_RANGE[self.data]
        Ts = self._corrected_poses(coords, pose_corrections, "merged_point_cloud")
        cloud = geometry.unproject_frames([self.frames[c]["depth"] for c in coords], [self.frames[c]["rgb_u8"] for c in coords], self.K,
                                          Ts, z0, z1)
        if voxel_size is None and nb_neighbors is None and not normals:
            return cloud
        pts, cols = cloud["points"], cloud["colors"]
        if not bool(torch.isfinite(pts).all(dim=1).any()):                 # no point at all: an empty cloud, not a refusal
            pts = pts[:0]
            points, index, nrm = pts, torch.zeros((0,), dtype=torch.int64, device=pts.device), pts
        else:
            centres, view_of = self._frame_viewpoints(frames) if normals else (None, None)
            points, index, nrm = geometry.prepare_cloud(pts, "merged_point_cloud", voxel_size,
                                                        None if nb_neighbors is None else (nb_neighbors, std_ratio),
                                                        normal_k if normals else None, centres, view_of)
        out = {"points": points, "colors": cols[index].contiguous(), "index": index.to(torch.int32)}
        if normals:
            out["normals"] = nrm
        return out

    def segment(self, plane_threshold, eps, min_points, max_planes=1, min_plane_inliers=None, voxel_size=None, frames=None,
                pose_corrections=None, num_iterations=1000, seed=0):
        """What is IN the scene (geometry.segment_cloud on merged_point_cloud(frames=, voxel_size=, pose_corrections=), either warp
        branch): up to max_planes planes by RANSAC (inlier distance plane_threshold; a plane needs
        min_plane_inliers points, default 3), then DBSCAN (eps, min_points) over what no plane took.  Returns {"points" (N,3),
        "colors" (N,3) uint8, "plane_labels" (N,) int32 (-1: no plane), "planes" (max_planes,4) least-squares planes (NaN: none),
        "plane_counts" (max_planes,) int32, "plane_ratio": plane inliers / valid points, "cluster_labels" (N,) int32 (-1: noise or
        on a plane), "n_clusters": an int (the one host read), "cluster_sizes" (n_clusters,) int32, "cluster_boxes": {"count",
        "lo", "hi"} of geometry.cluster_boxes}; tensors on the device."""
        from . import geometry
        pc = self.merged_point_cloud(frames, voxel_size=voxel_size, pose_corrections=pose_corrections)
        pts = pc["points"]
        if pts.shape[0] < 1:
            raise ValueError("segment: the scene's cloud has no points")
        seg = geometry.segment_cloud(pts, plane_threshold, eps, min_points, max_planes=max_planes,
                                     min_plane_inliers=3 if min_plane_inliers is None else min_plane_inliers,
                                     num_iterations=num_iterations, seed=seed)
        host = torch.stack([seg["n_clusters"].to(torch.int64), seg["plane_counts"].sum().to(torch.int64),
                            torch.isfinite(pts).all(dim=1).sum(), seg["flag"][0].to(torch.int64)]).cpu().numpy()
        if host[3]:
            raise ops.SgamHipError("segment: a union-find loop of the clustering reached its bound")
        n_clusters = int(host[0])
        return {"points": pts, "colors": pc["colors"], "plane_labels": seg["plane_labels"], "planes": seg["planes"],
                "plane_counts": seg["plane_counts"], "plane_ratio": float(host[1]) / float(host[2]) if host[2] else 0.0,
                "cluster_labels": seg["cluster_labels"], "n_clusters": n_clusters, "cluster_sizes": seg["sizes"][:n_clusters],
                "cluster_boxes": geometry.cluster_boxes(pts, seg["cluster_labels"], n_clusters)}

    def fid(self, reference, frames=None, dims=2048, inception=None, method="auto"):
        """Fréchet Inception distance (sgam_neurips22_amd/fid.py) between the RGB of the stored frames (all of them, or those at the
        grid coordinates `frames`; read where the store keeps them, on either warp branch) and `reference`: a (M,H,W,3) uint8
        tensor, another scene (its stored frames), a directory of images or a .npz of statistics (`mu`, `sigma`).  `inception`:
        an `InceptionV3` to use (default: the FID checkpoint, which must be on disk).  method "auto" takes the exact low-rank
        route when both sides are sets of frames with N1 * N2 small, the reference's sqrtm route otherwise ("lowrank" / "sqrtm"
        force one).  Only the features' small final factorisation runs on the host."""
        from . import fid as F
        mine = torch.stack([self.frames[c]["rgb_u8"] for c in self._stored_coords(frames, "fid")])
        if isinstance(reference, InfiniteSceneGeneration):
            reference = torch.stack([reference.frames[c]["rgb_u8"] for c in reference._stored_coords(None, "fid")])
        if inception is None:
            inception = F.InceptionV3([F.InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(self.device)
        return F.fid_between(mine, reference, inception, dims=dims, method=method, device=self.device)

    def _feature_metric_inputs(self, frames, dims, inception, what):
        """the scene's side of a feature-set metric as scene.fid resolves it: (stored frames (N,H,W,3) uint8, the InceptionV3)"""
        from . import fid as F
        mine = torch.stack([self.frames[c]["rgb_u8"] for c in self._stored_coords(frames, what)])
        if inception is None:
            inception = F.InceptionV3([F.InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(self.device)
        return mine, inception

    def kid(self, reference, frames=None, dims=2048, inception=None, subsets=100, subset_size=None, seed=0):
        """Kernel inception distance (sgam_neurips22_amd/feature_metrics.py) between the stored frames and `reference` (a (M,H,W,3)
        uint8 tensor, another scene or a directory of images; saved statistics do not carry the features it needs): the unbiased
        polynomial-kernel MMD^2 over `subsets` subsets of `subset_size` frames per side (default min(N1, N2, 1000)), whose
        expectation does not depend on the number of frames.  Returns {"kid", "kid_std", "values", "subsets", "subset_size"}."""
        from . import feature_metrics as FM
        mine, inception = self._feature_metric_inputs(frames, dims, inception, "kid")
        return FM.kid_between(mine, reference, inception, dims=dims, subsets=subsets, subset_size=subset_size, seed=seed,
                              device=self.device)

    def sample_quality(self, reference, frames=None, dims=2048, inception=None, k=3):
        """Improved precision / recall and density / coverage of the stored frames (the generated side) against `reference` (the
        real side; kinds as in `kid`), from k-th-neighbour balls in Inception feature space: fidelity (precision, density) apart
        from diversity (recall, coverage).  Returns {"precision", "recall", "density", "coverage", "k"}."""
        from . import feature_metrics as FM
        mine, inception = self._feature_metric_inputs(frames, dims, inception, "sample_quality")
        return FM.prdc_between(reference, mine, inception, dims=dims, k=k, device=self.device)

    def _metric_mesh(self, mesh_clean, mesh_simplify, what):
        """the run's marching-cubes mesh, cleaned and / or decimated as asked (no normals)"""
        if mesh_simplify is None:
            return self.clean_triangle_mesh(**dict(mesh_clean or {}, normals=False))["mesh"]
        return self.simplify_triangle_mesh(clean=mesh_clean, **self._simplify_arguments(mesh_simplify, what))["mesh"]

    def _metric_points(self, frames, source, mesh_clean, what, pose_corrections=None, mesh_simplify=None):
        """the scene's geometry as an (N,3) fp32 device cloud: the frame store's merged cloud, or the vertices of the (cleaned) mesh"""
        if source not in ("frames", "mesh"):
            raise ValueError(f"{what}: source 'frames' or 'mesh', not {source!r}")
        if source == "frames":
            if mesh_clean is not None or mesh_simplify is not None:
                raise ValueError(f"{what}: mesh_clean and mesh_simplify belong to source='mesh'")
            return self.merged_point_cloud(frames, pose_corrections=pose_corrections)["points"]
        if pose_corrections is not None:
            raise ValueError(f"{what}: pose_corrections belongs to source='frames' (the mesh was fused with the stored poses)")
        if frames is not None:
            raise ValueError(f"{what}: frames belongs to source='frames' (the mesh is the fusion of the whole run)")
        pts = self._metric_mesh(mesh_clean, mesh_simplify, what).vertices
        if pts.shape[0] < 1:
            raise ValueError(f"{what}: the mesh has no vertices")
        return pts

    def geometry_metrics(self, reference, threshold, frames=None, max_distance=None, voxel_size=None, align=None, source="frames",
                         mesh_clean=None, surface_samples=None, visible_from=None, accelerator="grid", pose_corrections=None,
                         mesh_simplify=None):
        """geometry.cloud_metrics of the merged cloud (of `frames`) against a reference geometry: an (M,3) fp32 device tensor,
        another scene (its merged cloud), or ground-truth frames {"depths": F device tensors (H,W) fp32, "Ts_w2c": (F,4,4), "K":
        3x3} unprojected the same way over this dataset's z range.  Returns chamfer, accuracy (scene -> reference), completeness
        (reference -> scene), precision / recall / fscore at `threshold`, n_pred, n_ref.  voxel_size: both clouds are first
        resampled on one shared voxel grid (geometry.cloud_metrics), so the scores do not depend on how many frames overlap.

        align: a dict {max_correspondence_distance (required), estimation="point_to_plane", max_iterations=30, normal_k=16,
        voxel_size=None}: the scene's cloud is first registered onto the reference (geometry.register_icp) — on the
        clouds without their NaN points, voxel-sampled at align's voxel_size for the registration only, the reference's normals
        from geometry.estimate_normals(k=normal_k) for point-to-plane — then the WHOLE cloud is moved by the result and scored as
        above, so that a rigid offset between the two frames of reference does not count as surface error.  The dict returned
        gains "transformation" ((4,4) fp64 device tensor, scene -> reference) and "alignment" (fitness, inlier_rmse, iterations,
        converged).  estimation="colored" (with lambda_geometric=0.968, gradient_k=16 in the dict; coloured ICP, for scenes whose
        geometry leaves the pose free) also reads both sides' colours: the scene's own, and the reference's — another scene's, or
        ground-truth frames given with "rgbs" (F device tensors (H,W,3) uint8); a reference without colours, and source="mesh",
        raise ValueError.  With "init": "global" and "global": {"voxel_size": v, ...} in the dict (the other keys are
        geometry.register_global's arguments) the two clouds need share no frame of reference: register_global (FPFH features,
        RANSAC, ICP on the sampled clouds) runs first and the registration above starts from its pose; "alignment" gains
        "global": that stage's fitness, inlier_rmse, correspondences, hypothesis, inliers, valid_hypotheses and transformation.
        Its normals are oriented towards the camera centres where the side is a frame store (this scene with source="frames",
        a reference that is a scene or ground-truth frames); for a reference given as a tensor pass "target_viewpoints" in
        "global".  Without "init" nothing changes.

        source="mesh" (rgbd_integration branch): the vertices of the run's marching-cubes mesh — cleaned by clean_triangle_mesh's
        arguments in the dict mesh_clean when given — are scored instead of the frame store's cloud, in which every overlap counts
        many times.  A reference that is a scene is taken the same way; voxel_size and align work as before.  The vertices of a
        raw marching-cubes mesh are spaced at the voxel scale, but a vertex set is not the surface: after mesh_clean's vertex
        clustering they are as sparse as the caller asked, and the distance to the nearest VERTEX is up to half an edge too large.

        surface_samples=n (source="mesh"): the (cleaned) mesh is scored as a SURFACE through meshops.surface_metrics (DESIGN
        §4.4.8): n area-uniform samples of it against the reference, and the reference's points against its triangles.  A
        reference that is a scene is its mesh surface too, and a tsdf.DeviceMesh (a ground-truth mesh) is accepted — only here;
        tensors and ground-truth frames stay clouds.  align registers the scene's surface samples onto the reference (its samples
        if it is a mesh), then the mesh's vertices are moved by the result (geometry.transform_points) before scoring.  voxel_size
        does not go with surface_samples: resampling is what the surface sampling replaces.

        visible_from (with surface_samples, and a reference that is a surface: a DeviceMesh or a scene): "frames" — the poses of
        the stored frames — or a (P,4,4) array of world -> camera poses in this scene's frame of reference, at this scene's
        intrinsics and frame resolution over the dataset's z range.  The reference's n samples are culled to those some pose sees,
        the reference's own mesh being the occluder (meshops.visible_points): accuracy / precision are as before,
        completeness / recall run over the visible samples only, n_ref counts them and the dict gains "n_ref_culled".  With align
        the poses are moved into the reference's frame by the inverse of the registration (pose @ inverse(transformation)) before
        the culling, which therefore happens in the reference's frame, after the registration.

        accelerator (with surface_samples) "grid" | "bvh": the structure the distances to a mesh and the visibility culling go
        through (meshops.TriangleGrid or meshops.TriangleBVH, DESIGN §4.4.10: for a reference whose triangles are not near one
        scale); the numbers do not depend on it.

        pose_corrections (source="frames"): optimize_poses' result or a dict {coord: 4x4}; the scene's cloud is
        merged_point_cloud(frames, pose_corrections=...), the drift between its own frames taken out, where align removes only a
        rigid offset of the whole scene.  None: the stored poses.

        mesh_simplify (source="mesh"): a dict of simplify_triangle_mesh's arguments; the (cleaned) mesh — this scene's and a
        reference scene's — is decimated before it is scored."""
        from . import geometry, meshops
        from .tsdf import DeviceMesh
        meshops._accelerator(accelerator, "geometry_metrics")
        if pose_corrections is not None and (source != "frames" or surface_samples is not None):
            raise ValueError("geometry_metrics: pose_corrections belongs to source='frames' (the mesh was fused with the stored poses)")
        if align is not None and self._align_options(align)["estimation"] == "colored":     # (refused before anything is computed)
            if source != "frames":
                raise ValueError("geometry_metrics: estimation 'colored' needs source='frames' (the mesh is scored without colours)")
            if not isinstance(reference, InfiniteSceneGeneration) and not (isinstance(reference, dict) and reference.get("rgbs") is not None):
                raise ValueError("geometry_metrics: estimation 'colored' needs a reference with colours: another scene, or ground-truth "
                                 "frames given with 'rgbs'")
        if surface_samples is not None:
            return self._surface_geometry_metrics(reference, threshold, frames, max_distance, voxel_size, align, source, mesh_clean,
                                                  surface_samples, visible_from, accelerator, mesh_simplify)
        if visible_from is not None:
            raise ValueError("geometry_metrics: visible_from needs surface_samples (the reference's surface samples are what is culled)")
        if isinstance(reference, DeviceMesh):
            raise ValueError("geometry_metrics: a reference that is a mesh needs surface_samples")
        ref = self._reference_geometry(reference, lambda scene: scene._metric_points(None, source, mesh_clean, "geometry_metrics",
                                                                                     mesh_simplify=mesh_simplify), False)
        pred = self._metric_points(frames, source, mesh_clean, "geometry_metrics", pose_corrections, mesh_simplify)
        if align is None:
            return geometry.cloud_metrics(pred, ref, threshold, max_distance=max_distance, voxel_size=voxel_size)
        opts = self._align_options(align)
        if ref.dim() != 2 or pred.device != ref.device:
            raise ValueError("geometry_metrics: align needs an (M,3) reference cloud on the scene's device")
        colored = None
        if opts["estimation"] == "colored":
            colored = dict(source_colors=self.merged_point_cloud(frames)["colors"], target_colors=self._reference_colors(reference),
                           lambda_geometric=opts["lambda_geometric"], gradient_k=opts["gradient_k"])
        start = self._global_init(opts, pred, ref.contiguous(), self._frame_viewpoints(frames) if source == "frames" else None,
                                  self._reference_viewpoints(reference, source))
        reg = _register_clouds(pred, ref.contiguous(), None, opts["max_correspondence_distance"], opts["estimation"], opts["max_iterations"],
                               opts["normal_k"], opts["voxel_size"], "geometry_metrics", colored=colored,
                               init=None if start is None else start["transformation"])
        out = geometry.cloud_metrics(geometry.transform_points(pred, reg["transformation"]), ref, threshold, max_distance=max_distance,
                                     voxel_size=voxel_size)
        return self._with_alignment(out, reg, start)

    def _frame_viewpoints(self, frames):
        """(camera centres (F,3) fp32 on the device, view_of (F*H*W,) int32) of merged_point_cloud(frames)'s uncompacted cloud"""
        from . import geometry
        coords = self._stored_coords(frames, "geometry_metrics")
        hw = int(self.frames[coords[0]]["depth"].numel())
        centres = geometry.camera_to_world([self.transform_grid[c[0]][c[1]]["T"] for c in coords])[:, :, 3]
        view_of = torch.arange(len(coords) * hw, device=self.device) // hw
        return torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float32)).to(self.device), view_of.to(torch.int32)

    def _reference_viewpoints(self, reference, source):
        """the camera centres behind a `reference` argument of geometry_metrics where it is a frame store, else None"""
        from . import geometry
        if isinstance(reference, InfiniteSceneGeneration):
            return reference._frame_viewpoints(None) if source == "frames" else None
        if isinstance(reference, dict):
            hw = int(reference["depths"][0].numel())
            centres = geometry.camera_to_world(reference["Ts_w2c"])[:, :, 3]
            view_of = torch.arange(len(reference["depths"]) * hw, device=self.device) // hw
            return torch.from_numpy(np.ascontiguousarray(centres, dtype=np.float32)).to(self.device), view_of.to(torch.int32)
        return None

    @staticmethod
    def _global_init(opts, pred, ref, source_viewpoints, target_viewpoints):
        """align's "init": None (no stage before the ICP) or "global": geometry.register_global's dict"""
        from . import geometry
        if opts["init"] is None:
            if opts["global"] is not None:
                raise ValueError("geometry_metrics: align's 'global' belongs to 'init': 'global'")
            return None
        if opts["init"] != "global":
            raise ValueError(f"geometry_metrics: align's init is 'global' or absent, not {opts['init']!r}")
        g = dict(opts["global"] or {})
        if "voxel_size" not in g:
            raise ValueError("geometry_metrics: align's 'global' needs voxel_size")
        g.setdefault("source_viewpoints", source_viewpoints)
        g.setdefault("target_viewpoints", target_viewpoints)
        return geometry.register_global(pred, ref, **g)

    def _reference_geometry(self, reference, of_scene, surface):
        """the geometry a `reference` argument of geometry_metrics stands for: of_scene(reference) for another scene, ground-truth
        frames unprojected over this dataset's z range, a tensor as it is and, where the scene is scored as a surface, a DeviceMesh"""
        from . import geometry
        from .tsdf import DeviceMesh
        if isinstance(reference, InfiniteSceneGeneration):
            return of_scene(reference)
        if isinstance(reference, dict):
            z0, z1 = self._Z_RANGE[self.data]
            return geometry.unproject_frames(list(reference["depths"]), None, reference["K"], reference["Ts_w2c"], z0, z1)["points"]
        if isinstance(reference, torch.Tensor) or (surface and isinstance(reference, DeviceMesh)):
            return reference
        raise ValueError(f"geometry_metrics: the reference is an (M,3) device tensor, a scene{', a DeviceMesh' if surface else ''} or a dict of "
                         "ground-truth frames")

    def _reference_colors(self, reference):
        """the uint8 colours of a `reference` argument of geometry_metrics, aligned with _reference_geometry's points of the frame
        store: another scene's, or those of ground-truth frames given with "rgbs" (geometry_metrics has refused every other kind)"""
        from . import geometry
        if isinstance(reference, InfiniteSceneGeneration):
            return reference.merged_point_cloud()["colors"]
        z0, z1 = self._Z_RANGE[self.data]
        return geometry.unproject_frames(list(reference["depths"]), list(reference["rgbs"]), reference["K"], reference["Ts_w2c"], z0, z1)["colors"]

    @staticmethod
    def _with_alignment(out, reg, start=None):
        """the metric dict of an aligned scene: the registration's pose and its quality attached (start: the global stage's dict)"""
        out["transformation"] = reg["transformation"]
        out["alignment"] = {k: reg[k] for k in ("fitness", "inlier_rmse", "iterations", "converged")}
        if start is not None:
            out["alignment"]["global"] = dict({k: start[k] for k in ("fitness", "inlier_rmse", "correspondences", "transformation")},
                                              hypothesis=start["ransac"]["hypothesis"], inliers=start["ransac"]["inliers"]["count"],
                                              valid_hypotheses=start["ransac"]["valid_hypotheses"])
        return out

    @staticmethod
    def _align_options(align):
        opts = dict(estimation="point_to_plane", max_iterations=30, normal_k=16, voxel_size=None, lambda_geometric=0.968, gradient_k=16,
                    init=None)
        opts["global"] = None
        unknown = sorted(set(align) - set(opts) - {"max_correspondence_distance"})
        if unknown:
            raise ValueError(f"geometry_metrics: align does not take {unknown}")
        if "max_correspondence_distance" not in align:
            raise ValueError("geometry_metrics: align needs max_correspondence_distance")
        opts.update(align)
        if opts["estimation"] != "colored" and ("lambda_geometric" in align or "gradient_k" in align):
            raise ValueError("geometry_metrics: align's lambda_geometric and gradient_k belong to estimation 'colored'")
        return opts

    def _visibility_poses(self, visible_from, what):
        """(P,4,4) float64 world -> camera poses of a visible_from argument: "frames" or an array"""
        if isinstance(visible_from, str):
            if visible_from != "frames":
                raise ValueError(f"{what}: visible_from is 'frames' or a (P,4,4) array of world -> camera poses, not {visible_from!r}")
            Ts = [self.transform_grid[c[0]][c[1]]["T"] for c in self._stored_coords(None, what)]
            return np.stack([np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, dtype=np.float64) for T in Ts])
        poses = np.asarray(visible_from.detach().cpu() if isinstance(visible_from, torch.Tensor) else visible_from, dtype=np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (4, 4) or poses.shape[0] < 1 or not np.isfinite(poses).all():
            raise ValueError(f"{what}: visible_from is 'frames' or a (P,4,4) array of finite world -> camera poses")
        return poses

    def _visibility_cull(self, mesh, poses, tolerance=1e-3, accelerator="grid"):
        """surface_metrics' cull: the samples of `mesh` that some pose sees at the scene's intrinsics and frame resolution"""
        from . import meshops
        H, W = self.image_resolution
        z0, z1 = self._Z_RANGE[self.data]
        grid = meshops._accelerator(accelerator, "geometry_metrics")(mesh)
        return lambda points: grid.visible_points(points, poses.astype(np.float32), self.K, H, W, z0, z1, tolerance)["visible"]

    def visible_surface(self, mesh=None, poses="frames", n_samples=4096, seed=0, tolerance=1e-3, accelerator="grid"):
        """Which part of a surface the cameras saw: n_samples area-uniform samples of `mesh` (a tsdf.DeviceMesh; None: the run's
        own marching-cubes mesh) and whether the poses ("frames": the stored frames', or (P,4,4) world -> camera) see them, the
        mesh itself being the occluder -> {"points" (n,3) fp32, "visible" (n,) bool, "count" (n,) int32}.  What geometry_metrics(...,
        visible_from=...) culls by.  accelerator "grid" | "bvh": the structure the rays go through (the same answers)."""
        from . import meshops
        tree = meshops._accelerator(accelerator, "visible_surface")
        if mesh is None:
            mesh = self.clean_triangle_mesh(normals=False)["mesh"]
        if mesh.n_triangles < 1:
            raise ValueError("visible_surface: the mesh has no triangles")
        points = meshops.sample_points(mesh, n_samples, seed, colors=False)["points"]
        H, W = self.image_resolution
        z0, z1 = self._Z_RANGE[self.data]
        seen = meshops.visible_points(points, mesh, self._visibility_poses(poses, "visible_surface").astype(np.float32), self.K, H, W, z0, z1,
                                      tolerance, method="grid", grid=tree(mesh) if tree is meshops.TriangleBVH else None)
        return {"points": points, "visible": seen["visible"], "count": seen["count"]}

    def _surface_geometry_metrics(self, reference, threshold, frames, max_distance, voxel_size, align, source, mesh_clean, surface_samples,
                                  visible_from=None, accelerator="grid", mesh_simplify=None):
        """geometry_metrics(surface_samples=n): the scene's (cleaned, decimated) mesh as a surface against the reference"""
        from . import geometry, meshops
        from .tsdf import DeviceMesh
        what = "geometry_metrics"
        if isinstance(surface_samples, bool) or not isinstance(surface_samples, (int, np.integer)) or surface_samples < 1:
            raise ValueError(f"{what}: surface_samples is a positive integer or None, not {surface_samples!r}")
        n = int(surface_samples)
        if source != "mesh":
            raise ValueError(f"{what}: surface_samples belongs to source='mesh'")
        if frames is not None:
            raise ValueError(f"{what}: frames belongs to source='frames' (the mesh is the fusion of the whole run)")
        if voxel_size is not None:
            raise ValueError(f"{what}: voxel_size does not go with surface_samples (the surface sampling replaces the resampling)")
        ref = self._reference_geometry(reference, lambda scene: scene._metric_mesh(mesh_clean, mesh_simplify, what), True)
        pred = self._metric_mesh(mesh_clean, mesh_simplify, what)
        if pred.n_triangles < 1:
            raise ValueError(f"{what}: the mesh has no triangles")
        poses = None
        if visible_from is not None:
            if not isinstance(ref, DeviceMesh):
                raise ValueError(f"{what}: visible_from needs a reference that is a surface (a DeviceMesh or a scene): a cloud or ground-truth "
                                 "frames have no triangles to occlude with")
            if ref.n_triangles < 1:
                raise ValueError(f"{what}: the reference mesh has no triangles")
            poses = self._visibility_poses(visible_from, what)
        if align is None:
            return meshops.surface_metrics(pred, ref, threshold, n_samples=n, max_distance=max_distance, accelerator=accelerator,
                                           cull=None if poses is None else self._visibility_cull(ref, poses, accelerator=accelerator))
        opts = self._align_options(align)
        ref_points = meshops.sample_points(ref, n, colors=False)["points"] if isinstance(ref, DeviceMesh) else ref
        if ref_points.dim() != 2 or ref_points.device != pred.vertices.device:
            raise ValueError(f"{what}: align needs an (M,3) reference cloud or a mesh on the scene's device")
        pred_points = meshops.sample_points(pred, n, colors=False)["points"]
        start = self._global_init(opts, pred_points, ref_points.contiguous(), None, None)
        reg = _register_clouds(pred_points, ref_points.contiguous(), None, opts["max_correspondence_distance"], opts["estimation"],
                               opts["max_iterations"], opts["normal_k"], opts["voxel_size"], what,
                               init=None if start is None else start["transformation"])
        moved = meshops.make_mesh(geometry.transform_points(pred.vertices[:pred.n_vertices].contiguous(), reg["transformation"]),
                                  pred.triangles[:pred.n_triangles].contiguous())
        cull = None
        if poses is not None:                                              # the cameras in the reference's frame
            cull = self._visibility_cull(ref, poses @ np.linalg.inv(reg["transformation"].cpu().numpy().astype(np.float64)), accelerator=accelerator)
        return self._with_alignment(meshops.surface_metrics(moved, ref, threshold, n_samples=n, max_distance=max_distance, cull=cull,
                                                            accelerator=accelerator), reg, start)

    def frame_drift(self, max_correspondence_distance, frames=None, estimation="point_to_plane", max_iterations=30, normal_k=16,
                    voxel_size=None, lambda_geometric=0.968, gradient_k=16):
        """How far, rigidly, each generated frame's geometry sits from the frames that existed when it was generated: one ICP per
        stored frame that has predecessors (in the store's order: frame index, then coordinate; or only those at the grid
        coordinates `frames`), on either warp branch.  Source = that frame's cloud, merged_point_cloud(frames=[c]); target
        = the merged cloud of the stored frames with a SMALLER frame index, its normals (point-to-plane) pointing towards each
        point's own camera: merged_point_cloud(frames=those, normals=True, normal_k=normal_k) — both without their NaN points,
        the source voxel-sampled and the target cleaned at `voxel_size` when given.  geometry.register_icp from the identity
        (DESIGN §4.4.6).  Returns one dict per frame: coord, index (the frame index), rotation_deg and translation (angle and
        norm of the residual rigid motion), fitness, inlier_rmse, iterations, converged, status.  A frame whose ICP is degenerate
        (status 2: too few correspondences, or a pose direction they leave free) reports NaN motion; it does not raise.

        estimation="colored" (coloured ICP): for frames whose geometry leaves the pose free — an aerial view of near-planar
        terrain slides along itself under point-to-plane and reports NaN — and whose colours do not.  The source's and the
        target's colours are the "colors" of the same two merged_point_cloud calls, the target's normals as for point-to-plane,
        its gradients geometry.color_gradients(points, normals, colors, k=gradient_k): geometry.register_icp(source, points,
        estimation="colored", target_normals=normals, source_colors=..., target_colors=colors, lambda_geometric=...)."""
        from . import geometry
        geometry.check_estimation(estimation, "frame_drift")
        coords, stored = self._stored_coords(frames, "frame_drift"), self._stored_coords(None, "frame_drift")
        out = []
        for c in coords:
            index = self.frames[c]["index"]
            earlier = [e for e in stored if self.frames[e]["index"] < index]
            if not earlier:
                continue
            source_cloud = self.merged_point_cloud(frames=[c])
            source = source_cloud["points"]
            target = self.merged_point_cloud(frames=earlier, voxel_size=voxel_size, normals=estimation != "point_to_point", normal_k=normal_k)
            entry = {"coord": c, "index": index}
            # (point-to-point without voxel_size: the target is the raw cloud, whose NaN points _register_clouds leaves out)
            if not all(bool(torch.isfinite(p).all(dim=1).any()) for p in (target["points"], source)):
                reg = {"rotation_deg": float("nan"), "translation": float("nan"), "fitness": 0.0, "inlier_rmse": float("nan"),
                       "iterations": 0, "converged": False, "status": 2}
            else:
                colored = None
                if estimation == "colored":
                    colored = dict(source_colors=source_cloud["colors"], target_colors=target["colors"], lambda_geometric=lambda_geometric,
                                   gradient_k=gradient_k)
                reg = _register_clouds(source, target["points"], target.get("normals"), max_correspondence_distance, estimation,
                                       max_iterations, normal_k, voxel_size, "frame_drift", sample_target=False, colored=colored)
                reg.update(_rigid_motion(reg["transformation"].cpu().numpy(), reg["status"]))
            entry.update({k: reg[k] for k in ("rotation_deg", "translation", "fitness", "inlier_rmse", "iterations", "converged", "status")})
            out.append(entry)
        return out

    def optimize_poses(self, max_correspondence_distance, frames=None, estimation="point_to_plane", voxel_size=None, normal_k=16, **options):
        """Multiway registration of the scene's own frames: what takes out the drift frame_drift measures.  One
        world-frame correction C_i per stored frame (in the store's order: frame index, then coordinate; or only those at the grid
        coordinates `frames`), on either warp branch, such that the clouds C_i * cloud_i agree; the first frame keeps the identity
        (or the one at position options["fixed"]).  Call by call:
            cloud_i = merged_point_cloud(frames=[c_i])
            points_i, index_i, normals_i = geometry.prepare_cloud(cloud_i["points"], "optimize_poses", voxel_size,
                                                                  normal_k=None if estimation == "point_to_point" else normal_k)
                (the NaN points dropped, voxel-sampled at voxel_size when given, the normals of what is left)
            colors_i = cloud_i["colors"][index_i]                         (estimation "colored" only)
            geometry.multiway_registration([points_i], max_correspondence_distance, estimation=estimation, normals=[normals_i],
                                           colors=[colors_i], normal_k=normal_k, **options)
        whose options (min_fitness, loop_closure_stride, registrations, max_icp_iterations, and optimize_pose_graph's) pass
        through: frames next to each other in the store's order give the certain edges, every other pair that overlaps a loop
        closure the line process may switch off.  Returns {"coords", "corrections" (F,4,4) fp64 on the device, "Ts_w2c" (F,4,4)
        float64: the corrected world -> camera poses T_i C_i^-1, "edges" [(i, j, uncertain)] by position in coords,
        "line_weights", "kept", "missing_odometry", "converged", "status", "iterations", "cost"}.  The store is not touched:
        merged_point_cloud(pose_corrections=result) and geometry_metrics(..., pose_corrections=result) apply the corrections."""
        from . import geometry
        what = "optimize_poses"
        geometry.check_estimation(estimation, what)
        coords = self._stored_coords(frames, what)
        points, normals, colors = [], [], []
        for c in coords:
            cloud = self.merged_point_cloud(frames=[c])
            p, index, nrm = geometry.prepare_cloud(cloud["points"], what, voxel_size, normal_k=None if estimation == "point_to_point" else normal_k)
            points.append(p), normals.append(nrm), colors.append(cloud["colors"][index].contiguous())
        out = geometry.multiway_registration(points, max_correspondence_distance, estimation=estimation,
                                             normals=None if estimation == "point_to_point" else normals,
                                             colors=colors if estimation == "colored" else None, normal_k=normal_k, **options)
        C = out["poses"]
        Ts = np.stack([np.asarray(self.transform_grid[c[0]][c[1]]["T"], dtype=np.float64) @ np.linalg.inv(Ci)
                       for c, Ci in zip(coords, C.cpu().numpy())])
        return {"coords": coords, "corrections": C, "Ts_w2c": Ts,
                **{k: out[k] for k in ("edges", "line_weights", "kept", "missing_odometry", "converged", "status", "iterations", "cost")}}

    def view_consistency(self, depth_tolerance, frames=None, pairs="earlier", pose_corrections=None, maps=False):
        """Whether the scene's frames agree with each other IN THE IMAGE (geometry.view_consistency): the pixels
        of stored frame s put into the camera of stored frame t with their own depth, and checked against the colours and depths
        frame t holds — next to frame_drift's rigid residual between clouds; on either warp branch.  Frames in the store's order
        (frame index, then coordinate; or only those at the grid coordinates `frames`), poses through pose_corrections as in
        merged_point_cloud, the dataset's z range, depth_tolerance in depth units.  pairs: "earlier" — every frame against each
        stored frame with a smaller frame index (what it was generated from, and everything before); "all" — every ordered pair;
        or a list of (coord_s, coord_t).

        Returns {"coords", "pairs" [(s, t)] by position in coords, "sums" (P,12) fp64 on the device, "per_pair" (one
        geometry.consistency_summary per pair), "per_frame" (one summary per source frame over its pairs, with "coord" and "index":
        a consistency curve next to the drift curve), "total"}; with maps=True also "class_map", "color_error", "depth_error"
        (P,H,W).  Neither the store nor the volume is touched."""
        from . import geometry
        what = "view_consistency"
        coords = self._stored_coords(frames, what)
        index = [self.frames[c]["index"] for c in coords]
        n = len(coords)
        if isinstance(pairs, str):
            if pairs not in ("earlier", "all"):
                raise ValueError(f"{what}: pairs is 'earlier', 'all' or a list of (coord_s, coord_t), not {pairs!r}")
            pos = [(s, t) for s in range(n) for t in range(n) if s != t and (pairs == "all" or index[t] < index[s])]
        else:
            where = {c: k for k, c in enumerate(coords)}
            pos = []
            for pr in pairs:
                cs, ct = (tuple(c) for c in pr)
                if cs not in where or ct not in where:
                    raise ValueError(f"{what}: no stored frame (among those chosen) at {[c for c in (cs, ct) if c not in where]}")
                pos.append((where[cs], where[ct]))
        if not pos:
            raise ValueError(f"{what}: no pairs (pairs={pairs!r} over {n} frame{'s' if n != 1 else ''})")
        z0, z1 = self._Z_RANGE[self.data]
        Ts = self._corrected_poses(coords, pose_corrections, what)
        res = geometry.view_consistency([self.frames[c]["depth"] for c in coords], [self.frames[c]["rgb_u8"] for c in coords], self.K,
                                        np.stack([np.asarray(T, dtype=np.float64) for T in Ts]), z0, z1, depth_tolerance, pairs=pos,
                                        maps=maps)
        rows = res["sums"].cpu().numpy()                                    # the one host read
        per_frame = []
        for s in sorted({s for s, _ in pos}):
            mine = [k for k, (a, _) in enumerate(pos) if a == s]
            per_frame.append({"coord": coords[s], "index": index[s], **geometry.consistency_summary(rows[mine])})
        return {"coords": coords, **res, "per_pair": [geometry.consistency_summary(r) for r in rows], "per_frame": per_frame,
                "total": geometry.consistency_summary(rows)}

    def rgbd_odometry(self, max_depth_diff, frames=None, pairs="earlier", pose_corrections=None, **options):
        """The image-space drift of the scene's frames (geometry.rgbd_odometry), next to frame_drift's: for every
        pair (s, t) of stored frames the pose M_st (camera s -> camera t) that minimises the reprojection error view_consistency
        measures, started from the stored relative pose T_t T_s^-1 (poses through pose_corrections as in merged_point_cloud), ALL
        pairs in one batched call; the residual rigid motion M_st (T_t T_s^-1)^-1 is what the stored poses are off by.  Frames in
        the store's order (or only those at the grid coordinates `frames`), the dataset's z range; pairs: "earlier" (every frame
        against each stored frame with a smaller frame index), "consecutive" (each frame against the one before it in the store's
        order), "all", or a list of (coord_s, coord_t); options: geometry.rgbd_odometry's (iterations, lambda_geometric, ...).  On
        either warp branch; neither the store nor the volume is touched.  Returns {"coords", "pairs" [(s, t)] by position in
        coords, "transformation" (P,4,4) fp64 device, "per_pair" [{"pair", "rotation_deg", "translation", "fitness", "rmse",
        "iterations", "status"}], "per_frame" [{"coord", "index", "rotation_deg", "translation"}: per source frame the means over
        its pairs that are not degenerate, NaN without one]}.  A degenerate pair (status 2) reports NaN motion."""
        from . import geometry
        what = "rgbd_odometry"
        coords = self._stored_coords(frames, what)
        index = [self.frames[c]["index"] for c in coords]
        n = len(coords)
        if isinstance(pairs, str):
            if pairs not in ("earlier", "consecutive", "all"):
                raise ValueError(f"{what}: pairs is 'earlier', 'consecutive', 'all' or a list of (coord_s, coord_t), not {pairs!r}")
            if pairs == "consecutive":
                pos = [(s, s - 1) for s in range(1, n)]
            else:
                pos = [(s, t) for s in range(n) for t in range(n) if s != t and (pairs == "all" or index[t] < index[s])]
        else:
            where = {c: k for k, c in enumerate(coords)}
            pos = []
            for pr in pairs:
                cs, ct = (tuple(c) for c in pr)
                if cs not in where or ct not in where:
                    raise ValueError(f"{what}: no stored frame (among those chosen) at {[c for c in (cs, ct) if c not in where]}")
                pos.append((where[cs], where[ct]))
        if not pos:
            raise ValueError(f"{what}: no pairs (pairs={pairs!r} over {n} frame{'s' if n != 1 else ''})")
        z0, z1 = self._Z_RANGE[self.data]
        Ts = [np.asarray(T, dtype=np.float64) for T in self._corrected_poses(coords, pose_corrections, what)]
        nominal = np.stack([Ts[t] @ np.linalg.inv(Ts[s]) for s, t in pos])
        res = geometry.rgbd_odometry([self.frames[c]["depth"] for c in coords], [self.frames[c]["rgb_u8"] for c in coords], self.K, pos,
                                     z0, z1, max_depth_diff, init=nominal, information=False, **options)
        P = len(pos)
        host = torch.cat([res["transformation"].reshape(P, 16)] + [res[k][:, None] for k in ("status", "fitness", "rmse", "iterations")],
                         dim=1).cpu().numpy()                                   # the one host read
        per_pair = []
        for k, pr in enumerate(pos):
            status = int(host[k, 16])
            motion = _rigid_motion(host[k, :16].reshape(4, 4) @ np.linalg.inv(nominal[k]), status)
            per_pair.append({"pair": pr, **motion, "fitness": float(host[k, 17]), "rmse": float(host[k, 18]), "iterations": int(host[k, 19]),
                             "status": status})
        per_frame = []
        for s in sorted({s for s, _ in pos}):
            mine = [e for e in per_pair if e["pair"][0] == s and e["status"] != 2]
            mean = lambda key: float(np.mean([e[key] for e in mine])) if mine else float("nan")  # noqa: E731
            per_frame.append({"coord": coords[s], "index": index[s], "rotation_deg": mean("rotation_deg"), "translation": mean("translation")})
        return {"coords": coords, "pairs": pos, "transformation": res["transformation"], "per_pair": per_pair, "per_frame": per_frame}

    def optimize_poses_rgbd(self, max_depth_diff, frames=None, **options):
        """optimize_poses with direct RGB-D odometry in place of one ICP per pair (geometry.multiway_rgbd): the
        stored frames (in the store's order, or those at the grid coordinates `frames`) with their stored poses and the dataset's z
        range; options: multiway_rgbd's (min_covisibility, loop_closure_stride, iterations, lambda_geometric, and
        optimize_pose_graph's).  On either warp branch; the store and the volume are not touched.  Returns exactly optimize_poses'
        keys, so merged_point_cloud, geometry_metrics, view_consistency and fuse_frames take the result as pose_corrections."""
        from . import geometry
        what = "optimize_poses_rgbd"
        coords = self._stored_coords(frames, what)
        z0, z1 = self._Z_RANGE[self.data]
        Ts = np.stack([np.asarray(self.transform_grid[c[0]][c[1]]["T"], dtype=np.float64) for c in coords])
        out = geometry.multiway_rgbd([self.frames[c]["depth"] for c in coords], [self.frames[c]["rgb_u8"] for c in coords], self.K, Ts, z0, z1,
                                     max_depth_diff, **options)
        C = out["poses"]
        return {"coords": coords, "corrections": C, "Ts_w2c": np.stack([T @ np.linalg.inv(Ci) for T, Ci in zip(Ts, C.cpu().numpy())]),
                **{k: out[k] for k in ("edges", "line_weights", "kept", "missing_odometry", "converged", "status", "iterations", "cost")}}

    def fuse_frames(self, frames=None, pose_corrections=None, color=True, max_bricks=None):
        """"Integrate scene", the last stage of the reconstruction pipeline: a NEW TsdfVolume (the dataset's VOLUME_PARAMS) into
        which every stored frame (in the store's order; or those at the grid coordinates `frames`) is integrated exactly once with
        its corrected pose (pose_corrections as in merged_point_cloud; None: the stored poses), one TsdfVolume.integrate per frame,
        with colour when `color`.  The box is the frusta of those corrected poses with _make_volume's margin.  Works on either warp
        branch — the forward-splat loop has no volume of its own — and is how optimize_poses' corrections reach a mesh:
        colour_volume() replays the loop's log with the stored poses.  check() is called; self.volume, the log and the store are
        left alone.  max_bricks: the pool's size (default: TsdfVolume's, from the scene's memory budget)."""
        from .tsdf import VOLUME_PARAMS, TsdfVolume, frustum_bounds, UNIT
        what = "fuse_frames"
        coords = self._stored_coords(frames, what)
        Ts = [np.asarray(T, dtype=np.float64) for T in self._corrected_poses(coords, pose_corrections, what)]
        voxel, trunc = VOLUME_PARAMS[self.data]
        H, W = self.image_resolution
        lo, hi = frustum_bounds(self.K, Ts, H, W, self._Z_RANGE[self.data][1], margin=trunc + voxel * UNIT)
        vol = TsdfVolume(voxel, trunc, lo, hi, self.device, color=bool(color), memory_budget_bytes=self.tsdf_memory_budget_bytes,
                         max_bricks=max_bricks)
        for c, T in zip(coords, Ts):
            vol.integrate(self.frames[c]["depth"], self.K, T, self.frames[c]["rgb_u8"] if color else None)
        vol.check()
        return vol

    def export_fused_mesh(self, out_dir, frames=None, pose_corrections=None, clean=None, simplify=None):
        """`fused_triangle_mesh.ply`: the marching-cubes mesh of fuse_frames(frames, pose_corrections) with vertex colours and
        normals, in export_triangle_mesh's layout; on either warp branch.  `clean`: a dict of meshops.clean's arguments; when given,
        `fused_triangle_mesh_clean.ply` — that mesh after the device clean-up — is written as well.  `simplify`: a dict of
        meshops.simplify_quadric_decimation's arguments; when given, `fused_triangle_mesh_simplified.ply` — the (cleaned, when
        `clean` is given too) mesh after quadric-error decimation, with its own normals — is written as well.  Returns {file
        name: number of triangles}."""
        from . import meshops, pointcloud
        if clean is not None:
            clean = self._clean_arguments(clean, "export_fused_mesh")
        if simplify is not None:
            simplify = self._simplify_arguments(simplify, "export_fused_mesh")
        os.makedirs(out_dir, exist_ok=True)
        vol = self.fuse_frames(frames=frames, pose_corrections=pose_corrections)
        mesh = vol.extract_triangle_mesh()
        out = {"fused_triangle_mesh.ply": pointcloud.write_triangle_mesh(os.path.join(out_dir, "fused_triangle_mesh.ply"), mesh["vertices"],
                                                                         mesh["triangles"], mesh.get("vertex_colors"),
                                                                         mesh["vertex_normals"])}
        if clean is not None:
            c = meshops.clean(vol.extract_mesh_device(), **clean)
            m = c["mesh"]
            col = None if m.vertex_colors is None else (m.vertex_colors / 255.0).cpu().numpy()
            nrm = None if c["vertex_normals"] is None else c["vertex_normals"].cpu().numpy()
            name = "fused_triangle_mesh_clean.ply"
            out[name] = pointcloud.write_triangle_mesh(os.path.join(out_dir, name), m.vertices.cpu().numpy(), m.triangles.cpu().numpy(), col, nrm)
        if simplify is not None:
            d = self._simplified(vol.extract_mesh_device(), clean, simplify)
            name = "fused_triangle_mesh_simplified.ply"
            out[name] = self._write_device_mesh(os.path.join(out_dir, name), d["mesh"], d["vertex_normals"])
        return out


def _rigid_motion(T, status):
    """angle (degrees) and translation norm of a 4x4 rigid motion; NaN for a degenerate registration (status 2)"""
    if status == 2:
        return {"rotation_deg": float("nan"), "translation": float("nan")}
    cos = min(1.0, max(-1.0, (float(np.trace(T[:3, :3])) - 1.0) / 2.0))
    return {"rotation_deg": float(np.degrees(np.arccos(cos))), "translation": float(np.linalg.norm(T[:3, 3]))}


def _register_clouds(source, target, target_normals, max_correspondence_distance, estimation, max_iterations, normal_k, voxel_size, what,
                     sample_target=True, colored=None, init=None):
    """geometry.register_icp of two device clouds for the scene-level callers: the NaN points dropped, both (or, with
    sample_target=False, the source only) voxel-sampled at voxel_size, the target's normals estimated (k = normal_k) where
    point-to-plane or colored has none given.  colored: {source_colors, target_colors (uint8, one per point of source / target as
    given: they follow their points through both steps), lambda_geometric, gradient_k} for estimation "colored".  init: the pose
    the registration starts from (the identity by default)."""
    from . import geometry
    geometry.check_estimation(estimation, what)
    if (estimation == "colored") != (colored is not None):
        raise ValueError(f"{what}: colours go with estimation 'colored'")
    src, si, _ = geometry.prepare_cloud(source, what, voxel_size)
    tgt, ti = target, slice(None)
    if target_normals is None:                    # (a target that comes with its normals is the caller's prepared cloud)
        tgt, ti, target_normals = geometry.prepare_cloud(target, what, voxel_size if sample_target else None,
                                                         normal_k=None if estimation == "point_to_point" else normal_k)
    extra = {}
    if colored is not None:
        sc, tc = colored["source_colors"], colored["target_colors"]
        if sc.shape[0] != source.shape[0] or tc.shape[0] != target.shape[0]:
            raise ValueError(f"{what}: one colour per point ({sc.shape[0]} for {source.shape[0]} and {tc.shape[0]} for {target.shape[0]})")
        extra = dict(source_colors=sc[si].contiguous(), target_colors=tc[ti].contiguous(), lambda_geometric=colored["lambda_geometric"],
                     gradient_k=colored["gradient_k"])
    return geometry.register_icp(src, tgt, max_correspondence_distance, estimation=estimation, max_iterations=max_iterations, init=init,
                                 target_normals=None if estimation == "point_to_point" else target_normals, **extra)


def _quat_from_rot(R):
    """unit quaternion (w, x, y, z) of a rotation matrix (the branch with the largest pivot)"""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.empty(4)
        q[0] = R[k, j] - R[j, k]
        q[1 + i] = 1.0 + R[i, i] - R[j, j] - R[k, k]
        q[1 + j] = R[j, i] + R[i, j]
        q[1 + k] = R[k, i] + R[i, k]
    return q / np.linalg.norm(q)


def _rot_from_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _slerp(qa, qb, s):
    """spherical interpolation of unit quaternions along the shorter arc"""
    d = float(np.dot(qa, qb))
    if d < 0:
        qb, d = -qb, -d
    if d > 1 - 1e-12:                                   # (nearly) equal rotations: the arc has no direction
        q = (1 - s) * qa + s * qb
    else:
        th = np.arccos(d)
        q = (np.sin((1 - s) * th) * qa + np.sin(s * th) * qb) / np.sin(th)
    return q / np.linalg.norm(q)


def step_unit(step, k):
    return step * k
