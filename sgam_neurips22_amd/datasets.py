"""The reference's training datasets (data/google_earth.py, data/clevr-infinite.py; for the codebook phase the single-frame
data/custom_codebook.py over data/base.py's ImagePaths) and the batch builder that feeds `VQModel.training_step`.

Dataset classes keep the reference's constructor keywords, on-disk layout, neighbour rules, source choice and the keys, shapes
and dtypes of a sample.  What differs is where the per-sample arithmetic runs: `BatchBuilder(backend="host")` is the
reference's own arithmetic (PIL, numpy float64, `F.interpolate`), collated like `default_collate`; `backend="device"` decodes
files into pinned staging on a thread pool and lets csrc/imageio.hip write the batch tensors, equal to the host batch in bits.
"""
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

_GL2CV = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])
SENTINEL, SENTINEL_REPLACEMENT = 65504, -99999


# ------------------------------------------------------------------------------------------------
# neighbour graph: plain sorted adjacency lists
# ------------------------------------------------------------------------------------------------
def neighbour_lists(positions, threshold, classes=None, block=1024):
    """adjacency of `distance <= threshold` between distinct nodes (and equal `classes` where given), float64, row blocks of
    the pairwise matrix: list of sorted index arrays, one per node"""
    P = np.asarray(positions, np.float64).reshape(-1, 3)
    n = len(P)
    out = [None] * n
    cls = None if classes is None else np.asarray(classes)
    for i0 in range(0, n, block):
        d = P[i0:i0 + block, None, :] - P[None, :, :]
        near = np.sqrt((d * d).sum(-1)) <= threshold
        if cls is not None:
            near &= cls[i0:i0 + block, None] == cls[None, :]
        near[np.arange(len(near)), np.arange(i0, i0 + len(near))] = False
        for r in range(len(near)):
            out[i0 + r] = np.flatnonzero(near[r])
    return out


class Scene:
    """one scene directory: kept nodes in ascending key order, their world-to-camera poses, file paths and neighbours (as keys)"""

    def __init__(self, keys, w2c, rgb_paths, depth_paths, neighbours):
        self.keys, self.w2c, self.rgb_paths, self.depth_paths, self.neighbours = keys, w2c, rgb_paths, depth_paths, neighbours
        self.index = {k: i for i, k in enumerate(keys)}

    def __len__(self):
        return len(self.keys)


def _poses(frames):
    c2w = np.array([np.array(f["transform_matrix"]) @ _GL2CV for f in frames], np.float64).reshape(-1, 4, 4)
    return c2w, (np.linalg.inv(c2w) if len(c2w) else c2w)


class _PairDataset:
    """shared half of the two datasets: index parsing, source choice, relative poses, host sample, device decode"""
    dataset_name = None

    def _init_common(self, split, n_src, dataset_dir, dataset, image_resolution, seed):
        self.split, self.src_num, self.dataset, self.dataset_dir = split, n_src, dataset, dataset_dir
        self.image_resolution = image_resolution
        self.seed = seed
        self._prng = None
        self._initpid = None
        self.grids = []
        self.cumulative_sum = [0]

    @property
    def prng(self):
        """per-process RandomState of the train split's source choice (re-made after a fork); `seed` makes it reproducible"""
        pid = os.getpid()
        if self._initpid != pid:
            self._initpid = pid
            self._prng = np.random.RandomState(seed=self.seed)
        return self._prng

    def __len__(self):
        return self.cumulative_sum[-1]

    def parse_idx(self, idx):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        g = int(np.searchsorted(self.cumulative_sum, idx, side="right")) - 1
        return g, self.grids[g].keys[idx - self.cumulative_sum[g]]

    def choose(self, global_index):
        """(scene, target key, source keys): train draws with replacement from the process RandomState, the other splits take
        the head of a shuffle seeded by the index"""
        g, key = self.parse_idx(global_index)
        scene = self.grids[g]
        nb = sorted(scene.neighbours[key])
        if self.split == "train":
            srcs = [nb[k] for k in self.prng.choice(len(nb), self.src_num)]
        else:
            nb = np.array(nb)
            np.random.RandomState(seed=global_index).shuffle(nb)
            srcs = [int(k) for k in nb[:self.src_num]]
        return scene, key, srcs

    def _relative(self, scene, key, srcs, K):
        """Ks, K_invs, R_rels, t_rels (float64 lists, padded to n_src) and the ones `src_masks`"""
        T_tgt = np.eye(4)
        T_tgt[:3, :3] = scene.w2c[scene.index[key]][:3, :3]
        T_tgt[:3, 3] = scene.w2c[scene.index[key]][:3, 3]
        Ks, K_invs, R_rels, t_rels = [], [], [], []
        for s in srcs:
            T_src = np.eye(4)
            T_src[:3, :3] = scene.w2c[scene.index[s]][:3, :3]
            T_src[:3, 3] = scene.w2c[scene.index[s]][:3, 3]
            T_rel = T_tgt @ np.linalg.inv(T_src)
            R_rels.append(T_rel[:3, :3])
            t_rels.append(T_rel[:3, 3])
            Ks.append(K)
            K_invs.append(np.linalg.inv(K))
        while len(K_invs) < self.src_num:
            Ks.append(np.eye(3))
            K_invs.append(np.eye(3))
            R_rels.append(np.eye(3))
            t_rels.append(np.zeros(3))
        mask = np.zeros(self.src_num)
        mask[:self.src_num] = 1
        return Ks, K_invs, R_rels, t_rels, mask

    def __getitem__(self, global_index):
        return self.host_sample(self.plan(global_index))

    def plan(self, global_index):
        scene, key, srcs = self.choose(global_index)
        i = scene.index
        return {"scene": scene, "tgt": key, "srcs": srcs, "tgt_rgb": scene.rgb_paths[i[key]], "tgt_depth": scene.depth_paths[i[key]],
                "src_rgb": [scene.rgb_paths[i[s]] for s in srcs], "src_depth": [scene.depth_paths[i[s]] for s in srcs]}


def _open_rgb_u8(path):
    from PIL import Image
    a = np.asarray(Image.open(path))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{path}: the device batch builder takes 8-bit RGB images, got {a.dtype} {a.shape} "
                         "(use backend='host')")
    return a


def _load_depth_f32(path):
    d = np.load(path)
    if d.dtype not in (np.float32, np.float16):
        raise ValueError(f"{path}: the device batch builder takes float32 / float16 depth maps, got {d.dtype} (use backend='host')")
    return d.astype(np.float32, copy=False)


class GoogleEarthBase(_PairDataset):
    """data/google_earth.py GoogleEarthBase.  Neighbours: same `frame_id % 4` (four headings per grid point), camera centres at
    most 0.3 apart; `chicago` scenes skipped, frames with `is_valid` false skipped, nodes without a neighbour dropped, at most
    the first 900 valid frames of a scene outside the train split."""
    dataset_name = "google_earth"
    NEIGHBOUR_DISTANCE, OFF_TRAIN_CAP = 0.3, 900

    def __init__(self, split, n_src=2, dataset_dir=None, dataset=None, image_resolution=None, depth_range=None,
                 use_extrapolation_mask=None, seed=None):
        self._init_common(split, n_src, dataset_dir, dataset, image_resolution, seed)
        self.use_extrapolation_mask, self.depth_range = use_extrapolation_mask, depth_range
        if not os.path.isdir(str(dataset_dir)):
            raise FileNotFoundError(f"GoogleEarth dataset_dir {dataset_dir!r} does not exist")
        self.K = np.load(f"{self.dataset_dir}/K.npy")
        self.K[0] = self.K[0] * self.image_resolution[1] / 512
        self.K[1] = self.K[1] * self.image_resolution[0] / 512
        for scene_dir in sorted(Path(self.dataset_dir, self.split).glob("*")):
            if "chicago" in str(scene_dir):
                continue
            with open(str(scene_dir / "transforms.json")) as f:
                scene = self.build_scene(json.load(f)["frames"], scene_dir)
            self.grids.append(scene)
            self.cumulative_sum.append(len(scene) + self.cumulative_sum[-1])

    def build_scene(self, frames, scene_dir):
        nodes = {}
        for fr in frames:
            if not fr["is_valid"]:
                continue
            nodes[int(fr["file_path"][-9:-4])] = fr
            if len(nodes) == self.OFF_TRAIN_CAP and self.split != "train":
                break
        keys = sorted(nodes)
        c2w, w2c = _poses([nodes[k] for k in keys])
        near = neighbour_lists(c2w[:, :3, 3], self.NEIGHBOUR_DISTANCE, classes=np.array(keys, np.int64) % 4)
        keep = [i for i in range(len(keys)) if len(near[i])]
        return Scene([keys[i] for i in keep], w2c[keep], [str(scene_dir / f"im_{keys[i]:05d}.png") for i in keep],
                     [str(scene_dir / f"dm_{keys[i]:05d}.npy") for i in keep],
                     {keys[i]: [keys[j] for j in near[i]] for i in keep})

    def small_arrays(self, p):
        Ks, K_invs, R_rels, t_rels, mask = self._relative(p["scene"], p["tgt"], p["srcs"], self.K)
        ids = list(p["srcs"]) + [-1] * (self.src_num - len(p["srcs"]))
        return {"Ks": np.stack(Ks), "K_invs": np.stack(K_invs), "R_rels": np.stack(R_rels), "tgt_frame_id": np.array([p["tgt"]]),
                "src_frame_ids": np.array(ids), "t_rels": np.stack(t_rels), "src_masks": mask}

    KEYS = ("Ks", "K_invs", "R_rels", "tgt_frame_id", "src_frame_ids", "t_rels", "dst_img", "src_imgs", "dst_depth", "src_depths",
            "src_masks", "tgt_pixel_mask")

    def host_sample(self, p):
        """the reference's `__getitem__` arithmetic on the host"""
        import torch.nn.functional as F
        from PIL import Image
        res = self.image_resolution
        img_dst = Image.open(p["tgt_rgb"])
        img_srcs = [Image.open(f) for f in p["src_rgb"]]
        dm_dst = np.load(p["tgt_depth"])
        dm_srcs = [np.load(f) for f in p["src_depth"]]
        h, w = img_dst.size[:2]          # (PIL's size is (width, height); the reference compares it in this order)
        if res is not None and (res[0] != h or res[1] != w):
            img_srcs = [im.resize((res[1], res[0]), resample=Image.LANCZOS) for im in img_srcs]
            img_dst = img_dst.resize((res[1], res[0]), resample=Image.LANCZOS)
            dm_srcs = [F.interpolate(torch.from_numpy(d[None, None]), size=res)[0][0].numpy() for d in dm_srcs]
            dm_dst = F.interpolate(torch.from_numpy(dm_dst[None, None]), size=res)[0][0].numpy()
        img_dst = np.array(img_dst) / 127.5 - 1.0
        img_srcs = [np.array(im) / 127.5 - 1.0 for im in img_srcs]
        for d in dm_srcs:
            d[d == SENTINEL] = SENTINEL_REPLACEMENT
        while len(img_srcs) < self.src_num:
            img_srcs.append(np.zeros_like(img_srcs[-1]))
            dm_srcs.append(np.zeros_like(dm_srcs[-1]))
        ex = self.small_arrays(p)
        ex.update({"dst_img": img_dst, "src_imgs": np.stack(img_srcs), "dst_depth": dm_dst[..., None],
                   "src_depths": np.stack(dm_srcs)[..., None], "tgt_pixel_mask": (dm_dst != SENTINEL)[None]})
        return {k: ex[k].astype(np.float32) for k in self.KEYS}

    # ---- device path: what a decode thread leaves in the staging slot, and what the kernels then do with all slots
    def decode(self, rgb_path, depth_path, is_src):
        return _open_rgb_u8(rgb_path), _load_depth_f32(depth_path)

    def check_file_size(self, hf, wf):
        res = self.image_resolution
        if (hf, wf) != tuple(res) and not (res[0] != wf or res[1] != hf):
            raise ValueError(f"files of {hf} x {wf} with image_resolution {list(res)}: the reference skips the resize here")


class GoogleEarthTrain(GoogleEarthBase):
    def __init__(self, size=None, n_src=2, dataset_dir=None, dataset=None, image_resolution=None, depth_range=None,
                 use_extrapolation_mask=None, seed=None):
        super().__init__("train", n_src, dataset_dir, dataset, image_resolution, depth_range, use_extrapolation_mask, seed)
        self.size = size


class GoogleEarthValidation(GoogleEarthBase):
    def __init__(self, size=None, n_src=2, dataset_dir=None, dataset=None, image_resolution=None, depth_range=None,
                 use_extrapolation_mask=None, seed=None):
        super().__init__("val", n_src, dataset_dir, dataset, image_resolution, depth_range, use_extrapolation_mask, seed)
        self.size = size


class GoogleEarthTest(GoogleEarthBase):
    def __init__(self, size=None, n_src=2, dataset_dir=None, dataset=None, image_resolution=None, depth_range=None,
                 use_extrapolation_mask=None, seed=None):
        super().__init__("test", n_src, dataset_dir, dataset, image_resolution, depth_range, use_extrapolation_mask, seed)
        self.size = size


class Blender3dBase(_PairDataset):
    """data/clevr-infinite.py Blender3dBase (CLEVR-infinite).  Every frame of `transforms.json` is a node, in file order;
    neighbours are camera centres at most 3 apart.  Depth files hold ray lengths and are converted to z-depth in float64."""
    dataset_name = "clevr-infinite"
    NEIGHBOUR_DISTANCE = 3

    def __init__(self, split, dataset_dir, n_src=2, dataset=None, image_resolution=None, seed=None):
        self._init_common(split, n_src, dataset_dir, dataset, image_resolution, seed)
        self.K = np.load(f"{self.dataset_dir}/K.npy")
        for scene_dir in sorted(Path(self.dataset_dir, self.split).glob("*")):
            with open(str(scene_dir / "transforms.json")) as f:
                frames = json.load(f)["frames"]
            c2w, w2c = _poses(frames)
            near = neighbour_lists(c2w[:, :3, 3], self.NEIGHBOUR_DISTANCE)
            keys = list(range(len(frames)))
            scene = Scene(keys, w2c, [str(scene_dir / f"im_{i:05d}.png") for i in keys],
                          [str(scene_dir / f"dm_{i:05d}.npy") for i in keys], {i: [int(j) for j in near[i]] for i in keys})
            self.grids.append(scene)
            self.cumulative_sum.append(len(scene) + self.cumulative_sum[-1])

    KEYS = ("Ks", "K_invs", "R_rels", "t_rels", "dst_img", "src_imgs", "dst_depth", "src_depths", "src_masks")

    def _K_for(self, h, w):
        K = self.K
        K = K * self.image_resolution[1] / w
        K = K * self.image_resolution[0] / h
        return K

    def check_file_size(self, hf, wf):
        res = self.image_resolution
        if res is not None and (res[0] != hf or res[1] != wf):
            raise ValueError(f"CLEVR-infinite files are {hf} x {wf} but image_resolution is {list(res)}: the reference has no "
                             "working resize for this dataset (its branch calls ndarray.resize); set image_resolution to the "
                             "file size")

    def small_arrays(self, p, h=None, w=None):
        if h is None:
            h, w = self.image_resolution
        Ks, K_invs, R_rels, t_rels, mask = self._relative(p["scene"], p["tgt"], p["srcs"], self._K_for(h, w))
        return {"Ks": np.stack(Ks), "K_invs": np.stack(K_invs), "R_rels": np.stack(R_rels), "t_rels": np.stack(t_rels),
                "src_masks": mask}

    def host_sample(self, p):
        from PIL import Image

        from .inference_pipeline import ray_to_z_depth
        img_dst = np.array(Image.open(p["tgt_rgb"])) / 127.5 - 1.0
        img_srcs = [np.array(Image.open(f)) / 127.5 - 1.0 for f in p["src_rgb"]]
        dm_dst = ray_to_z_depth(np.load(p["tgt_depth"]), self.K)[..., None]
        dm_srcs = [ray_to_z_depth(np.load(f), self.K)[..., None] for f in p["src_depth"]]
        h, w = img_dst.shape[:2]
        self.check_file_size(h, w)
        while len(img_srcs) < self.src_num:
            img_srcs.append(np.zeros_like(img_srcs[-1]))
            dm_srcs.append(np.zeros_like(dm_srcs[-1]))
        ex = self.small_arrays(p, h, w)
        ex.update({"dst_img": img_dst, "src_imgs": np.stack(img_srcs), "dst_depth": dm_dst, "src_depths": np.stack(dm_srcs)})
        return {k: ex[k].astype(np.float32) for k in self.KEYS}

    def decode(self, rgb_path, depth_path, is_src):
        from .inference_pipeline import ray_to_z_depth
        return _open_rgb_u8(rgb_path), ray_to_z_depth(np.load(depth_path), self.K).astype(np.float32)


class Blender3dTrain(Blender3dBase):
    def __init__(self, dataset_dir=None, n_src=2, dataset=None, image_resolution=None, seed=None):
        super().__init__("train", dataset_dir, n_src, dataset, image_resolution, seed)


class Blender3dValidation(Blender3dBase):
    def __init__(self, dataset_dir=None, n_src=2, dataset=None, image_resolution=None, seed=None):
        super().__init__("val", dataset_dir, n_src, dataset, image_resolution, seed)


class Blender3dTest(Blender3dBase):
    def __init__(self, dataset_dir=None, n_src=2, dataset=None, image_resolution=None, seed=None):
        super().__init__("test", dataset_dir, n_src, dataset, image_resolution, seed)


# ------------------------------------------------------------------------------------------------
# the codebook phase's single RGB-D frames (data/base.py ImagePaths, data/custom_codebook.py)
# ------------------------------------------------------------------------------------------------
class ImagePaths:
    """data/base.py ImagePaths for `google_earth` and `clevr-infinite`: sample i is {"image": the preprocessed file
    paths[i], "file_path_": paths[i]} plus one entry per key of `labels`.  A path with 'png' in it is an image —
    `Image.open(p).resize(image_resolution)`, Pillow's default BICUBIC, then `/ 127.5 - 1` as float32 — and otherwise one with
    'npy' in it a depth map: nearest `F.interpolate`, then the dataset's inverse-depth arithmetic in the file's dtype
    (google_earth) or in float64 with the ray -> z conversion (clevr-infinite, `convert_depth_flag`).  The reference's
    SmallestMaxSize + CenterCrop that follows the resize is the identity for a square resolution, and its crop fails for any
    other: square resolutions only.  `kitti360`, `random_crop` and `NumpyPaths` are not built."""

    def __init__(self, paths, image_resolution=None, random_crop=False, labels=None, convert_depth_flag=True, dataset_dir=None,
                 dataset=None, depth_range=None):
        if dataset == "kitti360":
            raise NotImplementedError("ImagePaths: the kitti360 branch is not built")
        if random_crop:
            raise NotImplementedError("ImagePaths: random_crop is not built")
        if image_resolution is None or len(image_resolution) != 2 or image_resolution[0] != image_resolution[1]:
            raise ValueError(f"ImagePaths: image_resolution must be square, got {image_resolution!r} (the reference's center crop "
                             "is larger than its resized image otherwise)")
        self.image_resolution, self.depth_range, self.dataset_dir = image_resolution, depth_range, dataset_dir
        self.random_crop, self.dataset = random_crop, dataset
        self.labels = dict() if labels is None else labels
        self.labels["file_path_"] = paths
        self._length = len(paths)
        self.convert_depth_flag = convert_depth_flag
        if convert_depth_flag:
            self.K = np.load(self.dataset_dir + "/K.npy")
            self.K[0][0] = self.K[0][0] * self.image_resolution[1] / 256
            self.K[0][2] = self.K[0][2] * self.image_resolution[1] / 256
            self.K[1][1] = self.K[1][1] * self.image_resolution[0] / 256
            self.K[1][2] = self.K[1][2] * self.image_resolution[0] / 256

    def __len__(self):
        return self._length

    def _rgb(self, image_path):
        from PIL import Image
        image = Image.open(image_path).resize(self.image_resolution)
        if not image.mode == "RGB":
            image = image.convert("RGB")
        image = np.array(image).astype(np.uint8)
        return (image / 127.5 - 1.0).astype(np.float32)

    def _resized_depth(self, image_path):
        import torch.nn.functional as F
        depth = np.load(image_path)
        depth = F.interpolate(torch.from_numpy(depth[None, None,]), size=self.image_resolution)[0][0].numpy()
        if self.convert_depth_flag:
            h, w = depth.shape[:2]
            xs, ys = np.meshgrid(np.linspace(0, w - 1, w), np.linspace(0, h - 1, h))
            depth = depth * self.K[0][0] / np.sqrt(
                self.K[0][0] ** 2 + (self.K[0][2] - ys - 0.5) ** 2 + (self.K[1][2] - xs - 0.5) ** 2)
        return depth

    def preprocess_image_google_earth(self, image_path):
        if "png" in image_path:
            return self._rgb(image_path)
        if "npy" in image_path:
            depth = self._resized_depth(image_path)
            depth = depth + 10
            inverse_depth = 1 / depth
            scaled_idepth = (inverse_depth - 1 / 14.765625) / (1 / 10.099975586 - 1 / 14.765625)
            return 2 * scaled_idepth - 1
        raise NotImplementedError(image_path)

    def preprocess_image_clevr_infinite(self, image_path):
        if "png" in image_path:
            return self._rgb(image_path)
        if "npy" in image_path:
            depth = self._resized_depth(image_path)
            inverse_depth = 1 / depth
            scaled_idepth = (inverse_depth - 1 / 16) / (1 / 7 - 1 / 16)
            return (2 * scaled_idepth - 1).astype(np.float32)
        raise NotImplementedError(image_path)

    def __getitem__(self, i):
        example = dict()
        if self.dataset == "google_earth":
            example["image"] = self.preprocess_image_google_earth(self.labels["file_path_"][i])
        elif self.dataset == "clevr-infinite":
            example["image"] = self.preprocess_image_clevr_infinite(self.labels["file_path_"][i])
        else:
            raise NotImplementedError(self.dataset)
        for k in self.labels:
            example[k] = self.labels[k][i]
        return example


class CustomBase:
    """data/custom_codebook.py: single frames from a list file (one PNG path per line, used as written; lines with `chicago`
    dropped).  The depth map of a frame is its path with every 'im' replaced by 'dm' and '.png' by '.npy'.  A sample is
    {"image": (H, W, 4) float32 (3 without `use_depth`), "file_path_": str}; with depth the path is cut at its first '.'."""
    single_frame = True
    split = None
    VALIDATION_SEED, VALIDATION_CAP = 3, 2500

    def _init_paths(self, image_resolution, images_list_file, use_depth, convert_depth_flag, dataset_dir, dataset, depth_range):
        self.dataset, self.dataset_dir, self.use_depth = dataset, dataset_dir, use_depth
        self.image_resolution = image_resolution
        with open(images_list_file, "r") as f:
            paths = [path for path in f.read().splitlines() if "chicago" not in path]
        if self.split != "train":
            random.Random(self.VALIDATION_SEED).shuffle(paths)       # the order of random.seed(3); random.shuffle(paths)
            paths = paths[:self.VALIDATION_CAP]
        kw = dict(image_resolution=image_resolution, random_crop=False, convert_depth_flag=convert_depth_flag, dataset_dir=dataset_dir,
                  dataset=dataset, depth_range=depth_range)
        self.data = ImagePaths(paths=paths, **kw)
        self.depth_data = None
        if use_depth:
            if dataset == "kitti360":
                raise NotImplementedError("the kitti360 branch is not built")
            self.depth_data = ImagePaths(paths=[p.replace("im", "dm").replace(".png", ".npy") for p in paths], **kw)

    def __len__(self):
        return len(self.data)

    def plan(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return {"index": i, "rgb": self.data.labels["file_path_"][i],
                "depth": None if self.depth_data is None else self.depth_data.labels["file_path_"][i]}

    def file_path(self, p):
        return p["rgb"].split(".")[0] if p["depth"] is not None else p["rgb"]

    def host_sample(self, p):
        """the reference's `__getitem__` arithmetic on the host"""
        example = self.data[p["index"]]
        if self.depth_data is not None:
            depth_example = self.depth_data[p["index"]]
            example["image"] = np.concatenate([example["image"], depth_example["image"][:, :, None]], 2)
            example["file_path_"] = example["file_path_"].split(".")[0]
        return example

    def __getitem__(self, i):
        return self.host_sample(self.plan(i))

    # ---- device path ----
    def decode(self, p):
        """(uint8 RGB frame, depth map as float32 or None, the depth file's dtype)"""
        rgb = _open_rgb_u8(p["rgb"])
        if p["depth"] is None:
            return rgb, None, None
        d = np.load(p["depth"])
        if d.dtype not in (np.float32, np.float16) or d.ndim != 2:
            raise ValueError(f"{p['depth']}: the device batch builder takes 2-d float32 / float16 depth maps, got {d.dtype} "
                             f"{d.shape} (use backend='host')")
        return rgb, d.astype(np.float32, copy=False), d.dtype

    def codec(self, depth_dtype):
        """(arith, K) of `imageio.frame_depth_codec` for depth files of `depth_dtype`"""
        if self.dataset == "clevr-infinite":
            if not self.depth_data.convert_depth_flag or self.depth_data.K.dtype != np.float64:
                raise ValueError("the device batch builder takes clevr-infinite with convert_depth_flag and a float64 K.npy "
                                 "(use backend='host')")
            return "float64", self.depth_data.K
        if self.dataset == "google_earth" and not self.depth_data.convert_depth_flag:
            return ("half" if depth_dtype == np.float16 else "float32"), None
        raise ValueError(f"the device batch builder has no depth arithmetic for dataset {self.dataset!r} with convert_depth_flag "
                         f"{self.depth_data.convert_depth_flag} (use backend='host')")


class CustomTrain(CustomBase):
    split = "train"

    def __init__(self, image_resolution, images_list_file, use_depth, convert_depth_flag, dataset_dir, dataset, depth_range):
        self._init_paths(image_resolution, images_list_file, use_depth, convert_depth_flag, dataset_dir, dataset, depth_range)


class CustomValidation(CustomBase):
    """the list shuffled by seed 3 (a private generator: the process-wide one is left alone), first 2500 kept"""
    split = "val"

    def __init__(self, image_resolution, images_list_file, use_depth, convert_depth_flag, dataset_dir, dataset, depth_range):
        self._init_paths(image_resolution, images_list_file, use_depth, convert_depth_flag, dataset_dir, dataset, depth_range)


# ------------------------------------------------------------------------------------------------
# batch builder
# ------------------------------------------------------------------------------------------------
_SMALL_KEYS = ("Ks", "K_invs", "R_rels", "tgt_frame_id", "src_frame_ids", "t_rels", "src_masks")


class _Staging:
    """pinned host staging of one in-flight batch: decoded frames, depth maps, the packed small arrays"""

    def __init__(self, slots, hf, wf, n_small, depth=True):
        self.u8 = torch.empty((slots, hf, wf, 3), dtype=torch.uint8).pin_memory()
        self.depth = torch.empty((slots, hf, wf), dtype=torch.float32).pin_memory() if depth else None
        self.small = torch.empty((n_small,), dtype=torch.float32).pin_memory()
        self.uploaded = None            # event: the last upload from these buffers has been read by the device


class BatchBuilder:
    """Iterator of batch dicts over `dataset`: one pass per `iter()`.  `backend="host"`: the reference's per-sample
    arithmetic on CPU threads, collated (CPU tensors).  `backend="device"`: threads decode PNG / npy into pinned staging for
    the next batch while the caller trains on this one; one upload per staging tensor on the current stream, then
    csrc/imageio.hip writes the batch tensors (device tensors, equal to the host batch in bits).  Source choice always runs
    on the calling thread, in batch order, so a seeded dataset gives the same batches with any `workers`.
    The single-frame datasets (`CustomTrain` / `CustomValidation`) go the same way with one staging slot per sample: their
    batch is {"image": (B, H, W, C), "file_path_": list of str}, written by two launches on the device backend."""

    def __init__(self, dataset, batch_size, backend=None, shuffle=False, drop_last=False, workers=4, seed=None, device=None):
        if backend is None:
            backend = "device" if torch.cuda.is_available() else "host"
        if backend not in ("device", "host"):
            raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
        self.dataset, self.batch_size, self.backend = dataset, int(batch_size), backend
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.workers = max(1, min(int(workers), 16))
        self.seed = int(seed) if seed is not None else int.from_bytes(os.urandom(4), "little")
        self.device = torch.device(device if device is not None else "cuda") if backend == "device" else torch.device("cpu")
        self._pool = None
        self._epoch, self._pos, self._keep_position = -1, 0, False
        self._order = None
        self._pending = None             # the prefetched batch: (position, dataset RNG state before its plan, work)
        self._stage, self._turn = [None, None], 0
        self._single = bool(getattr(dataset, "single_frame", False))
        self._depth_dtype = None         # single frames: the dtype of the depth files, fixed by the first one
        # measurement (scripts/loader_time.py): prefetch off puts a batch's whole decode inside its own __next__;
        # decode_wait_ms = what the last __next__ waited for the decode threads; with time_device, device_events brackets its device part
        self.prefetch, self.time_device = True, False
        self.decode_wait_ms, self.device_events = 0.0, None

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    # ---- position ----
    def _epoch_order(self):
        n = len(self.dataset)
        return np.random.RandomState([self.seed, self._epoch]).permutation(n) if self.shuffle else np.arange(n)

    def __iter__(self):
        if self._keep_position:
            self._keep_position = False
        else:
            self._epoch, self._pos = self._epoch + 1, 0
        self._order = self._epoch_order()
        self._drop_pending()
        return self

    def _drop_pending(self):
        """forget the prefetched batch, once its decode threads have stopped writing into the staging buffers"""
        if self._pending is not None and self.backend == "device":
            for f in self._pending[2][1]:
                f.exception()
        self._pending = None

    def state_dict(self):
        """where the NEXT batch starts: epoch, batch position and the train split's RandomState before that batch's choice"""
        if self._pending is not None:
            pos, rng = self._pending[0], self._pending[1]
        else:
            pos, rng = self._pos, self._rng_state()
        return {"seed": self.seed, "epoch": self._epoch, "position": pos, "dataset_rng": rng}

    def load_state_dict(self, state):
        self.seed, self._epoch, self._pos = int(state["seed"]), int(state["epoch"]), int(state["position"])
        if state.get("dataset_rng") is not None:
            r = state["dataset_rng"]
            self.dataset.prng.set_state((r["name"], r["keys"].numpy().astype(np.uint32), r["pos"], r["has_gauss"], r["cached_gaussian"]))
        self._drop_pending()
        self._keep_position = True

    def _rng_state(self):
        """the train split's RandomState as plain tensors and numbers (a checkpoint stays loadable with `weights_only=True`)"""
        if self._single or self.dataset.split != "train":
            return None
        name, keys, pos, has_gauss, cached = self.dataset.prng.get_state()
        return {"name": name, "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                "cached_gaussian": float(cached)}

    # ---- pipeline ----
    def _submit(self, pos):
        if pos >= len(self):
            return None
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="sgam-decode")
        rng = self._rng_state()
        idx = self._order[pos * self.batch_size:(pos + 1) * self.batch_size]
        plans = [self.dataset.plan(int(i)) for i in idx]
        if self.backend == "host":
            work = self._submit_host(plans)
        else:
            work = self._submit_frames(plans) if self._single else self._submit_device(plans)
        return pos, rng, work

    def __next__(self):
        if self._order is None:
            iter(self)
        if self._pending is None or self._pending[0] != self._pos:
            self._pending = self._submit(self._pos)
        if self._pending is None:
            raise StopIteration
        _, _, work = self._pending
        if self.backend == "host":
            batch = self._finish_host(work)
        else:
            batch = self._finish_frames(work) if self._single else self._finish_device(work)
        self._pos += 1
        self._pending = self._submit(self._pos) if self.prefetch else None      # decode of the next batch overlaps the caller's step
        return batch

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host backend ----
    def _submit_host(self, plans):
        return [self._pool.submit(self.dataset.host_sample, p) for p in plans]

    def _finish_host(self, futures):
        import time
        t0 = time.perf_counter()
        samples = [f.result() for f in futures]
        self.decode_wait_ms = (time.perf_counter() - t0) * 1e3
        return {k: torch.from_numpy(np.stack([s[k] for s in samples])) if isinstance(samples[0][k], np.ndarray)
                else [s[k] for s in samples] for k in samples[0]}            # (strings collate to a list, like default_collate)

    # ---- device backend ----
    def _staging(self, B, plans):
        """the staging buffers of this turn, made on the first batch (the file size is only known from a decoded frame)"""
        ds, N = self.dataset, self.dataset.src_num
        st = self._stage[self._turn]
        if st is None or st.u8.shape[0] != self.batch_size * (1 + N):
            from PIL import Image
            with Image.open(plans[0]["tgt_rgb"]) as im:
                wf, hf = im.size
            ds.check_file_size(hf, wf)
            n_small = self.batch_size * (N * (9 + 9 + 9 + 3 + 1 + 1) + 1)
            st = self._stage[self._turn] = _Staging(self.batch_size * (1 + N), hf, wf, n_small)
        if st.uploaded is not None:
            st.uploaded.synchronize()       # the device has read the previous contents
        self._turn ^= 1
        return st

    def _decode_into(self, st, slot, rgb_path, depth_path, is_src):
        rgb, depth = self.dataset.decode(rgb_path, depth_path, is_src)
        if rgb.shape[:2] != tuple(st.u8.shape[1:3]) or depth.shape != tuple(st.depth.shape[1:]):
            raise ValueError(f"{rgb_path}: frame of {rgb.shape[:2]} / depth of {depth.shape} in a dataset of {tuple(st.u8.shape[1:3])}")
        st.u8[slot].numpy()[...] = rgb
        st.depth[slot].numpy()[...] = depth

    def _submit_device(self, plans):
        B, N = len(plans), self.dataset.src_num
        st = self._staging(B, plans)
        futures, padded = [], []
        for b, p in enumerate(plans):        # slots: [0, B) targets, then B * N sources, sample-major
            futures.append(self._pool.submit(self._decode_into, st, b, p["tgt_rgb"], p["tgt_depth"], False))
            for n in range(N):
                if n < len(p["srcs"]):
                    futures.append(self._pool.submit(self._decode_into, st, self.batch_size + b * N + n, p["src_rgb"][n],
                                                     p["src_depth"][n], True))
                else:
                    padded.append((b, n))
        small = [self.dataset.small_arrays(p) for p in plans]
        return st, futures, padded, small, B

    def _finish_device(self, work):
        import time

        from . import imageio
        st, futures, padded, small, B = work
        t0 = time.perf_counter()
        for f in futures:
            f.result()
        self.decode_wait_ms = (time.perf_counter() - t0) * 1e3
        ds, N, dev = self.dataset, self.dataset.src_num, self.device
        H, W = ds.image_resolution
        ge = ds.dataset_name == "google_earth"
        # the small arrays: float32 like the sample's final cast, packed into one upload
        keys = [k for k in _SMALL_KEYS if k in small[0]]
        parts = [np.stack([s[k] for s in small]).astype(np.float32) for k in keys]
        n_small = sum(a.size for a in parts)
        st.small.numpy()[:n_small] = np.concatenate([a.ravel() for a in parts])
        with torch.cuda.device(dev):
            slots = st.u8.shape[0]
            if self.time_device:
                self.device_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.device_events[0].record()
            u8 = st.u8.to(dev, non_blocking=True)
            depth = st.depth.to(dev, non_blocking=True)
            packed = st.small[:n_small].to(dev, non_blocking=True)
            st.uploaded = torch.cuda.Event()
            st.uploaded.record()
            batch, o = {}, 0
            for k, a in zip(keys, parts):
                batch[k] = packed[o:o + a.size].view(a.shape)
                o += a.size
            f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
            batch["dst_img"], batch["src_imgs"] = f32(B, H, W, 3), f32(B, N, H, W, 3)
            batch["dst_depth"], batch["src_depths"] = f32(B, H, W, 1), f32(B, N, H, W, 1)
            Bs = self.batch_size            # (a last, shorter batch uses the head of each slot range)
            imageio.resize_lanczos_u8(u8[:B], (H, W), out_f32=batch["dst_img"])
            imageio.resize_lanczos_u8(u8[Bs:Bs + B * N], (H, W), out_f32=batch["src_imgs"].view(B * N, H, W, 3))
            if ge:
                batch["tgt_pixel_mask"] = f32(B, 1, H, W)
                imageio.resize_nearest(depth[:B], (H, W), out=batch["dst_depth"].view(B, H, W),
                                       mask_out=batch["tgt_pixel_mask"].view(B, H, W))
                imageio.resize_nearest(depth[Bs:Bs + B * N], (H, W), out=batch["src_depths"].view(B * N, H, W),
                                       replace_sentinel=(SENTINEL, SENTINEL_REPLACEMENT))
            else:
                imageio.resize_nearest(depth[:B], (H, W), out=batch["dst_depth"].view(B, H, W))
                imageio.resize_nearest(depth[Bs:Bs + B * N], (H, W), out=batch["src_depths"].view(B * N, H, W))
            for b, n in padded:              # a target with fewer than n_src neighbours: the reference pads with zero frames
                batch["src_imgs"][b, n].zero_()
                batch["src_depths"][b, n].zero_()
            assert slots >= Bs + B * N
            if self.time_device:
                self.device_events[1].record()
        return {k: batch[k] for k in ds.KEYS}

    # ---- device backend, single frames: one slot per sample, two launches ----
    def _submit_frames(self, plans):
        ds = self.dataset
        st = self._stage[self._turn]
        if st is None:
            from PIL import Image
            with Image.open(plans[0]["rgb"]) as im:
                wf, hf = im.size
            if plans[0]["depth"] is not None:
                self._depth_dtype = np.load(plans[0]["depth"], mmap_mode="r").dtype
                ds.codec(self._depth_dtype)         # a combination the device has no arithmetic for fails here, before any thread
            st = self._stage[self._turn] = _Staging(self.batch_size, hf, wf, 1, depth=plans[0]["depth"] is not None)
        if st.uploaded is not None:
            st.uploaded.synchronize()
        self._turn ^= 1
        return st, [self._pool.submit(self._decode_frame_into, st, b, p) for b, p in enumerate(plans)], [ds.file_path(p) for p in plans]

    def _decode_frame_into(self, st, slot, p):
        rgb, depth, dtype = self.dataset.decode(p)
        if rgb.shape[:2] != tuple(st.u8.shape[1:3]) or (depth is not None and depth.shape != tuple(st.depth.shape[1:])):
            raise ValueError(f"{p['rgb']}: frame of {rgb.shape[:2]} / depth of {None if depth is None else depth.shape} in a dataset "
                             f"of {tuple(st.u8.shape[1:3])} (use backend='host')")
        if depth is not None and dtype != self._depth_dtype:
            raise ValueError(f"{p['depth']}: {dtype} depth map in a dataset of {self._depth_dtype} maps: the device batch builder "
                             "computes a whole batch in one arithmetic (use backend='host')")
        st.u8[slot].numpy()[...] = rgb
        if depth is not None:
            st.depth[slot].numpy()[...] = depth

    def _finish_frames(self, work):
        import time

        from . import imageio
        st, futures, paths = work
        t0 = time.perf_counter()
        for f in futures:
            f.result()
        self.decode_wait_ms = (time.perf_counter() - t0) * 1e3
        ds, dev, B = self.dataset, self.device, len(paths)
        H, W = ds.image_resolution
        C = 3 if st.depth is None else 4
        with torch.cuda.device(dev):
            if self.time_device:
                self.device_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.device_events[0].record()
            u8 = st.u8.to(dev, non_blocking=True)
            depth = None if st.depth is None else st.depth.to(dev, non_blocking=True)
            st.uploaded = torch.cuda.Event()
            st.uploaded.record()
            image = torch.empty((B, H, W, C), dtype=torch.float32, device=dev)
            imageio.resize_bicubic_u8(u8[:B], (H, W), out_f32=image, channels=C)
            if depth is not None:
                arith, K = ds.codec(self._depth_dtype)
                imageio.frame_depth_codec(depth[:B], (H, W), ds.dataset, arith, K=K, out=image, channel=3)
            if self.time_device:
                self.device_events[1].record()
        return {"image": image, "file_path_": paths}
