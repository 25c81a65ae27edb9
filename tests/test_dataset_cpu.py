"""CPU: the training data path without a GPU (sgam_neurips22_amd/datasets.py, imageio.lanczos_tables, data.utils.utils): the
fixed-point oracle against PIL, the `host` backend against an in-test transcription of the reference's `__getitem__`
arithmetic, the neighbour rules on hand-built poses, source choice, and the data module on the shipped training configs'
`data.params` (tests/golden/train_configs/: settings only).  Everything is exact equality."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml
from PIL import Image

import resize_oracle
from sgam_neurips22_amd import datasets, imageio, testing

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [((512, 512), (256, 256)), ((300, 410), (256, 256)), ((64, 64), (256, 256)), ((512, 512), (100, 37))]
GL2CV = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]])


def extreme_images(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    return [np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8), checker]


def pil_resize(img, size):
    return np.array(Image.fromarray(img).resize((size[1], size[0]), resample=Image.LANCZOS))


@pytest.mark.parametrize("src,dst", SIZES)
def test_fixed_point_oracle_equals_pil(src, dst):
    rs = np.random.RandomState(1)
    for img in [rs.randint(0, 256, src + (3,), dtype=np.uint8)] + extreme_images(*src):
        assert np.array_equal(resize_oracle.resize_lanczos_u8(img, dst), pil_resize(img, dst))


@pytest.mark.parametrize("n_in,n_out", [(512, 256), (410, 256), (64, 256), (512, 37), (256, 256)])
def test_kernel_tables_equal_the_oracle_coefficients(n_in, n_out):
    """the tables the device kernel reads (imageio.lanczos_tables) are the oracle's coefficients; their int32 sums cannot overflow"""
    bounds, coef = imageio.lanczos_tables(n_in, n_out)
    ref = resize_oracle.axis_coefficients(n_in, n_out)
    assert bounds.dtype == coef.dtype == np.int32 and bounds.shape == (n_out, 2)
    for i, (lo, k) in enumerate(ref):
        assert bounds[i, 0] == lo and bounds[i, 1] == len(k) <= coef.shape[1]
        assert np.array_equal(coef[i, :len(k)], k) and not coef[i, len(k):].any()
    assert (np.abs(coef.astype(np.int64)).sum(1) * 255 + (1 << 21) < 2 ** 31).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()      # what the kernel's tile window relies on


# ---- the reference's __getitem__ arithmetic, transcribed: brute-force graph, per-sample float64 numpy, PIL, F.interpolate ----
def ref_nodes(dataset_dir, split, scene, kind):
    frames = json.load(open(os.path.join(dataset_dir, split, scene, "transforms.json")))["frames"]
    nodes = {}
    for i, fr in enumerate(frames):
        c2w = np.array(fr["transform_matrix"]) @ GL2CV
        w2c = np.linalg.inv(c2w)
        if kind == "google_earth":
            if not fr["is_valid"]:
                continue
            key = int(fr["file_path"][-9:-4])
        else:
            key = i
        nodes[key] = {"R": w2c[:3, :3], "t": w2c[:3, 3], "position": c2w[:3, 3],
                      "rgb": os.path.join(dataset_dir, split, scene, f"im_{key:05d}.png"),
                      "depth": os.path.join(dataset_dir, split, scene, f"dm_{key:05d}.npy")}
        if kind == "google_earth" and len(nodes) == 900 and split != "train":
            break
    edges = {k: [] for k in nodes}
    keys = sorted(nodes)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            i, j = keys[a], keys[b]
            if kind == "google_earth" and i % 4 != j % 4:
                continue
            if np.linalg.norm(nodes[i]["position"] - nodes[j]["position"]) <= (0.3 if kind == "google_earth" else 3):
                edges[i].append(j)
                edges[j].append(i)
    if kind == "google_earth":
        nodes = {k: v for k, v in nodes.items() if edges[k]}
    return nodes, edges


def ref_sample(dataset_dir, split, kind, res, n_src, global_index):
    """val / test split sample `global_index` the way the reference computes it"""
    scenes = sorted(os.listdir(os.path.join(dataset_dir, split)))
    off = 0
    for scene in scenes:
        nodes, edges = ref_nodes(dataset_dir, split, scene, kind)
        if global_index < off + len(nodes):
            break
        off += len(nodes)
    key = sorted(nodes)[global_index - off]
    nb = np.array(sorted(edges[key]))
    np.random.RandomState(seed=global_index).shuffle(nb)
    srcs = [nodes[k] for k in nb[:n_src]]
    ids = [int(k) for k in nb[:n_src]]
    K = np.load(os.path.join(dataset_dir, "K.npy"))
    img_dst = Image.open(nodes[key]["rgb"])
    img_srcs = [Image.open(s["rgb"]) for s in srcs]
    dm_dst = np.load(nodes[key]["depth"])
    dm_srcs = [np.load(s["depth"]) for s in srcs]
    if kind == "google_earth":
        K[0] = K[0] * res[1] / 512
        K[1] = K[1] * res[0] / 512
        h, w = img_dst.size[:2]
        if res[0] != h or res[1] != w:
            img_srcs = [im.resize((res[1], res[0]), resample=Image.LANCZOS) for im in img_srcs]
            img_dst = img_dst.resize((res[1], res[0]), resample=Image.LANCZOS)
            dm_srcs = [F.interpolate(torch.from_numpy(d[None, None]), size=res)[0][0].numpy() for d in dm_srcs]
            dm_dst = F.interpolate(torch.from_numpy(dm_dst[None, None]), size=res)[0][0].numpy()
        img_dst = np.array(img_dst) / 127.5 - 1.0
        img_srcs = [np.array(im) / 127.5 - 1.0 for im in img_srcs]
        for d in dm_srcs:
            d[d == 65504] = -99999
        dm_dst_out, dm_srcs_out = dm_dst[..., None], None
    else:
        img_dst = np.array(img_dst) / 127.5 - 1.0
        img_srcs = [np.array(im) / 127.5 - 1.0 for im in img_srcs]
        h, w = dm_dst.shape[:2]
        xs, ys = np.meshgrid(np.linspace(0, w - 1, w), np.linspace(0, h - 1, h))
        conv = lambda d: (d * K[0][0] / np.sqrt(K[0][0] ** 2 + (K[0][2] - ys - 0.5) ** 2 + (K[1][2] - xs - 0.5) ** 2))[..., None]  # noqa: E731
        dm_dst_out, dm_srcs = conv(dm_dst), [conv(d) for d in dm_srcs]
        h, w = img_dst.shape[:2]
        K = K * res[1] / w
        K = K * res[0] / h
    T_tgt = np.eye(4)
    T_tgt[:3, :3], T_tgt[:3, 3] = nodes[key]["R"], nodes[key]["t"]
    Ks, K_invs, R_rels, t_rels = [], [], [], []
    for s in srcs:
        T_src = np.eye(4)
        T_src[:3, :3], T_src[:3, 3] = s["R"], s["t"]
        T_rel = T_tgt @ np.linalg.inv(T_src)
        R_rels.append(T_rel[:3, :3])
        t_rels.append(T_rel[:3, 3])
        Ks.append(K)
        K_invs.append(np.linalg.inv(K))
    mask = np.zeros(n_src)
    mask[:n_src] = 1
    while len(K_invs) < n_src:
        Ks.append(np.eye(3))
        K_invs.append(np.eye(3))
        R_rels.append(np.eye(3))
        t_rels.append(np.zeros(3))
        img_srcs.append(np.zeros_like(img_srcs[-1]))
        dm_srcs.append(np.zeros_like(dm_srcs[-1]))
        ids.append(-1)
    ex = {"Ks": np.stack(Ks), "K_invs": np.stack(K_invs), "R_rels": np.stack(R_rels), "t_rels": np.stack(t_rels), "dst_img": img_dst,
          "src_imgs": np.stack(img_srcs), "dst_depth": dm_dst_out, "src_masks": mask}
    if kind == "google_earth":
        ex.update({"tgt_frame_id": np.array([key]), "src_frame_ids": np.array(ids), "src_depths": np.stack(dm_srcs)[..., None],
                   "tgt_pixel_mask": (dm_dst != 65504)[None]})
    else:
        ex["src_depths"] = np.stack(dm_srcs)
    return {k: v.astype(np.float32) for k, v in ex.items()}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kind,size,res,n_src", [("google_earth", 48, [32, 32], 1), ("google_earth", 48, [32, 32], 3),
                                                 ("clevr-infinite", 32, [32, 32], 2)])
def test_host_batch_equals_the_transcribed_reference(tmp_path, kind, size, res, n_src):
    """every key of the host sample and of the collated host batch, in bits and dtype (GoogleEarth resized 48 -> 32 with 65504
    in some depth maps and, at n_src = 3, targets with fewer neighbours than sources: the padding entries; CLEVR at native size)"""
    root = testing.synth_dataset_dir(tmp_path / "ds", kind, size=size)
    cls = datasets.GoogleEarthValidation if kind == "google_earth" else datasets.Blender3dValidation
    ds = cls(dataset_dir=root, dataset=kind, image_resolution=res, n_src=n_src)
    want = [ref_sample(root, "val", kind, res, n_src, i) for i in range(len(ds))]
    assert len(ds) == 24
    if kind == "google_earth":
        assert any((w["src_depths"] == -99999).any() for w in want) and any((w["tgt_pixel_mask"] == 0).any() for w in want)
        assert (n_src == 3) == any((w["src_frame_ids"] == -1).any() for w in want)
    for i, w in enumerate(want):
        got = ds[i]
        assert list(got) == list(ds.KEYS) and set(got) == set(w)
        for k in w:
            assert same_bits(got[k], w[k]), (i, k)
    loader = datasets.BatchBuilder(ds, 4, backend="host", workers=3)
    batches = list(loader)
    loader.close()
    assert len(batches) == len(loader) == 6
    for b, batch in enumerate(batches):
        for k in batch:
            assert batch[k].dtype == torch.float32
            assert same_bits(batch[k].numpy(), np.stack([want[4 * b + j][k] for j in range(4)])), (b, k)


def test_clevr_other_resolution_is_a_clear_error(tmp_path):
    root = testing.synth_dataset_dir(tmp_path / "ds", "clevr-infinite", size=32, splits=("val",))
    ds = datasets.Blender3dValidation(dataset_dir=root, dataset="clevr-infinite", image_resolution=[16, 16], n_src=1)
    with pytest.raises(ValueError, match="no working resize"):
        ds[0]


# ---- graph rules on hand-built poses ----
def write_scene(root, split, scene, positions, ids=None, valid=None):
    d = os.path.join(root, split, scene)
    os.makedirs(d, exist_ok=True)
    frames = []
    for i, p in enumerate(positions):
        c2w = np.eye(4)
        c2w[:3, 3] = p
        fid = i if ids is None else ids[i]
        frames.append({"file_path": f"./im_{fid:05d}.png", "is_valid": True if valid is None else bool(valid[i]),
                       "transform_matrix": c2w.tolist()})
    json.dump({"frames": frames}, open(os.path.join(d, "transforms.json"), "w"))
    np.save(os.path.join(root, "K.npy"), np.eye(3))


def test_google_earth_graph_rules(tmp_path):
    root = str(tmp_path)
    #            0: near 4 (same class)   1: near 0 in space, other class   4: exactly 0.3 from 0   8: 0.3000001 from 4 -> only via 4? no
    pos = {0: (0, 0, 0), 1: (0.01, 0, 0), 4: (0.3, 0, 0), 8: (0.7, 0, 0), 5: (0.05, 0, 0), 12: (0.3, 0.3000001, 0), 16: (9, 9, 9),
           20: (0.3, 0.1, 0)}
    ids = sorted(pos)
    valid = [i != 20 for i in ids]                                   # 20 would be a neighbour of 0, 4 and 12: it is invalid
    write_scene(root, "val", "plain", [pos[i] for i in ids], ids, valid)
    write_scene(root, "val", "chicago_1", [(0, 0, 0), (0.1, 0, 0)], [0, 4])
    ds = datasets.GoogleEarthValidation(dataset_dir=root, dataset="google_earth", image_resolution=[32, 32], n_src=1)
    assert len(ds.grids) == 1                                        # the chicago scene is skipped
    g = ds.grids[0]
    # 0 - 4 at exactly 0.3 are neighbours (<=); 1 - 5 share a class and are 0.04 apart; 0 - 1 are 0.01 apart but differ mod 4;
    # 12 is 0.3000001 from 4: no edge, no other neighbour -> dropped with the isolated 8 and 16
    assert g.keys == [0, 1, 4, 5]
    assert {k: list(v) for k, v in g.neighbours.items()} == {0: [4], 1: [5], 4: [0], 5: [1]}
    assert len(ds) == 4 and ds.parse_idx(2) == (0, 4)


def test_google_earth_900_cap_off_train(tmp_path):
    root = str(tmp_path)
    pos = [(0.001 * (i // 4), 0, 0) for i in range(1000)]
    for split in ("train", "val"):
        write_scene(root, split, "big", pos)
    val = datasets.GoogleEarthValidation(dataset_dir=root, dataset="google_earth", image_resolution=[32, 32], n_src=1)
    train = datasets.GoogleEarthTrain(dataset_dir=root, dataset="google_earth", image_resolution=[32, 32], n_src=1)
    assert len(val) == 900 and max(val.grids[0].keys) == 899 and len(train) == 1000
    assert max(max(v) for v in val.grids[0].neighbours.values()) == 899


def test_clevr_graph_threshold(tmp_path):
    root = str(tmp_path)
    write_scene(root, "val", "s", [(0, 0, 0), (3, 0, 0), (6.0000001, 0, 0), (50, 0, 0)])
    ds = datasets.Blender3dValidation(dataset_dir=root, dataset="clevr-infinite", image_resolution=[32, 32], n_src=1)
    assert {k: list(v) for k, v in ds.grids[0].neighbours.items()} == {0: [1], 1: [0], 2: [], 3: []}
    assert len(ds) == 4                                              # CLEVR keeps isolated frames, like the reference


def test_source_choice(tmp_path):
    root = testing.synth_dataset_dir(tmp_path / "ds", "google_earth", size=16)
    kw = dict(dataset_dir=root, dataset="google_earth", image_resolution=[16, 16], n_src=2)
    val = datasets.GoogleEarthValidation(**kw)
    assert [val.choose(i)[1:] for i in range(len(val))] == [val.choose(i)[1:] for i in range(len(val))]
    a, b = datasets.GoogleEarthTrain(seed=7, **kw), datasets.GoogleEarthTrain(seed=7, **kw)
    first = [a.choose(i)[2] for i in range(len(a))]
    assert first == [b.choose(i)[2] for i in range(len(b))]
    assert first != [a.choose(i)[2] for i in range(len(a))]           # the train split keeps drawing
    c = datasets.GoogleEarthTrain(seed=8, **kw)
    assert first != [c.choose(i)[2] for i in range(len(c))]
    # the draw is prng.choice(len(neighbours), n_src) from RandomState(seed), in call order
    rs = np.random.RandomState(7)
    d = datasets.GoogleEarthTrain(seed=7, **kw)
    for i in range(4):
        scene, key, srcs = d.choose(i)
        nb = sorted(scene.neighbours[key])
        assert srcs == [nb[k] for k in rs.choice(len(nb), 2)]


def test_seeded_loader_is_reproducible_and_resumable(tmp_path):
    root = testing.synth_dataset_dir(tmp_path / "ds", "google_earth", size=16)
    kw = dict(dataset_dir=root, dataset="google_earth", image_resolution=[16, 16], n_src=1)

    def ids(loader, n):
        it, out = iter(loader), []
        while len(out) < n:
            try:
                b = next(it)
            except StopIteration:
                it = iter(loader)
                continue
            out.append((b["tgt_frame_id"].flatten().tolist(), b["src_frame_ids"].flatten().tolist()))
        return out

    mk = lambda: datasets.BatchBuilder(datasets.GoogleEarthTrain(seed=3, **kw), 5, backend="host", shuffle=True, seed=11, workers=2)  # noqa: E731
    full = ids(mk(), 9)                                  # crosses an epoch boundary (24 samples, 5 batches per epoch)
    assert full == ids(mk(), 9)
    first = mk()
    head = ids(first, 3)
    state = first.state_dict()
    second = mk()
    second.load_state_dict(state)
    assert head + ids(second, 6) == full
    assert sorted(sum((t for t, _ in full[:5]), [])) == sorted(sum((t for t, _ in ids(datasets.BatchBuilder(
        datasets.GoogleEarthTrain(seed=3, **kw), 5, backend="host"), 5)), []))       # an epoch visits every sample once


def test_data_module_accepts_the_shipped_training_configs(tmp_path):
    from data.utils.utils import DataModuleFromConfig
    from sgam_neurips22_amd.config import instantiate_from_config
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "train_configs", "*.yaml")))
    assert len(paths) == 4
    for path in paths:
        cfg = yaml.safe_load(open(path))
        assert cfg["data"]["target"] == "data.utils.utils.DataModuleFromConfig"
        params = dict(cfg["data"]["params"])
        dm = DataModuleFromConfig(**params)
        assert dm.batch_size == params["batch_size"]
        if params["phase"] == "codebook":
            with pytest.raises(NotImplementedError, match="custom_codebook"):
                dm.setup()
            continue
        size = 16
        params["dataset_dir"] = testing.synth_dataset_dir(tmp_path / params["dataset"], params["dataset"], size=size)
        if params["dataset"] == "clevr-infinite":
            params["image_resolution"] = [size, size]
        dm = instantiate_from_config({"target": cfg["data"]["target"], "params": dict(params, backend="host")})
        tl, vl = dm.train_dataloader(), dm.val_dataloader()
        assert tl.shuffle and not vl.shuffle and vl.drop_last and type(dm.test_dataloader().dataset) is type(vl.dataset)
        assert type(tl.dataset).__name__ in ("GoogleEarthTrain", "Blender3dTrain") and tl.dataset.src_num == params["n_src"]
        batch = next(iter(tl))
        B, N = params["batch_size"], params["n_src"]
        H, W = params["image_resolution"]
        assert batch["dst_img"].shape == (B, H, W, 3) and batch["src_imgs"].shape == (B, N, H, W, 3)
        assert batch["dst_depth"].shape == (B, H, W, 1) and batch["src_depths"].shape == (B, N, H, W, 1)
        assert batch["Ks"].shape == batch["K_invs"].shape == batch["R_rels"].shape == (B, N, 3, 3) and batch["t_rels"].shape == (B, N, 3)
        tl.close()


def test_reference_import_paths():
    import importlib
    assert importlib.import_module("data.google_earth").GoogleEarthTrain is datasets.GoogleEarthTrain
    assert importlib.import_module("data.clevr-infinite").Blender3dValidation is datasets.Blender3dValidation


def test_google_earth_val_samples_equal_the_reference_fixture(tmp_path, golden):
    """samples recorded from the reference's own GoogleEarthValidation on the same seeded files (tests/golden/gen_golden_dataset.py)"""
    g = golden("dataset_ge_val.npz")
    root = testing.synth_dataset_dir(tmp_path / "ds", kind="google_earth", size=24, frames=12, splits=("val",), seed=21,
                                     scenes=("alpha_scene", "bravo_scene"))
    ds = datasets.GoogleEarthValidation(dataset_dir=root, dataset="google_earth", image_resolution=[16, 16], n_src=2)
    assert len(ds) == int(g["length"])
    indices = sorted({int(f.split(".")[0]) for f in g.files if "." in f})
    assert len(indices) == 4
    for i in indices:
        got = ds[i]
        assert set(got) == {f.split(".", 1)[1] for f in g.files if f.startswith(f"{i}.")}
        for k, v in got.items():
            assert same_bits(v, g[f"{i}.{k}"]), (i, k)
