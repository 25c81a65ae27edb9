"""GPU: the point-splat RGB-D render (csrc/point_raster.hip: sgam_points_render_rgbd_f32 through pointview.render_points_rgbd) —
depth bits, rgb, uint8 and winning index equal to the numpy twin (tests/points_oracle.py) bit for bit at edge shapes, the tie
rule, a frame at its own pose, an address table beyond 64 frames, views above and below the source size — and the scene-level
caller render_views(source="points") on both warp branches."""
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import pointview, testing

sys.path.insert(0, os.path.dirname(__file__))
from test_pointview_cpu import check_identity, edge_case, identity_case, twin  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _upload(case):
    return ([torch.from_numpy(d).to(DEV) for d in case["depths"]], [torch.from_numpy(c).to(DEV) for c in case["rgbs"]])


def _render(case, dev, radius=0, hole_fill=False, T_rel=None):
    out = pointview.render_points_rgbd(dev[0], dev[1], case["K_src"], case["Ts_src"], case["K_view"], case["Ts_view"], case["H"],
                                       case["W"], case["z_near"], case["z_far"], radius=radius, hole_fill=hole_fill, T_rel=T_rel,
                                       index=True)
    assert all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def _same(got, want, what):
    assert set(got) == set(want) == {"depth", "rgb", "rgb_u8", "index"}
    assert np.array_equal(got["index"], want["index"]), what
    assert np.array_equal(_bits(got["depth"]), _bits(want["depth"])), what
    assert np.array_equal(_bits(got["rgb"]), _bits(want["rgb"])), what
    assert got["rgb_u8"].dtype == np.uint8 and np.array_equal(got["rgb_u8"], want["rgb_u8"]), what


@pytest.fixture(scope="module")
def edge():
    case = edge_case()
    T_rel = pointview.relative_transforms(case["Ts_view"], case["Ts_src"])
    return case, _upload(case), T_rel


@pytest.mark.parametrize("hole_fill", [False, True])
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_edge_shapes_equal_the_twin(edge, radius, hole_fill):
    case, dev, T_rel = edge
    got = _render(case, dev, radius, hole_fill, T_rel=T_rel)
    assert got["depth"].shape == (2, 37, 53) and got["rgb"].shape == got["rgb_u8"].shape == (2, 37, 53, 3)
    want = twin(case, radius, hole_fill, T_rel=T_rel)
    assert (want["index"] >= 0).mean() > 0.2
    _same(got, want, (radius, hole_fill))


def test_exact_ties_go_to_the_earlier_frame():
    one = edge_case(F=1, P=1)
    case = dict(one, depths=one["depths"] * 2, rgbs=[one["rgbs"][0], 255 - one["rgbs"][0]], Ts_src=one["Ts_src"] * 2)
    dev = _upload(case)
    Hs, Ws = case["depths"][0].shape
    for radius in (0, 1):
        got = _render(case, dev, radius)
        hit = got["depth"] > 0
        assert hit.sum() > 200 and (got["index"][hit] < Hs * Ws).all() and (got["index"][~hit] == -1).all()
        _same(got, twin(case, radius), radius)
        again = _render(case, dev, radius)
        assert all(np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)) for k in got)


def test_a_frame_at_its_own_pose_reproduces_itself():
    case = identity_case("google_earth", 64, 64, seed=2)
    got = _render(case, _upload(case))
    check_identity(case, got)
    _same(got, twin(case), "identity")


def test_address_tables_beyond_64_frames():
    case = edge_case(F=70, Hs=8, Ws=8, P=1, H=45, W=43, seed=11)
    got = _render(case, _upload(case), radius=1, hole_fill=True)
    want = twin(case, 1, True)
    frames_seen = np.unique(want["index"][want["index"] >= 0] // 64)
    assert len(frames_seen) > 64 and (frames_seen >= 64).sum() >= 4             # frames beyond the 64th are seen
    _same(got, want, "F=70")


@pytest.mark.parametrize("size", [(16, 16), (96, 80)])
def test_views_below_and_above_the_source_size(size):
    case = edge_case(H=size[0], W=size[1], seed=5)
    for radius, hole_fill in ((0, True), (2, False)):
        _same(_render(case, _upload(case), radius, hole_fill), twin(case, radius, hole_fill), (size, radius, hole_fill))


# ---------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def model(golden):
    """the synthetic-weights model of test_gpu_flythrough.test_scene_fly_through"""
    from sgam_neurips22_amd.config import default_params
    from sgam_neurips22_amd.generative_sensing_module.model import VQModel
    g = golden("vqgan_full_ge256.npz")
    m = VQModel(**default_params("google_earth"))
    sd = testing.synthetic_state_dict(m.state_dict(), seed=0)
    sd["quantize.embedding.weight"] = testing.codebook_from_stats(float(g["zmean"]), float(g["zstd"]), 4096, 256, int(g["cb_seed"]))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _scene(model, **kw):
    from sgam_neurips22_amd.inference_pipeline import InfiniteSceneGeneration, synthetic_seed_frame
    scene = InfiniteSceneGeneration(model, "google_earth", output_dim=(4, 1), seed_frame=synthetic_seed_frame("google_earth", 0), **kw)
    scene.scene_expansion()
    assert len(scene.frames) == 4
    return scene


def test_views_of_a_splat_branch_scene(model, tmp_path):
    from PIL import Image
    splat = _scene(model)
    assert not splat.use_rgbd_integration and splat.volume is None
    poses = splat.flythrough_poses(n_between=1)
    assert poses.shape == (7, 4, 4)
    out = splat.render_views(poses, source="points", out_dir=str(tmp_path))
    assert set(out) == {"rgb", "depth", "rgb_u8"}
    assert out["rgb"].shape == (7, 256, 256, 3) and out["rgb"].dtype == torch.float32
    assert out["depth"].shape == (7, 256, 256) and out["depth"].dtype == torch.float32
    assert out["rgb_u8"].shape == (7, 256, 256, 3) and out["rgb_u8"].dtype == torch.uint8
    assert all(t.is_cuda for t in out.values())
    assert (out["depth"] > 0).float().mean().item() > 0.3
    assert sorted(os.listdir(tmp_path)) == sorted([f"view_{p:04d}.png" for p in range(7)] + [f"view_depth_{p:04d}.npy" for p in range(7)])
    for p in range(7):
        img = np.array(Image.open(tmp_path / f"view_{p:04d}.png"))
        assert img.dtype == np.uint8 and np.array_equal(img, out["rgb_u8"][p].cpu().numpy())
        assert np.array_equal(np.load(tmp_path / f"view_depth_{p:04d}.npy"), out["depth"][p].cpu().numpy())
    z0, z1 = (f32(z) for z in splat._Z_RANGE["google_earth"])
    coords = [c for c in splat._ordered_grid_coords]
    own = np.stack([splat.transform_grid[c[0]][c[1]]["T"] for c in coords])
    assert np.array_equal(own, poses[::2])
    raw = splat.render_views(own, source="points", point_radius=0, hole_fill=False)["depth"].cpu().numpy()
    for k, c in enumerate(coords):
        stored = splat.frames[c]["depth"].cpu().numpy()
        ok = np.isfinite(stored) & (stored >= z0) & (stored <= z1)
        assert ok.sum() > 1000
        # the frame's own point lands on its own pixel and the z-test keeps the minimum: both exact
        assert (raw[k][ok] > 0).all() and (raw[k][ok] <= stored[ok]).all()
        alone = splat.render_views(own[k:k + 1], source="points", point_radius=0, hole_fill=False, frames=[c])
        assert np.array_equal(_bits(alone["depth"][0].cpu().numpy()[ok]), _bits(stored[ok]))
        assert np.array_equal(alone["rgb_u8"][0].cpu().numpy()[ok], splat.frames[c]["rgb_u8"].cpu().numpy()[ok])
    with pytest.raises(ValueError, match="no stored frame"):
        splat.render_views(own[:1], source="points", frames=[(9, 9)])
    # the other sources are what they were: a splat scene has no volume to render, an unknown source is refused
    with pytest.raises(ValueError, match="rgbd_integration branch"):
        splat.render_views(poses)
    with pytest.raises(ValueError, match="rgbd_integration branch"):
        splat.render_views(poses, source="raycast")
    with pytest.raises(ValueError, match="not 'surfels'"):
        splat.render_views(poses, source="surfels")


def test_views_of_an_rgbd_branch_scene_survive_an_overwritten_source(model):
    scene = _scene(model, use_rgbd_integration=True, tsdf_memory_budget_bytes=1 << 30)
    poses = scene.flythrough_poses(n_between=1)
    out = scene.render_views(poses, source="points")
    assert out["rgb"].shape == (7, 256, 256, 3) and out["depth"].shape == (7, 256, 256) and out["rgb_u8"].dtype == torch.uint8
    assert all(t.is_cuda for t in out.values()) and (out["depth"] > 0).float().mean().item() > 0.3
    half = scene.render_views(poses[:2], source="points", point_radius=1, H=128, W=128)
    assert half["rgb"].shape == (2, 128, 128, 3) and (half["depth"] > 0).float().mean().item() > 0.3
    c0 = scene._ordered_grid_coords[0]
    scene.save_to_store(c0, *[scene.frames[c0][k] for k in ("rgb_u8", "rgb_f", "depth")])
    with pytest.raises(ValueError, match="overwritten"):
        scene.render_views(poses, source="mesh")
    again = scene.render_views(poses, source="points")             # (the overwritten frame now comes last: only exact z ties could tell)
    assert torch.equal(again["depth"], out["depth"]) and again["rgb_u8"].shape == out["rgb_u8"].shape
