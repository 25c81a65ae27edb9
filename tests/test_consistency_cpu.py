"""CPU: the reprojection view-consistency rule (csrc/view_consistency.hip) as tests/consistency_oracle.py restates it, against
cases derived by hand — the twin's outside reference — and a class picture predicted from the rule; geometry.consistency_summary's
arithmetic with its NaN and inf cases; the argument checks of the C entry points and of the Python front, none of which needs a GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

from sgam_neurips22_amd import _lib, geometry
from sgam_neurips22_amd.ops import SgamHipError

sys.path.insert(0, os.path.dirname(__file__))
import consistency_oracle as CO  # noqa: E402

# the hand cases: every number below is a dyadic rational, so every fp32 step of the rule is exact
K_HAND = np.array([[16.0, 0, 8], [0, 16.0, 4], [0, 0, 1]])
H_HAND, W_HAND = 8, 16
Z_HAND = (1.0, 4.0)
TAU_HAND = 0.05
TX = 0.28125                    # fx * TX / depth = 16 * 0.28125 / 2 = 2.25 pixels
TX_WRONG = 0.0625               # another half pixel


def camera_at(x=0.0, y=0.0, z=0.0):
    """world -> camera of a camera without rotation whose centre is at (x, y, z)"""
    T = np.eye(4)
    T[:3, 3] = [-x, -y, -z]
    return T


def hand_frames():
    """the source (R = 4 j) and the same ramp seen again from a camera moved by TX: R = 4 j' + 9; depth 2 everywhere"""
    depth = np.full((H_HAND, W_HAND), 2.0, np.float32)
    j = np.arange(W_HAND)
    src = np.zeros((H_HAND, W_HAND, 3), np.uint8)
    src[..., 0] = 4 * j
    src[..., 1] = 10 * np.arange(H_HAND)[:, None]
    src[..., 2] = 77
    tgt = src.copy()
    tgt[..., 0] = 4 * j + 9
    return depth, src, tgt


def hand_pair(T_s, T_t):
    depth, src, tgt = hand_frames()
    return CO.pair(depth, src, depth, tgt, K_HAND, CO.relative_pose(T_s, T_t), *Z_HAND, TAU_HAND)


def test_identical_poses():
    depth, src, _ = hand_frames()
    cls, ce, ez, sums = CO.pair(depth, src, depth, src, K_HAND, CO.relative_pose(np.eye(4), np.eye(4)), *Z_HAND, TAU_HAND)
    assert sums[CO.COVISIBLE] == (H_HAND - 1) * (W_HAND - 1) and sums[CO.OUT_OF_VIEW] == H_HAND + W_HAND - 1
    assert sums[:7].sum() == H_HAND * W_HAND and (cls[-1] == CO.OUT_OF_VIEW).all() and (cls[:, -1] == CO.OUT_OF_VIEW).all()
    assert (cls[:-1, :-1] == CO.COVISIBLE).all()
    assert not ce.any() and not ez.any() and not sums[7:].any()


def test_ramp_seen_from_a_moved_camera():
    cls, ce, ez, sums = hand_pair(camera_at(), camera_at(x=TX))
    assert sums[CO.COVISIBLE] == (H_HAND - 1) * (W_HAND - 3)
    assert (cls[:-1, 3:] == CO.COVISIBLE).all() and (cls[:, :3] == CO.OUT_OF_VIEW).all() and (cls[-1] == CO.OUT_OF_VIEW).all()
    assert not ce.any() and not ez.any() and not sums[7:].any()


def test_half_a_pixel_of_pose_error_is_two_grey_levels_and_the_correction_takes_it_out():
    T_t, T_wrong = camera_at(x=TX), camera_at(x=TX + TX_WRONG)
    cls, ce, ez, sums = hand_pair(camera_at(), T_wrong)
    cov = cls == CO.COVISIBLE
    assert cov.sum() == sums[CO.COVISIBLE] > 0 and (ce[cov] == 2.0).all() and not ce[~cov].any() and not ez.any()
    s = CO.summary(sums)
    assert s["color_mae"] == 2.0 / 3.0 and sums[7] == 2.0 * cov.sum() and sums[8] == 4.0 * cov.sum() and s["depth_mae"] == 0.0
    assert s["psnr"] == 10.0 * math.log10(255.0 ** 2 * 3.0 / 4.0)
    # the world-frame correction of the frame whose pose is wrong, applied as T_wrong C^-1
    C = np.linalg.inv(T_t) @ T_wrong
    fixed = T_wrong @ np.linalg.inv(C)
    assert np.array_equal(fixed, T_t)
    cls2, ce2, ez2, sums2 = hand_pair(camera_at(), fixed)
    assert sums2[CO.COVISIBLE] == (H_HAND - 1) * (W_HAND - 3) and not ce2.any() and not ez2.any() and not sums2[7:].any()
    assert CO.summary(sums2)["psnr"] == math.inf


def predicted_class(target, i, j, H, W, tau):
    """the rule at identity pose with source depth 2: pixel (i, j) lands exactly on (i, j), so Dn = D00 = target[i][j]"""
    if i > H - 2 or j > W - 2:
        return CO.OUT_OF_VIEW

    def valid(x):
        return math.isfinite(x) and Z_HAND[0] <= x <= Z_HAND[1]
    if not valid(target[i, j]):
        return CO.TARGET_HOLE
    if 2.0 - target[i, j] > tau:
        return CO.OCCLUDED
    if target[i, j] - 2.0 > tau:
        return CO.VIOLATION
    corners = [target[i, j], target[i, j + 1], target[i + 1, j], target[i + 1, j + 1]]
    return CO.COVISIBLE if all(valid(c) and abs(2.0 - c) <= tau for c in corners) else CO.EDGE


def class_picture():
    H, W = 12, 16
    target = np.full((H, W), 2.0, np.float32)
    target[1:3, 1:4] = 1.0              # nearer than the source's points: they are hidden behind it
    target[1:3, 6:9] = 3.5              # farther: the target sees through the source's points
    target[5:7, 2:5] = np.nan
    target[8, 8] = np.inf
    target[8, 12] = 0.0
    target[4, 12] = 2.04                # within tau: still covisible
    return H, W, target


def test_class_picture():
    H, W, target = class_picture()
    src = np.full((H, W), 2.0, np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    cls, ce, ez, sums = CO.pair(src, rgb, target, rgb, K_HAND, CO.relative_pose(np.eye(4), np.eye(4)), *Z_HAND, TAU_HAND)
    want = np.array([[predicted_class(target, i, j, H, W, TAU_HAND) for j in range(W)] for i in range(H)], np.uint8)
    assert np.array_equal(cls, want)
    # and spelled out: the blocks, the EDGE ring round the single bad corners, the last row and column
    assert (cls[1:3, 1:4] == CO.OCCLUDED).all() and (cls[1:3, 6:9] == CO.VIOLATION).all() and (cls[5:7, 2:5] == CO.TARGET_HOLE).all()
    for r, c in ((8, 8), (8, 12)):
        assert cls[r, c] == CO.TARGET_HOLE
        assert cls[r - 1, c - 1] == cls[r - 1, c] == cls[r, c - 1] == CO.EDGE
        assert cls[r + 1, c] == cls[r, c + 1] == cls[r + 1, c + 1] == cls[r - 2, c] == CO.COVISIBLE
    assert cls[0, 0] == CO.EDGE and cls[0, 4] == CO.COVISIBLE and cls[3, 2] == CO.COVISIBLE and cls[4, 1] == CO.EDGE
    assert (cls[-1] == CO.OUT_OF_VIEW).all() and (cls[:, -1] == CO.OUT_OF_VIEW).all()
    assert all(sums[k] == (want == k).sum() for k in range(7)) and sums[CO.INVALID] == 0
    # covisible next to the 2.04 corner: the bilinear depth is taken at weight 0, so the error is the corner's own
    assert cls[4, 12] == CO.COVISIBLE and ez[4, 12] == np.float32(2.0) - np.float32(2.04) and ez[4, 11] == 0.0
    # an invalid SOURCE depth is class 0 whatever the target holds
    src2 = src.copy()
    src2[0, 0], src2[0, 1], src2[0, 2], src2[0, 3] = np.nan, 0.5, -np.inf, 4.5
    cls2 = CO.pair(src2, rgb, target, rgb, K_HAND, CO.relative_pose(np.eye(4), np.eye(4)), *Z_HAND, TAU_HAND)[0]
    assert (cls2[0, :4] == CO.INVALID).all() and np.array_equal(cls2[1:], cls[1:])


def test_tie_at_the_tolerance_is_covisible():
    depth, src, _ = hand_frames()
    for target, want in ((2.5, -0.5), (1.5, 0.5)):
        cls, ce, ez, sums = CO.pair(depth, src, np.full_like(depth, target), src, K_HAND, CO.relative_pose(np.eye(4), np.eye(4)), *Z_HAND, 0.5)
        assert sums[CO.COVISIBLE] == (H_HAND - 1) * (W_HAND - 1) and (ez[:-1, :-1] == want).all()
        assert sums[9] == 0.5 * sums[CO.COVISIBLE] and sums[10] == 0.25 * sums[CO.COVISIBLE] and sums[11] == 0.25 * sums[CO.COVISIBLE]


def test_consistency_summary():
    row = np.array([5, 10, 3, 4, 2, 6, 20, 90.0, 1200.0, 1.0, 0.125, 0.5])
    s = geometry.consistency_summary(row)
    assert [s[n] for n in geometry.CONSISTENCY_CLASSES] == [5, 10, 3, 4, 2, 6, 20] and geometry.CONSISTENCY_CLASSES == CO.CLASSES
    assert s["n_valid"] == 45 and s["covisibility"] == 20 / 45 and s["violation_rate"] == 2 / 32
    assert s["color_mae"] == 90.0 / 60.0 and s["psnr"] == 10.0 * math.log10(255.0 ** 2 * 60.0 / 1200.0)
    assert s["depth_mae"] == 0.05 and s["depth_rmse"] == math.sqrt(0.125 / 20) and s["depth_rel"] == 0.025
    assert s == CO.summary(row)
    # several rows are added first; a tensor is read once
    rows = np.stack([row, 2 * row, np.zeros(12)])
    assert geometry.consistency_summary(rows) == geometry.consistency_summary(3 * row) == CO.summary(rows)
    assert geometry.consistency_summary(torch.from_numpy(rows)) == geometry.consistency_summary(rows)
    # exact colours: inf; nothing covisible, nothing valid: NaN where the denominator is 0
    exact = row.copy()
    exact[7:9] = 0
    assert geometry.consistency_summary(exact)["psnr"] == math.inf and geometry.consistency_summary(exact)["color_mae"] == 0.0
    none = np.array([5, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0])
    s = geometry.consistency_summary(none)
    assert s["covisibility"] == 0.0 and s["n_valid"] == 10
    assert all(math.isnan(s[k]) for k in ("violation_rate", "color_mae", "psnr", "depth_mae", "depth_rmse", "depth_rel"))
    s = geometry.consistency_summary(np.zeros(12))
    assert math.isnan(s["covisibility"]) and s["n_valid"] == 0
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))  # noqa: E731
    for r in (none, np.zeros(12), exact):
        got, want = geometry.consistency_summary(r), CO.summary(r)
        assert set(got) == set(want) and all(same(got[k], want[k]) for k in got)
    with pytest.raises(ValueError, match="12"):
        geometry.consistency_summary(np.zeros(11))


def test_c_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.sgam_abi_version() == _lib.ABI_VERSION == 10
    ws = lib.sgam_view_consistency_workspace_bytes
    assert ws(2, 2, 1) == 96 and ws(256, 256, 1) == 256 * 96 and ws(17, 19, 3) == 3 * 2 * 96 and ws(16, 16, 65535) == 65535 * 96
    assert ws(46340, 46340, 1) == ((46340 * 46340 + 255) // 256) * 96
    for bad in ((1, 16, 1), (16, 1, 1), (16, 16, 0), (16, 16, 65536), (65536, 32768, 1), (-4, 16, 1)):
        assert ws(*bad) == -1, bad
    # a valid call's arguments, then one of them spoilt at a time: SGAM_EINVAL before anything touches the device (the "device"
    # pointers are host buffers nothing reads)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    kinv = (ctypes.c_float * 9)(*np.linalg.inv(K_HAND).astype(np.float32).ravel())
    good = dict(depth_ptrs=p, rgb_ptrs=p, F=2, H=16, W=16, kinv9=ctypes.cast(kinv, ctypes.c_void_p), fx=16.0, fy=16.0, cx=8.0, cy=4.0,
                z_near=1.0, z_far=4.0, tau=0.05, pairs=p, T_rel=p, P=1, sums=p, class_map=None, color_error=None, depth_error=None,
                workspace=p, workspace_bytes=96, stream=None)
    nan = float("nan")
    for change in (dict(depth_ptrs=None), dict(rgb_ptrs=None), dict(kinv9=None), dict(pairs=None), dict(T_rel=None), dict(sums=None),
                   dict(workspace=None), dict(F=0), dict(H=1), dict(W=1), dict(P=0), dict(P=65536), dict(H=65536, W=32768),
                   dict(tau=-0.01), dict(tau=nan), dict(z_near=4.5), dict(z_near=nan), dict(z_far=nan), dict(workspace_bytes=95),
                   dict(workspace=ctypes.c_void_p(p.value + 8)), dict(P=2)):
        args = dict(good, **change)
        assert lib.sgam_view_consistency_f32(*args.values()) == -1, change


def test_python_front_refuses_bad_arguments_before_the_device():
    depth = [torch.full((H_HAND, W_HAND), 2.0) for _ in range(2)]
    rgb = [torch.zeros((H_HAND, W_HAND, 3), dtype=torch.uint8) for _ in range(2)]
    Ts = np.stack([np.eye(4), camera_at(x=TX)])
    call = lambda **kw: geometry.view_consistency(depth, rgb, K_HAND, kw.pop("Ts", Ts), kw.pop("z_near", 1.0), kw.pop("z_far", 4.0),  # noqa: E731
                                                  kw.pop("tau", 0.05), **kw)
    for kw, text in ((dict(tau=-1.0), "depth_tolerance"), (dict(tau=float("nan")), "depth_tolerance"), (dict(z_near=5.0), "z_near"),
                     (dict(z_far=float("nan")), "z_near"), (dict(Ts=Ts[:1]), "Ts_w2c"), (dict(pairs=[(0, 2)]), "pair"),
                     (dict(pairs=[(-1, 0)]), "pair"), (dict(pairs=[(0, 1.5)]), "pair"), (dict(pairs=[(0, 1, 1)]), "pairs"),
                     (dict(pairs=[]), "no pairs"), (dict(_max_pairs=0), "_max_pairs")):
        with pytest.raises(ValueError, match=text):
            call(**kw)
    with pytest.raises(SgamHipError, match="no CPU fallback"):            # and then there is no CPU path
        call()
