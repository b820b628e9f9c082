"""CPU checks of the alignment recipe's numpy model (tests/align_helpers.py) on the scenes the GPU tests use: the model alone recovers the
planted up direction and wall yaw within the errors recorded next to its constants (the GPU tests assert twice those), the normals
scene keeps the eigen-gap condition's exclusions under its share, and the pose mapping between the aligned and the own frame is exact.

The tests of the model alone (recovery, statuses and tie, gap share, the transform's order) read only tests/align_helpers.py and
piccolo_amd.synth: they pin the yardstick, not the product, and pass on a tree without the feature.  The pose-mapping test calls
piccolo_amd.localize and fails there, as every test of tests/test_align.py, test_align_abi.py and test_align_cfg.py does."""
import math

import numpy as np
import pytest

import align_helpers as ah


@pytest.mark.parametrize("k", range(len(ah.SCENES)))
def test_model_recovers_the_planted_up_and_yaw(k):
    xyz, _, up, yaw = ah.planted_scene(*ah.SCENES[k])
    info = ah.align_model(xyz, ah.SCENE_VOXEL, ah.SCENE_MIN_COUNT, 40.0, True)[0]
    up_err, yaw_err = ah.up_error_deg(info["up"], up), ah.yaw_error_deg(info["yaw"], yaw)
    print("scene", ah.SCENES[k], "up error %.4f deg, yaw error %.4f deg, weights %r" % (up_err, yaw_err, info["weights"]))
    assert info["status"] == 0 and all(w > 0 for w in info["weights"])
    # the recorded figures are these measurements: what the GPU tests double
    assert abs(up_err - ah.MODEL_UP_ERROR_DEG[k]) <= ah.MODEL_RECHECK_DEG and abs(yaw_err - ah.MODEL_YAW_ERROR_DEG[k]) <= ah.MODEL_RECHECK_DEG
    assert abs(math.degrees(info["tilt"]) - ah.SCENES[k][1]) <= up_err + 1e-9
    # the rotation is one: orthonormal, takes up to +z, and (with the yaw) the walls onto the axes
    R = info["rot"]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.abs(R @ info["up"] - [0, 0, 1]).max() < 1e-12
    walls = R @ ah.plant_rotation(*ah.SCENES[k][1:])[:, :2]                       # the room's x and y axes, aligned
    assert np.abs(walls[2]).max() < math.sin(math.radians(2 * up_err)) + 1e-9
    assert min(abs(walls[0, 0]), abs(walls[1, 0])) < math.sin(math.radians(yaw_err + up_err)) + 1e-9


def test_normals_scene_keeps_the_gap_exclusions_under_their_share():
    s = ah.NORMALS_SCENE
    xyz = ah.planted_scene("box", 7.0, 30.0, 20.0, n=s["points"])[0]
    cell, count, first = ah.grid_model(xyz, s["voxel"])
    lam, _ = ah.normals_model(ah.moments_model(xyz, cell, first, len(count)), count)
    eligible = (count >= s["min_count"]) & (lam[:, 2] > 0)
    gap = (lam[eligible, 1] - lam[eligible, 0]) / lam[eligible, 2]
    left_out = int((gap < ah.GAP).sum())
    print("eligible %d of %d voxels, %d left out by the gap condition" % (eligible.sum(), len(count), left_out))
    assert eligible.sum() > 500 and left_out <= ah.GAP_SHARE * eligible.sum()


def test_model_statuses_and_tie():
    """no voter inside the cone -> status 1 and the identity; no wall normals -> status 2; two equal bins -> the lower index"""
    z = np.array([[0, 0, 1.0]] * 4, np.float32)
    flat = ah.vote_model(np.array([[1.0, 0, 0]] * 4, np.float32), np.full(4, 0.5, np.float32), np.full(4, 10), 40.0, True)
    assert flat["status"] == 1 and np.array_equal(flat["rot"], np.eye(3)) and flat["weights"] == (0, 0, 0, 0)
    floor = ah.vote_model(z, np.full(4, 0.5, np.float32), np.full(4, 10), 40.0, True)
    assert floor["status"] == 2 and floor["yaw"] == 0.0 and floor["weights"][:2] == (4 * 10 * 2048, 4 * 10 * 2048)
    assert np.array_equal(floor["up"], [0, 0, 1.0])
    a, b = np.array([0.2, 0.1, 1.0]), np.array([-0.3, 0.25, 1.0])
    two = np.stack([a / np.linalg.norm(a), b / np.linalg.norm(b)]).astype(np.float32)
    tie = ah.vote_model(two, np.full(2, 0.75, np.float32), np.full(2, 7), 40.0, False)
    bins = np.flatnonzero(tie["hist"])
    assert len(bins) == 2 and tie["hist"][bins[0]] == tie["hist"][bins[1]]
    # (a bin's index is 64 row + column, the row from n_y / n_z: the first normal, with the smaller n_y / n_z, sits in the lower bin)
    assert ah.up_error_deg(tie["up"], two[0].astype(np.float64)) < 1e-3 and tie["weights"][1] == 7 * 3072


@pytest.mark.parametrize("seed", range(4))
def test_pose_mapping_is_exact_and_inverts(seed):
    from piccolo_amd import localize
    rng = np.random.default_rng(seed)
    Ra, a = ah.random_rotation(rng), rng.normal(size=(3, 1)) * (seed % 2)          # (the shipped alignment has a = 0; the mapping takes any)
    R, t = ah.random_rotation(rng).astype(np.float32), rng.normal(size=(3, 1)).astype(np.float32)
    x = rng.normal(size=(200, 3)).astype(np.float32).astype(np.float64) * 3
    t0, R0 = localize.pose_to_cloud_frame(t, R, Ra, a)
    assert t0.dtype == R0.dtype == np.float32 and t0.shape == (3, 1) and R0.shape == (3, 3)
    aligned = (Ra @ (x.T - a)).T
    under_aligned = (R.astype(np.float64) @ (aligned.T - t.astype(np.float64))).T
    under_mapped = (R0.astype(np.float64) @ (x.T - t0.astype(np.float64))).T
    scale = np.abs(under_aligned).max()
    assert np.abs(under_mapped - under_aligned).max() <= 1e-5 * scale
    tb, Rb = localize.pose_from_cloud_frame(t0, R0, Ra, a)
    assert np.abs(tb - t).max() <= 1e-5 * max(1.0, np.abs(t).max()) and np.abs(Rb - R).max() <= 1e-5
    # the reference's own ground-truth mapping (localize.py:185-186)
    gt_t, gt_R = localize.pose_from_cloud_frame(t, R, Ra, a)
    assert np.allclose(gt_t, Ra @ (t.astype(np.float64) - a), atol=1e-6) and np.allclose(gt_R, R.astype(np.float64) @ Ra.T, atol=1e-6)


def test_transform_model_is_the_stated_order():
    rng = np.random.default_rng(0)
    x, r, a = rng.normal(size=(5, 3)).astype(np.float32), ah.random_rotation(rng).astype(np.float32), rng.normal(size=3).astype(np.float32)
    out = ah.transform_model(x, r, a)
    for i in range(5):
        d = x[i] - a
        for k in range(3):
            assert out[i, k] == np.float32(np.float32(np.float32(r[k, 0] * d[0]) + np.float32(r[k, 1] * d[1])) + np.float32(r[k, 2] * d[2]))
    assert np.abs(out - (x.astype(np.float64) - a) @ r.astype(np.float64).T).max() < 1e-5
