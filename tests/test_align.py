"""GPU tests of the alignment entry points (pcl_align.hip; build-defined: the reference calls an undefined helper).  Moments and the vote are
compared BIT FOR BIT with the numpy model of tests/align_helpers.py (the vote fed the device's own normals and planarities); the normals
against numpy.linalg.eigh on the model's exact matrix; the end-to-end errors against twice the model's own, measured on the CPU
(tests/test_align_model.py, the constants next to align_helpers.SCENES).

Shapes: 1, 63, 64, 65 and 257 points (tails of a wave and of a block); 1,000 points in one voxel; 1,024 points in 1,024 voxels; 3,000 points
shuffled against the same points sorted by cell; hand-placed points on cell faces and around 0; 2 m voxels at +-32767; 20,000-point rooms
at 10 cm.  The loops: a 120,000-point OmniScenes tree as tests/test_dataset_harness.py builds it, its cloud file tilted by 7 degrees; a
20,000-point one-room Stanford tree, tilted alike, as a known room, in a room search and under voxel_size (30 iterations, 128 x 256).  The
vote's workspace is the test's own, filled with three words in turn, a guard region behind it."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import align_helpers as ah
from conftest import Cfg

pytestmark = pytest.mark.gpu

GUARD64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(got, want):
    got, want = (host(got) if torch.is_tensor(got) else np.asarray(got)), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check_moments(ops, xyz, voxel):
    """VoxelGrid.moments twice against the model, bit for bit -> (grid, the model's (cell, count, first), moments)"""
    cell, count, first = ah.grid_model(xyz, voxel)
    g = ops.VoxelGrid(T(xyz), voxel)
    assert same_bits(g.cell, cell) and same_bits(g.count, count) and same_bits(g.first, first)
    want = ah.moments_model(xyz, cell, first, len(count))
    for _ in range(2):
        got = g.moments()
        assert got.shape == (len(count), 9) and same_bits(got, want)
    return g, (cell, count, first), want


def raw_moments(ops, xyz, voxel, cell, first, nvoxels, out=None):
    """pcl_voxel_moments on the test's own buffers -> (moments, bad)"""
    from piccolo_amd.ops import _ptr, _stream
    X, Cl, F = T(np.asarray(xyz, np.float32)), T(np.asarray(cell, np.int32)), T(np.asarray(first, np.int64))
    out = torch.full((nvoxels, 9), GUARD64, dtype=torch.int64, device="cuda") if out is None else out
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    rc = ops._lib.load().pcl_voxel_moments(_ptr(X), len(xyz), float(voxel), _ptr(Cl), _ptr(F), nvoxels, _ptr(out), _ptr(bad), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, int(bad.item())


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_moments_tails_of_a_wave_and_a_block(ops, n):
    from piccolo_amd import synth
    xyz = synth.scanned_room(n, seed=n)[0]
    xyz[n // 2:] = xyz[: n - n // 2] + np.float32(0.001)                         # neighbours that share voxels, up to the last lane
    _, (_, count, _), want = check_moments(ops, xyz, 0.25)
    assert n == 1 or (count.max() > 1 and np.abs(want).max() > 0)


def test_moments_one_voxel_and_one_voxel_per_point(ops):
    xyz = (np.random.default_rng(0).random((1000, 3)) * 0.04 + 1.005).astype(np.float32)        # many waves on one row
    g, (_, count, _), want = check_moments(ops, xyz, 0.05)
    assert g.nvoxels == 1 and count.tolist() == [1000] and (want[0, [3, 6, 8]] > 0).all()
    k = np.random.default_rng(2).permutation(1024)                                                # every point its own voxel
    own = np.stack([k % 16, (k // 16) % 16, k // 256], axis=1).astype(np.float32) * np.float32(0.5) - np.float32(3.9)
    g, _, want = check_moments(ops, own, 0.5)
    assert g.nvoxels == 1024 and not want.any()


def _scatter(moments, count):
    """the exact integer A = count S2 - S1 S1^T per voxel, as tuples of Python integers"""
    out = []
    for m, c in zip(np.asarray(moments).tolist(), np.asarray(count).tolist()):
        out.append(tuple(c * m[k] - m[p] * m[q] for p, q, k in ((0, 0, 3), (0, 1, 4), (0, 2, 5), (1, 1, 6), (1, 2, 7), (2, 2, 8))))
    return out


def test_random_order_against_sorted_order(ops):
    """the moments are offsets from the voxel's FIRST point, which the order chooses: each order equals its model bit for bit, and what
    is made of them — the exact scatter matrix, hence normal, planarity and eigenvalues — has the same bits in both orders"""
    rng = np.random.default_rng(5)
    centres = (rng.integers(-6, 6, size=(300, 3)) + 0.5) * 0.2
    xyz = (centres[rng.integers(0, 300, size=3000)] + (rng.random((3000, 3)) - 0.5) * 0.19).astype(np.float32)
    shuffled = xyz[rng.permutation(3000)]
    keys = np.floor(shuffled.astype(np.float64) / 0.2).astype(np.int64)
    ordered = shuffled[np.lexsort(keys.T)]
    results = []
    for cloud in (shuffled, ordered):
        g, (cell, count, first), want = check_moments(ops, cloud, 0.2)
        normal, planarity, eig = g.normals(min_count=5, return_eig=True)
        key = [tuple(v) for v in np.floor(cloud[first].astype(np.float64) / 0.2).astype(np.int64).tolist()]
        order = sorted(range(len(key)), key=key.__getitem__)
        scatter = _scatter(host(g.moments()), count)
        results.append(([key[i] for i in order], [scatter[i] for i in order], host(normal)[order], host(planarity)[order], host(eig)[order]))
    a, b = results
    assert a[0] == b[0] and a[1] == b[1]
    assert same_bits(a[2], b[2]) and same_bits(a[3], b[3]) and same_bits(a[4], b[4]) and (a[3] > 0).sum() > 100


def test_moments_negative_coordinates_faces_and_the_range_edge(ops):
    v = 0.05
    faces = np.array([[0.05, -0.05, -0.0], [0.0, 0.0, 0.0], [-0.01, 0.0, 0.049], [-0.051, 0.1, -0.1], [0.0999, -0.0501, 0.0], [-0.05, -0.1, 0.05],
                      [0.075, -0.025, -0.01], [0.051, -0.049, -0.0499], [-0.0001, -0.0001, -0.0001], [-0.0499, -0.0499, -0.0499]], np.float32)
    _, (_, count, _), _ = check_moments(ops, np.concatenate([faces, faces[::-1] + np.float32(1e-3), -faces]), v)
    assert count.max() > 1
    # voxel = 2 m at the coordinates' range edge, both signs: offsets of nearly 2 m, |d| up to 131072, in cells 16383 and -16384
    rng = np.random.default_rng(9)
    edge = (32766.0 + rng.random((400, 3)) * 1.99).astype(np.float32)
    edge[:200] = -edge[:200]
    edge[0], edge[1], edge[200], edge[201] = 32766.0, 32767.99, -32766.01, -32767.99
    assert np.abs(edge).max() < 32768
    g, (_, count, _), want = check_moments(ops, edge, 2.0)
    assert g.nvoxels == 2 and np.abs(want[:, :3]).max() > 0 and want[:, 3].min() > 2 ** 38
    with pytest.raises(ValueError, match="at most 2"):
        ops.VoxelGrid(T(edge), 2.5).moments()


def test_bad_coordinates_and_foreign_cells_add_nothing_inside_guard_words(ops):
    """a poisoned (V, 9) buffer between guard words: fully defined afterwards, nothing written outside it; a bad coordinate sets its bit and
    adds nothing (as the first point of its voxel it silences the voxel); a cell outside [0, V) adds nothing"""
    from piccolo_amd import synth
    xyz = synth.scanned_room(3001, seed=11)[0]
    cell, count, first = ah.grid_model(xyz, 0.25)
    V = len(count)
    g = ops.VoxelGrid(T(xyz), 0.25)
    buf = torch.full(((V + 4) * 9,), GUARD64, dtype=torch.int64, device="cuda")
    out = buf[18:18 + 9 * V].view(V, 9)
    got = g.moments(out=out)
    assert got.data_ptr() == out.data_ptr() and same_bits(out, ah.moments_model(xyz, cell, first, V))
    assert (host(buf[:18]) == GUARD64).all() and (host(buf[18 + 9 * V:]) == GUARD64).all()
    later = int(np.flatnonzero((count[cell] > 2) & (np.arange(len(xyz)) != first[cell]))[0])     # not its voxel's first point
    head = int(first[np.flatnonzero(count > 2)[1]])                                                # a voxel's first point
    for value, bit in ((np.nan, 1), (np.inf, 1), (-np.inf, 1), (32768.0, 4), (-1e9, 4)):
        for point in (later, head):
            poisoned = xyz.copy()
            poisoned[point, 1] = value
            skip = np.zeros(len(xyz), bool)
            skip[point] = True
            if point == head:
                skip |= cell == cell[head]
            clean = np.where(np.isfinite(poisoned) & (np.abs(poisoned) < 32768), poisoned, 0).astype(np.float32)
            got, bad = raw_moments(ops, poisoned, 0.25, cell, first, V)
            assert bad == bit and same_bits(got, ah.moments_model(clean, cell, first, V, skip)), (value, point)
    foreign = cell.copy()
    foreign[5], foreign[700], foreign[2999] = -1, V, 2 ** 31 - 1
    skip = np.zeros(len(xyz), bool)
    skip[[5, 700, 2999]] = True
    got, bad = raw_moments(ops, xyz, 0.25, foreign, first, V)
    assert bad == 0 and same_bits(got, ah.moments_model(xyz, cell, first, V, skip))
    wild = first.copy()                                                                            # a first[] outside [0, n) silences its voxel
    wild[3], wild[4] = -1, len(xyz)
    got, bad = raw_moments(ops, xyz, 0.25, cell, wild, V)
    assert bad == 0 and same_bits(got, ah.moments_model(xyz, cell, first, V, (cell == 3) | (cell == 4)))


# ------------------------------------------------------------------------------------------------ normals
def angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(axis=1)))


def test_normals_against_eigh_on_the_exact_matrix(ops):
    s = ah.NORMALS_SCENE
    xyz = ah.planted_scene("box", 7.0, 30.0, 20.0, n=s["points"])[0]
    g, (_, count, _), want = check_moments(ops, xyz, s["voxel"])
    lam, vec = ah.normals_model(want, count)
    for _ in range(2):
        normal, planarity, eig = (host(t) for t in g.normals(min_count=s["min_count"], return_eig=True))
        assert same_bits(g.normals(min_count=s["min_count"])[0], normal)
    assert normal.dtype == planarity.dtype == eig.dtype == np.float32 and normal.shape == (len(count), 3) and planarity.shape == (len(count),)
    eligible = (count >= s["min_count"]) & (lam[:, 2] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        model_planarity = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    gap = eligible & (model_planarity >= ah.GAP)
    assert eligible.sum() > 500 and (eligible & ~gap).sum() <= ah.GAP_SHARE * eligible.sum()
    err = angle(normal[gap].astype(np.float64), vec[gap])
    print("normals: %d voxels, largest angle to eigh %.3g rad" % (gap.sum(), err.max()))
    assert err.max() <= 1e-6
    assert np.abs(np.linalg.norm(normal[eligible].astype(np.float64), axis=1) - 1).max() < 2e-7
    big = np.abs(normal[eligible]).argmax(axis=1)
    assert (normal[eligible][np.arange(eligible.sum()), big] > 0).all()                           # the sign rule
    assert (np.abs(planarity[eligible] - model_planarity[eligible]) <= 1e-5 * np.abs(model_planarity[eligible])).all()
    assert (np.abs(eig[eligible] - lam[eligible]) <= 1e-5 * np.abs(lam[eligible]) + 1e-12).all()
    assert (eig[eligible, 0] <= eig[eligible, 1]).all() and (eig[eligible, 1] <= eig[eligible, 2]).all()
    under = count < s["min_count"]
    assert under.any() and not normal[under].any() and not planarity[under].any() and not eig[under].any()   # exact zeros


def test_normals_of_degenerate_voxels(ops):
    # three collinear points along an axis: planarity exactly 0; along a diagonal: 0 up to double rounding
    for line, bound in ((np.array([[0.1, 0.2, 0.3], [0.2, 0.2, 0.3], [0.4, 0.2, 0.3]], np.float32), 0.0),
                        (np.array([[1, 1, 1], [2, 2, 2], [5, 5, 5]], np.float32) / np.float32(64), 1e-12)):
        normal, planarity = ops.VoxelGrid(T(line), 1.0).normals(min_count=3)
        assert planarity.shape == (1,) and 0.0 <= float(planarity[0]) <= bound, host(planarity)
    # coincident points: l2 = 0, zeros
    normal, planarity, eig = ops.VoxelGrid(T(np.full((5, 3), 0.3, np.float32)), 1.0).normals(min_count=3, return_eig=True)
    assert not host(normal).any() and not host(planarity).any() and not host(eig).any()
    # an exact plane z = const: the normal is (0, 0, 1) exactly, the smallest eigenvalue 0
    plane = ah.exact_plane(500)
    g = ops.VoxelGrid(T(plane), 2.0)
    normal, planarity, eig = (host(t) for t in g.normals(min_count=8, return_eig=True))
    assert g.nvoxels == 1 and normal.tolist() == [[0.0, 0.0, 1.0]] and eig[0, 0] == 0.0 and 0 < planarity[0] <= 1
    lam, _ = ah.normals_model(host(g.moments()), host(g.count))
    assert abs(planarity[0] - lam[0, 1] / lam[0, 2]) <= 1e-5 * planarity[0]
    with pytest.raises(ValueError, match="min_count"):
        g.normals(min_count=2)


# ------------------------------------------------------------------------------------------------ the vote
def same_vote(got, want):
    keys = ("cos_tilt", "sin_tilt", "cos_yaw", "sin_yaw", "tilt", "yaw")
    return (same_bits(got["up"], want["up"]) and same_bits(got["rot"], want["rot"]) and got["weights"] == want["weights"]
            and got["status"] == want["status"] and all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() for k in keys))


@pytest.mark.parametrize("k", range(len(ah.SCENES)))
def test_vote_is_the_models_and_recovers_the_planted_frame(ops, k):
    from piccolo_amd import data_utils, utils
    xyz, _, up, yaw = ah.planted_scene(*ah.SCENES[k])
    X = T(xyz)
    normal, planarity, grid = utils.voxel_normals(X, ah.SCENE_VOXEL, ah.SCENE_MIN_COUNT)
    for with_yaw in (True, False):
        got = ops.align_vote(normal, planarity, grid.count, max_tilt=40.0, yaw=with_yaw)
        want = ah.vote_model(host(normal), host(planarity), host(grid.count), 40.0, with_yaw)
        assert same_vote(got, want), (got, want)
        assert same_vote(got, ops.align_vote(normal, planarity, grid.count, max_tilt=40.0, yaw=with_yaw))
    got = ops.align_vote(normal, planarity, grid.count, max_tilt=40.0, yaw=True)
    up_err, yaw_err = ah.up_error_deg(got["up"], up), ah.yaw_error_deg(got["yaw"], yaw)
    print("scene", ah.SCENES[k], "device up error %.4f deg, yaw error %.4f deg" % (up_err, yaw_err))
    assert got["status"] == 0 and up_err <= 2 * ah.MODEL_UP_ERROR_DEG[k] and yaw_err <= 2 * ah.MODEL_YAW_ERROR_DEG[k]
    # the whole recipe through utils.align_cloud: the same record, the cloud under it bit for bit the model's fp32 restatement
    aligned, rot, trans, info = utils.align_cloud(X, voxel=ah.SCENE_VOXEL, yaw=True, min_count=ah.SCENE_MIN_COUNT)
    assert same_vote(info, got) and same_bits(rot, got["rot"]) and trans.shape == (3, 1) and trans.dtype == np.float64 and not trans.any()
    assert same_bits(aligned, ah.transform_model(xyz, rot.astype(np.float32), np.zeros(3, np.float32)))
    # the room's floor and ceiling are level again: over every point of theirs (by its place in the ROOM's frame, 5 sigma of the noise)
    # the height is 1.5 m up to the noise and to the lever of the asserted up error over the room's half diagonal of 5 m
    room_z = (xyz.astype(np.float64) @ ah.plant_rotation(*ah.SCENES[k][1:]))[:, 2]
    level = np.abs(np.abs(room_z) - 1.5) < 5 * ah.NOISE
    residual = np.abs(np.abs(host(aligned)[level, 2].astype(np.float64)) - 1.5)
    assert level.sum() > 5000 and residual.max() <= 5.0 * math.sin(math.radians(2 * ah.MODEL_UP_ERROR_DEG[k])) + 5 * ah.NOISE, residual.max()
    if k == 1:
        pn, pp = utils.point_normals(X, ah.SCENE_VOXEL, ah.SCENE_MIN_COUNT)
        cell = host(grid.cell).astype(np.int64)
        assert same_bits(pn, host(normal)[cell]) and same_bits(pp, host(planarity)[cell])
        a_trans, a_rot = data_utils.obtain_align_matrix(xyz.astype(np.float64), min_count=ah.SCENE_MIN_COUNT)
        assert a_trans.shape == (3, 1) and a_rot.dtype == a_trans.dtype == np.float64 and not a_trans.any()
        assert same_bits(a_rot, ops.align_vote(normal, planarity, grid.count)["rot"])


def test_vote_statuses_and_the_tie(ops):
    def both(normal, planarity, count, yaw):
        got = ops.align_vote(T(normal), T(planarity), T(count), max_tilt=40.0, yaw=yaw)
        want = ah.vote_model(normal, planarity, count, 40.0, yaw)
        assert same_vote(got, want), (got, want)
        return got
    half, ten = np.full(4, 0.5, np.float32), np.full(4, 10, np.int32)
    flat = both(np.array([[1.0, 0, 0]] * 4, np.float32), half, ten, True)                          # an empty cone
    assert flat["status"] == 1 and np.array_equal(flat["rot"], np.eye(3)) and flat["weights"] == (0, 0, 0, 0) and flat["tilt"] == 0.0
    far = both(np.array([[math.sin(1.0), 0, math.cos(1.0)]] * 4, np.float32), half, ten, False)    # 57 degrees off: outside max_tilt
    assert far["status"] == 1
    floor = both(np.array([[0, 0, 1.0], [0, 0, -1.0]] * 2, np.float32), half, ten, True)           # no walls
    assert floor["status"] == 2 and floor["yaw"] == 0.0 and np.array_equal(floor["rot"], np.eye(3)) and floor["weights"][:2] == (81920, 81920)
    a, b = np.array([0.2, 0.1, 1.0]), np.array([-0.3, 0.25, 1.0])
    two = np.stack([a / np.linalg.norm(a), b / np.linalg.norm(b)]).astype(np.float32)
    for order in ([0, 1], [1, 0]):                                                                 # two equal bins: the lower index, in any order
        tie = both(two[order], np.full(2, 0.75, np.float32), np.full(2, 7, np.int32), False)
        assert ah.up_error_deg(tie["up"], two[0]) < 1e-3 and tie["weights"] == (2 * 7 * 3072, 7 * 3072, 0, 0)
    # voxels that do not vote: zero normals, zero and out-of-range planarities, zero counts, a NaN
    n = np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 1.0], [0, 0, 1.0], [0, 0, 1.0], [np.nan, 0, 1.0], [1.0, 0, 0]], np.float32)
    p = np.array([0.5, 0.5, 0.0, 1.5, 0.5, 0.5, np.nan], np.float32)
    c = np.array([3, 3, 3, 3, 0, 3, 3], np.int32)
    only = both(n, p, c, True)
    assert only["weights"][0] == 3 * 2048 and only["status"] == 2


@pytest.mark.parametrize("n", [1, 65, 257])
def test_transform_cloud_is_the_stated_fp32_order(ops, n):
    rng = np.random.default_rng(n)
    xyz = (rng.normal(size=(n, 3)) * 5).astype(np.float32)
    rot, trans = ah.random_rotation(rng).astype(np.float32), rng.normal(size=3).astype(np.float32)
    want = ah.transform_model(xyz, rot, trans)
    for r, t in ((T(rot), T(trans)), (torch.from_numpy(rot.astype(np.float64)), torch.from_numpy(trans.reshape(3, 1)))):
        assert same_bits(ops.align_transform_cloud(T(xyz), r, t), want)


# ------------------------------------------------------------------------------------------------ the loop
def test_omniscenes_loop_on_a_tilted_cloud(ops, tmp_path):
    """test_dataset_harness.py's OmniScenes tree with the cloud FILE tilted by 7 degrees and the ground truth in that tilted frame:
    gravity_aligned = False with align_cloud localises in the aligned frame and reports in the file's own.  Plumbing and frames, not
    millimetres: the refinement is chaotic (README, "Parity")."""
    from PIL import Image
    import test_dataset_harness as dh
    from piccolo_amd import localize
    root = tmp_path / "omniscenes"
    xyz, rgb8 = dh._scene()
    P = ah.plant_rotation(7.0, 30.0, 0.0)
    dh._write_cloud(str(root / "pcd/room_1.txt"), (xyz.astype(np.float64) @ P.T).astype(np.float32), rgb8)
    video = "handheld_room_1_scene_2"
    os.makedirs(root / "extreme_pano" / video)
    os.makedirs(root / "extreme_pose" / video)
    for k, (t, ypr) in enumerate(dh.POSES):
        pano, R = dh._render(xyz, rgb8, t, ypr)                                  # R (x - t) = (R P^T) (P x - P t)
        big = np.repeat(np.repeat(pano, 4, axis=0), 4, axis=1)
        Image.fromarray(big).save(root / "extreme_pano" / video / ("%06d.jpg" % k), format="PNG")
        np.savetxt(root / "extreme_pose" / video / ("%06d.txt" % k), np.hstack([R.astype(np.float64) @ P.T, P @ t.reshape(3, 1).astype(np.float64)]))
    base = dict(dataset="OmniScenes", init_downsample_h=8, init_downsample_w=8, main_downsample_h=2, main_downsample_w=2, scene_number=2,
                **{**dh.COMMON, "num_intermediate": 40, "parallel": False})
    with pytest.raises(NotImplementedError):
        localize.localize_omniscenes(Cfg(gravity_aligned=False, **base), None, None, root=str(root))
    log = tmp_path / "log"
    table = localize.localize_omniscenes(Cfg(gravity_aligned=False, align_cloud=True, save_starting_point=True, **base), None, str(log),
                                         root=str(root)).cpu().numpy()
    assert table.shape == (2, 16) and np.isfinite(table).all()
    with open(log / "omniscenes_results.csv") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 3 and rows[0] == localize.OMNISCENES_HEADER and [r[3] for r in rows[1:]] == ["0", "0"]
    room = localize.LAST_RUN["align"]["room_1"]
    print("loop: tilt %.4f yaw %.4f status %d; errors %r" % (room["tilt"], room["yaw"], room["status"], table[:, 13:15].tolist()))
    assert room["status"] == 0 and abs(room["tilt"] - 7.0) <= 2 * max(ah.MODEL_UP_ERROR_DEG) and room["yaw"] == 0.0
    assert localize.LAST_RUN["total"] == 2
    # the frame the harness test requires to be localised, in the FILE's frame: the row's pose is the tilted frame's
    assert localize.omniscenes_success(table[1, 13], table[1, 14]), table[:, 13:15]
    assert np.abs(table[1, 0:3] - P @ dh.POSES[1][0]).max() < 0.1
    est = np.array(rows[2][4].split(), np.float64)
    assert np.abs(est - P @ dh.POSES[1][0]).max() < 0.1
    assert (log / "results" / video / "000001.png").exists() and (log / "starting_points" / video / "000001_0.png").exists()
    # with the yaw and the voxel keys beside it: the cloud is aligned, then down-sampled; the rows are still the file's frame
    again = localize.localize_omniscenes(Cfg(gravity_aligned=False, align_cloud=True, align_yaw=True, align_min_count=5, voxel_size=0.05,
                                             **{**base, "num_iter": 30}), None, str(tmp_path / "log2"), root=str(root)).cpu().numpy()
    assert again.shape == (2, 16) and np.isfinite(again).all()
    room = localize.LAST_RUN["align"]["room_1"]
    assert room["status"] == 0 and abs(room["tilt"] - 7.0) <= 2 * max(ah.MODEL_UP_ERROR_DEG) and abs(room["yaw"]) <= 2 * max(ah.MODEL_YAW_ERROR_DEG)
    with open(tmp_path / "log2" / "omniscenes_results.csv") as f:
        assert len(list(csv.reader(f))) == 3
    assert (tmp_path / "log2" / "results" / video / "000000.png").exists()


def test_stanford_loops_on_a_tilted_cloud(ops, tmp_path, monkeypatch):
    """a one-room Stanford tree whose cloud file is tilted by 7 degrees, known room and room search: the refinement sees the ALIGNED cloud
    (its floor level again), and every row is that refinement's pose mapped to the file's frame, bit for bit"""
    import json
    from PIL import Image
    import test_dataset_harness as dh
    from piccolo_amd import localize, synth
    root, (ph, pw) = tmp_path / "stanford", (128, 256)
    xyz, rgb = synth.scanned_room(20_000, seed=3)
    rgb8 = np.clip(np.round(rgb * 255), 0, 255).astype(np.uint8)
    P = ah.plant_rotation(7.0, 30.0, 0.0)
    dh._write_cloud(str(root / "pcd_not_aligned/area_3/office_1.txt"), (xyz.astype(np.float64) @ P.T).astype(np.float32), rgb8)
    os.makedirs(root / "pano/area_3")
    os.makedirs(root / "pose/area_3")
    X, C = T(xyz), T(rgb8.astype(np.float32) / np.float32(255))
    for k, (t, ypr) in enumerate(dh.POSES):
        pano = ops.make_pano(ops.transform_cloud(X, T(t), T(ypr)), C, (ph, pw)).cpu().numpy().astype(np.uint8)
        stem = "camera_c%03d_office_1_frame_equirectangular_domain" % k
        Image.fromarray(pano).save(root / "pano/area_3" / (stem + "_rgb.png"))
        with open(root / "pose/area_3" / (stem + "_pose.json"), "w") as f:
            json.dump({"camera_location": [float(v) for v in P @ t.astype(np.float64)],
                       "final_camera_rotation": dh._euler_for_stanford(synth.rot_from_ypr_np(ypr).astype(np.float64) @ P.T)}, f)
    seen = []
    refine, in_rooms = localize.refine_image, localize.localize_in_rooms

    def refine_image(img, X, C, tr, ro, cfg, scalar_summaries=None, weights=None):
        out = refine(img, X, C, tr, ro, cfg, scalar_summaries, weights=weights)
        seen.append((X, out[0], out[1]))
        return out

    def localize_in_rooms(img_init, img_main, rooms, cfg, init_dict):
        out = in_rooms(img_init, img_main, rooms, cfg, init_dict)
        seen.append((rooms[out[0]][0], out[1], out[2]))
        return out

    monkeypatch.setattr(localize, "refine_image", refine_image)
    monkeypatch.setattr(localize, "localize_in_rooms", localize_in_rooms)
    common = dict(dh.COMMON, num_trans=10, num_intermediate=12, num_input=6, num_iter=30, dataset="Stanford2D-3D-S", area=3, eval_full=True,
                  gravity_aligned=False, align_cloud=True, align_min_count=3)
    for name, keys in (("known", {}), ("search", dict(room_search=True)), ("voxel", dict(voxel_size=0.05))):
        del seen[:]
        log = tmp_path / ("log_" + name)
        table = localize.localize_stanford(Cfg(**keys, **common), None, str(log), root=str(root)).cpu().numpy()
        assert table.shape == (2, 16) and np.isfinite(table).all(), name
        room = localize.LAST_RUN["align"]["office_1"]
        assert room["status"] == 0 and abs(room["tilt"] - 7.0) <= 2 * max(ah.MODEL_UP_ERROR_DEG), (name, room)
        assert len(seen) == 2 and seen[0][0] is seen[1][0]
        z = host(seen[0][0])[:, 2]
        assert abs((z.max() - z.min()) - 3.0) < 0.1                              # level: the file's own z extent is a metre more
        info = localize._read_cloud(localize.data_utils.read_stanford, str(root / "pcd_not_aligned/area_3/office_1.txt"), 1, ops.device(),
                                    None, (0.1, 40.0, False, 3)).align
        for k, (_, t, R) in enumerate(seen):
            t0, R0 = localize.pose_to_cloud_frame(t, R, info.rot, info.trans)
            assert same_bits(table[k, 0:3], t0.reshape(3)) and same_bits(table[k, 3:12], R0.reshape(9)), (name, k)
        with open(log / "stanford_results.csv") as f:
            rows = list(csv.reader(f))
        assert len(rows) == 3 and rows[0][:10] == localize.STANFORD_HEADER and (name != "search" or rows[1][-1] == "office_1")
        assert (log / "results/area_3" / rows[1][1]).exists()


def test_vote_does_not_depend_on_what_its_workspace_held(ops):
    """the memory contract for the vote's workspace, on a buffer the test brings: filled with 0, 0xFFFFFFFF and 0x3F800000 in turn the
    record has the same bits, and a guard region behind the queried bytes stays as it was"""
    xyz = ah.planted_scene(*ah.SCENES[1])[0]
    from piccolo_amd import utils
    normal, planarity, grid = utils.voxel_normals(T(xyz), ah.SCENE_VOXEL, ah.SCENE_MIN_COUNT)
    want = ops.align_vote(normal, planarity, grid.count, yaw=True)
    nws = ops._lib.load().pcl_align_workspace_bytes(grid.nvoxels)
    assert nws % 4 == 0
    buf = torch.empty(nws // 4 + 64, dtype=torch.int32, device="cuda")
    for word in (0, -1, 0x3F800000):
        buf.fill_(word)
        got = ops.align_vote(normal, planarity, grid.count, yaw=True, ws=buf.view(torch.uint8)[:nws])
        assert same_vote(got, want), word
        assert (host(buf[nws // 4:]) == np.int32(word)).all()
    with pytest.raises(ValueError, match="workspace"):
        ops.align_vote(normal, planarity, grid.count, ws=buf.view(torch.uint8)[:nws - 1])
