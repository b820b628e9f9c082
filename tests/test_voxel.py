"""GPU tests of the voxel grid (pcl_voxel.hip; build-defined: the reference has nothing of the kind).  Every comparison is exact — the bits of
the device results against the numpy model of tests/voxel_helpers.py — and every operation runs twice, for run-to-run equality.

Shapes: 1, 63, 64, 65 and 257 points (tails of a wave and of a block); 4,096 points in one voxel and 4,096 in 4,096 voxels; 5,000 points in
about 500 voxels in random order with duplicates; 7,428 points sorted by cell in runs of 1 to 100; hand-placed points on cell faces, around 0 and in the two extreme cells; 20,000 points
of synth.scanned_room at 5 cm.  End to end: 20,000-point scanned rooms, 6 candidates x 10 iterations, a 64 x 128 panorama."""
import csv
import json
import os

import numpy as np
import pytest
import torch

import voxel_helpers as vh
from conftest import Cfg

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


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
    got, want = host(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check_grid(ops, xyz, voxel, ws=None, buffers=None):
    """VoxelGrid twice against the model, bit for bit -> (grid, (cell, count, first) of the model)"""
    cell, count, first = vh.grid(xyz, voxel)
    X = T(xyz)
    grids = [ops.VoxelGrid(X, voxel, ws=ws, buffers=buffers) for _ in range(2)]
    for g in grids:
        assert g.n == len(xyz) and g.nvoxels == len(count)
        assert same_bits(g.cell, cell) and same_bits(g.count, count) and same_bits(g.first, first)
    return grids[0], (cell, count, first)


def check_all(ops, xyz, rgb, voxel, caps=(1, 3)):
    g, (cell, count, first) = check_grid(ops, xyz, voxel)
    want_xyz, want_rgb = vh.centroids(xyz, cell, count), vh.centroids(rgb, cell, count)
    for _ in range(2):
        got_xyz, got_rgb = g.centroids(T(rgb))
        assert same_bits(got_xyz, want_xyz) and same_bits(got_rgb, want_rgb)
    for cap in tuple(caps) + (int(count.max()) + 1,):
        for _ in range(2):
            assert same_bits(g.weights(cap), vh.weights(cell, count, cap)), cap
    assert (host(g.weights(int(count.max()))) == 1).all()                       # a cap no count exceeds: all ones
    return g, (cell, count, first)


def colours(n, seed):
    return np.random.default_rng(1000 + seed).random((n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tails_of_a_wave_and_a_block(ops, n):
    from piccolo_amd import synth
    xyz = synth.scanned_room(n, seed=n)[0]
    xyz[n // 2:] = xyz[: n - n // 2] + np.float32(0.001)                         # neighbours that share voxels, up to the last lane
    _, (_, count, _) = check_all(ops, xyz, colours(n, n), 0.25)
    assert n == 1 or count.max() > 1


def test_all_points_in_one_voxel(ops):
    """every lane of every wave on one destination; a count beyond a wave"""
    n = 4096
    xyz = (np.random.default_rng(0).random((n, 3)) * 0.04 + 1.005).astype(np.float32)
    g, (_, count, first) = check_all(ops, xyz, colours(n, 1), 0.05, caps=(1, 3, 4096))
    assert g.nvoxels == 1 and count.tolist() == [n] and first.tolist() == [0]
    assert same_bits(g.weights(3), np.full(n, np.float32(3.0 / 4096.0)))


def test_every_point_its_own_voxel_in_the_exact_workspace(ops):
    """V = N: degenerate runs, the sums' table full — in a workspace of exactly pcl_voxel_workspace_bytes(n) bytes"""
    n = 4096
    k = np.random.default_rng(2).permutation(n)
    xyz = np.stack([k % 16, (k // 16) % 16, k // 256], axis=1).astype(np.float32) * np.float32(0.5) - np.float32(3.9)
    nws = ops._lib.load().pcl_voxel_workspace_bytes(n)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    g, (cell, count, first) = check_grid(ops, xyz, 0.5, ws=ws)
    assert g.nvoxels == n and (count == 1).all() and np.array_equal(first, np.arange(n)) and np.array_equal(cell, np.arange(n))
    rgb = colours(n, 2)
    for _ in range(2):
        got_xyz, got_rgb = g.centroids(T(rgb), ws=ws)
        assert same_bits(got_xyz, vh.centroids(xyz, cell, count)) and same_bits(got_rgb, vh.centroids(rgb, cell, count))
    assert (host(g.weights(1)) == 1).all()
    with pytest.raises(ValueError, match="workspace"):
        ops.VoxelGrid(T(xyz), 0.5, ws=ws[:-1])


def test_random_order_with_duplicates(ops):
    """5,000 points in about 500 voxels, shuffled, with exact duplicates: run heads and the first-occurrence numbering"""
    rng = np.random.default_rng(5)
    n = 5000
    centres = (rng.integers(-6, 6, size=(500, 3)) + 0.5) * 0.2
    xyz = (centres[rng.integers(0, 500, size=n)] + (rng.random((n, 3)) - 0.5) * 0.19).astype(np.float32)
    xyz[rng.integers(0, n, size=400)] = xyz[rng.integers(0, n, size=400)]          # exact duplicates
    xyz = xyz[rng.permutation(n)]
    g, (cell, count, first) = check_all(ops, xyz, colours(n, 5), 0.2)
    assert 350 < g.nvoxels <= 500 and (np.diff(first) > 0).all() and count.max() > 3
    assert np.array_equal(cell[first], np.arange(g.nvoxels))


def test_scan_order_runs_of_every_length(ops):
    """a cloud sorted by cell, as a scanner delivers it: runs of 1 .. 100 neighbouring points per voxel, which start and end inside waves,
    cross wave and block boundaries and exceed a wave — the combine of neighbouring lanes at every step of its scan — then voxels that come
    back later (A B A inside a wave: neighbouring RUNS of one voxel are not one run) and an alternating pair"""
    rng = np.random.default_rng(13)
    lengths = np.concatenate([np.arange(1, 101), [70], rng.integers(2, 64, size=59), np.array([3, 5, 3, 5, 2, 2]), np.ones(40, np.int64)])
    voxel_of_run = np.arange(len(lengths))
    voxel_of_run[-46:-40] = [7, 8, 7, 8, 7, 7]                                   # earlier voxels again, interleaved
    voxel_of_run[-40:] = np.tile([20, 21], 20)                                   # A B A B ...: every lane its own run, two destinations
    v = np.repeat(voxel_of_run, lengths)
    n = len(v)
    cells = np.stack([v % 13 - 6, (v // 13) % 7 - 3, v // 91 - 1], axis=1)
    xyz = ((cells + 0.05 + 0.9 * rng.random((n, 3))) * 0.1).astype(np.float32)
    assert n > 5120 + 256 and np.array_equal(vh.cells(xyz, 0.1), cells)                 # (5050 + 70 = 20 x 256: a run starts a block)
    g, (cell, count, first) = check_all(ops, xyz, colours(n, 13), 0.1)
    assert np.array_equal(cell, v) and g.nvoxels == len(lengths) - 46              # first-occurrence numbering of a sorted cloud: the runs' own
    assert count[99] == 100 and count[7] == 8 + 3 + 3 + 2 + 2 and count[20] == 21 + 20
    runs = np.flatnonzero(np.diff(v) != 0) + 1                                   # where a run starts: inside waves, on their edges, on a block's
    assert (runs % 64 == 0).any() and (runs % 64 == 63).any() and (runs % 64 == 1).any() and (runs % 256 == 0).any()


def test_faces_signs_and_extreme_cells(ops):
    """cells straddling 0 on every axis, k * voxel as float32 sees it, -0.0, and the cells -2^20 and 2^20 - 1 (voxel 2^-6: exact)"""
    voxel = 0.05
    k = np.arange(-40, 41)
    face = (k * np.float64(voxel)).astype(np.float32)
    xyz = np.zeros((3 * len(k) + 6, 3), np.float32)
    for a in range(3):
        xyz[a * len(k):(a + 1) * len(k), a] = face
    xyz[-6:] = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [0.05, -0.05, 0.05], [-0.05, 0.05, -0.05], [-1e-30, 1e-30, -0.049999], [0.049999, -1e-30, 1e-30]],
                        np.float32)
    assert vh.cells(np.array([[0.05, -0.05, -0.0]], np.float32), voxel).tolist() == [[1, -2, 0]]
    g, (cell, _, _) = check_all(ops, xyz, colours(len(xyz), 7), voxel)
    assert cell[-6] == cell[-5] and len(set(cell[-6:].tolist())) == 5              # -0.0 is cell 0; floor, not truncation, for the rest
    v6 = 2.0 ** -6
    lo, hi = np.float32(-16384.0), np.float32(16384.0 - v6)
    ext = np.array([[lo, lo, lo], [hi, hi, hi], [lo, hi, 0.0], [hi, lo, -0.0], [lo, lo, lo + np.float32(v6)], [0.0, 0.0, 0.0], [hi, hi, hi]], np.float32)
    assert vh.cells(ext[:2], v6).tolist() == [[-(1 << 20)] * 3, [(1 << 20) - 1] * 3]
    g, (cell, count, _) = check_all(ops, ext, colours(len(ext), 8), v6)
    assert g.nvoxels == 6 and cell[6] == cell[1] and count[1] == 2


# ------------------------------------------------------------------------------------------------ the bad set
@pytest.mark.parametrize("value,voxel,text", [(np.nan, 0.05, "NaN or infinite"), (np.inf, 0.05, "NaN or infinite"), (-np.inf, 0.05, "NaN or infinite"),
                                              (16384.0, 2.0 ** -6, r"outside \[-2\^20, 2\^20\)"), (40000.0, 0.05, "32768 or more")])
def test_each_bad_bit_raises_and_faults_nothing(ops, value, voxel, text):
    from piccolo_amd import synth, utils
    xyz, rgb = synth.scanned_room(300, seed=9)
    bad = xyz.copy()
    bad[123, 1] = value
    assert vh.bad_bits(bad, voxel) in (vh.BAD_NONFINITE, vh.BAD_CELL, vh.BAD_MAGNITUDE)
    for _ in range(2):
        with pytest.raises(ValueError, match=text):
            ops.VoxelGrid(T(bad), voxel)
    with pytest.raises(ValueError, match=text):
        utils.density_weights(T(bad), voxel)
    with pytest.raises(ValueError, match=text):
        utils.voxel_downsample(T(bad), T(rgb), voxel)
    if vh.bad_bits(np.float32([value])) != 0:                                    # a bad COLOUR: the centroids' own check
        g = ops.VoxelGrid(T(xyz), 0.05)
        c = rgb.copy()
        c[7, 2] = value
        with pytest.raises(ValueError, match=text):
            g.centroids(T(c))
        assert same_bits(g.centroids(T(rgb))[1], vh.downsample(xyz, rgb, 0.05)[1])      # ... and the grid is as good as before
    torch.cuda.synchronize()
    check_grid(ops, xyz, 0.05)                                                   # the device is well: the next call is exact


def test_two_bad_bits_are_both_named(ops):
    xyz = np.zeros((70, 3), np.float32)
    xyz[3, 0], xyz[66, 2] = np.nan, 40000.0
    with pytest.raises(ValueError, match="NaN or infinite.*32768 or more"):
        ops.VoxelGrid(T(xyz), 0.05)


# ------------------------------------------------------------------------------------------------ the memory contract
def test_results_do_not_depend_on_earlier_contents(ops):
    """count / first buffers of N entries pre-filled with a guard word: entries at and beyond V untouched; the workspace pre-filled with
    0, 0xFFFFFFFF and 0x3F800000 in turn: the same bits every time"""
    from piccolo_amd import synth
    n = 3001
    xyz, rgb = synth.scanned_room(n, seed=11)
    cell, count, first = vh.grid(xyz, 0.1)
    V = len(count)
    assert 1 < V < n
    nws = ops._lib.load().pcl_voxel_workspace_bytes(n)
    ws = torch.empty(nws // 4 + 1, dtype=torch.int32, device="cuda")
    want_xyz, want_rgb = vh.centroids(xyz, cell, count), vh.centroids(rgb, cell, count)
    for word in (0, -1, 0x3F800000):
        ws.fill_(word)
        cbuf = torch.full((n,), GUARD32, dtype=torch.int32, device="cuda")
        fbuf = torch.full((n,), GUARD64, dtype=torch.int64, device="cuda")
        g, _ = check_grid(ops, xyz, 0.1, ws=ws.view(torch.uint8), buffers=(cbuf, fbuf))
        assert g.count.data_ptr() == cbuf.data_ptr() and g.first.data_ptr() == fbuf.data_ptr()
        assert (host(cbuf[V:]) == GUARD32).all() and (host(fbuf[V:]) == GUARD64).all()
        ws.fill_(word)
        got_xyz, got_rgb = g.centroids(T(rgb), ws=ws.view(torch.uint8))
        assert same_bits(got_xyz, want_xyz) and same_bits(got_rgb, want_rgb), word


# ------------------------------------------------------------------------------------------------ down-sampling
_ROOM = {}


def room(seed=3, n=20_000):
    """(xyz, rgb) numpy, and the model's grid at 5 cm — computed once, shared, left unchanged"""
    if (seed, n) not in _ROOM:
        from piccolo_amd import synth
        xyz, rgb = synth.scanned_room(n, seed=seed)
        _ROOM[seed, n] = (xyz, rgb, vh.grid(xyz, 0.05))
    return _ROOM[seed, n]


def test_downsample_first_and_centroid(ops):
    from piccolo_amd import utils
    xyz, rgb, (cell, count, first) = room()
    assert count.max() >= 8 and np.median(count) <= 2                            # the scan is skewed
    for _ in range(2):
        fx, fr, fc, ff = utils.voxel_downsample(T(xyz), T(rgb), 0.05, how="first")
        assert same_bits(fx, xyz[first]) and same_bits(fr, rgb[first]) and same_bits(fc, count) and same_bits(ff, first)
        cx, cr, cc, cf = utils.voxel_downsample(T(xyz), T(rgb), 0.05)
        want = vh.downsample(xyz, rgb, 0.05)
        assert same_bits(cx, want[0]) and same_bits(cr, want[1]) and same_bits(cc, count) and same_bits(cf, first)
    # CPU tensors are uploaded; the point order is the caller's, not the packed cloud's Morton order
    cx2 = utils.voxel_downsample(torch.from_numpy(xyz), torch.from_numpy(rgb), 0.05)[0]
    assert same_bits(cx2, want[0])
    for cap in (1, 3, int(count.max()) + 5):
        for _ in range(2):
            assert same_bits(utils.density_weights(T(xyz), 0.05, cap), vh.weights(cell, count, cap)), cap
    w = host(utils.density_weights(T(xyz), 0.05))
    per_voxel = np.zeros(len(count))
    np.add.at(per_voxel, cell, w.astype(np.float64))
    assert np.abs(per_voxel - 1).max() < 1e-5                                    # cap = 1: every occupied voxel has total weight 1


# ------------------------------------------------------------------------------------------------ end to end
H, W = 64, 128
CFG = dict(lr=0.1, num_iter=10, patience=5, factor=0.8, out_of_room_quantile=0.05, num_input=6)


def scene(seed=3):
    from piccolo_amd import ops, synth
    xyz, rgb, _ = room(seed)
    t_gt, ypr_gt = synth.gt_pose(seed)
    X, C = T(xyz), T(rgb)
    img = synth.quantise_like_image_file(ops.make_pano(ops.transform_cloud(X, T(t_gt), T(ypr_gt)), C, (H, W)))
    trans, rot = synth.start_poses(t_gt, ypr_gt, 6, seed=seed)
    return X, C, img, trans, rot


def same_result(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b)) and len(a) == len(b)


def test_unit_density_weights_are_the_unweighted_refinement(ops):
    from piccolo_amd import omniloc as po, utils
    X, C, img, trans, rot = scene()
    w = utils.density_weights(X, 1e-4)
    _, count, _ = vh.grid(host(X), 1e-4)
    assert (count == 1).all() and bool((w == 1).all())                          # every point alone in its voxel: the precondition
    cfg = Cfg(**CFG)
    plain = po.omniloc_batch(img, X, C, T(trans.copy()), T(rot.copy()), cfg, {})
    weighted = po.omniloc_batch(img, X, C, T(trans.copy()), T(rot.copy()), cfg, {}, weights=w)
    assert same_result(plain, weighted)
    dense = po.omniloc_batch(img, X, C, T(trans.copy()), T(rot.copy()), cfg, {}, weights=utils.density_weights(X, 0.05))
    assert not torch.equal(dense[2], plain[2])                                  # at 5 cm the weights matter


def test_refinement_on_the_downsampled_cloud_is_the_models(ops):
    from piccolo_amd import omniloc as po, utils
    X, C, img, trans, rot = scene()
    cfg = Cfg(**CFG)
    for how in ("centroid", "first"):
        dx, dc, _, _ = utils.voxel_downsample(X, C, 0.05, how=how)
        mx, mc, _, _ = vh.downsample(host(X), host(C), 0.05, how=how)
        assert dx.shape[0] < X.shape[0] and same_bits(dx, mx) and same_bits(dc, mc)
        got = po.omniloc_batch(img, dx, dc, T(trans.copy()), T(rot.copy()), cfg, {})
        want = po.omniloc_batch(img, T(mx), T(mc), T(trans.copy()), T(rot.copy()), cfg, {})
        assert same_result(got, want), how


def test_density_weights_of_is_one_tensor_per_room(ops):
    from piccolo_amd import omniloc as po
    xyz, _, (cell, count, _) = room()
    X = T(xyz)
    a, b = po.density_weights_of(X, 0.05, 1), po.density_weights_of(X, 0.05, 1)
    assert a is b and same_bits(a, vh.weights(cell, count, 1))
    assert po.density_weights_of(X, 0.05, 3) is not a and po.density_weights_of(X, 0.1, 1) is not a
    assert po.density_weights_of(X, 0.05) is a                                   # (cap's default is 1)
    X2 = T(xyz)                                                                  # the room is read again: another tensor, another entry
    c = po.density_weights_of(X2, 0.05, 1)
    assert c is not a and torch.equal(c, a) and po.density_weights_of(X2, 0.05, 1) is c


def _write_cloud(path, xyz, rgb8):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for p, c in zip(xyz, rgb8):
            f.write("%.4f %.4f %.4f %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))


def test_read_cloud_under_voxel_size_returns_the_models_cloud(ops, tmp_path):
    from piccolo_amd import cfg_rules, data_utils, localize
    xyz, rgb, _ = room(seed=4, n=3000)
    path = str(tmp_path / "pcd" / "room.txt")
    _write_cloud(path, xyz, np.clip(np.round(rgb * 255), 0, 255).astype(np.uint8))
    dev = ops.device()
    X0, C0 = localize._read_cloud(data_utils.read_stanford, path, 1, dev)
    assert X0.shape == (3000, 3)
    for kw in (dict(voxel_size=0.1), dict(voxel_size=0.1, voxel_how="first")):
        voxel = cfg_rules.voxel_rules(Cfg(**kw))
        X, C = localize._read_cloud(data_utils.read_stanford, path, 1, dev, voxel)
        mx, mc, _, _ = vh.downsample(host(X0), host(C0), 0.1, how=voxel[1])
        assert X.shape[0] < 3000 and same_bits(X, mx) and same_bits(C, mc), kw
    # the one-entry cache still hands consecutive images of a room the very same tensors
    cloud = localize._cloud_cache(data_utils.read_stanford, 1, dev, cfg_rules.voxel_rules(Cfg(voxel_size=0.1)))
    first, again = cloud(path), cloud(path)
    assert first[0] is again[0] and first[1] is again[1] and same_bits(first[0], vh.downsample(host(X0), host(C0), 0.1)[0])


def test_stanford_loop_under_the_voxel_and_the_density_keys(ops, tmp_path, monkeypatch):
    """a one-room Stanford tree with two frames: localize_stanford with voxel_size, and again with the density keys, to a CSV of the usual
    columns; the voxel run refines the down-sampled cloud, the density run hands refine_image ONE weights tensor for both images"""
    from PIL import Image
    import test_dataset_harness as dh
    from piccolo_amd import localize, omniloc as po, synth
    root, (ph, pw) = tmp_path / "stanford", (128, 256)
    xyz, rgb, _ = room()
    rgb8 = np.clip(np.round(rgb * 255), 0, 255).astype(np.uint8)
    _write_cloud(str(root / "pcd_not_aligned/area_3/office_1.txt"), xyz, rgb8)
    os.makedirs(root / "pano/area_3")
    os.makedirs(root / "pose/area_3")
    X, C = T(xyz), T(rgb8.astype(np.float32) / np.float32(255))
    for k, (t, ypr) in enumerate(dh.POSES):
        pano = ops.make_pano(ops.transform_cloud(X, T(t), T(ypr)), C, (ph, pw)).cpu().numpy().astype(np.uint8)
        stem = "camera_c%03d_office_1_frame_equirectangular_domain" % k
        Image.fromarray(pano).save(root / "pano/area_3" / (stem + "_rgb.png"))
        with open(root / "pose/area_3" / (stem + "_pose.json"), "w") as f:
            json.dump({"camera_location": [float(v) for v in t],
                       "final_camera_rotation": dh._euler_for_stanford(synth.rot_from_ypr_np(ypr).astype(np.float64))}, f)
    seen = []
    refine = localize.refine_image

    def refine_image(img, X, C, tr, ro, cfg, scalar_summaries=None, weights=None):
        seen.append((X, weights))
        return refine(img, X, C, tr, ro, cfg, scalar_summaries, weights=weights)

    monkeypatch.setattr(localize, "refine_image", refine_image)
    common = dict(dh.COMMON, num_trans=10, num_intermediate=12, num_input=6, num_iter=30)
    from piccolo_amd import data_utils
    as_read = localize._read_cloud(data_utils.read_stanford, str(root / "pcd_not_aligned/area_3/office_1.txt"), 1, ops.device())[0]
    read = vh.grid(host(as_read), 0.05)                                          # (the coordinates as the text file holds them)
    for name, keys in (("voxel", dict(voxel_size=0.05)), ("density", dict(density_weights=True, density_voxel=0.05, density_cap=2))):
        del seen[:]
        log = tmp_path / ("log_" + name)
        cfg = Cfg(dataset="Stanford2D-3D-S", area=3, eval_full=True, **keys, **common)
        table = localize.localize_stanford(cfg, None, str(log), root=str(root)).cpu().numpy()
        assert table.shape == (2, 16) and not np.isnan(table).any(), name
        with open(log / "stanford_results.csv") as f:
            rows = list(csv.reader(f))
        assert rows[0] == localize.STANFORD_HEADER and [r[4] for r in rows[1:]] == ["0", "0"]
        assert len(seen) == 2 and seen[0][0] is seen[1][0]                      # one cloud for both images of the room
        if name == "voxel":
            assert seen[0][0].shape[0] == len(read[1]) < len(xyz) and seen[0][1] is None and seen[1][1] is None
        else:
            assert seen[0][0].shape[0] == len(xyz) and seen[0][1] is not None and seen[0][1] is seen[1][1]
            assert same_bits(seen[0][1], vh.weights(read[0], read[1], 2))
            assert seen[0][1] is po.density_weights_of(seen[0][0], 0.05, 2)
