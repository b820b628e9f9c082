"""CPU checks of the voxel grid's boundary: the four symbols are declared, bound and exported under ABI 12, every documented PCL_EINVAL is
answered before any device call (bogus non-null pointers, no device here), the numpy model of tests/voxel_helpers.py agrees with a
loop-per-point model of the same text, and synth.scanned_room is deterministic and density-skewed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_helpers as vh
from conftest import REPO

SYMBOLS = ("pcl_voxel_workspace_bytes", "pcl_voxel_grid", "pcl_voxel_centroids", "pcl_density_weights")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "piccolo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcl_[a-z0-9_]+)\s*\(", header))
    exported = set(re.findall(r"\bT (pcl_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert _lib.ABI_VERSION == 12 and lib.pcl_abi_version() == 12
    assert "#define PCL_ABI_VERSION 12" in open(os.path.join(REPO, "include", "piccolo_hip.h")).read()
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_voxel_key_kernel", b"pcl_voxel_finish_kernel", b"pcl_voxel_sums_kernel", b"pcl_density_weights_kernel"):
        assert kernel in blob, kernel


def test_workspace_query(lib):
    assert lib.pcl_voxel_workspace_bytes(0) == 0 and lib.pcl_voxel_workspace_bytes(-5) == 0
    assert lib.pcl_voxel_workspace_bytes((1 << 27) + 1) == 0
    sizes = [lib.pcl_voxel_workspace_bytes(n) for n in (1, 4096, 166_667, 1_000_000, 10_000_000)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes)
    # a small multiple of the cloud (24 bytes per point): the six int64 sums per voxel are the larger of the two layouts
    for n in (1_000_000, 10_000_000):
        assert 48 * n <= lib.pcl_voxel_workspace_bytes(n) <= 49 * n, lib.pcl_voxel_workspace_bytes(n) / n


def test_every_refusal_comes_before_a_device_call(lib):
    """bogus non-null pointers: a call that went on to the device would fault, and there is no device here"""
    P = ctypes.c_void_p(0x1000)
    n, big = 100, 1 << 20
    good_grid = [P, n, 0.05, P, P, P, P, P, P, big, None]
    assert lib.pcl_voxel_grid(*[None if k == 0 else a for k, a in enumerate(good_grid)]) == -1
    for k in (0, 3, 4, 5, 6, 7, 8):                                        # every pointer in turn
        args = list(good_grid)
        args[k] = None
        assert lib.pcl_voxel_grid(*args) == -1, k
    for bad_n in (0, -1, (1 << 27) + 1):
        assert lib.pcl_voxel_grid(P, bad_n, 0.05, P, P, P, P, P, P, big, None) == -1
    for voxel in (0.0, -0.05, float("nan"), float("inf"), -float("inf")):
        assert lib.pcl_voxel_grid(P, n, voxel, P, P, P, P, P, P, big, None) == -1, voxel
    assert lib.pcl_voxel_grid(P, n, 0.05, P, P, P, P, P, P, lib.pcl_voxel_workspace_bytes(n) - 1, None) == -2       # PCL_EWORKSPACE

    good_cen = [P, P, n, P, P, 10, P, P, P, P, big, None]
    for k in (0, 1, 3, 4, 6, 7, 8, 9):
        args = list(good_cen)
        args[k] = None
        assert lib.pcl_voxel_centroids(*args) == -1, k
    for bad_n, nvox in ((0, 10), (-3, 10), ((1 << 27) + 1, 10), (n, 0), (n, -1), (n, n + 1)):
        assert lib.pcl_voxel_centroids(P, P, bad_n, P, P, nvox, P, P, P, P, big, None) == -1, (bad_n, nvox)
    assert lib.pcl_voxel_centroids(P, P, n, P, P, 10, P, P, P, P, lib.pcl_voxel_workspace_bytes(n) - 1, None) == -2

    good_w = [P, P, n, 10, 1, P, None]
    for k in (0, 1, 5):
        args = list(good_w)
        args[k] = None
        assert lib.pcl_density_weights(*args) == -1, k
    for bad_n, nvox, cap in ((0, 10, 1), (-1, 10, 1), (n, 0, 1), (n, n + 1, 1), (n, 10, 0), (n, 10, -2)):
        assert lib.pcl_density_weights(P, P, bad_n, nvox, cap, P, None) == -1, (bad_n, nvox, cap)


def test_python_surface_refuses_on_the_host():
    """ValueError before a device is asked for: an empty cloud, a bad voxel, a bad cap, a list of colour sets, an unknown how"""
    import torch
    from piccolo_amd import omniloc, ops, utils
    xyz = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="empty point cloud"):
        ops.VoxelGrid(torch.zeros(0, 3), 0.05)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        ops.VoxelGrid(torch.zeros(4, 2), 0.05)
    for voxel in (0, -1.0, float("nan"), float("inf"), "0.05", None, True):
        with pytest.raises(ValueError, match="positive finite"):
            ops.VoxelGrid(xyz, voxel)
        with pytest.raises(ValueError, match="positive finite"):
            utils.density_weights(xyz, voxel)
        with pytest.raises(ValueError, match="positive finite"):
            omniloc.density_weights_of(xyz, voxel)
    for cap in (0, -1, 1.0, True, None, "2"):
        with pytest.raises(ValueError, match="int >= 1"):
            omniloc.density_weights_of(xyz, 0.05, cap)
        with pytest.raises(ValueError, match="int >= 1"):
            ops.density_cap(cap)
    with pytest.raises(ValueError, match="colour sets"):
        utils.voxel_downsample(xyz, [xyz, xyz], 0.05)
    with pytest.raises(ValueError, match="how"):
        utils.voxel_downsample(xyz, xyz, 0.05, how="mean")
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        utils.voxel_downsample(xyz, torch.zeros(3, 3), 0.05)


# ------------------------------------------------------------------------------------------------ the model itself
def _points(n, seed, voxel):
    """n float32 points in a few dozen voxels around 0, with duplicates, values on cell faces and -0.0"""
    rng = np.random.default_rng(seed)
    xyz = ((rng.random((n, 3)) - 0.5) * 6 * voxel).astype(np.float32)
    xyz[::7] = xyz[3]                                                     # exact duplicates
    k = rng.integers(-3, 4, size=(n // 5, 3))
    xyz[1::5][: len(k)] = (k * np.float64(voxel)).astype(np.float32)       # on faces, as float32 sees them
    xyz[2, 0], xyz[4, 1] = -0.0, 0.0
    rgb = rng.random((n, 3)).astype(np.float32)
    return xyz, rgb


@pytest.mark.parametrize("voxel,cap,seed", [(0.05, 1, 0), (0.05, 3, 1), (0.25, 2, 2), (1.0 / 3.0, 1, 3)])
def test_numpy_model_equals_the_loop_per_point_model(voxel, cap, seed):
    xyz, rgb = _points(300, seed, voxel)
    cell, count, first = vh.grid(xyz, voxel)
    b_cell, b_count, b_first, b_xyz, b_rgb, b_w = vh.brute(xyz, rgb, voxel, cap)
    assert cell.dtype == np.int32 and count.dtype == np.int32 and first.dtype == np.int64
    assert np.array_equal(cell, b_cell) and np.array_equal(count, b_count) and np.array_equal(first, b_first)
    assert 1 < len(count) < 300 and count.sum() == 300 and (np.diff(first) > 0).all() and count.max() > cap
    assert np.array_equal(vh.centroids(xyz, cell, count).view(np.uint32), b_xyz.view(np.uint32))
    assert np.array_equal(vh.centroids(rgb, cell, count).view(np.uint32), b_rgb.view(np.uint32))
    assert np.array_equal(vh.weights(cell, count, cap).view(np.uint32), b_w.view(np.uint32))
    fx, fr, fc, ff = vh.downsample(xyz, rgb, voxel, how="first")
    assert np.array_equal(fx.view(np.uint32), xyz[b_first].view(np.uint32)) and np.array_equal(fr.view(np.uint32), rgb[b_first].view(np.uint32))
    assert np.array_equal(fc, b_count) and np.array_equal(ff, b_first)


def test_model_cells_on_faces_and_signs():
    """the cases the rules name: 0.05f / 0.05 -> 1, -0.05f / 0.05 -> -2, -0.0 -> 0, floor for negatives"""
    xyz = np.array([[0.05, -0.05, -0.0], [-0.01, 0.0, 0.049], [-0.051, 0.1, -0.1]], np.float32)
    assert vh.cells(xyz, 0.05).tolist() == [[1, -2, 0], [-1, 0, 0], [-2, 2, -3]]
    assert vh.bad_bits(np.array([1.0, np.nan], np.float32), 0.05) == vh.BAD_NONFINITE
    assert vh.bad_bits(np.array([1.0, -np.inf], np.float32), 0.05) == vh.BAD_NONFINITE
    assert vh.bad_bits(np.array([16384.0], np.float32), 2.0 ** -6) == vh.BAD_CELL                       # cell 2^20: one too far
    assert vh.bad_bits(np.array([-16384.0, 16384.0 - 2.0 ** -6], np.float32), 2.0 ** -6) == 0            # cells -2^20 and 2^20 - 1
    assert vh.bad_bits(np.array([0.05 * (1 << 20)], np.float32), 0.05) == vh.BAD_CELL | vh.BAD_MAGNITUDE
    assert vh.bad_bits(np.array([40000.0], np.float32), 0.05) == vh.BAD_MAGNITUDE
    assert vh.bad_bits(np.array([40000.0], np.float32)) == vh.BAD_MAGNITUDE and vh.bad_bits(np.array([32767.9], np.float32), 0.05) == 0


# ------------------------------------------------------------------------------------------------ the density-skewed scene
def test_scanned_room_is_deterministic_and_skewed():
    from piccolo_amd import synth
    n = 60_000
    xyz, rgb = synth.scanned_room(n, seed=3)
    again = synth.scanned_room(n, seed=3)
    assert xyz.shape == rgb.shape == (n, 3) and xyz.dtype == rgb.dtype == np.float32
    assert np.array_equal(xyz, again[0]) and np.array_equal(rgb, again[1])
    assert not np.array_equal(xyz, synth.scanned_room(n, seed=4)[0])
    # on the room's faces, coloured by box_room's field
    on_face = np.isclose(np.abs(xyz), (synth.ROOM / 2)[None, :].astype(np.float32)).any(axis=1)
    assert on_face.all() and (np.abs(xyz) <= (synth.ROOM / 2 + 1e-6)[None, :]).all()
    assert np.abs(rgb - (0.5 + 0.45 * np.sin(xyz.astype(np.float64) @ synth._K.T + synth._PHI))).max() < 1e-5    # (the field, from the float32 points)
    # 5 cm voxels: the scan's counts are more skewed than the uniform-by-area room's
    skew = {}
    for name, cloud in (("scan", xyz), ("box", synth.box_room(n, seed=3)[0])):
        count = vh.grid(cloud, 0.05)[1]
        skew[name] = count.max() / np.median(count)
    assert skew["scan"] > 1.5 * skew["box"], skew
    # and denser near the scanner: the floor under it against the far wall
    s = np.array(synth.SCANNER)
    near = np.linalg.norm(xyz - s[None, :], axis=1) < 1.5
    far = xyz[:, 0] > synth.ROOM[0] / 2 - 1e-3
    assert near.sum() > far.sum()
    with pytest.raises(ValueError, match="inside the room"):
        synth.scanned_room(100, scanner=(5.0, 0.0, 0.0))

