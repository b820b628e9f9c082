"""CPU checks of the per-image colour-set entry points (ABI 10): the 32-bit addressing limit of the cloud's sizing function and the
argument checks, before anything touches a device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_cloud_sets_bytes_respects_the_32_bit_limit(lib):
    from piccolo_amd import ops
    for n in (1000, 120_000, 1_000_000, 10_000_000):
        plane = 4 * lib.pcl_cloud_stride(n)
        assert lib.pcl_cloud_sets_bytes(n, 1) == lib.pcl_cloud_bytes(n)
        assert lib.pcl_cloud_sets_bytes(n, 3) == plane * 12
        k = ops.max_color_sets(n)
        assert (3 + 3 * k) * plane < 1 << 31 <= (6 + 3 * k) * plane
        assert lib.pcl_cloud_sets_bytes(n, k) == (3 + 3 * k) * plane and lib.pcl_cloud_sets_bytes(n, k + 1) == 0
    assert 160 <= ops.max_color_sets(1_000_000) <= 180 and ops.max_color_sets(10_000_000) == 16
    # the largest cloud keeps its one colour set (pcl_cloud_pack's limits), but has no room for a second
    assert lib.pcl_cloud_sets_bytes(1 << 27, 1) == lib.pcl_cloud_bytes(1 << 27) and lib.pcl_cloud_sets_bytes(1 << 27, 2) == 0
    assert lib.pcl_cloud_sets_bytes(0, 2) == 0 and lib.pcl_cloud_sets_bytes(1000, 0) == 0 and lib.pcl_cloud_sets_bytes((1 << 27) + 1, 1) == 0


def test_color_set_entry_points_reject_bad_arguments(lib):
    vp = ctypes.c_void_p
    dummy = vp(256)                                      # never dereferenced: every call below fails its argument checks first
    rgbs = (vp * 2)(dummy, dummy)
    assert lib.pcl_cloud_pack_sets(None, rgbs, 2, None, 1000, dummy, None) == -1
    assert lib.pcl_cloud_pack_sets(dummy, None, 2, None, 1000, dummy, None) == -1
    assert lib.pcl_cloud_pack_sets(dummy, rgbs, 2, None, 1000, None, None) == -1
    assert lib.pcl_cloud_pack_sets(dummy, (vp * 2)(dummy, None), 2, None, 1000, dummy, None) == -1
    assert lib.pcl_cloud_pack_sets(dummy, rgbs, 0, None, 1000, dummy, None) == -1
    many = (vp * 17)(*([dummy] * 17))
    assert lib.pcl_cloud_pack_sets(dummy, many, 17, None, 10_000_000, dummy, None) == -1             # 17 sets of 10M points: past 2^31 bytes
    panos = (vp * 3)(dummy, dummy, dummy)
    # colour sets must be 1 or the image count
    assert lib.pcl_trim_loss_images_sets(dummy, 1000, 2, panos, 3, 1, 64, 128, dummy, 4, dummy, 4, dummy, 1, None, dummy, None, dummy, 1 << 20,
                                         None) == -1
    assert lib.pcl_hist_trim_images_sets_workspace_bytes(1000, 2, 3, 8, 64, 128, 4, 4) == 0
    assert lib.pcl_hist_trim_images_sets_workspace_bytes(1000, 3, 3, 8, 64, 128, 4, 4) > lib.pcl_hist_trim_images_workspace_bytes(1000, 3, 8, 64, 128, 4, 4)
    assert lib.pcl_hist_trim_images_sets_workspace_bytes(1000, 1, 3, 8, 64, 128, 4, 4) == lib.pcl_hist_trim_images_workspace_bytes(1000, 3, 8, 64, 128, 4, 4)
    assert lib.pcl_hist_trim_scores_images_sets(dummy, 1000, 2, (ctypes.c_void_p * 3)(dummy, dummy, dummy), 3, 8, 64, 128, dummy, dummy, 4, 4, dummy,
                                                dummy, dummy, dummy, 1 << 20, None) == -1


def test_gd_color_sets_must_split_the_candidates(lib):
    from piccolo_amd import _lib
    ok = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, 3, 3)
    assert lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(ok)) > 0
    # with sets the partials follow the one-image plan of 8 candidates: more chunks than the plan of 24
    shared = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, 3, 0)
    assert lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(ok)) > lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(shared))
    bad = _lib.GdHyper(0.1, 0.8, 5, 1, 0, 0.0, 0, 0, 0, 0, 5, 5)                      # 24 candidates do not split into 5 images
    assert lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(bad)) == 0
    c = ctypes.c_int(0)
    assert lib.pcl_gd_plan_hyper(120_000, 24, ctypes.byref(bad), ctypes.byref(c), None, None) == -1
    # no colour-set kernel with the depth mask: a depth-masked hyper whose grid is valid on its own (explicit 64 x 128 grid, stride 1) is
    # sized without colour sets and refused with them
    depth = _lib.GdHyper(0.1, 0.8, 5, 1, 1, 0.05, 64, 128, 1, 0, 3, 0)
    assert lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(depth)) > 0
    depth.color_sets = 3
    assert lib.pcl_gd_workspace_bytes(120_000, 24, 256, 512, ctypes.byref(depth)) == 0
    assert lib.pcl_gd_plan_hyper(120_000, 24, ctypes.byref(depth), ctypes.byref(c), None, None) == -1
