"""CPU checks of the rooms x images entry points (ABI 12): each room runs its single-room, SINGLE-IMAGE plan for all of its images'
candidates, the fuse rule over the blocks of all rooms and images together, the workspace, the argument checks (all before anything
touches a device), the unchanged pcl_gd_run_rooms, and the harness key room_search_images."""
import ctypes

import pytest

from test_room_search_abi import DUMMY, SHAPES, _hyper, _plan, _rooms

IMAGES = (1, 3, 8)


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def _plan_ri(lib, sizes, nimages, per_image, hyper):
    nch, G, fused = (ctypes.c_int * len(sizes))(), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.pcl_gd_plan_rooms_images(_rooms(sizes), len(sizes), nimages, per_image, ctypes.byref(hyper), nch, ctypes.byref(G), ctypes.byref(fused))
    return rc, list(nch), G.value, fused.value


def _hypers(nimages):
    """shared colours (0 and 1) and per-image sets"""
    return [_hyper(), _hyper(color_sets=1), _hyper(color_sets=nimages)]


def test_abi_version_is_12(lib):
    from piccolo_amd import _lib
    assert lib.pcl_abi_version() == _lib.ABI_VERSION == 12


@pytest.mark.parametrize("nimages", IMAGES)
@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_every_room_runs_its_single_image_plan(lib, sizes, per_image, nimages):
    for h in _hypers(nimages):
        rc, nch, G, _ = _plan_ri(lib, sizes, nimages, per_image, h)
        assert rc == 0
        for n, c in zip(sizes, nch):
            c1, G1, _ = _plan(lib, n, per_image)
            assert (c, G) == (c1, G1), (n, c, c1, G, G1)
            assert c % 8 == 0
            assert per_image % G == 0                    # a group of G poses never straddles two images


@pytest.mark.parametrize("nimages", IMAGES)
@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_fused_exactly_when_all_blocks_fit_and_fuse_minus_one_clears_it(lib, sizes, per_image, nimages):
    for h in _hypers(nimages):
        _, nch, G, fused = _plan_ri(lib, sizes, nimages, per_image, h)
        blocks = sum(c * nimages * per_image // G for c in nch)
        assert fused == (1 if blocks <= 1024 else 0), (blocks, fused)
    assert _plan_ri(lib, sizes, nimages, per_image, _hyper(fuse=-1))[3] == 0


@pytest.mark.parametrize("nimages", IMAGES)
@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_workspace_holds_every_rooms_partials_for_all_images_twice(lib, sizes, per_image, nimages):
    for h in _hypers(nimages):
        ws = lib.pcl_gd_rooms_images_workspace_bytes(_rooms(sizes), len(sizes), nimages, per_image, ctypes.byref(h))
        _, nch, _, _ = _plan_ri(lib, sizes, nimages, per_image, h)
        partials = sum(c * nimages * per_image * 8 * 4 for c in nch)
        assert ws >= 2 * partials
        h1 = _hyper()
        single = sum(lib.pcl_gd_workspace_bytes(n, per_image, 64, 128, ctypes.byref(h1)) for n in sizes)
        assert ws <= nimages * single + 4096 + 512 * len(sizes)
    # one image: the rooms chain's own workspace
    h = _hyper()
    assert lib.pcl_gd_rooms_images_workspace_bytes(_rooms(sizes), len(sizes), 1, per_image, ctypes.byref(h)) == \
        lib.pcl_gd_rooms_workspace_bytes(_rooms(sizes), len(sizes), per_image, ctypes.byref(h))


def test_rooms_images_entry_points_refuse_bad_arguments(lib):
    from piccolo_amd import _lib
    vp = ctypes.c_void_p
    h = _hyper()
    ok = _rooms([1000, 2000])
    ref = lambda hy: ctypes.byref(hy) if hy is not None else None  # noqa: E731
    rc_plan = lambda rooms, nr, ni, per, hy: lib.pcl_gd_plan_rooms_images(rooms, nr, ni, per, ref(hy), None, None, None)  # noqa: E731
    ws = lambda rooms, nr, ni, per, hy: lib.pcl_gd_rooms_images_workspace_bytes(rooms, nr, ni, per, ref(hy))  # noqa: E731

    def run(rooms, nr, ni, per, hy, pano=vp(DUMMY), state=vp(DUMMY), work=vp(DUMMY), work_bytes=1 << 30):
        return lib.pcl_gd_run_rooms_images(rooms, nr, ni, pano, _lib.PANO_F16, 64, 128, state, per, ref(hy), 10, None, work, work_bytes, None, None)
    for hy in (h, _hyper(color_sets=1), _hyper(color_sets=3)):
        assert rc_plan(ok, 2, 3, 6, hy) == 0 and ws(ok, 2, 3, 6, hy) > 0
    big = 30_000_000                                      # 3 + 3 * 8 planes of 30M floats pass 2^31 bytes; one set does not
    assert lib.pcl_cloud_sets_bytes(big, 8) == 0 and lib.pcl_cloud_sets_bytes(big, 1) > 0
    bad = [
        (ok, 2, 3, 6, _hyper(depth_mask=1)),                                                 # depth mask
        (None, 2, 3, 6, h), (ok, 2, 3, 6, None),                                             # null arguments
        (ok, 0, 3, 6, h), (_rooms([1000] * 33), 33, 3, 6, h), (ok, -1, 3, 6, h),             # nrooms outside 1..32
        (ok, 2, 0, 6, h), (ok, 2, -2, 6, h), (ok, 2, 3, 0, h), (ok, 2, 3, -1, h),            # nimages < 1, per_image < 1
        (_rooms([1000, big]), 2, 8, 6, _hyper(color_sets=8)),                                # a room whose 8 sets pass 2^31 bytes
        (ok, 2, 3, 6, _hyper(color_sets=2)), (ok, 2, 3, 6, _hyper(color_sets=4)), (ok, 2, 3, 6, _hyper(color_sets=-1)),   # sets: 0, 1 or nimages
        (_rooms([1000, 0]), 2, 3, 6, h), (_rooms([1000, (1 << 27) + 1]), 2, 3, 6, h),        # n outside 1..PCL_MAX_POINTS
        (_rooms([1000, 2000], cloud=None), 2, 3, 6, h), (_rooms([1000, 2000], box=None), 2, 3, 6, h),   # null cloud / box
    ]
    for args in bad:
        assert rc_plan(*args) == -1, args
        assert ws(*args) == 0, args
        assert run(*args) == -1, args
    assert rc_plan(_rooms([1000, big]), 2, 8, 6, h) == 0                                     # (shared colours: one set per room)
    assert run(ok, 2, 3, 6, h, pano=None) == -1 and run(ok, 2, 3, 6, h, state=None) == -1 and run(ok, 2, 3, 6, h, work=None) == -1
    assert run(ok, 2, 3, 6, _hyper(mode=7)) == -1
    assert run(ok, 2, 3, 6, h, work_bytes=16) == -2
    assert run(ok, 2, 3, 6, _hyper(color_sets=3), work_bytes=ws(ok, 2, 3, 6, _hyper(color_sets=3)) - 1) == -2
    # the init variant checks its arguments too
    init = lambda nr, ni, per, hy, state=vp(DUMMY), tr=vp(DUMMY): lib.pcl_gd_init_rooms_images(state, tr, vp(DUMMY), nr, ni, per, ref(hy), None)  # noqa: E731
    for args in [(0, 3, 6, h), (33, 3, 6, h), (2, 0, 6, h), (2, 3, 0, h), (2, 3, 6, None), (2, 3, 6, _hyper(color_sets=2))]:
        assert init(*args) == -1, args
    assert init(2, 3, 6, h, state=None) == -1 and init(2, 3, 6, h, tr=None) == -1


def test_pcl_gd_run_rooms_still_refuses_colour_sets(lib):
    from piccolo_amd import _lib
    vp = ctypes.c_void_p
    ok = _rooms([1000, 2000])
    h = _hyper(color_sets=2)
    assert lib.pcl_gd_plan_rooms(ok, 2, 6, ctypes.byref(h), None, None, None) == -1
    assert lib.pcl_gd_rooms_workspace_bytes(ok, 2, 6, ctypes.byref(h)) == 0
    assert lib.pcl_gd_run_rooms(ok, 2, vp(DUMMY), _lib.PANO_F16, 64, 128, vp(DUMMY), 6, ctypes.byref(h), 10, None, vp(DUMMY), 1 << 30, None, None) == -1


def test_room_search_images_is_not_images_per_launch(tmp_path):
    """room_search with room_search_images on an empty tree: no query images, and no images_per_launch error"""
    from conftest import Cfg
    from piccolo_amd import localize
    cfg = Cfg(dataset="Stanford2D-3D-S", room_search=True, room_search_images=4, area=None, room_name=None)
    from piccolo_amd._lib import PiccoloHipError
    try:                                                  # past the key checks the harness asks for the device: without one it stops there
        localize.localize_stanford(cfg, log_dir=None, root=str(tmp_path))
    except PiccoloHipError as e:
        assert "needs an MI355X" in str(e), e
    cfg = Cfg(dataset="Stanford2D-3D-S", room_search=True, images_per_launch=4, area=None, room_name=None)
    with pytest.raises(ValueError, match="room_search_images"):
        localize.localize_stanford(cfg, log_dir=None, root=str(tmp_path))


def test_shipped_b8_config_groups_eight_images():
    import os
    from piccolo_amd import parse_utils
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = parse_utils.parse_ini(os.path.join(here, "configs", "stanford_room_search_b8.ini"))
    base = parse_utils.parse_ini(os.path.join(here, "configs", "stanford_room_search.ini"))
    assert cfg.room_search is True and cfg.room_search_images == 8 and not hasattr(cfg, "images_per_launch")
    assert {k: v for k, v in cfg._asdict().items() if k != "room_search_images"} == base._asdict()


def test_chain_size_cut_off_sits_between_the_measured_win_and_the_measured_loss():
    """sharing a chain won at 4 and 8 rooms of 166,667 points x 6 candidates and lost at 4 rooms of 1M points x 32"""
    from piccolo_amd import omniloc as po
    assert po.rooms_images_chain_pays(4 * 166_667, 6) and po.rooms_images_chain_pays(8 * 166_667, 6)
    assert not po.rooms_images_chain_pays(4 * 1_000_000, 32)
