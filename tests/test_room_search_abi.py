"""CPU checks of the room-search entry points (ABI 11): each room's plan is its single-room plan, the fuse rule over the rooms' blocks
together, the workspace, the argument checks (all before anything touches a device), and the Stanford harness's room listing."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


DUMMY = 256                                              # a device address that is never dereferenced: sizing / planning are host-only


def _rooms(sizes, cloud=DUMMY, box=DUMMY):
    from piccolo_amd import _lib
    return (_lib.GdRoom * len(sizes))(*[_lib.GdRoom(cloud, n, box) for n in sizes])


def _hyper(**kw):
    from piccolo_amd import _lib
    h = _lib.GdHyper(0.1, 0.8, 5, _lib.GD_BATCH, 0, 0.0, 0, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def _plan_rooms(lib, sizes, per_room, hyper):
    nch, G, fused = (ctypes.c_int * len(sizes))(), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.pcl_gd_plan_rooms(_rooms(sizes), len(sizes), per_room, ctypes.byref(hyper), nch, ctypes.byref(G), ctypes.byref(fused))
    return rc, list(nch), G.value, fused.value


def _plan(lib, n, B):
    nch, G, fused = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.pcl_gd_plan(n, B, ctypes.byref(nch), ctypes.byref(G), ctypes.byref(fused)) == 0
    return nch.value, G.value, fused.value


SHAPES = [((700, 120_000, 166_667), 6), ((166_667,) * 8, 6), ((1_000_000,) * 4, 32), ((50, 3000, 2_500_000), 5), ((166_667,), 6),
          ((4096, 4097, 10_000, 300_000, 1_000_000), 1)]


@pytest.mark.parametrize("sizes,per_room", SHAPES)
def test_every_room_runs_its_single_room_plan(lib, sizes, per_room):
    rc, nch, G, _ = _plan_rooms(lib, sizes, per_room, _hyper())
    assert rc == 0
    for n, c in zip(sizes, nch):
        c1, G1, _ = _plan(lib, n, per_room)
        assert (c, G) == (c1, G1), (n, c, c1, G, G1)
        assert c % 8 == 0


@pytest.mark.parametrize("sizes,per_room", SHAPES)
def test_fused_exactly_when_all_rooms_blocks_fit_and_fuse_minus_one_clears_it(lib, sizes, per_room):
    _, nch, G, fused = _plan_rooms(lib, sizes, per_room, _hyper())
    blocks = sum(c * (per_room // G) for c in nch)
    assert fused == (1 if blocks <= 1024 else 0), (blocks, fused)
    assert _plan_rooms(lib, sizes, per_room, _hyper(fuse=-1))[3] == 0
    if len(sizes) == 1:
        assert fused == _plan(lib, sizes[0], per_room)[2]


@pytest.mark.parametrize("sizes,per_room", SHAPES)
def test_workspace_holds_every_rooms_partials_twice(lib, sizes, per_room):
    h = _hyper()
    ws = lib.pcl_gd_rooms_workspace_bytes(_rooms(sizes), len(sizes), per_room, ctypes.byref(h))
    _, nch, _, _ = _plan_rooms(lib, sizes, per_room, h)
    partials = sum(c * per_room * 8 * 4 for c in nch)
    assert ws >= 2 * partials
    # (the single-room workspace of each room, summed, is what the room partials need: no more than the table and alignment on top)
    assert ws <= sum(lib.pcl_gd_workspace_bytes(n, per_room, 64, 128, ctypes.byref(h)) for n in sizes) + 4096 + 512 * len(sizes)


def test_room_entry_points_refuse_bad_arguments(lib):
    from piccolo_amd import _lib
    vp = ctypes.c_void_p
    h = _hyper()
    ok = _rooms([1000, 2000])
    rc_plan = lambda rooms, nr, per, hy: lib.pcl_gd_plan_rooms(rooms, nr, per, ctypes.byref(hy) if hy is not None else None, None, None, None)  # noqa: E731
    ws = lambda rooms, nr, per, hy: lib.pcl_gd_rooms_workspace_bytes(rooms, nr, per, ctypes.byref(hy) if hy is not None else None)  # noqa: E731

    def run(rooms, nr, per, hy, pano=vp(DUMMY), state=vp(DUMMY), work=vp(DUMMY)):
        return lib.pcl_gd_run_rooms(rooms, nr, pano, _lib.PANO_F16, 64, 128, state, per, ctypes.byref(hy) if hy is not None else None, 10, None,
                                    work, 1 << 30, None, None)
    assert rc_plan(ok, 2, 6, h) == 0 and ws(ok, 2, 6, h) > 0
    bad = [
        (ok, 0, 6, h), (_rooms([1000] * 33), 33, 6, h), (ok, -1, 6, h),                 # nrooms outside 1..32
        (ok, 2, 0, h),                                                                   # no candidates
        (_rooms([1000, 0]), 2, 6, h), (_rooms([1000, -5]), 2, 6, h),                     # n <= 0
        (_rooms([1000, (1 << 27) + 1]), 2, 6, h),                                        # n > PCL_MAX_POINTS
        (_rooms([1000, 2000], cloud=None), 2, 6, h), (_rooms([1000, 2000], box=None), 2, 6, h),   # null cloud / box
        (ok, 2, 6, _hyper(depth_mask=1)),                                                # depth mask
        (ok, 2, 6, _hyper(color_sets=2)),                                                # colour sets
        (None, 2, 6, h), (ok, 2, 6, None),                                               # null arguments
    ]
    for args in bad:
        assert rc_plan(*args) == -1, args
        assert ws(*args) == 0, args
        assert run(*args) == -1, args
    assert lib.pcl_gd_plan_rooms(_rooms([(1 << 27)]), 1, 6, ctypes.byref(h), None, None, None) == 0      # the largest cloud is accepted
    # null panorama / state / workspace, a bad mode: refused before any HIP call
    assert run(ok, 2, 6, h, pano=None) == -1 and run(ok, 2, 6, h, state=None) == -1 and run(ok, 2, 6, h, work=None) == -1
    assert run(ok, 2, 6, _hyper(mode=7)) == -1
    assert lib.pcl_gd_run_rooms(ok, 2, vp(DUMMY), _lib.PANO_F16, 64, 128, vp(DUMMY), 6, ctypes.byref(h), 10, None, vp(DUMMY), 16, None, None) == -2


def test_stanford_room_listing_is_sorted_and_restricted_by_a_list(tmp_path):
    from piccolo_amd import localize
    d = tmp_path / "pcd_not_aligned" / "area_5"
    os.makedirs(d)
    for name in ("office_10", "hallway_2", "office_2", "WC_1", "conferenceRoom_1"):
        (d / (name + ".txt")).write_text("0 0 0 1 1 1\n")
    (d / "notes.md").write_text("not a room\n")
    os.makedirs(tmp_path / "pcd_not_aligned" / "area_6")
    (tmp_path / "pcd_not_aligned" / "area_6" / "lounge_1.txt").write_text("0 0 0 1 1 1\n")
    allr = localize.stanford_area_rooms(str(tmp_path), 5, True)
    assert allr == sorted(["office_10", "hallway_2", "office_2", "WC_1", "conferenceRoom_1"])
    assert localize.stanford_area_rooms(str(tmp_path), 5, ["office_2", "WC_1", "lounge_1"]) == ["WC_1", "office_2"]
    assert localize.stanford_area_rooms(str(tmp_path), 6, True) == ["lounge_1"]
    assert localize.stanford_area_rooms(str(tmp_path), 7, True) == []


def test_room_search_refuses_images_per_launch(tmp_path):
    from conftest import Cfg
    from piccolo_amd import localize
    cfg = Cfg(dataset="Stanford2D-3D-S", room_search=True, images_per_launch=4, area=None, room_name=None)
    with pytest.raises(ValueError, match="images_per_launch"):
        localize.localize_stanford(cfg, log_dir=None, root=str(tmp_path))
