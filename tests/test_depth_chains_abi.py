"""CPU checks of the depth-chain entry points (the depth mask inside a shared chain; additive to ABI 12): the three symbols, the plan (the
rooms x images plan of the same hyper-parameters without the mask, never fused), every room's own z-buffer grid and occluder stride, the
workspace, and the argument checks — all before anything touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

from test_room_search_abi import DUMMY, SHAPES, _hyper, _rooms

IMAGES = (1, 3, 8)
H, W = 256, 512
NAMES = ("pcl_gd_depth_chain_workspace_bytes", "pcl_gd_plan_depth_chain", "pcl_gd_run_depth_chain")
GRIDS = ((0, 0, 0), (0, 0, 1), (64, 128, 1), (24, 40, 0), (16, 32, 4))          # (depth_h, depth_w, depth_stride) of the hyper-parameters


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def _depth_hyper(dh=0, dw=0, stride=0, **kw):
    return _hyper(depth_mask=1, depth_tau=0.05, depth_h=dh, depth_w=dw, depth_stride=stride, **kw)


def _plan_dc(lib, sizes, nimages, per_image, hyper):
    arr = lambda: (ctypes.c_int * len(sizes))()      # noqa: E731
    nch, dh, dw, st, G = arr(), arr(), arr(), arr(), ctypes.c_int(-1)
    rc = lib.pcl_gd_plan_depth_chain(_rooms(sizes), len(sizes), nimages, per_image, H, W, ctypes.byref(hyper), nch, ctypes.byref(G), dh, dw, st)
    return rc, list(nch), G.value, list(zip(dh, dw, st))


def _default(lib, n, stride):
    dh, dw, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.pcl_depth_default(n, H, W, stride, ctypes.byref(dh), ctypes.byref(dw), None, ctypes.byref(st)) == 0
    return dh.value, dw.value, st.value


def test_the_three_symbols_exist_and_the_abi_is_still_12(lib):
    from piccolo_amd import _lib
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(here, "include", "piccolo_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes, name
        assert re.search(r" T %s$" % name, exported, re.M), name
    assert lib.pcl_abi_version() == _lib.ABI_VERSION == 12


@pytest.mark.parametrize("nimages", IMAGES)
@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_plan_is_the_rooms_images_plan_without_the_mask(lib, sizes, per_image, nimages):
    for sets in (0, 1, nimages):
        rc, nch, G, _ = _plan_dc(lib, sizes, nimages, per_image, _depth_hyper(color_sets=sets))
        assert rc == 0
        nch0, G0 = (ctypes.c_int * len(sizes))(), ctypes.c_int(-1)
        h0 = _hyper(color_sets=sets)
        assert lib.pcl_gd_plan_rooms_images(_rooms(sizes), len(sizes), nimages, per_image, ctypes.byref(h0), nch0, ctypes.byref(G0), None) == 0
        assert (nch, G) == (list(nch0), G0.value)


@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_every_room_resolves_its_own_grid_and_stride(lib, sizes, per_image):
    for dh, dw, stride in GRIDS:
        rc, _, _, grids = _plan_dc(lib, sizes, 3, per_image, _depth_hyper(dh, dw, stride))
        assert rc == 0
        for n, got in zip(sizes, grids):
            want = _default(lib, n, stride) if dh == 0 else (dh, dw, stride if stride else 1)
            assert got == want, (n, got, want)


def test_default_grids_of_the_documented_sizes(lib):
    _, _, _, grids = _plan_dc(lib, (700, 30_000, 60_000, 166_667), 2, 6, _depth_hyper())
    assert [g[:2] for g in grids] == [(16, 32), (32, 64), (48, 96), (80, 160)]


@pytest.mark.parametrize("nimages", IMAGES)
@pytest.mark.parametrize("sizes,per_image", SHAPES)
def test_workspace_holds_one_partials_buffer_and_two_zbuffer_sets(lib, sizes, per_image, nimages):
    for dh, dw, stride in GRIDS[:3]:
        for sets in (0, nimages):
            h = _depth_hyper(dh, dw, stride, color_sets=sets)
            ws = lib.pcl_gd_depth_chain_workspace_bytes(_rooms(sizes), len(sizes), nimages, per_image, H, W, ctypes.byref(h))
            rc, nch, _, grids = _plan_dc(lib, sizes, nimages, per_image, h)
            assert rc == 0 and ws > 0
            h0 = _hyper(color_sets=sets)
            plain = lib.pcl_gd_rooms_images_workspace_bytes(_rooms(sizes), len(sizes), nimages, per_image, ctypes.byref(h0))
            partials = sum(-(-c * nimages * per_image * 8 * 4 // 256) * 256 for c in nch)       # (each room's region 256-byte aligned)
            zsets = 2 * sum(nimages * per_image * gh * gw * 4 for gh, gw, _ in grids)
            assert ws >= plain - partials + zsets, (ws, plain, partials, zsets)
            single = len(sizes) == 1 and nimages == 1   # forwarded to pcl_gd_run: its workspace (two partials buffers) fits as well
            assert ws <= plain - partials + zsets + 8192 + 32 * len(sizes) + (partials if single else 0)    # tables and alignment, nothing else
            if single:
                h1 = _depth_hyper(dh, dw, stride)
                assert ws >= lib.pcl_gd_workspace_bytes(sizes[0], per_image, H, W, ctypes.byref(h1))


def test_depth_chain_entry_points_refuse_bad_arguments(lib):
    from piccolo_amd import _lib
    vp = ctypes.c_void_p
    h = _depth_hyper()
    ok = _rooms([1000, 2000])
    ref = lambda hy: ctypes.byref(hy) if hy is not None else None  # noqa: E731
    rc_plan = lambda rooms, nr, ni, per, hy: lib.pcl_gd_plan_depth_chain(rooms, nr, ni, per, H, W, ref(hy), None, None, None, None, None)  # noqa: E731
    ws = lambda rooms, nr, ni, per, hy: lib.pcl_gd_depth_chain_workspace_bytes(rooms, nr, ni, per, H, W, ref(hy))  # noqa: E731

    def run(rooms, nr, ni, per, hy, pano=vp(DUMMY), state=vp(DUMMY), work=vp(DUMMY), work_bytes=1 << 40):
        return lib.pcl_gd_run_depth_chain(rooms, nr, ni, pano, _lib.PANO_F16, H, W, state, per, ref(hy), 10, None, work, work_bytes, None, None)
    for hy in (h, _depth_hyper(color_sets=1), _depth_hyper(color_sets=3), _depth_hyper(64, 128, 1)):
        assert rc_plan(ok, 2, 3, 6, hy) == 0 and ws(ok, 2, 3, 6, hy) > 0
    big = 30_000_000
    bad = [
        (ok, 2, 3, 6, _hyper()), (ok, 2, 3, 6, _hyper(color_sets=3)),                        # depth_mask == 0
        (None, 2, 3, 6, h), (ok, 2, 3, 6, None),                                             # null arguments
        (ok, 0, 3, 6, h), (_rooms([1000] * 33), 33, 3, 6, h), (ok, -1, 3, 6, h),             # nrooms outside 1..32
        (ok, 2, 0, 6, h), (ok, 2, -2, 6, h), (ok, 2, 3, 0, h), (ok, 2, 3, -1, h),            # nimages < 1, per_image < 1
        (ok, 2, 3, 6, _depth_hyper(color_sets=2)), (ok, 2, 3, 6, _depth_hyper(color_sets=4)), (ok, 2, 3, 6, _depth_hyper(color_sets=-1)),
        (_rooms([1000, big]), 2, 8, 6, _depth_hyper(color_sets=8)),                          # a room whose 8 sets pass 2^31 bytes
        (ok, 2, 3, 6, _depth_hyper(1, 1)), (ok, 2, 3, 6, _depth_hyper(0, 64)), (ok, 2, 3, 6, _depth_hyper(64, 0)),   # 1 x 1 grid, half a grid
        (ok, 2, 3, 6, _depth_hyper(-8, -16)), (ok, 2, 3, 6, _depth_hyper(stride=65)), (ok, 2, 3, 6, _depth_hyper(stride=-1)),
        (ok, 2, 8, 8, _depth_hyper(4096, 4096)),                                             # 64 z-buffers of 64 MiB per room: 4 GiB
        (_rooms([1000, 0]), 2, 3, 6, h), (_rooms([1000, (1 << 27) + 1]), 2, 3, 6, h),        # n outside 1..PCL_MAX_POINTS
        (_rooms([1000, 2000], cloud=None), 2, 3, 6, h), (_rooms([1000, 2000], box=None), 2, 3, 6, h),   # null cloud / box
    ]
    for args in bad:
        assert rc_plan(*args) == -1, args
        assert ws(*args) == 0, args
        assert run(*args) == -1, args
    assert rc_plan(ok, 2, 7, 8, _depth_hyper(4096, 4096)) == 0                               # (56 z-buffers of 64 MiB: below 4 GiB per room)
    tau_bad = _depth_hyper()
    tau_bad.depth_tau = -0.5
    assert rc_plan(ok, 2, 3, 6, tau_bad) == -1 and run(ok, 2, 3, 6, tau_bad) == -1
    assert run(ok, 2, 3, 6, h, pano=None) == -1 and run(ok, 2, 3, 6, h, state=None) == -1 and run(ok, 2, 3, 6, h, work=None) == -1
    assert run(ok, 2, 3, 6, _depth_hyper(mode=7)) == -1
    assert run(ok, 2, 3, 6, h, work_bytes=16) == -2
    for args in [(ok, 2, 3, 6, _depth_hyper(color_sets=3)), (ok, 2, 1, 5, h), (_rooms([1000]), 1, 1, 6, h), (_rooms([1000]), 1, 4, 6, h)]:
        assert run(*args, work_bytes=ws(*args) - 1) == -2, args


def test_the_other_families_still_refuse_a_depth_masked_hyper(lib):
    ok = _rooms([1000, 2000])
    h = _depth_hyper()
    assert lib.pcl_gd_plan_rooms(ok, 2, 6, ctypes.byref(h), None, None, None) == -1
    assert lib.pcl_gd_plan_rooms_images(ok, 2, 3, 6, ctypes.byref(h), None, None, None) == -1
    hs = _depth_hyper(color_sets=3)
    assert lib.pcl_gd_workspace_bytes(1000, 18, H, W, ctypes.byref(hs)) == 0
    assert lib.pcl_gd_plan_hyper(1000, 18, ctypes.byref(hs), None, None, None) == -1


def test_rooms_share_a_depth_chain_when_their_tolerances_agree(lib):
    """the chain has ONE depth_tau; a room on its own takes the rule's tolerance of its own default grid (0.15 up to 72 rows)"""
    from conftest import Cfg
    from piccolo_amd import omniloc as po
    from piccolo_amd import ops
    small, large = [700, 30_000, 60_000, 100_000], [166_667, 1_000_000, 166_667]
    assert po.depth_tau_groups(small + large, 1024, 2048, Cfg()) == [list(range(7))]                      # no mask: nothing to agree on
    cfg = Cfg(depth_mask=True)
    assert po.depth_tau_groups(small, 1024, 2048, cfg) == [[0, 1, 2, 3]]
    assert {ops._depth_args(n, 1024, 2048, None, None)[2] for n in small} == {0.15000000596046448}
    assert po.depth_tau_groups(small + large, 1024, 2048, cfg) == [[0, 1, 2, 3], [4, 6], [5]]
    assert po.depth_tau_groups(small + large, 1024, 2048, Cfg(depth_mask=True, depth_tau=0.05)) == [list(range(7))]
    assert po.depth_tau_groups(small + large, 1024, 2048, Cfg(depth_mask=True, depth_res=[64, 128])) == [list(range(7))]
    with pytest.raises(ValueError, match="one tolerance"):
        ops._chain_depth_args(small + large, 1024, 2048, None, None)
    assert ops._chain_depth_args(small, 1024, 2048, None, None, 2)[:2] + ops._chain_depth_args(small, 1024, 2048, None, None, 2)[3:] == (0, 0, 2)
    assert ops._chain_depth_args(small + large, 1024, 2048, (64, 128), None) == (64, 128, ops.depth_tau_rule(64), 1)


def test_engine_arguments_from_cfg(lib):
    """what omniloc hands every GD engine for a cfg, written out; and the tolerance groups that read the same values"""
    from conftest import Cfg
    from piccolo_amd import omniloc as po
    assert po._engine_args(Cfg(), True) == dict(lr=0.1, patience=5, factor=0.9, batch_mode=True, fuse=None, depth_mask=False, depth_tau=None,
                                                depth_res=None, depth_stride=None)
    assert po._engine_args(Cfg(lr=0.05, patience=3, factor=0.8, gd_fuse=True, depth_mask=True), False) == dict(
        lr=0.05, patience=3, factor=0.8, batch_mode=False, fuse=None, depth_mask=True, depth_tau=None, depth_res=None, depth_stride=None)
    got = po._engine_args(Cfg(lr=1, patience=7.0, factor=1, gd_fuse=False, depth_mask=1, depth_tau=1, depth_res=[64.0, 128.0], depth_stride=2.0), 1)
    want = dict(lr=1.0, patience=7, factor=1.0, batch_mode=True, fuse=False, depth_mask=True, depth_tau=1.0, depth_res=(64, 128), depth_stride=2)
    assert got == want and [type(v) for v in got.values()] == [type(v) for v in want.values()]
    assert list(got) == ["lr", "patience", "factor", "batch_mode", "fuse", "depth_mask", "depth_tau", "depth_res", "depth_stride"]
    # without the mask its optional values still travel (the engines ignore them), with gd_fuse alone nothing else moves
    assert po._engine_args(Cfg(depth_tau=0.05, depth_res=(32, 64), depth_stride=4, gd_fuse=0)) == dict(
        lr=0.1, patience=5, factor=0.9, batch_mode=True, fuse=False, depth_mask=False, depth_tau=0.05, depth_res=(32, 64), depth_stride=4)
    points = [2_000, 160_000, 1_000_000]
    assert po.depth_tau_groups(points, 256, 512, Cfg(depth_mask=True)) == [[0], [1], [2]]          # (every room its own default grid: 3 tolerances)
    assert po.depth_tau_groups(points, 256, 512, Cfg(depth_mask=True, depth_tau=0.05)) == [[0, 1, 2]]
    assert po.depth_tau_groups(points, 256, 512, Cfg(depth_tau=0.05)) == [[0, 1, 2]]


def test_shared_colour_depth_chain_cut_off_sits_between_the_measured_wins_and_the_measured_loss():
    """with the depth mask and shared colours, one chain won at 2..7 images x 6 candidates per room and lost at 8 x 6"""
    from piccolo_amd import omniloc as po
    assert all(po.depth_shared_chain_pays(i, 6) for i in range(2, 8))
    assert not po.depth_shared_chain_pays(8, 6)
    assert not po.depth_shared_chain_pays(2, 32)          # (not measured: the route it had)
