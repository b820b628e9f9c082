"""CPU checks of the rooms boundary of the pose information and the Levenberg-Marquardt polish (additive to ABI 12):
pcl_pose_information_rooms, pcl_gn_refine_rooms and their sizing functions are declared, bound and exported, their kernels are in the
code object, the workspace is the rooms' single-call workspaces one after the other, and every listed refusal answers PCL_EINVAL before
anything touches a device (host-only: dummy addresses, never dereferenced)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_pose_information_rooms_workspace_bytes", "pcl_pose_information_rooms", "pcl_gn_rooms_workspace_bytes", "pcl_gn_refine_rooms")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def _rooms(sizes, hole=None):
    from piccolo_amd import _lib
    return (_lib.GdRoom * len(sizes))(*[_lib.GdRoom(None if r == hole else 0x100000 * (r + 1), n, None) for r, n in enumerate(sizes)])


def _panos(I, hole=None):
    return (ctypes.c_uint64 * I)(*[0 if i == hole else 0x900000 + 0x1000 * i for i in range(I)])


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        lead = r"\b%s\s+%s\s*\(\s*const\s+pcl_gd_room\s*\*\s*rooms_host\s*,\s*int\s+nrooms\s*,"
        if name.endswith("_bytes"):
            assert re.search(lead % ("size_t", name) + r"\s*int\s+nimages\s*\)", text), name
            assert _lib.SIGNATURES[name] == (ctypes.c_size_t, [ctypes.POINTER(_lib.GdRoom), ctypes.c_int, ctypes.c_int])
        else:
            assert re.search(lead % ("int", name) + r"\s*int\s+color_sets\s*,\s*const\s+uint64_t\s*\*\s*panos_host\s*,\s*int\s+nimages\s*,", text), name
            assert _lib.SIGNATURES[name][0] is ctypes.c_int
    # the images bindings with the room array and nrooms in place of cloud, weights, weight_sets and n
    for rooms, images in (("pcl_pose_information_rooms", "pcl_pose_information_images"), ("pcl_gn_refine_rooms", "pcl_gn_refine_images")):
        assert _lib.SIGNATURES[rooms][1] == [ctypes.POINTER(_lib.GdRoom), ctypes.c_int] + _lib.SIGNATURES[images][1][4:]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_pose_info_rooms_kernel", b"pcl_gn_pass_rooms_kernel", b"pcl_pose_info_finish_rooms_kernel", b"pcl_gn_step_rooms_kernel"):
        assert kernel in blob, kernel
    doc = re.search(r"/\* pcl_pose_information and pcl_gn_refine for the nrooms \* nimages winners.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    for word in ("BUILD-DEFINED", "BIT FOR BIT", "r * nimages + i", "color_sets == nimages", "box is ignored", "per 64 images", "PCL_EINVAL", "2^31",
                 "Deliberately left out", "depth chains", "calibrated"):
        assert word in doc, word
    # the neighbours no longer list the rooms chains as left out
    for start in (r"/\* Pose information matrix and covariance", r"/\* Levenberg-Marquardt pose polish"):
        left_out = re.search(start + r".*?(Deliberately left out:.*?)\*/", open(HEADER).read(), flags=re.S).group(1)
        assert "images / rooms / depth" not in left_out and "rooms chains: pcl_" in left_out


SIZE_CASES = [(300, 1025, 6_000, 20_000), (50, 3000, 2_500_000), (1025,), (700,) * 32]


@pytest.mark.parametrize("sizes", SIZE_CASES)
@pytest.mark.parametrize("nimages", [1, 3, 66])
def test_the_workspace_is_the_rooms_single_workspaces(lib, sizes, nimages):
    """sum over the rooms of pcl_pose_information_workspace_bytes(n_r, nimages), each already a multiple of the carve's 256 bytes;
    2,500,000 points reach the chunk cap of 1024"""
    want = sum(lib.pcl_pose_information_workspace_bytes(n, nimages) for n in sizes)
    assert want > 0 and all(lib.pcl_pose_information_workspace_bytes(n, nimages) % 256 == 0 for n in sizes)
    assert lib.pcl_pose_information_rooms_workspace_bytes(_rooms(sizes), len(sizes), nimages) == want
    assert lib.pcl_gn_rooms_workspace_bytes(_rooms(sizes), len(sizes), nimages) == want
    if 2_500_000 in sizes:
        assert lib.pcl_pose_information_workspace_bytes(2_500_000, 1) == 1024 * 32 * 4


def test_the_sizing_functions_answer_zero_for_what_the_calls_refuse(lib):
    for size in (lib.pcl_pose_information_rooms_workspace_bytes, lib.pcl_gn_rooms_workspace_bytes):
        ok = (300, 1025)
        assert size(_rooms(ok), 2, 3) > 0
        assert size(None, 2, 3) == 0
        assert size(_rooms(ok), 0, 3) == 0 and size(_rooms(ok), -1, 3) == 0 and size(_rooms((700,) * 33), 33, 3) == 0
        assert size(_rooms(ok), 2, 0) == 0 and size(_rooms(ok), 2, -2) == 0
        assert size(_rooms(ok, hole=1), 2, 3) == 0
        assert size(_rooms((300, 0)), 2, 3) == 0 and size(_rooms((300, -5)), 2, 3) == 0 and size(_rooms((300, (1 << 27) + 1)), 2, 3) == 0
        # more blocks than a grid holds: 32 rooms of 1024 chunks x 70,000 images
        assert size(_rooms((2_500_000,) * 32), 32, 70_000) == 0 and size(_rooms((2_500_000,) * 32), 32, 65_000) > 0


@pytest.mark.parametrize("which", ["info", "gn"])
def test_refusals_before_any_device_call(lib, which):
    from piccolo_amd import _lib
    t, r, st, o, inf, cv, tr, ws = (0x10000 * (i + 1) for i in range(8))
    good = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)
    size = lib.pcl_pose_information_rooms_workspace_bytes if which == "info" else lib.pcl_gn_rooms_workspace_bytes

    def call(sizes=(300, 1025, 6_000), rooms="ok", R=None, csets=1, panos="ok", I=3, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, hyper=good, iters=5,
             state=st, out=o, info=inf, cov=cv, trace=tr, work=ws, nbytes=None, hole=None, room_hole=None, **hv):
        R = len(sizes) if R is None else R
        rs = _rooms(sizes, room_hole) if rooms == "ok" else rooms
        ps = _panos(max(I, 1), hole) if panos == "ok" else panos
        nbytes = size(_rooms(sizes), len(sizes), I) if nbytes is None else nbytes
        if which == "info":
            return lib.pcl_pose_information_rooms(rs, R, csets, ps, I, fmt, H, W, trans, rot, stride, info, cov, work, nbytes, None)
        h = None if hyper is None else ctypes.byref(_lib.GnHyper(**dict(hyper, **hv)))
        return lib.pcl_gn_refine_rooms(rs, R, csets, ps, I, fmt, H, W, trans, rot, stride, h, iters, state, out, info, cov, trace, work, nbytes, None)
    # null required pointers
    for name in ("rooms", "trans", "rot", "info", "work", "panos"):
        assert call(**{name: None}) == -1, name
    # the rooms: their count, a null cloud, n out of range
    assert call(R=0) == -1 and call(R=-1) == -1 and call(sizes=(700,) * 33, nbytes=1 << 40) == -1
    for hole in (0, 1, 2):
        assert call(room_hole=hole) == -1, hole
    assert call(sizes=(300, 0, 700), nbytes=1 << 40) == -1 and call(sizes=(300, -1), nbytes=1 << 40) == -1
    assert call(sizes=(300, (1 << 27) + 1), nbytes=1 << 40) == -1
    # a zero panorama address, anywhere in the list — also past the first launch's 64
    for hole in (0, 1, 2):
        assert call(hole=hole) == -1, hole
    assert call(I=70, hole=69) == -1 and call(I=70, hole=64) == -1
    assert call(I=0, nbytes=1 << 20) == -1 and call(I=-3, nbytes=1 << 20) == -1
    # color_sets: 0 / 1 or nimages
    for csets in (-1, 2, 4):
        assert call(csets=csets) == -1, csets
    # a room whose colour sets pass 2^31 bytes: 2^24 points are 64 MiB a plane, 3 + 30 planes — in any room
    big = 1 << 24
    assert lib.pcl_cloud_sets_bytes(big, 10) == 0 and lib.pcl_cloud_sets_bytes(big, 9) > 0
    assert call(sizes=(300, big), I=10, csets=10) == -1 and call(sizes=(big, 300), I=10, csets=10) == -1
    # more blocks than a grid holds
    assert call(sizes=(2_500_000,) * 32, I=70_000, panos=_panos(70_000), nbytes=1 << 60) == -1
    # whatever the images calls refuse
    assert call(H=0) == -1 and call(W=-1) == -1
    assert call(fmt=3) == -1 and call(fmt=4) == -1 and call(fmt=7) == -1 and call(fmt=-1) == -1
    assert call(stride=2) == -1 and call(stride=0) == -1 and call(stride=-16) == -1
    assert call(fmt=0, H=1 << 14, W=1 << 13) == -1
    full = size(_rooms((300, 1025, 6_000)), 3, 3)
    assert call(nbytes=full - 1) == -1 and call(nbytes=0) == -1 and call(I=4, nbytes=full) == -1
    assert call(sizes=(300, 1025, 6_000, 700), nbytes=full) == -1
    if which == "gn":
        assert call(iters=-1) == -1 and call(iters=1001) == -1
        for name in ("hyper", "state", "out"):
            assert call(**{name: None}) == -1, name
        for key in good:
            for v in (float("nan"), float("inf")):
                assert call(**{key: v}) == -1, (key, v)
        assert call(lam0=0.0) == -1 and call(lam_up=1.0) == -1 and call(lam_down=1.5) == -1 and call(lam_min=2.0, lam_max=1.0) == -1
        assert call(step_cap=0.0) == -1 and call(tol=-1e-9) == -1


def test_the_rooms_kernels_are_outside_the_loss_kernel_hash(lib):
    from piccolo_amd import build
    assert lib.pcl_source_hash().decode() == build.loss_kernel_source_hash()
    for name in ("pcl_gn_rooms.hip", "pcl_gn_device.h", "pcl_gn.hip", "pcl_info.hip", "pcl_info_device.h", "pcl_point_pass.h"):
        text = open(os.path.join(build.CSRC, name)).read()
        assert "atomic" not in re.sub(r"//.*", "", text), name
    assert os.path.join(build.CSRC, "pcl_gn_rooms.hip") in build.sources()


def test_the_ops_layer_refuses_before_a_device_call():
    """a weighted room, rooms whose colour sets differ, a pose count that is not rooms x panoramas, too many rooms: ValueError from host
    checks alone (stand-in objects; nothing is packed)"""
    import torch
    from types import SimpleNamespace
    from piccolo_amd import _lib, ops

    def pano(H=32, W=64, fmt=_lib.PANO_F16):
        return SimpleNamespace(H=H, W=W, fmt=fmt, texels=(H, W, fmt), data=torch.zeros(1))

    def cloud(sets=1, weights=None):
        return SimpleNamespace(n=1025, color_sets=sets, weights=weights, data=torch.zeros(1))
    with pytest.raises(ValueError, match="0 rooms"):
        ops._rooms_call("f", [], [pano()], 0)
    with pytest.raises(ValueError, match="33 rooms"):
        ops._rooms_call("f", [cloud()] * 33, [pano()], 33)
    with pytest.raises(ValueError, match="no panorama"):
        ops._rooms_call("f", [cloud()], [], 0)
    with pytest.raises(ValueError, match="weighted room cloud"):
        ops._rooms_call("f", [cloud(), cloud(weights=torch.zeros(1))], [pano()], 2)
    with pytest.raises(ValueError, match="one colour set, or one per image"):
        ops._rooms_call("f", [cloud(1), cloud(2)], [pano(), pano()], 4)
    with pytest.raises(ValueError, match="3 colour sets for 2 images"):
        ops._rooms_call("f", [cloud(3), cloud(3)], [pano(), pano()], 4)
    with pytest.raises(ValueError, match="share size and texel format"):
        ops._rooms_call("f", [cloud()], [pano(), pano(fmt=_lib.PANO_U8)], 2)
    with pytest.raises(ValueError, match="one pose per"):
        ops._rooms_call("f", [cloud(), cloud()], [pano(), pano()], 3)
    clouds, panos, rooms, arr, sets = ops._rooms_call("f", [cloud(2), cloud(2)], [pano(), pano()], 4)
    assert len(rooms) == 2 and len(arr) == 2 and sets == 2 and rooms[1].n == 1025 and rooms[1].box is None
    for name in ("pose_information_rooms", "pose_information_rooms_at_winners", "gauss_newton_refine_rooms", "gauss_newton_refine_rooms_at_winners"):
        assert callable(getattr(ops, name)), name
