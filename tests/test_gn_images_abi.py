"""CPU checks of the several-image boundary of the pose information and the Levenberg-Marquardt polish (additive to ABI 12):
pcl_pose_information_images and pcl_gn_refine_images are declared, bound and exported, their kernels are in the code object, every listed
refusal answers PCL_EINVAL before anything touches a device, and the loss kernel's source hash is what it was."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_pose_information_images", "pcl_gn_refine_images")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+float\s*\*\s*cloud\s*,\s*const\s+float\s*\*\s*weights\s*,\s*int\s+weight_sets\s*,\s*int64_t\s+n\s*,"
                         r"\s*int\s+color_sets\s*,\s*const\s+uint64_t\s*\*\s*panos_host\s*,\s*int\s+nimages\s*," % name, text), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert len(_lib.SIGNATURES["pcl_pose_information_images"][1]) == 18 and len(_lib.SIGNATURES["pcl_gn_refine_images"][1]) == 23
    # the single-image bindings with weight_sets, color_sets, the address array and nimages in place of the panorama and B
    one, many = _lib.SIGNATURES["pcl_gn_refine"][1], _lib.SIGNATURES["pcl_gn_refine_images"][1]
    assert many[:7] == one[:2] + [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    assert many[7:13] == one[4:10] and many[13:] == one[11:]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_pose_info_images_kernel", b"pcl_gn_pass_images_kernel", b"pcl_pose_info_kernel", b"pcl_gn_pass_kernel",
                   b"pcl_point_residuals_images_kernel"):
        assert kernel in blob, kernel
    doc = re.search(r"/\* pcl_pose_information and pcl_gn_refine for the nimages winners.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    for word in ("BUILD-DEFINED", "bit for bit", "weight_sets == nimages", "color_sets ==", "groups of 64", "PCL_EINVAL", "2^31", "S1 / M",
                 "Deliberately left out", "rooms and depth chains", "calibrated"):
        assert word in doc, word


def test_the_new_kernels_are_outside_the_loss_kernel_hash(lib):
    from piccolo_amd import build
    assert lib.pcl_source_hash().decode() == build.loss_kernel_source_hash()
    for name in ("pcl_gn.hip", "pcl_info.hip", "pcl_info_device.h", "pcl_point_pass.h"):
        text = open(os.path.join(build.CSRC, name)).read()
        assert "atomic" not in re.sub(r"//.*", "", text), name
    # one definition of the address list, shared by the residual rows and the two new instances
    hits = [name for name in os.listdir(build.CSRC) if "struct PclResPanos" in open(os.path.join(build.CSRC, name)).read()]
    assert hits == ["pcl_point_pass.h"]


def _fake():
    return (0x10000 * (i + 1) for i in range(11))                      # never dereferenced on the host


def _panos(I, hole=None):
    return (ctypes.c_uint64 * I)(*[0 if i == hole else 0x900000 + 0x1000 * i for i in range(I)])


@pytest.mark.parametrize("which", ["info", "gn"])
def test_refusals_before_any_device_call(lib, which):
    from piccolo_amd import _lib
    c, wt, t, r, st, o, inf, cv, tr, ws, _ = _fake()
    good = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)
    size = lib.pcl_pose_information_workspace_bytes if which == "info" else lib.pcl_gn_workspace_bytes

    def call(cloud=c, w=None, wsets=0, n=1025, csets=1, panos="ok", I=3, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, hyper=good, iters=5, state=st,
             out=o, info=inf, cov=cv, trace=tr, work=ws, nbytes=None, hole=None, **hv):
        ps = _panos(max(I, 1), hole) if panos == "ok" else panos
        nbytes = size(n, I) if nbytes is None else nbytes
        if which == "info":
            return lib.pcl_pose_information_images(cloud, w, wsets, n, csets, ps, I, fmt, H, W, trans, rot, stride, info, cov, work, nbytes, None)
        h = None if hyper is None else ctypes.byref(_lib.GnHyper(**dict(hyper, **hv)))
        return lib.pcl_gn_refine_images(cloud, w, wsets, n, csets, ps, I, fmt, H, W, trans, rot, stride, h, iters, state, out, info, cov, trace, work,
                                        nbytes, None)
    # null required pointers
    for name in ("cloud", "trans", "rot", "info", "work", "panos"):
        assert call(**{name: None}) == -1, name
        assert call(w=wt, wsets=1, **{name: None}) == -1, name
    # a zero panorama address, anywhere in the list — also past the first launch's 64
    for hole in (0, 1, 2):
        assert call(hole=hole) == -1, hole
    assert call(I=70, hole=69) == -1 and call(I=70, hole=64) == -1
    assert call(I=0) == -1 and call(I=-3) == -1
    # weight_sets: 0 without weights, 1 or nimages with them
    assert call(w=None, wsets=1) == -1 and call(w=None, wsets=3) == -1
    for wsets in (0, 2, 4, -1):
        assert call(w=wt, wsets=wsets) == -1, wsets
    # color_sets: 0 / 1 or nimages
    for csets in (-1, 2, 4):
        assert call(csets=csets) == -1, csets
    # a weight or colour resource of 2^31 bytes or more: 2^24 points are 64 MiB a plane
    big = 1 << 24
    assert lib.pcl_cloud_stride(big) * 4 * 32 == 1 << 31
    assert call(n=big, I=32, w=wt, wsets=32, nbytes=1 << 40) == -1
    assert call(n=big, I=10, csets=10, nbytes=1 << 40) == -1            # 3 + 30 planes
    assert lib.pcl_cloud_sets_bytes(big, 10) == 0 and lib.pcl_cloud_sets_bytes(big, 9) > 0
    # whatever the single-image calls refuse
    assert call(n=0) == -1 and call(n=-1) == -1 and call(n=(1 << 27) + 1, nbytes=1 << 40) == -1
    assert call(H=0) == -1 and call(W=-1) == -1
    assert call(fmt=3) == -1 and call(fmt=4) == -1 and call(fmt=7) == -1 and call(fmt=-1) == -1
    assert call(stride=2) == -1 and call(stride=0) == -1 and call(stride=-16) == -1
    assert call(fmt=0, H=1 << 14, W=1 << 13) == -1
    assert call(nbytes=size(1025, 3) - 1) == -1 and call(nbytes=0) == -1 and call(I=4, nbytes=size(1025, 3)) == -1
    if which == "gn":
        assert call(iters=-1) == -1 and call(iters=1001) == -1
        for name in ("hyper", "state", "out"):
            assert call(**{name: None}) == -1, name
        for key in good:
            for v in (float("nan"), float("inf")):
                assert call(**{key: v}) == -1, (key, v)
        assert call(lam0=0.0) == -1 and call(lam_up=1.0) == -1 and call(lam_down=1.5) == -1 and call(lam_min=2.0, lam_max=1.0) == -1
        assert call(step_cap=0.0) == -1 and call(tol=-1e-9) == -1


def test_the_ops_layer_refuses_before_a_device_call():
    """planes of another shape, a pose count that is not the panorama count, panoramas of different texels, colour sets that are not one per
    image: ValueError from host checks alone (stand-in objects; nothing is packed)"""
    import torch
    from types import SimpleNamespace
    from piccolo_amd import _lib, ops
    stride = _lib.load().pcl_cloud_stride(1025)

    def pano(H=32, W=64, fmt=_lib.PANO_F16):
        return SimpleNamespace(H=H, W=W, fmt=fmt, texels=(H, W, fmt), data=torch.zeros(1))
    cloud = SimpleNamespace(n=1025, color_sets=1, weights=None, data=torch.zeros(1))
    with pytest.raises(ValueError, match="no panorama"):
        ops._images_call("f", cloud, [], 0, None)
    with pytest.raises(ValueError, match="one pose per panorama"):
        ops._images_call("f", cloud, [pano(), pano()], 3, None)
    with pytest.raises(ValueError, match="share size and texel format"):
        ops._images_call("f", cloud, [pano(), pano(fmt=_lib.PANO_U8)], 2, None)
    with pytest.raises(ValueError, match="u8p"):
        ops._images_call("f", cloud, [pano(fmt=_lib.PANO_U8P)] * 2, 2, None)
    with pytest.raises(ValueError, match="3 colour sets for 2 images"):
        ops._images_call("f", SimpleNamespace(n=1025, color_sets=3, weights=None), [pano(), pano()], 2, None)
    for planes in (torch.zeros(2, stride), torch.zeros(3, stride - 1), [1.0]):          # (not on the GPU; another shape; no tensor)
        with pytest.raises(ValueError, match="planes"):
            ops._images_call("f", cloud, [pano(), pano(), pano()], 3, planes)
    panos, arr, weights, sets = ops._images_call("f", cloud, [pano(), pano()], 2, None)
    assert len(arr) == 2 and weights is None and sets == 0
    for name in ("pose_information_images", "pose_information_images_at_winners", "gauss_newton_refine_images",
                 "gauss_newton_refine_images_at_winners"):
        assert callable(getattr(ops, name)), name
