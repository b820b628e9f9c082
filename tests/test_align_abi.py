"""CPU checks of the alignment entry points' boundary: the five symbols are declared, bound and exported under ABI 12, the record and
parameter structs have the header's layout, every documented PCL_EINVAL is answered before any device call (bogus non-null pointers, no
device here), and the Python surface refuses on the host."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

SYMBOLS = ("pcl_voxel_moments", "pcl_voxel_normals", "pcl_align_workspace_bytes", "pcl_align_vote", "pcl_align_transform_cloud")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = open(os.path.join(REPO, "include", "piccolo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcl_[a-z0-9_]+)\s*\(", header))
    exported = set(re.findall(r"\bT (pcl_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)))
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert _lib.ABI_VERSION == 12 and lib.pcl_abi_version() == 12 and "#define PCL_ABI_VERSION 12" in text
    # every declared symbol is bound and the other way round: the new ones did not unbalance the table
    assert declared == set(_lib.SIGNATURES)
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_voxel_moments_kernel", b"pcl_voxel_normals_kernel", b"pcl_align_hist_kernel", b"pcl_align_cone_kernel",
                   b"pcl_align_wall_mean_kernel", b"pcl_align_finish_kernel", b"pcl_align_transform_kernel"):
        assert kernel in blob, kernel
    # argument counts of the bindings are the prototypes'
    for name in SYMBOLS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        count = 0 if args.strip() == "void" else len(args.split(","))
        assert count == len(_lib.SIGNATURES[name][1]), name


def test_structs_have_the_headers_layout(lib):
    from piccolo_amd import _lib
    assert ctypes.sizeof(_lib.AlignParams) == 16 and _lib.AlignParams.yaw.offset == 8
    assert _lib.ALIGN_OUT_WORDS * 8 == (3 + 9 + 4) * 8 + 5 * 8
    header = open(os.path.join(REPO, "include", "piccolo_hip.h")).read()
    body = re.search(r"typedef struct pcl_align_out \{(.*?)\} PclAlignOut;", header, flags=re.S).group(1)
    fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", " ", body, flags=re.S).split(";")]
    assert fields[:5] == ["double up[3]", "double rot[9]", "double cos_tilt, sin_tilt, cos_yaw, sin_yaw", "int64_t weight[4]", "int64_t status"]
    assert lib.pcl_align_workspace_bytes(1) >= (64 * 64 + 360 + 4 * 3 + 4) * 8 and lib.pcl_align_workspace_bytes(1) % 256 == 0
    assert lib.pcl_align_workspace_bytes(1 << 27) == lib.pcl_align_workspace_bytes(1)
    assert [lib.pcl_align_workspace_bytes(v) for v in (0, -1, (1 << 27) + 1)] == [0, 0, 0]


def test_every_refusal_comes_before_a_device_call(lib):
    """bogus non-null pointers: a call that went on to the device would fault, and there is no device here"""
    from piccolo_amd import _lib
    P = ctypes.c_void_p(0x1000)
    n = 100
    good = [P, n, 0.1, P, P, 10, P, P, None]
    for k in (0, 3, 4, 6, 7):                                              # every pointer in turn
        args = list(good)
        args[k] = None
        assert lib.pcl_voxel_moments(*args) == -1, k
    for bad_n, nvox in ((0, 10), (-1, 10), ((1 << 27) + 1, 10), (n, 0), (n, -1), (n, n + 1)):
        assert lib.pcl_voxel_moments(P, bad_n, 0.1, P, P, nvox, P, P, None) == -1, (bad_n, nvox)
    for voxel in (0.0, -0.1, 2.0000001, 3.0, float("nan"), float("inf")):  # the range rule: at most 2 m
        assert lib.pcl_voxel_moments(P, n, voxel, P, P, 10, P, P, None) == -1, voxel

    good = [P, P, 10, 8, P, P, None, None]                                 # (eig may be null)
    for k in (0, 1, 4, 5):
        args = list(good)
        args[k] = None
        assert lib.pcl_voxel_normals(*args) == -1, k
    for nvox, min_count in ((0, 8), (-1, 8), ((1 << 27) + 1, 8), (10, 2), (10, 0), (10, -5)):
        assert lib.pcl_voxel_normals(P, P, nvox, min_count, P, P, P, None) == -1, (nvox, min_count)

    params, big = _lib.AlignParams(40.0, 1, 0), 1 << 20
    good = [P, P, P, 10, ctypes.byref(params), P, P, big, None]
    for k in (0, 1, 2, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert lib.pcl_align_vote(*args) == -1, k
    for nvox in (0, -1, (1 << 27) + 1):
        assert lib.pcl_align_vote(P, P, P, nvox, ctypes.byref(params), P, P, big, None) == -1, nvox
    for tilt in (0.0, -1.0, 45.0001, 90.0, float("nan"), float("inf")):
        bad = _lib.AlignParams(tilt, 0, 0)
        assert lib.pcl_align_vote(P, P, P, 10, ctypes.byref(bad), P, P, big, None) == -1, tilt
    assert lib.pcl_align_vote(P, P, P, 10, ctypes.byref(params), P, P, lib.pcl_align_workspace_bytes(10) - 1, None) == -2     # PCL_EWORKSPACE

    good = [P, n, P, P, P, None]
    for k in (0, 2, 3, 4):
        args = list(good)
        args[k] = None
        assert lib.pcl_align_transform_cloud(*args) == -1, k
    for bad_n in (0, -1, (1 << 27) + 1):
        assert lib.pcl_align_transform_cloud(P, bad_n, P, P, P, None) == -1, bad_n


def test_python_surface_refuses_on_the_host():
    """ValueError before a device is asked for, the text naming the argument"""
    import numpy as np
    import torch
    from piccolo_amd import data_utils, ops, utils
    xyz = torch.zeros(4, 3)
    for min_count in (2, 0, -1, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="min_count"):
            utils.voxel_normals(xyz, 0.1, min_count)
        with pytest.raises(ValueError, match="min_count"):
            utils.align_cloud(xyz, min_count=min_count)
        with pytest.raises(ValueError, match="min_count"):
            ops.voxel_normals_of(None, None, min_count)
    for voxel in (0, -1.0, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="positive finite"):
            utils.align_cloud(xyz, voxel=voxel)
    with pytest.raises(ValueError, match="voxel 2.5: at most 2"):
        utils.align_cloud(xyz, voxel=2.5)
    for tilt in (0, -5.0, 45.5, 90, float("nan"), None, True, "40"):
        with pytest.raises(ValueError, match="max_tilt"):
            utils.align_cloud(xyz, max_tilt=tilt)
        with pytest.raises(ValueError, match="max_tilt"):
            ops.align_vote(xyz, xyz[:, 0], xyz[:, 0], max_tilt=tilt)
    for yaw in (1, 0, None, "True"):
        with pytest.raises(ValueError, match="yaw"):
            utils.align_cloud(xyz, yaw=yaw)
        with pytest.raises(ValueError, match="yaw"):
            ops.align_vote(xyz, xyz[:, 0], xyz[:, 0], yaw=yaw)
    with pytest.raises(ValueError, match=r"normal must be \(V, 3\)"):
        ops.align_vote(torch.zeros(4, 2), xyz[:, 0], xyz[:, 0])
    with pytest.raises(ValueError, match=r"xyz must be \(N, 3\)"):
        ops.align_transform_cloud(torch.zeros(0, 3), torch.eye(3), torch.zeros(3))
    with pytest.raises(ValueError, match="min_count"):
        data_utils.obtain_align_matrix(np.zeros((4, 3)), min_count=1)
    # the drop-in module hands the reference the name it calls
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_data_utils", os.path.join(REPO, "dropin", "data_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.obtain_align_matrix is data_utils.obtain_align_matrix
