"""CPU checks of the pose-information boundary (additive to ABI 12): pcl_pose_information and its workspace query are declared, bound and
exported, the kernels are in the code object, the workspace size is monotone and 0 for a bad n or B, every listed refusal answers
PCL_EINVAL before anything touches a device, and the loss kernel's source hash is what it was."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_pose_information_workspace_bytes", "pcl_pose_information")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+pcl_pose_information_workspace_bytes\s*\(\s*int64_t\s+n\s*,\s*int\s+B\s*\)", text)
    assert re.search(r"\bint\s+pcl_pose_information\s*\(", text)
    assert _lib.SIGNATURES["pcl_pose_information_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert _lib.SIGNATURES["pcl_pose_information"][0] is ctypes.c_int and len(_lib.SIGNATURES["pcl_pose_information"][1]) == 16
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    assert b"pcl_pose_info_kernel" in blob and b"pcl_pose_info_finish_kernel" in blob
    # the header says that the quantity is the build's own, gives the units and lists what is left out
    doc = re.search(r"/\* Pose information matrix and covariance.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    for word in ("BUILD-DEFINED", "metres", "radians", "status", "Deliberately left out", "colour sets", "Gauss-Newton step", "calibrated"):
        assert word in doc, word


def test_the_new_kernel_is_outside_the_loss_kernel_hash(lib):
    """pcl_info.hip includes the loss kernel's device functions and is not one of the four files the loss-kernel hash covers: the library
    carries the hash of those four files alone, while the library hash (every source) knows the new file"""
    import hashlib
    from piccolo_amd import build
    assert lib.pcl_source_hash().decode() == build.loss_kernel_source_hash()
    h = hashlib.sha256()
    for name in ("pcl_loss.hip", "pcl_sample_device.h", "pcl_gd_device.h", "pcl_device.h"):
        h.update(open(os.path.join(build.CSRC, name), "rb").read())
    assert h.hexdigest()[:16] == build.loss_kernel_source_hash()
    assert os.path.join(build.CSRC, "pcl_info.hip") in build.sources()
    text = open(os.path.join(build.CSRC, "pcl_info.hip")).read()
    assert '#include "pcl_sample_device.h"' in text and "atomicAdd" not in text


def test_workspace_size_is_monotone_and_zero_for_a_bad_n_or_B(lib):
    size = lib.pcl_pose_information_workspace_bytes
    assert size(0, 1) == 0 and size(-5, 1) == 0 and size((1 << 27) + 1, 1) == 0
    assert size(1025, 0) == 0 and size(1025, -3) == 0
    assert size(1 << 27, 1 << 22) == 0                        # more blocks than a grid holds
    ns = (1, 2, 511, 512, 513, 1025, 2049, 50001, 166667, 1 << 20, 1 << 27)
    for B in (1, 2, 32, 33):
        sizes = [size(n, B) for n in ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    for n in ns:
        sizes = [size(n, B) for B in (1, 2, 3, 32, 33, 1000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert size(1025, 1) >= 2 * 32 * 4                        # three steps: two chunks of one 32-float row each


def test_refusals_before_any_device_call(lib):
    c, wt, p, t, r, o, cv, ws = 0x10000, 0x18000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000          # never dereferenced on the host
    need = lib.pcl_pose_information_workspace_bytes(1025, 3)

    def info(cloud=c, w=None, n=1025, pano=p, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, B=3, out=o, cov=cv, work=ws, nbytes=need):
        return lib.pcl_pose_information(cloud, w, n, pano, fmt, H, W, trans, rot, stride, B, out, cov, work, nbytes, None)
    for name in ("cloud", "pano", "trans", "rot", "out", "work"):
        assert info(**{name: None}) == -1, name
        assert info(w=wt, **{name: None}) == -1, name
    assert info(n=0) == -1 and info(n=-1) == -1 and info(n=(1 << 27) + 1, nbytes=1 << 40) == -1
    assert info(B=0) == -1 and info(B=-2) == -1
    assert info(n=1 << 27, B=1 << 22, nbytes=1 << 60) == -1  # more blocks than a grid holds
    assert info(H=0) == -1 and info(W=-1) == -1
    assert info(fmt=3) == -1 and info(fmt=4) == -1           # the trim launch's texel layouts U8P / U8V
    assert info(fmt=7) == -1 and info(fmt=-1) == -1
    assert info(stride=2) == -1 and info(stride=0) == -1 and info(stride=-16) == -1
    assert info(fmt=0, H=1 << 14, W=1 << 13) == -1           # a packed float4 panorama of 2 GiB
    assert info(nbytes=need - 1) == -1 and info(nbytes=0) == -1
    assert info(B=4) == -1                                    # the workspace of three poses is short for four
