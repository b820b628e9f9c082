"""CPU checks of the per-point residual and robust-weight boundary (additive to ABI 12): pcl_point_residuals, pcl_robust_weights and its
workspace query are declared, bound and exported, the workspace size is monotone and 0 for a bad n, and every listed refusal answers
PCL_EINVAL before anything touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_point_residuals", "pcl_robust_weights_workspace_bytes", "pcl_robust_weights")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+pcl_point_residuals\s*\(", text)
    assert re.search(r"\bsize_t\s+pcl_robust_weights_workspace_bytes\s*\(\s*int64_t\s+n\s*\)", text)
    assert re.search(r"\bint\s+pcl_robust_weights\s*\(", text)
    assert re.search(r"#define\s+PCL_ROBUST_TRUNC\s+0\b", text) and re.search(r"#define\s+PCL_ROBUST_HUBER\s+1\b", text)
    assert (_lib.ROBUST_TRUNC, _lib.ROBUST_HUBER) == (0, 1)
    assert _lib.SIGNATURES["pcl_point_residuals"][0] is ctypes.c_int and len(_lib.SIGNATURES["pcl_point_residuals"][1]) == 13
    assert _lib.SIGNATURES["pcl_robust_weights"][0] is ctypes.c_int and len(_lib.SIGNATURES["pcl_robust_weights"][1]) == 9
    assert _lib.SIGNATURES["pcl_robust_weights_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64])
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    assert all(k in blob for k in (b"pcl_point_residuals_kernel", b"pcl_rw_init_kernel", b"pcl_rw_hist_kernel", b"pcl_rw_plane_kernel"))
    # the header no longer lists change detection among what is left out, and says where weights can now come from
    left_out = re.search(r"Deliberately left out: weights in the initialisation stage.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    assert "change detection" not in left_out and "pcl_robust_weights" in left_out


def test_workspace_size_is_monotone_and_zero_for_a_bad_n(lib):
    size = lib.pcl_robust_weights_workspace_bytes
    assert size(0) == 0 and size(-5) == 0 and size((1 << 27) + 1) == 0
    sizes = [size(n) for n in (1, 2, 255, 256, 257, 1025, 50001, 166667, 1 << 20, 1 << 27)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))


def test_point_residuals_refusals_before_any_device_call(lib):
    c, p, t, r, o = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000          # never dereferenced on the host

    def res(cloud=c, n=1025, pano=p, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, B=3, out=o):
        return lib.pcl_point_residuals(cloud, n, pano, fmt, H, W, trans, rot, stride, B, None, out, None)
    for name in ("cloud", "pano", "trans", "rot", "out"):
        assert res(**{name: None}) == -1, name
    assert res(n=0) == -1 and res(n=-1) == -1 and res(n=(1 << 27) + 1) == -1
    assert res(B=0) == -1 and res(B=-2) == -1
    assert res(n=1 << 27, B=1 << 22) == -1                   # more blocks than a grid holds
    assert res(H=0) == -1 and res(W=-1) == -1
    assert res(fmt=3) == -1 and res(fmt=4) == -1             # the trim launch's texel layouts U8P / U8V
    assert res(fmt=7) == -1 and res(fmt=-1) == -1
    assert res(stride=2) == -1 and res(stride=0) == -1 and res(stride=-16) == -1
    assert res(fmt=0, H=1 << 14, W=1 << 13) == -1           # a packed float4 panorama of 2 GiB


def test_robust_weights_refusals_before_any_device_call(lib):
    row, plane, ws = 0x10000, 0x20000, 0x30000
    need = lib.pcl_robust_weights_workspace_bytes(1025)

    def rw(res=row, n=1025, kind=0, k=2.5, pl=plane, w=ws, nbytes=need):
        return lib.pcl_robust_weights(res, n, kind, k, pl, None, w, nbytes, None)
    assert rw(res=None) == -1 and rw(pl=None) == -1 and rw(w=None) == -1
    assert rw(n=0) == -1 and rw(n=-3) == -1 and rw(n=(1 << 27) + 1) == -1
    assert rw(kind=2) == -1 and rw(kind=-1) == -1
    assert rw(k=0.0) == -1 and rw(k=-1.0) == -1 and rw(k=float("inf")) == -1 and rw(k=float("nan")) == -1
    assert rw(nbytes=need - 1) == -1 and rw(nbytes=0) == -1
