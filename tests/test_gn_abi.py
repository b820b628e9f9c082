"""CPU checks of the Levenberg-Marquardt boundary (additive to ABI 12): pcl_gn_refine and its two size queries are declared, bound and
exported, the kernels are in the code object, the size queries are monotone and 0 for a bad n or B, every listed refusal answers
PCL_EINVAL before anything touches a device, and the loss kernel's source hash is what it was."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_gn_state_bytes", "pcl_gn_workspace_bytes", "pcl_gn_refine")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+pcl_gn_state_bytes\s*\(\s*int\s+B\s*\)", text)
    assert re.search(r"\bsize_t\s+pcl_gn_workspace_bytes\s*\(\s*int64_t\s+n\s*,\s*int\s+B\s*\)", text)
    assert re.search(r"\bint\s+pcl_gn_refine\s*\(", text)
    fields = re.search(r"typedef\s+struct\s+pcl_gn_hyper\s*\{(.*?)\}\s*pcl_gn_hyper\s*;", text, flags=re.S).group(1)
    names = re.findall(r"\b(lam0|lam_up|lam_down|lam_min|lam_max|step_cap|tol)\b", fields)
    assert names == [f[0] for f in _lib.GnHyper._fields_] and all(f[1] is ctypes.c_float for f in _lib.GnHyper._fields_)
    assert re.search(r"\bfloat\b", fields) and ctypes.sizeof(_lib.GnHyper) == 28
    assert _lib.SIGNATURES["pcl_gn_state_bytes"] == (ctypes.c_size_t, [ctypes.c_int])
    assert _lib.SIGNATURES["pcl_gn_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    assert _lib.SIGNATURES["pcl_gn_refine"][0] is ctypes.c_int and len(_lib.SIGNATURES["pcl_gn_refine"][1]) == 21
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_gn_init_kernel", b"pcl_gn_pass_kernel", b"pcl_gn_step_kernel", b"pcl_pose_info_kernel", b"pcl_pose_info_finish_kernel"):
        assert kernel in blob, kernel
    # the header says that the chain is the build's own, what it minimises and that this is not the sampling loss, the units, the status
    # codes and what is left out; the pose-information block keeps its own words
    doc = re.search(r"/\* Levenberg-Marquardt pose polish.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    for word in ("BUILD-DEFINED", "MEAN SQUARED residual", "NOT the sampling loss", "metres", "radians", "status: 0", "converged",
                 "Deliberately left out", "IRLS", "box clamp", "colour sets", "real data", "PCL_EINVAL"):
        assert word in doc, word
    older = re.search(r"/\* Pose information matrix and covariance.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    assert "Gauss-Newton step" in older and "Levenberg" not in older


def test_the_new_kernels_are_outside_the_loss_kernel_hash(lib):
    """pcl_gn.hip and pcl_info_device.h include the loss kernel's device functions and are not among the four files the loss-kernel hash
    covers; neither holds an atomic"""
    import hashlib
    from piccolo_amd import build
    assert lib.pcl_source_hash().decode() == build.loss_kernel_source_hash()
    h = hashlib.sha256()
    for name in ("pcl_loss.hip", "pcl_sample_device.h", "pcl_gd_device.h", "pcl_device.h"):
        h.update(open(os.path.join(build.CSRC, name), "rb").read())
    assert h.hexdigest()[:16] == build.loss_kernel_source_hash()
    assert os.path.join(build.CSRC, "pcl_gn.hip") in build.sources()
    for name in ("pcl_gn.hip", "pcl_info_device.h"):
        text = open(os.path.join(build.CSRC, name)).read()
        assert "atomic" not in re.sub(r"//.*", "", text), name
    assert '#include "pcl_info_device.h"' in open(os.path.join(build.CSRC, "pcl_gn.hip")).read()
    assert '#include "pcl_info_device.h"' in open(os.path.join(build.CSRC, "pcl_info.hip")).read()


def test_size_queries_are_monotone_and_zero_for_a_bad_n_or_B(lib):
    state, work = lib.pcl_gn_state_bytes, lib.pcl_gn_workspace_bytes
    assert state(0) == 0 and state(-1) == 0
    sizes = [state(B) for B in (1, 2, 3, 32, 33, 1000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert state(1000) >= 1000 * (45 * 8 + 12 * 4)            # the accepted sums in double and two poses, at the least
    assert work(0, 1) == 0 and work(-5, 1) == 0 and work((1 << 27) + 1, 1) == 0
    assert work(1025, 0) == 0 and work(1025, -3) == 0
    assert work(1 << 27, 1 << 22) == 0                        # more blocks than a grid holds
    ns = (1, 2, 511, 512, 513, 1025, 2049, 50001, 166667, 1 << 20, 1 << 27)
    for B in (1, 2, 32, 33):
        sizes = [work(n, B) for n in ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert sizes == [lib.pcl_pose_information_workspace_bytes(n, B) for n in ns]      # the same partial rows
    for n in ns:
        sizes = [work(n, B) for B in (1, 2, 3, 32, 33, 1000)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))


def test_refusals_before_any_device_call(lib):
    from piccolo_amd import _lib
    c, wt, p, t, r, st, o, inf, cv, tr, ws = (0x10000 * (i + 1) for i in range(11))           # never dereferenced on the host
    need = lib.pcl_gn_workspace_bytes(1025, 3)
    good = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)

    def gn(cloud=c, w=None, n=1025, pano=p, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, B=3, hyper=good, iters=5, state=st, out=o, info=inf,
           cov=cv, trace=tr, work=ws, nbytes=need, **hv):
        h = None if hyper is None else ctypes.byref(_lib.GnHyper(**dict(hyper, **hv)))
        return lib.pcl_gn_refine(cloud, w, n, pano, fmt, H, W, trans, rot, stride, B, h, iters, state, out, info, cov, trace, work, nbytes, None)
    # everything pcl_pose_information refuses
    for name in ("cloud", "pano", "trans", "rot", "info", "work"):
        assert gn(**{name: None}) == -1, name
        assert gn(w=wt, **{name: None}) == -1, name
    assert gn(n=0) == -1 and gn(n=-1) == -1 and gn(n=(1 << 27) + 1, nbytes=1 << 40) == -1
    assert gn(B=0) == -1 and gn(B=-2) == -1
    assert gn(n=1 << 27, B=1 << 22, nbytes=1 << 60) == -1
    assert gn(H=0) == -1 and gn(W=-1) == -1
    assert gn(fmt=3) == -1 and gn(fmt=4) == -1 and gn(fmt=7) == -1 and gn(fmt=-1) == -1
    assert gn(stride=2) == -1 and gn(stride=0) == -1 and gn(stride=-16) == -1
    assert gn(fmt=0, H=1 << 14, W=1 << 13) == -1
    assert gn(nbytes=need - 1) == -1 and gn(nbytes=0) == -1 and gn(B=4) == -1
    # its own
    assert gn(iters=-1) == -1 and gn(iters=1001) == -1
    for name in ("hyper", "state", "out"):
        assert gn(**{name: None}) == -1, name
    for key in good:
        for v in (float("nan"), float("inf"), -float("inf")):
            assert gn(**{key: v}) == -1, (key, v)
    assert gn(lam0=0.0) == -1 and gn(lam0=-1e-3) == -1
    assert gn(lam_up=1.0) == -1 and gn(lam_up=0.5) == -1
    assert gn(lam_down=0.0) == -1 and gn(lam_down=-0.1) == -1 and gn(lam_down=1.5) == -1
    assert gn(lam_min=2.0, lam_max=1.0) == -1
    assert gn(step_cap=0.0) == -1 and gn(step_cap=-0.1) == -1
    assert gn(tol=-1e-9) == -1
