"""CPU checks of the depth forms of the residuals, the pose information and the LM polish (additive to ABI 12; csrc/pcl_depth_info.hip): the
six symbols are declared, bound and exported, every null argument and every bad size is refused before a device is touched, the size
queries are positive multiples of 256, monotone in n, B and the grid and 0 for bad arguments, the per-point kernels' sources hold no
atomicAdd, and the loss-kernel hash still covers its four files alone."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_point_residuals_depth_workspace_bytes", "pcl_point_residuals_depth", "pcl_pose_information_depth_workspace_bytes",
       "pcl_pose_information_depth", "pcl_gn_depth_workspace_bytes", "pcl_gn_refine_depth")
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bsize_t\s+pcl_point_residuals_depth_workspace_bytes\s*\(\s*int\s+B\s*,\s*int\s+depth_h\s*,\s*int\s+depth_w\s*\)", text)
    for name in ("pcl_pose_information_depth_workspace_bytes", "pcl_gn_depth_workspace_bytes"):
        assert re.search(r"\bsize_t\s+%s\s*\(\s*int64_t\s+n\s*,\s*int\s+B\s*,\s*int\s+depth_h\s*,\s*int\s+depth_w\s*\)" % name, text), name
    for name in ("pcl_point_residuals_depth", "pcl_pose_information_depth", "pcl_gn_refine_depth"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert _lib.SIGNATURES["pcl_point_residuals_depth_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    for name in ("pcl_pose_information_depth_workspace_bytes", "pcl_gn_depth_workspace_bytes"):
        assert _lib.SIGNATURES[name] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int])
    for name, nargs in (("pcl_point_residuals_depth", 20), ("pcl_pose_information_depth", 21), ("pcl_gn_refine_depth", 26)):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and len(_lib.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, name                            # the binding has the declaration's parameter count
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_point_residuals_depth_kernel", b"pcl_pose_info_depth_kernel", b"pcl_gn_pass_depth_kernel", b"pcl_depth_pose_rows_kernel"):
        assert kernel in blob, kernel
    doc = re.search(r"/\* Residuals, pose information and LM polish under the depth mask.*?\*/", raw, flags=re.S).group(0)
    for word in ("BUILD-DEFINED", "exactly -1", "visible", "PCL_EWORKSPACE", "Deliberately left out", "graph capture", "real data"):
        assert word in doc, word


def test_the_sources_hold_no_atomics_and_the_loss_kernel_hash_covers_its_four_files(lib):
    """pcl_info.hip, pcl_gn.hip, the new translation unit and the pass they are built from hold no atomicAdd; of pcl_residual.hip the part in
    front of the robust weights does (the radix select behind it counts with integer atomics and always has).  The library carries the
    hash of the four loss-kernel files alone, which do not name the new file."""
    import hashlib
    from piccolo_amd import build
    for name in ("pcl_info.hip", "pcl_gn.hip", "pcl_depth_info.hip", "pcl_point_pass.h", "pcl_info_device.h", "pcl_gn_device.h"):
        assert "atomicAdd" not in open(os.path.join(build.CSRC, name)).read(), name
    res = open(os.path.join(build.CSRC, "pcl_residual.hip")).read()
    head, marker, _ = res.partition("// robust weights: the scale of every residual row")
    assert marker and "pcl_point_residuals_images" in head and "atomicAdd" not in head
    assert os.path.join(build.CSRC, "pcl_depth_info.hip") in build.sources()
    h = hashlib.sha256()
    for name in ("pcl_loss.hip", "pcl_sample_device.h", "pcl_gd_device.h", "pcl_device.h"):
        text = open(os.path.join(build.CSRC, name), "rb").read()
        assert b"pcl_depth_info" not in text and b"PclPassDepth" not in text, name
        h.update(text)
    assert h.hexdigest()[:16] == build.loss_kernel_source_hash() == lib.pcl_source_hash().decode()


def test_size_queries(lib):
    res, info, gnq = lib.pcl_point_residuals_depth_workspace_bytes, lib.pcl_pose_information_depth_workspace_bytes, lib.pcl_gn_depth_workspace_bytes
    # bad arguments: 0
    for B, dh, dw in ((0, 16, 32), (-1, 16, 32), (3, 1, 32), (3, 16, 1), (3, 0, 0), (3, -4, 32), (3, 1 << 24, 32), (3, 16, 1 << 24), (4, 1 << 14, 1 << 14)):
        assert res(B, dh, dw) == 0, (B, dh, dw)
        assert info(1025, B, dh, dw) == 0 and gnq(1025, B, dh, dw) == 0, (B, dh, dw)
    for n in (0, -5, (1 << 27) + 1):
        assert info(n, 3, 16, 32) == 0 and gnq(n, 3, 16, 32) == 0, n
    assert info(1 << 27, 1 << 22, 2, 2) == 0 and gnq(1 << 27, 1 << 22, 2, 2) == 0           # more blocks than a grid holds
    grids = ((2, 2), (16, 32), (24, 40), (64, 128), (64, 256), (200, 400))
    Bs = (1, 2, 3, 32, 33)
    ns = (1, 2, 511, 512, 513, 700, 1025, 33768, 166667, 1 << 20)
    for dh, dw in grids:
        sizes = [res(B, dh, dw) for B in Bs]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), (dh, dw)
        assert all(s >= B * 64 + B * dh * dw * 4 for s, B in zip(sizes, Bs))                 # pose records and z-buffers
    for B in Bs:
        sizes = [res(B, dh, dw) for dh, dw in grids]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), B
    for q, plain in ((info, lib.pcl_pose_information_workspace_bytes), (gnq, lib.pcl_gn_workspace_bytes)):
        for dh, dw in grids:
            for B in Bs:
                sizes = [q(n, B, dh, dw) for n in ns]
                assert all(s > 0 and s % 256 == 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), (dh, dw, B)
                # the three regions: what the residuals' query holds, then the plain call's partial rows
                assert all(s == res(B, dh, dw) + plain(n, B) for s, n in zip(sizes, ns)), (dh, dw, B)
            for n in ns:
                sizes = [q(n, B, dh, dw) for B in Bs]
                assert all(b >= a for a, b in zip(sizes, sizes[1:])), (dh, dw, n)
        for n in ns:
            for B in Bs:
                sizes = [q(n, B, dh, dw) for dh, dw in grids]
                assert all(b >= a for a, b in zip(sizes, sizes[1:])), (n, B)


# never dereferenced on the host
C, P, T_, R, O, V, WS, ST, OUT, INFO, COV, TR, ORD = (0x10000 * (i + 1) for i in range(13))


def _common_refusals(call, need):
    """what all three entry points refuse alike; call(**overrides) runs one with valid defaults"""
    for name in ("cloud", "pano", "trans", "rot", "work"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL and call(n=(1 << 27) + 1, nbytes=1 << 40) == EINVAL
    assert call(B=0) == EINVAL and call(B=-2) == EINVAL
    assert call(H=0) == EINVAL and call(W=-1) == EINVAL
    for fmt in (3, 4, 7, -1):                                 # the trim launch's texel layouts, and no layout at all
        assert call(fmt=fmt) == EINVAL, fmt
    assert call(fmt=0, H=1 << 14, W=1 << 13) == EINVAL        # a packed float4 panorama of 2 GiB
    for ps in (2, 0, -16):
        assert call(ps=ps) == EINVAL, ps
    for dh, dw in ((1, 32), (16, 1), (0, 0), (-3, 32), (1 << 24, 32), (16, 1 << 24), (1 << 15, 1 << 15)):
        assert call(dh=dh, dw=dw, nbytes=1 << 60) == EINVAL, (dh, dw)
    for tau in (-0.01, float("nan"), float("inf"), -float("inf")):
        assert call(tau=tau) == EINVAL, tau
    for st in (0, -1, 65, 1 << 20):
        assert call(stride=st) == EINVAL, st
    assert call(nbytes=need - 1) == EWORKSPACE and call(nbytes=0) == EWORKSPACE
    assert call(B=4) == EWORKSPACE                             # the workspace of three poses is short for four


def test_point_residuals_depth_refusals_before_any_device_call(lib):
    need = lib.pcl_point_residuals_depth_workspace_bytes(3, 16, 32)

    def call(cloud=C, n=1025, pano=P, fmt=2, H=32, W=64, trans=T_, rot=R, ps=3, B=3, dh=16, dw=32, tau=0.05, stride=1, order=None, out=O, vis=V, work=WS,
             nbytes=need):
        return lib.pcl_point_residuals_depth(cloud, n, pano, fmt, H, W, trans, rot, ps, B, dh, dw, tau, stride, order, out, vis, work, nbytes, None)
    _common_refusals(call, need)
    assert call(out=None) == EINVAL and call(out=None, order=ORD) == EINVAL
    assert call(n=1 << 27, B=1 << 22, dh=2, dw=2, nbytes=1 << 60) == EINVAL          # more blocks than a grid holds


def test_pose_information_depth_refusals_before_any_device_call(lib):
    need = lib.pcl_pose_information_depth_workspace_bytes(1025, 3, 16, 32)

    def call(cloud=C, n=1025, pano=P, fmt=2, H=32, W=64, trans=T_, rot=R, ps=3, B=3, dh=16, dw=32, tau=0.05, stride=1, objective=0, delta=0.0, info=INFO,
             cov=COV, work=WS, nbytes=need):
        return lib.pcl_pose_information_depth(cloud, n, pano, fmt, H, W, trans, rot, ps, B, dh, dw, tau, stride, objective, delta, info, cov, work, nbytes,
                                              None)
    _common_refusals(call, need)
    assert call(info=None) == EINVAL
    for objective in (-1, 2, 7):
        assert call(objective=objective) == EINVAL, objective
    for delta in (0.0, -1.0, 2.0 ** -21, 4.5, float("nan"), float("inf")):            # pcl_info_l1_args' rule, under objective 1 only
        assert call(objective=1, delta=delta) == EINVAL, delta
    assert call(objective=1, delta=1.0 / 64, nbytes=need - 1) == EWORKSPACE           # (a good delta gets as far as the workspace check)
    assert call(cov=None, nbytes=need - 1) == EWORKSPACE                              # (and so does a null cov under L2: it is nullable)
    assert call(n=1 << 27, B=1 << 22, dh=2, dw=2, nbytes=1 << 60) == EINVAL


def test_gn_refine_depth_refusals_before_any_device_call(lib):
    from piccolo_amd import _lib
    need = lib.pcl_gn_depth_workspace_bytes(1025, 3, 16, 32)
    good = dict(lam0=1e-3, lam_up=10.0, lam_down=0.1, lam_min=1e-9, lam_max=1e9, step_cap=0.1, tol=0.0)

    def call(cloud=C, n=1025, pano=P, fmt=2, H=32, W=64, trans=T_, rot=R, ps=3, B=3, dh=16, dw=32, tau=0.05, stride=1, objective=0, delta=0.0, hyper=good,
             iters=4, state=ST, out=OUT, info=INFO, cov=COV, trace=TR, work=WS, nbytes=need):
        hp = None if hyper is None else ctypes.byref(_lib.GnHyper(**hyper))
        return lib.pcl_gn_refine_depth(cloud, n, pano, fmt, H, W, trans, rot, ps, B, dh, dw, tau, stride, objective, delta, hp, iters, state, out, info,
                                       cov, trace, work, nbytes, None)
    _common_refusals(call, need)
    for name in ("hyper", "state", "out", "info"):
        assert call(**{name: None}) == EINVAL, name
    assert call(iters=-1) == EINVAL and call(iters=1001) == EINVAL
    for key, v in (("lam0", 0.0), ("lam_up", 1.0), ("lam_down", 0.0), ("lam_down", 1.5), ("step_cap", 0.0), ("tol", -1.0), ("lam0", float("nan"))):
        assert call(hyper=dict(good, **{key: v})) == EINVAL, (key, v)
    assert call(hyper=dict(good, lam_min=2.0, lam_max=1.0)) == EINVAL
    for objective in (-1, 2):
        assert call(objective=objective) == EINVAL, objective
    for delta in (0.0, 2.0 ** -21, 4.5, float("nan")):
        assert call(objective=1, delta=delta) == EINVAL, delta
    assert call(objective=1, delta=1.0 / 64, nbytes=need - 1) == EWORKSPACE
    assert call(cov=None, nbytes=need - 1) == EWORKSPACE and call(cov=None, trace=None, nbytes=need - 1) == EWORKSPACE      # both nullable


def test_python_surface_refuses_before_a_device(lib):
    """ops: return_visible without depth, a weighted cloud or a cloud of colour sets with depth — ValueError from dummies, no device"""
    from types import SimpleNamespace
    from piccolo_amd import ops
    pano = SimpleNamespace(H=32, W=64, fmt=2, data=None)
    plain = SimpleNamespace(n=1025, weights=None, color_sets=1, data=None, order=None)
    with pytest.raises(ValueError, match="return_visible goes with depth"):
        ops.point_residuals(plain, pano, None, None, return_visible=True)
    with pytest.raises(ValueError, match="return_visible goes with depth"):
        ops.point_residuals_at_winners(plain, pano, None, return_visible=True)
    weighted = SimpleNamespace(n=1025, weights=object(), color_sets=1, data=None, order=None)
    sets = SimpleNamespace(n=1025, weights=None, color_sets=3, data=None, order=None)
    calls = (lambda c: ops.point_residuals(c, pano, None, None, depth=True), lambda c: ops.point_residuals_at_winners(c, pano, None, depth=True),
             lambda c: ops.pose_information(c, pano, None, None, depth=True), lambda c: ops.pose_information_at_winners(c, pano, None, depth=True),
             lambda c: ops.gauss_newton_refine(c, pano, None, None, depth=True), lambda c: ops.gauss_newton_refine_at_winners(c, pano, None, depth=True))
    for f in calls:
        with pytest.raises(ValueError, match="weights do not combine with depth"):
            f(weighted)
        with pytest.raises(ValueError, match="colour sets"):
            f(sets)
