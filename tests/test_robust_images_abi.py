"""CPU checks of the boundary of the robust chain over several images (additive to ABI 12): pcl_gd_run_weight_sets with its size, plan and
init entry points, pcl_point_residuals_images and pcl_robust_weights_rows with its workspace query are declared, bound and exported, the
size queries answer 0 for out-of-range arguments and grow with the set count, and every listed refusal answers PCL_EINVAL before anything
touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")
NEW = ("pcl_gd_weight_sets_workspace_bytes", "pcl_gd_plan_weight_sets", "pcl_gd_init_weight_sets", "pcl_gd_run_weight_sets",
       "pcl_point_residuals_images", "pcl_robust_weights_rows_workspace_bytes", "pcl_robust_weights_rows")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def hyper(**kw):
    from piccolo_amd import _lib
    h = _lib.GdHyper()
    h.lr, h.factor, h.patience, h.mode = 0.1, 0.9, 5, _lib.GD_BATCH
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bsize_t\s+pcl_gd_weight_sets_workspace_bytes\s*\(\s*int64_t\s+n\s*,\s*int\s+B\s*,\s*int\s+nsets\s*,", text)
    assert re.search(r"\bint\s+pcl_gd_plan_weight_sets\s*\(", text) and re.search(r"\bint\s+pcl_gd_init_weight_sets\s*\(", text)
    # pcl_gd_run_weighted's signature plus nsets
    weighted = re.search(r"\bint\s+pcl_gd_run_weighted\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    sets = re.search(r"\bint\s+pcl_gd_run_weight_sets\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    names = lambda a: [re.sub(r"\s+", " ", p.strip()) for p in a.split(",")]      # noqa: E731
    assert [p for p in names(sets) if p != "int nsets"] == names(weighted) and "int nsets" in names(sets)
    assert re.search(r"\bint\s+pcl_point_residuals_images\s*\(", text)
    assert re.search(r"\bsize_t\s+pcl_robust_weights_rows_workspace_bytes\s*\(\s*int64_t\s+n\s*,\s*int\s+nrows\s*\)", text)
    assert re.search(r"\bint\s+pcl_robust_weights_rows\s*\(", text)
    assert len(_lib.SIGNATURES["pcl_gd_run_weight_sets"][1]) == len(_lib.SIGNATURES["pcl_gd_run_weighted"][1]) + 1
    assert len(_lib.SIGNATURES["pcl_point_residuals_images"][1]) == 14 and len(_lib.SIGNATURES["pcl_robust_weights_rows"][1]) == 10
    assert _lib.SIGNATURES["pcl_robust_weights_rows_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    for name in NEW:
        assert re.search(r"\bT %s\b" % name, out), name
        assert _lib.SIGNATURES[name][0] in (ctypes.c_int, ctypes.c_size_t)
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    blob = open(_lib.so_path(), "rb").read()
    for kernel in (b"pcl_loss_wsets_kernel", b"pcl_loss_fused_wsets_kernel", b"pcl_point_residuals_images_kernel", b"pcl_rw_init_kernel",
                   b"pcl_rw_hist_kernel", b"pcl_rw_plane_kernel"):
        assert kernel in blob, kernel
    left_out = re.search(r"Deliberately left out: weights in the initialisation stage.*?\*/", open(HEADER).read(), flags=re.S).group(0)
    assert "pcl_gd_run_weight_sets" in left_out


def test_size_queries_zero_out_of_range_and_monotone_in_the_sets(lib):
    h = hyper()
    size = lambda n, B, I, hh=h: lib.pcl_gd_weight_sets_workspace_bytes(n, B, I, ctypes.byref(hh))      # noqa: E731
    assert size(0, 6, 1) == 0 and size(-1, 6, 1) == 0 and size((1 << 27) + 1, 6, 1) == 0
    assert size(1025, 0, 1) == 0 and size(1025, 12, 0) == 0 and size(1025, 12, -3) == 0 and size(1025, 12, 5) == 0
    assert lib.pcl_gd_weight_sets_workspace_bytes(1025, 12, 3, None) == 0
    assert size(1025, 12, 3, hyper(depth_mask=1)) == 0 and size(1025, 12, 3, hyper(color_sets=2)) == 0
    assert size(1025, 12, 3, hyper(color_sets=3)) > 0 and size(1025, 12, 3, hyper(color_sets=1)) > 0
    for n, per in ((1025, 4), (50001, 6), (166667, 6), (1 << 20, 32)):
        sizes = [size(n, I * per, I) for I in (1, 2, 3, 5, 8, 16)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(b > a for a, b in zip(sizes, sizes[1:])), (n, per, sizes)
        # one set: pcl_gd_run's own workspace
        assert sizes[0] == lib.pcl_gd_workspace_bytes(n, per, 64, 128, ctypes.byref(h))
    rows = lib.pcl_robust_weights_rows_workspace_bytes
    assert rows(0, 1) == 0 and rows(-5, 2) == 0 and rows((1 << 27) + 1, 2) == 0
    assert rows(1025, 0) == 0 and rows(1025, -1) == 0 and rows(1025, 65536) == 0
    sizes = [rows(50001, I) for I in (1, 2, 3, 8, 64, 65535)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] == lib.pcl_robust_weights_workspace_bytes(50001)
    assert rows(1 << 27, 8) == rows(1025, 8)                   # (histograms only: the size does not depend on n)


def test_the_plan_is_the_single_image_plan(lib):
    h = hyper()
    for n, per in ((1025, 4), (50001, 6), (120000, 8), (166667, 6), (1 << 20, 32)):
        one = [ctypes.c_int() for _ in range(3)]
        assert lib.pcl_gd_plan(n, per, *[ctypes.byref(v) for v in one]) == 0
        for I in (1, 2, 3, 8):
            got = [ctypes.c_int() for _ in range(3)]
            assert lib.pcl_gd_plan_weight_sets(n, I * per, I, ctypes.byref(h), *[ctypes.byref(v) for v in got]) == 0
            assert (got[0].value, got[1].value) == (one[0].value, one[1].value), (n, per, I)
            assert per % got[1].value == 0                        # a group of poses never straddles two images
    assert lib.pcl_gd_plan_weight_sets(1025, 12, 5, ctypes.byref(h), None, None, None) == -1
    assert lib.pcl_gd_plan_weight_sets(1025, 12, 3, ctypes.byref(hyper(fuse=-1)), None, None, ctypes.byref(one[2])) == 0 and one[2].value == 0


def test_run_and_init_refusals_before_any_device_call(lib):
    c, w, p, st, box, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000          # never dereferenced on the host
    need = lib.pcl_gd_weight_sets_workspace_bytes(1025, 12, 3, ctypes.byref(hyper()))

    def run(cloud=c, weights=w, nsets=3, n=1025, pano=p, fmt=2, H=32, W=64, state=st, B=12, bx=box, h=hyper(), it=4, wsp=ws, nbytes=need):
        return lib.pcl_gd_run_weight_sets(cloud, weights, nsets, n, pano, fmt, H, W, state, B, bx, ctypes.byref(h) if h is not None else None, it,
                                          None, wsp, nbytes, None, None)
    assert run(nsets=0) == -1 and run(nsets=-2) == -1
    assert run(nsets=5) == -1 and run(B=13) == -1                                   # B % nsets != 0
    assert run(h=hyper(color_sets=2)) == -1 and run(h=hyper(color_sets=4)) == -1    # colour sets that are not the weight sets
    assert run(h=hyper(depth_mask=1)) == -1
    assert run(h=hyper(color_sets=-1)) == -1
    assert run(h=None) == -1
    assert run(n=0) == -1 and run(n=(1 << 27) + 1) == -1 and run(B=0) == -1
    assert run(cloud=None) == -1 and run(pano=None) == -1 and run(state=None) == -1 and run(bx=None) == -1 and run(wsp=None) == -1
    assert run(H=0) == -1 and run(it=-1) == -1 and run(h=hyper(mode=7)) == -1
    assert run(weights=None, nsets=5) == -1 and run(weights=None, h=hyper(depth_mask=1)) == -1      # the unweighted form refuses the same
    assert run(nbytes=need - 1) == -2                                                # PCL_EWORKSPACE, still before any launch

    def init(state=st, trans=c, rot=w, B=12, nsets=3, h=hyper()):
        return lib.pcl_gd_init_weight_sets(state, trans, rot, B, nsets, ctypes.byref(h) if h is not None else None, None)
    assert init(state=None) == -1 and init(trans=None) == -1 and init(rot=None) == -1 and init(h=None) == -1
    assert init(B=0) == -1 and init(nsets=0) == -1 and init(nsets=5) == -1
    assert init(h=hyper(color_sets=2)) == -1 and init(h=hyper(depth_mask=1)) == -1


def test_residuals_images_and_weights_rows_refusals_before_any_device_call(lib):
    c, t, r, o = 0x10000, 0x30000, 0x40000, 0x50000
    panos = (ctypes.c_uint64 * 3)(0x20000, 0x21000, 0x22000)
    holed = (ctypes.c_uint64 * 3)(0x20000, 0, 0x22000)

    def res(cloud=c, n=1025, sets=0, ps=panos, I=3, fmt=2, H=32, W=64, trans=t, rot=r, stride=3, out=o):
        return lib.pcl_point_residuals_images(cloud, n, sets, ps, I, fmt, H, W, trans, rot, stride, None, out, None)
    for name in ("cloud", "ps", "trans", "rot", "out"):
        assert res(**{name: None}) == -1, name
    assert res(ps=holed) == -1
    assert res(I=0) == -1 and res(I=-1) == -1
    assert res(sets=2) == -1 and res(sets=4) == -1 and res(sets=-1) == -1          # colour sets: 0 / 1 or one per image
    assert res(n=0) == -1 and res(n=(1 << 27) + 1) == -1
    assert res(n=1 << 27, sets=3) == -1                                             # a cloud of three sets past 2^31 bytes
    assert res(H=0) == -1 and res(W=-1) == -1 and res(fmt=3) == -1 and res(fmt=4) == -1 and res(fmt=9) == -1
    assert res(stride=2) == -1 and res(stride=0) == -1
    assert res(fmt=0, H=1 << 14, W=1 << 13) == -1

    row, plane, ws = 0x10000, 0x20000, 0x30000
    need = lib.pcl_robust_weights_rows_workspace_bytes(1025, 3)

    def rw(rs=row, n=1025, rows=3, kind=0, k=2.5, pl=plane, w=ws, nbytes=need):
        return lib.pcl_robust_weights_rows(rs, n, rows, kind, k, pl, None, w, nbytes, None)
    assert rw(rs=None) == -1 and rw(pl=None) == -1 and rw(w=None) == -1
    assert rw(n=0) == -1 and rw(n=(1 << 27) + 1) == -1
    assert rw(rows=0) == -1 and rw(rows=-1) == -1 and rw(rows=65536) == -1
    assert rw(kind=2) == -1 and rw(kind=-1) == -1
    assert rw(k=0.0) == -1 and rw(k=-1.0) == -1 and rw(k=float("inf")) == -1 and rw(k=float("nan")) == -1
    assert rw(nbytes=need - 1) == -1 and rw(nbytes=lib.pcl_robust_weights_rows_workspace_bytes(1025, 2)) == -1
