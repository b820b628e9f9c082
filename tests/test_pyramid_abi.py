"""The panorama pyramid's C boundary, without a device: the three symbols in header, binding and library, the ABI version they were added
under, pcl_pano_pyramid_bytes against the sum of pcl_pano_bytes, and what the sizing function and the calls refuse."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

SYMBOLS = ("pcl_pano_pyramid_bytes", "pcl_pano_pyramid", "pcl_gd_plateau_reset")
F32, U8, F16, U8P, U8V = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib
    return _lib.load()


def fmts(*codes):
    return (ctypes.c_int * len(codes))(*codes)


def test_header_binding_and_library_agree_on_the_three_symbols(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "piccolo_hip.h")).read(), flags=re.S)
    exported = set(re.findall(r"\bT (pcl_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)))
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and name in exported
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"size_t\s+pcl_pano_pyramid_bytes\(int H, int W, int levels, const int \*formats\)", text)
    assert re.search(r"int\s+pcl_pano_pyramid\(const float \*img_hwc, int H, int W, int levels, const int \*formats, void \*texels, float \*images, "
                     r"int \*not_exact,\s+void \*stream\)", text)
    assert re.search(r"int\s+pcl_gd_plateau_reset\(void \*state, int B, void \*stream\)", text)
    assert len(_lib.SIGNATURES["pcl_pano_pyramid_bytes"][1]) == 4 and len(_lib.SIGNATURES["pcl_pano_pyramid"][1]) == 9
    assert len(_lib.SIGNATURES["pcl_gd_plateau_reset"][1]) == 3
    # additive: the version the existing tests pin
    assert _lib.ABI_VERSION == 12 and lib.pcl_abi_version() == 12
    assert "#define PCL_ABI_VERSION 12" in open(os.path.join(REPO, "include", "piccolo_hip.h")).read()
    # the header states the rule
    head = open(os.path.join(REPO, "include", "piccolo_hip.h")).read()
    for words in ("cascaded", "ties up", "NO latitude weighting", "black iff there is no data under it"):
        assert words in head, words


def test_pyramid_bytes_is_the_sum_of_the_levels_each_rounded_up_to_256(lib):
    for H, W in ((2, 2), (6, 10), (16, 32), (48, 80), (272, 528), (1024, 2048), (2048, 4096)):
        for levels in (1, 2, 3, 4):
            if H % (1 << levels) or W % (1 << levels):
                continue
            for codes in ((F16,) * levels, (U8,) * levels, (F32,) * levels, (U8, F16, F32, U8)[:levels], (F32, U8, F16, F16)[:levels]):
                want = 0
                for l, c in enumerate(codes, 1):
                    size = lib.pcl_pano_bytes(H >> l, W >> l, c)
                    assert size == ((H >> l) + 2) * ((W >> l) + 2) * {F32: 16, U8: 4, F16: 8}[c]
                    assert want % 256 == 0                               # every level starts on a 256-byte boundary
                    want += (size + 255) // 256 * 256
                assert lib.pcl_pano_pyramid_bytes(H, W, levels, fmts(*codes)) == want, (H, W, codes)


def test_what_the_sizing_function_refuses(lib):
    ok = fmts(F16, F16, F16, F16, F16)
    assert lib.pcl_pano_pyramid_bytes(16, 32, 4, ok) > 0
    for levels in (0, 5, -1):
        assert lib.pcl_pano_pyramid_bytes(64, 64, levels, ok) == 0
    for H, W, levels in ((3, 4, 1), (4, 3, 1), (6, 8, 2), (8, 6, 2), (16, 24, 4), (24, 16, 4), (0, 16, 1), (16, 0, 1), (-16, 16, 1)):
        assert lib.pcl_pano_pyramid_bytes(H, W, levels, ok) == 0, (H, W, levels)
    for bad in (U8P, U8V, 5, -1):
        assert lib.pcl_pano_pyramid_bytes(16, 32, 1, fmts(bad)) == 0
        assert lib.pcl_pano_pyramid_bytes(16, 32, 2, fmts(F16, bad)) == 0
        assert lib.pcl_pano_pyramid_bytes(16, 32, 1, fmts(F16, bad)) > 0     # (only the first `levels` entries are read)
    assert lib.pcl_pano_pyramid_bytes(16, 32, 1, None) == 0


def test_the_calls_refuse_before_touching_a_device(lib):
    """PCL_EINVAL from host-side checks alone: this runs without a GPU (the pointers are never dereferenced)"""
    buf = (ctypes.c_char * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)              # 16-byte aligned for certain: p + 4 below is misaligned for certain
    ok = fmts(F16, F16, F16, F16)
    assert lib.pcl_pano_pyramid(None, 16, 32, 1, ok, p, None, p, None) == -1
    assert lib.pcl_pano_pyramid(p, 16, 32, 1, None, p, None, p, None) == -1
    assert lib.pcl_pano_pyramid(p, 16, 32, 1, ok, None, None, p, None) == -1
    assert lib.pcl_pano_pyramid(p, 16, 32, 1, ok, p, None, None, None) == -1
    for H, W, levels in ((16, 32, 0), (16, 32, 5), (15, 32, 1), (16, 31, 1), (16, 24, 4)):
        assert lib.pcl_pano_pyramid(p, H, W, levels, ok, p, None, p, None) == -1
    assert lib.pcl_pano_pyramid(p, 16, 32, 1, fmts(U8P), p, None, p, None) == -1
    assert lib.pcl_pano_pyramid(ctypes.c_void_p(p.value + 4), 16, 32, 1, ok, p, None, p, None) == -1      # (pixel pairs are read as 8-byte words)
    assert lib.pcl_gd_plateau_reset(None, 4, None) == -1
    assert lib.pcl_gd_plateau_reset(p, 0, None) == -1
    assert lib.pcl_gd_plateau_reset(p, -3, None) == -1


def test_the_python_side_refuses_shapes_on_the_host():
    from piccolo_amd import ops
    assert ops.PYRAMID_MAX_LEVELS == 4
    assert ops.pyramid_shape(16, 32, 4) == 4 and ops.pyramid_shape(2, 2, 1) == 1
    for H, W, levels in ((16, 32, 0), (16, 32, 5), (16, 32, True), (16, 32, 1.0), (6, 8, 2), (8, 6, 2), (0, 0, 1)):
        with pytest.raises(ValueError):
            ops.pyramid_shape(H, W, levels)
