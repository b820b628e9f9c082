"""CPU checks of the score maps' C boundary (pcl_score_maps, pcl_score_weights and their size queries; additive to ABI 12): declared, bound
and exported, every refusal answered with PCL_EINVAL before a device is touched (there is no GPU here), size queries 0 for a shape no call
accepts and monotone in n and K."""
import ctypes
import re
import subprocess

import pytest

from test_abi import declared_symbols

NAMES = ("pcl_score_maps_workspace_bytes", "pcl_score_maps", "pcl_score_weights_workspace_bytes", "pcl_score_weights")
P = ctypes.c_void_p(0x1000)          # a non-null address that is never dereferenced: every call below is refused before any HIP call


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    assert _lib.ABI_VERSION == 12 and lib.pcl_abi_version() == 12
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    exported = set(re.findall(r"\bT (pcl_[a-z0-9_]+)", out))
    for name in NAMES:
        assert name in declared_symbols() and name in _lib.SIGNATURES and name in exported, name


def maps(lib, cloud=P, n=1000, trans=P, rot=P, K=9, H=64, W=128, nsh=4, nsw=4, inter=P, nproj=P, nimg=P, order=None, s3=P, c3=P, s2=P, c2=P, ws=P,
         nws=None):
    nws = lib.pcl_score_maps_workspace_bytes(n, K, nsh, nsw) if nws is None else nws
    return lib.pcl_score_maps(cloud, n, trans, rot, K, H, W, nsh, nsw, inter, nproj, nimg, order, s3, c3, s2, c2, ws, nws, None)


def test_score_maps_refusals(lib):
    from piccolo_amd import _lib
    big = (1 << 27) + 1
    assert lib.pcl_score_maps_workspace_bytes(1000, 9, 4, 4) > 0
    for kw in (dict(nsh=2), dict(nsw=0), dict(K=0), dict(K=65536), dict(n=0), dict(n=big), dict(n=-1),
               dict(H=3), dict(W=3),                                       # bh / bw of zero pixels
               dict(H=0), dict(W=0), dict(H=65536), dict(W=65536),
               dict(s3=None, c3=None, s2=None, c2=None),                   # both output pairs null
               dict(s3=None), dict(c2=None),                               # half a pair
               dict(cloud=None), dict(trans=None), dict(rot=None), dict(inter=None), dict(nproj=None), dict(nimg=None), dict(ws=None),
               dict(nws=lib.pcl_score_maps_workspace_bytes(1000, 9, 4, 4) - 1), dict(nws=0)):
        assert maps(lib, **kw) == -1, kw
    for shape in ((0, 9, 4, 4), (big, 9, 4, 4), (1000, 0, 4, 4), (1000, 65536, 4, 4), (1000, 9, 2, 4), (1000, 9, 4, 0)):
        assert lib.pcl_score_maps_workspace_bytes(*shape) == 0, shape
    assert b"invalid argument" in lib.pcl_error_string(-1)
    assert _lib.SIGNATURES["pcl_score_maps"][0] is ctypes.c_int


def test_score_weights_refusals(lib):
    nws = lib.pcl_score_weights_workspace_bytes(1000)
    assert nws > 0

    def call(score=P, count=P, n=1000, min_count=1, floor=0.0, plane=P, rng=None, ws=P, nws=nws):
        return lib.pcl_score_weights(score, count, n, min_count, floor, plane, rng, ws, nws, None)
    for kw in (dict(floor=1.0), dict(floor=-0.01), dict(floor=float("nan")), dict(floor=2.0), dict(min_count=0), dict(min_count=-3), dict(n=0),
               dict(n=(1 << 27) + 1), dict(score=None), dict(count=None), dict(plane=None), dict(ws=None), dict(nws=nws - 1), dict(nws=0)):
        assert call(**kw) == -1, kw
    assert lib.pcl_score_weights_workspace_bytes(0) == 0 and lib.pcl_score_weights_workspace_bytes((1 << 27) + 1) == 0
    assert lib.pcl_score_weights_workspace_bytes(-5) == 0


def test_size_queries_are_monotone(lib):
    ns = (1, 1000, 166_667, 1_000_000, 1 << 27)
    Ks = (1, 9, 50, 64, 300, 65535)
    for nsh, nsw in ((3, 1), (4, 4), (16, 32)):
        for n in ns:
            sizes = [lib.pcl_score_maps_workspace_bytes(n, K, nsh, nsw) for K in Ks]
            assert all(a > 0 for a in sizes) and all(a < b for a, b in zip(sizes, sizes[1:])), (n, sizes)
        for K in Ks:
            sizes = [lib.pcl_score_maps_workspace_bytes(n, K, nsh, nsw) for n in ns]
            assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), (K, sizes)
    # the table is K x (nblk + 1) floats behind K 64-byte pose records, each region a multiple of 256 bytes
    align = lambda v: (v + 255) & ~255                                     # noqa: E731
    assert lib.pcl_score_maps_workspace_bytes(1_000_000, 64, 16, 32) == align(64 * 64) + align(64 * 449 * 4)
    sizes = [lib.pcl_score_weights_workspace_bytes(n) for n in ns]
    assert all(a > 0 for a in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
