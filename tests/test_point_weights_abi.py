"""CPU checks of the per-point-weights boundary: the four new symbols are declared, bound and exported, the sizing function behaves,
the ABI version is unchanged and null calls are refused before anything touches a device."""
import ctypes
import re
import subprocess

import pytest

from test_abi import declared_symbols

NEW = ("pcl_cloud_weights_bytes", "pcl_cloud_pack_weights", "pcl_sampling_loss_weighted", "pcl_gd_run_weighted")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_header_binding_and_library_have_the_weight_symbols(lib):
    from piccolo_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    exported = set(re.findall(r"\bT (pcl_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in declared_symbols() and name in _lib.SIGNATURES and name in exported, name


def test_weight_plane_size_and_abi_version(lib):
    assert lib.pcl_cloud_weights_bytes(1000) == 1024 * 4 and lib.pcl_cloud_weights_bytes(0) == 0
    assert lib.pcl_cloud_weights_bytes(256) == 256 * 4 and lib.pcl_cloud_weights_bytes(257) == 512 * 4
    assert lib.pcl_cloud_weights_bytes((1 << 27) + 1) == 0 and lib.pcl_cloud_weights_bytes(-5) == 0
    assert lib.pcl_abi_version() == 12


def test_weighted_entry_points_reject_null_arguments(lib):
    from piccolo_amd import _lib
    assert lib.pcl_cloud_pack_weights(None, None, 10, None, None, None) == -1
    assert lib.pcl_sampling_loss_weighted(None, None, 10, None, 0, 4, 8, None, None, 1, 1, None, None, 0, None) == -1
    assert lib.pcl_gd_run_weighted(None, None, 10, None, 0, 4, 8, None, 1, None, None, 1, None, None, 0, None, None) == -1
    # a hyper-parameter block alone does not make the call valid
    hy = _lib.GdHyper(0.1, 0.8, 5, _lib.GD_BATCH, 0, 0.0, 0, 0, 0, 0, 0, 0)
    assert lib.pcl_gd_run_weighted(None, None, 10, None, 0, 4, 8, None, 1, None, ctypes.byref(hy), 1, None, None, 0, None, None) == -1


def test_python_surface_takes_weights_last():
    import inspect
    from piccolo_amd import localize, omniloc, ops
    for f in (omniloc.omniloc, omniloc.omniloc_all, omniloc.omniloc_batch, omniloc.sampling_loss, omniloc.SamplingLoss.__init__,
              omniloc.BatchSamplingLoss.__init__, localize.refine_image, ops.Cloud.__init__):
        p = list(inspect.signature(f).parameters.values())[-1]
        assert p.name == "weights" and p.default is None, f
    assert ops.Cloud.weights is None and hasattr(ops.Cloud, "set_weights")
