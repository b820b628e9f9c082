"""CPU checks of pcl_gd_prune's boundary and of the prune schedule: the symbol is declared, bound and exported (ABI still 12), its
refusals answer PCL_EINVAL before anything touches a device, omniloc.prune_schedule reads the int and list forms of cfg.prune_iters /
cfg.prune_keep and refuses every malformed one, and the shipped pruned config parses to the expected lists."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO, Cfg

HEADER = os.path.join(REPO, "include", "piccolo_hip.h")


@pytest.fixture(scope="module")
def lib():
    from piccolo_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_declared_bound_and_exported(lib):
    from piccolo_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+pcl_gd_prune\s*\(", text)
    assert re.search(r"#define\s+PCL_GD_PRUNE_MAX\s+1024\b", text) and _lib.GD_PRUNE_MAX == 1024
    res, args = _lib.SIGNATURES["pcl_gd_prune"]
    assert res is ctypes.c_int and len(args) == 9
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.so_path()], text=True)
    assert re.search(r"\bT pcl_gd_prune\b", out)
    assert lib.pcl_abi_version() == 12 and _lib.ABI_VERSION == 12
    assert b"pcl_gd_prune_kernel" in open(_lib.so_path(), "rb").read()


def test_refusals_before_any_device_call(lib):
    """null / bogus pointers, no device: every listed refusal is PCL_EINVAL"""
    a, b, sv = 0x10000, 0x20000, 0x30000                     # never dereferenced on the host

    def prune(state_in, groups, per_group, keep, state_out, survivors):
        return lib.pcl_gd_prune(state_in, groups, per_group, keep, state_out, survivors, None, None, None)
    assert prune(None, 1, 8, 4, b, sv) == -1
    assert prune(a, 1, 8, 4, None, sv) == -1
    assert prune(a, 1, 8, 4, b, None) == -1
    assert prune(a, 1, 8, 4, a, sv) == -1                    # in place
    assert prune(a, 0, 8, 4, b, sv) == -1 and prune(a, -1, 8, 4, b, sv) == -1
    assert prune(a, 1, 8, 0, b, sv) == -1 and prune(a, 1, 8, -1, b, sv) == -1
    assert prune(a, 1, 8, 9, b, sv) == -1                    # keep > per_group
    assert prune(a, 1, 0, 1, b, sv) == -1
    assert prune(a, 1, 1025, 4, b, sv) == -1                 # per_group > PCL_GD_PRUNE_MAX
    assert prune(a, 1, 1025, 1025, b, sv) == -1
    assert prune(a, 1 << 21, 1024, 4, b, sv) == -1           # groups * per_group past 2^30
    assert prune(a + 8, 1, 8, 4, b, sv) == -1 and prune(a, 1, 8, 4, b + 4, sv) == -1      # records move as 16-byte words


def _cfg(**kw):
    return Cfg(num_iter=100, **kw)


def test_prune_schedule_int_and_list_forms():
    from piccolo_amd import omniloc as po
    assert po.prune_schedule(_cfg(), 32) is None
    assert po.prune_schedule(_cfg(prune_iters=None, prune_keep=None), 32) is None
    assert po.prune_schedule(_cfg(prune_iters=20, prune_keep=4), 6) == [(20, 6), (80, 4)]
    assert po.prune_schedule(_cfg(prune_iters=[20], prune_keep=[4]), 6) == [(20, 6), (80, 4)]
    assert po.prune_schedule(_cfg(prune_iters=[20, 40], prune_keep=[16, 8]), 32) == [(20, 32), (20, 16), (60, 8)]
    assert po.prune_schedule(_cfg(prune_iters=(20, 40), prune_keep=(8, 4)), 16) == [(20, 16), (20, 8), (60, 4)]
    assert po.prune_schedule(_cfg(prune_iters=[1, 99], prune_keep=[32, 32]), 32) == [(1, 32), (98, 32), (1, 32)]      # keep == per_image: a plain copy
    assert po.prune_schedule(_cfg(prune_iters=5, prune_keep=1024), 1024) == [(5, 1024), (95, 1024)]
    # the work ratio of the shipped schedule: sum candidates x iterations / (B x num_iter)
    assert sum(k * c for k, c in po.prune_schedule(_cfg(prune_iters=[20, 40], prune_keep=[16, 8]), 32)) / (32 * 100) == 0.45


@pytest.mark.parametrize("iters,keep,per_image", [
    ([20, 40], [16], 32),                    # unequal lengths
    (20, [16, 8], 32),
    (20, None, 32),                          # one key without the other
    (None, 8, 32),
    ([], [], 32),
    ([40, 20], [16, 8], 32),                 # not increasing
    ([20, 20], [16, 8], 32),                 # not strictly
    (0, 8, 32),                              # outside (0, num_iter)
    (100, 8, 32),
    ([20, 120], [16, 8], 32),
    ([20, 40], [8, 16], 32),                 # keep grows
    (20, 0, 32),                             # keep outside 1 .. per_image
    (20, 33, 32),
    (20, 8, 2048),                           # more than PCL_GD_PRUNE_MAX candidates per image
    (20, 1025, 2048),
    (20.0, 8, 32),                           # not ints
    ([20, 40], [16, True], 32),
    ("20", 8, 32),
])
def test_prune_schedule_refuses(iters, keep, per_image):
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError):
        po.prune_schedule(_cfg(prune_iters=iters, prune_keep=keep), per_image)


def test_pruned_config_parses_to_the_lists():
    from piccolo_amd import omniloc as po
    from piccolo_amd import parse_utils
    base = parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))._asdict()
    cfg = parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_prune.ini"))
    got = cfg._asdict()
    assert got.pop("prune_iters") == [20, 40] and got.pop("prune_keep") == [16, 8]
    assert got == base                                        # the b32 config plus the two keys
    assert po.prune_schedule(cfg, cfg.num_input) == [(20, 32), (20, 16), (60, 8)]
    assert po.prune_schedule(parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini")), 32) is None
    one = parse_utils.apply_override(parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini")), "prune_iters=20,prune_keep=4")
    assert po.prune_schedule(one, 32) == [(20, 32), (80, 4)]


def test_entry_points_that_return_every_candidate_refuse_the_keys():
    """omniloc and omniloc_all raise before they touch a device"""
    import torch
    from piccolo_amd import omniloc as po
    z = torch.zeros(4, 3)
    cfg = _cfg(prune_iters=20, prune_keep=2, num_input=4)
    with pytest.raises(ValueError):
        po.omniloc_all(torch.zeros(4, 8, 3), z, z, z.clone(), z.clone(), cfg, {})
    with pytest.raises(ValueError):
        po.omniloc(torch.zeros(4, 8, 3), z, z, z.clone(), z.clone(), 0, cfg, {})
