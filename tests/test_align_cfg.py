"""CPU checks of the alignment configuration: cfg_rules.align_rules reads its keys and refuses every malformed one, gravity_aligned = False
without the switch stays the loops' NotImplementedError word for word, dataset_plan carries the answer without growing a field, the
loops raise before they read a file, and the shipped config is the b32 one plus the stated keys."""
import os

import pytest

from conftest import REPO, Cfg

REFUSAL = ("gravity_aligned = False: the reference's own path stops at the undefined "
           "data_utils.obtain_align_matrix (localize.py:155); align the cloud beforehand")


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 6)
    kw.setdefault("parallel", True)
    return Cfg(**kw)


ON = dict(gravity_aligned=False, align_cloud=True)


@pytest.fixture(scope="module")
def rules():
    from piccolo_amd import cfg_rules
    return cfg_rules


def test_align_rules_reads_the_keys(rules):
    assert rules.align_rules(_cfg()) is None
    assert rules.align_rules(_cfg(align_cloud=None, align_voxel=None, align_max_tilt=None, align_yaw=None, align_min_count=None)) is None
    assert rules.align_rules(_cfg(align_cloud=False)) is None and rules.align_rules(_cfg(align_cloud=False, gravity_aligned=False)) is None
    assert rules.align_rules(_cfg(**ON)) == (0.1, 40.0, False, 8)
    got = rules.align_rules(_cfg(align_voxel=2, align_max_tilt=45, align_yaw=True, align_min_count=3, **ON))
    assert got == rules.AlignRules(2.0, 45.0, True, 3) and got._fields == ("voxel", "max_tilt", "yaw", "min_count")
    assert rules.align_rules(_cfg(align_voxel=0.25, align_max_tilt=12.5, align_yaw=False, **ON)) == (0.25, 12.5, False, 8)
    assert rules.ALIGN_KEYS == ("align_cloud", "align_voxel", "align_max_tilt", "align_yaw", "align_min_count")
    assert rules._EXTENSIONS["align"][0] == rules.ALIGN_KEYS and "align_cloud" in rules.__doc__


@pytest.mark.parametrize("key,value", [("align_voxel", 0.1), ("align_max_tilt", 30), ("align_yaw", True), ("align_yaw", False), ("align_min_count", 8)])
def test_side_keys_need_the_switch(rules, key, value):
    for switch in ({}, dict(align_cloud=False), dict(align_cloud=None)):
        with pytest.raises(ValueError, match="cfg.%s goes with cfg.align_cloud = True" % key):
            rules.align_rules(_cfg(gravity_aligned=False, **{key: value}, **switch))


def test_the_switch_needs_a_cloud_that_is_not_aligned(rules):
    for extra in ({}, dict(gravity_aligned=True)):
        with pytest.raises(ValueError, match="cfg.align_cloud goes with cfg.gravity_aligned = False"):
            rules.align_rules(_cfg(align_cloud=True, **extra))
    for loop in ("localize_stanford", "localize_omniscenes"):
        with pytest.raises(ValueError, match="nothing to align"):
            rules.dataset_plan(_cfg(align_cloud=True), loop)


@pytest.mark.parametrize("key,values,text", [
    ("align_cloud", (1, 0, "True", 1.0), "a bool"),
    ("align_yaw", (1, "yes", 0.0), "a bool"),
    ("align_voxel", (0, -0.1, float("nan"), float("inf"), "0.1", True), "a positive finite number"),
    ("align_voxel", (2.0001, 5), "at most 2"),
    ("align_max_tilt", (0, -1, 45.001, 90, float("nan"), "40", True), r"degrees in \(0, 45\]"),
    ("align_min_count", (2, 0, -3, 8.0, True, "8"), "an int >= 3")])
def test_malformed_values(rules, key, values, text):
    for v in values:
        with pytest.raises(ValueError, match="cfg.%s .*%s" % (key, text)):
            rules.align_rules(_cfg(**{**ON, key: v}))


def test_gravity_aligned_false_alone_stays_the_refusal():
    """no file is read: the roots do not exist"""
    from piccolo_amd import localize
    for loop, dataset in ((localize.localize_stanford, "Stanford2D-3D-S"), (localize.localize_omniscenes, "OmniScenes")):
        for extra in ({}, dict(align_cloud=False), dict(align_cloud=None)):
            with pytest.raises(NotImplementedError) as e:
                loop(_cfg(dataset=dataset, gravity_aligned=False, **extra), None, None, root="/nonexistent/root")
            assert str(e.value) == REFUSAL
        with pytest.raises(ValueError, match="cfg.align_voxel goes with cfg.align_cloud = True"):
            loop(_cfg(dataset=dataset, align_voxel=0.1), None, None, root="/nonexistent/root")
        with pytest.raises(ValueError, match="nothing to align"):
            loop(_cfg(dataset=dataset, align_cloud=True), None, None, root="/nonexistent/root")
        with pytest.raises(ValueError, match="align_min_count"):
            loop(_cfg(dataset=dataset, align_min_count=2, **ON), None, None, root="/nonexistent/root")


def test_dataset_plan_carries_the_answer_and_keeps_its_fields(rules):
    assert rules.DatasetPlan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")
    assert rules.DatasetPlan("plain", 1, True, None, None, False).align is None
    for loop in ("localize_stanford", "localize_omniscenes"):
        assert rules.dataset_plan(_cfg(), loop).align is None
        plan = rules.dataset_plan(_cfg(align_yaw=True, **ON), loop)
        assert plan == rules.DatasetPlan("plain", 1, True, None, None, False) and plan.align == (0.1, 40.0, True, 8)
        assert plan._fields == rules.DatasetPlan._fields
        moved = plan._replace(group_size=4)                                    # (a changed plan keeps the answer)
        assert moved.group_size == 4 and moved.align == plan.align and moved[:1] + moved[2:] == plan[:1] + plan[2:]
    # the aligned cloud is a cloud: the switch stands next to every other family, and the route is that family's
    for other, route in ((dict(images_per_launch=4), "plain"), (dict(robust_iters=20), "robust"), (dict(room_search=True, room_search_images=2), "rooms"),
                         (dict(depth_mask=True), "plain"), (dict(score_weights=True), "scored"), (dict(gn_iters=5, polish_images_per_launch=4), "polished"),
                         (dict(density_weights=True, density_voxel=0.05), "plain"), (dict(voxel_size=0.05), "plain"),
                         (dict(pose_covariance=True, polish_images_per_launch=2), "polished")):
        plan = rules.dataset_plan(_cfg(**other, **ON), "localize_stanford")
        assert plan.route == route and plan.align == (0.1, 40.0, False, 8), other
        assert plan == rules.dataset_plan(_cfg(**other), "localize_stanford")


def test_the_synthetic_driver_refuses_the_keys():
    from piccolo_amd import localize
    for key, value in (("align_cloud", True), ("align_voxel", 0.1), ("align_yaw", True)):
        with pytest.raises(ValueError, match="localize_synthetic does not take cfg.%s" % key):
            localize.localize_synthetic(_cfg(**{key: value}))


def test_shipped_config_is_b32_plus_the_stated_keys(rules):
    from piccolo_amd.parse_utils import parse_ini
    b32 = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))._asdict()
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_align.ini"))
    got = cfg._asdict()
    assert {k: v for k, v in got.items() if k not in b32} == dict(gravity_aligned=False, align_cloud=True, align_yaw=True)
    assert {k: v for k, v in got.items() if k in b32} == b32
    assert rules.align_rules(cfg) == (0.1, 40.0, True, 8)
    plan = rules.dataset_plan(cfg, "localize_stanford")
    assert plan == rules.DatasetPlan("plain", 1, True, None, None, False) and plan.align == (0.1, 40.0, True, 8)
