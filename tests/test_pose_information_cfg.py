"""CPU checks of cfg.pose_covariance: omniloc.pose_covariance_flag reads a bool and refuses everything else and the depth mask next to
it, and every entry point and harness path that returns no covariance refuses the key with a ValueError that names it — before it touches
a device."""
import pytest
import torch

from conftest import Cfg

KEY = "pose_covariance"


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    return Cfg(**kw)


def test_the_flag_is_a_bool_and_absent_by_default():
    from piccolo_amd import omniloc as po
    assert po.pose_covariance_flag(_cfg()) is False
    assert po.pose_covariance_flag(_cfg(pose_covariance=None)) is False
    assert po.pose_covariance_flag(_cfg(pose_covariance=False)) is False
    assert po.pose_covariance_flag(_cfg(pose_covariance=True)) is True
    assert po.pose_covariance_flag(_cfg(pose_covariance=False, depth_mask=True)) is False
    # the prune keys, the robust keys and weights= are allowed next to it
    assert po.pose_covariance_flag(_cfg(pose_covariance=True, prune_iters=10, prune_keep=2, depth_mask=False)) is True
    assert po.pose_covariance_flag(_cfg(pose_covariance=True, robust_iters=[20, 40])) is True


@pytest.mark.parametrize("value", [1, 0, "true", "yes", 1.0, [True], (True,), {"on": True}])
def test_a_value_that_is_not_a_bool_raises(value):
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match=KEY):
        po.pose_covariance_flag(_cfg(pose_covariance=value))


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


def test_omniloc_batch_refuses_before_it_touches_a_device():
    from piccolo_amd import omniloc as po
    run = lambda cfg, rgb=Z, **kw: po.omniloc_batch(IMG, Z, rgb, Z.clone(), Z.clone(), cfg, {}, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="depth_mask"):
        run(_cfg(num_input=4, pose_covariance=True, depth_mask=True))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, pose_covariance=True, depth_mask=True))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, pose_covariance=1))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, pose_covariance="on"))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, pose_covariance=True), rgb=[Z, Z])                 # a cloud of colour sets


@pytest.mark.parametrize("value", [True, False])
def test_entry_points_without_a_covariance_refuse_the_key(value):
    """omniloc, omniloc_all and the images / robust images / rooms / rooms x images entry points raise before they touch a device"""
    from piccolo_amd import omniloc as po
    cfg = _cfg(num_input=4, pose_covariance=value)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc(IMG, Z, Z, Z.clone(), Z.clone(), 0, cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_all(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(num_input=4, robust_iters=20, pose_covariance=value))
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG, IMG], [(Z, Z)], [[Z.clone(), Z.clone()]], [[Z.clone(), Z.clone()]], cfg)


def test_refine_image_non_parallel_branch_refuses_the_key():
    from piccolo_amd import localize
    with pytest.raises(ValueError, match=KEY):
        localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), _cfg(num_input=4, parallel=False, pose_covariance=True))


@pytest.mark.parametrize("kw", [dict(), dict(images_per_launch=4), dict(room_search=True), dict(room_search_images=4),
                                dict(robust_iters=20, robust_images_per_launch=2)])
def test_the_dataset_loops_refuse_at_configuration_time(kw, tmp_path):
    """the dataset loops raise before they read a file (the root does not even exist) or look for a device"""
    from piccolo_amd import localize
    cfg = _cfg(num_input=6, parallel=True, pose_covariance=True, dataset="stanford", **kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=KEY):
        localize.localize_stanford(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_omniscenes(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_synthetic(cfg)
