"""CPU checks of the robust chain's configuration: omniloc.robust_schedule reads the int and list forms of cfg.robust_iters with
cfg.robust_kind / cfg.robust_k and refuses every malformed one, and every entry point and harness path that does not run the robust chain
refuses the keys with a ValueError that names one — before it touches a device."""
import pytest
import torch

from conftest import Cfg


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    return Cfg(**kw)


def test_robust_schedule_int_and_list_forms():
    from piccolo_amd import omniloc as po
    assert po.robust_schedule(_cfg()) is None
    assert po.robust_schedule(_cfg(robust_iters=None, robust_kind=None, robust_k=None)) is None
    assert po.robust_schedule(_cfg(robust_iters=20)) == ([20], "trunc", 2.5)
    assert po.robust_schedule(_cfg(robust_iters=[20])) == ([20], "trunc", 2.5)
    assert po.robust_schedule(_cfg(robust_iters=(20, 40, 99), robust_kind="huber", robust_k=1.345)) == ([20, 40, 99], "huber", 1.345)
    assert po.robust_schedule(_cfg(robust_iters=[1], robust_k=3)) == ([1], "trunc", 3.0)
    assert po.robust_schedule(_cfg(num_iter=12, robust_iters=[4, 8])) == ([4, 8], "trunc", 2.5)
    assert po.robust_schedule(_cfg(robust_iters=5, depth_mask=False, prune_iters=None, prune_keep=None)) == ([5], "trunc", 2.5)


@pytest.mark.parametrize("kw,key", [
    (dict(robust_kind="huber"), "robust_kind"),                         # kind / k without the iterations
    (dict(robust_k=2.0), "robust_k"),
    (dict(robust_iters=[]), "robust_iters"),
    (dict(robust_iters=0), "robust_iters"),                             # outside (0, num_iter)
    (dict(robust_iters=100), "robust_iters"),
    (dict(robust_iters=[20, 120]), "robust_iters"),
    (dict(robust_iters=[40, 20]), "robust_iters"),                      # not increasing
    (dict(robust_iters=[20, 20]), "robust_iters"),                      # not strictly
    (dict(robust_iters=20.0), "robust_iters"),                          # not ints
    (dict(robust_iters=[20, True]), "robust_iters"),
    (dict(robust_iters="20"), "robust_iters"),
    (dict(robust_iters=20, robust_kind="cauchy"), "robust_kind"),
    (dict(robust_iters=20, robust_kind=1), "robust_kind"),
    (dict(robust_iters=20, robust_k=0), "robust_k"),
    (dict(robust_iters=20, robust_k=-2.5), "robust_k"),
    (dict(robust_iters=20, robust_k=float("inf")), "robust_k"),
    (dict(robust_iters=20, robust_k=float("nan")), "robust_k"),
    (dict(robust_iters=20, robust_k="2.5"), "robust_k"),
    (dict(robust_iters=20, robust_k=True), "robust_k"),
    (dict(robust_iters=20, depth_mask=True), "depth_mask"),
    (dict(robust_iters=20, prune_iters=10, prune_keep=2), "prune_iters"),
    (dict(robust_iters=20, prune_keep=2), "prune_iters"),
])
def test_robust_schedule_refuses(kw, key):
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match=key):
        po.robust_schedule(_cfg(**kw))


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


@pytest.mark.parametrize("key,value", [("robust_iters", 20), ("robust_kind", "trunc"), ("robust_k", 2.5)])
def test_entry_points_without_the_robust_chain_refuse_the_keys(key, value):
    """omniloc, omniloc_all and the images / rooms / rooms x images entry points raise before they touch a device"""
    from piccolo_amd import omniloc as po
    cfg = _cfg(num_input=4, **{key: value})
    with pytest.raises(ValueError, match=key):
        po.omniloc(IMG, Z, Z, Z.clone(), Z.clone(), 0, cfg, {})
    with pytest.raises(ValueError, match=key):
        po.omniloc_all(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {})
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)


def test_omniloc_batch_refuses_what_the_robust_chain_does_not_combine_with():
    from piccolo_amd import omniloc as po
    run = lambda cfg, **kw: po.omniloc_batch(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {}, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="weights"):
        run(_cfg(num_input=4, robust_iters=20), weights=torch.ones(4))
    with pytest.raises(ValueError, match="depth_mask"):
        run(_cfg(num_input=4, robust_iters=20, depth_mask=True))
    with pytest.raises(ValueError, match="prune"):
        run(_cfg(num_input=4, robust_iters=20, prune_iters=10, prune_keep=2))
    with pytest.raises(ValueError, match="robust_iters"):
        run(_cfg(num_input=4, robust_iters=100))


def test_refine_image_non_parallel_branch_refuses_the_keys():
    from piccolo_amd import localize
    with pytest.raises(ValueError, match="robust_iters"):
        localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), _cfg(num_input=4, parallel=False, robust_iters=20))


@pytest.mark.parametrize("kw,key", [
    (dict(images_per_launch=4), "images_per_launch"),
    (dict(room_search=True), "room_search"),
    (dict(room_search=["office_1"]), "room_search"),
    (dict(room_search_images=4), "room_search_images"),
    (dict(robust_kind="cauchy"), "robust_kind"),
])
def test_harness_refuses_at_configuration_time(kw, key, tmp_path):
    """the dataset loops raise before they read a file: the root does not even exist"""
    from piccolo_amd import localize
    cfg = _cfg(num_input=6, parallel=True, robust_iters=20, **kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=key):
        localize.localize_stanford(cfg, None, None, root)
    with pytest.raises(ValueError, match=key):
        localize.localize_omniscenes(cfg, None, None, root)
    localize._check_robust_cfg(_cfg(num_input=6, parallel=True, images_per_launch=4, room_search=True))        # no robust key: nothing to refuse
    localize._check_robust_cfg(_cfg(num_input=6, parallel=True, images_per_launch=1, robust_iters=20))
