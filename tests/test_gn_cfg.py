"""CPU checks of cfg.gn_iters / gn_step_cap / gn_lambda: omniloc.gn_schedule reads them and refuses everything else and the depth mask next
to them, and every entry point and harness path that polishes nothing refuses the keys with a ValueError that names one — before it
touches a device."""
import pytest
import torch

from conftest import Cfg

KEY = "gn_"


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    return Cfg(**kw)


def test_the_schedule_is_absent_by_default_and_reads_its_keys():
    from piccolo_amd import omniloc as po
    assert po.gn_schedule(_cfg()) is None
    assert po.gn_schedule(_cfg(gn_iters=None, gn_step_cap=None, gn_lambda=None)) is None
    assert po.gn_schedule(_cfg(depth_mask=True)) is None
    assert po.gn_schedule(_cfg(gn_iters=5)) == (5, {})
    assert po.gn_schedule(_cfg(gn_iters=1, gn_step_cap=0.05)) == (1, {"step_cap": 0.05})
    assert po.gn_schedule(_cfg(gn_iters=1000, gn_lambda=1e-2, gn_step_cap=1)) == (1000, {"step_cap": 1.0, "lam0": 1e-2})
    # the prune keys, the robust keys, pose_covariance and weights= are allowed next to them
    assert po.gn_schedule(_cfg(gn_iters=3, prune_iters=10, prune_keep=2, depth_mask=False, pose_covariance=True)) == (3, {})
    assert po.gn_schedule(_cfg(gn_iters=3, robust_iters=[20, 40])) == (3, {})


@pytest.mark.parametrize("kw", [dict(gn_iters=0), dict(gn_iters=-1), dict(gn_iters=1001), dict(gn_iters=True), dict(gn_iters=2.0), dict(gn_iters="5"),
                                dict(gn_iters=[5]), dict(gn_step_cap=0.1), dict(gn_lambda=1e-3), dict(gn_iters=5, gn_step_cap=0.0),
                                dict(gn_iters=5, gn_step_cap=-0.1), dict(gn_iters=5, gn_step_cap=float("inf")), dict(gn_iters=5, gn_step_cap=float("nan")),
                                dict(gn_iters=5, gn_step_cap="0.1"), dict(gn_iters=5, gn_step_cap=True), dict(gn_iters=5, gn_lambda=0),
                                dict(gn_iters=5, gn_lambda=-1.0), dict(gn_iters=5, gn_lambda=float("nan")), dict(gn_iters=5, gn_lambda=[1e-3]),
                                dict(gn_iters=5, gn_lambda=1e-60), dict(gn_iters=5, gn_step_cap=1e60), dict(gn_iters=5, depth_mask=True)])
def test_the_schedule_refuses(kw):
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match=KEY):
        po.gn_schedule(_cfg(**kw))


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


def test_omniloc_batch_refuses_before_it_touches_a_device():
    from piccolo_amd import omniloc as po
    run = lambda cfg, rgb=Z, **kw: po.omniloc_batch(IMG, Z, rgb, Z.clone(), Z.clone(), cfg, {}, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="depth_mask"):
        run(_cfg(num_input=4, gn_iters=3, depth_mask=True))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, gn_iters=0))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, gn_step_cap=0.1))
    with pytest.raises(ValueError, match=KEY):
        run(_cfg(num_input=4, gn_iters=3), rgb=[Z, Z])                           # a cloud of colour sets


@pytest.mark.parametrize("kw", [dict(gn_iters=3), dict(gn_step_cap=0.1), dict(gn_lambda=1e-3), dict(gn_iters=3, gn_step_cap=0.1, gn_lambda=1e-3)])
def test_entry_points_without_a_polish_refuse_the_keys(kw):
    """omniloc, omniloc_all and the images / robust images / rooms / rooms x images entry points raise before they touch a device"""
    from piccolo_amd import omniloc as po
    cfg = _cfg(num_input=4, **kw)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc(IMG, Z, Z, Z.clone(), Z.clone(), 0, cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_all(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(num_input=4, depth_mask=True, **kw))
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(num_input=4, robust_iters=20, **kw))
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG, IMG], [(Z, Z)], [[Z.clone(), Z.clone()]], [[Z.clone(), Z.clone()]], cfg)


def test_refine_image_non_parallel_branch_refuses_the_keys():
    from piccolo_amd import localize
    with pytest.raises(ValueError, match=KEY):
        localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), _cfg(num_input=4, parallel=False, gn_iters=3))
    with pytest.raises(ValueError, match="depth_mask"):                           # the parallel branch passes them on: gn_schedule's refusal
        localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), _cfg(num_input=4, parallel=True, gn_iters=3, depth_mask=True))


@pytest.mark.parametrize("kw", [dict(), dict(images_per_launch=4), dict(room_search=True), dict(room_search_images=4),
                                dict(robust_iters=20, robust_images_per_launch=2)])
def test_the_dataset_loops_refuse_at_configuration_time(kw, tmp_path):
    """the dataset loops raise before they read a file (the root does not even exist) or look for a device"""
    from piccolo_amd import localize
    cfg = _cfg(num_input=6, parallel=True, gn_iters=3, dataset="stanford", **kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=KEY):
        localize.localize_stanford(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_omniscenes(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_synthetic(cfg)


def test_the_ops_layer_refuses_bad_hyper_parameters_before_a_device_call():
    from piccolo_amd import ops
    for kw in (dict(lam0=0.0), dict(lam_up=1.0), dict(lam_down=0.0), dict(lam_down=1.5), dict(lam_min=2.0, lam_max=1.0), dict(step_cap=0.0),
               dict(tol=-1.0), dict(step_cap=float("nan")), dict(lam_max=float("inf")), dict(damping=1.0), dict(tol=True)):
        with pytest.raises(ValueError):
            ops.gn_hyper(**kw)
    h = ops.gn_hyper()
    assert (h.lam0, h.step_cap, h.tol) == (pytest.approx(1e-3), pytest.approx(0.1), 0.0)
    assert ops.gn_hyper(tol=1e-4, step_cap=0.5).step_cap == 0.5
