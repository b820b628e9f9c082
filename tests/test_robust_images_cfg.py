"""CPU checks of the configuration-time rules of the robust chain over several images: omniloc_batch_images_robust needs cfg.robust_iters,
refuses cfg.visualize and whatever robust_schedule refuses, and the harness key cfg.robust_images_per_launch needs cfg.robust_iters and
cfg.parallel — every refusal a ValueError before a device or a file is touched.  The shipped robust config parses to what it says."""
import os

import pytest
import torch

from conftest import REPO, Cfg

IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 4)
    return Cfg(**kw)


def _call(cfg, imgs=2, rgb=None, trans=None, rot=None):
    from piccolo_amd import omniloc as po
    trans = [Z.clone() for _ in range(imgs)] if trans is None else trans
    rot = [Z.clone() for _ in range(imgs)] if rot is None else rot
    return po.omniloc_batch_images_robust([IMG] * imgs, Z, Z if rgb is None else rgb, trans, rot, cfg)


@pytest.mark.parametrize("kw,match", [
    (dict(), "robust_iters"),                                            # the function is the robust chain: it needs the key
    (dict(robust_kind="huber"), "robust_kind"),                          # robust_schedule's rules
    (dict(robust_k=2.0), "robust_k"),
    (dict(robust_iters=100), "robust_iters"),
    (dict(robust_iters=[40, 20]), "robust_iters"),
    (dict(robust_iters=20, robust_kind="cauchy"), "robust_kind"),
    (dict(robust_iters=20, robust_k=0), "robust_k"),
    (dict(robust_iters=20, depth_mask=True), "depth_mask"),              # out of scope, as for one image
    (dict(robust_iters=20, prune_iters=10, prune_keep=2), "prune"),
    (dict(robust_iters=20, visualize=True), "visualize"),
])
def test_the_function_refuses_before_it_touches_a_device(kw, match):
    with pytest.raises(ValueError, match=match):
        _call(_cfg(**kw))


def test_the_function_refuses_mismatched_lists():
    cfg = _cfg(robust_iters=20)
    with pytest.raises(ValueError, match="images"):
        _call(cfg, imgs=2, trans=[Z.clone()])
    with pytest.raises(ValueError, match="images"):
        _call(cfg, imgs=2, rot=[Z.clone()] * 3)
    with pytest.raises(ValueError, match="images"):
        _call(cfg, imgs=0)
    with pytest.raises(ValueError, match="colour sets"):
        _call(cfg, imgs=2, rgb=[Z, Z.clone(), Z.clone()])
    with pytest.raises(ValueError, match="empty"):
        _call(cfg, imgs=2, rgb=[])


def test_the_plain_function_goes_on_refusing_and_names_the_new_one():
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match="omniloc_batch_images_robust"):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(robust_iters=20))


@pytest.mark.parametrize("kw,match", [
    (dict(robust_images_per_launch=4), "robust_iters"),                              # the key without the robust chain
    (dict(robust_images_per_launch=4, robust_iters=20, parallel=False), "parallel"),
    (dict(robust_images_per_launch=0, robust_iters=20), "robust_images_per_launch"),
    (dict(robust_images_per_launch=-2, robust_iters=20), "robust_images_per_launch"),
    (dict(robust_images_per_launch=2.0, robust_iters=20), "robust_images_per_launch"),
    (dict(robust_images_per_launch=True, robust_iters=20), "robust_images_per_launch"),
    (dict(robust_images_per_launch=4, robust_iters=20, images_per_launch=4), "images_per_launch"),      # still refused, and the message names the key
    (dict(robust_images_per_launch=4, robust_iters=20, images_per_launch=4), "robust_images_per_launch"),
    (dict(robust_images_per_launch=4, robust_iters=20, room_search=True), "room_search"),
    (dict(robust_images_per_launch=4, robust_iters=20, room_search_images=4), "room_search_images"),
    (dict(robust_images_per_launch=4, robust_iters=20, robust_kind="cauchy"), "robust_kind"),
])
def test_harness_refuses_at_configuration_time(kw, match, tmp_path):
    """the dataset loops raise before they read a file: the root does not even exist"""
    from piccolo_amd import localize
    kw.setdefault("parallel", True)
    cfg = _cfg(num_input=6, **kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=match):
        localize.localize_stanford(cfg, None, None, root)
    with pytest.raises(ValueError, match=match):
        localize.localize_omniscenes(cfg, None, None, root)


def test_group_size_follows_the_robust_key_only_under_the_robust_chain():
    from piccolo_amd import localize
    assert localize._group_size(_cfg(images_per_launch=8)) == 8
    assert localize._group_size(_cfg()) == 1
    assert localize._group_size(_cfg(robust_iters=20)) == 1
    assert localize._group_size(_cfg(robust_iters=20, images_per_launch=1, robust_images_per_launch=8)) == 8
    assert localize._group_size(_cfg(robust_iters=20, robust_images_per_launch=1)) == 1
    localize._check_robust_cfg(_cfg(parallel=True, robust_iters=20, robust_images_per_launch=8, images_per_launch=1))      # nothing to refuse
    localize._check_robust_cfg(_cfg(parallel=True, images_per_launch=8))


def test_the_shipped_robust_config():
    from piccolo_amd import localize, omniloc as po
    from piccolo_amd.parse_utils import parse_ini
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_robust.ini"))
    base = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))
    assert po.robust_schedule(cfg) == ([20, 40], "trunc", 2.5)
    assert cfg.robust_images_per_launch == 8 and cfg.images_per_launch == 1 and cfg.parallel is True
    localize._check_robust_cfg(cfg)
    assert localize._group_size(cfg) == 8
    extra = {"robust_iters", "robust_images_per_launch", "images_per_launch"}
    d, b = cfg._asdict() if hasattr(cfg, "_asdict") else vars(cfg), base._asdict() if hasattr(base, "_asdict") else vars(base)
    assert set(d) - set(b) == extra and all(d[k] == b[k] for k in b)
