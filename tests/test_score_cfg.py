"""CPU checks of the score-weight configuration: localize._check_score_cfg reads cfg.score_weights / score_split / score_floor /
score_min_count and refuses every malformed key and every combination the scored known-room path does not run, the dataset loops raise
before they read a file, the entry points that do not take the keys refuse them, and the shipped config is the b32 one plus the stated keys."""
import os

import pytest
import torch

from conftest import REPO, Cfg


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 6)
    kw.setdefault("parallel", True)
    return Cfg(**kw)


def test_check_score_cfg_reads_the_keys():
    from piccolo_amd import localize
    assert localize._check_score_cfg(_cfg()) is None
    assert localize._check_score_cfg(_cfg(score_weights=None, score_split=None, score_floor=None, score_min_count=None)) is None
    assert localize._check_score_cfg(_cfg(score_weights=False)) is None
    assert localize._check_score_cfg(_cfg(score_weights=True)) == (None, 0.0, 1)
    assert localize._check_score_cfg(_cfg(score_weights=True, score_split=[16, 32], score_floor=0.25, score_min_count=5)) == ((16, 32), 0.25, 5)
    assert localize._check_score_cfg(_cfg(score_weights=True, score_split=(3, 1), score_floor=0, images_per_launch=1, depth_mask=False,
                                          room_search=None, parallel=False)) == ((3, 1), 0.0, 1)


BAD = [
    (dict(score_split=[16, 32]), "score_split"),                         # the other keys without score_weights = True
    (dict(score_floor=0.5), "score_floor"),
    (dict(score_min_count=2), "score_min_count"),
    (dict(score_weights=False, score_floor=0.5), "score_floor"),
    (dict(score_weights=1), "score_weights"),                            # malformed
    (dict(score_weights="True"), "score_weights"),
    (dict(score_weights=True, score_split=16), "score_split"),
    (dict(score_weights=True, score_split=[16]), "score_split"),
    (dict(score_weights=True, score_split=[16, 32, 2]), "score_split"),
    (dict(score_weights=True, score_split=[2, 32]), "score_split"),
    (dict(score_weights=True, score_split=[16, 0]), "score_split"),
    (dict(score_weights=True, score_split=[16.0, 32]), "score_split"),
    (dict(score_weights=True, score_split=[True, 32]), "score_split"),
    (dict(score_weights=True, score_floor=1.0), "score_floor"),
    (dict(score_weights=True, score_floor=-0.1), "score_floor"),
    (dict(score_weights=True, score_floor=float("nan")), "score_floor"),
    (dict(score_weights=True, score_floor="0.5"), "score_floor"),
    (dict(score_weights=True, score_floor=True), "score_floor"),
    (dict(score_weights=True, score_min_count=0), "score_min_count"),
    (dict(score_weights=True, score_min_count=2.0), "score_min_count"),
    (dict(score_weights=True, score_min_count=True), "score_min_count"),
    (dict(score_weights=True, images_per_launch=4), "images_per_launch"),        # what the scored path does not combine with
    (dict(score_weights=True, robust_iters=20), "robust_iters"),
    (dict(score_weights=True, robust_kind="huber"), "robust_kind"),
    (dict(score_weights=True, robust_k=2.5), "robust_k"),
    (dict(score_weights=True, robust_iters=20, robust_images_per_launch=4), "robust"),
    (dict(score_weights=True, robust_images_per_launch=4), "robust_images_per_launch"),
    (dict(score_weights=True, gn_iters=5, polish_images_per_launch=4), "polish_images_per_launch"),
    (dict(score_weights=True, room_search=True), "room_search"),
    (dict(score_weights=True, room_search=["office_1"]), "room_search"),
    (dict(score_weights=True, room_search_images=4), "room_search_images"),
    (dict(score_weights=True, depth_mask=True), "depth_mask"),
]


@pytest.mark.parametrize("kw,key", BAD)
def test_harness_refuses_at_configuration_time(kw, key, tmp_path):
    """the dataset loops raise before they read a file: the root does not even exist"""
    from piccolo_amd import localize
    cfg = _cfg(**kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=key):
        localize._check_score_cfg(cfg)
    for loop in (localize.localize_stanford, localize.localize_omniscenes):
        with pytest.raises(ValueError, match=key):
            loop(cfg, None, None, root)
    assert not os.path.exists(root)


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


@pytest.mark.parametrize("key,value", [("score_weights", True), ("score_split", [16, 32]), ("score_floor", 0.25), ("score_min_count", 2)])
def test_entry_points_that_do_not_take_the_keys_refuse_them(key, value):
    """the several-image and rooms entry points and the synthetic driver raise before they touch a device"""
    from piccolo_amd import localize, omniloc as po
    assert po._EXTENSIONS["score"][0] == po.SCORE_KEYS == ("score_weights", "score_split", "score_floor", "score_min_count")
    cfg = _cfg(num_input=4, **{key: value})
    two = [Z.clone(), Z.clone()]
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images([IMG, IMG], Z, Z, two, two, cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, two, two, _cfg(num_input=4, robust_iters=20, **{key: value}))
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_images_polished([IMG, IMG], Z, Z, two, two, _cfg(num_input=4, gn_iters=5, **{key: value}))
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], two, two, cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)
    with pytest.raises(ValueError, match=key):
        po.omniloc_batch_rooms_images_polished([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], _cfg(num_input=4, gn_iters=5, **{key: value}))
    with pytest.raises(ValueError, match=key):
        localize.localize_synthetic(cfg)


def test_without_the_keys_nothing_is_refused():
    from piccolo_amd import omniloc as po
    po._refuse(_cfg(), "anything", "score")
    po._refuse(_cfg(score_weights=None, score_split=None), "anything", "score")


def test_shipped_config_is_b32_plus_the_stated_keys():
    from piccolo_amd import localize
    from piccolo_amd.parse_utils import parse_ini
    b32 = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32.ini"))._asdict()
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b32_score.ini"))
    got = cfg._asdict()
    extra = {k: v for k, v in got.items() if k not in b32}
    assert extra == dict(score_weights=True, score_split=[16, 32], images_per_launch=1)
    assert {k: v for k, v in got.items() if k in b32} == b32
    assert localize._check_score_cfg(cfg) == ((16, 32), 0.0, 1)
    assert cfg.lr == 0.1 and cfg.num_iter == 100 and cfg.patience == 5 and cfg.factor == 0.8
