"""CPU checks of the polished room search: omniloc_batch_rooms_images_polished refuses before it touches a device; the harness key
room_search_polish and its rules, each at configuration time with a root that does not exist; the old refusals of the room-search entry
points and of the loops are intact; the shipped config parses."""
import os

import pytest
import torch

from conftest import REPO, Cfg

Z = torch.zeros(4, 3)
IMG = torch.zeros(8, 16, 3)


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 4)
    return Cfg(**kw)


def _polished(cfg, R=2, I=2, rgb=None, nt=None, nr=None, per_room=None, rows=4):
    from piccolo_amd import omniloc as po
    rooms = [(Z, Z if rgb is None else rgb) for _ in range(R)]
    per_room = I if per_room is None else per_room
    starts = lambda n: [[torch.zeros(rows, 3) for _ in range(per_room)] for _ in range(R if n is None else n)]      # noqa: E731
    return po.omniloc_batch_rooms_images_polished([IMG] * I, rooms, starts(nt), starts(nr), cfg)


def test_the_entry_point_refuses_before_it_touches_a_device():
    with pytest.raises(ValueError, match="gn_iters or cfg.pose_covariance"):
        _polished(_cfg())
    with pytest.raises(ValueError, match="gn_iters or cfg.pose_covariance"):
        _polished(_cfg(pose_covariance=False, prune_iters=None))
    for kw in (dict(gn_iters=3), dict(pose_covariance=True), dict(gn_iters=3, pose_covariance=True)):
        with pytest.raises(ValueError, match="depth_mask"):
            _polished(_cfg(depth_mask=True, **kw))
        with pytest.raises(ValueError, match="visualize"):
            _polished(_cfg(visualize=True, **kw))
        for robust in (dict(robust_iters=20), dict(robust_kind="huber"), dict(robust_k=2.0)):
            with pytest.raises(ValueError, match="does not take cfg.robust_"):
                _polished(_cfg(**kw, **robust))
        # ragged lists
        with pytest.raises(ValueError, match="2 rooms, 2 images, 3 / 2 starting-pose sets"):
            _polished(_cfg(**kw), nt=3)
        with pytest.raises(ValueError, match="2 rooms, 2 images, 2 / 1 starting-pose sets"):
            _polished(_cfg(**kw), nr=1)
        with pytest.raises(ValueError, match="0 rooms"):
            _polished(_cfg(**kw), R=0)
        with pytest.raises(ValueError, match="one starting-pose set per image"):
            _polished(_cfg(**kw), per_room=3)
        with pytest.raises(ValueError, match="3 colour sets for 2 images"):
            _polished(_cfg(**kw), rgb=[Z, Z.clone(), Z.clone()])
    with pytest.raises(ValueError, match="same number of starting poses"):
        from piccolo_amd import omniloc as po
        po.omniloc_batch_rooms_images_polished([IMG], [(Z, Z), (Z, Z)], [[torch.zeros(4, 3)], [torch.zeros(3, 3)]],
                                               [[torch.zeros(4, 3)], [torch.zeros(4, 3)]], _cfg(gn_iters=3))
    # the schedules' own refusals
    with pytest.raises(ValueError, match="gn_"):
        _polished(_cfg(gn_iters=0))
    with pytest.raises(ValueError, match="gn_"):
        _polished(_cfg(gn_step_cap=0.1))
    with pytest.raises(ValueError, match="pose_covariance"):
        _polished(_cfg(pose_covariance=1))
    with pytest.raises(ValueError, match="prune"):
        _polished(_cfg(gn_iters=3, prune_iters=10))
    with pytest.raises(ValueError, match="prune_keep"):
        _polished(_cfg(gn_iters=3, prune_iters=10, prune_keep=5))                      # more than the 4 candidates per (room, image)


def test_the_room_searches_alone_go_on_refusing_the_keys():
    from piccolo_amd import omniloc as po
    for kw in (dict(gn_iters=3), dict(gn_step_cap=0.1), dict(pose_covariance=True), dict(robust_iters=20)):
        with pytest.raises(ValueError, match="omniloc_batch_rooms does not take"):
            po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(**kw))
        with pytest.raises(ValueError, match="omniloc_batch_rooms_images does not take"):
            po.omniloc_batch_rooms_images([IMG, IMG], [(Z, Z)], [[Z.clone(), Z.clone()]], [[Z.clone(), Z.clone()]], _cfg(**kw))
    assert po.ROOMS_POLISHED_ROW == po.POLISHED_ROW + 1 == 53


HARNESS = dict(parallel=True, dataset="stanford", num_input=6)


def test_room_search_polish_rules_at_configuration_time(tmp_path):
    from piccolo_amd import localize
    root = str(tmp_path / "nowhere")
    run = lambda **kw: localize.localize_stanford(_cfg(**dict(HARNESS, **kw)), None, None, root)      # noqa: E731
    # the old refusals are intact: a room search next to the keys, without the new key
    for search in (dict(room_search=True), dict(room_search=["office_1"]), dict(room_search=True, room_search_images=3)):
        with pytest.raises(ValueError, match="does not take cfg.gn_iters"):
            run(gn_iters=3, **search)
        with pytest.raises(ValueError, match="does not take cfg.pose_covariance"):
            run(pose_covariance=True, **search)
        with pytest.raises(ValueError, match="does not take cfg.gn_iters"):
            run(gn_iters=3, room_search_polish=False, **search)
        with pytest.raises(ValueError, match="polish_images_per_launch does not combine"):
            run(gn_iters=3, polish_images_per_launch=2, **search)
    # the new key
    for bad in (1, 0, "True", 2.0, [True]):
        with pytest.raises(ValueError, match="room_search_polish"):
            run(gn_iters=3, room_search=True, room_search_polish=bad)
    with pytest.raises(ValueError, match="goes with cfg.room_search"):
        run(gn_iters=3, room_search_polish=True)
    with pytest.raises(ValueError, match="goes with cfg.room_search"):
        run(gn_iters=3, room_search_polish=True, room_search_images=2)
    with pytest.raises(ValueError, match="goes with cfg.room_search"):
        run(gn_iters=3, room_search_polish=True, polish_images_per_launch=2)
    with pytest.raises(ValueError, match="goes with cfg.gn_iters"):
        run(room_search=True, room_search_polish=True)
    with pytest.raises(ValueError, match="goes with cfg.gn_iters"):
        run(room_search=True, room_search_polish=True, pose_covariance=False)
    with pytest.raises(ValueError, match="needs cfg.parallel"):
        run(gn_iters=3, room_search=True, room_search_polish=True, parallel=False)
    with pytest.raises(ValueError, match="polish_images_per_launch does not combine with cfg.room_search"):
        run(gn_iters=3, room_search=True, room_search_polish=True, polish_images_per_launch=2)
    with pytest.raises(ValueError, match="images_per_launch > 1"):
        run(gn_iters=3, room_search=True, room_search_polish=True, images_per_launch=2)
    with pytest.raises(ValueError, match="robust_"):
        run(gn_iters=3, room_search=True, room_search_polish=True, robust_iters=20)
    # the schedules' own refusals come at configuration time
    with pytest.raises(ValueError, match="depth_mask"):
        run(gn_iters=3, room_search=True, room_search_polish=True, depth_mask=True)
    with pytest.raises(ValueError, match="depth_mask"):
        run(pose_covariance=True, room_search=True, room_search_polish=True, depth_mask=True)
    with pytest.raises(ValueError, match="gn_"):
        run(gn_step_cap=0.1, room_search=True, room_search_polish=True)
    with pytest.raises(ValueError, match="gn_"):
        run(gn_iters=0, room_search=True, room_search_polish=True)
    with pytest.raises(ValueError, match="pose_covariance"):
        run(pose_covariance=1, room_search=True, room_search_polish=True)
    # a well-formed configuration passes every rule and gets as far as the (empty) file listing
    for kw in (dict(gn_iters=3), dict(pose_covariance=True), dict(gn_iters=5, pose_covariance=True, room_search_images=8)):
        assert localize._check_room_polish_cfg(_cfg(**dict(HARNESS, room_search=True, room_search_polish=True, **kw))) is True
    assert localize._check_room_polish_cfg(_cfg(**HARNESS)) is False and localize._check_room_polish_cfg(_cfg(room_search=True, **HARNESS)) is False


def test_the_shipped_room_search_polish_config():
    from piccolo_amd import localize, omniloc as po
    from piccolo_amd.parse_utils import parse_ini
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_room_search_b8_polish.ini"))
    assert po.gn_schedule(cfg) == (5, {}) and po.pose_covariance_flag(cfg) is True
    assert cfg.room_search is True and cfg.room_search_images == 8 and cfg.room_search_polish is True and cfg.parallel is True
    localize._check_robust_cfg(cfg)
    assert localize._check_room_polish_cfg(cfg) is True
    # the b8 room-search config plus the three keys
    plain = parse_ini(os.path.join(REPO, "configs", "stanford_room_search_b8.ini"))
    extra = {k: v for k, v in cfg._asdict().items() if not hasattr(plain, k) or getattr(plain, k) != v}      # (parse_ini gives a namedtuple)
    assert extra == dict(room_search_polish=True, gn_iters=5, pose_covariance=True)
