"""CPU checks of the polished chain over several query images: omniloc_batch_images_polished refuses before it touches a device; the harness
key polish_images_per_launch and its rules, each at configuration time with a root that does not exist; the CSV's sigma columns with and
without cfg.pose_covariance, through the one driver on a canned dataset."""
import csv

import numpy as np
import pytest
import torch

from conftest import Cfg

Z = torch.zeros(4, 3)
IMG = torch.zeros(8, 16, 3)


def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    kw.setdefault("num_input", 4)
    return Cfg(**kw)


def _polished(cfg, imgs=(IMG, IMG), rgb=Z, nt=2, nr=2):
    from piccolo_amd import omniloc as po
    return po.omniloc_batch_images_polished(list(imgs), Z, rgb, [Z.clone() for _ in range(nt)], [Z.clone() for _ in range(nr)], cfg)


def test_the_entry_point_refuses_before_it_touches_a_device():
    with pytest.raises(ValueError, match="gn_iters or cfg.pose_covariance"):
        _polished(_cfg())
    with pytest.raises(ValueError, match="gn_iters or cfg.pose_covariance"):
        _polished(_cfg(robust_iters=20, prune_iters=None))
    with pytest.raises(ValueError, match="gn_iters or cfg.pose_covariance"):
        _polished(_cfg(pose_covariance=False))
    for kw in (dict(gn_iters=3), dict(pose_covariance=True), dict(gn_iters=3, pose_covariance=True)):
        with pytest.raises(ValueError, match="depth_mask"):
            _polished(_cfg(depth_mask=True, **kw))
        with pytest.raises(ValueError, match="visualize"):
            _polished(_cfg(visualize=True, **kw))
        with pytest.raises(ValueError, match="2 images, 3 / 2 lists"):
            _polished(_cfg(**kw), nt=3)
        with pytest.raises(ValueError, match="2 images, 2 / 1 lists"):
            _polished(_cfg(**kw), nr=1)
        with pytest.raises(ValueError, match="0 images"):
            _polished(_cfg(**kw), imgs=(), nt=0, nr=0)
        with pytest.raises(ValueError, match="3 colour sets for 2 images"):
            _polished(_cfg(**kw), rgb=[Z, Z.clone(), Z.clone()])
    # the schedules' own refusals
    with pytest.raises(ValueError, match="gn_"):
        _polished(_cfg(gn_iters=0))
    with pytest.raises(ValueError, match="gn_"):
        _polished(_cfg(gn_step_cap=0.1))
    with pytest.raises(ValueError, match="pose_covariance"):
        _polished(_cfg(pose_covariance=1))
    with pytest.raises(ValueError, match="robust_"):
        _polished(_cfg(gn_iters=3, robust_kind="huber"))
    with pytest.raises(ValueError, match="prune"):
        _polished(_cfg(gn_iters=3, robust_iters=20, prune_iters=10, prune_keep=2))
    with pytest.raises(ValueError, match="prune"):
        _polished(_cfg(gn_iters=3, prune_iters=10))
    with pytest.raises(ValueError, match="prune_keep"):
        _polished(_cfg(gn_iters=3, prune_iters=10, prune_keep=5))                      # more than the 4 candidates per image


def test_the_plain_chain_refuses_ragged_lists_before_it_touches_a_device():
    """omniloc_batch_images checks its lists as the robust and polished forms do, with their messages"""
    from piccolo_amd import omniloc as po
    for batch_mode in (True, False):
        with pytest.raises(ValueError, match="omniloc_batch_images: 2 images, 3 / 2 lists of starting poses"):
            po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone() for _ in range(3)], [Z.clone(), Z.clone()], _cfg(), batch_mode=batch_mode)
        with pytest.raises(ValueError, match="omniloc_batch_images: 2 images, 2 / 1 lists of starting poses"):
            po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone()], _cfg(), batch_mode=batch_mode)
        with pytest.raises(ValueError, match="omniloc_batch_images: 0 images"):
            po.omniloc_batch_images([], Z, Z, [], [], _cfg(), batch_mode=batch_mode)
        with pytest.raises(ValueError, match="omniloc_batch_images: 3 colour sets for 2 images"):
            po.omniloc_batch_images([IMG, IMG], Z, [Z, Z.clone(), Z.clone()], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(),
                                    batch_mode=batch_mode)
    with pytest.raises(ValueError, match="omniloc_batch_images_robust: 2 images, 3 / 2 lists of starting poses"):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, [Z.clone() for _ in range(3)], [Z.clone(), Z.clone()], _cfg(robust_iters=20))


def test_the_chains_alone_go_on_refusing_the_keys():
    from piccolo_amd import omniloc as po
    two = ([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()])
    for kw in (dict(gn_iters=3), dict(pose_covariance=True)):
        with pytest.raises(ValueError, match="omniloc_batch_images_polished"):
            po.omniloc_batch_images(*two, _cfg(**kw))
        with pytest.raises(ValueError, match="omniloc_batch_images_polished"):
            po.omniloc_batch_images_robust(*two, _cfg(robust_iters=20, **kw))
    takers = {name: po._EXTENSIONS[name][2] for name in ("robust", "pose_covariance", "gn")}
    assert all("omniloc_batch_images_polished" in s for s in takers.values())
    assert "polish_images_per_launch" in takers["gn"] and "polish_images_per_launch" in takers["pose_covariance"]


def test_the_wrappers_refuse_before_they_touch_a_device():
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match="3 colour sets for 2 images"):
        po.pose_information_images([IMG, IMG], Z, [Z, Z.clone(), Z.clone()], Z[:2], Z[:2])
    with pytest.raises(ValueError, match="weights"):
        po.gauss_newton_refine_images([IMG, IMG], Z, [Z, Z.clone()], Z[:2], Z[:2], weights=torch.ones(4))


HARNESS = dict(parallel=True, dataset="stanford", num_input=6)


@pytest.mark.parametrize("loop", ["localize_stanford", "localize_omniscenes"])
def test_polish_images_per_launch_rules_at_configuration_time(tmp_path, loop):
    from piccolo_amd import localize
    root = str(tmp_path / "nowhere")
    run = lambda **kw: getattr(localize, loop)(_cfg(**dict(HARNESS, **kw)), None, None, root)      # noqa: E731
    for bad in (0, -1, True, 2.0, "3", [3]):
        with pytest.raises(ValueError, match="polish_images_per_launch"):
            run(gn_iters=3, polish_images_per_launch=bad)
    with pytest.raises(ValueError, match="needs cfg.parallel"):
        run(gn_iters=3, polish_images_per_launch=2, parallel=False)
    with pytest.raises(ValueError, match="goes with cfg.gn_iters"):
        run(polish_images_per_launch=2)
    with pytest.raises(ValueError, match="goes with cfg.gn_iters"):
        run(polish_images_per_launch=2, pose_covariance=False, robust_iters=20)
    for kw in (dict(room_search=True), dict(room_search=["office_1"]), dict(room_search_images=2), dict(robust_images_per_launch=2, robust_iters=20)):
        with pytest.raises(ValueError, match="polish_images_per_launch does not combine|robust_"):
            run(gn_iters=3, polish_images_per_launch=2, **kw)
    with pytest.raises(ValueError, match="images_per_launch > 1"):
        run(pose_covariance=True, polish_images_per_launch=2, images_per_launch=2)
    # the schedules' own refusals come at configuration time too
    with pytest.raises(ValueError, match="depth_mask"):
        run(gn_iters=3, polish_images_per_launch=2, depth_mask=True)
    with pytest.raises(ValueError, match="depth_mask"):
        run(pose_covariance=True, polish_images_per_launch=1, depth_mask=True)
    with pytest.raises(ValueError, match="gn_"):
        run(gn_step_cap=0.1, polish_images_per_launch=2)
    with pytest.raises(ValueError, match="gn_"):
        run(gn_iters=0, polish_images_per_launch=2)
    # without the key the loops refuse the keys as they always did
    with pytest.raises(ValueError, match="does not take cfg.gn_iters"):
        run(gn_iters=3)
    with pytest.raises(ValueError, match="does not take cfg.pose_covariance"):
        run(pose_covariance=True)


def test_localize_synthetic_goes_on_refusing():
    from piccolo_amd import localize
    with pytest.raises(ValueError, match="gn_"):
        localize.localize_synthetic(_cfg(gn_iters=3, polish_images_per_launch=2, **HARNESS))
    with pytest.raises(ValueError, match="pose_covariance"):
        localize.localize_synthetic(_cfg(pose_covariance=True, polish_images_per_launch=2, **HARNESS))


def test_group_size_and_sigmas():
    from piccolo_amd import localize
    assert localize._group_size(_cfg(gn_iters=3, polish_images_per_launch=5)) == 5
    assert localize._group_size(_cfg(gn_iters=3, robust_iters=20, polish_images_per_launch=3)) == 3      # a robust polished run
    assert localize._group_size(_cfg(robust_iters=20, robust_images_per_launch=4)) == 4 and localize._group_size(_cfg(images_per_launch=7)) == 7
    cov = np.diag([1e-4, 4e-4, 4e-4, 1e-6, 1e-6, 2e-6]).astype(np.float32)
    st, sr = localize.pose_sigmas(cov)
    assert st == pytest.approx(0.03, rel=1e-6) and sr == pytest.approx(np.degrees(0.002), rel=1e-6)
    assert all(np.isnan(v) for v in localize.pose_sigmas(np.full((6, 6), np.nan, np.float32)))


def test_the_shipped_polish_config():
    import os
    from conftest import REPO
    from piccolo_amd import localize, omniloc as po
    from piccolo_amd.parse_utils import parse_ini
    cfg = parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b8_polish.ini"))
    assert po.gn_schedule(cfg) == (5, {}) and po.pose_covariance_flag(cfg) is True
    assert cfg.polish_images_per_launch == 8 and cfg.images_per_launch == 1 and cfg.parallel is True
    assert cfg.num_input == 6 and cfg.sample_rate == 6                    # the shipped parallel shape
    localize._check_robust_cfg(cfg)
    assert localize._check_polish_cfg(cfg, "localize_stanford") == 8 and localize._group_size(cfg) == 8


class _FakeJob:
    def __init__(self, k):
        self.k, self.group_key = k, "a"


@pytest.mark.parametrize("want_cov", [True, False])
def test_the_csv_header_with_and_without_pose_covariance(tmp_path, want_cov):
    """the known-room driver on a canned dataset: 5 images, image 1 skipped, image 3's covariance NaN"""
    from piccolo_amd import localize
    n, header = 5, ["pano_name", "gt_trans", "gt_rot", "skipped?", "t", "R", "t_err", "r_err", "time (s)"]
    files = ["a/f%d.png" % k for k in range(n)]
    covs = {k: torch.eye(6) * (k + 1) * 1e-4 if k != 3 else torch.full((6, 6), float("nan")) for k in range(n)}
    groups, reported = [], []

    def localize_group(jobs):
        groups.append([j.k for j in jobs])
        return [(torch.full((3, 1), float(j.k)), torch.eye(3), torch.tensor(0.5)) + ((covs[j.k],) if want_cov else ()) for j in jobs]
    dataset = localize._Dataset(lambda k: (np.full(3, k, np.float32), np.eye(3, dtype=np.float32), k == 1), lambda k: _FakeJob(k), localize_group,
                                lambda k, job, result, row: reported.append(k))
    cfg = _cfg(gn_iters=3, polish_images_per_launch=2, **HARNESS, **({"pose_covariance": True} if want_cov else {}))
    plan = localize.dataset_plan(cfg, "localize_stanford")
    assert plan.route == "polished" and plan.group_size == 2 and plan.sigmas is want_cov
    table = localize._run_known_room(plan, None, str(tmp_path), files, dataset, "fake.csv", header, lambda f: [f], localize.stanford_success)
    assert groups == [[0, 2], [3, 4]] and reported == [0, 2, 3, 4] and tuple(table.shape) == (n, 16)
    with open(tmp_path / "fake.csv") as f:
        rows = list(csv.reader(f))
    if not want_cov:
        assert rows[0] == header and all(len(r) <= len(header) for r in rows)
        return
    assert rows[0] == header + ["sigma_t (m)", "sigma_r (degrees)"] == header + localize.SIGMA_HEADER
    assert len(rows[2]) == 4                                              # the skipped image's short row, as ever
    for k in (0, 2, 4):
        st, sr = localize.pose_sigmas(covs[k].numpy())
        assert len(rows[k + 1]) == len(header) + 2
        assert float(rows[k + 1][-2]) == np.float32(st) and float(rows[k + 1][-1]) == np.float32(sr)
    assert rows[4][-2:] == ["", ""]                                       # NaN covariance: both empty
