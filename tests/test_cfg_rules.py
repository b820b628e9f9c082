"""CPU pin of the extension keys' rules (piccolo_amd/cfg_rules.py): a deterministic grid of cfg dicts against outcomes recorded at the commit
before the rules got one home (tests/golden/cfg_refusals.json holds the outcomes alone; the grid is built here).

Plan section, PLAN_CASES = 335 cfgs, each for both dataset loops (670 outcomes): every family of keys absent, with each valid and each
invalid value; every pair of families; each family against each grouping setting x parallel x depth_mask; a few routes that need three
things at once.  An outcome is the exact ValueError message, or the fields of dataset_plan's DatasetPlan.
Entry section, ENTRY_CASES = 53 cfgs (the single-family and family-pair ones) for each of the 10 entry points and for prune_schedule at 4
candidates per image (583 calls): a call is recorded only where that commit raised ValueError before it touched a device, and the same
message is demanded again; ENTRY_LEFT_OUT = 169 calls are left out — 124 that an entry point did not refuse, which went on to the device,
and 45 cfgs whose prune_schedule is valid or absent.  Nothing here needs a device."""
import itertools
import json
import os

import pytest
import torch

from conftest import REPO, Cfg

BASE = dict(num_iter=100, num_input=4, parallel=True, dataset="stanford", num_points=64, num_images=1)
# family -> (valid settings, the first the one the crossings use; one invalid setting per rule its schedule states)
FAMILIES = {
    "prune": ([dict(prune_iters=20, prune_keep=2), dict(prune_iters=[20, 40], prune_keep=[3, 2])],
              [dict(prune_iters=20), dict(prune_keep=2), dict(prune_iters=2.5, prune_keep=2), dict(prune_iters=[10, 20], prune_keep=[2]),
               dict(prune_iters=100, prune_keep=2), dict(prune_iters=20, prune_keep=0), dict(prune_iters=[20, 40], prune_keep=[2, 3]),
               dict(prune_iters=20, prune_keep=5)]),
    "robust": ([dict(robust_iters=20), dict(robust_iters=[20, 40], robust_kind="huber", robust_k=1.5)],
               [dict(robust_kind="huber"), dict(robust_k=2.0), dict(robust_iters=20.0), dict(robust_iters=100), dict(robust_iters=[40, 20]),
                dict(robust_iters=20, robust_kind="cauchy"), dict(robust_iters=20, robust_k=0)]),
    "pose_covariance": ([dict(pose_covariance=True), dict(pose_covariance=False)], [dict(pose_covariance=1)]),
    "gn": ([dict(gn_iters=5), dict(gn_iters=5, gn_step_cap=0.1, gn_lambda=1e-3), dict(gn_iters=5, gn_objective="l1", gn_delta=0.01)],
           [dict(gn_iters=5, gn_objective="l3"), dict(gn_step_cap=0.1), dict(gn_objective="l1"), dict(gn_iters=5, gn_delta=0.01),
            dict(gn_iters=5, gn_objective="l1", gn_delta=0), dict(gn_iters=5, gn_objective="l1", gn_delta=1e-9), dict(gn_iters=0),
            dict(gn_iters=5, gn_step_cap=0), dict(gn_iters=5, gn_lambda=1e-60)]),
    "score": ([dict(score_weights=True), dict(score_weights=True, score_split=[16, 32], score_floor=0.25, score_min_count=5),
               dict(score_weights=False)],
              [dict(score_split=[16, 32]), dict(score_weights=1), dict(score_weights=True, score_split=[2, 32]),
               dict(score_weights=True, score_floor=1.0), dict(score_weights=True, score_min_count=0)]),
}
GROUPINGS = [dict(images_per_launch=1), dict(images_per_launch=4), dict(robust_images_per_launch=4), dict(polish_images_per_launch=4),
             dict(room_search=True), dict(room_search=["office_1", "hallway_2"]), dict(room_search_images=4), dict(room_search_polish=True),
             dict(room_search=True, room_search_images=4), dict(room_search=True, room_search_polish=True),
             dict(room_search=True, room_search_images=4, room_search_polish=True)]
BAD_GROUPINGS = [dict(robust_iters=20, robust_images_per_launch=0), dict(gn_iters=5, polish_images_per_launch=0),
                 dict(gn_iters=5, polish_images_per_launch=True), dict(gn_iters=5, room_search=True, room_search_polish=1),
                 dict(room_search=True, images_per_launch=4), dict(room_search=["office_1"], room_search_images=4, images_per_launch=4)]
# routes that need three things at once: a robust polished run, the covariance next to the polish, a polished search of several images
ROUTES = [dict(robust_iters=20, gn_iters=5, polish_images_per_launch=4), dict(gn_iters=5, pose_covariance=True, polish_images_per_launch=4),
          dict(prune_iters=20, prune_keep=2, pose_covariance=True, polish_images_per_launch=1),
          dict(gn_iters=5, pose_covariance=True, room_search=True, room_search_images=4, room_search_polish=True),
          dict(gn_iters=5, gn_objective="l1", room_search=True, room_search_polish=True),
          dict(robust_iters=20, robust_images_per_launch=4, polish_images_per_launch=4, gn_iters=5)]


def entry_cases():
    """every family absent, with each valid and each invalid value; every pair of families (their first valid values)"""
    cases = [{}] + [kw for ok, bad in FAMILIES.values() for kw in ok + bad]
    return cases + [dict(FAMILIES[a][0][0], **FAMILIES[b][0][0]) for a, b in itertools.combinations(FAMILIES, 2)]


def plan_cases():
    """entry_cases, then every family (absent too) x grouping x parallel x depth_mask, the malformed grouping keys and ROUTES"""
    firsts = [{}] + [ok[0] for ok, _ in FAMILIES.values()]
    crossed = [dict(family, parallel=parallel, depth_mask=mask, **grouping)
               for family in firsts for grouping in GROUPINGS for parallel in (True, False) for mask in (True, False)]
    return entry_cases() + crossed + BAD_GROUPINGS + ROUTES + [dict(kw, parallel=False) for kw in ROUTES]


def cfg_of(kw):
    return Cfg(**dict(BASE, **kw))


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


def _two():
    return [Z.clone(), Z.clone()]


def entry_points():
    """name -> call(cfg), with the dummy tensors of the *_cfg tests: a refusal comes before any of them is looked at"""
    from piccolo_amd import localize, omniloc as po
    return {
        "omniloc": lambda cfg: po.omniloc(IMG, Z, Z, Z.clone(), Z.clone(), 0, cfg, {}),
        "omniloc_all": lambda cfg: po.omniloc_all(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {}),
        "omniloc_batch": lambda cfg: po.omniloc_batch(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {}),
        "omniloc_batch_images": lambda cfg: po.omniloc_batch_images([IMG, IMG], Z, Z, _two(), _two(), cfg),
        "omniloc_batch_images_robust": lambda cfg: po.omniloc_batch_images_robust([IMG, IMG], Z, Z, _two(), _two(), cfg),
        "omniloc_batch_images_polished": lambda cfg: po.omniloc_batch_images_polished([IMG, IMG], Z, Z, _two(), _two(), cfg),
        "omniloc_batch_rooms": lambda cfg: po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], _two(), _two(), cfg),
        "omniloc_batch_rooms_images": lambda cfg: po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg),
        "omniloc_batch_rooms_images_polished": lambda cfg: po.omniloc_batch_rooms_images_polished([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg),
        "localize_synthetic": lambda cfg: localize.localize_synthetic(cfg),
        "prune_schedule": lambda cfg: po.prune_schedule(cfg, 4),          # (no entry point: the schedule the batch refinements read, host only)
    }


ENTRY_POINTS = ("omniloc", "omniloc_all", "omniloc_batch", "omniloc_batch_images", "omniloc_batch_images_robust", "omniloc_batch_images_polished",
                "omniloc_batch_rooms", "omniloc_batch_rooms_images", "omniloc_batch_rooms_images_polished", "localize_synthetic", "prune_schedule")
LOOPS = ("localize_stanford", "localize_omniscenes")
PLAN_CASES, ENTRY_CASES, ENTRY_LEFT_OUT = 335, 53, 169


@pytest.fixture(scope="module")
def recorded():
    """{"messages": [...], "plan": {loop: [outcome, ...]}, "entry": {entry point: [outcome, ...]}}, an outcome an index into messages, the
    plan's fields as a list, or None (left out) -> the same with every index replaced by its message"""
    with open(os.path.join(REPO, "tests", "golden", "cfg_refusals.json")) as f:
        rec = json.load(f)
    text = lambda o: rec["messages"][o] if isinstance(o, int) else o      # noqa: E731
    return {part: {who: [text(o) for o in outcomes] for who, outcomes in rec[part].items()} for part in ("plan", "entry")}


def test_the_grid_is_the_recorded_one(recorded):
    assert len(plan_cases()) == PLAN_CASES and len(entry_cases()) == ENTRY_CASES and tuple(entry_points()) == ENTRY_POINTS
    assert set(recorded["plan"]) == set(LOOPS) and all(len(recorded["plan"][loop]) == PLAN_CASES for loop in LOOPS)
    assert set(recorded["entry"]) == set(ENTRY_POINTS) and all(len(recorded["entry"][who]) == ENTRY_CASES for who in ENTRY_POINTS)
    assert sum(msg is None for who in ENTRY_POINTS for msg in recorded["entry"][who]) == ENTRY_LEFT_OUT
    # both kinds of outcome occur for both loops, and every route is taken somewhere
    for loop in LOOPS:
        assert any(isinstance(o, str) for o in recorded["plan"][loop]) and any(isinstance(o, list) for o in recorded["plan"][loop])
    routes = {o[0] for o in recorded["plan"]["localize_stanford"] if isinstance(o, list)}
    assert routes == {"plain", "robust", "polished", "scored", "rooms", "rooms-polished"}


@pytest.mark.parametrize("loop", LOOPS)
def test_dataset_plan_gives_the_recorded_outcome(recorded, loop):
    """the message where the loop refused the cfg at configuration time, else the plan: route, group size, parallel, score triple,
    room-search value, sigma columns"""
    from piccolo_amd import cfg_rules
    assert cfg_rules.DatasetPlan._fields == ("route", "group_size", "parallel", "score", "room_search", "sigmas")
    wrong = []
    for n, (kw, want) in enumerate(zip(plan_cases(), recorded["plan"][loop])):
        try:
            got = json.loads(json.dumps(list(cfg_rules.dataset_plan(cfg_of(kw), loop))))
        except ValueError as e:
            got = str(e)
        if got != want:
            wrong.append((n, kw, got, want))
    assert not wrong, wrong[:5]


@pytest.mark.parametrize("loop", LOOPS)
def test_the_loops_raise_the_plan_s_refusals_before_they_read_a_file(recorded, loop, tmp_path):
    """the loop itself, with a root that does not exist, on the entry cases: the recorded message where there is one"""
    from piccolo_amd import localize
    root = str(tmp_path / "nowhere")
    for kw, want in zip(entry_cases(), recorded["plan"][loop]):
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                getattr(localize, loop)(cfg_of(kw), None, None, root)
            assert str(e.value) == want, kw
    assert not os.path.exists(root)


@pytest.mark.parametrize("who", ENTRY_POINTS)
def test_the_entry_points_refuse_what_they_refused(recorded, who):
    call = entry_points()[who]
    refused = [(kw, want) for kw, want in zip(entry_cases(), recorded["entry"][who]) if want is not None]
    assert refused
    for kw, want in refused:
        with pytest.raises(ValueError) as e:
            call(cfg_of(kw))
        assert str(e.value) == want, kw
