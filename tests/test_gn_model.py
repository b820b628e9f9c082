"""The float64 model of the Levenberg-Marquardt pose polish (tests/gn_helpers.py), on the CPU: on the four cases of
info_helpers.CASES from both scene poses the accepted F never rises, the counters add up and the returned pose is the best trial; the
trace checks the GPU test applies to the device pass on the model's own trace and catch every planted mistake of the model; and the
free-run yardstick of the GPU test is finite and kept by the model itself for every start chosen."""
import numpy as np
import pytest

import gn_helpers as gn
import grad_helpers as gh
import info_helpers as ih

# which (configuration, case, pose) catches which planted variant (asserted below); the configurations are those the GPU trace test runs
CATCHERS = {
    "step_sign": [("default", "G2", 0), ("default", "tall", 1), ("tiny_cap", "odd", 0)],
    "lam_identity": [("default", "G2", 0), ("default", "odd", 1), ("default", "tiny", 0), ("default", "tall", 1)],
    "accept_le": [("tiny_cap", "tiny", 0), ("tiny_cap", "tiny", 1)],
    "lam_not_raised": [("tiny_cap", "tiny", 0), ("gentle", "tall", 0)],
    "lam_down_at_0": [("default", "G2", 1), ("gentle", "tall", 0), ("tiny_cap", "odd", 1)],
    "cap_per_component": [("tiny_cap", "G2", 0), ("tiny_cap", "tall", 1), ("default", "tiny", 0)],
    "solve_on_trial": [("gentle", "tall", 0)],
    "f_from_s1": [("default", "G2", 0), ("default", "odd", 1), ("default", "tiny", 0), ("default", "tall", 1)],
}


@pytest.mark.parametrize("name", ih.CASES)
def test_the_model_descends(oracle, name):
    """10 iterations from both poses of grad_helpers.scene, default hyper-parameters: F_acc never rises, accepted + rejected = evaluations,
    the returned pose is the best trial, and the trace checks find nothing"""
    ev = gn.scene_evaluator(oracle, name)
    for b in range(gh.N_POSES):
        h = gn.hyper()
        r = gn.lm(ev, gn.scene_pose(oracle, name, b), 10, h)
        tr = r["trace"]
        acc = tr[tr[:, 7] > 0]
        print("%s pose %d: sigma^2 %.6f -> %.6f, %d accepted, %d rejected, status %d, flags %s" % (name, b, r["sigma2_start"], r["sigma2"], r["accepted"],
                                                                                                   r["rejected"], r["status"], tr[:, 7].astype(int)))
        assert (np.diff(acc[:, 6]) < 0).all()
        assert r["accepted"] + r["rejected"] == r["evaluations"] == 11 and r["status"] == 0
        assert r["sigma2"] == tr[: r["evaluations"], 6].min() == acc[-1, 6] and np.array_equal(r["theta"], acc[-1, :6])
        assert r["sigma2"] < r["sigma2_start"]
        assert gn.trace_violations(r, h, 10, ev) == []


@pytest.mark.parametrize("config", list(gn.CONFIGS))
def test_the_model_passes_its_own_trace_checks(oracle, config):
    for name in ih.CASES:
        ev = gn.scene_evaluator(oracle, name)
        for b in range(gh.N_POSES):
            h = gn.hyper(**gn.CONFIGS[config])
            assert gn.trace_violations(gn.lm(ev, gn.scene_pose(oracle, name, b), gn.TRACE_ITERS, h), h, gn.TRACE_ITERS, ev) == [], (config, name, b)


def test_a_weight_plane_enters_the_model(oracle):
    """the weighted model passes the same checks, and weights scaled by 4 change no pose, no lambda, no flag and no F"""
    ev1, ev4 = gn.scene_evaluator(oracle, "odd", gn.weight_plane("odd")), gn.scene_evaluator(oracle, "odd", 4 * gn.weight_plane("odd"))
    h = gn.hyper()
    r1, r4 = (gn.lm(ev, gn.scene_pose(oracle, "odd", 1), gn.TRACE_ITERS, h) for ev in (ev1, ev4))
    assert gn.trace_violations(r1, h, gn.TRACE_ITERS, ev1) == []
    assert np.array_equal(r1["trace"][:, :9], r4["trace"][:, :9]) and np.array_equal(4 * r1["trace"][:, 9], r4["trace"][:, 9])
    plain = gn.lm(gn.scene_evaluator(oracle, "odd"), gn.scene_pose(oracle, "odd", 1), gn.TRACE_ITERS, h)
    assert not np.array_equal(plain["trace"][:, 6], r1["trace"][:, 6])


@pytest.mark.parametrize("variant", list(gn.VARIANTS))
def test_planted_variants_break_the_trace_checks(oracle, variant):
    """each planted mistake of lm() breaks what the device's trace test asserts, on every (configuration, case, pose) named in CATCHERS"""
    for config, name, b in CATCHERS[variant]:
        ev = gn.scene_evaluator(oracle, name)
        h = gn.hyper(**gn.CONFIGS[config])
        bad = gn.trace_violations(gn.lm(ev, gn.scene_pose(oracle, name, b), gn.TRACE_ITERS, h, variant), h, gn.TRACE_ITERS, ev)
        print("%s on %s / %s pose %d: %s" % (variant, config, name, b, bad[:2]))
        assert bad, (gn.VARIANTS[variant], config, name, b)


def test_the_first_evaluation_can_refuse(oracle):
    """a scene whose panorama is black: M = 0, the chain freezes with status 1 after one evaluation and returns the caller's pose"""
    xyz, rgb, img = gh.scene(oracle, "tiny")[:3]
    th0 = gn.scene_pose(oracle, "tiny", 0)
    r = gn.lm(lambda th: gn.evaluate(oracle, (xyz, rgb, np.zeros_like(img)), th), th0, 4, gn.hyper())
    assert (r["status"], r["evaluations"], r["accepted"], r["rejected"]) == (1, 1, 0, 1) and np.array_equal(r["theta"], th0)


@pytest.mark.parametrize("name", gn.FREE_CASES)
def test_the_free_run_yardstick(oracle, name):
    """the model converges near every start of the free-run test, its final sigma^2 over the start and its 12 one-ulp neighbours spans a
    finite [lo, hi], and the model's own run from the start keeps the bound the device is held to"""
    for i, start in enumerate(gn.free_starts(oracle, name)):
        lo, hi, own = gn.free_yardstick(oracle, name, i)
        bound = gn.free_bound(lo, hi)
        print("%s start %d: model sigma^2 in [%.9g, %.9g], own %.9g, bound %.9g (sigma^2 at the start %.6f, at the centre %.9g)"
              % (name, i, lo, hi, own, bound, gn.scene_evaluator(oracle, name)(start)["F"], gn.free_centre(oracle, name)[1]))
        assert np.isfinite([lo, hi]).all() and lo <= own <= hi <= bound
        assert hi < 0.5 * gn.scene_evaluator(oracle, name)(start)["F"]                  # the start is not the minimum: something is polished
