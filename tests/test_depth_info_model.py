"""The float64 composition the device's depth forms are held to (tests/depth_info_helpers.py), on the CPU, with the model's own z-buffer
(depth_helpers.reference_zbuffer) standing in for the device's:
  * with a tolerance so large that nothing is hidden the masked sums are info_helpers' unmasked sums exactly;
  * under the real tolerance something is hidden, the sums change, and the model keeps its own bounds (the check does not fire on what it
    should pass) while a planted mistake — hidden points counted, the mask of another pose — breaks them;
  * for every case used on the GPU, the two tiny clouds included, the share of points expected_visible leaves undecided is at most
    depth_helpers.LEFT_OUT_CAP, and no pair's black decision differs between the fp64 and the fp32 model;
  * the LM chain on the masked evaluator (the mask rebuilt at every trial pose) passes gn_helpers' trace checks."""
import numpy as np
import pytest

import depth_helpers as dh
import depth_info_helpers as dih
import gn_helpers as gn
import info_helpers as ih


def _identity(oracle, case):
    xyz, rgb = dih.scene(oracle)[:2]
    return np.arange(len(dih.case_points(case, xyz, rgb)[0]))


def _own_visibility(cm, b):
    """(visible per point against the model's own z-buffer, expect, decided)"""
    z = dh.reference_zbuffer(cm, b)
    expect, decided = dh.expected_visible(cm, b, z)
    return expect, decided


def test_the_cases_are_the_projects_cases():
    for name in ("W1", "W4", "W7", "C1"):
        k = dh.CASES[name]
        assert dih.CASES[name] == (None, k["grid"], k["stride"], k["tau"])
    assert dih.CASES["W1"][1] == (64, 256) and dih.CASES["W4"][1:3] == ((64, 128), 2) and dih.CASES["W7"][3] == 0.1 and dih.CASES["C1"][1] == (24, 40)
    assert dih.CASES["t513"] == (513, (16, 32), 1, 0.0) and dih.CASES["t700"] == (700, (16, 32), 1, 0.0)
    assert (dih.H, dih.W) == (128, 256)


@pytest.mark.parametrize("case", list(dih.CASES))
def test_undecided_share_stays_under_the_projects_cap(oracle, case):
    order = _identity(oracle, case)
    cm = dih.case_model(oracle, case, order)
    for b in range(dh.B_POSES):
        expect, decided = _own_visibility(cm, b)
        assert 1.0 - decided.mean() <= dh.LEFT_OUT_CAP, (case, b, 1.0 - decided.mean())
        assert expect[decided].any()
        if dih.CASES[case][0] is None:
            assert not expect[decided].all(), (case, b)        # the occluder hides something from every pose
        m64, m32 = (dih.take(m, order) for m in dih.point_models(oracle, b))
        assert dih.bounds(m64, m32, np.ones(len(order), bool))["undecided_kept"] == 0, (case, b)


@pytest.mark.parametrize("case", ["W1", "t700"])
def test_nothing_hidden_is_the_unmasked_model_exactly(oracle, case):
    order = _identity(oracle, case)
    cm = dih.case_model(oracle, case, order, tau=dih.NOTHING_HIDDEN_TAU)
    for b in range(dh.B_POSES):
        expect, decided = _own_visibility(cm, b)
        assert expect.all()
        m64 = dih.take(dih.point_models(oracle, b)[0], order)
        masked = dih.masked_info(m64, expect)
        plain = ih.info_model(m64, m64["kept"], np.ones(len(order)))
        for key in ("M", "S1", "S2", "sigma2"):
            assert masked[key] == plain[key], (case, b, key)
        for key in ("H", "b", "cov"):
            assert np.array_equal(masked[key], plain[key]), (case, b, key)


@pytest.mark.parametrize("case", ["W1", "W4", "W7", "C1"])
def test_the_masked_model_keeps_its_bounds_and_planted_mistakes_break_them(oracle, case):
    order = _identity(oracle, case)
    cm = dih.case_model(oracle, case, order)
    vis = [_own_visibility(cm, b)[0] for b in range(dh.B_POSES)]
    for b in range(dh.B_POSES):
        m64, m32 = (dih.take(m, order) for m in dih.point_models(oracle, b))
        bd = dih.bounds(m64, m32, vis[b])
        assert 0 < bd["ref"]["M"] < m64["kept"].sum()                     # something is hidden that would have counted
        assert bd["border_share"] <= 0.01, (case, b, bd["border_share"])
        assert ih.violations(bd["ref"], bd) == [], (case, b)
        assert ih.violations(bd["yard"], bd) == [] or bd["yard"]["M"] != bd["ref"]["M"], (case, b)
        assert np.linalg.cond(bd["ref"]["H"]) < 1e8, (case, b)
        # hidden points counted (the unmasked sums), and the mask of another pose
        unmasked = ih.info_model(m64, m64["kept"], np.ones(len(order)))
        assert ih.violations(unmasked, bd) != [], (case, b)
        other = dih.masked_info(m64, vis[(b + 1) % dh.B_POSES])
        assert ih.violations(other, bd) != [], (case, b)


@pytest.mark.parametrize("case", ["C1", "t700"])
def test_the_chain_on_the_masked_evaluator_passes_the_trace_checks(oracle, case):
    """gn_helpers.lm on the evaluator that rebuilds the mask at every trial pose: the trace checks hold with that evaluator, sigma^2 does not
    grow, and the unmasked evaluator gives another chain (the mask enters)"""
    order = _identity(oracle, case)
    xyz, rgb, img, trans, rot = dih.scene(oracle)
    ev = dih.masked_evaluator(oracle, case, order)
    h = gn.hyper()
    th0 = np.concatenate([trans[0], rot[0]]).astype(np.float32)
    r = gn.lm(ev, th0, 3, h)
    assert gn.trace_violations(r, h, 3, ev) == []
    assert r["sigma2"] <= r["sigma2_start"]
    x, c = dih.case_points(case, xyz, rgb)
    plain = gn.lm(lambda th: gn.evaluate(oracle, (x, c, img), th), th0, 3, h)
    assert not np.array_equal(plain["trace"][:, 6], r["trace"][:, 6])
