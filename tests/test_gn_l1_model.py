"""The float64 model of the Huber-L1 form of the Levenberg-Marquardt polish (tests/gn_l1_helpers.py), on the CPU:
its two limits (delta below every residual: b_rho / M is the sampling loss's gradient; delta above every residual: the L2 form over
delta), the objective never rises along a chain and the sampling loss ends below its start, the device bound holds for an fp32
restatement of the pass and breaks for every planted mistake, gn_schedule reads cfg.gn_objective / gn_delta and refuses what it should,
the entry points that polish nothing refuse the two keys, the rooms paths refuse "l1", and the four new exports answer -1 on null
arguments."""
import ctypes

import numpy as np
import pytest
import torch

import gn_helpers as gn
import gn_l1_helpers as g1
import grad_helpers as gh
import info_helpers as ih
from conftest import Cfg

KEY = "gn_"
CHAIN_DELTAS = (1.0 / 255, 1.0 / 64, 0.05)

# which (case, pose, delta, weighted) catches which planted variant of gn_l1_helpers.l1_sums (asserted below)
CATCHERS = {
    "phi_squared": [("G2", 0, 1.0 / 64, False), ("tall", 1, 1.0 / 255, True)],
    "no_floor": [("G2", 0, 0.05, False), ("odd", 1, 0.05, True)],
    "m_phi": [("G2", 1, 1.0 / 64, False), ("tiny", 0, 1.0 / 255, True)],
    "s1_phi": [("odd", 0, 1.0 / 64, False), ("tall", 0, 1.0 / 255, True)],
    "rho_no_offset": [("G2", 0, 1.0 / 64, False), ("tiny", 1, 1.0 / 255, True)],
    "rho_no_half": [("G2", 0, 0.05, False), ("odd", 1, 0.05, True)],
    "b_phi_twice": [("odd", 0, 1.0 / 64, False), ("tall", 1, 1.0 / 255, True)],
}


def _kept_rows(oracle, name, b):
    m = gh.case_model(oracle, name, b)
    return m, m["kept"]


# ================================================================================================================== the two limits
@pytest.mark.parametrize("name", ih.CASES)
def test_small_delta_is_the_sampling_loss(oracle, name):
    """delta = 2^-12 is below every kept residual of both poses: b_rho / M equals the oracle's sampling_loss gradient [grad_t, grad_ypr] to
    1e-12 relative, and S_rho = S1 - delta / 2 M"""
    xyz, rgb, img, _, trans, rot = gh.scene(oracle, name)
    d = g1.DELTA_SMALL
    for b in range(gh.N_POSES):
        m, kept = _kept_rows(oracle, name, b)
        assert m["loss"][kept].min() > d, (name, b, m["loss"][kept].min())
        r = g1.evaluate_l1(oracle, (xyz, rgb, img), gn.scene_pose(oracle, name, b), d)
        o = oracle.sampling_loss(xyz, rgb, img, trans[b:b + 1], rot[b:b + 1], dtype=np.float64)
        want = np.concatenate([o["grad_t"][0], o["grad_ypr"][0]])
        assert o["count"][0] == r["M"]
        assert np.abs(r["b"] / r["M"] - want).max() <= 1e-12 * np.abs(want).max(), (name, b)
        assert abs(r["S1"] / r["M"] - o["loss"][0]) <= 1e-12 * o["loss"][0]
        assert abs(r["S2"] - (r["S1"] - d / 2 * r["M"])) <= 1e-12 * r["S1"]


@pytest.mark.parametrize("name", ih.CASES)
def test_saturated_delta_is_the_l2_form(oracle, name):
    """delta = 2 is above every residual: H_rho = H / 2 and b_rho = b / 2 of info_helpers.info_model, and S_rho = S2 / 4 — exactly in
    float64 (powers of two)"""
    xyz, rgb, img = gh.scene(oracle, name)[:3]
    for b in range(gh.N_POSES):
        m, kept = _kept_rows(oracle, name, b)
        assert m["loss"][kept].max() < g1.DELTA_SATURATED
        r = g1.evaluate_l1(oracle, (xyz, rgb, img), gn.scene_pose(oracle, name, b), g1.DELTA_SATURATED)
        l2 = ih.info_model(m, kept, np.ones(len(xyz)))
        assert np.array_equal(r["H"], l2["H"] / 2) and np.array_equal(r["b"], l2["b"] / 2) and r["S2"] == l2["S2"] / 4
        assert r["M"] == l2["M"] and r["S1"] == l2["S1"]


# ============================================================================================================== the chain descends
@pytest.mark.parametrize("name", ih.CASES)
def test_the_objective_never_rises_and_the_sampling_loss_falls(oracle, name):
    """gn_helpers.lm, unchanged, on evaluate_l1 from both start poses, delta in {1/255, 1/64, 0.05}, 10 iterations: F_rho never rises along the
    accepted poses, the final S1 / M is below the start's, and gn_helpers.trace_violations finds nothing"""
    for delta in CHAIN_DELTAS:
        ev = g1.scene_evaluator_l1(oracle, name, delta)
        for b in range(gh.N_POSES):
            h = gn.hyper()
            th0 = gn.scene_pose(oracle, name, b)
            r = gn.lm(ev, th0, 10, h)
            tr = r["trace"]
            acc = tr[: r["evaluations"]][tr[: r["evaluations"], 7] > 0]
            start, end = ev(th0), ev(r["theta"])
            print("%s pose %d delta %.5f: F_rho %.6f -> %.6f, S1/M %.6f -> %.6f, %d accepted, %d rejected, status %d"
                  % (name, b, delta, r["sigma2_start"], r["sigma2"], start["S1"] / start["M"], end["S1"] / end["M"], r["accepted"], r["rejected"],
                     r["status"]))
            assert (np.diff(acc[:, 6]) < 0).all() and r["accepted"] > 1
            assert r["sigma2"] < r["sigma2_start"]
            assert end["S1"] / end["M"] < start["S1"] / start["M"], (name, b, delta)
            assert gn.trace_violations(r, h, 10, ev) == []


def test_a_weight_plane_enters_the_model(oracle):
    w = gn.weight_plane("odd")
    ev1, ev4 = g1.scene_evaluator_l1(oracle, "odd", 1.0 / 64, w), g1.scene_evaluator_l1(oracle, "odd", 1.0 / 64, 4 * w)
    h = gn.hyper()
    r1, r4 = (gn.lm(ev, gn.scene_pose(oracle, "odd", 1), gn.TRACE_ITERS, h) for ev in (ev1, ev4))
    assert gn.trace_violations(r1, h, gn.TRACE_ITERS, ev1) == []
    assert np.array_equal(r1["trace"][:, :9], r4["trace"][:, :9]) and np.array_equal(4 * r1["trace"][:, 9], r4["trace"][:, 9])
    plain = gn.lm(g1.scene_evaluator_l1(oracle, "odd", 1.0 / 64), gn.scene_pose(oracle, "odd", 1), gn.TRACE_ITERS, h)
    assert not np.array_equal(plain["trace"][:, 6], r1["trace"][:, 6])


# ================================================================================================================ the device bound
@pytest.mark.parametrize("name", ih.CASES)
def test_the_model_and_an_fp32_restatement_keep_the_bound(oracle, name):
    """violations_l1 of the float64 model itself and of the pass's arithmetic restated in fp32 numpy on the fp32 model's rows: none, for
    both poses, with and without a weight plane, at delta = 1/64, 1/255, and at the two limits"""
    for delta in g1.DELTAS + (g1.DELTA_SMALL, g1.DELTA_SATURATED):
        for plane in (None, gn.weight_plane(name)):
            for b in range(gh.N_POSES):
                bd = g1.bounds_l1(oracle, name, b, delta, plane)
                assert g1.violations_l1(bd["ref"], bd) == []
                got = g1.device_restatement(oracle, bd, delta)
                bad = g1.violations_l1(got, bd)
                nH = np.sqrt(np.outer(np.diag(bd["ref"]["H"]), np.diag(bd["ref"]["H"])))
                print("%s pose %d delta %.6f weighted %d: fp32 restatement |dH|/norm %.3e (bound %.3e), b %.3e of its bound, S_rho %.3e of its bound"
                      % (name, b, delta, plane is not None, (np.abs(got["H"] - bd["ref"]["H"]) / nH).max(), (bd["BH"] / nH).max(),
                         (np.abs(got["b"] - bd["ref"]["b"]) / bd["Bb"]).max(), abs(got["S2"] - bd["ref"]["S2"]) / bd["BS2"]))
                assert bad == [], (name, b, delta, plane is not None, bad)


@pytest.mark.parametrize("variant", list(g1.VARIANTS))
def test_planted_variants_break_the_bound(oracle, variant):
    """each planted mistake of l1_sums breaks what the device's record test asserts, on every case named for it in CATCHERS"""
    for name, b, delta, weighted in CATCHERS[variant]:
        bd = g1.bounds_l1(oracle, name, b, delta, gn.weight_plane(name) if weighted else None, variant=variant)
        bad = g1.violations_l1(bd["got"], bd)
        print("%s on %s pose %d delta %.5f weighted %d: %s" % (variant, name, b, delta, weighted, bad))
        assert bad, (g1.VARIANTS[variant], name, b, delta)


# ===================================================================================================================== the cfg keys
def _cfg(**kw):
    kw.setdefault("num_iter", 100)
    return Cfg(**kw)


def test_the_schedule_is_unchanged_without_the_keys_and_reads_them():
    from piccolo_amd import omniloc as po, ops
    assert po.GN_KEYS[:3] == ("gn_iters", "gn_step_cap", "gn_lambda") and set(po.GN_KEYS[3:]) == {"gn_objective", "gn_delta"}
    assert po.gn_schedule(_cfg()) is None
    assert po.gn_schedule(_cfg(gn_iters=None, gn_objective=None, gn_delta=None)) is None
    assert po.gn_schedule(_cfg(gn_iters=5)) == (5, {})
    assert po.gn_schedule(_cfg(gn_iters=5, gn_objective="l2")) == (5, {})
    assert po.gn_schedule(_cfg(gn_iters=1, gn_step_cap=0.05, gn_objective="l2")) == (1, {"step_cap": 0.05})
    assert po.gn_schedule(_cfg(gn_iters=5, gn_objective="l1")) == (5, {"objective": "l1"})
    assert po.gn_schedule(_cfg(gn_iters=5, gn_objective="l1", gn_delta=1 / 255)) == (5, {"objective": "l1", "delta": 1 / 255})
    assert po.gn_schedule(_cfg(gn_iters=2, gn_lambda=1e-2, gn_objective="l1", gn_delta=4)) == (2, {"lam0": 1e-2, "objective": "l1", "delta": 4.0})
    assert po.gn_schedule(_cfg(gn_iters=2, gn_objective="l1", gn_delta=2.0 ** -20, pose_covariance=True, prune_iters=10, prune_keep=2))[1]["delta"] == 2.0 ** -20
    assert ops.GN_L1_DELTA == 1 / 64 and float(np.float32(ops.GN_L1_DELTA)) == ops.GN_L1_DELTA


@pytest.mark.parametrize("kw,key", [
    (dict(gn_iters=5, gn_objective="L1"), "gn_objective"), (dict(gn_iters=5, gn_objective="huber"), "gn_objective"),
    (dict(gn_iters=5, gn_objective=1), "gn_objective"), (dict(gn_iters=5, gn_objective=True), "gn_objective"),
    (dict(gn_objective="l1"), "gn_objective"), (dict(gn_objective="l2"), "gn_objective"), (dict(gn_delta=1 / 64), "gn_delta"),
    (dict(gn_objective="l1", gn_delta=1 / 64), "gn_"), (dict(gn_iters=5, gn_delta=1 / 64), "gn_delta"),
    (dict(gn_iters=5, gn_objective="l2", gn_delta=1 / 64), "gn_delta"), (dict(gn_iters=5, gn_objective="l1", gn_delta=0.0), "gn_delta"),
    (dict(gn_iters=5, gn_objective="l1", gn_delta=-1 / 64), "gn_delta"), (dict(gn_iters=5, gn_objective="l1", gn_delta=float("nan")), "gn_delta"),
    (dict(gn_iters=5, gn_objective="l1", gn_delta=float("inf")), "gn_delta"), (dict(gn_iters=5, gn_objective="l1", gn_delta="0.01"), "gn_delta"),
    (dict(gn_iters=5, gn_objective="l1", gn_delta=True), "gn_delta"), (dict(gn_iters=5, gn_objective="l1", gn_delta=2.0 ** -21), "gn_delta"),
    (dict(gn_iters=5, gn_objective="l1", gn_delta=4.5), "gn_delta"), (dict(gn_iters=5, gn_objective="l1", depth_mask=True), "gn_")])
def test_the_schedule_refuses(kw, key):
    from piccolo_amd import omniloc as po
    with pytest.raises(ValueError, match=key):
        po.gn_schedule(_cfg(**kw))


def test_the_ops_layer_refuses_before_a_device_call():
    """ops.gn_objective is what every objective= / delta= pair goes through first; objective and delta are no hyper-parameters"""
    from piccolo_amd import ops
    assert ops.gn_objective("x") is None and ops.gn_objective("x", "l2") is None and ops.gn_objective("x", None) is None
    assert ops.gn_objective("x", "l1") == ops.GN_L1_DELTA and ops.gn_objective("x", "l1", 0.05) == 0.05
    for args in (("l3",), (1,), ("l2", 0.1), (None, 0.1), ("l1", 0.0), ("l1", float("nan")), ("l1", float("inf")), ("l1", 5.0), ("l1", 1e-7),
                 ("l1", "0.1"), ("l1", True)):
        with pytest.raises(ValueError):
            ops.gn_objective("x", *args)
    for kw in (dict(objective="l1"), dict(delta=0.1)):
        with pytest.raises(ValueError, match="unknown hyper-parameter"):
            ops.gn_hyper(**kw)


IMG, Z = torch.zeros(4, 8, 3), torch.zeros(4, 3)


@pytest.mark.parametrize("kw", [dict(gn_objective="l1"), dict(gn_objective="l2"), dict(gn_delta=1 / 64), dict(gn_iters=3, gn_objective="l1", gn_delta=1 / 64)])
def test_entry_points_without_a_polish_refuse_the_keys(kw):
    """every entry point that refuses gn_iters refuses gn_objective and gn_delta, before it touches a device"""
    from piccolo_amd import localize, omniloc as po
    cfg = _cfg(num_input=4, **kw)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc(IMG, Z, Z, Z.clone(), Z.clone(), 0, cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_all(IMG, Z, Z, Z.clone(), Z.clone(), cfg, {})
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_images_robust([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], _cfg(num_input=4, robust_iters=20, **kw))
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms(IMG, [(Z, Z), (Z, Z)], [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG], [(Z, Z)], [[Z.clone()]], [[Z.clone()]], cfg)
    with pytest.raises(ValueError, match=KEY):
        po.omniloc_batch_rooms_images([IMG, IMG], [(Z, Z)], [[Z.clone(), Z.clone()]], [[Z.clone(), Z.clone()]], cfg)
    with pytest.raises(ValueError, match=KEY):
        localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), _cfg(num_input=4, parallel=False, **kw))


@pytest.mark.parametrize("kw", [dict(), dict(images_per_launch=4), dict(room_search=True), dict(room_search_images=4)])
def test_the_dataset_loops_refuse_at_configuration_time(kw, tmp_path):
    from piccolo_amd import localize
    cfg = _cfg(num_input=6, parallel=True, gn_iters=3, gn_objective="l1", dataset="stanford", **kw)
    root = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match=KEY):
        localize.localize_stanford(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_omniscenes(cfg, None, None, root)
    with pytest.raises(ValueError, match=KEY):
        localize.localize_synthetic(cfg)


def test_the_entry_points_that_polish_refuse_bad_values_before_a_device():
    from piccolo_amd import localize, omniloc as po
    run = lambda cfg, rgb=Z: po.omniloc_batch(IMG, Z, rgb, Z.clone(), Z.clone(), cfg, {})      # noqa: E731
    many = lambda cfg: po.omniloc_batch_images_polished([IMG, IMG], Z, Z, [Z.clone(), Z.clone()], [Z.clone(), Z.clone()], cfg)      # noqa: E731
    for call in (run, many, lambda cfg: localize.refine_image(IMG, Z, Z, Z.clone(), Z.clone(), cfg)):
        with pytest.raises(ValueError, match="gn_objective"):
            call(_cfg(num_input=4, parallel=True, gn_iters=3, gn_objective="l3"))
        with pytest.raises(ValueError, match="gn_delta"):
            call(_cfg(num_input=4, parallel=True, gn_iters=3, gn_objective="l1", gn_delta=8.0))
        with pytest.raises(ValueError, match="gn_delta"):
            call(_cfg(num_input=4, parallel=True, gn_iters=3, gn_delta=0.01))
        with pytest.raises(ValueError, match="gn_objective"):
            call(_cfg(num_input=4, parallel=True, gn_objective="l1"))


def test_the_rooms_paths_refuse_l1(tmp_path):
    """omniloc_batch_rooms_images_polished, a room search with cfg.room_search_polish and ops.gauss_newton_refine_rooms have no L1 form"""
    from piccolo_amd import localize, omniloc as po, ops
    with pytest.raises(ValueError, match="gn_objective"):
        po.omniloc_batch_rooms_images_polished([IMG, IMG], [(Z, Z)], [[Z.clone(), Z.clone()]], [[Z.clone(), Z.clone()]],
                                               _cfg(num_input=4, gn_iters=3, gn_objective="l1"))
    cfg = _cfg(num_input=6, parallel=True, gn_iters=3, gn_objective="l1", dataset="stanford", room_search=True, room_search_polish=True)
    with pytest.raises(ValueError, match="gn_objective"):
        localize.localize_stanford(cfg, None, None, str(tmp_path / "nowhere"))
    l1_forms = {form for form, objective in ops._POSE_FORMS if objective == "l1"}
    assert ("rooms", "l2") in ops._POSE_FORMS and l1_forms == {"single", "images", "depth"}      # (and gn_hyper refuses objective=)
    with pytest.raises(ValueError, match='objective="l1" has no rooms form'):
        ops._pose_form("gauss_newton_refine_rooms", "rooms", 1.0 / 64)
    # "l2" passes the refusal (and fails later, on what the call lacks)
    po._refuse_l1(po.gn_schedule(_cfg(gn_iters=3, gn_objective="l2")), "x")


def test_the_shipped_config_parses():
    """configs/stanford_mi355x_b8_polish_l1.ini is stanford_mi355x_b8_polish.ini plus gn_objective = l1"""
    import os
    from conftest import REPO
    from piccolo_amd import omniloc as po, parse_utils
    a = parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b8_polish.ini"))._asdict()
    b = parse_utils.parse_ini(os.path.join(REPO, "configs", "stanford_mi355x_b8_polish_l1.ini"))._asdict()
    assert b.pop("gn_objective") == "l1" and a == b
    assert po.gn_schedule(Cfg(gn_objective="l1", **b)) == (5, {"objective": "l1"})


# ================================================================================================================== null arguments
@pytest.mark.parametrize("name", ["pcl_pose_information_l1", "pcl_pose_information_images_l1", "pcl_gn_refine_l1", "pcl_gn_refine_images_l1"])
def test_null_arguments_answer_minus_one(name):
    """declared in the header, bound, exported; all-null / all-zero arguments answer -1 (PCL_EINVAL) before any HIP call — and so does a
    delta out of range or not finite next to arguments that are otherwise null"""
    import os
    from conftest import REPO
    from piccolo_amd import _lib
    assert name in _lib.SIGNATURES
    with open(os.path.join(REPO, "include", "piccolo_hip.h")) as f:
        assert ("int %s(" % name) in f.read()
    lib = _lib.load()
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and args[-2] is ctypes.c_float and args[-1] is ctypes.c_void_p
    # the twin's parameters without `cov` (one pointer of the run of output pointers), plus a float delta before the stream
    twin = list(_lib.SIGNATURES[name[:-3]][1])
    del twin[twin.index(ctypes.c_size_t) - 2]
    twin.insert(len(twin) - 1, ctypes.c_float)
    assert list(args) == twin
    for delta in (0.0, 1.0 / 64, float("nan"), float("inf"), 8.0):
        call = [None if a is ctypes.c_void_p or hasattr(a, "contents") else 0 for a in args]
        call[-2] = delta
        assert getattr(lib, name)(*call) == -1, (name, delta)
    assert lib.pcl_abi_version() == 12
