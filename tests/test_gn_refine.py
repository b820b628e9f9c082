"""The Levenberg-Marquardt pose polish on the device (pcl_gn_refine; build-defined) against ops.pose_information and
the float64 model of tests/gn_helpers.py.  Every decision of a device chain is checked TEACHER-FORCED: the yardstick of evaluation k is
pose_information at the pose the device itself tried, so a chain that takes another branch than the model is still held to the algorithm.
The CPU side — the model descends, the same trace checks catch every planted mistake — is tests/test_gn_model.py."""
import numpy as np
import pytest

import gn_helpers as gn
import grad_helpers as gh
import info_helpers as ih

gpu = pytest.mark.gpu
FMTS = ("f16", "u8", "f32")
FIELDS = ("trans", "rot", "sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats", "cov")


@pytest.fixture(scope="module")
def ops():
    import torch
    from piccolo_amd import ops as o
    o._lib.load()
    assert torch.cuda.is_available()
    return o


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


_CLOUDS, _PANOS = {}, {}


def _pano(ops, oracle, name, fmt):
    from parity_helpers import T
    if (name, fmt) not in _PANOS:
        _PANOS[name, fmt] = ops.Pano(T(gh.scene(oracle, name)[2]), fmt=fmt)
    return _PANOS[name, fmt]


def _cloud(ops, oracle, name, weights=None, tag=None):
    from parity_helpers import T
    if (name, tag) not in _CLOUDS:
        xyz, rgb = gh.scene(oracle, name)[:2]
        _CLOUDS[name, tag] = ops.Cloud(T(xyz), T(rgb), weights=None if weights is None else T(np.asarray(weights, np.float32)))
    return _CLOUDS[name, tag]


def _poses(oracle, name):
    return np.stack([gn.scene_pose(oracle, name, b) for b in range(gh.N_POSES)])


def _refine(ops, cloud, pano, thetas, iters, **hyper):
    from parity_helpers import T
    thetas = np.asarray(thetas, np.float32).reshape(-1, 6)
    return ops.gauss_newton_refine(cloud, pano, T(thetas[:, :3].copy()), T(thetas[:, 3:].copy()), iters=iters, trace=True, **hyper)


def _runs(res):
    """the device's dict of GPU tensors -> one run dict per pose in gn_helpers.lm()'s layout"""
    host = {key: v.cpu().numpy() for key, v in res.items()}
    out = []
    for i in range(host["trans"].shape[0]):
        r = dict(theta=np.concatenate([host["trans"][i], host["rot"][i]]), trace=host["trace"][:, i])
        for key in ("sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats", "cov"):
            r[key] = host[key][i]
        out.append(r)
    return out


def _info_at(ops, cloud, pano, thetas):
    """ops.pose_information at every pose of thetas (m, 6) in ONE call -> lookup theta -> dict(F, M, ok, H, b float64 of the fp32 values, and
    the fp32 rows themselves)"""
    from parity_helpers import T
    uniq = {np.asarray(t, np.float32).tobytes(): np.asarray(t, np.float32) for t in thetas}
    th = np.stack(list(uniq.values()))
    H, b, st, cov = (t.cpu().numpy() for t in ops.pose_information(cloud, pano, T(th[:, :3].copy()), T(th[:, 3:].copy())))
    table = {key: dict(F=st[i, 3], M=st[i, 0], ok=st[i, 4] != 1, H=H[i].astype(np.float64), b=b[i].astype(np.float64), H32=H[i], b32=b[i], stats=st[i],
                       cov=cov[i]) for i, key in enumerate(uniq)}
    return lambda theta: table[np.asarray(theta, np.float32).tobytes()]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _final_equals_pose_information(run, at):
    ref = at(run["theta"])
    return _same(run["H"], ref["H32"]) and _same(run["b"], ref["b32"]) and _same(run["stats"], ref["stats"]) and _same(run["cov"], ref["cov"])


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_zero_iterations_are_pose_information(ops, oracle, name, fmt):
    """iters = 0: the returned pose is the caller's bit for bit, H, b, stats and cov equal ops.pose_information at that pose bit for bit,
    one evaluation, accepted, status 0 — with and without a weight plane"""
    from parity_helpers import T
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    for cloud in (_cloud(ops, oracle, name), _cloud(ops, oracle, name, gn.weight_plane(name), "w")):
        res = _refine(ops, cloud, pano, th, 0)
        ref = ops.pose_information(cloud, pano, T(th[:, :3].copy()), T(th[:, 3:].copy()))
        assert same_bits(res["trans"], T(th[:, :3].copy())) and same_bits(res["rot"], T(th[:, 3:].copy()))
        for key, want in zip(("H", "b", "stats", "cov"), ref):
            assert same_bits(res[key], want), (name, fmt, key)
        assert (res["evaluations"] == 1).all() and (res["accepted"] == 1).all() and (res["rejected"] == 0).all() and (res["status"] == 0).all()
        assert same_bits(res["sigma2"], ref[2][:, 3]) and same_bits(res["sigma2_start"], ref[2][:, 3])
        assert res["trace"].shape == (1, 2, 16) and same_bits(res["trace"][0, :, 6], ref[2][:, 3]) and (res["trace"][0, :, 7] == 1).all()


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_trace_is_the_algorithm(ops, oracle, parity, name, fmt):
    """iters = 6 from both scene poses, with and without a weight plane, under the default hyper-parameters (f16 also under the two other
    configurations of gn_helpers.CONFIGS), teacher-forced (gn_helpers.trace_violations): for every evaluation F and M equal
    ops.pose_information at the trace's theta_try bit for bit; the accepted flags are the fp32 rule applied to the trace's own F; the lambda
    column is the fp32 recurrence; the counters agree with the flags; the returned pose is the last accepted trial and the returned info
    and cov equal pose_information there bit for bit; every step theta_try(k + 1) - theta_acc(k) is within
    20 cond(H + lambda diag H) 2^-24 ||delta||inf + ulp(theta) of the float64 solve on pose_information's fp32 H and b at theta_acc(k), cap
    included (gn_helpers.step_bound)."""
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    for config in gn.CONFIGS if fmt == "f16" else ("default",):
        h = gn.hyper(**gn.CONFIGS[config])
        for tag, cloud in (("plain", _cloud(ops, oracle, name)), ("weighted", _cloud(ops, oracle, name, gn.weight_plane(name), "w"))):
            runs = _runs(_refine(ops, cloud, pano, th, gn.TRACE_ITERS, **gn.CONFIGS[config]))
            at = _info_at(ops, cloud, pano, np.concatenate([r["trace"][: int(r["evaluations"]), :6] for r in runs]))
            for b, r in enumerate(runs):
                label = "%s %s %s %s pose %d" % (name, fmt, config, tag, b)
                worst = []
                bad = gn.trace_violations(r, h, gn.TRACE_ITERS, at, report=lambda a, bd: worst.append((a, bd)))
                print("%s: sigma^2 %.6f -> %.6f, flags %s, status %d, worst step %s" % (label, r["sigma2_start"], r["sigma2"],
                                                                                      r["trace"][:, 7].astype(int), r["status"], worst))
                assert bad == [], (label, bad)
                assert _final_equals_pose_information(r, at), label
                assert r["status"] in (0, 3) and r["accepted"] >= 1
                for a, bd in worst:
                    parity(label + ": worst step against the float64 solve", a, bd)


@gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", gn.FREE_CASES)
def test_a_free_run_ends_where_the_model_ends(ops, oracle, parity, name, fmt):
    """iters = 8 from the starts +- 0.05 m / +- 0.03 rad around the model's own converged pose, default hyper-parameters: the device's final
    sigma^2 is at most hi + 3 (hi - lo) + 13 x 2^-24 hi, [lo, hi] the span of the model's final sigma^2 over the start and its 12 one-ulp
    neighbours (gn_helpers.free_yardstick, free_bound; the model itself keeps it: tests/test_gn_model.py)."""
    starts = gn.free_starts(oracle, name)
    runs = _runs(_refine(ops, _cloud(ops, oracle, name), _pano(ops, oracle, name, fmt), np.stack(starts), gn.FREE_ITERS))
    for i, r in enumerate(runs):
        lo, hi, own = gn.free_yardstick(oracle, name, i)
        print("%s %s start %d: device sigma^2 %.9g (start %.9g, %d accepted, %d rejected, status %d); model [%.9g, %.9g], bound %.9g"
              % (name, fmt, i, r["sigma2"], r["sigma2_start"], r["accepted"], r["rejected"], r["status"], lo, hi, gn.free_bound(lo, hi)))
    for i, r in enumerate(runs):
        lo, hi, own = gn.free_yardstick(oracle, name, i)
        parity("%s %s start %d: final sigma^2" % (name, fmt, i), r["sigma2"], gn.free_bound(lo, hi), hi - lo)


@gpu
def test_poses_are_independent_and_a_frozen_pose_is_gated(ops, oracle):
    """`odd`, f16, B = 3 — the two scene poses and the model's converged pose — with tol between their first steps, so that the third
    converges early (status 3, fewer than iters + 1 evaluations): every pose's outputs and trace rows equal its own B = 1 call bit for bit.
    Then a panorama whose first three quarters of columns are black and a pose 1000 m away that sees the whole cloud inside them: status 1, the caller's
    pose, one evaluation, M = 0 — and its neighbours in the batch equal their own calls bit for bit; an all-black panorama: all three."""
    import torch
    from parity_helpers import T
    name, iters = "odd", 6
    ev = gn.scene_evaluator(oracle, name)
    th = np.stack([gn.scene_pose(oracle, name, 0), gn.scene_pose(oracle, name, 1), gn.free_centre(oracle, name)[0]])
    first = [np.abs(gn.solve_step(ev(t)["H"], ev(t)["b"], 1e-3, 0.1)).max() for t in th]
    assert first[2] < 0.1 * min(first[:2])
    tol = float(np.sqrt(first[2] * min(first[:2])))
    cloud, pano = _cloud(ops, oracle, name), _pano(ops, oracle, name, "f16")
    both = _refine(ops, cloud, pano, th, iters, tol=tol)
    assert both["status"][2] == 3 and both["evaluations"][2] < iters + 1 and (both["evaluations"][:2] > both["evaluations"][2]).all()
    for i in range(3):
        one = _refine(ops, cloud, pano, th[i:i + 1], iters, tol=tol)
        for key in FIELDS:
            assert same_bits(both[key][i:i + 1], one[key]), (i, key)
        assert same_bits(both["trace"][:, i:i + 1], one["trace"]), i
    assert (both["trace"][int(both["evaluations"][2]):, 2] == 0).all()
    # one pose of three sees nothing
    xyz, rgb, img = gh.scene(oracle, name)[:3]
    half = img.copy()
    half[:, : 3 * img.shape[1] // 4] = 0
    far = [np.array([sx * 1000.0, 0, 0, 0, 0, 0], np.float32) for sx in (1, -1)]
    far = [t for t in far if gn.evaluate(oracle, (xyz, rgb, half), t)["M"] == 0]
    assert far, "neither far pose sees the cloud inside the black columns"
    th = np.stack([th[0], far[0], th[1]])
    hp = ops.Pano(T(half), fmt="f16")
    batch = _refine(ops, cloud, hp, th, iters)
    assert batch["status"].tolist() == [0, 1, 0] and batch["evaluations"].tolist() == [iters + 1, 1, iters + 1]
    assert same_bits(batch["trans"][1], T(th[1, :3].copy())) and same_bits(batch["rot"][1], T(th[1, 3:].copy()))
    assert batch["stats"][1, 0] == 0 and batch["stats"][1, 4] == 1 and torch.isnan(batch["cov"][1]).all() and batch["accepted"][1] == 0
    assert (batch["trace"][1:, 1] == 0).all() and batch["trace"][0, 1, 7] == 0
    for i in (0, 2):
        one = _refine(ops, cloud, hp, th[i:i + 1], iters)
        for key in FIELDS:
            assert same_bits(batch[key][i:i + 1], one[key]), (i, key)
        assert same_bits(batch["trace"][:, i:i + 1], one["trace"]), i
    black = _refine(ops, cloud, ops.Pano(torch.zeros_like(T(img)), fmt="f16"), th, iters)
    assert (black["status"] == 1).all() and (black["evaluations"] == 1).all() and same_bits(black["trans"], T(th[:, :3].copy()))
    assert same_bits(black["rot"], T(th[:, 3:].copy())) and (black["stats"][:, 0] == 0).all() and torch.isnan(black["cov"]).all()


@gpu
@pytest.mark.parametrize("name", ih.CASES)
def test_weights(ops, oracle, name):
    """a unit weight plane gives the unweighted call's bits; weights scaled by 4 change no pose, no lambda, no flag and no sigma^2 bit (M,
    H and b x 4, cov / 4: the factorisation runs on a power-of-two scaling)"""
    th, iters = _poses(oracle, name), 6
    n = gh.CASES[name][0]
    pano = _pano(ops, oracle, name, "f16")
    plain = _refine(ops, _cloud(ops, oracle, name), pano, th, iters)
    ones = _refine(ops, _cloud(ops, oracle, name, np.ones(n), "ones"), pano, th, iters)
    for key in FIELDS + ("trace",):
        assert same_bits(plain[key], ones[key]), (name, key)
    w = gn.weight_plane(name)
    w1, w4 = _refine(ops, _cloud(ops, oracle, name, w, "w"), pano, th, iters), _refine(ops, _cloud(ops, oracle, name, 4 * w, "w4"), pano, th, iters)
    for key in ("trans", "rot", "sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status"):
        assert same_bits(w1[key], w4[key]), (name, key)
    assert same_bits(w1["trace"][:, :, :9], w4["trace"][:, :, :9]) and same_bits(4 * w1["trace"][:, :, 9], w4["trace"][:, :, 9])
    assert same_bits(4 * w1["H"], w4["H"]) and same_bits(4 * w1["b"], w4["b"]) and same_bits(4 * w1["stats"][:, :3], w4["stats"][:, :3])
    assert same_bits(w1["stats"][:, 3:], w4["stats"][:, 3:]) and same_bits(0.25 * w1["cov"], w4["cov"])
    assert not same_bits(w1["sigma2"], plain["sigma2"])


@gpu
def test_omniloc_batch_polishes_its_winner(ops, oracle):
    """omniloc_batch on the scene of test_omniloc_batch_returns_the_covariance_of_its_winner (2049 points, 64 x 128, 4 candidates, 6
    iterations): without the key the three entries are the chain's winners row, bit for bit; with gn_iters = 3 they equal what
    gauss_newton_refine_at_winners plus one forward-only sampling_loss give from the same winners row, with pose_covariance the fourth
    entry is that call's cov, and the written-back leaves are the chain's — plain, with weights=, with the robust keys (under the chain's
    last weight plane) and with the prune keys.  With a step cap so small that theta_try rounds to theta_acc no step is accepted and the
    chain's own entries come back bit for bit."""
    import torch
    from conftest import Cfg
    from parity_helpers import T
    from piccolo_amd import localize, omniloc as po, synth
    xyz, rgb, img = gh.scene(oracle, "odd")[:3]
    n = len(xyz)
    t_gt, ypr_gt = synth.gt_pose(gh.SEED)
    trans, rot = synth.start_poses(t_gt, ypr_gt, 4, seed=gh.SEED)
    x, c, im = T(xyz), T(rgb), T(img)
    w = T((0.25 + 0.75 * np.random.default_rng(3).random(n)).astype(np.float32))
    base = dict(num_iter=6, num_input=4, lr=0.1, patience=5, factor=0.9)
    pano, box = po.packed_pano(im, n_points=n), po.quantile_box_of(x, 0.05)

    def batch(weights=None, **kw):
        t, r = T(trans).clone(), T(rot).clone()
        out = po.omniloc_batch(im, x, c, t, r, Cfg(**base, **kw), {}, weights=weights)
        return [o.clone() for o in out], [t.cpu(), r.cpu()]

    def check(engine_win, plane_cloud, weights=None, **kw):
        win = engine_win.cpu()
        without, leaves0 = batch(weights, **kw)
        assert len(without) == 3 and same_bits(without[0].reshape(3), win[0, 0:3]) and same_bits(without[1].reshape(9), win[0, 3:12])
        assert same_bits(without[2].reshape(1), win[0, 12:13])
        res = ops.gauss_newton_refine_at_winners(plane_cloud, pano, engine_win, iters=3)
        assert float(res["accepted"][0]) > 1 and float(res["status"][0]) in (0.0, 3.0)
        want_R = ops.rot_from_ypr(res["rot"])[0].cpu()
        want_loss = ops.sampling_loss(plane_cloud, pano, res["trans"], res["rot"], with_grad=False)[0, 0:1].cpu()
        for extra in (dict(), dict(pose_covariance=True)):
            got, leaves1 = batch(weights, gn_iters=3, **extra, **kw)
            assert len(got) == 3 + len(extra)
            assert same_bits(got[0].reshape(3), res["trans"][0].cpu()) and same_bits(got[1], want_R) and same_bits(got[2].reshape(1), want_loss)
            assert got[0].shape == (3, 1) and got[1].shape == (3, 3) and got[2].shape == () and not got[0].is_cuda
            assert not same_bits(got[0], without[0])
            assert all(same_bits(a, b) for a, b in zip(leaves0, leaves1))
            if extra:
                assert got[3].shape == (6, 6) and not got[3].is_cuda and same_bits(got[3], res["cov"][0].cpu())
        # no step accepted: the chain's own entries, and the covariance at the chain's pose
        got, _ = batch(weights, gn_iters=3, gn_step_cap=1e-12, pose_covariance=True, **kw)
        assert all(same_bits(a, b) for a, b in zip(got[:3], without))
        assert same_bits(got[3], batch(weights, pose_covariance=True, **kw)[0][3])
        return res

    def engine(cloud):
        return ops.GradientDescent(cloud, pano, T(trans), T(rot), box)
    # plain
    cloud = po.packed_cloud(x, c)
    gd = engine(cloud)
    gd.run(6)
    win = gd.winner(1)
    res = check(win, cloud)
    own = po.gauss_newton_refine(im, x, c, win[:, 0:3].contiguous(), win[:, 13:16].contiguous(), iters=3)
    assert all(same_bits(own[key], res[key]) for key in FIELDS)
    ref = localize.refine_image(im, x, c, T(trans).clone(), T(rot).clone(), Cfg(parallel=True, gn_iters=3, pose_covariance=True, **base))
    assert len(ref) == 4 and same_bits(ref[0].reshape(3), res["trans"][0].cpu()) and same_bits(ref[3], res["cov"][0].cpu())
    assert len(localize.refine_image(im, x, c, T(trans).clone(), T(rot).clone(), Cfg(parallel=True, gn_iters=3, **base))) == 3
    # the caller's weights
    cw = po.packed_cloud(x, c, w)
    gd = engine(cw)
    gd.run(6)
    res_w = check(gd.winner(1), cw, weights=w)
    assert not same_bits(res_w["trans"], res["trans"])
    # the robust chain: under its last weight plane
    gd = engine(cloud)
    gd.run_robust(6, [2, 4], "trunc", 2.5)
    plane = gd._run_weights()
    assert plane is not None and cloud.weights is None
    check(gd.winner(1), cloud.weighted_view(plane.clone()), robust_iters=[2, 4])
    # a pruned chain: 4 candidates for 3 iterations, the best 2 for the rest
    gd = engine(cloud)
    gd.run(3)
    child, _ = gd.pruned(2)
    child.run(3)
    check(child.winner(1), cloud, prune_iters=3, prune_keep=2)
    with pytest.raises(ValueError, match="gn_iters"):
        batch(gn_iters=3, depth_mask=True)
