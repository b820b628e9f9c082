"""The Huber-L1 form of the pose information record and of the Levenberg-Marquardt polish on the device (pcl_pose_information_l1,
pcl_pose_information_images_l1, pcl_gn_refine_l1, pcl_gn_refine_images_l1; build-defined) against the float64 model
of tests/gn_l1_helpers.py, against the plain (L2) calls where the two must agree, and through omniloc_batch and
omniloc_batch_images_polished under cfg.gn_objective = "l1".  The CPU side — the model's limits, its descent, the bound and the planted
mistakes it catches, the cfg keys — is tests/test_gn_l1_model.py.

Bounded comparisons run under 0/1 weights ok (the decisive pairs of the pose, as in test_pose_information: no border pair enters a
sum), times gn_helpers.weight_plane where the case is weighted: gn_l1_helpers.bounds_l1 propagates a per-point bound that holds for
those pairs only."""
import numpy as np
import pytest

import gn_helpers as gn
import gn_l1_helpers as g1
import grad_helpers as gh
import info_helpers as ih

pytestmark = pytest.mark.gpu
FMTS = ("f16", "u8", "f32")
U = ih.U
FIELDS = ("trans", "rot", "sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats")


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


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


_CLOUDS, _PANOS = {}, {}


def _pano(ops, oracle, name, fmt, flt=False):
    from parity_helpers import T
    if (name, fmt, flt) not in _PANOS:
        _PANOS[name, fmt, flt] = ops.Pano(T(gh.scene(oracle, name)[3 if flt else 2]), fmt=fmt)
    return _PANOS[name, fmt, flt]


def _cloud(ops, oracle, name, weights=None, tag=None):
    from parity_helpers import T
    if (name, tag) not in _CLOUDS:
        xyz, rgb = gh.scene(oracle, name)[:2]
        _CLOUDS[name, tag] = ops.Cloud(T(xyz), T(rgb), weights=None if weights is None else T(np.asarray(weights, np.float32)))
    return _CLOUDS[name, tag]


def _poses(oracle, name):
    return np.stack([gn.scene_pose(oracle, name, b) for b in range(gh.N_POSES)])


def _tr(thetas):
    from parity_helpers import T
    thetas = np.asarray(thetas, np.float32).reshape(-1, 6)
    return T(thetas[:, :3].copy()), T(thetas[:, 3:].copy())


def rows(out):
    """(H, b, stats, cov) GPU tensors -> one dict of float64 numpy values per pose (cov: None for an L1 record)"""
    H, b, st = (t.cpu().numpy().astype(np.float64) for t in out[:3])
    return [dict(H=H[i], b=b[i], M=st[i, 0], S1=st[i, 1], S2=st[i, 2], sigma2=st[i, 3], status=st[i, 4]) for i in range(len(H))]


def _bounded_cloud(ops, oracle, name, b, weighted):
    plane = gn.weight_plane(name) if weighted else None
    return _cloud(ops, oracle, name, g1.case_weights(oracle, name, b, plane), ("ok", b, weighted)), plane


# ------------------------------------------------------------------------------------------- (a), (b): the record against the model
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_record_against_the_model(ops, oracle, parity, name, fmt):
    """(a) ops.pose_information(objective="l1") against gn_l1_helpers.l1_sums in float64 inside bounds_l1: both poses, 0/1 weights ok and
    ok x gn_helpers.weight_plane, delta = 1/64 and 1/255 — M exactly, S1, S_rho, F_rho and every entry of H_rho and b_rho; cov is None and
    the status 0.  (b) in every such run M and S1 equal the plain call's at the same pose bit for bit."""
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    for weighted in (False, True):
        for b in range(gh.N_POSES):
            cloud, plane = _bounded_cloud(ops, oracle, name, b, weighted)
            plain = ops.pose_information(cloud, pano, *_tr(th[b]))
            for delta in g1.DELTAS:
                out = ops.pose_information(cloud, pano, *_tr(th[b]), objective="l1", delta=delta)
                assert out[3] is None and out[0].shape == (1, 6, 6) and out[1].shape == (1, 6) and out[2].shape == (1, 5)
                assert same_bits(out[2][:, 0:2], plain[2][:, 0:2]), (name, fmt, b, weighted, delta)            # (b)
                g, bd = rows(out)[0], g1.bounds_l1(oracle, name, b, delta, plane)
                ref = bd["ref"]
                tag = "%s %s pose %d weighted %d delta 1/%d" % (name, fmt, b, weighted, round(1 / delta))
                nH = np.sqrt(np.outer(np.diag(ref["H"]), np.diag(ref["H"])))
                q = np.abs(g["H"] - ref["H"]) / bd["BH"]
                at = np.unravel_index(np.argmax(q), q.shape)
                nb = np.sqrt(np.diag(ref["H"]) * ref["M"])
                print("%s: M %g (model %g), status %d; H tightest entry %s %.3e of bound %.3e; b %.3e, S1 %.3e, S_rho %.3e, F_rho %.3e of their bounds"
                      % (tag, g["M"], ref["M"], g["status"], at, (np.abs(g["H"] - ref["H"]) / nH)[at], (bd["BH"] / nH)[at],
                         (np.abs(g["b"] - ref["b"]) / bd["Bb"]).max(), abs(g["S1"] - ref["S1"]) / bd["BS1"], abs(g["S2"] - ref["S2"]) / bd["BS2"],
                         abs(g["sigma2"] - ref["sigma2"]) / bd["Bsig"]))
                assert g["M"] == ref["M"] and g["status"] == 0, tag
                parity(tag + ": H_rho, tightest entry, / sqrt(H_kk H_ll)", (np.abs(g["H"] - ref["H"]) / nH)[at], (bd["BH"] / nH)[at])
                parity(tag + ": b_rho, worst entry, / sqrt(M H_kk)", (np.abs(g["b"] - ref["b"]) / nb).max(), (bd["Bb"] / nb).max())
                parity(tag + ": S_rho", abs(g["S2"] - ref["S2"]), bd["BS2"])
                parity(tag + ": F_rho", abs(g["sigma2"] - ref["sigma2"]), bd["Bsig"])
                assert g1.violations_l1(g, bd) == [], tag
                assert np.array_equal(g["H"], g["H"].T)


# --------------------------------------------------------------------------------------------------------------- (c), (d): the limits
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_saturated_limit_is_half_the_plain_record(ops, oracle, name, fmt):
    """(c) delta = 2 is above every residual: phi is the host's 1 / delta = 0.5 for every point, an exact factor — H and b of the L1 record
    are exactly half the plain record's, bit for bit, M and S1 are the plain ones, and S_rho is S2 / 4 to the sums' roundings (all terms are
    positive: ADDS + 2 roundings each way, relative); without weights and under a weight plane, both poses in one call"""
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    for cloud in (_cloud(ops, oracle, name), _cloud(ops, oracle, name, gn.weight_plane(name), "w")):
        plain = ops.pose_information(cloud, pano, *_tr(th))
        l1 = ops.pose_information(cloud, pano, *_tr(th), objective="l1", delta=g1.DELTA_SATURATED)
        assert same_bits(l1[0], 0.5 * plain[0]) and same_bits(l1[1], 0.5 * plain[1]), (name, fmt)
        assert same_bits(l1[2][:, 0:2], plain[2][:, 0:2]) and same_bits(l1[2][:, 4], plain[2][:, 4])
        # (S_rho is S2 / 4 up to rounding only: l l rounds before the factor where the plain pass fuses it into the sum)
        s2 = (l1[2][:, 2] / (0.25 * plain[2][:, 2]) - 1).abs().max().item()
        assert s2 <= (g1.ADDS + 2) * U, s2
        assert (plain[0] != 0).any()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_small_delta_limit_is_the_sampling_loss_gradient(ops, oracle, parity, name, fmt):
    """(d) delta = 2^-12 is below every kept residual: b_rho / M against the gradient ops.sampling_loss(with_grad=True) returns at that pose
    under the same 0/1 weights ok, within the sum of the two kernels' bounds — the L1 pass's Bb / M of bounds_l1, and for the loss kernel
    the same per-point bound d_i on j summed, (sum w d_i + (ADDS + 8) u sum w |j_ik|) / M + 2 u |g_k|: info_helpers.ADDS roundings inside a
    block as in the pass, at most eight chunk sums on top (pcl_gd_plan cuts these clouds into 8), the division and the output.  Its loss is
    S1 / M within the two S1 bounds, and its count is M exactly."""
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    d = g1.DELTA_SMALL
    for b in range(gh.N_POSES):
        cloud, _ = _bounded_cloud(ops, oracle, name, b, False)
        bd = g1.bounds_l1(oracle, name, b, d)
        sel, w, m64 = bd["sel"], bd["w"][bd["sel"]], bd["m64"]
        assert m64["loss"][sel].min() > d
        out = ops.pose_information(cloud, pano, *_tr(th[b]), objective="l1", delta=d)
        g = rows(out)[0]
        loss = ops.sampling_loss(cloud, pano, *_tr(th[b]), with_grad=True).cpu().numpy().astype(np.float64)[0]
        assert loss[1] == g["M"] == bd["ref"]["M"]
        j = np.abs(m64["grad"][sel])
        rn = j.max(1)
        worst = gh.three_stats(gh.point_errors(bd["m32"]["grad"], m64["grad"], sel))[2]
        di = gh.FACTOR * worst * np.maximum(rn, max(float(np.median(rn)), 1e-300))
        M = g["M"]
        B_loss = ((w * di).sum() + (ih.ADDS + 8) * U * (w[:, None] * j).sum(0)) / M + 2 * U * np.abs(loss[2:8])
        B_l1 = bd["Bb"] / M + U * np.abs(g["b"] / M)
        err = np.abs(g["b"] / M - loss[2:8])
        tag = "%s %s pose %d" % (name, fmt, b)
        print("%s: |b_rho / M - grad| / bound %s" % (tag, err / (B_loss + B_l1)))
        parity(tag + ": b_rho / M against the loss kernel's gradient, worst entry / bound", (err / (B_loss + B_l1)).max(), 1.0)
        B_s1 = (2 * bd["BS1"] + (ih.ADDS + 8) * U * bd["ref"]["S1"]) / M + 2 * U * loss[0]
        parity(tag + ": S1 / M against the loss kernel's loss", abs(g["S1"] / M - loss[0]), B_s1)
        # S_rho = S1 - delta / 2 M in the model; on the device within the two sums' bounds
        parity(tag + ": S_rho against S1 - delta / 2 M", abs(g["S2"] - (g["S1"] - d / 2 * M)), bd["BS1"] + bd["BS2"])


# ------------------------------------------------------------------------------------------------------------------ (e): the trace
def _refine(ops, cloud, pano, thetas, iters, delta, **hyper):
    return ops.gauss_newton_refine(cloud, pano, *_tr(thetas), iters=iters, trace=True, objective="l1", delta=delta, **hyper)


def _runs(res):
    host = {key: v.cpu().numpy() for key, v in res.items() if v is not None}
    out = []
    for i in range(host["trans"].shape[0]):
        r = dict(theta=np.concatenate([host["trans"][i], host["rot"][i]]), trace=host["trace"][:, i])
        for key in ("sigma2_start", "sigma2", "lam", "accepted", "rejected", "evaluations", "status", "H", "b", "stats"):
            r[key] = host[key][i]
        out.append(r)
    return out


def _info_at(ops, cloud, pano, thetas, delta):
    """the device's own L1 record at every pose of thetas in ONE call -> lookup theta -> dict(F, M, ok, H, b, the fp32 rows)"""
    uniq = {np.asarray(t, np.float32).tobytes(): np.asarray(t, np.float32) for t in thetas}
    th = np.stack(list(uniq.values()))
    H, b, st, cov = ops.pose_information(cloud, pano, *_tr(th), objective="l1", delta=delta)
    assert cov is None
    H, b, st = H.cpu().numpy(), b.cpu().numpy(), st.cpu().numpy()
    table = {key: dict(F=st[i, 3], M=st[i, 0], ok=st[i, 4] != 1, H=H[i].astype(np.float64), b=b[i].astype(np.float64), H32=H[i], b32=b[i], stats=st[i])
             for i, key in enumerate(uniq)}
    return lambda theta: table[np.asarray(theta, np.float32).tobytes()]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ih.CASES)
def test_the_trace_is_the_algorithm(ops, oracle, parity, name, fmt):
    """(e) gauss_newton_refine(objective="l1", trace=True), gn_helpers.TRACE_ITERS iterations from both scene poses, with and without a
    weight plane, delta = 1/64 (f16: all of gn_helpers.CONFIGS, and delta = 1/255 under the defaults), teacher-forced:
    gn_helpers.trace_violations, unchanged, with the device's own L1 record as info_at — F = F_rho and M bit for bit per evaluation, the
    flags, lambda and counters by the fp32 rules, every step against the float64 solve on the record's H_rho, b_rho — finds nothing; the
    returned H, b, stats equal the L1 record at the returned pose bit for bit, cov is None, and the sampling loss S1 / M of the returned
    record is printed next to the start's."""
    th = _poses(oracle, name)
    pano = _pano(ops, oracle, name, fmt)
    grid = [(c, 1.0 / 64) for c in (gn.CONFIGS if fmt == "f16" else ("default",))] + ([("default", 1.0 / 255)] if fmt == "f16" else [])
    for config, delta in grid:
        h = gn.hyper(**gn.CONFIGS[config])
        for tag, cloud in (("plain", _cloud(ops, oracle, name)), ("weighted", _cloud(ops, oracle, name, gn.weight_plane(name), "w"))):
            res = _refine(ops, cloud, pano, th, gn.TRACE_ITERS, delta, **gn.CONFIGS[config])
            assert res["cov"] is None
            runs = _runs(res)
            at = _info_at(ops, cloud, pano, np.concatenate([r["trace"][: int(r["evaluations"]), :6] for r in runs]), delta)
            for b, r in enumerate(runs):
                label = "%s %s %s %s delta 1/%d pose %d" % (name, fmt, config, tag, round(1 / delta), b)
                worst = []
                bad = gn.trace_violations(r, h, gn.TRACE_ITERS, at, report=lambda a, bd: worst.append((a, bd)))
                first, last = at(r["trace"][0, :6])["stats"], r["stats"]
                print("%s: F_rho %.6f -> %.6f, S1/M %.6f -> %.6f, flags %s, status %d, worst step %s"
                      % (label, r["sigma2_start"], r["sigma2"], first[1] / first[0], last[1] / last[0], r["trace"][:, 7].astype(int), r["status"], worst))
                assert bad == [], (label, bad)
                ref = at(r["theta"])
                assert _same(r["H"], ref["H32"]) and _same(r["b"], ref["b32"]) and _same(r["stats"], ref["stats"]), label
                assert r["status"] in (0, 3) and r["accepted"] >= 1
                for a, bd in worst:
                    parity(label + ": worst step against the float64 solve", a, bd)


# --------------------------------------------------------------------------------------------------------------- (f): the free run
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", gn.FREE_CASES)
def test_a_free_run_ends_where_the_model_ends(ops, oracle, parity, name, fmt):
    """(f) gn_helpers' free run with evaluate_l1 as the model, delta = 1/64: FREE_ITERS iterations from the starts FREE_OFFSETS around the L1
    model's own converged pose; the device's final F_rho is at most gn_helpers.free_bound(lo, hi), [lo, hi] the span of the model's final
    F_rho over the start and its 12 one-ulp neighbours"""
    delta = 1.0 / 64
    starts = g1.free_starts(oracle, name, delta)
    runs = _runs(_refine(ops, _cloud(ops, oracle, name), _pano(ops, oracle, name, fmt), np.stack(starts), gn.FREE_ITERS, delta))
    for i, r in enumerate(runs):
        lo, hi, own = g1.free_yardstick(oracle, name, delta, i)
        print("%s %s start %d: device F_rho %.9g (start %.9g, %d accepted, %d rejected, status %d); model [%.9g, %.9g], bound %.9g"
              % (name, fmt, i, r["sigma2"], r["sigma2_start"], r["accepted"], r["rejected"], r["status"], lo, hi, gn.free_bound(lo, hi)))
    for i, r in enumerate(runs):
        lo, hi, own = g1.free_yardstick(oracle, name, delta, i)
        assert hi < 0.5 * float(r["sigma2_start"])                     # the start is not the minimum: something is polished
        parity("%s %s start %d: final F_rho" % (name, fmt, i), r["sigma2"], gn.free_bound(lo, hi), hi - lo)


# ------------------------------------------------------------------------------------------------------------- (g): independence
def test_poses_of_a_batch_are_independent(ops, oracle):
    """(g) `odd`, f16, B = 3 — the two scene poses and the L1 model's converged pose — with tol between their first steps, so that the third
    converges early (status 3): every pose's outputs and trace rows equal its own B = 1 call bit for bit; the record call likewise"""
    name, iters, delta = "odd", 6, 1.0 / 64
    ev = g1.scene_evaluator_l1(oracle, name, delta)
    th = np.stack([gn.scene_pose(oracle, name, 0), gn.scene_pose(oracle, name, 1), g1.free_centre(oracle, name, delta)[0]])
    first = [np.abs(gn.solve_step(ev(t)["H"], ev(t)["b"], 1e-3, 0.1)).max() for t in th]
    assert first[2] < 0.1 * min(first[:2])
    tol = float(np.sqrt(first[2] * min(first[:2])))
    cloud, pano = _cloud(ops, oracle, name), _pano(ops, oracle, name, "f16")
    both = _refine(ops, cloud, pano, th, iters, delta, tol=tol)
    assert both["status"][2] == 3 and both["evaluations"][2] < iters + 1 and (both["evaluations"][:2] > both["evaluations"][2]).all()
    rec = ops.pose_information(cloud, pano, *_tr(th), objective="l1", delta=delta)
    for i in range(3):
        one = _refine(ops, cloud, pano, th[i:i + 1], iters, delta, tol=tol)
        for key in FIELDS:
            assert same_bits(both[key][i:i + 1], one[key]), (i, key)
        assert same_bits(both["trace"][:, i:i + 1], one["trace"]), i
        alone = ops.pose_information(cloud, pano, *_tr(th[i]), objective="l1", delta=delta)
        assert all(same_bits(a[i:i + 1], c) for a, c in zip(rec[:3], alone[:3]))
    assert (both["trace"][int(both["evaluations"][2]):, 2] == 0).all()


_SECOND = {}


def _second_image(oracle, name):
    """a second k / 255 panorama of a case's room, rendered a few centimetres and hundredths of a radian from the first (the fp16-level
    and u8 texels hold k / 255 images only, and a chain has one texel format)"""
    if name not in _SECOND:
        from piccolo_amd import synth
        xyz, rgb, img = gh.scene(oracle, name)[:3]
        t_gt, ypr_gt = synth.gt_pose(gh.SEED)
        t2, ypr2 = np.asarray(t_gt) + np.array([0.05, -0.03, 0.02]), np.asarray(ypr_gt) + np.array([0.03, 0.0, -0.02])
        _SECOND[name] = oracle.make_pano_u8(synth.transform_cloud(xyz, t2, ypr2), rgb, img.shape[:2]).astype(np.float32) / 255
        assert (_SECOND[name] != img).any()
    return _SECOND[name]


def _planes(ops, n, I, seed=0):
    from parity_helpers import T
    stride = ops._lib.load().pcl_cloud_stride(n)
    out = np.zeros((I, stride), np.float32)
    for i in range(I):
        out[i, :n] = np.floor((0.25 + 0.75 * np.random.default_rng(1000 * seed + n + i).random(n)) * 1024) / 1024
    return T(out)


@pytest.mark.parametrize("form", ["shared", "sets", "planes"])
@pytest.mark.parametrize("name", ["odd", "tall"])
def test_image_rows_are_the_single_calls(ops, oracle, name, form):
    """(g) the images forms, three images (the case's panorama, a second rendering of its room and the first again), u8 and f16: row i of
    pose_information_images(objective="l1") and of gauss_newton_refine_images(objective="l1", trace=True) — and of the *_at_winners forms —
    equals the single-image L1 call for that pose, panorama, colour set and plane, bit for bit; with shared colours, with a colour set
    per image, and with a weight plane per image.  The batch holds a pose that is not finite (status 1, gated at k = 0)."""
    import torch
    from parity_helpers import T
    xyz, rgb, img = gh.scene(oracle, name)[:3]
    imgf = _second_image(oracle, name)
    I, iters, delta = 3, 4, 1.0 / 64
    x = T(xyz)
    rgbs = [T(rgb), T(np.roll(rgb, 1, axis=0).copy()), T((rgb * np.float32(0.9)).astype(np.float32))]
    singles = [ops.Cloud(x, rgbs[i] if form == "sets" else rgbs[0]) for i in range(I)]
    cloud = ops.Cloud.with_color_sets(x, rgbs, order=singles[0].order) if form == "sets" else singles[0]
    planes = _planes(ops, cloud.n, I) if form == "planes" else None
    if planes is not None:
        singles = [c.weighted_view(planes[i]) for i, c in enumerate(singles)]
    th = np.stack([gn.scene_pose(oracle, name, 0), gn.scene_pose(oracle, name, 1), gn.scene_pose(oracle, name, 0)])
    th[2, :3] += np.float32(0.02)
    for fmt in ("u8", "f16"):
        panos = [ops.Pano(T(im), fmt=fmt) for im in (img, imgf, img)]
        trans, rot = _tr(th)
        win = torch.full((I, 16), float("nan"), device="cuda")
        win[:, 0:3], win[:, 13:16] = trans, rot
        rec = ops.pose_information_images(cloud, panos, trans, rot, planes=planes, objective="l1", delta=delta)
        rec16 = ops.pose_information_images_at_winners(cloud, panos, win, planes=planes, objective="l1", delta=delta)
        assert rec[3] is None and all(same_bits(a, c) for a, c in zip(rec[:3], rec16[:3]))
        bad = trans.clone()
        bad[1, 1] = float("nan")
        res = ops.gauss_newton_refine_images(cloud, panos, bad, rot, iters=iters, trace=True, planes=planes, objective="l1", delta=delta)
        win[:, 0:3] = bad
        res16 = ops.gauss_newton_refine_images_at_winners(cloud, panos, win, iters=iters, trace=True, planes=planes, objective="l1", delta=delta)
        assert res["cov"] is None and res["trace"].shape == (iters + 1, I, 16)
        for i in range(I):
            alone = ops.pose_information(singles[i], panos[i], trans[i:i + 1], rot[i:i + 1], objective="l1", delta=delta)
            assert all(same_bits(a[i:i + 1], c) for a, c in zip(rec[:3], alone[:3])), (name, form, fmt, i)
            one = ops.gauss_newton_refine(singles[i], panos[i], bad[i:i + 1], rot[i:i + 1], iters=iters, trace=True, objective="l1", delta=delta)
            for key in FIELDS:
                assert same_bits(res[key][i:i + 1], one[key]) and same_bits(res16[key][i:i + 1], one[key]), (name, form, fmt, i, key)
            assert same_bits(res["trace"][:, i:i + 1], one["trace"]) and same_bits(res16["trace"][:, i:i + 1], one["trace"])
        assert res["status"].tolist()[1] == 1 and res["evaluations"].tolist()[1] == 1 and float(res["accepted"][0]) > 1
        assert not same_bits(rec[0][0], rec[0][1])
        if form != "shared":
            assert not same_bits(rec[0][0:1], ops.pose_information(singles[1], panos[0], trans[0:1], rot[0:1], objective="l1", delta=delta)[0])


def test_sixty_five_images_run_in_two_launches(ops, oracle):
    """(g) 65 poses / panoramas / colour sets / planes of `tiny` at iters = 1: the pass runs once per 64 addresses, the colour set, the plane
    and the partial row counted from the call's first image; rows 0, 62, 63 and 64 equal their single L1 calls bit for bit"""
    from parity_helpers import T
    xyz, rgb, img = gh.scene(oracle, "tiny")[:3]
    imgf = _second_image(oracle, "tiny")
    I, delta = 65, 1.0 / 64
    x = T(xyz)
    rng = np.random.default_rng(3)
    rgbs = [T(np.roll(rgb, k, axis=0).copy()) for k in range(I)]
    keep = [0, 62, 63, 64]
    singles = {i: ops.Cloud(x, rgbs[i]) for i in keep}
    cloud = ops.Cloud.with_color_sets(x, rgbs, order=singles[0].order)
    p = [ops.Pano(T(im), fmt="u8") for im in (img, imgf)]
    panos = [p[k % 2] for k in range(I)]
    base = _poses(oracle, "tiny")
    th = np.stack([base[k % 2] + np.concatenate([0.01 * rng.random(3), np.zeros(3)]).astype(np.float32) for k in range(I)])
    trans, rot = _tr(th)
    planes = _planes(ops, cloud.n, I, seed=7)
    res = ops.gauss_newton_refine_images(cloud, panos, trans, rot, iters=1, trace=True, planes=planes, objective="l1", delta=delta)
    rec = ops.pose_information_images(cloud, panos, trans, rot, planes=planes, objective="l1", delta=delta)
    assert res["trace"].shape == (2, I, 16)
    for i in keep:
        single = singles[i].weighted_view(planes[i])
        one = ops.gauss_newton_refine(single, panos[i], trans[i:i + 1], rot[i:i + 1], iters=1, trace=True, objective="l1", delta=delta)
        for key in FIELDS:
            assert same_bits(res[key][i:i + 1], one[key]), (i, key)
        assert same_bits(res["trace"][:, i:i + 1], one["trace"]), i
        alone = ops.pose_information(single, panos[i], trans[i:i + 1], rot[i:i + 1], objective="l1", delta=delta)
        assert all(same_bits(a[i:i + 1], c) for a, c in zip(rec[:3], alone[:3])), i
    assert not same_bits(res["H"][0], res["H"][64]) and not same_bits(res["H"][63], res["H"][64])


# --------------------------------------------------------------------------------------------------------- (h), (i), (j): the front ends
BASE = dict(num_iter=6, num_input=4, lr=0.1, patience=5, factor=0.9)


def _front_scene(oracle):
    from parity_helpers import T
    from piccolo_amd import synth
    xyz, rgb, img = gh.scene(oracle, "odd")[:3]
    t_gt, ypr_gt = synth.gt_pose(gh.SEED)
    trans, rot = synth.start_poses(t_gt, ypr_gt, 4, seed=gh.SEED)
    img2 = _second_image(oracle, "odd")
    return T(xyz), T(rgb), T(img), T(img2), trans, rot, len(xyz)


@pytest.mark.parametrize("delta", [None, 1.0 / 255])
def test_omniloc_batch_polishes_its_winner_on_the_l1_objective(ops, oracle, delta):
    """(h) omniloc_batch on test_gn_refine's scene (2049 points, 64 x 128, 4 candidates, 6 iterations) with gn_iters = 3, gn_objective = "l1"
    (and gn_delta): the three entries equal the hand-driven composition bit for bit — engine, winners row,
    gauss_newton_refine_at_winners(objective="l1"), one forward-only sampling_loss at the polished pose —, with pose_covariance the fourth
    entry is pose_information's cov at the RETURNED pose (omniloc.pose_covariance's bits there), and the written-back leaves are the
    chain's; plain, with weights=, with the robust keys (under the chain's last plane) and with the prune keys.  With a step cap so small
    that no step is accepted the chain's own entries come back bit for bit, with the covariance at the chain's pose.  (j) gn_objective =
    "l2" equals the absent key bit for bit."""
    from conftest import Cfg
    from parity_helpers import T
    from piccolo_amd import localize, omniloc as po
    x, c, im, _, trans, rot, n = _front_scene(oracle)
    w = T((0.25 + 0.75 * np.random.default_rng(3).random(n)).astype(np.float32))
    pano, box = po.packed_pano(im, n_points=n), po.quantile_box_of(x, 0.05)
    l1 = dict(gn_objective="l1") if delta is None else dict(gn_objective="l1", gn_delta=delta)
    okw = dict(objective="l1") if delta is None else dict(objective="l1", delta=delta)

    def batch(weights=None, **kw):
        t, r = T(trans).clone(), T(rot).clone()
        out = po.omniloc_batch(im, x, c, t, r, Cfg(**BASE, **kw), {}, weights=weights)
        return [o.clone() for o in out], [t.cpu(), r.cpu()]

    def check(engine_win, plane_cloud, weights=None, **kw):
        win = engine_win.cpu()
        without, leaves0 = batch(weights, **kw)
        assert len(without) == 3 and same_bits(without[0].reshape(3), win[0, 0:3]) and same_bits(without[2].reshape(1), win[0, 12:13])
        res = ops.gauss_newton_refine_at_winners(plane_cloud, pano, engine_win, iters=3, **okw)
        assert res["cov"] is None and float(res["accepted"][0]) > 1 and float(res["status"][0]) in (0.0, 3.0)
        want_R = ops.rot_from_ypr(res["rot"])[0].cpu()
        want_loss = ops.sampling_loss(plane_cloud, pano, res["trans"], res["rot"], with_grad=False)[0, 0:1].cpu()
        want_cov = ops.pose_information(plane_cloud, pano, res["trans"], res["rot"])[3][0].cpu()
        for extra in (dict(), dict(pose_covariance=True)):
            got, leaves1 = batch(weights, gn_iters=3, **l1, **extra, **kw)
            assert len(got) == 3 + len(extra)
            assert same_bits(got[0].reshape(3), res["trans"][0].cpu()) and same_bits(got[1], want_R) and same_bits(got[2].reshape(1), want_loss)
            assert got[0].shape == (3, 1) and got[1].shape == (3, 3) and got[2].shape == () and not got[0].is_cuda
            assert not same_bits(got[0], without[0])
            assert all(same_bits(a, b) for a, b in zip(leaves0, leaves1))
            if extra:
                assert got[3].shape == (6, 6) and not got[3].is_cuda and same_bits(got[3], want_cov)
        # no step accepted: the chain's own entries, and the covariance at the chain's pose
        got, _ = batch(weights, gn_iters=3, gn_step_cap=1e-12, pose_covariance=True, **l1, **kw)
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
    own = po.gauss_newton_refine(im, x, c, win[:, 0:3].contiguous(), win[:, 13:16].contiguous(), iters=3, **okw)
    assert all(same_bits(own[key], res[key]) for key in FIELDS) and own["cov"] is None
    cov = po.pose_covariance(im, x, c, res["trans"], res["rot"])[0][0].cpu()
    got = batch(gn_iters=3, pose_covariance=True, **l1)[0]
    assert same_bits(got[3], cov)
    ref = localize.refine_image(im, x, c, T(trans).clone(), T(rot).clone(), Cfg(parallel=True, gn_iters=3, pose_covariance=True, **l1, **BASE))
    assert len(ref) == 4 and all(same_bits(a, b) for a, b in zip(ref, got))
    # the polish works on another objective than the L2 one: another pose
    l2 = batch(gn_iters=3)[0]
    assert not same_bits(l2[0], got[0])
    if delta is None:
        # (j) "l2" is the absent key, bit for bit
        for extra in (dict(), dict(pose_covariance=True), dict(gn_step_cap=0.05, gn_lambda=1e-2)):
            a, b = batch(gn_iters=3, **extra)[0], batch(gn_iters=3, gn_objective="l2", **extra)[0]
            assert len(a) == len(b) and all(same_bits(p, q) for p, q in zip(a, b))
        a = ops.gauss_newton_refine_at_winners(cloud, pano, win, iters=3, trace=True)
        b = ops.gauss_newton_refine_at_winners(cloud, pano, win, iters=3, trace=True, objective="l2")
        assert all(same_bits(a[key], b[key]) for key in FIELDS + ("cov", "trace"))
        assert all(same_bits(p, q) for p, q in zip(ops.pose_information_at_winners(cloud, pano, win),
                                                   ops.pose_information_at_winners(cloud, pano, win, objective="l2")))
        # the default delta is ops.GN_L1_DELTA
        d = ops.gauss_newton_refine_at_winners(cloud, pano, win, iters=3, objective="l1", delta=ops.GN_L1_DELTA)
        assert all(same_bits(d[key], res[key]) for key in FIELDS)
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


@pytest.mark.parametrize("chain", ["plain", "robust"])
def test_omniloc_batch_images_polished_on_the_l1_objective(ops, oracle, chain):
    """(i) omniloc_batch_images_polished for the two panoramas of `odd` (shared colours; pcl_gd_plan cuts 2049 points into the same chunks
    for 4 and for 8 candidates) with gn_iters = 3, gn_objective = "l1": t, R (and cov) per image equal omniloc_batch's under the same cfg
    bit for bit; a polished entry's loss is float32(S1) / float32(M) of the ONE L1 chain's record at the chain's winners, an unpolished
    one's the chain's own; (j) gn_objective = "l2" equals the absent key bit for bit."""
    import torch
    from conftest import Cfg
    from parity_helpers import T
    from piccolo_amd import omniloc as po
    x, c, im, imf, trans, rot, n = _front_scene(oracle)
    ims = [im, imf]
    I = len(ims)
    extra = dict(robust_iters=[2, 4]) if chain == "robust" else {}

    def starts():
        return [T(trans).clone() for _ in range(I)], [T(rot).clone() for _ in range(I)]

    def images(**kw):
        tl, rl = starts()
        return po.omniloc_batch_images_polished(ims, x, c, tl, rl, Cfg(**BASE, **extra, **kw))

    def singles(**kw):
        tl, rl = starts()
        return [po.omniloc_batch(ims[i], x, c, tl[i], rl[i], Cfg(**BASE, **extra, **kw), {}) for i in range(I)]

    def expected(cfg):
        panos = po._chain_panos(ims, n)
        tl, rl = starts()
        gd = po._refine(x, c, panos, torch.cat(tl), torch.cat(rl), po.quantile_box_of(x, 0.05), cfg, True, weight_sets=I if extra else 0)
        wins = gd.winners(I)
        planes = gd.weight_planes() if extra else None
        gs = po.gn_schedule(cfg)
        res = ops.gauss_newton_refine_images_at_winners(po.packed_cloud(x, c), panos, wins, iters=gs[0], planes=planes, **gs[1])
        acc, status, stats, own = res["accepted"].cpu().numpy(), res["status"].cpu().numpy(), res["stats"].cpu().numpy(), wins[:, 12].cpu().numpy()
        took = (acc > 1) & ((status == 0) | (status == 3))
        return took, [np.float32(stats[i, 1]) / np.float32(stats[i, 0]) if took[i] else own[i] for i in range(I)]
    seen = set()
    for kw in (dict(gn_iters=3, gn_objective="l1"), dict(gn_iters=3, gn_objective="l1", pose_covariance=True),
               dict(gn_iters=3, gn_objective="l1", gn_delta=1.0 / 255, pose_covariance=True),
               dict(gn_iters=1, gn_step_cap=1e-30, gn_objective="l1", pose_covariance=True)):
        got, one = images(**kw), singles(**kw)
        took, losses = expected(Cfg(**BASE, **extra, **kw))
        for i in range(I):
            assert len(got[i]) == len(one[i]) == (4 if "pose_covariance" in kw else 3)
            assert same_bits(got[i][0], one[i][0]) and same_bits(got[i][1], one[i][1]), (chain, kw, i)
            if "pose_covariance" in kw:
                assert got[i][3].shape == (6, 6) and same_bits(got[i][3], one[i][3]) and torch.isfinite(got[i][3]).all(), (chain, kw, i)
            assert np.float32(got[i][2].item()).tobytes() == np.float32(losses[i]).tobytes(), (chain, kw, i, got[i][2], losses[i])
            if took[i]:
                assert abs(float(got[i][2]) - float(one[i][2])) <= 2 * n * 2.0 ** -24 * abs(float(one[i][2]))
            else:
                assert same_bits(got[i][2], one[i][2])
            seen.add(bool(took[i]))
    assert seen == {True, False}
    a, b = images(gn_iters=3, pose_covariance=True), images(gn_iters=3, gn_objective="l2", pose_covariance=True)
    assert all(same_bits(p, q) for ra, rb in zip(a, b) for p, q in zip(ra, rb))
    l1 = images(gn_iters=3, gn_objective="l1", pose_covariance=True)
    assert not same_bits(a[0][0], l1[0][0])
